"""The int8 format of the low-rank KV cache (K21) restated in plain torch, group by group, independent of asvd4llm_amd.ops: the oracle of
tests/test_lowrank_kv_q8_host.py and tests/test_gpu_lowrank_kv_q8.py.

  row x[0 .. r) fp16, r a multiple of 16; groups of 32 consecutive columns, the last one 16 wide when r % 32 == 16
  amax = max |x| of the group, s = amax / 127 in fp32, code = clamp(rint(float(x) / s), -127, 127)
  amax == 0: s = 0, codes 0.  A NaN or an Inf in the group: s = NaN, codes 0.
  d = fp16(float(code) * s)
Every step is one fp32 operation of torch on fp32 tensors (division, round half to even, product), then one rounding to fp16."""
import torch

GROUP = 32


def n_groups(r):
    return -(-r // GROUP)


def quant(x):
    """x [..., r] (values representable in fp16) -> codes int8 [..., r], scales fp32 [..., ceil(r / 32)]"""
    r = x.shape[-1]
    assert r >= 16 and r % 16 == 0
    xf = x.to(torch.float16).to(torch.float32)
    codes = torch.zeros(x.shape, dtype=torch.int8, device=x.device)
    scales = torch.zeros(*x.shape[:-1], n_groups(r), dtype=torch.float32, device=x.device)
    c127 = torch.tensor(127.0, dtype=torch.float32, device=x.device)
    for j in range(n_groups(r)):
        g = xf[..., j * GROUP:min((j + 1) * GROUP, r)]
        finite = torch.isfinite(g).all(-1)
        amax = torch.where(finite, g.abs().amax(-1), torch.zeros_like(g[..., 0]))
        s = amax / c127.expand_as(amax)
        live = finite & (amax > 0)
        q = torch.round(g / torch.where(live, s, torch.ones_like(s))[..., None]).clamp(-127, 127)
        codes[..., j * GROUP:min((j + 1) * GROUP, r)] = torch.where(live[..., None], q, torch.zeros_like(q)).to(torch.int8)
        scales[..., j] = torch.where(finite, s, torch.full_like(s, float("nan")))
    return codes, scales


def dequant(codes, scales):
    """fp16 [..., r]: one fp32 product per element, one rounding"""
    r = codes.shape[-1]
    out = torch.empty(codes.shape, dtype=torch.float16, device=codes.device)
    for j in range(n_groups(r)):
        sl = slice(j * GROUP, min((j + 1) * GROUP, r))
        out[..., sl] = (codes[..., sl].to(torch.float32) * scales[..., j:j + 1]).to(torch.float16)
    return out


def bound(x, scales):
    """|d - x| <= 0.5 s (1 + 2^-10) + 2^-11 |x| + 2^-25: half a step, then the fp16 rounding of d"""
    r = x.shape[-1]
    s = scales.repeat_interleave(GROUP, -1)[..., :r].double()
    return 0.5 * s * (1 + 2.0 ** -10) + 2.0 ** -11 * x.double().abs() + 2.0 ** -25


def graded(g, shape):
    """random rows whose columns fall like the sqrt(sigma) of a latent: N(0, 1) x logspace(0, -3, r), in fp16"""
    r = shape[-1]
    return (torch.randn(*shape, generator=g) * torch.logspace(0, -3, r)).half()


def special_rows(g, r):
    """[6, r] fp16 rows of the cases the format names: graded, an all-zero group, a group of 6e-8 subnormals, a 65504 entry, and (rows 4, 5)
    a NaN and an Inf; returns the rows and the (row, column) of the two non-finite entries"""
    x = graded(g, (6, r))
    x[1, :min(GROUP, r)] = 0
    x[2, :min(GROUP, r)] = 6e-8
    x[3, r - 1] = 65504.0
    nan_at, inf_at = (4, r - 3), (5, 2)
    x[nan_at] = float("nan")
    x[inf_at] = float("-inf")
    return x, nan_at, inf_at
