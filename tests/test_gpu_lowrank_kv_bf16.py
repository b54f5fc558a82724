"""K22 on the device: decode attention on the low-rank KV cache in bf16 (the ADT = ASVD_BF16 form of csrc/lowrank_kv.hip, reached through the
asvd_lowrank_kv_*_a16 entries).  Bit-exact scores on integer data, the whole op against the fp64 restatement (tests/lowrank_kv_restate.py),
masking and isolation, the int8 cache against the bf16 call on the dequantised cache bit for bit, the fp16 entries untouched, the modules
behind their switch, and graph capture.

Seen on an MI355X, relative to the largest output (DESIGN.md 4 "K22"): whole op e_kernel <= 8.5e-3 with e_dense <= 8.0e-3 (bar max(2 e_dense, 2^-6));
LowRankKVAttention.decode 3.3e-3 - 3.8e-3 against 3.6e-3 - 4.2e-3 of its torch path; greedy_decode 5.7e-3 / 1.04e-2 (bf16 / int8 cache) against
6.0e-3 / 8.7e-3 of the torch path."""
import copy
import ctypes
import json

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import exact_data as X
from tests import lowrank_kv_q8_restate as Q
from tests import lowrank_kv_restate as R

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
HEADS = [(1, 1), (12, 12), (12, 3), (32, 32), (32, 8), (40, 40), (40, 10)]   # the list of tests/test_gpu_lowrank_kv.py
FLOOR = 2.0 ** -6    # four times one bf16 rounding (2^-8): the fp16 tests' 2^-9 = 4 * 2^-11 restated for bf16's unit roundoff
SEEN = {"e_kernel": 0.0, "e_dense": 0.0}


def _i16(t):
    return t.view(torch.int16)


def _i32(t):
    return t.view(torch.int32)


# ---- 1. exact scores --------------------------------------------------------------------------------------------------------------------

def _exact_scores_case(dev, H, H_kv, D, r_k, Tmax, scale, mode, seed):
    """q in -2..2 and A_k in -1..1: sum_d |q||A_k| <= 2 * 128 = 256, the largest run of integers bf16 holds exactly, so q~ is exact; C_k in
    -3..3.  Every partial sum is an integer below 2^24: exact in fp32 in any order."""
    from asvd4llm_amd import ops
    g = torch.Generator().manual_seed(seed)
    B = 3
    q = X._ints(g, -2, 2, (B, H, D)).to(BF)
    ck = X._ints(g, -3, 3, (B, Tmax, r_k)).to(BF)
    Ak = X._ints(g, -1, 1, (H_kv * D, r_k)).to(BF)
    lens = [Tmax, Tmax // 2, max(Tmax - 1, 0)]
    rope = None
    if mode == "half":
        idx = torch.randint(0, 4, (Tmax, D // 2), generator=g)
        rope = (torch.tensor([1.0, 0.0, -1.0, 0.0])[idx], torch.tensor([0.0, 1.0, 0.0, -1.0])[idx])   # exact signed permutations
    grp = H // H_kv
    Kabs = (ck.double().abs() @ Ak.double().abs().T).view(B, Tmax, H_kv, D)
    qt_abs = torch.einsum("bhd,hdr->bhr", q.double().abs(), Ak.double().abs().view(H_kv, D, r_k).repeat_interleave(grp, 0))
    pre = {"max |q~| (bf16 exact)": (qt_abs.max().item(), 256.0),
           "max sum |q||K|": (torch.einsum("bhd,bthd->bht", q.double().abs(), Kabs.repeat_interleave(grp, 2)).max().item(), X.LIMIT),
           "max sum |q~||C_k|": (torch.einsum("bhr,btr->bht", qt_abs, ck.double().abs()).max().item(), X.LIMIT)}
    X.check_pre(pre)
    S64, live = R.kv_scores(q, ck, lens, Ak, H_kv, 1.0, None, rope)
    S_int = S64.to(torch.int64)
    assert torch.equal(S_int.double(), S64)
    expect = (S_int.double() * scale).float()
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    got = ops.lowrank_kv_scores(q.to(dev), ck.to(dev), lens_d, Ak.to(dev), H_kv, scale, rope=tuple(t.to(dev) for t in rope) if rope else None)
    assert got.dtype == torch.float32 and got.shape == (B, H, Tmax)
    assert torch.equal(got.cpu(), expect), (H, H_kv, D, r_k, Tmax, scale, mode, (got.cpu() != expect).sum().item())


@pytest.mark.parametrize("mode", ["none", "half"])
@pytest.mark.parametrize("H,H_kv", HEADS)
def test_scores_bit_exact_on_integer_data(gpu, H, H_kv, mode):
    off = HEADS.index((H, H_kv)) + (3 if mode == "half" else 0)
    for n, T in enumerate([1, 2, 31, 32, 33, 127, 128, 129]):   # around the 32-token tile and the 4-tile workgroup
        D = (64, 128)[(n + off) % 2]
        r_k = (16, 48, 272)[(n + off) % 3]
        scale = (1.0, 0.125)[(n // 2 + off) % 2]
        _exact_scores_case(gpu, H, H_kv, D, r_k, T, scale, mode, X.seed_of("k22", H, H_kv, T, mode))


# ---- 2. the whole op against the restatement ----------------------------------------------------------------------------------------------

def _data(H, H_kv, D, r_k, r_v, Tmax, B, with_bv, seed, dt=BF):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g)
    return dict(q=rnd(B, H, D).to(dt), ck=rnd(B, Tmax, r_k).to(dt), cv=rnd(B, Tmax, r_v).to(dt), Ak=(rnd(H_kv * D, r_k) / r_k ** 0.5).to(dt),
                Av=(rnd(H_kv * D, r_v) / r_v ** 0.5).to(dt), bv=rnd(H_kv * D).to(dt) if with_bv else None)


def _dense_route(d, lens, H_kv, scale, rope):
    """existing code, not the code under test: bf16 F.linear reconstruction of K and V, torch SDPA in bf16 (the fp16 test's _dense_route)"""
    B, H, D = d["q"].shape
    dt = d["q"].dtype
    out = torch.zeros(B, H, D, dtype=dt, device=d["q"].device)
    for b in range(B):
        T = lens[b]
        if T == 0:
            continue
        K = F.linear(d["ck"][b, :T], d["Ak"]).view(T, H_kv, D)
        V = F.linear(d["cv"][b, :T], d["Av"], d["bv"]).view(T, H_kv, D)
        if rope is not None:
            K = R.rotate_half_table(K.float().transpose(0, 1), rope[0][:T], rope[1][:T]).transpose(0, 1).to(dt)
        K, V = K.transpose(0, 1).repeat_interleave(H // H_kv, 0), V.transpose(0, 1).repeat_interleave(H // H_kv, 0)
        out[b] = F.scaled_dot_product_attention(d["q"][b][None, :, None, :], K[None], V[None], scale=scale)[0, :, 0]
    return out


def _run(dev, d, lens, H_kv, scale, rope, **kw):
    from asvd4llm_amd import ops
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    return ops.lowrank_kv_decode(d["q"], d["ck"], d["cv"], lens_d, d["Ak"], d["Av"], H_kv, scale, bv=d["bv"], rope=rope, **kw)


def _whole_op(dev, H, H_kv, D, r_k, r_v, Tmax, lens, with_bv, mode, seed):
    from asvd4llm_amd import ops
    d = _data(H, H_kv, D, r_k, r_v, Tmax, len(lens), with_bv, seed)
    scale = D ** -0.5
    rope = ops.rope_table(Tmax, D, 10000.0) if mode == "half" else None
    ref = R.kv_decode(d["q"], d["ck"], d["cv"], lens, d["Ak"], d["Av"], H_kv, scale, None, d["bv"], rope)
    dd = {k: (v.to(dev) if v is not None else None) for k, v in d.items()}
    rope_d = tuple(t.to(dev) for t in rope) if rope else None
    out = _run(dev, dd, lens, H_kv, scale, rope_d)
    assert out.dtype == BF and out.shape == (len(lens), H, D)
    dense = _dense_route(dd, lens, H_kv, scale, rope_d)
    top = ref.abs().max().item()
    e_k = (out.double().cpu() - ref).abs().max().item() / top
    e_d = (dense.double().cpu() - ref).abs().max().item() / top
    print(f"K22 H={H} H_kv={H_kv} D={D} r=({r_k},{r_v}) Tmax={Tmax} lens={lens} bv={with_bv} {mode}: e_kernel={e_k:.3e} e_dense={e_d:.3e}")
    SEEN["e_kernel"], SEEN["e_dense"] = max(SEEN["e_kernel"], e_k), max(SEEN["e_dense"], e_d)
    for b, n in enumerate(lens):
        if n == 0:
            assert torch.equal(out[b].cpu(), torch.zeros(H, D, dtype=BF))
    assert e_k <= max(2 * e_d, FLOOR), (e_k, e_d)
    return dd, rope_d, out


@pytest.mark.parametrize("mode", ["none", "half"])
@pytest.mark.parametrize("H,H_kv", [(12, 3), (32, 8), (40, 40)])
def test_whole_op_against_restatement(gpu, H, H_kv, mode):
    from asvd4llm_amd import ops
    Tmax, lens = 200, [200, 0, 67, 129]
    tile, L, ns = ops.lowrank_kv_plan(4, H, Tmax)
    assert (tile, L, ns) == (32, 64, 4)   # the lengths: the whole buffer, nothing, a split and three tokens, two splits and one token
    for D in (64, 128):
        for r_k, r_v in ((16, 48), (272, 144)):
            for with_bv in (False, True):
                _whole_op(gpu, H, H_kv, D, r_k, r_v, Tmax, lens, with_bv, mode, X.seed_of("k22w", H, H_kv, D, r_k, with_bv, mode))
    _whole_op(gpu, H, H_kv, 64, 48, 16, 1, [1], True, mode, X.seed_of("k22w1", H, mode))   # B = 1, a buffer of one token


def test_largest_errors_seen(gpu):
    """prints what DESIGN.md cites (the bound is asserted per case above)"""
    print("K22_ERRORS " + json.dumps(SEEN))
    assert SEEN["e_kernel"] > 0.0


# ---- 3. masking and isolation -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["none", "half"])
def test_masking_isolation_determinism_and_strides(gpu, mode):
    from asvd4llm_amd import ops
    H, H_kv, D, r_k, r_v = 12, 3, 64, 48, 80
    Tmax, lens = 130, [130, 0, 37, 65]
    scale = D ** -0.5
    dd, rope_d, out = _whole_op(gpu, H, H_kv, D, r_k, r_v, Tmax, lens, True, mode, X.seed_of("k22m", mode))
    assert torch.equal(_i16(_run(gpu, dd, lens, H_kv, scale, rope_d)), _i16(out))   # two calls, equal bits
    # NaN and 3e38 at positions >= len, in both caches and in every byte of the workspace (0xff bytes are NaNs, 0x7f bytes 3.39e38 as fp32)
    nb = ops.lowrank_kv_work(len(lens), H, Tmax, r_k, r_v, gpu).numel()
    for fill, byte in ((float("nan"), 0xFF), (3e38, 0x7F)):
        bad = dict(dd, ck=dd["ck"].clone(), cv=dd["cv"].clone())
        for b, n in enumerate(lens):
            bad["ck"][b, n:] = fill
            bad["cv"][b, n:] = fill
        work = torch.full((nb,), byte, dtype=torch.uint8, device=gpu)
        assert torch.equal(_i16(_run(gpu, bad, lens, H_kv, scale, rope_d, work=work)), _i16(out)), fill
        # the scores entry: zeros at t >= len whatever the cache and the workspace hold there
        lens_d = torch.tensor(lens, dtype=torch.int32, device=gpu)
        work.fill_(byte)
        S = ops.lowrank_kv_scores(dd["q"], bad["ck"], lens_d, dd["Ak"], H_kv, scale, rope=rope_d, work=work)
        S0 = ops.lowrank_kv_scores(dd["q"], dd["ck"], lens_d, dd["Ak"], H_kv, scale, rope=rope_d)
        assert torch.equal(_i32(S), _i32(S0)) and torch.isfinite(S).all()
    # a NaN row in one sequence stays there
    bad = dict(dd, ck=dd["ck"].clone(), cv=dd["cv"].clone())
    bad["ck"][0, 3] = float("nan")
    o_bad = _run(gpu, bad, lens, H_kv, scale, rope_d)
    assert torch.isnan(o_bad[0]).any() and torch.equal(_i16(o_bad[1:]), _i16(out[1:]))
    bad["ck"], bad["cv"][3, 64] = dd["ck"], float("nan")
    o_bad = _run(gpu, bad, lens, H_kv, scale, rope_d)
    assert torch.isnan(o_bad[3]).any() and torch.equal(_i16(o_bad[:3]), _i16(out[:3]))

    # a wider and longer NaN-filled buffer, the cache a view of it
    def view(c, pad):
        big = torch.full((c.shape[0] + 1, Tmax + 2, c.shape[2] + pad), float("nan"), dtype=BF, device=gpu)
        big[: c.shape[0], :Tmax, : c.shape[2]] = c
        return big[: c.shape[0], :Tmax, : c.shape[2]]

    strided = dict(dd, ck=view(dd["ck"], 8), cv=view(dd["cv"], 24))
    assert not strided["ck"].is_contiguous() and strided["ck"].stride(1) == r_k + 8
    assert torch.equal(_i16(_run(gpu, strided, lens, H_kv, scale, rope_d)), _i16(out))
    with pytest.raises(ValueError):
        _run(gpu, dict(dd, ck=view(dd["ck"], 4)), lens, H_kv, scale, rope_d)
    with pytest.raises(ValueError):
        _run(gpu, dict(dd, ck=dd["ck"].half()), lens, H_kv, scale, rope_d)     # a mixed call is refused on the device as on the CPU


# ---- 4. the int8 cache -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["none", "half"])
@pytest.mark.parametrize("r", [16, 48, 272])
def test_int8_cache_equals_the_bf16_call_on_the_dequantised_cache(gpu, r, mode):
    """codes and scales of the K21 format (unchanged), read by the bf16 kernels as bf16(fp16(code * s)): the bits of the bf16 call on
    lowrank_kv_dequant(codes, scales).bfloat16().  Beyond the lengths: codes 127 / -128 and scales NaN / Inf."""
    from asvd4llm_amd import ops
    B = 3
    r_v = {16: 48, 48: 272, 272: 16}[r]
    for T in (33, 129):
        for (H, H_kv), D in (((12, 3), 64), ((40, 40), 128)):
            g = torch.Generator().manual_seed(X.seed_of("k22q", r, T, H, D, mode))
            q = torch.randn(B, H, D, generator=g).to(BF).to(gpu)
            Ak = (torch.randn(H_kv * D, r, generator=g) / r ** 0.5).to(BF).to(gpu)
            Av = (torch.randn(H_kv * D, r_v, generator=g) / r_v ** 0.5).to(BF).to(gpu)
            bv = torch.randn(H_kv * D, generator=g).to(BF).to(gpu)
            ck, sk = (t.to(gpu) for t in Q.quant(Q.graded(g, (B, T, r))))
            cv, sv = (t.to(gpu) for t in Q.quant(Q.graded(g, (B, T, r_v))))
            lens = [T, T // 2, T - 1]
            for n, (code_fill, scale_fill) in enumerate(((127, float("nan")), (-128, float("inf")))):
                for b, ln in enumerate(lens):
                    for c, s in ((ck, sk), (cv, sv)):
                        c[b, ln:] = code_fill
                        s[b, ln:] = scale_fill
                dk, dv = ops.lowrank_kv_dequant(ck, sk).bfloat16(), ops.lowrank_kv_dequant(cv, sv).bfloat16()
                lens_d = torch.tensor(lens, dtype=torch.int32, device=gpu)
                rope = ops.rope_table(T, D, 10000.0, gpu) if mode == "half" else None
                key = (r, T, H, D, mode, code_fill)
                want = ops.lowrank_kv_scores(q, dk, lens_d, Ak, H_kv, D ** -0.5, rope=rope)
                got = ops.lowrank_kv_scores_q8(q, ck, sk, lens_d, Ak, H_kv, D ** -0.5, rope=rope)
                assert got.dtype == torch.float32 and torch.equal(_i32(got), _i32(want)), (key, (got != want).sum().item())
                assert got[0].abs().max().item() > 0 and torch.isfinite(got).all()
                want = ops.lowrank_kv_decode(q, dk, dv, lens_d, Ak, Av, H_kv, D ** -0.5, bv=bv, rope=rope)
                got = ops.lowrank_kv_decode_q8(q, ck, cv, sk, sv, lens_d, Ak, Av, H_kv, D ** -0.5, bv=bv, rope=rope)
                assert got.dtype == BF and torch.equal(_i16(got), _i16(want)), (key, (got != want).sum().item())
                assert torch.isfinite(got).all()
                if n == 0:   # the double rounding is real: the fp16 call on the fp16 values is another result
                    f16 = ops.lowrank_kv_decode_q8(q.half(), ck, cv, sk, sv, lens_d, Ak.half(), Av.half(), H_kv, D ** -0.5, bv=bv.half(), rope=rope)
                    assert f16.dtype == torch.float16 and not torch.equal(f16.float(), got.float())


# ---- 5. the fp16 entries keep their bits ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["none", "half"])
def test_fp16_through_the_old_entry_and_through_a16(gpu, mode):
    from asvd4llm_amd import _lib as L
    from asvd4llm_amd import ops
    H, H_kv, D, r_k, r_v, Tmax, lens = 12, 3, 64, 48, 80, 130, [130, 0, 67]
    d = _data(H, H_kv, D, r_k, r_v, Tmax, len(lens), True, X.seed_of("k22f", mode), dt=torch.float16)
    d = {k: v.to(gpu) for k, v in d.items()}
    rope = ops.rope_table(Tmax, D, 10000.0, gpu) if mode == "half" else None
    lens_d = torch.tensor(lens, dtype=torch.int32, device=gpu)
    old = ops.lowrank_kv_decode(d["q"], d["ck"], d["cv"], lens_d, d["Ak"], d["Av"], H_kv, D ** -0.5, bv=d["bv"], rope=rope)   # asvd_lowrank_kv_decode
    work = ops.lowrank_kv_work(len(lens), H, Tmax, r_k, r_v, gpu)
    new = torch.empty_like(old)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    rc = L.load(True).asvd_lowrank_kv_decode_a16(p(d["q"]), p(d["ck"]), p(d["cv"]), p(lens_d), p(d["Ak"]), p(d["Av"]), None, p(d["bv"]),
                                                 p(rope[0]) if rope else None, p(rope[1]) if rope else None, L.F16, 1 if rope else 0, D ** -0.5,
                                                 len(lens), H, H_kv, D, r_k, r_v, Tmax, d["ck"].stride(1), d["ck"].stride(0), d["cv"].stride(1),
                                                 d["cv"].stride(0), p(new), p(work), work.numel(),
                                                 ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream))
    assert rc == 0
    torch.cuda.synchronize(gpu)
    assert torch.equal(_i16(new), _i16(old)) and old[0].abs().max().item() > 0
    bf = ops.lowrank_kv_decode(*(d[k].bfloat16() for k in ("q", "ck", "cv")), lens_d, d["Ak"].bfloat16(), d["Av"].bfloat16(), H_kv, D ** -0.5,
                               bv=d["bv"].bfloat16(), rope=rope)
    assert bf.dtype == BF and not torch.equal(bf.float(), old.float())   # and the bf16 form is another function


# ---- 6. modules ---------------------------------------------------------------------------------------------------------------------------

def _attention(dev, rope_mode, seed=5, r_k=48, r_v=32, H=4):
    """BLinear weights are signed powers of two falling over the rank and the hidden states are in {-1, 0, 1}: a latent is an integer of at
    most 256 in magnitude times a power of two, EXACT in bf16, fp32 alike, so every run below holds the same cache"""
    from asvd4llm_amd import ops
    from asvd4llm_amd.kv_cache import FactorPair, LowRankKVAttention
    g = torch.Generator().manual_seed(seed)
    hid = 256
    D = hid // H
    mk = lambda i, o, b=False: nn.Linear(i, o, bias=b)

    def pair(r, bias):
        Bl, Al = mk(hid, r), mk(r, hid, bias)
        Bl.weight.data = torch.randint(-1, 2, (r, hid), generator=g).float() * (2.0 ** -(torch.arange(r) // 8).float())[:, None]
        Al.weight.data = torch.randn(hid, r, generator=g) / r ** 0.5
        return FactorPair(Bl, Al)
    q_proj, o_proj = mk(hid, hid), mk(hid, hid)
    q_proj.weight.data = torch.randn(hid, hid, generator=g) / hid ** 0.5 / 4
    o_proj.weight.data = torch.randn(hid, hid, generator=g) / hid ** 0.5
    rope = ops.rope_table(16, D, 10000.0, dev) if rope_mode == "half" else None
    att = LowRankKVAttention(q_proj, pair(r_k, False), pair(r_v, rope_mode == "none"), o_proj, H, H, rope=rope, kv_bf16=True)
    return att.to(BF).to(dev)


def _run_steps(att, hidden, dtype, kernel, quant, kv_bf16=True):
    from asvd4llm_amd.kv_cache import LowRankKVCache
    att = copy.deepcopy(att).to(dtype)
    att.kernel, att.kv_bf16 = kernel, kv_bf16
    cache = LowRankKVCache(1, hidden.shape[0], 16, att.ranks, hidden.device, dtype, quant=quant)
    with torch.no_grad():
        outs = [att.prefill(hidden[:, :7].to(dtype), cache, 0)[:, -1:]]
        for s in range(7, 12):
            outs.append(att.decode(hidden[:, s:s + 1].to(dtype), cache, 0))
    return torch.cat(outs, 1).double(), cache


@pytest.mark.parametrize("quant", [None, "int8"])
@pytest.mark.parametrize("rope_mode", ["none", "half"])
def test_attention_wrapper_decodes_bf16_on_the_kernel(gpu, rope_mode, quant):
    att = _attention(gpu, rope_mode)
    g = torch.Generator().manual_seed(6)
    hidden = torch.randint(-1, 2, (2, 12, 256), generator=g).to(BF).to(gpu)
    one = hidden[:, :1]
    assert att.refusal(one) is None
    ref, c_ref = _run_steps(att, hidden, torch.float32, False, quant)     # the wrapper's torch path in fp32
    torch_bf, c_t = _run_steps(att, hidden, BF, False, quant)             # its torch path in bf16, on the same cache
    kern, c_k = _run_steps(att, hidden, BF, True, quant)
    assert c_k.ck[0].dtype == (torch.int8 if quant else BF)
    for a, b in ((c_k, c_t), (c_k, c_ref)):                               # exact latents: one cache for all three runs
        assert torch.equal(a.ck[0][:, :12].float(), b.ck[0][:, :12].float()) and torch.equal(a.cv[0][:, :12].float(), b.cv[0][:, :12].float())
        if quant:
            assert torch.equal(_i32(a.sk[0][:, :12].contiguous()), _i32(b.sk[0][:, :12].contiguous()))
    top = ref[:, 1:].abs().max().item()
    e_k = (kern - ref)[:, 1:].abs().max().item() / top
    e_t = (torch_bf - ref)[:, 1:].abs().max().item() / top
    print(f"K22 wrapper {rope_mode} quant={quant}: e_kernel={e_k:.3e} e_torch={e_t:.3e}")
    assert e_k <= max(2 * e_t, FLOOR), (e_k, e_t)
    assert not torch.equal(kern[:, 1:], torch_bf[:, 1:])                  # the two routes are different arithmetic: the kernel did run
    assert torch.equal(kern[:, :1], torch_bf[:, :1])                      # prefill is the torch path on both
    # the switch off: "not fp16", the torch path's bits
    off = copy.deepcopy(att)
    off.kv_bf16 = False
    assert off.refusal(one) == "not fp16"
    same, _ = _run_steps(att, hidden, BF, True, quant, kv_bf16=False)
    assert torch.equal(same, torch_bf)
    # factors of another dtype
    mixed = copy.deepcopy(att)
    mixed.v_proj.ALinear.half()
    assert mixed.refusal(one) == "mixed dtypes" and att.refusal(one.float()) == "not fp16" and att.refusal(one.cpu()) == "not on the device"


def _truncated_pair(lin, r):
    from asvd4llm_amd.kv_cache import FactorPair
    U, S, Vh = torch.linalg.svd(lin.weight.data.double(), full_matrices=False)
    Bl, Al = nn.Linear(lin.in_features, r, bias=False), nn.Linear(r, lin.out_features, bias=False)
    Bl.weight.data = (S[:r].sqrt()[:, None] * Vh[:r]).to(lin.weight.dtype).contiguous()
    Al.weight.data = (U[:, :r] * S[:r].sqrt()[None, :]).to(lin.weight.dtype).contiguous()   # the kernel takes contiguous ALinear weights
    return FactorPair(Bl, Al)


@pytest.mark.parametrize("kv_quant", [None, "int8"])
def test_greedy_decode_on_the_bf16_tiny_llama(gpu, kv_quant):
    from asvd4llm_amd.kv_cache import decode_routes, greedy_decode, kv_ranks
    from asvd4llm_amd.model_zoo import random_init_model
    model = random_init_model("tiny-llama", dtype=BF, num_attention_heads=2, num_key_value_heads=2)
    for l in model.model.layers:
        l.self_attn.k_proj, l.self_attn.v_proj = _truncated_pair(l.self_attn.k_proj, 48), _truncated_pair(l.self_attn.v_proj, 32)
    model = model.to(gpu)
    assert kv_ranks(model) == [(48, 32), (48, 32)]
    assert decode_routes(model, kv_bf16=True) == ["kernel"] * 2 and decode_routes(model, kv_bf16=False) == ["not fp16"] * 2
    ids = torch.randint(0, 512, (2, 9), generator=torch.Generator().manual_seed(7)).to(gpu)
    ref_model = copy.deepcopy(model).float()
    n_new = 6
    toks, ref = greedy_decode(ref_model, ids, n_new, cache="lowrank", kernel=False, kv_quant=kv_quant)
    kw = dict(cache="lowrank", forced=toks, kv_quant=kv_quant)
    _, tor = greedy_decode(model, ids, n_new, kernel=False, kv_bf16=True, **kw)
    _, ker = greedy_decode(model, ids, n_new, kernel=True, kv_bf16=True, **kw)
    top = ref.abs().max().item()
    e_k = (ker.float() - ref).abs().max().item() / top
    e_t = (tor.float() - ref).abs().max().item() / top
    print(f"K22 greedy_decode bf16 tiny-llama kv_quant={kv_quant}: e_kernel={e_k:.3e} e_torch={e_t:.3e}")
    assert e_k <= max(2 * e_t, FLOOR), (e_k, e_t)
    assert torch.equal(ker[0], tor[0]) and not torch.equal(ker[1:], tor[1:])   # the prefill is shared, the decode steps took different arithmetic
    # the switch off: the kernel flag changes nothing for a bf16 model
    _, off_k = greedy_decode(model, ids, n_new, kernel=True, kv_bf16=False, **kw)
    _, off_t = greedy_decode(model, ids, n_new, kernel=False, kv_bf16=False, **kw)
    assert torch.equal(off_k, off_t) and torch.equal(off_t, tor)


# ---- 7. capture -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["none", "half"])
def test_bf16_decode_is_graph_capturable(gpu, mode):
    from asvd4llm_amd import ops
    H, H_kv, D, r_k, r_v, Tmax, lens = 12, 3, 64, 48, 80, 130, [130, 0, 67]
    d = _data(H, H_kv, D, r_k, r_v, Tmax, len(lens), True, X.seed_of("k22g", mode))
    d = {k: v.to(gpu) for k, v in d.items()}
    rope = ops.rope_table(Tmax, D, 10000.0, gpu) if mode == "half" else None
    lens_d = torch.tensor(lens, dtype=torch.int32, device=gpu)
    eager = _run(gpu, d, lens, H_kv, D ** -0.5, rope)
    work = ops.lowrank_kv_work(len(lens), H, Tmax, r_k, r_v, gpu)
    out = torch.zeros_like(eager)
    call = lambda: ops.lowrank_kv_decode(d["q"], d["ck"], d["cv"], lens_d, d["Ak"], d["Av"], H_kv, D ** -0.5, bv=d["bv"], rope=rope, work=work, out=out)
    s = torch.cuda.Stream(device=gpu)
    s.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(s):
        call()   # the library handle exists before capture
    torch.cuda.current_stream(gpu).wait_stream(s)
    torch.cuda.synchronize(gpu)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for _ in range(2):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize(gpu)
        assert torch.equal(_i16(out), _i16(eager))
