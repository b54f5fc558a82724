"""Group-wise RTN quantization on the GPU (csrc/rtn_quant.hip and csrc/w8_linear.hip through the group_size keyword of ops, the modules,
quantization and export): the quantizer against the slice-wise restatement (tests/group_restate.py) bit for bit, the dequantization against the
quantizer's output bit for bit, the grouped forwards against the per-row kernels (tolerance-free), against exact integer-valued data and against
nn.Linear on the dequantized weight, the accuracy the feature exists for, and a model quantized to 4.5 bits per weight through the CLI pipeline,
export and back."""
import contextlib
import copy
import io
import json
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import exact_data as E
from tests.group_restate import GROUPS, graded_matrix, group_restate, n_groups, rel_err
from tests.rtn_restate import codes_of
from tests.test_gpu_rtn import DT, same, weight_like
from tests.test_gpu_w8_linear import _check_bar
from tests.test_gpu_wb_linear import FORWARD_SHAPES

pytestmark = pytest.mark.gpu

WIDTHS = [8, 6, 4]


# ---- the quantizer ------------------------------------------------------------------------------------------------------------------

def check(w, bits, G):
    from asvd4llm_amd import ops
    out, q, scale, zero, flagged = ops.rtn_quant(w, bits, want_params=True, group_size=G)
    r_out, r_q, r_scale, r_zero, ready = group_restate(w, bits, G)
    assert flagged == (not ready)
    assert out.dtype == w.dtype and out.shape == w.shape
    assert scale.shape == zero.shape == (w.shape[0], n_groups(w.shape[1], G)) and scale.is_contiguous() and zero.is_contiguous()
    assert same(out, r_out)
    assert same(scale, r_scale) and same(zero, r_zero)
    if ready:
        assert torch.equal(q.cpu(), codes_of(r_q))
    plain = ops.rtn_quant(w, bits, group_size=G)      # without the parameters: the same weight
    assert same(plain, r_out)


# a single element; one short group; ragged last groups off the vector width (1001 = 7 * 128 + 105) and on it (352 = 2 * 128 + 96); rows of many
# whole groups; rows the per-row kernel takes in two passes (20000 = 156 * 128 + 32)
QUANT_SHAPES = [(1, 1), (5, 16), (37, 1001), (3, 352), (300, 4096), (8, 20000)]


@pytest.mark.parametrize("shape", QUANT_SHAPES, ids=[f"{m}x{n}" for m, n in QUANT_SHAPES])
@pytest.mark.parametrize("dt", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("bits", WIDTHS)
@pytest.mark.parametrize("G", GROUPS)
def test_quantizer_equals_the_restatement(gpu, shape, dt, bits, G):
    w = weight_like(*shape, DT[dt], seed=shape[0] * 7 + shape[1] + bits + G).to(gpu)   # rows >= 8: zero, one-signed, constant, NaN, Inf rows
    check(w, bits, G)


@pytest.mark.parametrize("dt", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("G", GROUPS)
def test_quantizer_on_strided_views(gpu, dt, G):
    base = weight_like(60, 1300, DT[dt], seed=5 + G).to(gpu)
    check(base[:, :1024], 4, G)           # ld != cols, rows 16-byte aligned: vector path
    check(base[:, 7:1111], 4, G)          # rows start off 16-byte alignment: element path
    check(base[3:50:2, 100:1201], 6, G)   # every other row, a ragged last group


@pytest.mark.parametrize("G", GROUPS)
def test_all_zero_group_and_a_nan_in_one_group(gpu, G):
    from asvd4llm_amd import ops
    w = weight_like(12, 1104, torch.float16, seed=G, edges=False)
    w[2, G:2 * G] = 0.0                                     # an all-zero group inside a live row: xmin / xmax become -1 / +1
    w[5, 1104 - 10:] = 0.0                                  # zeros at the end of the ragged last group only: not an all-zero group
    w = w.to(gpu)
    out, q, scale, zero, flagged = ops.rtn_quant(w, 4, want_params=True, group_size=G)
    assert not flagged and same(scale[2, 1].cpu(), torch.tensor(2.0) / torch.tensor(15.0)) and bool((out[2, G:2 * G] == 0).all())
    check(w, 4, G)
    dirty = w.clone()
    dirty[7, 3 * G + 5] = float("nan")
    d_out, d_q, d_scale, d_zero, d_flagged = ops.rtn_quant(dirty, 4, want_params=True, group_size=G)
    check(dirty, 4, G)
    bad = torch.zeros(12, 1104, dtype=torch.bool)
    bad[7, 3 * G:4 * G] = True                              # the NaN poisons its own group ...
    assert torch.equal(torch.isnan(d_out).cpu(), bad) and bool(torch.isnan(d_scale[7, 3]))
    keep = ~bad.to(gpu)
    assert torch.equal(d_out[keep].view(torch.int16), out[keep].view(torch.int16))   # ... and every other group keeps the bits of the clean run
    pk = torch.ones_like(scale, dtype=torch.bool)
    pk[7, 3] = False
    assert torch.equal(d_scale[pk], scale[pk]) and torch.equal(d_zero[pk], zero[pk]) and torch.equal(d_q[keep], q[keep])


def test_a_group_of_scale_zero_flags_the_tensor(gpu):
    from asvd4llm_amd import ops
    w = weight_like(16, 512, torch.float32, seed=9, edges=False)
    w[10, 128:256] = torch.tensor([(k % 5 - 2) * 1.4e-45 for k in range(128)])   # a denormal-only GROUP: its scale is 0, the row's is not
    w = w.to(gpu)
    keep = w.clone()
    assert ops.rtn_quant(w, 4, want_params=True)[4] is False
    res = ops.rtn_quant_batched([w, keep[:8]], 4, want_params=True, group_size=128)
    assert res[0][4] is True and res[0][0] is w and torch.equal(w, keep) and res[1][4] is False
    assert same(res[1][0], group_restate(keep[:8], 4, 128)[0])
    check(w, 4, 128)
    check(w, 4, 64)


def test_group_size_is_checked(gpu):
    from asvd4llm_amd import ops
    w = torch.zeros(4, 128, device=gpu).half()
    q = torch.zeros(4, 128, dtype=torch.uint8, device=gpu)
    s1, s2 = torch.ones(4, 1, device=gpu), torch.ones(4, 2, device=gpu)
    x = torch.zeros(2, 128, device=gpu).half()
    for G in (32, 256, 1, -64):
        for bad in (lambda: ops.rtn_quant(w, 4, group_size=G), lambda: ops.w8_dequant(q, s1, s1, torch.float16, group_size=G),
                    lambda: ops.w8_linear(x, q, s1, s1, group_size=G), lambda: ops.wb_linear(x, q[:, :64], 4, s1, s1, group_size=G),
                    lambda: ops.wb_dequant(q[:, :64], 4, 128, s1, s1, torch.float16, group_size=G)):
            with pytest.raises(ValueError, match="group_size"):
                bad()
    assert ops.w8_linear(x, q, s1, s1, group_size=128).shape == (2, 4) and ops.w8_linear(x, q, s2, s2, group_size=64).shape == (2, 4)
    for bad in (lambda: ops.w8_linear(x, q, s2, s2, group_size=128), lambda: ops.w8_linear(x, q, s1, s1, group_size=64),
                lambda: ops.w8_linear(x, q, s1.view(4), s1.view(4), group_size=128), lambda: ops.w8_dequant(q, s2, s2, torch.float16, group_size=128),
                lambda: ops.wb_linear(x, q[:, :64].contiguous(), 4, s2, s2, group_size=128),
                lambda: ops.wb_dequant(q[:, :64].contiguous(), 4, 128, s1, s1, torch.float16, group_size=64),
                lambda: ops.w8_linear(x[:, :120].contiguous(), q[:, :120], s1, s1, group_size=128)):     # K % 16 != 0
        with pytest.raises(ValueError):
            bad()


# ---- dequantization -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("bits", WIDTHS)
@pytest.mark.parametrize("G", GROUPS)
def test_dequant_reproduces_the_quantizers_output(gpu, dt, bits, G):
    from asvd4llm_amd import ops
    for rows, cols, off in ((300, 4096, 8), (37, 1001, 3), (3, 352, 16), (5, 16, 5), (1, 1, 1)):
        w = weight_like(rows, cols, DT[dt], seed=rows + cols + off + bits + G, edges=False).to(gpu)
        out, q, scale, zero, flagged = ops.rtn_quant(w, bits, want_params=True, group_size=G)
        assert not flagged and bool(torch.isfinite(out).all())
        assert same(ops.w8_dequant(q, scale, zero, DT[dt], group_size=G), out)
        big = torch.full((rows, cols + 64), 7.0, dtype=DT[dt], device=gpu)
        ops.w8_dequant(q, scale, zero, DT[dt], out=big[:, off:off + cols], group_size=G)
        assert same(big[:, off:off + cols].contiguous(), out)
        assert bool((big[:, :off] == 7).all()) and bool((big[:, off + cols:] == 7).all())   # nothing written outside the view
        if bits != 8:
            qb = ops.wb_pack(q, bits)
            assert same(ops.wb_dequant(qb, bits, cols, scale, zero, DT[dt], group_size=G), out)
            big.fill_(7.0)
            ops.wb_dequant(qb, bits, cols, scale, zero, DT[dt], out=big[:, off:off + cols], group_size=G)
            assert same(big[:, off:off + cols].contiguous(), out)
            assert bool((big[:, :off] == 7).all()) and bool((big[:, off + cols:] == 7).all())


# ---- forward, tolerance-free --------------------------------------------------------------------------------------------------------

def _linear(x, q, bits, scale, zero, bias, G):
    """the forward of a width: one code per byte at 8 bits, bit-packed rows at 6 and 4"""
    from asvd4llm_amd import ops
    if bits == 8:
        return ops.w8_linear(x, q, scale, zero, bias, group_size=G)
    return ops.wb_linear(x, ops.wb_pack(q, bits), bits, scale, zero, bias, group_size=G)


def _codes(N, K, bits, g):
    return torch.randint(0, 1 << bits, (N, K), device="cuda", generator=g, dtype=torch.uint8)


def _group_params(N, K, bits, G, g):
    """random per-group scale / zero [N, ng]"""
    ng = n_groups(K, G)
    scale = torch.rand(N, ng, device="cuda", generator=g) * 0.01 + 1e-3
    zero = torch.randint(0, 1 << bits, (N, ng), device="cuda", generator=g).float()
    return scale, zero


@pytest.mark.parametrize("T,N,K", FORWARD_SHAPES)
@pytest.mark.parametrize("bits", WIDTHS)
@pytest.mark.parametrize("G", GROUPS)
def test_forward_with_one_scale_per_row_has_the_bits_of_the_per_row_kernel(gpu, T, N, K, bits, G):
    g = torch.Generator(device="cuda").manual_seed(T * 7 + N + K + bits + G)
    x = torch.randn(T, K, device="cuda", generator=g).half()
    q = _codes(N, K, bits, g)
    scale = torch.rand(N, device="cuda", generator=g) * 0.01 + 1e-3
    zero = torch.randint(0, 1 << bits, (N,), device="cuda", generator=g).float()
    ng = n_groups(K, G)
    gs, gz = scale[:, None].expand(N, ng).contiguous(), zero[:, None].expand(N, ng).contiguous()
    for bias in (None, torch.randn(N, device="cuda", generator=g).half()):
        want = _linear(x, q, bits, scale, zero, bias, 0)
        got = _linear(x, q, bits, gs, gz, bias, G)
        assert bool(torch.isfinite(want).all()) and bool((want != 0).any())
        assert torch.equal(got.view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("T,N,K", FORWARD_SHAPES)
@pytest.mark.parametrize("bits", [6, 4])
@pytest.mark.parametrize("G", GROUPS)
def test_bit_packed_grouped_forward_has_the_bits_of_the_byte_grouped_forward(gpu, T, N, K, bits, G):
    g = torch.Generator(device="cuda").manual_seed(T * 5 + N + K + bits + G)
    x = torch.randn(T, K, device="cuda", generator=g).half()
    q = _codes(N, K, bits, g)
    scale, zero = _group_params(N, K, bits, G, g)
    for bias in (None, torch.randn(N, device="cuda", generator=g).half()):
        want = _linear(x, q, 8, scale, zero, bias, G)
        got = _linear(x, q, bits, scale, zero, bias, G)
        assert bool(torch.isfinite(want).all()) and bool((want != 0).any())
        assert torch.equal(got.view(torch.int16), want.view(torch.int16))
        assert torch.equal(_linear(x, q, bits, scale, zero, bias, G).view(torch.int16), got.view(torch.int16))   # two calls: the same bits
        assert torch.equal(_linear(x, q, 8, scale, zero, bias, G).view(torch.int16), want.view(torch.int16))
    if K > G:   # the scales are really taken per group: swapping two groups' parameters changes the result
        other = scale.flip(1).contiguous()
        assert not torch.equal(_linear(x, q, bits, other, zero, None, G), _linear(x, q, bits, scale, zero, None, G))


@pytest.mark.parametrize("bits", [6, 4])
@pytest.mark.parametrize("G", GROUPS)
def test_grouped_forward_with_non_finite_activations(gpu, bits, G):
    T, N, K = 5, 100, 1104
    g = torch.Generator(device="cuda").manual_seed(31 + bits + G)
    x = torch.randn(T, K, device="cuda", generator=g).half()
    x[1, 7], x[1, 600], x[1, 1100] = float("nan"), float("inf"), float("-inf")
    x[3, K - 1] = float("inf")
    q = _codes(N, K, bits, g)
    scale, zero = _group_params(N, K, bits, G, g)
    bias = torch.randn(N, device="cuda", generator=g).half()
    want = _linear(x, q, 8, scale, zero, bias, G)
    got = _linear(x, q, bits, scale, zero, bias, G)
    assert bool(torch.isnan(want[1]).all()) and bool(torch.isfinite(want[[0, 2, 4]]).all())
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and same(got, want)
    clean = x.clone()
    clean[1], clean[3] = 0.0, 0.0
    ref = _linear(clean, q, bits, scale, zero, bias, G)
    assert torch.equal(got[[0, 2, 4]], ref[[0, 2, 4]])       # the other token rows keep their bits
    w = (scale.repeat_interleave(G, 1)[:, :K] * (q.float() - zero.repeat_interleave(G, 1)[:, :K])).half()
    y3 = x[3].double() @ w.double().T + bias.double()       # row 3: one +Inf activation: +-Inf by the sign of its weight, NaN where that is 0
    assert torch.equal(torch.isnan(got[3]), torch.isnan(y3)) and torch.equal(torch.isposinf(got[3]), torch.isposinf(y3))


# ---- forward, exact -----------------------------------------------------------------------------------------------------------------

def _exact_data(g, T, K, N, bits, G):
    """in the manner of tests/exact_data.py k12_*: x in {-1, 0, 1}; codes over the width with both ends in every row; integer zeros per group;
    per-group scales powers of two in 2^-4 .. 2^0 (spanning at most 2^4 within a row); an integer bias"""
    max_code = (1 << bits) - 1
    ng = n_groups(K, G)
    x = E._ints(g, -1, 1, (T, K)).half()
    q = E._ints(g, 0, max_code, (N, K))
    n = torch.arange(N)
    q[n, n % K] = 0
    q[n, (n + 1) % K] = max_code
    zero = E._ints(g, 0, max_code, (N, ng)).float()
    zero[n % 8 == 3] = 0.0
    zero[n % 8 == 7] = float(max_code)
    scale = torch.pow(2.0, -E._ints(g, 0, 4, (N, ng)).float())
    bias = E._ints(g, -64, 64, (N,)).half()
    return x, q.to(torch.uint8), scale, zero, bias


def _exact_expect(x, q, scale, zero, bias, G):
    """(y fp16, pre): the fp64 value rounded once.  Every term of output n is an integer multiple of min_g scale[n, g], and the bias (an integer,
    scales <= 1) as well, so the fp32 sums are exact in any order while sum |terms| / min_g scale < 2^24"""
    K = q.shape[1]
    sc, zr = (p.double().repeat_interleave(G, 1)[:, :K] for p in (scale, zero))
    w = sc * (q.double() - zr)
    assert torch.equal(w.half().double(), w), "scale * (q - zero) is not exact in fp16"
    y64 = x.double() @ w.T + bias.double()
    mag = x.double().abs() @ w.abs().T + bias.double().abs()
    unit = scale.double().min(dim=1).values
    assert float((scale.double().max(dim=1).values / unit).max()) <= 2.0 ** 4
    pre = {"max_n sum_k |x| |q - zero| scale_g / min_g scale": ((mag / unit[None, :]).max().item(), E.LIMIT)}
    return E._to_f16(y64), pre


@pytest.mark.parametrize("T,N,K", [(5, 37, 1104), (16, 64, 144)])
@pytest.mark.parametrize("bits", WIDTHS)
@pytest.mark.parametrize("G", GROUPS)
def test_grouped_forward_is_exact_on_integer_valued_data(gpu, T, N, K, bits, G):
    g = torch.Generator().manual_seed(E.seed_of("k14", T, N, K, bits, G))
    x, q, scale, zero, bias = _exact_data(g, T, K, N, bits, G)
    want, pre = _exact_expect(x, q, scale, zero, bias, G)
    E.check_pre(pre)
    got = _linear(x.to(gpu), q.to(gpu), bits, scale.to(gpu), zero.to(gpu), bias.to(gpu), G)
    assert bool((want != 0).any()) and torch.equal(got.cpu(), want)


# ---- forward, bounded ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T,N,K", [(1, 4096, 4096), (16, 4096, 1840)])
def test_grouped_forward_vs_linear_on_the_dequantized_weight_and_fp64(gpu, T, N, K):
    from asvd4llm_amd import ops
    g = torch.Generator(device="cuda").manual_seed(N + K + T)
    x = torch.randn(T, K, device="cuda", generator=g).half()
    w = (torch.randn(N, K, device="cuda", generator=g) / K ** 0.5).half()
    Wh, q, s, zr, flagged = ops.rtn_quant(w, 4, want_params=True, group_size=128)
    assert not flagged
    bias = torch.randn(N, device="cuda", generator=g).half()
    y = ops.wb_linear(x, ops.wb_pack(q, 4), 4, s, zr, bias, group_size=128)
    _check_bar(y, F.linear(x, Wh, bias), x.double() @ Wh.double().T + bias.double())


# ---- accuracy: the feature's purpose ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [0, 1, 2])
def test_groups_halve_the_four_bit_error_of_factor_shaped_weights(gpu, seed):
    from asvd4llm_amd import ops
    w = graded_matrix(seed)
    e_row = rel_err(ops.rtn_quant(w.to(gpu), 4), w)
    e128, e64 = (rel_err(ops.rtn_quant(w.to(gpu), 4, group_size=G), w) for G in (128, 64))
    print(f"seed {seed}: per row {e_row:.4f} G=128 {e128:.4f} ({e128 / e_row:.3f}x) G=64 {e64:.4f} ({e64 / e_row:.3f}x)")
    assert e128 <= 0.6 * e_row
    assert e64 <= e128
    assert e128 == rel_err(group_restate(w, 4, 128)[0], w)    # the kernel is the restatement


# ---- module dispatch ----------------------------------------------------------------------------------------------------------------

def _module_pair(kind, in_f, out_f, dtype, gpu, seed, bits, G):
    """(grouped W8Linear / WBLinear, nn.Linear holding the fake-quantized weight) of one seeded Linear"""
    from asvd4llm_amd import ops
    from asvd4llm_amd.modules.w8_linear import W8Linear
    from asvd4llm_amd.modules.wb_linear import WBLinear
    torch.manual_seed(seed)
    lin = nn.Linear(in_f, out_f, bias=True).to(dtype).to(gpu)
    out, q, scale, zero, flagged = ops.rtn_quant(lin.weight.data, bits, want_params=True, group_size=G)
    assert not flagged
    lin.weight.data = out
    cls = WBLinear if kind == "wb" else W8Linear
    return cls.from_codes(q, scale, zero, lin.bias.data, bits, dtype, group_size=G), lin


@pytest.mark.parametrize("kind,bits", [("w8", 8), ("w8", 4), ("wb", 6), ("wb", 4)])
@pytest.mark.parametrize("G", GROUPS)
def test_grouped_module_dispatch(gpu, monkeypatch, kind, bits, G):
    from asvd4llm_amd import ops
    from asvd4llm_amd.modules import w8_linear as W8
    name = "wb_linear" if kind == "wb" else "w8_linear"
    calls = []
    real = getattr(ops, name)
    monkeypatch.setattr(ops, name, lambda *a, **k: (calls.append((a[0].shape[0], k.get("group_size"))), real(*a, **k))[1])
    m, lin = _module_pair(kind, 352, 192, torch.float16, gpu, 0, bits, G)      # 352: a ragged last group at both sizes
    assert m.group_size == G and m.scales.shape == (192, n_groups(352, G)) and same(m.dequantize(), lin.weight.data)
    g = torch.Generator().manual_seed(1)

    def bar(y, ref, x):
        exact = x.double() @ lin.weight.double().T + lin.bias.double()
        _check_bar(y.reshape(-1, y.shape[-1]), ref.reshape(-1, ref.shape[-1]), exact.reshape(-1, exact.shape[-1]))

    with torch.no_grad():
        x = torch.randn(2, 7, 352, generator=g).half().to(gpu)
        y = m(x)
        assert calls == [(14, G)] and y.shape == (2, 7, 192)       # decode-sized fp16 input: the grouped kernel
        bar(y, lin(x), x)
        calls.clear()
        edge = torch.randn(W8.W8_FORWARD_MAX_TOKENS + 1, 352, generator=g).half().to(gpu)
        ye = m(edge)                                                # beyond the constant: dequantize + F.linear
        assert calls == [] and ye.shape == (W8.W8_FORWARD_MAX_TOKENS + 1, 192)
        bar(ye, lin(edge), edge)
        m(edge[:-1])
        assert calls == [(W8.W8_FORWARD_MAX_TOKENS, G)]
        calls.clear()
        mb, linb = _module_pair(kind, 352, 48, torch.bfloat16, gpu, 2, bits, G)   # a bf16 module: dequantize + F.linear
        xb = torch.randn(5, 352, generator=g).bfloat16().to(gpu)
        assert torch.equal(mb(xb), linb(xb)) and calls == []
        mo, lino = _module_pair(kind, 200, 48, torch.float16, gpu, 3, bits, G)    # in_features % 16 != 0: kept off the kernel
        xo = torch.randn(4, 200, generator=g).half().to(gpu)
        assert not mo.kernel_rows_ok() and m.kernel_rows_ok()
        assert torch.equal(mo(xo), lino(xo)) and calls == []
    xg = torch.randn(3, 352, generator=g).half().to(gpu).requires_grad_(True)
    yg = m(xg)                                                      # autograd: dequantize + F.linear, gradients reach x
    assert calls == []
    yg.sum().backward()
    xr = xg.detach().clone().requires_grad_(True)
    lin(xr).sum().backward()
    assert xg.grad is not None and torch.equal(xg.grad, xr.grad)
    bar(yg.detach(), lin(xr).detach(), xg.detach())


def test_grouped_packed_svdlinear_under_the_fused_forward_switch(gpu, monkeypatch):
    from asvd4llm_amd import ops
    from asvd4llm_amd.modules.svd_linear import SVDLinear
    from asvd4llm_amd.modules.wb_linear import WBLinear
    g = torch.Generator(device="cuda").manual_seed(21)
    A = (torch.randn(192, 64, device="cuda", generator=g) / 8).half()
    B = (torch.randn(64, 256, device="cuda", generator=g) / 16).half()
    bias = torch.randn(192, device="cuda", generator=g).half()
    (Ah, Aq, As, Az, _), (Bh, Bq, Bs, Bz, _) = ops.rtn_quant_batched([A, B], 4, want_params=True, group_size=64)
    fake = SVDLinear._from_factors(Ah, Bh, bias, 64)
    packed = SVDLinear._from_factors(Ah.clone(), Bh.clone(), bias, 64)
    packed.ALinear = WBLinear.from_codes(Aq, As, Az, bias, 4, torch.float16, group_size=64)
    packed.BLinear = WBLinear.from_codes(Bq, Bs, Bz, None, 4, torch.float16, group_size=64)
    calls = []
    real = ops.wb_linear
    monkeypatch.setattr(ops, "wb_linear", lambda *a, **k: (calls.append(k.get("group_size")), real(*a, **k))[1])
    x = torch.randn(1, 3, 256, device="cuda", generator=g).half()
    with torch.no_grad():
        monkeypatch.delenv("ASVD_FUSED_FORWARD", raising=False)
        want, ref = packed(x), fake(x)
        assert calls == [64, 64]
        calls.clear()
        monkeypatch.setenv("ASVD_FUSED_FORWARD", "1")
        y = packed(x)
        assert calls == [64, 64] and getattr(packed, "_fused", None) is None and torch.equal(y, want)   # two kernel calls, no fused copies
    exact = (x.double() @ Bh.double().T).half().double() @ Ah.double().T + bias.double()
    _check_bar(want.reshape(3, -1), ref.reshape(3, -1), exact.reshape(3, -1))


# ---- the pipeline -------------------------------------------------------------------------------------------------------------------

_PIPE = {}


def _grouped_pipeline(name, tmp_path_factory):
    """asvd.main with --weight_quant rtn_int4 --weight_quant_storage bitpacked --weight_quant_group_size 128 (the other arguments of
    tests/test_gpu_wb_linear._bitpacked_pipeline); returns the model, deep copies taken just before the step — one fake-quantized with
    rtn_quant_sequential, one packed one code per byte, both with the same groups — and the step's output"""
    if name in _PIPE:
        return _PIPE[name]
    import asvd
    from asvd4llm_amd import evaluate_utils, quantization
    seen = {}
    real_pack = quantization.rtn_pack_sequential

    def step(model, wbits, storage="bytes", group_size=0):
        seen["cmp"], seen["bytes"] = copy.deepcopy(model), copy.deepcopy(model)
        seen["model"], seen["args"] = model, (wbits, storage, group_size)
        seen["packed"] = real_pack(model, wbits, storage=storage, group_size=group_size)
        return seen["packed"]

    mp = pytest.MonkeyPatch()
    try:
        mp.setenv("ASVD_STRICT", "1")
        mp.chdir(tmp_path_factory.mktemp("g4pipe_" + name))
        mp.setattr(quantization, "rtn_pack_sequential", step)
        mp.setattr(quantization, "rtn_quant_sequential", lambda *a, **k: pytest.fail("the fake path must not run for bit-packed storage"))
        mp.setattr(evaluate_utils, "evaluate_model", lambda model, *a, **k: seen.setdefault("evaluated", {"synthetic_ppl": 0.0}))
        args = asvd.build_parser().parse_args(["--model_id", name, "--random_init", "--act_aware", "--alpha", "0.5", "--n_calib_samples", "4",
                                               "--calib_dataset", "synthetic", "--scaling_method", "abs_mean", "--param_ratio_target", "0.9",
                                               "--exclude_lm_head", "--weight_quant", "rtn_int4", "--weight_quant_storage", "bitpacked",
                                               "--weight_quant_group_size", "128"])
        out = io.StringIO()
        with contextlib.redirect_stdout(out), contextlib.redirect_stderr(io.StringIO()):
            asvd.main(args)
    finally:
        mp.undo()
    assert seen["args"] == (4, "bits", 128) and "evaluated" in seen
    with contextlib.redirect_stdout(io.StringIO()):
        quantization.rtn_quant_sequential(seen["cmp"], 4, group_size=128)
        quantization.rtn_pack_sequential(seen["bytes"], 4, group_size=128)
    seen["stdout"] = out.getvalue()
    _PIPE[name] = seen
    return seen


def _bytes(mod):
    return sum(t.numel() * t.element_size() for t in list(mod.parameters(recurse=False)) + [b for b in mod.buffers(recurse=False)])


@pytest.mark.parametrize("name", ["tiny-llama", "tiny-opt"])
def test_four_bit_grouped_pipeline_is_the_fake_quantized_model(gpu, name, tmp_path_factory, monkeypatch):
    from asvd4llm_amd import ops
    from asvd4llm_amd.modules.svd_linear import SVDLinear
    from asvd4llm_amd.modules.w8_linear import W8Linear
    from asvd4llm_amd.modules.wb_linear import WBLinear
    from asvd4llm_amd.quantization import rtn_targets
    seen = _grouped_pipeline(name, tmp_path_factory)
    model, cmp_model, bytes_model = seen["model"], seen["cmp"], seen["bytes"]
    targets = rtn_targets(cmp_model)
    assert targets and seen["packed"] == len(targets)             # a randn model flags nothing: NO target may be left unpacked
    assert f"rtn int4 g128 bit-packed: {len(targets)} weights in" in seen["stdout"]
    mods, bmods = dict(model.named_modules()), dict(bytes_model.named_modules())
    svds = [m for m in model.modules() if isinstance(m, SVDLinear)]
    assert svds and all(isinstance(m.ALinear, WBLinear) and isinstance(m.BLinear, WBLinear) for m in svds)
    packed_bytes = want_packed = want_fp16 = 0
    for n, lin in targets:
        m = mods[n]
        ng = n_groups(lin.in_features, 128)
        assert type(m) is WBLinear and m.bits == 4 and m.group_size == 128 and m.weight_dtype == torch.float16, n
        assert (m.in_features, m.out_features) == (lin.in_features, lin.out_features) and m.scales.shape == m.zeros.shape == (lin.out_features, ng), n
        assert type(bmods[n]) is W8Linear and bmods[n].group_size == 128 and same(bmods[n].scales, m.scales) and same(bmods[n].zeros, m.zeros), n
        assert bool(torch.isfinite(lin.weight).all())
        assert same(m.dequantize(), lin.weight.data), n           # bit-equal to rtn_quant_sequential(..., 4, group_size=128) on the deep copy
        bias_bytes = 0 if lin.bias is None else 2 * lin.out_features
        packed_bytes += _bytes(m)
        want_packed += lin.out_features * ops.wb_row_bytes(lin.in_features, 4) + 8 * lin.out_features * ng + bias_bytes
        want_fp16 += 2 * lin.out_features * lin.in_features
    assert packed_bytes == want_packed                             # the size is derivable: asserted exactly, 8 ng bytes of parameters per row
    assert any(lin.in_features % 128 for _, lin in targets)        # ragged last groups are part of the run
    assert f"{want_fp16} -> {want_packed - sum(0 if l.bias is None else 2 * l.out_features for _, l in targets)} bytes" in seen["stdout"]
    # a decode-sized batch: the logits of the byte-packed model with the same groups, bit for bit
    calls = []
    real = ops.wb_linear
    monkeypatch.setattr(ops, "wb_linear", lambda *a, **k: (calls.append(k.get("group_size")), real(*a, **k))[1])
    ids = torch.randint(0, model.config.vocab_size, (1, 8), generator=torch.Generator().manual_seed(11)).to(gpu)
    with torch.no_grad():
        y_bits = model(input_ids=ids)[0]
        eligible = [n for n, _ in targets if mods[n].kernel_rows_ok()]
        assert eligible and calls == [128] * len(eligible)
        y_bytes = bytes_model(input_ids=ids)[0]
    assert bool(torch.isfinite(y_bytes).all()) and torch.equal(y_bits.view(torch.int16), y_bytes.view(torch.int16))


@pytest.mark.parametrize("name", ["tiny-llama", "tiny-opt"])
def test_four_bit_grouped_model_exports_and_loads(gpu, name, tmp_path_factory, tmp_path):
    from asvd4llm_amd.export import load_asvd_repo, save_asvd_repo, truncation_ranks_of
    from asvd4llm_amd.modules.wb_linear import WBLinear
    seen = _grouped_pipeline(name, tmp_path_factory)
    model = seen["model"]
    path = str(tmp_path / "repo")
    with contextlib.redirect_stdout(io.StringIO()):
        ranks = save_asvd_repo(model, path)
    cfg = json.load(open(os.path.join(path, "config.json")))
    assert cfg["weight_quant"] == {"method": "rtn", "bits": 4, "storage": "bitstream64", "group_size": 128} and "auto_map" not in cfg
    loaded = load_asvd_repo(path, dtype=torch.float16, device=gpu)
    assert truncation_ranks_of(loaded) == ranks and ranks
    want = {n: m for n, m in model.named_modules() if isinstance(m, WBLinear)}
    have = {n: m for n, m in loaded.named_modules() if isinstance(m, WBLinear)}
    assert set(want) == set(have) and want
    for n, m in want.items():
        h = have[n]
        assert (h.bits, h.group_size, h.weight_dtype, h.in_features, h.out_features) == (4, 128, torch.float16, m.in_features, m.out_features), n
        for key in ("qbits", "scales", "zeros", "bias"):
            a, b = getattr(m, key), getattr(h, key)
            assert (a is None) == (b is None), (n, key)
            if a is not None:
                assert same(a, b), (n, key)
    ids = torch.randint(0, model.config.vocab_size, (1, 8), generator=torch.Generator().manual_seed(12)).to(gpu)
    with torch.no_grad():
        assert torch.equal(loaded(input_ids=ids)[0], model(input_ids=ids)[0])
    for other in (64, None):   # a checkpoint whose scales contradict the group size of config.json
        bad = dict(cfg, weight_quant=dict(cfg["weight_quant"]))
        if other is None:
            del bad["weight_quant"]["group_size"]
        else:
            bad["weight_quant"]["group_size"] = other
        json.dump(bad, open(os.path.join(path, "config.json"), "w"))
        with pytest.raises(ValueError, match="scales"):
            load_asvd_repo(path, dtype=torch.float16, device=gpu)
