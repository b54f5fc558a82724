"""bf16 activations on the packed-weight kernels (K19) on the device: K12 / K13 / K14, the pair launch K16 and the token-tiled GEMM K17 in their
bf16 form.  The weight contract (the bits of ops.w8_dequant(..., torch.bfloat16)) is held by an identity probe without any tolerance; sums are
checked bit for bit on the integer data of tests/test_packed_bf16_host.py and against bf16 F.linear and fp64 on real-valued data; then the
non-finite rows, the module dispatch behind its switch, and asvd.main with --model_dtype bfloat16."""
import contextlib
import copy
import ctypes
import io

import pytest
import torch
import torch.nn.functional as F

from tests import exact_data as E
from tests.test_packed_bf16_host import bf16_data, bf16_expect, spread

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def _twice(f):
    """every call is repeated once and gives the same bits"""
    y, y2 = f(), f()
    assert _same(y, y2)
    return y


def _forward(kernel, x, q, bits, scale, zero, bias, group, dtype=BF):
    """one of the three single-layer forwards on codes q (one per byte): "decode" is K12 / K14 on byte rows at 8 storage bits and K13 / K14 on
    bitstream rows at 6 / 4; "gemm" is K17 on the same storage"""
    from asvd4llm_amd import ops
    codes = q if bits == 8 else ops.wb_pack(q, bits)
    if kernel == "gemm":
        return _twice(lambda: ops.packed_gemm(x, codes, bits, scale, zero, bias, group_size=group, weight_dtype=dtype))
    if bits == 8:
        return _twice(lambda: ops.w8_linear(x, q, scale, zero, bias, group_size=group, weight_dtype=dtype))
    return _twice(lambda: ops.wb_linear(x, codes, bits, scale, zero, bias, group_size=group, weight_dtype=dtype))


def _dev(*ts):
    return [None if t is None else t.cuda() for t in ts]


# (storage bits, largest code, group): byte rows with 8-bit and with 6-bit codes (the latter with half-integer zeros), bitstream rows, groups
VARIANTS = [(8, 255, 0), (8, 63, 0), (8, 255, 64), (8, 63, 128), (6, 63, 0), (6, 63, 64), (4, 15, 0), (4, 15, 128)]


# ---- 1. the weight is the fake quantizer's: an identity probe ------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel,T,K,bits,group", [("decode", 144, 144, 8, 0), ("decode", 256, 352, 8, 0), ("decode", 256, 352, 6, 0),
                                                    ("decode", 256, 352, 4, 0), ("decode", 256, 352, 8, 64), ("decode", 256, 352, 4, 64),
                                                    ("decode", 256, 352, 6, 128), ("decode", 256, 352, 8, 128),
                                                    ("gemm", 33, 352, 8, 0), ("gemm", 129, 352, 4, 64), ("gemm", 129, 352, 6, 128), ("gemm", 33, 144, 4, 0)])
def test_identity_probe_returns_the_dequantized_weight(gpu, kernel, T, K, bits, group):
    from asvd4llm_amd import ops
    N = 70
    g = torch.Generator(device="cuda").manual_seed(E.seed_of(T, K, bits, group))
    w = (torch.randn(N, K, device="cuda", generator=g) * (1 + 3 * torch.rand(N, 1, device="cuda", generator=g)) / K ** 0.5).to(BF)
    out, q, scale, zero, flagged = ops.rtn_quant(w, bits, want_params=True, group_size=group)
    assert not flagged and out.dtype == BF
    wd = ops.w8_dequant(q, scale, zero, BF, group_size=group)
    assert _same(wd, out)                                             # the dense weight IS the fake quantizer's output
    assert bool((torch.log2(scale) != torch.log2(scale).floor()).any()) and bool(torch.isfinite(wd).all())   # real-valued parameters
    offsets = sorted({0, max(0, K - T)} | ({(K - T) // 2} if K > 2 * T else set()))
    covered = torch.zeros(K, dtype=torch.bool)
    for off in offsets:
        x = torch.zeros(T, K, device="cuda", dtype=BF)
        t = torch.arange(min(T, K - off), device="cuda")
        x[t, t + off] = 1.0
        y = _forward(kernel, x, q, bits, scale, zero, None, group)
        assert _same(y[: len(t)], wd[:, off: off + len(t)].T.contiguous()), (off,)
        covered[off: off + len(t)] = True
    assert bool(covered.all()) or K > 2 * T


# ---- 2. integer data, bit for bit -----------------------------------------------------------------------------------------------------------

K_LIST = [16, 144, 352, 128 * 3, 128 * 9]


def _integer_case(kernel, T, K, N, bits, max_code, group, with_bias):
    from asvd4llm_amd import ops
    g = torch.Generator().manual_seed(E.seed_of(T, K, N, bits, max_code, group))
    x, q, scale, zero, bias = bf16_data(g, T, K, N, with_bias, max_code, group=group)
    y_ref, y64, pre = bf16_expect(x, q, spread(scale, K, group), spread(zero, K, group), bias)
    E.check_pre(pre)
    xd, qd, sd, zd, bd = _dev(x, q, scale, zero, bias)
    y = _forward(kernel, xd, qd, bits, sd, zd, bd, group)
    assert _same(y.cpu(), y_ref), (kernel, T, K, N, bits, max_code, group, int((y.cpu().view(torch.int16) != y_ref.view(torch.int16)).sum()))
    if bits != 8 and kernel == "decode":   # the bitstream kernel gives the bits of the byte kernel on the same codes
        assert _same(y, ops.w8_linear(xd, qd, sd, zd, bd, group_size=group, weight_dtype=BF))
    return int((y_ref.double() != y64).sum())


@pytest.mark.parametrize("T,N", E.K12_TN)
@pytest.mark.parametrize("bits,max_code,group", VARIANTS)
def test_decode_kernels_on_integer_data(gpu, T, N, bits, max_code, group):
    rounded = sum(_integer_case("decode", T, K, N, bits, max_code, group, bool((K + N) % 2)) for K in K_LIST)
    assert rounded > 0 or max_code == 15     # the last rounding is exercised (4-bit codes give sums that are mostly exact in bf16)


def test_decode_kernel_on_unaligned_rows(gpu):
    for max_code in (255, 63):
        assert _integer_case("decode", 4, 1001, 37, 8, max_code, 0, True) > 0   # K % 8 != 0: element loads throughout


@pytest.mark.parametrize("T", [17, 33, 129, 256])
@pytest.mark.parametrize("N", [70, 600])
def test_gemm_on_integer_data(gpu, T, N):
    rounded = 0
    for bits, max_code, group in VARIANTS:
        for K in (144, 352, 128 * 9):
            rounded += _integer_case("gemm", T, K, N, bits, max_code, group, bool((K + N + bits) % 2))
    assert rounded > 0


def _pair_data(T, K, r, N, group, with_bias):
    """an integer pair: z_ref = bf16(x wB^T) is the first rounding point, y_ref = bf16(z_ref wA^T + bias) the second.  The second stage sums
    products of TWO fractional factors, so the data is coarser than the single-layer recipe, within its limits: codes 0..15 at every storage width
    and integer zeros, so wB and wA are multiples of 2^-4, z (and bf16(z): rounding only drops low bits) a multiple of 2^-4, every term of y a
    multiple of 2^-8, and the fp32 sums exact while sum |z||wA| / 2^-8 < 2^24 (asserted)"""
    g = torch.Generator().manual_seed(E.seed_of(T, K, r, N, group))
    x, qB, sB, zB, _ = bf16_data(g, T, K, r, False, 15, group=group, half_zeros=False)
    _, qA, sA, zA, bias = bf16_data(g, 1, r, N, with_bias, 15, group=group, half_zeros=False)
    z_ref, z64, pre = bf16_expect(x, qB, spread(sB, K, group), spread(zB, K, group), None)
    E.check_pre(pre)
    wA = spread(sA, r, group).double() * (qA.double() - spread(zA, r, group).double())
    assert torch.equal(wA.bfloat16().double(), wA)
    zd = z_ref.double()
    assert torch.equal((zd * 16).round(), zd * 16) and torch.equal((wA * 16).round(), wA * 16)
    y64 = zd @ wA.T
    mag = zd.abs() @ wA.abs().T
    if bias is not None:
        y64, mag = y64 + bias.double(), mag + bias.double().abs()
    E.check_pre({"max sum_j |z||wA| / 2^-8": ((mag * 256).max().item(), E.LIMIT)})
    y32 = y64.float()
    assert torch.equal(y32.double(), y64)
    return (x, qB, sB, zB, qA, sA, zA, bias), z_ref, y32.bfloat16(), int((z_ref.double() != z64).sum()), int((y32.bfloat16().double() != y64).sum())


@pytest.mark.parametrize("T,K,r,N", [(5, 64, 48, 70), (16, 352, 128, 600)])
@pytest.mark.parametrize("bits,group", [(8, 0), (8, 64), (6, 0), (4, 128), (4, 64)])
def test_pair_on_integer_data_and_against_its_two_launches(gpu, T, K, r, N, bits, group):
    from asvd4llm_amd import ops
    data, z_ref, y_ref, z_rounded, y_rounded = _pair_data(T, K, r, N, group, bits != 6)
    x, qB, sB, zB, qA, sA, zA, bias = _dev(*data)
    cB, cA = (qB, qA) if bits == 8 else (ops.wb_pack(qB, bits), ops.wb_pack(qA, bits))
    work = ops.lowrank_packed_work(T, r, gpu)
    y = _twice(lambda: ops.lowrank_packed_forward(x, cB, sB, zB, cA, sA, zA, bits, bias, work, group_size=group, weight_dtype=BF))
    ops.lowrank_check(work)
    z = _forward("decode", x, qB, bits, sB, zB, None, group)
    y_two = _forward("decode", z, qA, bits, sA, zA, bias, group)
    assert _same(z.cpu(), z_ref) and _same(y_two.cpu(), y_ref)
    assert _same(y, y_two)                                            # the pair launch equals its two launches
    assert _same(y.cpu(), y_ref)
    assert y_rounded > 0 and (z_rounded > 0 or K == 64)               # both roundings to bf16 are exercised (64 terms of z stay exact)
    # the intermediate the launch left in its workspace is the bf16 z
    zw = work[256: 256 + T * r * 2].view(BF).view(T, r)
    assert _same(zw.cpu(), z_ref)


# ---- 3. the new entries with ASVD_F16 are the _f16 entries ----------------------------------------------------------------------------------

@pytest.mark.parametrize("bits,group", [(8, 0), (8, 64), (6, 0), (4, 128)])
def test_a16_entries_with_f16_return_the_bits_of_the_f16_entries(gpu, bits, group):
    from asvd4llm_amd import _lib, ops
    lib = _lib.load(True)
    T, K, r, N = 8, 352, 128, 70
    g = torch.Generator(device="cuda").manual_seed(bits + group)
    x = torch.randn(T, K, device="cuda", generator=g).half()
    x2 = torch.randn(40, K, device="cuda", generator=g).half()
    wB = (torch.randn(r, K, device="cuda", generator=g) / K ** 0.5).half()
    wA = (torch.randn(N, r, device="cuda", generator=g) / r ** 0.5).half()
    bias = torch.randn(N, device="cuda", generator=g).half()
    _, qB, sB, zB, _ = ops.rtn_quant(wB, bits, want_params=True, group_size=group)
    _, qA, sA, zA, _ = ops.rtn_quant(wA, bits, want_params=True, group_size=group)
    cB, cA = (qB, qA) if bits == 8 else (ops.wb_pack(qB, bits), ops.wb_pack(qA, bits))
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    new = lambda n=T: torch.full((n, r), float("nan"), device="cuda", dtype=torch.float16)  # noqa: E731
    ya, yf = new(), new()
    if bits == 8:
        assert lib.asvd_w8_linear_a16(p(x), _lib.F16, T, p(cB), cB.stride(0), p(sB), p(zB), group, None, r, K, p(ya), st) == 0
        if group:
            assert lib.asvd_w8_linear_grouped_f16(p(x), T, p(cB), cB.stride(0), p(sB), p(zB), group, None, r, K, p(yf), st) == 0
        else:
            assert lib.asvd_w8_linear_f16(p(x), T, p(cB), cB.stride(0), p(sB), p(zB), None, r, K, p(yf), st) == 0
    else:
        assert lib.asvd_wb_linear_a16(p(x), _lib.F16, T, p(cB), cB.stride(0), bits, p(sB), p(zB), group, None, r, K, p(ya), st) == 0
        if group:
            assert lib.asvd_wb_linear_grouped_f16(p(x), T, p(cB), cB.stride(0), bits, p(sB), p(zB), group, None, r, K, p(yf), st) == 0
        else:
            assert lib.asvd_wb_linear_f16(p(x), T, p(cB), cB.stride(0), bits, p(sB), p(zB), None, r, K, p(yf), st) == 0
    assert _same(ya, yf) and bool(torch.isfinite(ya).all())
    ga, gf = new(40), new(40)
    assert lib.asvd_packed_gemm_a16(p(x2), _lib.F16, 40, p(cB), cB.stride(0), bits, p(sB), p(zB), group, None, r, K, p(ga), st) == 0
    assert lib.asvd_packed_gemm_f16(p(x2), 40, p(cB), cB.stride(0), bits, p(sB), p(zB), group, None, r, K, p(gf), st) == 0
    assert _same(ga, gf) and bool(torch.isfinite(ga).all())
    pa, pf = (torch.full((T, N), float("nan"), device="cuda", dtype=torch.float16) for _ in range(2))
    wa, wf = ops.lowrank_packed_work(T, r, gpu), ops.lowrank_packed_work(T, r, gpu)
    args = (p(cB), cB.stride(0), p(sB), p(zB), p(cA), cA.stride(0), p(sA), p(zA), bits, group, p(bias), N, K, r)
    assert lib.asvd_lowrank_packed_a16(p(x), _lib.F16, T, *args, p(pa), p(wa), wa.numel(), st) == 0
    assert lib.asvd_lowrank_packed_f16(p(x), T, *args, p(pf), p(wf), wf.numel(), st) == 0
    assert _same(pa, pf) and bool(torch.isfinite(pa).all())
    # and a dtype that is no activation type is refused on the device as well
    assert lib.asvd_w8_linear_a16(p(x), _lib.F32, T, p(qB), qB.stride(0), p(sB), p(zB), 0, None, r, K, p(ya), st) == _lib.E_BADARG
    # the ops default is the fp16 path it always was
    if bits == 8:
        assert _same(ops.w8_linear(x, qB, sB, zB, group_size=group), ya)
    else:
        assert _same(ops.wb_linear(x, cB, bits, sB, zB, group_size=group), ya)


# ---- 4. real-valued data ------------------------------------------------------------------------------------------------------------------

def _check_bar(y, ref, exact):
    """the bar of tests/test_gpu_w8_linear.py::_check_bar with its two constants scaled by 2^3 for bf16's three fewer significand bits"""
    scale = exact.abs().max().item()
    err = (y.double() - exact).abs().max().item() / scale
    err_ref = (ref.double() - exact).abs().max().item() / scale
    diff = (y.float() - ref.float()).abs().max().item()
    print(f"err {err:.3e} err_ref {err_ref:.3e} |y - ref| {diff / scale:.3e} (relative to |exact|_max)")
    assert err <= 2 * err_ref + 2 ** -7, (err, err_ref)
    assert diff <= 3.2e-2 * scale, (diff, scale)


@pytest.mark.parametrize("T,K,N", [(3, 4096, 4096), (33, 1024, 2686)])
@pytest.mark.parametrize("bits,group", [(8, 0), (6, 64), (4, 128)])
def test_real_valued_data_against_bf16_linear_and_fp64(gpu, T, K, N, bits, group):
    from asvd4llm_amd import ops
    g = torch.Generator(device="cuda").manual_seed(T + bits)
    x = torch.randn(T, K, device="cuda", generator=g).to(BF)
    w = (torch.randn(N, K, device="cuda", generator=g) / K ** 0.5).to(BF)
    bias = torch.randn(N, device="cuda", generator=g).to(BF)
    out, q, scale, zero, flagged = ops.rtn_quant(w, bits, want_params=True, group_size=group)
    assert not flagged
    ref = F.linear(x, out, bias)
    exact = x.double() @ out.double().T + bias.double()
    for kernel in ("decode", "gemm"):
        y = _forward(kernel, x, q, bits, scale, zero, bias, group)
        assert y.dtype == BF and y.shape == (T, N)
        _check_bar(y, ref, exact)


# ---- 5. non-finite rows ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel,bits,max_code,group", [("decode", 8, 255, 0), ("decode", 4, 15, 64), ("gemm", 8, 63, 128), ("gemm", 6, 63, 0)])
def test_a_non_finite_token_row_changes_that_row_only(gpu, kernel, bits, max_code, group):
    T, K, N = 33, 1008, 70
    for value, positive, row, k in ((float("nan"), False, 32, 77), (float("inf"), True, 5, 1007), (float("-inf"), True, 0, 0)):
        g = torch.Generator().manual_seed(E.seed_of(K, N, bits, group, row))
        x, q, scale, zero, bias = bf16_data(g, T, K, N, True, max_code, group=group, positive=positive)
        xd, qd, sd, zd, bd = _dev(x, q, scale, zero, bias)
        clean = _forward(kernel, xd, qd, bits, sd, zd, bd, group)
        y_ref, _, pre = bf16_expect(x, q, spread(scale, K, group), spread(zero, K, group), bias)
        E.check_pre(pre)
        assert _same(clean.cpu(), y_ref)
        xb = E.with_bad_value(x, row, k, value)
        y = _forward(kernel, xb.cuda(), qd, bits, sd, zd, bd, group).cpu()
        others = torch.arange(T) != row
        assert _same(y[others], y_ref[others]), (value, row)          # every other row keeps its bits
        w = spread(scale, K, group).double() * (q.double() - spread(zero, K, group).double())
        want = (xb[row].double()[None, :] @ w.T + bias.double()).float().to(BF)[0]
        assert torch.equal(E.value_class(y[row]), E.value_class(want)), (value, row)
        assert int((E.value_class(want) != 0).sum()) > 0


# ---- 6. module dispatch ---------------------------------------------------------------------------------------------------------------------

def _module(kind, in_f, out_f, bits, group, seed=0, bias=True, dtype=BF):
    from asvd4llm_amd import ops
    from asvd4llm_amd.modules.w8_linear import W8Linear
    from asvd4llm_amd.modules.wb_linear import WBLinear
    g = torch.Generator(device="cuda").manual_seed(seed)
    w = (torch.randn(out_f, in_f, device="cuda", generator=g) * 0.05).to(dtype)
    b = torch.randn(out_f, device="cuda", generator=g).to(dtype) if bias else None
    _, q, scale, zero, flagged = ops.rtn_quant(w, bits, want_params=True, group_size=group)
    assert not flagged
    return (WBLinear if kind == "wb" else W8Linear).from_codes(q, scale, zero, b, bits, dtype, group_size=group)


@pytest.mark.parametrize("kind,bits,group", [("w8", 8, 0), ("w8", 6, 64), ("wb", 6, 0), ("wb", 4, 128)])
def test_module_dispatch_is_opt_in(gpu, monkeypatch, kind, bits, group):
    from asvd4llm_amd import ops
    from asvd4llm_amd.modules import packed_linear
    monkeypatch.delenv("ASVD_PACKED_BF16", raising=False)
    monkeypatch.delenv("ASVD_PACKED_GEMM", raising=False)
    m = _module(kind, 96, 80, bits, group)
    gemm, decode = [], []
    real_gemm, decode_name = ops.packed_gemm, "wb_linear" if kind == "wb" else "w8_linear"
    real_decode = getattr(ops, decode_name)
    monkeypatch.setattr(ops, "packed_gemm", lambda *a, **k: (gemm.append((a[0].shape[0], k.get("weight_dtype"))), real_gemm(*a, **k))[1])
    monkeypatch.setattr(ops, decode_name, lambda *a, **k: (decode.append((a[0].shape[0], k.get("weight_dtype"))), real_decode(*a, **k))[1])
    g = torch.Generator(device="cuda").manual_seed(5)
    x64 = torch.randn(2, 32, 96, device="cuda", generator=g).to(BF)
    x8 = torch.randn(8, 96, device="cuda", generator=g).to(BF)
    x16 = torch.randn(16, 96, device="cuda", generator=g).to(BF)
    big = torch.randn(packed_linear.PACKED_GEMM_MAX_TOKENS + 1, 96, device="cuda", generator=g).to(BF)
    with torch.no_grad():
        off64, off8 = m(x64), m(x8)                                    # switched off: no kernel call, the dense path's bits
        m.packed_gemm = True
        assert _same(m(x64), off64)                                    # the GEMM switch alone does not move a bf16 module
        m.packed_gemm = False
        assert gemm == [] and decode == []
        assert _same(off64, F.linear(x64, m.dequantize(), m.bias)) and _same(off8, F.linear(x8, m.dequantize(), m.bias))
        for how in ("env", "attribute"):
            if how == "env":
                monkeypatch.setenv("ASVD_PACKED_BF16", "1")
            else:
                monkeypatch.delenv("ASVD_PACKED_BF16")
                m.packed_bf16 = True
            gemm.clear(), decode.clear()
            y8, y16 = m(x8), m(x16)
            assert decode == [(8, BF), (16, BF)] and gemm == [] and y8.dtype == BF and y8.shape == (8, 80), how
            _check_bar(y8, off8, x8.double() @ m.dequantize().double().T + m.bias.double())
            y64 = m(x64)                                                # 64 tokens without the GEMM switch: dense
            assert _same(y64, off64) and gemm == [] and len(decode) == 2
            m.packed_gemm = True
            y64 = m(x64)
            ymax = m(big[:-1])
            assert gemm == [(64, BF), (packed_linear.PACKED_GEMM_MAX_TOKENS, BF)] and y64.shape == (2, 32, 80) and ymax.shape[0] == big.shape[0] - 1
            _check_bar(y64.reshape(64, 80), off64.reshape(64, 80), (x64.double() @ m.dequantize().double().T + m.bias.double()).reshape(64, 80))
            assert _same(m(big), F.linear(big, m.dequantize(), m.bias)) and len(gemm) == 2     # beyond the maximum: dense
            yh = m(x8.half())                                           # an fp16 input to a bf16 module keeps the dense path
            assert yh.dtype == torch.float16 and len(decode) == 2 and len(gemm) == 2
            assert _same(yh, F.linear(x8.half(), m.dequantize().half(), m.bias.half()))
            m.packed_gemm = False
        m.packed_bf16 = False
        decode.clear()
        assert _same(m(x8), off8) and decode == []
    # an fp16 module is what it was, switch or not
    monkeypatch.setenv("ASVD_PACKED_BF16", "1")
    mh = _module(kind, 96, 80, bits, group, dtype=torch.float16)
    decode.clear()
    with torch.no_grad():
        yh = mh(x8.half())
        assert decode == [(8, torch.float16)] and yh.dtype == torch.float16
        assert mh(x8).dtype == BF and len(decode) == 1                 # a bf16 input to an fp16 module: dense


@pytest.mark.parametrize("kind,bits,group", [("w8", 8, 0), ("wb", 4, 64), ("wb", 6, 128)])
def test_packed_pair_takes_the_one_launch_under_both_switches(gpu, monkeypatch, kind, bits, group):
    import torch.nn as nn
    from asvd4llm_amd import ops
    from asvd4llm_amd.modules.svd_linear import SVDLinear
    monkeypatch.delenv("ASVD_PACKED_BF16", raising=False)
    monkeypatch.delenv("ASVD_FUSED_PACKED", raising=False)
    m = SVDLinear.__new__(SVDLinear)
    nn.Module.__init__(m)
    m.BLinear = _module(kind, 352, 128, bits, group, seed=1, bias=False)
    m.ALinear = _module(kind, 128, 80, bits, group, seed=2)
    m.truncation_rank = 128
    calls = []
    for name in ("w8_linear", "wb_linear", "lowrank_packed_forward"):
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _n=name, _r=real, **k: (calls.append((_n, k.get("weight_dtype"))), _r(*a, **k))[1])
    x = torch.randn(2, 4, 352, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3)).to(BF)
    single = "wb_linear" if kind == "wb" else "w8_linear"
    with torch.no_grad():
        dense = m(x)
        assert calls == [] and m.fused_packed_refusal(x) == "switched off"
        m.fused_packed = True
        assert m.fused_packed_refusal(x) == "not fp16" and _same(m(x), dense) and calls == []
        monkeypatch.setenv("ASVD_PACKED_BF16", "1")
        m.fused_packed = False
        two = m(x)                                                     # the two module calls on their kernels
        assert calls == [(single, BF), (single, BF)] and two.shape == (2, 4, 80)
        m.fused_packed = True
        assert m.fused_packed_refusal(x) is None
        calls.clear()
        one = m(x)
        assert calls == [("lowrank_packed_forward", BF)] and _same(one, two)
        assert m.fused_packed_refusal(x.half()) == "not fp16" and m.fused_packed_refusal(torch.zeros(17, 352, device="cuda", dtype=BF)) == "token count"
        m.check_fused_forward()
    exact = (x.double() @ m.BLinear.dequantize().double().T).to(BF).double() @ m.ALinear.dequantize().double().T + m.ALinear.bias.double()
    _check_bar(one.reshape(8, 80), dense.reshape(8, 80), exact.reshape(8, 80))


# ---- 7. asvd.main --model_dtype bfloat16 ------------------------------------------------------------------------------------------------------

def test_bf16_pipeline_packs_a_bf16_model_that_reaches_the_kernels(gpu, tmp_path, monkeypatch):
    import asvd
    from asvd4llm_amd import evaluate_utils, ops, quantization
    from asvd4llm_amd.modules.svd_linear import SVDLinear
    from asvd4llm_amd.modules.wb_linear import WBLinear
    from asvd4llm_amd.quantization import rtn_targets
    seen = {}
    real_pack = quantization.rtn_pack_sequential

    def step(model, wbits, storage="bytes", group_size=0):
        seen["cmp"], seen["model"], seen["args"] = copy.deepcopy(model), model, (wbits, storage, group_size)
        seen["packed"] = real_pack(model, wbits, storage=storage, group_size=group_size)
        return seen["packed"]

    monkeypatch.delenv("ASVD_PACKED_BF16", raising=False)
    monkeypatch.setenv("ASVD_STRICT", "1")
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(quantization, "rtn_pack_sequential", step)
    monkeypatch.setattr(evaluate_utils, "evaluate_model", lambda model, *a, **k: seen.setdefault("evaluated", {"synthetic_ppl": 0.0}))
    args = asvd.build_parser().parse_args(["--model_id", "tiny-llama", "--random_init", "--model_dtype", "bfloat16", "--act_aware", "--alpha", "0.5",
                                           "--n_calib_samples", "2", "--calib_dataset", "synthetic", "--scaling_method", "abs_mean",
                                           "--param_ratio_target", "0.9", "--exclude_lm_head", "--rank_align", "16", "--weight_quant", "rtn_int4",
                                           "--weight_quant_storage", "bitpacked", "--weight_quant_group_size", "64"])
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        asvd.main(args)
    monkeypatch.setattr(quantization, "rtn_pack_sequential", real_pack)
    assert seen["args"] == (4, "bits", 64) and "evaluated" in seen
    model, cmp_model = seen["model"], seen["cmp"]
    assert all(p.dtype == BF for p in cmp_model.parameters())
    with contextlib.redirect_stdout(io.StringIO()):
        quantization.rtn_quant_sequential(cmp_model, 4, group_size=64)
    targets = rtn_targets(cmp_model)
    mods = dict(model.named_modules())
    assert targets and seen["packed"] == len(targets)
    assert any(isinstance(m, SVDLinear) for m in model.modules())
    for n, lin in targets:
        m = mods[n]
        assert type(m) is WBLinear and m.bits == 4 and m.group_size == 64 and m.weight_dtype == BF, n
        assert lin.weight.dtype == BF and _same(m.dequantize(), lin.weight.data), n     # the fake-quantized bf16 model, bit for bit
        assert m.kernel_rows_ok(), n                                                    # --rank_align 16: every layer allows 16-byte loads
    calls = []
    for name in ("wb_linear", "packed_gemm"):
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _n=name, _r=real, **k: (calls.append((_n, a[0].shape[0], k.get("weight_dtype"))), _r(*a, **k))[1])
    ids = torch.randint(0, model.config.vocab_size, (1, 4), generator=torch.Generator().manual_seed(11)).to(gpu)
    with torch.no_grad():
        off = model(input_ids=ids)[0]
        assert calls == [] and off.dtype == BF                          # off by default: dequantize + F.linear
        ref = cmp_model(input_ids=ids)[0]
        assert _same(off, ref)
        exact = copy.deepcopy(cmp_model).double()(input_ids=ids)[0]
        monkeypatch.setenv("ASVD_PACKED_BF16", "1")
        on = model(input_ids=ids)[0]
    assert calls == [("wb_linear", 4, BF)] * len(targets)               # every packed layer of every decoder block
    n_blocks = model.config.num_hidden_layers
    assert all(any(n.startswith(f"model.layers.{i}.") for n, _ in targets) for i in range(n_blocks))
    assert on.dtype == BF and bool(torch.isfinite(on).all())
    V = on.shape[-1]
    _check_bar(on.reshape(-1, V), ref.reshape(-1, V), exact.reshape(-1, V))
