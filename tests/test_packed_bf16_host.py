"""bf16 activations on the packed-weight kernels (K19), host side: the four asvd_*_a16 entries and their argument checks, the `weight_dtype`
keyword of the ops, the opt-in switch of the modules, the dispatch predicate of the packed pair, --model_dtype, and the bf16 integer-data
generator the GPU tests (tests/test_gpu_packed_bf16.py) compare against bit for bit.  No device."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import exact_data as E
from tests.conftest import ROOT

F32, F16, BF16 = 0, 1, 2   # ASVD_F32, ASVD_F16, ASVD_BF16


# ---- the bf16 integer-data generator ---------------------------------------------------------------------------------------------------
# tests/exact_data.py's K12 recipe, restricted so that every weight is exact in bf16 (8 significant bits): x in {-1, 0, 1}; scale a power of two
# 2^-1 .. 2^-4 (no row at 4); an INTEGER zero for 8-bit codes (|q - zero| <= 255 fits 8 bits; q - (z + 1/2) would need 9), half-integer zeros only
# with codes <= 63 (|2 q - 2 z| <= 127); integer bias in -64..64.  Every term of an output is then a multiple of a unit u_n and every partial
# sum is exact in fp32 in any order while sum |x||w| / u_n < 2^24: the only rounding is the last one, fp32 -> bf16.

def bf16_data(g, T, K, N, with_bias, max_code=255, group=0, positive=False, half_zeros=True):
    """(x bf16 [T, K], q uint8 [N, K], scale, zero fp32, bias bf16 or None).  scale / zero are [N], or [N, ceil(K / group)] with one pair per
    `group` columns.  half_zeros=False: integer zeros at every width (a coarser unit, for two-stage sums).  positive: zero = 0 and codes >= 1, every weight > 0 (a +Inf in x then gives +Inf, not NaN, in fp64)."""
    x = E._ints(g, -1, 1, (T, K)).bfloat16()
    q = E._ints(g, 1 if positive else 0, max_code, (N, K))
    n = torch.arange(N)
    if K >= 2 and not positive:   # both ends of the code range in every row
        q[n, n % K] = 0
        q[n, (n + 1) % K] = max_code
    npar = N * ((K + group - 1) // group if group else 1)
    j = torch.arange(npar)
    zero = E._ints(g, 0, max_code, (npar,)).float()
    zero[j % 16 == 3] = 0.0
    zero[j % 16 == 7] = float(max_code)
    if max_code <= 63 and half_zeros:
        half = j % 16 == 11
        zero[half] = zero[half].clamp(max=max_code - 1) + 0.5
    if positive:
        zero[:] = 0.0
    scale = torch.pow(2.0, -E._ints(g, 1, 4, (npar,)).float())
    if group:
        scale, zero = scale.view(N, -1).contiguous(), zero.view(N, -1).contiguous()
    bias = E._ints(g, -64, 64, (N,)).bfloat16() if with_bias else None
    return x, q.to(torch.uint8), scale, zero, bias


def spread(p, K, group):
    """scale / zero as bf16_weight / bf16_expect take them: [N, 1] per row, [N, K] per group"""
    return p[:, None] if p.dim() == 1 else p.repeat_interleave(group, dim=1)[:, :K]


def bf16_weight(q, scale, zero):
    """fp64 w = scale (q - zero), scale / zero broadcastable against q ([N, 1] per row, [N, K] per group); asserted exact in bf16, so it IS
    the kernel's bf16 weight"""
    w = scale.double() * (q.double() - zero.double())
    assert torch.equal(w.bfloat16().double(), w), "scale * (q - zero) is not exact in bf16"
    return w


def bf16_expect(x, q, scale, zero, bias):
    """(y_ref bf16 [T, N], y64, pre); scale / zero [N] (per row) or [N, K] (spread over their columns)"""
    sc, zr = (p[:, None] if p.dim() == 1 else p for p in (scale, zero))
    w = bf16_weight(q, sc, zr)
    xd = x.double()
    y64 = xd @ w.T
    mag = xd.abs() @ w.abs().T
    unit = torch.where(zr.double() == zr.double().floor(), sc.double(), sc.double() / 2).amin(1)   # powers of two: the smallest divides all
    if bias is not None:
        y64 = y64 + bias.double()
        mag = mag + bias.double().abs()
        unit = unit.clamp(max=1.0)
    pre = {"max_n sum_k |x||w| / unit_n": ((mag / unit[None, :]).max().item(), E.LIMIT)}
    y32 = y64.float()
    assert torch.equal(y32.double(), y64), "y is not exact in fp32: the conversion would round twice"
    return y32.bfloat16(), y64, pre


def test_bf16_generator_is_exact_and_rounds():
    T, K, N = 33, 352, 70
    for max_code, with_bias in ((255, True), (63, True), (255, False)):
        g = torch.Generator().manual_seed(E.seed_of(T, K, N, max_code))
        x, q, scale, zero, bias = bf16_data(g, T, K, N, with_bias, max_code)
        assert (zero != zero.floor()).any() == (max_code <= 63)
        assert set(x.float().unique().tolist()) == {-1.0, 0.0, 1.0} and int(q.max()) == max_code and int(q.min()) == 0
        y_ref, y64, pre = bf16_expect(x, q, scale, zero, bias)
        E.check_pre(pre)
        rounded = int((y_ref.double() != y64).sum())
        print(f"max_code {max_code}: {rounded} of {y64.numel()} outputs need the bf16 rounding; pre {pre}")
        assert rounded >= y64.numel() // 4                               # the rounding path is exercised
        # CPU F.linear in bf16 on the exact weight accumulates in fp32 and rounds once: the expectation, bit for bit
        w = bf16_weight(q, scale[:, None], zero[:, None]).bfloat16()
        assert torch.equal(F.linear(x, w, bias).view(torch.int16), y_ref.view(torch.int16))
    # per group: the same argument with the smallest unit of a row
    g = torch.Generator().manual_seed(E.seed_of(T, K, N, 64))
    x, q, scale, zero, bias = bf16_data(g, T, K, N, True, 63, group=64)
    assert scale.shape == zero.shape == (N, 6) and (zero != zero.floor()).any()
    y_ref, y64, pre = bf16_expect(x, q, spread(scale, K, 64), spread(zero, K, 64), bias)
    E.check_pre(pre)
    assert int((y_ref.double() != y64).sum()) >= y64.numel() // 4
    x, q, scale, zero, bias = bf16_data(g, 4, 64, 8, False, 255, positive=True)
    assert int(q.min()) >= 1 and not zero.any() and bool((bf16_weight(q, scale[:, None], zero[:, None]) > 0).all())
    # the restriction is needed: 8-bit codes with a half-integer zero are NOT exact in bf16
    q = torch.tensor([[255, 0]], dtype=torch.uint8)
    with pytest.raises(AssertionError, match="not exact in bf16"):
        bf16_weight(q, torch.tensor([[0.5]]), torch.tensor([[0.5]]))
    # and a broken precondition is caught
    with pytest.raises(AssertionError, match="precondition"):
        E.check_pre({"x": (2.0 ** 24, E.LIMIT)})


# ---- C ABI -----------------------------------------------------------------------------------------------------------------------------

A16 = {
    "asvd_w8_linear_a16": "const void* x, int act_dtype, int64_t T, const void* q, int64_t ldq, const float* scale, const float* zero, int64_t group, "
                          "const void* bias, int64_t N, int64_t K, void* y, void* stream",
    "asvd_wb_linear_a16": "const void* x, int act_dtype, int64_t T, const void* q, int64_t ld_bytes, int bits, const float* scale, const float* zero, "
                          "int64_t group, const void* bias, int64_t N, int64_t K, void* y, void* stream",
    "asvd_packed_gemm_a16": "const void* x, int act_dtype, int64_t T, const void* q, int64_t ld_bytes, int bits, const float* scale, "
                            "const float* zero, int64_t group, const void* bias, int64_t N, int64_t K, void* y, void* stream",
    "asvd_lowrank_packed_a16": "const void* x, int act_dtype, int64_t T, const void* qB, int64_t ldB, const float* scaleB, const float* zeroB, "
                               "const void* qA, int64_t ldA, const float* scaleA, const float* zeroA, int bits, int64_t group, const void* bias, "
                               "int64_t N, int64_t K, int64_t r, void* y, void* work, size_t work_bytes, void* stream",
}
_CTYPE = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t}


def test_a16_entries_are_exported_with_the_headers_signatures(built_lib):
    from asvd4llm_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "asvd_hip.h")).read(), flags=re.S)
    for name, want in A16.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
        assert m, f"{name} is not declared in asvd_hip.h"
        params = [" ".join(p.split()) for p in m.group(1).split(",")]
        assert params == [p.strip() for p in want.split(",")], name
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and hasattr(built_lib, name)
        assert args == [ctypes.c_void_p if "*" in p else _CTYPE[p.rsplit(" ", 1)[0]] for p in params], name
    guide = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(name in guide for name in A16) and "ASVD_PACKED_BF16" in guide


def test_a16_entries_reject_bad_arguments_without_device(built_lib):
    lib = built_lib
    p, nul = ctypes.c_void_p(4096), None   # non-null but never dereferenced: every check below fails before any HIP call
    odd16, odd2 = ctypes.c_void_p(4104), ctypes.c_void_p(4097)
    bad_group = (dict(group=32), dict(group=96), dict(group=256), dict(group=-64))
    acts = (F16, BF16)

    # K12 / K14: one code per byte
    def w8(act=BF16, **kw):
        a = dict(x=p, T=4, q=p, ld=128, scale=p, zero=p, group=0, bias=nul, N=8, K=128, y=p)
        a.update(kw)
        return lib.asvd_w8_linear_a16(a["x"], act, a["T"], a["q"], a["ld"], a["scale"], a["zero"], a["group"], a["bias"], a["N"], a["K"], a["y"], nul)

    for act in acts:
        for bad in (dict(x=nul), dict(q=nul), dict(scale=nul), dict(zero=nul), dict(y=nul), dict(T=0), dict(T=257), dict(T=-1), dict(N=0), dict(K=0),
                    dict(ld=127), dict(x=odd2), dict(y=odd2), dict(bias=odd2)) + bad_group:
            assert w8(act, **bad) == -1, (act, bad)
        for group in (64, 128):   # grouped: 16-byte loads only
            for bad in (dict(K=120, ld=128), dict(x=odd16), dict(q=odd16), dict(ld=136)):
                assert w8(act, group=group, **bad) == -1, (act, group, bad)

    # K13 / K14: bitstream rows
    ldb = {6: 96, 4: 64}

    def wb(act=BF16, bits=4, **kw):
        a = dict(x=p, T=4, q=p, ld=ldb.get(bits, 64), scale=p, zero=p, group=0, bias=nul, N=8, K=128, y=p)
        a.update(kw)
        return lib.asvd_wb_linear_a16(a["x"], act, a["T"], a["q"], a["ld"], bits, a["scale"], a["zero"], a["group"], a["bias"], a["N"], a["K"],
                                      a["y"], nul)

    for act in acts:
        for bits in (6, 4):
            for bad in (dict(x=nul), dict(q=nul), dict(scale=nul), dict(zero=nul), dict(y=nul), dict(T=0), dict(T=257), dict(N=0), dict(K=0),
                        dict(K=120), dict(x=odd16), dict(q=odd16), dict(ld=ldb[bits] + 8), dict(ld=ldb[bits] - 16), dict(y=odd2),
                        dict(bias=odd2)) + bad_group:
                for group in (0, 64, 128):
                    assert wb(act, bits, **dict(dict(group=group), **bad)) == -1, (act, bits, group, bad)
        for bits in (0, 2, 5, 7, 8, 16):
            assert wb(act, bits) == -1, bits

    # K17
    ldg = {8: 128, 6: 96, 4: 64}
    top = lib.asvd_packed_gemm_max_tokens()

    def pg(act=BF16, bits=8, **kw):
        a = dict(x=p, T=64, q=p, ld=ldg.get(bits, 128), scale=p, zero=p, group=0, bias=nul, N=8, K=128, y=p)
        a.update(kw)
        return lib.asvd_packed_gemm_a16(a["x"], act, a["T"], a["q"], a["ld"], bits, a["scale"], a["zero"], a["group"], a["bias"], a["N"], a["K"],
                                        a["y"], nul)

    for act in acts:
        for bits in (8, 6, 4):
            for bad in (dict(x=nul), dict(q=nul), dict(scale=nul), dict(zero=nul), dict(y=nul), dict(T=0), dict(T=-1), dict(T=top + 1),
                        dict(K=24), dict(K=120), dict(K=0), dict(N=0), dict(x=odd16), dict(q=odd16), dict(ld=ldg[bits] + 8),
                        dict(ld=ldg[bits] - 16), dict(y=odd2), dict(bias=odd2)) + bad_group:
                for group in (0, 64, 128):
                    assert pg(act, bits, **dict(dict(group=group), **bad)) == -1, (act, bits, group, bad)
        for bits in (0, 2, 5, 7, 16, -4):
            assert pg(act, bits) == -1, bits

    # K16
    ldp = {8: (128, 64), 6: (96, 48), 4: (64, 32)}

    def lp(act=BF16, bits=8, **kw):
        a = dict(x=p, T=4, qB=p, ldB=ldp[bits][0] if bits in ldp else 128, sB=p, zB=p, qA=p, ldA=ldp[bits][1] if bits in ldp else 64, sA=p, zA=p,
                 group=0, bias=nul, N=8, K=128, r=64, y=p, work=p, nbytes=256 + 32 * 64 * 2)
        a.update(kw)
        return lib.asvd_lowrank_packed_a16(a["x"], act, a["T"], a["qB"], a["ldB"], a["sB"], a["zB"], a["qA"], a["ldA"], a["sA"], a["zA"], bits,
                                           a["group"], a["bias"], a["N"], a["K"], a["r"], a["y"], a["work"], a["nbytes"], nul)

    for act in acts:
        for bits in (8, 6, 4):
            for bad in (dict(x=nul), dict(qB=nul), dict(sB=nul), dict(zB=nul), dict(qA=nul), dict(sA=nul), dict(zA=nul), dict(y=nul),
                        dict(work=nul), dict(T=0), dict(T=257), dict(T=-1), dict(K=120), dict(K=136, ldB=160), dict(r=56), dict(r=72, ldA=96),
                        dict(K=0), dict(r=0), dict(N=0), dict(x=odd16), dict(qB=odd16), dict(qA=odd16), dict(work=odd16),
                        dict(ldB=ldp[bits][0] + 8), dict(ldA=ldp[bits][1] + 8), dict(ldB=ldp[bits][0] - 16), dict(ldA=ldp[bits][1] - 16),
                        dict(y=odd2), dict(bias=odd2)) + bad_group:
                assert lp(act, bits, **bad) == -1, (act, bits, bad)
            for group in (0, 64, 128):
                assert lp(act, bits, group=group, nbytes=256 + 32 * 64 * 2 - 1) == -2, (act, bits, group)   # ASVD_E_WORKSPACE: z is 2 bytes wide
        for bits in (0, 2, 5, 7, 16, -4):
            assert lp(act, bits) == -1, bits

    # the activation dtype: fp32 and anything that is no dtype at all, with every other argument valid
    for act in (F32, 3, -1, 16):
        assert w8(act) == -1 and wb(act) == -1 and pg(act) == -1 and lp(act) == -1, act
        for group in (64, 128):
            assert w8(act, group=group) == -1 and wb(act, group=group) == -1 and pg(act, group=group) == -1 and lp(act, group=group) == -1


# ---- ops -------------------------------------------------------------------------------------------------------------------------------

def test_ops_weight_dtype_keyword_checks_come_before_any_launch():
    from asvd4llm_amd import _lib, ops
    bf = torch.bfloat16
    x = torch.zeros(4, 64, dtype=bf)
    q8, q4 = torch.zeros(16, 64, dtype=torch.uint8), torch.zeros(16, 32, dtype=torch.uint8)
    qa8, qa4 = torch.zeros(32, 16, dtype=torch.uint8), torch.zeros(32, 32, dtype=torch.uint8)   # the A factor 16 -> 32
    s, z, sa = torch.ones(16), torch.zeros(16), torch.ones(32)
    b16, ba = torch.zeros(16, dtype=bf), torch.zeros(32, dtype=bf)
    work = torch.zeros(256 + 32 * 16 * 2, dtype=torch.uint8)
    calls = {
        "w8_linear": lambda x, bias, **k: ops.w8_linear(x, q8, s, z, bias, **k),
        "wb_linear": lambda x, bias, **k: ops.wb_linear(x, q4, 4, s, z, bias, **k),
        "packed_gemm": lambda x, bias, **k: ops.packed_gemm(x, q4, 4, s, z, bias, **k),
        "packed_gemm 8": lambda x, bias, **k: ops.packed_gemm(x, q8, 8, s, z, bias, **k),
        "pair": lambda x, bias, **k: ops.lowrank_packed_forward(x, q4, s, z, qa4, sa, sa, 4, None if bias is None else ba.to(bias.dtype), work, **k),
        "pair 8": lambda x, bias, **k: ops.lowrank_packed_forward(x, q8, s, z, qa8, sa, sa, 8, None if bias is None else ba.to(bias.dtype), work, **k),
    }
    for name, f in calls.items():
        for bad in (lambda: f(x.half(), None, weight_dtype=bf),                  # fp16 x against a bf16 weight
                    lambda: f(x, b16.half(), weight_dtype=bf),                   # fp16 bias
                    lambda: f(x.float(), None, weight_dtype=torch.float32),      # there is no fp32 kernel
                    lambda: f(x, None, weight_dtype=torch.float32),
                    lambda: f(x, None, weight_dtype=torch.float64),
                    lambda: f(x, None),                                          # without the keyword a bf16 x is still an error
                    lambda: f(x, None, weight_dtype=torch.float16),
                    lambda: f(x.half(), b16, weight_dtype=torch.float16)):       # bf16 bias against an fp16 weight
            with pytest.raises(ValueError):
                bad()
        for ok in (lambda: f(x, None, weight_dtype=bf), lambda: f(x, b16, weight_dtype=bf), lambda: f(x.half(), b16.half())):
            with pytest.raises(_lib.AsvdHipError):   # valid arguments on the CPU: there is no fallback
                ok()


# ---- modules ---------------------------------------------------------------------------------------------------------------------------

def test_switch_is_off_by_default_and_cpu_inputs_keep_the_dense_path(monkeypatch):
    from asvd4llm_amd import ops
    from asvd4llm_amd.modules import packed_linear
    from asvd4llm_amd.modules.w8_linear import W8Linear
    from asvd4llm_amd.modules.wb_linear import WBLinear
    monkeypatch.delenv("ASVD_PACKED_BF16", raising=False)
    monkeypatch.delenv("ASVD_PACKED_GEMM", raising=False)
    assert not packed_linear.packed_bf16_enabled()
    for name in ("w8_linear", "wb_linear", "packed_gemm"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: pytest.fail(f"ops.{_n} was called for a CPU input"))
    bf = torch.bfloat16
    x = torch.randn(4, 32).to(bf)
    for m in (W8Linear(32, 8, bits=8, weight_dtype=bf), WBLinear(32, 8, bits=4, weight_dtype=bf, group_size=64)):
        assert m.bias.dtype == bf and not hasattr(m, "packed_bf16")
        assert not m._kernel_dtype_ok(x) and m._kernel_input(x, 16) is None              # off: not even the dtype question passes
        dense = m(x)
        assert dense.dtype == bf and torch.equal(dense, F.linear(x, m.dequantize(), m.bias))
        monkeypatch.setenv("ASVD_PACKED_BF16", "1")
        assert packed_linear.packed_bf16_enabled() and m._kernel_dtype_ok(x)
        assert m._kernel_input(x, 16) is None and torch.equal(m(x), dense)                # on: a CPU input still takes the dense path
        assert not m._kernel_dtype_ok(x.half()) and not m._kernel_dtype_ok(x.float())     # mixed dtypes never pass
        monkeypatch.delenv("ASVD_PACKED_BF16")
        m.packed_bf16 = True
        assert m._kernel_dtype_ok(x) and m._kernel_input(x, 16) is None and torch.equal(m(x), dense)
        m.packed_gemm = True
        assert m._gemm_input(torch.zeros(64, 32, dtype=bf), 16) is None
        m.bias = m.bias.half()                                                            # a bias of another dtype than the weight
        assert not m._kernel_dtype_ok(x)
    # fp16 modules do not look at the switch, and a bf16 input to them is mixed
    m = W8Linear(32, 8, bits=8)
    assert m._kernel_dtype_ok(x.half()) and not m._kernel_dtype_ok(x)
    m.packed_bf16 = True
    assert m._kernel_dtype_ok(x.half()) and not m._kernel_dtype_ok(x)
    assert not W8Linear(32, 8, bits=8, weight_dtype=torch.float32)._kernel_dtype_ok(x.float())


def _factor(kind, in_f, out_f, bits, G, bias=False, dtype=torch.bfloat16):
    from asvd4llm_amd.modules.w8_linear import W8Linear
    from asvd4llm_amd.modules.wb_linear import WBLinear
    return (WBLinear if kind == "wb" else W8Linear)(in_f, out_f, bias=bias, bits=bits, weight_dtype=dtype, group_size=G)


def _pair(kind="wb", bits=4, G=64, K=64, r=32, N=48, a=None, b=None, dtype=torch.bfloat16):
    """an SVDLinear whose factors are CPU-built packed modules (zero codes: only the dispatch is looked at)"""
    from asvd4llm_amd.modules.svd_linear import SVDLinear
    m = SVDLinear.__new__(SVDLinear)
    nn.Module.__init__(m)
    m.BLinear = b if b is not None else _factor(kind, K, r, bits, G, dtype=dtype)
    m.ALinear = a if a is not None else _factor(kind, r, N, bits, G, bias=True, dtype=dtype)
    m.truncation_rank = r
    m.fused_packed = True
    return m


def test_pair_dispatch_predicate(monkeypatch):
    from asvd4llm_amd import ops
    monkeypatch.delenv("ASVD_FUSED_PACKED", raising=False)
    monkeypatch.delenv("ASVD_PACKED_BF16", raising=False)
    bf = torch.bfloat16
    x = torch.zeros(2, 3, 64, dtype=bf)
    with torch.no_grad():
        for kind, bits in (("wb", 4), ("wb", 6), ("w8", 8)):
            for G in (0, 64, 128):
                m = _pair(kind, bits, G)
                assert m.fused_packed_refusal(x) == "not fp16", (kind, bits, G)            # fused_packed alone: bf16 stays where it was
                m.packed_bf16 = True                                                      # both switches: everything but the device holds
                assert m.fused_packed_refusal(x) == "not on the device", (kind, bits, G)
                m.fused_packed = False
                assert m.fused_packed_refusal(x) == "switched off"
        m = _pair()
        monkeypatch.setenv("ASVD_PACKED_BF16", "1")
        assert m.fused_packed_refusal(x) == "not on the device"
        monkeypatch.delenv("ASVD_PACKED_BF16")
        assert m.fused_packed_refusal(x) == "not fp16"
        m.ALinear.packed_bf16 = True                                                      # the switch on ONE factor is not the pair's
        assert m.fused_packed_refusal(x) == "not fp16"
        m.BLinear.packed_bf16 = True
        assert m.fused_packed_refusal(x) == "not on the device"
        # every other non-fp16 case keeps its reason, with both switches on
        monkeypatch.setenv("ASVD_PACKED_BF16", "1")
        assert _pair().fused_packed_refusal(x.half()) == "not fp16"                       # fp16 input to a bf16 pair
        assert _pair().fused_packed_refusal(x.float()) == "not fp16"
        assert _pair(dtype=torch.float16).fused_packed_refusal(x) == "not fp16"           # bf16 input to an fp16 pair
        assert _pair(dtype=torch.float32).fused_packed_refusal(x.float()) == "not fp16"
        assert _pair(a=_factor("wb", 32, 48, 4, 64, dtype=torch.float16)).fused_packed_refusal(x) == "not fp16"          # mixed pairs
        assert _pair(b=_factor("wb", 64, 32, 4, 64, dtype=torch.float16)).fused_packed_refusal(x) == "not fp16"
        assert _pair(dtype=torch.float16, a=_factor("wb", 32, 48, 4, 64)).fused_packed_refusal(x.half()) == "not fp16"   # test_packed_pair_host's
        mixed_bias = _pair()
        mixed_bias.ALinear.bias = mixed_bias.ALinear.bias.half()
        assert mixed_bias.fused_packed_refusal(x) == "not fp16"
        assert _pair(dtype=torch.float16).fused_packed_refusal(x.half()) == "not on the device"                          # fp16 is untouched
        # the other questions are asked of a bf16 pair as of an fp16 one
        assert _pair().fused_packed_refusal(torch.zeros(17, 64, dtype=bf)) == "token count"
        assert _pair(K=72).fused_packed_refusal(torch.zeros(3, 72, dtype=bf)) == "code rows without 16-byte loads"
        assert _pair(b=_factor("wb", 64, 32, 4, 64, bias=True)).fused_packed_refusal(x) == "BLinear has a bias"
        # a CPU forward is the two calls
        monkeypatch.setattr(ops, "lowrank_packed_forward", lambda *a, **k: pytest.fail("no fused launch off the device"))
        m = _pair()
        xr = torch.randn(3, 64).to(bf)
        assert torch.equal(m(xr), m.ALinear(m.BLinear(xr)))


# ---- CLI -------------------------------------------------------------------------------------------------------------------------------

def test_model_dtype_flag(monkeypatch):
    import asvd
    from asvd4llm_amd import model_zoo
    p = asvd.build_parser()
    assert p.parse_args([]).model_dtype == "float16"
    assert p.parse_args(["--model_dtype", "bfloat16"]).model_dtype == "bfloat16"
    with pytest.raises(SystemExit):
        p.parse_args(["--model_dtype", "float32"])
    assert "--model_dtype" in asvd.__doc__
    seen = []

    class Stop(Exception):
        pass

    def fake(name, dtype=None, device=None):
        seen.append(dtype)
        raise Stop

    monkeypatch.setattr(model_zoo, "random_init_model", fake)
    for flag, want in (([], torch.float16), (["--model_dtype", "bfloat16"], torch.bfloat16), (["--model_dtype", "float16"], torch.float16)):
        with pytest.raises(Stop):
            asvd.build_model(p.parse_args(["--model_id", "tiny-llama", "--random_init", *flag]))
        assert seen[-1] == want
