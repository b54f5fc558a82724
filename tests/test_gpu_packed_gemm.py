"""The token-tiled GEMM on packed RTN codes (K17: asvd_packed_gemm_f16, ops.packed_gemm, the packed_gemm switch of W8Linear / WBLinear).

1. exact data (tests/exact_data.py): every fp32 sum is exact in any order, so y must equal the fp64 expectation bit for bit;
2. random data against fp64 and F.linear on the dequantized weight, under the bar of tests/test_gpu_w8_linear.py, and two calls agree;
3. the bitstream forms return the bits of the one-code-per-byte form on the same codes;
4. a NaN / +Inf / -Inf in one token row changes that row only;
5. the module dispatch (opt-in, off by default);
6. a packed tiny model with the switch on.

The host dispatch picks a tile of 32 m tokens x 32 m features, m = 4, 2, 1, from (T, N, CU count).  On a 256-CU device the small shapes all run
m = 1 (four k groups), so the exact and the row-isolation tests add shapes with enough features for m = 2 and m = 4 (EXTRA_EXACT, ISOLATION)."""
import contextlib
import copy
import functools
import io

import pytest
import torch
import torch.nn.functional as F

from tests import exact_data as E
from tests.test_gpu_w8_linear import _check_bar

pytestmark = pytest.mark.gpu

CASES = [(bits, group) for bits in (8, 6, 4) for group in (0, 64, 128)]
MAX_CODE = {8: 255, 6: 63, 4: 15}
EXACT_T = [17, 33, 127, 128, 129, 257, 300]
EXACT_KN = [(16, 1), (48, 33), (112, 64), (128, 65), (144, 200), (352, 300), (1008, 37), (2064, 130)]
# (T, K, N) with enough tiles for m = 4 (3 x 44 tiles of 128), m = 2 (5 x 27 and 3 x 88 tiles of 64) on 256 CUs; K with a partial last step,
# and a step count that leaves k groups without a step in the last super-step
EXTRA_EXACT = [(257, 144, 5600), (300, 352, 1700), (257, 1008, 5600), (129, 2064, 5600)]


def _bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int16), b.view(torch.int16))


@functools.lru_cache(maxsize=None)
def _exact_case(T, K, N, with_bias, max_code, positive=False):
    """host data and the fp64 expectation of one exact case, computed once and shared by the group sizes (never modified)"""
    g = torch.Generator().manual_seed(E.seed_of(T, K, N, int(with_bias), max_code, int(positive)))
    x, q, scale, zero, bias = E.k12_data(g, T, K, N, with_bias, max_code, positive)
    y_ref, _, pre = E.k12_expect(x, q, scale, zero, bias)
    E.check_pre(pre)
    return x, q, scale, zero, bias, y_ref


def _params(scale, zero, K, group):
    """the row's pair, once per group: the same weight with group-wise parameters"""
    if not group:
        return scale, zero
    ng = (K + group - 1) // group
    return scale[:, None].expand(-1, ng).contiguous(), zero[:, None].expand(-1, ng).contiguous()


def _codes(q_dev, bits, offset_view=False):
    """the code tensor ops.packed_gemm takes at storage width `bits`; offset_view (bits 8): a column-offset view, row stride > K"""
    from asvd4llm_amd import ops
    if bits != 8:
        return ops.wb_pack(q_dev, bits)
    if not offset_view:
        return q_dev
    N, K = q_dev.shape
    buf = torch.full((N, K + 32), 255, dtype=torch.uint8, device=q_dev.device)
    buf[:, 16:16 + K] = q_dev
    return buf[:, 16:16 + K]


def _run_exact(gpu, T, K, N, with_bias, bits, group, offset_view=False):
    from asvd4llm_amd import ops
    x, q, scale, zero, bias, y_ref = _exact_case(T, K, N, with_bias, MAX_CODE[bits])
    s, z = _params(scale, zero, K, group)
    codes = _codes(q.to(gpu), bits, offset_view)
    y = ops.packed_gemm(x.to(gpu), codes, bits, s.to(gpu), z.to(gpu), None if bias is None else bias.to(gpu), group_size=group)
    assert _bits_equal(y.cpu(), y_ref), (T, K, N, with_bias, bits, group, offset_view, int((y.cpu() != y_ref).sum()))


# ---- 1. exact ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits,group", CASES)
def test_exact_data_bit_for_bit(gpu, bits, group):
    for K, N in EXACT_KN:
        for T in EXACT_T:
            for with_bias in (False, True):
                _run_exact(gpu, T, K, N, with_bias, bits, group)
            if bits == 8:
                _run_exact(gpu, T, K, N, bool((T + N) % 2), bits, group, offset_view=True)


@pytest.mark.parametrize("bits,group", CASES)
def test_exact_data_on_the_wider_tiles(gpu, bits, group):
    for T, K, N in EXTRA_EXACT:
        for with_bias in (False, True):
            _run_exact(gpu, T, K, N, with_bias, bits, group)
        if bits == 8:
            _run_exact(gpu, T, K, N, True, bits, group, offset_view=True)


# ---- 2. fp64 and F.linear -----------------------------------------------------------------------------------------------------------------

RANDOM_SHAPES = [(64, 4096, 4096), (200, 4096, 1024), (130, 1024, 11008), (512, 768, 3072)]


@pytest.mark.parametrize("T,K,N", RANDOM_SHAPES)
@pytest.mark.parametrize("bits,group", CASES)
def test_against_fp64_and_f_linear(gpu, bits, group, T, K, N):
    from asvd4llm_amd import ops
    g = torch.Generator(device="cuda").manual_seed(T + K + N + bits + group)
    w = (torch.randn(N, K, device="cuda", generator=g) * 0.02).half()
    x = torch.randn(T, K, device="cuda", generator=g).half()
    bias = torch.randn(N, device="cuda", generator=g).half()
    out, q, scale, zero, flagged = ops.rtn_quant(w, bits, want_params=True, group_size=group)
    assert not flagged
    codes = _codes(q, bits)
    y = ops.packed_gemm(x, codes, bits, scale, zero, bias, group_size=group)
    ref = F.linear(x, out, bias)
    exact = x.double() @ out.double().T + bias.double()
    _check_bar(y, ref, exact)
    assert torch.equal(y, ops.packed_gemm(x, codes, bits, scale, zero, bias, group_size=group))


# ---- 3. storage forms ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [6, 4])
@pytest.mark.parametrize("group", [0, 64, 128])
def test_bitstream_forms_give_the_bits_of_the_byte_form(gpu, bits, group):
    from asvd4llm_amd import ops
    for T, K, N in [(129, 352, 300), (64, 1008, 130), (300, 2064, 37), (130, 1024, 11008), (512, 768, 3072)]:
        g = torch.Generator(device="cuda").manual_seed(T + K + N + bits + group)
        w = (torch.randn(N, K, device="cuda", generator=g) * 0.02).half()
        x = torch.randn(T, K, device="cuda", generator=g).half()
        _, q, scale, zero, flagged = ops.rtn_quant(w, bits, want_params=True, group_size=group)
        assert not flagged
        y8 = ops.packed_gemm(x, q, 8, scale, zero, None, group_size=group)
        yb = ops.packed_gemm(x, ops.wb_pack(q, bits), bits, scale, zero, None, group_size=group)
        assert _bits_equal(yb, y8), (T, K, N)


# ---- 4. row isolation ---------------------------------------------------------------------------------------------------------------------

# (K, N) at T = 129: on 256 CUs m = 4 (2 x 64 tiles of 128), m = 2 (3 x 44 tiles of 64), m = 1
ISOLATION = [(144, 8100), (352, 2800), (352, 300)]
BAD = [(float("nan"), 127, 100), (float("inf"), 63, 143), (float("-inf"), 31, 0), (float("nan"), 128, 17)]   # value, token row, k


@pytest.mark.parametrize("bits,group", CASES)
def test_a_bad_value_stays_in_its_token_row(gpu, bits, group):
    from asvd4llm_amd import ops
    T = 129
    for K, N in ISOLATION:
        x, q, scale, zero, bias, y_ref = _exact_case(T, K, N, True, MAX_CODE[bits], positive=True)
        s, z = (t.to(gpu) for t in _params(scale, zero, K, group))
        codes, b = _codes(q.to(gpu), bits), bias.to(gpu)
        clean = ops.packed_gemm(x.to(gpu), codes, bits, s, z, b, group_size=group).cpu()
        assert _bits_equal(clean, y_ref)
        for value, row, k in BAD:
            xb = E.with_bad_value(x, row, k, value)
            y = ops.packed_gemm(xb.to(gpu), codes, bits, s, z, b, group_size=group).cpu()
            others = torch.arange(T) != row
            assert _bits_equal(y[others], clean[others]), (K, N, value, row)
            assert _bits_equal(y[0], clean[0]) and (row == T - 1 or _bits_equal(y[T - 1], clean[T - 1]))
            want = E.k12_row_ref(xb[row], q, scale, zero, bias)
            assert torch.equal(E.value_class(y[row]), E.value_class(want)), (K, N, value, row)
            assert int((E.value_class(want) != 0).sum()) > 0


# ---- 5. module dispatch -------------------------------------------------------------------------------------------------------------------

def _module(kind, in_f, out_f, bits, group, gpu, seed=0, bias=True):
    from asvd4llm_amd import ops
    from asvd4llm_amd.modules.w8_linear import W8Linear
    from asvd4llm_amd.modules.wb_linear import WBLinear
    g = torch.Generator(device="cuda").manual_seed(seed)
    w = (torch.randn(out_f, in_f, device="cuda", generator=g) * 0.05).half()
    b = torch.randn(out_f, device="cuda", generator=g).half() if bias else None
    _, q, scale, zero, flagged = ops.rtn_quant(w, bits, want_params=True, group_size=group)
    assert not flagged
    cls = WBLinear if kind == "wb" else W8Linear
    return cls.from_codes(q, scale, zero, b, bits, torch.float16, group_size=group)


@pytest.mark.parametrize("kind,bits,group", [("w8", 8, 0), ("w8", 6, 64), ("wb", 6, 0), ("wb", 4, 128)])
def test_module_dispatch_is_opt_in(gpu, monkeypatch, kind, bits, group):
    from asvd4llm_amd import ops
    from asvd4llm_amd.modules import packed_linear
    monkeypatch.delenv("ASVD_PACKED_GEMM", raising=False)
    m = _module(kind, 96, 80, bits, group, gpu)
    odd = _module("w8", 72, 80, 8, 0, gpu)                       # in_features % 16 != 0
    gemm, decode = [], []
    real_gemm, decode_name = ops.packed_gemm, "wb_linear" if kind == "wb" else "w8_linear"
    real_decode = getattr(ops, decode_name)
    monkeypatch.setattr(ops, "packed_gemm", lambda *a, **k: (gemm.append(a[0].shape[0]), real_gemm(*a, **k))[1])
    monkeypatch.setattr(ops, decode_name, lambda *a, **k: (decode.append(a[0].shape[0]), real_decode(*a, **k))[1])
    g = torch.Generator(device="cuda").manual_seed(5)
    x64 = torch.randn(2, 32, 96, device="cuda", generator=g).half()
    x8 = torch.randn(8, 96, device="cuda", generator=g).half()
    with torch.no_grad():
        off64, off8 = m(x64), m(x8)                                # the switch unset: today's paths
        assert gemm == [] and decode == [8]
        assert _bits_equal(off64, m._dense_forward(x64)) and off64.shape == (2, 32, 80)
        for how in ("env", "attribute"):
            if how == "env":
                monkeypatch.setenv("ASVD_PACKED_GEMM", "1")
            else:
                monkeypatch.delenv("ASVD_PACKED_GEMM")
                m.packed_gemm = odd.packed_gemm = True
            gemm.clear(), decode.clear()
            y64, y8 = m(x64), m(x8)
            assert gemm == [64] and decode == [8] and y64.shape == (2, 32, 80), how
            assert _bits_equal(y8, off8)
            exact = x64.double() @ m.dequantize().double().T + m.bias.double()
            _check_bar(y64.reshape(64, 80), off64.reshape(64, 80), exact.reshape(64, 80))
            gemm.clear()
            big = torch.randn(packed_linear.PACKED_GEMM_MAX_TOKENS + 1, 96, device="cuda", generator=g).half()
            assert _bits_equal(m(big), m._dense_forward(big)) and gemm == []            # above the maximum
            yf = m(x64.float())                                                         # not fp16
            assert yf.dtype == torch.float32 and gemm == []
            xo = torch.randn(64, 72, device="cuda", generator=g).half()
            assert _bits_equal(odd(xo), odd._dense_forward(xo)) and gemm == []          # rows without 16-byte loads
            y_max = m(big[:packed_linear.PACKED_GEMM_MAX_TOKENS])
            assert gemm == [packed_linear.PACKED_GEMM_MAX_TOKENS] and y_max.shape[0] == packed_linear.PACKED_GEMM_MAX_TOKENS
        m.packed_gemm = False
        gemm.clear()
        assert _bits_equal(m(x64), off64) and gemm == []


# ---- 6. a packed tiny model -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("storage,bits,group", [("bytes", 8, 0), ("bits", 4, 64)])
def test_packed_tiny_model_with_the_switch_on(gpu, monkeypatch, storage, bits, group):
    from asvd4llm_amd import ops
    from asvd4llm_amd.quantization import rtn_pack_sequential
    from tests.tiny_lm import TinyLM
    monkeypatch.delenv("ASVD_PACKED_GEMM", raising=False)
    model = TinyLM(d=64, f=176, n_layers=2, vocab=50, seed=3).half().to(gpu)
    with contextlib.redirect_stdout(io.StringIO()):
        n = rtn_pack_sequential(model, bits, group_size=group, **({"storage": "bits"} if storage == "bits" else {}))
    assert n == 14
    calls = []
    real = ops.packed_gemm
    monkeypatch.setattr(ops, "packed_gemm", lambda *a, **k: (calls.append(a[0].shape[0]), real(*a, **k))[1])
    ids = torch.randint(0, 50, (2, 40), generator=torch.Generator().manual_seed(11)).to(gpu)
    with torch.no_grad():
        off = model(input_ids=ids)[0]
        assert calls == []
        exact = copy.deepcopy(model).double()(input_ids=ids)[0]
        monkeypatch.setenv("ASVD_PACKED_GEMM", "1")
        on = model(input_ids=ids)[0]
    assert calls == [80] * 14 and on.shape == off.shape == (2, 40, 50) and bool(torch.isfinite(on).all())
    _check_bar(on.reshape(80, 50), off.reshape(80, 50), exact.reshape(80, 50))
