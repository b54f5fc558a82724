"""The one-launch packed factor pair on the GPU (K16: csrc/w8_linear.hip lowrank_packed_kernel through ops.lowrank_packed_forward and the
fused_packed switch of SVDLinear).  The contract has no tolerance: the fused launch returns the bits of the two launches it replaces
(ops.w8_linear / ops.wb_linear applied twice), at every storage width and scale layout; on integer-valued data both equal the fp64 evaluation
rounded once at z and once at y."""
import contextlib
import io

import pytest
import torch
import torch.nn as nn

from tests import exact_data as E
from tests.group_restate import n_groups

pytestmark = pytest.mark.gpu

WIDTHS = [8, 6, 4]
GROUPS = [0, 64, 128]
# (T, K, r, N)
SHAPES = [
    (1, 16, 16, 1),           # no whole iteration in either phase; a single chunk
    (3, 144, 48, 37),         # one whole iteration + a 16-code tail; r < 64: a padded bitstream block, phase 2 tail-only; ragged feature tile
    (16, 1104, 208, 70),      # eight whole iterations + an 80-code tail; ragged last groups at both group sizes in both phases
    (4, 512, 1840, 264),      # a long phase-2 reduction: 14 whole iterations + 48 codes; two-iteration load groups and leftovers on every wave
    (33, 256, 64, 96),        # two token tiles, the second with one row
    (2, 64, 2688, 11008),     # more phase-2 units than CUs (a workgroup runs two units and reuses its LDS); idle workgroups in phase 1
    (2, 11008, 32, 4096),     # a long phase-1 reduction with four phase-1 units
]


def _bits_equal(a, b):
    return a.dtype == b.dtype == torch.float16 and a.shape == b.shape and torch.equal(a.view(torch.int16), b.view(torch.int16))


def _store(q, bits):
    """the code buffer of a storage width: one code per byte at 8 bits, bitstream rows at 6 and 4"""
    from asvd4llm_amd import ops
    return q if bits == 8 else ops.wb_pack(q, bits)


def _one(x, codes, bits, scale, zero, bias, G):
    from asvd4llm_amd import ops
    if bits == 8:
        return ops.w8_linear(x, codes, scale, zero, bias, group_size=G)
    return ops.wb_linear(x, codes, bits, scale, zero, bias, group_size=G)


def _two(x, pair, bits, bias, G):
    """the two launches the fused one replaces"""
    (Bc, Bs, Bz), (Ac, As, Az) = pair
    return _one(_one(x, Bc, bits, Bs, Bz, None, G), Ac, bits, As, Az, bias, G)


def _fused(x, pair, bits, bias, G, work=None):
    from asvd4llm_amd import ops
    (Bc, Bs, Bz), (Ac, As, Az) = pair
    work = ops.lowrank_packed_work(x.shape[0], Bc.shape[0], x.device) if work is None else work
    return ops.lowrank_packed_forward(x, Bc, Bs, Bz, Ac, As, Az, bits, bias, work, group_size=G)


_PAIRS = {}


def _graded_pair(K, r, N, bits, G):
    """(B, A) code buffers and parameters of a factor pair whose columns fall like logspace(0, -1.5) (what sqrt(sigma) does to ASVD factors),
    quantized by the product's quantizer; x and a bias to go with them.  One per (shape, width, group), shared by the tests."""
    from asvd4llm_amd import ops
    key = (K, r, N, bits, G)
    if key not in _PAIRS:
        if len(_PAIRS) > 8:
            _PAIRS.clear()          # the 11008-wide pairs are 30 M codes each: keep a few
        g = torch.Generator(device="cuda").manual_seed(E.seed_of(K, r, N, bits, G))
        fall = torch.logspace(0, -1.5, r, device="cuda")
        A = (torch.randn(N, r, device="cuda", generator=g) / r ** 0.5 * fall).half()
        B = (torch.randn(r, K, device="cuda", generator=g) / K ** 0.5 * fall[:, None] * 4).half()
        (_, Aq, As, Az, fa), (_, Bq, Bs, Bz, fb) = ops.rtn_quant_batched([A, B], bits, want_params=True, group_size=G)
        assert not fa and not fb
        bias = torch.randn(N, device="cuda", generator=g).half() / 8
        _PAIRS[key] = (((_store(Bq, bits), Bs, Bz), (_store(Aq, bits), As, Az)), bias, g)
    return _PAIRS[key]


# ---- 1. bit identity ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T,K,r,N", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
@pytest.mark.parametrize("bits", WIDTHS)
@pytest.mark.parametrize("G", GROUPS)
def test_fused_pair_has_the_bits_of_the_two_launches(gpu, T, K, r, N, bits, G):
    pair, bias, g = _graded_pair(K, r, N, bits, G)
    x = torch.randn(T, K, device="cuda", generator=g).half()
    for b in (None, bias):
        want = _two(x, pair, bits, b, G)
        got = _fused(x, pair, bits, b, G)
        assert bool(torch.isfinite(want).all()) and bool((want != 0).any())
        assert _bits_equal(got, want), (T, K, r, N, bits, G, b is not None, int((got.view(torch.int16) != want.view(torch.int16)).sum()))


# ---- 2. reuse and determinism -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits,G", [(8, 0), (4, 128), (6, 64)])
def test_one_workspace_serves_calls_of_different_token_counts(gpu, bits, G):
    from asvd4llm_amd import _lib, ops
    K, r, N = 1104, 208, 70
    pair, bias, g = _graded_pair(K, r, N, bits, G)
    work = ops.lowrank_packed_work(16, r, gpu)
    xs = [torch.randn(T, K, device="cuda", generator=g).half() * s for T, s in ((16, 1.0), (3, 5.0), (16, 1.0))]
    xs[2] = xs[0].clone()
    ys = [_fused(x, pair, bits, bias, G, work) for x in xs]       # stale rows of z and the barrier's generation must not reach a later result
    for x, y in zip(xs, ys):
        assert _bits_equal(y, _two(x, pair, bits, bias, G))
    assert _bits_equal(ys[0], ys[2])
    state = work[:16].view(torch.int32).tolist()
    assert state[0] == 0 and state[1] == 3 and state[2] == 0      # arrivals reset, three generations, nobody gave up
    with pytest.raises(_lib.AsvdHipError, match=r"\(-2\)"):
        _fused(torch.zeros(33, K, device="cuda").half(), pair, bits, bias, G, work)    # two token tiles do not fit a workspace of one


# ---- 3. exact data ----------------------------------------------------------------------------------------------------------------------

def _grouped(p, cols, G):
    return p if not G else p[:, None].expand(p.shape[0], n_groups(cols, G)).contiguous()


@pytest.mark.parametrize("T,K,r,N", [(4, 144, 48, 37), (16, 1104, 208, 70)])
@pytest.mark.parametrize("bits", WIDTHS)
@pytest.mark.parametrize("G", GROUPS)
def test_fused_pair_is_exact_on_integer_valued_data(gpu, T, K, r, N, bits, G):
    """k12_data for both factors (codes 0..15 and 0..3 fit every width), k12_expect composed twice: z = fp16(x wB^T) is the first rounding point, y =
    fp16(z wA^T + bias) the second.  Stage 2 sees z, a multiple of 2^-p (p <= 5: the units of stage 1), in place of integers: its precondition
    is k12_expect's with the unit scaled by 2^-p."""
    g = torch.Generator().manual_seed(E.seed_of(T, K, r, N, 16))
    x, qB, sB, zB, _ = E.k12_data(g, T, K, r, False, max_code=15)
    _, qA, sA, zA, bias = E.k12_data(g, T, r, N, True, max_code=3)      # small codes: stage 2 sums z, which is no longer in {-1, 0, 1}
    z_ref, _, pre1 = E.k12_expect(x, qB, sB, zB, None)
    E.check_pre(pre1)
    E.check_pre({"max |z| (fp16 range)": (z_ref.double().abs().max().item(), E.F16_MAX)})
    p = next(p for p in range(11) if torch.equal((z_ref.double() * 2 ** p).round(), z_ref.double() * 2 ** p))
    assert p <= 5
    y_ref, y64, pre2 = E.k12_expect(z_ref, qA, sA, zA, bias)
    E.check_pre({name + " / 2^-p": (value * 2 ** p, limit) for name, (value, limit) in pre2.items()})
    dev = lambda t: t.to(gpu)
    pair = ((_store(dev(qB), bits), _grouped(dev(sB), K, G), _grouped(dev(zB), K, G)),
            (_store(dev(qA), bits), _grouped(dev(sA), r, G), _grouped(dev(zA), r, G)))
    got = _fused(dev(x), pair, bits, dev(bias), G)
    assert _bits_equal(got.cpu(), y_ref)
    assert _bits_equal(_two(dev(x), pair, bits, dev(bias), G).cpu(), y_ref)
    if K > 1000:   # the case is worth its name: y holds entries that fp16 had to round
        assert E.round_stats(y64[torch.isfinite(y_ref)])[0] > 0


# ---- 4. non-finite rows -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits,G", [(8, 0), (4, 128), (6, 64)])
def test_non_finite_row_keeps_to_itself(gpu, bits, G):
    T, K, r, N = 5, 1104, 208, 70
    pair, bias, g = _graded_pair(K, r, N, bits, G)
    x = torch.randn(T, K, device="cuda", generator=g).half()
    bad = E.with_bad_value(E.with_bad_value(E.with_bad_value(x, 2, 7, float("nan")), 2, 600, float("inf")), 2, K - 1, float("-inf"))
    clean, got, want = _fused(x, pair, bits, bias, G), _fused(bad, pair, bits, bias, G), _two(bad, pair, bits, bias, G)
    others = [0, 1, 3, 4]
    assert _bits_equal(got[others], clean[others]) and bool(torch.isfinite(got[others]).all())
    assert bool(torch.isnan(got[2]).all()) and _bits_equal(got, want)      # the bad row: the two launches' bits


# ---- 5. the give-up word ----------------------------------------------------------------------------------------------------------------

def test_give_up_word_poisons_the_output_and_is_reported(gpu, monkeypatch):
    """never provoked: the word is set from the host"""
    from asvd4llm_amd import _lib, ops
    monkeypatch.delenv("ASVD_DEBUG", raising=False)
    T, K, r, N = 3, 1104, 208, 70
    pair, bias, g = _graded_pair(K, r, N, 4, 64)
    x = torch.randn(T, K, device="cuda", generator=g).half()
    work = ops.lowrank_packed_work(T, r, gpu)
    want = _two(x, pair, 4, bias, 64)
    assert _bits_equal(_fused(x, pair, 4, bias, 64, work), want)
    work[:16].view(torch.int32)[2] = 1
    y = _fused(x, pair, 4, bias, 64, work)
    assert y.shape == (T, N) and bool(torch.isnan(y).all())
    with pytest.raises(_lib.AsvdHipError, match="gave up"):
        ops.lowrank_check(work)
    assert int(work[:16].view(torch.int32)[2].item()) == 0
    ops.lowrank_check(work)                                              # cleared: no second report
    assert _bits_equal(_fused(x, pair, 4, bias, 64, work), want)
    monkeypatch.setenv("ASVD_DEBUG", "1")                                # every launch reads the word
    work[:16].view(torch.int32)[2] = 1
    with pytest.raises(_lib.AsvdHipError, match="gave up"):
        _fused(x, pair, 4, bias, 64, work)


# ---- 6. the module ----------------------------------------------------------------------------------------------------------------------

def _svd_pair(kind, bits, G, K=256, r=64, N=192, bits_a=None):
    from asvd4llm_amd import ops
    from asvd4llm_amd.modules.svd_linear import SVDLinear
    from asvd4llm_amd.modules.w8_linear import W8Linear
    from asvd4llm_amd.modules.wb_linear import WBLinear
    g = torch.Generator(device="cuda").manual_seed(21 + bits + G)
    A = (torch.randn(N, r, device="cuda", generator=g) / 8).half()
    B = (torch.randn(r, K, device="cuda", generator=g) / 16).half()
    bias = torch.randn(N, device="cuda", generator=g).half()
    (_, Bq, Bs, Bz, _), = ops.rtn_quant_batched([B], bits, want_params=True, group_size=G)
    (_, Aq, As, Az, _), = ops.rtn_quant_batched([A], bits_a or bits, want_params=True, group_size=G)
    cls = WBLinear if kind == "wb" else W8Linear
    m = SVDLinear._from_factors(A, B, bias, r)
    m.ALinear = cls.from_codes(Aq, As, Az, bias, bits_a or bits, torch.float16, group_size=G)
    m.BLinear = cls.from_codes(Bq, Bs, Bz, None, bits, torch.float16, group_size=G)
    return m, g


@pytest.mark.parametrize("kind,bits,G", [("w8", 8, 0), ("wb", 4, 64)])
def test_module_switch(gpu, monkeypatch, kind, bits, G):
    from asvd4llm_amd import ops
    from asvd4llm_amd.modules import svd_linear as S
    monkeypatch.delenv("ASVD_FUSED_PACKED", raising=False)
    monkeypatch.delenv("ASVD_FUSED_FORWARD", raising=False)
    calls = []
    for name in ("lowrank_packed_forward", "w8_linear", "wb_linear", "lowrank_check"):
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _n=name, _r=real, **k: (calls.append(_n), _r(*a, **k))[1])
    single = "wb_linear" if kind == "wb" else "w8_linear"
    m, g = _svd_pair(kind, bits, G)
    x = torch.randn(2, 3, 256, device="cuda", generator=g).half()
    with torch.no_grad():
        want = m(x)
        assert calls == [single, single] and not getattr(m, "_fused_packed", None)
        calls.clear()
        monkeypatch.setenv("ASVD_FUSED_FORWARD", "1")              # K10's switch alone: two calls, no padded copies
        assert _bits_equal(m(x), want) and calls == [single, single] and getattr(m, "_fused", None) is None
        assert not getattr(m, "_fused_packed", None)
        monkeypatch.delenv("ASVD_FUSED_FORWARD")
        calls.clear()
        assert m.fused_packed_refusal(x) == "switched off"
        monkeypatch.setenv("ASVD_FUSED_PACKED", "1")               # the environment variable
        assert m.fused_packed_refusal(x) is None
        y = m(x)
        assert calls == ["lowrank_packed_forward"] and y.shape == want.shape and _bits_equal(y, want)
        monkeypatch.delenv("ASVD_FUSED_PACKED")
        calls.clear()
        m.fused_packed = True                                      # the attribute
        assert _bits_equal(m(x), want) and calls == ["lowrank_packed_forward"]
        sid = torch.cuda.current_stream(gpu).cuda_stream
        assert list(m._fused_packed) == [sid] and m._fused_packed[sid].numel() == 256 + 32 * 64 * 2
        calls.clear()
        # 17 tokens and a forward hook on BLinear: two calls each (17 tokens: neither kernel, dequantize + F.linear)
        x17 = torch.randn(S.FUSED_PACKED_MAX_TOKENS + 1, 256, device="cuda", generator=g).half()
        m(x17)
        assert calls == []
        assert _bits_equal(m(x17[:-1]), m.ALinear(m.BLinear(x17[:-1]))) and calls == ["lowrank_packed_forward", single, single]
        calls.clear()
        seen = []
        h = m.BLinear.register_forward_hook(lambda mod, inp, out: seen.append(out.shape))
        assert _bits_equal(m(x), want) and calls == [single, single] and seen == [(2, 3, 64)]
        h.remove()
        calls.clear()
        off = torch.randn(3, 264, device="cuda", generator=g).half()[:, 8:]     # a strided view: made contiguous, as the factors' forward does
        assert _bits_equal(m(off), m.ALinear(m.BLinear(off))) and calls == ["lowrank_packed_forward", single, single]
        calls.clear()
        # a second stream gets a workspace of its own
        side = torch.cuda.Stream(device=gpu)
        side.wait_stream(torch.cuda.current_stream(gpu))
        with torch.cuda.stream(side):
            y2 = m(x)
        side.synchronize()
        assert _bits_equal(y2, want) and set(m._fused_packed) == {sid, side.cuda_stream}
        assert m._fused_packed[sid].data_ptr() != m._fused_packed[side.cuda_stream].data_ptr()
        calls.clear()
        m.check_fused_forward()                                    # visits both
        assert calls == ["lowrank_check", "lowrank_check"]
        m.refresh_fused()
        assert m._fused_packed == {}
        m.check_fused_forward()


def test_pair_of_different_widths_takes_two_calls(gpu, monkeypatch):
    from asvd4llm_amd import ops
    monkeypatch.delenv("ASVD_FUSED_FORWARD", raising=False)
    monkeypatch.setenv("ASVD_FUSED_PACKED", "1")
    monkeypatch.setattr(ops, "lowrank_packed_forward", lambda *a, **k: pytest.fail("a 6-bit BLinear and a 4-bit ALinear are no pair"))
    m, g = _svd_pair("wb", 6, 64, bits_a=4)
    x = torch.randn(3, 256, device="cuda", generator=g).half()
    with torch.no_grad():
        assert m.fused_packed_refusal(x) == "different storage widths"
        assert _bits_equal(m(x), m.ALinear(m.BLinear(x)))


# ---- 7. the pipeline --------------------------------------------------------------------------------------------------------------------

def test_compressed_and_packed_model_decodes_to_the_same_logits(gpu, monkeypatch):
    from asvd4llm_amd import ops
    from asvd4llm_amd.modules.svd_linear import SVDLinear
    from asvd4llm_amd.modules.wb_linear import WBLinear
    from asvd4llm_amd.quantization import _find_linears, _set_submodule, rtn_pack_sequential
    from tests.tiny_lm import TinyLM
    monkeypatch.delenv("ASVD_FUSED_PACKED", raising=False)
    monkeypatch.delenv("ASVD_FUSED_FORWARD", raising=False)
    model = TinyLM(d=64, f=176, n_layers=2, vocab=50, seed=3).half().to(gpu)
    for block in model.model.layers:
        for name, lin in _find_linears(block):
            _set_submodule(block, name, SVDLinear.from_linear(lin, 0.5, rank_align=16))
    with contextlib.redirect_stdout(io.StringIO()):
        n = rtn_pack_sequential(model, 4, storage="bits", group_size=64)
    svds = [m for m in model.modules() if isinstance(m, SVDLinear)]
    assert len(svds) == 14 and n == 28
    assert all(type(m.ALinear) is WBLinear and type(m.BLinear) is WBLinear and m.truncation_rank % 16 == 0 for m in svds)
    calls = []
    real = ops.lowrank_packed_forward
    monkeypatch.setattr(ops, "lowrank_packed_forward", lambda *a, **k: (calls.append(a[0].shape[0]), real(*a, **k))[1])
    ids = torch.randint(0, 50, (1, 3), generator=torch.Generator().manual_seed(11)).to(gpu)
    with torch.no_grad():
        want = model(input_ids=ids)[0]
        assert calls == [] and not any(getattr(m, "_fused_packed", None) for m in svds)
        monkeypatch.setenv("ASVD_FUSED_PACKED", "1")
        got = model(input_ids=ids)[0]
    assert calls == [3] * 14 and bool(torch.isfinite(want).all())
    assert _bits_equal(got, want)
    assert all(len(m._fused_packed) == 1 for m in svds)
    for m in svds:
        m.check_fused_forward()
