"""RTN codes stored at their own width on the GPU (csrc/w8_linear.hip through ops.wb_pack / wb_dequant / wb_linear, modules/wb_linear.py,
quantization.rtn_pack_sequential(storage="bits"), export): the pack kernel writes the format of tests/bitpack_restate.py byte for byte, the
dequantization is w8_dequant on the same codes — hence the fake quantizer's output — bit for bit, the forward has the BITS of the W8A16 kernel on
the same codes, and a model bit-packed through the CLI pipeline is the fake-quantized model at the derivable size, with the logits of the
byte-packed model bit for bit, through export and back."""
import contextlib
import copy
import io
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import bitpack_restate as R
from tests.test_gpu_rtn import DT, SHAPES, same, weight_like
from tests.test_gpu_w8_linear import _check_bar, _quantized

pytestmark = pytest.mark.gpu

WIDTHS = [6, 4]


def _random_codes(N, K, bits, g):
    """(q, scale, zero) with every code of the width in use"""
    q = torch.randint(0, 1 << bits, (N, K), device="cuda", generator=g, dtype=torch.uint8)
    scale = torch.rand(N, device="cuda", generator=g) * 0.01 + 1e-3
    zero = torch.randint(0, 1 << bits, (N,), device="cuda", generator=g).float()
    return q, scale, zero


# ---- pack -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows,K", [(37, 1001), (300, 4096), (5, 16), (1, 1)])
@pytest.mark.parametrize("bits", WIDTHS)
def test_pack_equals_the_restatement(gpu, rows, K, bits):
    from asvd4llm_amd import ops
    g = torch.Generator(device="cuda").manual_seed(rows + K + bits)
    q = torch.randint(0, 1 << bits, (rows, K), device="cuda", generator=g, dtype=torch.uint8)
    want = R.pack(q.cpu().numpy(), bits)
    out = torch.full((rows, R.row_bytes(K, bits)), 0xff, dtype=torch.uint8, device="cuda")   # the padding bits must be WRITTEN as zeros
    got = ops.wb_pack(q, bits, out=out)
    assert got is out and got.shape == (rows, ops.wb_row_bytes(K, bits)) and np.array_equal(got.cpu().numpy(), want)
    codes, padding = R.unpack(got.cpu().numpy(), bits, K)
    assert np.array_equal(codes, q.cpu().numpy()) and not padding.any()
    big = torch.full((rows, K + 37), 0xff, dtype=torch.uint8, device="cuda")                 # from a strided view, neighbours of every code set
    big[:, 5:5 + K] = q
    assert np.array_equal(ops.wb_pack(big[:, 5:5 + K], bits).cpu().numpy(), want)
    assert np.array_equal(ops.wb_pack(q | 0xc0, bits).cpu().numpy(), want)                   # bits beyond the width are masked


# ---- dequantization ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=[f"{m}x{n}" for m, n in SHAPES])
@pytest.mark.parametrize("dt", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("bits", WIDTHS)
def test_dequant_equals_w8_dequant_and_the_fake_quantizers_output(gpu, shape, dt, bits):
    from asvd4llm_amd import ops
    w = weight_like(*shape, DT[dt], seed=shape[0] * 5 + shape[1] + bits, edges=False).to(gpu)
    out, q, scale, zero, flagged = ops.rtn_quant(w, bits, want_params=True)
    assert not flagged and bool(torch.isfinite(out).all())
    back = ops.wb_dequant(ops.wb_pack(q, bits), bits, shape[1], scale, zero, DT[dt])
    assert same(back, ops.w8_dequant(q, scale, zero, DT[dt])) and same(back, out)


@pytest.mark.parametrize("dt", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("bits", WIDTHS)
def test_dequant_into_a_strided_destination(gpu, dt, bits):
    from asvd4llm_amd import ops
    for rows, cols, off in ((300, 4096, 8), (300, 4096, 3), (37, 1001, 5), (3, 1, 1)):
        w = weight_like(rows, cols, DT[dt], seed=rows + cols + off, edges=False).to(gpu)
        out, q, scale, zero, flagged = ops.rtn_quant(w, bits, want_params=True)
        qb = ops.wb_pack(q, bits)
        big = torch.full((rows, cols + 64), 7.0, dtype=DT[dt], device=gpu)
        ops.wb_dequant(qb, bits, cols, scale, zero, DT[dt], out=big[:, off:off + cols])
        assert same(big[:, off:off + cols].contiguous(), out)
        assert bool((big[:, :off] == 7).all()) and bool((big[:, off + cols:] == 7).all())   # nothing written outside the view
        wide = torch.zeros((rows, qb.shape[1] + 16), dtype=torch.uint8, device=gpu)         # rows with a leading dimension
        wide[:, :qb.shape[1]] = qb
        assert same(ops.wb_dequant(wide[:, :qb.shape[1]], bits, cols, scale, zero, DT[dt]), out)


@pytest.mark.parametrize("bits", WIDTHS)
def test_dequant_with_unit_scale_returns_the_codes(gpu, bits):
    from asvd4llm_amd import ops
    g = torch.Generator(device="cuda").manual_seed(bits)
    q = torch.randint(0, 1 << bits, (9, 1001), device="cuda", generator=g, dtype=torch.uint8)
    one, nought = torch.ones(9, device="cuda"), torch.zeros(9, device="cuda")
    assert torch.equal(ops.wb_dequant(ops.wb_pack(q, bits), bits, 1001, one, nought, torch.float32), q.float())


# ---- forward ----------------------------------------------------------------------------------------------------------------------

# one partial chunk; a missing g = 1 block; exactly one iteration; a tail after whole iterations; all four waves busy; the two-iteration load
# groups (from K = 1024); five tail chunks.  T = 33: a second token tile with one valid row; feature tiles 8 wide at small N, 32 wide at
# T = 256, N = 1029
FORWARD_SHAPES = [(1, 1, 16), (5, 37, 48), (2, 8, 64), (3, 300, 128), (16, 64, 144), (33, 37, 512), (4, 128, 1024), (7, 100, 1104), (256, 1029, 144),
                  (1, 4096, 1840)]


@pytest.mark.parametrize("T,N,K", FORWARD_SHAPES)
@pytest.mark.parametrize("bits", WIDTHS)
def test_forward_has_the_bits_of_the_w8_kernel(gpu, T, N, K, bits):
    from asvd4llm_amd import ops
    g = torch.Generator(device="cuda").manual_seed(T * 7 + N + K + bits)
    x = torch.randn(T, K, device="cuda", generator=g).half()
    q, scale, zero = _random_codes(N, K, bits, g)
    qb = ops.wb_pack(q, bits)
    for bias in (None, torch.randn(N, device="cuda", generator=g).half()):
        want = ops.w8_linear(x, q, scale, zero, bias)
        got = ops.wb_linear(x, qb, bits, scale, zero, bias)
        assert bool(torch.isfinite(want).all()) and bool((want != 0).any())
        assert torch.equal(got.view(torch.int16), want.view(torch.int16))
        assert torch.equal(ops.wb_linear(x, qb, bits, scale, zero, bias).view(torch.int16), got.view(torch.int16))   # two calls: the same bits


@pytest.mark.parametrize("bits", WIDTHS)
def test_forward_with_non_finite_activations(gpu, bits):
    from asvd4llm_amd import ops
    T, N, K = 5, 100, 1104
    g = torch.Generator(device="cuda").manual_seed(31 + bits)
    x = torch.randn(T, K, device="cuda", generator=g).half()
    x[1, 7], x[1, 600], x[1, 1100] = float("nan"), float("inf"), float("-inf")
    x[3, K - 1] = float("inf")
    q, scale, zero = _random_codes(N, K, bits, g)
    bias = torch.randn(N, device="cuda", generator=g).half()
    want = ops.w8_linear(x, q, scale, zero, bias)
    got = ops.wb_linear(x, ops.wb_pack(q, bits), bits, scale, zero, bias)
    assert bool(torch.isnan(want[1]).all()) and bool(torch.isfinite(want[[0, 2, 4]]).all())
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and same(got, want)


@pytest.mark.parametrize("T,N,K", [(1, 4096, 4096), (16, 4096, 1840)])
@pytest.mark.parametrize("bits", WIDTHS)
def test_forward_vs_the_fake_quantized_linear_and_fp64(gpu, T, N, K, bits):
    from asvd4llm_amd import ops
    g = torch.Generator(device="cuda").manual_seed(N + K + T + bits)
    x = torch.randn(T, K, device="cuda", generator=g).half()
    Wh, q, s, zr = _quantized(N, K, g, bits)
    bias = torch.randn(N, device="cuda", generator=g).half()
    y = ops.wb_linear(x, ops.wb_pack(q, bits), bits, s, zr, bias)
    _check_bar(y, F.linear(x, Wh, bias), x.double() @ Wh.double().T + bias.double())


def test_ops_argument_checks(gpu):
    from asvd4llm_amd import _lib, ops
    x = torch.zeros(4, 64, device="cuda").half()
    qb = torch.zeros(8, 48, dtype=torch.uint8, device="cuda")
    s = torch.ones(8, device="cuda")
    assert ops.wb_linear(x, qb, 6, s, s).shape == (4, 8)
    for bad in (lambda: ops.wb_linear(torch.zeros(257, 64, device="cuda").half(), qb, 6, s, s),
                lambda: ops.wb_linear(x.float(), qb, 6, s, s),
                lambda: ops.wb_linear(x, qb, 4, s, s),                       # 48-byte rows are not 64 codes of 4 bits
                lambda: ops.wb_linear(x, qb, 8, s, s),
                lambda: ops.wb_linear(x[:, :56].contiguous(), qb, 6, s, s),  # K % 16 != 0
                lambda: ops.wb_linear(x, qb, 6, s[:4], s)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(ValueError):
        ops.wb_linear(x.view(-1)[4:4 + 3 * 64].view(3, 64), qb, 6, s, s)     # x 8 bytes off 16-byte alignment
    with pytest.raises(ValueError):
        ops.wb_dequant(qb, 6, 65, s, s, torch.float16)                      # 65 codes need two blocks
    with pytest.raises(ValueError):
        ops.wb_pack(qb.float(), 6)
    with pytest.raises(ValueError):
        ops.wb_pack(qb, 5)
    with pytest.raises(_lib.AsvdHipError):
        ops.wb_linear(x.cpu(), qb, 6, s, s)


# ---- module dispatch --------------------------------------------------------------------------------------------------------------

def _module_pair(in_f, out_f, dtype, gpu, seed, bits=6, bias=True):
    """(WBLinear, nn.Linear holding the fake-quantized weight) of one seeded Linear"""
    from asvd4llm_amd import ops
    from asvd4llm_amd.modules.wb_linear import WBLinear
    torch.manual_seed(seed)
    lin = nn.Linear(in_f, out_f, bias=bias).to(dtype).to(gpu)
    out, q, scale, zero, flagged = ops.rtn_quant(lin.weight.data, bits, want_params=True)
    assert not flagged
    lin.weight.data = out
    return WBLinear.from_codes(q, scale, zero, lin.bias.data if bias else None, bits, dtype), lin


@pytest.mark.parametrize("bits", WIDTHS)
def test_module_dispatch(gpu, monkeypatch, bits):
    from asvd4llm_amd import ops
    from asvd4llm_amd.modules import wb_linear as W
    from asvd4llm_amd.modules.w8_linear import W8Linear
    calls = []
    real = ops.wb_linear
    monkeypatch.setattr(ops, "wb_linear", lambda *a, **k: (calls.append(a[0].shape[0]), real(*a, **k))[1])
    m, lin = _module_pair(256, 192, torch.float16, gpu, 0, bits)
    assert same(m.dequantize(), lin.weight.data) and m.qbits.shape == (192, R.row_bytes(256, bits))
    g = torch.Generator().manual_seed(1)

    def bar(y, ref, x, mod_ref):
        exact = x.double() @ mod_ref.weight.double().T + mod_ref.bias.double()
        _check_bar(y.reshape(-1, y.shape[-1]), ref.reshape(-1, ref.shape[-1]), exact.reshape(-1, exact.shape[-1]))

    with torch.no_grad():
        x = torch.randn(2, 7, 256, generator=g).half().to(gpu)
        y = m(x)
        assert calls == [14] and y.shape == (2, 7, 192)          # decode-sized fp16 input: the kernel
        bar(y, lin(x), x, lin)
        m8 = W8Linear.from_codes(m.codes(), m.scales, m.zeros, m.bias, bits, torch.float16)
        assert torch.equal(y, m8(x))                              # the byte-packed module's bits
        calls.clear()
        big = torch.randn(300, 256, generator=g).half().to(gpu)   # more tokens than the kernel is dispatched for
        yb = m(big)
        assert calls == [] and yb.shape == (300, 192)
        bar(yb, lin(big), big, lin)
        edge = torch.randn(W.WB_FORWARD_MAX_TOKENS + 1, 256, generator=g).half().to(gpu)
        m(edge)
        assert calls == []
        m(edge[:-1])
        assert calls == [W.WB_FORWARD_MAX_TOKENS]
        calls.clear()
        mb, linb = _module_pair(256, 192, torch.bfloat16, gpu, 2, bits)   # a bf16 module: dequantize + F.linear
        xb = torch.randn(5, 256, generator=g).bfloat16().to(gpu)
        yb = mb(xb)
        assert calls == [] and yb.dtype == torch.bfloat16 and torch.equal(yb, linb(xb))
        mo, lino = _module_pair(70, 48, torch.float16, gpu, 3, bits)      # in_features % 16 != 0: kept off the kernel
        xo = torch.randn(4, 70, generator=g).half().to(gpu)
        assert not mo.kernel_rows_ok() and m.kernel_rows_ok()
        assert torch.equal(mo(xo), lino(xo)) and calls == []
    xg = torch.randn(3, 256, generator=g).half().to(gpu).requires_grad_(True)
    yg = m(xg)                                                            # autograd: dequantize + F.linear, gradients reach x
    assert calls == []
    yg.sum().backward()
    xr = xg.detach().clone().requires_grad_(True)
    lin(xr).sum().backward()
    assert xg.grad is not None and torch.equal(xg.grad, xr.grad)
    bar(yg.detach(), lin(xr).detach(), xg.detach(), lin)
    from asvd4llm_amd.quantization import _find_linears
    assert not isinstance(m, nn.Linear) and not isinstance(m, W8Linear) and _find_linears(nn.Sequential(m)) == []


def test_bitpacked_svdlinear_under_the_fused_forward_switch(gpu, monkeypatch):
    from asvd4llm_amd import ops
    from asvd4llm_amd.modules.svd_linear import SVDLinear
    from asvd4llm_amd.modules.wb_linear import WBLinear
    g = torch.Generator(device="cuda").manual_seed(21)
    Ah, Aq, As, Az = _quantized(192, 64, g, 6)
    Bh, Bq, Bs, Bz = _quantized(64, 256, g, 6)
    bias = torch.randn(192, device="cuda", generator=g).half()
    fake = SVDLinear._from_factors(Ah, Bh, bias, 64)
    packed = SVDLinear._from_factors(Ah.clone(), Bh.clone(), bias, 64)
    packed.ALinear = WBLinear.from_codes(Aq, As, Az, bias, 6, torch.float16)
    packed.BLinear = WBLinear.from_codes(Bq, Bs, Bz, None, 6, torch.float16)
    calls = []
    real = ops.wb_linear
    monkeypatch.setattr(ops, "wb_linear", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    x = torch.randn(1, 3, 256, device="cuda", generator=g).half()      # decode-sized, in_features % 64 == 0: what the fused launch takes
    with torch.no_grad():
        monkeypatch.delenv("ASVD_FUSED_FORWARD", raising=False)
        want, ref = packed(x), fake(x)
        assert len(calls) == 2
        for switch in ("env", "attr"):
            calls.clear()
            if switch == "env":
                monkeypatch.setenv("ASVD_FUSED_FORWARD", "1")
            else:
                monkeypatch.delenv("ASVD_FUSED_FORWARD")
                packed.fused_forward = True
            y = packed(x)
            assert len(calls) == 2 and getattr(packed, "_fused", None) is None, switch   # two kernel calls, no padded copies
            assert torch.equal(y, want)
            packed.check_fused_forward()
    exact = (x.double() @ Bh.double().T).half().double() @ Ah.double().T + bias.double()
    _check_bar(want.reshape(3, -1), ref.reshape(3, -1), exact.reshape(3, -1))


# ---- the pipeline -----------------------------------------------------------------------------------------------------------------

_PIPE = {}


def _bitpacked_pipeline(name, tmp_path_factory):
    """asvd.main with --weight_quant rtn_int6 --weight_quant_storage bitpacked (the other arguments of tests/test_gpu_w8_linear._packed_pipeline);
    returns the bit-packed model, deep copies taken just before the step — one fake-quantized with rtn_quant_sequential, one packed with
    storage="bytes" — and what the evaluation saw"""
    if name in _PIPE:
        return _PIPE[name]
    import asvd
    from asvd4llm_amd import evaluate_utils, quantization
    seen = {}
    real_pack, real_eval = quantization.rtn_pack_sequential, evaluate_utils.evaluate_model

    def step(model, wbits, storage="bytes"):
        seen["cmp"], seen["bytes"] = copy.deepcopy(model), copy.deepcopy(model)
        seen["model"], seen["bits"], seen["storage"] = model, wbits, storage
        for m in model.modules():
            if type(m).__name__ == "SVDLinear":
                m._fused = ("stale",)
        seen["packed"] = real_pack(model, wbits, storage=storage)
        return seen["packed"]

    def evaluate(model, *a, **k):
        seen["eval_args"] = (a, k)
        seen["result"] = real_eval(model, *a, **k)
        return seen["result"]

    mp = pytest.MonkeyPatch()
    try:
        mp.setenv("ASVD_STRICT", "1")
        mp.chdir(tmp_path_factory.mktemp("wbpipe_" + name))
        mp.setattr(quantization, "rtn_pack_sequential", step)
        mp.setattr(quantization, "rtn_quant_sequential", lambda *a: pytest.fail("the fake path must not run for bit-packed storage"))
        mp.setattr(evaluate_utils, "evaluate_model", evaluate)
        args = asvd.build_parser().parse_args(["--model_id", name, "--random_init", "--act_aware", "--alpha", "0.5", "--n_calib_samples", "4",
                                               "--calib_dataset", "synthetic", "--scaling_method", "abs_mean", "--param_ratio_target", "0.9",
                                               "--exclude_lm_head", "--weight_quant", "rtn_int6", "--weight_quant_storage", "bitpacked"])
        out = io.StringIO()
        with contextlib.redirect_stdout(out), contextlib.redirect_stderr(io.StringIO()):
            asvd.main(args)
    finally:
        mp.undo()
    assert seen["bits"] == 6 and seen["storage"] == "bits"
    with contextlib.redirect_stdout(io.StringIO()):
        quantization.rtn_quant_sequential(seen["cmp"], 6)
        quantization.rtn_pack_sequential(seen["bytes"], 6)
    a, k = seen["eval_args"]
    seen["cmp_result"] = real_eval(seen["cmp"], *a, **k)
    seen["stdout"] = out.getvalue()
    _PIPE[name] = seen
    return seen


def _bytes(mod):
    return sum(t.numel() * t.element_size() for t in list(mod.parameters(recurse=False)) + [b for b in mod.buffers(recurse=False)])


@pytest.mark.parametrize("name", ["tiny-llama", "tiny-opt"])
def test_bitpacked_pipeline_is_the_fake_quantized_model(gpu, name, tmp_path_factory, monkeypatch):
    from asvd4llm_amd import ops
    from asvd4llm_amd.modules.svd_linear import SVDLinear
    from asvd4llm_amd.modules.wb_linear import WBLinear
    from asvd4llm_amd.quantization import rtn_targets
    seen = _bitpacked_pipeline(name, tmp_path_factory)
    model, cmp_model, bytes_model = seen["model"], seen["cmp"], seen["bytes"]
    targets = rtn_targets(cmp_model)
    assert targets and seen["packed"] == len(targets)             # a randn model flags nothing: NO target may be left unpacked
    assert f"rtn int6 bit-packed: {len(targets)} weights in" in seen["stdout"]
    mods = dict(model.named_modules())
    svds = [m for m in model.modules() if isinstance(m, SVDLinear)]
    assert svds and all(isinstance(m.ALinear, WBLinear) and isinstance(m.BLinear, WBLinear) and m._fused is None for m in svds)
    packed_bytes = want_packed = want_fp16 = 0
    for n, lin in targets:
        m = mods[n]
        assert type(m) is WBLinear and m.bits == 6 and m.weight_dtype == torch.float16, n
        assert (m.in_features, m.out_features) == (lin.in_features, lin.out_features), n
        assert bool(torch.isfinite(lin.weight).all())
        assert same(m.dequantize(), lin.weight.data), n           # bit-equal to the fake-quantized weight
        assert (m.bias is None) == (lin.bias is None)
        if lin.bias is not None:
            assert same(m.bias, lin.bias.data), n
        bias_bytes = 0 if lin.bias is None else 2 * lin.out_features
        packed_bytes += _bytes(m)
        want_packed += lin.out_features * ops.wb_row_bytes(lin.in_features, 6) + 8 * lin.out_features + bias_bytes
        want_fp16 += 2 * lin.out_features * lin.in_features
    assert packed_bytes == want_packed                             # the size is derivable: asserted exactly
    assert f"{want_fp16} -> {want_packed - sum(0 if l.bias is None else 2 * l.out_features for _, l in targets)} bytes" in seen["stdout"]
    # everything that is not a target: bit-identical (lm_head, embeddings, norms, biases)
    tnames = {n for n, _ in targets}
    rest = {n: p for n, p in cmp_model.state_dict().items() if n.rpartition(".")[0] not in tnames}
    got = model.state_dict()
    assert any("lm_head" in n or "embed" in n for n in rest) and any("norm" in n for n in rest)
    for n, p in rest.items():
        assert same(got[n], p), n
    # (i) the calibration sequences are 2048 tokens long: the evaluation ran through dequantize + F.linear
    ppl, ppl_cmp = seen["result"]["synthetic_ppl"], seen["cmp_result"]["synthetic_ppl"]
    print(f"{name}: synthetic_ppl bit-packed {ppl!r} fake {ppl_cmp!r}")
    assert abs(ppl - ppl_cmp) <= 2e-4 * ppl_cmp
    # (ii) a decode-sized batch: the logits of the byte-packed model, bit for bit (kernel bit-equality on the layers both send to their kernel,
    # the same dequantized weight through the same GEMM on the others)
    calls = []
    real = ops.wb_linear
    monkeypatch.setattr(ops, "wb_linear", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    ids = torch.randint(0, model.config.vocab_size, (1, 8), generator=torch.Generator().manual_seed(11)).to(gpu)
    bmods = dict(bytes_model.named_modules())
    with torch.no_grad():
        y_bits = model(input_ids=ids)[0]
        eligible = [n for n, _ in targets if mods[n].kernel_rows_ok()]
        assert eligible and all((mods[n].in_features % 16 == 0) == (n in eligible) for n, _ in targets)
        assert eligible == [n for n, _ in targets if bmods[n].kernel_rows_ok()]
        assert len(calls) == len(eligible)
        y_bytes = bytes_model(input_ids=ids)[0]
    assert bool(torch.isfinite(y_bytes).all()) and torch.equal(y_bits.view(torch.int16), y_bytes.view(torch.int16))


@pytest.mark.parametrize("name", ["tiny-llama", "tiny-opt"])
def test_bitpacked_model_exports_and_loads(gpu, name, tmp_path_factory, tmp_path):
    from asvd4llm_amd.export import load_asvd_repo, save_asvd_repo, truncation_ranks_of
    from asvd4llm_amd.modules.wb_linear import WBLinear
    seen = _bitpacked_pipeline(name, tmp_path_factory)
    model = seen["model"]
    path = str(tmp_path / "repo")
    with contextlib.redirect_stdout(io.StringIO()) as out:
        ranks = save_asvd_repo(model, path)
    assert ranks == truncation_ranks_of(model) and ranks and "no auto_map" in out.getvalue()
    cfg = json.load(open(os.path.join(path, "config.json")))
    assert cfg["weight_quant"] == {"method": "rtn", "bits": 6, "storage": "bitstream64"} and "auto_map" not in cfg
    assert cfg["truncation_ranks"] == ranks and not [f for f in os.listdir(path) if f.endswith(".py")]
    loaded = load_asvd_repo(path, dtype=torch.float16, device=gpu)
    assert truncation_ranks_of(loaded) == ranks
    want = {n: m for n, m in model.named_modules() if isinstance(m, WBLinear)}
    have = {n: m for n, m in loaded.named_modules() if isinstance(m, WBLinear)}
    assert set(want) == set(have) and want
    for n, m in want.items():
        h = have[n]
        assert (h.bits, h.weight_dtype, h.in_features, h.out_features) == (6, torch.float16, m.in_features, m.out_features), n
        for key in ("qbits", "scales", "zeros", "bias"):
            a, b = getattr(m, key), getattr(h, key)
            assert (a is None) == (b is None), (n, key)
            if a is not None:
                assert same(a, b), (n, key)
    ids = torch.randint(0, model.config.vocab_size, (1, 8), generator=torch.Generator().manual_seed(12)).to(gpu)
    with torch.no_grad():
        assert torch.equal(loaded(input_ids=ids)[0], model(input_ids=ids)[0])


def test_four_bits_through_the_python_api(gpu):
    from asvd4llm_amd.model_zoo import random_init_model
    from asvd4llm_amd.modules.wb_linear import WBLinear
    from asvd4llm_amd.quantization import rtn_pack_sequential, rtn_quant_sequential, rtn_targets
    torch.manual_seed(5)
    model = random_init_model("tiny-llama", dtype=torch.float16).to(gpu)
    fake = copy.deepcopy(model)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        rtn_quant_sequential(fake, 4)
        n = rtn_pack_sequential(model, 4, storage="bits")
    targets = rtn_targets(fake)
    assert targets and n == len(targets) and f"rtn int4 bit-packed: {n} weights" in out.getvalue()
    mods = dict(model.named_modules())
    for name, lin in targets:
        m = mods[name]
        assert type(m) is WBLinear and m.bits == 4 and m.qbits.shape == (lin.out_features, R.row_bytes(lin.in_features, 4)), name
        assert same(m.dequantize(), lin.weight.data), name
    with pytest.raises(ValueError):
        rtn_pack_sequential(model, 8, storage="bits")
