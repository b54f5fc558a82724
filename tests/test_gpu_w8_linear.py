"""Packed RTN weights on the GPU (csrc/w8_linear.hip through ops.w8_linear / ops.w8_dequant, modules/w8_linear.py,
quantization.rtn_pack_sequential, export): the dequantization is the fake quantizer's output bit for bit, the W8A16 forward is as accurate as
nn.Linear on the fake-quantized weight (the bar of tests/test_gpu_lowrank_forward.py), and a model packed through the CLI pipeline is the
fake-quantized model: same weights, same perplexity, same logits within that bar, at the derivable size, through export and back."""
import contextlib
import copy
import ctypes
import io
import json
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests.test_gpu_rtn import DT, SHAPES, same, weight_like

pytestmark = pytest.mark.gpu


# ---- dequantization ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=[f"{m}x{n}" for m, n in SHAPES])
@pytest.mark.parametrize("dt", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("bits", [8, 6])
def test_dequant_is_the_fake_quantizers_output(gpu, shape, dt, bits):
    from asvd4llm_amd import ops
    w = weight_like(*shape, DT[dt], seed=shape[0] * 5 + shape[1] + bits, edges=False).to(gpu)
    out, q, scale, zero, flagged = ops.rtn_quant(w, bits, want_params=True)
    assert not flagged and bool(torch.isfinite(out).all())
    back = ops.w8_dequant(q, scale, zero, DT[dt])
    assert same(back, out)


@pytest.mark.parametrize("dt", ["f16", "bf16", "f32"])
def test_dequant_into_a_strided_destination_and_from_strided_codes(gpu, dt):
    from asvd4llm_amd import ops
    for rows, cols, off in ((300, 4096, 8), (300, 4096, 3), (37, 1001, 5)):
        w = weight_like(rows, cols, DT[dt], seed=rows + cols + off, edges=False).to(gpu)
        out, q, scale, zero, flagged = ops.rtn_quant(w, 8, want_params=True)
        big = torch.full((rows, cols + 64), 7.0, dtype=DT[dt], device=gpu)
        ops.w8_dequant(q, scale, zero, DT[dt], out=big[:, off:off + cols])
        assert same(big[:, off:off + cols].contiguous(), out)
        assert bool((big[:, :off] == 7).all()) and bool((big[:, off + cols:] == 7).all())   # nothing written outside the view
        qbig = torch.zeros((rows, cols + 32), dtype=torch.uint8, device=gpu)
        qbig[:, off:off + cols] = q
        assert same(ops.w8_dequant(qbig[:, off:off + cols], scale, zero, DT[dt]), out)


def test_dequant_on_the_fixture_rows(gpu, golden):
    from asvd4llm_amd import ops
    from tests.rtn_restate import codes_of
    z = golden.npz("rtn_ref.npz")
    done = 0
    for c in z["cases"]:
        case, d, b = str(c).split(":")
        if not bool(z[case + "_ready"]):
            continue
        q = codes_of(torch.from_numpy(z[case + "_q"])).to(gpu)
        got = ops.w8_dequant(q, torch.from_numpy(z[case + "_scale"]).to(gpu), torch.from_numpy(z[case + "_zero"]).to(gpu), DT[d])
        assert same(got.float(), torch.from_numpy(z[case + "_out"])), case   # value-equal, NaN rows matching NaN rows
        done += 1
    assert done >= 6


# ---- forward ----------------------------------------------------------------------------------------------------------------------

def _quantized(N, K, g, bits=8):
    """(w_hat fp16, q, scale, zero) of a seeded weight: w_hat is the fake-quantized weight, the other three its packed form"""
    from asvd4llm_amd import ops
    w = (torch.randn(N, K, device="cuda", generator=g) / K ** 0.5).half()
    out, q, scale, zero, flagged = ops.rtn_quant(w, bits, want_params=True)
    assert not flagged
    return out, q, scale, zero


def _check_bar(y, ref, exact):
    scale = exact.abs().max().item()
    err_w8 = (y.double() - exact).abs().max().item() / scale
    err_ref = (ref.double() - exact).abs().max().item() / scale
    print(f"err_w8 {err_w8:.3e} err_ref {err_ref:.3e} |y - ref| {(y.float() - ref.float()).abs().max().item() / scale:.3e} (relative to |exact|_max)")
    assert err_w8 <= 2 * err_ref + 2 ** -10, (err_w8, err_ref)
    assert (y.float() - ref.float()).abs().max().item() <= 4e-3 * scale


# the shapes of tests/test_gpu_lowrank_forward.py, as a B stage then an A stage
LOWRANK_SHAPES = [(1, 4096, 1843, 4096, False), (16, 4096, 1024, 4096, True), (2, 4096, 1024, 4096, True), (3, 11008, 1500, 4096, True),
                  (4, 4096, 2686, 11008, False), (33, 4096, 2686, 11008, False), (7, 11008, 1500, 4096, True), (256, 768, 345, 3072, True),
                  (5, 64, 3, 70, True)]


@pytest.mark.parametrize("T,K,r,N,with_bias", LOWRANK_SHAPES)
@pytest.mark.parametrize("bits", [8, 6])
def test_two_stage_forward_vs_fake_quantized_linears_and_fp64(gpu, T, K, r, N, with_bias, bits):
    from asvd4llm_amd import ops
    g = torch.Generator(device="cuda").manual_seed(T * 7 + r + bits)
    x = torch.randn(T, K, device="cuda", generator=g).half()
    Bh, Bq, Bs, Bz = _quantized(r, K, g, bits)
    Ah, Aq, As, Az = _quantized(N, r, g, bits)
    bias = torch.randn(N, device="cuda", generator=g).half() if with_bias else None
    z = ops.w8_linear(x, Bq, Bs, Bz, None)
    y = ops.w8_linear(z, Aq, As, Az, bias)
    assert torch.equal(z, ops.w8_linear(x, Bq, Bs, Bz, None)) and torch.equal(y, ops.w8_linear(z, Aq, As, Az, bias))   # deterministic
    ref = F.linear(F.linear(x, Bh), Ah, bias)
    exact = (x.double() @ Bh.double().T).half().double() @ Ah.double().T   # z rounded to fp16 where both paths round it
    if bias is not None:
        exact = exact + bias.double()
    _check_bar(y, ref, exact)


PLAIN_SHAPES = [(4096, 4096), (11008, 4096), (4096, 11008)]   # [out, in]


@pytest.mark.parametrize("N,K", PLAIN_SHAPES, ids=[f"{n}x{k}" for n, k in PLAIN_SHAPES])
@pytest.mark.parametrize("T", [1, 3, 16, 33, 256])
def test_plain_linear_forward(gpu, N, K, T):
    from asvd4llm_amd import ops
    g = torch.Generator(device="cuda").manual_seed(N + K + T)
    x = torch.randn(T, K, device="cuda", generator=g).half()
    Wh, q, s, zr = _quantized(N, K, g)
    bias = torch.randn(N, device="cuda", generator=g).half() if T % 2 else None
    y = ops.w8_linear(x, q, s, zr, bias)
    assert torch.equal(y, ops.w8_linear(x, q, s, zr, bias))
    exact = x.double() @ Wh.double().T
    if bias is not None:
        exact = exact + bias.double()
    _check_bar(y, F.linear(x, Wh, bias), exact)


@pytest.mark.parametrize("T,K,N", [(5, 70, 37), (8, 352, 128), (33, 352, 64), (3, 1001, 37), (1, 1, 1), (2, 8, 300), (40, 200, 33)])
def test_forward_with_ragged_k(gpu, T, K, N):
    """K that is no multiple of 16 (tiny-llama's intermediate size is 352), of 8, of anything; codes with a leading dimension and rows that
    start off 16-byte alignment"""
    from asvd4llm_amd import ops
    g = torch.Generator(device="cuda").manual_seed(T + K + N)
    x = torch.randn(T, K, device="cuda", generator=g).half()
    Wh, q, s, zr = _quantized(N, K, g)
    bias = torch.randn(N, device="cuda", generator=g).half()
    exact = x.double() @ Wh.double().T + bias.double()
    ref = F.linear(x, Wh, bias)
    y = ops.w8_linear(x, q, s, zr, bias)
    assert torch.equal(y, ops.w8_linear(x, q, s, zr, bias))
    _check_bar(y, ref, exact)
    for off in (16, 5):
        qbig = torch.full((N, K + 48), 255, dtype=torch.uint8, device="cuda")
        qbig[:, off:off + K] = q
        assert torch.equal(ops.w8_linear(x, qbig[:, off:off + K], s, zr, bias), y)   # same arithmetic whatever the load path


def test_bad_arguments_return_codes_and_raise_without_a_launch(gpu):
    from asvd4llm_amd import _lib, ops
    lib = _lib.load(True)
    x = torch.zeros(4, 64, device="cuda").half()
    q = torch.zeros(8, 64, dtype=torch.uint8, device="cuda")
    s = torch.ones(8, device="cuda")
    y = torch.full((4, 8), 3.0, device="cuda").half()
    vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    call = lambda xx, T, ldq, yy: lib.asvd_w8_linear_f16(xx, T, vp(q), ldq, vp(s), vp(s), None, 8, 64, yy, None)  # noqa: E731
    assert call(None, 4, 64, vp(y)) == _lib.E_BADARG
    assert call(vp(x), 0, 64, vp(y)) == _lib.E_BADARG
    assert call(vp(x), lib.asvd_w8_linear_max_tokens() + 1, 64, vp(y)) == _lib.E_BADARG
    assert call(vp(x), 4, 63, vp(y)) == _lib.E_BADARG                                    # ldq < K
    assert call(ctypes.c_void_p(x.data_ptr() + 1), 4, 64, vp(y)) == _lib.E_BADARG        # misaligned x
    assert call(vp(x), 4, 64, ctypes.c_void_p(y.data_ptr() + 1)) == _lib.E_BADARG        # misaligned y
    out = torch.full((8, 64), 3.0, device="cuda").half()
    assert lib.asvd_w8_dequant(vp(q), 63, vp(s), vp(s), 8, 64, vp(out), _lib.F16, 64, None) == _lib.E_BADARG
    assert lib.asvd_w8_dequant(vp(q), 64, vp(s), vp(s), 8, 64, vp(out), 7, 64, None) == _lib.E_BADARG
    assert lib.asvd_w8_dequant(vp(q), 64, None, vp(s), 8, 64, vp(out), _lib.F16, 64, None) == _lib.E_BADARG
    torch.cuda.synchronize()
    assert bool((y == 3).all()) and bool((out == 3).all())   # nothing ran
    assert call(vp(x), 4, 64, vp(y)) == _lib.OK
    with pytest.raises(ValueError):
        ops.w8_linear(torch.zeros(257, 64, device="cuda").half(), q, s, s, None)
    with pytest.raises(ValueError):
        ops.w8_linear(x.float(), q, s, s, None)
    with pytest.raises(ValueError):
        ops.w8_linear(x, q[:, :32], s, s, None)
    with pytest.raises(ValueError):
        ops.w8_dequant(q, s[:4], s, torch.float16)
    with pytest.raises(_lib.AsvdHipError):
        ops.w8_linear(x.cpu(), q, s, s, None)


# ---- module dispatch --------------------------------------------------------------------------------------------------------------

def _module_pair(in_f, out_f, dtype, gpu, seed, bias=True):
    """(W8Linear, nn.Linear holding the fake-quantized weight) of one seeded Linear"""
    from asvd4llm_amd import ops
    from asvd4llm_amd.modules.w8_linear import W8Linear
    torch.manual_seed(seed)
    lin = nn.Linear(in_f, out_f, bias=bias).to(dtype).to(gpu)
    out, q, scale, zero, flagged = ops.rtn_quant(lin.weight.data, 8, want_params=True)
    assert not flagged
    lin.weight.data = out
    return W8Linear.from_codes(q, scale, zero, lin.bias.data if bias else None, 8, dtype), lin


def test_module_dispatch(gpu, monkeypatch):
    from asvd4llm_amd import ops
    from asvd4llm_amd.modules import w8_linear as W
    calls = []
    real = ops.w8_linear
    monkeypatch.setattr(ops, "w8_linear", lambda *a, **k: (calls.append(a[0].shape[0]), real(*a, **k))[1])
    m, lin = _module_pair(256, 192, torch.float16, gpu, 0)
    assert same(m.dequantize(), lin.weight.data)
    g = torch.Generator().manual_seed(1)

    def bar(y, ref, x, mod_ref):
        exact = x.double() @ mod_ref.weight.double().T + mod_ref.bias.double()
        _check_bar(y.reshape(-1, y.shape[-1]), ref.reshape(-1, ref.shape[-1]), exact.reshape(-1, exact.shape[-1]))

    with torch.no_grad():
        x = torch.randn(2, 7, 256, generator=g).half().to(gpu)
        y = m(x)
        assert calls == [14] and y.shape == (2, 7, 192)          # decode-sized fp16 input: the kernel
        bar(y, lin(x), x, lin)
        calls.clear()
        big = torch.randn(300, 256, generator=g).half().to(gpu)   # more tokens than the kernel is dispatched for
        yb = m(big)
        assert calls == [] and yb.shape == (300, 192)
        bar(yb, lin(big), big, lin)
        edge = torch.randn(W.W8_FORWARD_MAX_TOKENS + 1, 256, generator=g).half().to(gpu)
        m(edge)
        assert calls == []
        m(edge[:-1])
        assert calls == [W.W8_FORWARD_MAX_TOKENS]
        calls.clear()
        mb, linb = _module_pair(256, 192, torch.bfloat16, gpu, 2)   # a bf16 module: dequantize + F.linear
        xb = torch.randn(5, 256, generator=g).bfloat16().to(gpu)
        yb = mb(xb)
        assert calls == [] and yb.dtype == torch.bfloat16
        assert torch.equal(yb, linb(xb))                            # the same weight through the same GEMM
    with torch.no_grad():
        mo, lino = _module_pair(70, 48, torch.float16, gpu, 3)     # rows that allow no 16-byte loads: measured slower on the kernel, kept off it
        xo = torch.randn(4, 70, generator=g).half().to(gpu)
        assert not mo.kernel_rows_ok() and m.kernel_rows_ok()
        yo = mo(xo)
        assert calls == [] and torch.equal(yo, lino(xo))
    xg = torch.randn(3, 256, generator=g).half().to(gpu).requires_grad_(True)
    yg = m(xg)                                                      # autograd: dequantize + F.linear, gradients reach x
    assert calls == []
    yg.sum().backward()
    xr = xg.detach().clone().requires_grad_(True)
    lin(xr).sum().backward()
    assert xg.grad is not None and torch.equal(xg.grad, xr.grad)
    bar(yg.detach(), lin(xr).detach(), xg.detach(), lin)
    # a packed module is invisible to the nn.Linear selections
    from asvd4llm_amd.quantization import _find_linears
    assert not isinstance(m, nn.Linear) and _find_linears(nn.Sequential(m)) == []


def test_packed_svdlinear_under_the_fused_forward_switch(gpu, monkeypatch):
    """ASVD_FUSED_FORWARD=1 / module.fused_forward select the one-launch kernel for plain nn.Linear factors; a packed SVDLinear must fall
    through to ALinear(BLinear(x)) — two W8 launches — and build no padded copies"""
    from asvd4llm_amd import ops
    from asvd4llm_amd.modules.svd_linear import SVDLinear
    from asvd4llm_amd.modules.w8_linear import W8Linear
    g = torch.Generator(device="cuda").manual_seed(21)
    Ah, Aq, As, Az = _quantized(192, 64, g)
    Bh, Bq, Bs, Bz = _quantized(64, 256, g)
    bias = torch.randn(192, device="cuda", generator=g).half()
    fake = SVDLinear._from_factors(Ah, Bh, bias, 64)
    packed = SVDLinear._from_factors(Ah.clone(), Bh.clone(), bias, 64)
    packed.ALinear = W8Linear.from_codes(Aq, As, Az, bias, 8, torch.float16)
    packed.BLinear = W8Linear.from_codes(Bq, Bs, Bz, None, 8, torch.float16)
    calls = []
    real = ops.w8_linear
    monkeypatch.setattr(ops, "w8_linear", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    x = torch.randn(1, 3, 256, device="cuda", generator=g).half()      # decode-sized, in_features % 64 == 0: what the fused launch takes
    big = torch.randn(40, 256, device="cuda", generator=g).half()      # prefill-sized
    with torch.no_grad():
        monkeypatch.delenv("ASVD_FUSED_FORWARD", raising=False)
        want, want_big = packed(x), packed(big)
        ref = fake(x)
        assert len(calls) == 2 and getattr(fake, "_fused", None) is None
        for switch in ("env", "attr"):
            calls.clear()
            if switch == "env":
                monkeypatch.setenv("ASVD_FUSED_FORWARD", "1")
            else:
                monkeypatch.delenv("ASVD_FUSED_FORWARD")
                packed.fused_forward = True
            y = packed(x)
            assert len(calls) == 2 and getattr(packed, "_fused", None) is None, switch
            assert torch.equal(y, want) and torch.equal(packed(big), want_big)
            packed.check_fused_forward()                                  # nothing to check, nothing raised
    exact = (x.double() @ Bh.double().T).half().double() @ Ah.double().T + bias.double()
    _check_bar(want.reshape(3, -1), ref.reshape(3, -1), exact.reshape(3, -1))


# ---- the pipeline -----------------------------------------------------------------------------------------------------------------

_PIPE = {}


def _packed_pipeline(name, tmp_path_factory):
    """asvd.main with --weight_quant rtn_int8 --weight_quant_storage packed (the arguments of tests/test_gpu_rtn._run_pipeline); returns the
    packed model, a deep copy taken just before the step and fake-quantized with rtn_quant_sequential, and what the evaluation saw"""
    if name in _PIPE:
        return _PIPE[name]
    import asvd
    from asvd4llm_amd import evaluate_utils, quantization
    seen = {}
    real_pack, real_eval = quantization.rtn_pack_sequential, evaluate_utils.evaluate_model

    def step(model, wbits):
        seen["cmp"] = copy.deepcopy(model)
        seen["model"], seen["bits"] = model, wbits
        for m in model.modules():
            if type(m).__name__ == "SVDLinear":
                m._fused = ("stale",)
        seen["packed"] = real_pack(model, wbits)
        return seen["packed"]

    def evaluate(model, *a, **k):
        seen["eval_args"] = (a, k)
        seen["result"] = real_eval(model, *a, **k)
        return seen["result"]

    mp = pytest.MonkeyPatch()
    try:
        mp.setenv("ASVD_STRICT", "1")
        mp.chdir(tmp_path_factory.mktemp("pipe_" + name))
        mp.setattr(quantization, "rtn_pack_sequential", step)
        mp.setattr(quantization, "rtn_quant_sequential", lambda *a: pytest.fail("the fake path must not run for packed storage"))
        mp.setattr(evaluate_utils, "evaluate_model", evaluate)
        args = asvd.build_parser().parse_args(["--model_id", name, "--random_init", "--act_aware", "--alpha", "0.5", "--n_calib_samples", "4",
                                               "--calib_dataset", "synthetic", "--scaling_method", "abs_mean", "--param_ratio_target", "0.9",
                                               "--exclude_lm_head", "--weight_quant", "rtn_int8", "--weight_quant_storage", "packed"])
        out = io.StringIO()
        with contextlib.redirect_stdout(out), contextlib.redirect_stderr(io.StringIO()):
            asvd.main(args)
    finally:
        mp.undo()
    assert seen["bits"] == 8
    with contextlib.redirect_stdout(io.StringIO()):
        quantization.rtn_quant_sequential(seen["cmp"], 8)
    a, k = seen["eval_args"]
    seen["cmp_result"] = real_eval(seen["cmp"], *a, **k)
    seen["stdout"] = out.getvalue()
    _PIPE[name] = seen
    return seen


def _bytes(mod):
    return sum(t.numel() * t.element_size() for t in list(mod.parameters(recurse=False)) + [b for b in mod.buffers(recurse=False)])


@pytest.mark.parametrize("name", ["tiny-llama", "tiny-opt"])
def test_packed_pipeline_is_the_fake_quantized_model(gpu, name, tmp_path_factory, monkeypatch):
    from asvd4llm_amd import ops
    from asvd4llm_amd.modules.svd_linear import SVDLinear
    from asvd4llm_amd.modules.w8_linear import W8Linear
    from asvd4llm_amd.quantization import rtn_targets
    seen = _packed_pipeline(name, tmp_path_factory)
    model, cmp_model = seen["model"], seen["cmp"]
    targets = rtn_targets(cmp_model)
    assert targets and seen["packed"] == len(targets)             # a randn model flags nothing: NO target may be left unpacked
    assert not any(type(m) is nn.Linear for blk in model.get_submodule(targets[0][0].split('.0.')[0]) for m in blk.modules())   # no Linear left in the blocks
    assert f"rtn int8 packed: {len(targets)} weights in" in seen["stdout"]
    mods = dict(model.named_modules())
    svds = [m for m in model.modules() if isinstance(m, SVDLinear)]
    assert svds and all(isinstance(m.ALinear, W8Linear) and isinstance(m.BLinear, W8Linear) and m._fused is None for m in svds)
    assert {n for n, m in model.named_modules() if isinstance(m, SVDLinear)} == {n for n, m in cmp_model.named_modules() if isinstance(m, SVDLinear)}
    packed_bytes = fp16_bytes = want_packed = want_fp16 = 0
    for n, lin in targets:
        m = mods[n]
        assert type(m) is W8Linear and m.bits == 8 and m.weight_dtype == torch.float16, n
        assert bool(torch.isfinite(lin.weight).all())
        assert same(m.dequantize(), lin.weight.data), n           # bit-equal to the comparison weight
        assert (m.bias is None) == (lin.bias is None)
        if lin.bias is not None:
            assert same(m.bias, lin.bias.data), n
        bias_bytes = 0 if lin.bias is None else 2 * lin.out_features
        packed_bytes += _bytes(m)
        fp16_bytes += _bytes(lin)
        want_packed += lin.out_features * lin.in_features + 8 * lin.out_features + bias_bytes
        want_fp16 += 2 * lin.out_features * lin.in_features + bias_bytes
    assert packed_bytes == want_packed and fp16_bytes == want_fp16   # the size is derivable: asserted exactly
    assert f"{want_fp16 - sum(0 if l.bias is None else 2 * l.out_features for _, l in targets)} -> " in seen["stdout"]
    # everything that is not a target: bit-identical (lm_head, embeddings, norms, biases)
    tnames = {n for n, _ in targets}
    rest = {n: p for n, p in cmp_model.state_dict().items() if n.rpartition(".")[0] not in tnames}
    got = model.state_dict()
    assert any("lm_head" in n or "embed" in n for n in rest) and any("norm" in n for n in rest)
    for n, p in rest.items():
        assert same(got[n], p), n
    # (i) the calibration sequences are 2048 tokens long: the evaluation ran through dequantize + F.linear
    ppl, ppl_cmp = seen["result"]["synthetic_ppl"], seen["cmp_result"]["synthetic_ppl"]
    print(f"{name}: synthetic_ppl packed {ppl!r} fake {ppl_cmp!r}")
    assert abs(ppl - ppl_cmp) <= 2e-4 * ppl_cmp
    # (ii) a decode-sized batch: every packed layer takes the kernel
    calls = []
    real = ops.w8_linear
    monkeypatch.setattr(ops, "w8_linear", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    ids = torch.randint(0, model.config.vocab_size, (1, 8), generator=torch.Generator().manual_seed(11)).to(gpu)
    with torch.no_grad():
        y_packed = model(input_ids=ids)[0]
        monkeypatch.setenv("ASVD_FUSED_FORWARD", "1")             # the opt-in one-launch forward leaves packed factors alone
        y_packed2 = model(input_ids=ids)[0]
        monkeypatch.delenv("ASVD_FUSED_FORWARD")
        assert all(m._fused is None for m in svds)
        # the kernel serves the layers whose code rows allow 16-byte loads (in_features % 16 == 0); factors of other ranks dequantize
        eligible = [n for n, _ in targets if mods[n].kernel_rows_ok()]
        assert eligible and all((mods[n].in_features % 16 == 0) == (n in eligible) for n, _ in targets)
        assert len(calls) == 2 * len(eligible)
        y_cmp = cmp_model(input_ids=ids)[0]
        exact = copy.deepcopy(cmp_model).double()(input_ids=ids)[0]
    assert torch.equal(y_packed, y_packed2)
    scale = exact.abs().max().item()
    err_packed = (y_packed.double() - exact).abs().max().item()
    err_ref = (y_cmp.double() - exact).abs().max().item()
    print(f"{name}: logits err_packed {err_packed / scale:.3e} err_ref {err_ref / scale:.3e} (relative to |exact|_max)")
    assert err_packed <= 2 * err_ref + 2 ** -10 * scale


@pytest.mark.parametrize("name", ["tiny-llama", "tiny-opt"])
def test_packed_model_exports_and_loads(gpu, name, tmp_path_factory, tmp_path):
    from asvd4llm_amd.export import load_asvd_repo, save_asvd_repo, truncation_ranks_of
    from asvd4llm_amd.modules.w8_linear import W8Linear
    seen = _packed_pipeline(name, tmp_path_factory)
    model = seen["model"]
    path = str(tmp_path / "repo")
    with contextlib.redirect_stdout(io.StringIO()) as out:
        ranks = save_asvd_repo(model, path)
    assert ranks == truncation_ranks_of(model) and ranks
    assert "no auto_map" in out.getvalue()
    cfg = json.load(open(os.path.join(path, "config.json")))
    assert cfg["weight_quant"] == {"method": "rtn", "bits": 8, "storage": "uint8"} and "auto_map" not in cfg
    assert cfg["truncation_ranks"] == ranks
    assert not [f for f in os.listdir(path) if f.endswith(".py")]
    loaded = load_asvd_repo(path, dtype=torch.float16, device=gpu)
    assert loaded.truncation_ranks == ranks and truncation_ranks_of(loaded) == ranks
    want = {n: m for n, m in model.named_modules() if isinstance(m, W8Linear)}
    have = {n: m for n, m in loaded.named_modules() if isinstance(m, W8Linear)}
    assert set(want) == set(have) and want
    for n, m in want.items():
        h = have[n]
        assert h.bits == 8 and h.weight_dtype == torch.float16
        for key in ("qweight", "scales", "zeros", "bias"):
            a, b = getattr(m, key), getattr(h, key)
            assert (a is None) == (b is None), (n, key)
            if a is not None:
                assert same(a, b), (n, key)
    ids = torch.randint(0, model.config.vocab_size, (1, 8), generator=torch.Generator().manual_seed(12)).to(gpu)
    with torch.no_grad():
        assert torch.equal(loaded(input_ids=ids)[0], model(input_ids=ids)[0])
    # a model without packed weights is exported as before: auto_map and both remote-code files
    plain = str(tmp_path / "plain")
    save_asvd_repo(seen["cmp"], plain)
    cfg = json.load(open(os.path.join(plain, "config.json")))
    assert "auto_map" in cfg and "weight_quant" not in cfg
    assert len([f for f in os.listdir(plain) if f.endswith(".py")]) == 2
