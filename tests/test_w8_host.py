"""Packed RTN weights (--weight_quant_storage packed), host side: W8Linear's CPU dequantization against the reference-generated fixture
and against the CPU restatement of the quantizer, the CLI switch, the state-dict layout of a packed SVDLinear, argument checks of the C entry
points and the kernels' resources.  No GPU."""
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests.conftest import ROOT
from tests.rtn_restate import codes_of, rtn_restate

DT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}


def _value_equal(a, b):
    """equal values, NaN matching NaN"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.where(np.isnan(a), 0, a), np.where(np.isnan(b), 0, b))


def _bit_equal(a, b):
    iv = {torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.float32: torch.int32}[a.dtype]
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(iv), b.view(iv))


def test_dequantize_on_the_reference_fixture(golden):
    from asvd4llm_amd.modules.w8_linear import W8Linear
    z = golden.npz("rtn_ref.npz")
    for d in ("f16", "bf16", "f32"):
        for b in (8, 6):
            case = f"{d}_int{b}"
            q = torch.from_numpy(z[case + "_q"])
            assert int(torch.isnan(q).sum()) > 0                       # the fixture holds non-finite rows: their codes are 0
            m = W8Linear.from_codes(codes_of(q), torch.from_numpy(z[case + "_scale"]), torch.from_numpy(z[case + "_zero"]), None, b, DT[d])
            w = m.dequantize()
            assert w.dtype == DT[d] and _value_equal(w.float().numpy(), z[case + "_out"]), case


@pytest.mark.parametrize("shape", [(37, 70), (128, 352), (64, 4096)])
@pytest.mark.parametrize("dt", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("bits", [8, 6])
def test_dequantize_equals_the_restatement_on_finite_inputs(shape, dt, bits):
    from asvd4llm_amd.modules.w8_linear import W8Linear
    g = torch.Generator().manual_seed(shape[0] + shape[1] + bits)
    w = (torch.randn(*shape, generator=g) * 0.02).to(DT[dt])
    out, q, scale, zero, ready = rtn_restate(w, bits)
    assert ready
    m = W8Linear.from_codes(codes_of(q), scale, zero, None, bits, DT[dt])
    assert _bit_equal(m.dequantize(), out)
    assert m.in_features == shape[1] and m.out_features == shape[0] and m.bits == bits and m.weight_dtype == DT[dt]
    x = torch.randn(3, shape[1], generator=g).to(DT[dt]).float()
    if dt == "f32":                                                    # CPU forward: F.linear on the dequantized weight
        assert torch.equal(m(x), nn.functional.linear(x, out))


def test_w8linear_is_not_an_nn_linear():
    from asvd4llm_amd.modules.w8_linear import W8Linear
    from asvd4llm_amd.quantization import _find_linears
    m = W8Linear(16, 8, bias=True, bits=6, weight_dtype=torch.bfloat16)
    assert not isinstance(m, nn.Linear) and _find_linears(nn.Sequential(m, nn.Linear(8, 8)))[0][0] == "1"
    assert m.qweight.dtype == torch.uint8 and m.qweight.shape == (8, 16) and m.scales.dtype == m.zeros.dtype == torch.float32
    assert m.bias.dtype == torch.bfloat16 and not list(m.parameters())
    m.half()                                                           # a dtype cast of the model leaves scale and zero in fp32 ...
    assert m.scales.dtype == m.zeros.dtype == torch.float32 and m.qweight.dtype == torch.uint8
    assert m.bias.dtype == torch.bfloat16 and m.weight_dtype == torch.bfloat16   # ... and the bias with the weight it belongs to
    with pytest.raises(ValueError):
        W8Linear(4, 4, bits=9)


@pytest.mark.parametrize("cast", ["double", "float", "bfloat16"])
def test_forward_after_a_cast_of_the_model(cast):
    """.double() / .float() / .bfloat16() on a packed fp16 model: the weight the codes stand for does not change, forward() converts it (and
    the bias) to the input's dtype for the GEMM"""
    from asvd4llm_amd.modules.w8_linear import W8Linear
    g = torch.Generator().manual_seed(4)
    w = (torch.randn(24, 40, generator=g) * 0.05).half()
    out, q, scale, zero, ready = rtn_restate(w, 8)
    bias = torch.randn(24, generator=g).half()
    m = W8Linear.from_codes(codes_of(q), scale, zero, bias, 8, torch.float16)
    holder = nn.Sequential(m)
    getattr(holder, cast)()
    dt = {"double": torch.float64, "float": torch.float32, "bfloat16": torch.bfloat16}[cast]
    assert m.bias.dtype == torch.float16 and m.scales.dtype == torch.float32 and m.weight_dtype == torch.float16
    assert _bit_equal(m.dequantize(), out)
    x = torch.randn(3, 40, generator=g).to(dt)
    y = holder(x)
    assert y.dtype == dt and torch.equal(y, nn.functional.linear(x, out.to(dt), bias.to(dt)))


def test_parser_has_the_storage_switch():
    import asvd
    p = asvd.build_parser()
    assert p.parse_args([]).weight_quant_storage == "fake"
    assert p.parse_args(["--weight_quant", "rtn_int8", "--weight_quant_storage", "packed"]).weight_quant_storage == "packed"
    with pytest.raises(SystemExit):
        p.parse_args(["--weight_quant_storage", "int4"])


def _args(**kw):
    d = dict(weight_quant="rtn_int8", dist=False, gather_factors="rank0")
    d.update(kw)
    return types.SimpleNamespace(**d)


def test_cli_calls_the_packing_step_only_for_packed(monkeypatch):
    import asvd
    from asvd4llm_amd import quantization
    fake, packed = [], []
    monkeypatch.setattr(quantization, "rtn_quant_sequential", lambda model, wbits: fake.append((model, wbits)))
    monkeypatch.setattr(quantization, "rtn_pack_sequential", lambda model, wbits: packed.append((model, wbits)))
    model = object()
    asvd.run_weight_quant(model, _args())                                            # a namespace without the field: today's path
    asvd.run_weight_quant(model, _args(weight_quant_storage="fake", weight_quant="rtn_int6"))
    assert fake == [(model, 8), (model, 6)] and packed == []
    asvd.run_weight_quant(model, _args(weight_quant_storage="packed"))
    asvd.run_weight_quant(model, _args(weight_quant_storage="packed", weight_quant="rtn_int6"))
    assert fake == [(model, 8), (model, 6)] and packed == [(model, 8), (model, 6)]
    for flag in ("awq_int8", "awq_int4"):
        with pytest.raises(NotImplementedError, match="awq"):
            asvd.run_weight_quant(model, _args(weight_quant_storage="packed", weight_quant=flag))
    assert len(fake) == 2 and len(packed) == 2


def test_cli_packs_on_the_ranks_that_hold_factors(monkeypatch):
    import asvd
    from asvd4llm_amd import quantization
    seen = []
    monkeypatch.setattr(quantization, "rtn_quant_sequential", lambda model, wbits: seen.append(("fake", wbits)))
    monkeypatch.setattr(quantization, "rtn_pack_sequential", lambda model, wbits: seen.append(("packed", wbits)))
    monkeypatch.setenv("RANK", "1")
    asvd.run_weight_quant(None, _args(dist=True, gather_factors="rank0", weight_quant_storage="packed"))
    asvd.run_weight_quant(None, _args(dist=True, gather_factors="rank0"))
    assert seen == []
    asvd.run_weight_quant(None, _args(dist=True, gather_factors="all", weight_quant_storage="packed"))
    assert seen == [("packed", 8)]
    monkeypatch.setenv("RANK", "0")
    asvd.run_weight_quant(None, _args(dist=True, gather_factors="rank0", weight_quant="rtn_int6", weight_quant_storage="packed"))
    assert seen == [("packed", 8), ("packed", 6)]


def _packed_svdlinear(in_f, out_f, rank, bias, seed=0, dtype=torch.float16):
    from asvd4llm_amd.modules.svd_linear import SVDLinear
    from asvd4llm_amd.modules.w8_linear import W8Linear
    g = torch.Generator().manual_seed(seed)
    A = (torch.randn(out_f, rank, generator=g) * 0.05).to(dtype)
    B = (torch.randn(rank, in_f, generator=g) * 0.05).to(dtype)
    b = torch.randn(out_f, generator=g).to(dtype) if bias else None
    m = SVDLinear._from_factors(A, B, b, rank)
    for name, w, bb in (("ALinear", A, b), ("BLinear", B, None)):
        out, q, scale, zero, ready = rtn_restate(w, 8)
        assert ready
        setattr(m, name, W8Linear.from_codes(codes_of(q), scale, zero, bb, 8, dtype))
    return m


@pytest.mark.parametrize("bias", [True, False])
def test_state_dict_of_a_packed_svdlinear(bias):
    from asvd4llm_amd.modules.svd_linear import SVDLinear, _plain_linear_without_hooks
    from asvd4llm_amd.modules.w8_linear import W8Linear
    m = _packed_svdlinear(48, 40, 7, bias)
    assert m.truncation_rank == 7 and not _plain_linear_without_hooks(m.ALinear) and not _plain_linear_without_hooks(m.BLinear)
    sd = m.state_dict()
    want = {"ALinear.qweight": (torch.uint8, (40, 7)), "ALinear.scales": (torch.float32, (40,)), "ALinear.zeros": (torch.float32, (40,)),
            "BLinear.qweight": (torch.uint8, (7, 48)), "BLinear.scales": (torch.float32, (7,)), "BLinear.zeros": (torch.float32, (7,))}
    if bias:
        want["ALinear.bias"] = (torch.float16, (40,))
    assert {k: (v.dtype, tuple(v.shape)) for k, v in sd.items()} == want
    # an empty skeleton of the same shape takes the checkpoint strictly
    empty = SVDLinear._from_factors(torch.empty(40, 7, dtype=torch.float16), torch.empty(7, 48, dtype=torch.float16),
                                    torch.empty(40, dtype=torch.float16) if bias else None, 7)
    empty.ALinear = W8Linear(7, 40, bias=bias, bits=8, weight_dtype=torch.float16)
    empty.BLinear = W8Linear(48, 7, bias=False, bits=8, weight_dtype=torch.float16)
    missing, unexpected = empty.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    for k, v in empty.state_dict().items():
        assert v.dtype == sd[k].dtype and torch.equal(v, sd[k]), k
    assert _bit_equal(empty.ALinear.dequantize(), m.ALinear.dequantize()) and _bit_equal(empty.BLinear.dequantize(), m.BLinear.dequantize())
    x = torch.randn(2, 3, 48, generator=torch.Generator().manual_seed(1))
    mf = _packed_svdlinear(48, 40, 7, bias, dtype=torch.float32)        # CPU forward falls through to ALinear(BLinear(x))
    y = mf(x)
    ref = nn.functional.linear(nn.functional.linear(x, mf.BLinear.dequantize()), mf.ALinear.dequantize(), mf.ALinear.bias)
    assert y.shape == (2, 3, 40) and torch.equal(y, ref)


def test_export_round_trip_of_packed_layers_on_the_host(tmp_path):
    """save_asvd_repo / load_asvd_repo with W8Linear modules, on the CPU: weight_quant in config.json, no auto_map, no remote-code files,
    buffers back bit for bit"""
    import json
    from asvd4llm_amd.export import load_asvd_repo, save_asvd_repo
    from asvd4llm_amd.model_zoo import random_init_model
    from asvd4llm_amd.modules.w8_linear import W8Linear
    model = random_init_model("tiny-llama", dtype=torch.float32)
    layer = model.model.layers[0]
    lin = layer.mlp.down_proj
    layer.mlp.down_proj = _packed_svdlinear(lin.in_features, lin.out_features, 5, False, dtype=torch.float32)
    q_lin = layer.self_attn.q_proj
    out, q, scale, zero, ready = rtn_restate(q_lin.weight.data, 6)
    layer.self_attn.q_proj = W8Linear.from_codes(codes_of(q), scale, zero, None, 6, torch.float32)
    path = str(tmp_path / "repo")
    with pytest.raises(ValueError, match="bit widths"):
        save_asvd_repo(model, path)                                    # int8 factors next to an int6 layer: refused
    layer.self_attn.q_proj = W8Linear.from_codes(codes_of(rtn_restate(q_lin.weight.data, 8)[1]), *rtn_restate(q_lin.weight.data, 8)[2:4], None, 8,
                                                 torch.float32)
    ranks = save_asvd_repo(model, path)
    assert ranks == {"model.layers.0.mlp.down_proj": 5}
    cfg = json.load(open(os.path.join(path, "config.json")))
    assert cfg["weight_quant"] == {"method": "rtn", "bits": 8, "storage": "uint8"} and "auto_map" not in cfg
    assert not [f for f in os.listdir(path) if f.endswith(".py")]
    assert (cfg.get("torch_dtype") or cfg.get("dtype")) == "float32"   # what the codes were packed from
    with pytest.raises(ValueError, match="packed from float32"):
        load_asvd_repo(path, dtype=torch.float16)                      # another dtype would round every weight once more
    loaded = load_asvd_repo(path, dtype=torch.float32)
    want = {n: m for n, m in model.named_modules() if isinstance(m, W8Linear)}
    have = {n: m for n, m in loaded.named_modules() if isinstance(m, W8Linear)}
    assert set(want) == set(have) and len(want) == 3
    for n in want:
        for key in ("qweight", "scales", "zeros"):
            assert torch.equal(getattr(want[n], key), getattr(have[n], key)), (n, key)
    ids = torch.randint(0, model.config.vocab_size, (1, 6), generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        assert torch.equal(loaded(input_ids=ids)[0], model.eval()(input_ids=ids)[0])


def test_w8_entry_points_reject_bad_arguments_without_device(built_lib):
    lib = built_lib
    assert lib.asvd_w8_linear_max_tokens() == 256
    p = ctypes.c_void_p(4096)   # non-null but never dereferenced: every check below fails before any HIP call
    nul = None
    ok = dict(x=p, T=4, q=p, ldq=64, scale=p, zero=p, bias=nul, N=8, K=64, y=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.asvd_w8_linear_f16(a["x"], a["T"], a["q"], a["ldq"], a["scale"], a["zero"], a["bias"], a["N"], a["K"], a["y"], nul)

    for bad in (dict(x=nul), dict(q=nul), dict(scale=nul), dict(zero=nul), dict(y=nul), dict(T=0), dict(T=257), dict(ldq=63), dict(N=0), dict(K=0),
                dict(x=ctypes.c_void_p(4097)), dict(y=ctypes.c_void_p(4099))):
        assert call(**bad) == -1, bad
    assert lib.asvd_w8_dequant(nul, 64, p, p, 8, 64, p, 1, 64, nul) == -1
    assert lib.asvd_w8_dequant(p, 64, nul, p, 8, 64, p, 1, 64, nul) == -1
    assert lib.asvd_w8_dequant(p, 64, p, p, 8, 64, nul, 1, 64, nul) == -1
    assert lib.asvd_w8_dequant(p, 63, p, p, 8, 64, p, 1, 64, nul) == -1      # ldq < cols
    assert lib.asvd_w8_dequant(p, 64, p, p, 8, 64, p, 1, 63, nul) == -1      # ldo < cols
    assert lib.asvd_w8_dequant(p, 64, p, p, 0, 64, p, 1, 64, nul) == -1
    assert lib.asvd_w8_dequant(p, 64, p, p, 8, 64, p, 5, 64, nul) == -1      # dtype
    assert lib.asvd_w8_dequant(p, 64, p, p, 8, 64, ctypes.c_void_p(4098), 0, 64, nul) == -1   # fp32 destination off its alignment


def test_ops_w8_have_no_cpu_fallback():
    from asvd4llm_amd import _lib, ops
    q = torch.zeros(4, 8, dtype=torch.uint8)
    with pytest.raises(_lib.AsvdHipError):
        ops.w8_linear(torch.zeros(2, 8).half(), q, torch.ones(4), torch.zeros(4))
    with pytest.raises(_lib.AsvdHipError):
        ops.w8_dequant(q, torch.ones(4), torch.zeros(4), torch.float16)


def test_w8_kernels_compile_for_gfx950_without_scratch(tmp_path):
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not installed")
    from asvd4llm_amd.build import EXTRA_FLAGS, SOURCES
    src = "w8_linear.hip"
    assert src in SOURCES
    out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only"] + EXTRA_FLAGS.get(src, []) +
                         ["-c", os.path.join(ROOT, "asvd4llm_amd", "csrc", src), "-o", str(tmp_path / "o.o"),
                          "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", out.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out.stderr)]
    assert len(names) == len(scratch) and len(names) >= 4      # the forward kernel and one dequantization kernel per dtype
    assert all(s == 0 for s in scratch), list(zip(names, scratch))
