"""RTN weight quantization (--weight_quant rtn_int8 / rtn_int6), host side: the CPU restatement against the reference's own outputs, the
layer selection against the reference's, the CLI dispatch, argument checks of the C entry points and the kernel's resources.  No GPU."""
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


def _bits_equal(a, b):
    """equal bit patterns, any NaN equal to any NaN"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and \
        np.array_equal(np.where(np.isnan(a), 0, a).view(np.uint32), np.where(np.isnan(b), 0, b).view(np.uint32))


def _cases(golden):
    z = golden.npz("rtn_ref.npz")
    return z, [tuple(str(c).split(":")) for c in z["cases"]]


def test_restatement_equals_reference_bit_for_bit(golden):
    z, cases = _cases(golden)
    assert {c[0] for c in cases} >= {"f16_int8", "f16_int6", "bf16_int8", "bf16_int6", "f32_int8", "f32_int6", "f32den_int8"}
    for case, d, b in cases:
        x = z[case + "_x"]
        w = torch.from_numpy(x).to(DT[d])
        assert _bits_equal(w.float().numpy(), x)  # the stored input is exact in its dtype
        out, q, scale, zero, ready = rtn_restate(w, int(b))
        assert ready == bool(z[case + "_ready"]), case
        assert _bits_equal(out.float().numpy(), z[case + "_out"]), case
        assert _bits_equal(q.numpy(), z[case + "_q"]), case
        assert _bits_equal(scale.numpy(), z[case + "_scale"]), case
        assert _bits_equal(zero.numpy(), z[case + "_zero"]), case


def test_fixture_covers_the_edge_rows(golden):
    z, cases = _cases(golden)
    for case, d, b in cases:
        x, out, scale = z[case + "_x"], z[case + "_out"], z[case + "_scale"]
        if case == "f32den_int8":
            assert (scale == 0).any() and np.array_equal(out, x)  # unchanged tensor (Quantizer.ready() is False)
            continue
        assert (x == 0).all(axis=1).any()                              # all-zero row
        assert ((x > 0).all(axis=1)).any() and ((x < 0).all(axis=1)).any()
        assert ((x == x[:, :1]).all(axis=1) & (x[:, 0] != 0)).any()   # constant row
        assert np.isnan(x).any(axis=1).any() and np.isinf(x).any(axis=1).any()
        bad = ~np.isfinite(x).all(axis=1)
        assert np.isnan(out[bad]).all()                                 # NaN / Inf rows come out all NaN
        ok = ~bad
        t = x[ok] / scale[ok, None]
        assert (np.abs(t - np.floor(t)) == 0.5).sum() >= 8              # exact .5 ties in x / scale
        assert np.isfinite(out[ok]).all()


def test_restatement_codes_and_dequantization_agree():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(64, 100, generator=g).half()
    out, q, scale, zero, ready = rtn_restate(x, 6)
    assert ready and q.min() >= 0 and q.max() <= 63
    c = codes_of(q)
    assert torch.equal((scale[:, None] * (c.float() - zero[:, None])).half(), out)


def _model_with_factors(name, replaced):
    from asvd4llm_amd.model_zoo import random_init_model
    from asvd4llm_amd.modules.svd_linear import SVDLinear
    model = random_init_model(name, dtype=torch.float32)
    for full, rank in replaced.items():
        father_name, child = full.rsplit(".", 1)
        father = model.get_submodule(father_name)
        lin = getattr(father, child)
        A = torch.zeros(lin.out_features, rank)
        B = torch.zeros(rank, lin.in_features)
        setattr(father, child, SVDLinear._from_factors(A, B, lin.bias.data if lin.bias is not None else None, rank))
    return model


@pytest.mark.parametrize("name", ["tiny-llama", "tiny-opt"])
def test_rtn_targets_match_reference_selection(golden, name):
    from asvd4llm_amd.quantization import rtn_targets
    ref = golden.json("rtn_layers.json")[name]
    model = _model_with_factors(name, ref["replaced"])
    got = [n for n, _ in rtn_targets(model)]
    assert got == ref["changed"]
    names = set(got)
    assert not any("lm_head" in n or "embed" in n for n in names)
    assert any(n.endswith(".ALinear") for n in names) and any(n.endswith(".BLinear") for n in names)
    mods = dict(model.named_modules())
    assert all(type(mods[n]) is nn.Linear for n in names)


def test_rtn_targets_find_blocks_by_structure():
    """a model whose name says neither llama nor opt: the blocks are found by what they hold"""
    from asvd4llm_amd.quantization import rtn_targets

    class Block(nn.Module):
        def __init__(self):
            super().__init__()
            self.inner = nn.Sequential(nn.Linear(8, 16), nn.GELU(), nn.Linear(16, 8))

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.embed = nn.Embedding(10, 8)
            self.blocks = nn.ModuleList([Block(), Block()])
            self.head = nn.Linear(8, 10)

    assert [n for n, _ in rtn_targets(Net())] == ["blocks.0.inner.0", "blocks.0.inner.2", "blocks.1.inner.0", "blocks.1.inner.2"]


def _args(**kw):
    d = dict(weight_quant="rtn_int8", dist=False, gather_factors="rank0")
    d.update(kw)
    return types.SimpleNamespace(**d)


@pytest.mark.parametrize("flag,bits", [("rtn_int8", 8), ("rtn_int6", 6)])
def test_cli_dispatches_rtn(monkeypatch, flag, bits):
    import asvd
    from asvd4llm_amd import quantization
    seen = []
    monkeypatch.setattr(quantization, "rtn_quant_sequential", lambda model, wbits: seen.append((model, wbits)))
    model = object()
    asvd.run_weight_quant(model, _args(weight_quant=flag))
    assert seen == [(model, bits)]
    assert asvd.build_parser().parse_args(["--weight_quant", flag]).weight_quant == flag


def test_cli_quantizes_on_the_ranks_that_hold_factors(monkeypatch):
    import asvd
    from asvd4llm_amd import quantization
    seen = []
    monkeypatch.setattr(quantization, "rtn_quant_sequential", lambda model, wbits: seen.append(wbits))
    monkeypatch.setenv("RANK", "1")
    asvd.run_weight_quant(None, _args(dist=True, gather_factors="rank0"))
    assert seen == []
    asvd.run_weight_quant(None, _args(dist=True, gather_factors="all"))
    assert seen == [8]
    monkeypatch.setenv("RANK", "0")
    asvd.run_weight_quant(None, _args(dist=True, gather_factors="rank0", weight_quant="rtn_int6"))
    assert seen == [8, 6]


@pytest.mark.parametrize("flag", ["awq_int8", "awq_int4"])
def test_cli_awq_names_the_missing_package(monkeypatch, flag):
    import asvd
    from asvd4llm_amd import quantization
    monkeypatch.setattr(quantization, "rtn_quant_sequential", lambda model, wbits: pytest.fail("rtn must not run for awq"))
    with pytest.raises(NotImplementedError, match="awq"):
        asvd.run_weight_quant(None, _args(weight_quant=flag))


def test_cli_calls_the_step_after_the_search():
    src = open(os.path.join(ROOT, "asvd.py")).read()
    body = src[src.index("def main(args)"):]
    assert body.index("binary_search_truncation_rank(model") < body.index("run_weight_quant(model, args)") < body.index("args.save_repo and")


def test_rtn_entry_points_reject_bad_arguments_without_device(built_lib):
    lib = built_lib
    nul = None
    assert lib.asvd_rtn_quant(nul, 1, 8, 8, 8, 8, nul, 8, nul, nul, nul, nul, nul) == -1
    # non-null but never dereferenced: every check below fails before any HIP call
    p = ctypes.c_void_p(4096)
    flag = ctypes.c_void_p(8192)
    assert lib.asvd_rtn_quant(p, 1, 8, 8, 8, 8, p, 8, nul, nul, nul, nul, nul) == -1      # no flag word
    assert lib.asvd_rtn_quant(p, 1, 8, 8, 8, 0, p, 8, nul, nul, nul, flag, nul) == -1     # bits 0
    assert lib.asvd_rtn_quant(p, 1, 8, 8, 8, 9, p, 8, nul, nul, nul, flag, nul) == -1     # bits 9 (codes are uint8)
    assert lib.asvd_rtn_quant(p, 7, 8, 8, 8, 8, p, 8, nul, nul, nul, flag, nul) == -1     # dtype
    assert lib.asvd_rtn_quant(p, 1, 0, 8, 8, 8, p, 8, nul, nul, nul, flag, nul) == -1     # rows
    assert lib.asvd_rtn_quant(p, 1, 8, 8, 4, 8, p, 8, nul, nul, nul, flag, nul) == -1     # ldw < cols
    assert lib.asvd_rtn_quant(p, 1, 8, 8, 8, 8, p, 4, nul, nul, nul, flag, nul) == -1     # ldo < cols
    assert lib.asvd_rtn_quant_batched(0, nul, nul, nul, nul, nul, 8, nul, nul, nul, nul, nul, nul, nul) == -1
    vp2, i2, l2 = ctypes.c_void_p * 2, ctypes.c_int * 2, ctypes.c_int64 * 2
    ws, outs, dts = vp2(4096, 4096), vp2(4096, None), i2(1, 2)
    shape = l2(8, 8)
    assert lib.asvd_rtn_quant_batched(2, ws, dts, shape, shape, shape, 8, outs, shape, nul, nul, nul, flag, nul) == -1  # a NULL out
    assert lib.asvd_rtn_quant_batched(2, ws, dts, shape, shape, shape, 8, vp2(4096, 4096), shape, nul, nul, nul, nul, nul) == -1  # no flags


def test_ops_rtn_quant_has_no_cpu_fallback():
    from asvd4llm_amd import _lib, ops
    with pytest.raises(_lib.AsvdHipError):
        ops.rtn_quant(torch.zeros(4, 4), 8)


def test_rtn_kernel_compiles_for_gfx950_without_scratch(tmp_path):
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not installed")
    from asvd4llm_amd.build import EXTRA_FLAGS, SOURCES
    src = "rtn_quant.hip"
    assert src in SOURCES
    out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only"] + EXTRA_FLAGS.get(src, []) +
                         ["-c", os.path.join(ROOT, "asvd4llm_amd", "csrc", src), "-o", str(tmp_path / "o.o"),
                          "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", out.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out.stderr)]
    assert len(names) == len(scratch) and len(names) >= 1
    assert all(s == 0 for s in scratch), list(zip(names, scratch))
