"""RTN weight quantization on the GPU (csrc/rtn_quant.hip through ops.rtn_quant / rtn_quant_batched and asvd4llm_amd.quantization): bit for bit
against the CPU restatement of the reference's quantizer (tests/rtn_restate.py, itself pinned by tests/golden/rtn_ref.npz), on decoder shapes,
edge rows, strided views, mixed batches, and end to end through the CLI pipeline."""
import contextlib
import io
import math
import os
import re
import subprocess
import sys

import pytest
import torch

from tests.conftest import ROOT
from tests.rtn_restate import codes_of, rtn_restate

pytestmark = pytest.mark.gpu

DT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}


def same(a, b):
    """equal values and equal bit patterns (signed zeros included), NaN positions equal"""
    a, b = a.detach().cpu(), b.detach().cpu()
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    na, nb = torch.isnan(a), torch.isnan(b)
    if not torch.equal(na, nb):
        return False
    if not a.is_floating_point():
        return torch.equal(a, b)
    iv = {torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.float32: torch.int32}[a.dtype]
    return torch.equal(a.masked_fill(na, 0).view(iv), b.masked_fill(nb, 0).view(iv))


def weight_like(rows, cols, dtype, seed, edges=True):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(rows, cols, generator=g) * 0.02
    if edges and rows >= 8:
        w[1] = 0.0                         # all-zero row
        w[2] = w[2].abs() + 1e-3           # all positive
        w[3] = -(w[3].abs() + 1e-3)        # all negative
        w[4] = 0.375                       # constant
        w[5, cols // 2] = float("nan")     # NaN row
        w[6, cols - 1] = float("inf")      # Inf row
        w[7, 0] = float("-inf")
    return w.to(dtype)


def check(w, bits):
    from asvd4llm_amd import ops
    out, q, scale, zero, flagged = ops.rtn_quant(w, bits, want_params=True)
    r_out, r_q, r_scale, r_zero, ready = rtn_restate(w, bits)
    assert flagged == (not ready)
    assert out.dtype == w.dtype and out.shape == w.shape
    assert same(out, r_out)
    assert same(scale, r_scale) and same(zero, r_zero)
    if ready:
        assert torch.equal(q.cpu(), codes_of(r_q))


SHAPES = [(4096, 4096), (11008, 4096), (4096, 11008), (4096, 1843), (1843, 11008), (4096, 1), (40, 13824), (37, 1001)]


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{m}x{n}" for m, n in SHAPES])
@pytest.mark.parametrize("dt", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("bits", [8, 6])
def test_kernel_equals_restatement(gpu, shape, dt, bits):
    w = weight_like(*shape, DT[dt], seed=shape[0] * 7 + shape[1] + bits).to(gpu)
    check(w, bits)


@pytest.mark.parametrize("dt", ["f16", "bf16", "f32"])
def test_strided_views(gpu, dt):
    base = weight_like(300, 4200, DT[dt], seed=5).to(gpu)
    check(base[:, :4096], 8)          # ld != cols, rows 16-byte aligned: vector path
    check(base[:, 7:4103], 6)         # rows start off 16-byte alignment: element path
    check(base[3:250:2, 100:3000], 8)  # every other row


def test_fixture_rows_on_the_kernel(gpu, golden):
    from asvd4llm_amd import ops
    z = golden.npz("rtn_ref.npz")
    for c in z["cases"]:
        case, d, b = str(c).split(":")
        w = torch.from_numpy(z[case + "_x"]).to(DT[d]).to(gpu)
        out, q, scale, zero, flagged = ops.rtn_quant(w, int(b), want_params=True)
        assert flagged == (not bool(z[case + "_ready"])), case
        assert same(out.float(), torch.from_numpy(z[case + "_out"])), case
        assert same(scale, torch.from_numpy(z[case + "_scale"])) and same(zero, torch.from_numpy(z[case + "_zero"])), case
        if not flagged:
            assert torch.equal(q.cpu(), codes_of(torch.from_numpy(z[case + "_q"]))), case


def test_flagged_tensor_is_returned_unchanged(gpu):
    from asvd4llm_amd import ops
    w = weight_like(64, 512, torch.float32, seed=9, edges=False)
    w[10] = torch.tensor([(k % 5 - 2) * 1.4e-45 for k in range(512)])  # denormal-only row: its scale is 0
    w = w.to(gpu)
    keep = w.clone()
    other = weight_like(64, 512, torch.float32, seed=10).to(gpu)
    res = ops.rtn_quant_batched([w, other], 8, want_params=True)
    assert res[0][4] is True and res[1][4] is False
    assert res[0][0] is w and torch.equal(w, keep)
    assert same(res[1][0], rtn_restate(other, 8)[0])


def test_batched_mixed_equals_per_tensor(gpu):
    from asvd4llm_amd import ops
    specs = [(4096, 1843, "f16"), (1843, 4096, "bf16"), (300, 13824, "f32"), (37, 1001, "f16"), (4096, 1, "bf16"), (512, 8192, "f32"),
             (128, 352, "f16"), (64, 64, "f32"), (11008, 128, "f16"), (96, 4096, "bf16"), (10, 20, "f16"), (256, 256, "bf16"),
             (33, 4097, "f32"), (8, 13824, "f16"), (16, 16, "f32"), (1, 4096, "f16"), (77, 999, "bf16"), (640, 2048, "f16")]  # 18: two launches
    ws = [weight_like(m, n, DT[d], seed=i).to(gpu) for i, (m, n, d) in enumerate(specs)]
    ws.append(weight_like(300, 4200, torch.float16, seed=99).to(gpu)[:, 8:4104])
    for bits in (8, 6):
        batched = ops.rtn_quant_batched(ws, bits, want_params=True)
        for w, got in zip(ws, batched):
            one = ops.rtn_quant(w, bits, want_params=True)
            for a, b in zip(got[:4], one[:4]):
                assert same(a, b)
            assert got[4] == one[4] is False
            assert same(got[0], rtn_restate(w, bits)[0])


def _run_pipeline(name, tmp_path, monkeypatch):
    """asvd.main through calibration, search, decomposition and --weight_quant rtn_int8; returns (model, parameters just before the step,
    the evaluation result)"""
    import asvd
    from asvd4llm_amd import evaluate_utils, quantization
    monkeypatch.chdir(tmp_path)
    seen = {}
    real_step, real_eval = quantization.rtn_quant_sequential, evaluate_utils.evaluate_model

    def step(model, wbits):
        seen["before"] = {n: p.detach().clone() for n, p in model.named_parameters()}
        seen["model"], seen["bits"] = model, wbits
        # the one-launch forward's copies exist before the step: they must not survive it
        for m in model.modules():
            if type(m).__name__ == "SVDLinear":
                m._fused = ("stale",)
        return real_step(model, wbits)

    def evaluate(*a, **k):
        seen["result"] = real_eval(*a, **k)
        return seen["result"]

    monkeypatch.setattr(quantization, "rtn_quant_sequential", step)
    monkeypatch.setattr(evaluate_utils, "evaluate_model", evaluate)
    args = asvd.build_parser().parse_args(["--model_id", name, "--random_init", "--act_aware", "--alpha", "0.5", "--n_calib_samples", "4",
                                           "--calib_dataset", "synthetic", "--scaling_method", "abs_mean", "--param_ratio_target", "0.9",
                                           "--exclude_lm_head", "--weight_quant", "rtn_int8"])  # the search then factorises block Linears
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        asvd.main(args)
    assert seen["bits"] == 8
    return seen["model"], seen["before"], seen["result"]


@pytest.mark.parametrize("name", ["tiny-llama", "tiny-opt"])
def test_pipeline_quantizes_exactly_the_targets(gpu, name, tmp_path, monkeypatch):
    from asvd4llm_amd.modules.svd_linear import SVDLinear
    from asvd4llm_amd.quantization import rtn_targets
    monkeypatch.setenv("ASVD_STRICT", "1")
    model, before, result = _run_pipeline(name, tmp_path, monkeypatch)
    targets = {n + ".weight" for n, _ in rtn_targets(model)}
    svds = [m for m in model.modules() if isinstance(m, SVDLinear)]
    assert svds, "the search factorised nothing"
    assert any(t.endswith("ALinear.weight") for t in targets) and any(t.endswith("BLinear.weight") for t in targets)
    params = dict(model.named_parameters())
    assert set(params) == set(before)
    changed = 0
    for n, p in params.items():
        if n in targets:
            assert same(p.data, rtn_restate(before[n], 8)[0]), n
            changed += not torch.equal(p.data, before[n])
        else:
            assert torch.equal(p.data, before[n]), n   # lm_head, embeddings, norms, biases: untouched
    assert any("lm_head" in n or "embed" in n for n in params if n not in targets)
    assert changed >= len(targets) // 2
    assert all(m._fused is None for m in svds)     # refresh_fused on every SVDLinear
    assert math.isfinite(result["synthetic_ppl"])

    # the opt-in one-launch forward, built after the step, runs on the quantized factors
    monkeypatch.setenv("ASVD_FUSED_FORWARD", "1")
    g = torch.Generator().manual_seed(3)
    used = eligible = 0
    with torch.no_grad():
        for m in svds:
            x = (torch.randn(1, 3, m.BLinear.in_features, generator=g) * 0.5).half().to(gpu)
            y = m(x)
            y_two = m.ALinear(m.BLinear(x))
            used += m._fused is not None
            eligible += m.BLinear.in_features % 64 == 0 and m.ALinear.out_features <= 8192
            assert (y.float() - y_two.float()).abs().max().item() <= 4e-3 * y_two.float().abs().max().item() + 1e-3
    assert used == eligible


def test_cli_run_with_rtn_int8(gpu, tmp_path):
    env = dict(os.environ, ASVD_STRICT="1", PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "asvd.py"), "--model_id", "tiny-llama", "--random_init", "--act_aware", "--alpha", "0.5",
                          "--n_calib_samples", "4", "--calib_dataset", "synthetic", "--scaling_method", "abs_mean", "--param_ratio_target", "0.9",
                          "--rank_align", "8", "--weight_quant", "rtn_int8"], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "rtn int8:" in out.stdout
    m = re.search(r"'synthetic_ppl': ([0-9.eE+-]+|nan|inf)", out.stdout)
    assert m and math.isfinite(float(m.group(1))), out.stdout[-2000:]
