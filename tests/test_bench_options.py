"""bench.py's plain run against --full, and --dump-outputs: what the timed path computed in its last step, as float32 .npy files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.conftest import ROOT

BENCH = os.path.join(ROOT, "bench.py")


def _line(p):
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.timeout(300)
def test_dry_run_keeps_the_extras_behind_full():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    plain = _line(subprocess.run([sys.executable, BENCH, "--dry_run", "--steps", "2"], env=env, capture_output=True, text=True, timeout=240))
    assert plain["sharded_model"] is None and plain["steps"] == 2
    full = _line(subprocess.run([sys.executable, BENCH, "--dry_run", "--full", "--steps", "2"], env=env, capture_output=True, text=True, timeout=240))
    assert full["sharded_model"]["plan_identical_on_all_ranks"] is True and full["sharded_model"]["linears"] == 22


def test_dump_outputs_is_a_fixed_sample_within_the_budget(tmp_path):
    """dump_outputs on host tensors of the default bench shapes (the device path only adds a copy): the whole S / scales / flags, the same seeded
    positions of U, V, A, B in every problem, float32, at most 64 MB, and the same files from two calls"""
    sys.path.insert(0, ROOT)
    import bench
    B, m, n, r = 32, 4096, 4096, 512
    g = torch.Generator().manual_seed(5)
    U0 = torch.randn(m, n, generator=g)
    U = [U0 + b for b in range(B)]
    V = [U0 - b for b in range(B)]
    S = [torch.rand(n, generator=g).sort(descending=True).values for _ in range(B)]
    scales = [torch.rand(n, generator=g).half() for _ in range(B)]
    flags = torch.zeros((B, 3), dtype=torch.int32)
    outs = [(U[b][:, :r].half(), V[b][:, :r].T.contiguous().half(), flags[b]) for b in range(B)]
    total = bench.dump_outputs(str(tmp_path / "a"), U, S, V, scales, outs)
    bench.dump_outputs(str(tmp_path / "b"), U, S, V, scales, outs)
    assert total <= 64 << 20
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(["S.npy", "scales.npy", "nan_flags.npy", "U_sample.npy", "V_sample.npy", "A_sample.npy", "B_sample.npy"])
    got = {f: np.load(tmp_path / "a" / f) for f in names}
    for f in names:
        assert got[f].dtype == np.float32 and got[f].shape[0] == B, f
        assert np.array_equal(got[f], np.load(tmp_path / "b" / f)), f
    assert np.array_equal(got["S.npy"], torch.stack(S).numpy())
    assert np.array_equal(got["scales.npy"], torch.stack(scales).float().numpy())
    assert not got["nan_flags.npy"].any()
    # U[b] = U0 + b: one set of positions for every problem of the batch
    s = got["U_sample.npy"]
    assert s.shape[1] > 1000 and np.allclose(s - s[0], np.arange(B, dtype=np.float32)[:, None])
    assert np.allclose(got["V_sample.npy"] - got["V_sample.npy"][0], -np.arange(B, dtype=np.float32)[:, None])


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_plain_bench_prints_the_headline_and_dumps_its_last_timed_step(gpu, tmp_path):
    """a plain run: exactly --steps timed steps, the headline keys and none of the --full extras; the dumped spectrum is that of the synthetic
    inputs (the same from run to run) under the dumped scales"""
    sys.path.insert(0, ROOT)
    import bench
    env = dict(os.environ, ASVD_STRICT="1")
    env.pop("WORLD_SIZE", None)
    args = ["--gpus", "1", "--batch", "4", "--m", "768", "--n", "512", "--rank", "64", "--steps", "3", "--warmup", "1", "--prewarm_s", "0"]
    recs, dumps = [], []
    for tag in ("a", "b"):
        d = tmp_path / tag
        recs.append(_line(subprocess.run([sys.executable, BENCH] + args + ["--dump-outputs", str(d)], capture_output=True, text=True, timeout=400,
                                         env=env, cwd=str(tmp_path))))
        dumps.append({f[:-4]: np.load(d / f) for f in os.listdir(d)})
    rec = recs[0]
    assert rec["metric"] == "weight-matrix SVDs/sec (4096x4096 fp32)" and rec["unit"] == "SVD/s" and rec["higher_is_better"] is True
    assert rec["dtype"] == "f32" and rec["steps"] == 3 and len(rec["step_wall_ms"]) == 3 and rec["n_gpus"] == 1
    assert rec["value"] > 0 and rec["ms_per_step"] > 0 and abs(rec["value"] - 4 * 1e3 / rec["ms_per_step"]) <= 1e-6 * rec["value"]
    for extra in ("roofline", "full_model", "cpu_baseline", "parity", "k9_reconstruct", "latency_batch1_ms"):
        assert extra not in rec, extra
    a, b = dumps
    assert set(a) == {"S", "scales", "nan_flags", "U_sample", "V_sample", "A_sample", "B_sample"}
    assert all(v.dtype == np.float32 for v in a.values())
    assert a["S"].shape == (4, 512) and a["scales"].shape == (4, 512) and a["nan_flags"].shape == (4, 3) and not a["nan_flags"].any()
    assert np.array_equal(a["scales"], b["scales"])
    assert np.allclose(a["S"], b["S"], rtol=1e-5, atol=0)
    assert np.abs(a["A_sample"]).max() > 0 and np.abs(a["B_sample"]).max() > 0
    for p in range(4):
        W, _ = bench.synth(768, 512, seed=233 + p)
        ref = torch.linalg.svdvals(W.double() * torch.from_numpy(a["scales"][p]).double())
        assert np.allclose(a["S"][p], ref.numpy(), rtol=1e-4, atol=1e-5 * float(ref[0])), p
