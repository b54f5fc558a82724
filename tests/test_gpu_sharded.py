"""The HIP path, sharded: two processes (torch.distributed, gloo rendezvous on 127.0.0.1) share the one GPU of the box and run the
REAL pipeline — calib_input_distribution -> calib_sensitivity_ppl -> binary_search_truncation_rank(--gather_factors rank0) — on the
hand-written kernels; rank 0's final model must be the single-process run's (BASELINE configs[3]/[4] logic on real kernels:
LPT layer shards, the fp64 sensitivity all-gather, the replicated search, owner-only decomposition, point-to-point factor exchange
with GPU tensors).  The world-size-2 tests in test_distributed_gloo.py cover the same logic on CPU with an oracle stand-in for
`from_linear`; here nothing is replaced."""
import contextlib
import io
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _build(kind, dev):
    from tests.tiny_lm import TinyLM, WideLM
    if kind == "tiny":
        model = TinyLM(d=64, f=176, n_layers=2, vocab=50, seed=3)
    else:
        model = WideLM(d=64, width=4096, f=176, vocab=50, seed=3)
    return model.to(dev)


def _worker(rank, ws, port, q, tmpdir, kind, shard_calib):
    os.chdir(tmpdir)
    os.environ["ASVD_STRICT"] = "1"
    import torch.distributed as dist
    torch.cuda.set_device(0)  # both ranks on the one GPU: separate processes, separate HIP contexts, separate workspaces
    if ws > 1:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=rank, world_size=ws)
    try:
        from asvd4llm_amd import _lib
        from asvd4llm_amd.act_aware_utils import calib_input_distribution
        from asvd4llm_amd.binary_search import binary_search_truncation_rank
        from asvd4llm_amd.modules.svd_linear import SVDLinear
        from asvd4llm_amd.sensitivity import calib_sensitivity_ppl
        from tests.tiny_lm import default_args
        _lib.load(require_device=True)
        dev = torch.device("cuda", 0)
        model = _build(kind, dev)
        g = torch.Generator().manual_seed(5)
        calib = [{"input_ids": torch.randint(0, 50, (1, 24), generator=g)} for _ in range(4)]
        args = default_args(n_calib_samples=4, param_ratio_target=0.75, gather_factors="rank0", offload_raw_to_cpu=False,
                            shard_calib=shard_calib)
        out = io.StringIO()
        with contextlib.redirect_stdout(out), contextlib.redirect_stderr(io.StringIO()):
            calib_input_distribution(model, calib, "abs_mean", use_cache=False, shard_samples=shard_calib)
            scal = {n: m.scaling_diag_matrix.float().cpu().numpy().copy() for n, m in model.named_modules()
                    if hasattr(m, "scaling_diag_matrix") and torch.is_tensor(m.scaling_diag_matrix)}  # before the search replaces modules
            sens = calib_sensitivity_ppl(model, calib, args, use_cache=False)
            binary_search_truncation_rank(model, sens, calib, args)
        torch.cuda.synchronize()
        swept = sum(1 for l in out.getvalue().splitlines() if (l.startswith("model.") or l.startswith("lm_head")) and len(l.split()) == 3)
        kinds = {n: type(m).__name__ for n, m in model.named_modules() if n in model._asvd_layers_min_ratio}
        ranks = {n: int(m.truncation_rank) for n, m in model.named_modules() if isinstance(m, SVDLinear)}
        state = {k: v.detach().float().cpu().numpy().copy() for k, v in model.state_dict().items()}
        q.put((rank, sens, dict(model._asvd_layers_min_ratio), kinds, ranks, state, swept, scal, getattr(model, "_asvd_factor_exchange", None)))
    finally:
        if ws > 1:
            dist.destroy_process_group()


def _run(tmp_path, ws, kind, shard_calib=False, tag=""):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = []
    for r in range(ws):
        d = tmp_path / f"{kind}{tag}_w{ws}_{r}"
        d.mkdir()
        procs.append(ctx.Process(target=_worker, args=(r, ws, port, q, str(d), kind, shard_calib)))
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=600) for _ in range(ws)], key=lambda t: t[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    return res


def _product(state, name):
    import numpy as np
    return state[name + ".ALinear.weight"].astype(np.float64) @ state[name + ".BLinear.weight"].astype(np.float64)


@pytest.mark.timeout(1200)
@pytest.mark.parametrize("kind", ["tiny", "wide"])
def test_two_ranks_one_gpu_equal_single_process(tmp_path, kind):
    import numpy as np
    (r1,) = _run(tmp_path, 1, kind)
    _, sens1, ratios1, kinds1, ranks1, state1, swept1, scal1, _ = r1
    n_lin = len(sens1)
    assert swept1 == n_lin * 6 and sum(1 for k in kinds1.values() if k == "SVDLinear") >= 3
    res = _run(tmp_path, 2, kind)
    assert res[0][6] + res[1][6] == n_lin * 6 and 0 < res[0][6] < n_lin * 6  # the sweep was split, nothing evaluated twice
    for rk, sens, ratios, kinds, ranks, state, swept, scal, xch in res:
        assert list(sens.keys()) == list(sens1.keys())
        for name in sens1:  # a layer's perplexities do not depend on which rank (or which batch of same-shape layers) factorised it
            for ratio, v in sens1[name].items():
                assert abs(sens[name][ratio] - v) <= 2e-4 * abs(v), (name, ratio, sens[name][ratio], v)
        assert ratios == ratios1  # the replicated search picks the same cut on every rank
        for n in scal1:
            assert np.array_equal(scal[n], scal1[n]), n  # replicated hook pass: identical statistics
    rk, sens, ratios, kinds, ranks, state, swept, scal, xch = res[0]
    assert kinds == kinds1 and ranks == ranks1, "rank 0 does not hold the complete compressed model"
    assert xch is not None and xch["mode"] == "rank0" and xch["received"] >= 1  # factors crossed process boundaries as GPU tensors
    assert state.keys() == state1.keys()
    for name, k in kinds1.items():
        if k != "SVDLinear":
            continue
        P, P1 = _product(state, name), _product(state1, name)
        assert np.linalg.norm(P - P1) <= 2e-4 * np.linalg.norm(P1), name  # same factorisation up to the batch it was solved in
    n_svd_other = sum(1 for k in res[1][3].values() if k == "SVDLinear")
    assert 0 < n_svd_other < sum(1 for k in kinds1.values() if k == "SVDLinear")  # rank 1 keeps only its shard


@pytest.mark.timeout(900)
def test_calibration_samples_sharded_allreduce(tmp_path):
    """--shard_calib: each rank runs the hook pass over its own calibration samples and the [C] accumulators are all-reduced (sum for
    abs_mean).  The statistics equal the replicated pass up to the rounding of a different summation order in the activation dtype."""
    import numpy as np
    (r1,) = _run(tmp_path, 1, "tiny")
    res = _run(tmp_path, 2, "tiny", shard_calib=True, tag="sc")
    scal1 = r1[7]
    for rk in range(2):
        scal = res[rk][7]
        assert scal.keys() == scal1.keys()
        for n in scal1:
            assert np.allclose(scal[n], scal1[n], rtol=1e-5, atol=1e-7), n
    for n in scal1:
        assert np.array_equal(res[0][7][n], res[1][7][n]), n  # every rank ends with the same accumulators


@pytest.mark.timeout(1200)
def test_bench_two_ranks_on_one_gpu_run_the_whole_multi_gpu_leg(tmp_path):
    """`bench.py --gpus 2` as the driver launches it, except that both ranks share cuda:0 and the collectives run over gloo (RCCL refuses two ranks
    per device): the timed weak-scaling loop with the real kernels (each rank its own batch, split over the chip halves), barrier + max over ranks,
    per-rank rates, then the sharded model leg — LPT shard, every rank decomposes its own Linears, the all-gather of the sensitivities, the
    replicated search, the factor gather into rank 0 — and ONE JSON line on rank 0."""
    import json
    import subprocess
    import sys
    from tests.conftest import ROOT
    import os
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dist_backend", "gloo", "--same_gpu", "--batch", "4", "--steps", "1", "--warmup", "1",
           "--prewarm_s", "0", "--full", "--sharded_model", "llama-7b-2layers"]
    env = dict(os.environ, ASVD_STRICT="1")
    env.pop("WORLD_SIZE", None)
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=1100, env=env, cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["value"] > 0 and d["scaling"] == "weak" and len(d["per_rank_svds_per_s"]) == 2
    sm = d["sharded_model"]
    assert "error" not in sm, sm
    assert sm["linears"] == 15 and sum(sm["layers_per_rank"]) == 15 and min(sm["layers_per_rank"]) >= 1
    assert sm["collective_world_size"] == 2 and sm["plan_identical_on_all_ranks"]
    assert sm["gather_factors_s"] > 0 and sm["gather_factors_bytes_into_rank0"] > 1e6     # rank 1's factors reached rank 0
    assert sm["decompose_s"] > 0 and sm["load_flops_max_over_mean"] < 1.3
    # two processes on ONE device: the library sees the other rank (the lock file of include/asvd_hip.h, "REFUSALS") and does not split its
    # batches over "the first half + the second half" of CUs both ranks would claim — detected, not configured
    assert d["config"]["batch_split_over_chip_halves"] is False and d["config"]["split_refused_device_shared_or_masked"] is True, d["config"]
    dv = d["devices"]
    assert dv["visible_device_count"] >= 1 and len(dv["per_rank"]) == 2 and [x["rank"] for x in dv["per_rank"]] == [0, 1]
    assert all(x["device_index"] == 0 and x["pci_bus_id"] for x in dv["per_rank"]) and dv["host_group_backend"] == "gloo"


@pytest.mark.timeout(1200)
def test_bench_keeps_the_line_when_the_rccl_group_cannot_be_created(tmp_path):
    """The first multi-GPU run must not be able to lose the line (VERDICT r5 task 4): `--dist_backend nccl` with the creation of the RCCL group
    forced to fail (ASVD_BENCH_FAIL_NCCL).  Rendezvous, the barriers around the timed region and the MAX-reduce run on the gloo host group, so
    n_gpus, value and the per-rank rates are there; the sharded-model leg falls back to the host group and says so."""
    import json
    import subprocess
    import sys
    from tests.conftest import ROOT
    import os
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dist_backend", "nccl", "--same_gpu", "--batch", "4", "--steps", "1", "--warmup", "1",
           "--prewarm_s", "0", "--full", "--sharded_model", "llama-7b-2layers"]
    env = dict(os.environ, ASVD_STRICT="1", ASVD_BENCH_FAIL_NCCL="1")
    env.pop("WORLD_SIZE", None)
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=1100, env=env, cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["value"] > 0 and d["scaling"] == "weak" and len(d["per_rank_svds_per_s"]) == 2 and all(v > 0 for v in d["per_rank_svds_per_s"])
    sm = d["sharded_model"]
    assert "error" not in sm, sm
    assert "RCCL group unavailable" in sm["collective_backend_note"] and sm["collective_backend"].startswith("gloo")
    assert sm["collective_world_size"] == 2 and sm["plan_identical_on_all_ranks"] and sm["gather_factors_bytes_into_rank0"] > 1e6


@pytest.mark.timeout(900)
def test_bench_watchdog_keeps_the_line_when_the_sharded_leg_does_not_come_back(tmp_path):
    """N > 1: the untimed sharded-model leg runs collectives that may never have run on the node; if it does not finish within --sharded_timeout_s the
    bench line — complete before the leg starts — is printed by rank 0 with the reason, every rank ends with exit code 0 (here: a timeout far
    below the leg's run time)."""
    import json
    import os
    import subprocess
    import sys
    from tests.conftest import ROOT
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dist_backend", "gloo", "--same_gpu", "--batch", "4", "--steps", "1", "--warmup", "0",
           "--prewarm_s", "0", "--full", "--sharded_model", "llama-7b-2layers", "--sharded_timeout_s", "0.05"]
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=800, env=env, cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["value"] > 0 and len(d["per_rank_svds_per_s"]) == 2
    assert "did not finish" in d["sharded_model"]["error"]
