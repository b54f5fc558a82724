"""Time of the re-orthonormalisation pass (K18, asvd_reorth_batched) and its price on top of the SVD it repairs.

  python tools/bench_reorth.py [--batch 32] [--m 4096] [--ks 4096,1843] [--reps 3] [--no_svd] [--out profiles/reorth.json]

Part 1, the entry point alone at batch x m x k: on an orthonormal input (0 passes: ONE Gram pass, nothing written) and on
Q0 = Haar (I + eps triu(randn)), eps = 1e-2 and 2e-3 (p passes: p + 1 Gram passes and p updates; eps = 1e-2 at k = 4096 has a diagonal defect
eps^2 k = 0.4 and is REFUSED by the 0.25 guard: that line times the refusal, one Gram pass).  Every repetition starts from a fresh copy made outside the timed
window; the window is a host clock around the host-synchronous call plus a device synchronise.  Derived (named as such): the update's share per
pass = (t_perturbed - (p + 1) t_gram) / p.
Part 2, ops.svd_batched(..., ortho=True) against the same call without it, alternating, in this process: the `geo3` / abs_max / alpha 1 batch
and the `llm_like` batch of bench.py under abs_mean / alpha 0.5 (its weights are flat, its SCALED matrix is graded too: 2 - 7 passes measured).
No device: the script fails (there is no CPU path)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--m", type=int, default=4096)
    ap.add_argument("--ks", default="4096,1843")
    ap.add_argument("--eps", default="1e-2,2e-3", help="perturbations of the Haar input; 1e-2 at k = 4096 enters above the 0.25 guard (E_jj ~ eps^2 k) and is refused")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no_svd", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from asvd4llm_amd import ops
    from tests import families as F
    assert torch.cuda.is_available(), "bench_reorth needs a gfx950 device"
    dev = torch.device("cuda", 0)
    B, m = a.batch, a.m
    records = []

    def emit(rec):
        records.append(rec)
        print(json.dumps(rec), flush=True)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    g = torch.Generator().manual_seed(5)
    for k in [int(x) for x in a.ks.split(",") if x]:
        H = F.haar(m, k, g, dev)                                      # fp64, on the device (input generation only)
        N = torch.triu(torch.randn(k, k, generator=g, dtype=torch.float64)).to(dev)
        perms = [torch.randperm(m, generator=g).to(dev) for _ in range(B)]   # row permutations of a Haar matrix are Haar
        t_gram = None
        for label, eps in [("orthonormal", 0.0)] + [("eps_" + e, float(e)) for e in a.eps.split(",") if e]:
            src = H if eps == 0.0 else H @ (torch.eye(k, dtype=torch.float64, device=dev) + eps * N)
            masters = [src[p].float().contiguous() for p in perms]
            ops.reorth_batched([q.clone() for q in masters[:2]])     # warm-up: code objects, attributes
            times, infos = [], None
            for _ in range(a.reps):
                work = [q.clone() for q in masters]
                ms, infos = timed(lambda: ops.reorth_batched(work))
                times.append(round(ms, 2))
            emit({"what": "asvd_reorth_batched", "batch": B, "m": m, "k": k, "input": label, "ms": times, "ms_min": min(times),
                  "passes_min": min(i.passes for i in infos), "passes_max": max(i.passes for i in infos), "status_max": max(i.status for i in infos),
                  "e_before_max": max(i.e_before for i in infos), "e_after_max": max(i.e_after for i in infos)})
            del masters, work, src
            rec = records[-1]
            if eps == 0.0:
                t_gram = rec["ms_min"]
            p = rec["passes_max"]
            if p > 0 and rec["passes_min"] == p:
                emit({"what": "derived per pass", "batch": B, "m": m, "k": k, "input": label, "gram_ms": t_gram, "update_ms": round((rec["ms_min"] - (p + 1) * t_gram) / p, 2),
                      "note": "gram_ms = the 0-pass call (one Gram pass incl. its host synchronisation); update_ms = (t - (p + 1) gram_ms) / p"})
        del H, N, perms
        torch.cuda.empty_cache()

    if not a.no_svd:
        n = m

        def llm_like(seed):
            gg = torch.Generator().manual_seed(seed)
            W = torch.randn(m, n, generator=gg) * 0.02
            W[:, torch.randperm(n, generator=gg)[:max(1, int(0.005 * n))]] *= 20
            scal = 32 * torch.randn(n, generator=gg).abs()
            scal[torch.randperm(n, generator=gg)[:max(1, int(0.01 * n))]] *= 30
            return W, scal.half()

        for kind, stat, alpha in (("geo3", "abs_max", 1.0), ("llm_like", "abs_mean", 0.5)):
            mats, stats = [], []
            if kind == "llm_like":
                for b in range(B):
                    W, st = llm_like(1000 + b)
                    mats.append(W.to(dev))
                    stats.append(st.to(dev))
            else:
                gg = torch.Generator().manual_seed(77)
                Pm, Qm, sig = F.haar(m, n, gg, dev), F.haar(n, n, gg, dev), F.spectrum(kind, n).to(dev)
                for b in range(B):
                    pm, pn = torch.randperm(m, generator=gg).to(dev), torch.randperm(n, generator=gg).to(dev)
                    W = (Pm[pm] * sig) @ Qm[pn].T
                    mats.append((W * (0.02 * (m * n) ** 0.5 / float(W.norm()))).float().contiguous())
                    stats.append(F.make_stat(stat, n, seed=b).to(dev))
                del Pm, Qm
            scs = ops.make_scale_batched(stats, None, alpha)
            ops.svd_batched(mats[:4], scs[:4], ortho=True)            # warm-up of both paths
            plain, fixed, infos = [], [], None
            for _ in range(a.reps):                                   # alternating, same process
                ms, out = timed(lambda: ops.svd_batched(mats, scs))
                plain.append(round(ms, 1))
                del out
                ms, out = timed(lambda: ops.svd_batched(mats, scs, ortho=True))
                fixed.append(round(ms, 1))
                infos = out[3]
                del out
            emit({"what": "ops.svd_batched ortho=True vs plain", "family": kind, "stat": stat, "alpha": alpha, "batch": B, "m": m, "n": n, "plain_ms": plain,
                  "ortho_ms": fixed, "overhead": round(min(fixed) / min(plain) - 1.0, 4), "sweeps_max": max(i.sweeps for i in infos),
                  "reorth_passes_min": min(i.reorth.passes for i in infos), "reorth_passes_max": max(i.reorth.passes for i in infos),
                  "reorth_status_max": max(i.reorth.status for i in infos), "e_before_max": max(i.reorth.e_before for i in infos),
                  "e_after_max": max(i.reorth.e_after for i in infos)})
            del mats, scs, stats
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(records, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
