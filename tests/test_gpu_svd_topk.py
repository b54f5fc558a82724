"""The SVD at the rank the sensitivity sweep requests (k < min(m, n)), and the fallback paths that run the whole batch.

Every real run asks asvd_svd_batched for k = the largest rank among the sweep's candidate ratios (sensitivity.py: `_asvd_rank_hint`), and every
rank the binary search uses later is a slice of those factors.  With k < min(m, n) the driver enforces convergence only on the first
kb = ceil(k / 32) + 1 panels, stops the sweeps as soon as those are done, sorts ALL columns by norm and gathers the top k (rank_kernel /
gather_kernel), and the tall epilogue (row un-permutation, long-side product, sigma and column scales) runs on a ragged k.  Each call here is
checked against a plain high-precision reference of the same fp32 matrix Ws = W diag(s), never against the library's own full call alone:
  * the fp64 spectrum of Ws (torch on the device, a CHECKER) with the bar, floor and oracle slack of check_family (tests/test_gpu_families.py);
  * Eckart-Young at every slice rank of the sweep and at k: |Ws - U_r S_r V_r^T|_F^2 - sum_{j>r} sigma_j^2 <= (1e-3)^2 |Ws|_F^2 — a leading set
    that is not the top k fails it;
  * orthonormality and triplet residuals on a spread over [0, k) AND on the last 64 columns (the boundary panel and its margin);
  * the CPU oracle's own rank-r reconstructions (oracle/asvd_oracle.py) where its vectors are affordable (<= 2048);
  * the same matrix with the full k: no more sweeps, the same leading k singular values (2e-6 sigma_1), the same rank-r reconstructions (1e-4).
Path bits are asserted by every case: a case that silently left the arithmetic it is meant to test would otherwise look green."""
from types import SimpleNamespace

import pytest
import torch
import torch.nn as nn

from oracle import asvd_oracle as O
from tests import families as F
from tests.test_gpu_families import EPS32, family_case
from tests.test_gpu_svd import REC_TOL, SIG_TOL, llm_like

pytestmark = pytest.mark.gpu


def sweep_ranks(m, n, rank_align=1):
    """(k, R) of the sensitivity sweep for an out x in = m x n Linear: R the slice ranks of its candidate ratios, k = max(R) the rank hint its
    factorisation is asked for (sensitivity.py: `_ppl_candidates`, `_asvd_rank_hint`).  Not hard-coded: the tests follow the sweep."""
    from asvd4llm_amd import sensitivity
    from asvd4llm_amd.modules.svd_linear import SVDLinear
    args = SimpleNamespace(compress_kv_cache=False, rank_align=rank_align)
    lin = nn.Linear(n, m, bias=False, device="meta")
    R = sorted({SVDLinear.compute_rank(lin, r, rank_align) for r in sensitivity._ppl_candidates(args)})
    return R[-1], R


def reference(gpu, Ws, oracle_vectors):
    """(fp64 spectrum of the fp32 Ws on the device, the CPU oracle's (U, S, V) or None)"""
    S64 = torch.linalg.svdvals(Ws.to(gpu).double()).cpu()
    return S64, (O.exact_svd(Ws) if oracle_vectors else None)


def check_topk(gpu, Ws, got, k, R, S64, oracle=None, full=None, exact_rank=None, unique=True, tag=()):
    """Asserts the contract of a k-truncated call `got` = (U, S, V, info) on the fp32 matrix Ws (CPU).  R: slice ranks (those > k are ignored).
    oracle: CPU (U, S, V) of Ws.  full: (U, S, V, info) of the full-k call on the same matrix in the same batch.  exact_rank: Ws is exactly of
    this rank (its null columns have no defined singular direction: their values are bounded absolutely, their vectors are not sampled).
    unique=False: a cut falls inside an exactly degenerate cluster, where no rank-r reconstruction is unique (not compared)."""
    U, S, V, info = got
    m, n = Ws.shape
    assert U.shape == (m, k) and S.shape == (k,) and V.shape == (n, k), tag
    assert info.status == 0, tag + (info,)
    Sc = S.cpu().double()
    assert bool((Sc[:-1] >= Sc[1:]).all()), tag + ("singular values not sorted",)
    ks = k if exact_rank is None else min(k, exact_rank)
    # sigma: relative bar against the fp64 spectrum above the floor of the fp32 input; within the bar of the fp32 oracle up to its own error
    floor = EPS32 * S64[0]
    e64 = ((Sc[:ks] - S64[:ks]).abs() - floor).clamp(min=0.0) / S64[:ks]
    assert e64.max().item() <= SIG_TOL, tag + ("sigma vs fp64", e64.max().item(), int(e64.argmax()))
    if ks < k:
        assert (Sc[ks:].abs().max() / S64[0]).item() <= 1e-5, tag + ("null columns", Sc[ks:].abs().max().item())
    if oracle is not None:
        So = oracle[1][:k].double()
        excess = ((Sc - So).abs() - (So - S64[:k]).abs() - floor)[:ks] / S64[:ks]
        assert excess.max().item() <= SIG_TOL, tag + ("sigma vs the fp32 oracle beyond its own error", excess.max().item())
        assert ((Sc - So).abs().max() / So[0]).item() <= SIG_TOL, tag
    Wsd = Ws.to(gpu).double()
    Ud, Sd, Vd = U.double(), S.double(), V.double()
    # orthonormality and triplet residuals (bars of check_family): a spread over [0, ks) and the last 64 columns.  The side whose vectors are the
    # rotated columns themselves is orthonormal to 1e-5 flat; the other side is computed from it (reduced path: the long side, X v / sigma; direct
    # path: the short side, backsolved) and carries the sigma_1 / sigma_j amplification, while its own defining equation has residual ~ 0
    idx = torch.unique(torch.cat([torch.arange(0, ks, max(1, ks // 128)), torch.arange(max(0, ks - 64), ks)])).to(gpu)
    eye = torch.eye(idx.numel(), dtype=torch.float64, device=gpu)
    amp = (Sd[0] / Sd[idx]).clamp(min=1.0)
    amp2 = torch.maximum(amp.unsqueeze(0), amp.unsqueeze(1))
    short, long_ = (Vd, Ud) if m >= n else (Ud, Vd)
    res_u = (Wsd @ Vd[:, idx] - Ud[:, idx] * Sd[idx]).norm(dim=0) / Sd[0]
    res_v = (Wsd.T @ Ud[:, idx] - Vd[:, idx] * Sd[idx]).norm(dim=0) / Sd[0]
    res_long, res_short = (res_u, res_v) if m >= n else (res_v, res_u)   # the residual of the equation that defines the long / short side
    rot, der, res_der, res_rot = (short, long_, res_long, res_short) if info.reduced else (long_, short, res_short, res_long)
    go = (rot[:, idx].T @ rot[:, idx] - eye).abs()
    assert go.max().item() <= 1e-5, tag + ("orthonormality of the rotated side", go.max().item())
    gd = (der[:, idx].T @ der[:, idx] - eye).abs()
    assert bool((gd <= 1e-4 + 2e-6 * amp2).all()), tag + ("orthonormality of the computed side", gd.max().item(), amp.max().item())
    # (the bar of check_family is 2e-5; the int8 long-side product leaves 2.1e-5 on the DOMINANT column of 5120^2 pow1 / abs_max / alpha 1 — with
    # the full k too, and 4e-6 through the bf16 form, ASVD_NN_I8=0 — measured on an MI355X; sigma_1 is refined from the same product and stays
    # within its 1e-4 bar, but the error enters both residuals of that triplet)
    assert res_der.max().item() <= 5e-5, tag + ("defining residual of the computed side", res_der.max().item())
    assert bool((res_rot <= 5e-5 + 1e-6 * amp).all()), tag + ("residual of the rotated side", res_rot.max().item(), amp.max().item())
    if full is not None:
        Uf, Sf, Vf, info_f = full
        assert info.sweeps <= info_f.sweeps, tag + (info, info_f)
        assert ((S - Sf[:k]).abs().max() / Sf[0]).item() <= 2e-6, tag + ("sigma vs the full-k call",)
    # Eckart-Young at every slice rank and at k; the reconstructions against the oracle's and the full-k call's
    tot2 = (S64 ** 2).sum().item()
    for r in sorted({r for r in R if r <= k} | {k}):
        Rg = (Ud[:, :r] * Sd[:r]) @ Vd[:, :r].T
        err2 = ((Wsd - Rg) ** 2).sum().item()
        tail2 = (S64[r:] ** 2).sum().item()
        assert abs(err2 - tail2) <= (REC_TOL ** 2) * tot2, tag + ("Eckart-Young", r, err2, tail2, tot2)
        if not unique:
            continue
        if oracle is not None:
            Uo, So, Vo = (t.to(gpu).double() for t in oracle)
            rec = ((Rg - (Uo[:, :r] * So[:r]) @ Vo[:, :r].T).norm() / Wsd.norm()).item()
            assert rec <= REC_TOL, tag + ("reconstruction vs the oracle's", r, rec)
        if full is not None:
            Rf = (Uf[:, :r].double() * Sf[:r].double()) @ Vf[:, :r].double().T
            rel = ((Rg - Rf).norm() / Rf.norm()).item()
            assert rel <= 1e-4, tag + ("reconstruction vs the full-k call", r, rel)


def healthy(info):
    return info.status == 0 and info.reduced and not info.reduce_fallback and not info.plain_retry


def run_family(gpu, kind, stat, alpha, m, n, seed, ks, oracle_vectors, tag):
    """one matrix, its references and its full-k call computed once; every (k, R) of `ks` checked against them.  Returns the infos."""
    from asvd4llm_amd import ops
    W, s = family_case(kind, stat, alpha, m, n, seed, device=(gpu if max(m, n) >= 2048 else "cpu"))
    Wd, sd = W.to(gpu), (None if s is None else s.to(gpu))
    Ws = O.scaled_weight(W, s)
    S64, orc = reference(gpu, Ws, oracle_vectors)
    full = ops.svd(Wd, sd)
    infos = [full[3]]
    for k, R in ks:
        got = ops.svd(Wd, sd, k=k)
        check_topk(gpu, Ws, got, k, R, S64, oracle=orc, full=full, unique=kind != "cluster8" or s is not None, tag=tag + (k,))
        infos.append(got[3])
    return infos


# ---- 2a / 2b: the input families at the sweep's k ------------------------------------------------------------------------------------------
@pytest.mark.timeout(1200)
@pytest.mark.parametrize("alpha", [0.5, 1.0])
@pytest.mark.parametrize("stat", F.STATS)
@pytest.mark.parametrize("kind", F.SPECTRA)
def test_topk_families_1024(gpu, kind, stat, alpha):
    """k = 460 (ragged: 14 full panels + 12 columns) and the --rank_align 128 hint 512; the oracle's vectors compared"""
    infos = run_family(gpu, kind, stat, alpha, 1024, 1024, 101, [sweep_ranks(1024, 1024), sweep_ranks(1024, 1024, 128)], True, (kind, stat, alpha))
    assert all(healthy(i) for i in infos), infos


@pytest.mark.timeout(1200)
@pytest.mark.parametrize("kind,stat,alpha", [(k, "abs_max", 1.0) for k in F.SPECTRA] + [("pow1", "abs_mean", 0.5), ("lowrank_noise", "abs_mean", 0.5)])
def test_topk_families_2048(gpu, kind, stat, alpha):
    """2048^2 (the ring visit of the eigen-solves) at k = 921"""
    infos = run_family(gpu, kind, stat, alpha, 2048, 2048, 202, [sweep_ranks(2048, 2048)], True, (kind, stat, alpha))
    assert all(healthy(i) for i in infos), infos


# ---- 2c: production shapes at the sweep's k (size-independent checks) ----------------------------------------------------------------------
PROD = [((4096, 4096), "llm_like", None, None), ((4096, 4096), "pow1", "abs_max", 1.0), ((4096, 4096), "lowrank_noise", "abs_mean", 0.5),
        ((11008, 4096), "llm_like", None, None), ((11008, 4096), "pow1", "abs_max", 1.0),
        ((4096, 11008), "llm_like", None, None), ((4096, 11008), "pow1", "abs_max", 1.0),
        ((5120, 5120), "llm_like", None, None), ((5120, 5120), "pow1", "abs_max", 1.0)]


@pytest.mark.timeout(1500)
@pytest.mark.parametrize("shape,kind,stat,alpha", PROD)
def test_topk_production_shapes(gpu, monkeypatch, shape, kind, stat, alpha):
    """4096^2 at k = 1843 and the aligned 1920, 11008 x 4096 and the WIDE 4096 x 11008 at the ragged k = 2686, 5120^2 at k = 2304 (a multiple of 32)"""
    from asvd4llm_amd import ops
    m, n = shape
    ks = [sweep_ranks(m, n)] + ([sweep_ranks(m, n, 128)] if shape == (4096, 4096) else [])
    tag = (shape, kind, stat, alpha)
    if kind == "llm_like":
        W, s = llm_like(m, n, seed=41)
        Wd, sd = W.to(gpu), s.to(gpu)
        Ws = O.scaled_weight(W, s)
        S64, _ = reference(gpu, Ws, False)
        full = ops.svd(Wd, sd)
        infos = [full[3]]
        for k, R in ks:
            got = ops.svd(Wd, sd, k=k)
            check_topk(gpu, Ws, got, k, R, S64, full=full, tag=tag + (k,))
            infos.append(got[3])
    else:
        infos = run_family(gpu, kind, stat, alpha, m, n, 303, ks, False, tag)
    assert all(healthy(i) for i in infos), infos
    if kind == "lowrank_noise":
        # rank n/4 + noise is the family whose int8 Cholesky can break down and be repeated on the fp64 Gram matrix (GRAM_RETRY: one of a batch of 32
        # does in profiles/r6_families.txt).  Whether THIS matrix does is a rounding event — on an MI355X it does not — so the arithmetic of the
        # retry is selected outright and checked at the sweep's k as well
        monkeypatch.setenv("ASVD_GRAM_I8", "0")
        infos = run_family(gpu, kind, stat, alpha, m, n, 303, ks, False, tag + ("fp64 Gram",))
        assert all(healthy(i) and not i.gram_retry for i in infos), infos


@pytest.mark.timeout(1200)
def test_topk_split_batch_each_problem_against_the_reference(gpu):
    """4 x 4096^2 at k = 1843: the default split over the two chip halves runs; every problem is checked against its own reference"""
    from asvd4llm_amd import ops
    k, R = sweep_ranks(4096, 4096)
    mats, scs = zip(*[llm_like(4096, 4096, seed=60 + b) for b in range(4)])
    md, sdv = [W.to(gpu) for W in mats], [s.to(gpu) for s in scs]
    U, S, V, infos = ops.svd_batched(md, sdv, k=k)
    Uf, Sf, Vf, infos_f = ops.svd_batched(md, sdv)
    assert all(healthy(i) and i.split for i in infos + infos_f), infos + infos_f
    for b in range(4):
        Ws = O.scaled_weight(mats[b], scs[b])
        S64, _ = reference(gpu, Ws, False)
        check_topk(gpu, Ws, (U[b], S[b], V[b], infos[b]), k, R, S64, full=(Uf[b], Sf[b], Vf[b], infos_f[b]), tag=("split", b))


# ---- 2d: edge values of k ------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(900)
@pytest.mark.parametrize("shape", [(1536, 1024), (1024, 1536)])
def test_topk_edge_k(gpu, shape):
    """nb = 32 panels: k at and around panel boundaries; 960 is the largest k with kb < nb, 961 the first with kb = nb; 1023 leaves one column"""
    from asvd4llm_amd import ops
    m, n = shape
    _, R = sweep_ranks(m, n)
    W, s = llm_like(m, n, seed=43)
    Wd, sd = W.to(gpu), s.to(gpu)
    Ws = O.scaled_weight(W, s)
    S64, orc = reference(gpu, Ws, True)
    full = ops.svd(Wd, sd)
    assert healthy(full[3]), full[3]
    for k in (1, 31, 32, 33, 63, 65, 960, 961, 1023):
        got = ops.svd(Wd, sd, k=k)
        assert healthy(got[3]), (k, got[3])
        check_topk(gpu, Ws, got, k, R, S64, oracle=orc, full=full, tag=(shape, k))


# ---- 2e: a cut inside an exactly degenerate cluster ---------------------------------------------------------------------------------------
def test_topk_cut_inside_degenerate_cluster(gpu):
    """unscaled cluster8 at 1024^2 (clusters of 128 equal values): k = 460 and the slices 204, 307, 358, 409 cut inside a cluster, where no
    rank-r reconstruction is unique; sigma, residuals and Eckart-Young hold for any basis of the cluster"""
    infos = run_family(gpu, "cluster8", None, 1.0, 1024, 1024, 404, [sweep_ranks(1024, 1024)], True, ("cluster8", None))
    assert all(healthy(i) for i in infos), infos


# ---- 2f: dominant directions that start behind the leading panels -------------------------------------------------------------------------
def late_dominant(n=1024, n_par=300, seed=47):
    """n x n: n - n_par Gaussian columns of norm ~1 in random directions, then n_par columns of norm 0.3 along two random directions (mixed
    1 : 0.6) with 1e-2 relative noise.  Together the small columns make sigma_1 ~ 4.5 and sigma_2 ~ 2.7 above the bulk (edge ~ 1.8), but
    they sit LAST: behind the leading panels in the norm-sorted order of the reduction, and by position on the direct path (which does not sort)."""
    g = torch.Generator().manual_seed(seed)
    W = torch.empty(n, n, dtype=torch.float64)
    W[:, :n - n_par] = torch.randn(n, n - n_par, generator=g, dtype=torch.float64) / n ** 0.5
    d = torch.linalg.qr(torch.randn(n, 2, generator=g, dtype=torch.float64))[0]
    c = torch.randn(n_par, 2, generator=g, dtype=torch.float64) * torch.tensor([1.0, 0.6], dtype=torch.float64)
    P = d @ c.T
    P = 0.3 * P / P.norm(dim=0, keepdim=True)
    W[:, n - n_par:] = P + 0.3e-2 * torch.randn(n, n_par, generator=g, dtype=torch.float64) / n ** 0.5
    return W.float()


@pytest.mark.parametrize("direct", [False, True])
def test_topk_dominant_directions_start_in_the_tail(gpu, monkeypatch, direct):
    from asvd4llm_amd import ops
    W = late_dominant()
    if direct:
        monkeypatch.setenv("ASVD_NO_REDUCE", "1")
    S64, orc = reference(gpu, W, True)
    assert S64[1] > 1.3 * S64[2] and S64[2] < 2.0, S64[:4]   # the construction: two values clearly above the bulk
    Wd = W.to(gpu)
    full = ops.svd(Wd)
    for k in (32, 64):
        got = ops.svd(Wd, k=k)
        for i in (full[3], got[3]):
            assert i.status == 0 and not i.plain_retry and not i.reduce_fallback, i
            assert i.reduced == (not direct), i
        check_topk(gpu, W, got, k, [2], S64, oracle=orc, full=full, tag=("late", direct, k))


# ---- 3: the fallback paths, which run the whole batch ---------------------------------------------------------------------------------------
def exact_low_rank(m, n, rank, seed):
    """fp32 [m, n] of EXACT rank `rank`: a product of small integer matrices (every sum exact in fp32), scaled by a power of two"""
    g = torch.Generator().manual_seed(seed)
    A = torch.randint(-2, 3, (m, rank), generator=g, dtype=torch.float64)
    B = torch.randint(-2, 3, (rank, n), generator=g, dtype=torch.float64)
    return ((A @ B) * 2.0 ** -9).float()


@pytest.mark.timeout(1200)
@pytest.mark.parametrize("shape", [(4096, 4096), (4096, 11008)])
def test_topk_rank_deficient_neighbour_runs_the_direct_path(gpu, shape):
    """[llm_like, exactly rank-1024 product] below the split threshold: the Cholesky of the second breaks down and the WHOLE call runs the direct
    path (which does not sort its columns) at the sweep's k; both problems must still meet the contract (unit scale on the product: exact rank)"""
    from asvd4llm_amd import ops
    m, n = shape
    k, R = sweep_ranks(m, n)
    W0, s0 = llm_like(m, n, seed=51)
    W1, s1 = exact_low_rank(m, n, 1024, seed=52), torch.ones(n, dtype=s0.dtype)
    md, sdv = [W0.to(gpu), W1.to(gpu)], [s0.to(gpu), s1.to(gpu)]
    U, S, V, infos = ops.svd_batched(md, sdv, k=k)
    Uf, Sf, Vf, infos_f = ops.svd_batched(md, sdv)
    for i in infos + infos_f:
        assert i.status == 0 and i.reduce_fallback and not i.reduced and not i.split, i
    for b, (W, s) in enumerate(((W0, s0), (W1, s1))):
        Ws = O.scaled_weight(W, s)
        S64, _ = reference(gpu, Ws, False)
        check_topk(gpu, Ws, (U[b], S[b], V[b], infos[b]), k, R, S64, full=(Uf[b], Sf[b], Vf[b], infos_f[b]),
                   exact_rank=(1024 if b else None), tag=(shape, b))


@pytest.mark.timeout(900)
def test_topk_nan_and_inf_neighbours(gpu):
    """[healthy, NaN in W, Inf in W, healthy] at 2048^2, k = 921: the bad problems report ASVD_N_NAN, the healthy ones meet the contract on
    whatever path the batch took.  Observed on an MI355X: GRAM_RETRY | REDUCE_FALLBACK | PLAIN_RETRY (the int8 and the fp64 Cholesky both
    break down on the non-finite Gram matrices, and the direct path's split-fp16 sweeps turn the bad problems NaN)."""
    from asvd4llm_amd import ops
    k, R = sweep_ranks(2048, 2048)
    pairs = [llm_like(2048, 2048, seed=70 + b) for b in range(4)]
    pairs[1][0][100, 200] = float("nan")
    pairs[2][0][1500, 7] = float("inf")
    md, sdv = [W.to(gpu) for W, _ in pairs], [s.to(gpu) for _, s in pairs]
    U, S, V, infos = ops.svd_batched(md, sdv, k=k)
    Uf, Sf, Vf, infos_f = ops.svd_batched(md, sdv)
    assert [i.status for i in infos] == [0, 2, 2, 0] and [i.status for i in infos_f] == [0, 2, 2, 0], infos
    assert infos[0].reduce_fallback, infos[0]
    for b in (0, 3):
        Ws = O.scaled_weight(*pairs[b])
        S64, orc = reference(gpu, Ws, True)
        check_topk(gpu, Ws, (U[b], S[b], V[b], infos[b]), k, R, S64, oracle=orc, full=(Uf[b], Sf[b], Vf[b], infos_f[b]), tag=("nan/inf", b))


@pytest.mark.parametrize("value", [float("inf"), float("nan")])
@pytest.mark.parametrize("shape", [(256, 192), (96, 64), (1024, 1024)])
def test_single_nonfinite_entry_reports_status(gpu, shape, value):
    """one Inf or NaN entry: ASVD_N_NAN on the reduced path (>= 128 columns) and on the small direct path (< 128 columns).  A NaN column once
    passed as a zero column through the retry of the reduction with the fp64 Gram matrix (its norm was taken as 0): status 0, finite factors."""
    from asvd4llm_amd import ops
    W, s = llm_like(*shape, seed=53)
    W[shape[0] // 3, shape[1] // 2] = value
    _, _, _, info = ops.svd(W.to(gpu), s.to(gpu), k=sweep_ranks(*shape)[0])
    assert info.status == 2, info


def test_prefactorize_with_nan_and_rank_deficient_layers(gpu, monkeypatch):
    """4 same-shape fp16 Linears at 1024^2 in ONE prefactorize chunk at the sweep's rank hint: two healthy, one with a NaN weight, one exactly
    rank-deficient (so the whole chunk runs the direct path).  The finite layers are cached and every ratio of the sweep is a slice that meets
    the oracle's reconstruction; the NaN layer is not cached, falls back as the reference does, and raises in strict mode."""
    from asvd4llm_amd import ops, sensitivity
    from asvd4llm_amd.modules.svd_linear import SVDLinear
    torch.manual_seed(0)
    weights = [llm_like(1024, 1024, seed=80 + i)[0] for i in range(4)]
    weights[2][17, 33] = float("nan")
    weights[3] = exact_low_rank(1024, 1024, 256, seed=84)   # integers x 2^-9: exact in fp16, and so is every product with an fp16 scale
    lins = []
    for i, W in enumerate(weights):
        lin = nn.Linear(1024, 1024, bias=False).half().to(gpu)
        lin.weight.data.copy_(W.half())
        lin.scaling_diag_matrix = F.make_stat("abs_mean", 1024, seed=90 + i).to(gpu)
        lins.append(lin)
    ratios = sensitivity._ppl_candidates(SimpleNamespace(compress_kv_cache=False))
    for lin in lins:
        lin._asvd_rank_hint = max(SVDLinear.compute_rank(lin, r) for r in ratios)
    calls = []
    real = ops.svd_batched

    def counting(mats, *a, **kw):
        calls.append(len(mats))
        return real(mats, *a, **kw)

    monkeypatch.setattr(ops, "svd_batched", counting)
    SVDLinear.prefactorize(lins, act_aware=True, alpha=0.5, ranks={l: l._asvd_rank_hint for l in lins})
    assert calls == [4], calls
    for i, lin in enumerate(lins):
        if i == 2:
            assert getattr(lin, "_asvd_factor_cache", None) is None
            continue
        info = lin._asvd_svd_info
        assert info.status == 0 and info.reduce_fallback, info
        for ratio in ratios:
            m = SVDLinear.from_linear(lin, ratio, act_aware=True, alpha=0.5)
            assert isinstance(m, SVDLinear), (i, ratio)
            o = O.from_linear_oracle(lin.weight.data.cpu(), lin.scaling_diag_matrix.cpu(), ratio, alpha=0.5, act_aware=True)
            e_live, e_scaled = O.recon_parity(m.ALinear.weight.data, m.BLinear.weight.data, o["A"], o["B"], lin.weight.data.cpu(), o["s"])
            assert e_live <= 3e-3 and e_scaled <= 3e-3, (i, ratio, e_live, e_scaled)
    assert calls == [4], calls   # every ratio was a slice of the cached factors: no re-factorisation
    bad = lins[2]
    with pytest.raises(FloatingPointError):
        SVDLinear.from_linear(bad, 0.9, act_aware=True, alpha=0.5)
    monkeypatch.setenv("ASVD_STRICT", "0")
    fb = SVDLinear.from_linear(bad, 0.9, act_aware=True, alpha=0.5)
    assert type(fb) is nn.Linear   # svd_linear.py:68,84-98 of the reference: a freshly initialised Linear
    assert getattr(bad, "_asvd_factor_cache", None) is None
