"""K18 on the device: asvd_reorth_batched alone (shapes, perturbations, refusals), through ops.svd(..., ortho=True) on the graded families, and
through SVDLinear.  Checker arithmetic is fp64 torch on the device; the inputs and the restatement come from tests/reorth_restate.py."""
import math

import pytest
import torch

from oracle import asvd_oracle as O
from tests import reorth_restate as R
from tests.test_gpu_families import family_case, retained_rank
from tests.test_gpu_svd import REC_TOL

pytestmark = pytest.mark.gpu
SENTINEL = 7.25


def _padded(Q0s, ldq, gpu):
    """device copies of the inputs inside [m, ldq] buffers whose padding columns hold a sentinel; returns (buffers, views [m, k])"""
    bufs, views = [], []
    for Q0 in Q0s:
        m, k = Q0.shape
        buf = torch.full((m, ldq), SENTINEL, dtype=torch.float32, device=gpu)
        buf[:, :k] = Q0.to(gpu)
        bufs.append(buf)
        views.append(buf[:, :k])
    return bufs, views


def _lower(Q, Q0):
    """|tril(Q^T Q0, -1)| and the smallest diagonal entry: R = Q^T Q0 upper triangular with a positive diagonal <=> order and nested spans kept"""
    Rm = Q.double().T @ Q0.double()
    return torch.tril(Rm, -1).abs().max().item() if Rm.shape[0] > 1 else 0.0, torch.diagonal(Rm).min().item()


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("eps", R.EPSILONS)
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_shapes_and_perturbations(gpu, shape, eps, batch):
    from asvd4llm_amd import ops
    m, k, ldq = shape
    Q0s = [R.make_input(m, k, eps, seed) for seed in range(batch)]
    bufs, Qs = _padded(Q0s, ldq, gpu)
    infos = ops.reorth_batched(Qs)
    bufs2, Qs2 = _padded(Q0s, ldq, gpu)
    infos2 = ops.reorth_batched(Qs2)
    for b in range(batch):
        Q0, Q, info = Q0s[b].to(gpu), Qs[b], infos[b]
        ref_passes = R.restated(m, k, eps, b)[2]
        d_before, d_after = R.defect(Q0), R.defect(Q)
        low, dmin = _lower(Q, Q0)
        dist = (Q.double() - R.cholesky_qr(Q0)).abs().max().item()
        print(f"{m}x{k} ld {ldq} eps {eps} [{b}/{batch}]: {info}  fp64 defect {d_before:.3g} -> {d_after:.3g}  passes {info.passes} (restatement "
              f"{ref_passes})  |tril(R,-1)| {low:.3g}  distance from the fp64 Cholesky-QR factor {dist:.3g}")
        assert info.status == 0, info
        assert d_after <= 1e-5
        assert low <= 1e-5 and dmin > 0.0
        assert info.e_after <= R.TOL
        assert abs(info.e_before - d_before) <= 1e-6 and abs(info.e_after - d_after) <= 1e-6
        if eps == 0.0:
            assert info.passes == 0 and torch.equal(Q, Q0)
        else:
            assert 1 <= info.passes <= ref_passes + 1
        if ldq > k:
            assert bool((bufs[b][:, k:] == SENTINEL).all())
        assert torch.equal(bufs[b], bufs2[b]) and (info.passes, info.e_before, info.e_after) == (infos2[b].passes, infos2[b].e_before, infos2[b].e_after)


def test_more_rows_than_one_exact_segment(gpu):
    """m = 32768 + 64: the int32 accumulators of the digit products are exact for 32768 rows, so the Gram pass runs two row segments and adds
    them (another path of the E kernel); the bars are those of the shapes above"""
    from asvd4llm_amd import ops
    m, k, eps = 32768 + 64, 33, 1e-4
    Q0 = R.make_input(m, k, eps).to(gpu)
    Q = Q0.clone()
    info = ops.reorth(Q)
    d_before, d_after = R.defect(Q0), R.defect(Q)
    low, dmin = _lower(Q, Q0)
    print(f"{m}x{k} eps {eps}: {info}  fp64 defect {d_before:.3g} -> {d_after:.3g}  (restatement {R.restated(m, k, eps)[2]} passes)  |tril(R,-1)| {low:.3g}")
    assert info.status == 0 and d_after <= 1e-5 and low <= 1e-5 and dmin > 0.0 and info.e_after <= R.TOL
    assert abs(info.e_before - d_before) <= 1e-6 and abs(info.e_after - d_after) <= 1e-6
    assert 1 <= info.passes <= R.restated(m, k, eps)[2] + 1


def _bad_problem(kind):
    if kind == "zero_column":
        Z = R.make_input(160, 96, 0.0, 5).clone()
        Z[:, 40] = 0.0
        return Z, R.N_NOCONV
    if kind == "nan_entry":
        Z = R.make_input(160, 96, 0.0, 5).clone()
        Z[3, 5] = float("nan")
        return Z, R.N_NAN
    return R.make_input(160, 96, 0.1), R.N_NOCONV   # entry max |E| > 0.25 (held by tests/test_reorth_host.py on the restatement)


@pytest.mark.parametrize("kind", ["zero_column", "nan_entry", "eps_0.1"])
def test_refusals_leave_the_problem_untouched_and_the_others_alone(gpu, kind):
    from asvd4llm_amd import ops
    bad0, want = _bad_problem(kind)
    bad = bad0.to(gpu).clone()
    info = ops.reorth(bad)
    print(kind, info)
    assert info.status == want and info.status > 0 and info.passes == 0
    assert torch.equal(bad.view(torch.int32), bad0.to(gpu).view(torch.int32))   # bit patterns: NaN != NaN
    if kind == "eps_0.1":
        assert info.e_before > R.REFUSE
    # in the middle of a batch: the two good problems get the bits of a batch without it
    good = [R.make_input(160, 96, 1e-2, 0), R.make_input(160, 96, 1e-4, 1)]
    three = [good[0].to(gpu).clone(), bad0.to(gpu).clone(), good[1].to(gpu).clone()]
    two = [good[0].to(gpu).clone(), good[1].to(gpu).clone()]
    i3, i2 = ops.reorth_batched(three), ops.reorth_batched(two)
    assert (i3[0].status, i3[1].status, i3[2].status) == (0, want, 0) and i3[1].passes == 0
    assert torch.equal(three[1].view(torch.int32), bad0.to(gpu).view(torch.int32))
    assert torch.equal(three[0], two[0]) and torch.equal(three[2], two[1])
    assert (i3[0].passes, i3[2].passes) == (i2[0].passes, i2[1].passes) and i3[0].passes >= 1


def _lower_of_change_of_basis(Q, Q0):
    """The same property for a Q that is NOT yet orthonormal.  Every pass is Q <- Q U with U upper triangular, so Q0 = Q M with M upper triangular
    and a positive diagonal; M = (Q^T Q)^-1 Q^T Q0.  R = Q^T Q0 = (Q^T Q) M is M only when Q^T Q = I: after one pass of an eps = 1e-2 input
    Q^T Q - I is still 1.4e-2 and tril(R, -1) holds entries of that size whatever the kernel does (measured on MI355X: 3.4e-3), so the
    stopped-early case is checked on M, which reduces to R for the converged cases above."""
    Qd, Q0d = Q.double(), Q0.double()
    M = torch.linalg.solve(Qd.T @ Qd, Qd.T @ Q0d)
    return torch.tril(M, -1).abs().max().item(), torch.diagonal(M).min().item()


def test_max_passes_is_a_hard_stop(gpu):
    from asvd4llm_amd import ops
    Q0 = R.make_input(160, 96, 1e-2).to(gpu)
    Q = Q0.clone()
    info = ops.reorth(Q, max_passes=1)
    print(info)
    assert info.status == R.N_NOCONV and info.passes == 1
    assert abs(info.e_after - R.defect(Q)) <= 1e-6 and info.e_after > R.TOL
    low, dmin = _lower_of_change_of_basis(Q, Q0)
    print(f"|tril(M, -1)| {low:.3g}, min diag {dmin:.3g}; |tril(Q^T Q0, -1)| {_lower(Q, Q0)[0]:.3g}")
    assert low <= 1e-5 and dmin > 0.0


# ---- through the SVD ------------------------------------------------------------------------------------------------------------------
SVD_CASES = [(kind, m, n, None) for kind in ("geo3", "pow1") for (m, n) in ((1024, 1024), (1376, 512), (512, 1376))] + [("lowrank_noise", 1024, 1024, "r")]


@pytest.mark.parametrize("kind,m,n,kmode", SVD_CASES, ids=lambda v: str(v))
def test_svd_ortho_on_graded_families(gpu, kind, m, n, kmode):
    from asvd4llm_amd import ops
    W, s = family_case(kind, "abs_max", 1.0, m, n, seed=3)
    r = retained_rank(m, n)
    k = r if kmode == "r" else min(m, n)
    Wg, sg = W.to(gpu), s.to(gpu)
    U0, S0, V0, info0 = ops.svd(Wg, sg, k=k)
    U, S, V, info = ops.svd(Wg, sg, k=k, ortho=True)
    assert info0.reorth is None and info0.status == 0 and info.status == 0
    assert info.reorth is not None and info.reorth.status == 0, info.reorth
    long_is_u = m >= n
    short, short0, long_, long0 = (V, V0, U, U0) if long_is_u else (U, U0, V, V0)
    assert torch.equal(S, S0) and torch.equal(short, short0)
    d_plain, d_fixed = R.defect(long0), R.defect(long_)
    print(f"{kind} {m}x{n} k {k}: long-side |Q^T Q - I| plain {d_plain:.3g} -> repaired {d_fixed:.3g}  {info.reorth}")
    assert d_fixed <= 1e-5
    Wsd = O.scaled_weight(W, s).to(gpu).double()
    Ud, Sd, Vd = U.double(), S.double(), V.double()
    res = (Wsd @ Vd - Ud * Sd) if long_is_u else (Wsd.T @ Ud - Vd * Sd)
    res_long = (res.norm(dim=0) / Sd[0]).max().item()
    print(f"    long-side triplet residual / sigma_1: {res_long:.3g}")
    assert res_long <= 2e-5
    S64 = torch.linalg.svdvals(Wsd)
    Rg = (Ud[:, :r] * Sd[:r]) @ Vd[:, :r].T
    err2, tot2, tail2 = ((Wsd - Rg) ** 2).sum().item(), (S64 ** 2).sum().item(), (S64[r:] ** 2).sum().item()
    assert abs(err2 - tail2) <= (REC_TOL ** 2) * tot2, (err2, tail2, tot2)


# ---- through the modules --------------------------------------------------------------------------------------------------------------
def _graded_linear(gpu, dtype):
    from tests import families as F
    W = F.make_weight("geo3", 192, 320, seed=11)   # out 192 < in 320: V is the long side, and BLinear.weight = V^T under sigma_fuse="U"
    lin = torch.nn.Linear(320, 192, bias=False)
    lin.weight.data = W.clone()
    return lin.to(dtype).to(gpu)


def test_module_sigma_fuse_u_emits_an_orthonormal_factor(gpu, monkeypatch):
    from asvd4llm_amd.modules.svd_linear import SVDLinear
    monkeypatch.delenv("ASVD_SVD_ORTHO", raising=False)
    lin = _graded_linear(gpu, torch.float16)
    mod = SVDLinear.from_linear(lin, 0.9, sigma_fuse="U", ortho=True)
    assert lin._asvd_svd_info.reorth is not None and lin._asvd_svd_info.reorth.status == 0
    B = mod.BLinear.weight.data
    assert B.dtype == torch.float16
    g = (B.double() @ B.double().T - torch.eye(B.shape[0], dtype=torch.float64, device=gpu)).abs().max().item()
    print("fp16 BLinear.weight: |B B^T - I| =", g)
    # rows of unit norm whose entries are each rounded to fp16 (2^-11 relative): |sum_k (b_ik b_jk)(1 + d)(1 + d') - delta_ij| <= 2 x 2^-11 by
    # Cauchy-Schwarz, on top of the fp32 factor's 1e-5
    assert g <= 2 * 2.0 ** -11 + 1e-5
    # the environment switch gives the bits of the keyword (the cache is dropped: a cached factorisation would make this vacuous)
    SVDLinear.drop_factor_cache(lin)
    monkeypatch.setenv("ASVD_SVD_ORTHO", "1")
    mod_env = SVDLinear.from_linear(lin, 0.9, sigma_fuse="U")
    assert lin._asvd_svd_info.reorth is not None
    assert torch.equal(mod_env.BLinear.weight.data, B) and torch.equal(mod_env.ALinear.weight.data, mod.ALinear.weight.data)
    # and the two kinds of cached factors never mix
    monkeypatch.delenv("ASVD_SVD_ORTHO")
    SVDLinear.from_linear(lin, 0.9, sigma_fuse="U")
    assert lin._asvd_svd_info.reorth is None


def test_module_sigma_fuse_uv_reconstructs_like_the_plain_call(gpu, monkeypatch):
    from asvd4llm_amd.modules.svd_linear import SVDLinear
    monkeypatch.delenv("ASVD_SVD_ORTHO", raising=False)
    lin = _graded_linear(gpu, torch.float32)
    Wd = lin.weight.data.double()
    r = SVDLinear.compute_rank(lin, 0.9)
    S64 = torch.linalg.svdvals(Wd)
    tail = math.sqrt((S64[r:] ** 2).sum().item() / (S64 ** 2).sum().item())
    for ortho in (False, True):
        SVDLinear.drop_factor_cache(lin)
        mod = SVDLinear.from_linear(lin, 0.9, sigma_fuse="UV", ortho=ortho)
        rel = ((mod.ALinear.weight.data.double() @ mod.BLinear.weight.data.double() - Wd).norm() / Wd.norm()).item()
        print(f"ortho={ortho}: |W - A B| / |W| = {rel:.6g} (discarded spectrum {tail:.6g})")
        assert abs(rel - tail) <= REC_TOL   # the project's reconstruction bar, for both calls
