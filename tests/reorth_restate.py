"""Restatement of the re-orthonormalisation pass of asvd_reorth_batched (include/asvd_hip.h, K18) in torch: E in fp64, Q stored in fp32.

    E = Q^T Q - I,   T = striu(E) + diag(E) / 2,   Q <- Q - Q T       until max |E| <= tol

and the inputs the tests share: Q0 = Haar(m, k) (I + eps triu(randn)), built in fp64 and rounded to fp32."""
import functools
import math

import torch

from tests.families import haar

OK, N_NOCONV, N_NAN = 0, 1, 2
MAX_PASSES, TOL, REFUSE = 8, 2e-6, 0.25

# (m, k, ldq): k = 1, k and m that are no multiples of 32, a padded leading dimension, one / several / many 32-column blocks, more than one row tile
SHAPES = [(64, 1, 1), (96, 33, 33), (160, 96, 96), (300, 130, 136), (1030, 257, 257), (2048, 512, 512)]
EPSILONS = [0.0, 1e-4, 1e-2]
PASS_BOUND = {0.0: 0, 1e-4: 2, 1e-2: 4}  # what the CPU simulation of the issue showed


@functools.lru_cache(maxsize=None)
def make_input(m, k, eps, seed=0):
    """fp32 [m, k]; computed once per (m, k, eps, seed) and shared: callers clone before they write"""
    g = torch.Generator().manual_seed(1000 * seed + 17)
    H = haar(m, k, g)
    N = torch.triu(torch.randn(k, k, generator=g, dtype=torch.float64))
    return (H @ (torch.eye(k, dtype=torch.float64) + eps * N)).float()


def defect(Q):
    """max |Q^T Q - I| in fp64 (on whatever device Q lives)"""
    Qd = Q.double()
    return (Qd.T @ Qd - torch.eye(Q.shape[1], dtype=torch.float64, device=Q.device)).abs().max().item()


def restate(Q0, max_passes=MAX_PASSES, tol=TOL):
    """(Q fp32, status, passes, e_before, e_after) with the refusals of the entry point: non-finite entry defect -> N_NAN, > 0.25 -> N_NOCONV,
    both with Q untouched; >= 1 or non-finite inside the loop, or max_passes reached above tol -> N_NOCONV"""
    Q = Q0.clone()
    k = Q.shape[1]
    eye = torch.eye(k, dtype=torch.float64, device=Q.device)
    e0 = e = defect(Q)
    if not math.isfinite(e0):
        return Q, N_NAN, 0, e0, e0
    if e0 > REFUSE:
        return Q, N_NOCONV, 0, e0, e0
    passes = 0
    while e > tol:
        if passes >= max_passes:
            return Q, N_NOCONV, passes, e0, e
        Qd = Q.double()
        E = Qd.T @ Qd - eye
        T = torch.triu(E, 1) + 0.5 * torch.diag(torch.diagonal(E))
        Q = (Qd - Qd @ T).float()
        passes += 1
        e = defect(Q)
        if not math.isfinite(e) or e >= 1.0:
            return Q, N_NOCONV, passes, e0, e
    return Q, OK, passes, e0, e


@functools.lru_cache(maxsize=None)
def restated(m, k, eps, seed=0):
    return restate(make_input(m, k, eps, seed))


def cholesky_qr(Q0):
    """the fp64 Cholesky-QR factor of Q0: Q0 R^-1 with R^T R = Q0^T Q0, R upper triangular with positive diagonal — the limit of the passes"""
    Qd = Q0.double()
    R = torch.linalg.cholesky(Qd.T @ Qd).T
    return torch.linalg.solve_triangular(R, Qd, upper=True, left=False)
