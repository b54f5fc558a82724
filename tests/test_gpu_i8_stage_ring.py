"""The stage ring of the int8 tile loop (gi_tile_loop, csrc/i8_digits.h) at its edges: fewer stages than the ring has slots, exactly as many,
wrap-around, panels past the end of either operand (their loads are clamped to the last panel and their products dropped by the callers), both
block orders of the triangular grid, accumulation across launches and both weight counts.  Everything is integer arithmetic: the checks are
equalities against numpy int64 (through the Gram hook: the same 4e-16 of the fp64 combination that tests/test_gpu_gram_i8.py allows)."""
import ctypes

import numpy as np
import pytest
import torch

from tests.test_gpu_gram_i8 import _check_exact

pytestmark = pytest.mark.gpu


def _matrix(rows, cols, seed):
    """Gaussian columns; the LAST real panel holds the largest entries of the matrix, so that a clamped read of it that leaked into a stored
    entry would be the largest error it could make"""
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(rows, cols, generator=g)
    X[:, cols - 32:] *= 1000.0
    return X


# ---- through asvd_test_gram (five weights, the plane set on both sides, triangular grid) ----

@pytest.mark.parametrize("rows", [64, 128, 192, 256, 448])   # 1, 2, 3, 4 and 7 stages of 64 rows
def test_gram_stage_counts_with_clamped_panels(gpu, rows):
    """192 columns = 6 panels: the second block row and block column hold two real and two clamped panels; 3 blocks: the plain block order"""
    _check_exact(gpu, [_matrix(rows, 192, rows)])


def test_gram_one_block_half_clamped(gpu):
    """64 columns = 2 panels in one 128 x 128 block: half of both operands is clamped"""
    _check_exact(gpu, [_matrix(192, 64, 1)])


def test_gram_xcd_block_order(gpu):
    """2048 columns = 16 x 16 blocks, 136 in the upper triangle, a multiple of 8: the XCD-aware order"""
    _check_exact(gpu, [_matrix(128, 2048, 2)])


def test_gram_one_stage_launches_accumulate(gpu):
    """four launches of one stage each, added into G; two problems"""
    _check_exact(gpu, [_matrix(256, 192, 3), _matrix(256, 192, 4)], seg_rows=64)


# ---- through asvd_test_i8_tile (four or five weights, two different plane sets, rectangular grid) ----

def _planes(D, np_, kgs):
    """digits D [3][K = 16 kgs][32 np_] int8 (reduction index, column) -> planes [3][np_][kgs][32][16], the layout of csrc/i8_digits.h"""
    return np.ascontiguousarray(D.reshape(3, kgs, 16, np_, 32).transpose(0, 3, 1, 4, 2))


def _tile(gpu, DA, DB, kgs, nw):
    from asvd4llm_amd import _lib as L
    lib = L.load(True)
    npA, npB = DA.shape[2] // 32, DB.shape[2] // 32
    pa = torch.from_numpy(_planes(DA, npA, kgs)).to(gpu)
    pb = torch.from_numpy(_planes(DB, npB, kgs)).to(gpu)
    out = torch.full((nw, 32 * npA, 32 * npB), -1, dtype=torch.int32, device=gpu)
    rc = lib.asvd_test_i8_tile(ctypes.c_void_p(pa.data_ptr()), npA * kgs * 512, npA, ctypes.c_void_p(pb.data_ptr()), npB * kgs * 512, npB, kgs, nw,
                               ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _want(DA, DB, nw):
    A, B = DA.astype(np.int64), DB.astype(np.int64)
    want = np.zeros((nw, A.shape[2], B.shape[2]), np.int64)
    for a in range(3):
        for c in range(3):
            if a + c < nw:
                want[a + c] += A[a].T @ B[c]
    assert np.abs(want).max() < 2 ** 31
    return want


@pytest.mark.parametrize("nw", [4, 5])
@pytest.mark.parametrize("kgs", [4, 8, 12, 28])   # 1, 2, 3 and 7 stages
def test_tile_loop_two_plane_sets(gpu, nw, kgs):
    """5 panels against 3: two block rows (the second with one real panel), one block column with one clamped panel"""
    rng = np.random.default_rng(100 * nw + kgs)
    DA = rng.integers(-128, 128, size=(3, 16 * kgs, 160), dtype=np.int8)
    DB = rng.integers(-128, 128, size=(3, 16 * kgs, 96), dtype=np.int8)
    got = _tile(gpu, DA, DB, kgs, nw)
    assert np.array_equal(got.astype(np.int64), _want(DA, DB, nw))


def test_tile_loop_extreme_digits(gpu):
    """digits at +-127 / -128 over K = 448, all signs aligned in some entries: 3 x 128 x 128 x 448 = 2.2e7 per weight, far inside int32, and every
    partial sum is the largest the case can produce"""
    kgs, nw = 28, 5
    rng = np.random.default_rng(7)
    DA = np.where(rng.random((3, 16 * kgs, 160)) < 0.5, -128, 127).astype(np.int8)
    DB = np.where(rng.random((3, 16 * kgs, 96)) < 0.5, -128, 127).astype(np.int8)
    DA[:, :, 0] = -128
    DB[:, :, 0] = -128          # entry (0, 0): every product is 2^14
    DA[:, :, 159] = 127
    DB[:, :, 95] = -128         # last real column of either side: every product is -127 * 128
    got = _tile(gpu, DA, DB, kgs, nw)
    want = _want(DA, DB, nw)
    assert want[2, 0, 0] == 3 * 16384 * 16 * kgs
    assert np.array_equal(got.astype(np.int64), want)
