"""K18 (asvd_reorth_batched) without a device: exported symbols, size query and argument validation, the CLI flag, the factor-cache key, and
the restatement of the pass (tests/reorth_restate.py) held to the pass counts of the CPU simulation before any kernel is compared with it."""
import ctypes
import types

import pytest
import torch

from tests import reorth_restate as R


def test_symbols_exported(built_lib):
    from asvd4llm_amd import _lib
    for name in ("asvd_reorth_worksize", "asvd_reorth_batched"):
        assert hasattr(built_lib, name) and name in _lib.SIGNATURES


def test_worksize(built_lib):
    nb = ctypes.c_size_t()
    assert built_lib.asvd_reorth_worksize(1, 4096, 4096, ctypes.byref(nb)) == 0 and nb.value > 0
    # one problem: 48 MiB of digit planes + 64 MiB of T; a batch of 32 runs in sub-batches of at most 1 GiB (include/asvd_hip.h)
    assert 112 * 2**20 <= nb.value <= 113 * 2**20
    nb32 = ctypes.c_size_t()
    assert built_lib.asvd_reorth_worksize(32, 4096, 4096, ctypes.byref(nb32)) == 0 and nb.value < nb32.value <= 2**30 + 2**20
    assert built_lib.asvd_reorth_worksize(0, 4096, 4096, ctypes.byref(nb)) == -1
    assert built_lib.asvd_reorth_worksize(1, 8, 9, ctypes.byref(nb)) == -1
    assert built_lib.asvd_reorth_worksize(1, 8, 0, ctypes.byref(nb)) == -1
    assert built_lib.asvd_reorth_worksize(1, 4096, 4096, None) == -1


def test_bad_arguments_need_no_device(built_lib):
    """every one of these returns ASVD_E_BADARG before the first device call: the pointers are never dereferenced"""
    arr = (ctypes.c_void_p * 1)(0x1000)
    work = ctypes.c_void_p(0x1000)
    big = 1 << 40

    def call(batch, q, m, k, ldq, w=work, wb=big):
        return built_lib.asvd_reorth_batched(batch, q, m, k, ldq, 0, 0.0, w, wb, None, None)

    assert call(1, None, 64, 8, 8) == -1
    assert call(1, arr, 64, 8, 8, w=None) == -1
    assert call(1, (ctypes.c_void_p * 1)(0), 64, 8, 8) == -1     # NULL entry
    assert call(0, arr, 64, 8, 8) == -1
    assert call(1, arr, 64, 0, 8) == -1
    assert call(1, arr, 8, 9, 9) == -1                            # m < k
    assert call(1, arr, 64, 8, 7) == -1                           # ldq < k
    assert call(1, (ctypes.c_void_p * 1)(0x1002), 64, 8, 8) == -1  # misaligned Q
    assert call(1, arr, 64, 8, 8, wb=16) == -2                    # short workspace: ASVD_E_WORKSPACE, still no device call


def test_cli_flag():
    import asvd
    p = asvd.build_parser()
    assert p.parse_args([]).svd_ortho is False
    assert p.parse_args(["--svd_ortho"]).svd_ortho is True


def test_ortho_setting_resolution(monkeypatch):
    from asvd4llm_amd.modules import svd_linear as M
    monkeypatch.delenv("ASVD_SVD_ORTHO", raising=False)
    assert M._ortho(None) is False and M._ortho(True) is True and M._ortho(False) is False
    monkeypatch.setenv("ASVD_SVD_ORTHO", "1")
    assert M._ortho(None) is True and M._ortho(False) is False


def test_binary_search_and_sweep_read_the_flag_with_getattr():
    from asvd4llm_amd import sensitivity
    assert sensitivity._ortho_kw(types.SimpleNamespace()) == {}
    assert sensitivity._ortho_kw(types.SimpleNamespace(svd_ortho=False)) == {}
    assert sensitivity._ortho_kw(types.SimpleNamespace(svd_ortho=True)) == {"ortho": True}


class _OnDevice(torch.Tensor):
    """a CPU tensor that answers is_cuda like a device tensor: _cache_key refuses host weights before it builds the key"""
    is_cuda = property(lambda self: True)


def test_cache_key_differs_between_the_settings(monkeypatch):
    from asvd4llm_amd import ops
    from asvd4llm_amd.modules.svd_linear import SVDLinear
    monkeypatch.setattr(ops, "fro_norm_sq", lambda t: (t.float() ** 2).sum())   # the K8 kernel, restated for the host
    w = torch.randn(8, 6).as_subclass(_OnDevice)
    lin = types.SimpleNamespace(weight=types.SimpleNamespace(data=w, _version=0))
    k_off, _ = SVDLinear._cache_key(lin, False, 1)
    k_off2, _ = SVDLinear._cache_key(lin, False, 1, False)
    k_on, _ = SVDLinear._cache_key(lin, False, 1, True)
    assert k_off == k_off2 and k_off != k_on and k_off[:-1] == k_on[:-1]


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("eps", R.EPSILONS)
def test_restatement_meets_the_simulated_pass_counts(shape, eps):
    m, k, _ = shape
    for seed in range(3):   # the three problems of the GPU tests' batches
        Q0 = R.make_input(m, k, eps, seed)
        Q, status, passes, e0, e1 = R.restated(m, k, eps, seed)
        print(f"{m}x{k} eps {eps} seed {seed}: entry {e0:.3g} passes {passes} exit {e1:.3g}")
        assert status == R.OK and e1 <= R.TOL
        assert passes <= R.PASS_BOUND[eps]
        if eps == 0.0:
            assert passes == 0 and torch.equal(Q, Q0)
        else:
            assert (Q.double() - R.cholesky_qr(Q0)).abs().max().item() <= 1e-6   # the limit is the Cholesky-QR factor


def test_restatement_refuses():
    Q0 = R.make_input(160, 96, 0.1)
    Q, status, passes, e0, _ = R.restate(Q0)
    assert e0 > R.REFUSE and status == R.N_NOCONV and passes == 0 and torch.equal(Q, Q0)
    Z = R.make_input(160, 96, 0.0).clone()
    Z[:, 40] = 0.0
    assert R.restate(Z)[1:3] == (R.N_NOCONV, 0)
    Z = R.make_input(160, 96, 0.0).clone()
    Z[3, 5] = float("nan")
    assert R.restate(Z)[1:3] == (R.N_NAN, 0)
    Q, status, passes, _, _ = R.restate(R.make_input(160, 96, 1e-2), max_passes=1)
    assert (status, passes) == (R.N_NOCONV, 1)
