"""The clip search of the RTN quantizer, host side (no GPU): the numpy restatement (tests/mse_restate.py) against the reference's own choices
(tests/golden/rtn_mse_ref.npz, written by tools/make_golden_rtn_mse.py), the command-line flag, and the argument checks of the C entry."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import mse_restate as M
from tests.conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "rtn_mse_ref.npz")


def load_fixture():
    """[(case, dtype name, bits, group, x float32, out float32, scale, zero)]"""
    z = np.load(GOLDEN)

    def f32(a, dname):
        if dname == "bf16":
            return (a.astype(np.uint32) << 16).view(np.float32)
        return a.astype(np.float32)

    res = []
    for entry in z["cases"]:
        case, dname, bits, G, xkey = str(entry).split(":")
        res.append((case, dname, int(bits), int(G), f32(z[xkey], dname), f32(z[case + "_out"], dname), z[case + "_scale"], z[case + "_zero"]))
    return res


FIXTURE = load_fixture()
DT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}


def test_the_fixture_holds_the_cases_of_the_issue():
    have = {(c.split("_")[0], d, b, G) for c, d, b, G, *_ in FIXTURE}
    assert have == {("edge", d, b, G) for d in DT for b in (3, 4, 8) for G in (0, 128, 64)} | {("graded", "f16", b, G) for b in (3, 4, 8) for G in (0, 128, 64)}
    for case, dname, bits, G, x, out, scale, zero in FIXTURE:
        ng = len(M.slices(x.shape[1], G))
        assert scale.dtype == zero.dtype == np.float32 and scale.size == zero.size == x.shape[0] * ng and out.shape == x.shape, case
        assert ng > 1 or not G, case    # the grouped cases really have several groups, a ragged one among them
        assert not G or x.shape[1] % G, case


@pytest.mark.parametrize("case", FIXTURE, ids=[c[0] for c in FIXTURE])
def test_the_references_pair_is_a_restated_candidate_and_the_fp64_argmin(case):
    name, dname, bits, G, x, out, scale, zero = case
    worst = M.check_choice(x, bits, G, scale, zero, exact=True)
    assert worst == 0.0
    # ... and its output is the final pass with that pair, rounded once to the dtype
    w = torch.from_numpy(x).to(DT[dname])
    r_out, _ = M.final_restate(w, bits, G, torch.from_numpy(scale), torch.from_numpy(zero))
    assert np.all(M.same_f32(r_out.float().numpy(), out))


def test_the_search_changes_pairs_and_lowers_the_error():
    """the fixture is no restatement of plain RTN: on the graded matrix at 4 bits most rows leave their base pair, and the error falls as the issue
    measured it (relative Frobenius error with the search 0.874-0.880 of the error without, per row)"""
    name, dname, bits, G, x, out, scale, zero = next(c for c in FIXTURE if c[0] == "graded_f16_int4_g0")
    _, _, bscale, bzero = M.base_pair(x, 4)
    assert np.mean(M.bits_of(scale) != M.bits_of(bscale)) > 0.9
    plain, _ = M.quant_f32(x, bscale, bzero, 4)
    plain = torch.from_numpy(plain).half().double().numpy()
    ratio = np.linalg.norm(out.astype(np.float64) - x) / np.linalg.norm(plain - x)
    assert 0.86 <= ratio <= 0.89, ratio


def test_restated_search_on_edge_units():
    x = np.zeros((4, 48), dtype=np.float32)
    x[1, :] = np.linspace(-1, 2, 48)
    x[1, 5] = np.nan
    x[2, :] = np.linspace(-1, 2, 48)
    x[2, 7] = np.inf
    x[3, :] = np.linspace(-1, 2, 48)
    out, q, scale, zero, ready = M.mse_restate_f32(x, 4)
    _, _, bscale, bzero = M.base_pair(x, 4)
    assert ready and np.array_equal(M.bits_of(scale[:3]), M.bits_of(bscale[:3])) and np.array_equal(M.bits_of(zero[:3]), M.bits_of(bzero[:3]))
    assert scale[0] == np.float32(2) / np.float32(15) and np.all(out[0] == 0)      # all zero: every error ties at 0, index 0 wins
    assert scale[3] <= bscale[3] and M.check_choice(x, 4, 0, scale, zero, exact=True) == 0.0
    assert M.n_candidates() == 80 and M.n_candidates(50, 0.5) == 25 and M.n_candidates(100, 0.7) == 70
    s1, z1 = M.candidate_pairs(*M.base_pair(x, 4)[:2], 4)
    assert np.array_equal(M.bits_of(s1[0]), M.bits_of(bscale)) and np.array_equal(M.bits_of(z1[0]), M.bits_of(bzero))   # candidate 0 is the base pair


# ---- the command line -----------------------------------------------------------------------------------------------------------------

def _args(*extra):
    import asvd
    return asvd.build_parser().parse_args(["--model_id", "tiny-llama", "--random_init", *extra])


@pytest.mark.parametrize("wq", ["rtn_int8", "rtn_int6", "rtn_int4"])
@pytest.mark.parametrize("storage,group", [("fake", 0), ("packed", 64), ("bitpacked", 128)])
def test_flag_is_valid_with_every_rtn_width_storage_and_group(wq, storage, group):
    import asvd
    args = _args("--weight_quant", wq, "--weight_quant_storage", storage, "--weight_quant_group_size", str(group), "--weight_quant_mse")
    assert args.weight_quant_mse is True
    asvd.check_weight_quant_args(args)


def test_flag_is_off_by_default_and_an_error_without_rtn():
    import asvd
    assert _args("--weight_quant", "rtn_int4").weight_quant_mse is False
    asvd.check_weight_quant_args(_args())
    asvd.check_weight_quant_args(_args("--weight_quant", "awq_int4"))      # without the flag: refused later, by run_weight_quant, as before
    for bad in ([], ["--weight_quant", "none"], ["--weight_quant", "awq_int4"], ["--weight_quant", "awq_int8"]):
        args = _args(*bad, "--weight_quant_mse")
        with pytest.raises(ValueError, match="weight_quant_mse"):
            asvd.check_weight_quant_args(args)
        with pytest.raises(ValueError, match="weight_quant_mse"):
            asvd.main(args)                                                  # main refuses before it loads anything


def test_run_weight_quant_passes_the_keyword_only_when_set(monkeypatch):
    import asvd
    from asvd4llm_amd import quantization
    seen = []
    monkeypatch.setattr(quantization, "rtn_quant_sequential", lambda model, bits, **kw: seen.append(("fake", bits, kw)))
    monkeypatch.setattr(quantization, "rtn_pack_sequential", lambda model, bits, **kw: seen.append(("pack", bits, kw)))
    asvd.run_weight_quant(None, _args("--weight_quant", "rtn_int4", "--weight_quant_mse"))
    asvd.run_weight_quant(None, _args("--weight_quant", "rtn_int4"))
    asvd.run_weight_quant(None, _args("--weight_quant", "rtn_int4", "--weight_quant_storage", "bitpacked", "--weight_quant_group_size", "128", "--weight_quant_mse"))
    asvd.run_weight_quant(None, _args("--weight_quant", "rtn_int8", "--weight_quant_storage", "packed", "--weight_quant_mse"))
    assert seen == [("fake", 4, {"mse": True}), ("fake", 4, {}), ("pack", 4, {"storage": "bits", "group_size": 128, "mse": True}),
                    ("pack", 8, {"mse": True})]


# ---- the C entry and its wrapper ------------------------------------------------------------------------------------------------------------

def test_bad_search_parameters_are_rejected_without_a_device(built_lib):
    """asvd_rtn_quant_mse_batched checks norm, grid, maxshrink and the candidate count before anything else, so the refusal needs no device: the
    other arguments here are complete and would pass their own checks (the pointers are never followed on this path)"""
    lib = built_lib
    buf = (ctypes.c_float * 64)()
    flags = (ctypes.c_int * 1)()
    vp, i64 = ctypes.c_void_p * 1, ctypes.c_int64 * 1
    ptr = vp(ctypes.addressof(buf))

    def call(group, norm, grid, maxshrink):
        return lib.asvd_rtn_quant_mse_batched(1, ptr, (ctypes.c_int * 1)(0), i64(4), i64(16), i64(16), 4, ptr, i64(16), None, None, None,
                                              ctypes.cast(flags, ctypes.c_void_p), None, group, norm, grid, maxshrink)

    nan, inf = float("nan"), float("inf")
    for group, norm, grid, maxshrink in [(0, 0.0, 100, 0.8), (0, -2.4, 100, 0.8), (0, nan, 100, 0.8), (0, inf, 100, 0.8), (0, 2.4, 0, 0.8),
                                         (0, 2.4, -5, 0.8), (0, 2.4, 100, 0.0), (0, 2.4, 100, -0.5), (0, 2.4, 100, 1.5), (0, 2.4, 100, nan),
                                         (0, 2.4, 1, 0.5),          # int(0.5 * 1) = 0 candidates
                                         (0, 2.4, 1000, 0.8),       # 800 candidates
                                         (0, 2.4, 257, 1.0),        # 257 candidates
                                         (32, 2.4, 100, 0.8), (256, 2.4, 100, 0.8), (-64, 2.4, 100, 0.8)]:
        assert call(group, norm, grid, maxshrink) == -1, (group, norm, grid, maxshrink)


def test_wrapper_checks_the_search_parameters():
    from asvd4llm_amd import ops
    assert ops._mse_params(2.4, 100, 0.8) == (2.4, 100, 0.8) and ops._mse_params(2, 256, 1) == (2.0, 256, 1.0)
    for norm, grid, maxshrink in [(0, 100, 0.8), (float("nan"), 100, 0.8), (float("inf"), 100, 0.8), (2.4, 0, 0.8), (2.4, 10.5, 0.8),
                                  (2.4, 100, 0), (2.4, 100, 1.01), (2.4, 1, 0.5), (2.4, 1000, 0.8)]:
        with pytest.raises(ValueError, match="mse_"):
            ops._mse_params(norm, grid, maxshrink)
