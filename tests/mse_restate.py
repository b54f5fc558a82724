"""CPU restatement of the clip search of the reference's Quantizer (quantization.py:94-111, mse=True; perchannel=True, sym=False, weight=True) in
numpy, written from the contract and checked against the reference's own choices (tests/golden/rtn_mse_ref.npz, tests/test_mse_host.py).
A unit is a row, or one group of a row.  The CANDIDATE pairs are restated op for op in fp32 and are compared bit for bit; the error of a candidate is
restated in fp64 (E64), which is the criterion the kernel's choice is judged by: the kernel may evaluate its sums faster, so its choice is required to
be a candidate and to be within a derived factor of the fp64 minimum, not to be the reference's bit for bit.  Test code only: the product path is
csrc/rtn_quant.hip."""
import numpy as np
import torch

NORM, GRID, MAXSHRINK = 2.4, 100, 0.8      # the reference's defaults (Quantizer.configure)
REL = 1e-4                                  # E64(chosen) <= (1 + REL) min_i E64(i): see tests/test_gpu_rtn_mse.py


def base_pair(x, bits):
    """x: float32 [units, cols].  (xmin, xmax, scale, zero) of every unit, each float32 [units], as tests/rtn_restate.py computes them"""
    x = np.asarray(x, dtype=np.float32)
    maxq = np.float32(2 ** bits - 1)
    with np.errstate(all="ignore"):
        xmin = np.minimum(x.min(axis=1), np.float32(0))
        xmax = np.maximum(x.max(axis=1), np.float32(0))
        both = (xmin == 0) & (xmax == 0)
        xmin[both] = -1
        xmax[both] = 1
        scale = ((xmax - xmin) / maxq).astype(np.float32)
        zero = np.rint(-xmin / scale).astype(np.float32)
    return xmin, xmax, scale, zero


def n_candidates(grid=GRID, maxshrink=MAXSHRINK):
    return int(maxshrink * grid)            # Python's own double product, as the reference's range() takes it


def candidate_pairs(xmin, xmax, bits, grid=GRID, maxshrink=MAXSHRINK):
    """(scale1, zero1), each float32 [n, units]: candidate i shrinks the range by p = float32(1 - i / grid), the subtraction and the division in
    double; every later operation is rounded to float32 on its own"""
    maxq = np.float32(2 ** bits - 1)
    scales, zeros = [], []
    with np.errstate(all="ignore"):
        for i in range(n_candidates(grid, maxshrink)):
            p = np.float32(1 - i / grid)
            xmin1 = (p * xmin).astype(np.float32)
            xmax1 = (p * xmax).astype(np.float32)
            scale1 = ((xmax1 - xmin1).astype(np.float32) / maxq).astype(np.float32)
            zero1 = np.rint((-xmin1 / scale1).astype(np.float32)).astype(np.float32)
            scales.append(scale1)
            zeros.append(zero1)
    return np.stack(scales), np.stack(zeros)


def quant_f32(x, scale, zero, bits):
    """the final pass in fp32: (out, q) with scale / zero float32 [units]"""
    maxq = np.float32(2 ** bits - 1)
    with np.errstate(all="ignore"):
        q = np.clip(np.rint(x / scale[:, None]) + zero[:, None], np.float32(0), maxq).astype(np.float32)
        out = (scale[:, None] * (q - zero[:, None])).astype(np.float32)
    return out, q


def e64(x, scale, zero, bits, norm=NORM):
    """sum_k |out_k - x_k|^norm per unit: out in fp32 as the final pass computes it, the difference, the power and the sum in fp64.  [units]"""
    out, _ = quant_f32(x, scale, zero, bits)
    with np.errstate(all="ignore"):
        return (np.abs(out.astype(np.float64) - x.astype(np.float64)) ** float(norm)).sum(axis=1)


def all_e64(x, bits, norm=NORM, grid=GRID, maxshrink=MAXSHRINK):
    """(scale1 [n, units], zero1 [n, units], E64 [n, units], base scale, base zero)"""
    x = np.asarray(x, dtype=np.float32)
    xmin, xmax, scale, zero = base_pair(x, bits)
    s1, z1 = candidate_pairs(xmin, xmax, bits, grid, maxshrink)
    errs = np.stack([e64(x, s1[i], z1[i], bits, norm) for i in range(s1.shape[0])])
    return s1, z1, errs, scale, zero


def argmin64(errs):
    """per unit: (index of the first smallest finite error, or -1 when none is finite: the unit keeps its base pair; that smallest error)"""
    e = np.where(np.isfinite(errs), errs, np.inf)
    idx = e.argmin(axis=0)                  # the first of equal minima: the lowest index wins ties
    best = e[idx, np.arange(e.shape[1])]
    return np.where(np.isfinite(best), idx, -1), best


def mse_restate_f32(x, bits, norm=NORM, grid=GRID, maxshrink=MAXSHRINK):
    """the search by the fp64 criterion: (out fp32, q fp32, scale [units], zero [units], ready)"""
    x = np.asarray(x, dtype=np.float32)
    s1, z1, errs, scale, zero = all_e64(x, bits, norm, grid, maxshrink)
    idx, _ = argmin64(errs)
    u = np.arange(x.shape[0])
    ok = (idx >= 0) & np.isfinite(scale) & (scale != 0)
    scale = np.where(ok, s1[np.maximum(idx, 0), u], scale).astype(np.float32)
    zero = np.where(ok, z1[np.maximum(idx, 0), u], zero).astype(np.float32)
    out, q = quant_f32(x, scale, zero, bits)
    return out, q, scale, zero, bool(np.all(scale != 0))


def bits_of(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_f32(a, b):
    """elementwise: equal bits, or both NaN (a NaN's sign and payload are the platform's)"""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return (bits_of(a) == bits_of(b)) | (np.isnan(a) & np.isnan(b))


def slices(cols, G):
    """column ranges of the units of a row: the whole row (G = 0), or its groups, the last one holding what is left"""
    return [(0, cols)] if not G else [(c, min(c + G, cols)) for c in range(0, cols, G)]


def check_choice(x, bits, G, scale, zero, norm=NORM, grid=GRID, maxshrink=MAXSHRINK, rel=REL, exact=False):
    """the properties a chosen (scale, zero) per unit must have.  x: float32 [rows, cols]; scale, zero: float32 [rows] (G = 0) or [rows, ng].
    (a) the pair is one of the restated candidates, bit for bit — the base pair for a unit none of whose candidates has a finite error;
    (b) E64(chosen) <= (1 + rel) min_i E64(i); with exact=True the pair must be THE fp64 argmin (the lowest index among equal minima);
    never worse: E64(chosen) <= (1 + rel) E64(base pair).
    Returns the largest E64(chosen) / min - 1 seen, for the record."""
    x = np.asarray(x, dtype=np.float32)
    scale = np.asarray(scale, dtype=np.float32).reshape(x.shape[0], -1)
    zero = np.asarray(zero, dtype=np.float32).reshape(x.shape[0], -1)
    worst = 0.0
    for j, (c0, c1) in enumerate(slices(x.shape[1], G)):
        xs = x[:, c0:c1]
        s1, z1, errs, bscale, bzero = all_e64(xs, bits, norm, grid, maxshrink)
        idx, best = argmin64(errs)
        sb, zb = bits_of(scale[:, j]), bits_of(zero[:, j])
        member = (bits_of(s1) == sb[None, :]) & (bits_of(z1) == zb[None, :])
        is_base = same_f32(scale[:, j], bscale) & same_f32(zero[:, j], bzero)
        searched = (idx >= 0) & np.isfinite(bscale) & (bscale != 0)
        assert np.all(is_base[~searched]), f"group {j}: a unit without a finite candidate left its base pair: rows {np.nonzero(~is_base & ~searched)[0]}"
        assert np.all(member.any(axis=0)[searched]), f"group {j}: pair outside the candidate set: rows {np.nonzero(~member.any(axis=0) & searched)[0]}"
        rows = np.nonzero(searched)[0]
        if exact:
            want_s, want_z = s1[idx[rows], rows], z1[idx[rows], rows]
            assert np.array_equal(bits_of(want_s), sb[rows]) and np.array_equal(bits_of(want_z), zb[rows]), f"group {j}: not the fp64 argmin"
        chosen = e64(xs[rows], scale[rows, j], zero[rows, j], bits, norm)
        base = e64(xs[rows], bscale[rows], bzero[rows], bits, norm)
        assert np.all(chosen <= (1 + rel) * best[rows]), f"group {j}: E64(chosen) / min - 1 = {np.max(chosen / best[rows] - 1):.3e}"
        assert np.all(chosen[np.isfinite(base)] <= (1 + rel) * base[np.isfinite(base)]), f"group {j}: worse than the base pair"
        nz = best[rows] > 0
        if nz.any():
            worst = max(worst, float(np.max(chosen[nz] / best[rows][nz] - 1)))
    return worst


def final_restate(w, bits, G, scale, zero):
    """the final pass with GIVEN pairs: (out in w.dtype on the CPU, codes uint8) for a torch tensor w and torch scale / zero [rows] or [rows, ng]"""
    x = w.detach().cpu().float().numpy()
    scale = scale.detach().cpu().numpy().reshape(x.shape[0], -1)
    zero = zero.detach().cpu().numpy().reshape(x.shape[0], -1)
    outs, qs = [], []
    for j, (c0, c1) in enumerate(slices(x.shape[1], G)):
        o, q = quant_f32(x[:, c0:c1], scale[:, j], zero[:, j], bits)
        outs.append(o)
        qs.append(q)
    out, q = np.concatenate(outs, axis=1), np.concatenate(qs, axis=1)
    q = np.where(np.isnan(q), np.float32(0), q).astype(np.uint8)
    return torch.from_numpy(out).to(w.dtype), torch.from_numpy(q)
