"""Generate tests/golden/rtn_mse_ref.npz by IMPORTING the reference's quantization module (read-only checkout: $ASVD_REFERENCE, default a
`reference` directory next to this repository) on the host, as tools/make_golden_rtn.py does.  Run once in the build container
(`python tools/make_golden_rtn_mse.py`); never on the GPU box: only the vectors travel.  The fixture is data — inputs, and the scale, zero and
output of the reference's own Quantizer (quantization.py:31-145) configured with perchannel=True, sym=False, mse=True (norm 2.4, grid 100,
maxshrink 0.8) — no reference source text.

Cases (`cases`: "<case>:<dtype>:<bits>:<group>:<input key>"), for dtype f16 / bf16 / f32, bits 3 / 4 / 8 and group 0 / 128 / 64:
  edge_<dtype>_int<bits>_g<group>      the crafted edge rows of tools/make_golden_rtn.py (zero, one-signed, constant, tie, NaN, +-Inf rows, rows with
                                       zeros, weight-like rows): 48 columns per row, 200 columns with groups (128 + 72; 64 + 64 + 64 + 8), where the
                                       NaN / Inf sit in the first group only
  graded_f16_int<bits>_g<group>        tests/group_restate.py::graded_matrix(0), 37 x 1104 fp16
Per case: <case>_scale, <case>_zero float32 [rows] or [rows, ng]; <case>_out the quantized weight in the case's dtype, stored as float16 (f16), as
the upper 16 bits of the float32 (bf16, uint16) or as float32; the input under <input key>, stored the same way.  With groups the Quantizer runs on
every column slice [rows, G] (the last one shorter) as a weight of its own, which is what quantizing the weight reshaped to groups means."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("ASVD_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))
OUT = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)

import quantization as ref_q  # noqa: E402

from tests.group_restate import graded_matrix  # noqa: E402

DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
BITS = (3, 4, 8)
GROUPS = (0, 128, 64)


def crafted_rows(bits, dtype, g, cols):
    """the edge rows of tools/make_golden_rtn.py at `cols` columns: [20, cols] float32 holding values representable in `dtype`"""
    maxq = 2 ** bits - 1
    rows = [torch.zeros(cols),                                                # all zero -> xmin, xmax = -1, +1
            torch.rand(cols, generator=g) * 3 + 0.25,                         # all positive
            -(torch.rand(cols, generator=g) * 3 + 0.25),                      # all negative
            torch.full((cols,), 0.75), torch.full((cols,), -1.5)]             # constant rows
    ties = torch.arange(cols, dtype=torch.float32) % 16 + 0.5                 # x / scale = k + 0.5 exactly at p = 1
    ties[0], ties[1] = 0.0, float(maxq)
    rows.append(ties)
    mixed = -(torch.arange(cols, dtype=torch.float32) % 8) - 0.5
    mixed[0], mixed[1] = -float((maxq + 1) // 2), float((maxq - 1) // 2)
    rows.append(mixed)
    for idx, val in ((5, float("nan")), (7, float("inf")), (3, float("-inf"))):
        r = torch.randn(cols, generator=g)
        r[idx] = val
        rows.append(r)
    small = torch.randn(cols, generator=g) * 1e-3
    small[::3] = 0.0
    rows.append(small)                                                        # zeros inside a row
    for _ in range(9):
        rows.append(torch.randn(cols, generator=g) * 0.02)                    # weight-like rows
    return torch.stack(rows).to(dtype).float()


def reference_quant(w, bits):
    """the reference's Quantizer with the search on, called as rtn_quant_sequential calls it: (out in w.dtype, scale [rows], zero [rows])"""
    quantizer = ref_q.Quantizer()
    quantizer.configure(bits, perchannel=True, sym=False, mse=True)
    quantizer.find_params(w.float(), weight=True)
    assert bool(quantizer.ready())
    out = quantizer.quantize(w.float()).to(w.dtype)
    return out, quantizer.scale.reshape(-1).float(), quantizer.zero.reshape(-1).float()


def reference_quant_grouped(w, bits, G):
    if not G:
        return reference_quant(w, bits)
    parts = [reference_quant(w[:, c:c + G].contiguous(), bits) for c in range(0, w.shape[1], G)]
    return torch.cat([p[0] for p in parts], 1), torch.stack([p[1] for p in parts], 1), torch.stack([p[2] for p in parts], 1)


def stored(t, dname):
    """a tensor of the case's dtype as the smallest exact numpy array"""
    if dname == "f16":
        return t.half().numpy()
    if dname == "bf16":
        return (t.float().contiguous().view(torch.int32) >> 16).to(torch.int16).numpy().view(np.uint16)
    return t.float().numpy()


def main():
    g = torch.Generator().manual_seed(2401)
    arrays, cases = {}, []
    for dname, dtype in DTYPES.items():
        for bits in BITS:
            for cols in (48, 200):
                key = f"edge_{dname}_int{bits}_x{cols}"
                w = crafted_rows(bits, dtype, g, cols).to(dtype)
                arrays[key] = stored(w, dname)
                for G in GROUPS:
                    if bool(G) != (cols == 200):
                        continue
                    case = f"edge_{dname}_int{bits}_g{G}"
                    out, scale, zero = reference_quant_grouped(w, bits, G)
                    arrays.update({f"{case}_out": stored(out, dname), f"{case}_scale": scale.numpy(), f"{case}_zero": zero.numpy()})
                    cases.append(f"{case}:{dname}:{bits}:{G}:{key}")
    w = graded_matrix(0)
    arrays["graded_x"] = stored(w, "f16")
    for bits in BITS:
        for G in GROUPS:
            case = f"graded_f16_int{bits}_g{G}"
            out, scale, zero = reference_quant_grouped(w, bits, G)
            arrays.update({f"{case}_out": stored(out, "f16"), f"{case}_scale": scale.numpy(), f"{case}_zero": zero.numpy()})
            cases.append(f"{case}:f16:{bits}:{G}:graded_x")
    arrays["cases"] = np.array(cases)
    path = os.path.join(OUT, "rtn_mse_ref.npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path} ({os.path.getsize(path)} bytes, {len(cases)} cases)")


if __name__ == "__main__":
    main()
