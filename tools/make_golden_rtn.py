"""Generate tests/golden/rtn_ref.npz and tests/golden/rtn_layers.json by IMPORTING the reference's quantization module (read-only
checkout: $ASVD_REFERENCE, default a `reference` directory next to this repository) on the host.  Run once in the build container
(`python tools/make_golden_rtn.py`); never on the GPU box: only the vectors travel.  The fixtures are data — inputs and outputs of the
reference's own Quantizer (quantization.py:31-145) and rtn_quant_sequential (:157-175) — no reference source text.

rtn_ref.npz, per case `<dtype>_int<bits>` (plus `f32den_int8`, the tensor the reference leaves unchanged):
  <case>_x      input  [rows, cols] as float32 (fp16 / bf16 values are exact in fp32)
  <case>_out    quantizer.quantize(x.float()).to(dtype), as float32
  <case>_q      clamp(round(x / scale) + zero, 0, maxq) with the quantizer's scale / zero, float32 (NaN where the reference has NaN)
  <case>_scale, <case>_zero   find_params' per-row scale / zero, float32 [rows]
  <case>_ready  1 if Quantizer.ready() (every scale != 0), else 0
rtn_layers.json: for tiny-llama and tiny-opt (asvd4llm_amd.model_zoo shapes) with a few Linears replaced by the reference's SVDLinear, the
full names of the nn.Linear modules whose weight rtn_quant_sequential changed, in module order, and the replaced layers with their ranks."""
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("ASVD_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))
OUT = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)

import quantization as ref_q  # noqa: E402
from modules.svd_linear import SVDLinear as RefSVDLinear  # noqa: E402

DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
COLS = 48


def crafted_rows(bits, dtype, g):
    """edge rows + random rows, [rows, COLS] float32 holding values representable in `dtype`"""
    maxq = 2 ** bits - 1
    rows = []
    rows.append(torch.zeros(COLS))                                           # all zero -> xmin, xmax = -1, +1
    rows.append(torch.rand(COLS, generator=g) * 3 + 0.25)                    # all positive
    rows.append(-(torch.rand(COLS, generator=g) * 3 + 0.25))                 # all negative
    rows.append(torch.full((COLS,), 0.75))                                   # constant positive
    rows.append(torch.full((COLS,), -1.5))                                   # constant negative
    ties = torch.arange(COLS, dtype=torch.float32) % 16 + 0.5                # min 0, max maxq: scale 1, x / scale = k + 0.5 exactly
    ties[0], ties[1] = 0.0, float(maxq)
    rows.append(ties)
    mixed = -(torch.arange(COLS, dtype=torch.float32) % 8) - 0.5             # min -(maxq+1)/2, max (maxq-1)/2: scale 1, negative ties
    mixed[0], mixed[1] = -float((maxq + 1) // 2), float((maxq - 1) // 2)
    rows.append(mixed)
    half = torch.randn(COLS, generator=g)
    half[5] = float("nan")
    rows.append(half)                                                        # NaN row
    inf = torch.randn(COLS, generator=g)
    inf[7] = float("inf")
    rows.append(inf)                                                         # +Inf row
    ninf = torch.randn(COLS, generator=g)
    ninf[3] = float("-inf")
    rows.append(ninf)                                                        # -Inf row
    small = torch.randn(COLS, generator=g) * 1e-3
    small[::3] = 0.0
    rows.append(small)                                                       # zeros inside a row
    for _ in range(9):
        rows.append(torch.randn(COLS, generator=g) * 0.02)                   # weight-like rows
    x = torch.stack(rows)
    return x.to(dtype).float()


def reference_quant(x, bits, dtype):
    """the reference's own Quantizer on W = x.to(dtype), as rtn_quant_sequential calls it (quantization.py:166-169)"""
    w = x.to(dtype)
    quantizer = ref_q.Quantizer()
    quantizer.configure(bits, perchannel=True, sym=False, mse=False)
    quantizer.find_params(w.float(), weight=True)
    out = quantizer.quantize(w.float()).to(dtype)
    scale, zero = quantizer.scale.reshape(-1), quantizer.zero.reshape(-1)
    maxq = float(2 ** bits - 1)
    q = torch.clamp(torch.round(w.float() / scale[:, None]) + zero[:, None], 0, maxq)
    return out.float(), q, scale.float(), zero.float(), int(bool(quantizer.ready()))


def make_npz():
    g = torch.Generator().manual_seed(233)
    arrays = {}
    cases = []
    for dname, dtype in DTYPES.items():
        for bits in (8, 6):
            case = f"{dname}_int{bits}"
            x = crafted_rows(bits, dtype, g)
            out, q, scale, zero, ready = reference_quant(x, bits, dtype)
            assert ready == 1, case
            arrays.update({f"{case}_x": x.numpy(), f"{case}_out": out.numpy(), f"{case}_q": q.numpy(), f"{case}_scale": scale.numpy(),
                           f"{case}_zero": zero.numpy(), f"{case}_ready": np.array(ready)})
            cases.append((case, dname, bits))
    # fp32 tensor with one row whose values are all of denormal size: its scale underflows to 0 and the reference returns x unchanged
    x = torch.randn(6, COLS, generator=g) * 0.02
    x[2] = torch.tensor([(k % 5 - 2) * 1.4e-45 for k in range(COLS)])
    out, q, scale, zero, ready = reference_quant(x, 8, torch.float32)
    assert ready == 0 and torch.equal(out, x)
    case = "f32den_int8"
    arrays.update({f"{case}_x": x.numpy(), f"{case}_out": out.numpy(), f"{case}_q": q.numpy(), f"{case}_scale": scale.numpy(),
                   f"{case}_zero": zero.numpy(), f"{case}_ready": np.array(ready)})
    cases.append((case, "f32", 8))
    arrays["cases"] = np.array([f"{c}:{d}:{b}" for c, d, b in cases])
    path = os.path.join(OUT, "rtn_ref.npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path} ({os.path.getsize(path)} bytes, {len(cases)} cases)")


REPLACED = {"tiny-llama": {"model.layers.0.self_attn.q_proj": 16, "model.layers.1.mlp.down_proj": 24},
            "tiny-opt": {"model.decoder.layers.0.self_attn.k_proj": 16, "model.decoder.layers.1.fc2": 24}}


def _replace(model, name, rank, g):
    father_name, child = name.rsplit(".", 1)
    father = model.get_submodule(father_name)
    lin = getattr(father, child)
    U = torch.randn(lin.out_features, rank, generator=g)
    S = torch.rand(rank, generator=g) + 0.5
    V = torch.randn(lin.in_features, rank, generator=g)
    setattr(father, child, RefSVDLinear(U, S, V, lin.bias.data.clone() if lin.bias is not None else None))


def make_layers():
    from asvd4llm_amd.model_zoo import random_init_model
    g = torch.Generator().manual_seed(7)
    res = {}
    for mname, repl in REPLACED.items():
        model = random_init_model(mname, dtype=torch.float32)
        for name, rank in repl.items():
            _replace(model, name, rank, g)
        before = {n: m.weight.data.clone() for n, m in model.named_modules() if type(m) is nn.Linear}
        with contextlib.redirect_stdout(io.StringIO()):
            ref_q.rtn_quant_sequential(model, 8)
        changed = [n for n, m in model.named_modules() if type(m) is nn.Linear and not torch.equal(m.weight.data, before[n])]
        res[mname] = {"replaced": repl, "changed": changed}
    path = os.path.join(OUT, "rtn_layers.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(f"wrote {path}: " + ", ".join(f"{k}: {len(v['changed'])} layers" for k, v in res.items()))


if __name__ == "__main__":
    make_npz()
    make_layers()
