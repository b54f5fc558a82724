"""CPU restatement of the reference's RTN quantizer (quantization.py:17-21,31-145: perchannel=True, sym=False, mse=False, weight=True) in
numpy, written from the contract and checked against the reference's own outputs (tests/golden/rtn_ref.npz).  Test code only: the product
path is csrc/rtn_quant.hip."""
import numpy as np
import torch


def rtn_restate_f32(x, bits):
    """x: float32 [rows, cols] (the weight upcast to fp32).  Returns (out fp32, q fp32, scale [rows], zero [rows], ready)."""
    x = np.asarray(x, dtype=np.float32)
    maxq = np.float32(2 ** bits - 1)
    with np.errstate(all="ignore"):
        xmin = np.minimum(x.min(axis=1), np.float32(0))   # numpy's min / minimum propagate NaN, as torch's do
        xmax = np.maximum(x.max(axis=1), np.float32(0))
        both = (xmin == 0) & (xmax == 0)
        xmin[both] = -1
        xmax[both] = 1
        scale = ((xmax - xmin) / maxq).astype(np.float32)
        zero = np.rint(-xmin / scale).astype(np.float32)
        q = np.clip(np.rint(x / scale[:, None]) + zero[:, None], np.float32(0), maxq).astype(np.float32)
        out = (scale[:, None] * (q - zero[:, None])).astype(np.float32)
    return out, q, scale, zero, bool(np.all(scale != 0))


def rtn_restate(w, bits):
    """torch tensor in / out, any of fp16 / bf16 / fp32 on any device: (out in w.dtype on CPU, q, scale, zero, ready); out == w when not
    ready (the reference returns the tensor unchanged)"""
    w_cpu = w.detach().cpu()
    out, q, scale, zero, ready = rtn_restate_f32(w_cpu.float().numpy(), bits)
    res = torch.from_numpy(out).to(w.dtype) if ready else w_cpu.clone()
    return res, torch.from_numpy(q), torch.from_numpy(scale), torch.from_numpy(zero), ready


def codes_of(q):
    """the uint8 codes the kernel writes: q where it is a number, 0 where it is NaN"""
    q = q.clone()
    q[torch.isnan(q)] = 0
    return q.to(torch.uint8)
