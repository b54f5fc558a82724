"""CPU restatement of group-wise RTN quantization: tests/rtn_restate.py (the reference's Quantizer with perchannel=True, sym=False, mse=False,
pinned by tests/golden/rtn_ref.npz) applied slice by slice.  Group j of row n is the one-row tensor w[n, jG:(j+1)G]; the last group of a row
holds what is left when the column count is no multiple of G.  Test code only: the product path is csrc/rtn_quant.hip."""
import numpy as np
import torch

from tests.rtn_restate import rtn_restate_f32

GROUPS = [64, 128]


def n_groups(cols, G):
    return (cols + G - 1) // G


def group_restate_f32(x, bits, G):
    """x: float32 [rows, cols].  Returns (out fp32 [rows, cols], q fp32 [rows, cols], scale [rows, ng], zero [rows, ng], ready): ready is the
    reference's Quantizer.ready() over the tensor reshaped to groups (no group of scale 0)."""
    x = np.asarray(x, dtype=np.float32)
    parts = [rtn_restate_f32(x[:, c:c + G], bits) for c in range(0, x.shape[1], G)]
    out, q = (np.concatenate([p[i] for p in parts], axis=1) for i in (0, 1))
    scale, zero = (np.ascontiguousarray(np.stack([p[i] for p in parts], axis=1)) for i in (2, 3))
    return out, q, scale, zero, all(p[4] for p in parts)


def group_restate(w, bits, G):
    """torch tensor in / out, any of fp16 / bf16 / fp32 on any device: (out in w.dtype on CPU, q, scale, zero, ready); out == w when not ready"""
    w_cpu = w.detach().cpu()
    out, q, scale, zero, ready = group_restate_f32(w_cpu.float().numpy(), bits, G)
    res = torch.from_numpy(out).to(w.dtype) if ready else w_cpu.clone()
    return res, torch.from_numpy(q), torch.from_numpy(scale), torch.from_numpy(zero), ready


def graded_matrix(seed, rows=37, K=1104):
    """a factor-shaped weight: randn / sqrt(K) with column j scaled by logspace(0, -1.5, K)[j] (sqrt(sigma) falling about 30x across the rank),
    in fp16"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(rows, K, generator=g) / K ** 0.5 * torch.logspace(0, -1.5, K)).half()


def rel_err(out, w):
    """relative Frobenius error, in fp64"""
    return ((out.double().cpu() - w.double().cpu()).norm() / w.double().cpu().norm()).item()
