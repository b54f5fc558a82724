"""Benchmark of the RTN weight-quantization step (--weight_quant rtn_int8 / rtn_int6; csrc/rtn_quant.hip) on the decoder Linears of a
Llama-2-7B-shaped model: the 32 blocks of the dense model (q/k/v/o 4096x4096, gate/up 11008x4096, down 4096x11008, fp16), and the same
model after ASVD at param ratio 0.9 with rank_align 128 (every Linear an SVDLinear at that ratio: ALinear [out, r] and BLinear [r, in] —
a uniform stand-in for the searched plan, which depends on calibration data).  Prints ONE JSON line.

Per shape set: kernel time (device events around the 32 per-block batched launches, no host sync in between; median of --iters),
algorithmic bytes (one read + one write of every weight: 2 x elements x 2 B), GB/s and the fraction of the 8 TB/s HBM spec over kernel time,
the same step through asvd4llm_amd.quantization's per-block path (with its flag read-back), and the reference's torch sequence
(quantization.py:17-21,31-145 restated op for op in torch: .float(), row min / max, scale, zero, round, clamp, dequantize, cast back) timed
on the same GPU, with every output compared bit for bit.
--group_size 64 | 128 times the group-wise form (asvd_rtn_quant_grouped_batched: one scale and zero per group of that many columns) against the
same torch sequence applied to the weight reshaped to groups (the whole groups as [rows * n, G], what is left of every row as [rows, rest]).
--mse times the clip search (K15, asvd_rtn_quant_mse_batched, the reference's defaults: norm 2.4, grid 100, maxshrink 0.8 = 80 candidates) against
a torch-op sequence of the same search written for this tool (torch_search below) on the same device tensors.  The torch sequence makes several
hundred passes over an fp32 copy of every weight, so it is timed on the first block only (--torch_blocks) and reported per block and scaled to the
set.  The two choose by differently rounded sums, so they are compared by what they achieve: the fraction of units with the same scale and the
relative Frobenius error of both outputs."""
import argparse
import ctypes
import json
import os
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from asvd4llm_amd import _lib as L  # noqa: E402
from asvd4llm_amd import ops  # noqa: E402
from asvd4llm_amd.modules.svd_linear import SVDLinear  # noqa: E402

HBM_SPEC = 8.0e12
HIDDEN, INTER, BLOCKS = 4096, 11008, 32
BLOCK_LINEARS = [(HIDDEN, HIDDEN)] * 4 + [(INTER, HIDDEN)] * 2 + [(HIDDEN, INTER)]   # [out, in]


def shape_sets(ratio=0.9, align=128):
    dense = [list(BLOCK_LINEARS) for _ in range(BLOCKS)]
    asvd = []
    for _ in range(BLOCKS):
        blk = []
        for out_f, in_f in BLOCK_LINEARS:
            lin = types.SimpleNamespace(weight=types.SimpleNamespace(numel=lambda o=out_f, i=in_f: o * i), in_features=in_f, out_features=out_f)
            r = SVDLinear.compute_rank(lin, ratio, align)
            blk += [(out_f, r), (r, in_f)]
        asvd.append(blk)
    return {"llama2_7b_dense": dense, f"llama2_7b_asvd{ratio}_align{align}": asvd}


@torch.no_grad()
def torch_sequence(w, bits):
    """the reference's per-tensor torch ops on the device (find_params + quantize + cast back)"""
    x = w.float()
    tmp = torch.zeros(x.shape[0], device=x.device)
    xmin = torch.minimum(x.min(1)[0], tmp)
    xmax = torch.maximum(x.max(1)[0], tmp)
    t = (xmin == 0) & (xmax == 0)
    xmin[t] = -1
    xmax[t] = +1
    maxq = torch.tensor(2 ** bits - 1, device=x.device)
    scale = ((xmax - xmin) / maxq).reshape(-1, 1)
    zero = torch.round(-xmin.reshape(-1, 1) / scale)
    if not torch.all(scale != 0):
        return w
    q = torch.clamp(torch.round(x / scale) + zero, 0, maxq)
    return (scale * (q - zero)).to(w.dtype)


@torch.no_grad()
def torch_sequence_grouped(w, bits, group):
    """torch_sequence on the weight reshaped to groups; unchanged when any group's scale is 0"""
    rows, cols = w.shape
    whole = cols // group * group
    srcs = ([w[:, :whole].reshape(-1, group)] if whole else []) + ([w[:, whole:].contiguous()] if cols > whole else [])
    parts = [torch_sequence(a, bits) for a in srcs]
    if any(p is a for p, a in zip(parts, srcs)):   # torch_sequence returns its input when a scale is 0
        return w
    return torch.cat([p.reshape(rows, -1) for p in parts], dim=1)


@torch.no_grad()
def torch_search(w, bits, norm=2.4, grid=100, maxshrink=0.8):
    """the clip search as a sequence of torch ops on the device: per row, the range shrunk by p = 1 - i / grid for i < int(maxshrink * grid), the
    pair with the smallest sum |q(x) - x|^norm kept (strictly smaller only), then the quantization with the kept pair.  Returns (out, scale)."""
    x = w.float()
    maxq = float(2 ** bits - 1)
    lo = torch.clamp(x.amin(1), max=0.0)
    hi = torch.clamp(x.amax(1), min=0.0)
    dead = (lo == 0) & (hi == 0)
    lo[dead], hi[dead] = -1.0, 1.0
    scale = (hi - lo) / maxq
    zero = torch.round(-lo / scale)
    best = torch.full_like(scale, float("inf"))
    for i in range(int(maxshrink * grid)):
        p = 1 - i / grid
        lo1, hi1 = p * lo, p * hi
        s1 = (hi1 - lo1) / maxq
        z1 = torch.round(-lo1 / s1)
        d = torch.clamp(torch.round(x / s1[:, None]) + z1[:, None], 0, maxq)
        d.sub_(z1[:, None]).mul_(s1[:, None]).sub_(x).abs_().pow_(norm)
        err = d.sum(1)
        better = err < best
        best = torch.where(better, err, best)
        scale = torch.where(better, s1, scale)
        zero = torch.where(better, z1, zero)
    q = torch.clamp(torch.round(x / scale[:, None]) + zero[:, None], 0, maxq)
    return (scale[:, None] * (q - zero[:, None])).to(w.dtype), scale


@torch.no_grad()
def torch_search_grouped(w, bits, group):
    """torch_search on the weight reshaped to groups: (out, scale [rows, ng])"""
    rows, cols = w.shape
    whole = cols // group * group
    srcs = ([w[:, :whole].reshape(-1, group)] if whole else []) + ([w[:, whole:].contiguous()] if cols > whole else [])
    parts = [torch_search(a, bits) for a in srcs]
    return torch.cat([o.reshape(rows, -1) for o, _ in parts], dim=1), torch.cat([s.reshape(rows, -1) for _, s in parts], dim=1)


def bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int16), b.view(torch.int16))


def median(xs):
    s = sorted(xs)
    return s[len(s) // 2]


def run_set_mse(blocks, bits, iters, warmup, dev, seed, group, torch_blocks):
    """the search kernel on every block (events around the per-block launches), the torch sequence on the first `torch_blocks` blocks"""
    lib = L.load(True)
    g = torch.Generator(device=dev).manual_seed(seed)
    ws = [[(torch.randn(m, n, generator=g, device=dev, dtype=torch.float32) * 0.02).half() for m, n in blk] for blk in blocks]
    outs = [[torch.empty_like(w) for w in blk] for blk in ws]
    scales = [[torch.empty(w.shape[0], ops.n_groups(w.shape[1], group) if group else 1, device=dev) for w in blk] for blk in ws]
    flags = torch.zeros(BLOCKS * 16, dtype=torch.int32, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ncand = int(0.8 * 100)
    calls = []
    for b, (blk, oblk, sblk) in enumerate(zip(ws, outs, scales)):
        n = len(blk)
        vp, i64 = ctypes.c_void_p * n, ctypes.c_int64 * n
        calls.append((n, vp(*[w.data_ptr() for w in blk]), (ctypes.c_int * n)(*[L.F16] * n), i64(*[w.shape[0] for w in blk]),
                      i64(*[w.shape[1] for w in blk]), i64(*[w.stride(0) for w in blk]), bits, vp(*[o.data_ptr() for o in oblk]),
                      i64(*[o.stride(0) for o in oblk]), vp(*[s.data_ptr() for s in sblk]), None, None,
                      ctypes.c_void_p(flags.data_ptr() + 4 * 16 * b), stream, group, 2.4, 100, 0.8))

    def launch_all():
        for c in calls:
            L.check(lib.asvd_rtn_quant_mse_batched(*c), "asvd_rtn_quant_mse_batched")

    def timed(fn, n):
        ts = []
        for _ in range(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return ts

    timed(launch_all, warmup)
    kern = timed(launch_all, iters)
    assert int(flags.sum().item()) == 0
    reference = (lambda w: torch_search_grouped(w, bits, group)) if group else (lambda w: torch_search(w, bits))
    tb = ws[:torch_blocks]

    def ref_path():
        return [[reference(w) for w in blk] for blk in tb]
    timed(ref_path, 1)
    ref_ms = timed(ref_path, max(1, min(iters, 3)))
    units = same = 0
    err_k = err_t = 0.0
    for blk, oblk, sblk in zip(tb, outs, scales):      # what both achieve, on the blocks the torch sequence ran
        for w, o, s in zip(blk, oblk, sblk):
            t_out, t_scale = reference(w)
            units += s.numel()
            same += int((s.reshape(-1) == t_scale.reshape(-1)).sum().item())
            wn = w.double().norm()
            err_k = max(err_k, float((o.double() - w.double()).norm() / wn))
            err_t = max(err_t, float((t_out.double() - w.double()).norm() / wn))
    elems = sum(w.numel() for blk in ws for w in blk)
    k, t = median(kern), median(ref_ms)
    t_all = t * len(ws) / len(tb)
    return {"tensors": sum(len(b) for b in ws), "elements": elems, "candidates": ncand, "kernel_ms": round(k, 3),
            "kernel_ms_all": [round(x, 3) for x in kern], "kernel_ps_per_weight_and_candidate": round(k * 1e9 / (elems * ncand), 4),
            "torch_blocks": len(tb), "torch_sequence_ms_per_block": round(t / len(tb), 2), "torch_sequence_ms_all": [round(x, 2) for x in ref_ms],
            "torch_sequence_ms_scaled_to_set": round(t_all, 1), "speedup_vs_torch": round(t_all / k, 2),
            "units_compared": units, "units_with_the_same_scale": same, "max_rel_fro_err_kernel": round(err_k, 6),
            "max_rel_fro_err_torch": round(err_t, 6)}


def run_set(blocks, bits, iters, warmup, dev, seed, group=0):
    lib = L.load(True)
    g = torch.Generator(device=dev).manual_seed(seed)
    ws = [[(torch.randn(m, n, generator=g, device=dev, dtype=torch.float32) * 0.02).half() for m, n in blk] for blk in blocks]
    outs = [[torch.empty_like(w) for w in blk] for blk in ws]
    flags = torch.zeros(BLOCKS * 16, dtype=torch.int32, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    calls = []
    for b, (blk, oblk) in enumerate(zip(ws, outs)):   # ABI argument arrays built once: the timed window holds launches only
        n = len(blk)
        vp, i64 = ctypes.c_void_p * n, ctypes.c_int64 * n
        calls.append((n, vp(*[w.data_ptr() for w in blk]), (ctypes.c_int * n)(*[L.F16] * n), i64(*[w.shape[0] for w in blk]),
                      i64(*[w.shape[1] for w in blk]), i64(*[w.stride(0) for w in blk]), bits, vp(*[o.data_ptr() for o in oblk]),
                      i64(*[o.stride(0) for o in oblk]), None, None, None, ctypes.c_void_p(flags.data_ptr() + 4 * 16 * b), stream))

    def launch_all():
        for c in calls:
            if group:
                L.check(lib.asvd_rtn_quant_grouped_batched(*c, group), "asvd_rtn_quant_grouped_batched")
            else:
                L.check(lib.asvd_rtn_quant_batched(*c), "asvd_rtn_quant_batched")

    reference = (lambda w: torch_sequence_grouped(w, bits, group)) if group else (lambda w: torch_sequence(w, bits))

    def timed(fn, n):
        ts = []
        for _ in range(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return ts

    timed(launch_all, warmup)
    kern = timed(launch_all, iters)
    assert int(flags.sum().item()) == 0

    def ops_path():
        for blk in ws:
            ops.rtn_quant_batched(blk, bits, group_size=group)
    timed(ops_path, max(1, warmup // 2))
    ops_ms = timed(ops_path, iters)

    def ref_path():
        return [[reference(w) for w in blk] for blk in ws]
    timed(ref_path, 1)
    ref_ms = timed(ref_path, max(1, iters // 2))

    mismatched, compared = 0, 0
    for blk, oblk in zip(ws, outs):
        for w, o in zip(blk, oblk):
            compared += 1
            mismatched += not bits_equal(o, reference(w))
    elems = sum(w.numel() for blk in ws for w in blk)
    nbytes = 2 * elems * 2
    k = median(kern)
    return {"tensors": sum(len(b) for b in ws), "launches": sum((n + 15) // 16 for n, *_ in calls), "elements": elems, "bytes": nbytes,
            "kernel_ms": round(k, 4), "kernel_ms_all": [round(t, 4) for t in kern], "gbps": round(nbytes / (k * 1e-3) / 1e9, 1),
            "frac_of_hbm_spec": round(nbytes / (k * 1e-3) / HBM_SPEC, 4), "ops_path_ms": round(median(ops_ms), 4),
            "torch_sequence_ms": round(median(ref_ms), 4), "speedup_vs_torch": round(median(ref_ms) / k, 2),
            "bit_exact_vs_torch": mismatched == 0, "tensors_compared": compared, "tensors_mismatched": mismatched}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bits", type=int, default=8)
    ap.add_argument("--group_size", type=int, default=0, choices=[0, 64, 128], help="64 / 128: the group-wise quantizer (K14)")
    ap.add_argument("--mse", action="store_true", help="time the clip search (K15) against a torch-op sequence of the same search")
    ap.add_argument("--torch_blocks", type=int, default=1, help="--mse: blocks the torch sequence is timed on (it is scaled to the set)")
    ap.add_argument("--sets", type=str, default="", help="comma-separated substrings: only the shape sets whose name contains one")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=233)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    L.load(require_device=True)
    res = {"metric": "rtn_quant_mse_kernel" if args.mse else "rtn_quant_kernel", "bits": args.bits, "dtype": "float16", "hbm_spec_Bps": HBM_SPEC, "sets": {}}
    if args.group_size:
        res["group_size"] = args.group_size
    for name, blocks in shape_sets().items():
        if args.sets and not any(k in name for k in args.sets.split(",")):
            continue
        if args.mse:
            res["sets"][name] = run_set_mse(blocks, args.bits, args.iters, args.warmup, dev, args.seed, args.group_size, args.torch_blocks)
        else:
            res["sets"][name] = run_set(blocks, args.bits, args.iters, args.warmup, dev, args.seed, args.group_size)
        torch.cuda.empty_cache()
    if not args.mse:
        res["bit_exact_vs_torch"] = all(s["bit_exact_vs_torch"] for s in res["sets"].values())
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
