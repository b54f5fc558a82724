"""Benchmark of the packed (uint8 codes, W8A16 kernel: csrc/w8_linear.hip) forward against the fake-quantized fp16 weights through nn.Linear,
on the decoder Linears of a Llama-2-7B-shaped model: the dense model and the model after ASVD at param ratio 0.9 with rank_align 128 (the
shape sets of tools/bench_rtn.py).  Prints ONE JSON line.  Needs a gfx950 device; there is no fallback.

One pass walks the Linears of all 32 blocks, every block with its OWN weights (fp16 set ~13 / ~11 GB, packed set ~6.5 / ~6 GB: far beyond the
256 MiB Infinity Cache, so a pass streams from HBM; a loop over one layer would time the cache).  An SVDLinear is BLinear then ALinear, the
intermediate feeding the second.  Per token count (--tokens, default 1, 4, 16, 64):
  (a) nn.Linear modules holding the fake-quantized fp16 weights (what --weight_quant rtn_int8 leaves today),
  (b) W8Linear modules holding the codes of the same quantization (--weight_quant_storage packed),
alternating, device events around each pass, median / min / max / spread (max - min) of --iters passes after --warmup.  At these sizes an eager
pass is bound by the host (Python and launch cost per layer, for both paths), so every figure is reported twice: "eager" as a user's forward runs,
and "graph" with one pass of each path captured into a device graph and replayed (no host work inside the timed window: what the device does).  (b) also gets its
algorithmic bytes (codes + 8 bytes per row + activations in and out), GB/s and the share of the 8 TB/s HBM spec, and the largest difference
between the outputs of (a) and (b) over all layers, relative to the largest output.
--code_bits 6 | 4 quantizes to that width and adds
  (c) WBLinear modules holding the same codes at their own width (--weight_quant_storage bitpacked; csrc/w8_linear.hip, K13),
timed in the same alternation and reported under "bitpacked" with the columns of (b), plus its time over (b)'s and whether it is slower than
(b) by more than (b)'s own spread.  Without --code_bits the output is what it was.
--group_size 64 | 128 adds
  (d) the modules of the narrowest path above ((c) with --code_bits 6 | 4, else (b)) on the SAME code buffers with group-wise scales and zeros
      (csrc/w8_linear.hip, K14; every group of a row carries the row's pair, so (d) stands for the same weights and must give that path's bits),
timed in the same alternation and reported under "grouped": its time over the per-row pass of the same width, the share of weight-side bytes the
[N, ng] parameters add (8 / (G bits / 8) per code byte) and whether the slowdown stays within that share plus the per-row pass's own spread.
--fused_pair runs the ASVD shape set only and adds
  (e) every factor pair of the narrowest path above ((d), else (c), else (b)) through ONE launch (csrc/w8_linear.hip, K16: SVDLinear with
      fused_packed on the same modules, so on the same code buffers; it must give that path's bits),
timed in the same alternation, eager and graph replay (the per-stream workspaces are created by a warm-up pass on the capture stream, before
capture), and reported under "fused_pair": `fused_over_two_launch`, its time over the two-launch pass of the same modules, and whether it is faster
than that pass by more than the pass's own spread (max - min), the noise floor of the comparison.
--gemm measures the token-tiled GEMM on the codes (csrc/w8_linear.hip, K17) instead, at --tokens beyond decode size (default 32 .. 2048), on the
modules of the narrowest path above.  Per shape set and token count it times three passes in alternation, graph replay (device time):
  (g) the packed GEMM (the modules with packed_gemm on and the dispatch maximum lifted, so every token count takes the kernel),
  (h) the dense path, dequantize + F.linear (PackedLinear._dense_forward: what the modules do for these inputs with the switch off),
  (a) nn.Linear on the resident fake-quantized fp16 weights (context only: it keeps two to four times the memory),
and reports `gemm_over_dense`, whether (g) is not slower than (h) by more than (h)'s spread, (g)'s algorithmic GB/s and TFLOP/s, the largest
N K 2-byte temporary (h) allocates per layer, and the largest difference of (g) from (a).
--dtype bf16 (with any of the above) builds every weight, module and input in bf16 and switches the bf16 form of the kernels on (K19,
packed_bf16 on every packed module and pair): (a) is then bf16 nn.Linear on the fake-quantized bf16 weights.  Without --gemm it adds
  (f) dequantize + F.linear in bf16 on the modules of the narrowest path (PackedLinear._dense_forward: what a bf16 module does with the switch off),
timed in the same alternation and reported under "dense_path" with `narrowest_over_dense`, the narrowest packed pass's time over it.  The keys
keep their names ("fp16_linear" is the nn.Linear pass in --dtype); the output carries "dtype": "bf16".  Without --dtype the output is what it was."""
import argparse
import json
import os
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from asvd4llm_amd import _lib as L  # noqa: E402
from asvd4llm_amd import ops  # noqa: E402
from asvd4llm_amd.modules import w8_linear as W  # noqa: E402
from asvd4llm_amd.modules import svd_linear as S  # noqa: E402
from asvd4llm_amd.modules import wb_linear as WB  # noqa: E402
from bench_rtn import HBM_SPEC, median, shape_sets  # noqa: E402

TOKENS = (1, 4, 16, 64)
DT = torch.float16   # --dtype: the dtype of weights, modules and inputs


class DensePath(nn.Module):
    """path (f): dequantize + F.linear on a packed module, whatever its forward() dispatches"""

    def __init__(self, mod):
        super().__init__()
        self.mod = mod

    def forward(self, x):
        return self.mod._dense_forward(x)


def fused_pair_of(b_mod, a_mod):
    """an SVDLinear around two packed modules, with the one-launch forward switched on"""
    m = S.SVDLinear.__new__(S.SVDLinear)
    nn.Module.__init__(m)
    m.BLinear, m.ALinear, m.truncation_rank, m.fused_packed = b_mod, a_mod, b_mod.out_features, True
    m.packed_bf16 = DT == torch.bfloat16
    return m


def build_set(blocks, factored, bits, dev, seed, bitpacked=False, group=0, fused_pair=False, dense=False):
    """per block a list of layers; a layer is a list of (fp16 nn.Linear, W8Linear[, WBLinear]) stages applied in order (BLinear, ALinear for a
    factored layer: bench_rtn lists them as ALinear [out, r], BLinear [r, in])"""
    g = torch.Generator(device=dev).manual_seed(seed)
    out = []
    for blk in blocks:
        ws = [(torch.randn(m, n, generator=g, device=dev, dtype=torch.float32) * 0.02).to(DT) for m, n in blk]
        res = ops.rtn_quant_batched(ws, bits, want_params=True)
        stages = []
        for fake, q, scale, zero, flagged in res:
            assert not flagged
            lin = nn.Linear(fake.shape[1], fake.shape[0], bias=False, device="meta")
            lin.weight = nn.Parameter(fake, requires_grad=False)
            stage = (lin, W.W8Linear.from_codes(q, scale, zero, None, bits, DT))
            if bitpacked:
                stage += (WB.WBLinear.from_codes(q, scale, zero, None, bits, DT),)
            if group:   # the per-row pair of every row, once per group: the same weights on the same code buffer
                ng = ops.n_groups(q.shape[1], group)
                gs, gz = scale[:, None].expand(-1, ng).contiguous(), zero[:, None].expand(-1, ng).contiguous()
                stage += ((WB.WBLinear.from_bits(stage[2].qbits, q.shape[1], gs, gz, None, bits, DT, group_size=group),) if bitpacked
                          else (W.W8Linear.from_codes(q, gs, gz, None, bits, DT, group_size=group),))
            for mod in stage[1:]:
                mod.packed_bf16 = DT == torch.bfloat16
            stages.append(stage)
        narrow = 1 + bool(bitpacked) + bool(group)   # index of the narrowest packed path
        if fused_pair and factored:   # path (e) sits in the BLinear stage and maps x to y; the ALinear stage passes it on
            for i in range(0, len(stages), 2):
                stages[i + 1] += (fused_pair_of(stages[i + 1][-1], stages[i][-1]),)
                stages[i] += (nn.Identity(),)
        if dense:
            stages = [s + (DensePath(s[narrow]),) for s in stages]
        out.append([[stages[i + 1], stages[i]] for i in range(0, len(stages), 2)] if factored else [[s] for s in stages])
    return out


@torch.no_grad()
def run_pass(layers, xs, which):
    for blk in layers:
        for layer in blk:
            y = xs[layer[0][0].in_features]
            for stage in layer:
                y = stage[which](y)
    return y


def timed_paths(layers, xs, iters, warmup, graph, npaths=2):
    times = [[] for _ in range(npaths)]
    if graph:   # one pass of each path, captured once (a linear chain of launches) and replayed
        run = []
        cap = torch.cuda.Stream()   # what a path creates per stream on first use (the workspaces of the fused pair) exists before capture
        cap.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(cap):
            for which in range(npaths):
                run_pass(layers, xs, which)
        torch.cuda.current_stream().wait_stream(cap)
        for which in range(npaths):
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr, stream=cap):
                run_pass(layers, xs, which)
            run.append(gr.replay)
    else:
        run = [lambda which=which: run_pass(layers, xs, which) for which in range(npaths)]
    for it in range(warmup + iters):
        for which, ts in enumerate(times):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run[which]()
            e1.record()
            e1.synchronize()
            if it >= warmup:
                ts.append(e0.elapsed_time(e1))
    return times


@torch.no_grad()
def max_difference(layers, xs, which=1):
    worst, top = 0.0, 0.0
    for blk in layers:
        for layer in blk:
            ya = yb = xs[layer[0][0].in_features]
            for stage in layer:
                ya, yb = stage[0](ya), stage[which](yb)
            worst = max(worst, (ya.float() - yb.float()).abs().max().item())
            top = max(top, ya.float().abs().max().item())
    return worst, top


GEMM_TOKENS = (32, 64, 128, 256, 512, 2048)


@torch.no_grad()
def run_pass_fn(layers, xs, fn):
    for blk in layers:
        for layer in blk:
            y = xs[layer[0][0].in_features]
            for stage in layer:
                y = fn(stage)(y)
    return y


def timed_graphs(passes, iters, warmup):
    """every pass captured into a device graph (after one eager run on the capture stream), replayed in alternation, events around each replay"""
    cap = torch.cuda.Stream()
    cap.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(cap):
        for f in passes:
            f()
    torch.cuda.current_stream().wait_stream(cap)
    run = []
    for f in passes:
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=cap):
            f()
        run.append(gr.replay)
    times = [[] for _ in passes]
    for it in range(warmup + iters):
        for r, ts in zip(run, times):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r()
            e1.record()
            e1.synchronize()
            if it >= warmup:
                ts.append(e0.elapsed_time(e1))
    return times


def run_set_gemm(blocks, factored, args, dev):
    bitpacked = args.code_bits != 8
    layers = build_set(blocks, factored, args.bits, dev, args.seed, bitpacked, args.group_size)
    stages = [s for blk in layers for layer in blk for s in layer]
    for s in stages:
        s[-1].packed_gemm = True
    narrow = [s[-1] for s in stages]
    code_bytes = sum((m.qbits if bitpacked else m.qweight).numel() + 8 * m.scales.numel() for m in narrow)
    res = {"launches_per_pass": len(stages), "module": type(narrow[0]).__name__, "storage_bits": args.code_bits, "group_size": args.group_size,
           "fp16_weight_bytes": sum(2 * s[0].weight.numel() for s in stages), "code_bytes": code_bytes,
           "largest_dense_temporary_bytes": max(2 * s[0].weight.numel() for s in stages), "tokens": {}}
    g = torch.Generator(device=dev).manual_seed(args.seed + 1)
    for T in args.tokens:
        xs = {k: torch.randn(T, k, generator=g, device=dev).to(DT) for k in {layer[0][0].in_features for blk in layers for layer in blk}}
        launched, real = [], ops.packed_gemm
        ops.packed_gemm = lambda *a, **k: (launched.append(1), real(*a, **k))[1]
        run_pass_fn(layers, xs, lambda s: s[-1])
        ops.packed_gemm = real
        assert len(launched) == len(stages), "a module did not dispatch the GEMM"
        passes = [lambda: run_pass_fn(layers, xs, lambda s: s[-1]), lambda: run_pass_fn(layers, xs, lambda s: s[-1]._dense_forward),
                  lambda: run_pass_fn(layers, xs, lambda s: s[0])]
        worst = top = 0.0
        for layer in layers[0]:
            ya, yg = run_pass_fn([[layer]], xs, lambda s: s[0]), run_pass_fn([[layer]], xs, lambda s: s[-1])
            worst, top = max(worst, (ya.float() - yg.float()).abs().max().item()), max(top, ya.float().abs().max().item())
        tg, td, tf = (stats(t) for t in timed_graphs(passes, args.iters, args.warmup))
        flops = sum(2.0 * T * s[0].weight.numel() for s in stages)
        nbytes = code_bytes + sum(2 * T * (s[0].in_features + s[0].out_features) for s in stages)
        res["tokens"][str(T)] = {"gemm": tg, "dense_path": td, "fp16_linear": tf,
                                 "gemm_over_dense": round(tg["median_ms"] / td["median_ms"], 4),
                                 "gemm_over_fp16_linear": round(tg["median_ms"] / tf["median_ms"], 4),
                                 "gemm_not_slower_than_dense": tg["median_ms"] <= td["median_ms"] + td["spread_ms"],
                                 "gemm_gbps": round(nbytes / (tg["median_ms"] * 1e-3) / 1e9, 1),
                                 "gemm_tflops": round(flops / (tg["median_ms"] * 1e-3) / 1e12, 2),
                                 "dense_tflops": round(flops / (td["median_ms"] * 1e-3) / 1e12, 2),
                                 "max_rel_diff_block0": worst / top if top else 0.0}
    del layers
    return res


def stats(ts):
    return {"median_ms": round(median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4), "spread_ms": round(max(ts) - min(ts), 4),
            "all_ms": [round(t, 4) for t in ts]}


def run_set(blocks, factored, args, dev):
    bitpacked = args.code_bits != 8
    fused = bool(args.fused_pair and factored)
    dense = args.dtype == "bf16"
    layers = build_set(blocks, factored, args.bits, dev, args.seed, bitpacked, args.group_size, fused, dense)
    base_path = 2 if bitpacked else 1                       # the per-row pass (d) is compared with
    npaths = 2 + bitpacked + bool(args.group_size) + fused + dense
    grp_path = 1 + bitpacked + bool(args.group_size)        # (d) when it runs
    two_path = grp_path                                     # the narrowest packed pass: the two-launch pass of the modules (e) fuses
    fused_path, dense_path = two_path + 1, npaths - 1       # (e) and (f) when they run
    stages = [s for blk in layers for layer in blk for s in layer]
    code_bytes = sum(s[1].qweight.numel() + 8 * s[1].out_features for s in stages)
    fp16_bytes = sum(2 * s[0].weight.numel() for s in stages)
    res = {"launches_per_pass": len(stages), "fp16_weight_bytes": fp16_bytes, "packed_weight_bytes": code_bytes, "tokens": {}}
    if bitpacked:
        bit_bytes = sum(s[2].qbits.numel() + 8 * s[2].out_features for s in stages)
        res["bitpacked_weight_bytes"] = bit_bytes
    if args.group_size:
        base_bytes = bit_bytes if bitpacked else code_bytes
        grp_bytes = sum(s[grp_path].scales.numel() * 8 - 8 * s[grp_path].out_features for s in stages) + base_bytes
        res.update({"grouped_weight_bytes": grp_bytes, "grouped_extra_byte_share": round(grp_bytes / base_bytes - 1, 4)})
    g = torch.Generator(device=dev).manual_seed(args.seed + 1)
    for T in args.tokens:
        xs = {k: torch.randn(T, k, generator=g, device=dev).to(DT) for k in {layer[0][0].in_features for blk in layers for layer in blk}}
        act_bytes = sum(2 * T * (s[0].in_features + s[0].out_features) for s in stages)
        nbytes = code_bytes + act_bytes
        diff, top = max_difference(layers, xs)
        rec = {"kernel_dispatched": T <= W.W8_FORWARD_MAX_TOKENS, "packed_bytes": nbytes, "max_abs_diff": diff, "max_abs_output": top,
               "max_rel_diff": diff / top if top else 0.0}
        if bitpacked:
            diff_c, _ = max_difference(layers, xs, 2)
            rec.update({"bitpacked_kernel_dispatched": T <= WB.WB_FORWARD_MAX_TOKENS, "bitpacked_bytes": bit_bytes + act_bytes,
                        "bitpacked_max_abs_diff": diff_c, "bitpacked_max_rel_diff": diff_c / top if top else 0.0})
        for mode in ("eager", "graph"):
            times = timed_paths(layers, xs, args.iters, args.warmup, mode == "graph", npaths)
            a, b = stats(times[0]), stats(times[1])
            rec[mode] = {"fp16_linear": a, "packed": b, "packed_over_fp16": round(b["median_ms"] / a["median_ms"], 4),
                         "packed_not_slower": b["median_ms"] <= a["median_ms"] + a["spread_ms"],
                         "packed_gbps": round(nbytes / (b["median_ms"] * 1e-3) / 1e9, 1),
                         "packed_frac_of_hbm_spec": round(nbytes / (b["median_ms"] * 1e-3) / HBM_SPEC, 4),
                         "fp16_gbps": round((fp16_bytes + act_bytes) / (a["median_ms"] * 1e-3) / 1e9, 1)}
            if bitpacked:   # against (b), the one-byte-per-code pass of the same run; (b)'s spread is the noise floor of that comparison
                c = stats(times[2])
                rec[mode].update({"bitpacked": c, "bitpacked_over_fp16": round(c["median_ms"] / a["median_ms"], 4),
                                  "bitpacked_over_packed": round(c["median_ms"] / b["median_ms"], 4),
                                  "bitpacked_minus_packed_ms": round(c["median_ms"] - b["median_ms"], 4),
                                  "bitpacked_not_slower_than_packed": c["median_ms"] <= b["median_ms"] + b["spread_ms"],
                                  "bitpacked_gbps": round((bit_bytes + act_bytes) / (c["median_ms"] * 1e-3) / 1e9, 1),
                                  "bitpacked_frac_of_hbm_spec": round((bit_bytes + act_bytes) / (c["median_ms"] * 1e-3) / HBM_SPEC, 4)})
            if args.group_size:   # against the per-row pass of the same width on the same codes; that pass's spread is the noise floor
                base, d = stats(times[base_path]), stats(times[grp_path])
                share = grp_bytes / base_bytes - 1
                rec[mode].update({"grouped": d, "grouped_over_per_row": round(d["median_ms"] / base["median_ms"], 4),
                                  "grouped_minus_per_row_ms": round(d["median_ms"] - base["median_ms"], 4),
                                  "grouped_within_byte_share_plus_spread": d["median_ms"] <= base["median_ms"] * (1 + share) + base["spread_ms"],
                                  "grouped_gbps": round((grp_bytes + act_bytes) / (d["median_ms"] * 1e-3) / 1e9, 1),
                                  "grouped_frac_of_hbm_spec": round((grp_bytes + act_bytes) / (d["median_ms"] * 1e-3) / HBM_SPEC, 4)})
            if fused:   # against the two launches per pair of the same modules; that pass's spread is the noise floor
                two, e = stats(times[two_path]), stats(times[fused_path])
                rec[mode].update({"fused_pair": e, "two_launch": two, "fused_over_two_launch": round(e["median_ms"] / two["median_ms"], 4),
                                  "fused_minus_two_launch_ms": round(e["median_ms"] - two["median_ms"], 4),
                                  "two_launch_spread_ms": two["spread_ms"],
                                  "fused_faster_by_more_than_spread": e["median_ms"] < two["median_ms"] - two["spread_ms"]})
            if dense:   # (f): what a bf16 module does with the switch off; its spread is the noise floor
                nar, f = stats(times[two_path]), stats(times[dense_path])
                rec[mode].update({"dense_path": f, "narrowest_over_dense": round(nar["median_ms"] / f["median_ms"], 4),
                                  "narrowest_not_slower_than_dense": nar["median_ms"] <= f["median_ms"] + f["spread_ms"]})
        if args.group_size:
            diff_d, _ = max_difference(layers, xs, grp_path)
            same_bits = all(torch.equal(run_pass([[layer]], xs, grp_path), run_pass([[layer]], xs, base_path)) for layer in layers[0])
            rec.update({"grouped_max_rel_diff": diff_d / top if top else 0.0, "grouped_bits_equal_per_row_block0": same_bits})
        if fused:
            rec["fused_pair_dispatched"] = all(layer[0][fused_path].fused_packed_refusal(xs[layer[0][0].in_features]) is None for blk in layers for layer in blk)
            rec["fused_pair_bits_equal_two_launch"] = all(torch.equal(run_pass([[layer]], xs, fused_path), run_pass([[layer]], xs, two_path))
                                                          for blk in layers for layer in blk)
        res["tokens"][str(T)] = rec
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bits", type=int, default=8)
    ap.add_argument("--code_bits", type=int, default=8, choices=[8, 6, 4],
                    help="6 / 4: quantize to that width (overrides --bits) and add path (c), WBLinear on the codes stored at their own width")
    ap.add_argument("--group_size", type=int, default=0, choices=[0, 64, 128],
                    help="64 / 128: add path (d), the narrowest packed path on the same codes with group-wise scales and zeros")
    ap.add_argument("--fused_pair", action="store_true",
                    help="ASVD shape set only: add path (e), every factor pair of the narrowest packed path in one launch (K16), next to its two launches")
    ap.add_argument("--gemm", action="store_true",
                    help="measure the token-tiled GEMM on the codes (K17) against dequantize + F.linear and fp16 nn.Linear at --tokens (default 32 .. 2048)")
    ap.add_argument("--dtype", type=str, default="fp16", choices=["fp16", "bf16"],
                    help="bf16: weights, modules and inputs in bf16 on the bf16 form of the kernels (K19, packed_bf16 on); adds the dense path (f)")
    ap.add_argument("--blocks", type=int, default=0, help="--gemm: decoder blocks per shape set (0: all 32)")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=233)
    ap.add_argument("--tokens", type=lambda v: [int(t) for t in v.split(",")], default=None, help="token counts, comma separated")
    ap.add_argument("--rank_align", type=int, default=128, help="rank alignment of the ASVD shape set (1: ranks such as 1843, whose rows allow no 16-byte loads)")
    ap.add_argument("--force_kernel", action="store_true", help="measure the kernel at every token count and for every row alignment, whatever W8Linear.forward dispatches")
    args = ap.parse_args()
    if args.tokens is None:
        args.tokens = list(GEMM_TOKENS if args.gemm else TOKENS)
    if args.gemm and (args.force_kernel or args.fused_pair or args.rank_align % 16):
        ap.error("--gemm goes without --force_kernel / --fused_pair and needs --rank_align to be a multiple of 16")
    if args.iters < 10:
        ap.error("--iters must be at least 10")
    if args.code_bits != 8:
        args.bits = args.code_bits
        if args.force_kernel and args.rank_align % 16:
            ap.error("--force_kernel with --code_bits 6 / 4 needs --rank_align to be a multiple of 16: the bit-packed kernel takes K % 16 == 0 only")
    if args.fused_pair and args.rank_align % 16:
        ap.error("--fused_pair needs --rank_align to be a multiple of 16: the fused pair takes K % 16 == 0 and r % 16 == 0 only")
    if args.group_size and args.force_kernel and args.rank_align % 16:
        ap.error("--force_kernel with --group_size needs --rank_align to be a multiple of 16: the grouped kernels take K % 16 == 0 only")
    L.load(require_device=True)
    dev = torch.device("cuda", 0)
    global DT
    DT = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    if args.force_kernel:
        W.W8_FORWARD_MAX_TOKENS = ops.W8_MAX_TOKENS
        W.W8Linear.kernel_rows_ok = lambda self: True   # rows that allow no 16-byte loads too (--rank_align 1)
        WB.WB_FORWARD_MAX_TOKENS = ops.W8_MAX_TOKENS
        S.FUSED_PACKED_MAX_TOKENS = ops.W8_MAX_TOKENS
    if args.gemm:
        from asvd4llm_amd.modules import packed_linear as P
        P.PACKED_GEMM_MAX_TOKENS = ops.PACKED_GEMM_MAX_TOKENS   # measure the kernel at every token count, whatever forward() dispatches
        res = {"metric": "w8_gemm", "bits": args.bits, "iters": args.iters, "warmup": args.warmup, "rank_align": args.rank_align,
               "timing": "graph replay, device events", "sets": {}}
        if args.dtype != "fp16":
            res["dtype"] = args.dtype
        for name, blocks in shape_sets(0.9, args.rank_align).items():
            res["sets"][name] = run_set_gemm(blocks[:args.blocks] if args.blocks else blocks, "asvd" in name, args, dev)
            torch.cuda.empty_cache()
        print(json.dumps(res), flush=True)
        return
    res = {"metric": "w8_forward", "bits": args.bits, "hbm_spec_Bps": HBM_SPEC, "iters": args.iters, "warmup": args.warmup,
           "dispatch_max_tokens": W.W8_FORWARD_MAX_TOKENS, "force_kernel": bool(args.force_kernel), "rank_align": args.rank_align, "sets": {}}
    if args.dtype != "fp16":
        res["dtype"] = args.dtype
    if args.group_size:
        res["group_size"] = args.group_size
    if args.code_bits != 8:
        res.update({"code_bits": args.code_bits, "bitpacked_dispatch_max_tokens": WB.WB_FORWARD_MAX_TOKENS})
    if args.fused_pair:
        res.update({"fused_pair": True, "fused_pair_dispatch_max_tokens": S.FUSED_PACKED_MAX_TOKENS})
    for name, blocks in shape_sets(0.9, args.rank_align).items():
        if args.fused_pair and "asvd" not in name:
            continue
        res["sets"][name] = run_set(blocks, "asvd" in name, args, dev)
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
