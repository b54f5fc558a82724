"""Benchmark of decode attention on a low-rank KV cache (K20, csrc/lowrank_kv.hip) against the dense baseline: a full fp16 K / V cache through
torch scaled_dot_product_attention, one new token per sequence.  Prints ONE JSON line.  Needs a gfx950 device; there is no fallback.

Shapes: the attention of Llama-2-7B (H = 32, D = 128) and 13B (H = 40), r_k = r_v in --ranks (512 / 1024 / 2048: kv_cache_ratio 0.25 / 0.5 / 1.0
at 7B), T in --tokens cached tokens (every sequence full), B in --batch, both rope modes.  Neither side includes the projections of the new token.

Per shape the two caches of `layers` layers are built from the same factors (K = rot(C_k A_k^T), V = C_v A_v^T in fp16), `layers` chosen so that
either cache passes 512 MiB where memory allows (beyond the 256 MiB Infinity Cache: a pass over the layers streams from HBM, a loop over one
layer would time the cache).  One pass = the call on every layer.  The two passes alternate, device events around each, --iters passes after
--warmup; median / min / max per LAYER in microseconds.  "eager" is the call as a user makes it (host work included), "graph" one pass captured
into a device graph and replayed (what the device does; also the evidence that the K20 sequence is capturable).  Also: the cache bytes per
token and layer of both, the algorithmic bytes and flops of the K20 step, and the largest difference of the two outputs relative to the largest
output (both are fp16 routes to the same value).

--quant int8 adds a third pass per shape: the same latents as int8 codes and one fp32 scale per token and 32 columns (K21: quantised by
asvd_lowrank_kv_quant, decoded by asvd_lowrank_kv_decode_q8), alternating with the other two, eager and graph-replayed; its cache bytes per token,
its time over the fp16 low-rank route's of the same run, and the largest difference of its output from the fp16 low-rank route's.  The run that
profiles/lowrank_kv_q8.json holds: python tools/bench_kv_decode.py --quant int8 > profiles/lowrank_kv_q8.json

--dtype bf16 runs every pass in bf16 (K22): a bf16 dense baseline (bf16 K / V through torch SDPA), the bf16 low-rank route
(asvd_lowrank_kv_decode_a16) and, with --quant int8, the bf16 route on the same int8 format (the latents are quantised from their fp16
conversion, as the cache class does).  A run of one dtype holds no time of the other: for bf16 against fp16 run the tool once per dtype back to
back.  profiles/lowrank_kv_bf16.json holds {"bf16": <the --dtype bf16 --quant int8 line>, "fp16": <the --quant int8 line of the same session>}."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from asvd4llm_amd import _lib as L  # noqa: E402
from asvd4llm_amd import ops  # noqa: E402
from asvd4llm_amd.kv_cache import rotate_half  # noqa: E402


def stats(xs, layers):
    xs = sorted(x * 1e3 / layers for x in xs)   # ms per pass -> us per layer
    return {"median_us": round(xs[len(xs) // 2], 2), "min_us": round(xs[0], 2), "max_us": round(xs[-1], 2)}


def time_alternating(fns, warmup, iters):
    for _ in range(warmup):
        for f in fns:
            f()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(iters):
        for n, f in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ms[n].append(a.elapsed_time(b))
    return ms


def capture(f):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        f()   # workspaces and library handles exist before capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        f()
    return g.replay


def one_shape(dev, H, D, r, T, B, mode, args):
    scale = D ** -0.5
    low_layer, dense_layer = B * T * 2 * r * 2, B * T * 2 * H * D * 2
    layers = max(1, min(args.max_layers, -(-(512 << 20) // min(low_layer, dense_layer))))
    rope = ops.rope_table(T, D, 10000.0, dev) if mode == "half" else None
    g = torch.Generator(device=dev).manual_seed(1)
    dt = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    rnd = lambda *s: torch.randn(*s, generator=g, device=dev, dtype=torch.float16).to(dt)   # one stream of draws for both dtypes
    Ak, Av = (rnd(H * D, r).float() / r ** 0.5).to(dt), (rnd(H * D, r).float() / r ** 0.5).to(dt)
    lens = torch.full((B,), T, dtype=torch.int32, device=dev)
    q = rnd(B, H, D)
    ck, cv, Ks, Vs = [], [], [], []
    for _ in range(layers):
        ck.append(rnd(B, T, r))
        cv.append(rnd(B, T, r))
        K = F.linear(ck[-1], Ak).view(B, T, H, D)
        if rope is not None:
            K = rotate_half(K.float(), rope[0][None, :, None, :], rope[1][None, :, None, :]).to(dt)
        Ks.append(K.transpose(1, 2).contiguous())
        Vs.append(F.linear(cv[-1], Av).view(B, T, H, D).transpose(1, 2).contiguous())
    q8 = []
    if args.quant == "int8":
        for i in range(layers):
            t = [torch.empty(B, T, r, dtype=torch.int8, device=dev), torch.empty(B, T, r, dtype=torch.int8, device=dev),
                 torch.empty(B, T, ops.lowrank_kv_groups(r), dtype=torch.float32, device=dev),
                 torch.empty(B, T, ops.lowrank_kv_groups(r), dtype=torch.float32, device=dev)]
            ops.lowrank_kv_quant(ck[i].half(), t[0], t[2])   # the format is defined on fp16 values
            ops.lowrank_kv_quant(cv[i].half(), t[1], t[3])
            q8.append(t)
    work = ops.lowrank_kv_work(B, H, T, r, r, dev)
    out = torch.empty(B, H, D, dtype=dt, device=dev)
    q4 = q[:, :, None, :]

    def k20():
        for i in range(layers):
            ops.lowrank_kv_decode(q, ck[i], cv[i], lens, Ak, Av, H, scale, rope=rope, work=work, out=out)

    def k21():
        for c_k, c_v, s_k, s_v in q8:
            ops.lowrank_kv_decode_q8(q, c_k, c_v, s_k, s_v, lens, Ak, Av, H, scale, rope=rope, work=work, out=out)

    def dense():
        for i in range(layers):
            F.scaled_dot_product_attention(q4, Ks[i], Vs[i], scale=scale)

    ref = F.scaled_dot_product_attention(q4, Ks[0], Vs[0], scale=scale)[:, :, 0].float()
    got = ops.lowrank_kv_decode(q, ck[0], cv[0], lens, Ak, Av, H, scale, rope=rope).float()
    rec = {"dtype": args.dtype, "H": H, "D": D, "r_k": r, "r_v": r, "T": T, "B": B, "rope": mode, "layers": layers,
           "cache_bytes_per_token_layer": {"lowrank": 2 * r * 2, "dense": 2 * H * D * 2},
           "max_diff_over_max_out": float((got - ref).abs().max() / ref.abs().max())}
    # what one K20 step must move and compute, per layer: both caches once, both ALinear weights once per sequence at most (once if they
    # stay in cache), scores written and read; flops: q~ or the rebuild, scores, the latent sum, the up-projection
    rec["k20_bytes"] = B * T * 2 * r * 2 + 2 * H * D * r * 2 + 2 * B * H * T * 4
    rec["k20_flops"] = (2 * B * T * r * H * D + 2 * B * T * H * D if mode == "half" else 2 * B * H * D * r + 2 * B * T * r * H) \
        + 2 * B * T * r * H + 2 * B * H * D * r
    routes = [k20, dense]
    if q8:
        routes.append(k21)
        got8 = ops.lowrank_kv_decode_q8(q, *q8[0], lens, Ak, Av, H, scale, rope=rope).float()
        rec["cache_bytes_per_token_layer"]["lowrank_int8"] = 2 * (r + 4 * ops.lowrank_kv_groups(r))
        rec["int8_max_diff_from_lowrank_over_max_out"] = float((got8 - got).abs().max() / ref.abs().max())
    e = time_alternating(routes, args.warmup, args.iters)
    rec["eager"] = {"k20": stats(e[0], layers), "dense": stats(e[1], layers)}
    if q8:
        rec["eager"]["k21_int8"] = stats(e[2], layers)
        rec["int8_over_lowrank_eager"] = round(rec["eager"]["k21_int8"]["median_us"] / rec["eager"]["k20"]["median_us"], 3)
    try:
        reps = [capture(f) for f in routes]
        gm = time_alternating(reps, args.warmup, args.iters)
        rec["graph"] = {"k20": stats(gm[0], layers), "dense": stats(gm[1], layers)}
        if q8:
            rec["graph"]["k21_int8"] = stats(gm[2], layers)
            rec["int8_over_lowrank_graph"] = round(rec["graph"]["k21_int8"]["median_us"] / rec["graph"]["k20"]["median_us"], 3)
        rec["k20_over_dense_graph"] = round(rec["graph"]["k20"]["median_us"] / rec["graph"]["dense"]["median_us"], 3)
        rec["k20_GBps_graph"] = round(rec["k20_bytes"] / rec["graph"]["k20"]["median_us"] / 1e3, 1)
    except Exception as ex:   # reported, not hidden: the eager figures stand alone then
        rec["graph"] = f"capture failed: {type(ex).__name__}: {str(ex)[:200]}"
    rec["k20_over_dense_eager"] = round(rec["eager"]["k20"]["median_us"] / rec["eager"]["dense"]["median_us"], 3)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--heads", type=int, nargs="+", default=[32, 40])
    ap.add_argument("--ranks", type=int, nargs="+", default=[512, 1024, 2048])
    ap.add_argument("--tokens", type=int, nargs="+", default=[512, 2048, 4096])
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--modes", nargs="+", default=["none", "half"], choices=["none", "half"])
    ap.add_argument("--head_dim", type=int, default=128)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--max_layers", type=int, default=16)
    ap.add_argument("--dtype", choices=["fp16", "bf16"], default="fp16", help="bf16: every pass in bf16 (K22: the asvd_lowrank_kv_*_a16 entries)")
    ap.add_argument("--quant", choices=["none", "int8"], default="none", help="int8: a third pass on the int8 form of the low-rank cache (K21)")
    args = ap.parse_args()
    L.load(require_device=True)
    dev = torch.device("cuda", 0)
    recs = []
    for H in args.heads:
        for r in args.ranks:
            for T in args.tokens:
                for B in args.batch:
                    for mode in args.modes:
                        recs.append(one_shape(dev, H, args.head_dim, r, T, B, mode, args))
                        print(f"[bench_kv_decode] {json.dumps(recs[-1])}", file=sys.stderr, flush=True)
                        torch.cuda.empty_cache()
    print(json.dumps({"bench": "kv_decode", "device": torch.cuda.get_device_name(0), "runs": 1, "iters_per_run": args.iters, "warmup": args.warmup, "quant": args.quant, "dtype": args.dtype,
                      "timing": "device events around one pass over `layers` layers, the routes alternating; per-layer microseconds",
                      "results": recs}))


if __name__ == "__main__":
    main()
