"""asvd.py — the reference CLI (asvd.py:14-201) on the MI355X hot path.  Same flags, same pipeline order:
load model -> calibration data -> calib_input_distribution -> sensitivity sweep -> binary search + decomposition -> eval.

Additive flags only: --calib_dataset synthetic (no network in this image), --random_init <hf config name|json> to build a
shape-faithful randomly initialised model when no checkpoint is on disk, --exclude_lm_head, --dist (torchrun: one rank per
GPU, layers sharded, RCCL all-gather of sensitivities), --model_dtype float16|bfloat16 (the dtype the model is loaded in; float16 is the
reference's)."""
import argparse
import os

import numpy as np
import torch


MODEL_DTYPES = {"float16": torch.float16, "bfloat16": torch.bfloat16}


def build_model(args):
    from transformers import AutoConfig, AutoModelForCausalLM, AutoTokenizer
    tokenizer = None
    dtype = MODEL_DTYPES[getattr(args, "model_dtype", "float16")]
    if args.random_init:
        from asvd4llm_amd.model_zoo import random_init_model
        # synthetic weights are created on the GPU (seconds instead of ~2 minutes for a 7B-shaped model); ASVD_INIT_ON_CPU=1 keeps the host stream
        init_dev = None if os.environ.get("ASVD_INIT_ON_CPU") == "1" or not torch.cuda.is_available() else "cuda"
        model = random_init_model(args.model_id, dtype=dtype, device=init_dev)
    else:
        tokenizer = AutoTokenizer.from_pretrained(args.model_id, trust_remote_code=True)
        model = AutoModelForCausalLM.from_pretrained(args.model_id, torch_dtype=dtype, trust_remote_code=True)
    dev = torch.device("cuda", torch.cuda.current_device())
    model = model.to(dev)
    return model, tokenizer


def check_weight_quant_args(args):
    """flag combinations that are errors whatever the model; called before anything is loaded"""
    if getattr(args, "weight_quant_mse", False) and not args.weight_quant.startswith("rtn_"):
        raise ValueError(f"--weight_quant_mse is the clip search of the RTN quantizer: it needs --weight_quant rtn_int8, rtn_int6 or rtn_int4 "
                         f"(got --weight_quant {args.weight_quant})")


def run_weight_quant(model, args):
    """--weight_quant (asvd.py:49-58 of the reference), after the search and the factor gather.  Under --dist with --gather_factors rank0 only
    rank 0 holds the complete model; the other ranks stop before evaluation, so only rank 0 quantizes.  The result is per row (or per group of
    a row, --weight_quant_group_size), so it does not depend on which rank computes it."""
    if args.weight_quant.startswith("awq"):
        raise NotImplementedError(f"--weight_quant {args.weight_quant} needs the `awq` package (AutoAWQ), which this build does not provide; "
                                  "use rtn_int8, rtn_int6 or rtn_int4 (with --weight_quant_group_size 128)")
    bits = {"rtn_int8": 8, "rtn_int6": 6, "rtn_int4": 4}[args.weight_quant]
    storage = getattr(args, "weight_quant_storage", "fake")
    group = int(getattr(args, "weight_quant_group_size", 0) or 0)
    if group not in (0, 64, 128):
        raise ValueError(f"--weight_quant_group_size must be 0, 64 or 128 (got {group})")
    kw = {"group_size": group} if group else {}   # per row: exactly the calls made before the flag existed
    if getattr(args, "weight_quant_mse", False):
        kw["mse"] = True
    if storage == "bitpacked" and bits == 8:
        raise ValueError("--weight_quant_storage bitpacked with rtn_int8: 8-bit codes are already one per byte: use packed")
    if args.dist and args.gather_factors == "rank0" and int(os.environ.get("RANK", "0")) != 0:
        return
    if storage == "bitpacked":
        # ... with the codes stored at their own width (WBLinear modules: 6 or 4 bits per weight; the same weights and, at decode sizes, the
        # same output bits as `packed`)
        from asvd4llm_amd.quantization import rtn_pack_sequential
        rtn_pack_sequential(model, bits, storage="bits", **kw)
        return
    if storage == "packed":
        # the same quantization with the weights kept as uint8 codes (W8Linear modules, W8A16 forward kernel at decode sizes)
        from asvd4llm_amd.quantization import rtn_pack_sequential
        rtn_pack_sequential(model, bits, **kw)
        return
    from asvd4llm_amd.quantization import rtn_quant_sequential
    rtn_quant_sequential(model, bits, **kw)


def run_kv_cache_decode(model, calib_loader, args):
    """--kv_cache_decode_tokens N: what the compressed k_proj / v_proj buy at run time.  Prints the bytes one token occupies in the ordinary
    and in the low-rank KV cache (all layers), then greedy-decodes N tokens from the first calibration sample on both caches (K20 on the low-rank
    one, asvd4llm_amd/kv_cache.py) and prints the largest difference of their logits.  --kv_cache_quant int8 adds the int8 form of the low-rank
    cache (K21): its bytes per token, and the same forced token stream decoded on it.  One line says which route the decode steps on the
    low-rank cache take: the kernel, or the reason LowRankKVAttention refuses it (a bf16 model: "not fp16" unless ASVD_KV_BF16=1, K22)."""
    from asvd4llm_amd.kv_cache import decode_routes, greedy_decode, is_llama_family, kv_ranks
    from asvd4llm_amd.ops import lowrank_kv_groups
    dense = 0
    ranks, pairs = {}, {}
    for name, m in model.named_modules():
        if name.endswith(("k_proj", "v_proj")):
            width = m.ALinear.out_features if hasattr(m, "ALinear") else m.out_features
            dense += 2 * width
            ranks.setdefault(name.rsplit(".", 1)[0], []).append(m.BLinear.out_features if hasattr(m, "BLinear") else width)
            pairs.setdefault(name.rsplit(".", 1)[0], []).append(hasattr(m, "BLinear") and hasattr(m, "ALinear"))
    pairs = [all(v) for v in pairs.values()]   # a layer is cached low-rank (and quantised) where k_proj and v_proj are both factor pairs
    ranks = kv_ranks(model) if is_llama_family(model) else [tuple(v) for v in ranks.values()]   # the runner's cache: what is realised
    low = 2 * sum(sum(r) for r in ranks)
    print(f"kv cache ranks (k, v) per layer: {ranks}")
    print(f"kv cache bytes per token: dense {dense}, low-rank {low} (ratio {low / max(dense, 1):.4f})")
    int8 = getattr(args, "kv_cache_quant", "none") == "int8"
    if int8 and any(p and (r[0] % 16 or r[1] % 16) for p, r in zip(pairs, ranks)):
        print("kv cache int8: the format needs ranks that are multiples of 16 (--rank_align 16); skipped")
        int8 = False
    if int8:   # a byte per code and an fp32 scale per 32 columns where the layer is low-rank, fp16 K and V elsewhere
        low8 = sum(sum(w + 4 * lowrank_kv_groups(w) for w in r) if p else 2 * sum(r) for p, r in zip(pairs, ranks))
        print(f"kv cache bytes per token: int8 low-rank {low8} (ratio {low8 / max(dense, 1):.4f} of dense, {low8 / max(low, 1):.4f} of low-rank); "
              f"int8 layers: {[i for i, p in enumerate(pairs) if p]}")
    if not is_llama_family(model):
        print("kv cache decode: the greedy runner serves Llama-family models only; this model is served at the LowRankKVAttention level")
        return
    ids = calib_loader[0]["input_ids"][:, :64].to(next(model.parameters()).device)
    n = int(args.kv_cache_decode_tokens)
    routes = decode_routes(model)
    print("kv cache decode route: " + ", ".join(f"{r} ({routes.count(r)} layers)" for r in dict.fromkeys(routes))
          + "  [kernel: K20 on the low-rank cache; anything else names why a layer's decode steps stay in torch"
          + ("; a bf16 model takes the kernel with ASVD_KV_BF16=1" if "not fp16" in routes else "") + "]")
    toks_low, logits_low = greedy_decode(model, ids, n, cache="lowrank")
    toks_dense, logits_dense = greedy_decode(model, ids, n, cache="dense", forced=toks_low)
    diff = (logits_low.float() - logits_dense.float()).abs().max().item()
    print(f"kv cache decode: {n} tokens, largest logit difference {diff:.4e} (largest logit {logits_dense.float().abs().max().item():.4e}), "
          f"tokens equal: {bool((toks_low == toks_dense).all())}")
    if int8:
        toks_q8, logits_q8 = greedy_decode(model, ids, n, cache="lowrank", forced=toks_low, kv_quant="int8")
        diff8 = (logits_q8.float() - logits_dense.float()).abs().max().item()
        print(f"kv cache decode, int8 low-rank cache: {n} tokens, largest logit difference {diff8:.4e} against the dense cache "
              f"(fp16 low-rank cache: {diff:.4e}), tokens equal: {bool((toks_q8 == toks_dense).all())}")


def main(args):
    check_weight_quant_args(args)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    torch.cuda.manual_seed_all(args.seed)

    if args.dist:
        import torch.distributed as dist
        local_rank = int(os.environ.get("LOCAL_RANK", 0))
        torch.cuda.set_device(local_rank % max(1, torch.cuda.device_count()))  # gloo: several ranks may share a GPU
        dist.init_process_group(args.dist_backend)  # "nccl" = RCCL over xGMI; "gloo": CPU rendezvous (several ranks on one GPU, tests)

    from asvd4llm_amd.act_aware_utils import calib_fisher_info, calib_input_distribution
    from asvd4llm_amd.binary_search import binary_search_truncation_rank
    from asvd4llm_amd.datautils import get_calib_data
    from asvd4llm_amd.evaluate_utils import evaluate_model
    from asvd4llm_amd.sensitivity import calib_sensitivity_ppl, calib_sensitivity_stable_rank

    model, tokenizer = build_model(args)
    if args.exclude_lm_head:
        from asvd4llm_amd.model_zoo import hide_lm_head
        hide_lm_head(model)

    if not args.raw_model:
        calib_loader = get_calib_data(args.calib_dataset, tokenizer, args.model_id, args.n_calib_samples, seed=args.seed, use_bos=args.use_bos,
                                      vocab_size=model.config.vocab_size)
        if "fisher" in args.scaling_method:
            calib_fisher_info(model, calib_loader, args.use_cache)
        if "abs" in args.scaling_method:
            calib_input_distribution(model, calib_loader, args.scaling_method, args.use_cache, shard_samples=args.shard_calib)
        if args.sensitivity_metric == "ppl":
            sensitivity = calib_sensitivity_ppl(model, calib_loader, args, args.use_cache)
        elif args.sensitivity_metric == "stable_rank":
            sensitivity = calib_sensitivity_stable_rank(model, calib_loader, args, args.use_cache)

        binary_search_truncation_rank(model, sensitivity, calib_loader, args)

        if args.weight_quant != "none":
            run_weight_quant(model, args)

        if getattr(args, "kv_cache_decode_tokens", 0) > 0 and (not args.dist or int(os.environ.get("RANK", "0")) == 0):
            run_kv_cache_decode(model, calib_loader, args)

        if args.save_repo and (not args.dist or int(os.environ.get("RANK", "0")) == 0):
            # exported-repo layout of huggingface_repos/build_asvd_repo.py:58-92 (truncation_ranks + ALinear/BLinear keys)
            from asvd4llm_amd.export import save_asvd_repo
            ranks = save_asvd_repo(model, args.save_repo, tokenizer if hasattr(tokenizer, "save_pretrained") else None)
            print(f"saved ASVD repo with {len(ranks)} factorised layers to {args.save_repo}")

    if args.dist and int(os.environ.get("RANK", "0")) != 0 and args.gather_factors != "all":
        # only rank 0 holds the complete compressed model (factors gathered point-to-point): it alone evaluates and reports
        import torch.distributed as dist
        dist.destroy_process_group()  # no collective follows the factor exchange
        return
    eval_ids = torch.cat([_["input_ids"] for _ in calib_loader], 0) if (not args.raw_model and args.calib_dataset == "synthetic") else None
    result = evaluate_model(model, tokenizer, args.model_id, "mmlu" if args.eval_mmlu else args.eval_tasks, eval_ppl=args.eval_ppl, limit=-1,
                            use_bos=args.use_bos, eval_ids=eval_ids)
    print(result)
    if not args.dist or int(os.environ.get("RANK", "0")) == 0:
        if not os.path.exists("output"):
            os.makedirs("output")
        with open("output/result.txt", "a+") as f:
            f.write(f"{args}\n")
            f.write(f"{result}\n")
    if args.dist:
        import torch.distributed as dist
        if dist.is_initialized():
            dist.destroy_process_group()


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument("--model_id", type=str, default="facebook/opt-1.3b", help="Pretrained model ID")
    parser.add_argument("--ppl_target", type=float, default=-1, help="target ppl")
    parser.add_argument("--param_ratio_target", type=float, default=-1, help="target param ratio")
    parser.add_argument("--act_aware", action="store_true", help="use act aware svd (ASVD)")
    parser.add_argument("--alpha", type=float, default=0.5, help="hyper-parameter alpha for ASVD")
    parser.add_argument("--n_calib_samples", type=int, default=32, help="number of samples used for calibration")
    parser.add_argument("--calib_dataset", type=str, default="wikitext2",
                        choices=["wikitext2", "c4", "ptb", "alpaca", "selfgen", "synthetic"], help="calibration dataset")
    parser.add_argument("--scaling_method", type=str, default="abs_mean", choices=["abs_mean", "abs_max", "fisher", "fisher_abs_mean"],
                        help="scaling method")
    parser.add_argument("--sensitivity_metric", type=str, default="ppl", choices=["ppl", "stable_rank"], help="search metric")
    parser.add_argument("--use_cache", action="store_true", help="use cached calibration results")
    parser.add_argument("--weight_quant", type=str, default="none", choices=["none", "rtn_int8", "rtn_int6", "rtn_int4", "awq_int8", "awq_int4"],
                        help="weight quantization method")
    parser.add_argument("--weight_quant_storage", type=str, default="fake", choices=["fake", "packed", "bitpacked"],
                        help="rtn_int8 / rtn_int6 / rtn_int4: `fake` writes the quantized weights back in their dtype (the reference's behaviour); `packed` keeps "
                             "them as uint8 codes with per-row fp32 scale and zero (one byte per weight, also for int6) and runs decode-sized "
                             "inputs on the W8A16 kernel; `bitpacked` (rtn_int6 / rtn_int4) stores the codes at 6 / 4 bits per weight and runs the kernel "
                             "that unpacks them in registers; all three stand for the same weights bit for bit")
    parser.add_argument("--weight_quant_group_size", type=int, default=0, choices=[0, 64, 128],
                        help="rtn_*: 0 keeps one scale and zero per output row (the reference's RTN); 64 / 128 keep one pair per group of that many "
                             "input columns (8 bytes per group: 4.5 bits per weight for rtn_int4 with 128), which about halves the quantization "
                             "error of the ASVD factor pairs and is what makes rtn_int4 usable; valid with every storage")
    parser.add_argument("--weight_quant_mse", action="store_true",
                        help="rtn_*: take every scale and zero from the clip search of the reference's Quantizer (mse=True: 80 shrunk ranges per row "
                             "or group, the smallest sum |q(x) - x|^2.4 wins) instead of the plain min / max; valid with every storage and group "
                             "size, an error with awq_* or without --weight_quant")
    parser.add_argument("--eval_mmlu", action="store_true", help="evaluate mmlu")
    parser.add_argument("--eval_ppl", default="wikitext2,ptb", type=str)
    parser.add_argument("--eval_tasks", type=str, default="")
    parser.add_argument("--sigma_fuse", type=str, default="UV", help="sigma fuse method", choices=["U", "V", "UV"])
    parser.add_argument("--seed", type=int, default=233, help="random seed, which can significantly affect the calibration results")
    parser.add_argument("--compress_kv_cache", action="store_true", help="compress kv cache by asvd for k_proj and v_proj")
    parser.add_argument("--kv_cache_ratio_target", type=float, default=-1, help="kv cache ratio")
    parser.add_argument("--rank_align", type=int, default=1, help="align rank in SVD")
    parser.add_argument("--raw_model", action="store_true", help="use the raw model without ASVD")
    parser.add_argument("--use_bos", action="store_true", help="use bos token in calibration")
    # ---- additive, build-only flags ----
    parser.add_argument("--random_init", action="store_true", help="shape-faithful random-init model named by --model_id (no checkpoints offline)")
    parser.add_argument("--model_dtype", type=str, default="float16", choices=sorted(MODEL_DTYPES),
                        help="dtype the model is loaded in (float16: the reference's behaviour).  A bfloat16 model packs (--weight_quant_storage) into "
                             "modules with weight_dtype bfloat16, whose bf16 inputs take the packed kernels once ASVD_PACKED_BF16=1 switches them on")
    parser.add_argument("--svd_ortho", action="store_true",
                        help="re-orthonormalise the long side's singular vectors after every factorisation (K18: U = W V / sigma loses orthogonality on "
                             "graded spectra, 2e-3 .. 2.5e-2 measured); matters under --sigma_fuse U / V, where one emitted factor is the raw vector "
                             "matrix.  Off by default; ASVD_SVD_ORTHO=1 is the environment switch of the library")
    parser.add_argument("--kv_cache_decode_tokens", type=int, default=0,
                        help="after the compression print the bytes per token of the ordinary and of the low-rank KV cache (k_proj / v_proj kept as "
                             "their r-wide BLinear outputs) and greedy-decode this many tokens on both (Llama-family models; the low-rank cache runs "
                             "the K20 decode-attention kernel where it serves the shape).  0 (default): nothing happens")
    parser.add_argument("--kv_cache_quant", choices=["none", "int8"], default="none",
                        help="read by the --kv_cache_decode_tokens report only.  int8: also print the bytes per token of the int8 low-rank cache (K21: "
                             "8-bit codes and one fp32 scale per token and 32 latent columns) and decode the same token stream on it")
    parser.add_argument("--exclude_lm_head", action="store_true", help="do not hook/sweep/compress lm_head (the reference includes it)")
    parser.add_argument("--save_repo", type=str, default="", help="write the compressed model in the exported HF-repo layout of the reference (truncation_ranks in config.json)")
    parser.add_argument("--no_fused_sweep", dest="fused_sweep", action="store_false",
                        help="evaluate every (layer, ratio) with full model forwards as the reference does (default: prefix-cached evaluator, same values)")
    parser.add_argument("--no_fused_ratios", dest="fused_ratios", action="store_false",
                        help="evaluate every candidate ratio of a layer in its own suffix pass (default: all ratios as one batched pass; "
                             "same search trace, perplexities equal to ~1e-4 relative in fp16)")
    parser.add_argument("--sweep_samples_per_pass", type=int, default=1,
                        help="calibration samples per batched suffix pass of the sensitivity sweep (ratios x samples rows per GEMM).  1 (default) keeps the "
                             "perplexities and the search trace of rounds 2-5 bit for bit; 4 shortens the Llama-2-7B-shaped sweep by 6.5 %% (712 vs 762 s, "
                             "profiles/r6_e2e_llama2_7b_ncalib32_*.json) with the same per-sample arithmetic on 4x taller GEMMs: perplexities equal to "
                             "<= 5e-4 relative in fp16, which can reorder near-tied layers in the search")
    parser.add_argument("--gather_factors", type=str, default="rank0", choices=["rank0", "all", "none"],
                        help="--dist: after the sharded decomposition send every layer's A/B factors to rank 0 (point-to-point), to all ranks "
                             "(broadcast), or nowhere")
    parser.add_argument("--dist", action="store_true", help="torchrun launch: one rank per GPU, layers sharded, RCCL all-gather of sensitivities")
    parser.add_argument("--dist_backend", type=str, default="nccl", choices=["nccl", "gloo"],
                        help="--dist: process-group backend; nccl is RCCL over xGMI (one rank per GPU), gloo lets several ranks share one GPU")
    parser.add_argument("--shard_calib", action="store_true",
                        help="--dist: every rank runs the calibration hook pass over its own samples and the [C] accumulators are all-reduced "
                             "(default: replicated pass, identical statistics without a collective)")
    return parser


if __name__ == "__main__":
    main(build_parser().parse_args())
