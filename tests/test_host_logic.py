"""Host-side logic of the package (traversal order, search, sharding map) against the reference-generated fixtures. CPU only."""
import contextlib
import io
import types

import pytest
import torch
import torch.nn as nn

from asvd4llm_amd import parallel
from asvd4llm_amd.modules.svd_linear import SVDLinear
from asvd4llm_amd.sensitivity import collect_linear_info
from tests.tiny_lm import TinyLM, default_args, load_golden_tiny


def test_reverse_dfs_order_tiny(golden):
    t = golden.json("tiny_lm.json")
    model, _ = load_golden_tiny(golden)
    order = [i["full_name"] for i in collect_linear_info(model).values()]
    assert order == t["order"]
    assert order[0] == "lm_head" and order[1].startswith("model.layers.1.mlp")


def test_reverse_dfs_order_hf(golden):
    from transformers import LlamaConfig, LlamaForCausalLM, OPTConfig, OPTForCausalLM
    ref = golden.json("linear_order_hf.json")
    llama = LlamaForCausalLM(LlamaConfig(hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=2,
                                         vocab_size=64))
    opt = OPTForCausalLM(OPTConfig(hidden_size=32, ffn_dim=64, num_hidden_layers=2, num_attention_heads=2, vocab_size=64, word_embed_proj_dim=32,
                                   max_position_embeddings=64))
    assert [i["full_name"] for i in collect_linear_info(llama).values()] == ref["llama"]
    assert [i["full_name"] for i in collect_linear_info(opt).values()] == ref["opt"]


def test_compute_rank_matches_reference_table(golden):
    t = golden.json("rank_table.json")
    for out_f, in_f, ratio, align, rank in t["rows"]:
        lin = types.SimpleNamespace(weight=types.SimpleNamespace(numel=lambda o=out_f, i=in_f: o * i), in_features=in_f, out_features=out_f)
        assert SVDLinear.compute_rank(lin, ratio, align) == rank


def _run_search(golden, tag, monkeypatch, **kw):
    from asvd4llm_amd import binary_search as bs
    t = golden.json("tiny_lm.json")
    rec = t["search"][tag]
    model, scal = load_golden_tiny(golden)
    calls = []

    def fake_from_linear(linear, param_ratio, act_aware=False, ic_split=1, oc_split=1, alpha=1, sigma_fuse="UV", rank_align=1):
        r = SVDLinear.compute_rank(linear, param_ratio, rank_align)
        calls.append((param_ratio, act_aware, alpha, sigma_fuse, rank_align))
        m = nn.Identity()
        m.truncation_rank = r
        return m

    monkeypatch.setattr(SVDLinear, "from_linear", staticmethod(fake_from_linear))
    sens = {k: {float(r): v for r, v in d.items()} for k, d in rec["sens"].items()}
    calib = [{"input_ids": torch.tensor(ids)} for ids in t["calib_ids"]]
    args = default_args(offload_raw_to_cpu=False, **kw)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), contextlib.redirect_stderr(io.StringIO()):
        bs.binary_search_truncation_rank(model, sens, calib, args)
    lines = [l for l in buf.getvalue().splitlines() if l.startswith("low=") or l.startswith("===")]
    assert lines == rec["trace"]
    got = {}
    for n, m in model.named_modules():
        if hasattr(m, "truncation_rank"):
            got[n] = m.truncation_rank
        elif isinstance(m, nn.Linear):
            got[n] = -1
    assert got == rec["ranks"]
    assert all(c[1] is True and c[2] == 0.5 and c[3] == "UV" for c in calls)


def test_binary_search_ratio_target(golden, monkeypatch):
    _run_search(golden, "ratio0.8", monkeypatch, param_ratio_target=0.8)


def test_binary_search_ratio_target_2(golden, monkeypatch):
    _run_search(golden, "ratio0.6", monkeypatch, param_ratio_target=0.6)


def test_binary_search_kv_mode(golden, monkeypatch):
    _run_search(golden, "kv0.5", monkeypatch, compress_kv_cache=True, kv_cache_ratio_target=0.5)


@pytest.mark.parametrize("tag", ["ppl54.1", "ppl54.3", "ppl60"])
def test_binary_search_ppl_target_vs_reference(golden, monkeypatch, tag):
    """--ppl_target (binary_search.py:64-87): every probe compresses the WHOLE model to the plan of the cut and measures its perplexity.
    Fixture: the reference's own run on the tiny LM (factorisation patched to the exact one).  Here the factors come from the CPU oracle
    (tests only), so the bisection must walk the same (low, mid, high), see the same perplexities (to 1e-4) and end on the same ranks."""
    from asvd4llm_amd import binary_search as bs
    from tests.tiny_lm import oracle_from_linear, parse_search_trace
    t = golden.json("tiny_lm.json")
    rec = golden.json("search_extra.json")["tiny_ppl_target"][tag]
    model, scal = load_golden_tiny(golden)
    for n, m in model.named_modules():
        if isinstance(m, nn.Linear):
            m.scaling_diag_matrix = scal[n]
    monkeypatch.setattr(SVDLinear, "from_linear", staticmethod(oracle_from_linear))
    monkeypatch.setattr(SVDLinear, "drop_factor_cache", staticmethod(lambda l: None))
    sens = {k: {float(r): v for r, v in d.items()} for k, d in t["sensitivity_ppl"].items()}
    calib = [{"input_ids": torch.tensor(ids)} for ids in t["calib_ids"]]
    args = default_args(offload_raw_to_cpu=False, ppl_target=rec["ppl_target"], param_ratio_target=-1)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), contextlib.redirect_stderr(io.StringIO()):
        bs.binary_search_truncation_rank(model, sens, calib, args)
    lines = [l for l in buf.getvalue().splitlines() if l.startswith("low=") or l.startswith("===")]
    assert [l for l in lines if l.startswith("===")] == [l for l in rec["trace"] if l.startswith("===")]
    got, want = parse_search_trace(lines), parse_search_trace(rec["trace"])
    assert len(got) == len(want) >= 6
    for g, w in zip(got, want):
        assert g[:3] == w[:3] and abs(g[3] - w[3]) <= 1e-4 * w[3] and g[4] == w[4], (g, w)
    ranks = {}
    for n, m in model.named_modules():
        if hasattr(m, "truncation_rank"):
            ranks[n] = m.truncation_rank
        elif isinstance(m, nn.Linear):
            ranks[n] = -1
    assert ranks == rec["ranks"]
    from asvd4llm_amd.evaluate_utils import evaluate_perplexity
    ids = torch.cat([c["input_ids"] for c in calib], 0)
    assert abs(evaluate_perplexity(model, ids, 3) - rec["ppl_after"]) <= 1e-4 * rec["ppl_after"]


@pytest.mark.parametrize("tag", ["ratio0.9", "ratio0.95", "ratio0.8"])
def test_binary_search_at_model_scale_vs_reference(golden, monkeypatch, tag):
    """The search over the 1350 candidates of a Llama-2-7B-shaped model (225 Linears x 6 ratios, many exact ties in the sensitivities): the
    trace lines — float sums included — and the plan of the last probed cut must be the reference's, character for character."""
    from asvd4llm_amd import binary_search as bs
    from tests.tiny_lm import ShapedLlama
    fx = golden.json("search_extra.json")["llama7b_shaped"]
    rec = fx["runs"][tag]
    model = ShapedLlama(**{k: fx["shape"][k] for k in ("hidden", "inter", "layers", "vocab")})
    from asvd4llm_amd.sensitivity import collect_linear_info
    assert [i["full_name"] for i in collect_linear_info(model).values()] == fx["order"]

    def recorder(linear, param_ratio, act_aware=False, ic_split=1, oc_split=1, alpha=1, sigma_fuse="UV", rank_align=1):
        m = nn.Identity()
        m.param_ratio = param_ratio
        return m

    monkeypatch.setattr(SVDLinear, "from_linear", staticmethod(recorder))
    monkeypatch.setattr(SVDLinear, "drop_factor_cache", staticmethod(lambda l: None))
    sens = {k: {float(r): v for r, v in d.items()} for k, d in fx["sens"].items()}
    args = default_args(offload_raw_to_cpu=False, param_ratio_target=rec["param_ratio_target"])
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), contextlib.redirect_stderr(io.StringIO()):
        bs.binary_search_truncation_rank(model, sens, [{"input_ids": torch.zeros(1, 4, dtype=torch.long)}], args)
    lines = [l for l in buf.getvalue().splitlines() if l.startswith("low=") or l.startswith("===")]
    assert lines == rec["trace"]
    plan = {n: m.param_ratio for n, m in model.named_modules() if hasattr(m, "param_ratio")}
    assert plan == rec["plan"]


def test_lpt_assign_balanced_and_deterministic():
    costs = [parallel.svd_flops(32000, 4096)] + [parallel.svd_flops(*s) for _ in range(32)
                                                   for s in [(11008, 4096), (11008, 4096), (4096, 11008), (4096, 4096), (4096, 4096),
                                                             (4096, 4096), (4096, 4096)]]
    assert len(costs) == 225
    own = parallel.lpt_assign(costs, 8)
    assert own == parallel.lpt_assign(list(costs), 8)
    load = [sum(c for c, o in zip(costs, own) if o == r) for r in range(8)]
    assert max(load) / (sum(load) / 8) < 1.05
    assert abs(sum(costs) - 5.026e14) / 5.026e14 < 1e-3  # SURVEY.md §8d whole-model flop figure
    assert parallel.lpt_assign(costs, 1) == [0] * 225


def test_perplexity_quirk_matches_reference(golden):
    from asvd4llm_amd.evaluate_utils import evaluate_perplexity
    t = golden.json("tiny_lm.json")
    model, _ = load_golden_tiny(golden)
    ids = torch.cat([torch.tensor(i) for i in t["calib_ids"]], 0)
    ppl = evaluate_perplexity(model, ids, 3)
    assert abs(ppl - t["ppl_raw"]) <= 1e-5 * t["ppl_raw"]


def test_sweep_shard_is_balanced_on_the_sweep_cost_model():
    """configs[3] / [4] are 99 % sweep: the LPT shard of calib_sensitivity_ppl must be balanced on the predicted sweep seconds per layer (suffix
    forwards behind the layer + its factorisation), not on SVD flops.  Llama-2-7B / 13B shapes at 8 ranks: max / mean <= 1.05."""
    import bench
    table = bench.predicted_sweep_balance(8)
    for name in ("llama-2-7b", "llama-2-13b"):
        rec = table[name]
        assert rec["sweep_s_max_over_mean"] <= 1.05, rec
        assert rec["decompose_flops_max_over_mean"] <= 1.05, rec
        assert rec["predicted_sweep_s_per_rank_max"] <= 1.05 * rec["predicted_sweep_s_one_gpu"] / 8
    # the model reproduces the measured one-GPU sweep of round 4 (755 s of forwards + factorisations, profiles/r4_e2e_llama2_7b_ncalib32.json) to 5 %
    assert abs(table["llama-2-7b"]["predicted_sweep_s_one_gpu"] - 755.0) / 755.0 < 0.05
    # structure of the cost: lm_head replays nothing, a layer of block 0 replays the whole model, a layer of the last block one block
    costs = bench.model_sweep_costs("llama-2-7b")
    names = [n for n, _, _ in bench.model_linears("llama-2-7b")]
    c = dict(zip(names, costs))
    assert c["model.layers.0.self_attn.q_proj"] > 15 * c["model.layers.31.self_attn.q_proj"] > 0
    assert c["lm_head"] < c["model.layers.31.mlp.down_proj"]


def test_sweep_costs_for_model_reads_the_block_structure():
    """the model-based wrapper (what calib_sensitivity_ppl calls) on the tiny Llama: deeper blocks are cheaper, the head is cheapest, every
    rank computes the same owner map"""
    from asvd4llm_amd.sensitivity import collect_linear_info
    from tests.tiny_lm import ShapedLlama
    model = ShapedLlama(hidden=64, inter=176, layers=3, vocab=320)
    linears = list(collect_linear_info(model).items())
    costs = parallel.sweep_costs_for_model(model, linears, 6, 4, 128)
    by = {info["full_name"]: c for (_, info), c in zip(linears, costs)}
    assert by["model.layers.0.mlp.up_proj"] > by["model.layers.1.mlp.up_proj"] > by["model.layers.2.mlp.up_proj"] > by["lm_head"] > 0
    assert parallel.lpt_assign(costs, 2) == parallel.lpt_assign(list(costs), 2)
    flat = parallel.sweep_costs_for_model(model, linears, 6, 4, 128, prefix_cached=False)
    assert max(flat) / min(flat) < 1.5   # full forwards: every evaluation costs the same, only the factorisations differ


def test_every_profile_path_a_bench_string_cites_exists():
    """`roofline.traffic_source` pointed at profiles/r5f_pmc_*.txt, files that were committed under another name.  Every
    `profiles/...` path (or glob) that bench.py can print, and the `source` of profiles/pmc_traffic.json, must resolve in the tree."""
    import glob
    import json
    import os
    import re
    from tests.conftest import ROOT
    cited = set(re.findall(r"profiles/[A-Za-z0-9_.*\-]+", open(os.path.join(ROOT, "bench.py")).read()))
    pmc = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))
    cited |= set(re.findall(r"profiles/[A-Za-z0-9_.*\-]+", pmc.get("source", "")))
    cited = {c.rstrip(".") for c in cited}
    assert cited, "bench.py cites its evidence"
    missing = sorted(c for c in cited if not glob.glob(os.path.join(ROOT, c)))
    assert not missing, f"bench.py / pmc_traffic.json cite files that are not in the tree: {missing}"


def test_decomposition_follows_the_sweep_owner_map_only_while_the_factor_caches_exist():
    """the sweep's shard is balanced on suffix-forward seconds (late-block layers are cheap: their owners hold many more layers), which
    is the right map for the final decomposition only while the sweep's factorisations are still cached with those owners.  With keep_svd_cache
    off, other arguments, or another world size the decomposition is balanced on its own cost, the SVD flops."""
    import types
    import torch.nn as nn
    from asvd4llm_amd import parallel
    from asvd4llm_amd.binary_search import _decompose_owner_map
    lins = [nn.Linear(64, 64, bias=False) for _ in range(6)] + [nn.Linear(64, 176, bias=False) for _ in range(3)]
    info = {l: {"full_name": f"l{i}"} for i, l in enumerate(lins)}
    flops_map = {f"l{i}": o for i, o in enumerate(parallel.lpt_assign([parallel.svd_flops(l.out_features, l.in_features) for l in lins], 2))}
    sweep_map = {f"l{i}": (0 if i < 2 else 1) for i in range(9)}      # deliberately lopsided
    assert sweep_map != flops_map
    args = types.SimpleNamespace(alpha=0.5, scaling_method="abs_mean", shard_decompose=True)
    model = types.SimpleNamespace()
    assert _decompose_owner_map(model, info, args, 2, True) == flops_map                       # no sweep ran in this process
    model._asvd_sweep_owner = dict(sweep_map)
    assert _decompose_owner_map(model, info, args, 2, True) == flops_map                       # a map without the record of what was kept: not trusted
    model._asvd_sweep_owner_meta = {"factors_kept": True, "alpha": 0.5, "scaling_method": "abs_mean", "world_size": 2}
    assert _decompose_owner_map(model, info, args, 2, True) == sweep_map                       # caches live: follow the sweep's owners
    model._asvd_sweep_owner_meta["factors_kept"] = False
    assert _decompose_owner_map(model, info, args, 2, True) == flops_map                       # --no keep_svd_cache: every layer is re-factorised
    model._asvd_sweep_owner_meta = {"factors_kept": True, "alpha": 1.0, "scaling_method": "abs_mean", "world_size": 2}
    assert _decompose_owner_map(model, info, args, 2, True) == flops_map                       # stale: the model was swept with another alpha
    model._asvd_sweep_owner_meta = {"factors_kept": True, "alpha": 0.5, "scaling_method": "abs_mean", "world_size": 4}
    assert _decompose_owner_map(model, info, args, 2, True) == flops_map                       # stale: another world size


def test_sweep_rank_hint_is_the_rank_of_the_largest_candidate_ratio():
    """the k every factorisation of the sweep asks for (tests/test_gpu_svd_topk.py takes it from here): the largest candidate rank, which is the
    oracle's rank at the largest candidate ratio, aligned or not"""
    from oracle import asvd_oracle as O
    from tests.test_gpu_svd_topk import sweep_ranks
    for m, n in ((1024, 1024), (2048, 2048), (4096, 4096), (11008, 4096), (4096, 11008), (5120, 5120), (13824, 5120), (32000, 4096)):
        for align in (1, 128):
            k, R = sweep_ranks(m, n, align)
            assert k == max(R) == O.rank_from_ratio(m, n, 0.9, align) and len(R) >= 3
    assert sweep_ranks(4096, 4096)[0] == 1843 and sweep_ranks(4096, 11008)[0] == 2686 and sweep_ranks(4096, 4096, 128)[0] == 1920
