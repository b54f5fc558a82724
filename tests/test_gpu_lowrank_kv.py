"""K20 on the device: decode attention on a low-rank KV cache (csrc/lowrank_kv.hip) against the fp64 restatement
(tests/lowrank_kv_restate.py), bit-exact scores on integer data, padding, isolation, strides, the modules and the CLI."""
import copy
import json
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import exact_data as X
from tests import lowrank_kv_restate as R
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

HEADS = [(1, 1), (12, 12), (12, 3), (32, 32), (32, 8), (40, 40), (40, 10)]   # (H, H_kv): below / at / above one 32-head block, H_kv = H and H / 4
FLOOR = 2.0 ** -9    # three fp16 roundings on the kernel's path (q~ or nothing, p, the output), each <= 2^-11 relative
SEEN = {"e_kernel": 0.0, "e_dense": 0.0}


def _plan(B, H, Tmax):
    from asvd4llm_amd import ops
    return ops.lowrank_kv_plan(B, H, Tmax)


# ---- 1. exact scores --------------------------------------------------------------------------------------------------------------------

def _exact_scores_case(dev, H, H_kv, D, r_k, Tmax, scale, mode, seed):
    from asvd4llm_amd import ops
    g = torch.Generator().manual_seed(seed)
    B = 3
    q = X._ints(g, -3, 3, (B, H, D)).half()
    ck = X._ints(g, -3, 3, (B, Tmax, r_k)).half()
    Ak = X._ints(g, -1, 1, (H_kv * D, r_k)).half()
    lens = [Tmax, Tmax // 2, max(Tmax - 1, 0)]
    rope = None
    if mode == "half":
        idx = torch.randint(0, 4, (Tmax, D // 2), generator=g)
        rope = (torch.tensor([1.0, 0.0, -1.0, 0.0])[idx], torch.tensor([0.0, 1.0, 0.0, -1.0])[idx])   # exact signed permutations
    # integer arithmetic (fp64 holds every value below 2^53 exactly; converted to int64 at the end)
    grp = H // H_kv
    Kabs = (ck.double().abs() @ Ak.double().abs().T).view(B, Tmax, H_kv, D)
    qt_abs = torch.einsum("bhd,hdr->bhr", q.double().abs(), Ak.double().abs().view(H_kv, D, r_k).repeat_interleave(grp, 0))
    pre = {"max |q~| (fp16 exact)": (qt_abs.max().item(), 2049.0),
           "max sum |q||K|": (torch.einsum("bhd,bthd->bht", q.double().abs(), Kabs.repeat_interleave(grp, 2)).max().item(), X.LIMIT),
           "max sum |q~||C_k|": (torch.einsum("bhr,btr->bht", qt_abs, ck.double().abs()).max().item(), X.LIMIT)}
    X.check_pre(pre)
    S64, live = R.kv_scores(q, ck, lens, Ak, H_kv, 1.0, None, rope)
    S_int = S64.to(torch.int64)
    assert torch.equal(S_int.double(), S64)
    expect = (S_int.double() * scale).float()
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    got = ops.lowrank_kv_scores(q.to(dev), ck.to(dev), lens_d, Ak.to(dev), H_kv, scale, rope=tuple(t.to(dev) for t in rope) if rope else None)
    assert got.dtype == torch.float32 and got.shape == (B, H, Tmax)
    assert torch.equal(got.cpu(), expect), (H, H_kv, D, r_k, Tmax, scale, mode, (got.cpu() != expect).sum().item())


@pytest.mark.parametrize("mode", ["none", "half"])
@pytest.mark.parametrize("H,H_kv", HEADS)
def test_scores_bit_exact_on_integer_data(gpu, H, H_kv, mode):
    tile, _, _ = _plan(3, H, 64)
    assert tile == 32
    # every T of {1, 2, tile - 1, tile, tile + 1} and the same around the 4-tile workgroup, with D, r_k and the scale rotating through all their values
    Ts = [1, 2, tile - 1, tile, tile + 1, 4 * tile - 1, 4 * tile, 4 * tile + 1]
    off = HEADS.index((H, H_kv)) + (3 if mode == "half" else 0)
    for n, T in enumerate(Ts):
        D = (64, 128)[(n + off) % 2]
        r_k = (16, 48, 272)[(n + off) % 3]
        scale = (1.0, 0.125)[(n // 2 + off) % 2]
        _exact_scores_case(gpu, H, H_kv, D, r_k, T, scale, mode, X.seed_of("k20", H, H_kv, T, mode))


def test_scores_cover_every_listed_size(gpu):
    """the rotation above reaches every D, r_k and scale in both modes (a change of the lists must keep that true)"""
    seen = set()
    for mode in ("none", "half"):
        for H, H_kv in HEADS:
            off = HEADS.index((H, H_kv)) + (3 if mode == "half" else 0)
            for n in range(8):
                seen.add((mode, "D", (64, 128)[(n + off) % 2]))
                seen.add((mode, "r", (16, 48, 272)[(n + off) % 3]))
                seen.add((mode, "s", (1.0, 0.125)[(n // 2 + off) % 2]))
    assert len(seen) == 2 * (2 + 3 + 2)


# ---- 2. the whole op against the restatement ----------------------------------------------------------------------------------------------

def _data(H, H_kv, D, r_k, r_v, Tmax, B, with_bv, seed):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g)
    d = dict(q=rnd(B, H, D).half(), ck=rnd(B, Tmax, r_k).half(), cv=rnd(B, Tmax, r_v).half(), Ak=(rnd(H_kv * D, r_k) / r_k ** 0.5).half(),
             Av=(rnd(H_kv * D, r_v) / r_v ** 0.5).half(), bv=rnd(H_kv * D).half() if with_bv else None)
    return d


def _dense_route(d, lens, H_kv, scale, rope):
    """existing code, not the code under test: fp16 F.linear reconstruction of K and V, torch SDPA in fp16 (one sequence at a time, so
    that an empty sequence needs no mask)"""
    B, H, D = d["q"].shape
    out = torch.zeros(B, H, D, dtype=torch.float16, device=d["q"].device)
    for b in range(B):
        T = lens[b]
        if T == 0:
            continue
        K = F.linear(d["ck"][b, :T], d["Ak"]).view(T, H_kv, D)
        V = F.linear(d["cv"][b, :T], d["Av"], d["bv"]).view(T, H_kv, D)
        if rope is not None:
            K = R.rotate_half_table(K.float().transpose(0, 1), rope[0][:T], rope[1][:T]).transpose(0, 1).half()
        K, V = K.transpose(0, 1).repeat_interleave(H // H_kv, 0), V.transpose(0, 1).repeat_interleave(H // H_kv, 0)
        out[b] = F.scaled_dot_product_attention(d["q"][b][None, :, None, :], K[None], V[None], scale=scale)[0, :, 0]
    return out


def _run(dev, d, lens, H_kv, scale, rope, **kw):
    from asvd4llm_amd import ops
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    return ops.lowrank_kv_decode(d["q"], d["ck"], d["cv"], lens_d, d["Ak"], d["Av"], H_kv, scale, bv=d["bv"], rope=rope, **kw)


def _whole_op(dev, H, H_kv, D, r_k, r_v, Tmax, lens, with_bv, mode, seed):
    from asvd4llm_amd import ops
    d = _data(H, H_kv, D, r_k, r_v, Tmax, len(lens), with_bv, seed)
    scale = D ** -0.5
    rope = ops.rope_table(Tmax, D, 10000.0) if mode == "half" else None
    ref = R.kv_decode(d["q"], d["ck"], d["cv"], lens, d["Ak"], d["Av"], H_kv, scale, None, d["bv"], rope)
    dd = {k: (v.to(dev) if v is not None else None) for k, v in d.items()}
    rope_d = tuple(t.to(dev) for t in rope) if rope else None
    out = _run(dev, dd, lens, H_kv, scale, rope_d)
    dense = _dense_route(dd, lens, H_kv, scale, rope_d)
    top = ref.abs().max().item()
    e_k = (out.double().cpu() - ref).abs().max().item() / top
    e_d = (dense.double().cpu() - ref).abs().max().item() / top
    print(f"K20 H={H} H_kv={H_kv} D={D} r=({r_k},{r_v}) Tmax={Tmax} lens={lens} bv={with_bv} {mode}: e_kernel={e_k:.3e} e_dense={e_d:.3e}")
    SEEN["e_kernel"], SEEN["e_dense"] = max(SEEN["e_kernel"], e_k), max(SEEN["e_dense"], e_d)
    for b, n in enumerate(lens):
        if n == 0:
            assert torch.equal(out[b].cpu(), torch.zeros(H, D, dtype=torch.float16))
    assert e_k <= max(2 * e_d, FLOOR), (e_k, e_d)
    return dd, rope_d, out


# (H, H_kv, D, r_k, r_v, with_bv, mode): both modes, with and without b_v, r_k != r_v from {16, 80, 272}, every head shape
CONFIGS = [(1, 1, 64, 16, 80, True, "none"), (12, 12, 128, 80, 16, False, "half"), (12, 3, 64, 272, 16, True, "half"), (32, 32, 64, 80, 272, False, "none"),
           (32, 8, 128, 16, 272, True, "none"), (40, 40, 64, 272, 80, True, "half"), (40, 10, 128, 80, 16, False, "none"), (32, 8, 64, 16, 80, False, "half")]


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "-".join(map(str, c)))
def test_whole_op_against_restatement(gpu, cfg):
    H, H_kv, D, r_k, r_v, with_bv, mode = cfg
    Tmax = 130
    tile, L, ns = _plan(3, H, Tmax)
    assert (tile, L, ns) == (32, 64, 3)   # the lengths below sit around these: one below / at / one above the tile and the split
    cases = [[1, tile - 1, tile], [tile + 1, L - 1, L], [L + 1, 2 * L + 1, Tmax], [0, 1, Tmax]]   # L + 1, 2 L + 1: a last split of one token
    for n, lens in enumerate(cases):
        _whole_op(gpu, H, H_kv, D, r_k, r_v, Tmax, lens, with_bv, mode, X.seed_of("k20w", n, *cfg[:5]))
    _whole_op(gpu, H, H_kv, D, r_k, r_v, 1, [1], with_bv, mode, X.seed_of("k20w1", *cfg[:5]))            # B = 1, a buffer of one token
    _whole_op(gpu, H, H_kv, D, r_k, r_v, 33, [33, 32], with_bv, mode, X.seed_of("k20w33", *cfg[:5]))      # a buffer that ends inside a tile


def test_largest_errors_seen(gpu):
    """prints what profiles/lowrank_kv.json and DESIGN.md cite (the bound is asserted per case above)"""
    print("K20_ERRORS " + json.dumps(SEEN))
    assert SEEN["e_kernel"] > 0.0


# ---- 3. padding never leaks -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cfg", [CONFIGS[2], CONFIGS[4]], ids=["half", "none"])
def test_padding_never_leaks(gpu, cfg):
    H, H_kv, D, r_k, r_v, with_bv, mode = cfg
    Tmax, lens = 130, [0, 37, 65]
    dd, rope_d, out = _whole_op(gpu, H, H_kv, D, r_k, r_v, Tmax, lens, with_bv, mode, 77)
    assert torch.equal(out[0], torch.zeros_like(out[0]))
    for fill in (float("nan"), 6e4):
        bad = dict(dd)
        bad["ck"], bad["cv"] = dd["ck"].clone(), dd["cv"].clone()
        for b, n in enumerate(lens):
            bad["ck"][b, n:] = fill
            bad["cv"][b, n:] = fill
        again = _run(gpu, bad, lens, H_kv, D ** -0.5, rope_d)
        assert torch.equal(again.view(torch.int16), out.view(torch.int16)), fill


# ---- 4. isolation and determinism -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cfg", [CONFIGS[2], CONFIGS[3]], ids=["half", "none"])
def test_isolation_determinism_and_streams(gpu, cfg):
    from asvd4llm_amd import ops
    H, H_kv, D, r_k, r_v, with_bv, mode = cfg
    Tmax, lens = 130, [130, 70, 129]
    dd, rope_d, out = _whole_op(gpu, H, H_kv, D, r_k, r_v, Tmax, lens, with_bv, mode, 78)
    scale = D ** -0.5
    assert torch.equal(_run(gpu, dd, lens, H_kv, scale, rope_d).view(torch.int16), out.view(torch.int16))
    bad = dict(dd)
    bad["ck"] = dd["ck"].clone()
    bad["ck"][0, 3, 5] = float("nan")
    o_bad = _run(gpu, bad, lens, H_kv, scale, rope_d)
    assert torch.isnan(o_bad[0]).any()
    assert torch.equal(o_bad[1:].view(torch.int16), out[1:].view(torch.int16))
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        work = ops.lowrank_kv_work(3, H, Tmax, r_k, r_v, gpu)
        o_side = _run(gpu, dd, lens, H_kv, scale, rope_d, work=work)
    side.synchronize()
    assert torch.equal(o_side.view(torch.int16), out.view(torch.int16))


# ---- 5. strides ---------------------------------------------------------------------------------------------------------------------------------

def test_strided_cache_views(gpu):
    H, H_kv, D, r_k, r_v, with_bv, mode = CONFIGS[7]
    Tmax, lens = 70, [70, 33, 64]
    dd, rope_d, out = _whole_op(gpu, H, H_kv, D, r_k, r_v, Tmax, lens, with_bv, mode, 79)

    def view(c, pad):
        big = torch.full((c.shape[0] + 1, Tmax + 2, c.shape[2] + pad), float("nan"), dtype=torch.float16, device=gpu)
        big[: c.shape[0], :Tmax, : c.shape[2]] = c
        return big[: c.shape[0], :Tmax, : c.shape[2]]

    strided = dict(dd, ck=view(dd["ck"], 8), cv=view(dd["cv"], 24))
    assert not strided["ck"].is_contiguous() and strided["ck"].stride(1) == r_k + 8
    assert torch.equal(_run(gpu, strided, lens, H_kv, D ** -0.5, rope_d).view(torch.int16), out.view(torch.int16))
    with pytest.raises(ValueError):
        _run(gpu, dict(dd, ck=view(dd["ck"], 4)), lens, H_kv, D ** -0.5, rope_d)
    with pytest.raises(ValueError):
        _run(gpu, dict(dd, cv=view(dd["cv"], 2)), lens, H_kv, D ** -0.5, rope_d)


# ---- 6. modules -----------------------------------------------------------------------------------------------------------------------------------

def _attention(dev, rope_mode, seed=5):
    from asvd4llm_amd import ops
    from asvd4llm_amd.kv_cache import LowRankKVAttention
    from asvd4llm_amd.modules.svd_linear import SVDLinear
    torch.manual_seed(seed)
    hid, H, D = 256, 4, 64
    mk = lambda: nn.Linear(hid, hid, bias=False).half().to(dev)
    q_proj, k_lin, v_lin, o_proj = mk(), mk(), mk(), mk()
    k_proj = SVDLinear.from_linear(k_lin, 48 * 2 * hid / hid ** 2, rank_align=16)
    v_proj = SVDLinear.from_linear(v_lin, 32 * 2 * hid / hid ** 2, rank_align=16)
    assert (k_proj.truncation_rank, v_proj.truncation_rank) == (48, 32)
    rope = ops.rope_table(16, D, 10000.0, dev) if rope_mode == "half" else None
    return LowRankKVAttention(q_proj, k_proj, v_proj, o_proj, H, H, rope=rope)


def _run_steps(att, hidden, dtype, kernel, hook=None):
    from asvd4llm_amd.kv_cache import LowRankKVCache
    att = copy.deepcopy(att).to(dtype)
    att.kernel = kernel
    if hook is not None:
        hook(att)
    cache = LowRankKVCache(1, hidden.shape[0], 16, att.ranks, hidden.device, dtype)
    with torch.no_grad():
        outs = [att.prefill(hidden[:, :7].to(dtype), cache, 0)[:, -1:]]
        for s in range(7, 12):
            outs.append(att.decode(hidden[:, s:s + 1].to(dtype), cache, 0))
    return torch.cat(outs, 1).double()


@pytest.mark.parametrize("rope_mode", ["none", "half"])
def test_attention_wrapper_decode_and_refusals(gpu, rope_mode):
    from asvd4llm_amd.kv_cache import FactorPair, LowRankKVAttention
    att = _attention(gpu, rope_mode)
    g = torch.Generator().manual_seed(6)
    hidden = torch.randn(2, 12, 256, generator=g).half().to(gpu)
    assert att.refusal(hidden[:, :1]) is None
    ref = _run_steps(att, hidden, torch.float64, False)           # the wrapper's torch path in fp64
    torch_fp16 = _run_steps(att, hidden, torch.float16, False)    # the same path in fp16: the dense route of this test
    kern = _run_steps(att, hidden, torch.float16, True)
    top = ref[:, 1:].abs().max().item()
    e_k = (kern - ref)[:, 1:].abs().max().item() / top
    e_d = (torch_fp16 - ref)[:, 1:].abs().max().item() / top
    print(f"K20 wrapper {rope_mode}: e_kernel={e_k:.3e} e_dense={e_d:.3e}")
    assert e_k <= max(2 * e_d, FLOOR), (e_k, e_d)
    assert not torch.equal(kern[:, 1:], torch_fp16[:, 1:])        # the two routes are different arithmetic: the kernel did run
    # a refused call answers on the same cache, within the same bound
    hooked = _run_steps(att, hidden, torch.float16, True, hook=lambda a: a.k_proj.BLinear.register_forward_hook(lambda m, i, o: None))
    assert (hooked - ref)[:, 1:].abs().max().item() / top <= max(2 * e_d, FLOOR)
    assert torch.equal(hooked, torch_fp16)
    # every reason is named
    one = hidden[:, :1]
    reasons = {}
    a = copy.deepcopy(att); a.kernel = False; reasons["switched off"] = a.refusal(one)
    a = copy.deepcopy(att); a.k_proj.BLinear.register_forward_hook(lambda m, i, o: None); reasons["hooks"] = a.refusal(one)

    class Packed(nn.Linear):
        pass
    a = copy.deepcopy(att); a.v_proj.ALinear.__class__ = Packed; reasons["packed factors"] = a.refusal(one)
    reasons["token count"] = att.refusal(hidden[:, :2])
    reasons["not fp16"] = att.refusal(one.float())
    mk = lambda i, o, b=False: nn.Linear(i, o, bias=b).half().to(gpu)
    a = LowRankKVAttention(att.q_proj, FactorPair(mk(256, 40), mk(40, 256)), att.v_proj, att.o_proj, 4, 4, rope=att.rope)
    reasons["ranks"] = a.refusal(one)
    a = LowRankKVAttention(att.q_proj, att.k_proj, att.v_proj, att.o_proj, 8, 8, rope=None)
    reasons["head size"] = a.refusal(one)
    if rope_mode == "half":
        a = LowRankKVAttention(att.q_proj, FactorPair(mk(256, 48), mk(48, 256, True)), att.v_proj, att.o_proj, 4, 4, rope=att.rope)
        reasons["key bias under rotation"] = a.refusal(one)
    with torch.enable_grad():
        reasons["autograd"] = att.refusal(one.clone().requires_grad_(True))
    reasons["not on the device"] = att.refusal(one.cpu())
    assert all(k == v for k, v in reasons.items()), reasons


def test_greedy_decode_on_compressed_tiny_llama(gpu):
    from asvd4llm_amd.kv_cache import LowRankKVCache, greedy_decode, kv_ranks
    from asvd4llm_amd.model_zoo import random_init_model
    from asvd4llm_amd.modules.svd_linear import SVDLinear
    model = random_init_model("tiny-llama", dtype=torch.float16, num_attention_heads=2, num_key_value_heads=2).to(gpu)
    for l in model.model.layers:
        l.self_attn.k_proj = SVDLinear.from_linear(l.self_attn.k_proj, 0.5, rank_align=16)
        l.self_attn.v_proj = SVDLinear.from_linear(l.self_attn.v_proj, 0.5, rank_align=16)
    assert kv_ranks(model) == [(32, 32), (32, 32)]
    g = torch.Generator().manual_seed(7)
    ids = torch.randint(0, 512, (2, 9), generator=g).to(gpu)
    ref_model = copy.deepcopy(model).float()
    n_new = 6
    toks_ref, ref = greedy_decode(ref_model, ids, n_new, cache="lowrank", kernel=False)
    toks_low, low = greedy_decode(model, ids, n_new, cache="lowrank", kernel=True, forced=toks_ref)   # one token stream for all three
    toks_dense, dense = greedy_decode(model, ids, n_new, cache="dense", forced=toks_ref)
    top = ref.abs().max().item()
    e_low = (low.float() - ref).abs().max().item() / top
    e_dense = (dense.float() - ref).abs().max().item() / top
    print(f"K20 greedy_decode tiny-llama: e_lowrank={e_low:.3e} e_dense={e_dense:.3e} tokens equal: {torch.equal(toks_low, toks_ref)}")
    assert e_low <= max(2 * e_dense, 2.0 ** -10), (e_low, e_dense)
    assert not torch.equal(low[1:], dense[1:])   # decode steps took different arithmetic
    c = LowRankKVCache(2, 2, 15, kv_ranks(model), gpu)
    assert c.bytes_per_token() * 4 == c.dense_bytes_per_token(2, 64)   # param ratio 0.5 of a 128 x 128 projection is rank 32: a quarter of the cache


# ---- 7. CLI -------------------------------------------------------------------------------------------------------------------------------------------

def test_cli_kv_cache_decode(gpu, tmp_path):
    # not ASVD_STRICT: the kv-cache sweep tries ratios up to 1.9, whose ranks pass the 128-wide projections of this model once aligned to 16; the
    # reference prints "svd failed" and keeps a plain Linear for such a candidate, ASVD_STRICT=1 (which the gpu fixture sets) would raise instead
    env = dict(os.environ, PYTHONPATH=ROOT)
    env.pop("ASVD_STRICT", None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "asvd.py"), "--model_id", "tiny-llama", "--random_init", "--act_aware", "--alpha", "0.5",
                          "--n_calib_samples", "4", "--calib_dataset", "synthetic", "--scaling_method", "abs_mean", "--compress_kv_cache",
                          "--kv_cache_ratio_target", "0.5", "--rank_align", "16", "--kv_cache_decode_tokens", "4"], cwd=str(tmp_path), env=env,
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    m = re.search(r"kv cache bytes per token: dense (\d+), low-rank (\d+) \(ratio ([0-9.]+)\)", out.stdout)
    assert m, out.stdout[-2000:]
    dense, low, ratio = int(m.group(1)), int(m.group(2)), float(m.group(3))
    assert dense == 2 * 2 * 128 * 2 and 0 < low < dense and abs(ratio - low / dense) < 1e-3   # 2 layers x (K + V) x 128 x fp16
    ranks = [int(x) for x in re.findall(r"\d+", re.search(r"kv cache ranks \(k, v\) per layer: (.*)", out.stdout).group(1))]
    assert len(ranks) == 4   # two layers, (k, v) each
    assert low == 2 * sum(ranks)
    m = re.search(r"kv cache decode: 4 tokens, largest logit difference ([0-9.eE+-]+)", out.stdout)
    assert m and float(m.group(1)) >= 0.0, out.stdout[-2000:]
