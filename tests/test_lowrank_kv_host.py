"""Host-side checks of the low-rank KV cache path (K20): the fp64 restatement the GPU tests rest on, the rotation convention, the
absorbed products the kernel uses, the cache bookkeeping, the torch runner, and the C ABI's argument refusal.  No GPU."""
import ctypes

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import lowrank_kv_restate as R


def _case(g, B, H, H_kv, D, T, r_k, r_v, bias=True):
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    q, ck, cv = rnd(B, H, D), rnd(B, T, r_k), rnd(B, T, r_v)
    Ak, Av = rnd(H_kv * D, r_k) / r_k ** 0.5, rnd(H_kv * D, r_v) / r_v ** 0.5
    bk, bv = (rnd(H_kv * D), rnd(H_kv * D)) if bias else (None, None)
    return q, ck, cv, Ak, Av, bk, bv


@pytest.mark.parametrize("H,H_kv,rope", [(4, 4, False), (4, 1, False), (4, 4, True), (8, 2, True)])
def test_restatement_equals_sdpa_fp64(H, H_kv, rope):
    from asvd4llm_amd import ops
    g = torch.Generator().manual_seed(1)
    B, D, T = 3, 64, 9
    q, ck, cv, Ak, Av, bk, bv = _case(g, B, H, H_kv, D, T, 48, 32)
    lens = [9, 4, 1]
    tab = tuple(t.double() for t in ops.rope_table(T, D, 10000.0)) if rope else None
    out = R.kv_decode(q, ck, cv, lens, Ak, Av, H_kv, 0.125, bk, bv, tab)
    K, V = R.rebuild(ck, Ak, bk, H_kv, H), R.rebuild(cv, Av, bv, H_kv, H)
    if rope:
        K = R.rotate_half_table(K, *tab)
    mask = (torch.arange(T)[None, :] < torch.tensor(lens)[:, None])[:, None, None, :]
    ref = F.scaled_dot_product_attention(q[:, :, None, :], K, V, attn_mask=mask, scale=0.125)[:, :, 0]
    assert (out - ref).abs().max().item() <= 1e-12 * ref.abs().max().item()
    zero = R.kv_decode(q, ck, cv, [0, 4, 1], Ak, Av, H_kv, 0.125, bk, bv, tab)
    assert torch.equal(zero[0], torch.zeros(H, D, dtype=torch.float64)) and torch.equal(zero[1:], out[1:])


def test_rotation_convention_is_the_installed_transformers():
    from transformers import LlamaConfig
    from transformers.models.llama.modeling_llama import LlamaRotaryEmbedding, apply_rotary_pos_emb
    from asvd4llm_amd import ops
    D, T, H = 64, 37, 2
    cfg = LlamaConfig(hidden_size=H * D, num_attention_heads=H, num_key_value_heads=H, num_hidden_layers=1, intermediate_size=64, vocab_size=32)
    emb = LlamaRotaryEmbedding(cfg)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(1, H, T, D, generator=g)
    cos, sin = emb(x, torch.arange(T)[None, :])
    hf, _ = apply_rotary_pos_emb(x, x, cos, sin)
    tab = ops.rope_table(T, D, 10000.0)
    assert tab[0].dtype == torch.float32 and tab[0].shape == (T, D // 2)
    mine = R.rotate_half_table(x, *tab)
    assert (mine - hf).abs().max().item() <= 4 * 2.0 ** -23 * x.abs().max().item()   # the same fp32 angles: a few ulps of the products


@pytest.mark.parametrize("H,H_kv", [(4, 4), (8, 2)])
def test_absorbed_forms_equal_the_plain_form(H, H_kv):
    g = torch.Generator().manual_seed(3)
    B, D, T, r_k, r_v = 2, 64, 11, 48, 32
    q, ck, cv, Ak, Av, bk, bv = _case(g, B, H, H_kv, D, T, r_k, r_v)
    lens, scale, grp = [11, 5], 0.125, H // H_kv
    # scores through q~ = A_k[kv(h)]^T q_h, no key bias
    S, live = R.kv_scores(q, ck, lens, Ak, H_kv, scale)
    qt = torch.stack([torch.stack([Ak.view(H_kv, D, r_k)[h // grp].T @ q[b, h] for h in range(H)]) for b in range(B)])
    S2 = scale * torch.einsum("bhr,btr->bht", qt, ck) * live[:, None, :]
    assert (S - S2).abs().max().item() <= 1e-12 * S.abs().max().item()
    # the key bias changes no output without rotation
    o_b = R.kv_decode(q, ck, cv, lens, Ak, Av, H_kv, scale, bk, bv)
    o_nb = R.kv_decode(q, ck, cv, lens, Ak, Av, H_kv, scale, None, bv)
    assert (o_b - o_nb).abs().max().item() <= 1e-12 * o_b.abs().max().item()
    # the latent value sum: (p C_v) A_v[kv(h)]^T + b_v
    Sm = S.masked_fill(~live[:, None, :], float("-inf"))
    p = torch.softmax(Sm, -1)
    lat = torch.einsum("bht,btr->bhr", p, cv)
    o2 = torch.stack([torch.stack([Av.view(H_kv, D, r_v)[h // grp] @ lat[b, h] + bv.view(H_kv, D)[h // grp] for h in range(H)]) for b in range(B)])
    assert (o_nb - o2).abs().max().item() <= 1e-12 * o2.abs().max().item()


def test_cache_bookkeeping_on_cpu():
    from asvd4llm_amd.kv_cache import LowRankKVCache
    c = LowRankKVCache(2, 3, 10, (48, 32), "cpu")
    g = torch.Generator().manual_seed(4)
    a, b = torch.randn(3, 7, 48, generator=g).half(), torch.randn(3, 7, 32, generator=g).half()
    assert c.append(0, a[:, :4], b[:, :4]) == [0, 0, 0]                       # a chunk
    assert c.append(0, a[:, 4:5], b[:, 4:5]) == [4, 4, 4]                     # one token
    assert c.append(0, a[:, 5:7], b[:, 5:7], counts=[2, 0, 1]) == [5, 5, 5]   # ragged
    assert c.host_lens[0] == [7, 5, 6] and c.lens[0].tolist() == [7, 5, 6] and c.lens[1].tolist() == [0, 0, 0]
    assert c.lens.dtype == torch.int32
    assert torch.equal(c.ck[0][0, :7], a[0]) and torch.equal(c.cv[0][2, :6], b[2, :6]) and torch.equal(c.ck[0][1, :5], a[1, :5])
    assert c.append(0, a[:, :1], b[:, :1]) == [7, 5, 6]                       # single token at different lengths
    assert torch.equal(c.ck[0][1, 5], a[1, 0]) and c.lens[0].tolist() == [8, 6, 7]
    with pytest.raises(IndexError):
        c.append(0, a[:, :3], b[:, :3])
    assert c.lens[0].tolist() == [8, 6, 7]                                    # a refused append changes nothing
    with pytest.raises(ValueError):
        c.append(1, a[:, :1, :32], b[:, :1])
    assert c.bytes_per_token(0) == (48 + 32) * 2 and c.bytes_per_token() == 2 * 160
    assert c.dense_bytes_per_token(4, 64, 0) == 2 * 4 * 64 * 2
    # Llama-2-7B, r_k = r_v = 1024: 4096 B per token and layer against 16384 B dense
    c7 = LowRankKVCache(1, 1, 1, (1024, 1024), "cpu")
    assert c7.bytes_per_token(0) == 4096 and c7.dense_bytes_per_token(32, 128, 0) == 16384
    per_layer = LowRankKVCache(2, 1, 1, [(16, 32), (48, 64)], "cpu")
    assert per_layer.bytes_per_token() == (16 + 32 + 48 + 64) * 2 and per_layer.ck[1].shape == (1, 1, 48)


def _full_rank_pair(lin):
    from asvd4llm_amd.kv_cache import FactorPair
    U, S, Vh = torch.linalg.svd(lin.weight.data.double(), full_matrices=False)
    r = S.numel()
    Bl, Al = nn.Linear(lin.in_features, r, bias=False), nn.Linear(r, lin.out_features, bias=lin.bias is not None)
    Bl.weight.data = (S.sqrt()[:, None] * Vh).to(lin.weight.dtype)
    Al.weight.data = (U * S.sqrt()[None, :]).to(lin.weight.dtype)
    if lin.bias is not None:
        Al.bias.data = lin.bias.data.clone()
    return FactorPair(Bl, Al)


def test_greedy_decode_torch_path_matches_the_model_recomputed_from_scratch():
    """fp32 tiny-llama (2 layers, 2 heads, D = 64) with k_proj / v_proj replaced by full-rank factor pairs.  Bound: both sides evaluate the
    same function in fp32 with different summation orders.  Per layer the residual stream passes ~6 matrix products / normalisations whose
    fp32 summation error is each a few 2^-24 relative to the stream; over 2 layers and the head that is ~2 * 6 + 2 = 14 roundings of size
    ~2^-23 each amplified by at most O(10) through the norms: 14 * 10 * 2^-23 < 2^-15.  Measured against the largest logit."""
    from asvd4llm_amd.kv_cache import greedy_decode
    from asvd4llm_amd.model_zoo import random_init_model
    model = random_init_model("tiny-llama", dtype=torch.float32, num_attention_heads=2, num_key_value_heads=2)
    for l in model.model.layers:
        l.self_attn.k_proj, l.self_attn.v_proj = _full_rank_pair(l.self_attn.k_proj), _full_rank_pair(l.self_attn.v_proj)
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(0, 512, (2, 6), generator=g)
    bound = 2.0 ** -15
    toks, logits = greedy_decode(model, ids, 4, cache="lowrank", kernel=False)
    toks_d, logits_d = greedy_decode(model, ids, 4, cache="dense", kernel=False)
    assert toks.shape == (2, 4) and logits.shape == (4, 2, 512)
    with torch.no_grad():
        for s in range(4):
            ref = model(torch.cat([ids, toks[:, :s]], 1)).logits[:, -1]
            top = ref.abs().max().item()
            assert (logits[s] - ref).abs().max().item() <= bound * top, s
            assert (logits_d[s] - ref).abs().max().item() <= bound * top, s
            assert (logits[s] - logits_d[s]).abs().max().item() <= bound * top, s
    assert torch.equal(toks, logits.argmax(-1).T)


def test_greedy_decode_keeps_k_and_v_of_a_layer_the_search_left_uncompressed():
    """layer 0 compressed (rank 48 / 32 pairs, so the model changes), layer 1 left as nn.Linear: the runner serves both in one cache, and
    the low-rank and the dense cache still compute the same function (bound as above)"""
    from asvd4llm_amd.kv_cache import FactorPair, greedy_decode, kv_ranks
    from asvd4llm_amd.model_zoo import random_init_model
    model = random_init_model("tiny-llama", dtype=torch.float32, num_attention_heads=2, num_key_value_heads=2)
    a = model.model.layers[0].self_attn
    a.k_proj = FactorPair(nn.Linear(128, 48, bias=False), nn.Linear(48, 128, bias=False))
    a.v_proj = FactorPair(nn.Linear(128, 32, bias=False), nn.Linear(32, 128, bias=False))
    assert kv_ranks(model) == [(48, 32), (128, 128)]
    ids = torch.randint(0, 512, (2, 5), generator=torch.Generator().manual_seed(8))
    toks, logits = greedy_decode(model, ids, 3, cache="lowrank", kernel=False)
    toks_d, logits_d = greedy_decode(model, ids, 3, cache="dense", forced=toks)
    with torch.no_grad():
        for s in range(3):
            ref = model(torch.cat([ids, toks[:, :s]], 1)).logits[:, -1]
            assert (logits[s] - ref).abs().max().item() <= 2.0 ** -15 * ref.abs().max().item()
            assert (logits_d[s] - ref).abs().max().item() <= 2.0 ** -15 * ref.abs().max().item()


def test_attention_wrapper_refuses_off_the_device():
    from asvd4llm_amd.kv_cache import FactorPair, LowRankKVAttention
    mk = lambda i, o: nn.Linear(i, o, bias=False)
    att = LowRankKVAttention(mk(128, 128), FactorPair(mk(128, 48), mk(48, 128)), FactorPair(mk(128, 32), mk(32, 128)), mk(128, 128), 2, 2)
    assert att.refusal(torch.zeros(1, 1, 128)) == "not fp16"
    assert att.half().refusal(torch.zeros(1, 1, 128).half()) == "not on the device"
    with pytest.raises(TypeError):
        LowRankKVAttention(mk(128, 128), mk(128, 128), mk(128, 128), mk(128, 128), 2, 2)


def test_worksize_and_plan_hand_count(built_lib):
    nb = ctypes.c_size_t()
    # B 2, H 12 (Hpad 32), Tmax 100 (Tld 112): 16 splits wanted, 64 tokens at the least per split -> 2 splits
    assert built_lib.asvd_lowrank_kv_worksize(2, 12, 100, 48, 32, ctypes.byref(nb)) == 0
    assert nb.value == 2 * 32 * 48 * 2 + 2 * 12 * 112 * 4 + 2 * 2 * 32 * 2 * 4 + 2 * 2 * 32 * 32 * 4
    tile, split, n = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    assert built_lib.asvd_lowrank_kv_plan(2, 12, 100, ctypes.byref(tile), ctypes.byref(split), ctypes.byref(n)) == 0
    assert (tile.value, split.value, n.value) == (32, 64, 2)
    assert built_lib.asvd_lowrank_kv_plan(1, 32, 4096, ctypes.byref(tile), ctypes.byref(split), ctypes.byref(n)) == 0
    assert (split.value, n.value) == (256, 16)
    assert built_lib.asvd_lowrank_kv_plan(8, 40, 4096, ctypes.byref(tile), ctypes.byref(split), ctypes.byref(n)) == 0
    assert (split.value, n.value) == (256, 16)   # 16 workgroups per split: 256 CUs / 16
    assert built_lib.asvd_lowrank_kv_worksize(2, 12, 100, 40, 32, ctypes.byref(nb)) == -1
    assert built_lib.asvd_lowrank_kv_worksize(2, 12, 100, 48, 32, None) == -1
    assert built_lib.asvd_lowrank_kv_worksize(0, 12, 100, 48, 32, ctypes.byref(nb)) == -1


def test_bad_arguments_are_refused_without_a_device(built_lib):
    """every rule of the header, one at a time, against a call that passes them all up to the device (host buffers: nothing is launched
    because each call below is refused)"""
    buf = (ctypes.c_char * 4096)()
    base = (ctypes.addressof(buf) + 15) & ~15
    P = lambda off=0: ctypes.c_void_p(base + off)
    F16, BF16 = 1, 2
    good = dict(q=P(), ck=P(), cv=P(), lens=P(), Ak=P(), Av=P(), bk=None, bv=None, cos=P(), sin=P(), dtype=F16, mode=1, scale=1.0, B=1, H=4, H_kv=2,
                D=64, r_k=16, r_v=32, Tmax=8, krs=16, kbs=128, vrs=32, vbs=256, out=P(), work=P(), wb=1 << 30, stream=None)
    order = list(good)

    def decode(**kw):
        a = {**good, **kw}
        return built_lib.asvd_lowrank_kv_decode(*[a[k] for k in order])

    def scores(**kw):
        a = {**good, **kw}
        names = ["q", "ck", "lens", "Ak", "bk", "cos", "sin", "dtype", "mode", "scale", "B", "H", "H_kv", "D", "r_k", "Tmax", "krs", "kbs", "out", "work",
                 "wb", "stream"]
        return built_lib.asvd_lowrank_kv_scores(*[a[k] for k in names])

    bad = [dict(q=None), dict(ck=None), dict(lens=None), dict(Ak=None), dict(work=None), dict(dtype=BF16), dict(dtype=0), dict(mode=2), dict(D=96),
           dict(D=32), dict(H=0), dict(H_kv=3), dict(B=0), dict(Tmax=0), dict(r_k=24), dict(r_k=0), dict(krs=20), dict(krs=8), dict(kbs=100),
           dict(q=P(2)), dict(ck=P(8)), dict(Ak=P(4)), dict(work=P(8)), dict(lens=P(2)), dict(cos=None), dict(sin=None), dict(cos=P(4)),
           dict(bk=P())]   # a key bias under rotation
    for kw in bad:
        assert decode(**kw) == -1, kw
        assert scores(**kw) == -1, kw
    for kw in [dict(cv=None), dict(Av=None), dict(out=None), dict(r_v=40), dict(r_v=0), dict(vrs=24), dict(vrs=36), dict(vbs=4), dict(cv=P(8)),
               dict(Av=P(2)), dict(out=P(8))]:
        assert decode(**kw) == -1, kw
    assert decode(wb=16) == -2 and scores(wb=16) == -2   # workspace too small: refused before any launch as well
