"""Host-side checks of the int8 low-rank KV cache (K21): the format's restatement and its error bound, ops' torch definition against it bit
for bit, the cache bookkeeping, the torch runner on an int8 cache, and the C ABI's argument refusal.  No GPU."""
import ctypes

import pytest
import torch
import torch.nn as nn

from tests import lowrank_kv_q8_restate as Q

RANKS = [16, 48, 80, 272]   # one 16-wide group alone; 32 + 16; 32 + 32 + 16; eight groups and a tail


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16) if t.dtype == torch.float16 else t


@pytest.mark.parametrize("r", RANKS)
def test_restatement_properties(r):
    g = torch.Generator().manual_seed(100 + r)
    x, nan_at, inf_at = Q.special_rows(g, r)
    codes, scales = Q.quant(x)
    d = Q.dequant(codes, scales)
    assert codes.dtype == torch.int8 and scales.dtype == torch.float32 and scales.shape == (6, Q.n_groups(r)) and d.dtype == torch.float16
    assert codes.abs().max().item() <= 127
    ok = x[:4]
    err = (d[:4].double() - ok.double()).abs()
    assert torch.isfinite(d[:4]).all()
    assert (err <= Q.bound(ok, scales[:4])).all(), (err - Q.bound(ok, scales[:4])).max().item()
    # the all-zero group: scale 0, codes 0; the subnormal group survives (127 codes of the largest entry); 65504 reads back exactly
    assert scales[1, 0].item() == 0.0 and not codes[1, :min(32, r)].any()
    assert (codes[2, :min(32, r)] == 127).all() and torch.equal(d[2, :min(32, r)], x[2, :min(32, r)])
    assert d[3, r - 1].item() == 65504.0
    # a NaN or Inf entry turns exactly its own group of its own row to NaN and nothing else
    want = torch.zeros(6, r, dtype=torch.bool)
    for row, col in (nan_at, inf_at):
        lo, hi = col // 32 * 32, min(col // 32 * 32 + 32, r)
        want[row, lo:hi] = True
        assert torch.isnan(scales[row, col // 32]) and not codes[row, lo:hi].any()
    assert torch.equal(torch.isnan(d), want) and not torch.isinf(d).any()
    assert torch.isnan(scales).sum().item() == 2
    # the rest of the two rows is still within the bound
    fin = ~torch.isnan(d[4:])
    assert ((d[4:].double() - x[4:].double()).abs()[fin] <= Q.bound(torch.where(fin, x[4:], torch.zeros_like(x[4:])), torch.nan_to_num(scales[4:]))[fin]).all()


@pytest.mark.parametrize("r", RANKS + [1024])
def test_ops_definition_equals_the_restatement_bit_for_bit(r):
    from asvd4llm_amd import ops
    g = torch.Generator().manual_seed(200 + r)
    x, _, _ = Q.special_rows(g, r)
    x = torch.stack([x, Q.graded(g, (6, r))])   # [2, 6, r]
    codes, scales = Q.quant(x)
    c2, s2 = ops.lowrank_kv_quant_torch(x)
    assert c2.dtype == torch.int8 and s2.dtype == torch.float32 and ops.lowrank_kv_groups(r) == Q.n_groups(r)
    assert torch.equal(c2, codes) and torch.equal(_bits(s2), _bits(scales))
    # every int8 code, -128 included, against a spread of scales
    allc = torch.arange(-128, 128, dtype=torch.int16).to(torch.int8).expand(7, 256).contiguous()
    sc = torch.tensor([0.0, 1e-10, 3.3e-5, 1.0, 515.78, float("nan"), float("inf")])[:, None].expand(7, 8).contiguous()
    assert torch.equal(_bits(ops.lowrank_kv_dequant(allc, sc)), _bits(Q.dequant(allc, sc)))
    assert torch.equal(_bits(ops.lowrank_kv_dequant(codes, scales)), _bits(Q.dequant(codes, scales)))
    # fp32 and bf16 inputs go through fp16
    c3, s3 = ops.lowrank_kv_quant_torch(x[1].float())
    assert torch.equal(c3, codes[1]) and torch.equal(_bits(s3), _bits(scales[1]))
    with pytest.raises(ValueError):
        ops.lowrank_kv_quant_torch(torch.zeros(2, 24))
    with pytest.raises(ValueError):
        ops.lowrank_kv_dequant(codes.float(), scales)


def test_int8_cache_bookkeeping_on_cpu():
    from asvd4llm_amd.kv_cache import DenseKVCache, LowRankKVCache
    # Llama-2-7B, r_k = r_v = 1024: 2 * (1024 + 32 * 4) B per token and layer
    c7 = LowRankKVCache(1, 1, 1, (1024, 1024), "cpu", quant="int8")
    assert c7.bytes_per_token(0) == 2304 and c7.dense_bytes_per_token(32, 128, 0) == 16384
    assert LowRankKVCache(1, 1, 1, (1024, 1024), "cpu").bytes_per_token(0) == 4096
    # per-layer lists: layer 0 fp16, layer 1 int8 with a 16-wide tail group on the key side
    mixed = LowRankKVCache(2, 1, 4, [(16, 32), (48, 64)], "cpu", quant=[None, "int8"])
    assert mixed.quant == [None, "int8"] and mixed.ck[0].dtype == torch.float16 and mixed.sk[0] is None and mixed.sv[0] is None
    assert mixed.ck[1].dtype == torch.int8 and mixed.ck[1].shape == (1, 4, 48) and mixed.sk[1].shape == (1, 4, 2) and mixed.sv[1].shape == (1, 4, 2)
    assert mixed.sk[1].dtype == torch.float32
    assert mixed.bytes_per_token(0) == (16 + 32) * 2 and mixed.bytes_per_token(1) == (48 + 2 * 4) + (64 + 2 * 4)
    assert mixed.bytes_per_token() == mixed.bytes_per_token(0) + mixed.bytes_per_token(1)
    for bad in ("int4", ["int8"], [None, "int8", None]):
        with pytest.raises(ValueError):
            LowRankKVCache(2, 1, 4, (16, 32), "cpu", quant=bad)
    with pytest.raises(ValueError):
        LowRankKVCache(1, 1, 4, (24, 32), "cpu", quant="int8")
    with pytest.raises(TypeError):
        DenseKVCache(1, 1, 4, 2, 64, "cpu", torch.float16, "int8")   # the dense cache gets no quantisation

    c = LowRankKVCache(2, 3, 10, (48, 32), "cpu", quant="int8")
    for t in (c.ck[0], c.cv[0]):
        t.fill_(-77)
    for t in (c.sk[0], c.sv[0]):
        t.fill_(-5.0)
    g = torch.Generator().manual_seed(4)
    a, b = Q.graded(g, (3, 7, 48)), Q.graded(g, (3, 7, 32))
    a[1, 2, 40] = float("nan")
    dq = lambda x: Q.dequant(*Q.quant(x))
    assert c.append(0, a[:, :4], b[:, :4]) == [0, 0, 0]                       # a chunk (uniform path)
    assert c.append(0, a[:, 4:5], b[:, 4:5]) == [4, 4, 4]                     # one token
    assert c.append(0, a[:, 5:7], b[:, 5:7], counts=[2, 0, 1]) == [5, 5, 5]   # ragged
    assert c.host_lens[0] == [7, 5, 6] and c.lens[0].tolist() == [7, 5, 6] and c.lens[1].tolist() == [0, 0, 0]
    k, v = c.read(0, 7)
    assert k.dtype == torch.float16 and k.shape == (3, 7, 48) and v.shape == (3, 7, 32)
    for s, n in enumerate([7, 5, 6]):
        assert torch.equal(_bits(k[s, :n]), _bits(dq(a[s, :n]))) and torch.equal(_bits(v[s, :n]), _bits(dq(b[s, :n])))
        # rows at and beyond the lengths keep the sentinel
        assert (c.ck[0][s, n:] == -77).all() and (c.cv[0][s, n:] == -77).all() and (c.sk[0][s, n:] == -5.0).all() and (c.sv[0][s, n:] == -5.0).all()
    assert torch.isnan(k[1, 2, 32:]).all() and not torch.isnan(k[1, 2, :32]).any()
    assert c.append(0, a[:, :1].float(), b[:, :1].bfloat16().float()) == [7, 5, 6]    # other dtypes go through .half()
    k2, _ = c.read(0, 8, torch.float32)
    assert k2.dtype == torch.float32 and torch.equal(k2[1, 5], dq(a[1, 0]).float()) and c.lens[0].tolist() == [8, 6, 7]
    with pytest.raises(IndexError):
        c.append(0, a[:, :3], b[:, :3])
    assert c.lens[0].tolist() == [8, 6, 7]                                    # a refused append changes nothing
    with pytest.raises(ValueError):
        c.append(1, a[:, :1, :32], b[:, :1])
    plain = LowRankKVCache(1, 3, 10, (48, 32), "cpu")                         # read() of an fp16 layer is the plain slice
    plain.append(0, a[:, :4], b[:, :4])
    pk, pv = plain.read(0, 4)
    assert torch.equal(_bits(pk[0]), _bits(a[0, :4])) and torch.equal(_bits(pv[2]), _bits(b[2, :4]))


def _truncated_pair(lin, r):
    from asvd4llm_amd.kv_cache import FactorPair
    U, S, Vh = torch.linalg.svd(lin.weight.data.double(), full_matrices=False)
    Bl, Al = nn.Linear(lin.in_features, r, bias=False), nn.Linear(r, lin.out_features, bias=False)
    Bl.weight.data = (S[:r].sqrt()[:, None] * Vh[:r]).to(lin.weight.dtype)
    Al.weight.data = (U[:, :r] * S[:r].sqrt()[None, :]).to(lin.weight.dtype)
    return FactorPair(Bl, Al)


@pytest.mark.parametrize("ranks", [(48, 32), (112, 80)])
def test_greedy_decode_on_an_int8_cache_torch_path(ranks):
    """fp32 tiny-llama with k_proj / v_proj replaced by truncated-SVD factor pairs; 24-token prompts, 8 forced tokens.  The bar is 2^-6 of the
    largest logit of the unquantised run.  Measured with the restatement wrapped round BLinear: 2.9e-3 to 5.2e-3 over four seeds and both rank
    pairs (an fp16 cache gives 1.7e-4).  Through the cache class, this model and this prompt: 5.6e-3 at ranks (48, 32) and 6.4e-3 at
    (112, 80), 0.41 of the bar."""
    from asvd4llm_amd.kv_cache import greedy_decode, kv_ranks
    from asvd4llm_amd.model_zoo import random_init_model
    model = random_init_model("tiny-llama", dtype=torch.float32, num_attention_heads=2, num_key_value_heads=2)
    for l in model.model.layers:
        l.self_attn.k_proj, l.self_attn.v_proj = _truncated_pair(l.self_attn.k_proj, ranks[0]), _truncated_pair(l.self_attn.v_proj, ranks[1])
    assert kv_ranks(model) == [ranks, ranks]
    ids = torch.randint(0, 512, (2, 24), generator=torch.Generator().manual_seed(11))
    toks, ref = greedy_decode(model, ids, 8, cache="lowrank", kernel=False)
    toks_q, low = greedy_decode(model, ids, 8, cache="lowrank", kernel=False, forced=toks, kv_quant="int8")
    top = ref.abs().max().item()
    e = (low - ref).abs().max().item() / top
    print(f"K21 greedy_decode int8 cache, torch path, ranks {ranks}: largest logit difference {e:.3e} of the largest logit")
    assert e <= 2.0 ** -6, e
    assert not torch.equal(low, ref)   # the cache really quantised
    with pytest.raises(ValueError):
        greedy_decode(model, ids, 1, cache="dense", kv_quant="int8")
    with pytest.raises(ValueError):
        greedy_decode(model, ids, 1, cache="lowrank", kernel=False, kv_quant="int4")


def test_greedy_decode_int8_keeps_an_uncompressed_layer_in_fp():
    """layer 0 compressed, layer 1 left as nn.Linear: only layer 0 becomes int8, layer 1 keeps K and V in the cache's dtype"""
    from asvd4llm_amd import kv_cache
    from asvd4llm_amd.model_zoo import random_init_model
    model = random_init_model("tiny-llama", dtype=torch.float32, num_attention_heads=2, num_key_value_heads=2)
    a = model.model.layers[0].self_attn
    a.k_proj, a.v_proj = _truncated_pair(a.k_proj, 48), _truncated_pair(a.v_proj, 32)
    seen = []
    orig = kv_cache.LowRankKVCache.__init__

    def spy(self, *args, **kw):
        orig(self, *args, **kw)
        seen.append(self)
    kv_cache.LowRankKVCache.__init__ = spy
    try:
        ids = torch.randint(0, 512, (2, 5), generator=torch.Generator().manual_seed(8))
        toks, ref = kv_cache.greedy_decode(model, ids, 3, cache="lowrank", kernel=False)
        _, low = kv_cache.greedy_decode(model, ids, 3, cache="lowrank", kernel=False, forced=toks, kv_quant="int8")
    finally:
        kv_cache.LowRankKVCache.__init__ = orig
    assert seen[0].quant == [None, None] and seen[1].quant == ["int8", None]
    assert seen[1].ck[0].dtype == torch.int8 and seen[1].ck[1].dtype == torch.float32 and seen[1].widths == [(48, 32), (128, 128)]
    assert (low - ref).abs().max().item() <= 2.0 ** -6 * ref.abs().max().item() and not torch.equal(low, ref)


def test_q8_bad_arguments_are_refused_without_a_device(built_lib):
    """every rule of the header for the three K21 entries, one at a time, against a call that passes them all up to the device (host
    buffers: nothing is launched because each call below is refused)"""
    buf = (ctypes.c_char * 4096)()
    base = (ctypes.addressof(buf) + 15) & ~15
    P = lambda off=0: ctypes.c_void_p(base + off)
    F16, BF16 = 1, 2

    qgood = dict(x=P(), xrs=48, xbs=480, codes=P(), crs=48, cbs=480, scales=P(), srs=2, sbs=20, dtype=F16, B=2, n=3, r=48, stream=None)

    def quant(**kw):
        a = {**qgood, **kw}
        return built_lib.asvd_lowrank_kv_quant(*[a[k] for k in qgood])

    for kw in [dict(x=None), dict(codes=None), dict(scales=None), dict(dtype=BF16), dict(dtype=0), dict(r=24), dict(r=0), dict(r=40), dict(B=0), dict(n=0),
               dict(x=P(8)), dict(codes=P(8)), dict(scales=P(2)), dict(xrs=52), dict(xrs=40), dict(xbs=100), dict(crs=56), dict(crs=32), dict(cbs=472),
               dict(cbs=96), dict(srs=1), dict(sbs=4)]:
        assert quant(**kw) == -1, kw

    good = dict(q=P(), ck=P(), cv=P(), sk=P(), sv=P(), lens=P(), Ak=P(), Av=P(), bk=None, bv=None, cos=P(), sin=P(), dtype=F16, mode=1, scale=1.0, B=2,
                H=4, H_kv=2, D=64, r_k=48, r_v=80, Tmax=8, krs=48, kbs=384, vrs=80, vbs=640, skrs=2, skbs=16, svrs=3, svbs=24, out=P(), work=P(),
                wb=1 << 30, stream=None)
    order = list(good)

    def decode(**kw):
        a = {**good, **kw}
        return built_lib.asvd_lowrank_kv_decode_q8(*[a[k] for k in order])

    def scores(**kw):
        a = {**good, **kw}
        names = ["q", "ck", "sk", "lens", "Ak", "bk", "cos", "sin", "dtype", "mode", "scale", "B", "H", "H_kv", "D", "r_k", "Tmax", "krs", "kbs", "skrs",
                 "skbs", "out", "work", "wb", "stream"]
        return built_lib.asvd_lowrank_kv_scores_q8(*[a[k] for k in names])

    bad = [dict(q=None), dict(ck=None), dict(sk=None), dict(lens=None), dict(Ak=None), dict(work=None), dict(dtype=BF16), dict(dtype=0), dict(mode=2),
           dict(D=96), dict(D=32), dict(H=0), dict(H_kv=3), dict(B=0), dict(Tmax=0), dict(r_k=24), dict(r_k=0), dict(krs=56), dict(krs=32), dict(kbs=392),
           dict(kbs=96), dict(q=P(2)), dict(ck=P(8)), dict(sk=P(2)), dict(Ak=P(4)), dict(work=P(8)), dict(lens=P(2)), dict(cos=None), dict(sin=None),
           dict(cos=P(4)), dict(skrs=1), dict(skbs=8), dict(bk=P())]   # krs 56: a multiple of 8 but not of 16; the last: a key bias under rotation
    for kw in bad:
        assert decode(**kw) == -1, kw
        assert scores(**kw) == -1, kw
    for kw in [dict(cv=None), dict(sv=None), dict(Av=None), dict(out=None), dict(r_v=40), dict(r_v=0), dict(vrs=88), dict(vrs=64), dict(vbs=8),
               dict(cv=P(8)), dict(sv=P(1)), dict(Av=P(2)), dict(out=P(8)), dict(svrs=2), dict(svbs=16)]:
        assert decode(**kw) == -1, kw
    assert decode(wb=16) == -2 and scores(wb=16) == -2   # workspace too small: refused before any launch as well
