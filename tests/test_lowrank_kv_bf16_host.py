"""Decode attention on the low-rank KV cache for bf16 models (K22), host side: the four asvd_lowrank_kv_*_a16 entries (declared, exported,
their argument refusal with ASVD_BF16), the dtype rules of the ops, the opt-in switch and the refusals of LowRankKVAttention, and bf16 appends
to an int8 cache.  No device."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn as nn

from tests.conftest import ROOT

F16, BF16 = 1, 2   # ASVD_F16, ASVD_BF16

_SCORES = ("const void* q, const void* ck, const void* lens, const void* Ak, const void* bk, const void* cos_tab, const void* sin_tab, int dtype, "
           "int rope_mode, float scale, int64_t B, int64_t H, int64_t H_kv, int64_t D, int64_t r_k, int64_t Tmax, int64_t ck_row_stride, "
           "int64_t ck_batch_stride, void* scores_out, void* work, size_t work_bytes, void* stream")
_DECODE = ("const void* q, const void* ck, const void* cv, const void* lens, const void* Ak, const void* Av, const void* bk, const void* bv, "
           "const void* cos_tab, const void* sin_tab, int dtype, int rope_mode, float scale, int64_t B, int64_t H, int64_t H_kv, int64_t D, int64_t r_k, "
           "int64_t r_v, int64_t Tmax, int64_t ck_row_stride, int64_t ck_batch_stride, int64_t cv_row_stride, int64_t cv_batch_stride, void* out, "
           "void* work, size_t work_bytes, void* stream")
_SCORES_Q8 = ("const void* q, const void* ck, const void* sk, const void* lens, const void* Ak, const void* bk, const void* cos_tab, "
              "const void* sin_tab, int dtype, int rope_mode, float scale, int64_t B, int64_t H, int64_t H_kv, int64_t D, int64_t r_k, int64_t Tmax, "
              "int64_t ck_row_stride, int64_t ck_batch_stride, int64_t sk_row_stride, int64_t sk_batch_stride, void* scores_out, void* work, "
              "size_t work_bytes, void* stream")
_DECODE_Q8 = ("const void* q, const void* ck, const void* cv, const void* sk, const void* sv, const void* lens, const void* Ak, const void* Av, "
              "const void* bk, const void* bv, const void* cos_tab, const void* sin_tab, int dtype, int rope_mode, float scale, int64_t B, int64_t H, "
              "int64_t H_kv, int64_t D, int64_t r_k, int64_t r_v, int64_t Tmax, int64_t ck_row_stride, int64_t ck_batch_stride, int64_t cv_row_stride, "
              "int64_t cv_batch_stride, int64_t sk_row_stride, int64_t sk_batch_stride, int64_t sv_row_stride, int64_t sv_batch_stride, void* out, "
              "void* work, size_t work_bytes, void* stream")
A16 = {"asvd_lowrank_kv_scores_a16": _SCORES, "asvd_lowrank_kv_decode_a16": _DECODE, "asvd_lowrank_kv_scores_q8_a16": _SCORES_Q8,
       "asvd_lowrank_kv_decode_q8_a16": _DECODE_Q8}
_CTYPE = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t, "float": ctypes.c_float}


# ---- C ABI -----------------------------------------------------------------------------------------------------------------------------

def test_a16_entries_are_declared_exported_and_documented(built_lib):
    from asvd4llm_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "asvd_hip.h")).read(), flags=re.S)
    for name, want in A16.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
        assert m, f"{name} is not declared in asvd_hip.h"
        params = [" ".join(p.split()) for p in m.group(1).split(",")]
        assert params == [p.strip() for p in want.split(",")], name
        # the argument list of the entry it extends, word for word
        old = re.search(r"\bint\s+" + name[:-4] + r"\s*\(([^)]*)\)\s*;", src)
        assert old and [" ".join(p.split()) for p in old.group(1).split(",")] == params, name
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and hasattr(built_lib, name)
        assert args == [ctypes.c_void_p if "*" in p else _CTYPE[p.rsplit(" ", 1)[0]] for p in params], name
        assert args == _lib.SIGNATURES[name[:-4]][1], name
    guide = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(name in guide for name in A16) and "ASVD_KV_BF16" in guide


def _host_pointers():
    buf = (ctypes.c_char * 4096)()
    base = (ctypes.addressof(buf) + 15) & ~15
    return buf, (lambda off=0: ctypes.c_void_p(base + off))


@pytest.mark.parametrize("dtype", [BF16, F16])
def test_a16_entries_refuse_bad_arguments_without_a_device(built_lib, dtype):
    """the list of tests/test_lowrank_kv_host.py, against the _a16 entries with ASVD_BF16 (and ASVD_F16) set: host buffers, nothing is launched
    because every call below is refused"""
    buf, P = _host_pointers()
    good = dict(q=P(), ck=P(), cv=P(), lens=P(), Ak=P(), Av=P(), bk=None, bv=None, cos=P(), sin=P(), dtype=dtype, mode=1, scale=1.0, B=1, H=4, H_kv=2,
                D=64, r_k=16, r_v=32, Tmax=8, krs=16, kbs=128, vrs=32, vbs=256, out=P(), work=P(), wb=1 << 30, stream=None)
    order = list(good)
    snames = ["q", "ck", "lens", "Ak", "bk", "cos", "sin", "dtype", "mode", "scale", "B", "H", "H_kv", "D", "r_k", "Tmax", "krs", "kbs", "out", "work", "wb",
              "stream"]

    def decode(fn=built_lib.asvd_lowrank_kv_decode_a16, **kw):
        a = {**good, **kw}
        return fn(*[a[k] for k in order])

    def scores(fn=built_lib.asvd_lowrank_kv_scores_a16, **kw):
        a = {**good, **kw}
        return fn(*[a[k] for k in snames])

    bad = [dict(q=None), dict(ck=None), dict(lens=None), dict(Ak=None), dict(work=None), dict(dtype=0), dict(dtype=3), dict(mode=2), dict(D=96),
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
    # the entries without the suffix keep their rule: fp16 only
    assert decode(fn=built_lib.asvd_lowrank_kv_decode, dtype=BF16) == -1 and scores(fn=built_lib.asvd_lowrank_kv_scores, dtype=BF16) == -1
    assert decode(fn=built_lib.asvd_lowrank_kv_decode, dtype=BF16, wb=16) == -1   # the dtype first: not -2


@pytest.mark.parametrize("dtype", [BF16, F16])
def test_q8_a16_entries_refuse_bad_arguments_without_a_device(built_lib, dtype):
    """the list of tests/test_lowrank_kv_q8_host.py against the _q8_a16 entries"""
    buf, P = _host_pointers()
    good = dict(q=P(), ck=P(), cv=P(), sk=P(), sv=P(), lens=P(), Ak=P(), Av=P(), bk=None, bv=None, cos=P(), sin=P(), dtype=dtype, mode=1, scale=1.0, B=2,
                H=4, H_kv=2, D=64, r_k=48, r_v=80, Tmax=8, krs=48, kbs=384, vrs=80, vbs=640, skrs=2, skbs=16, svrs=3, svbs=24, out=P(), work=P(),
                wb=1 << 30, stream=None)
    order = list(good)
    snames = ["q", "ck", "sk", "lens", "Ak", "bk", "cos", "sin", "dtype", "mode", "scale", "B", "H", "H_kv", "D", "r_k", "Tmax", "krs", "kbs", "skrs", "skbs",
              "out", "work", "wb", "stream"]

    def decode(fn=built_lib.asvd_lowrank_kv_decode_q8_a16, **kw):
        a = {**good, **kw}
        return fn(*[a[k] for k in order])

    def scores(fn=built_lib.asvd_lowrank_kv_scores_q8_a16, **kw):
        a = {**good, **kw}
        return fn(*[a[k] for k in snames])

    bad = [dict(q=None), dict(ck=None), dict(sk=None), dict(lens=None), dict(Ak=None), dict(work=None), dict(dtype=0), dict(dtype=3), dict(mode=2),
           dict(D=96), dict(D=32), dict(H=0), dict(H_kv=3), dict(B=0), dict(Tmax=0), dict(r_k=24), dict(r_k=0), dict(krs=56), dict(krs=32), dict(kbs=392),
           dict(kbs=96), dict(q=P(2)), dict(ck=P(8)), dict(sk=P(2)), dict(Ak=P(4)), dict(work=P(8)), dict(lens=P(2)), dict(cos=None), dict(sin=None),
           dict(cos=P(4)), dict(skrs=1), dict(skbs=8), dict(bk=P())]
    for kw in bad:
        assert decode(**kw) == -1, kw
        assert scores(**kw) == -1, kw
    for kw in [dict(cv=None), dict(sv=None), dict(Av=None), dict(out=None), dict(r_v=40), dict(r_v=0), dict(vrs=88), dict(vrs=64), dict(vbs=8),
               dict(cv=P(8)), dict(sv=P(1)), dict(Av=P(2)), dict(out=P(8)), dict(svrs=2), dict(svbs=16)]:
        assert decode(**kw) == -1, kw
    assert decode(wb=16) == -2 and scores(wb=16) == -2
    assert decode(fn=built_lib.asvd_lowrank_kv_decode_q8, dtype=BF16) == -1 and scores(fn=built_lib.asvd_lowrank_kv_scores_q8, dtype=BF16) == -1


# ---- ops: one dtype, checked before the device is asked for -------------------------------------------------------------------------------

def _op_args(dt, B=2, H=4, H_kv=2, D=64, r_k=16, r_v=32, T=8):
    z = lambda *s: torch.zeros(*s, dtype=dt)
    return dict(q=z(B, H, D), ck=z(B, T, r_k), cv=z(B, T, r_v), lens=torch.zeros(B, dtype=torch.int32), Ak=z(H_kv * D, r_k), Av=z(H_kv * D, r_v),
                H_kv=H_kv, scale=0.125)


def test_ops_refuse_mixed_dtypes_and_fp32_on_the_cpu():
    from asvd4llm_amd import ops
    bf, hf = torch.bfloat16, torch.float16
    a = _op_args(bf)
    order = ["q", "ck", "cv", "lens", "Ak", "Av", "H_kv", "scale"]
    call = lambda d, **kw: ops.lowrank_kv_decode(*[d[k] for k in order], **kw)
    mixed = [dict(ck=a["ck"].to(hf)), dict(cv=a["cv"].to(hf)), dict(Ak=a["Ak"].to(hf)), dict(Av=a["Av"].to(hf)), dict(q=a["q"].to(hf)),
             dict(q=a["q"].float())]
    for kw in mixed:
        with pytest.raises(ValueError):
            call({**a, **kw})
    with pytest.raises(ValueError):
        call(a, out=torch.zeros(2, 4, 64, dtype=hf))           # an fp16 out with bf16 inputs
    with pytest.raises(ValueError):
        call(a, bv=torch.zeros(128, dtype=hf))
    with pytest.raises(ValueError):
        call(_op_args(torch.float32))
    with pytest.raises(ValueError):
        call(_op_args(hf), out=torch.zeros(2, 4, 64, dtype=bf))  # and the other way round
    for kw in (dict(ck=a["ck"].to(hf)), dict(Ak=a["Ak"].to(hf)), dict(q=a["q"].float())):
        d = {**a, **kw}
        with pytest.raises(ValueError):
            ops.lowrank_kv_scores(d["q"], d["ck"], d["lens"], d["Ak"], 2, 0.125)
        with pytest.raises(ValueError):
            ops.lowrank_kv_scores(d["q"], d["ck"], d["lens"], d["Ak"], 2, 0.125, bk=torch.zeros(128, dtype=torch.float32))
    # the int8 forms: q, Ak, Av, the biases and out are one dtype
    codes = lambda r: torch.zeros(2, 8, r, dtype=torch.int8)
    sc = lambda r: torch.zeros(2, 8, ops.lowrank_kv_groups(r))
    q8 = lambda d, **kw: ops.lowrank_kv_decode_q8(d["q"], codes(16), codes(32), sc(16), sc(32), d["lens"], d["Ak"], d["Av"], 2, 0.125, **kw)
    for kw in (dict(Ak=a["Ak"].to(hf)), dict(Av=a["Av"].to(hf)), dict(q=a["q"].float())):
        with pytest.raises(ValueError):
            q8({**a, **kw})
    with pytest.raises(ValueError):
        q8(a, out=torch.zeros(2, 4, 64, dtype=hf))
    with pytest.raises(ValueError):
        ops.lowrank_kv_scores_q8(a["q"], codes(16), sc(16), a["lens"], a["Ak"].to(hf), 2, 0.125)
    # all-bf16 arguments pass every rule and stop at the device: not a dtype error any more
    from asvd4llm_amd._lib import AsvdHipError
    with pytest.raises(AsvdHipError):
        call(a)
    with pytest.raises(AsvdHipError):
        q8(a)


# ---- the switch and the refusals --------------------------------------------------------------------------------------------------------

def _att(kv_bf16=None, bias=False):
    from asvd4llm_amd.kv_cache import FactorPair, LowRankKVAttention
    mk = lambda i, o, b=False: nn.Linear(i, o, bias=b)
    return LowRankKVAttention(mk(128, 128), FactorPair(mk(128, 48), mk(48, 128)), FactorPair(mk(128, 32), mk(32, 128, bias)), mk(128, 128), 2, 2,
                              kv_bf16=kv_bf16)


def test_attention_wrapper_bf16_switch_and_refusals(monkeypatch):
    monkeypatch.delenv("ASVD_KV_BF16", raising=False)
    h = torch.zeros(1, 1, 128, dtype=torch.bfloat16)
    off = _att().bfloat16()
    assert off.kv_bf16 is False and off.refusal(h) == "not fp16"                     # off: as before
    assert _att(kv_bf16=False).bfloat16().refusal(h) == "not fp16"
    on = _att(kv_bf16=True).bfloat16()
    assert on.kv_bf16 is True and on.refusal(h) == "not on the device"               # on: the dtype rule passes, the remaining rules follow
    assert on.refusal(h.float()) == "not fp16" and on.refusal(h.half()) == "not fp16"  # fp32 always; fp16 hidden on bf16 factors
    assert _att(kv_bf16=True).half().refusal(h) == "mixed dtypes"                    # bf16 hidden, fp16 factors
    assert _att(kv_bf16=True).refusal(h) == "mixed dtypes"                           # ... or fp32 factors
    half_v = _att(kv_bf16=True).bfloat16()
    half_v.v_proj.ALinear.half()
    assert half_v.refusal(h) == "mixed dtypes"
    biased = _att(kv_bf16=True, bias=True).bfloat16()
    assert biased.refusal(h) == "not on the device"
    biased.v_proj.ALinear.bias.data = biased.v_proj.ALinear.bias.data.half()
    assert biased.refusal(h) == "mixed dtypes"                                       # a bias of another dtype
    # fp16 modules do not see the switch
    assert _att(kv_bf16=True).half().refusal(h.half()) == "not on the device" and _att().half().refusal(h.half()) == "not on the device"
    assert _att(kv_bf16=True).refusal(h.float()) == "not fp16"
    assert on.refusal(torch.zeros(1, 2, 128, dtype=torch.bfloat16)) == "token count"  # earlier rules keep their place
    # the environment: read when kv_bf16 is None, at construction
    monkeypatch.setenv("ASVD_KV_BF16", "1")
    env = _att().bfloat16()
    assert env.kv_bf16 is True and env.refusal(h) == "not on the device" and _att().half().refusal(h) == "mixed dtypes"
    assert _att(kv_bf16=False).bfloat16().refusal(h) == "not fp16"                   # an explicit argument wins
    monkeypatch.setenv("ASVD_KV_BF16", "0")
    assert _att().bfloat16().refusal(h) == "not fp16"


def test_greedy_decode_passes_the_switch_on(monkeypatch):
    """on the CPU every decode step is refused either way; what is checked is that greedy_decode hands kv_bf16 to its attention layers and that
    the torch path's result does not depend on it"""
    from asvd4llm_amd import kv_cache
    from asvd4llm_amd.model_zoo import random_init_model
    monkeypatch.delenv("ASVD_KV_BF16", raising=False)
    model = random_init_model("tiny-llama", dtype=torch.bfloat16, num_attention_heads=2, num_key_value_heads=2)
    mk = lambda i, o: nn.Linear(i, o, bias=False).bfloat16()
    for l in model.model.layers:
        l.self_attn.k_proj, l.self_attn.v_proj = kv_cache.FactorPair(mk(128, 48), mk(48, 128)), kv_cache.FactorPair(mk(128, 32), mk(32, 128))
    seen = []
    orig = kv_cache.LowRankKVAttention.__init__

    def spy(self, *a, **kw):
        orig(self, *a, **kw)
        seen.append(self.kv_bf16)
    monkeypatch.setattr(kv_cache.LowRankKVAttention, "__init__", spy)
    ids = torch.randint(0, 512, (2, 5), generator=torch.Generator().manual_seed(3))
    toks, a = kv_cache.greedy_decode(model, ids, 2, kv_bf16=True)
    _, b = kv_cache.greedy_decode(model, ids, 2, forced=toks)
    assert seen == [True, True, False, False] and torch.equal(a, b)
    assert kv_cache.decode_routes(model, kv_bf16=True) == ["not on the device"] * 2 and kv_cache.decode_routes(model) == ["not fp16"] * 2
    assert kv_cache.decode_routes(model, kernel=False) == ["switched off"] * 2


# ---- bf16 rows into an int8 cache ---------------------------------------------------------------------------------------------------------

def test_int8_cache_appended_with_bf16_rows_on_the_cpu():
    from asvd4llm_amd import ops
    from asvd4llm_amd.kv_cache import LowRankKVCache
    g = torch.Generator().manual_seed(9)
    fall = lambda r: 10.0 ** (-3.0 * torch.arange(r) / r)
    a = (torch.randn(3, 7, 48, generator=g) * fall(48)).bfloat16()
    b = (torch.randn(3, 7, 80, generator=g) * fall(80)).bfloat16()
    a[1, 2, 40] = 7e4           # beyond fp16: an Inf after .half(), a NaN group
    c = LowRankKVCache(1, 3, 10, (48, 80), "cpu", torch.bfloat16, quant="int8")
    c.append(0, a[:, :4], b[:, :4])
    c.append(0, a[:, 4:5], b[:, 4:5])
    c.append(0, a[:, 5:7], b[:, 5:7], counts=[2, 0, 1])
    lens = [7, 5, 6]
    assert c.host_lens[0] == lens and c.ck[0].dtype == torch.int8 and c.dtype == torch.bfloat16
    k, v = c.read(0, 7, torch.bfloat16)
    assert k.dtype == torch.bfloat16 and v.dtype == torch.bfloat16
    want = lambda rows: ops.lowrank_kv_dequant(*ops.lowrank_kv_quant_torch(rows)).bfloat16()
    for s, n in enumerate(lens):
        assert torch.equal(k[s, :n].view(torch.int16), want(a[s, :n]).view(torch.int16))
        assert torch.equal(v[s, :n].view(torch.int16), want(b[s, :n]).view(torch.int16))
        # the codes are those of the fp16 rows: the format is defined on fp16 values
        qc, qs = ops.lowrank_kv_quant_torch(a[s, :n].half())
        assert torch.equal(c.ck[0][s, :n], qc) and torch.equal(c.sk[0][s, :n].view(torch.int32), qs.view(torch.int32))
    assert torch.isnan(k[1, 2, 32:]).all() and not torch.isnan(k[1, 2, :32]).any() and not torch.isnan(k[0]).any()
    kd, _ = c.read(0, 7)   # the cache's own dtype is the default
    assert kd.dtype == torch.bfloat16 and torch.equal(kd[0].view(torch.int16), k[0].view(torch.int16))
