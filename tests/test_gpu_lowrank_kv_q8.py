"""K21 on the device: the int8 low-rank KV cache.  The quantiser kernel against the restatement (tests/lowrank_kv_q8_restate.py) bit for
bit; K20 on codes against K20 on the dequantised cache bit for bit, scores and whole op; the whole op against the fp64 restatement
(tests/lowrank_kv_restate.py) on the dequantised cache; padding, isolation, streams, strides; the modules; the CLI."""
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
from tests import lowrank_kv_q8_restate as Q
from tests import lowrank_kv_restate as R
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

FLOOR = 2.0 ** -9    # K20's own: three fp16 roundings on the kernel's path (q~ or nothing, p, the output), each <= 2^-11 relative
SEEN = {"e_kernel": 0.0, "e_dense": 0.0}


def _i16(t):
    return t.view(torch.int16)


def _i32(t):
    return t.view(torch.int32)


# ---- 5. the quantiser kernel, bit for bit ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("r", [16, 48, 272])
def test_quantiser_kernel_equals_the_restatement(gpu, r):
    from asvd4llm_amd import ops
    ng = Q.n_groups(r)
    for B in (1, 3):
        for n in (1, 5, 33):
            for t0 in (0, 7):
                g = torch.Generator().manual_seed(X.seed_of("k21q", B, n, r, t0))
                x = Q.graded(g, (B * n, r))
                special, _, _ = Q.special_rows(g, r)
                for k in range(0, B * n, 2):   # every other row is one of the named cases, the non-finite ones included
                    x[k] = special[(k // 2 + t0 + n) % 6]
                x = x.view(B, n, r)
                want_c, want_s = Q.quant(x)
                # a larger and wider cache full of sentinels; the destination is the slice [:, t0 : t0 + n, :r]
                codes = torch.full((B + 1, 42, r + 16), -77, dtype=torch.int8, device=gpu)
                scales = torch.full((B + 1, 42, ng + 1), -5.0, dtype=torch.float32, device=gpu)
                c0, s0 = codes.clone(), scales.clone()
                ops.lowrank_kv_quant(x.to(gpu), codes[:B, t0:t0 + n, :r], scales[:B, t0:t0 + n, :ng])
                assert torch.equal(codes[:B, t0:t0 + n, :r].cpu(), want_c), (B, n, r, t0)
                assert torch.equal(_i32(scales[:B, t0:t0 + n, :ng].cpu().contiguous()), _i32(want_s)), (B, n, r, t0)
                inside_c, inside_s = torch.zeros_like(codes, dtype=torch.bool), torch.zeros_like(scales, dtype=torch.bool)
                inside_c[:B, t0:t0 + n, :r] = True
                inside_s[:B, t0:t0 + n, :ng] = True
                assert torch.equal(codes[~inside_c], c0[~inside_c]) and torch.equal(scales[~inside_s], s0[~inside_s]), (B, n, r, t0)
                # the torch definition on the device is the same function
                c_t, s_t = ops.lowrank_kv_quant_torch(x.to(gpu))
                assert torch.equal(c_t.cpu(), want_c) and torch.equal(_i32(s_t.cpu()), _i32(want_s))
                assert torch.equal(_i16(ops.lowrank_kv_dequant(c_t, s_t).cpu()), _i16(Q.dequant(want_c, want_s)))


def test_quantiser_wrapper_refuses_before_the_device(gpu):
    from asvd4llm_amd import ops
    x = torch.zeros(2, 3, 48, dtype=torch.float16, device=gpu)
    codes, scales = torch.zeros(2, 3, 48, dtype=torch.int8, device=gpu), torch.zeros(2, 3, 2, device=gpu)
    ops.lowrank_kv_quant(x, codes, scales)
    for bad in [dict(x=x.float()), dict(x=x[:, :, :40]), dict(codes=codes[:, :2]), dict(codes=codes.half()), dict(scales=scales[:, :, :1]),
                dict(scales=scales.double()), dict(codes=torch.zeros(2, 3, 56, dtype=torch.int8, device=gpu)[:, :, :48]), dict(x=x.cpu())]:
        a = {**dict(x=x, codes=codes, scales=scales), **bad}
        with pytest.raises(ValueError):
            ops.lowrank_kv_quant(a["x"], a["codes"], a["scales"])


# ---- 6. scores on codes = scores on the dequantised cache -------------------------------------------------------------------------------------

SCORE_HEADS = [(1, 1), (12, 3), (32, 8), (40, 10)]


@pytest.mark.parametrize("mode", ["none", "half"])
@pytest.mark.parametrize("H,H_kv", SCORE_HEADS)
def test_scores_on_codes_equal_scores_on_the_dequantised_cache(gpu, H, H_kv, mode):
    from asvd4llm_amd import ops
    B = 3
    for T in (1, 31, 32, 33, 127, 128, 129):   # around the 32-token tile and the 4-tile workgroup
        for r_k in (16, 48, 272):              # a 16-wide group alone, a tail group, many groups and a tail
            for D in (64, 128):
                g = torch.Generator().manual_seed(X.seed_of("k21s", H, H_kv, T, r_k, D, mode))
                q = torch.randn(B, H, D, generator=g).half().to(gpu)
                Ak = (torch.randn(H_kv * D, r_k, generator=g) / r_k ** 0.5).half().to(gpu)
                codes, scales = Q.quant(Q.graded(g, (B, T, r_k)))
                dq = Q.dequant(codes, scales).to(gpu)
                lens = torch.tensor([T, T // 2, max(T - 1, 0)], dtype=torch.int32, device=gpu)
                rope = ops.rope_table(T, D, 10000.0, gpu) if mode == "half" else None
                want = ops.lowrank_kv_scores(q, dq, lens, Ak, H_kv, D ** -0.5, rope=rope)
                got = ops.lowrank_kv_scores_q8(q, codes.to(gpu), scales.to(gpu), lens, Ak, H_kv, D ** -0.5, rope=rope)
                assert got.dtype == torch.float32 and got.shape == (B, H, T)
                assert torch.equal(_i32(got), _i32(want)), (H, H_kv, T, r_k, D, mode, (got != want).sum().item())
                assert got[0].abs().max().item() > 0


# ---- 7. the whole op ------------------------------------------------------------------------------------------------------------------------

# (H, H_kv, D, r_k, r_v, with_bv, mode): K20's own list
CONFIGS = [(1, 1, 64, 16, 80, True, "none"), (12, 12, 128, 80, 16, False, "half"), (12, 3, 64, 272, 16, True, "half"), (32, 32, 64, 80, 272, False, "none"),
           (32, 8, 128, 16, 272, True, "none"), (40, 40, 64, 272, 80, True, "half"), (40, 10, 128, 80, 16, False, "none"), (32, 8, 64, 16, 80, False, "half")]


def _data(dev, H, H_kv, D, r_k, r_v, Tmax, B, with_bv, seed):
    """random graded latents quantised by the KERNEL; returns the int8 cache, its dequantised fp16 form and the rest, all on the device"""
    from asvd4llm_amd import ops
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g)
    d = dict(q=rnd(B, H, D).half(), Ak=(rnd(H_kv * D, r_k) / r_k ** 0.5).half(), Av=(rnd(H_kv * D, r_v) / r_v ** 0.5).half(),
             bv=rnd(H_kv * D).half() if with_bv else None)
    d = {k: (v.to(dev) if v is not None else None) for k, v in d.items()}
    for name, r in (("k", r_k), ("v", r_v)):
        x = Q.graded(g, (B, Tmax, r)).to(dev)   # of size ~1 in the leading columns, like ck / cv of K20's test, falling by 10^-3 over the rank
        codes = torch.empty(B, Tmax, r, dtype=torch.int8, device=dev)
        scales = torch.empty(B, Tmax, Q.n_groups(r), dtype=torch.float32, device=dev)
        ops.lowrank_kv_quant(x, codes, scales)
        d["c" + name], d["s" + name], d["d" + name] = codes, scales, ops.lowrank_kv_dequant(codes, scales)
    return d


def _dense_route(d, lens, H_kv, scale, rope):
    """existing code, not the code under test, on the dequantised cache: fp16 F.linear reconstruction of K and V, torch SDPA in fp16"""
    B, H, D = d["q"].shape
    out = torch.zeros(B, H, D, dtype=torch.float16, device=d["q"].device)
    for b in range(B):
        T = lens[b]
        if T == 0:
            continue
        K = F.linear(d["dk"][b, :T], d["Ak"]).view(T, H_kv, D)
        V = F.linear(d["dv"][b, :T], d["Av"], d["bv"]).view(T, H_kv, D)
        if rope is not None:
            K = R.rotate_half_table(K.float().transpose(0, 1), rope[0][:T], rope[1][:T]).transpose(0, 1).half()
        K, V = K.transpose(0, 1).repeat_interleave(H // H_kv, 0), V.transpose(0, 1).repeat_interleave(H // H_kv, 0)
        out[b] = F.scaled_dot_product_attention(d["q"][b][None, :, None, :], K[None], V[None], scale=scale)[0, :, 0]
    return out


def _run_q8(dev, d, lens, H_kv, scale, rope, **kw):
    from asvd4llm_amd import ops
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    return ops.lowrank_kv_decode_q8(d["q"], d["ck"], d["cv"], d["sk"], d["sv"], lens_d, d["Ak"], d["Av"], H_kv, scale, bv=d["bv"], rope=rope, **kw)


def _run_f16(dev, d, lens, H_kv, scale, rope):
    from asvd4llm_amd import ops
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    return ops.lowrank_kv_decode(d["q"], d["dk"], d["dv"], lens_d, d["Ak"], d["Av"], H_kv, scale, bv=d["bv"], rope=rope)


def _whole_op(dev, H, H_kv, D, r_k, r_v, Tmax, lens, with_bv, mode, seed):
    from asvd4llm_amd import ops
    d = _data(dev, H, H_kv, D, r_k, r_v, Tmax, len(lens), with_bv, seed)
    scale = D ** -0.5
    rope = ops.rope_table(Tmax, D, 10000.0) if mode == "half" else None
    rope_d = tuple(t.to(dev) for t in rope) if rope else None
    out = _run_q8(dev, d, lens, H_kv, scale, rope_d)
    same = _run_f16(dev, d, lens, H_kv, scale, rope_d)
    assert torch.equal(_i16(out), _i16(same)), (H, H_kv, D, r_k, r_v, Tmax, lens, mode, (out != same).sum().item())
    cpu = lambda t: t.cpu() if t is not None else None
    ref = R.kv_decode(cpu(d["q"]), cpu(d["dk"]), cpu(d["dv"]), lens, cpu(d["Ak"]), cpu(d["Av"]), H_kv, scale, None, cpu(d["bv"]), rope)
    dense = _dense_route(d, lens, H_kv, scale, rope_d)
    top = ref.abs().max().item()
    e_k = (out.double().cpu() - ref).abs().max().item() / top
    e_d = (dense.double().cpu() - ref).abs().max().item() / top
    print(f"K21 H={H} H_kv={H_kv} D={D} r=({r_k},{r_v}) Tmax={Tmax} lens={lens} bv={with_bv} {mode}: e_kernel={e_k:.3e} e_dense={e_d:.3e}")
    SEEN["e_kernel"], SEEN["e_dense"] = max(SEEN["e_kernel"], e_k), max(SEEN["e_dense"], e_d)
    for b, n in enumerate(lens):
        if n == 0:
            assert torch.equal(out[b].cpu(), torch.zeros(H, D, dtype=torch.float16))
    assert e_k <= max(2 * e_d, FLOOR), (e_k, e_d)
    return d, rope_d, out


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "-".join(map(str, c)))
def test_whole_op_on_codes(gpu, cfg):
    from asvd4llm_amd import ops
    H, H_kv, D, r_k, r_v, with_bv, mode = cfg
    Tmax = 130
    tile, L, ns = ops.lowrank_kv_plan(3, H, Tmax)
    assert (tile, L, ns) == (32, 64, 3)   # the int8 entries take K20's plan: the lengths below sit around its tile and split
    cases = [[1, tile - 1, tile], [tile + 1, L - 1, L], [L + 1, 2 * L + 1, Tmax], [0, 1, Tmax]]
    for n, lens in enumerate(cases):
        _whole_op(gpu, H, H_kv, D, r_k, r_v, Tmax, lens, with_bv, mode, X.seed_of("k21w", n, *cfg[:5]))
    _whole_op(gpu, H, H_kv, D, r_k, r_v, 1, [1], with_bv, mode, X.seed_of("k21w1", *cfg[:5]))
    _whole_op(gpu, H, H_kv, D, r_k, r_v, 33, [33, 32], with_bv, mode, X.seed_of("k21w33", *cfg[:5]))


def test_largest_errors_seen(gpu):
    """prints what profiles/lowrank_kv_q8.json and DESIGN.md cite (the bound is asserted per case above)"""
    print("K21_ERRORS " + json.dumps(SEEN))
    assert SEEN["e_kernel"] > 0.0


# ---- 8. padding and isolation ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cfg", [CONFIGS[2], CONFIGS[4]], ids=["half", "none"])
def test_padding_never_leaks(gpu, cfg):
    H, H_kv, D, r_k, r_v, with_bv, mode = cfg
    Tmax, lens = 130, [0, 37, 65]
    d, rope_d, out = _whole_op(gpu, H, H_kv, D, r_k, r_v, Tmax, lens, with_bv, mode, 77)
    assert torch.equal(out[0], torch.zeros_like(out[0]))
    for code_fill in (127, -128):
        for scale_fill in (float("nan"), float("inf"), 3e38):
            bad = dict(d)
            for k in ("ck", "cv", "sk", "sv"):
                bad[k] = d[k].clone()
            for b, n in enumerate(lens):
                bad["ck"][b, n:] = code_fill
                bad["cv"][b, n:] = code_fill
                bad["sk"][b, n:] = scale_fill
                bad["sv"][b, n:] = scale_fill
            again = _run_q8(gpu, bad, lens, H_kv, D ** -0.5, rope_d)
            assert torch.equal(_i16(again), _i16(out)), (code_fill, scale_fill)


@pytest.mark.parametrize("cfg", [CONFIGS[2], CONFIGS[3]], ids=["half", "none"])
def test_isolation_determinism_and_streams(gpu, cfg):
    from asvd4llm_amd import ops
    H, H_kv, D, r_k, r_v, with_bv, mode = cfg
    Tmax, lens = 130, [130, 70, 129]
    d, rope_d, out = _whole_op(gpu, H, H_kv, D, r_k, r_v, Tmax, lens, with_bv, mode, 78)
    scale = D ** -0.5
    assert torch.equal(_i16(_run_q8(gpu, d, lens, H_kv, scale, rope_d)), _i16(out))
    for which in ("sk", "sv"):
        bad = dict(d)
        bad[which] = d[which].clone()
        bad[which][0, 3, 0] = float("nan")
        o_bad = _run_q8(gpu, bad, lens, H_kv, scale, rope_d)
        assert not torch.isfinite(o_bad[0]).all(), which
        assert torch.equal(_i16(o_bad[1:]), _i16(out[1:])), which
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        work = ops.lowrank_kv_work(3, H, Tmax, r_k, r_v, gpu)
        o_side = _run_q8(gpu, d, lens, H_kv, scale, rope_d, work=work)
    side.synchronize()
    assert torch.equal(_i16(o_side), _i16(out))


def test_strided_code_and_scale_views(gpu):
    H, H_kv, D, r_k, r_v, with_bv, mode = CONFIGS[7]
    Tmax, lens = 70, [70, 33, 64]
    d, rope_d, out = _whole_op(gpu, H, H_kv, D, r_k, r_v, Tmax, lens, with_bv, mode, 79)

    def view(c, pad, fill):
        big = torch.full((c.shape[0] + 1, Tmax + 2, c.shape[2] + pad), fill, dtype=c.dtype, device=gpu)
        big[: c.shape[0], :Tmax, : c.shape[2]] = c
        return big[: c.shape[0], :Tmax, : c.shape[2]]

    strided = dict(d, ck=view(d["ck"], 16, -128), cv=view(d["cv"], 48, 127), sk=view(d["sk"], 1, float("nan")), sv=view(d["sv"], 3, float("nan")))
    assert not strided["ck"].is_contiguous() and strided["ck"].stride(1) == r_k + 16 and strided["sk"].stride(1) == Q.n_groups(r_k) + 1
    assert torch.equal(_i16(_run_q8(gpu, strided, lens, H_kv, D ** -0.5, rope_d)), _i16(out))
    with pytest.raises(ValueError):
        _run_q8(gpu, dict(d, ck=view(d["ck"], 8, 0)), lens, H_kv, D ** -0.5, rope_d)    # a row stride of 8 bytes more: 16 bytes for fp16, not for codes
    with pytest.raises(ValueError):
        _run_q8(gpu, dict(d, cv=view(d["cv"], 4, 0)), lens, H_kv, D ** -0.5, rope_d)
    with pytest.raises(ValueError):
        _run_q8(gpu, dict(d, sk=d["sk"][:, :, :0]), lens, H_kv, D ** -0.5, rope_d)


# ---- 9. modules -------------------------------------------------------------------------------------------------------------------------------

def _attention(dev, rope_mode, seed=5, r_k=48, r_v=32, H=4, k_bias=False):
    """BLinear weights are signed powers of two falling over the rank and the hidden states small integers, so the latents are EXACT in fp16,
    fp32 and fp64 alike: every run below, whatever its precision, quantises the same rows to the same codes"""
    from asvd4llm_amd import ops
    from asvd4llm_amd.kv_cache import FactorPair, LowRankKVAttention
    g = torch.Generator().manual_seed(seed)
    hid = 256
    D = hid // H
    mk = lambda i, o, b=False: nn.Linear(i, o, bias=b)

    def pair(r, bias):
        Bl, Al = mk(hid, r), mk(r, hid, bias)
        Bl.weight.data = torch.randint(-1, 2, (r, hid), generator=g).float() * (2.0 ** -(torch.arange(r) // 8).float())[:, None]
        Al.weight.data = torch.randn(hid, r, generator=g) / r ** 0.5
        return FactorPair(Bl, Al)
    q_proj, o_proj = mk(hid, hid), mk(hid, hid)
    q_proj.weight.data = torch.randn(hid, hid, generator=g) / hid ** 0.5 / 4
    o_proj.weight.data = torch.randn(hid, hid, generator=g) / hid ** 0.5
    rope = ops.rope_table(16, D, 10000.0, dev) if rope_mode == "half" else None
    att = LowRankKVAttention(q_proj, pair(r_k, k_bias), pair(r_v, rope_mode == "none"), o_proj, H, H, rope=rope)
    return att.half().to(dev)


def _run_steps(att, hidden, dtype, kernel, hook=None, quant="int8"):
    from asvd4llm_amd.kv_cache import LowRankKVCache
    att = copy.deepcopy(att).to(dtype)
    att.kernel = kernel
    if hook is not None:
        hook(att)
    cache = LowRankKVCache(1, hidden.shape[0], 16, att.ranks, hidden.device, dtype, quant=quant)
    with torch.no_grad():
        outs = [att.prefill(hidden[:, :7].to(dtype), cache, 0)[:, -1:]]
        for s in range(7, 12):
            outs.append(att.decode(hidden[:, s:s + 1].to(dtype), cache, 0))
    return torch.cat(outs, 1).double(), cache


def _same_cache(a, b, n=12):
    return all(torch.equal(x[0][:, :n].cpu(), y[0][:, :n].cpu()) for x, y in ((a.ck, b.ck), (a.cv, b.cv))) \
        and all(torch.equal(_i32(x[0][:, :n].cpu().contiguous()), _i32(y[0][:, :n].cpu().contiguous())) for x, y in ((a.sk, b.sk), (a.sv, b.sv))) \
        and a.host_lens == b.host_lens and torch.equal(a.lens.cpu(), b.lens.cpu())


@pytest.mark.parametrize("rope_mode", ["none", "half"])
def test_attention_wrapper_on_an_int8_cache(gpu, rope_mode):
    from asvd4llm_amd.kv_cache import LowRankKVCache
    att = _attention(gpu, rope_mode)
    g = torch.Generator().manual_seed(6)
    hidden = torch.randint(-2, 3, (2, 12, 256), generator=g).half().to(gpu)
    assert att.refusal(hidden[:, :1]) is None
    ref, c_ref = _run_steps(att, hidden, torch.float64, False)           # the wrapper's torch path in fp64, on the same codes
    torch_fp16, c_t = _run_steps(att, hidden, torch.float16, False)      # the same path in fp16: the dense route of this test
    kern, c_k = _run_steps(att, hidden, torch.float16, True)
    assert c_k.ck[0].dtype == torch.int8 and c_k.sk[0].dtype == torch.float32
    assert _same_cache(c_k, c_t) and _same_cache(c_k, c_ref)             # exact latents: one set of codes for all three runs
    top = ref[:, 1:].abs().max().item()
    e_k = (kern - ref)[:, 1:].abs().max().item() / top
    e_d = (torch_fp16 - ref)[:, 1:].abs().max().item() / top
    print(f"K21 wrapper {rope_mode}: e_kernel={e_k:.3e} e_dense={e_d:.3e}")
    assert e_k <= max(2 * e_d, FLOOR), (e_k, e_d)
    assert not torch.equal(kern[:, 1:], torch_fp16[:, 1:])               # the two routes are different arithmetic: the kernel did run
    assert torch.equal(kern[:, :1], torch_fp16[:, :1])                   # prefill is the torch path on both
    plain, _ = _run_steps(att, hidden, torch.float16, True, quant=None)
    assert not torch.equal(plain, kern)                                  # and the cache really quantised
    # every refusal lands on the torch path, with the int8 cache as the kernel's run leaves it
    one = hidden[:, :1]

    class Packed(nn.Linear):
        pass

    def packed(a):
        a.v_proj.ALinear.__class__ = Packed
    hooks = {"hooks": lambda a: a.k_proj.BLinear.register_forward_hook(lambda m, i, o: None), "packed factors": packed}
    for why, hook in hooks.items():
        a = copy.deepcopy(att)
        hook(a)
        assert a.refusal(one) == why
        got, c = _run_steps(att, hidden, torch.float16, True, hook=hook)
        assert torch.equal(got, torch_fp16) and _same_cache(c, c_k), why
    a = copy.deepcopy(att)
    a.kernel = False
    assert a.refusal(one) == "switched off"                              # torch_fp16 above is this run
    # two tokens in one decode call
    assert att.refusal(hidden[:, :2]) == "token count"
    c2 = LowRankKVCache(1, 2, 16, att.ranks, gpu, torch.float16, quant="int8")
    with torch.no_grad():
        att.prefill(hidden[:, :7], c2, 0)
        two = att.decode(hidden[:, 7:9], c2, 0)
    assert (two.double() - ref[:, 1:3]).abs().max().item() / top <= max(2 * e_d, FLOOR) and c2.host_lens[0] == [9, 9]
    assert torch.equal(c2.ck[0][:, :9], c_k.ck[0][:, :9]) and torch.equal(_i32(c2.sv[0][:, :9].contiguous()), _i32(c_k.sv[0][:, :9].contiguous()))
    # fp32 modules and inputs: the cache quantises through .half(), the same codes again
    assert att.refusal(one.float()) == "not fp16"
    f32, c32 = _run_steps(att, hidden, torch.float32, True)
    assert _same_cache(c32, c_k) and (f32 - ref)[:, 1:].abs().max().item() / top <= max(2 * e_d, FLOOR)
    with torch.enable_grad():
        assert att.refusal(one.clone().requires_grad_(True)) == "autograd"
    # on the CPU
    assert att.refusal(one.cpu()) == "not on the device"
    on_cpu = copy.deepcopy(att).cpu()
    on_cpu.rope = tuple(t.cpu() for t in att.rope) if att.rope else None
    cpu, c_cpu = _run_steps(on_cpu, hidden.cpu(), torch.float32, True)
    assert _same_cache(c_cpu, c_k) and (cpu - ref.cpu())[:, 1:].abs().max().item() / top <= max(2 * e_d, FLOOR)
    # shapes the kernel does not serve
    small = _attention(gpu, rope_mode, H=8)
    assert small.refusal(one) == "head size"
    a_t, c_a = _run_steps(small, hidden, torch.float16, False)
    a_k, c_b = _run_steps(small, hidden, torch.float16, True)
    assert torch.equal(a_t, a_k) and _same_cache(c_a, c_b)
    if rope_mode == "half":
        biased = _attention(gpu, rope_mode, k_bias=True)
        assert biased.refusal(one) == "key bias under rotation"
        a_t, c_a = _run_steps(biased, hidden, torch.float16, False)
        a_k, c_b = _run_steps(biased, hidden, torch.float16, True)
        assert torch.equal(a_t, a_k) and _same_cache(c_a, c_b)
    # a rank that is no multiple of 16 has no int8 form: the cache says so (the fp16 cache serves it on the torch path)
    odd = _attention(gpu, rope_mode, r_k=40)
    assert odd.refusal(one) == "ranks"
    with pytest.raises(ValueError):
        LowRankKVCache(1, 2, 16, odd.ranks, gpu, torch.float16, quant="int8")


def test_greedy_decode_int8_on_compressed_tiny_llama(gpu):
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
    _, dense = greedy_decode(model, ids, n_new, cache="dense", forced=toks_ref)
    _, low16 = greedy_decode(model, ids, n_new, cache="lowrank", kernel=True, forced=toks_ref)
    _, q8_k = greedy_decode(model, ids, n_new, cache="lowrank", kernel=True, forced=toks_ref, kv_quant="int8")
    _, q8_t = greedy_decode(model, ids, n_new, cache="lowrank", kernel=False, forced=toks_ref, kv_quant="int8")
    top = ref.abs().max().item()
    e_dense = (dense.float() - ref).abs().max().item() / top
    e_kt = (q8_k.float() - q8_t.float()).abs().max().item() / top
    e_q = (q8_k.float() - low16.float()).abs().max().item() / top
    print(f"K21 greedy_decode tiny-llama: kernel against torch on the int8 cache {e_kt:.3e} (e_dense={e_dense:.3e}); int8 against fp16 cache {e_q:.3e}")
    assert e_kt <= max(2 * e_dense, 2.0 ** -10), (e_kt, e_dense)   # the margin K20's test gives its kernel against the dense cache
    assert not torch.equal(q8_k[1:], q8_t[1:])                      # decode steps took different arithmetic
    assert not torch.equal(q8_k, low16)                             # the cache really quantised
    c = LowRankKVCache(2, 2, 15, kv_ranks(model), gpu, quant="int8")
    assert c.bytes_per_token() == 2 * 2 * (32 + 4) and c.bytes_per_token() * 16 == 9 * LowRankKVCache(2, 2, 15, kv_ranks(model), gpu).bytes_per_token()


# ---- 10. CLI ----------------------------------------------------------------------------------------------------------------------------------

def test_cli_kv_cache_decode_int8(gpu, tmp_path):
    # not ASVD_STRICT, for the reason tests/test_gpu_lowrank_kv.py gives: the kv-cache sweep tries ratios whose aligned ranks pass this model's width
    env = dict(os.environ, PYTHONPATH=ROOT)
    env.pop("ASVD_STRICT", None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "asvd.py"), "--model_id", "tiny-llama", "--random_init", "--act_aware", "--alpha", "0.5",
                          "--n_calib_samples", "4", "--calib_dataset", "synthetic", "--scaling_method", "abs_mean", "--compress_kv_cache",
                          "--kv_cache_ratio_target", "0.5", "--rank_align", "16", "--kv_cache_decode_tokens", "4", "--kv_cache_quant", "int8"],
                         cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    m = re.search(r"kv cache bytes per token: dense (\d+), low-rank (\d+) \(ratio ([0-9.]+)\)", out.stdout)
    assert m, out.stdout[-2000:]
    dense, low = int(m.group(1)), int(m.group(2))
    m = re.search(r"kv cache bytes per token: int8 low-rank (\d+) \(ratio ([0-9.]+) of dense, ([0-9.]+) of low-rank\); int8 layers: \[([0-9, ]*)\]",
                  out.stdout)
    assert m, out.stdout[-2000:]
    low8 = int(m.group(1))
    assert 0 < low8 < low < dense, (low8, low, dense)
    assert abs(float(m.group(2)) - low8 / dense) < 1e-3 and abs(float(m.group(3)) - low8 / low) < 1e-3
    ranks = [int(x) for x in re.findall(r"\d+", re.search(r"kv cache ranks \(k, v\) per layer: (.*)", out.stdout).group(1))]
    q8_layers = [int(x) for x in re.findall(r"\d+", m.group(4))]
    assert len(ranks) == 4 and q8_layers and all(i in q8_layers for i in range(2) if min(ranks[2 * i:2 * i + 2]) < 128)   # a layer the search compressed is int8
    # a byte per code and 4 per group where the layer is int8; a layer the search left uncompressed keeps fp16 K and V
    assert low8 == sum(sum(r + 4 * Q.n_groups(r) for r in ranks[2 * i:2 * i + 2]) if i in q8_layers else 2 * sum(ranks[2 * i:2 * i + 2]) for i in range(2))
    m = re.search(r"kv cache decode, int8 low-rank cache: 4 tokens, largest logit difference ([0-9.eE+-]+) against the dense cache "
                  r"\(fp16 low-rank cache: ([0-9.eE+-]+)\)", out.stdout)
    assert m, out.stdout[-2000:]
    d8, d16 = float(m.group(1)), float(m.group(2))
    assert d8 == d8 and 0.0 <= d8 < float("inf") and 0.0 <= d16 < float("inf")
