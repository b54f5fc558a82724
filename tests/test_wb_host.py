"""RTN codes stored at their own width (--weight_quant_storage bitpacked), host side: the storage format against its numpy restatement,
WBLinear's CPU pack and dequantization against W8Linear on the same codes and against the reference-generated fixture, the module's state,
the CLI switch, export and load, and the argument checks of the C entry points.  No GPU."""
import ctypes
import json
import os
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import bitpack_restate as R
from tests.rtn_restate import codes_of, rtn_restate

DT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
WIDTHS = [6, 4]


def _bit_equal(a, b):
    iv = {torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.float32: torch.int32}[a.dtype]
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(iv), b.view(iv))


def _value_equal(a, b):
    """equal values, NaN matching NaN"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.where(np.isnan(a), 0, a), np.where(np.isnan(b), 0, b))


def _codes(rows, K, bits, seed):
    return np.random.default_rng(seed).integers(0, 1 << bits, size=(rows, K), dtype=np.uint8)


# ---- the format -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [1, 15, 16, 63, 64, 65, 1001, 1840])
@pytest.mark.parametrize("bits", WIDTHS)
def test_restatement_round_trip(K, bits):
    q = _codes(7, K, bits, K + bits)
    q[0] = (1 << bits) - 1                                            # every bit of every code set: a lost or misplaced bit shows
    p = R.pack(q, bits)
    assert p.dtype == np.uint8 and p.shape == (7, R.row_bytes(K, bits)) == (7, -(-K // 64) * 8 * bits)
    assert R.row_bytes(K, bits) % 16 == 0 and R.row_bytes(64, 6) == 48 and R.row_bytes(64, 4) == 32 and R.row_bytes(1840, 6) == 29 * 48
    back, padding = R.unpack(p, bits, K)
    assert np.array_equal(back, q) and not padding.any()
    for k in sorted({0, K - 1, min(5, K - 1), min(10, K - 1), min(21, K - 1), min(26, K - 1)}):   # 5 and 10 of a group of 16 straddle a word
        assert np.array_equal(R.word_reading(p, bits, k), q[:, k]), k
    # code k sits in bits [bits k, bits (k + 1)) of the row read as ONE little-endian integer
    row = int.from_bytes(p[1].tobytes(), "little")
    assert [(row >> (bits * k)) & ((1 << bits) - 1) for k in range(K)] == q[1].tolist()


def test_which_codes_straddle_a_word():
    for bits, want in ((6, [5, 10]), (4, [])):
        assert [k for k in range(16) if (bits * k) // 32 != (bits * k + bits - 1) // 32] == want


@pytest.mark.parametrize("K", [1, 15, 16, 63, 64, 65, 1001, 1840])
@pytest.mark.parametrize("bits", WIDTHS)
def test_cpu_pack_equals_the_restatement(K, bits):
    from asvd4llm_amd.modules.wb_linear import WBLinear
    q = _codes(5, K, bits, 3 * K + bits)
    m = WBLinear.from_codes(torch.from_numpy(q), torch.ones(5), torch.zeros(5), None, bits, torch.float32)
    assert m.qbits.dtype == torch.uint8 and np.array_equal(m.qbits.numpy(), R.pack(q, bits))
    assert m.in_features == K and m.out_features == 5 and np.array_equal(m.codes().numpy(), q)
    # codes beyond the width are masked, not spilled into the neighbours
    wide = torch.from_numpy(q) | 0xc0
    assert torch.equal(WBLinear.from_codes(wide, torch.ones(5), torch.zeros(5), None, bits, torch.float32).qbits,
                       torch.from_numpy(R.pack(q & ((1 << bits) - 1), bits)))


# ---- CPU dequantization -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(37, 70), (128, 352), (64, 4096)])
@pytest.mark.parametrize("dt", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("bits", WIDTHS)
def test_cpu_dequantize_equals_w8linear_on_the_same_codes(shape, dt, bits):
    from asvd4llm_amd.modules.w8_linear import W8Linear
    from asvd4llm_amd.modules.wb_linear import WBLinear
    g = torch.Generator().manual_seed(shape[0] + shape[1] + bits)
    w = (torch.randn(*shape, generator=g) * 0.02).to(DT[dt])
    out, q, scale, zero, ready = rtn_restate(w, bits)
    assert ready
    m8 = W8Linear.from_codes(codes_of(q), scale, zero, None, bits, DT[dt])
    mb = WBLinear.from_codes(codes_of(q), scale, zero, None, bits, DT[dt])
    assert _bit_equal(mb.dequantize(), m8.dequantize()) and _bit_equal(mb.dequantize(), out)
    assert mb.qbits.shape == (shape[0], R.row_bytes(shape[1], bits)) and mb.weight_dtype == DT[dt] and mb.bits == bits
    if dt == "f32":                                                    # CPU forward: F.linear on the dequantized weight
        x = torch.randn(3, shape[1], generator=g)
        assert torch.equal(mb(x), nn.functional.linear(x, out))


def test_cpu_dequantize_on_the_reference_fixture(golden):
    from asvd4llm_amd.modules.wb_linear import WBLinear
    z = golden.npz("rtn_ref.npz")
    for d in ("f16", "bf16", "f32"):
        case = f"{d}_int6"
        q = torch.from_numpy(z[case + "_q"])
        assert int(torch.isnan(q).sum()) > 0                           # the fixture holds non-finite rows: their codes are 0
        m = WBLinear.from_codes(codes_of(q), torch.from_numpy(z[case + "_scale"]), torch.from_numpy(z[case + "_zero"]), None, 6, DT[d])
        w = m.dequantize()
        assert w.dtype == DT[d] and _value_equal(w.float().numpy(), z[case + "_out"]), case


# ---- the module -------------------------------------------------------------------------------------------------------------------

def test_wblinear_state_and_casts():
    from asvd4llm_amd.modules.w8_linear import W8Linear
    from asvd4llm_amd.modules.wb_linear import WBLinear
    from asvd4llm_amd.quantization import _find_linears
    m = WBLinear(70, 8, bias=True, bits=6, weight_dtype=torch.bfloat16)
    assert not isinstance(m, nn.Linear) and not isinstance(m, W8Linear) and not isinstance(W8Linear(4, 4), WBLinear)
    assert _find_linears(nn.Sequential(m, nn.Linear(8, 8)))[0][0] == "1" and len(_find_linears(nn.Sequential(m, nn.Linear(8, 8)))) == 1
    assert {k: (v.dtype, tuple(v.shape)) for k, v in m.state_dict().items()} == {
        "qbits": (torch.uint8, (8, 96)), "scales": (torch.float32, (8,)), "zeros": (torch.float32, (8,)), "bias": (torch.bfloat16, (8,))}
    assert m.in_features == 70 and m.out_features == 8 and not list(m.parameters())
    assert set(WBLinear(64, 3, bias=False, bits=4).state_dict()) == {"qbits", "scales", "zeros"} and WBLinear(64, 3, bits=4).qbits.shape == (3, 32)
    for cast in ("half", "double"):
        getattr(m, cast)()                                             # a dtype cast of the model leaves scale, zero and bias alone
        assert m.scales.dtype == m.zeros.dtype == torch.float32 and m.qbits.dtype == torch.uint8
        assert m.bias.dtype == torch.bfloat16 and m.weight_dtype == torch.bfloat16
    for bad in (8, 5):
        with pytest.raises(ValueError):
            WBLinear(16, 4, bits=bad)
        with pytest.raises(ValueError):
            WBLinear.from_codes(torch.zeros(4, 16, dtype=torch.uint8), torch.ones(4), torch.zeros(4), None, bad, torch.float16)
    with pytest.raises(ValueError):
        WBLinear.from_bits(torch.zeros(4, 47, dtype=torch.uint8), 64, torch.ones(4), torch.zeros(4), None, 6, torch.float16)
    assert not WBLinear(70, 8, bits=6).kernel_rows_ok() and WBLinear(80, 8, bits=6).kernel_rows_ok()


def test_forward_after_a_cast_of_the_model():
    from asvd4llm_amd.modules.wb_linear import WBLinear
    g = torch.Generator().manual_seed(4)
    w = (torch.randn(24, 40, generator=g) * 0.05).half()
    out, q, scale, zero, ready = rtn_restate(w, 6)
    bias = torch.randn(24, generator=g).half()
    m = WBLinear.from_codes(codes_of(q), scale, zero, bias, 6, torch.float16)
    holder = nn.Sequential(m).double()
    assert m.bias.dtype == torch.float16 and m.scales.dtype == torch.float32 and _bit_equal(m.dequantize(), out)
    x = torch.randn(3, 40, generator=g).double()
    assert torch.equal(holder(x), nn.functional.linear(x, out.double(), bias.double()))


# ---- the command line -------------------------------------------------------------------------------------------------------------

def _args(**kw):
    d = dict(weight_quant="rtn_int6", dist=False, gather_factors="rank0")
    d.update(kw)
    return types.SimpleNamespace(**d)


def test_parser_accepts_bitpacked():
    import asvd
    p = asvd.build_parser()
    assert p.parse_args(["--weight_quant", "rtn_int6", "--weight_quant_storage", "bitpacked"]).weight_quant_storage == "bitpacked"
    assert p.parse_args([]).weight_quant_storage == "fake"
    with pytest.raises(SystemExit):
        p.parse_args(["--weight_quant_storage", "int4"])


def test_cli_dispatch(monkeypatch):
    import asvd
    from asvd4llm_amd import quantization
    seen = []
    monkeypatch.setattr(quantization, "rtn_quant_sequential", lambda *a, **k: seen.append(("fake", a, k)))
    monkeypatch.setattr(quantization, "rtn_pack_sequential", lambda *a, **k: seen.append(("pack", a, k)))
    model = object()
    asvd.run_weight_quant(model, _args(weight_quant_storage="bitpacked"))
    assert seen == [("pack", (model, 6), {"storage": "bits"})]
    with pytest.raises(ValueError, match="use packed"):
        asvd.run_weight_quant(model, _args(weight_quant="rtn_int8", weight_quant_storage="bitpacked"))
    assert len(seen) == 1
    seen.clear()
    asvd.run_weight_quant(model, _args(weight_quant_storage="fake"))
    asvd.run_weight_quant(model, _args(weight_quant_storage="packed"))
    asvd.run_weight_quant(model, _args(weight_quant="rtn_int8", weight_quant_storage="packed"))
    assert seen == [("fake", (model, 6), {}), ("pack", (model, 6), {}), ("pack", (model, 8), {})]   # two positional arguments, as before


def test_cli_bitpacks_on_the_ranks_that_hold_factors(monkeypatch):
    import asvd
    from asvd4llm_amd import quantization
    seen = []
    monkeypatch.setattr(quantization, "rtn_pack_sequential", lambda model, wbits, **k: seen.append((wbits, k)))
    monkeypatch.setenv("RANK", "1")
    asvd.run_weight_quant(None, _args(dist=True, gather_factors="rank0", weight_quant_storage="bitpacked"))
    assert seen == []
    asvd.run_weight_quant(None, _args(dist=True, gather_factors="all", weight_quant_storage="bitpacked"))
    assert seen == [(6, {"storage": "bits"})]
    monkeypatch.setenv("RANK", "0")
    asvd.run_weight_quant(None, _args(dist=True, gather_factors="rank0", weight_quant_storage="bitpacked"))
    assert seen == [(6, {"storage": "bits"})] * 2


def test_rtn_pack_sequential_refuses_other_widths_and_storages():
    from asvd4llm_amd.quantization import rtn_pack_sequential
    for bits in (8, 5, 3):
        with pytest.raises(ValueError, match="4 or 6"):
            rtn_pack_sequential(nn.Linear(4, 4), bits, storage="bits")   # before the model is looked at
    with pytest.raises(ValueError, match="storage"):
        rtn_pack_sequential(nn.Linear(4, 4), 6, storage="nibbles")


# ---- export -----------------------------------------------------------------------------------------------------------------------

def _bitpacked(w, bits, bias=None):
    from asvd4llm_amd.modules.wb_linear import WBLinear
    out, q, scale, zero, ready = rtn_restate(w, bits)
    assert ready
    return WBLinear.from_codes(codes_of(q), scale, zero, bias, bits, w.dtype)


def _bitpacked_svdlinear(in_f, out_f, rank, bits, seed=0, dtype=torch.float32):
    from asvd4llm_amd.modules.svd_linear import SVDLinear
    g = torch.Generator().manual_seed(seed)
    A = (torch.randn(out_f, rank, generator=g) * 0.05).to(dtype)
    B = (torch.randn(rank, in_f, generator=g) * 0.05).to(dtype)
    m = SVDLinear._from_factors(A, B, None, rank)
    m.ALinear, m.BLinear = _bitpacked(A, bits), _bitpacked(B, bits)
    return m


def test_export_round_trip_on_the_host(tmp_path):
    from asvd4llm_amd.export import load_asvd_repo, save_asvd_repo
    from asvd4llm_amd.model_zoo import random_init_model
    from asvd4llm_amd.modules.w8_linear import W8Linear
    from asvd4llm_amd.modules.wb_linear import WBLinear
    model = random_init_model("tiny-llama", dtype=torch.float32)
    layer = model.model.layers[0]
    lin = layer.mlp.down_proj
    layer.mlp.down_proj = _bitpacked_svdlinear(lin.in_features, lin.out_features, 5, 6)
    q_w = layer.self_attn.q_proj.weight.data
    path = str(tmp_path / "repo")
    layer.self_attn.q_proj = _bitpacked(q_w, 4)
    with pytest.raises(ValueError, match="bit widths"):
        save_asvd_repo(model, path)                                    # 6-bit factors next to a 4-bit layer: refused
    out, q, scale, zero, _ = rtn_restate(q_w, 6)
    layer.self_attn.q_proj = W8Linear.from_codes(codes_of(q), scale, zero, None, 6, torch.float32)
    with pytest.raises(ValueError, match="storage form"):
        save_asvd_repo(model, path)                                    # one code per byte next to bit-packed: refused
    layer.self_attn.q_proj = _bitpacked(q_w, 6)
    ranks = save_asvd_repo(model, path)
    assert ranks == {"model.layers.0.mlp.down_proj": 5}
    cfg = json.load(open(os.path.join(path, "config.json")))
    assert cfg["weight_quant"] == {"method": "rtn", "bits": 6, "storage": "bitstream64"} and "auto_map" not in cfg
    assert not [f for f in os.listdir(path) if f.endswith(".py")]
    with pytest.raises(ValueError, match="packed from float32"):
        load_asvd_repo(path, dtype=torch.float16)
    loaded = load_asvd_repo(path, dtype=torch.float32)
    want = {n: m for n, m in model.named_modules() if isinstance(m, WBLinear)}
    have = {n: m for n, m in loaded.named_modules() if isinstance(m, WBLinear)}
    assert set(want) == set(have) and len(want) == 3
    for n in want:
        assert (have[n].in_features, have[n].out_features, have[n].bits) == (want[n].in_features, want[n].out_features, 6), n
        for key in ("qbits", "scales", "zeros"):
            assert torch.equal(getattr(want[n], key), getattr(have[n], key)), (n, key)
    assert "model.layers.0.self_attn.q_proj.qbits" in loaded.state_dict()
    ids = torch.randint(0, model.config.vocab_size, (1, 6), generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        assert torch.equal(loaded(input_ids=ids)[0], model.eval()(input_ids=ids)[0])
    # rows that are not the bitstream of the architecture's in_features are refused
    cfg["weight_quant"]["bits"] = 4
    json.dump(cfg, open(os.path.join(path, "config.json"), "w"))
    with pytest.raises(ValueError, match="does not fit"):
        load_asvd_repo(path, dtype=torch.float32)


# ---- C entry points ---------------------------------------------------------------------------------------------------------------

def test_row_bytes_query(built_lib):
    from asvd4llm_amd import ops
    lib = built_lib
    for K in (1, 63, 64, 65, 1840, 4096, 11008):
        for bits in (4, 6):
            assert lib.asvd_wb_row_bytes(K, bits) == R.row_bytes(K, bits) == ops.wb_row_bytes(K, bits)
    for K, bits in ((64, 8), (64, 5), (64, 0), (0, 6), (-3, 4)):
        assert lib.asvd_wb_row_bytes(K, bits) == -1
        with pytest.raises(ValueError):
            ops.wb_row_bytes(K, bits)


def test_wb_entry_points_reject_bad_arguments_without_device(built_lib):
    lib = built_lib
    p, nul = ctypes.c_void_p(4096), None   # non-null but never dereferenced: every check below fails before any HIP call
    ok = dict(x=p, T=4, q=p, ld=48, bits=6, scale=p, zero=p, bias=nul, N=8, K=64, y=p)

    def linear(**kw):
        a = dict(ok, **kw)
        return lib.asvd_wb_linear_f16(a["x"], a["T"], a["q"], a["ld"], a["bits"], a["scale"], a["zero"], a["bias"], a["N"], a["K"], a["y"], nul)

    for bad in (dict(x=nul), dict(q=nul), dict(scale=nul), dict(zero=nul), dict(y=nul), dict(T=0), dict(T=257), dict(N=0), dict(K=0), dict(bits=5),
                dict(bits=8), dict(K=72, ld=96), dict(K=65, ld=96), dict(ld=32), dict(ld=47), dict(ld=56), dict(K=128, ld=48),
                dict(x=ctypes.c_void_p(4098)), dict(x=ctypes.c_void_p(4104)), dict(q=ctypes.c_void_p(4100)), dict(y=ctypes.c_void_p(4097)),
                dict(bias=ctypes.c_void_p(4097))):
        assert linear(**bad) == -1, bad
    assert linear(bits=4, ld=16) == -1 and linear(bits=4, ld=40) == -1      # 4 bits: a row of 64 codes is 32 bytes; 40 is not 16-byte aligned

    def pack(q=p, ldq=64, rows=8, cols=64, bits=6, out=p, ld=48):
        return lib.asvd_wb_pack(q, ldq, rows, cols, bits, out, ld, nul)

    for bad in (dict(q=nul), dict(out=nul), dict(ldq=63), dict(ld=47), dict(ld=44), dict(bits=5), dict(bits=8), dict(rows=0), dict(cols=0),
                dict(cols=65, ldq=65), dict(out=ctypes.c_void_p(4098))):
        assert pack(**bad) == -1, bad

    def dequant(q=p, ld=48, bits=6, scale=p, zero=p, rows=8, cols=64, out=p, dt=1, ldo=64):
        return lib.asvd_wb_dequant(q, ld, bits, scale, zero, rows, cols, out, dt, ldo, nul)

    for bad in (dict(q=nul), dict(scale=nul), dict(zero=nul), dict(out=nul), dict(ld=47), dict(bits=5), dict(bits=8), dict(rows=0), dict(cols=0),
                dict(cols=65, ldo=65), dict(ldo=63), dict(dt=5), dict(out=ctypes.c_void_p(4097)), dict(out=ctypes.c_void_p(4098), dt=0),
                dict(q=ctypes.c_void_p(4098))):
        assert dequant(**bad) == -1, bad


def test_ops_wb_have_no_cpu_fallback():
    from asvd4llm_amd import _lib, ops
    q = torch.zeros(4, 16, dtype=torch.uint8)
    qb = torch.zeros(4, 48, dtype=torch.uint8)
    with pytest.raises(_lib.AsvdHipError):
        ops.wb_pack(q, 6)
    with pytest.raises(_lib.AsvdHipError):
        ops.wb_dequant(qb, 6, 16, torch.ones(4), torch.zeros(4), torch.float16)
    with pytest.raises(_lib.AsvdHipError):
        ops.wb_linear(torch.zeros(2, 16).half(), qb, 6, torch.ones(4), torch.zeros(4))
