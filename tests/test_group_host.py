"""Group-wise RTN quantization (--weight_quant_group_size), host side: the restatement's accuracy on factor-shaped weights (the feature's
purpose), the CPU dequantization of grouped W8Linear / WBLinear modules against the restatement, the command-line wiring, the export's config key
and shape check, and the argument checks of the grouped C entry points.  No GPU."""
import ctypes
import json
import os
import types

import pytest
import torch
import torch.nn as nn

from tests.group_restate import GROUPS, graded_matrix, group_restate, n_groups, rel_err
from tests.rtn_restate import codes_of, rtn_restate


def _bit_equal(a, b):
    iv = {torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.float32: torch.int32}[a.dtype]
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(iv), b.view(iv))


# ---- the restatement ----------------------------------------------------------------------------------------------------------------

def test_restatement_of_one_group_is_the_row_restatement():
    g = torch.Generator().manual_seed(0)
    w = (torch.randn(9, 300, generator=g) * 0.02).half()
    for G in GROUPS:
        out, q, scale, zero, ready = group_restate(w, 4, G)
        assert ready and scale.shape == zero.shape == (9, n_groups(300, G)) and scale.is_contiguous()
        for j in range(n_groups(300, G)):
            o, qq, s, z, _ = rtn_restate(w[:, j * G:(j + 1) * G], 4)
            assert _bit_equal(out[:, j * G:(j + 1) * G], o) and torch.equal(q[:, j * G:(j + 1) * G], qq)
            assert torch.equal(scale[:, j], s) and torch.equal(zero[:, j], z)
    wide = (torch.randn(9, 64, generator=g) * 0.02).half()        # one whole group: the per-row quantizer
    assert _bit_equal(group_restate(wide, 6, 64)[0], rtn_restate(wide, 6)[0])


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_groups_halve_the_four_bit_error_of_factor_shaped_weights(seed):
    """the 37 x 1104 graded matrix: at 4 bits the relative Frobenius error with groups of 128 is at most 0.6 of the per-row error (measured
    0.505 - 0.512), and groups of 64 are no worse than groups of 128"""
    w = graded_matrix(seed)
    e_row = rel_err(rtn_restate(w, 4)[0], w)
    e128, e64 = (rel_err(group_restate(w, 4, G)[0], w) for G in (128, 64))
    print(f"seed {seed}: per row {e_row:.4f} G=128 {e128:.4f} ({e128 / e_row:.3f}x) G=64 {e64:.4f} ({e64 / e_row:.3f}x)")
    assert e128 <= 0.6 * e_row
    assert e64 <= e128


# ---- modules ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("G", GROUPS)
@pytest.mark.parametrize("bits", [8, 6, 4])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32])
def test_cpu_dequantize_of_grouped_modules_equals_the_restatement(G, bits, dtype):
    from asvd4llm_amd.modules.w8_linear import W8Linear
    from asvd4llm_amd.modules.wb_linear import WBLinear
    g = torch.Generator().manual_seed(G + bits)
    for out_f, in_f in ((24, 352), (7, 1001), (5, 16), (3, 128)):   # a ragged last group, an odd one, one short group, exactly one / two groups
        w = (torch.randn(out_f, in_f, generator=g) * 0.05).to(dtype)
        out, q, scale, zero, ready = group_restate(w, bits, G)
        assert ready
        m = W8Linear.from_codes(codes_of(q), scale, zero, None, bits, dtype, group_size=G)
        assert m.group_size == G and m.scales.shape == (out_f, n_groups(in_f, G)) and _bit_equal(m.dequantize(), out)
        assert f"group_size={G}" in m.extra_repr()
        if bits != 8:
            mb = WBLinear.from_codes(codes_of(q), scale, zero, None, bits, dtype, group_size=G)
            assert mb.group_size == G and _bit_equal(mb.dequantize(), out) and f"group_size={G}" in mb.extra_repr()
            x = torch.randn(3, in_f, generator=g).to(dtype)
            assert torch.equal(mb(x), nn.functional.linear(x, out)) and torch.equal(m(x), mb(x))


def test_module_shapes_and_refusals():
    from asvd4llm_amd.modules.w8_linear import W8Linear
    from asvd4llm_amd.modules.wb_linear import WBLinear
    assert W8Linear(352, 8).scales.shape == (8,) and W8Linear(352, 8).group_size == 0 and "group_size" not in W8Linear(352, 8).extra_repr()
    assert W8Linear(352, 8, group_size=128).scales.shape == (8, 3) and W8Linear(352, 8, group_size=64).zeros.shape == (8, 6)
    assert WBLinear(352, 8, bits=4, group_size=128).scales.shape == (8, 3) and WBLinear(352, 8, bits=4).zeros.shape == (8,)
    assert WBLinear(352, 8, bits=4, group_size=64).kernel_rows_ok() and not WBLinear(360, 8, bits=4, group_size=64).kernel_rows_ok()
    for bad in (32, 256, 1, -64):
        with pytest.raises(ValueError, match="group_size"):
            W8Linear(352, 8, group_size=bad)
        with pytest.raises(ValueError, match="group_size"):
            WBLinear(352, 8, bits=4, group_size=bad)
    q = torch.zeros(8, 352, dtype=torch.uint8)
    with pytest.raises(ValueError, match="scales / zeros"):
        W8Linear.from_codes(q, torch.ones(8), torch.zeros(8), None, 4, torch.float16, group_size=128)      # per-row parameters for a grouped layer
    with pytest.raises(ValueError, match="scales / zeros"):
        WBLinear.from_codes(q, torch.ones(8, 6), torch.zeros(8, 6), None, 4, torch.float16, group_size=128)  # the parameters of G = 64
    m = nn.Sequential(W8Linear(352, 8, group_size=128, weight_dtype=torch.float16)).double()                # a cast of the model keeps fp32
    assert m[0].scales.dtype == torch.float32 and m[0].scales.shape == (8, 3)


# ---- the command line ---------------------------------------------------------------------------------------------------------------

def _args(**kw):
    d = dict(weight_quant="rtn_int4", dist=False, gather_factors="rank0")
    d.update(kw)
    return types.SimpleNamespace(**d)


def test_parser_takes_the_group_size_and_rtn_int4():
    import asvd
    p = asvd.build_parser()
    assert p.parse_args([]).weight_quant_group_size == 0
    for G in (0, 64, 128):
        a = p.parse_args(["--weight_quant", "rtn_int4", "--weight_quant_storage", "bitpacked", "--weight_quant_group_size", str(G)])
        assert (a.weight_quant, a.weight_quant_storage, a.weight_quant_group_size) == ("rtn_int4", "bitpacked", G)
    with pytest.raises(SystemExit):
        p.parse_args(["--weight_quant_group_size", "32"])


def test_cli_passes_the_group_size_only_when_it_is_set(monkeypatch):
    import asvd
    from asvd4llm_amd import quantization
    seen = []
    monkeypatch.setattr(quantization, "rtn_quant_sequential", lambda *a, **k: seen.append(("fake", a, k)))
    monkeypatch.setattr(quantization, "rtn_pack_sequential", lambda *a, **k: seen.append(("pack", a, k)))
    model = object()
    for storage in ("fake", "packed", "bitpacked"):
        asvd.run_weight_quant(model, _args(weight_quant_storage=storage))                               # no group size on the namespace
        asvd.run_weight_quant(model, _args(weight_quant_storage=storage, weight_quant_group_size=0))
        asvd.run_weight_quant(model, _args(weight_quant_storage=storage, weight_quant_group_size=128))
    assert seen == [("fake", (model, 4), {}), ("fake", (model, 4), {}), ("fake", (model, 4), {"group_size": 128}),
                    ("pack", (model, 4), {}), ("pack", (model, 4), {}), ("pack", (model, 4), {"group_size": 128}),
                    ("pack", (model, 4), {"storage": "bits"}), ("pack", (model, 4), {"storage": "bits"}),
                    ("pack", (model, 4), {"storage": "bits", "group_size": 128})]
    seen.clear()
    asvd.run_weight_quant(model, _args(weight_quant="rtn_int8", weight_quant_storage="packed", weight_quant_group_size=64))
    assert seen == [("pack", (model, 8), {"group_size": 64})]
    with pytest.raises(ValueError, match="group_size"):
        asvd.run_weight_quant(model, _args(weight_quant_group_size=32))
    assert len(seen) == 1


def test_sequential_steps_refuse_other_group_sizes_before_the_model_is_looked_at():
    from asvd4llm_amd.quantization import rtn_pack_sequential, rtn_quant_sequential
    for G in (32, 96, 256):
        with pytest.raises(ValueError, match="group_size"):
            rtn_quant_sequential(nn.Linear(4, 4), 4, group_size=G)
        with pytest.raises(ValueError, match="group_size"):
            rtn_pack_sequential(nn.Linear(4, 4), 4, storage="bits", group_size=G)


# ---- export -------------------------------------------------------------------------------------------------------------------------

def _grouped(w, bits, G, kind):
    from asvd4llm_amd.modules.w8_linear import W8Linear
    from asvd4llm_amd.modules.wb_linear import WBLinear
    out, q, scale, zero, ready = group_restate(w, bits, G) if G else rtn_restate(w, bits)
    assert ready
    return (WBLinear if kind == "bits" else W8Linear).from_codes(codes_of(q), scale, zero, None, bits, w.dtype, group_size=G)


@pytest.mark.parametrize("kind,storage", [("bits", "bitstream64"), ("bytes", "uint8")])
def test_export_writes_the_group_size_and_load_checks_it(tmp_path, kind, storage):
    from asvd4llm_amd.export import load_asvd_repo, save_asvd_repo
    from asvd4llm_amd.model_zoo import random_init_model
    from asvd4llm_amd.modules.packed_linear import PackedLinear
    model = random_init_model("tiny-llama", dtype=torch.float32)
    layer = model.model.layers[0]
    q_w, d_w = layer.self_attn.q_proj.weight.data, layer.mlp.down_proj.weight.data   # down_proj: in_features 352, a ragged last group
    path = str(tmp_path / "repo")
    layer.self_attn.q_proj, layer.mlp.down_proj = _grouped(q_w, 4, 0, kind), _grouped(d_w, 4, 0, kind)
    save_asvd_repo(model, path)
    cfg = json.load(open(os.path.join(path, "config.json")))
    assert cfg["weight_quant"] == {"method": "rtn", "bits": 4, "storage": storage}            # per row: no group_size key
    layer.self_attn.q_proj = _grouped(q_w, 4, 128, kind)
    with pytest.raises(ValueError, match="group sizes"):
        save_asvd_repo(model, path)                                                           # per-row next to grouped layers: refused
    layer.mlp.down_proj = _grouped(d_w, 4, 128, kind)
    save_asvd_repo(model, path)
    cfg = json.load(open(os.path.join(path, "config.json")))
    assert cfg["weight_quant"] == {"method": "rtn", "bits": 4, "storage": storage, "group_size": 128}
    loaded = load_asvd_repo(path, dtype=torch.float32)
    want = {n: m for n, m in model.named_modules() if isinstance(m, PackedLinear)}
    have = {n: m for n, m in loaded.named_modules() if isinstance(m, PackedLinear)}
    assert set(want) == set(have) and len(want) == 2
    for n in want:
        assert type(have[n]) is type(want[n]) and have[n].group_size == 128 and have[n].bits == 4, n
        assert have[n].scales.shape == (want[n].out_features, n_groups(want[n].in_features, 128)), n
        for key in ("qbits" if kind == "bits" else "qweight", "scales", "zeros"):
            assert torch.equal(getattr(want[n], key), getattr(have[n], key)), (n, key)
    ids = torch.randint(0, model.config.vocab_size, (1, 6), generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        assert torch.equal(loaded(input_ids=ids)[0], model.eval()(input_ids=ids)[0])
    # a checkpoint whose scales contradict the group size of config.json is refused: another size, and none
    for other in (64, None):
        bad = dict(cfg, weight_quant=dict(cfg["weight_quant"]))
        if other is None:
            del bad["weight_quant"]["group_size"]
        else:
            bad["weight_quant"]["group_size"] = other
        json.dump(bad, open(os.path.join(path, "config.json"), "w"))
        with pytest.raises(ValueError, match="scales"):
            load_asvd_repo(path, dtype=torch.float32)
    bad["weight_quant"]["group_size"] = 32
    json.dump(bad, open(os.path.join(path, "config.json"), "w"))
    with pytest.raises(ValueError, match="group_size"):
        load_asvd_repo(path, dtype=torch.float32)


# ---- C entry points -----------------------------------------------------------------------------------------------------------------

def test_grouped_entry_points_reject_bad_arguments_without_device(built_lib):
    lib = built_lib
    p, nul = ctypes.c_void_p(4096), None   # non-null but never dereferenced: every check below fails before any HIP call
    flag = ctypes.c_void_p(8192)

    def quant(w=p, dt=1, rows=8, cols=256, ldw=256, bits=4, out=p, ldo=256, flag=flag, group=128):
        return lib.asvd_rtn_quant_grouped(w, dt, rows, cols, ldw, bits, out, ldo, nul, nul, nul, flag, nul, group)

    for bad in (dict(group=0), dict(group=32), dict(group=96), dict(group=256), dict(group=-128), dict(w=nul), dict(out=nul), dict(flag=nul),
                dict(bits=0), dict(bits=9), dict(dt=7), dict(rows=0), dict(cols=0), dict(ldw=255), dict(ldo=255)):
        assert quant(**bad) == -1, bad
    vp2, i2, l2 = ctypes.c_void_p * 2, ctypes.c_int * 2, ctypes.c_int64 * 2
    ws, dts, shape = vp2(4096, 4096), i2(1, 2), l2(8, 8)
    for group in (0, 32, 100):
        assert lib.asvd_rtn_quant_grouped_batched(2, ws, dts, shape, shape, shape, 4, ws, shape, nul, nul, nul, flag, nul, group) == -1
    assert lib.asvd_rtn_quant_grouped_batched(2, ws, dts, shape, shape, shape, 4, vp2(4096, None), shape, nul, nul, nul, flag, nul, 64) == -1
    assert lib.asvd_rtn_quant_grouped_batched(2, ws, dts, shape, shape, shape, 4, ws, shape, nul, nul, nul, nul, nul, 64) == -1      # no flags
    assert lib.asvd_rtn_quant_grouped_batched(0, nul, nul, nul, nul, nul, 4, nul, nul, nul, nul, nul, nul, nul, 64) == -1

    ok = dict(x=p, T=4, q=p, ld=64, bits=4, scale=p, zero=p, group=64, bias=nul, N=8, K=128, y=p)

    def w8(**kw):
        a = dict(ok, ld=128)   # one code per byte: a row of 128 codes
        a.update(kw)
        return lib.asvd_w8_linear_grouped_f16(a["x"], a["T"], a["q"], a["ld"], a["scale"], a["zero"], a["group"], a["bias"], a["N"], a["K"],
                                              a["y"], nul)

    def wb(**kw):
        a = dict(ok, **kw)
        return lib.asvd_wb_linear_grouped_f16(a["x"], a["T"], a["q"], a["ld"], a["bits"], a["scale"], a["zero"], a["group"], a["bias"], a["N"],
                                              a["K"], a["y"], nul)

    common = (dict(group=0), dict(group=32), dict(group=192), dict(x=nul), dict(q=nul), dict(scale=nul), dict(zero=nul), dict(y=nul), dict(T=0),
              dict(T=257), dict(N=0), dict(K=0), dict(x=ctypes.c_void_p(4104)), dict(q=ctypes.c_void_p(4100)), dict(y=ctypes.c_void_p(4097)),
              dict(bias=ctypes.c_void_p(4097)))
    for bad in common + (dict(K=72, ld=80), dict(K=120, ld=128), dict(K=8, ld=16), dict(ld=120), dict(ld=136)):   # K % 16 != 0, short / misaligned ld
        assert w8(**bad) == -1, bad
    for bad in common + (dict(K=72), dict(K=120), dict(bits=5), dict(bits=8), dict(ld=32), dict(ld=56)):
        assert wb(**bad) == -1, bad

    def dq8(q=p, ldq=256, scale=p, zero=p, group=128, rows=8, cols=256, out=p, dt=1, ldo=256):
        return lib.asvd_w8_dequant_grouped(q, ldq, scale, zero, group, rows, cols, out, dt, ldo, nul)

    def dqb(q=p, ld=128, bits=4, scale=p, zero=p, group=128, rows=8, cols=256, out=p, dt=1, ldo=256):
        return lib.asvd_wb_dequant_grouped(q, ld, bits, scale, zero, group, rows, cols, out, dt, ldo, nul)

    for bad in (dict(group=0), dict(group=16), dict(group=129), dict(q=nul), dict(scale=nul), dict(zero=nul), dict(out=nul), dict(rows=0),
                dict(cols=0), dict(ldo=255), dict(dt=5), dict(out=ctypes.c_void_p(4097))):
        assert dq8(**bad) == -1 and dqb(**bad) == -1, bad
    assert dq8(ldq=255) == -1 and dqb(ld=96) == -1 and dqb(bits=8) == -1 and dqb(q=ctypes.c_void_p(4098)) == -1


def test_grouped_ops_have_no_cpu_fallback():
    from asvd4llm_amd import _lib, ops
    q = torch.zeros(4, 128, dtype=torch.uint8)
    s = torch.ones(4, 1)
    with pytest.raises(_lib.AsvdHipError):
        ops.rtn_quant(torch.zeros(4, 128), 4, group_size=128)
    with pytest.raises(_lib.AsvdHipError):
        ops.w8_dequant(q, s, s, torch.float16, group_size=128)
    with pytest.raises(_lib.AsvdHipError):
        ops.w8_linear(torch.zeros(2, 128).half(), q, s, s, group_size=128)
    with pytest.raises(_lib.AsvdHipError):
        ops.wb_linear(torch.zeros(2, 128).half(), torch.zeros(4, 64, dtype=torch.uint8), 4, s, s, group_size=128)
