"""The one-launch packed factor pair (K16: asvd_lowrank_packed_f16, ops.lowrank_packed_forward, SVDLinear.fused_packed), host side: the exported
symbols and their agreement between the header, _lib.py and INTEGRATION.md, the workspace query, the argument checks of the entry, and the dispatch
predicate of SVDLinear.forward on CPU-built modules.  No GPU."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn as nn

from tests.conftest import ROOT

NAMES = ("asvd_lowrank_packed_work_bytes", "asvd_lowrank_packed_f16")
CTYPES = {"const void*": "vp", "void*": "vp", "const float*": "vp", "int64_t": "i64", "int": "ctypes.c_int", "size_t": "sz"}


def _header_args(name):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "asvd_hip.h")).read(), flags=re.S)
    m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, name
    return [CTYPES[a.strip().rsplit(" ", 1)[0].strip()] for a in m.group(1).split(",")]


def test_symbols_agree_between_header_binding_and_integration_guide(built_lib):
    from asvd4llm_amd import _lib
    c = ctypes
    py = {c.c_void_p: "vp", c.c_int64: "i64", c.c_int: "ctypes.c_int", c.c_size_t: "sz"}
    guide = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert hasattr(built_lib, name), name
        want = _header_args(name)
        assert [py[t] for t in _lib.SIGNATURES[name][1]] == want, name
        m = re.search(r"lib\." + name + r"\.argtypes = \[([^\]]*)\]", guide)
        assert m and [a.strip() for a in m.group(1).split(",")] == want, name
    assert _lib.SIGNATURES[NAMES[0]][0] is c.c_size_t and _lib.SIGNATURES[NAMES[1]][0] is c.c_int
    assert "lib.asvd_lowrank_packed_work_bytes.restype = sz" in guide and "ASVD_FUSED_PACKED" in guide
    assert len(_header_args(NAMES[1])) == 20


def test_work_bytes(built_lib):
    f = built_lib.asvd_lowrank_packed_work_bytes
    assert f(1, 16) == 256 + 32 * 16 * 2
    assert f(33, 208) == 256 + 64 * 208 * 2
    assert f(32, 64) == 256 + 32 * 64 * 2 and f(16, 1840) == 256 + 32 * 1840 * 2


def test_entry_rejects_bad_arguments_without_device(built_lib):
    lib = built_lib
    p, nul = ctypes.c_void_p(4096), None   # non-null but never dereferenced: every check below fails before any HIP call
    odd16, odd2 = ctypes.c_void_p(4104), ctypes.c_void_p(4097)
    # a pair 128 -> 64 -> 8 at 4 tokens; ld in bytes: one code per byte at 8 bits, bitstream rows of 64-code blocks otherwise
    ld = {8: (128, 64), 6: (96, 48), 4: (64, 32)}

    def call(bits=8, **kw):
        a = dict(x=p, T=4, qB=p, ldB=ld[bits][0] if bits in ld else 128, sB=p, zB=p, qA=p, ldA=ld[bits][1] if bits in ld else 64, sA=p, zA=p, bits=bits,
                 group=0, bias=nul, N=8, K=128, r=64, y=p, work=p, nbytes=256 + 32 * 64 * 2)
        a.update(kw)
        return lib.asvd_lowrank_packed_f16(a["x"], a["T"], a["qB"], a["ldB"], a["sB"], a["zB"], a["qA"], a["ldA"], a["sA"], a["zA"], a["bits"],
                                           a["group"], a["bias"], a["N"], a["K"], a["r"], a["y"], a["work"], a["nbytes"], nul)

    for bits in (8, 6, 4):
        for bad in (dict(x=nul), dict(qB=nul), dict(sB=nul), dict(zB=nul), dict(qA=nul), dict(sA=nul), dict(zA=nul), dict(y=nul), dict(work=nul),
                    dict(T=0), dict(T=257), dict(T=-1),
                    dict(group=32), dict(group=96), dict(group=256), dict(group=-64),
                    dict(K=120), dict(K=136, ldB=160), dict(r=56), dict(r=72, ldA=96), dict(K=0), dict(r=0), dict(N=0),
                    dict(x=odd16), dict(qB=odd16), dict(qA=odd16), dict(work=odd16),
                    dict(ldB=ld[bits][0] + 8), dict(ldA=ld[bits][1] + 8),             # not a multiple of 16
                    dict(ldB=ld[bits][0] - 16), dict(ldA=ld[bits][1] - 16),           # shorter than a row
                    dict(y=odd2), dict(bias=odd2)):
            assert call(bits, **bad) == -1, (bits, bad)
        for group in (0, 64, 128):
            assert call(bits, group=group, nbytes=256 + 32 * 64 * 2 - 1) == -2, (bits, group)     # ASVD_E_WORKSPACE
            assert call(bits, group=group, T=33, nbytes=256 + 32 * 64 * 2) == -2, (bits, group)   # two token tiles need twice the rows
    for bits in (0, 2, 5, 7, 16, -4):
        assert call(bits) == -1, bits
    # the row length that the width implies: a byte row of 128 codes does not pass as a 4-bit row and the reverse
    assert call(8, ldB=64) == -1 and call(8, ldA=32) == -1


def test_ops_have_no_cpu_fallback():
    from asvd4llm_amd import _lib, ops
    q = torch.zeros(16, 16, dtype=torch.uint8)
    s = torch.ones(16)
    with pytest.raises(_lib.AsvdHipError):
        ops.lowrank_packed_forward(torch.zeros(2, 16).half(), q, s, s, q, s, s, 8, None, torch.zeros(2048, dtype=torch.uint8))


# ---- the dispatch predicate of SVDLinear.forward --------------------------------------------------------------------------------------

def _factor(kind, in_f, out_f, bits, G, bias=False, dtype=torch.float16):
    from asvd4llm_amd.modules.w8_linear import W8Linear
    from asvd4llm_amd.modules.wb_linear import WBLinear
    cls = WBLinear if kind == "wb" else W8Linear
    return cls(in_f, out_f, bias=bias, bits=bits, weight_dtype=dtype, group_size=G)


def _pair(kind="wb", bits=4, G=64, K=64, r=32, N=48, a=None, b=None):
    """an SVDLinear whose factors are CPU-built packed modules (zero codes: only the dispatch is looked at)"""
    from asvd4llm_amd.modules.svd_linear import SVDLinear
    m = SVDLinear.__new__(SVDLinear)
    nn.Module.__init__(m)
    m.BLinear = b if b is not None else _factor(kind, K, r, bits, G)
    m.ALinear = a if a is not None else _factor(kind, r, N, bits, G, bias=True)
    m.truncation_rank = r
    m.fused_packed = True
    return m


def test_dispatch_predicate(monkeypatch):
    from asvd4llm_amd.modules import svd_linear as S
    monkeypatch.delenv("ASVD_FUSED_PACKED", raising=False)
    assert S.FUSED_PACKED_MAX_TOKENS == 16
    x = torch.zeros(2, 3, 64).half()
    with torch.no_grad():
        # everything but the device holds: the predicate gets to its last question.  (On the device it answers None: tests/test_gpu_packed_pair.py.)
        for kind, bits in (("wb", 4), ("wb", 6), ("w8", 8), ("w8", 4)):
            for G in (0, 64, 128):
                assert _pair(kind, bits, G).fused_packed_refusal(x) == "not on the device", (kind, bits, G)
        m = _pair()
        m.fused_packed = False
        assert m.fused_packed_refusal(x) == "switched off"
        monkeypatch.setenv("ASVD_FUSED_FORWARD", "1")           # K10's switch is not this one
        assert m.fused_packed_refusal(x) == "switched off"
        monkeypatch.setenv("ASVD_FUSED_PACKED", "1")
        assert m.fused_packed_refusal(x) == "not on the device"
        monkeypatch.delenv("ASVD_FUSED_PACKED")
        monkeypatch.delenv("ASVD_FUSED_FORWARD")
        # mixed classes, a plain Linear, a subclass
        assert _pair(a=_factor("w8", 32, 48, 4, 64)).fused_packed_refusal(x) == "not a pair of W8Linear or a pair of WBLinear"
        assert _pair(b=_factor("w8", 64, 32, 4, 64)).fused_packed_refusal(x) == "not a pair of W8Linear or a pair of WBLinear"
        assert _pair(a=nn.Linear(32, 48).half()).fused_packed_refusal(x) == "not a pair of W8Linear or a pair of WBLinear"
        sub = type("Sub", (type(_factor("wb", 32, 48, 4, 64)),), {})(32, 48, bias=False, bits=4, group_size=64)
        assert _pair(a=sub).fused_packed_refusal(x) == "not a pair of W8Linear or a pair of WBLinear"
        # widths: bit-packed 6 against 4; one code per byte is ONE storage width whatever the quantizer's
        assert _pair(a=_factor("wb", 32, 48, 6, 64)).fused_packed_refusal(x) == "different storage widths"
        assert _pair("w8", 8, 64, a=_factor("w8", 32, 48, 4, 64)).fused_packed_refusal(x) == "not on the device"
        # group sizes
        assert _pair(a=_factor("wb", 32, 48, 4, 128)).fused_packed_refusal(x) == "different group sizes"
        assert _pair(b=_factor("wb", 64, 32, 4, 0)).fused_packed_refusal(x) == "different group sizes"
        # a BLinear bias
        assert _pair(b=_factor("wb", 64, 32, 4, 64, bias=True)).fused_packed_refusal(x) == "BLinear has a bias"
        # hooks on either factor, and in the module registry
        for which in ("ALinear", "BLinear"):
            for reg in ("register_forward_hook", "register_forward_pre_hook"):
                m = _pair()
                h = getattr(getattr(m, which), reg)(lambda *a: None)
                assert m.fused_packed_refusal(x) == "hooks", (which, reg)
                h.remove()
                assert m.fused_packed_refusal(x) == "not on the device"
        h = nn.modules.module.register_module_forward_hook(lambda *a: None)
        try:
            assert _pair().fused_packed_refusal(x) == "hooks"
        finally:
            h.remove()
        # 17 tokens (16 pass), no tokens
        assert _pair().fused_packed_refusal(torch.zeros(17, 64).half()) == "token count"
        assert _pair().fused_packed_refusal(torch.zeros(16, 64).half()) == "not on the device"
        assert _pair().fused_packed_refusal(torch.zeros(0, 64).half()) == "token count"
        # fp32 input, a bf16 factor
        assert _pair().fused_packed_refusal(x.float()) == "not fp16"
        assert _pair(a=_factor("wb", 32, 48, 4, 64, dtype=torch.bfloat16)).fused_packed_refusal(x) == "not fp16"
        # in_features % 16 != 0, and a rank that is no multiple of 16
        assert _pair(K=72).fused_packed_refusal(torch.zeros(3, 72).half()) == "code rows without 16-byte loads"
        assert _pair(r=24).fused_packed_refusal(x) == "code rows without 16-byte loads"
        assert _pair().fused_packed_refusal(torch.zeros(3, 128).half()) == "shapes"
    xg = torch.zeros(3, 64).half().requires_grad_(True)
    assert _pair().fused_packed_refusal(xg) == "autograd"


def test_cpu_forward_takes_the_two_calls_and_refresh_drops_the_workspaces(monkeypatch):
    from asvd4llm_amd import ops
    monkeypatch.setattr(ops, "lowrank_packed_forward", lambda *a, **k: pytest.fail("no fused launch off the device"))
    m = _pair()
    x = torch.randn(3, 64).half()
    with torch.no_grad():
        assert torch.equal(m(x), m.ALinear(m.BLinear(x)))
    m._fused_packed = {1: torch.zeros(4)}
    m.refresh_fused()
    assert m._fused_packed == {} and m._fused is None
    m.check_fused_forward()
