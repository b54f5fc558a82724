"""The token-tiled GEMM on packed RTN codes (K17: asvd_packed_gemm_f16, ops.packed_gemm, the packed_gemm switch of the packed Linears), host side:
the exported symbols and their agreement between the header, _lib.py and INTEGRATION.md, the token maximum, the argument checks of the entry and
of the op, and the dispatch predicate on CPU-built modules.  No GPU."""
import ctypes
import os
import re

import pytest
import torch

from tests.conftest import ROOT

NAMES = ("asvd_packed_gemm_max_tokens", "asvd_packed_gemm_f16")
CTYPES = {"const void*": "vp", "void*": "vp", "const float*": "vp", "int64_t": "i64", "int": "ctypes.c_int", "size_t": "sz", "void": None}


def _header_args(name):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "asvd_hip.h")).read(), flags=re.S)
    m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, name
    if m.group(1).strip() == "void":
        return []
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
        assert m and [a.strip() for a in m.group(1).split(",") if a.strip()] == want, name
    assert _lib.SIGNATURES[NAMES[0]][0] is c.c_int64 and _lib.SIGNATURES[NAMES[1]][0] is c.c_int
    assert "lib.asvd_packed_gemm_max_tokens.restype = i64" in guide and "ASVD_PACKED_GEMM" in guide
    assert len(_header_args(NAMES[1])) == 13


def test_token_maximum(built_lib):
    from asvd4llm_amd import ops
    from asvd4llm_amd.modules import packed_linear
    top = built_lib.asvd_packed_gemm_max_tokens()
    assert top >= 65536 and top == ops.PACKED_GEMM_MAX_TOKENS
    assert 16 < packed_linear.PACKED_GEMM_MAX_TOKENS <= top


def test_entry_rejects_bad_arguments_without_device(built_lib):
    lib = built_lib
    top = lib.asvd_packed_gemm_max_tokens()
    p, nul = ctypes.c_void_p(4096), None   # non-null but never dereferenced: every check below fails before any HIP call
    odd16, odd2 = ctypes.c_void_p(4104), ctypes.c_void_p(4097)
    ld = {8: 128, 6: 96, 4: 64}            # bytes of a row of 128 codes

    def call(bits=8, **kw):
        a = dict(x=p, T=64, q=p, ld=ld.get(bits, 128), bits=bits, scale=p, zero=p, group=0, bias=nul, N=8, K=128, y=p)
        a.update(kw)
        return lib.asvd_packed_gemm_f16(a["x"], a["T"], a["q"], a["ld"], a["bits"], a["scale"], a["zero"], a["group"], a["bias"], a["N"], a["K"],
                                        a["y"], nul)

    for bits in (8, 6, 4):
        for bad in (dict(x=nul), dict(q=nul), dict(scale=nul), dict(zero=nul), dict(y=nul),
                    dict(T=0), dict(T=-1), dict(T=top + 1),
                    dict(group=32), dict(group=96), dict(group=256), dict(group=-64),
                    dict(K=24), dict(K=120), dict(K=0), dict(N=0),
                    dict(x=odd16), dict(q=odd16), dict(ld=ld[bits] + 8),      # misaligned x, q, ld_bytes
                    dict(ld=ld[bits] - 16),                                   # shorter than a row
                    dict(y=odd2), dict(bias=odd2)):
            for group in (0, 64, 128):
                assert call(bits, **dict(dict(group=group), **bad)) == -1, (bits, group, bad)
    for bits in (0, 2, 5, 7, 16, -4):
        assert call(bits) == -1, bits
    assert call(8, ld=64) == -1            # a 4-bit row length does not pass as a byte row


def test_op_raises_value_errors_before_any_launch():
    from asvd4llm_amd import _lib, ops
    x = torch.zeros(64, 32).half()
    q8, q4 = torch.zeros(8, 32, dtype=torch.uint8), torch.zeros(8, 32, dtype=torch.uint8)   # 32 codes: 32 bytes, or one 4-bit block of 32 bytes
    s, z = torch.ones(8), torch.zeros(8)
    for bad in (lambda: ops.packed_gemm(torch.zeros(64, 48).half(), q8, 8, s, z),           # K of x against the codes
                lambda: ops.packed_gemm(x, torch.zeros(8, 24, dtype=torch.uint8), 4, s, z),  # not the row bytes of 32 4-bit codes
                lambda: ops.packed_gemm(x, q8, 8, torch.ones(7), z),                         # scale of another row count
                lambda: ops.packed_gemm(x, q8, 8, s, z, bias=torch.zeros(9).half()),
                lambda: ops.packed_gemm(x, q8, 8, torch.ones(8, 2), torch.zeros(8, 2), group_size=64),   # [8, 1] groups expected
                lambda: ops.packed_gemm(x.float(), q8, 8, s, z),                             # x not fp16
                lambda: ops.packed_gemm(x.bfloat16(), q8, 8, s, z),
                lambda: ops.packed_gemm(x, q8.int(), 8, s, z),
                lambda: ops.packed_gemm(x, q8, 8, torch.ones(8, 2)[:, 0], z),                # scales not contiguous
                lambda: ops.packed_gemm(x, q8, 8, s, torch.zeros(8, 2)[:, 0]),
                lambda: ops.packed_gemm(x, q8, 8, s.double(), z),
                lambda: ops.packed_gemm(x.t().contiguous().t(), q8, 8, s, z),                # x not contiguous
                lambda: ops.packed_gemm(torch.zeros(64, 24).half(), torch.zeros(8, 24, dtype=torch.uint8), 8, s, z),   # K % 16
                lambda: ops.packed_gemm(torch.zeros(0, 32).half(), q8, 8, s, z),             # no tokens
                lambda: ops.packed_gemm(x, q8, 5, s, z),
                lambda: ops.packed_gemm(x, q8, 8, s, z, group_size=32)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(_lib.AsvdHipError):   # valid arguments on the CPU: there is no fallback
        ops.packed_gemm(x, q8, 8, s, z)
    with pytest.raises(_lib.AsvdHipError):
        ops.packed_gemm(x, q4, 4, s, z)


def test_switch_is_off_by_default_and_cpu_inputs_keep_the_dense_path(monkeypatch):
    from asvd4llm_amd import ops
    from asvd4llm_amd.modules import packed_linear
    from asvd4llm_amd.modules.w8_linear import W8Linear
    from asvd4llm_amd.modules.wb_linear import WBLinear
    monkeypatch.delenv("ASVD_PACKED_GEMM", raising=False)
    assert not packed_linear.packed_gemm_enabled()
    monkeypatch.setattr(ops, "packed_gemm", lambda *a, **k: pytest.fail("the GEMM op was called for a CPU input"))
    x = torch.zeros(64, 32)
    for m in (W8Linear(32, 8, bits=8, weight_dtype=torch.float32), WBLinear(32, 8, bits=4, weight_dtype=torch.float32)):
        assert m._gemm_input(x, 16) is None
        monkeypatch.setenv("ASVD_PACKED_GEMM", "1")
        assert packed_linear.packed_gemm_enabled() and m._gemm_input(x, 16) is None and m(x).shape == (64, 8)
        monkeypatch.delenv("ASVD_PACKED_GEMM")
        m.packed_gemm = True
        assert m._gemm_input(x, 16) is None and m(x).shape == (64, 8)
