"""No kernel of libasvd_hip may use scratch memory (VGPR spills / indexed local arrays).  Measured on MI355X / ROCm 7.2 (DESIGN.md 3.8 a):
a kernel with spills gave nondeterministic corruption as soon as kernels of several streams were in flight.  hipcc cross-compiles
without a GPU; the compiler's own resource remarks are the evidence."""
import os
import re
import subprocess

import pytest

from asvd4llm_amd.build import SOURCES  # every translation unit of the library: a source added to the build is checked without further ado

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "asvd4llm_amd", "csrc")


def _has_kernels(src):
    """does the translation unit (the file and the project headers it includes) define a __global__ function?"""
    seen, todo = set(), [src]
    while todo:
        name = todo.pop()
        if name in seen or not os.path.exists(os.path.join(CSRC, name)):
            continue
        seen.add(name)
        text = open(os.path.join(CSRC, name)).read()
        if "__global__" in text:
            return True
        todo += re.findall(r'#include "([^"]+)"', text)
    return False


def test_only_the_host_side_source_has_no_kernels():
    assert [s for s in SOURCES if not _has_kernels(s)] == ["comm.hip"]


@pytest.mark.parametrize("src", SOURCES)
def test_no_kernel_uses_scratch(src, tmp_path):
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not installed")
    from asvd4llm_amd.build import EXTRA_FLAGS  # the flags the library is built with
    out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only"] + EXTRA_FLAGS.get(src, []) +
                         ["-c", os.path.join(CSRC, src), "-o", str(tmp_path / "o.o"), "-Rpass-analysis=kernel-resource-usage"],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", out.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out.stderr)]
    assert len(names) == len(scratch) and len(names) >= (1 if _has_kernels(src) else 0), (src, names)
    bad = [(n, s) for n, s in zip(names, scratch) if s != 0]
    assert not bad, bad
