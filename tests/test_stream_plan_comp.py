"""The host plan of the compensated merge (MergeCompPlan in csrc/hdp_stream_plan.h) on the CPU.

tests/stream_plan_comp_check.cpp is compiled against the header alone with the host compiler -- plain, and with
-fsanitize=address,undefined -- as a stand-alone program, and walks items the way stream_group_kernel walks them:

* all of W, C and dW 16-byte aligned, and each of them off 16 bytes in turn (every offset its own alignment
  allows), with n in {0, 1, 7, 8, 9, chunk-1, chunk, chunk+1, 3 chunk + 43}: every element is covered exactly
  once by vector, edge or element-wise work, nothing outside the item; every vector access is 16-byte aligned on
  all three pointers; any pointer off 16 bytes sends the item element by element;
* the chunks walked are the chunks the batcher sums, the bytes it reports 12 per element;
* the batcher: 0, 1, kCap, kCap + 1 and 2 kCap + 1 live items with empty ones in between give launches of kCap,
  ..., rest items in order; kCap is the most that fits the 4 KB argument block; a failed launch ends the call;
* the validation: every refusal (list, n < 0, each null pointer, each misalignment) with the item's index.

Nothing is loaded into Python.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "stream_plan_comp_check.cpp")
INC = os.path.join(ROOT, "hd-pissa_amd", "csrc")
API = os.path.join(ROOT, "include")


def _cxx():
    for c in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        if c and shutil.which(c):
            return c
    return None


@pytest.mark.parametrize("flags", [("-O2",), ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")],
                         ids=["plain", "asan-ubsan"])
def test_stream_plan_comp(tmp_path, flags):
    cxx = _cxx()
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path / "stream_plan_comp_check")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", *flags, "-I", INC, "-I", API, SRC, "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    assert p.stdout.strip().splitlines()[-1].startswith("OK "), p.stdout[-2000:]


def test_python_constants_match_the_plan():
    """_lib's launch cap and chunk are the header's (the GPU tests size their cases by them)."""
    import re
    from hdpissa_amd import _lib
    with open(os.path.join(INC, "hdp_stream_plan.h")) as f:
        text = f.read()
    m = re.search(r"struct MergeCompPlan \{.*?kCap = (\d+), kU = (\d+), kVec = (\d+)", text, flags=re.S)
    assert m, "MergeCompPlan not found"
    cap, ku, vec = (int(x) for x in m.groups())
    assert _lib.MERGE_COMP_MAX == cap and _lib.MERGE_COMP_CHUNK == 256 * ku * vec and vec == 8
