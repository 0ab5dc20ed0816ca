"""The host plan of the grouped stream kernels (csrc/hdp_stream_plan.h) on the CPU.

The stochastic-rounding merge, the grouped copy and the shadow cast write their destinations from one chunk walk
(hdp_elementwise.hip: stream_group_kernel), and which bytes a workgroup touches is decided by the split in
that header.  tests/stream_plan_check.cpp is compiled against the header alone with the host compiler --
plain, and with -fsanitize=address,undefined -- and, for every op, walks items at every dst / src offset of
0..31 bytes with n in {0, 1, vec-1, vec, vec+1, chunk-1, chunk, chunk+1, 3 chunk + 43} the way the kernel
walks them:

* every unit of the item is covered exactly once by vector, edge or unit-by-unit work, nothing outside it;
* every vector access is 16-byte aligned on both sides;
* the chunks walked are the chunks the batcher sums, the bytes it reports the op's bytes per unit;
* a stochastic-rounding item with elem0 % 8 != 0 runs unit by unit;
* the batcher: 0, 1, cap, cap + 1 and 2 cap + 1 live items with empty ones in between give launches of
  cap, ..., rest items in order, with their chunk totals and bytes; a failed launch ends the call;
* the validation: list and item refusals with the item's index and the texts the C ABI tests match.

Nothing is loaded into Python.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "stream_plan_check.cpp")
INC = os.path.join(ROOT, "hd-pissa_amd", "csrc")
API = os.path.join(ROOT, "include")


def _cxx():
    for c in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        if c and shutil.which(c):
            return c
    return None


@pytest.mark.parametrize("flags", [("-O2",), ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")],
                         ids=["plain", "asan-ubsan"])
def test_stream_plan(tmp_path, flags):
    cxx = _cxx()
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path / "stream_plan_check")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", *flags, "-I", INC, "-I", API, SRC, "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    assert p.stdout.strip().splitlines()[-1].startswith("OK "), p.stdout[-2000:]


def test_plan_header_reads_no_environment_and_needs_no_hip():
    with open(os.path.join(INC, "hdp_stream_plan.h")) as f:
        text = f.read()
    assert "getenv" not in text
    assert "hip_runtime" not in text and "hdp_common.h" not in text
