"""The K2 sweep's range planner (csrc/hdp_probe_plan.h) on the CPU.

The planner cuts a phase's flattened 16-row steps into the workgroups' ranges by cost.  Its minimum range
length is a memory-safety invariant (a stripe's piece buffer holds ceil(S / kSwMinSteps) + 2 pieces), so it
is checked on its own: tests/probe_plan_check.cpp is compiled with the host compiler against the header
alone -- plain, and with -fsanitize=address,undefined -- and run on ~1000 seeded random side lists (1-300
sides, S 1-64, 1-22 stripes, weights 1-4, 1-4096 workgroups) and on the LLaMA-2-7B group layout:

* boundaries non-decreasing, from 0 to U, one more than the ranges;
* every range >= kSwMinSteps steps (the grid shrinks where it must);
* the pieces of every stripe within the buffer's capacity;
* equal weights give exactly w * U / G (what the closed form gave before the planner existed).
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "probe_plan_check.cpp")
INC = os.path.join(ROOT, "hd-pissa_amd", "csrc")


def _cxx():
    for c in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        if c and shutil.which(c):
            return c
    return None


@pytest.mark.parametrize("flags", [("-O2",), ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")],
                         ids=["plain", "asan-ubsan"])
def test_probe_plan(tmp_path, flags):
    cxx = _cxx()
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path / "probe_plan_check")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", *flags, "-I", INC, SRC, "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    assert p.stdout.strip().splitlines()[-1].startswith("OK "), p.stdout[-2000:]
