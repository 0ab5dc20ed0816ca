"""The K2 sweep's host plan (csrc/hdp_sweep_plan.h) on the CPU.

Everything the sweep kernels read is planned on the host: which modules share an X stream, the three
phases' side descriptors, the reduce and finish tables, the workgroups' ranges and start tables, the
finish's job list and the blob they are uploaded as.  Memory safety rests on that plan, so the header is
free of HIP and tests/sweep_plan_check.cpp is compiled against it alone with the host compiler -- plain,
and with -fsanitize=address,undefined -- and run on the LLaMA-2-7B layer at r 16 / 32 / 64, groups whose
sets must not form, ragged shapes (T 1-33, N 4-1028, in % 4 != 0), an r-slice pair and ~300 seeded random
groups, in float32 and bf16, at 1 / 7 / 256 / 1024 / 4096 resident workgroups:

* ranges: boundaries non-decreasing from 0 to U, every range >= kSwMinSteps steps (or a single range),
  pieces per stripe within the buffers, the job list = exactly the split stripes with their counts;
* start tables: (side, stripe, step) reproduces the boundary, the piece index = earlier workgroups on
  the stripe;
* coverage: every r-block of every module's X and G side projected once and OUTER-ed once, a set's
  stacked side holds each member's blocks once;
* workspace: every slab, piece and Y pointer with its extent inside the owning module's buffer, areas
  disjoint, the blob's sections aligned, disjoint and within the table space, tables + areas within the
  workspace query;
* planning twice gives the same bytes.

Nothing is loaded into Python.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "sweep_plan_check.cpp")
INC = os.path.join(ROOT, "hd-pissa_amd", "csrc")


def _cxx():
    for c in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        if c and shutil.which(c):
            return c
    return None


@pytest.mark.parametrize("flags", [("-O2",), ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")],
                         ids=["plain", "asan-ubsan"])
def test_sweep_plan(tmp_path, flags):
    cxx = _cxx()
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path / "sweep_plan_check")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", *flags, "-I", INC, SRC, "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    assert p.stdout.strip().splitlines()[-1].startswith("OK "), p.stdout[-2000:]


def test_planner_header_reads_no_environment():
    """The knobs are read in hdp_probe.hip, once per launch; the planner gets them as a struct."""
    with open(os.path.join(INC, "hdp_sweep_plan.h")) as f:
        text = f.read()
    assert "getenv" not in text
    assert "hip_runtime" not in text and "hdp_common.h" not in text
