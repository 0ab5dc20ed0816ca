"""The K4 host plan (csrc/hdp_delta_plan.h) on the CPU.

Everything the K4 kernels read is decided on the host: each item's descriptor and its 16-byte flags, the one
kernel instance a plan launches (math, staging, rounding, cache policy, deferred merge), the tile prefix,
where every item's packed panels and scale table lie, and the thread spaces of the pack, scale and fused
Adam-pack kernels.  Memory safety rests on that plan, so the header is free of HIP and
tests/k4_plan_check.cpp is compiled against it alone with the host compiler -- plain, and with
-fsanitize=address,undefined -- and run on the BASELINE layers (LLaMA-2-7B r 16, Mistral-7B r 64,
LLaMA-2-13B r 128) at nseg 1 / 2 / 4 / 8, the ragged shapes of the GPU tests at r 1 / 4 / 20 / 100 / 128,
shard row blocks, 1-row items and 300 seeded random plans, each under every combination of math, staging,
HDP_K4_DEFER, HDP_K4_STORE, HDP_K4_RND and eight cache policies:

* choice: one existing instance, normalised; 256-row tiles exactly for wide / H2; round dropped exactly
  for single-segment bf16 merges; H2 with round only on even ceil(r / 8); fused <=> H2, single-segment,
  MERGE; a deferred merge never below its variant's minimum chunk count on any item;
* panel image: every panel a consumer addresses inside its item's L or R extent, L / R / items back to
  back, bases 16-byte aligned, extents summing to the allocation;
* scale tables: 64-float aligned, disjoint, scales + partials + constant maxima inside, summing to the
  allocation;
* thread spaces: 256-aligned prefixes covering each item's threads with less than 256 to spare;
* vec_l / vec_r, every refusal of an item with its code, the 32-bit grid limits, and planning twice
  giving the same bytes.

Nothing is loaded into Python.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "k4_plan_check.cpp")
INC = os.path.join(ROOT, "hd-pissa_amd", "csrc")
API = os.path.join(ROOT, "include")


def _cxx():
    for c in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        if c and shutil.which(c):
            return c
    return None


@pytest.mark.parametrize("flags", [("-O2",), ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")],
                         ids=["plain", "asan-ubsan"])
def test_k4_plan(tmp_path, flags):
    cxx = _cxx()
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path / "k4_plan_check")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", *flags, "-I", INC, "-I", API, SRC, "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    assert p.stdout.strip().splitlines()[-1].startswith("OK "), p.stdout[-2000:]


def test_planner_header_reads_no_environment():
    """The knobs are read in hdp_delta.hip (k4_knobs); the planner gets them as a struct."""
    with open(os.path.join(INC, "hdp_delta_plan.h")) as f:
        text = f.read()
    assert "getenv" not in text
    assert "hip_runtime" not in text and "hdp_common.h" not in text
