"""The compensated-merge contract on the host (CPU): the header the kernel shares (csrc/hdp_comp.h), compiled with
the host compiler -- plain and with -fsanitize=address,undefined -- behind tests/comp_check.cpp (a stand-alone
program), against the numpy replica (hdpissa_amd/rounding.py: comp_merge_bits) bit for bit on the table of
tests/comp_cases.py; what the contract says of the special values, checked on the replica's own output; and the
replica's properties (dW = 0 and c = 0 change nothing; w' + c' keeps the float32 sum to within 2^-8 of a residual
that is at most half an ulp of w', so to within 2^-9 ulp of w')."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from comp_cases import H, NSPECIAL, bf16_bits, comp_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "comp_check.cpp")
INC = os.path.join(ROOT, "hd-pissa_amd", "csrc")


def _cxx():
    for c in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        if c and shutil.which(c):
            return c
    return None


@pytest.fixture(scope="module", params=[("-O2",), ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")],
                ids=["plain", "asan-ubsan"])
def comp_exe(request, tmp_path_factory):
    cxx = _cxx()
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("comp") / "comp_check")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", *request.param, "-I", INC, SRC, "-o", exe], check=True)

    def run(wb, cb, dw):
        args = []
        for a, b, c in zip(wb, cb, np.asarray(dw, np.float32).view(np.uint32)):
            args += [f"{int(a):x}", f"{int(b):x}", f"{int(c):x}"]
        p = subprocess.run([exe, *args], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
        out = np.array([[int(x, 16) for x in line.split()] for line in p.stdout.splitlines()], dtype=np.uint16)
        return out[:, 0], out[:, 1]
    return run


def _is_nan(b):
    return (b & 0x7FFF) > 0x7F80


@pytest.mark.parametrize("seed", [7, 8])
def test_header_equals_replica(comp_exe, seed):
    from hdpissa_amd.rounding import comp_merge_bits
    wb, cb, dw = comp_cases(seed, 1022)
    want_w, want_c = comp_merge_bits(wb, cb, dw)
    got_w, got_c = comp_exe(wb, cb, dw)
    assert got_w.shape == want_w.shape and got_c.shape == want_c.shape
    assert np.array_equal(_is_nan(want_w), _is_nan(got_w)), "NaN positions differ"
    ok = ~_is_nan(want_w)
    bad = np.nonzero(((got_w != want_w) & ok) | (got_c != want_c))[0]
    assert bad.size == 0, (f"bits differ at {bad[:8]}: got {got_w[bad[:8]]} {got_c[bad[:8]]} "
                           f"want {want_w[bad[:8]]} {want_c[bad[:8]]}")


def test_special_values_follow_the_contract():
    from hdpissa_amd.rounding import comp_merge_bits
    wb, cb, dw = comp_cases(7, 14)
    w, c = (x[-NSPECIAL:] for x in comp_merge_bits(wb, cb, dw))
    mh = bf16_bits(-(2.0 ** -8))
    assert (w[0], c[0]) == (0x3F81, 0) and (w[1], c[1]) == (0x3F81, 0) and (w[2], c[2]) == (0x3F80, 0)
    assert (w[3], c[3]) == (0x3F80, H) and (w[4], c[4]) == (0x3F82, mh)
    assert w[5] == 0x3F82 and c[5] != 0
    assert (w[6], c[6]) == (0xBF80, mh)
    assert (w[7], c[7]) == (0x7F80, 0) and (w[8], c[8]) == (0xFF80, 0)           # carry to inf: c' = +0
    assert (w[9], c[9]) == (0x7F80, 0) and (w[10], c[10]) == (0xFF80, 0)
    assert (w[11], c[11]) == (0x7F80, 0) and (w[12], c[12]) == (0xFF80, 0)       # inf in W
    assert (w[13], c[13]) == (0x7F80, 0) and (w[14], c[14]) == (0xFF80, 0)       # inf in dW
    assert np.all(_is_nan(w[15:19])) and np.all(w[15:19] & 0x40) and np.all(c[15:19] == 0)   # quiet NaN, c' = +0
    assert (w[19], c[19]) == (0x0001, 0)                                           # subnormals are kept
    assert w[20] in (0x0001, 0x0002) and w[21] != 0x0080 and (w[21] & 0x7F80) == 0 and w[22] != 0
    assert (w[23], c[23]) == (0, 0) and (w[24], c[24]) == (0, 0) and w[25] == 0x8000 and (w[26], c[26]) == (0, 0)


def test_replica_keeps_the_sum_and_zero_changes_nothing():
    from hdpissa_amd.rounding import comp_merge_bits
    wb, cb, dw = comp_cases(11, 1 << 14)
    wb, cb, dw = wb[:-NSPECIAL], cb[:-NSPECIAL], dw[:-NSPECIAL]
    f = lambda b: (b.astype(np.uint32) << 16).view(np.float32)  # noqa: E731
    w1, c1 = comp_merge_bits(wb, cb, dw)
    s = ((f(cb) + dw).astype(np.float32) + f(wb)).astype(np.float32)
    res = s.astype(np.float64) - f(w1).astype(np.float64)
    ulp = np.exp2(np.frexp(np.abs(f(w1)))[1].astype(np.float64) - 8.0)
    assert np.all(np.abs(res) <= 0.5 * ulp)                                       # at most half an ulp of w'
    # c' is the residual rounded to 8 significant bits: it loses at most 2^-8 of it, so at most 2^-9 ulp of w'
    lost = np.abs(res - f(c1).astype(np.float64))
    assert np.all(lost <= np.abs(res) * 2.0 ** -8) and np.all(lost <= ulp * 2.0 ** -9)
    z = np.zeros_like(dw)
    w2, c2 = comp_merge_bits(wb, np.zeros_like(cb), z)
    assert np.array_equal(w2, wb) and np.all(c2 == 0)
    # a pair the merge produced keeps its value w + c under dW = 0, to the same 2^-9 ulp (the bits may move: a c'
    # that rounded up to exactly half an ulp is a tie the next merge may resolve to the other neighbour)
    w3, c3 = comp_merge_bits(w1, c1, z)
    v1 = f(w1).astype(np.float64) + f(c1).astype(np.float64)
    v3 = f(w3).astype(np.float64) + f(c3).astype(np.float64)
    assert np.all(np.abs(v3 - v1) <= ulp * 2.0 ** -9)
    assert np.mean(w3 == w1) > 0.98


def test_header_needs_no_hip():
    with open(os.path.join(INC, "hdp_comp.h")) as fh:
        text = fh.read()
    assert "hip_runtime" not in text and "hdp_common.h" not in text
