"""Adapter dropout on the host (CPU): the numpy replica of the RNG contract against the Random123 known
answers, the statistics of its mask, the C-ABI's argument checks (no GPU touched) and the op-set gate of the
layer constructor; and the header the kernels share (csrc/hdp_philox.h), compiled with the host compiler --
plain and with -fsanitize=address,undefined -- behind tests/philox_check.cpp: its Philox, its threshold and
dropout_keep4 at every residue of e0 (the fused kernel's indexing when `in` is no multiple of 4) against the
replica, from 0 and around element 2^34."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch.nn as nn

from cpu_ops import CpuOps

KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("counter,key,want", KAT)
def test_philox_known_answers(counter, key, want):
    from hdpissa_amd.dropout import philox4x32_10
    got = philox4x32_10(counter, key)
    assert tuple(int(np.asarray(w).reshape(-1)[0]) for w in got) == want


def test_philox_vectorised_equals_scalar():
    from hdpissa_amd.dropout import philox4x32_10
    c0 = np.array([0, 0xffffffff, 0x243f6a88], dtype=np.uint32)
    c1 = np.array([0, 0xffffffff, 0x85a308d3], dtype=np.uint32)
    got = philox4x32_10((c0, c1, 7, 9), (3, 5))
    for j in range(3):
        one = philox4x32_10((int(c0[j]), int(c1[j]), 7, 9), (3, 5))
        assert [int(w[j]) for w in got] == [int(np.asarray(w).reshape(-1)[0]) for w in one]


def test_threshold():
    from hdpissa_amd.dropout import dropout_threshold
    assert dropout_threshold(0.5) == 1 << 31
    assert dropout_threshold(1.0) == 0xFFFFFFFF
    assert dropout_threshold(0.0) == 0
    assert dropout_threshold(0.1) == int(math.floor(float(np.float32(0.1)) * 2.0 ** 32))


@pytest.mark.parametrize("out,inn,p,seed,offset", [
    (392, 520, 0.1, 0x1234567890ABCDEF, (3 << 32) | 5),
    (264, 136, 0.5, (1 << 33) + 17, (1 << 40) + 2),
    (7, 13, 0.25, 42, 0),  # n not a multiple of 4
    (256, 256, 0.9, 2 ** 63 + 11, 2 ** 64 - 1),
])
def test_mask_reference_keep_count(out, inn, p, seed, offset):
    from hdpissa_amd.dropout import dropout_mask_reference
    m = dropout_mask_reference(out, inn, p, seed, offset)
    assert m.shape == (out, inn) and m.dtype == np.uint8 and set(np.unique(m)) <= {0, 1}
    n = out * inn
    assert abs(int(m.sum()) - n * (1 - p)) <= 6 * math.sqrt(n * p * (1 - p))
    assert np.array_equal(m, dropout_mask_reference(out, inn, p, seed, offset))


def test_mask_reference_offsets_and_seeds_differ():
    from hdpissa_amd.dropout import dropout_mask_reference
    a = dropout_mask_reference(64, 96, 0.5, 99, 0)
    assert not np.array_equal(a, dropout_mask_reference(64, 96, 0.5, 99, 1))
    assert not np.array_equal(a, dropout_mask_reference(64, 96, 0.5, 99, 1 << 32))
    assert not np.array_equal(a, dropout_mask_reference(64, 96, 0.5, 100, 0))


def test_mask_reference_element_rule():
    """Element e = o * in + i takes word [e & 3] of the block with counter e >> 2."""
    from hdpissa_amd.dropout import dropout_mask_reference, dropout_threshold, philox4x32_10
    out, inn, p, seed, offset = 5, 12, 0.3, (7 << 32) | 9, (2 << 32) | 4
    m = dropout_mask_reference(out, inn, p, seed, offset)
    th = dropout_threshold(p)
    for o, i in [(0, 0), (0, 3), (1, 1), (4, 11), (3, 6)]:
        e = o * inn + i
        w = philox4x32_10((e >> 2, 0, 4, 2), (9, 7))[e & 3]
        assert int(m[o, i]) == int(int(np.asarray(w).reshape(-1)[0]) >= th)


# ---- the kernels' own header (csrc/hdp_philox.h) on the host: tests/philox_check.cpp prints what it computes ----
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PHILOX_SRC = os.path.join(ROOT, "tests", "philox_check.cpp")
PHILOX_INC = os.path.join(ROOT, "hd-pissa_amd", "csrc")
H_SEED = (0x1234 << 32) | 0x9E3779B9   # above 2^32
H_OFF = (5 << 32) | 0xFFFFFFFE         # above 2^32
KEEP_PS = [0.3, 0.5, 1e-9, 0.999]
HI = 1 << 34  # element index whose block index is 2^32: the counter's low word wraps, the high word becomes 1


def _cxx():
    for c in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        if c and shutil.which(c):
            return c
    return None


def _pbits(p):
    return hex(int(np.float32(p).view(np.uint32)))


@pytest.fixture(scope="module", params=[("-O2",), ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")],
                ids=["plain", "asan-ubsan"])
def philox_exe(request, tmp_path_factory):
    cxx = _cxx()
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("philox") / "philox_check")
    # g++ does not know the header's `#pragma unroll`
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", *request.param, "-I", PHILOX_INC,
                    PHILOX_SRC, "-o", exe], check=True)

    def run(*args):
        p = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
        return p.stdout.split()
    return run


def _nibbles(keep):
    """keep[j] = 1 if element e_start + j is kept -> dropout_keep4 of e_start + j, j = 0 .. len - 4."""
    k = np.asarray(keep, dtype=np.int64)
    return k[:-3] | (k[1:-2] << 1) | (k[2:-1] << 2) | (k[3:] << 3)


def _keep_by_hand(e, p, seed, offset):
    """The contract with the counter written out: no use of dropout_mask_reference."""
    from hdpissa_amd.dropout import dropout_threshold, philox4x32_10
    e = np.asarray(e, dtype=np.uint64)
    blk = e >> np.uint64(2)
    words = philox4x32_10((blk & np.uint64(0xFFFFFFFF), blk >> np.uint64(32), offset & 0xFFFFFFFF, offset >> 32),
                          (seed & 0xFFFFFFFF, seed >> 32))
    word = np.choose((e & np.uint64(3)).astype(np.int64), [np.broadcast_to(w, e.shape) for w in words])
    return (word >= np.uint32(dropout_threshold(p))).astype(np.int64)


def test_header_philox_known_answers(philox_exe):
    for counter, key, want in KAT:
        got = philox_exe("philox", *counter, *key)
        assert tuple(int(w, 16) for w in got) == want


def test_header_threshold(philox_exe):
    from hdpissa_amd.dropout import dropout_threshold
    ps = [0.1, 0.3, 0.5, 0.999, 1e-9, 2.0 ** -33, 1.0 - 2.0 ** -24]
    got = [int(t) for t in philox_exe("thresh", *[_pbits(p) for p in ps])]
    assert got == [dropout_threshold(p) for p in ps]
    assert got[2] == 1 << 31 and got[5] == 0 and got[4] == 4          # 2^-33: nothing is ever dropped
    assert got[6] == (1 << 32) - 256                                    # 1 - 2^-24 is a float32: exact


@pytest.mark.parametrize("p", KEEP_PS)
def test_header_keep4_from_zero(philox_exe, p):
    """dropout_keep4(e0) at 4096 consecutive e0, all four residues: the second block and the shift."""
    from hdpissa_amd.dropout import dropout_mask_reference
    n = 4096
    keep = dropout_mask_reference(1, n + 3, p, H_SEED, H_OFF).reshape(-1)
    want = _nibbles(keep)
    assert np.array_equal(keep, _keep_by_hand(np.arange(n + 3), p, H_SEED, H_OFF))
    (got,) = philox_exe("keep4", H_SEED, H_OFF, _pbits(p), 0, n)
    assert len(got) == n
    bad = [e for e in range(n) if int(got[e], 16) != want[e]]
    assert not bad, f"p = {p}: dropout_keep4 differs from the replica at e0 = {bad[:8]} ({len(bad)} of {n})"


@pytest.mark.parametrize("p", KEEP_PS)
def test_header_keep4_around_2_to_34(philox_exe, p):
    """Block indices 2^32 - 512 .. 2^32 + 512: the low counter word wraps and the high word is non-zero; at
    e0 = 2^34 - 3 .. 2^34 - 1 the two blocks of one nibble differ in the high word."""
    start, n = HI - 2048, 4096
    want = _nibbles(_keep_by_hand(start + np.arange(n + 3), p, H_SEED, H_OFF))
    (got,) = philox_exe("keep4", H_SEED, H_OFF, _pbits(p), start, n)
    assert len(got) == n
    bad = [start + j for j in range(n) if int(got[j], 16) != want[j]]
    assert not bad, f"p = {p}: dropout_keep4 differs from the replica at e0 = {bad[:8]} ({len(bad)} of {n})"


def test_header_keep4_expectation_sees_the_residue():
    """The expected nibbles would catch a keep4 that ignored e0 & 3, or the counter's high word."""
    for start in (0, HI - 2048):
        e = start + np.arange(4096 + 3)
        want = _nibbles(_keep_by_hand(e, 0.5, H_SEED, H_OFF))
        j = np.arange(4096)
        assert np.any(want[j] != want[j & ~3])
    lo = _nibbles(_keep_by_hand(np.arange(4096 + 3), 0.5, H_SEED, H_OFF))
    hi = _nibbles(_keep_by_hand(HI + np.arange(4096 + 3), 0.5, H_SEED, H_OFF))
    assert np.any(lo != hi)
    assert not np.array_equal(lo, _nibbles(_keep_by_hand(np.arange(4096 + 3), 0.5, H_SEED, H_OFF & 0xFFFFFFFF)))
    assert not np.array_equal(lo, _nibbles(_keep_by_hand(np.arange(4096 + 3), 0.5, H_SEED & 0xFFFFFFFF, H_OFF)))


def _lib_or_skip():
    from hdpissa_amd._lib import LIB_PATH, lib
    if not os.path.exists(LIB_PATH):
        pytest.skip("libhdpissa.so not built (run __graft_entry__.build())")
    return lib()


def test_abi_argument_checks_without_gpu():
    L = _lib_or_skip()
    args = (None, None, 0, None, None, 0, None, None, 1.0, 0)
    assert L.hdp_probe_grads_dropout(4, 4, 4, 200, *args, 0.1, 1, 2, None, 0, None) == 1
    assert b"r = 200" in L.hdp_last_error()
    assert L.hdp_probe_grads_dropout(4, 4, 4, 16, *args, 1.5, 1, 2, None, 0, None) == 1
    assert b"p = 1.5" in L.hdp_last_error()
    assert L.hdp_probe_grads_dropout(4, 4, 4, 16, *args, 0.0, 1, 2, None, 0, None) == 1
    assert b"p = 0" in L.hdp_last_error()
    assert L.hdp_dropout_mask(4, 4, 1.5, 1, 2, None, None) == 1
    assert b"p = 1.5" in L.hdp_last_error()
    assert L.hdp_probe_dropout_workspace_bytes(1024, 4096, 4096, 16) == 4 * 2 * 32 * 16 * 4096
    assert L.hdp_probe_dropout_workspace_bytes(1024, 4096, 4096, 200) == 0


def test_signatures_cover_the_new_exports():
    from hdpissa_amd._lib import SIGNATURES
    for name in ("hdp_probe_dropout_workspace_bytes", "hdp_probe_grads_dropout", "hdp_dropout_mask"):
        assert name in SIGNATURES


def test_backend_without_masked_probe_still_refuses():
    from hdpissa_amd import CustomLinearLayer
    assert not hasattr(CpuOps(), "probe_grads_dropout")
    with pytest.raises(NotImplementedError):
        CustomLinearLayer(nn.Linear(16, 8), "q", 0, 1, 2, 16.0, dropout=0.1, ops=CpuOps())


def test_backend_with_masked_probe_is_accepted():
    """The constructor's gate is the op set: CpuOps plus a probe_grads_dropout attribute passes it."""
    from hdpissa_amd import CustomLinearLayer

    class Ops(CpuOps):
        def probe_grads_dropout(self, *a, **k):  # never called: no backward here
            raise AssertionError

    layer = CustomLinearLayer(nn.Linear(16, 8), "q", 0, 1, 2, 16.0, dropout=0.1, ops=Ops())
    assert layer.dropout_rate == 0.1 and layer.dropout_calls == 0 and layer.last_dropout_state is None
