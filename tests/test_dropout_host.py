"""Adapter dropout on the host (CPU): the numpy replica of the RNG contract against the Random123 known
answers, the statistics of its mask, the C-ABI's argument checks (no GPU touched) and the op-set gate of the
layer constructor."""
import math
import os

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
