"""Host replica of the adapter-dropout RNG contract (numpy only).

The masked probe backward (``hdp_probe_grads_dropout``) and ``hdp_dropout_mask`` decide element
``e = o * in + i`` of the ``out x in`` product with Philox4x32-10:

  key     = (lo32(seed), hi32(seed))
  counter = (lo32(e >> 2), hi32(e >> 2), lo32(offset), hi32(offset))
  word    = output[e & 3]
  dropped iff word < thresh,  thresh = min(2^32 - 1, floor(double(float32(p)) * 2^32))

and kept elements are scaled by ``1 / (1 - p)``.  This module computes the same mask on the host.
"""
from __future__ import annotations

import numpy as np

PHILOX_M0 = 0xD2511F53
PHILOX_M1 = 0xCD9E8D57
PHILOX_W0 = 0x9E3779B9
PHILOX_W1 = 0xBB67AE85
_MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """Philox4x32 with 10 rounds.  ``counter``: four uint32 values or arrays (broadcast against each
    other), ``key``: two.  Returns the four output words as a tuple of uint32 arrays."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & _MASK32 for c in counter)
    k0, k1 = (np.asarray(k, dtype=np.uint64) & _MASK32 for k in key)
    m0, m1 = np.uint64(PHILOX_M0), np.uint64(PHILOX_M1)
    w0, w1 = np.uint64(PHILOX_W0), np.uint64(PHILOX_W1)
    s32 = np.uint64(32)
    for _ in range(10):
        p0 = m0 * c0  # 32 x 32 -> 64 bits: exact in uint64
        p1 = m1 * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & _MASK32, (p0 >> s32) ^ c3 ^ k1, p0 & _MASK32
        k0 = (k0 + w0) & _MASK32
        k1 = (k1 + w1) & _MASK32
    return tuple(np.asarray(c, dtype=np.uint64).astype(np.uint32) for c in (c0, c1, c2, c3))


def dropout_threshold(p: float) -> int:
    """min(2^32 - 1, floor(double(float32(p)) * 2^32)): an element is dropped iff its word is below it."""
    t = int(np.floor(float(np.float32(p)) * 4294967296.0))
    return max(0, min(0xFFFFFFFF, t))


def dropout_mask_reference(out: int, in_: int, p: float, seed: int, offset: int) -> np.ndarray:
    """The keep mask (uint8, ``out x in``, 1 = kept) of one masked call."""
    n = int(out) * int(in_)
    nblk = (n + 3) // 4
    blk = np.arange(nblk, dtype=np.uint64)
    seed, offset = int(seed) & 0xFFFFFFFFFFFFFFFF, int(offset) & 0xFFFFFFFFFFFFFFFF
    words = philox4x32_10((blk & _MASK32, blk >> np.uint64(32), offset & 0xFFFFFFFF, offset >> 32),
                          (seed & 0xFFFFFFFF, seed >> 32))
    flat = np.stack([np.broadcast_to(w, (nblk,)) for w in words], axis=1).reshape(-1)[:n]
    return (flat >= np.uint32(dropout_threshold(p))).astype(np.uint8).reshape(int(out), int(in_))
