"""Host replicas of the two opt-in bf16 merge contracts (numpy only): the stochastic-rounding merge (DESIGN.md
2.2, kernel ``csrc/hdp_sr.h`` / ``hdp_merge_group_sr``) and, at the end of the module, the compensated merge
(``csrc/hdp_comp.h`` / ``hdp_merge_group_comp``).

With ``merge_rounding="stochastic"`` a bf16 W takes its update as ``W = sr(float32(W) + dW)``.  For element
``e = o * in + i`` (64-bit) of the module's W:

  s      = float32(W[e]) + dW[e]                      one IEEE float32 add
  u      = bits(s)
  out    = (u & 0x7F800000) == 0x7F800000 ? round-to-nearest-even bf16 of s : (u + r16(e)) >> 16
  words  = philox4x32_10(counter = (lo32(e >> 3), hi32(e >> 3), lo32(offset), hi32(offset)),
                         key = (lo32(seed), hi32(seed)))
  r16(e) = (words[(e & 7) >> 1] >> (16 * (e & 1))) & 0xFFFF

``offset = (index of the module in the stepper's layer list << 32) | (t mod 2^32)`` and ``seed`` is the
stepper's ``sr_seed``.  This module computes the same bits on the host.
"""
from __future__ import annotations

import numpy as np

from .dropout import philox4x32_10

# default sr_seed = (torch.initial_seed() + SR_SEED_OFFSET) mod 2^64: odd, so never the dropout stream's seed
SR_SEED_OFFSET = 0x9E3779B97F4A7C15
_U64 = 0xFFFFFFFFFFFFFFFF
_M32 = np.uint64(0xFFFFFFFF)


def sr_offset(module_index: int, t: int) -> int:
    """The Philox offset of one module's merge at optimizer step ``t``."""
    return ((int(module_index) << 32) | (int(t) & 0xFFFFFFFF)) & _U64


def default_sr_seed(initial_seed: int) -> int:
    return (int(initial_seed) + SR_SEED_OFFSET) & _U64


def sr_r16(e, seed: int, offset: int) -> np.ndarray:
    """The 16 random bits (uint32 array, values < 65536) of the elements ``e`` (uint64 indices)."""
    e = np.asarray(e, dtype=np.uint64)
    seed, offset = int(seed) & _U64, int(offset) & _U64
    blk = e >> np.uint64(3)
    ublk, inv = np.unique(blk, return_inverse=True)  # one Philox block per 8 elements
    words = philox4x32_10((ublk & _M32, ublk >> np.uint64(32), offset & 0xFFFFFFFF, offset >> 32),
                          (seed & 0xFFFFFFFF, seed >> 32))
    table = np.stack([np.broadcast_to(w, ublk.shape) for w in words], axis=1)  # [blocks, 4] uint32
    j = (e & np.uint64(7)).astype(np.int64)
    word = table[inv.reshape(e.shape), j >> 1].astype(np.uint32)
    return (word >> (np.uint32(16) * (j & 1).astype(np.uint32))) & np.uint32(0xFFFF)


def rne_bf16_bits(u) -> np.ndarray:
    """float32 bits -> bf16 bits (uint32 array), round-to-nearest-even, NaN -> quiet NaN (the project's
    float -> bf16 conversion)."""
    u = np.asarray(u, dtype=np.uint32)
    nan = (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    r = ((u.astype(np.uint64) + np.uint64(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1)).astype(np.uint64))
         >> np.uint64(16)).astype(np.uint32)
    return np.where(nan, (u >> np.uint32(16)) | np.uint32(0x40), r)


def sr_round_bits(u, r16) -> np.ndarray:
    """Bits of the float32 sum and the elements' random bits -> the rounded bf16 bits (uint16 array)."""
    u = np.asarray(u, dtype=np.uint32)
    special = (u & np.uint32(0x7F800000)) == np.uint32(0x7F800000)
    sr = ((u.astype(np.uint64) + np.asarray(r16).astype(np.uint64)) >> np.uint64(16)).astype(np.uint32)
    return np.where(special, rne_bf16_bits(u), sr).astype(np.uint16)


def sr_merge_bits(w_bits, dW, elem0: int, seed: int, offset: int) -> np.ndarray:
    """``w_bits``: the bf16 bits (uint16) of consecutive elements ``elem0, elem0 + 1, ...`` of a W, ``dW``
    their float32 updates -> the merged bf16 bits (uint16, the shape of ``w_bits``)."""
    w_bits = np.asarray(w_bits, dtype=np.uint16)
    dW = np.asarray(dW, dtype=np.float32).reshape(w_bits.shape)
    w = (w_bits.astype(np.uint32) << np.uint32(16)).view(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        s = (w + dW).astype(np.float32)
    e = np.uint64(int(elem0)) + np.arange(w_bits.size, dtype=np.uint64).reshape(w_bits.shape)
    return sr_round_bits(s.view(np.uint32), sr_r16(e, seed, offset))


def sr_merge_reference(W, dW, elem0: int, seed: int, offset: int):
    """The same on a bfloat16 torch tensor ``W`` (any device; returns a new host tensor of W's shape)."""
    import torch
    bits = W.detach().contiguous().cpu().view(torch.int16).numpy().view(np.uint16)
    d = dW.detach().contiguous().cpu().float().numpy().reshape(bits.shape)
    out = sr_merge_bits(bits, d, elem0, seed, offset)
    return torch.from_numpy(out.view(np.int16).copy()).view(torch.bfloat16).view(W.shape)


# ---- merge_rounding="compensated": a bf16 W with a bf16 compensation term C (Kahan summation) -------------
# For one element, w and c the bf16 bits read as float32 by << 16, dW float32:
#   a  = float32(c) + dW             one IEEE float32 add (c and dW are both small against w: added first, their
#                                    sum keeps bits that either would lose against w)
#   s  = a + float32(w)              one IEEE float32 add
#   w' = rne_bf16(s)                 inf stays inf, NaN stays quiet NaN, a carry at the top gives inf
#   c' = rne_bf16(s - float32(w'))   if s and float32(w') are both finite (the difference is exact in float32)
#   c' = +0.0                        otherwise
# No random bits and no dependence on the element's index, the rank, the bucket or the launch.
def comp_merge_bits(w_bits, c_bits, dW):
    """``w_bits`` / ``c_bits``: the bf16 bits (uint16) of W and of its compensation term, ``dW`` their float32
    updates -> ``(w_bits', c_bits')`` (uint16 arrays of the shape of ``w_bits``)."""
    w_bits = np.asarray(w_bits, dtype=np.uint16)
    c_bits = np.asarray(c_bits, dtype=np.uint16).reshape(w_bits.shape)
    dW = np.asarray(dW, dtype=np.float32).reshape(w_bits.shape)
    w = (w_bits.astype(np.uint32) << np.uint32(16)).view(np.float32)
    c = (c_bits.astype(np.uint32) << np.uint32(16)).view(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        a = (c + dW).astype(np.float32)
        s = (a + w).astype(np.float32)
        wo = rne_bf16_bits(s.view(np.uint32))
        res = (s - (wo << np.uint32(16)).view(np.float32)).astype(np.float32)
    finite = (wo & np.uint32(0x7F80)) != np.uint32(0x7F80)  # (s not finite -> w' not finite)
    co = np.where(finite, rne_bf16_bits(res.view(np.uint32)), np.uint32(0))
    return wo.astype(np.uint16), co.astype(np.uint16)


def comp_merge_reference(W, C, dW):
    """The same on bfloat16 torch tensors ``W`` and ``C`` (any device; returns new host tensors of W's shape)."""
    import torch

    def bits(t):
        return t.detach().contiguous().cpu().view(torch.int16).numpy().view(np.uint16)

    wb = bits(W)
    d = dW.detach().contiguous().cpu().float().numpy().reshape(wb.shape)
    wo, co = comp_merge_bits(wb, bits(C).reshape(wb.shape), d)

    def back(b):
        return torch.from_numpy(b.view(np.int16).copy()).view(torch.bfloat16).view(W.shape)

    return back(wo), back(co)
