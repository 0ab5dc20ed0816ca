// The stochastic-rounding merge contract (merge_rounding="stochastic"): bf16 W <- sr(W + dW)
// from the float32 sum.  For element e (row-major index o * in + i of the module's W, 64-bit):
//   s      = float32(bf16 W[e]) + dW[e]                 one IEEE float32 add
//   u      = bits(s)
//   out    = exponent of s all ones ? round-to-nearest-even bf16 of s (inf stays inf, NaN stays NaN)
//                                   : (u + r16(e)) >> 16
//   r16(e) = (words[(e & 7) >> 1] >> (16 * (e & 1))) & 0xFFFF
//   words  = philox4x32_10(counter = (lo32(e >> 3), hi32(e >> 3), lo32(offset), hi32(offset)), key = seed)
// One Philox block serves the eight bf16 values of one 16-byte vector.  A sum that is a bf16 value keeps its
// bits (low half 0: no r16 carries); a carry into the exponent is correct rounding, to infinity at the top of
// the range.  Host and device share this text (no HIP needed); hdpissa_amd/rounding.py is the numpy replica.
#pragma once

#include <stdint.h>

#include "hdp_philox.h"

namespace hdp {

struct SrKey {
  uint32_t seed_lo, seed_hi, off_lo, off_hi;
};

HDP_HD SrKey sr_key(uint64_t seed, uint64_t offset) {
  return SrKey{static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32), static_cast<uint32_t>(offset),
               static_cast<uint32_t>(offset >> 32)};
}

// the Philox block of elements 8 * blk .. 8 * blk + 7
HDP_HD Philox4 sr_block(uint64_t blk, const SrKey& k) {
  return philox4x32_10(static_cast<uint32_t>(blk), static_cast<uint32_t>(blk >> 32), k.off_lo, k.off_hi, k.seed_lo,
                       k.seed_hi);
}

// the 16 random bits of the element at position j = e & 7 of its block
HDP_HD uint32_t sr_r16_of(const Philox4& b, unsigned j) {
  const uint32_t word = b.w[(j & 7u) >> 1];
  return (word >> (16u * (j & 1u))) & 0xFFFFu;
}

HDP_HD uint32_t sr_r16(uint64_t e, const SrKey& k) { return sr_r16_of(sr_block(e >> 3, k), static_cast<unsigned>(e & 7)); }

HDP_HD uint32_t sr_f32_bits(float f) { return __builtin_bit_cast(uint32_t, f); }
HDP_HD float sr_bits_f32(uint32_t u) { return __builtin_bit_cast(float, u); }

// float32 bits -> bf16 bits, round-to-nearest-even, NaN -> quiet NaN (hdp_common.h's f32_to_bf16)
HDP_HD uint32_t sr_rne_bf16(uint32_t u) {
  if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

// the bits of the float32 sum -> the stochastically rounded bf16 bits.  (The device code takes the non-finite
// case as a branch per element, all but never taken; a form that computes both results and selects was
// measured slower: DESIGN section 5.)
HDP_HD uint32_t sr_round(uint32_t u, uint32_t r16) {
  return (u & 0x7F800000u) == 0x7F800000u ? sr_rne_bf16(u) : (u + r16) >> 16;
}

// one element: bf16 bits of W, float32 dW, the element's 16 random bits -> the new bf16 bits of W
HDP_HD uint16_t sr_merge1(uint16_t w, float dw, uint32_t r16) {
  const float s = sr_bits_f32(static_cast<uint32_t>(w) << 16) + dw;
  return static_cast<uint16_t>(sr_round(sr_f32_bits(s), r16));
}

}  // namespace hdp
