// The compensated merge contract (merge_rounding="compensated"): a bf16 W with a bf16
// compensation term C (Kahan summation) takes a float32 dW.  For one element, w and c the bf16 bits read as
// float32 by << 16:
//   a  = float32(c) + dW               one IEEE float32 add (both terms are small: see DESIGN 2.3)
//   s  = a + float32(w)                one IEEE float32 add
//   w' = rne_bf16(s)                   round to nearest even; inf stays inf, NaN stays quiet NaN, carry to inf
//   c' = rne_bf16(s - float32(w'))     if s and float32(w') are both finite (the difference is exact in float32)
//   c' = +0.0                          otherwise
// No multiplies (nothing to contract), subnormals kept, no RNG, no dependence on the element's index or on the
// launch.  s non-finite makes w' non-finite, so "both finite" is "w' finite".  Host and device share this text
// (no HIP needed); hdpissa_amd/rounding.py (comp_merge_bits) is the numpy replica.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define HDP_COMP_HD __host__ __device__ __forceinline__
#else
#define HDP_COMP_HD inline
#endif

namespace hdp {

HDP_COMP_HD uint32_t comp_f32_bits(float f) { return __builtin_bit_cast(uint32_t, f); }
HDP_COMP_HD float comp_bits_f32(uint32_t u) { return __builtin_bit_cast(float, u); }

// float32 bits -> bf16 bits, round-to-nearest-even, NaN -> quiet NaN (the project's f32_to_bf16)
HDP_COMP_HD uint32_t comp_rne_bf16(uint32_t u) {
  if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

struct CompPair {
  uint32_t w, c;  // bf16 bits (the upper halves 0)
};

// wf, cf: the element's weight and compensation as float32 (bf16 bits << 16)
HDP_COMP_HD CompPair comp_merge_f(float wf, float cf, float dw) {
  const float a = cf + dw;
  const float s = a + wf;
  CompPair o;
  o.w = comp_rne_bf16(comp_f32_bits(s));
  // (w' finite: s is finite too, the difference is finite and exact, and the NaN branch of the rounding
  // cannot be taken)
  const uint32_t r = comp_f32_bits(s - comp_bits_f32(o.w << 16));
  o.c = (o.w & 0x7f80u) == 0x7f80u ? 0u : (r + 0x7fffu + ((r >> 16) & 1u)) >> 16;
  return o;
}

// one element: bf16 bits of W and C, float32 dW -> the new bf16 bits of W and C
HDP_COMP_HD CompPair comp_merge1(uint16_t w, uint16_t c, float dw) {
  return comp_merge_f(comp_bits_f32(static_cast<uint32_t>(w) << 16), comp_bits_f32(static_cast<uint32_t>(c) << 16), dw);
}

}  // namespace hdp
