// The adapter-dropout RNG contract: Philox4x32-10 keyed by the seed, counter = (element
// index >> 2, offset), word [e & 3] of the block decides element e = o * in + i; dropped iff word < thresh.
// Host and device share this text; hdpissa_amd/dropout.py is the numpy replica.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define HDP_HD __host__ __device__ __forceinline__
#else
#define HDP_HD inline
#endif

namespace hdp {

struct Philox4 {
  uint32_t w[4];
};

HDP_HD Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = static_cast<uint64_t>(M0) * c0;
    const uint64_t p1 = static_cast<uint64_t>(M1) * c2;
    const uint32_t n0 = static_cast<uint32_t>(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n2 = static_cast<uint32_t>(p0 >> 32) ^ c3 ^ k1;
    c1 = static_cast<uint32_t>(p1);
    c3 = static_cast<uint32_t>(p0);
    c0 = n0;
    c2 = n2;
    k0 += W0;
    k1 += W1;
  }
  return Philox4{{c0, c1, c2, c3}};
}

// min(2^32 - 1, floor(double(float32(p)) * 2^32))
inline uint32_t dropout_threshold(float p) {
  const double t = static_cast<double>(p) * 4294967296.0;
  if (!(t > 0.0)) return 0u;
  return t >= 4294967295.0 ? 0xFFFFFFFFu : static_cast<uint32_t>(t);
}

struct DropoutKey {
  uint32_t seed_lo, seed_hi, off_lo, off_hi, thresh;
};

// Keep bits of the four consecutive elements e0 .. e0 + 3 (bit j set = element e0 + j is kept).  One
// Philox block when e0 is a multiple of 4 (every tile row of a layer whose `in` is a multiple of 4).
HDP_HD unsigned dropout_keep4(uint64_t e0, const DropoutKey& k) {
  const uint64_t blk = e0 >> 2;
  const unsigned sh = static_cast<unsigned>(e0 & 3);
  const Philox4 a = philox4x32_10(static_cast<uint32_t>(blk), static_cast<uint32_t>(blk >> 32), k.off_lo, k.off_hi,
                                  k.seed_lo, k.seed_hi);
  // (the keep bit is a statement of its own: with `bits |= (a.w[j] >= ... ? 1u : 0u) << j` in one expression,
  // g++ 11 -fsanitize=undefined indexes w with an uninitialized copy of j -- tests/test_dropout_host.py builds
  // this header that way; the device code is the same either way)
  unsigned bits = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const unsigned kept = a.w[j] >= k.thresh ? 1u : 0u;
    bits |= kept << j;
  }
  if (sh == 0) return bits;
  const uint64_t nb = blk + 1;
  const Philox4 b = philox4x32_10(static_cast<uint32_t>(nb), static_cast<uint32_t>(nb >> 32), k.off_lo, k.off_hi,
                                  k.seed_lo, k.seed_hi);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const unsigned kept = b.w[j] >= k.thresh ? 1u : 0u;
    bits |= kept << (4 + j);
  }
  return (bits >> sh) & 15u;
}

}  // namespace hdp
