// Stand-alone driver of the adapter-dropout RNG header (hd-pissa_amd/csrc/hdp_philox.h): built and run by
// tests/test_dropout_host.py with the host compiler, plain and under -fsanitize=address,undefined.  It only
// prints what the header computes; the Python side compares with the numpy replica.
//   philox_check philox c0 c1 c2 c3 k0 k1        -> the four output words (hex)
//   philox_check thresh pbits...                 -> dropout_threshold of each float32 bit pattern (decimal)
//   philox_check keep4 seed offset pbits e0 n    -> dropout_keep4(e0 + j), j = 0 .. n - 1, one hex digit each
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "hdp_philox.h"

static uint64_t u64(const char* s) { return std::strtoull(s, nullptr, 0); }

static float f32_of_bits(const char* s) {
  const uint32_t b = static_cast<uint32_t>(u64(s));
  float f;
  std::memcpy(&f, &b, sizeof f);
  return f;
}

int main(int argc, char** argv) {
  if (argc == 8 && !std::strcmp(argv[1], "philox")) {
    uint32_t v[6];
    for (int j = 0; j < 6; ++j) v[j] = static_cast<uint32_t>(u64(argv[2 + j]));
    const hdp::Philox4 w = hdp::philox4x32_10(v[0], v[1], v[2], v[3], v[4], v[5]);
    std::printf("%08x %08x %08x %08x\n", w.w[0], w.w[1], w.w[2], w.w[3]);
    return 0;
  }
  if (argc >= 3 && !std::strcmp(argv[1], "thresh")) {
    for (int j = 2; j < argc; ++j) std::printf("%lu\n", static_cast<unsigned long>(hdp::dropout_threshold(f32_of_bits(argv[j]))));
    return 0;
  }
  if (argc == 7 && !std::strcmp(argv[1], "keep4")) {
    const uint64_t seed = u64(argv[2]), offset = u64(argv[3]), e0 = u64(argv[5]), n = u64(argv[6]);
    const hdp::DropoutKey key{static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32), static_cast<uint32_t>(offset),
                              static_cast<uint32_t>(offset >> 32), hdp::dropout_threshold(f32_of_bits(argv[4]))};
    for (uint64_t j = 0; j < n; ++j) std::printf("%x", hdp::dropout_keep4(e0 + j, key) & 15u);
    std::printf("\n");
    return 0;
  }
  std::fprintf(stderr, "usage: philox_check philox|thresh|keep4 ...\n");
  return 2;
}
