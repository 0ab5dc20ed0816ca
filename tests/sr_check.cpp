// Stand-alone driver of the stochastic-rounding header (hd-pissa_amd/csrc/hdp_sr.h): built and run by
// tests/test_sr_host.py with the host compiler, plain and under -fsanitize=address,undefined.  It only prints
// what the header computes; the Python side compares with the numpy replica (hdpissa_amd/rounding.py).
//   sr_check r16 seed offset e0 n                  -> r16(e0 + j), j = 0 .. n - 1 (hex, one per line)
//   sr_check merge seed offset e0 wbits dwbits ... -> sr_merge1 of element e0 + j on the j-th (bf16 bits of W,
//                                                     float32 bits of dW) pair (hex bf16 bits, one per line)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "hdp_sr.h"

static uint64_t u64(const char* s) { return std::strtoull(s, nullptr, 0); }

static float f32_of_bits(uint32_t b) {
  float f;
  std::memcpy(&f, &b, sizeof f);
  return f;
}

int main(int argc, char** argv) {
  if (argc == 6 && !std::strcmp(argv[1], "r16")) {
    const hdp::SrKey key = hdp::sr_key(u64(argv[2]), u64(argv[3]));
    const uint64_t e0 = u64(argv[4]), n = u64(argv[5]);
    for (uint64_t j = 0; j < n; ++j) std::printf("%x\n", hdp::sr_r16(e0 + j, key));
    return 0;
  }
  if (argc >= 5 && (argc - 5) % 2 == 0 && !std::strcmp(argv[1], "merge")) {
    const hdp::SrKey key = hdp::sr_key(u64(argv[2]), u64(argv[3]));
    const uint64_t e0 = u64(argv[4]);
    for (int a = 5; a + 1 < argc; a += 2) {
      const uint64_t e = e0 + static_cast<uint64_t>((a - 5) / 2);
      const uint16_t w = static_cast<uint16_t>(u64(argv[a]));
      const float dw = f32_of_bits(static_cast<uint32_t>(u64(argv[a + 1])));
      std::printf("%x\n", static_cast<unsigned>(hdp::sr_merge1(w, dw, hdp::sr_r16(e, key))));
    }
    return 0;
  }
  std::fprintf(stderr, "usage: sr_check r16|merge ...\n");
  return 2;
}
