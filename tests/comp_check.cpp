// Stand-alone driver of the compensated-merge header (hd-pissa_amd/csrc/hdp_comp.h): built and run by
// tests/test_comp_contract.py with the host compiler, plain and under -fsanitize=address,undefined.  It only
// prints what the header computes; the Python side compares with the numpy replica (hdpissa_amd/rounding.py).
//   comp_check wbits cbits dwbits ...  -> comp_merge1 on every (bf16 bits of W, bf16 bits of C, float32 bits of
//                                         dW) triple: "w' c'" as hex bf16 bits, one pair per line
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "hdp_comp.h"

static uint32_t u32(const char* s) { return static_cast<uint32_t>(std::strtoul(s, nullptr, 16)); }

static float f32_of_bits(uint32_t b) {
  float f;
  std::memcpy(&f, &b, sizeof f);
  return f;
}

int main(int argc, char** argv) {
  if (argc < 1 || (argc - 1) % 3 != 0) {
    std::fprintf(stderr, "usage: comp_check wbits cbits dwbits ...\n");
    return 2;
  }
  for (int a = 1; a + 2 < argc; a += 3) {
    const hdp::CompPair o = hdp::comp_merge1(static_cast<uint16_t>(u32(argv[a])), static_cast<uint16_t>(u32(argv[a + 1])),
                                             f32_of_bits(u32(argv[a + 2])));
    std::printf("%x %x\n", static_cast<unsigned>(o.w), static_cast<unsigned>(o.c));
  }
  return 0;
}
