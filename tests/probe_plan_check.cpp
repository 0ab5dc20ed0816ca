// Stand-alone check of the K2 sweep's range planner (hd-pissa_amd/csrc/hdp_probe_plan.h): built and run by
// tests/test_probe_plan.py with the host compiler, plain and under -fsanitize=address,undefined.
// Exit status 0 and a last line "OK <cases>" mean every property held.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "hdp_probe_plan.h"

using hdp::PlanSide;

static const int kMin = 8;  // kSwMinSteps of hdp_probe.hip
static int g_fail = 0;

#define EXPECT(cond, ...)                       \
  do {                                          \
    if (!(cond)) {                              \
      if (g_fail++ < 20) {                      \
        std::printf("FAIL %s: ", #cond);        \
        std::printf(__VA_ARGS__);               \
        std::printf("\n");                      \
      }                                         \
    }                                           \
  } while (0)

static int64_t total_steps(const std::vector<PlanSide>& s) {
  int64_t U = 0;
  for (const PlanSide& x : s) U += (int64_t)x.nct * x.S;
  return U;
}

// the properties every plan has; returns the largest range cost
static int64_t check_plan(const std::vector<PlanSide>& sides, int G, int tag) {
  std::vector<int64_t> b;
  const int Gp = hdp::plan_ranges(sides, G, kMin, b);
  const int64_t U = total_steps(sides);
  EXPECT(Gp >= 1 && Gp <= G, "case %d: G' = %d of %d", tag, Gp, G);
  EXPECT((int)b.size() == Gp + 1, "case %d: %zu bounds for G' = %d", tag, b.size(), Gp);
  if ((int)b.size() != Gp + 1) return 0;
  EXPECT(b[0] == 0 && b[Gp] == U, "case %d: ends %lld .. %lld, U = %lld", tag, (long long)b[0], (long long)b[Gp],
         (long long)U);
  const int64_t least = U < kMin ? U : kMin;
  for (int w = 0; w < Gp; ++w) {
    EXPECT(b[w + 1] >= b[w], "case %d: bounds decrease at %d", tag, w);
    EXPECT(b[w + 1] - b[w] >= least, "case %d: range %d has %lld steps (< %lld)", tag, w,
           (long long)(b[w + 1] - b[w]), (long long)least);
  }
  // the grid only shrinks where the minimum forces it
  const int64_t cap = U / kMin < 1 ? 1 : U / kMin;
  EXPECT(Gp == (G < cap ? G : (int)cap), "case %d: G' = %d, G = %d, cap = %lld", tag, Gp, G, (long long)cap);
  // pieces per stripe within the buffers' capacity ceil(S / kMin) + 2 (sweep_kmax)
  for (const PlanSide& s : sides)
    for (int ct = 0; ct < s.nct; ++ct) {
      const int64_t u0 = s.pre + (int64_t)ct * s.S;
      const int k0 = hdp::plan_owner(b, u0), k1 = hdp::plan_owner(b, u0 + s.S - 1);
      EXPECT(b[k0] <= u0 && u0 < b[k0 + 1], "case %d: owner of %lld", tag, (long long)u0);
      EXPECT(k1 - k0 + 1 <= (s.S + kMin - 1) / kMin + 2, "case %d: %d pieces in a stripe of %d steps", tag, k1 - k0 + 1,
             s.S);
    }
  // range costs
  int64_t worst = 0;
  size_t i = 0;
  for (int w = 0; w < Gp; ++w) {
    int64_t cost = 0, u = b[w];
    while (u < b[w + 1]) {
      while (u >= sides[i].pre + (int64_t)sides[i].nct * sides[i].S) ++i;
      const int64_t end = sides[i].pre + (int64_t)sides[i].nct * sides[i].S;
      const int64_t n = (end < b[w + 1] ? end : b[w + 1]) - u;
      cost += n * sides[i].weight;
      u += n;
    }
    worst = cost > worst ? cost : worst;
  }
  return worst;
}

static void check_equal(std::vector<PlanSide> sides, int G, int weight, int tag) {
  for (PlanSide& s : sides) s.weight = weight;
  std::vector<int64_t> b;
  const int Gp = hdp::plan_ranges(sides, G, kMin, b);
  const int64_t U = total_steps(sides);
  for (int w = 0; w <= Gp && w < (int)b.size(); ++w)
    EXPECT(b[w] == (int64_t)w * U / Gp, "case %d: equal weights %d, bound %d = %lld, expected %lld", tag, weight, w,
           (long long)b[w], (long long)((int64_t)w * U / Gp));
}

int main() {
  std::mt19937_64 rng(20240607);
  auto uni = [&](int lo, int hi) { return lo + (int)(rng() % (uint64_t)(hi - lo + 1)); };
  int cases = 0;
  for (int c = 0; c < 1000; ++c, ++cases) {
    const int n = c < 40 ? 1 + c % 4 : uni(1, 300);
    std::vector<PlanSide> sides(n);
    int64_t pre = 0;
    for (PlanSide& s : sides) {
      s = PlanSide{pre, uni(1, 22), uni(1, 64), uni(1, 4)};
      pre += (int64_t)s.nct * s.S;
    }
    const int G = c % 7 == 0 ? uni(1, 8) : uni(1, 4096);
    check_plan(sides, G, c);
    check_equal(sides, G, 1 + c % 4, c);
  }
  // LLaMA-2-7B float32 r = 16 group, T = 691 (44 steps): per layer the q/k/v set (3 blocks), o_proj (1), the
  // gate/up set (2) and down_proj's G side (1), 8 stripes of 512 columns each; 256 workgroups
  for (int T : {691, 1024, 17}) {
    const int S = (T + 15) / 16;
    std::vector<PlanSide> sides;
    int64_t pre = 0;
    for (int layer = 0; layer < 32; ++layer)
      for (int nb : {3, 1, 2, 1}) {
        static const int wA[5] = {64, 64, 74, 88, 98};  // kSwWeightA of hdp_probe.hip
        sides.push_back(PlanSide{pre, 8, S, wA[nb]});
        pre += 8 * S;
      }
    const int64_t worst = check_plan(sides, 256, 10000 + T);
    check_equal(sides, 256, 64, 10000 + T);
    std::vector<int64_t> b;
    const int Gp = hdp::plan_ranges(sides, 256, kMin, b);
    int64_t C = 0;
    for (const PlanSide& s : sides) C += (int64_t)s.nct * s.S * s.weight;
    if (T >= 691) {
      // the heaviest range is within two steps' cost of the mean; the equal split's heaviest holds only 3-block steps
      EXPECT(worst <= C / Gp + 2 * 98, "7B T = %d: worst range cost %lld, mean %lld", T, (long long)worst,
             (long long)(C / Gp));
      const int64_t uniform_worst = (pre / Gp) * 88;
      EXPECT(worst < uniform_worst, "7B T = %d: weighted worst %lld vs equal split %lld", T, (long long)worst,
             (long long)uniform_worst);
    }
    ++cases;
  }
  // fewer steps than the minimum: one workgroup
  {
    std::vector<PlanSide> one{PlanSide{0, 1, 3, 2}};
    std::vector<int64_t> b;
    EXPECT(hdp::plan_ranges(one, 64, kMin, b) == 1 && b.size() == 2 && b[0] == 0 && b[1] == 3, "U < minimum");
    ++cases;
  }
  if (g_fail) {
    std::printf("%d failures\n", g_fail);
    return 1;
  }
  std::printf("OK %d\n", cases);
  return 0;
}
