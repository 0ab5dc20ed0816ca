// Host planner of the K2 sweep's persistent schedule: how the flattened 16-row steps of one phase
// are cut into the contiguous ranges of its resident workgroups.  Pure C++ (no HIP), so it is
// tested on its own (tests/test_probe_plan.py).
#pragma once
#include <cstdint>
#include <vector>

namespace hdp {

// one module side of a phase: its first flattened step, stripes, steps per stripe and the cost of
// one of its steps (any unit; only ratios matter)
struct PlanSide {
  int64_t pre;
  int nct, S;
  int weight;
};

// Cuts the U = sum nct * S steps into ranges of (nearly) equal COST: bounds[k] = the largest step u
// whose cumulative cost does not exceed k / G of the total, so equal weights give exactly
// k * U / G.  Every range then gets at least min_steps steps (clamped from both ends) -- the piece
// buffers of a stripe hold ceil(S / min_steps) + 2 pieces, a shorter range would write past them.
// The grid shrinks to U / min_steps workgroups where it has to (one workgroup when U < min_steps).
// Returns the number of ranges G' <= G; bounds has G' + 1 entries, non-decreasing, from 0 to U.
inline int plan_ranges(const std::vector<PlanSide>& sides, int G, int min_steps, std::vector<int64_t>& bounds) {
  int64_t U = 0;
  for (const PlanSide& s : sides) U += (int64_t)s.nct * s.S;
  if (min_steps < 1) min_steps = 1;
  const int64_t cap = U / min_steps;
  if (G > cap) G = (int)cap;
  if (G < 1) G = 1;
  bounds.assign((size_t)G + 1, 0);
  bounds[G] = U;
  // cumulative cost at the start of every side
  std::vector<int64_t> c0(sides.size() + 1, 0);
  for (size_t i = 0; i < sides.size(); ++i) {
    const int64_t w = sides[i].weight > 0 ? sides[i].weight : 1;
    c0[i + 1] = c0[i] + w * sides[i].nct * sides[i].S;
  }
  const int64_t C = c0[sides.size()];
  size_t i = 0;
  for (int k = 1; k < G; ++k) {
    // the largest u with cost(u) * G <= k * C  (128-bit: C * G may pass 2^63 on absurd inputs)
    const __int128 target = (__int128)k * C;
    while (i + 1 < sides.size() && (__int128)c0[i + 1] * G <= target) ++i;
    const int64_t w = sides[i].weight > 0 ? sides[i].weight : 1;
    const int64_t n = (int64_t)sides[i].nct * sides[i].S;
    int64_t in = (int64_t)((target - (__int128)c0[i] * G) / ((__int128)w * G));
    if (in > n) in = n;
    bounds[k] = sides[i].pre + in;
  }
  for (int k = 1; k < G; ++k)
    if (bounds[k] < bounds[k - 1] + min_steps) bounds[k] = bounds[k - 1] + min_steps;
  for (int k = G - 1; k >= 1; --k)
    if (bounds[k] > bounds[k + 1] - min_steps) bounds[k] = bounds[k + 1] - min_steps;
  return G;
}

// the range that holds step u: the largest w with bounds[w] <= u (u < U)
inline int plan_owner(const std::vector<int64_t>& bounds, int64_t u) {
  int lo = 0, hi = (int)bounds.size() - 1;  // bounds[lo] <= u < bounds[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) / 2;
    if (bounds[mid] <= u) lo = mid; else hi = mid;
  }
  return lo;
}

}  // namespace hdp
