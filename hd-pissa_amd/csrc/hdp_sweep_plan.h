// Host plan of the K2 sweep (hdp_probe.hip): the structs the host fills and the device reads, the
// workspace layout of a module, and the two planning stages of a launch -- which modules share an X
// stream, the three phases' side lists, the reduce / finish descriptors, the workgroups' ranges and
// start tables, the finish's job list, and the one blob all of it is uploaded as.  Pure C++ (no HIP,
// no environment): hipcc and the host compiler build the same code, and tests/sweep_plan_check.cpp
// runs it on the CPU (tests/test_sweep_plan.py, plain and under ASan/UBSan).  The stages only do
// arithmetic on the pointers they are given; they never dereference one.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "hdp_probe_plan.h"

namespace hdp {

// one module of a probe group as the host plans it (pointers into the caller's tensors and the
// group workspace)
struct ProbeDesc {
  const void* X;
  const void* G;
  const float* A;
  const float* B;   // B (out x r) or B^T (r x out) when b_t
  float* gA;
  float* gB;
  float* slabH;     // split / sweep: [ksh][T][rp]
  float* slabJ;     // split / sweep: [ksj][T][rp]
  float* partA;     // [kst][rp][in]
  float* partB;     // [kst][out][rp]
  float* yH;        // sweep: H = X A^T [T][rp]
  float* yJ;        // sweep: J = G B   [T][rp]
  int64_t T, in, out;
  float scale;
  int r, b_t, accumulate;
  int ksh, ksj, kst;
  int colh, colj;   // P1 columns per wave (multiples of 16)
  int ldb;          // row stride of gB: r, or the module's full rank when this is one of its r-slices
};

// a group as planned on the host (sweep path: any size, descriptors uploaded per flush)
struct HostGroup {
  int n = 0, rp = 16, RB = 1;
  std::vector<ProbeDesc> d;
};

constexpr int kSwWaves = 8;          // streaming waves of a sweep workgroup
constexpr int kSwC = 64 * kSwWaves;  // stripe width (columns)
constexpr int kSwMinSteps = 8;       // >= 128 rows per workgroup: bounds the pieces per stripe
constexpr int kSwMaxBlk = 4;         // r-blocks of one stream side (FUSE: of all modules sharing its X)

// Cost of one 16-row step of a side with nb r-blocks, relative to nb = 1 (x 64), in phase A of a float32
// shared-X group (the FUSE X6 PROJ instance).  A step's MFMA and LDS work grows with nb while its bytes do
// not, so the q/k/v sets (3 blocks) and gate/up (2) take longer per step than o_proj / down_proj (1); an
// equal split of the steps left the light workgroups idle at the phase's end (LLaMA-2-7B group: 420 -> 370 us).
// Measured per step on homogeneous groups at the LLaMA-2-7B shapes (tools/probe_weights.py):
// profiles/r07_probe_weights.jsonl -- 1 : 1.15 : 1.37 : 1.54.  Phase C (f32 OUTER) measured 1 : 0.94 : 1.13 :
// 1.49: its 3-block steps are not the 1.3 x that would explain its time, so it keeps the equal split.
constexpr int kSwWeightA[kSwMaxBlk + 1] = {64, 64, 74, 88, 98};

// one module side (a stream Z = X or G) of one sweep phase
struct SweepDesc {
  const void* Z;          // T x N, row-major, x_dtype
  const float* F;         // f_rk: F[j][n] at j * N + n (A, B^T);  else F[n][j] at n * r + j (B)
  float* slab_out;        // PROJ:  [nct][T][rp] stripe partials of Z F^T
  const float* y_in;      // OUTER: the other stream's projection, row t at y_in + t * yrs, a lane's
                          //        RB values at + li * yls (probe_yreduce_kernel's layout)
  float* part;            // OUTER: [nct][kmax][rp][kSwC]  or  [nct][kmax][kSwC][rp] (part_t)
  int64_t T, N, pre;      // pre: first flattened step of this module side
  int r, f_rk, part_t, nct, S, kmax;  // S = 16-row steps per stripe
  // OUTER, a stripe covered by ONE workgroup segment: its gradient block written directly,
  // g (+)= scale * acc (part_t 0: gA [r][N]; 1: gB [N][ldb]); the finish pass skips it
  float* g;
  float scale;
  int acc, ldb;
  int yrs, yls;           // Y row / lane strides (floats)
  // Shared-X instances (FUSE): the side is r-block-wise -- nb blocks of 16 rows, block b possibly of
  // another module that reads the same X (q/k/v, gate/up).  Block b: F rows Fb[b] (rbr[b] of them),
  // slab columns slab_b[b] and pieces part_b[b] (row strides rpm = the members' 16 RB), gradient
  // rows gb[b] with scale sc[b] / accumulate accb[b].
  int nb, rpm;
  const float* Fb[kSwMaxBlk];
  float* slab_b[kSwMaxBlk];
  float* part_b[kSwMaxBlk];
  float* gb[kSwMaxBlk];
  float sc[kSwMaxBlk];
  int rbr[kSwMaxBlk], accb[kSwMaxBlk];
};

// Y[t][j] = sum_ct slab[ct][t][j] (probe_yreduce_kernel), one per module and reduce pass
struct YRedDesc {
  const float* slab;  // [nct][T][rp] (rp = 16 RB of the module)
  float* y;           // element (t, j = 16 b + li) -> y[t * ys + b + li * sl]
  int64_t T;
  int nct, ys, sl, pad;
};

// gA[j][n] (+)= s * sum_k pieceA[ct][k][j][n % kSwC];  gB[n][j] (+)= s * sum_k pieceB[ct][k][n % kSwC][j]
struct SwFinishSide {
  const float* part;
  int64_t pre;     // the OUTER phase's flattened steps before this side
  int S, kmax;
  int ph;          // which OUTER phase wrote the pieces: 0 = phase B, 1 = phase C
  int pad;
};
struct FinDesc {
  float* gA;
  float* gB;
  int in, out, r, acc;
  float scale;
  int ldb;  // row stride of gB (= r, or the full rank when the module is an r-slice of a wider one)
  SwFinishSide sx, sg;
};

// the device reads these as the host wrote them: both compilers must agree on the layouts
static_assert(sizeof(SweepDesc) == 304, "SweepDesc layout");
static_assert(sizeof(YRedDesc) == 40, "YRedDesc layout");
static_assert(sizeof(SwFinishSide) == 32, "SwFinishSide layout");
static_assert(sizeof(FinDesc) == 104, "FinDesc layout");

// ---------------------------------------------------------------------------------------
// workspace planning
// ---------------------------------------------------------------------------------------
// Per-flush descriptor tables: one host blob copied to the head of the group's device workspace
// in stream order.
// WG start tables (4 ints) and range boundaries (1 int, + the end) per phase, up to 4096 WGs/phase
constexpr size_t kTableFixed = 3 * 4096 * 5 * sizeof(int) + 8192;
constexpr size_t kTablePerModule = 3 * sizeof(SweepDesc) + 2 * sizeof(YRedDesc) + sizeof(FinDesc) + 64;

inline int rb_of(int r) {
  const int rb = (r + 15) / 16;
  return rb <= 1 ? 1 : rb <= 2 ? 2 : rb <= 4 ? 4 : 8;
}

// a module's work area: offsets of its buffers, the area's size, and `bytes` = the area plus the
// module's share of the group's tables (what the workspace query returns)
struct ModPlan {
  int ksh, ksj, kst, colh, colj;
  size_t off_slabH, off_slabJ, off_partA, off_partB, off_yH, off_yJ, area, bytes;
};

// the finish's job list (one int4 per split stripe) is part of the group's tables: room for every stripe
inline size_t finish_jobs_bytes(int64_t in, int64_t out) {
  return (size_t)(((in + kSwC - 1) / kSwC + (out + kSwC - 1) / kSwC) * 16 + 255) / 256 * 256;
}

// pieces per stripe (capacity): what ranges of >= kSwMinSteps steps can produce
inline int sweep_kmax(int64_t T) { return (int)(((T + 15) / 16 + kSwMinSteps - 1) / kSwMinSteps) + 2; }

// table space at the head of a sweep group's workspace (Item: anything with .in and .out -- the
// caller's items before the work areas are carved, the planned modules at the launch)
template <class Item>
inline size_t sweep_table_bytes(const Item* it, int n) {
  size_t b = kTableFixed + (size_t)n * kTablePerModule;
  for (int i = 0; i < n; ++i) b += finish_jobs_bytes(it[i].in, it[i].out);
  return b;
}

inline ModPlan plan_sweep_module(int64_t T, int64_t in, int64_t out, int r) {
  ModPlan p;
  const int RB = rb_of(r), rp = 16 * RB;
  size_t off = 0;
  auto take = [&](size_t n) { size_t o = off; off += (n * 4 + 255) / 256 * 256; return o; };
  p.ksh = (int)((in + kSwC - 1) / kSwC);
  p.ksj = (int)((out + kSwC - 1) / kSwC);
  p.colh = p.colj = 0;
  p.kst = sweep_kmax(T);  // pieces per stripe (capacity)
  // slabs [nct][T16][rp] and projections [T16][rp] floats (T16 = T rounded up to 16 rows)
  const size_t T16 = (size_t)((T + 15) / 16) * 16;
  p.off_slabH = take((size_t)p.ksh * T16 * rp);
  p.off_slabJ = take((size_t)p.ksj * T16 * rp);
  p.off_partA = take((size_t)p.ksh * p.kst * rp * kSwC);
  p.off_partB = take((size_t)p.ksj * p.kst * rp * kSwC);
  // projections: [T16][rp], or the padded shared-X layout [T16][16 lanes][4 blocks] (r-block <= 2)
  const size_t yrow = RB <= 2 ? 64 : 2 * (size_t)rp;
  p.off_yH = take(T16 * yrow);
  p.off_yJ = take(T16 * yrow);
  p.area = off;
  // + this module's share of the group's tables and counters
  p.bytes = off + kTablePerModule + kTableFixed + 256 + finish_jobs_bytes(in, out);
  return p;
}

// a module's buffers at `area` (the start of its work area in the group workspace)
inline void place_module(ProbeDesc& d, const ModPlan& p, char* area) {
  d.slabH = reinterpret_cast<float*>(area + p.off_slabH);
  d.slabJ = reinterpret_cast<float*>(area + p.off_slabJ);
  d.partA = reinterpret_cast<float*>(area + p.off_partA);
  d.partB = reinterpret_cast<float*>(area + p.off_partB);
  d.yH = reinterpret_cast<float*>(area + p.off_yH);
  d.yJ = reinterpret_cast<float*>(area + p.off_yJ);
  d.ksh = p.ksh;
  d.ksj = p.ksj;
  d.kst = p.kst;
  d.colh = p.colh;
  d.colj = p.colj;
}

// ---------------------------------------------------------------------------------------
// launch planning
// ---------------------------------------------------------------------------------------
// The launch's switches, read from the environment by hdp_probe.hip once per launch (tests flip them per
// case).  The planner uses share_x and balance; k32 and x6 only choose kernel instances.
struct SweepKnobs {
  bool share_x = true;  // HDP_PROBE_SHARE_X=0: no X-sharing sets
  bool balance = true;  // HDP_PROBE_BALANCE=0: the equal split w * U / G in every phase
  int k32 = 2;          // HDP_PROBE_K32: 0 off, 1 r-block 4 only, 2 (default) PROJ phases at every r-block and
                        // the OUTER phase at r-block 4, 3 every phase and r-block
  bool x6 = true;       // HDP_PROBE_X6=0: float32 phase A of a shared-X group keeps f32 MFMA
};

// a failed check: the HDP_E* code (hdpissa.h) and the message for set_error; code 0 = planned
struct SweepError {
  int code;
  const char* msg;
};
constexpr int kSweepEInval = 1;  // HDP_EINVAL

// Shared X (hp:139 is called with ONE hidden state per projection group of a decoder layer: q/k/v
// read the same normed x, gate/up the same x; autograd saves that one tensor for each of them).
// Modules of a group whose X is the same tensor (same pointer, T and in; B given transposed) are
// packed into sets of at most kSwMaxBlk r-blocks; a set streams its X ONCE per pass for all of its
// modules (phase A: PROJ against the stacked A rows; phase C: OUTER against the stacked
// projections of their G) instead of once per module.  A set is formed only when X is the smaller
// side (in <= sum of its modules' out): X is then the stream read twice.
inline std::vector<std::vector<int>> shared_x_sets(const HostGroup& ga, bool share_x) {
  std::vector<std::vector<int>> sets;
  const int n = ga.n;
  if (ga.RB > 2 || !share_x) return sets;
  for (int i = 0; i < n; ++i)
    if (!ga.d[i].b_t) return sets;
  std::vector<char> used(n, 0);
  for (int i = 0; i < n; ++i) {
    if (used[i]) continue;
    const ProbeDesc& p = ga.d[i];
    std::vector<int> cur{i};
    int64_t outs = p.out;
    for (int k = i + 1; k < n && (int)(cur.size() + 1) * ga.RB <= kSwMaxBlk; ++k) {
      const ProbeDesc& q = ga.d[k];
      if (!used[k] && q.X == p.X && q.T == p.T && q.in == p.in) {
        cur.push_back(k);
        outs += q.out;
      }
    }
    if (cur.size() < 2 || outs < p.in) continue;
    for (int k : cur) used[k] = 1;
    sets.push_back(cur);
  }
  return sets;
}

// the plain side descriptor of one module stream (X: PROJ -> H, OUTER with J -> pieces A; G: PROJ
// -> J, OUTER with H -> pieces B^T), its r-block view filled for the FUSE instances
inline SweepDesc side_desc(const ProbeDesc& p, bool xs, int RB, int S) {
  const int rp = 16 * RB;
  SweepDesc d{};
  d.Z = xs ? p.X : p.G;
  d.F = xs ? p.A : p.B;
  d.slab_out = xs ? p.slabH : p.slabJ;
  d.y_in = xs ? p.yJ : p.yH;
  d.part = xs ? p.partA : p.partB;
  d.T = p.T;
  d.N = xs ? p.in : p.out;
  d.pre = 0;
  d.r = p.r;
  d.f_rk = xs ? 1 : p.b_t;
  d.part_t = xs ? 0 : 1;
  d.nct = xs ? p.ksh : p.ksj;
  d.S = S;
  d.kmax = p.kst;
  d.g = xs ? p.gA : p.gB;
  d.scale = p.scale;
  d.acc = p.accumulate;
  d.ldb = xs ? p.r : p.ldb;
  d.yrs = rp;
  d.yls = RB;
  d.nb = RB;
  d.rpm = rp;
  for (int b = 0; b < kSwMaxBlk; ++b) {
    const int rows = p.r - 16 * b;
    d.rbr[b] = b < RB ? (rows < 0 ? 0 : rows > 16 ? 16 : rows) : 0;
    d.Fb[b] = d.F + (int64_t)16 * b * d.N;  // f_rk rows (FUSE requires B^T)
    d.slab_b[b] = d.slab_out + 16 * b;
    d.part_b[b] = d.part_t ? d.part + 16 * b : d.part + (int64_t)16 * b * kSwC;
    d.gb[b] = d.part_t ? d.g + 16 * b : d.g + (int64_t)16 * b * d.N;
    d.sc[b] = p.scale;
    d.accb[b] = p.accumulate;
  }
  return d;
}

// Stage 1: everything that does not depend on how many workgroups are resident.
// Phases A (PROJ over S1), R1 (reduce S1 slabs), B (PROJ + OUTER over S2), R2 (reduce S2 slabs), C
// (OUTER over S1), D (finish).  With X-sharing sets phases A and C run the FUSE instance (4 r-blocks,
// runtime nb) over every S1 side; phase B, the reduces and the finish keep their kernels (descriptor
// strides).
struct SweepSides {
  // bf16 data at r-block 4: phase B is PROJ only (bf16 MFMA, split fragments -- fused with OUTER they
  // do not fit beside its accumulators) and S2's OUTER joins S1's in phase C: S2 is read twice, its
  // projection costs a fifth of the f32 MFMA issue time
  bool split_b = false;
  bool fuse = false;      // the group has X-sharing sets
  bool v4 = true;         // 4 elements per finish thread: every module allows it
  bool weighted = false;  // phase A's ranges by cost (kSwWeightA): float32 shared-X group
  std::vector<std::vector<int>> sets;
  std::vector<SweepDesc> sd[3];  // the phases' sides, in flattened-step order (pre set)
  std::vector<YRedDesc> yd[2];   // R1, R2: per module
  std::vector<FinDesc> fd;       // per module
  int64_t U[3] = {0, 0, 0};      // steps per phase
  int64_t yblk = 1;              // the reduces' grid x
  // what the timers count: stream bytes / flop per phase, and the workspace bytes the reduces move
  double bytes_ph[3] = {0, 0, 0}, flop_ph[3] = {0, 0, 0}, slab[2] = {0, 0};
};

inline void plan_sweep_sides(const HostGroup& ga, bool bf16, const SweepKnobs& kn, SweepSides& s) {
  const int n = ga.n, RB = ga.RB, rp = 16 * RB;
  const bool SPLIT_B = RB >= 4 && bf16;
  const int ES = bf16 ? 2 : 4;
  s.split_b = SPLIT_B;
  if (!SPLIT_B) s.sets = shared_x_sets(ga, kn.share_x);
  const std::vector<std::vector<int>>& sets = s.sets;
  const bool fuse = !sets.empty();
  s.fuse = fuse;
  s.weighted = fuse && !bf16 && kn.balance;
  std::vector<int> set_of(n, -1), blk0(n, 0);
  for (int k = 0; k < (int)sets.size(); ++k)
    for (int m = 0; m < (int)sets[k].size(); ++m) {
      set_of[sets[k][m]] = k;
      blk0[sets[k][m]] = m * RB;
    }
  std::vector<char> s1x(n);
  std::vector<int> at_c(n, -1), at_b(n, -1);  // each module's X / G side: index in its OUTER phase
  auto add = [&](int ph, SweepDesc d) {
    d.pre = s.U[ph];
    s.U[ph] += (int64_t)d.nct * d.S;
    int rows = 0;
    for (int b = 0; b < d.nb && b < kSwMaxBlk; ++b) rows += d.rbr[b];
    s.bytes_ph[ph] += (double)ES * d.T * d.N;
    s.flop_ph[ph] += 2.0 * d.T * d.N * (fuse && (ph != 1) ? rows : d.r) * (ph == 1 && !SPLIT_B ? 2.0 : 1.0);
    s.sd[ph].push_back(d);
    return (int)s.sd[ph].size() - 1;
  };
  for (int k = 0; k < 2; ++k) s.yd[k].resize(n);
  s.fd.resize(n);
  for (int i = 0; i < n; ++i) {
    const ProbeDesc& p = ga.d[i];
    const int S = (int)((p.T + 15) / 16);
    const int si = set_of[i];
    s1x[i] = si >= 0 ? 1 : (p.in <= p.out);  // S1 = the smaller stream, read twice (a set: its X)
    SweepDesc x = side_desc(p, true, RB, S), gg = side_desc(p, false, RB, S);
    if (si >= 0) {
      const ProbeDesc& lead = ga.d[sets[si][0]];
      // this module's G side reads its H in phase B: member m's [T][16 lanes][RB] slice of the set's
      // H buffer (lead's yH, rows of 64 floats: the plain layout per member, member-major)
      gg.y_in = lead.yH + 16 * blk0[i];
      gg.yrs = 4 * 16;
      if (sets[si][0] == i) {  // the set's X side (phases A and C), r-blocks of every member
        SweepDesc fx = x;
        fx.nb = RB * (int)sets[si].size();
        fx.y_in = lead.yJ;  // the set's padded J (phase C)
        fx.yrs = 4 * 16;
        fx.yls = 4;
        for (int m = 0; m < (int)sets[si].size(); ++m) {
          const SweepDesc xm = side_desc(ga.d[sets[si][m]], true, RB, S);
          for (int bb = 0; bb < RB; ++bb) {
            const int b = m * RB + bb;
            fx.Fb[b] = xm.Fb[bb];
            fx.rbr[b] = xm.rbr[bb];
            fx.slab_b[b] = xm.slab_b[bb];
            fx.part_b[b] = xm.part_b[bb];
            fx.gb[b] = xm.gb[bb];
            fx.sc[b] = xm.sc[bb];
            fx.accb[b] = xm.accb[bb];
          }
        }
        add(0, fx);
        at_c[i] = add(2, fx);
        for (int m : sets[si]) at_c[m] = at_c[i];
      }
      at_b[i] = add(1, gg);
    } else {
      const SweepDesc& d1 = s1x[i] ? x : gg;
      SweepDesc d2 = s1x[i] ? gg : x;
      SweepDesc d1c = d1;
      if (fuse) {  // phase C runs the FUSE instance: Y_S2 in the padded layout
        d1c.yrs = 4 * 16;
        d1c.yls = 4;
      }
      add(0, d1);
      if (SPLIT_B) {  // S2's OUTER, right after S1's in phase C
        add(1, d2);
        const int c1 = add(2, d1c);
        const int c2 = add(2, d2);
        at_c[i] = s1x[i] ? c1 : c2;  // X side
        at_b[i] = s1x[i] ? c2 : c1;  // G side (both in phase C)
      } else {
        const int bi = add(1, d2);
        const int ci = add(2, d1c);
        at_c[i] = s1x[i] ? ci : bi;
        at_b[i] = s1x[i] ? bi : ci;
      }
    }
    // R1: S1's slabs -> the projection phase B reads; R2: S2's slabs -> the one phase C reads
    if (si >= 0) {
      const ProbeDesc& lead = ga.d[sets[si][0]];
      s.yd[0][i] = YRedDesc{p.slabH, lead.yH + 16 * blk0[i], p.T, p.ksh, 4 * 16, RB, 0};
      s.yd[1][i] = YRedDesc{p.slabJ, lead.yJ + blk0[i], p.T, p.ksj, 4 * 16, 4, 0};
    } else {
      const SweepDesc& d1 = s1x[i] ? x : gg;
      const SweepDesc& d2 = s1x[i] ? gg : x;
      s.yd[0][i] = YRedDesc{d1.slab_out, s1x[i] ? p.yH : p.yJ, p.T, d1.nct, rp, RB, 0};
      s.yd[1][i] = YRedDesc{d2.slab_out, s1x[i] ? p.yJ : p.yH, p.T, d2.nct, fuse ? 4 * 16 : rp, fuse ? 4 : RB, 0};
    }
    const int64_t yb = (p.T * rp / 4 + 255) / 256;
    s.yblk = yb > s.yblk ? yb : s.yblk;
    s.fd[i] = FinDesc{p.gA, p.gB, (int)p.in, (int)p.out, p.r, p.accumulate, p.scale, p.ldb, {}, {}};
    s.v4 = s.v4 && p.r % 4 == 0 && p.ldb % 4 == 0 && p.in % 4 == 0 && (reinterpret_cast<uintptr_t>(p.gA) & 15) == 0 &&
           (reinterpret_cast<uintptr_t>(p.gB) & 15) == 0 && (reinterpret_cast<uintptr_t>(p.partA) & 15) == 0 &&
           (reinterpret_cast<uintptr_t>(p.partB) & 15) == 0;
  }
  // finish: the pieces of X's OUTER and of G's (SwFinishSide::ph 0 = phase B, 1 = phase C); every
  // module's pieces are in its own part buffers (a shared-X set's OUTER writes each member's rows there)
  for (int i = 0; i < n; ++i) {
    const ProbeDesc& p = ga.d[i];
    const bool x_in_c = SPLIT_B || s1x[i], g_in_c = SPLIT_B || !s1x[i];
    const SweepDesc& dx = s.sd[x_in_c ? 2 : 1][at_c[i]];
    const SweepDesc& dg = s.sd[g_in_c ? 2 : 1][at_b[i]];
    s.fd[i].sx = SwFinishSide{p.partA, dx.pre, dx.S, dx.kmax, x_in_c ? 1 : 0, 0};
    s.fd[i].sg = SwFinishSide{p.partB, dg.pre, dg.S, dg.kmax, g_in_c ? 1 : 0, 0};
    // workspace bytes the reduce passes move (slabs + Y) -- counted as algorithmic for these launches:
    // they are the price of the stripe decomposition
    for (int k = 0; k < 2; ++k) s.slab[k] += 4.0 * p.T * rp * (s.yd[k][i].nct + 1);
  }
}

// resident workgroups of one phase: the kernel instance's occupancy x CUs (`slots`, from the caller),
// capped so each gets >= kSwMinSteps steps
inline int phase_grid(int64_t U, int slots) {
  const int64_t cap = U / kSwMinSteps;
  return (int)(cap < 1 ? 1 : (cap < slots ? cap : slots));
}

// the ranges of one phase's workgroups (plan_ranges); weights = per-nb step costs, or null for equal steps
inline int phase_ranges(const std::vector<SweepDesc>& d, int G, const int* weights, std::vector<int64_t>& bounds) {
  std::vector<PlanSide> sides(d.size());
  for (size_t i = 0; i < d.size(); ++i) {
    const int nb = d[i].nb < 1 ? 1 : d[i].nb > kSwMaxBlk ? kSwMaxBlk : d[i].nb;
    sides[i] = PlanSide{d[i].pre, d[i].nct, d[i].S, weights ? weights[nb] : 1};
  }
  return plan_ranges(sides, G, kSwMinSteps, bounds);
}

// where workgroup w of G starts: (module, stripe, step) of flattened step bounds[w], and the workgroups before
// it on that stripe (its first segment's piece index); bnd = the device's bounds
inline void phase_starts(const std::vector<SweepDesc>& d, const std::vector<int64_t>& bounds, int G, int* out,
                         int* bnd) {
  int m = 0;
  for (int w = 0; w <= G; ++w) bnd[w] = (int)bounds[w];
  for (int w = 0; w < G; ++w) {
    const int64_t lo = bounds[w];
    while (m + 1 < (int)d.size() && lo >= d[m + 1].pre) ++m;
    const int64_t rem = lo - d[m].pre;
    out[4 * w] = m;
    out[4 * w + 1] = (int)(rem / d[m].S);
    out[4 * w + 2] = (int)(rem % d[m].S);
    out[4 * w + 3] = w - plan_owner(bounds, lo - rem % d[m].S);
  }
}

// Stage 2: the tables that depend on the resident workgroups of each phase's kernel instance.
struct SweepTables {
  int G[3] = {0, 0, 0};            // workgroups per phase (the launch grids)
  std::vector<int64_t> bounds[3];  // their ranges: G + 1 boundaries, 0 .. U
  int njobs = 0;                   // split stripes: the finish's jobs
  double pieces = 0;               // bytes the finish moves (its timer)
  // one blob: [sd A | sd B | sd C | wst A | wst B | wst C | bnd A | bnd B | bnd C | yd R1 | yd R2 | fd | jobs],
  // sections at multiples of 256 bytes
  size_t o_sd[3] = {0, 0, 0}, o_w[3] = {0, 0, 0}, o_b[3] = {0, 0, 0}, o_y[2] = {0, 0}, o_f = 0, o_j = 0;
  std::vector<char> blob;
};

inline SweepError plan_sweep_tables(const HostGroup& ga, const SweepSides& s, const int slots[3], SweepTables& t) {
#define HDP_PLAN_CHECK(cond, text) \
  do {                             \
    if (!(cond)) return SweepError{kSweepEInval, text}; \
  } while (0)
  const int n = ga.n, rp = 16 * ga.RB;
  for (int ph = 0; ph < 3; ++ph) t.G[ph] = phase_grid(s.U[ph], slots[ph]);
  HDP_PLAN_CHECK(t.G[0] <= 4096 && t.G[1] <= 4096 && t.G[2] <= 4096, "probe sweep: grid above the table size");
  HDP_PLAN_CHECK(s.yblk < 65536 && n < 65536, "probe sweep: group too large");
  // the workgroups' ranges: cost-weighted in phase A of a float32 shared-X group, equal steps elsewhere
  for (int ph = 0; ph < 3; ++ph) {
    HDP_PLAN_CHECK(s.U[ph] < (1ll << 31), "probe sweep: too many steps in one phase");
    t.G[ph] = phase_ranges(s.sd[ph], t.G[ph], s.weighted && ph == 0 ? kSwWeightA : nullptr, t.bounds[ph]);
    // memory safety: a stripe's piece buffer holds sweep_kmax pieces, which is what ranges of >= kSwMinSteps
    // steps can produce (a single workgroup may hold fewer: one piece per stripe)
    const int64_t least = s.U[ph] < kSwMinSteps ? s.U[ph] : kSwMinSteps;
    const std::vector<int64_t>& b = t.bounds[ph];
    bool ok = (int)b.size() == t.G[ph] + 1 && b[0] == 0 && b[t.G[ph]] == s.U[ph];
    for (int w = 0; ok && w < t.G[ph]; ++w) ok = b[w + 1] - b[w] >= least;
    HDP_PLAN_CHECK(ok, "probe sweep: a workgroup range below the minimum step count");
  }
  size_t off = 0;
  auto place = [&](size_t bytes) { size_t o = off; off += (bytes + 255) / 256 * 256; return o; };
  for (int ph = 0; ph < 3; ++ph) t.o_sd[ph] = place(sizeof(SweepDesc) * s.sd[ph].size());
  for (int ph = 0; ph < 3; ++ph) t.o_w[ph] = place(sizeof(int) * 4 * t.G[ph]);
  for (int ph = 0; ph < 3; ++ph) t.o_b[ph] = place(sizeof(int) * (t.G[ph] + 1));
  for (int k = 0; k < 2; ++k) t.o_y[k] = place(sizeof(YRedDesc) * n);
  t.o_f = place(sizeof(FinDesc) * n);
  // the finish's jobs: the stripes that more than one workgroup segment covered (the others wrote their
  // gradient blocks in phase B / C)
  std::vector<int> jobs;
  t.pieces = 0;
  for (int i = 0; i < n; ++i) {
    const ProbeDesc& p = ga.d[i];
    for (int side = 0; side < 2; ++side) {
      const SwFinishSide& fs = side == 0 ? s.fd[i].sx : s.fd[i].sg;
      const int nct = side == 0 ? p.ksh : p.ksj;
      const std::vector<int64_t>& b = t.bounds[fs.ph + 1];  // phase B = 1, C = 2
      for (int ct = 0; ct < nct; ++ct) {
        const int64_t u0 = fs.pre + (int64_t)ct * fs.S;
        const int np = plan_owner(b, u0 + fs.S - 1) - plan_owner(b, u0) + 1;
        if (np > 1) {
          HDP_PLAN_CHECK(np <= fs.kmax, "probe sweep: a stripe has more pieces than its buffer holds");
          jobs.push_back(i);
          jobs.push_back(2 * ct + side);
          jobs.push_back(np);
          jobs.push_back(0);
          // the finish reads the pieces and updates the gradient of split stripes only
          t.pieces += 4.0 * p.r * kSwC * ((double)np + (p.accumulate ? 2 : 1));
        }
      }
    }
  }
  t.njobs = (int)(jobs.size() / 4);
  HDP_PLAN_CHECK((int64_t)t.njobs * (rp * kSwC / 256) < (1ll << 31), "probe sweep: finish grid too large");
  t.o_j = place(sizeof(int) * jobs.size());
  HDP_PLAN_CHECK(off <= sweep_table_bytes(ga.d.data(), n), "probe sweep: descriptor tables exceed their space");
#undef HDP_PLAN_CHECK
  t.blob.resize(off);
  char* blob = t.blob.data();
  for (int ph = 0; ph < 3; ++ph) {
    if (!s.sd[ph].empty()) memcpy(blob + t.o_sd[ph], s.sd[ph].data(), sizeof(SweepDesc) * s.sd[ph].size());
    phase_starts(s.sd[ph], t.bounds[ph], t.G[ph], reinterpret_cast<int*>(blob + t.o_w[ph]),
                 reinterpret_cast<int*>(blob + t.o_b[ph]));
  }
  for (int k = 0; k < 2; ++k) memcpy(blob + t.o_y[k], s.yd[k].data(), sizeof(YRedDesc) * n);
  memcpy(blob + t.o_f, s.fd.data(), sizeof(FinDesc) * n);
  if (t.njobs) memcpy(blob + t.o_j, jobs.data(), sizeof(int) * jobs.size());
  return SweepError{0, nullptr};
}

}  // namespace hdp
