// Host plan of the K4 delta GEMM (hdp_delta.hip): the descriptor the kernels read, the geometry constants
// the packed-panel image and the scale tables rest on, the validation of one item, and everything a grouped
// plan decides before its first HIP call -- which one kernel instance runs, the tile prefix, the image and
// table offsets of every item, and the thread-space prefixes of the pack, scale and fused Adam-pack kernels.
// Pure C++ (no HIP, no environment): hipcc and the host compiler build the same code, and
// tests/k4_plan_check.cpp runs it on the CPU (tests/test_k4_plan.py, plain and under ASan/UBSan).  The
// planner only does arithmetic on the pointers it is given; it never dereferences one.
#pragma once
#include <algorithm>
#include <climits>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "hdpissa.h"

namespace hdp {

#if defined(__HIP__)
using k4_img_t = __bf16;  // the kernels' view of a panel element (fp16 under H2: the same pointers reinterpreted)
#define HDP_K4_HD __host__ __device__
#else
using k4_img_t = uint16_t;
#define HDP_K4_HD
#endif

struct DeltaArgs {
  int64_t out, in;
  int r, nseg;
  const float* dA;
  const float* dB;
  int64_t dstr;
  const float* A;
  const float* B;
  int64_t fstr;
  void* dst;
  int vec_l;   // L rows 16-B aligned (r % 4 == 0, aligned bases and strides)
  int vec_r;   // R rows 16-B aligned (in % 4 == 0, aligned bases and strides)
  k4_img_t* limg;  // packed bf16x3 panels (plans with x3 math; see MX3P), else null
  k4_img_t* rimg;  //   (fp16x2 panels for H2 plans: the same pointers reinterpreted)
  float* ktab;     // H2 plans: the item's per-k scale table (see h2_tab_floats), else null
};
// the device reads it as the host wrote it: both compilers must agree on the layout
static_assert(sizeof(DeltaArgs) == 112, "DeltaArgs layout");
static_assert(offsetof(DeltaArgs, out) == 0 && offsetof(DeltaArgs, in) == 8 && offsetof(DeltaArgs, r) == 16 &&
                  offsetof(DeltaArgs, nseg) == 20 && offsetof(DeltaArgs, dA) == 24 && offsetof(DeltaArgs, dB) == 32 &&
                  offsetof(DeltaArgs, dstr) == 40 && offsetof(DeltaArgs, A) == 48 && offsetof(DeltaArgs, B) == 56 &&
                  offsetof(DeltaArgs, fstr) == 64 && offsetof(DeltaArgs, dst) == 72 && offsetof(DeltaArgs, vec_l) == 80 &&
                  offsetof(DeltaArgs, vec_r) == 84 && offsetof(DeltaArgs, limg) == 88 &&
                  offsetof(DeltaArgs, rimg) == 96 && offsetof(DeltaArgs, ktab) == 104,
              "DeltaArgs layout");

constexpr int kDT = 128;               // workgroup tile (both dims; the wide and H2 kernels take 2 kDT rows)
constexpr int kX3Steps = 8;            // steps (16 k-slots) of one x3 chunk (MX3::kSteps)
constexpr int kPanel = 3 * kDT * 16;   // bf16 elements per packed x3 panel
constexpr int kPanelH = 2 * kDT * 16;  // fp16 elements per H2 panel: [2 parts][128][16 k]

// A deferred merge finishes the previous tile's W inside the next tile's chunk loop: every tile of the
// plan needs at least this many chunks (X3WDefer<DEF>::min_chunks; H2 counts 32-k chunks)
constexpr int k4_defer_min_chunks(int def) { return def == 1 ? 11 : def == 2 ? 6 : def == 4 ? 7 : 0; }
constexpr int kDeferBf16MinChunks = 4;  // DEF 3, the deferred bf16 merge of delta_h2_kernel

// chunks of one item's k loop: ceil(r / 8) per segment; the H2 image pads the count to even (its kernel
// takes two 16-k panels per 32-k chunk)
inline int64_t k4_chunks(int r, int nseg, bool h2) {
  const int64_t nch = (int64_t)nseg * ((r + kX3Steps - 1) / kX3Steps);
  return h2 ? (nch + 1) / 2 * 2 : nch;
}

// H2 per-item table (floats): [0] = 2^-E, [4 ..) sl[K], then sr[K], then the scale pass's
// partial maxima: L [seg][ceil(out / 256)][2r], R [seg][ceil(in / 256)][2r]; with
// k = (2 seg + half) r + step (half 0: dB | A - dA, half 1: B | dA)
inline int64_t h2_tab_floats(int64_t out, int64_t in, int r, int nseg) {
  const int64_t K = 2ll * r * nseg;
  return 4 + 2 * K + (int64_t)nseg * ((out + 255) / 256 + (in + 255) / 256) * 2 * r + 2 * r;
}
// the fused Adam + pack path (single-segment plans): constant maxima max_o |B[o][k]| (r floats), then
// max_c |A[k][c]| (r floats), behind the scale pass's partials
HDP_K4_HD inline int64_t h2_cmax_off(int64_t out, int64_t in, int r, int nseg) {
  return 4 + 4ll * r * nseg + (int64_t)nseg * ((out + 255) / 256 + (in + 255) / 256) * 2 * r;
}
// threads of k4_h2_adam_pack_kernel for one item: one per 4 factor entries, or per 8 k-slots when r % 8 == 0
inline int64_t h2_ap_threads(int64_t out, int64_t in, int r) {
  if (r % 8 == 0) return out * (r / 8) + (in + 3) / 4 * (r / 8);
  const int64_t qr = (r + 3) / 4;
  return out * qr + (in + 3) / 4 * qr;
}

// what the environment and the two process-wide setters say (hdp_delta.hip fills it; k4_knobs())
struct K4Knobs {
  int math = HDP_MATH_AUTO;  // HDP_K4_MATH / hdp_delta_set_math
  int stage = HDP_X3_WIDE;   // HDP_K4_X3_STAGE / hdp_delta_set_x3_stage
  bool store_f32 = false;    // HDP_K4_STORE=f32: float32 STORE plans keep the f32 form at K = 32
  bool rnd_x3 = false;       // HDP_K4_RND=x3: bf16 ROUND merges stay on bf16x3
  bool defer_set = false;    // HDP_K4_DEFER given
  int defer = 0;             //   its value
  int pol = 3;               // HDP_DELTA_POL & 15: float32 MERGE cache policy (bit 0 nt stores, bit 1 nt W loads)
};

struct K4Error {
  int code = HDP_OK;
  char msg[256] = {0};
};
#define HDP_K4_CHECK(cond, ...)                          \
  do {                                                   \
    if (!(cond)) {                                       \
      K4Error e_;                                        \
      e_.code = HDP_EINVAL;                              \
      std::snprintf(e_.msg, sizeof(e_.msg), __VA_ARGS__); \
      return e_;                                         \
    }                                                    \
  } while (0)

inline bool k4_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// validate one module's operands and fill its descriptor (shared by both entry points)
inline K4Error k4_make_args(const char* who, int64_t out, int64_t in, int r, int nseg, const float* dA, const float* dB,
                            int64_t delta_seg_stride, const float* A, const float* B, int64_t factor_seg_stride,
                            void* dst, int dst_dtype, int mode, int round_bf16, DeltaArgs& a) {
  HDP_K4_CHECK(out > 0 && in > 0 && r > 0 && nseg > 0, "%s: bad shape out=%lld in=%lld r=%d nseg=%d", who,
               (long long)out, (long long)in, r, nseg);
  // (out <= 2^31 / in first: the product itself must not overflow)
  HDP_K4_CHECK(out <= INT32_MAX / in &&
                   out * in * (dst_dtype == HDP_BF16 && mode == HDP_DW_MERGE ? 2 : 4) < ((int64_t)1 << 31),
               "%s: matrix too large (%lld x %lld; the kernel addresses one module's dst with 31-bit offsets)", who,
               (long long)out, (long long)in);
  HDP_K4_CHECK(dA && dB && A && B && dst, "%s: null pointer", who);
  HDP_K4_CHECK(mode == HDP_DW_STORE || mode == HDP_DW_MERGE, "%s: bad mode %d", who, mode);
  HDP_K4_CHECK(dst_dtype == HDP_F32 || dst_dtype == HDP_BF16, "%s: bad dtype %d", who, dst_dtype);
  HDP_K4_CHECK(mode == HDP_DW_MERGE || dst_dtype == HDP_F32, "%s: STORE mode writes float32", who);
  HDP_K4_CHECK(!(round_bf16 && mode == HDP_DW_MERGE && dst_dtype == HDP_F32),
               "%s: round_bf16 applies to bf16 W_res (or STORE), not to a float32 merge", who);
  HDP_K4_CHECK(nseg == 1 || (delta_seg_stride > 0 && factor_seg_stride > 0), "%s: segment strides must be positive",
               who);
  a.out = out;
  a.in = in;
  a.r = r;
  a.nseg = nseg;
  a.dA = dA;
  a.dB = dB;
  a.dstr = delta_seg_stride;
  a.A = A;
  a.B = B;
  a.fstr = factor_seg_stride;
  a.dst = dst;
  const bool strides4 = nseg == 1 || (delta_seg_stride % 4 == 0 && factor_seg_stride % 4 == 0);
  a.vec_l = (r % 4 == 0) && k4_al16(dB) && k4_al16(B) && strides4;
  a.vec_r = (in % 4 == 0) && k4_al16(dA) && k4_al16(A) && strides4;
  a.limg = a.rimg = nullptr;
  a.ktab = nullptr;
  return K4Error{};
}

// algorithmic work of one module: dst written (and W read for MERGE) once + the 4 factor
// operands once; 4 r nseg flop per element
inline double k4_args_bytes(const DeltaArgs& a, int mode, int dst_dtype) {
  const double wes = (mode == HDP_DW_MERGE && dst_dtype == HDP_BF16) ? 2.0 : 4.0;
  return (double)a.out * a.in * (mode == HDP_DW_MERGE ? 2.0 * wes : 4.0) + 8.0 * a.r * (a.out + a.in) * a.nseg;
}
inline double k4_args_flops(const DeltaArgs& a) { return 4.0 * a.out * a.in * a.r * a.nseg; }
inline int64_t k4_args_tiles(const DeltaArgs& a, int tr = kDT) {
  return ((a.out + tr - 1) / tr) * ((a.in + kDT - 1) / kDT);
}

// AUTO takes the exact f32 MFMA while K4 is HBM-bound (K = 2 r nseg <= 32) and a split form above that
inline bool k4_use_x3(int math, int r, int nseg) {
  return math == HDP_MATH_X3 || math == HDP_MATH_H2 || (math == HDP_MATH_AUTO && 2ll * r * nseg > 32);
}

// One launched plan-kernel instance.  Normalised: a field the instance does not take is zero.
enum { K4_F32 = 0, K4_X3_REGS = 1, K4_X3_GLDS = 2, K4_X3_WIDE = 3, K4_H2 = 4 };
struct K4Choice {
  int family = K4_F32;  // delta_group_kernel<.., MF32> / delta_x3p / delta_x3g / delta_x3w / delta_h2
  int mode = 0, dtype = 0;
  int round = 0;        // STORE, bf16 MERGE: the per-segment bf16 rounding (H2: RND)
  int pol = 0;          // float32 MERGE: cache policy instance
  int def = 0;          // deferred merge: 1 / 2 (wide f32), 2 / 4 (H2 f32), 3 (H2 bf16)
};

// the instances hdp_delta.hip has (pick_k4 names one kernel for each)
inline bool k4_choice_valid(const K4Choice& c) {
  if (c.family < K4_F32 || c.family > K4_H2) return false;
  if (c.round != 0 && c.round != 1) return false;
  const bool h2 = c.family == K4_H2;
  if (c.mode == HDP_DW_STORE) return c.dtype == HDP_F32 && c.pol == 0 && c.def == 0 && !(h2 && c.round);
  if (c.mode != HDP_DW_MERGE) return false;
  if (c.dtype == HDP_BF16) return c.pol == 0 && (c.def == 0 || (h2 && c.def == 3));
  if (c.dtype != HDP_F32 || c.round) return false;
  if (h2) return c.pol == 3 ? (c.def == 0 || c.def == 2 || c.def == 4) : (c.pol == 0 && c.def == 0);
  const bool pol_ok = c.pol == 0 || c.pol == 1 || c.pol == 2 || c.pol == 3 || c.pol == 4 || c.pol == 7 ||
                      c.pol == 11 || c.pol == 15;
  return pol_ok && (c.def == 0 || (c.family == K4_X3_WIDE && c.pol == 3 && (c.def == 1 || c.def == 2)));
}

struct K4ItemOff {
  int64_t limg, rimg;  // elements into the plan's panel image (L base, R base)
  int64_t ktab;        // floats into the plan's scale tables (H2)
};

struct K4Plan {
  K4Choice choice;
  int tile_rows = kDT;  // 2 kDT for the wide and H2 kernels
  int multiseg = 0;
  int fused = 0;        // H2 single-segment MERGE: hdp_delta_plan_run_adam applies
  int64_t total = 0;    // tiles
  int64_t img_elems = 0, ktab_floats = 0;
  int64_t pack_total = 0, ap_total = 0;  // thread spaces (multiples of 256)
  int sblocks = 0;                       // k4_h2_scale_kernel workgroups
  double bytes = 0.0, flops = 0.0;
  double pack_bytes = 0.0;  // x3 / H2 operand preparation: factors read by the scale pass (H2) and the pack,
                            // panels written (24 B per (row or column, k-slot) for H2, 20 B for x3)
  double adam_bytes = 0.0;  // fused Adam + pack: g, m, v read, m, v, delta, g written (28 B per entry),
                            // + A read and 8 B of R panel per A entry, 4 B of L panel per B entry
  std::vector<DeltaArgs> args;   // limg / rimg / ktab null: patched from `off` once the buffers exist
  std::vector<K4ItemOff> off;
  std::vector<int64_t> start;    // tile prefix (n + 1)
  std::vector<int64_t> pstart;   // x3 / H2: pack kernel thread-space prefix (256-aligned)
  std::vector<int> sstart;       // H2: k4_h2_scale_kernel workgroup prefix
  std::vector<int64_t> apst;     // fused: k4_h2_adam_pack_kernel thread-space prefix (256-aligned)

  bool x3() const { return choice.family != K4_F32; }
  bool h2() const { return choice.family == K4_H2; }
};

// everything hdp_delta_plan_create decides before its first HIP call
inline K4Error k4_plan(const hdp_delta_item* items, int n, int dst_dtype, int mode, int round_bf16,
                       const K4Knobs& kn, K4Plan& p) {
  HDP_K4_CHECK(items && n > 0, "hdp_delta_plan_create: need a plan pointer and n > 0 items");
  p = K4Plan{};
  p.args.resize(n);
  int kmax_r = 0, kmax_seg = 1;
  int64_t nch_min = INT64_MAX;  // fewest x3 chunks of any item's k loop
  bool even_segs = true;        // every segment ends on a 32-k chunk boundary
  for (int i = 0; i < n; ++i) {
    const hdp_delta_item& it = items[i];
    const K4Error e = k4_make_args("hdp_delta_plan_create", it.out, it.in, it.r, it.nseg, it.dA, it.dB,
                                   it.delta_seg_stride, it.A, it.B, it.factor_seg_stride, it.dst, dst_dtype, mode,
                                   round_bf16, p.args[i]);
    if (e.code != HDP_OK) return e;
    p.bytes += k4_args_bytes(p.args[i], mode, dst_dtype);
    p.flops += k4_args_flops(p.args[i]);
    p.multiseg |= it.nseg > 1;
    if (2ll * it.r * it.nseg > 2ll * kmax_r * kmax_seg) {
      kmax_r = it.r;
      kmax_seg = it.nseg;
    }
    nch_min = std::min(nch_min, k4_chunks(it.r, it.nseg, false));
    even_segs = even_segs && (k4_chunks(it.r, 1, false) & 1) == 0;
  }
  const bool merge = mode == HDP_DW_MERGE, bf16 = dst_dtype == HDP_BF16;
  // float32 STORE plans at K = 32 (Wn = 1, r = 16): the exact f32 MFMA form is MFMA-bound there (half the
  // bytes of a MERGE behind the same 64-cycle f32 MFMAs), so AUTO takes H2 from K = 32 on; HDP_K4_STORE=f32
  // keeps the f32 form
  const bool store_h2 = mode == HDP_DW_STORE && !round_bf16 && kn.math == HDP_MATH_AUTO &&
                        2ll * kmax_r * kmax_seg >= 32 && !kn.store_f32;
  const bool x3 = k4_use_x3(kn.math, kmax_r, kmax_seg) || store_h2;
  // a bf16 MERGE of single-segment items (Wn = 1): the ROUND form's dW = bf16(0 - bracket) added as
  // bf16(W + bf16(dW)) is bit-identical to the plain form, whose epilogue adds bf16(-acc) -- so it
  // runs without the running sum (and on the wide x3 kernel, which the ROUND form's registers spill)
  if (round_bf16 && merge && bf16 && !p.multiseg) round_bf16 = 0;
  // H2 (AUTO or HDP_MATH_H2) for float32 results and for bf16 merges without per-rank rounding
  // (single-segment plans, see above).  bf16 ROUND merges (Wn > 1) run on H2 too when every segment ends
  // on a 32-k chunk boundary (ceil(r / 8) even, i.e. r % 16 == 0 for the BASELINE configs): per-segment
  // bf16 folds in the kernel (RND); HDP_K4_RND=x3 keeps them on bf16x3
  const bool rnd_h2 = round_bf16 && merge && bf16 && even_segs && !kn.rnd_x3;
  const bool h2 = x3 && (kn.math == HDP_MATH_AUTO || kn.math == HDP_MATH_H2) && (!round_bf16 || rnd_h2);
  int stage = x3 ? kn.stage : HDP_X3_REGS;
  if (h2) stage = HDP_X3_WIDE;  // the same 256 x 128 tile geometry
  // the wide x3 kernel's bf16 ROUND merge (running sum + accumulators + bf16 W) spills: X3G there
  else if (stage == HDP_X3_WIDE && merge && bf16 && round_bf16) stage = HDP_X3_GLDS;

  K4Choice& c = p.choice;
  c.family = h2 ? K4_H2 : !x3 ? K4_F32 : stage == HDP_X3_WIDE ? K4_X3_WIDE : stage == HDP_X3_GLDS ? K4_X3_GLDS : K4_X3_REGS;
  c.mode = mode;
  c.dtype = dst_dtype;
  c.round = (merge && !bf16) ? 0 : round_bf16 != 0;
  if (merge && !bf16) {
    // the cache-policy instances that exist; H2 has the plain one and pol 3
    const int pol = kn.pol;
    const bool inst = h2 ? pol == 3 : (pol == 1 || pol == 2 || pol == 3 || pol == 4 || pol == 7 || pol == 11 || pol == 15);
    c.pol = inst ? pol : 0;
  }
  // deferred W merge: every tile needs the variant's minimum chunk count
  if (h2 && merge && !bf16 && c.pol == 3) {
    // X3WDefer<4> (W loads two chunks ahead) where every tile has >= 7 32-k chunks: LLaMA-2-7B shapes at
    // Wn = 8, 4 layers 2.415 -> 2.341 ms (tools/delta_bench.py --pol 3, r04); X3WDefer<2> from 6 on
    const int64_t nch2 = (nch_min + 1) / 2;
    int want = kn.defer_set ? kn.defer : 4;
    if (want == 4 && nch2 < k4_defer_min_chunks(4)) want = 2;
    c.def = (want != 0 && nch2 >= k4_defer_min_chunks(2)) ? (want == 4 ? 4 : 2) : 0;
  } else if (h2 && merge && bf16) {
    // (Mistral-7B r = 64, 8 layers: 3.28 -> 3.15 ms per run, tools/delta_bench.py, r03)
    const bool want = !(kn.defer_set && kn.defer == 0);
    c.def = (want && (nch_min + 1) / 2 >= kDeferBf16MinChunks) ? 3 : 0;
  } else if (c.family == K4_X3_WIDE && merge && !bf16 && c.pol == 3) {
    int want = kn.defer_set ? kn.defer : 0;  // measured slower so far (register pressure): opt-in
    if (want == 1 && nch_min < k4_defer_min_chunks(1)) want = 2;
    if (want == 2 && nch_min < k4_defer_min_chunks(2)) want = 0;
    c.def = (want == 1 || want == 2) ? want : 0;
  }
  HDP_K4_CHECK(k4_choice_valid(c), "hdp_delta_plan_create: no kernel instance for family %d mode %d dtype %d", c.family,
               mode, dst_dtype);

  p.tile_rows = (c.family == K4_X3_WIDE || h2) ? 2 * kDT : kDT;
  p.start.assign(n + 1, 0);
  for (int i = 0; i < n; ++i) p.start[i + 1] = p.start[i] + k4_args_tiles(p.args[i], p.tile_rows);
  p.total = p.start[n];
  p.fused = h2 && !p.multiseg && merge;

  // x3: panels of 16 k per (chunk, row or column block) -- L [chunk][nRB], then R [chunk][nCB]; H2: the
  // chunk count padded to even, a pack thread per PAIR of chunks, and the scale tables
  p.off.assign(n, K4ItemOff{0, 0, 0});
  if (x3) {
    const int64_t panel = h2 ? kPanelH : kPanel;
    int64_t sblocks = 0;
    p.pstart.assign(n + 1, 0);
    if (h2) p.sstart.assign(n + 1, 0);
    for (int i = 0; i < n; ++i) {
      const DeltaArgs& a = p.args[i];
      const int64_t nch = k4_chunks(a.r, a.nseg, h2);
      const int64_t nRB = (a.out + kDT - 1) / kDT, nCB = (a.in + kDT - 1) / kDT;
      p.off[i].limg = p.img_elems;
      p.off[i].rimg = p.img_elems + nch * nRB * panel;
      p.img_elems += nch * (nRB + nCB) * panel;
      const int64_t th = (h2 ? nch / 2 : nch) * (nRB + nCB) * kDT;
      p.pstart[i + 1] = p.pstart[i] + (th + 255) / 256 * 256;
      p.pack_bytes += (h2 ? 24.0 : 20.0) * a.r * a.nseg * (double)(a.out + a.in);
      if (h2) {
        p.off[i].ktab = p.ktab_floats;
        p.ktab_floats += (h2_tab_floats(a.out, a.in, a.r, a.nseg) + 63) / 64 * 64;
        sblocks += a.nseg * ((a.out + 255) / 256 + (a.in + 255) / 256);
        HDP_K4_CHECK(sblocks <= INT_MAX, "hdp_delta_plan_create: scale grid too large");
        p.sstart[i + 1] = (int)sblocks;
      }
    }
    p.pack_total = p.pstart[n];
    p.sblocks = (int)sblocks;
  }
  if (p.fused) {
    p.apst.assign(n + 1, 0);
    for (int i = 0; i < n; ++i) {
      const DeltaArgs& a = p.args[i];
      p.adam_bytes += (double)a.r * ((28.0 + 4.0) * a.out + (28.0 + 4.0 + 8.0) * a.in);
      p.apst[i + 1] = p.apst[i] + (h2_ap_threads(a.out, a.in, a.r) + 255) / 256 * 256;
    }
    p.ap_total = p.apst[n];
  }
  // the launches narrow these to 32 bits
  HDP_K4_CHECK(p.total <= INT_MAX, "hdp_delta_plan_create: grid too large (%lld tiles)", (long long)p.total);
  HDP_K4_CHECK(p.pack_total / 256 <= INT_MAX, "hdp_delta_plan_create: pack grid too large");
  HDP_K4_CHECK(p.ap_total / 256 <= INT_MAX, "hdp_delta_plan_create: Adam-pack grid too large");
  return K4Error{};
}

}  // namespace hdp
