// Stand-alone check of the K4 host plan (hd-pissa_amd/csrc/hdp_delta_plan.h): built and run by
// tests/test_k4_plan.py with the host compiler, plain and under -fsanitize=address,undefined.
// Exit status 0 and a last line "OK <plans>" mean every property held.
//
// The items carry made-up addresses (suitably aligned, or misaligned on purpose): the planner only does
// arithmetic on pointers and never reads through one.  The panel image and the scale tables are laid out
// from made-up bases the same way hdp_delta_plan_create patches limg / rimg / ktab, and every address a
// consumer kernel forms from (out, in, r, nseg) is held to the planned extents.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "hdp_delta_plan.h"

using namespace hdp;

static int g_fail = 0;
static long g_plans = 0;
static std::string g_case;

#define EXPECT(cond, ...)                                     \
  do {                                                        \
    if (!(cond)) {                                            \
      if (g_fail++ < 30) {                                    \
        std::printf("FAIL [%s] %s: ", g_case.c_str(), #cond); \
        std::printf(__VA_ARGS__);                             \
        std::printf("\n");                                    \
      }                                                       \
    }                                                         \
  } while (0)

struct Shape {
  int64_t out, in;
  int r;
};

static int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
template <class T> static T* fake(uint64_t addr) { return reinterpret_cast<T*>(static_cast<uintptr_t>(addr)); }

// items as the step builds them: per module the delta and factor arenas hold nseg segments back to back
static std::vector<hdp_delta_item> make_items(const std::vector<Shape>& s, int nseg, int dst_es = 4) {
  std::vector<hdp_delta_item> v;
  uint64_t at = 0x100000000ull;
  auto room = [&](int64_t bytes) {
    const uint64_t o = at;
    at += (uint64_t)(bytes + 255) / 256 * 256;
    return o;
  };
  for (const Shape& m : s) {
    hdp_delta_item it;
    it.out = m.out;
    it.in = m.in;
    it.r = m.r;
    it.nseg = nseg;
    const int64_t seg = (int64_t)m.r * (m.out + m.in);
    const int64_t stride = (seg + 3) / 4 * 4;
    it.delta_seg_stride = it.factor_seg_stride = stride;
    const uint64_t d = room(4 * stride * nseg), f = room(4 * stride * nseg);
    it.dA = fake<const float>(d);
    it.dB = fake<const float>(d + 4 * (uint64_t)m.r * m.in);
    it.A = fake<const float>(f);
    it.B = fake<const float>(f + 4 * (uint64_t)m.r * m.in);
    it.dst = fake<void>(room(m.out * m.in * dst_es));
    v.push_back(it);
  }
  return v;
}

static bool same_plan(const K4Plan& a, const K4Plan& b) {
  auto veq = [](const auto& x, const auto& y) {
    return x.size() == y.size() && (x.empty() || std::memcmp(x.data(), y.data(), x.size() * sizeof(x[0])) == 0);
  };
  return std::memcmp(&a.choice, &b.choice, sizeof(K4Choice)) == 0 && a.tile_rows == b.tile_rows &&
         a.multiseg == b.multiseg && a.fused == b.fused && a.total == b.total && a.img_elems == b.img_elems &&
         a.ktab_floats == b.ktab_floats && a.pack_total == b.pack_total && a.ap_total == b.ap_total &&
         a.sblocks == b.sblocks && a.bytes == b.bytes && a.flops == b.flops && a.pack_bytes == b.pack_bytes &&
         a.adam_bytes == b.adam_bytes && veq(a.args, b.args) && veq(a.off, b.off) && veq(a.start, b.start) &&
         veq(a.pstart, b.pstart) && veq(a.sstart, b.sstart) && veq(a.apst, b.apst);
}

// the panel image against its consumers: k4_pack_kernel / MX3P::load / the wide kernel (x3), k4_h2_pack_kernel /
// k4_h2_adam_pack_kernel / delta_h2_kernel (H2) all address panel (c, blk) of a side at
// base + (c * nB + blk) * panel, c below the (H2: even-padded) chunk count
static void check_image(const K4Plan& p, const std::vector<hdp_delta_item>& items, bool h2) {
  const uint64_t kImg = 0x7000000000ull;  // 16-B aligned, as hipMalloc returns
  const int64_t panel = h2 ? 2 * 128 * 16 : 3 * 128 * 16;
  int64_t sum = 0, prev_end = 0;
  for (size_t i = 0; i < items.size(); ++i) {
    const hdp_delta_item& it = items[i];
    int64_t nch = (int64_t)it.nseg * cdiv(it.r, 8);
    if (h2) nch += nch & 1;
    const int64_t nRB = cdiv(it.out, 128), nCB = cdiv(it.in, 128);
    const int64_t lext = nch * nRB * panel, rext = nch * nCB * panel;
    const int64_t lb = p.off[i].limg, rb = p.off[i].rimg;
    EXPECT(lb == prev_end && rb == lb + lext, "item %zu: L at %lld, R at %lld, previous end %lld", i, (long long)lb,
           (long long)rb, (long long)prev_end);  // L, R and the items: back to back, so disjoint
    EXPECT((kImg + 2 * (uint64_t)lb) % 16 == 0 && (kImg + 2 * (uint64_t)rb) % 16 == 0, "item %zu: base alignment", i);
    for (int64_t c = 0; c < nch; ++c) {
      for (int64_t blk = 0; blk < nRB; ++blk) {
        const int64_t a = lb + (c * nRB + blk) * panel;
        EXPECT(a >= lb && a + panel <= lb + lext, "item %zu: L panel (%lld, %lld)", i, (long long)c, (long long)blk);
      }
      for (int64_t blk = 0; blk < nCB; ++blk) {
        const int64_t a = rb + (c * nCB + blk) * panel;
        EXPECT(a >= rb && a + panel <= rb + rext, "item %zu: R panel (%lld, %lld)", i, (long long)c, (long long)blk);
      }
    }
    prev_end = rb + rext;
    sum += lext + rext;
  }
  EXPECT(sum == p.img_elems, "extents %lld, img_elems %lld", (long long)sum, (long long)p.img_elems);
}

struct Input {
  std::vector<Shape> shapes;
  int nseg;
  std::vector<hdp_delta_item> items;
  K4Plan first[2];  // the first plan seen without / with H2: its image was walked panel by panel
  bool seen[2] = {false, false};
};

static void check_plan(Input& in, int dtype, int mode, int round, const K4Knobs& kn) {
  const std::vector<hdp_delta_item>& items = in.items;
  const int n = (int)items.size();
  K4Plan p;
  const K4Error e = k4_plan(items.data(), n, dtype, mode, round, kn, p);
  ++g_plans;
  EXPECT(e.code == HDP_OK, "refused: %s", e.msg);
  if (e.code != HDP_OK) return;
  const K4Choice& c = p.choice;
  const bool merge = mode == HDP_DW_MERGE, bf16 = dtype == HDP_BF16;
  const bool h2 = c.family == K4_H2, x3 = c.family != K4_F32;
  bool multiseg = false, even = true;
  int64_t kmax = 0, nch_min = INT64_MAX;
  for (const hdp_delta_item& it : items) {
    multiseg |= it.nseg > 1;
    even = even && cdiv(it.r, 8) % 2 == 0;
    kmax = std::max<int64_t>(kmax, 2ll * it.r * it.nseg);
    nch_min = std::min<int64_t>(nch_min, (int64_t)it.nseg * cdiv(it.r, 8));
  }

  // ---- the choice
  EXPECT(k4_choice_valid(c), "family %d mode %d dtype %d round %d pol %d def %d", c.family, c.mode, c.dtype, c.round,
         c.pol, c.def);
  EXPECT(c.mode == mode && c.dtype == dtype, "mode / dtype");
  EXPECT(p.h2() == h2 && p.x3() == x3, "family predicates");
  EXPECT((p.tile_rows == 256) == (c.family == K4_X3_WIDE || h2) && (p.tile_rows == 256 || p.tile_rows == 128),
         "tile rows %d for family %d", p.tile_rows, c.family);
  const bool drop_round = merge && bf16 && !multiseg;
  EXPECT(c.round == ((round && !drop_round) ? 1 : 0), "round %d from %d (single-segment bf16 merge: %d)", c.round, round,
         drop_round);
  EXPECT(!(h2 && c.round) || (even && merge && bf16 && !kn.rnd_x3), "H2 with round");
  EXPECT(p.multiseg == (multiseg ? 1 : 0), "multiseg");
  EXPECT(p.fused == ((h2 && !multiseg && merge) ? 1 : 0), "fused %d", p.fused);
  if (c.def) {
    const int64_t have = h2 ? (nch_min + 1) / 2 : nch_min;
    const int need = c.def == 3 ? 4 : c.def == 1 ? 11 : c.def == 2 ? 6 : 7;
    EXPECT(have >= need, "def %d with %lld chunks on some item", c.def, (long long)have);
    EXPECT(!(kn.defer_set && kn.defer == 0), "def %d under HDP_K4_DEFER=0", c.def);
  }
  if (merge && !bf16) EXPECT(c.pol == kn.pol || c.pol == 0, "pol %d from %d", c.pol, kn.pol);
  if (merge && !bf16 && !h2) EXPECT(c.pol == kn.pol, "pol %d from %d: every tested policy has an instance", c.pol, kn.pol);
  if (merge && !bf16 && h2) EXPECT(c.pol == (kn.pol == 3 ? 3 : 0), "H2 pol %d from %d", c.pol, kn.pol);
  // the math knob: f32 and x3 are obeyed as given, H2 but for a ROUND plan it cannot fold, AUTO by K
  if (kn.math == HDP_MATH_F32) EXPECT(!x3, "HDP_MATH_F32 took family %d", c.family);
  if (kn.math == HDP_MATH_X3) EXPECT(x3 && !h2, "HDP_MATH_X3 took family %d", c.family);
  if (kn.math == HDP_MATH_H2)
    EXPECT(x3 && h2 == !(c.round && !(merge && bf16 && even && !kn.rnd_x3)), "HDP_MATH_H2 took family %d", c.family);
  if (kn.math == HDP_MATH_AUTO) {
    const bool store_h2 = !merge && !round && kmax >= 32 && !kn.store_f32;
    EXPECT(x3 == (kmax > 32 || store_h2), "AUTO at K = %lld took family %d", (long long)kmax, c.family);
  }
  if (x3 && !h2) {
    const int want = (kn.stage == HDP_X3_WIDE && merge && bf16 && c.round) ? HDP_X3_GLDS : kn.stage;
    EXPECT(c.family == (want == HDP_X3_WIDE ? K4_X3_WIDE : want == HDP_X3_GLDS ? K4_X3_GLDS : K4_X3_REGS),
           "stage %d took family %d", kn.stage, c.family);
  }

  // ---- tiles
  EXPECT((int)p.start.size() == n + 1 && p.start[0] == 0, "tile prefix size");
  for (int i = 0; i < n; ++i)
    EXPECT(p.start[i + 1] - p.start[i] == cdiv(items[i].out, p.tile_rows) * cdiv(items[i].in, 128), "tiles of item %d", i);
  EXPECT(p.total == p.start[n], "total");

  // ---- descriptors: the caller's operands, image and table pointers still null
  EXPECT((int)p.args.size() == n && (int)p.off.size() == n, "sizes");
  for (int i = 0; i < n; ++i) {
    const DeltaArgs& a = p.args[i];
    const hdp_delta_item& it = items[i];
    EXPECT(a.out == it.out && a.in == it.in && a.r == it.r && a.nseg == it.nseg && a.dA == it.dA && a.dB == it.dB &&
               a.A == it.A && a.B == it.B && a.dst == it.dst && a.dstr == it.delta_seg_stride &&
               a.fstr == it.factor_seg_stride && !a.limg && !a.rimg && !a.ktab,
           "descriptor %d", i);
  }

  // ---- panel image and pack thread space
  if (!x3) {
    EXPECT(p.img_elems == 0 && p.pack_total == 0 && p.pstart.empty() && p.ktab_floats == 0, "f32 plan with an image");
  } else {
    if (!in.seen[h2]) {
      check_image(p, items, h2);
      in.first[h2] = p;
      in.seen[h2] = true;
    } else {  // the layout depends on the shapes and on H2 alone
      const K4Plan& f = in.first[h2];
      EXPECT(p.img_elems == f.img_elems && std::memcmp(p.off.data(), f.off.data(), n * sizeof(K4ItemOff)) == 0,
             "image layout differs between two plans of the same shapes");
    }
    EXPECT((int)p.pstart.size() == n + 1 && p.pstart[0] == 0, "pack prefix size");
    for (int i = 0; i < n; ++i) {
      const hdp_delta_item& it = items[i];
      int64_t nch = (int64_t)it.nseg * cdiv(it.r, 8);
      if (h2) nch = (nch + 1) / 2;  // a thread per pair of chunks
      const int64_t th = nch * (cdiv(it.out, 128) + cdiv(it.in, 128)) * 128;  // nL + nR
      const int64_t span = p.pstart[i + 1] - p.pstart[i];
      EXPECT(p.pstart[i] % 256 == 0 && span >= th && span < th + 256, "pack span %lld for %lld threads", (long long)span,
             (long long)th);
    }
    EXPECT(p.pack_total == p.pstart[n] && p.pack_total % 256 == 0, "pack total");
  }

  // ---- scale tables and the scale kernel's workgroups (H2)
  if (!h2) {
    EXPECT(p.ktab_floats == 0 && p.sblocks == 0 && p.sstart.empty(), "scale tables without H2");
  } else {
    int64_t end = 0;
    EXPECT((int)p.sstart.size() == n + 1 && p.sstart[0] == 0, "scale prefix size");
    for (int i = 0; i < n; ++i) {
      const hdp_delta_item& it = items[i];
      const int64_t K = 2ll * it.r * it.nseg;
      const int64_t partials = (int64_t)it.nseg * (cdiv(it.out, 256) + cdiv(it.in, 256)) * 2 * it.r;
      const int64_t tab = h2_tab_floats(it.out, it.in, it.r, it.nseg);
      EXPECT(p.off[i].ktab == end && end % 64 == 0, "table %d at %lld", i, (long long)p.off[i].ktab);
      EXPECT(4 + 2 * K + partials <= tab, "table %d: scales and partials", i);
      EXPECT(h2_cmax_off(it.out, it.in, it.r, it.nseg) == 4 + 2 * K + partials, "table %d: constant maxima offset", i);
      EXPECT(h2_cmax_off(it.out, it.in, it.r, it.nseg) + 2 * it.r <= tab, "table %d: constant maxima", i);
      // k4_h2_bound_kernel passes nseg = 1, k4_h2_cmax_kernel a.nseg: one place on fused plans
      if (p.fused) EXPECT(h2_cmax_off(it.out, it.in, it.r, 1) == h2_cmax_off(it.out, it.in, it.r, it.nseg), "cmax %d", i);
      end += cdiv(tab, 64) * 64;
      EXPECT(p.sstart[i + 1] - p.sstart[i] == it.nseg * (cdiv(it.out, 256) + cdiv(it.in, 256)), "scale blocks %d", i);
    }
    EXPECT(end == p.ktab_floats, "ktab_floats");
    EXPECT(p.sblocks == p.sstart[n], "sblocks");
  }

  // ---- fused Adam + pack thread space
  if (!p.fused) {
    EXPECT(p.ap_total == 0 && p.apst.empty(), "Adam-pack space without fused");
  } else {
    EXPECT((int)p.apst.size() == n + 1 && p.apst[0] == 0, "Adam-pack prefix size");
    for (int i = 0; i < n; ++i) {
      const hdp_delta_item& it = items[i];
      const int64_t per = it.r % 8 == 0 ? it.r / 8 : cdiv(it.r, 4);
      const int64_t th = it.out * per + cdiv(it.in, 4) * per;
      EXPECT(h2_ap_threads(it.out, it.in, it.r) == th, "h2_ap_threads %d", i);
      const int64_t span = p.apst[i + 1] - p.apst[i];
      EXPECT(p.apst[i] % 256 == 0 && span >= th && span < th + 256, "Adam-pack span %d", i);
    }
    EXPECT(p.ap_total == p.apst[n] && p.ap_total % 256 == 0, "Adam-pack total");
  }

  // ---- planning twice gives identical bytes
  K4Plan q;
  k4_plan(items.data(), n, dtype, mode, round, kn, q);
  EXPECT(same_plan(p, q), "second plan differs");
}

static const int kPols[] = {0, 1, 2, 3, 4, 7, 11, 15};
static const int kDefers[] = {-1, 0, 1, 2, 3, 4};  // -1: unset
static const int kMaths[] = {HDP_MATH_AUTO, HDP_MATH_F32, HDP_MATH_X3, HDP_MATH_H2};
static const int kStages[] = {HDP_X3_REGS, HDP_X3_GLDS, HDP_X3_WIDE};

// one input under every knob combination; modes < 0: every valid (dtype, mode, round), else that one
static void sweep(Input& in, const char* name, int only = -1) {
  static const int kModes[5][3] = {{HDP_F32, HDP_DW_MERGE, 0},
                                   {HDP_BF16, HDP_DW_MERGE, 0},
                                   {HDP_BF16, HDP_DW_MERGE, 1},
                                   {HDP_F32, HDP_DW_STORE, 0},
                                   {HDP_F32, HDP_DW_STORE, 1}};
  for (int m = 0; m < 5; ++m) {
    if (only >= 0 && m != only) continue;
    in.items = make_items(in.shapes, in.nseg, kModes[m][0] == HDP_BF16 ? 2 : 4);
    for (int math : kMaths)
      for (int stage : kStages)
        for (int defer : kDefers)
          for (int sf = 0; sf < 2; ++sf)
            for (int rx = 0; rx < 2; ++rx)
              for (int pol : kPols) {
                K4Knobs kn;
                kn.math = math;
                kn.stage = stage;
                kn.defer_set = defer >= 0;
                kn.defer = std::max(defer, 0);
                kn.store_f32 = sf != 0;
                kn.rnd_x3 = rx != 0;
                kn.pol = pol;
                char buf[200];
                std::snprintf(buf, sizeof(buf), "%s nseg %d dtype %d mode %d round %d | math %d stage %d defer %d store_f32 %d rnd_x3 %d pol %d",
                              name, in.nseg, kModes[m][0], kModes[m][1], kModes[m][2], math, stage, defer, sf, rx, pol);
                g_case = buf;
                check_plan(in, kModes[m][0], kModes[m][1], kModes[m][2], kn);
              }
  }
}

static void check_vec_flags() {
  g_case = "vec flags";
  const uint64_t base = 0x200000000ull;
  struct Case {
    int64_t in;
    int r, nseg;
    uint64_t mis_dA, mis_dB, mis_A, mis_B;  // byte offsets off a 16-B boundary
    int64_t dstr, fstr;
    int vec_l, vec_r;
  };
  const Case cases[] = {
      {320, 16, 1, 0, 0, 0, 0, 0, 0, 1, 1},        // aligned, single segment: the strides do not matter
      {320, 16, 2, 0, 0, 0, 0, 8192, 8192, 1, 1},  // aligned
      {320, 16, 1, 4, 0, 0, 0, 0, 0, 1, 0},        // dA misaligned: R
      {320, 16, 1, 0, 0, 8, 0, 0, 0, 1, 0},        // A misaligned: R
      {320, 16, 1, 0, 4, 0, 0, 0, 0, 0, 1},        // dB misaligned: L
      {320, 16, 1, 0, 0, 0, 12, 0, 0, 0, 1},       // B misaligned: L
      {320, 16, 2, 0, 0, 0, 0, 8194, 8192, 0, 0},  // a delta stride that is no multiple of 4: both
      {320, 16, 2, 0, 0, 0, 0, 8192, 8190, 0, 0},  // a factor stride
      {320, 18, 1, 0, 0, 0, 0, 0, 0, 0, 1},        // r % 4 != 0: L
      {322, 16, 1, 0, 0, 0, 0, 0, 0, 1, 0},        // in % 4 != 0: R
      {322, 18, 1, 0, 0, 0, 0, 0, 0, 0, 0},
  };
  for (const Case& c : cases) {
    DeltaArgs a;
    const K4Error e = k4_make_args("t", 200, c.in, c.r, c.nseg, fake<const float>(base + c.mis_dA),
                                   fake<const float>(base + 0x100000 + c.mis_dB), c.dstr,
                                   fake<const float>(base + 0x200000 + c.mis_A),
                                   fake<const float>(base + 0x300000 + c.mis_B), c.fstr, fake<void>(base + 0x400000),
                                   HDP_F32, HDP_DW_MERGE, 0, a);
    EXPECT(e.code == HDP_OK, "%s", e.msg);
    EXPECT(a.vec_l == c.vec_l && a.vec_r == c.vec_r, "in %lld r %d nseg %d: vec_l %d vec_r %d", (long long)c.in, c.r, c.nseg,
           a.vec_l, a.vec_r);
  }
}

static void check_refusals() {
  g_case = "refusals";
  const float* P = fake<const float>(0x300000000ull);
  void* D = fake<void>(0x310000000ull);
  DeltaArgs a;
  auto refused = [&](const char* what, const K4Error& e, const char* text) {
    EXPECT(e.code == HDP_EINVAL && std::strstr(e.msg, text), "%s: code %d, \"%s\"", what, e.code, e.msg);
  };
  auto mk = [&](int64_t out, int64_t in, int r, int nseg, const float* dA, const float* dB, int64_t ds, const float* A,
                const float* B, int64_t fs, void* dst, int dt, int mode, int rnd) {
    return k4_make_args("who", out, in, r, nseg, dA, dB, ds, A, B, fs, dst, dt, mode, rnd, a);
  };
  refused("out", mk(0, 8, 4, 1, P, P, 0, P, P, 0, D, HDP_F32, HDP_DW_MERGE, 0), "who: bad shape");
  refused("r", mk(8, 8, 0, 1, P, P, 0, P, P, 0, D, HDP_F32, HDP_DW_MERGE, 0), "bad shape");
  refused("nseg", mk(8, 8, 4, 0, P, P, 0, P, P, 0, D, HDP_F32, HDP_DW_MERGE, 0), "bad shape");
  refused("dA", mk(8, 8, 4, 1, nullptr, P, 0, P, P, 0, D, HDP_F32, HDP_DW_MERGE, 0), "null pointer");
  refused("dB", mk(8, 8, 4, 1, P, nullptr, 0, P, P, 0, D, HDP_F32, HDP_DW_MERGE, 0), "null pointer");
  refused("A", mk(8, 8, 4, 1, P, P, 0, nullptr, P, 0, D, HDP_F32, HDP_DW_MERGE, 0), "null pointer");
  refused("B", mk(8, 8, 4, 1, P, P, 0, P, nullptr, 0, D, HDP_F32, HDP_DW_MERGE, 0), "null pointer");
  refused("dst", mk(8, 8, 4, 1, P, P, 0, P, P, 0, nullptr, HDP_F32, HDP_DW_MERGE, 0), "null pointer");
  refused("mode", mk(8, 8, 4, 1, P, P, 0, P, P, 0, D, HDP_F32, 2, 0), "bad mode 2");
  refused("dtype", mk(8, 8, 4, 1, P, P, 0, P, P, 0, D, 2, HDP_DW_MERGE, 0), "bad dtype 2");
  refused("store bf16", mk(8, 8, 4, 1, P, P, 0, P, P, 0, D, HDP_BF16, HDP_DW_STORE, 0), "STORE mode writes float32");
  refused("round f32 merge", mk(8, 8, 4, 1, P, P, 0, P, P, 0, D, HDP_F32, HDP_DW_MERGE, 1), "round_bf16 applies to bf16");
  refused("delta stride", mk(8, 8, 4, 2, P, P, 0, P, P, 64, D, HDP_F32, HDP_DW_MERGE, 0), "segment strides must be positive");
  refused("factor stride", mk(8, 8, 4, 2, P, P, 64, P, P, -64, D, HDP_F32, HDP_DW_MERGE, 0), "segment strides");
  // 31-bit byte offsets into one module's dst: 2^29 float32 / STORE elements, 2^30 bf16 MERGE elements
  const int64_t f32_lim = (int64_t)1 << 29, bf_lim = (int64_t)1 << 30;
  EXPECT(mk(1, f32_lim - 1, 4, 1, P, P, 0, P, P, 0, D, HDP_F32, HDP_DW_MERGE, 0).code == HDP_OK, "f32 below the limit");
  refused("f32 at the limit", mk(1, f32_lim, 4, 1, P, P, 0, P, P, 0, D, HDP_F32, HDP_DW_MERGE, 0), "matrix too large");
  refused("f32 at the limit", mk(1 << 15, 1 << 14, 4, 1, P, P, 0, P, P, 0, D, HDP_F32, HDP_DW_STORE, 0), "matrix too large");
  EXPECT(mk(bf_lim - 1, 1, 4, 1, P, P, 0, P, P, 0, D, HDP_BF16, HDP_DW_MERGE, 0).code == HDP_OK, "bf16 below the limit");
  refused("bf16 at the limit", mk(bf_lim, 1, 4, 1, P, P, 0, P, P, 0, D, HDP_BF16, HDP_DW_MERGE, 0), "matrix too large");
  refused("overflowing product", mk((int64_t)1 << 40, (int64_t)1 << 40, 4, 1, P, P, 0, P, P, 0, D, HDP_F32, HDP_DW_MERGE, 0),
          "matrix too large");

  // the plan: its items' refusals, and the counts a launch narrows to 32 bits
  K4Plan p;
  K4Knobs kn;
  hdp_delta_item it{8, 8, 4, 1, P, P, 0, P, P, 0, D};
  refused("n = 0", k4_plan(&it, 0, HDP_F32, HDP_DW_MERGE, 0, kn, p), "n > 0 items");
  refused("no items", k4_plan(nullptr, 1, HDP_F32, HDP_DW_MERGE, 0, kn, p), "n > 0 items");
  hdp_delta_item two[2] = {it, it};
  two[1].B = nullptr;
  refused("second item", k4_plan(two, 2, HDP_F32, HDP_DW_MERGE, 0, kn, p), "hdp_delta_plan_create: null pointer");
  {  // tiles: 1025 items of 2^21 tiles of 128 rows
    std::vector<hdp_delta_item> many(1025, hdp_delta_item{(int64_t)1 << 28, 1, 4, 1, P, P, 0, P, P, 0, D});
    kn.math = HDP_MATH_F32;
    refused("tiles", k4_plan(many.data(), 1025, HDP_F32, HDP_DW_MERGE, 0, kn, p), "grid too large");
    EXPECT(k4_plan(many.data(), 1023, HDP_F32, HDP_DW_MERGE, 0, kn, p).code == HDP_OK, "1023 x 2^21 tiles fit");
  }
  {  // pack threads: 2^17 chunks x 2^21 row blocks x 128
    hdp_delta_item big{(int64_t)1 << 28, 1, 1 << 20, 1, P, P, 0, P, P, 0, D};
    kn.math = HDP_MATH_X3;
    refused("pack grid", k4_plan(&big, 1, HDP_F32, HDP_DW_MERGE, 0, kn, p), "pack grid too large");
  }
  {  // scale workgroups: 2^12 segments x 2^20 blocks of 256 rows
    hdp_delta_item big{(int64_t)1 << 28, 1, 16, 1 << 12, P, P, 1 << 20, P, P, 1 << 20, D};
    kn.math = HDP_MATH_H2;
    refused("scale grid", k4_plan(&big, 1, HDP_F32, HDP_DW_MERGE, 0, kn, p), "scale grid too large");
  }
  {  // Adam-pack threads alone: 24 items of out x r / 8 = 2^28 x 2^7 (their pack threads: 24 x 2^6 x 2^21 x 128 < 2^39)
    std::vector<hdp_delta_item> big(24, hdp_delta_item{(int64_t)1 << 28, 1, 1 << 10, 1, P, P, 0, P, P, 0, D});
    kn.math = HDP_MATH_H2;
    refused("Adam-pack grid", k4_plan(big.data(), 24, HDP_F32, HDP_DW_MERGE, 0, kn, p), "Adam-pack grid too large");
    EXPECT(k4_plan(big.data(), 1, HDP_F32, HDP_DW_MERGE, 0, kn, p).code == HDP_OK && p.fused, "one such item fits");
  }
}

int main() {
  std::vector<Input> inputs;
  std::vector<std::string> names;
  auto add = [&](const char* name, std::vector<Shape> s, int nseg) {
    Input in;
    in.shapes = std::move(s);
    in.nseg = nseg;
    inputs.push_back(std::move(in));
    names.push_back(name);
  };
  auto layer = [](int64_t h, int64_t kv, int64_t ffn, int r) {  // q k v o gate up down
    return std::vector<Shape>{{h, h, r}, {kv, h, r}, {kv, h, r}, {h, h, r}, {ffn, h, r}, {ffn, h, r}, {h, ffn, r}};
  };
  for (int nseg : {1, 2, 4, 8}) {
    add("llama2-7b r16", layer(4096, 4096, 11008, 16), nseg);
    add("mistral-7b r64", layer(4096, 1024, 14336, 64), nseg);
    add("llama2-13b r128", layer(5120, 5120, 13824, 128), nseg);
    for (int r : {1, 4, 20, 100, 128})
      add("ragged", {{200, 320, r}, {384, 250, r}, {75, 130, r}, {128, 192, r}}, nseg);
    add("mixed r", {{200, 320, 16}, {384, 250, 100}, {75, 130, 1}, {128, 192, 128}, {64, 333, 20}}, nseg);
    // shard exchange: a rank's row block of W (8 and 16 rows), and a 1-row item
    add("shard rows", {{8, 4096, 16}, {16, 4096, 16}, {16, 11008, 16}, {8, 250, 20}}, nseg);
    add("one row", {{1, 130, 4}}, nseg);
    add("one row wide r", {{1, 4096, 64}, {4096, 1, 64}}, nseg);
  }
  const size_t fixed = inputs.size();
  std::mt19937 rng(20240611);
  auto pick = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };
  for (int t = 0; t < 300; ++t) {
    std::vector<Shape> s(pick(1, 12));
    for (Shape& m : s) {
      m.out = pick(1, 5) == 1 ? pick(1, 40) : pick(1, 1500);
      m.in = pick(1, 5) == 1 ? pick(1, 40) : pick(1, 1500);
      m.r = pick(1, 4) == 1 ? 8 * pick(1, 16) : pick(1, 130);
    }
    static const int kSeg[] = {1, 1, 2, 3, 4, 8};
    add("random", std::move(s), kSeg[pick(0, 5)]);
  }
  // every (dtype, mode, round) for the fixed inputs; one of the five, in turn, per random plan
  for (size_t i = 0; i < inputs.size(); ++i) sweep(inputs[i], names[i].c_str(), i < fixed ? -1 : (int)(i % 5));
  check_vec_flags();
  check_refusals();
  if (g_fail) {
    std::printf("%d checks failed\n", g_fail);
    return 1;
  }
  std::printf("OK %ld plans\n", g_plans);
  return 0;
}
