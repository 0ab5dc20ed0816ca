// Stand-alone check of the K2 sweep's host plan (hd-pissa_amd/csrc/hdp_sweep_plan.h): built and run by
// tests/test_sweep_plan.py with the host compiler, plain and under -fsanitize=address,undefined.
// Exit status 0 and a last line "OK <plans>" mean every property held.
//
// Groups are carved from a real host buffer the way hdp_probe_grads_group carves the device workspace
// (tables first, then the modules' work areas), and the tensors from a second one, so every pointer the
// planner computes stays inside an object.  Neither buffer is ever read or written: the planner only does
// arithmetic on the pointers.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <random>
#include <vector>

#include "hdp_sweep_plan.h"

using namespace hdp;

static int g_fail = 0;
static const char* g_case = "";

#define EXPECT(cond, ...)                             \
  do {                                                \
    if (!(cond)) {                                    \
      if (g_fail++ < 30) {                            \
        std::printf("FAIL [%s] %s: ", g_case, #cond); \
        std::printf(__VA_ARGS__);                     \
        std::printf("\n");                            \
      }                                               \
    }                                                 \
  } while (0)

// one module as a caller would pass it; xid: modules with the same xid read the same X tensor
struct Mod {
  int64_t T, in, out;
  int r, b_t, xid, accumulate;
};

struct Group {
  HostGroup ga;
  std::vector<ModPlan> plan;
  std::vector<char*> area;  // every module's work area
  size_t tab_bytes = 0, ws_bytes = 0, query_bytes = 0;
  std::unique_ptr<char[]> ws_mem, tensor_mem;
  char* ws = nullptr;
};

static char* align_up(char* p, size_t a) {
  return reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(p) + a - 1) / a * a);
}

// r_total > 0: the modules are r-slices of one module of that rank (two per Mod: rows [0, r) and [r, 2r))
static void build(Group& g, const std::vector<Mod>& mods, int RB, int r_total = 0) {
  const int nm = (int)mods.size();
  // tensors: X per xid, G, A, B, gA, gB per module (float32 sizes: bf16 activations fit as well)
  size_t tb = 256;
  auto room = [&](size_t floats) { size_t o = tb; tb += (floats * 4 + 15) / 16 * 16; return o; };
  std::map<int, size_t> xoff;
  std::vector<size_t> oG(nm), oA(nm), oB(nm), ogA(nm), ogB(nm), oX(nm);
  for (int i = 0; i < nm; ++i) {
    const Mod& m = mods[i];
    const int rt = r_total ? r_total : m.r;
    if (!xoff.count(m.xid)) xoff[m.xid] = room((size_t)m.T * m.in);
    oX[i] = xoff[m.xid];
    oG[i] = room((size_t)m.T * m.out);
    oA[i] = room((size_t)rt * m.in);
    oB[i] = room((size_t)rt * m.out);
    ogA[i] = room((size_t)rt * m.in);
    ogB[i] = room((size_t)rt * m.out);
  }
  g.tensor_mem.reset(new char[tb + 16]);
  char* tp = align_up(g.tensor_mem.get(), 16);
  // the caller's items: a module, or the two r-slices of it
  struct Item {
    Mod m;
    int src, j0, ldb;
    int64_t in, out;
  };
  std::vector<Item> items;
  for (int i = 0; i < nm; ++i) {
    if (r_total) {
      for (int j0 = 0; j0 < r_total; j0 += mods[i].r) items.push_back(Item{mods[i], i, j0, r_total, mods[i].in, mods[i].out});
    } else {
      items.push_back(Item{mods[i], i, 0, mods[i].r, mods[i].in, mods[i].out});
    }
  }
  const int n = (int)items.size();
  g.tab_bytes = sweep_table_bytes(items.data(), n);
  g.plan.resize(n);
  size_t off = g.tab_bytes;
  g.query_bytes = 0;
  for (int i = 0; i < n; ++i) {
    const Mod& m = items[i].m;
    g.plan[i] = plan_sweep_module(m.T, m.in, m.out, m.r);
    off += g.plan[i].area;
    g.query_bytes += g.plan[i].bytes;  // hdp_probe_workspace_bytes of a sweep module (of a sliced one: at least)
  }
  g.ws_bytes = off;
  g.ws_mem.reset(new char[g.ws_bytes + 256]);
  g.ws = align_up(g.ws_mem.get(), 256);
  g.ga = HostGroup{};
  g.ga.RB = RB;
  g.ga.rp = 16 * RB;
  g.area.clear();
  off = g.tab_bytes;
  for (int i = 0; i < n; ++i) {
    const Item& it = items[i];
    const Mod& m = it.m;
    ProbeDesc d{};
    float* A = reinterpret_cast<float*>(tp + oA[it.src]);
    float* B = reinterpret_cast<float*>(tp + oB[it.src]);
    float* gA = reinterpret_cast<float*>(tp + ogA[it.src]);
    float* gB = reinterpret_cast<float*>(tp + ogB[it.src]);
    d.X = tp + oX[it.src];
    d.G = tp + oG[it.src];
    d.A = A + (int64_t)it.j0 * m.in;
    d.B = B + (int64_t)it.j0 * m.out;  // (slices need B^T)
    d.gA = gA + (int64_t)it.j0 * m.in;
    d.gB = gB + it.j0;
    place_module(d, g.plan[i], g.ws + off);
    g.area.push_back(g.ws + off);
    d.T = m.T;
    d.in = m.in;
    d.out = m.out;
    d.scale = 1e-16f * (float)(i + 1);
    d.r = m.r;
    d.b_t = m.b_t;
    d.accumulate = m.accumulate;
    d.ldb = it.ldb;
    off += g.plan[i].area;
    g.ga.d.push_back(d);
  }
  g.ga.n = n;
}

// ---- workspace spans ---------------------------------------------------------------------------
enum Kind { kSlab, kPart, kY };

// [b, b + floats) must lie inside one buffer of the right kind of the module whose area holds b
static void check_span(const Group& g, const void* begin, int64_t floats, Kind kind, const char* what) {
  const char* b = reinterpret_cast<const char*>(begin);
  const int n = g.ga.n;
  int i = (int)(std::upper_bound(g.area.begin(), g.area.end(), const_cast<char*>(b)) - g.area.begin()) - 1;
  EXPECT(i >= 0 && i < n && b < g.area[i] + g.plan[i].area, "%s: pointer outside every module area", what);
  if (i < 0 || i >= n || b >= g.area[i] + g.plan[i].area) return;
  const ModPlan& p = g.plan[i];
  const ProbeDesc& d = g.ga.d[i];
  const size_t T16 = (size_t)((d.T + 15) / 16) * 16, rp = (size_t)g.ga.rp;
  const size_t yrow = g.ga.RB <= 2 ? 64 : 2 * rp;
  const size_t offs[7] = {p.off_slabH, p.off_slabJ, p.off_partA, p.off_partB, p.off_yH, p.off_yJ, p.area};
  const size_t ext[6] = {(size_t)p.ksh * T16 * rp,          (size_t)p.ksj * T16 * rp, (size_t)p.ksh * p.kst * rp * kSwC,
                         (size_t)p.ksj * p.kst * rp * kSwC, T16 * yrow,               T16 * yrow};
  const Kind kinds[6] = {kSlab, kSlab, kPart, kPart, kY, kY};
  const size_t o = (size_t)(b - g.area[i]);
  int k = 0;
  while (k < 5 && o >= offs[k + 1]) ++k;
  EXPECT(kinds[k] == kind, "%s: module %d, buffer %d is not of kind %d", what, i, k, (int)kind);
  EXPECT(offs[k] + ext[k] * 4 <= offs[k + 1], "module %d: buffer %d overruns the next", i, k);
  EXPECT(floats >= 0 && o + (size_t)floats * 4 <= offs[k] + ext[k] * 4,
         "%s: module %d buffer %d: offset %zu + %lld floats past its %zu floats", what, i, k, o - offs[k], (long long)floats,
         ext[k]);
}

// the r-blocks a sweep instance touches of side d in phase ph: the block view in the FUSE phases (A and C of a
// group with sets), the plain fields otherwise
struct Blk {
  const float* slab;
  const float* part;
  const float* g;
  int rows;
};
static std::vector<Blk> blocks_of(const SweepDesc& d, bool fuse_phase, int RB) {
  std::vector<Blk> v;
  if (fuse_phase) {
    for (int b = 0; b < d.nb; ++b) v.push_back(Blk{d.slab_b[b], d.part_b[b], d.gb[b], d.rbr[b]});
  } else {
    for (int b = 0; b < RB; ++b) {
      const int rows = d.r - 16 * b;
      v.push_back(Blk{d.slab_out + 16 * b, d.part_t ? d.part + 16 * b : d.part + (int64_t)16 * b * kSwC,
                      d.part_t ? d.g + 16 * b : d.g + (int64_t)16 * b * d.N, rows < 0 ? 0 : rows > 16 ? 16 : rows});
    }
  }
  return v;
}

struct Expect {
  int nsets = -1;              // < 0: not checked
  std::vector<int> set_sizes;  // sorted
};

static int g_plans = 0;

static void check_plan(const Group& g, bool bf16, const SweepKnobs& kn, const int slots[3], const Expect& ex) {
  const HostGroup& ga = g.ga;
  const int n = ga.n, RB = ga.RB, rp = 16 * RB;
  SweepSides s;
  plan_sweep_sides(ga, bf16, kn, s);
  SweepTables t;
  const SweepError e = plan_sweep_tables(ga, s, slots, t);
  ++g_plans;
  EXPECT(e.code == 0, "plan failed: %s", e.msg ? e.msg : "?");
  if (e.code != 0) return;

  // ---- sets ----
  EXPECT(s.fuse == !s.sets.empty(), "fuse flag");
  EXPECT(s.split_b == (RB >= 4 && bf16), "split_b");
  if (ex.nsets >= 0) {
    EXPECT((int)s.sets.size() == ex.nsets, "%zu sets, expected %d", s.sets.size(), ex.nsets);
    std::vector<int> sz;
    for (const auto& st : s.sets) sz.push_back((int)st.size());
    std::sort(sz.begin(), sz.end());
    EXPECT(sz == ex.set_sizes, "set sizes");
  }
  std::vector<int> in_set(n, -1);
  for (int k = 0; k < (int)s.sets.size(); ++k) {
    const auto& st = s.sets[k];
    EXPECT(st.size() >= 2 && (int)st.size() * RB <= kSwMaxBlk, "set of %zu members at r-block %d", st.size(), RB);
    int64_t outs = 0;
    for (int m : st) {
      EXPECT(in_set[m] < 0, "module %d in two sets", m);
      in_set[m] = k;
      const ProbeDesc &a = ga.d[st[0]], &b = ga.d[m];
      EXPECT(a.X == b.X && a.T == b.T && a.in == b.in && b.b_t, "set member %d does not share its lead's X", m);
      outs += b.out;
    }
    EXPECT(outs >= ga.d[st[0]].in, "set formed although X is the larger side");
  }
  bool v4 = true;
  auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  for (int i = 0; i < n; ++i) {  // (the work areas follow the tables: 16-B aligned for an even n only)
    const ProbeDesc& p = ga.d[i];
    v4 = v4 && p.in % 4 == 0 && p.r % 4 == 0 && p.ldb % 4 == 0 && al16(p.gA) && al16(p.gB) && al16(p.partA) && al16(p.partB);
  }
  EXPECT(s.v4 == v4, "v4 = %d, expected %d", (int)s.v4, (int)v4);

  // ---- the blob: sections 256-byte aligned, disjoint, within the table space ----
  const char* blob = t.blob.data();
  {
    struct Sec {
      size_t o, bytes;
    };
    std::vector<Sec> sec;
    for (int ph = 0; ph < 3; ++ph) sec.push_back(Sec{t.o_sd[ph], sizeof(SweepDesc) * s.sd[ph].size()});
    for (int ph = 0; ph < 3; ++ph) sec.push_back(Sec{t.o_w[ph], sizeof(int) * 4 * t.G[ph]});
    for (int ph = 0; ph < 3; ++ph) sec.push_back(Sec{t.o_b[ph], sizeof(int) * (t.G[ph] + 1)});
    for (int k = 0; k < 2; ++k) sec.push_back(Sec{t.o_y[k], sizeof(YRedDesc) * n});
    sec.push_back(Sec{t.o_f, sizeof(FinDesc) * n});
    sec.push_back(Sec{t.o_j, sizeof(int) * 4 * t.njobs});
    size_t end = 0;
    for (size_t k = 0; k < sec.size(); ++k) {
      EXPECT(sec[k].o % 256 == 0, "section %zu at %zu", k, sec[k].o);
      EXPECT(sec[k].o >= end, "section %zu overlaps the one before", k);
      end = sec[k].o + sec[k].bytes;
    }
    EXPECT(end <= t.blob.size(), "sections end at %zu of %zu", end, t.blob.size());
    EXPECT(t.blob.size() <= sweep_table_bytes(ga.d.data(), n), "blob %zu above the table space %zu", t.blob.size(),
           sweep_table_bytes(ga.d.data(), n));
    EXPECT(sweep_table_bytes(ga.d.data(), n) == g.tab_bytes, "table space of items and of planned modules differ");
    EXPECT(g.ws_bytes <= g.query_bytes, "tables + areas %zu above the workspace query's %zu", g.ws_bytes, g.query_bytes);
  }
  // areas: in order, disjoint, after the tables, inside the workspace
  for (int i = 0; i < n; ++i) {
    EXPECT(g.area[i] >= g.ws + g.tab_bytes, "area %d inside the tables", i);
    EXPECT(i + 1 == n ? g.area[i] + g.plan[i].area <= g.ws + g.ws_bytes : g.area[i] + g.plan[i].area <= g.area[i + 1],
           "area %d overlaps", i);
  }

  // ---- ranges, start tables ----
  for (int ph = 0; ph < 3; ++ph) {
    const std::vector<int64_t>& b = t.bounds[ph];
    const int G = t.G[ph];
    const std::vector<SweepDesc>& sd = s.sd[ph];
    EXPECT(G >= 1 && G <= slots[ph] && G <= 4096, "phase %d: G = %d of %d", ph, G, slots[ph]);
    EXPECT((int)b.size() == G + 1 && b[0] == 0 && b[G] == s.U[ph], "phase %d: bounds", ph);
    if ((int)b.size() != G + 1) return;
    int64_t U = 0;
    for (const SweepDesc& d : sd) {
      EXPECT(d.pre == U, "phase %d: pre %lld, expected %lld", ph, (long long)d.pre, (long long)U);
      U += (int64_t)d.nct * d.S;
    }
    EXPECT(U == s.U[ph], "phase %d: U", ph);
    EXPECT(memcmp(blob + t.o_sd[ph], sd.data(), sizeof(SweepDesc) * sd.size()) == 0, "phase %d: descriptors in the blob", ph);
    const int* wst = reinterpret_cast<const int*>(blob + t.o_w[ph]);
    const int* bnd = reinterpret_cast<const int*>(blob + t.o_b[ph]);
    EXPECT(bnd[G] == b[G], "phase %d: last boundary", ph);
    for (int w = 0; w < G; ++w) {
      EXPECT(b[w + 1] >= b[w], "phase %d: bounds decrease at %d", ph, w);
      EXPECT(b[w + 1] - b[w] >= kSwMinSteps || G == 1, "phase %d: range %d has %lld steps", ph, w, (long long)(b[w + 1] - b[w]));
      EXPECT(bnd[w] == b[w], "phase %d: boundary %d in the blob", ph, w);
      const int m = wst[4 * w], ct = wst[4 * w + 1], st = wst[4 * w + 2], pc = wst[4 * w + 3];
      EXPECT(m >= 0 && m < (int)sd.size(), "phase %d wg %d: side %d", ph, w, m);
      if (m < 0 || m >= (int)sd.size()) continue;
      EXPECT(ct >= 0 && ct < sd[m].nct && st >= 0 && st < sd[m].S, "phase %d wg %d: stripe %d step %d", ph, w, ct, st);
      EXPECT(sd[m].pre + (int64_t)ct * sd[m].S + st == b[w], "phase %d wg %d: start is not its boundary", ph, w);
      const int64_t u0 = sd[m].pre + (int64_t)ct * sd[m].S;  // earlier workgroups on this stripe
      int before = 0;
      for (int v = w - 1; v >= 0 && b[v + 1] > u0; --v) ++before;
      EXPECT(pc == before, "phase %d wg %d: piece %d, %d workgroups before it on the stripe", ph, w, pc, before);
    }
  }

  // ---- coverage: every r-block of every module side projected once and OUTER-ed once ----
  std::map<const float*, int> slab_key, part_key;  // pointer of block bb -> (module * 2 + side) * 8 + bb
  for (int i = 0; i < n; ++i)
    for (int bb = 0; bb < RB; ++bb) {
      const ProbeDesc& p = ga.d[i];
      slab_key[p.slabH + 16 * bb] = (i * 2 + 0) * 8 + bb;
      slab_key[p.slabJ + 16 * bb] = (i * 2 + 1) * 8 + bb;
      part_key[p.partA + (int64_t)16 * bb * kSwC] = (i * 2 + 0) * 8 + bb;
      part_key[p.partB + 16 * bb] = (i * 2 + 1) * 8 + bb;
    }
  EXPECT((int)slab_key.size() == 2 * n * RB && (int)part_key.size() == 2 * n * RB, "block pointers collide");
  std::vector<int> nproj(2 * n * 8, 0), nouter(2 * n * 8, 0);
  for (int ph = 0; ph < 3; ++ph) {
    const bool proj = ph == 0 || ph == 1, outer = ph == 2 || (ph == 1 && !s.split_b);
    const bool fuse_phase = s.fuse && ph != 1;
    for (const SweepDesc& d : s.sd[ph]) {
      const int64_t T16 = (d.T + 15) / 16 * 16;
      EXPECT(d.S == (int)(T16 / 16) && d.nct == (int)((d.N + kSwC - 1) / kSwC), "side geometry");
      EXPECT(d.kmax == sweep_kmax(d.T), "kmax");
      EXPECT(fuse_phase ? d.nb >= 1 && d.nb <= kSwMaxBlk : d.nb == RB, "nb = %d", d.nb);
      const std::vector<Blk> blk = blocks_of(d, fuse_phase, RB);
      int rows = 0, rsum = 0;
      std::vector<int> owners;
      for (const Blk& b : blk) {
        rows += b.rows;
        const auto ks = slab_key.find(b.slab);
        const auto kp = part_key.find(b.part);
        EXPECT(ks != slab_key.end() && kp != part_key.end() && ks->second == kp->second,
               "phase %d: a block's slab and pieces belong to different module sides", ph);
        if (ks == slab_key.end()) continue;
        const int key = ks->second, i = key / 16, side = (key / 8) & 1, bb = key % 8;
        const ProbeDesc& p = ga.d[i];
        EXPECT((side == 0) == (d.part_t == 0), "side of the block's owner");
        EXPECT((side == 0 ? (const void*)p.X : p.G) == d.Z && (side == 0 ? p.in : p.out) == d.N && p.T == d.T,
               "phase %d: module %d does not read this stream", ph, i);
        const int want = p.r - 16 * bb < 0 ? 0 : p.r - 16 * bb > 16 ? 16 : p.r - 16 * bb;
        EXPECT(b.rows == want, "phase %d: module %d block %d has %d rows, expected %d", ph, i, bb, b.rows, want);
        EXPECT(b.g == (side == 0 ? p.gA + (int64_t)16 * bb * p.in : p.gB + 16 * bb), "gradient rows of module %d block %d", i, bb);
        if (proj) ++nproj[key];
        if (outer) ++nouter[key];
        if (bb == 0) {
          owners.push_back(i);
          rsum += p.r;
        }
        // the block's module buffers, with the extents the kernels use
        if (proj) check_span(g, b.slab - 16 * bb, (int64_t)d.nct * T16 * rp, kSlab, "slab");
        if (outer) check_span(g, side == 0 ? b.part - (int64_t)16 * bb * kSwC : b.part - 16 * bb, (int64_t)d.nct * d.kmax * rp * kSwC, kPart, "pieces");
      }
      if (fuse_phase && d.nb > RB) {  // a set's X side: each member's blocks once, all of their rows
        std::vector<int> o = owners;
        std::sort(o.begin(), o.end());
        EXPECT(std::adjacent_find(o.begin(), o.end()) == o.end() && (int)o.size() * RB == d.nb, "a set member appears twice");
        EXPECT(rows == rsum, "set side: %d rows, members' r sum to %d", rows, rsum);
        EXPECT(in_set[owners[0]] >= 0 && s.sets[in_set[owners[0]]] == owners, "set side's blocks are not its set's members in order");
      }
      if (outer) {  // rows t < T16 of Y: a lane reads its blocks at y_in + t * yrs + li * yls
        const int nread = fuse_phase ? 4 : RB;
        check_span(g, d.y_in, (T16 - 1) * d.yrs + 15 * d.yls + nread, kY, "y_in");
      }
    }
  }
  for (int i = 0; i < n; ++i)
    for (int side = 0; side < 2; ++side)
      for (int bb = 0; bb < RB; ++bb) {
        const int key = (i * 2 + side) * 8 + bb;
        EXPECT(nproj[key] == 1 && nouter[key] == 1, "module %d side %d block %d: projected %d times, OUTER %d times", i, side,
               bb, nproj[key], nouter[key]);
      }
  // reduces: slabs [nct][T][rp] in, Y rows t < T out (element (t, 16 b + li) at y[t * ys + b + li * sl])
  for (int k = 0; k < 2; ++k) {
    EXPECT(memcmp(blob + t.o_y[k], s.yd[k].data(), sizeof(YRedDesc) * n) == 0, "reduce %d descriptors in the blob", k);
    for (int i = 0; i < n; ++i) {
      const YRedDesc& y = s.yd[k][i];
      const ProbeDesc& p = ga.d[i];
      EXPECT(y.T == p.T && ((y.slab == p.slabH && y.nct == p.ksh) || (y.slab == p.slabJ && y.nct == p.ksj)), "reduce %d module %d", k, i);
      check_span(g, y.slab, (int64_t)y.nct * y.T * rp, kSlab, "reduce slab");
      check_span(g, y.y, (y.T - 1) * y.ys + (RB - 1) + 15 * y.sl + 1, kY, "reduce y");
    }
    EXPECT(s.yd[0][0].slab != s.yd[1][0].slab, "both reduces read the same slabs");
  }
  EXPECT(s.yblk >= 1, "yblk");
  for (int i = 0; i < n; ++i) EXPECT(s.yblk * 256 * 4 >= ga.d[i].T * rp, "yblk %lld too small for module %d", (long long)s.yblk, i);

  // ---- finish sides and jobs ----
  EXPECT(memcmp(blob + t.o_f, s.fd.data(), sizeof(FinDesc) * n) == 0, "finish descriptors in the blob");
  std::map<std::pair<int, int>, int> want;  // (module, 2 ct + side) -> pieces, split stripes only
  for (int i = 0; i < n; ++i) {
    const ProbeDesc& p = ga.d[i];
    const FinDesc& f = s.fd[i];
    EXPECT(f.gA == p.gA && f.gB == p.gB && f.in == p.in && f.out == p.out && f.r == p.r && f.ldb == p.ldb && f.acc == p.accumulate, "finish %d", i);
    for (int side = 0; side < 2; ++side) {
      const SwFinishSide& fs = side == 0 ? f.sx : f.sg;
      const int nct = side == 0 ? p.ksh : p.ksj;
      EXPECT(fs.part == (side == 0 ? p.partA : p.partB), "finish %d side %d: pieces", i, side);
      EXPECT(fs.ph == 0 || fs.ph == 1, "finish phase");
      EXPECT(fs.ph == 1 || !s.split_b, "pieces from phase B although it is PROJ-only");
      // the OUTER side that writes these pieces sits at fs.pre of that phase
      bool found = false;
      const bool fuse_phase = s.fuse && fs.ph == 1;
      for (const SweepDesc& d : s.sd[fs.ph + 1]) {
        if (d.pre != fs.pre) continue;
        for (const Blk& b : blocks_of(d, fuse_phase, RB)) found = found || b.part == fs.part;
        EXPECT(d.S == fs.S && d.kmax == fs.kmax && d.nct == nct, "finish %d side %d: geometry of its OUTER side", i, side);
      }
      EXPECT(found, "finish %d side %d: no OUTER side at step %lld writes its pieces", i, side, (long long)fs.pre);
      const std::vector<int64_t>& b = t.bounds[fs.ph + 1];
      for (int ct = 0; ct < nct; ++ct) {
        const int64_t u0 = fs.pre + (int64_t)ct * fs.S, u1 = u0 + fs.S;
        int np = 0;
        for (int w = 0; w + 1 < (int)b.size(); ++w) np += b[w] < u1 && b[w + 1] > u0;
        EXPECT(np >= 1 && np <= fs.kmax, "module %d side %d stripe %d: %d pieces, buffer of %d", i, side, ct, np, fs.kmax);
        if (np > 1) want[{i, 2 * ct + side}] = np;
      }
    }
  }
  const int* jobs = reinterpret_cast<const int*>(blob + t.o_j);
  EXPECT(t.njobs == (int)want.size(), "%d jobs, %zu split stripes", t.njobs, want.size());
  for (int j = 0; j < t.njobs; ++j) {
    const auto it = want.find({jobs[4 * j], jobs[4 * j + 1]});
    EXPECT(it != want.end() && it->second == jobs[4 * j + 2] && jobs[4 * j + 3] == 0, "job %d: module %d code %d pieces %d", j,
           jobs[4 * j], jobs[4 * j + 1], jobs[4 * j + 2]);
    if (it != want.end()) want.erase(it);  // (once)
  }

  // ---- determinism ----
  SweepSides s2;
  plan_sweep_sides(ga, bf16, kn, s2);
  SweepTables t2;
  const SweepError e2 = plan_sweep_tables(ga, s2, slots, t2);
  EXPECT(e2.code == 0 && t2.blob.size() == t.blob.size() && memcmp(t2.blob.data(), blob, t.blob.size()) == 0, "planning twice gives different blobs");
}

static const int kResident[5] = {1, 7, 256, 1024, 4096};

// both dtypes, every resident count in every phase
static void check_group(const char* name, const Group& g, const SweepKnobs& kn, const Expect& f32, const Expect& bf16) {
  g_case = name;
  for (int dt = 0; dt < 2; ++dt)
    for (int k = 0; k < 5; ++k) {
      const int slots[3] = {kResident[k], kResident[(k + 1) % 5], kResident[(k + 3) % 5]};
      check_plan(g, dt == 1, kn, slots, dt ? bf16 : f32);
    }
}

// q/k/v on one X, o, gate/up on one X, down
static std::vector<Mod> llama7b_layer(int r, int64_t T) {
  return {Mod{T, 4096, 4096, r, 1, 0, 0},  Mod{T, 4096, 4096, r, 1, 0, 1},  Mod{T, 4096, 4096, r, 1, 0, 0}, Mod{T, 4096, 4096, r, 1, 1, 1},
          Mod{T, 4096, 11008, r, 1, 2, 0}, Mod{T, 4096, 11008, r, 1, 2, 1}, Mod{T, 11008, 4096, r, 1, 3, 0}};
}

int main() {
  const SweepKnobs on;
  SweepKnobs no_share, no_balance;
  no_share.share_x = false;
  no_balance.balance = false;
  const Expect none{0, {}}, any{-1, {}};
  {  // LLaMA-2-7B layer, r 16: {q, k, v} and {gate, up}
    Group g;
    build(g, llama7b_layer(16, 1024), 1);
    check_group("7b r16", g, on, Expect{2, {2, 3}}, Expect{2, {2, 3}});
    check_group("7b r16 equal split", g, no_balance, Expect{2, {2, 3}}, Expect{2, {2, 3}});
    check_group("7b r16 no sharing", g, no_share, none, none);
    g_case = "7b r16 phases";
    SweepSides s;
    plan_sweep_sides(g.ga, false, on, s);
    EXPECT(s.fuse && s.weighted && s.sd[0].size() == 4 && s.sd[1].size() == 7 && s.sd[2].size() == 4, "phase sizes %zu %zu %zu",
           s.sd[0].size(), s.sd[1].size(), s.sd[2].size());
    EXPECT(s.sd[0][0].nb == 3 && s.sd[0][1].nb == 1 && s.sd[0][2].nb == 2 && s.sd[0][3].nb == 1, "phase A blocks");
    SweepSides sb;
    plan_sweep_sides(g.ga, true, on, sb);
    EXPECT(sb.fuse && !sb.weighted, "bf16 phase A is not weighted");
  }
  {  // r 32: sets of at most kSwMaxBlk / RB = 2 members -- {q, k}, v alone, {gate, up}
    Group g;
    build(g, llama7b_layer(32, 1024), 2);
    check_group("7b r32", g, on, Expect{2, {2, 2}}, Expect{2, {2, 2}});
    g_case = "7b r32 sets";
    SweepSides s;
    plan_sweep_sides(g.ga, false, on, s);
    EXPECT(s.sets.size() == 2 && s.sets[0] == std::vector<int>({0, 1}) && s.sets[1] == std::vector<int>({4, 5}), "r32 sets");
  }
  {  // r 64: no sets; bf16: phase B PROJ-only, phase C holds both OUTER sides of every module
    Group g;
    build(g, llama7b_layer(64, 1024), 4);
    check_group("7b r64", g, on, none, none);
    g_case = "7b r64 phases";
    SweepSides sf, sb;
    plan_sweep_sides(g.ga, false, on, sf);
    plan_sweep_sides(g.ga, true, on, sb);
    EXPECT(!sf.split_b && sf.sd[1].size() == 7 && sf.sd[2].size() == 7, "f32 phases");
    EXPECT(sb.split_b && sb.sd[0].size() == 7 && sb.sd[1].size() == 7 && sb.sd[2].size() == 14, "bf16 phases");
    for (const FinDesc& f : sb.fd) EXPECT(f.sx.ph == 1 && f.sg.ph == 1, "bf16 r64: pieces from phase C");
  }
  {  // sets not formed: sum of out < in; a module without B^T; sharing switched off
    Group g;
    build(g, {Mod{64, 4096, 1024, 16, 1, 0, 0}, Mod{64, 4096, 1024, 16, 1, 0, 1}}, 1);
    check_group("out < in", g, on, none, none);
    Group h;
    build(h, {Mod{64, 1024, 1024, 16, 1, 0, 0}, Mod{64, 1024, 1024, 16, 1, 0, 1}, Mod{64, 512, 512, 16, 0, 1, 0}}, 1);
    check_group("b not transposed", h, on, none, none);
    Group k;
    build(k, {Mod{64, 1024, 1024, 16, 1, 0, 0}, Mod{64, 1024, 1024, 16, 1, 0, 1}}, 1);
    check_group("shared", k, on, Expect{1, {2}}, Expect{1, {2}});
    check_group("share off", k, no_share, none, none);
  }
  // ragged: fewer than one stripe, one stripe plus a sliver, in % 4 != 0 (v4 off)
  for (int64_t T : {1, 9, 17, 33})
    for (int64_t N : {4, 100, 520, 1028}) {
      char name[64];
      std::snprintf(name, sizeof(name), "ragged T %d N %d", (int)T, (int)N);
      for (int r : {5, 16, 24, 40}) {
        Group g;
        build(g, {Mod{T, N, 1028 - N + 4, r, 1, 0, 1}, Mod{T, N, N, r, 1, 0, 0}, Mod{T, N + 1, N + 2, r, 1, 1, 0}}, rb_of(r));
        check_group(name, g, on, any, any);
        g_case = name;
        SweepSides s;
        plan_sweep_sides(g.ga, false, on, s);
        EXPECT(!s.v4, "in %% 4 != 0 but v4");
      }
    }
  {  // r 100 as two r-slices of 50 (ldb 100) on r-block 4
    Group g;
    build(g, {Mod{200, 1024, 2048, 50, 1, 0, 1}, Mod{77, 2048, 520, 50, 1, 1, 0}}, 4, 100);
    check_group("r-slices", g, on, none, none);
    g_case = "r-slices";
    EXPECT(g.ga.n == 4 && g.ga.d[1].gB == g.ga.d[0].gB + 50 && g.ga.d[1].ldb == 100, "slices");
  }
  // seeded random groups: one r-block per group, random X sharing
  std::mt19937_64 rng(20241020);
  auto uni = [&](int64_t lo, int64_t hi) { return lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1)); };
  for (int c = 0; c < 300; ++c) {
    const int n = (int)uni(1, 12), RB = 1 << uni(0, 2);
    const int rlo = RB == 1 ? 1 : 8 * RB + 1, rhi = 16 * RB;
    const bool all_bt = uni(0, 4) != 0;
    std::vector<Mod> mods;
    for (int i = 0; i < n; ++i) {
      Mod m{uni(1, 600), uni(4, 3000), uni(4, 3000), (int)uni(rlo, rhi), all_bt || uni(0, 1) ? 1 : 0, i, (int)uni(0, 1)};
      if (c % 3 == 0) m.in = m.in / 8 * 8 + 8, m.out = m.out / 8 * 8 + 8;  // (vector-friendly shapes: v4 can hold)
      if (c % 3 == 0) m.r = (m.r + 3) / 4 * 4;
      if (i > 0 && uni(0, 1)) {  // read an earlier module's X
        const Mod& o = mods[(size_t)uni(0, i - 1)];
        m.T = o.T;
        m.in = o.in;
        m.xid = o.xid;
      }
      mods.push_back(m);
    }
    char name[32];
    std::snprintf(name, sizeof(name), "random %d", c);
    Group g;
    build(g, mods, RB);
    g_case = name;
    const int slots[3] = {kResident[c % 5], kResident[(c / 5) % 5], kResident[(c / 25) % 5]};
    SweepKnobs kn;
    kn.share_x = c % 7 != 0;
    kn.balance = c % 2 == 0;
    check_plan(g, false, kn, slots, any);
    check_plan(g, true, kn, slots, any);
  }
  if (g_fail) {
    std::printf("%d failures\n", g_fail);
    return 1;
  }
  std::printf("OK %d\n", g_plans);
  return 0;
}
