// CPU check of MergeCompPlan in csrc/hdp_stream_plan.h (tests/test_stream_plan_comp.py builds and runs it, plain
// and under ASan/UBSan), in the manner of tests/stream_plan_check.cpp: items with each of W, C and dW off 16
// bytes in turn and the sizes around a vector and a chunk are walked the way stream_group_kernel walks them, and
// every element must be covered exactly once, inside the item, with 16-byte aligned vector accesses on all three
// pointers.  Then the batcher at the cap, and every refusal message.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hdp_stream_plan.h"

using namespace hdp;
using P = MergeCompPlan;

static long g_checks = 0;
static void fail(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vfprintf(stdout, fmt, ap);
  va_end(ap);
  fputc('\n', stdout);
  exit(1);
}
#define CHECK(cond, ...)            \
  do {                              \
    ++g_checks;                     \
    if (!(cond)) fail(__VA_ARGS__); \
  } while (0)

// never dereferenced
static const uintptr_t kW = 0x7f0000100000ull, kC = 0x7f0000500000ull, kD = 0x7f0000900000ull;

static hdp_merge_comp_item item(uintptr_t w, uintptr_t c, uintptr_t d, int64_t n) {
  return hdp_merge_comp_item{reinterpret_cast<void*>(w), reinterpret_cast<void*>(c), reinterpret_cast<const float*>(d), n};
}

static_assert(P::kVec == 8 && P::kBytes == 12, "an element is the unit: 8 per vector, 12 bytes of traffic each");
static_assert(sizeof(StreamArgs<P>) <= 4096 && sizeof(StreamArgs<P>) + sizeof(hdp_merge_comp_item) > 4096,
              "kCap is what fits the 4 KB argument block");

// one item, walked as stream_group_kernel walks it; returns the chunks it owns
static int64_t walk(const hdp_merge_comp_item& it, uintptr_t w, uintptr_t c, uintptr_t d, bool want_vec) {
  constexpr int64_t CH = (int64_t)kStreamThreads * P::kU;
  const int64_t n = P::count(it);
  const StreamSplit sp = P::split(it);
  CHECK(sp.vec == want_vec, "W %%16 = %d, C %%16 = %d, dW %%16 = %d, n = %lld: vec = %d, want %d", (int)(w & 15), (int)(c & 15),
        (int)(d & 15), (long long)n, (int)sp.vec, (int)want_vec);
  if (sp.vec) {
    const int64_t nv = n / P::kVec;
    CHECK(sp.head == 0 && sp.nv == nv && sp.nch == (nv ? (nv + CH - 1) / CH : 1), "n = %lld: split %lld %lld %lld", (long long)n,
          (long long)sp.head, (long long)sp.nv, (long long)sp.nch);
  } else {
    CHECK(sp.head == 0 && sp.nv == 0 && sp.nch == (n + CH * P::kVec - 1) / (CH * P::kVec), "n = %lld: unit split", (long long)n);
  }
  std::vector<unsigned char> cover((size_t)n, 0);
  auto touch = [&](int64_t j, int64_t cnt) {
    CHECK(j >= 0 && j + cnt <= n, "n = %lld: elements [%lld, %lld) outside the item", (long long)n, (long long)j,
          (long long)(j + cnt));
    for (int64_t k = 0; k < cnt; ++k) ++cover[(size_t)(j + k)];
  };
  for (int64_t ch = 0; ch < sp.nch; ++ch)
    for (int lane = 0; lane < kStreamThreads; ++lane) {
      if (sp.vec) {
        for (int u = 0; u < P::kU; ++u) {
          const int64_t i = ch * CH + lane + (int64_t)u * kStreamThreads;
          if (i >= sp.nv) continue;
          const int64_t off = i * P::kVec;
          CHECK((w + (uintptr_t)off * 2) % 16 == 0 && (c + (uintptr_t)off * 2) % 16 == 0 && (d + (uintptr_t)off * 4) % 16 == 0 &&
                    (d + (uintptr_t)off * 4 + 16) % 16 == 0,
                "vector %lld is not 16-byte aligned", (long long)i);
          touch(off, P::kVec);
        }
        if (ch == 0) {
          const int64_t j = stream_edge_unit<P>(sp, lane, n);
          if (j >= 0) touch(j, 1);
        }
      } else {
        const int64_t e0 = ch * CH * P::kVec + lane;
        for (int64_t o = 0; o < CH * P::kVec; o += (int64_t)kStreamThreads * P::kElemU)
          for (int u = 0; u < P::kElemU; ++u) {
            const int64_t i = e0 + o + (int64_t)u * kStreamThreads;
            if (i < n) touch(i, 1);
          }
      }
    }
  for (int64_t j = 0; j < n; ++j)
    CHECK(cover[(size_t)j] == 1, "W %%16 = %d, C %%16 = %d, dW %%16 = %d, n = %lld: element %lld covered %d times", (int)(w & 15),
          (int)(c & 15), (int)(d & 15), (long long)n, (long long)j, (int)cover[(size_t)j]);
  return sp.nch;
}

static void splits() {
  constexpr int64_t chunk = (int64_t)kStreamThreads * P::kU * P::kVec;
  static_assert((P::kU * P::kVec) % P::kElemU == 0, "whole element-wise steps per chunk");
  const int64_t ns[] = {0, 1, 7, 8, 9, chunk - 1, chunk, chunk + 1, 3 * chunk + 43};
  // all aligned; then each of W, C and dW off 16 bytes in turn (every offset its alignment allows); then all three
  struct Off {
    int w, c, d;
  };
  std::vector<Off> offs = {{0, 0, 0}, {16, 32, 48}};
  for (int o = 2; o < 16; o += 2) {
    offs.push_back({o, 0, 0});
    offs.push_back({0, o, 0});
  }
  for (int o = 4; o < 16; o += 4) offs.push_back({0, 0, o});
  offs.push_back({2, 6, 4});
  for (const Off& f : offs)
    for (int64_t n : ns) {
      const uintptr_t w = kW + f.w, c = kC + f.c, d = kD + f.d;
      const hdp_merge_comp_item it = item(w, c, d, n);
      CHECK(P::check(it) == nullptr, "a valid item is refused");
      const bool want_vec = ((w | c | d) & 15) == 0;
      int64_t got_chunks = 0, launches = 0;
      double got_bytes = 0;
      const int rc = stream_batch<P>(1, &it, NoKey{}, [&](const StreamArgs<P>& ga, int64_t chunks, double bytes) {
        ++launches;
        got_chunks = chunks;
        got_bytes = bytes;
        CHECK(ga.n == 1 && memcmp(&ga.it[0], &it, sizeof it) == 0, "the batcher changed the item");
        return 0;
      });
      CHECK(rc == 0 && launches == (n ? 1 : 0), "n = %lld: %lld launches", (long long)n, (long long)launches);
      if (n == 0) continue;
      const int64_t nch = walk(it, w, c, d, want_vec);
      CHECK(nch == got_chunks, "the kernel walks %lld chunks, the batcher counts %lld", (long long)nch, (long long)got_chunks);
      CHECK(got_bytes == 12.0 * (double)n, "bytes %g", got_bytes);
    }
}

static void batches() {
  constexpr int cap = P::kCap;
  constexpr int64_t chunk = (int64_t)kStreamThreads * P::kU * P::kVec;
  for (int live : {0, 1, cap, cap + 1, 2 * cap + 1}) {
    // empty items in front, after every third live item and at the end; sizes and alignments vary
    std::vector<hdp_merge_comp_item> items;
    std::vector<int> live_at;
    items.push_back(item(0, 0, 0, 0));
    for (int k = 0; k < live; ++k) {
      const int64_t n = 1 + (int64_t)k * 977 % (2 * chunk + 5);
      live_at.push_back((int)items.size());
      const uintptr_t at = (uintptr_t)k * (1u << 20);
      items.push_back(item(kW + at + (k % 5 == 4 ? 4 : 0), kC + at + (k % 7 == 6 ? 2 : 0), kD + at + (k % 11 == 10 ? 8 : 0), n));
      if (k % 3 == 2) items.push_back(item(0, 0, 0, 0));
    }
    items.push_back(item(0, 0, 0, 0));
    char err[200];
    CHECK(stream_check<P>("comp", (int)items.size(), items.data(), err, sizeof err), "valid list refused: %s", err);
    int seen = 0, launches = 0;
    const int rc = stream_batch<P>((int)items.size(), items.data(), NoKey{}, [&](const StreamArgs<P>& ga, int64_t chunks, double bytes) {
      const int want = live - seen < cap ? live - seen : cap;
      CHECK(ga.n == want && want > 0, "%d live items: launch %d holds %d, want %d", live, launches, ga.n, want);
      int64_t sum_chunks = 0;
      double sum_units = 0;
      for (int j = 0; j < ga.n; ++j) {
        const hdp_merge_comp_item& src = items[(size_t)live_at[(size_t)(seen + j)]];
        CHECK(memcmp(&ga.it[j], &src, sizeof src) == 0, "launch %d slot %d is not live item %d", launches, j, seen + j);
        sum_chunks += P::split(src).nch;
        sum_units += (double)P::count(src);
      }
      CHECK(chunks == sum_chunks && chunks >= ga.n, "launch %d: %lld chunks, want %lld", launches, (long long)chunks,
            (long long)sum_chunks);
      CHECK(bytes == 12.0 * sum_units, "launch %d: %g bytes, want %g", launches, bytes, 12.0 * sum_units);
      CHECK(stream_grid(chunks) >= 1 && stream_grid(chunks) <= (unsigned)kStreamGrid && stream_grid(chunks) <= chunks, "grid");
      seen += ga.n;
      ++launches;
      return 0;
    });
    CHECK(rc == 0 && seen == live && launches == (live + cap - 1) / cap, "%d live items: %d launches, %d items seen", live, launches,
          seen);
    int calls = 0;
    const int rc2 = stream_batch<P>((int)items.size(), items.data(), NoKey{}, [&](const StreamArgs<P>&, int64_t, double) {
      ++calls;
      return 2;
    });
    CHECK(rc2 == (live ? 2 : 0) && calls == (live ? 1 : 0), "a failed launch must end the call");
  }
}

static void refusals() {
  const char* op = "hdp_merge_group_comp";
  char err[200];
  CHECK(stream_check<P>(op, 0, nullptr, err, sizeof err), "empty list refused");
  CHECK(!stream_check<P>(op, 1, nullptr, err, sizeof err) && strstr(err, "bad item list") && strstr(err, op), "null list: %s", err);
  CHECK(!stream_check<P>(op, -1, nullptr, err, sizeof err) && strstr(err, "bad item list"), "n < 0: %s", err);
  hdp_merge_comp_item items[3] = {item(kW, kC, kD, 64), item(0, 0, 0, 0), item(kW, kC, kD, -1)};
  CHECK(!stream_check<P>(op, 3, items, err, sizeof err) && strstr(err, "item 2") && strstr(err, "n < 0") && strstr(err, op),
        "negative count: %s", err);
  items[2] = item(0, kC, kD, 8);
  CHECK(!stream_check<P>(op, 3, items, err, sizeof err) && strstr(err, "item 2") && strstr(err, "null pointer"), "null W: %s", err);
  items[2] = item(kW, 0, kD, 8);
  CHECK(!stream_check<P>(op, 3, items, err, sizeof err) && strstr(err, "item 2") && strstr(err, "null pointer"), "null C: %s", err);
  items[2] = item(kW, kC, 0, 8);
  CHECK(!stream_check<P>(op, 3, items, err, sizeof err) && strstr(err, "item 2") && strstr(err, "null pointer"), "null dW: %s", err);
  items[2] = item(kW + 1, kC, kD, 8);
  CHECK(!stream_check<P>(op, 3, items, err, sizeof err) && strstr(err, "item 2") && strstr(err, "W and C must be 2-byte"), "odd W: %s", err);
  items[2] = item(kW, kC + 1, kD, 8);
  CHECK(!stream_check<P>(op, 3, items, err, sizeof err) && strstr(err, "item 2") && strstr(err, "W and C must be 2-byte"), "odd C: %s", err);
  items[2] = item(kW, kC, kD + 2, 8);
  CHECK(!stream_check<P>(op, 3, items, err, sizeof err) && strstr(err, "item 2") && strstr(err, "dW 4-byte aligned"), "odd dW: %s", err);
  items[2] = item(kW + 1, kC + 1, kD + 2, 0);  // (an empty item's pointers are not looked at)
  CHECK(stream_check<P>(op, 3, items, err, sizeof err), "an empty item is refused: %s", err);
  CHECK(stream_check<P>(op, 2, items, err, sizeof err), "the valid prefix is refused");
}

int main() {
  splits();
  batches();
  refusals();
  printf("OK %ld checks\n", g_checks);
  return 0;
}
