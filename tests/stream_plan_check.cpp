// CPU check of csrc/hdp_stream_plan.h (tests/test_stream_plan.py builds and runs it, plain and under
// ASan/UBSan).  For every op: items at every dst / src offset of 0..31 bytes and the sizes around a vector
// and a chunk are walked the way stream_group_kernel walks them, and every unit must be covered exactly
// once, inside the item, with 16-byte aligned vector accesses.  Then the batcher: launch sizes, chunk totals
// and bytes for item lists around the cap, with empty items in between, and the validation messages.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

#include "hdp_stream_plan.h"

using namespace hdp;

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

static const uintptr_t kDstBase = 0x7f0000100000ull, kSrcBase = 0x7f0000900000ull;  // never dereferenced

template <class P>
struct Make;
template <>
struct Make<MergeSrPlan> {
  static hdp_merge_sr_item item(uintptr_t d, uintptr_t s, int64_t n, int64_t elem0) {
    return hdp_merge_sr_item{reinterpret_cast<void*>(d), reinterpret_cast<const float*>(s), n, elem0, 7u};
  }
};
template <>
struct Make<CopyPlan> {
  static hdp_copy_item item(uintptr_t d, uintptr_t s, int64_t n, int64_t) {
    return hdp_copy_item{reinterpret_cast<void*>(d), reinterpret_cast<const void*>(s), n};
  }
};
template <>
struct Make<ShadowPlan> {
  static hdp_shadow_item item(uintptr_t d, uintptr_t s, int64_t n, int64_t) {
    return hdp_shadow_item{reinterpret_cast<void*>(d), reinterpret_cast<const float*>(s), n};
  }
};

// one item, walked as stream_group_kernel walks it; returns the chunks it owns
template <class P>
static int64_t walk(const char* op, const typename P::Item& it, uintptr_t d, uintptr_t s, int dsz, int ssz, bool want_vec,
                    int64_t want_head) {
  constexpr int64_t CH = (int64_t)kStreamThreads * P::kU;
  const int64_t n = P::count(it);
  const StreamSplit sp = P::split(it);
  CHECK(sp.vec == want_vec, "%s: d %%32 = %d, s %%32 = %d, n = %lld: vec = %d, want %d", op, (int)(d & 31), (int)(s & 31),
        (long long)n, (int)sp.vec, (int)want_vec);
  if (sp.vec) {
    const int64_t head = want_head < n ? want_head : n, nv = (n - head) / P::kVec;
    CHECK(sp.head == head && sp.nv == nv && sp.nch == (nv ? (nv + CH - 1) / CH : 1), "%s: n = %lld: split %lld %lld %lld",
          op, (long long)n, (long long)sp.head, (long long)sp.nv, (long long)sp.nch);
  } else {
    CHECK(sp.head == 0 && sp.nv == 0 && sp.nch == (n + CH * P::kVec - 1) / (CH * P::kVec), "%s: n = %lld: unit split", op,
          (long long)n);
  }
  std::vector<unsigned char> cover((size_t)n, 0);
  auto touch = [&](int64_t j, int64_t cnt) {
    CHECK(j >= 0 && j + cnt <= n, "%s: n = %lld: units [%lld, %lld) outside the item", op, (long long)n, (long long)j,
          (long long)(j + cnt));
    for (int64_t k = 0; k < cnt; ++k) ++cover[(size_t)(j + k)];
  };
  for (int64_t c = 0; c < sp.nch; ++c)
    for (int lane = 0; lane < kStreamThreads; ++lane) {
      if (sp.vec) {
        for (int u = 0; u < P::kU; ++u) {
          const int64_t i = c * CH + lane + (int64_t)u * kStreamThreads;
          if (i >= sp.nv) continue;
          const int64_t off = sp.head + i * P::kVec;
          CHECK((d + (uintptr_t)off * dsz) % 16 == 0 && (s + (uintptr_t)off * ssz) % 16 == 0,
                "%s: vector %lld of an item at d %%16 = %d, s %%16 = %d is not 16-byte aligned", op, (long long)i,
                (int)(d & 15), (int)(s & 15));
          touch(off, P::kVec);
        }
        if (c == 0) {
          const int64_t j = stream_edge_unit<P>(sp, lane, n);
          if (j >= 0) touch(j, 1);
        }
      } else {
        const int64_t e0 = c * CH * P::kVec + lane;
        for (int64_t o = 0; o < CH * P::kVec; o += (int64_t)kStreamThreads * P::kElemU)
          for (int u = 0; u < P::kElemU; ++u) {
            const int64_t i = e0 + o + (int64_t)u * kStreamThreads;
            if (i < n) touch(i, 1);
          }
      }
    }
  for (int64_t j = 0; j < n; ++j)
    CHECK(cover[(size_t)j] == 1, "%s: d %%32 = %d, s %%32 = %d, n = %lld: unit %lld covered %d times", op, (int)(d & 31),
          (int)(s & 31), (long long)n, (long long)j, (int)cover[(size_t)j]);
  return sp.nch;
}

// dsz / ssz: bytes per unit of dst / src; copy: vectors whenever dst and src sit alike
template <class P>
static void splits(const char* op, int dsz, int ssz, bool copy) {
  constexpr int64_t vec = P::kVec, chunk = (int64_t)kStreamThreads * P::kU * P::kVec;
  const int64_t ns[] = {0, 1, vec - 1, vec, vec + 1, chunk - 1, chunk, chunk + 1, 3 * chunk + 43};
  const bool sr = std::is_same<P, MergeSrPlan>::value;
  for (int doff = 0; doff < 32; doff += dsz)
    for (int soff = 0; soff < 32; soff += ssz)
      for (int64_t n : ns)
        for (int64_t elem0 : {(int64_t)0, (int64_t)8, (int64_t)3, (int64_t)((1ll << 33) + 4)}) {
          if (!sr && elem0) continue;
          const uintptr_t d = kDstBase + doff, s = kSrcBase + soff;
          const typename P::Item it = Make<P>::item(d, s, n, elem0);
          CHECK(P::check(it) == nullptr, "%s: a valid item is refused", op);
          const bool want_vec = copy ? ((d ^ s) & 15) == 0 : ((d | s) & 15) == 0 && elem0 % 8 == 0;
          int64_t got_chunks = 0, launches = 0;
          double got_bytes = 0;
          const int rc = stream_batch<P>(1, &it, typename P::Key{}, [&](const StreamArgs<P>& ga, int64_t chunks, double bytes) {
            ++launches;
            got_chunks = chunks;
            got_bytes = bytes;
            CHECK(ga.n == 1 && memcmp(&ga.it[0], &it, sizeof it) == 0, "%s: the batcher changed the item", op);
            return 0;
          });
          CHECK(rc == 0 && launches == (n ? 1 : 0), "%s: n = %lld: %lld launches", op, (long long)n, (long long)launches);
          if (n == 0) continue;
          const int64_t nch = walk<P>(op, it, d, s, dsz, ssz, want_vec, copy ? (int64_t)((16 - (d & 15)) & 15) : 0);
          CHECK(nch == got_chunks, "%s: the kernel walks %lld chunks, the batcher counts %lld", op, (long long)nch,
                (long long)got_chunks);
          CHECK(got_bytes == P::kBytes * (double)n, "%s: bytes %g", op, got_bytes);
        }
}

template <class P>
static void batches(const char* op) {
  constexpr int cap = P::kCap;
  constexpr int64_t chunk = (int64_t)kStreamThreads * P::kU * P::kVec;
  for (int live : {0, 1, cap, cap + 1, 2 * cap + 1}) {
    // empty items in front, after every third live item and at the end; sizes and alignments vary
    std::vector<typename P::Item> items;
    std::vector<int> live_at;
    items.push_back(Make<P>::item(0, 0, 0, 0));
    for (int k = 0; k < live; ++k) {
      const int64_t n = 1 + (int64_t)k * 977 % (2 * chunk + 5);
      live_at.push_back((int)items.size());
      items.push_back(Make<P>::item(kDstBase + (uintptr_t)k * (1u << 20) + (k % 5 == 4 ? 4 : 0), kSrcBase + (uintptr_t)k * (1u << 20), n, 0));
      if (k % 3 == 2) items.push_back(Make<P>::item(0, 0, 0, 0));
    }
    items.push_back(Make<P>::item(0, 0, 0, 0));
    char err[200];
    CHECK(stream_check<P>(op, (int)items.size(), items.data(), err, sizeof err), "%s: valid list refused: %s", op, err);
    int seen = 0, launches = 0;
    const int rc = stream_batch<P>((int)items.size(), items.data(), typename P::Key{}, [&](const StreamArgs<P>& ga, int64_t chunks, double bytes) {
      const int want = live - seen < cap ? live - seen : cap;
      CHECK(ga.n == want && want > 0, "%s: %d live items: launch %d holds %d, want %d", op, live, launches, ga.n, want);
      int64_t sum_chunks = 0;
      double sum_units = 0;
      for (int j = 0; j < ga.n; ++j) {
        const typename P::Item& src = items[(size_t)live_at[(size_t)(seen + j)]];
        CHECK(memcmp(&ga.it[j], &src, sizeof src) == 0, "%s: launch %d slot %d is not live item %d", op, launches, j, seen + j);
        sum_chunks += P::split(src).nch;
        sum_units += (double)P::count(src);
      }
      CHECK(chunks == sum_chunks && chunks >= ga.n, "%s: launch %d: %lld chunks, want %lld", op, launches, (long long)chunks,
            (long long)sum_chunks);
      CHECK(bytes == P::kBytes * sum_units, "%s: launch %d: %g bytes, want %g", op, launches, bytes, P::kBytes * sum_units);
      CHECK(stream_grid(chunks) >= 1 && stream_grid(chunks) <= (unsigned)kStreamGrid && stream_grid(chunks) <= chunks, "%s: grid", op);
      seen += ga.n;
      ++launches;
      return 0;
    });
    CHECK(rc == 0 && seen == live && launches == (live + cap - 1) / cap, "%s: %d live items: %d launches, %d items seen", op,
          live, launches, seen);
    // a failing launch ends the call with its status
    int calls = 0;
    const int rc2 = stream_batch<P>((int)items.size(), items.data(), typename P::Key{}, [&](const StreamArgs<P>&, int64_t, double) {
      ++calls;
      return 2;
    });
    CHECK(rc2 == (live ? 2 : 0) && calls == (live ? 1 : 0), "%s: a failed launch must end the call", op);
  }
}

template <class P>
static void refusals(const char* op, const char* neg_text) {
  char err[200];
  CHECK(stream_check<P>(op, 0, nullptr, err, sizeof err), "%s: empty list refused", op);
  CHECK(!stream_check<P>(op, 1, nullptr, err, sizeof err) && strstr(err, "bad item list"), "%s: null list: %s", op, err);
  CHECK(!stream_check<P>(op, -1, nullptr, err, sizeof err) && strstr(err, "bad item list"), "%s: n < 0: %s", op, err);
  typename P::Item items[3] = {Make<P>::item(kDstBase, kSrcBase, 64, 0), Make<P>::item(0, 0, 0, 0), Make<P>::item(kDstBase, kSrcBase, -1, 0)};
  CHECK(!stream_check<P>(op, 3, items, err, sizeof err) && strstr(err, "item 2") && strstr(err, neg_text) && strstr(err, op),
        "%s: negative count: %s", op, err);
  items[2] = Make<P>::item(0, kSrcBase, 8, 0);
  CHECK(!stream_check<P>(op, 3, items, err, sizeof err) && strstr(err, "item 2") && strstr(err, "null pointer"), "%s: null dst: %s", op, err);
  items[2] = Make<P>::item(kDstBase, 0, 8, 0);
  CHECK(!stream_check<P>(op, 3, items, err, sizeof err) && strstr(err, "item 2") && strstr(err, "null pointer"), "%s: null src: %s", op, err);
  CHECK(stream_check<P>(op, 2, items, err, sizeof err), "%s: the valid prefix is refused", op);
}

int main() {
  splits<MergeSrPlan>("merge sr", 2, 4, false);
  splits<CopyPlan>("copy", 1, 1, true);
  splits<ShadowPlan>("shadow", 2, 4, false);

  batches<MergeSrPlan>("merge sr");
  batches<CopyPlan>("copy");
  batches<ShadowPlan>("shadow");

  refusals<MergeSrPlan>("hdp_merge_group_sr", "n < 0");
  refusals<CopyPlan>("hdp_copy_group", "bytes < 0");
  refusals<ShadowPlan>("hdp_shadow_group", "n < 0");
  char err[200];
  const hdp_merge_sr_item sr_bad[2] = {{reinterpret_cast<void*>(kDstBase), reinterpret_cast<const float*>(kSrcBase), 8, 0, 0},
                                       {reinterpret_cast<void*>(kDstBase), reinterpret_cast<const float*>(kSrcBase), 8, -8, 0}};
  CHECK(!stream_check<MergeSrPlan>("sr", 2, sr_bad, err, sizeof err) && strstr(err, "item 1") && strstr(err, "elem0 < 0"), "sr elem0: %s", err);
  const hdp_merge_sr_item sr_odd[1] = {{reinterpret_cast<void*>(kDstBase + 1), reinterpret_cast<const float*>(kSrcBase), 8, 0, 0}};
  CHECK(!stream_check<MergeSrPlan>("sr", 1, sr_odd, err, sizeof err) && strstr(err, "aligned"), "sr odd W: %s", err);
  const hdp_shadow_item sh_odd[1] = {{reinterpret_cast<void*>(kDstBase), reinterpret_cast<const float*>(kSrcBase + 2), 8}};
  CHECK(!stream_check<ShadowPlan>("shadow", 1, sh_odd, err, sizeof err) && strstr(err, "aligned"), "shadow odd src: %s", err);

  printf("OK %ld checks\n", g_checks);
  return 0;
}
