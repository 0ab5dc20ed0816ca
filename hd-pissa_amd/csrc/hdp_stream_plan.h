// Host plan of the grouped HBM-streaming kernels that share one chunk walk (hdp_elementwise.hip: the
// stochastic-rounding merge, the compensated merge, the grouped copy and the float32 -> bf16 shadow cast): how one item splits into
// vector, edge and element-wise work, the validation of one item, and the batcher that cuts an item list into launches.  Pure C++ (no HIP, no environment):
// hipcc and the host compiler build the same code, the kernel calls the same split the host sums chunks
// with, and tests/stream_plan_check.cpp walks it on the CPU (tests/test_stream_plan.py, plain and under
// ASan/UBSan).  Nothing here dereferences an item's pointers.
//
// A "unit" is what an item counts: an element (the merge, the shadow cast) or a byte (the copy).  A vector
// is kVec units = 16 bytes of dst; a chunk is kStreamThreads x kU vectors, what one workgroup takes at a time.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "hdpissa.h"

namespace hdp {

#if defined(__HIP__)
#define HDP_SP_HD __host__ __device__ inline
#else
#define HDP_SP_HD inline
#endif

constexpr int kStreamThreads = 256;
constexpr int kStreamGrid = 2048;  // workgroups of one launch at most (8 per CU)

// The split of one item (count > 0).  vec: head units [0, head), then nv vectors, then the tail; head and
// tail ride on the lanes of the item's first chunk, so an item with nv == 0 still owns one chunk.  !vec: the
// item runs unit by unit over chunks of kStreamThreads x kU x kVec units, kElemU units per lane in flight.
struct StreamSplit {
  bool vec;
  int64_t head, nv, nch;
};

template <class P>
HDP_SP_HD StreamSplit stream_split(bool vec, int64_t head, int64_t count) {
  constexpr int64_t CH = (int64_t)kStreamThreads * P::kU;
  StreamSplit s;
  s.vec = vec;
  if (vec) {
    s.head = head < count ? head : count;
    s.nv = (count - s.head) / P::kVec;
    s.nch = s.nv ? (s.nv + CH - 1) / CH : 1;
  } else {
    s.head = 0;
    s.nv = 0;
    s.nch = (count + CH * P::kVec - 1) / (CH * P::kVec);
  }
  return s;
}

// The unit a lane of the item's first chunk moves on its own, or -1: lanes [0, kVec) take the head,
// lanes [kVec, 2 kVec) the tail
template <class P>
HDP_SP_HD int64_t stream_edge_unit(const StreamSplit& s, int lane, int64_t count) {
  if (lane < s.head) return lane;
  const int64_t j = s.head + s.nv * P::kVec + (lane - P::kVec);
  return lane >= P::kVec && lane < 2 * P::kVec && j < count ? j : -1;
}

HDP_SP_HD uintptr_t stream_addr(const void* p) { return reinterpret_cast<uintptr_t>(p); }
HDP_SP_HD bool stream_aligned16(const void* a, const void* b) { return ((stream_addr(a) | stream_addr(b)) & 15u) == 0; }

struct NoKey {};
struct SrSeed {
  uint32_t lo, hi;
};

// ---- the ops: item type, launch cap, vectors per lane, units per vector, units per lane of the unit-by-unit
// ---- path, algorithmic bytes per unit, the split and the validation of one item (check: null, or the text
// ---- that follows "item <i>")
// bf16 W = sr(float32(W) + dW): one Philox block per vector, so a vector starts at an element index % 8 == 0
struct MergeSrPlan {
  using Item = hdp_merge_sr_item;
  using Key = SrSeed;
  static constexpr int kCap = 64, kU = 8, kVec = 8, kElemU = 4;
  static constexpr double kBytes = 8;
  static HDP_SP_HD int64_t count(const Item& it) { return it.n; }
  static HDP_SP_HD StreamSplit split(const Item& it) {
    return stream_split<MergeSrPlan>(stream_aligned16(it.W, it.dW) && it.elem0 % 8 == 0, 0, it.n);
  }
  static const char* check(const Item& it) {
    if (it.n < 0 || it.elem0 < 0) return " has n < 0 or elem0 < 0";
    if (it.n && !(it.W && it.dW)) return " has a null pointer";
    if (it.n && ((stream_addr(it.W) & 1u) || (stream_addr(it.dW) & 3u))) return ": W must be 2-byte and dW 4-byte aligned";
    return nullptr;
  }
};

// dst <- src, bytes: vectors when dst and src sit alike within 16 bytes, behind a head up to dst's boundary
struct CopyPlan {
  using Item = hdp_copy_item;
  using Key = NoKey;
  static constexpr int kCap = 170, kU = 8, kVec = 16, kElemU = 16;
  static constexpr double kBytes = 2;
  static HDP_SP_HD int64_t count(const Item& it) { return it.bytes; }
  static HDP_SP_HD StreamSplit split(const Item& it) {
    const uintptr_t d = stream_addr(it.dst), q = stream_addr(it.src);
    return stream_split<CopyPlan>(((d ^ q) & 15u) == 0, (int64_t)((16u - (d & 15u)) & 15u), it.bytes);
  }
  static const char* check(const Item& it) {
    if (it.bytes < 0) return " has bytes < 0";
    if (it.bytes && !(it.dst && it.src)) return " has a null pointer";
    return nullptr;
  }
};

// bf16 dst <- float32 src
struct ShadowPlan {
  using Item = hdp_shadow_item;
  using Key = NoKey;
  static constexpr int kCap = 170, kU = 8, kVec = 8, kElemU = 16;
  static constexpr double kBytes = 6;
  static HDP_SP_HD int64_t count(const Item& it) { return it.n; }
  static HDP_SP_HD StreamSplit split(const Item& it) {
    return stream_split<ShadowPlan>(stream_aligned16(it.dst, it.src), 0, it.n);
  }
  static const char* check(const Item& it) {
    if (it.n < 0) return " has n < 0";
    if (it.n && !(it.dst && it.src)) return " has a null pointer";
    if (it.n && ((stream_addr(it.dst) & 1u) || (stream_addr(it.src) & 3u))) return ": dst must be 2-byte and src 4-byte aligned";
    return nullptr;
  }
};

// bf16 (W, C) <- compensated merge of float32 dW (hdp_comp.h): vectors when W, C and dW are all 16-byte aligned
struct MergeCompPlan {
  using Item = hdp_merge_comp_item;
  using Key = NoKey;
  static constexpr int kCap = 127, kU = 4, kVec = 8, kElemU = 4;
  static constexpr double kBytes = 12;  // read W 2, C 2, dW 4; write W 2, C 2
  static HDP_SP_HD int64_t count(const Item& it) { return it.n; }
  static HDP_SP_HD StreamSplit split(const Item& it) {
    return stream_split<MergeCompPlan>(stream_aligned16(it.W, it.C) && stream_aligned16(it.dW, it.dW), 0, it.n);
  }
  static const char* check(const Item& it) {
    if (it.n < 0) return " has n < 0";
    if (it.n && !(it.W && it.C && it.dW)) return " has a null pointer";
    if (it.n && (((stream_addr(it.W) | stream_addr(it.C)) & 1u) || (stream_addr(it.dW) & 3u)))
      return ": W and C must be 2-byte and dW 4-byte aligned";
    return nullptr;
  }
};

// ---- one launch's kernel arguments: the items by value (the 4 KB kernel-argument block sets the caps)
template <class P>
struct StreamArgs {
  int n;
  typename P::Key key;
  typename P::Item it[P::kCap];
};
static_assert(sizeof(StreamArgs<MergeSrPlan>) <= 4096 && sizeof(StreamArgs<CopyPlan>) <= 4096 &&
                  sizeof(StreamArgs<ShadowPlan>) <= 4096 && sizeof(StreamArgs<MergeCompPlan>) <= 4096,
              "stream kernel arguments must stay within 4 KB");

// ---- the batcher
// every item of the list, before anything is launched: true, or false with the message in err
template <class P>
bool stream_check(const char* who, int n, const typename P::Item* items, char* err, size_t cap) {
  if (n < 0 || (n > 0 && !items)) {
    snprintf(err, cap, "%s: bad item list", who);
    return false;
  }
  for (int i = 0; i < n; ++i)
    if (const char* why = P::check(items[i])) {
      snprintf(err, cap, "%s: item %d%s", who, i, why);
      return false;
    }
  return true;
}

inline unsigned stream_grid(int64_t chunks) { return (unsigned)(chunks < kStreamGrid ? chunks : kStreamGrid); }

// launches of at most P::kCap non-empty items: emit(args, chunks, algorithmic bytes) -> status, 0 to go on
template <class P, class Emit>
int stream_batch(int n, const typename P::Item* items, const typename P::Key& key, Emit&& emit) {
  StreamArgs<P> ga;
  ga.n = 0;
  ga.key = key;
  int64_t chunks = 0;
  double units = 0;
  auto flush = [&]() -> int {
    if (ga.n == 0) return 0;
    const int rc = emit(ga, chunks, P::kBytes * units);
    ga.n = 0;
    chunks = 0;
    units = 0;
    return rc;
  };
  for (int i = 0; i < n; ++i) {
    if (P::count(items[i]) == 0) continue;
    ga.it[ga.n] = items[i];
    chunks += P::split(items[i]).nch;
    units += (double)P::count(items[i]);
    if (++ga.n == P::kCap)
      if (const int rc = flush()) return rc;
  }
  return flush();
}

}  // namespace hdp
