// K5 merge (hp:394) and K3 Adam-on-factors (hp:356-373): HBM-streaming kernels.
//
// Both are pure streams with no reuse: 16-byte vector accesses per lane.  Roofline:
//   merge f32 W : 12 B/element (read W, read dW, write W)
//   merge bf16 W:  8 B/element (read W 2, read dW 4, write W 2)
//   adam        : 24 B/element (read g, m, v; write m, v, delta) (+4 with zero_grad)
#include "hdp_common.h"
#include "hdp_comp.h"
#include "hdp_sr.h"
#include "hdp_stream_plan.h"

namespace hdp {

constexpr int kEwThreads = 256;
static_assert(kEwThreads == kStreamThreads, "the stream plan counts chunks in workgroups of kEwThreads");
typedef uint16_t u16x8 __attribute__((ext_vector_type(8)));

static int ew_grid(int64_t vec_items, int per_thread) {
  int64_t blocks = (vec_items + (int64_t)kEwThreads * per_thread - 1) / ((int64_t)kEwThreads * per_thread);
  if (blocks > 256 * 8) blocks = 256 * 8;
  if (blocks < 1) blocks = 1;
  return (int)blocks;
}

// ---------------------------------------------------------------------------------------
// merge: W += dW.  Contiguous chunks: a workgroup owns kMergeU x 256 consecutive vectors at a time
// (every load of the chunk issued before its first store; each byte touched once, so non-temporal
// loads and stores) and walks chunks blockIdx.x, + grid, ... of one flat chunk space over a bucket's
// items.  tools/merge_bw.hip on a 1 GiB float32 slab: this form 5.76 TB/s (0.72 of 8) against 4.61 for
// the grid-stride loop with two vectors per lane it replaces (profiles/r03_merge_bw_v2.txt).
// ---------------------------------------------------------------------------------------
constexpr int kMergeU = 4;            // vectors per lane per chunk
constexpr int kMergeGrid = 2048;      // workgroups (8 per CU)
constexpr int kMergeGroupMax = 64;
struct MergeGroupArgs {
  int n;
  void* W[kMergeGroupMax];
  const float* dW[kMergeGroupMax];
  int64_t nv[kMergeGroupMax];  // f32: float4 vectors; bf16: 8-element vectors
};
static_assert(sizeof(MergeGroupArgs) <= 4096, "merge group kernel arguments must stay within 4 KB");

template <bool BF>
__global__ __launch_bounds__(kEwThreads) void merge_chunk_kernel(MergeGroupArgs ga) {
  // bf16 W with float32 dW: 8 vectors per lane (r04, tools/merge_bench.py: 0.69 -> 0.735 of HBM; float32 W and
  // the bf16-dW merge are faster at 4)
  constexpr int U = BF ? 2 * kMergeU : kMergeU;
  constexpr int64_t CH = (int64_t)kEwThreads * U;  // vectors per chunk
  int it = 0;
  int64_t base = 0, nch = (ga.nv[0] + CH - 1) / CH;      // item it owns chunks [base, base + nch)
  for (int64_t c = blockIdx.x;; c += gridDim.x) {        // c, it, base: workgroup-uniform
    while (c >= base + nch) {
      base += nch;
      if (++it == ga.n) return;
      nch = (ga.nv[it] + CH - 1) / CH;
    }
    const int64_t nv = ga.nv[it];
    const int64_t v0 = (c - base) * CH + threadIdx.x;
    const HDP_GLOBAL f32x4* D4 = reinterpret_cast<const HDP_GLOBAL f32x4*>(gptr(ga.dW[it]));
    if constexpr (!BF) {
      HDP_GLOBAL f32x4* W4 = reinterpret_cast<HDP_GLOBAL f32x4*>(gptr(reinterpret_cast<float*>(ga.W[it])));
      f32x4 w[U], d[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t i = v0 + u * kEwThreads;
        if (i < nv) {
          d[u] = __builtin_nontemporal_load(D4 + i);
          w[u] = __builtin_nontemporal_load(W4 + i);
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t i = v0 + u * kEwThreads;
        if (i < nv) __builtin_nontemporal_store(w[u] + d[u], W4 + i);
      }
    } else {
      HDP_GLOBAL u16x8* W8 = reinterpret_cast<HDP_GLOBAL u16x8*>(gptr(reinterpret_cast<uint16_t*>(ga.W[it])));
      u16x8 w[U];
      f32x4 d0[U], d1[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t i = v0 + u * kEwThreads;
        if (i < nv) {
          d0[u] = __builtin_nontemporal_load(D4 + 2 * i);
          d1[u] = __builtin_nontemporal_load(D4 + 2 * i + 1);
          w[u] = __builtin_nontemporal_load(W8 + i);
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t i = v0 + u * kEwThreads;
        if (i < nv) {  // bf16(W + bf16(dW)), two elements per packed conversion
          typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
          const u32x4 wv = __builtin_bit_cast(u32x4, w[u]);
          u32x4 o;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const f32x4& dd = k < 2 ? d0[u] : d1[u];
            const uint32_t dp = cvt_pk_bf16(dd[(2 * k) & 3], dd[(2 * k + 1) & 3]);
            o[k] = cvt_pk_bf16(__uint_as_float(wv[k] << 16) + __uint_as_float(dp << 16),
                               __uint_as_float(wv[k] & 0xffff0000u) + __uint_as_float(dp & 0xffff0000u));
          }
          __builtin_nontemporal_store(__builtin_bit_cast(u16x8, o), W8 + i);
        }
      }
    }
  }
}

// bf16 W += bf16 dW (the rank-ordered bf16 exchange): 8-element vectors, 6 B per element
__global__ __launch_bounds__(kEwThreads) void merge_bf16dw_kernel(MergeGroupArgs ga) {
  constexpr int64_t CH = (int64_t)kEwThreads * kMergeU;
  int it = 0;
  int64_t base = 0, nch = (ga.nv[0] + CH - 1) / CH;
  for (int64_t c = blockIdx.x;; c += gridDim.x) {
    while (c >= base + nch) {
      base += nch;
      if (++it == ga.n) return;
      nch = (ga.nv[it] + CH - 1) / CH;
    }
    const int64_t nv = ga.nv[it];
    const int64_t v0 = (c - base) * CH + threadIdx.x;
    HDP_GLOBAL u16x8* W8 = reinterpret_cast<HDP_GLOBAL u16x8*>(gptr(reinterpret_cast<uint16_t*>(ga.W[it])));
    const HDP_GLOBAL u16x8* D8 =
        reinterpret_cast<const HDP_GLOBAL u16x8*>(gptr(reinterpret_cast<const uint16_t*>(ga.dW[it])));
    u16x8 w[kMergeU], d[kMergeU];
#pragma unroll
    for (int u = 0; u < kMergeU; ++u) {
      const int64_t i = v0 + u * kEwThreads;
      if (i < nv) {
        d[u] = __builtin_nontemporal_load(D8 + i);
        w[u] = __builtin_nontemporal_load(W8 + i);
      }
    }
#pragma unroll
    for (int u = 0; u < kMergeU; ++u) {
      const int64_t i = v0 + u * kEwThreads;
      if (i < nv) {
        typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
        const u32x4 wv = __builtin_bit_cast(u32x4, w[u]), dv = __builtin_bit_cast(u32x4, d[u]);
        u32x4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k)
          o[k] = cvt_pk_bf16(__uint_as_float(wv[k] << 16) + __uint_as_float(dv[k] << 16),
                             __uint_as_float(wv[k] & 0xffff0000u) + __uint_as_float(dv[k] & 0xffff0000u));
        __builtin_nontemporal_store(__builtin_bit_cast(u16x8, o), W8 + i);
      }
    }
  }
}

__global__ void merge_bf16dw_scalar_kernel(uint16_t* W, const uint16_t* dW, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    W[i] = f32_to_bf16(bf16_to_f32(W[i]) + bf16_to_f32(dW[i]));
}

static int merge_chunk_launch(const MergeGroupArgs& ga, bool bf16, double bytes, hipStream_t st) {
  // the chunk the kernel walks (merge_chunk_kernel<BF>'s U): the grid never exceeds the chunk count
  const int64_t CH = (int64_t)kEwThreads * (bf16 ? 2 * kMergeU : kMergeU);
  int64_t chunks = 0;
  for (int i = 0; i < ga.n; ++i) chunks += (ga.nv[i] + CH - 1) / CH;
  if (chunks == 0) return HDP_OK;
  const unsigned grid = (unsigned)(chunks < kMergeGrid ? chunks : kMergeGrid);
  KTimer kt(K_MERGE, st, bytes);
  if (bf16) hipLaunchKernelGGL(merge_chunk_kernel<true>, dim3(grid), dim3(kEwThreads), 0, st, ga);
  else hipLaunchKernelGGL(merge_chunk_kernel<false>, dim3(grid), dim3(kEwThreads), 0, st, ga);
  HDP_CHECK_LAUNCH();
  return HDP_OK;
}

// scalar tail / unaligned fallback
__global__ void merge_scalar_kernel(void* W, int dt, const float* dW, int64_t begin, int64_t n) {
  for (int64_t i = begin + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    if (dt == HDP_F32) {
      reinterpret_cast<float*>(W)[i] += dW[i];
    } else {
      uint16_t* w = reinterpret_cast<uint16_t*>(W);
      w[i] = f32_to_bf16(bf16_to_f32(w[i]) + round_bf16(dW[i]));
    }
  }
}

// ---------------------------------------------------------------------------------------
// The grouped stream kernels behind one walk: the stochastic-rounding merge of hdp_sr.h, the compensated merge of
// hdp_comp.h, the grouped copy of the shard exchange's pack and scatter, and the float32 -> bf16 cast of the
// compute copies (compute_dtype=).
// (The round-to-nearest merges above keep their own kernels: through this walk they measured 2-6 % slower,
// DESIGN section 5.)  stream_group_kernel<Op>:
//   * one flat chunk space over a launch's items; a workgroup walks chunks blockIdx.x, + grid, ... and owns
//     Op::kU x 256 consecutive 16-byte vectors (of dst) at a time, every load of the chunk issued before its
//     first store, non-temporal both ways (each byte is touched once).  tools/merge_bw.hip on a 1 GiB
//     float32 slab: this form 5.76 TB/s (0.72 of 8) against 4.61 for a grid-stride loop with two vectors per
//     lane (profiles/r03_merge_bw_v2.txt);
//   * an item that can take vectors (hdp_stream_plan.h: dst and src 16-byte aligned; the copy: sitting alike
//     within 16 bytes, behind head bytes up to dst's boundary; SR: elem0 % 8 == 0 as well, one Philox block
//     per vector) has its head and tail units moved one per lane by its first chunk, so an item shorter than
//     one vector still owns that chunk;
//   * any other item runs unit by unit over the same chunk walk, in the same launch, with the same bits.
// An Op is its plan (item type, cap, kU, kVec, split) plus the arithmetic: vec_chunk for a lane's kU vectors
// of one chunk, load1 / store1 for one unit (edge lanes and unit-by-unit items).  SR costs ~40 32-bit multiplies and ~60 other VALU operations per 64 bytes of traffic.
// ---------------------------------------------------------------------------------------
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
template <class T>
__device__ __forceinline__ HDP_GLOBAL T* gptr_as(void* p) { return gptr(reinterpret_cast<T*>(p)); }
template <class T>
__device__ __forceinline__ const HDP_GLOBAL T* gptr_as(const void* p) { return gptr(reinterpret_cast<const T*>(p)); }

// (inline, not __forceinline__: inlined ahead of the optimiser, hipcc makes one wide vector of a chunk's
// register arrays and waits for every load on its own -- 256 VGPRs for the copy against 70)
#define HDP_OP_FN static __device__ inline

// bf16 W = sr(float32(W) + dW) (contract in hdp_sr.h), 8 B per element: element j of an item has e = elem0 + j,
// a vector one Philox block
struct MergeSrOp : MergeSrPlan {
  struct Elem {
    uint16_t w;
    float d;
  };
  HDP_OP_FN SrKey key_of(const Item& it, const SrSeed& seed) {
    return SrKey{seed.lo, seed.hi, static_cast<uint32_t>(it.offset), static_cast<uint32_t>(it.offset >> 32)};
  }
  HDP_OP_FN Elem load1(const Item& it, int64_t j) { return Elem{gptr_as<uint16_t>(it.W)[j], gptr(it.dW)[j]}; }
  HDP_OP_FN void store1(const Item& it, const SrSeed& seed, int64_t j, const Elem& e) {
    gptr_as<uint16_t>(it.W)[j] =
        sr_merge1(e.w, e.d, sr_r16(static_cast<uint64_t>(it.elem0) + static_cast<uint64_t>(j), key_of(it, seed)));
  }
  HDP_OP_FN void vec_chunk(const Item& it, const SrSeed& seed, const StreamSplit& sp, int64_t v0) {
    constexpr int U = kU;
    const int64_t nv = sp.nv;
    const uint64_t e0 = static_cast<uint64_t>(it.elem0);
    const SrKey key = key_of(it, seed);
    const HDP_GLOBAL f32x4* D4 = gptr_as<f32x4>(it.dW);
    HDP_GLOBAL u16x8* W8 = gptr_as<u16x8>(it.W);
    u16x8 w[U];
    f32x4 d0[U], d1[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = v0 + u * kEwThreads;
      if (i < nv) {
        d0[u] = __builtin_nontemporal_load(D4 + 2 * i);
        d1[u] = __builtin_nontemporal_load(D4 + 2 * i + 1);
        w[u] = __builtin_nontemporal_load(W8 + i);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = v0 + u * kEwThreads;
      if (i < nv) {
        const Philox4 rb = sr_block((e0 >> 3) + static_cast<uint64_t>(i), key);  // (elem0 % 8 == 0)
        const u32x4 wv = __builtin_bit_cast(u32x4, w[u]);
        u32x4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) {  // word k: elements 2k (low halves) and 2k + 1 (high halves)
          const f32x4& dd = k < 2 ? d0[u] : d1[u];
          const float s0 = __uint_as_float(wv[k] << 16) + dd[(2 * k) & 3];
          const float s1 = __uint_as_float(wv[k] & 0xffff0000u) + dd[(2 * k + 1) & 3];
          o[k] = sr_round(__float_as_uint(s0), rb.w[k] & 0xFFFFu) | (sr_round(__float_as_uint(s1), rb.w[k] >> 16) << 16);
        }
        __builtin_nontemporal_store(__builtin_bit_cast(u16x8, o), W8 + i);
      }
    }
  }
};

// bf16 (W, C) <- the compensated merge of float32 dW (contract in hdp_comp.h), 12 B per element: a vector is two
// 16-byte dW loads, one W load and one C load, then one W store and one C store
struct MergeCompOp : MergeCompPlan {
  struct Elem {
    uint16_t w, c;
    float d;
  };
  HDP_OP_FN Elem load1(const Item& it, int64_t j) {
    return Elem{gptr_as<uint16_t>(it.W)[j], gptr_as<uint16_t>(it.C)[j], gptr(it.dW)[j]};
  }
  HDP_OP_FN void store1(const Item& it, const NoKey&, int64_t j, const Elem& e) {
    const CompPair o = comp_merge1(e.w, e.c, e.d);
    gptr_as<uint16_t>(it.W)[j] = static_cast<uint16_t>(o.w);
    gptr_as<uint16_t>(it.C)[j] = static_cast<uint16_t>(o.c);
  }
  HDP_OP_FN void vec_chunk(const Item& it, const NoKey&, const StreamSplit& sp, int64_t v0) {
    constexpr int U = kU;
    const int64_t nv = sp.nv;
    const HDP_GLOBAL f32x4* D4 = gptr_as<f32x4>(it.dW);
    HDP_GLOBAL u32x4* W8 = gptr_as<u32x4>(it.W);
    HDP_GLOBAL u32x4* C8 = gptr_as<u32x4>(it.C);
    u32x4 w[U], cc[U];
    f32x4 d0[U], d1[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = v0 + u * kEwThreads;
      if (i < nv) {
        d0[u] = __builtin_nontemporal_load(D4 + 2 * i);
        d1[u] = __builtin_nontemporal_load(D4 + 2 * i + 1);
        w[u] = __builtin_nontemporal_load(W8 + i);
        cc[u] = __builtin_nontemporal_load(C8 + i);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = v0 + u * kEwThreads;
      if (i < nv) {
        u32x4 ow, oc;
#pragma unroll
        for (int k = 0; k < 4; ++k) {  // word k: elements 2k (low halves) and 2k + 1 (high halves)
          const f32x4& dd = k < 2 ? d0[u] : d1[u];
          const CompPair lo = comp_merge_f(__uint_as_float(w[u][k] << 16), __uint_as_float(cc[u][k] << 16), dd[(2 * k) & 3]);
          const CompPair hi = comp_merge_f(__uint_as_float(w[u][k] & 0xffff0000u), __uint_as_float(cc[u][k] & 0xffff0000u),
                                           dd[(2 * k + 1) & 3]);
          ow[k] = lo.w | (hi.w << 16);
          oc[k] = lo.c | (hi.c << 16);
        }
        __builtin_nontemporal_store(ow, W8 + i);
        __builtin_nontemporal_store(oc, C8 + i);
      }
    }
  }
};

// dst <- src, bytes
struct CopyOp : CopyPlan {
  using Elem = uint8_t;
  HDP_OP_FN Elem load1(const Item& it, int64_t j) { return gptr_as<uint8_t>(it.src)[j]; }
  HDP_OP_FN void store1(const Item& it, const NoKey&, int64_t j, Elem x) { gptr_as<uint8_t>(it.dst)[j] = x; }
  HDP_OP_FN void vec_chunk(const Item& it, const NoKey&, const StreamSplit& sp, int64_t v0) {
    HDP_GLOBAL u32x4* D4 = reinterpret_cast<HDP_GLOBAL u32x4*>(gptr_as<uint8_t>(it.dst) + sp.head);
    const HDP_GLOBAL u32x4* S4 = reinterpret_cast<const HDP_GLOBAL u32x4*>(gptr_as<uint8_t>(it.src) + sp.head);
    u32x4 x[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int64_t i = v0 + u * kEwThreads;
      if (i < sp.nv) x[u] = __builtin_nontemporal_load(S4 + i);
    }
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int64_t i = v0 + u * kEwThreads;
      if (i < sp.nv) __builtin_nontemporal_store(x[u], D4 + i);
    }
  }
};

// bf16 dst <- f32_to_bf16(float32 src), 6 B per element: two 16-byte loads and one 16-byte store per vector
struct ShadowOp : ShadowPlan {
  using Elem = float;
  HDP_OP_FN Elem load1(const Item& it, int64_t j) { return gptr(it.src)[j]; }
  HDP_OP_FN void store1(const Item& it, const NoKey&, int64_t j, Elem x) { gptr_as<uint16_t>(it.dst)[j] = f32_to_bf16(x); }
  HDP_OP_FN void vec_chunk(const Item& it, const NoKey&, const StreamSplit& sp, int64_t v0) {
    HDP_GLOBAL u32x4* D8 = gptr_as<u32x4>(it.dst);
    const HDP_GLOBAL f32x4* S4 = gptr_as<f32x4>(it.src);
    f32x4 x0[kU], x1[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int64_t i = v0 + u * kEwThreads;
      if (i < sp.nv) {
        x0[u] = __builtin_nontemporal_load(S4 + 2 * i);
        x1[u] = __builtin_nontemporal_load(S4 + 2 * i + 1);
      }
    }
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int64_t i = v0 + u * kEwThreads;
      if (i < sp.nv) {
        const u32x4 o{(uint32_t)f32_to_bf16(x0[u][0]) | ((uint32_t)f32_to_bf16(x0[u][1]) << 16),
                      (uint32_t)f32_to_bf16(x0[u][2]) | ((uint32_t)f32_to_bf16(x0[u][3]) << 16),
                      (uint32_t)f32_to_bf16(x1[u][0]) | ((uint32_t)f32_to_bf16(x1[u][1]) << 16),
                      (uint32_t)f32_to_bf16(x1[u][2]) | ((uint32_t)f32_to_bf16(x1[u][3]) << 16)};
        __builtin_nontemporal_store(o, D8 + i);
      }
    }
  }
};
#undef HDP_OP_FN

template <class Op>
__global__ __launch_bounds__(kEwThreads) void stream_group_kernel(StreamArgs<Op> ga) {
  constexpr int64_t CH = (int64_t)kEwThreads * Op::kU;  // vectors per chunk
  int it = 0;
  StreamSplit sp = Op::split(ga.it[0]);
  int64_t base = 0;                                     // item it owns chunks [base, base + sp.nch)
  for (int64_t c = blockIdx.x;; c += gridDim.x) {      // c, it, base, sp: workgroup-uniform
    while (c >= base + sp.nch) {
      base += sp.nch;
      if (++it == ga.n) return;
      sp = Op::split(ga.it[it]);
    }
    const typename Op::Item& item = ga.it[it];
    const int64_t n = Op::count(item);
    if (!sp.vec) {  // unit by unit over the chunk
      // (x is zeroed for every step: left unwritten where i >= n, hipcc carries its registers round the chunk
      // loop and costs registers on the vector path)
      constexpr int N = Op::kElemU;
      static_assert(Op::kU * Op::kVec % N == 0, "whole steps per chunk");
      const int64_t e0 = (c - base) * CH * Op::kVec + threadIdx.x;
#pragma nounroll
      for (int64_t o = 0; o < CH * Op::kVec; o += (int64_t)kEwThreads * N) {
        typename Op::Elem x[N] = {};
#pragma unroll
        for (int u = 0; u < N; ++u) {
          const int64_t i = e0 + o + u * kEwThreads;
          if (i < n) x[u] = Op::load1(item, i);
        }
#pragma unroll
        for (int u = 0; u < N; ++u) {
          const int64_t i = e0 + o + u * kEwThreads;
          if (i < n) Op::store1(item, ga.key, i, x[u]);
        }
      }
      continue;
    }
    Op::vec_chunk(item, ga.key, sp, (c - base) * CH + threadIdx.x);
    if (c == base) {  // the item's first chunk: head and tail units, one per lane
      const int64_t j = stream_edge_unit<Op>(sp, threadIdx.x, n);
      if (j >= 0) Op::store1(item, ga.key, j, Op::load1(item, j));
    }
  }
}

// every item checked before the first launch, then one launch per Op::kCap non-empty items
template <class Op>
static int stream_group_run(const char* who, int kid, int n, const typename Op::Item* items, const typename Op::Key& key,
                            void* stream) {
  char err[192];
  if (!stream_check<Op>(who, n, items, err, sizeof(err))) {
    set_error("%s", err);
    return HDP_EINVAL;
  }
  hipStream_t st = as_stream(stream);
  return stream_batch<Op>(n, items, key, [&](const StreamArgs<Op>& ga, int64_t chunks, double bytes) -> int {
    {
      KTimer kt(kid, st, bytes);
      hipLaunchKernelGGL(stream_group_kernel<Op>, dim3(stream_grid(chunks)), dim3(kEwThreads), 0, st, ga);
    }
    HDP_CHECK_LAUNCH();
    return HDP_OK;
  });
}

// ---------------------------------------------------------------------------------------
// Rank-ordered bf16 fold (hp:389-392 for a bf16 model): out = 0; out = bf16(out + parts[i]) for
// i = 0 .. nparts - 1, one 4-element vector per lane and grid-stride; the parts are read once.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(kEwThreads) void fold_bf16_kernel(const float* __restrict__ parts, int nparts,
                                                                int64_t stride, uint16_t* __restrict__ out,
                                                                int64_t n, int vec) {
  const int64_t nv = vec ? n / 4 : 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (int64_t)gridDim.x * blockDim.x) {
    float run[4] = {0.f, 0.f, 0.f, 0.f};
    for (int p = 0; p < nparts; ++p) {
      const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const HDP_GLOBAL f32x4*>(gptr(parts + p * stride)) + i);
#pragma unroll
      for (int q = 0; q < 4; ++q) run[q] = bf16_to_f32(f32_to_bf16(run[q] + v[q]));
    }
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    const u32x2 o{(uint32_t)f32_to_bf16(run[0]) | ((uint32_t)f32_to_bf16(run[1]) << 16),
                  (uint32_t)f32_to_bf16(run[2]) | ((uint32_t)f32_to_bf16(run[3]) << 16)};
    *reinterpret_cast<HDP_GLOBAL u32x2*>(gptr(out + 4 * i)) = o;
  }
  for (int64_t e = 4 * nv + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
    float run = 0.f;
    for (int p = 0; p < nparts; ++p) run = bf16_to_f32(f32_to_bf16(run + parts[p * stride + e]));
    out[e] = f32_to_bf16(run);
  }
}

// ---------------------------------------------------------------------------------------
// Adam on factors.  Every operation is rounded separately (contract(off) on plain operators:
// HIP's __fmul_rn / __fadd_rn are header-scope * and + that hipcc still fuses into FMAs) so the
// float32 result follows torch's op-by-op evaluation of hp:356-373 (AdamScalars, adam1 and
// adam_refused live in hdp_common.h: K4's fused Adam + H2 pack runs the same arithmetic).
// ---------------------------------------------------------------------------------------
// The probe's hand-off error word: the step's host check sees only probe launches that
// have completed, so the last groups of the accumulation window may still be running when it passes.
// Adam reads the word in stream order: while it is set the update is refused on the device -- m and v
// stay as they were and delta is written as 0, so the K4 / K5 merge that follows adds exactly 0 to
// W_res -- and the next flush / step raises on the host.

// contiguous chunks of kAdamU x 256 vectors per workgroup step (the merge's form: every load of the
// chunk issued before its stores)
constexpr int kAdamU = 2;
// CLIP: under a clip record (hdp_clip_state) -- its skip flag joins the refusal and its coefficient
// scales the gradient (adam1_clip); without one the kernel is the instruction sequence it always was
template <bool ZERO, bool CLIP>
__global__ __launch_bounds__(kEwThreads) void adam_kernel(float* __restrict__ grad, float* __restrict__ m,
                                                          float* __restrict__ v, float* __restrict__ delta,
                                                          int64_t n4, AdamScalars s, const int* err,
                                                          const hdp_clip_state* clip) {
  constexpr int64_t CH = (int64_t)kEwThreads * kAdamU;
  bool refused = adam_refused(err);
  float coef = 1.f;
  if constexpr (CLIP) refused |= clip_read(clip, coef);
  HDP_GLOBAL f32x4* G = reinterpret_cast<HDP_GLOBAL f32x4*>(gptr(grad));
  HDP_GLOBAL f32x4* M = reinterpret_cast<HDP_GLOBAL f32x4*>(gptr(m));
  HDP_GLOBAL f32x4* V = reinterpret_cast<HDP_GLOBAL f32x4*>(gptr(v));
  HDP_GLOBAL f32x4* D = reinterpret_cast<HDP_GLOBAL f32x4*>(gptr(delta));
  for (int64_t c = (int64_t)blockIdx.x * CH; c < n4; c += (int64_t)gridDim.x * CH) {
    f32x4 g[kAdamU], mm[kAdamU], vv[kAdamU];
#pragma unroll
    for (int u = 0; u < kAdamU; ++u) {
      const int64_t i = c + u * kEwThreads + threadIdx.x;
      if (i < n4) {
        g[u] = G[i];
        mm[u] = M[i];
        vv[u] = V[i];
      }
    }
#pragma unroll
    for (int u = 0; u < kAdamU; ++u) {
      const int64_t i = c + u * kEwThreads + threadIdx.x;
      if (i >= n4) continue;
      if (refused) {
        D[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (ZERO) G[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        continue;
      }
      f32x4 dd;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float gq = g[u][q], mq = mm[u][q], vq = vv[u][q], dq;
        if constexpr (CLIP) adam1_clip(gq, mq, vq, dq, s, coef);
        else adam1(gq, mq, vq, dq, s);
        mm[u][q] = mq;
        vv[u][q] = vq;
        dd[q] = dq;
      }
      M[i] = mm[u];
      V[i] = vv[u];
      D[i] = dd;
      if (ZERO) G[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }
}

template <bool CLIP>
__global__ void adam_scalar_kernel(float* grad, float* m, float* v, float* delta, int64_t begin,
                                   int64_t n, AdamScalars s, int zero, const int* err,
                                   const hdp_clip_state* clip) {
  bool refused = adam_refused(err);
  float coef = 1.f;
  if constexpr (CLIP) refused |= clip_read(clip, coef);
  for (int64_t i = begin + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    if (refused) {
      delta[i] = 0.f;
      if (zero) grad[i] = 0.f;
      continue;
    }
    float g = grad[i], mq = m[i], vq = v[i], d;
    if constexpr (CLIP) adam1_clip(g, mq, vq, d, s, coef);
    else adam1(g, mq, vq, d, s);
    m[i] = mq;
    v[i] = vq;
    delta[i] = d;
    if (zero) grad[i] = 0.f;
  }
}

// ---------------------------------------------------------------------------------------
// Global gradient norm (hdp_grad_sumsq / hdp_clip_finish): sum of double(float32(g * grad_scale))^2 over
// an arena.  A streaming read in K3's form -- a workgroup owns kSumsqU x 256 consecutive 16-byte vectors
// at a time, every load of the chunk issued before its first use, non-temporal (each byte is read once
// here; K3 reads it again, from HBM either way at arena sizes) -- with one float64 accumulator per lane.
// The lanes are reduced in a fixed order (xor butterfly over the wave, then the 4 waves through LDS in
// wave order) and every workgroup writes ONE partial to its own workspace slot: no atomics, the same
// bits on every run.  A float32 square would underflow for raw gradients and overflow for gs ~ 1e25;
// the float64 square of a float32 does neither.
// ---------------------------------------------------------------------------------------
constexpr int kSumsqU = 2;               // vectors per lane per chunk (K3's)
constexpr int kSumsqScalarBlocks = 64;   // scalar kernel (unaligned base / n % 4 tail): slots of its own

__device__ __forceinline__ double sumsq_block_reduce(double acc, double* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(kEwThreads) void grad_sumsq_kernel(const float* __restrict__ grad, int64_t n4,
                                                                float grad_scale, double* __restrict__ part) {
#pragma clang fp contract(off)
  constexpr int64_t CH = (int64_t)kEwThreads * kSumsqU;
  __shared__ double red[kEwThreads / 64];
  const HDP_GLOBAL f32x4* G = reinterpret_cast<const HDP_GLOBAL f32x4*>(gptr(grad));
  double acc = 0.0;
  for (int64_t c = (int64_t)blockIdx.x * CH; c < n4; c += (int64_t)gridDim.x * CH) {
    f32x4 g[kSumsqU];
#pragma unroll
    for (int u = 0; u < kSumsqU; ++u) {
      const int64_t i = c + u * kEwThreads + threadIdx.x;
      g[u] = i < n4 ? __builtin_nontemporal_load(G + i) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int u = 0; u < kSumsqU; ++u)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const double gs = (double)(g[u][q] * grad_scale);  // the float32 product K3 forms, then widened
        acc += gs * gs;
      }
  }
  const double tot = sumsq_block_reduce(acc, red);
  if (threadIdx.x == 0) *gptr(part + blockIdx.x) = tot;
}

__global__ __launch_bounds__(kEwThreads) void grad_sumsq_scalar_kernel(const float* __restrict__ grad, int64_t begin,
                                                                       int64_t n, float grad_scale,
                                                                       double* __restrict__ part) {
#pragma clang fp contract(off)
  __shared__ double red[kEwThreads / 64];
  double acc = 0.0;
  for (int64_t i = begin + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const double gs = (double)(grad[i] * grad_scale);
    acc += gs * gs;
  }
  const double tot = sumsq_block_reduce(acc, red);
  if (threadIdx.x == 0) part[blockIdx.x] = tot;
}

// vals[0] + vals[1] + ... in index order, one workgroup of kEwThreads; the result is thread 0's.  The
// workgroup stages kSumTile values at a time in LDS with coalesced loads and thread 0 adds them from there:
// a serial loop over global memory pays one HBM round trip per value (2048 partials: ~0.1 ms, more than the
// streaming kernel takes over a 40 M arena)
constexpr int kSumTile = 2048;
__device__ __forceinline__ double ordered_sum(const double* __restrict__ vals, int n, double* lds) {
#pragma clang fp contract(off)
  double s = 0.0;
  for (int base = 0; base < n; base += kSumTile) {  // (workgroup-uniform)
    const int cnt = n - base < kSumTile ? n - base : kSumTile;
    for (int i = threadIdx.x; i < cnt; i += kEwThreads) lds[i] = vals[base + i];
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll 8
      for (int i = 0; i < cnt; ++i) s += lds[i];
    }
    __syncthreads();
  }
  return s;
}

// out[0] = vals[0] + vals[1] + ... in index order (the per-workgroup partials: at most 2048 + 64)
__global__ __launch_bounds__(kEwThreads) void sum_f64_kernel(const double* __restrict__ vals, int n,
                                                             double* __restrict__ out) {
  __shared__ double lds[kSumTile];
  const double s = ordered_sum(vals, n, lds);
  if (threadIdx.x == 0) *out = s;
}

// the clip record from the per-arena / per-rank sums, added in index order (one workgroup)
__global__ __launch_bounds__(kEwThreads) void clip_finish_kernel(const double* __restrict__ sums, int n,
                                                                 float max_norm, hdp_clip_state* st) {
#pragma clang fp contract(off)
  __shared__ double lds[kSumTile];
  const double s = ordered_sum(sums, n, lds);
  if (threadIdx.x != 0) return;
  const bool skip = !(fabs(s) <= 1.7976931348623157e308);  // inf or NaN
  const float norm = (float)sqrt(s);                           // IEEE sqrt, then one rounding to float32
  const float q = max_norm / (norm + 1e-6f);                   // IEEE float32 division
  st->sumsq = s;
  st->norm = norm;
  st->coef = skip ? 1.f : (q < 1.0f ? q : 1.0f);
  st->skip = skip ? 1 : 0;
  st->skipped_total += skip ? 1 : 0;
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace hdp

using namespace hdp;

extern "C" int hdp_merge(void* W, int w_dtype, const float* dW, int64_t n, void* stream) {
  HDP_CHECK_ARG(n >= 0, "hdp_merge: n < 0");
  HDP_CHECK_ARG(w_dtype == HDP_F32 || w_dtype == HDP_BF16, "hdp_merge: bad dtype %d", w_dtype);
  if (n == 0) return HDP_OK;
  HDP_CHECK_ARG(W && dW, "hdp_merge: null pointer");
  hipStream_t st = as_stream(stream);
  int64_t done = 0;
  const bool al = aligned16(W) && aligned16(dW);
  if (al) {
    const int64_t vec = w_dtype == HDP_F32 ? 4 : 8;
    MergeGroupArgs ga;
    ga.n = 1;
    ga.W[0] = W;
    ga.dW[0] = dW;
    ga.nv[0] = n / vec;
    if (ga.nv[0]) {
      const int rc = merge_chunk_launch(ga, w_dtype == HDP_BF16, (w_dtype == HDP_F32 ? 12.0 : 8.0) * vec * ga.nv[0], st);
      if (rc) return rc;
    }
    done = ga.nv[0] * vec;
  }
  if (done < n) {
    const int64_t rest = n - done;
    int blocks = (int)((rest + 255) / 256);
    if (blocks > 2048) blocks = 2048;
    {
      KTimer kt(K_MERGE, st, (w_dtype == HDP_F32 ? 12.0 : 8.0) * rest);
      hipLaunchKernelGGL(merge_scalar_kernel, dim3(blocks), dim3(256), 0, st, W, w_dtype, dW, done, n);
    }
    HDP_CHECK_LAUNCH();
  }
  return HDP_OK;
}

// every item of a merge list before the first launch: the merges work on W in place
static int merge_items_check(const char* who, int n, const hdp_merge_item* items) {
  HDP_CHECK_ARG(n >= 0 && (n == 0 || items), "%s: bad item list", who);
  for (int i = 0; i < n; ++i) {
    HDP_CHECK_ARG(items[i].n >= 0, "%s: item %d has n < 0", who, i);
    HDP_CHECK_ARG(items[i].n == 0 || (items[i].W && items[i].dW), "%s: item %d has a null pointer", who, i);
  }
  return HDP_OK;
}

extern "C" int hdp_merge_group(int n, const hdp_merge_item* items, int w_dtype, void* stream) {
  if (const int rc = merge_items_check("hdp_merge_group", n, items)) return rc;
  HDP_CHECK_ARG(w_dtype == HDP_F32 || w_dtype == HDP_BF16, "hdp_merge_group: bad dtype %d", w_dtype);
  hipStream_t st = as_stream(stream);
  const int64_t vec = w_dtype == HDP_F32 ? 4 : 8;
  MergeGroupArgs ga;
  ga.n = 0;
  double bytes = 0;
  auto launch = [&]() -> int {
    if (ga.n == 0) return HDP_OK;
    const int rc = merge_chunk_launch(ga, w_dtype == HDP_BF16, bytes, st);
    ga.n = 0;
    bytes = 0;
    return rc;
  };
  for (int i = 0; i < n; ++i) {
    const hdp_merge_item& it = items[i];
    if (it.n == 0) continue;
    if (!aligned16(it.W) || !aligned16(it.dW) || it.n % vec != 0) {  // this item on its own
      const int rc = hdp_merge(it.W, w_dtype, it.dW, it.n, stream);
      if (rc) return rc;
      continue;
    }
    ga.W[ga.n] = it.W;
    ga.dW[ga.n] = it.dW;
    ga.nv[ga.n] = it.n / vec;
    bytes += (w_dtype == HDP_F32 ? 12.0 : 8.0) * it.n;
    if (++ga.n == kMergeGroupMax) {
      const int rc = launch();
      if (rc) return rc;
    }
  }
  return launch();
}

extern "C" int hdp_merge_group_bf16dw(int n, const hdp_merge_item* items, void* stream) {
  if (const int rc = merge_items_check("hdp_merge_group_bf16dw", n, items)) return rc;
  hipStream_t st = as_stream(stream);
  MergeGroupArgs ga;
  ga.n = 0;
  double bytes = 0;
  int64_t chunks = 0;
  constexpr int64_t CH = (int64_t)kEwThreads * kMergeU;
  auto launch = [&]() -> int {
    if (ga.n == 0) return HDP_OK;
    const unsigned grid = (unsigned)(chunks < kMergeGrid ? chunks : kMergeGrid);
    {
      KTimer kt(K_MERGE, st, bytes);
      hipLaunchKernelGGL(merge_bf16dw_kernel, dim3(grid), dim3(kEwThreads), 0, st, ga);
    }
    HDP_CHECK_LAUNCH();
    ga.n = 0;
    bytes = 0;
    chunks = 0;
    return HDP_OK;
  };
  for (int i = 0; i < n; ++i) {
    const hdp_merge_item& it = items[i];
    if (it.n == 0) continue;
    if (!aligned16(it.W) || !aligned16(it.dW) || it.n % 8 != 0) {  // this item element-wise
      int blocks = (int)((it.n + 255) / 256);
      if (blocks > 2048) blocks = 2048;
      {
        KTimer kt(K_MERGE, st, 6.0 * it.n);
        hipLaunchKernelGGL(merge_bf16dw_scalar_kernel, dim3(blocks), dim3(256), 0, st,
                           reinterpret_cast<uint16_t*>(it.W), reinterpret_cast<const uint16_t*>(it.dW), it.n);
      }
      HDP_CHECK_LAUNCH();
      continue;
    }
    ga.W[ga.n] = it.W;
    ga.dW[ga.n] = it.dW;
    ga.nv[ga.n] = it.n / 8;
    chunks += (ga.nv[ga.n] + CH - 1) / CH;
    bytes += 6.0 * it.n;
    if (++ga.n == kMergeGroupMax) {
      const int rc = launch();
      if (rc) return rc;
    }
  }
  return launch();
}

extern "C" int hdp_merge_group_sr(int n, const hdp_merge_sr_item* items, uint64_t seed, void* stream) {
  const SrSeed key{static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32)};
  return stream_group_run<MergeSrOp>("hdp_merge_group_sr", K_MERGE_SR, n, items, key, stream);
}

extern "C" int hdp_merge_group_comp(int n, const hdp_merge_comp_item* items, void* stream) {
  return stream_group_run<MergeCompOp>("hdp_merge_group_comp", K_MERGE_COMP, n, items, NoKey{}, stream);
}

extern "C" int hdp_copy_group(int n, const hdp_copy_item* items, void* stream) {
  return stream_group_run<CopyOp>("hdp_copy_group", K_COPY, n, items, NoKey{}, stream);
}

extern "C" int hdp_shadow_group(int n, const hdp_shadow_item* items, void* stream) {
  return stream_group_run<ShadowOp>("hdp_shadow_group", K_SHADOW, n, items, NoKey{}, stream);
}

static int adam_factors_impl(const char* who, float* grad, float* m, float* v, float* delta, int64_t n,
                             const AdamScalars& s, int zero_grad, const hdp_clip_state* clip, void* stream) {
  HDP_CHECK_ARG(n >= 0, "%s: n < 0", who);
  if (n == 0) return HDP_OK;
  HDP_CHECK_ARG(grad && m && v && delta, "%s: null pointer", who);
  HDP_CHECK_ARG(s.bc1 != 0.f && s.bc2 != 0.f, "%s: bias correction is zero (t == 0?)", who);
  hipStream_t st = as_stream(stream);
  const int* err = probe_err_device();
  int64_t done = 0;
  if (aligned16(grad) && aligned16(m) && aligned16(v) && aligned16(delta)) {
    const int64_t n4 = n / 4;
    if (n4) {
      KTimer kt(K_ADAM, st, 28.0 * 4 * n4);
      const dim3 grid(ew_grid(n4, kAdamU));
#define HDP_ADAM_LAUNCH(Z, C) \
  hipLaunchKernelGGL((adam_kernel<Z, C>), grid, dim3(kEwThreads), 0, st, grad, m, v, delta, n4, s, err, clip)
      if (clip) {
        if (zero_grad) HDP_ADAM_LAUNCH(true, true);
        else HDP_ADAM_LAUNCH(false, true);
      } else {
        if (zero_grad) HDP_ADAM_LAUNCH(true, false);
        else HDP_ADAM_LAUNCH(false, false);
      }
#undef HDP_ADAM_LAUNCH
      HDP_CHECK_LAUNCH();
    }
    done = n4 * 4;
  }
  if (done < n) {
    const int64_t rest = n - done;
    int blocks = (int)((rest + 255) / 256);
    if (blocks > 2048) blocks = 2048;
    {
      KTimer kt(K_ADAM, st, 28.0 * rest);
      if (clip)
        hipLaunchKernelGGL(adam_scalar_kernel<true>, dim3(blocks), dim3(256), 0, st, grad, m, v, delta, done, n, s,
                           zero_grad, err, clip);
      else
        hipLaunchKernelGGL(adam_scalar_kernel<false>, dim3(blocks), dim3(256), 0, st, grad, m, v, delta, done, n, s,
                           zero_grad, err, clip);
    }
    HDP_CHECK_LAUNCH();
  }
  return HDP_OK;
}

extern "C" int hdp_adam_factors(float* grad, float* m, float* v, float* delta, int64_t n,
                                float grad_scale, float beta1, float one_minus_beta1, float beta2,
                                float one_minus_beta2, float bc1, float bc2, float lr, float eps,
                                int zero_grad, void* stream) {
  const AdamScalars s{grad_scale, beta1, one_minus_beta1, beta2, one_minus_beta2, bc1, bc2, lr, eps};
  return adam_factors_impl("hdp_adam_factors", grad, m, v, delta, n, s, zero_grad, nullptr, stream);
}

extern "C" int hdp_adam_factors_clip(float* grad, float* m, float* v, float* delta, int64_t n,
                                     float grad_scale, float beta1, float one_minus_beta1, float beta2,
                                     float one_minus_beta2, float bc1, float bc2, float lr, float eps,
                                     int zero_grad, const hdp_clip_state* clip, void* stream) {
  const AdamScalars s{grad_scale, beta1, one_minus_beta1, beta2, one_minus_beta2, bc1, bc2, lr, eps};
  return adam_factors_impl("hdp_adam_factors_clip", grad, m, v, delta, n, s, zero_grad, clip, stream);
}

// workspace: one double per workgroup of the vector kernel (at most ew_grid's 2048), then one per
// workgroup of the scalar kernel
static int sumsq_slots(int64_t n, int* vec_slots) {
  const int64_t n4 = n / 4;
  const int vs = n4 ? ew_grid(n4, kSumsqU) : 0;
  if (vec_slots) *vec_slots = vs;
  return vs + kSumsqScalarBlocks;
}

extern "C" size_t hdp_grad_sumsq_workspace_bytes(int64_t n) {
  return n > 0 ? sizeof(double) * (size_t)sumsq_slots(n, nullptr) : 0;
}

extern "C" int hdp_grad_sumsq(const float* grad, int64_t n, float grad_scale, double* out_sum, void* workspace,
                              size_t workspace_bytes, void* stream) {
  HDP_CHECK_ARG(n >= 0, "hdp_grad_sumsq: n < 0");
  HDP_CHECK_ARG(out_sum && (reinterpret_cast<uintptr_t>(out_sum) & 7u) == 0,
                "hdp_grad_sumsq: null or misaligned out_sum");
  HDP_CHECK_ARG((reinterpret_cast<uintptr_t>(grad) & 3u) == 0, "hdp_grad_sumsq: grad not 4-byte aligned");
  HDP_CHECK_ARG(n == 0 || grad, "hdp_grad_sumsq: null grad");
  HDP_CHECK_ARG(n == 0 || (workspace && workspace_bytes >= hdp_grad_sumsq_workspace_bytes(n)),
                "hdp_grad_sumsq: workspace of %zu bytes, need %zu", workspace_bytes,
                hdp_grad_sumsq_workspace_bytes(n));
  HDP_CHECK_ARG(n == 0 || (reinterpret_cast<uintptr_t>(workspace) & 7u) == 0, "hdp_grad_sumsq: workspace not 8-byte aligned");
  hipStream_t st = as_stream(stream);
  double* part = reinterpret_cast<double*>(workspace);
  int used = 0;
  int64_t done = 0;
  if (n > 0 && aligned16(grad)) {
    const int64_t n4 = n / 4;
    if (n4) {
      int vs = 0;
      sumsq_slots(n, &vs);
      KTimer kt(K_SUMSQ, st, 4.0 * 4 * n4);
      hipLaunchKernelGGL(grad_sumsq_kernel, dim3(vs), dim3(kEwThreads), 0, st, grad, n4, grad_scale, part);
      used = vs;
    }
    HDP_CHECK_LAUNCH();
    done = n4 * 4;
  }
  if (done < n) {
    const int64_t rest = n - done;
    int blocks = (int)((rest + kEwThreads - 1) / kEwThreads);
    if (blocks > kSumsqScalarBlocks) blocks = kSumsqScalarBlocks;
    {
      KTimer kt(K_SUMSQ, st, 4.0 * rest);
      hipLaunchKernelGGL(grad_sumsq_scalar_kernel, dim3(blocks), dim3(kEwThreads), 0, st, grad, done, n, grad_scale,
                         part + used);
    }
    HDP_CHECK_LAUNCH();
    used += blocks;
  }
  {
    KTimer kt(K_CLIP_FINISH, st, 8.0 * used);
    hipLaunchKernelGGL(sum_f64_kernel, dim3(1), dim3(kEwThreads), 0, st, part, used, out_sum);
  }
  HDP_CHECK_LAUNCH();
  return HDP_OK;
}

extern "C" int hdp_clip_finish(const double* sums, int nsums, float max_norm, hdp_clip_state* state, void* stream) {
  HDP_CHECK_ARG(nsums >= 0, "hdp_clip_finish: nsums < 0");
  HDP_CHECK_ARG(state, "hdp_clip_finish: null state");
  HDP_CHECK_ARG((reinterpret_cast<uintptr_t>(state) & 7u) == 0 && (reinterpret_cast<uintptr_t>(sums) & 7u) == 0,
                "hdp_clip_finish: state and sums must be 8-byte aligned");
  HDP_CHECK_ARG(nsums == 0 || sums, "hdp_clip_finish: null sums");
  HDP_CHECK_ARG(max_norm > 0.f, "hdp_clip_finish: max_norm must be > 0 (got %g)", (double)max_norm);
  hipStream_t st = as_stream(stream);
  {
    KTimer kt(K_CLIP_FINISH, st, 8.0 * nsums);
    hipLaunchKernelGGL(clip_finish_kernel, dim3(1), dim3(kEwThreads), 0, st, sums, nsums, max_norm, state);
  }
  HDP_CHECK_LAUNCH();
  return HDP_OK;
}

extern "C" int hdp_fold_bf16(const float* parts, int nparts, int64_t stride, void* out, int64_t n, void* stream) {
  HDP_CHECK_ARG(n >= 0 && nparts >= 1 && stride >= n, "hdp_fold_bf16: bad sizes (n=%lld nparts=%d stride=%lld)",
                (long long)n, nparts, (long long)stride);
  if (n == 0) return HDP_OK;
  HDP_CHECK_ARG(parts && out, "hdp_fold_bf16: null pointer");
  const int vec = aligned16(parts) && stride % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 7) == 0;
  int64_t blocks = ((vec ? n / 4 : n) + kEwThreads - 1) / kEwThreads;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  hipStream_t st = as_stream(stream);
  {
    KTimer kt(K_FOLD, st, (4.0 * nparts + 2.0) * n);
    hipLaunchKernelGGL(fold_bf16_kernel, dim3((unsigned)blocks), dim3(kEwThreads), 0, st, parts, nparts, stride,
                       reinterpret_cast<uint16_t*>(out), n, vec);
  }
  HDP_CHECK_LAUNCH();
  return HDP_OK;
}
