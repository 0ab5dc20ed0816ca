// K2 with adapter dropout (hp:139 with dropout > 0): the reference drops elements of the dense out x in
// product B A, so the factor gradients become
//   gA (+)= s/(1-p) B^T (M . D),   gB (+)= s/(1-p) (M . D) A^T,   D = G^T X  (out x in)
// with the keep mask M of hdp_philox.h.  D exists only tile by tile: a workgroup forms one 128 x 128 tile of
// D^T (rows i, columns o) on MFMA over all T tokens, masks the accumulators in registers (a lane holds four
// consecutive i of one o per register group: one Philox block), and contracts the masked tile from LDS
// against B and A on the f32 MFMA.  Partial sums go to the workspace (gA per out-tile, gB per in-tile) and
// a finish kernel folds them in tile order: no float atomics, bitwise reproducible.
#include "hdp_common.h"
#include "hdp_philox.h"

namespace hdp {
namespace {

constexpr int kTile = 128;   // D^T tile edge; 4 waves as 2 (i) x 2 (o), each 2 x 2 MFMA tiles of 32 x 32
constexpr int kThreads = 256;
constexpr int kGroupI = 8;   // tiles of 8 in-rows x all out-columns are adjacent in launch order (L2 reuse)
constexpr int kLds = 65536;  // the masked tile, 128 x 128 f32 (the staging buffers alias its start)

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// Staging of one k chunk of X and G, both [t][128 columns] as they lie in memory, in two LDS buffers (chunk c
// in buffer c & 1: one barrier per chunk).  float32: 32 t of 512-byte rows (an MFMA operand is one ds_read_b32
// per lane, lanes along the row).  bf16: 32 t of 320-byte rows: the four rows of a transposed read then start
// 16 banks apart (80 dwords mod 64), conflict-free.
template <int DT>
struct Stage;
template <>
struct Stage<HDP_F32> {
  static constexpr int ES = 4, EPV = 4, KC = 32, ROWB = 512;
};
template <>
struct Stage<HDP_BF16> {
  static constexpr int ES = 2, EPV = 8, KC = 32, ROWB = 320;
};

struct DropArgs {
  const void* X;
  const void* G;
  const float* A;
  const float* B;
  float* WA;  // [nOT][r][in]
  float* WB;  // [nIT][out][r]
  int64_t T, in, out;
  int r, b_transposed, nIT, nOT, vecx, vecg;
  DropoutKey key;
};

// 16 bytes of row `row` starting at column `col` (zero beyond the matrix).  `vec`: the row length is a whole
// number of 16-byte granules and the base is 16-byte aligned, so a column inside the row has its granule inside.
template <int DT>
__device__ __forceinline__ u32x4 ld16(const void* base, int64_t ld, int64_t row, int64_t col, int64_t nrows, int vec) {
  using S = Stage<DT>;
  u32x4 z = {0u, 0u, 0u, 0u};
  if (row >= nrows || col >= ld) return z;
  const int64_t idx = row * ld + col;
  if (vec) return *reinterpret_cast<const HDP_GLOBAL u32x4*>(gptr(reinterpret_cast<const char*>(base)) + idx * S::ES);
  uint32_t w[4] = {0u, 0u, 0u, 0u};
  if constexpr (DT == HDP_F32) {
    const HDP_GLOBAL uint32_t* p = gptr(reinterpret_cast<const uint32_t*>(base)) + idx;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (col + j < ld) w[j] = p[j];
  } else {
    const HDP_GLOBAL uint16_t* p = gptr(reinterpret_cast<const uint16_t*>(base)) + idx;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (col + j < ld) w[j >> 1] |= static_cast<uint32_t>(p[j]) << (16 * (j & 1));
  }
  return u32x4{w[0], w[1], w[2], w[3]};
}

// float index of element (o, i) of the masked tile in LDS.  The XOR keeps four consecutive i together (a
// lane's 16-byte store) and spreads both contractions' operand reads over the banks: a read along i at two
// neighbouring o, and a read along o at fixed i.
__device__ __forceinline__ int dm_idx(int o, int i) { return o * kTile + (i ^ (((o & 15) << 2) ^ ((o & 1) << 4))); }

template <int DT>
__global__ __launch_bounds__(kThreads) void probe_dropout_kernel(DropArgs a) {
  using S = Stage<DT>;
  __shared__ __attribute__((aligned(16))) char smem[kLds];
  constexpr int XSB = S::KC * S::ROWB;  // bytes of one operand's chunk
  constexpr int VPR = kTile / S::EPV;   // 16-byte granules per staged row
  constexpr int NV = S::KC * VPR / kThreads;  // granules per thread, operand and chunk
  static_assert(4 * XSB <= kLds && S::KC * VPR == NV * kThreads, "staging: two buffers of whole granules per thread");

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wi = wave >> 1, wo = wave & 1;
  const int l31 = lane & 31, h = lane >> 5;

  // tile of this workgroup: bands of kGroupI in-tiles, in-tile fastest inside a band
  const int ntiles = a.nIT * a.nOT;
  const int id = xcd_remap(static_cast<int>(blockIdx.x), ntiles);
  const int width = kGroupI * a.nOT;
  const int first = (id / width) * kGroupI;
  const int gsz = (a.nIT - first) < kGroupI ? (a.nIT - first) : kGroupI;
  const int it = first + (id % width) % gsz, ot = (id % width) / gsz;
  const int64_t ibase = static_cast<int64_t>(it) * kTile, obase = static_cast<int64_t>(ot) * kTile;

  u32x4 px[NV], pg[NV];
  auto fetch = [&](int64_t t0) {
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int v = tid + kThreads * j, row = v / VPR, cv = v % VPR;
      px[j] = ld16<DT>(a.X, a.in, t0 + row, ibase + cv * S::EPV, a.T, a.vecx);
      pg[j] = ld16<DT>(a.G, a.out, t0 + row, obase + cv * S::EPV, a.T, a.vecg);
    }
  };
  auto stash = [&](char* buf) {
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int v = tid + kThreads * j, row = v / VPR, cv = v % VPR;
      *reinterpret_cast<u32x4*>(buf + row * S::ROWB + cv * 16) = px[j];
      *reinterpret_cast<u32x4*>(buf + XSB + row * S::ROWB + cv * 16) = pg[j];
    }
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int no = 0; no < 2; ++no)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[mi][no][q] = 0.f;

  // ---- D^T tile: acc[mi][no] (i = 64 wi + 32 mi + row, o = 64 wo + 32 no + col) += X^T G over all t ----
  const int64_t nchunk = (a.T + S::KC - 1) / S::KC;
  fetch(0);
  for (int64_t c = 0; c < nchunk; ++c) {
    // a wave passes this barrier only after its reads of chunk c - 1, so chunk c + 1 may overwrite that buffer
    char* buf = smem + (c & 1) * 2 * XSB;
    stash(buf);
    __syncthreads();
    if (c + 1 < nchunk) fetch((c + 1) * S::KC);
    if constexpr (DT == HDP_F32) {
      // v_mfma_f32_32x32x2_f32: A[row i = l & 31][k = l >> 5] = X[t][i], B[k][col o = l & 31] = G[t][o]
      const float* xs = reinterpret_cast<const float*>(buf);
      const float* gs = reinterpret_cast<const float*>(buf + XSB);
#pragma unroll
      for (int k0 = 0; k0 < S::KC; k0 += 2) {
        const int row = (k0 + h) * kTile;
        float av[2], bv[2];
#pragma unroll
        for (int m = 0; m < 2; ++m) {
          av[m] = xs[row + wi * 64 + m * 32 + l31];
          bv[m] = gs[row + wo * 64 + m * 32 + l31];
        }
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
          for (int no = 0; no < 2; ++no)
            acc[mi][no] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[mi], bv[no], acc[mi][no], 0, 0, 0);
      }
    } else {
      // v_mfma_f32_32x32x16_bf16: lane (row / col = l & 31, half h) holds k = 8 h + 0..7, i.e. eight t of
      // one column of the staged [t][column] image: two transposed reads of 4 t x 16 columns per 16 lanes
      // (lane 4 q + p of a group addresses row q, columns 4 p .. 4 p + 3; lane n receives column n)
      typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
      const int n = lane & 15, q = n >> 2, p = n & 3, g1 = (lane >> 4) & 1;
#pragma unroll
      for (int k0 = 0; k0 < S::KC; k0 += 16) {
        const int rowb = (k0 + 8 * h + q) * S::ROWB;
        bf16x8 fa[2], fb[2];
#pragma unroll
        for (int m = 0; m < 2; ++m) {
          const int ca = (wi * 64 + m * 32 + 16 * g1 + 4 * p) * 2, cb = (wo * 64 + m * 32 + 16 * g1 + 4 * p) * 2;
          const s16x4 a0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(buf + rowb + ca));
          const s16x4 a1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(buf + rowb + 4 * S::ROWB + ca));
          const s16x4 b0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(buf + XSB + rowb + cb));
          const s16x4 b1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(buf + XSB + rowb + 4 * S::ROWB + cb));
          fa[m] = __builtin_bit_cast(bf16x8, (s16x8)__builtin_shufflevector(a0, a1, 0, 1, 2, 3, 4, 5, 6, 7));
          fb[m] = __builtin_bit_cast(bf16x8, (s16x8)__builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7));
        }
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
          for (int no = 0; no < 2; ++no)
            acc[mi][no] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[mi], fb[no], acc[mi][no], 0, 0, 0);
      }
    }
  }
  __syncthreads();  // the masked tile below aliases the staging buffers

  // ---- mask the accumulators, lay the tile out in LDS as [o][i] --------------------------------------
  // C/D map of the 32 x 32 forms: col = l & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (l >> 5): registers
  // 4 g .. 4 g + 3 of a lane are four consecutive i of one o
  HDP_MFMA_FENCE();
  float* dm = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int no = 0; no < 2; ++no) {
      const int ol = wo * 64 + no * 32 + l31;
      const int64_t o = obase + ol;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int il = wi * 64 + mi * 32 + 8 * g + 4 * h;
        const int64_t i4 = ibase + il;
        unsigned keep = 0u;
        if (o < a.out && i4 < a.in) keep = dropout_keep4(static_cast<uint64_t>(o) * static_cast<uint64_t>(a.in) + static_cast<uint64_t>(i4), a.key);
        f32x4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = ((keep >> j) & 1u) ? acc[mi][no][4 * g + j] : 0.f;
        *reinterpret_cast<f32x4*>(dm + dm_idx(ol, il)) = v;
      }
    }
  __syncthreads();

  // ---- the two skinny contractions of the masked tile on v_mfma_f32_16x16x4_f32 ------------------------
  // (A[row = l & 15][k = l >> 4], B[k = l >> 4][col = l & 15]; C/D col = l & 15, row = 4 (l >> 4) + reg)
  //   units 0 .. 8 nRB - 1:        PA[rho][i] = sum_o B[o][rho] Dm[o][i]   (16 rho x 16 i per unit)
  //   units 8 nRB .. 16 nRB - 1:   PB[o][rho] = sum_i Dm[o][i] A[rho][i]   (16 o x 16 rho per unit)
  const int nRB = (a.r + 15) >> 4;
  const int c16 = lane & 15, k4 = lane >> 4;
  for (int u = wave; u < 16 * nRB; u += 4) {
    f32x4 c0 = {0.f, 0.f, 0.f, 0.f}, c1 = {0.f, 0.f, 0.f, 0.f};
    if (u < 8 * nRB) {
      const int rb = u >> 3, ib = u & 7;
      const int rho = rb * 16 + c16;
#pragma unroll 4
      for (int k0 = 0; k0 < kTile; k0 += 8) {
        float av[2], bv[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const int ol = k0 + 4 * s + k4;
          const int64_t o = obase + ol;
          av[s] = 0.f;
          if (rho < a.r && o < a.out) av[s] = a.b_transposed ? gld1(a.B + static_cast<int64_t>(rho) * a.out + o) : gld1(a.B + o * a.r + rho);
          bv[s] = dm[dm_idx(ol, ib * 16 + c16)];
        }
        c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[0], bv[0], c0, 0, 0, 0);
        c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[1], bv[1], c1, 0, 0, 0);
      }
      HDP_MFMA_FENCE();
      const int64_t i = ibase + ib * 16 + c16;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int rr = rb * 16 + 4 * k4 + reg;
        if (rr < a.r && i < a.in) gst1(a.WA + (static_cast<int64_t>(ot) * a.r + rr) * a.in + i, c0[reg] + c1[reg]);
      }
    } else {
      const int v = u - 8 * nRB;
      const int ob = v / nRB, rb = v % nRB;
      const int rho = rb * 16 + c16;
#pragma unroll 4
      for (int k0 = 0; k0 < kTile; k0 += 8) {
        float av[2], bv[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const int il = k0 + 4 * s + k4;
          const int64_t i = ibase + il;
          av[s] = dm[dm_idx(ob * 16 + c16, il)];
          bv[s] = 0.f;
          if (rho < a.r && i < a.in) bv[s] = gld1(a.A + static_cast<int64_t>(rho) * a.in + i);
        }
        c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[0], bv[0], c0, 0, 0, 0);
        c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[1], bv[1], c1, 0, 0, 0);
      }
      HDP_MFMA_FENCE();
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int64_t o = obase + ob * 16 + 4 * k4 + reg;
        if (o < a.out && rho < a.r) gst1(a.WB + (static_cast<int64_t>(it) * a.out + o) * a.r + rho, c0[reg] + c1[reg]);
      }
    }
  }
}

// g[idx] (+)= scale * (W[0][idx] + W[1][idx] + ...), tile order; idx over gA (nA entries) then gB (nB)
__global__ __launch_bounds__(kThreads) void probe_dropout_finish_kernel(const float* WA, const float* WB, float* gA, float* gB,
                                                                      int64_t nA, int64_t nB, int nOT, int nIT, float scale,
                                                                      int accumulate) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (idx >= nA + nB) return;
  const bool isA = idx < nA;
  const int64_t k = isA ? idx : idx - nA, stride = isA ? nA : nB;
  const float* w = (isA ? WA : WB) + k;
  float* g = (isA ? gA : gB) + k;
  const int np = isA ? nOT : nIT;
  float s = 0.f;
  for (int t = 0; t < np; ++t) s += gld1(w + t * stride);
  const float v = scale * s;
  gst1(g, accumulate ? gld1(g) + v : v);
}

__global__ __launch_bounds__(kThreads) void dropout_mask_kernel(uint8_t* mask, int64_t n, DropoutKey key) {
  const int64_t e0 = (static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x) * 4;
  if (e0 >= n) return;
  const unsigned keep = dropout_keep4(static_cast<uint64_t>(e0), key);
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (e0 + j < n) mask[e0 + j] = static_cast<uint8_t>((keep >> j) & 1u);
}

inline int64_t tiles_of(int64_t n) { return (n + kTile - 1) / kTile; }

inline DropoutKey make_key(float p, uint64_t seed, uint64_t offset) {
  return DropoutKey{static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32), static_cast<uint32_t>(offset),
                    static_cast<uint32_t>(offset >> 32), dropout_threshold(p)};
}

}  // namespace
}  // namespace hdp

using namespace hdp;

extern "C" size_t hdp_probe_dropout_workspace_bytes(int64_t T, int64_t in, int64_t out, int r) {
  if (T <= 0 || in <= 0 || out <= 0 || r <= 0 || r > 128) return 0;
  const size_t fl = static_cast<size_t>(tiles_of(out)) * r * in + static_cast<size_t>(tiles_of(in)) * out * r;
  return (fl * sizeof(float) + 255) & ~static_cast<size_t>(255);
}

extern "C" int hdp_probe_grads_dropout(int64_t T, int64_t in, int64_t out, int r, const void* X, const void* G, int x_dtype,
                                       const float* A, const float* B, int b_transposed, float* gA, float* gB, float scale,
                                       int accumulate, float p, uint64_t seed, uint64_t offset, void* workspace,
                                       size_t workspace_bytes, void* stream) {
  HDP_CHECK_ARG(in > 0 && out > 0 && r > 0 && T >= 0, "hdp_probe_grads_dropout: bad shape");
  HDP_CHECK_ARG(r <= 128, "hdp_probe_grads_dropout: r = %d > 128 is not supported", r);
  HDP_CHECK_ARG(p > 0.f && p < 1.f, "hdp_probe_grads_dropout: p = %g is not inside (0, 1)", static_cast<double>(p));
  HDP_CHECK_ARG(x_dtype == HDP_F32 || x_dtype == HDP_BF16, "hdp_probe_grads_dropout: bad dtype %d", x_dtype);
  HDP_CHECK_ARG(A && B && gA && gB, "hdp_probe_grads_dropout: null pointer");
  const int64_t nIT = tiles_of(in), nOT = tiles_of(out);
  HDP_CHECK_ARG(nIT * nOT < (1ll << 31) && static_cast<int64_t>(r) * (in + out) < (1ll << 38),
                "hdp_probe_grads_dropout: shape too large");
  hipStream_t st = as_stream(stream);
  const int64_t nA = static_cast<int64_t>(r) * in, nB = out * static_cast<int64_t>(r);
  if (T == 0) {
    if (!accumulate) {
      HDP_CHECK_HIP(hipMemsetAsync(gA, 0, sizeof(float) * nA, st));
      HDP_CHECK_HIP(hipMemsetAsync(gB, 0, sizeof(float) * nB, st));
    }
    return HDP_OK;
  }
  HDP_CHECK_ARG(X && G && workspace, "hdp_probe_grads_dropout: null pointer");
  HDP_CHECK_ARG((reinterpret_cast<uintptr_t>(A) & 15) == 0 && (reinterpret_cast<uintptr_t>(X) & 15) == 0 &&
                    (reinterpret_cast<uintptr_t>(G) & 15) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0 &&
                    (!b_transposed || (reinterpret_cast<uintptr_t>(B) & 15) == 0),
                "hdp_probe_grads_dropout: X, G, A, the workspace (and B^T) must be 16-byte aligned");
  const size_t need = hdp_probe_dropout_workspace_bytes(T, in, out, r);
  HDP_CHECK_ARG(need <= workspace_bytes, "hdp_probe_grads_dropout: workspace %zu bytes too small (need %zu)",
                workspace_bytes, need);
  const int epv = x_dtype == HDP_F32 ? 4 : 8;
  const double es = x_dtype == HDP_F32 ? 4.0 : 2.0;
  DropArgs a{};
  a.X = X;
  a.G = G;
  a.A = A;
  a.B = B;
  a.WA = static_cast<float*>(workspace);
  a.WB = a.WA + nOT * nA;
  a.T = T;
  a.in = in;
  a.out = out;
  a.r = r;
  a.b_transposed = b_transposed ? 1 : 0;
  a.nIT = static_cast<int>(nIT);
  a.nOT = static_cast<int>(nOT);
  a.vecx = in % epv == 0;
  a.vecg = out % epv == 0;
  a.key = make_key(p, seed, offset);
  const double part = 4.0 * (static_cast<double>(nOT) * nA + static_cast<double>(nIT) * nB);
  {
    KTimer kt(K_PROBE_DROPOUT, st, es * T * (in + out) + 4.0 * (nA + nB) + part,
              2.0 * T * in * out + 4.0 * r * static_cast<double>(in) * out);
    if (x_dtype == HDP_F32)
      hipLaunchKernelGGL(probe_dropout_kernel<HDP_F32>, dim3(static_cast<unsigned>(nIT * nOT)), dim3(kThreads), 0, st, a);
    else
      hipLaunchKernelGGL(probe_dropout_kernel<HDP_BF16>, dim3(static_cast<unsigned>(nIT * nOT)), dim3(kThreads), 0, st, a);
  }
  HDP_CHECK_LAUNCH();
  {
    KTimer kt(K_PROBE_DROPOUT_FINISH, st, part + 4.0 * (nA + nB) * (accumulate ? 2.0 : 1.0),
              static_cast<double>(nOT) * nA + static_cast<double>(nIT) * nB);
    hipLaunchKernelGGL(probe_dropout_finish_kernel, dim3(static_cast<unsigned>((nA + nB + kThreads - 1) / kThreads)),
                       dim3(kThreads), 0, st, a.WA, a.WB, gA, gB, nA, nB, a.nOT, a.nIT, scale / (1.0f - p),
                       accumulate ? 1 : 0);
  }
  HDP_CHECK_LAUNCH();
  HDP_POST_LAUNCH(st);
  return HDP_OK;
}

extern "C" int hdp_dropout_mask(int64_t out, int64_t in, float p, uint64_t seed, uint64_t offset, uint8_t* mask,
                                void* stream) {
  HDP_CHECK_ARG(in > 0 && out > 0, "hdp_dropout_mask: bad shape");
  HDP_CHECK_ARG(p > 0.f && p < 1.f, "hdp_dropout_mask: p = %g is not inside (0, 1)", static_cast<double>(p));
  HDP_CHECK_ARG(mask, "hdp_dropout_mask: null pointer");
  HDP_CHECK_ARG(out < (1ll << 40) / in, "hdp_dropout_mask: shape too large");
  const int64_t n = out * in;
  const int64_t blocks = ((n + 3) / 4 + kThreads - 1) / kThreads;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(dropout_mask_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, st, mask, n,
                     make_key(p, seed, offset));
  HDP_CHECK_LAUNCH();
  HDP_POST_LAUNCH(st);
  return HDP_OK;
}
