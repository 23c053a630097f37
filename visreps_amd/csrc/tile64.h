// The 64 x 64 fp64 tile pipeline of cov.hip (k_cov) and xcov.hip (k_xcov, k_xgemm_nt):
// G = A^T B over a slice of the contraction on the fp64 MFMA (v_mfma_f64_16x16x4_f64).
//
// 16-deep stages of the two operand panels are staged into LDS as doubles (entry (k, c) at
// k * T64_LD + c), double-buffered: load the next stage into registers, MFMA on the current one,
// store the next, barrier. 4 waves as 2 x 2, each 32 x 32. The contraction is split into S
// slices so small outputs still fill the chip; a slice writes its fp64 partial tile
// ([S][ntile][64 * 64]) and the kernel's reduce adds the slices in slice order (slice_sum): no
// floating-point atomics, bit-identical run to run.
//
// A kernel supplies how a stage is loaded and stored. Panels that are row-major along the
// contraction share panel_load / panel_store here. The loaders that are contiguous along the
// contraction (cov_load_t / cov_store_t / cov_store_t64 in cov.hip, xg_load / xg_store in
// xcov.hip) stay with their kernels: they hold different registers across the loop (float4,
// converted at the store, against double4, converted at the load).
#pragma once

#include "internal.h"

namespace vr {

constexpr int T64 = 64;              // tile edge
constexpr int T64_K = 16;            // contraction entries per stage
constexpr int T64_LD = T64 + 16;     // LDS row pitch (doubles): 4 k-rows of a fragment read hit 2 bank sets
constexpr int T64_THREADS = 256;
constexpr int T64_STAGE = T64_K * T64_LD;  // doubles per panel per stage

// this thread's 4 columns of a 16-row stage: row kr = tid >> 4, columns 4 (tid & 15).
// rows (nullable): position r of the contraction -> row of M
__device__ inline f32x4 panel_load(const float* M, int64_t ld, int64_t ncol, bool vec, const int32_t* rows,
                                   int64_t col0, int64_t k, int64_t k1) {
  const int kr = threadIdx.x >> 4, c = (threadIdx.x & 15) * 4;
  const int64_t r = k + kr;
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (r >= k1) return v;
  const int64_t row = rows != nullptr ? (int64_t)rows[r] : r;
  const float* src = M + row * ld + col0 + c;
  if (vec && col0 + c + 4 <= ncol) {
    v = *reinterpret_cast<const f32x4*>(src);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (col0 + c + e < ncol) ? src[e] : 0.f;
  }
  return v;
}

// ... centred about m, the means of the thread's 4 columns, while staged
__device__ inline void panel_store(double* lds, const f32x4 v, const double m[4], int64_t k, int64_t k1) {
  const int kr = threadIdx.x >> 4, c = (threadIdx.x & 15) * 4;
  const bool in = k + kr < k1;
  double* dst = lds + kr * T64_LD + c;
#pragma unroll
  for (int e = 0; e < 4; ++e) dst[e] = in ? (double)v[e] - m[e] : 0.0;  // padded rows add exact zeros
}

// The MFMAs of one LDS stage pair: A panel entry (k, i), B panel entry (k, j). Lane l supplies
// A[m = l & 15][k = l >> 4] and B[k = l >> 4][n = l & 15] (fm = l & 15, fk = l >> 4).
__device__ inline void mma_stage(const double* As, const double* Bs, int wr, int wc, int fk, int fm,
                                 f64x4 acc[2][2]) {
#pragma unroll
  for (int ks = 0; ks < T64_K / 4; ++ks) {
    const int kr = ks * 4 + fk;
    double a[2], b[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      a[m] = As[kr * T64_LD + wr * 32 + m * 16 + fm];
      b[m] = Bs[kr * T64_LD + wc * 32 + m * 16 + fm];
    }
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int nn = 0; nn < 2; ++nn)
        acc[m][nn] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[m], b[nn], acc[m][nn], 0, 0, 0);
  }
}

// C/D of the f64 MFMA: col = lane & 15, row = (lane >> 4) + 4 r
__device__ inline void store_tile(double* out, int wr, int wc, int fk, int fm, const f64x4 acc[2][2]) {
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int nn = 0; nn < 2; ++nn)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int li = wr * 32 + m * 16 + fk + 4 * r;
        const int lj = wc * 32 + nn * 16 + fm;
        out[li * T64 + lj] = acc[m][nn][r];
      }
}

// One workgroup's partial tile: nk stages from contraction position k0, stored to out
// ([64][64] doubles). load(side, k) returns this thread's registers of the stage at k of panel
// side (0: A, 1: B); store(side, dst, v, k) stages them. diag: both panels are the same (k_cov's
// diagonal tiles), only A is staged. lds: [buf][A/B]. An empty slice (nk = 0) stores an
// all-zero tile.
template <class Load, class Store>
__device__ inline void tile_pipeline(double (&lds)[2][2][T64_STAGE], int64_t k0, int nk, bool diag, Load load,
                                     Store store, double* out) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int wr = wid >> 1, wc = wid & 1;
  f64x4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = f64x4{0.0, 0.0, 0.0, 0.0};

  decltype(load(0, k0)) ga = {}, gb = ga;
  if (nk > 0) {
    ga = load(0, k0);
    if (!diag) gb = load(1, k0);
    store(0, lds[0][0], ga, k0);
    if (!diag) store(1, lds[0][1], gb, k0);
  }
  __syncthreads();
  const int fk = lane >> 4, fm = lane & 15;
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    const double* As = lds[cur][0];
    const double* Bs = diag ? As : lds[cur][1];
    const bool more = kt + 1 < nk;
    const int64_t kn = k0 + (int64_t)(kt + 1) * T64_K;
    if (more) {
      ga = load(0, kn);
      if (!diag) gb = load(1, kn);
    }
    mma_stage(As, Bs, wr, wc, fk, fm, acc);
    if (more) {
      store(0, lds[cur ^ 1][0], ga, kn);
      if (!diag) store(1, lds[cur ^ 1][1], gb, kn);
    }
    __syncthreads();
  }
  store_tile(out, wr, wc, fk, fm, acc);
}

// entry e of tile `tile`: its S slice partials added in slice order
__device__ inline double slice_sum(const double* partial, int S, int ntile, int tile, int e) {
  double s = 0.0;
  for (int q = 0; q < S; ++q) s += partial[((int64_t)q * ntile + tile) * (T64 * T64) + e];
  return s;
}

}  // namespace vr
