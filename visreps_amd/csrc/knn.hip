// Two nearest neighbours of every row of X (n x d, fp32), exact: the kernel behind the Facco
// Two-NN intrinsic dimensionality (the reference's analysis/compute_twoNN_ID.py:27-78),
//   r1 <= r2 the two smallest Euclidean distances from a row to the other rows, ID = 1 / mean log(r2 / r1).
// A fast fp32-MFMA candidate search, a certificate, and an exact fp64 scan where the certificate
// cannot hold. The n x n distance matrix never exists.
//
// k_knn_colsum / k_knn_colmean   fp64 column sums (row chunks added in chunk order), mean rounded to fp32.
// k_knn_stage   y = fl32(x - mean) into a scratch copy padded with zeros to 128 rows x 32 columns
//               (distances are translation-invariant; post-ReLU activations share a large offset),
//               and the fp64 squared norms a_i of the staged rows. X is never written.
// k_knn_amax    the largest norm (NaN sticks).
// k_knn_cand    the tiling of k_gram (rdm.hip): 128 x 128 tiles, double-buffered LDS panels of 32 k,
//               four waves as 2 x 2, v_mfma_f32_32x32x2_f32. A workgroup owns 128 query points as
//               the tile's columns and walks a range of row tiles; the tile
//                 s~_ij = fl32(fl32(a_i + a_j) - 2 g~_ij)
//               is not stored: in the 32 x 32 C/D layout a lane owns one column and 16 of its rows,
//               so each lane keeps, for each of its two columns, the KN_C + 1 smallest s~ over the
//               rows i != j, i < n it has seen, with their indices (a sorted insertion list in
//               registers; rows are masked by index, never by value). All tiles are walked and
//               only columns select: no cross-lane work in the loop, twice the MFMA work of the
//               triangle. The four lanes that share a column are merged through LDS in a fixed
//               order at the end of the walk.
// k_knn_merge   the row ranges (splits) of a column in split order: KN_C candidates and the cut,
//               the (KN_C + 1)-th smallest s~.
// k_knn_rerank  one wave per point: sum_k ((double)x_ik - (double)x_jk)^2 of the caller's rows for
//               the KN_C candidates (differences of fp32 values are exact in fp64), the two
//               smallest by (value, index), r = sqrt. The row is proven iff
//                 r2^2 + E_j < cut_j - E_j,   E_j = efac (a_j + a_max)
//               (every row outside the candidates has s~ >= cut, so its exact squared distance is
//               >= cut - E_j > r2^2); otherwise it is appended to the fallback list.
// k_knn_exact_rows   the same fp64 arithmetic (wave_dist2) against all rows for the listed rows, the
//               rows cut into chunks so that a few listed rows still fill the device;
//               k_knn_exact_merge picks the two smallest by (value, index) over the chunks.
// k_twonn_reduce     kept = #{r1 > 0}, sum of log(r2 / r1) in a fixed order, [1 / mean, kept].
//
// k neighbours, 1 <= k <= 16 (vr_knn_f32): the same pass with the list length L = C + 1 a template
// parameter of kn_insert, k_knn_cand and k_knn_merge, C(k) = 4, 12, 24 for k <= 2, 8, 16. L = 5 is
// the two-neighbour search's code; longer lists are kept one per thread and selected from the tile
// of s~ in LDS (see k_knn_cand). The certificate is the one below with r_k for r2 (the bound is per
// pair and does not depend on k). The exact paths keep their k smallest as a list spread over the
// lanes of a wave: k_knn_rerank_k, k_knn_exact_rows_k, k_knn_exact_merge_k. On top of the lists:
// k_mle_reduce   the k-neighbour maximum-likelihood dimension, k_twonn_reduce's order and, at k = 2, bits.
// k_mutual_knn   overlap counts of two neighbour lists, and their totals under relabellings of one.
//
// The bound. With u = 2^-24, A_i the exact squared norm of the staged row y_i, G_ij the exact dot
// of staged rows and D_ij^2 the exact squared distance of the caller's rows:
//   staging   y_ik = (x_ik - m_k)(1 + delta), |delta| <= u, so y_i - y_j = (x_i - x_j) + e_i - e_j
//             with |e_i| <= u sqrt(A_i);  | |y_i - y_j| - D_ij | <= u (sqrt A_i + sqrt A_j) =: eps and
//             | |y_i - y_j|^2 - D_ij^2 | <= eps (2 |y_i - y_j| + eps) <= (2 + u) u (sqrt A_i + sqrt A_j)^2
//             <= (4 + 2 u) u (A_i + A_j);
//   norms     a_i is an fp64 sum of exact squares (relative error <= d 2^-53) rounded to fp32:
//             |fl32(a_i) - A_i| <= (u + d 2^-52) A_i;
//   dot       any order of d fp32 multiply-adds: |g~ - G| <= gamma_d sum_k |y_ik y_jk| <= gamma_d (A_i + A_j) / 2,
//             gamma_d = d u / (1 - d u);
//   epilogue  fl32(a_i + a_j) adds u (1 + u)(A_i + A_j); the fused -2 g~ + t rounds once,
//             u |s~| <= 2 u (1 + gamma_d + 2 u)(A_i + A_j).
// Sum: |s~_ij - D_ij^2| <= (gamma_d + (8 + small) u)(A_i + A_j). The kernel uses
//   efac = 1.001 (gamma_d + 9 u),  E_j = efac (a_j + a_max) >= the bound for every i,
// with the fp64 norms (their relative error d 2^-53 is inside the 1.001), and d u >= 1/2 or a
// non-finite norm makes E non-finite: every row then takes the exact scan.
//
// No floating-point atomics; every list is built in a fixed order and the exact paths pick by
// (value, index): r and nn are bit-identical run to run. The fallback list is appended with an
// integer atomic: its order varies, the rows' results do not depend on it.
#include <algorithm>
#include <cmath>
#include <limits>

#include "internal.h"

namespace vr {

typedef float kf32x4 __attribute__((ext_vector_type(4)));
typedef float kf32x16 __attribute__((ext_vector_type(16)));

constexpr int KN_C = 4;            // candidates reranked per point
constexpr int KN_L = KN_C + 1;     // list length: the candidates and the cut
constexpr int KN_T = 128;          // tile edge
constexpr int KN_K = 32;           // k per LDS stage
constexpr int KN_LD = KN_K + 4;    // padded LDS row: conflict-free ds_read_b128 (as k_gram)
constexpr int KN_STAGE = KN_T * KN_LD;
constexpr int KN_THREADS = 256;
constexpr int KN_SMAX = 16;        // most row ranges per column block (sizes the workspace)
constexpr int KN_RCH = 64;         // row chunks of the column sums
constexpr int64_t KN_NMAX = (int64_t)1 << 20;
constexpr int KN_XBLK = 2048;      // workgroups the exact scan of a few rows is cut into

// ---- staging ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_knn_colsum(const float* __restrict__ X, int64_t n, int64_t d, int64_t ldx,
                                                    int64_t rows_per, double* __restrict__ part) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= d) return;
  const int64_t r0 = (int64_t)blockIdx.y * rows_per, r1 = min(n, r0 + rows_per);
  double s = 0.0;
  int64_t r = r0;
  for (; r + 16 <= r1; r += 16) {  // 16 loads in flight; the additions keep the row order
    float x[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) x[u] = X[(r + u) * ldx + c];
#pragma unroll
    for (int u = 0; u < 16; ++u) s += (double)x[u];
  }
  for (; r < r1; ++r) s += (double)X[r * ldx + c];
  part[(int64_t)blockIdx.y * d + c] = s;
}

// T = float for the search's staging, double for knn_col_mean_f64 (there mu may be part: one chunk,
// each thread reads its own entry before it writes it)
template <class T>
__global__ __launch_bounds__(256) void k_knn_colmean(const double* part, int64_t n, int64_t d, int chunks, T* mu) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= d) return;
  double s = 0.0;
  for (int b = 0; b < chunks; ++b) s += part[(int64_t)b * d + c];
  mu[c] = (T)(s / (double)n);
}

// block sum of 256 threads: wave shuffle tree, then the four waves in order
__device__ inline double kn_block_sum(double v, double* red) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  if (lane == 0) red[w] = v;
  __syncthreads();
  const double s = (red[0] + red[1]) + (red[2] + red[3]);
  __syncthreads();
  return s;
}

// one block per staged row r < n_pad; rows >= n and columns >= d are exact zeros
__global__ __launch_bounds__(256) void k_knn_stage(const float* __restrict__ X, int64_t n, int64_t d, int64_t ldx,
                                                   const float* __restrict__ mu, float* __restrict__ Y,
                                                   int64_t ldy, double* __restrict__ a64,
                                                   float* __restrict__ a32) {
  __shared__ double red[4];
  const int64_t r = blockIdx.x;
  float* y = Y + r * ldy;
  double q = 0.0;
  if (r < n) {
    const float* x = X + r * ldx;
    for (int64_t k = threadIdx.x; k < ldy; k += 256) {
      float v = 0.f;
      if (k < d) {
        v = __fsub_rn(x[k], mu[k]);
        q = fma((double)v, (double)v, q);
      }
      y[k] = v;
    }
  } else {
    for (int64_t k = threadIdx.x; k < ldy; k += 256) y[k] = 0.f;
  }
  q = kn_block_sum(q, red);
  if (threadIdx.x == 0) {
    a64[r] = q;
    a32[r] = (float)q;
  }
}

// NaN-sticky maximum: a NaN norm makes every certificate fail
__device__ inline double kn_max(double m, double a) { return (a > m || a != a) ? a : m; }

__global__ __launch_bounds__(256) void k_knn_amax(const double* __restrict__ a64, int64_t n, double* __restrict__ amax,
                                                  int32_t* __restrict__ fail_count) {
  __shared__ double red[4];
  double m = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 256) m = kn_max(m, a64[i]);
  for (int o = 32; o > 0; o >>= 1) m = kn_max(m, __shfl_down(m, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    *amax = kn_max(kn_max(red[0], red[1]), kn_max(red[2], red[3]));
    *fail_count = 0;
  }
}

// ---- candidate pass --------------------------------------------------------------------
// ascending list of L (value, index); a new value enters only if strictly smaller than the last
template <int L>
__device__ inline void kn_insert(float (&v)[L], int32_t (&id)[L], float s, int32_t i) {
  if (!(s < v[L - 1])) return;
  v[L - 1] = s;
  id[L - 1] = i;
#pragma unroll
  for (int q = L - 1; q > 0; --q) {
    const bool sw = v[q] < v[q - 1];
    const float tv = v[q];
    const int32_t ti = id[q];
    v[q] = sw ? v[q - 1] : tv;
    id[q] = sw ? id[q - 1] : ti;
    v[q - 1] = sw ? tv : v[q - 1];
    id[q - 1] = sw ? ti : id[q - 1];
  }
}

struct KnParams {
  const float* Y;     // n_pad x ldy staged rows
  int64_t ldy;        // multiple of KN_K
  const float* a32;   // n_pad norms
  int64_t n, n_pad;
  int T, S;           // row tiles, row ranges per column block
  float* listV;       // [S][n_pad][L]
  int32_t* listI;
};

// L = KN_L keeps the lists per lane (two columns each, four lanes per column), selected from the
// accumulators in place: the form and the arithmetic of the two-neighbour search. A longer list
// (L = 13, 25) would cost 2 L (value, index) pairs per lane and 64 copies of the insertion chain,
// so there the tile of s~ goes through the panel buffer (free after the k loop's last barrier):
// thread t owns column t & 127 and rows 64 (t >> 7) .. of the tile, reads them in row order and
// keeps one list. One chain per unrolled read, L pairs per thread, two parts per column to merge.
template <int L>
__global__ __launch_bounds__(KN_THREADS, 2) void k_knn_cand(KnParams P) {
  constexpr bool kLane = (L == KN_L);
  constexpr int NLIST = kLane ? 2 : 1;   // lists per thread
  constexpr int NPART = kLane ? 4 : 2;   // lists per column and workgroup
  constexpr int kQUnroll = L <= 13 ? 4 : 2;  // steps of a k stage unrolled
  static_assert(KN_T * KN_T <= 2 * 2 * KN_STAGE, "the tile of s~ must fit the panel buffer");
  static_assert(KN_T * NPART * L * 2 <= 2 * 2 * KN_STAGE, "the lists to merge must fit the panel buffer");
  __shared__ __attribute__((aligned(16))) float lds[2 * 2 * KN_STAGE];  // [buf][A/B]
  __shared__ float an[KN_T];
  const int id = (int)xcd_remap(blockIdx.x, gridDim.x);
  const int bj = id / P.S, split = id % P.S;
  const int t0 = (int)((int64_t)split * P.T / P.S), t1 = (int)((int64_t)(split + 1) * P.T / P.S);
  const int64_t col0 = (int64_t)bj * KN_T;
  const int nk = (int)(P.ldy / KN_K);

  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int wr = wid >> 1, wc = wid & 1, h = lane >> 5, l32 = lane & 31;

  float lv[NLIST][L];
  int32_t li[NLIST][L];
  float aj[2];
  int32_t jc[2];
#pragma unroll
  for (int nn = 0; nn < 2; ++nn) {
    jc[nn] = (int32_t)(col0 + wc * 64 + nn * 32 + l32);  // < n_pad
    aj[nn] = P.a32[jc[nn]];
  }
#pragma unroll
  for (int nn = 0; nn < NLIST; ++nn)
#pragma unroll
    for (int e = 0; e < L; ++e) {
      lv[nn][e] = std::numeric_limits<float>::infinity();
      li[nn][e] = -1;
    }
  const int tc = threadIdx.x & (KN_T - 1), tp = threadIdx.x >> 7;  // L > KN_L: the thread's column and half

  // thread t stages float4 t + 256 s of a 128 x 32 panel: row f >> 3, columns 4 (f & 7) ..
  auto load_panel = [&](int64_t r0, int64_t k, kf32x4 (&v)[4]) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int f = threadIdx.x + KN_THREADS * s;
      v[s] = *reinterpret_cast<const kf32x4*>(P.Y + (r0 + (f >> 3)) * P.ldy + k + (f & 7) * 4);
    }
  };
  auto store_panel = [&](float* dst, const kf32x4 (&v)[4]) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int f = threadIdx.x + KN_THREADS * s;
      *reinterpret_cast<kf32x4*>(dst + (f >> 3) * KN_LD + (f & 7) * 4) = v[s];
    }
  };

  for (int bi = t0; bi < t1; ++bi) {
    const int64_t row0 = (int64_t)bi * KN_T;
    const bool diag = (bi == bj);
    if (threadIdx.x < KN_T) an[threadIdx.x] = P.a32[row0 + threadIdx.x];

    kf32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;

    kf32x4 ga[4], gb[4];
    load_panel(row0, 0, ga);
    if (!diag) load_panel(col0, 0, gb);
    store_panel(lds, ga);
    if (!diag) store_panel(lds + KN_STAGE, gb);
    __syncthreads();

    for (int kt = 0; kt < nk; ++kt) {
      const int cur = kt & 1;
      const float* As = lds + cur * 2 * KN_STAGE;
      const float* Bs = diag ? As : As + KN_STAGE;
      const bool more = kt + 1 < nk;
      const int64_t kn = (int64_t)(kt + 1) * KN_K;
      if (more) {  // lands under the MFMAs
        load_panel(row0, kn, ga);
        if (!diag) load_panel(col0, kn, gb);
      }
      // lane half h owns k in [16 h, 16 h + 16) of the stage: a fixed permutation of the sum over k
      // (L = 25: two steps unrolled, not four; with all four the 50 list registers spill)
#pragma unroll kQUnroll
      for (int q = 0; q < 4; ++q) {
        kf32x4 av[2], bv[2];
#pragma unroll
        for (int m = 0; m < 2; ++m) {
          av[m] = *reinterpret_cast<const kf32x4*>(As + (wr * 64 + m * 32 + l32) * KN_LD + h * 16 + q * 4);
          bv[m] = *reinterpret_cast<const kf32x4*>(Bs + (wc * 64 + m * 32 + l32) * KN_LD + h * 16 + q * 4);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int nn = 0; nn < 2; ++nn)
              acc[m][nn] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[m][e], bv[nn][e], acc[m][nn], 0, 0, 0);
      }
      if (more) {
        float* nxt = lds + (cur ^ 1) * 2 * KN_STAGE;
        store_panel(nxt, ga);
        if (!diag) store_panel(nxt + KN_STAGE, gb);
      }
      __syncthreads();
    }

    // C/D of the 32 x 32 MFMA: column l32, rows (r & 3) + 8 (r >> 2) + 4 h. Select per column.
    const int lbase = wr * 64 + 4 * h;
    const int32_t irow0 = (int32_t)row0, n32 = (int32_t)P.n;
    if constexpr (kLane) {
#pragma unroll
      for (int nn = 0; nn < 2; ++nn)
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int lr = lbase + m * 32 + (r & 3) + 8 * (r >> 2);
            const int32_t i = irow0 + lr;  // < n_pad <= 2^20
            const float s = __fmaf_rn(-2.f, acc[m][nn][r], __fadd_rn(an[lr], aj[nn]));
            if (i < n32 && i != jc[nn]) kn_insert<L>(lv[nn], li[nn], s, i);
          }
    } else {
      float* tile = lds;  // [row 128][column 128]: a wave stores 32 consecutive columns of two rows
#pragma unroll
      for (int nn = 0; nn < 2; ++nn)
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int lr = lbase + m * 32 + (r & 3) + 8 * (r >> 2);
            tile[lr * KN_T + wc * 64 + nn * 32 + l32] =
                __fmaf_rn(-2.f, acc[m][nn][r], __fadd_rn(an[lr], aj[nn]));
          }
      __syncthreads();
      const int32_t j = (int32_t)col0 + tc;
#pragma unroll 4
      for (int q = 0; q < KN_T / 2; ++q) {  // a wave reads 64 consecutive columns of one row
        const int lr = tp * (KN_T / 2) + q;
        const int32_t i = irow0 + lr;
        const float s = tile[lr * KN_T + tc];
        if (i < n32 && i != j) kn_insert<L>(lv[0], li[0], s, i);
      }
    }
    __syncthreads();  // an and the panels are rewritten by the next tile
  }

  // the lists of a column through LDS, merged in part order: the four lanes (wr, h), or the two halves
  float* lf = lds;  // [col 128][part NPART][L][2]
#pragma unroll
  for (int nn = 0; nn < NLIST; ++nn) {
    const int c = kLane ? wc * 64 + nn * 32 + l32 : tc;
    const int part = kLane ? wr * 2 + h : tp;
#pragma unroll
    for (int e = 0; e < L; ++e) {
      float* p = lf + (((c * NPART) + part) * L + e) * 2;
      p[0] = lv[nn][e];
      p[1] = __int_as_float(li[nn][e]);
    }
  }
  __syncthreads();
  if (threadIdx.x < KN_T) {
    float mv[L];
    int32_t mi[L];
#pragma unroll
    for (int e = 0; e < L; ++e) {
      mv[e] = std::numeric_limits<float>::infinity();
      mi[e] = -1;
    }
    for (int p = 0; p < NPART; ++p)
#pragma unroll
      for (int e = 0; e < L; ++e) {
        const float* q = lf + (((threadIdx.x * NPART) + p) * L + e) * 2;
        kn_insert<L>(mv, mi, q[0], __float_as_int(q[1]));
      }
    const int64_t o = ((int64_t)split * P.n_pad + col0 + threadIdx.x) * L;
#pragma unroll
    for (int e = 0; e < L; ++e) {
      P.listV[o + e] = mv[e];
      P.listI[o + e] = mi[e];
    }
  }
}

// one thread per point: the S range lists in range order; L - 1 candidates and the cut
template <int L>
__global__ __launch_bounds__(256) void k_knn_merge(const float* __restrict__ listV, const int32_t* __restrict__ listI,
                                                   int64_t n, int64_t n_pad, int S, int32_t* __restrict__ cand,
                                                   float* __restrict__ cut) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  float mv[L];
  int32_t mi[L];
#pragma unroll
  for (int e = 0; e < L; ++e) {
    mv[e] = std::numeric_limits<float>::infinity();
    mi[e] = -1;
  }
  for (int s = 0; s < S; ++s) {
    const int64_t o = ((int64_t)s * n_pad + j) * L;
#pragma unroll
    for (int e = 0; e < L; ++e) kn_insert<L>(mv, mi, listV[o + e], listI[o + e]);
  }
#pragma unroll
  for (int e = 0; e < L - 1; ++e) cand[j * (L - 1) + e] = mi[e];
  cut[j] = mv[L - 1];
}

// ---- exact arithmetic ------------------------------------------------------------------
// sum_k ((double)a_k - (double)b_k)^2 by one wave: lane l takes k = l, l + 64, .. in order with a
// fused multiply-add, then an xor butterfly (every lane ends with the same bits). The one
// definition of a squared distance on the exact paths.
__device__ inline double wave_dist2(const float* __restrict__ a, const float* __restrict__ b, int64_t d) {
  double s = 0.0;
  for (int64_t k = threadIdx.x & 63; k < d; k += 64) {
    const double t = (double)a[k] - (double)b[k];
    s = fma(t, t, s);
  }
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  return s;
}

// the two smallest by (value, index)
struct Best2 {
  double v0, v1;
  int32_t i0, i1;
};
__device__ inline bool kn_less(double v, int32_t i, double w, int32_t j) { return v < w || (v == w && i < j); }
__device__ inline void best2_init(Best2& b) {
  b.v0 = b.v1 = std::numeric_limits<double>::infinity();
  b.i0 = b.i1 = 0x7fffffff;
}
__device__ inline void best2_add(Best2& b, double v, int32_t i) {
  if (kn_less(v, i, b.v0, b.i0)) {
    b.v1 = b.v0;
    b.i1 = b.i0;
    b.v0 = v;
    b.i0 = i;
  } else if (kn_less(v, i, b.v1, b.i1)) {
    b.v1 = v;
    b.i1 = i;
  }
}
__device__ inline void best2_write(const Best2& b, int64_t j, double* __restrict__ r, int32_t* __restrict__ nn) {
  r[2 * j] = sqrt(b.v0);
  r[2 * j + 1] = sqrt(b.v1);
  if (nn) {
    nn[2 * j] = b.i0 == 0x7fffffff ? -1 : b.i0;
    nn[2 * j + 1] = b.i1 == 0x7fffffff ? -1 : b.i1;
  }
}

// one wave per point
__global__ __launch_bounds__(256) void k_knn_rerank(const float* __restrict__ X, int64_t n, int64_t d, int64_t ldx,
                                                    const int32_t* __restrict__ cand, const float* __restrict__ cut,
                                                    const double* __restrict__ a64, const double* __restrict__ amax,
                                                    double efac, double* __restrict__ r, int32_t* __restrict__ nn,
                                                    int32_t* __restrict__ fail_list, int32_t* __restrict__ fail_count) {
  const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= n) return;
  Best2 b;
  best2_init(b);
  bool all = true;
  for (int c = 0; c < KN_C; ++c) {
    const int32_t i = cand[j * KN_C + c];
    if (i < 0 || i >= n) {  // uniform over the wave
      all = false;
      continue;
    }
    best2_add(b, wave_dist2(X + j * ldx, X + (int64_t)i * ldx, d), i);
  }
  if ((threadIdx.x & 63) != 0) return;
  const double E = efac * (a64[j] + *amax);
  const double c = (double)cut[j];
  const bool proven = all && c < std::numeric_limits<double>::infinity() && (b.v1 + E < c - E);
  best2_write(b, j, r, nn);
  if (!proven) fail_list[atomicAdd(fail_count, 1)] = (int32_t)j;
}

// block (x, y): listed row x (list == nullptr: row x) against the rows of chunk y, wave w the rows
// w, w + 4, .. of the chunk; the two smallest by (value, index) of the chunk go to part[x * Q + y].
// The choice by (value, index) does not depend on how the rows are cut into chunks.
__global__ __launch_bounds__(256) void k_knn_exact_rows(const float* __restrict__ X, int64_t n, int64_t d,
                                                        int64_t ldx, const int32_t* __restrict__ list,
                                                        int64_t rows_per, Best2* __restrict__ part) {
  __shared__ Best2 wb[4];
  const int64_t j = list ? (int64_t)list[blockIdx.x] : (int64_t)blockIdx.x;
  const int w = threadIdx.x >> 6;
  Best2 b;
  best2_init(b);
  if (j >= 0 && j < n) {  // uniform over the block
    const int64_t i0 = (int64_t)blockIdx.y * rows_per, i1 = min(n, i0 + rows_per);
    for (int64_t i = i0 + w; i < i1; i += 4)
      if (i != j) best2_add(b, wave_dist2(X + j * ldx, X + i * ldx, d), (int32_t)i);
  }
  if ((threadIdx.x & 63) == 0) wb[w] = b;
  __syncthreads();
  if (threadIdx.x == 0) {
    Best2 m = wb[0];
    for (int q = 1; q < 4; ++q) {
      best2_add(m, wb[q].v0, wb[q].i0);
      best2_add(m, wb[q].v1, wb[q].i1);
    }
    part[(int64_t)blockIdx.x * gridDim.y + blockIdx.y] = m;
  }
}

// one thread per listed row: its Q chunks
__global__ __launch_bounds__(256) void k_knn_exact_merge(const Best2* __restrict__ part, int64_t rows, int Q,
                                                         int64_t n, const int32_t* __restrict__ list,
                                                         double* __restrict__ r, int32_t* __restrict__ nn) {
  const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (x >= rows) return;
  const int64_t j = list ? (int64_t)list[x] : x;
  if (j < 0 || j >= n) return;
  Best2 m = part[x * Q];
  for (int q = 1; q < Q; ++q) {
    const Best2 p = part[x * Q + q];
    best2_add(m, p.v0, p.i0);
    best2_add(m, p.v1, p.i1);
  }
  best2_write(m, j, r, nn);
}

__global__ void k_knn_nan(double* __restrict__ r, int32_t* __restrict__ nn, int64_t n) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= 2 * n) return;
  r[e] = __builtin_nan("");
  if (nn) nn[e] = -1;
}

// ---- k neighbours: the exact paths of vr_knn_f32 ------------------------------------------
// A sorted list of k <= KN_KMAX (value, index) spread over a wave: lane e keeps element e, lanes
// >= k keep (inf, INT_MAX). Every value a wave handles on the exact paths is wave-uniform
// (wave_dist2 ends with the same bits in every lane), so an insertion is one ballot and one
// shift by a lane: no list in registers, no dynamic register index.
constexpr int KN_KMAX = 16;
constexpr int32_t KN_NONE = 0x7fffffff;

__device__ inline void wl_insert(double& myv, int32_t& myi, double v, int32_t i, int k, int lane) {
  const bool lt = lane < k && kn_less(v, i, myv, myi);
  const unsigned long long m = __ballot(lt);
  if (m == 0) return;  // uniform: not among the k smallest
  const int pos = __ffsll(m) - 1;
  const double pv = __shfl_up(myv, 1, 64);
  const int32_t pi = __shfl_up(myi, 1, 64);
  if (lane == pos) {
    myv = v;
    myi = i;
  } else if (lane > pos && lane < k) {
    myv = pv;
    myi = pi;
  }
}

__device__ inline void wl_write(double myv, int32_t myi, int64_t j, int k, int lane, double* __restrict__ r,
                                int32_t* __restrict__ nn) {
  if (lane >= k) return;
  const bool none = myi == KN_NONE;
  r[j * k + lane] = none ? __builtin_nan("") : sqrt(myv);
  if (nn) nn[j * k + lane] = none ? -1 : myi;
}

// one wave per point: lane c takes the exact squared distance to candidate c (C <= 24), its rank
// by (value, index) among the C is a count over the lanes, and ranks < k are the result. Proven
// iff all C candidates are rows and r_k^2 + E_j < cut_j - E_j.
__global__ __launch_bounds__(256) void k_knn_rerank_k(const float* __restrict__ X, int64_t n, int64_t d, int64_t ldx,
                                                      const int32_t* __restrict__ cand, int C,
                                                      const float* __restrict__ cut, const double* __restrict__ a64,
                                                      const double* __restrict__ amax, double efac, int k,
                                                      double* __restrict__ r, int32_t* __restrict__ nn,
                                                      int32_t* __restrict__ fail_list,
                                                      int32_t* __restrict__ fail_count) {
  const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= n) return;
  const int lane = threadIdx.x & 63;
  double myv = std::numeric_limits<double>::infinity();
  int32_t myi = KN_NONE;
  bool all = true;
  for (int c = 0; c < C; ++c) {
    const int32_t i = cand[j * C + c];
    if (i < 0 || i >= n) {  // uniform over the wave
      all = false;
      continue;
    }
    const double v = wave_dist2(X + j * ldx, X + (int64_t)i * ldx, d);
    if (lane == c) {
      myv = v;
      myi = i;
    }
  }
  int rank = 0;
  for (int f = 0; f < C; ++f) {
    const double wv = __shfl(myv, f, 64);
    const int32_t wi = __shfl(myi, f, 64);
    rank += kn_less(wv, wi, myv, myi) ? 1 : 0;
  }
  // a row with a missing candidate is rewritten whole by the exact scan
  if (lane < C && rank < k) {
    r[j * k + rank] = sqrt(myv);
    if (nn) nn[j * k + rank] = myi == KN_NONE ? -1 : myi;
  }
  const unsigned long long kth = __ballot(lane < C && rank == k - 1);
  const double vk = __shfl(myv, kth ? __ffsll(kth) - 1 : 0, 64);
  if (lane != 0) return;
  const double E = efac * (a64[j] + *amax);
  const double c = (double)cut[j];
  const bool proven = all && kth != 0 && c < std::numeric_limits<double>::infinity() && (vk + E < c - E);
  if (!proven) fail_list[atomicAdd(fail_count, 1)] = (int32_t)j;
}

// k_knn_exact_rows for k neighbours: block (x, y) as there; the k smallest by (value, index) of
// the chunk, ascending, go to part[(x * Q + y) * k ..] (missing ones (inf, INT_MAX)).
__global__ __launch_bounds__(256) void k_knn_exact_rows_k(const float* __restrict__ X, int64_t n, int64_t d,
                                                          int64_t ldx, const int32_t* __restrict__ list,
                                                          int64_t rows_per, int k, double* __restrict__ partV,
                                                          int32_t* __restrict__ partI) {
  __shared__ double wv[4][KN_KMAX];
  __shared__ int32_t wi[4][KN_KMAX];
  const int64_t j = list ? (int64_t)list[blockIdx.x] : (int64_t)blockIdx.x;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double myv = std::numeric_limits<double>::infinity();
  int32_t myi = KN_NONE;
  if (j >= 0 && j < n) {  // uniform over the block
    const int64_t i0 = (int64_t)blockIdx.y * rows_per, i1 = min(n, i0 + rows_per);
    for (int64_t i = i0 + w; i < i1; i += 4)
      if (i != j) wl_insert(myv, myi, wave_dist2(X + j * ldx, X + i * ldx, d), (int32_t)i, k, lane);
  }
  if (lane < k) {
    wv[w][lane] = myv;
    wi[w][lane] = myi;
  }
  __syncthreads();
  if (w != 0) return;
  for (int q = 1; q < 4; ++q)
    for (int e = 0; e < k; ++e) wl_insert(myv, myi, wv[q][e], wi[q][e], k, lane);
  if (lane < k) {
    const int64_t o = ((int64_t)blockIdx.x * gridDim.y + blockIdx.y) * k + lane;
    partV[o] = myv;
    partI[o] = myi;
  }
}

// one wave per listed row: its Q chunks
__global__ __launch_bounds__(256) void k_knn_exact_merge_k(const double* __restrict__ partV,
                                                           const int32_t* __restrict__ partI, int64_t rows, int Q,
                                                           int64_t n, const int32_t* __restrict__ list, int k,
                                                           double* __restrict__ r, int32_t* __restrict__ nn) {
  const int64_t x = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (x >= rows) return;
  const int64_t j = list ? (int64_t)list[x] : x;
  if (j < 0 || j >= n) return;
  const int lane = threadIdx.x & 63;
  double myv = std::numeric_limits<double>::infinity();
  int32_t myi = KN_NONE;
  for (int q = 0; q < Q; ++q)
    for (int e = 0; e < k; ++e) {
      const int64_t o = (x * Q + q) * k + e;
      wl_insert(myv, myi, partV[o], partI[o], k, lane);
    }
  wl_write(myv, myi, j, k, lane, r, nn);
}

// ---- Two-NN reduction ------------------------------------------------------------------
// thread t adds rows t, t + 256, .. in order; then the block in a fixed order
__global__ __launch_bounds__(256) void k_twonn_reduce(const double* __restrict__ r, int64_t n, double* __restrict__ out) {
  __shared__ double red[4];
  double s = 0.0, c = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 256) {
    const double r1 = r[2 * i], r2 = r[2 * i + 1];
    if (r1 > 0.0) {
      s += log(r2 / r1);
      c += 1.0;
    }
  }
  s = kn_block_sum(s, red);
  c = kn_block_sum(c, red);
  if (threadIdx.x == 0) {
    out[0] = c > 0.0 ? 1.0 / (s / c) : __builtin_nan("");
    out[1] = c;
  }
}

// ---- k-neighbour reductions ---------------------------------------------------------------
// The Levina-Bickel estimator in MacKay and Ghahramani's form from r (n, k), k >= 2: a row counts
// iff r_1 > 0 and r_k is finite, s_i = (1 / (k - 1)) sum_{j < k} log(r_k / r_j), out = [1 / mean s_i,
// counted]. The summation order of k_twonn_reduce; at k = 2 its terms, so its bits.
__global__ __launch_bounds__(256) void k_mle_reduce(const double* __restrict__ r, int64_t n, int k,
                                                    double* __restrict__ out) {
  __shared__ double red[4];
  double s = 0.0, c = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 256) {
    const double r1 = r[i * k], rk = r[i * k + k - 1];
    if (r1 > 0.0 && rk - rk == 0.0) {  // rk finite
      double t = 0.0;
      for (int j = 0; j < k - 1; ++j) t += log(rk / r[i * k + j]);
      s += t / (double)(k - 1);
      c += 1.0;
    }
  }
  s = kn_block_sum(s, red);
  c = kn_block_sum(c, red);
  if (threadIdx.x == 0) {
    out[0] = c > 0.0 ? 1.0 / (s / c) : __builtin_nan("");
    out[1] = c;
  }
}

// Overlap of two neighbour lists. Thread = row i, block y = MK_SLOTS relabellings: slot 0 the
// identity (counts[i] and totals[0]), slot 1 + p the permutation p, where row i counts the a in
// N_A(i) with perm[a] in N_B(perm[i]). Both lists sit in registers behind static indices (entries
// past k are -1, which no row index equals). Integer sums: a wave tree, then one integer atomic.
constexpr int MK_SLOTS = 8;

__global__ __launch_bounds__(256) void k_mutual_knn(const int32_t* __restrict__ nnA, const int32_t* __restrict__ nnB,
                                                    int64_t n, int k, const int32_t* __restrict__ perms,
                                                    int64_t slots, int32_t* __restrict__ counts,
                                                    unsigned long long* __restrict__ totals) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool valid = i < n;
  int32_t a[KN_KMAX];
#pragma unroll
  for (int e = 0; e < KN_KMAX; ++e) a[e] = (valid && e < k) ? nnA[i * k + e] : -1;
  const int64_t s0 = (int64_t)blockIdx.y * MK_SLOTS, s1 = min(slots, s0 + MK_SLOTS);
  for (int64_t s = s0; s < s1; ++s) {
    const int32_t* pm = s == 0 ? nullptr : perms + (s - 1) * n;
    int cnt = 0;
    const int64_t pi = !valid ? -1 : pm ? (int64_t)pm[i] : i;
    if (pi >= 0 && pi < n) {
      int32_t b[KN_KMAX];
#pragma unroll
      for (int e = 0; e < KN_KMAX; ++e) b[e] = e < k ? nnB[pi * k + e] : -1;
#pragma unroll
      for (int e = 0; e < KN_KMAX; ++e) {
        const int32_t ae = a[e];
        if (ae < 0 || ae >= n) continue;
        const int32_t pa = pm ? pm[ae] : ae;
        bool hit = false;
#pragma unroll
        for (int f = 0; f < KN_KMAX; ++f) hit = hit || (b[f] == pa && pa >= 0);
        cnt += hit ? 1 : 0;
      }
    }
    if (s == 0 && valid && counts) counts[i] = cnt;
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o, 64);
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(totals + s, (unsigned long long)cnt);
  }
}

struct KnLayout {
  int64_t n_pad, d_pad;
  int T, S, chunks;
  double* colpart;
  float* mu;
  float* Y;
  double* a64;
  float* a32;
  double* amax;
  float* listV;
  int32_t* listI;
  int32_t* cand;
  float* cut;
  int32_t* fail_list;
  int32_t* fail_count;
  Best2* xpart;  // chunk results of the exact scan (two neighbours)
  double* xpartV;  // k neighbours: [rows * Q][k]
  int32_t* xpartI;
  size_t bytes;
};

// C candidates per row; k = 0 is the two-neighbour search (its Best2 chunk results), k >= 1 sizes
// the chunk lists of vr_knn_f32
static KnLayout kn_layout(void* ws, int64_t n, int64_t d, int C = KN_C, int k = 0) {
  KnLayout L;
  const int64_t nn = std::max<int64_t>(n, 1), dd = std::max<int64_t>(d, 1);
  L.n_pad = (nn + KN_T - 1) / KN_T * KN_T;
  L.d_pad = (dd + KN_K - 1) / KN_K * KN_K;
  L.T = (int)(L.n_pad / KN_T);
  // enough workgroups to fill the device, at most KN_SMAX ranges and one tile per range
  L.S = (int)std::min<int64_t>(std::min<int64_t>(L.T, KN_SMAX), (1024 + L.T - 1) / L.T);
  L.chunks = (int)std::min<int64_t>(KN_RCH, (nn + 255) / 256);
  Carver c(ws);
  L.colpart = c.take<double>((size_t)KN_RCH * dd);
  L.mu = c.take<float>((size_t)dd);
  L.Y = c.take<float>((size_t)L.n_pad * L.d_pad);
  L.a64 = c.take<double>((size_t)L.n_pad);
  L.a32 = c.take<float>((size_t)L.n_pad);
  L.amax = c.take<double>(1);
  L.listV = c.take<float>((size_t)KN_SMAX * L.n_pad * (C + 1));
  L.listI = c.take<int32_t>((size_t)KN_SMAX * L.n_pad * (C + 1));
  L.cand = c.take<int32_t>((size_t)L.n_pad * C);
  L.cut = c.take<float>((size_t)L.n_pad);
  L.fail_list = c.take<int32_t>((size_t)L.n_pad);
  L.fail_count = c.take<int32_t>(1);
  L.xpart = nullptr;
  L.xpartV = nullptr;
  L.xpartI = nullptr;
  if (k == 0) {
    L.xpart = c.take<Best2>((size_t)L.n_pad + KN_XBLK);
  } else {
    L.xpartV = c.take<double>(((size_t)L.n_pad + KN_XBLK) * k);
    L.xpartI = c.take<int32_t>(((size_t)L.n_pad + KN_XBLK) * k);
  }
  L.bytes = c.bytes();
  return L;
}

static thread_local int64_t g_last_fallback = 0;

// the exact scan of `rows` rows (list, or rows 0 .. rows - 1): Q row chunks each, rows * Q < rows + KN_XBLK
static int exact_scan(const float* X, int64_t n, int64_t d, int64_t ldx, const int32_t* list, int64_t rows,
                      const KnLayout& Y, double* r, int32_t* nn, hipStream_t st) {
  const int64_t q_max = std::min<int64_t>(256, (n + 3) / 4);
  const int Q = (int)std::max<int64_t>(1, std::min<int64_t>(q_max, (KN_XBLK + rows - 1) / rows));
  const int64_t rows_per = (n + Q - 1) / Q;
  KtScope kt(KT_KNN_EXACT, (double)rows * (double)n, st);
  k_knn_exact_rows<<<dim3((unsigned)rows, (unsigned)Q), 256, 0, st>>>(X, n, d, ldx, list, rows_per, Y.xpart);
  VR_CHECK_LAUNCH();
  k_knn_exact_merge<<<(unsigned)((rows + 255) / 256), 256, 0, st>>>(Y.xpart, rows, Q, n, list, r, nn);
  VR_CHECK_LAUNCH();
  return VR_OK;
}

static thread_local int64_t g_last_fallback_k = 0;

// candidates reranked per row: C(k) >= k + 2, one k_knn_cand instantiation each
static int knn_candidates(int k) { return k < 1 || k > KN_KMAX ? -1 : k <= 2 ? KN_C : k <= 8 ? 12 : 24; }

static int exact_scan_k(const float* X, int64_t n, int64_t d, int64_t ldx, const int32_t* list, int64_t rows,
                        const KnLayout& Y, int k, double* r, int32_t* nn, hipStream_t st) {
  const int64_t q_max = std::min<int64_t>(256, (n + 3) / 4);
  const int Q = (int)std::max<int64_t>(1, std::min<int64_t>(q_max, (KN_XBLK + rows - 1) / rows));
  const int64_t rows_per = (n + Q - 1) / Q;
  KtScope kt(KT_KNN_EXACT, (double)rows * (double)n, st);
  k_knn_exact_rows_k<<<dim3((unsigned)rows, (unsigned)Q), 256, 0, st>>>(X, n, d, ldx, list, rows_per, k, Y.xpartV,
                                                                       Y.xpartI);
  VR_CHECK_LAUNCH();
  k_knn_exact_merge_k<<<(unsigned)((rows + 3) / 4), 256, 0, st>>>(Y.xpartV, Y.xpartI, rows, Q, n, list, k, r, nn);
  VR_CHECK_LAUNCH();
  return VR_OK;
}

template <int L>
static int launch_cand(const KnLayout& Y, int64_t n, hipStream_t st) {
  {
    KnParams P;
    P.Y = Y.Y;
    P.ldy = Y.d_pad;
    P.a32 = Y.a32;
    P.n = n;
    P.n_pad = Y.n_pad;
    P.T = Y.T;
    P.S = Y.S;
    P.listV = Y.listV;
    P.listI = Y.listI;
    KtScope kt(KT_KNN_CAND, 2.0 * (double)Y.n_pad * (double)Y.n_pad * (double)Y.d_pad, st);
    k_knn_cand<L><<<(unsigned)(Y.T * Y.S), KN_THREADS, 0, st>>>(P);
    VR_CHECK_LAUNCH();
  }
  return VR_OK;
}

template <int L>
static int launch_merge(const KnLayout& Y, int64_t n, hipStream_t st) {
  k_knn_merge<L><<<(unsigned)((n + 255) / 256), 256, 0, st>>>(Y.listV, Y.listI, n, Y.n_pad, Y.S, Y.cand, Y.cut);
  VR_CHECK_LAUNCH();
  return VR_OK;
}

// fp64 column means with no workspace: one chunk of rows, summed in row order into mean itself
int knn_col_mean_f64(const float* X, int64_t n, int64_t d, int64_t ldx, double* mean, hipStream_t st) {
  const unsigned grid = (unsigned)((d + 255) / 256);
  k_knn_colsum<<<dim3(grid, 1), 256, 0, st>>>(X, n, d, ldx, n, mean);
  VR_CHECK_LAUNCH();
  k_knn_colmean<double><<<grid, 256, 0, st>>>(mean, n, d, 1, mean);
  VR_CHECK_LAUNCH();
  return VR_OK;
}

}  // namespace vr

using namespace vr;

extern "C" {

size_t vr_knn2_workspace(int64_t n, int64_t d) {
  return kn_layout(nullptr, std::min<int64_t>(std::max<int64_t>(n, 0), KN_NMAX), d).bytes;
}

int64_t vr_knn2_last_fallback_rows(void) { return g_last_fallback; }

int vr_knn2_f32(const float* X, int64_t n, int64_t d, int64_t ldx, double* r, int32_t* nn, void* ws,
                size_t ws_bytes, void* stream) {
  clear_error();
  VR_REQUIRE(n >= 0 && n <= KN_NMAX && d >= 1 && ldx >= d, "vr_knn2_f32: bad shape n=%lld d=%lld ldx=%lld",
             (long long)n, (long long)d, (long long)ldx);
  VR_REQUIRE(X != nullptr && r != nullptr, "vr_knn2_f32: null pointer");
  const size_t need = kn_layout(nullptr, n, d).bytes;
  if (ws_bytes < need || ws == nullptr) {
    set_error("vr_knn2_f32: workspace %zu < %zu", ws_bytes, need);
    return VR_EWORKSPACE;
  }
  g_last_fallback = 0;
  if (n == 0) return VR_OK;
  hipStream_t st = as_stream(stream);
  if (n < 3) {
    k_knn_nan<<<(unsigned)((2 * n + 255) / 256), 256, 0, st>>>(r, nn, n);
    VR_CHECK_LAUNCH();
    return VR_OK;
  }
  const KnLayout Y = kn_layout(ws, n, d);
  if (n <= KN_C + 1) {  // no cut: every row takes the exact scan
    VR_TRY(exact_scan(X, n, d, ldx, nullptr, n, Y, r, nn, st));
    g_last_fallback = n;
    return VR_OK;
  }
  {
    KtScope kt(KT_KNN_STAGE, 2.0 * (double)n * (double)d * sizeof(float), st);
    const int64_t rows_per = (n + Y.chunks - 1) / Y.chunks;
    k_knn_colsum<<<dim3((unsigned)((d + 255) / 256), (unsigned)Y.chunks), 256, 0, st>>>(X, n, d, ldx, rows_per,
                                                                                      Y.colpart);
    VR_CHECK_LAUNCH();
    k_knn_colmean<float><<<(unsigned)((d + 255) / 256), 256, 0, st>>>(Y.colpart, n, d, Y.chunks, Y.mu);
    VR_CHECK_LAUNCH();
    k_knn_stage<<<(unsigned)Y.n_pad, 256, 0, st>>>(X, n, d, ldx, Y.mu, Y.Y, Y.d_pad, Y.a64, Y.a32);
    VR_CHECK_LAUNCH();
    k_knn_amax<<<1, 256, 0, st>>>(Y.a64, n, Y.amax, Y.fail_count);
    VR_CHECK_LAUNCH();
  }
  {
    KnParams P;
    P.Y = Y.Y;
    P.ldy = Y.d_pad;
    P.a32 = Y.a32;
    P.n = n;
    P.n_pad = Y.n_pad;
    P.T = Y.T;
    P.S = Y.S;
    P.listV = Y.listV;
    P.listI = Y.listI;
    // every tile is walked once: 2 (128)^2 d_pad FLOP each
    KtScope kt(KT_KNN_CAND, 2.0 * (double)Y.n_pad * (double)Y.n_pad * (double)Y.d_pad, st);
    k_knn_cand<KN_L><<<(unsigned)(Y.T * Y.S), KN_THREADS, 0, st>>>(P);
    VR_CHECK_LAUNCH();
  }
  const double u = 0x1p-24, du = (double)d * u;
  const double efac = du < 0.5 ? 1.001 * (du / (1.0 - du) + 9.0 * u) : std::numeric_limits<double>::infinity();
  {
    KtScope kt(KT_KNN_RERANK, (double)n * KN_C, st);
    k_knn_merge<KN_L><<<(unsigned)((n + 255) / 256), 256, 0, st>>>(Y.listV, Y.listI, n, Y.n_pad, Y.S, Y.cand, Y.cut);
    VR_CHECK_LAUNCH();
    k_knn_rerank<<<(unsigned)((n + 3) / 4), 256, 0, st>>>(X, n, d, ldx, Y.cand, Y.cut, Y.a64, Y.amax, efac, r, nn,
                                                         Y.fail_list, Y.fail_count);
    VR_CHECK_LAUNCH();
  }
  // the one read-back of the call: how many rows the certificate could not prove
  int32_t failed = 0;
  VR_CHECK_HIP(hipMemcpyAsync(&failed, Y.fail_count, sizeof(failed), hipMemcpyDeviceToHost, st));
  VR_CHECK_HIP(hipStreamSynchronize(st));
  if (failed < 0 || failed > n) {
    set_error("vr_knn2_f32: fallback count %d outside [0, %lld]", (int)failed, (long long)n);
    return VR_EINTERNAL;
  }
  if (failed > 0) VR_TRY(exact_scan(X, n, d, ldx, Y.fail_list, failed, Y, r, nn, st));
  g_last_fallback = failed;
  return VR_OK;
}

int vr_twonn_id_f64(const double* r, int64_t n, double* out, void* stream) {
  clear_error();
  VR_REQUIRE(n >= 0, "vr_twonn_id_f64: bad n=%lld", (long long)n);
  VR_REQUIRE(out != nullptr && (n == 0 || r != nullptr), "vr_twonn_id_f64: null pointer");
  k_twonn_reduce<<<1, 256, 0, as_stream(stream)>>>(r, n, out);
  VR_CHECK_LAUNCH();
  return VR_OK;
}

int vr_knn_candidates(int k) { return knn_candidates(k); }

size_t vr_knn_workspace(int64_t n, int64_t d, int k) {
  const int C = knn_candidates(k);
  if (C < 0) return 0;
  return kn_layout(nullptr, std::min<int64_t>(std::max<int64_t>(n, 0), KN_NMAX), d, C, k).bytes;
}

int64_t vr_knn_last_fallback_rows(void) { return g_last_fallback_k; }

int vr_knn_f32(const float* X, int64_t n, int64_t d, int64_t ldx, int k, double* r, int32_t* nn, void* ws,
               size_t ws_bytes, void* stream) {
  clear_error();
  const int C = knn_candidates(k);
  VR_REQUIRE(C > 0, "vr_knn_f32: k=%d outside [1, %d]", k, KN_KMAX);
  VR_REQUIRE(n >= 0 && n <= KN_NMAX && d >= 1 && ldx >= d, "vr_knn_f32: bad shape n=%lld d=%lld ldx=%lld",
             (long long)n, (long long)d, (long long)ldx);
  VR_REQUIRE(X != nullptr && r != nullptr, "vr_knn_f32: null pointer");
  const size_t need = kn_layout(nullptr, n, d, C, k).bytes;
  if (ws_bytes < need || ws == nullptr) {
    set_error("vr_knn_f32: workspace %zu < %zu", ws_bytes, need);
    return VR_EWORKSPACE;
  }
  g_last_fallback_k = 0;
  if (n == 0) return VR_OK;
  hipStream_t st = as_stream(stream);
  const KnLayout Y = kn_layout(ws, n, d, C, k);
  if (n <= C + 1) {  // no cut: every row takes the exact scan (slots from n - 1 on: NaN, -1)
    VR_TRY(exact_scan_k(X, n, d, ldx, nullptr, n, Y, k, r, nn, st));
    g_last_fallback_k = n;
    return VR_OK;
  }
  {
    KtScope kt(KT_KNN_STAGE, 2.0 * (double)n * (double)d * sizeof(float), st);
    const int64_t rows_per = (n + Y.chunks - 1) / Y.chunks;
    k_knn_colsum<<<dim3((unsigned)((d + 255) / 256), (unsigned)Y.chunks), 256, 0, st>>>(X, n, d, ldx, rows_per,
                                                                                      Y.colpart);
    VR_CHECK_LAUNCH();
    k_knn_colmean<float><<<(unsigned)((d + 255) / 256), 256, 0, st>>>(Y.colpart, n, d, Y.chunks, Y.mu);
    VR_CHECK_LAUNCH();
    k_knn_stage<<<(unsigned)Y.n_pad, 256, 0, st>>>(X, n, d, ldx, Y.mu, Y.Y, Y.d_pad, Y.a64, Y.a32);
    VR_CHECK_LAUNCH();
    k_knn_amax<<<1, 256, 0, st>>>(Y.a64, n, Y.amax, Y.fail_count);
    VR_CHECK_LAUNCH();
  }
  VR_TRY(C == KN_C ? launch_cand<KN_L>(Y, n, st) : C == 12 ? launch_cand<13>(Y, n, st) : launch_cand<25>(Y, n, st));
  const double u = 0x1p-24, du = (double)d * u;
  const double efac = du < 0.5 ? 1.001 * (du / (1.0 - du) + 9.0 * u) : std::numeric_limits<double>::infinity();
  {
    KtScope kt(KT_KNN_RERANK, (double)n * C, st);
    VR_TRY(C == KN_C ? launch_merge<KN_L>(Y, n, st) : C == 12 ? launch_merge<13>(Y, n, st)
                                                              : launch_merge<25>(Y, n, st));
    k_knn_rerank_k<<<(unsigned)((n + 3) / 4), 256, 0, st>>>(X, n, d, ldx, Y.cand, C, Y.cut, Y.a64, Y.amax, efac, k, r,
                                                           nn, Y.fail_list, Y.fail_count);
    VR_CHECK_LAUNCH();
  }
  int32_t failed = 0;
  VR_CHECK_HIP(hipMemcpyAsync(&failed, Y.fail_count, sizeof(failed), hipMemcpyDeviceToHost, st));
  VR_CHECK_HIP(hipStreamSynchronize(st));
  if (failed < 0 || failed > n) {
    set_error("vr_knn_f32: fallback count %d outside [0, %lld]", (int)failed, (long long)n);
    return VR_EINTERNAL;
  }
  if (failed > 0) VR_TRY(exact_scan_k(X, n, d, ldx, Y.fail_list, failed, Y, k, r, nn, st));
  g_last_fallback_k = failed;
  return VR_OK;
}

int vr_mle_id_f64(const double* r, int64_t n, int k, double* out, void* stream) {
  clear_error();
  VR_REQUIRE(n >= 0 && k >= 2 && k <= KN_KMAX, "vr_mle_id_f64: bad n=%lld k=%d", (long long)n, k);
  VR_REQUIRE(out != nullptr && (n == 0 || r != nullptr), "vr_mle_id_f64: null pointer");
  k_mle_reduce<<<1, 256, 0, as_stream(stream)>>>(r, n, k, out);
  VR_CHECK_LAUNCH();
  return VR_OK;
}

int vr_mutual_knn_i32(const int32_t* nnA, const int32_t* nnB, int64_t n, int k, const int32_t* perms, int64_t P,
                      int32_t* counts, int64_t* totals, void* stream) {
  clear_error();
  VR_REQUIRE(n >= 0 && n <= KN_NMAX && k >= 1 && k <= KN_KMAX && P >= 0 && P <= ((int64_t)1 << 18),
             "vr_mutual_knn_i32: bad n=%lld k=%d P=%lld", (long long)n, k, (long long)P);
  VR_REQUIRE(totals != nullptr && (n == 0 || (nnA != nullptr && nnB != nullptr)) && (P == 0 || perms != nullptr),
             "vr_mutual_knn_i32: null pointer");
  hipStream_t st = as_stream(stream);
  VR_CHECK_HIP(hipMemsetAsync(totals, 0, (size_t)(1 + P) * sizeof(int64_t), st));
  if (n == 0) return VR_OK;
  const dim3 grid((unsigned)((n + 255) / 256), (unsigned)((1 + P + MK_SLOTS - 1) / MK_SLOTS));
  k_mutual_knn<<<grid, 256, 0, st>>>(nnA, nnB, n, k, perms, 1 + P, counts,
                                     reinterpret_cast<unsigned long long*>(totals));
  VR_CHECK_LAUNCH();
  return VR_OK;
}

}  // extern "C"
