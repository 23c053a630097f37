// PLS-SVD cross-decomposition (analysis/cross_decomposition.py): replaces, in
// visreps/analysis/cross_decomposition.py:30-79, GaussianRandomProjection.fit_transform, the K
// PLSSVD fits of the shuffled KFold and the per-component np.corrcoef / np.cov of the test scores.
//
// All K training folds come from one pass over the rows. With the rows in fold order and centred
// about the global fp64 column means, k_xcov gives each test fold's moment block
//   S_f = sum_{r in fold f} (x_r - mx)^T (y_r - my)                       (p x q, fp64)
// and k_seg_colstats its column sums and sums of squares. Fold f's training rows are all the
// others, so with T = sum_f S_f, n_tr = n - n_f, m the training mean about the global mean and s
// the training ddof=1 standard deviation (0 replaced by 1, as scikit-learn's _center_scale_xy),
//   C_f = (T - S_f - n_tr m_x m_y^T) / (s_x s_y^T)
// is the standardised training cross-covariance X_s^T Y_s that PLSSVD decomposes. Its SVD is
// the top of the spectrum of the symmetric J = [[0, C], [C^T, 0]] (Jordan-Wielandt): eigenvalue
// sigma_j with eigenvector [u_j; v_j] / sqrt(2), which vr_eigh_top_f64 (eigvals.hip) solves with
// no squaring of the condition number.
//
// k_xcov           64 x 64 tiles of the p x q rectangle on tile64.h's pipeline (fp64 MFMA, 16-row
//                  stages, double-buffered LDS): the X and Y panels are centred in fp64 while
//                  staged. One launch per segment; a segment is cut into S row slices,
//                  k_xcov_reduce adds the slices in order.
// k_seg_colstats   per-segment column sums and sums of squares of the same centred values.
// k_fold_stats     training mean and standard deviation of one fold from the segment statistics.
// k_fold_assemble  J of one fold (exactly symmetric, exactly zero diagonal blocks).
// k_xgemm_nt       G[i, j] = sum_k (A[i, k] - a_mean[k]) B[j, k], both operands K-contiguous, on
//                  the same pipeline with split-K: the projection Z = X R^T (products of two fp32
//                  values are exact in fp64, the sum is rounded once to fp32) and the test scores.
// k_svd_extract    u, v from the eigenvector rows: halves normalised, svd_flip's u-based sign,
//                  divided by the training standard deviation; null components flagged.
// k_svd_weights    the same outputs from the unit rows of vr_svd_jacobi_f64 (svd.hip), for
//                  vr_plssvd_folds_svd_f64: C of every run fold at once (k_fold_xcov), one batched
//                  Jacobi SVD, then the scores as above.
// k_col_corr_cov   Pearson r and ddof=1 covariance of paired score columns, two passes.
// Roofline: fp64 MFMA. Algorithmic FLOPs: k_xcov 2 n p q, k_xgemm_nt 2 M N K.
#include <algorithm>
#include <cfloat>
#include <cmath>

#include "tile64.h"

namespace vr {

// ------------------------------------------------------------------------------------
// segmented cross-moments
// ------------------------------------------------------------------------------------
struct XcovParams {
  const float* X;
  const float* Y;
  int64_t p, q, ldx, ldy;
  const int32_t* rows;  // nullable: position r of the fold order -> row of X and Y
  const double* mx;     // global column means
  const double* my;
  double* partial;      // this segment's [S][ntile][T64 * T64]
  int TJ, ntile, S;
  int64_t k0, k1, kslice;  // the segment's positions [k0, k1), positions per slice (multiple of T64_K)
  bool vecx, vecy;
};

__global__ __launch_bounds__(T64_THREADS, 2) void k_xcov(XcovParams P) {
  __shared__ __attribute__((aligned(16))) double lds[2][2][T64_STAGE];  // [buf][X/Y]
  const int id = (int)xcd_remap(blockIdx.x, gridDim.x);
  const int tile = id / P.S, slice = id % P.S;
  const int bi = tile / P.TJ, bj = tile % P.TJ;
  const int64_t ci = (int64_t)bi * T64, cj = (int64_t)bj * T64;
  const int64_t k0 = min(P.k1, P.k0 + (int64_t)slice * P.kslice);
  const int64_t k1 = min(P.k1, k0 + P.kslice);
  const int nk = (int)((k1 - k0 + T64_K - 1) / T64_K);

  double mA[4], mB[4];
  {
    const int c = (threadIdx.x & 15) * 4;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      mA[e] = (ci + c + e < P.p) ? P.mx[ci + c + e] : 0.0;
      mB[e] = (cj + c + e < P.q) ? P.my[cj + c + e] : 0.0;
    }
  }
  auto load = [&](int side, int64_t k) {
    return side ? panel_load(P.Y, P.ldy, P.q, P.vecy, P.rows, cj, k, k1)
                : panel_load(P.X, P.ldx, P.p, P.vecx, P.rows, ci, k, k1);
  };
  auto store = [&](int side, double* dst, const f32x4 v, int64_t k) { panel_store(dst, v, side ? mB : mA, k, k1); };
  // an empty slice (or an empty segment) stores its all-zero tile
  tile_pipeline(lds, k0, nk, false, load, store, P.partial + ((int64_t)slice * P.ntile + tile) * (T64 * T64));
}

// S_f = sum of the slices in slice order; grid (ntile, F)
__global__ __launch_bounds__(256) void k_xcov_reduce(const double* __restrict__ partial, int S, int ntile, int TJ,
                                                     int64_t p, int64_t q, double* __restrict__ out) {
  const int tile = blockIdx.x;
  const int64_t f = blockIdx.y;
  const int bi = tile / TJ, bj = tile % TJ;
  const double* part = partial + f * (int64_t)S * ntile * (T64 * T64);
  double* o = out + f * p * q;
  for (int e = threadIdx.x; e < T64 * T64; e += blockDim.x) {
    const int64_t i = (int64_t)bi * T64 + e / T64, j = (int64_t)bj * T64 + e % T64;
    if (i >= p || j >= q) continue;
    o[i * q + j] = slice_sum(part, S, ntile, tile, e);
  }
}

// Column sums and sums of squares of (double)M[rows[r]][c] - mean[c] over r in [k0, k1): 4 row
// groups of 64 column lanes, each group adds its rows (k0 + g, k0 + g + 4, ..) in order, the
// groups are added in order.
__global__ __launch_bounds__(256) void k_seg_colstats(const float* __restrict__ M, int64_t ld, int64_t ncol,
                                                      const int32_t* __restrict__ rows,
                                                      const double* __restrict__ mean, int64_t k0, int64_t k1,
                                                      double* __restrict__ sum, double* __restrict__ ssq) {
  __shared__ double red[2][4][64];
  const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int64_t c = (int64_t)blockIdx.x * 64 + lane;
  double s = 0.0, s2 = 0.0;
  if (c < ncol) {
    const double mu = mean[c];
    for (int64_t r = k0 + g; r < k1; r += 4) {
      const int64_t row = rows != nullptr ? (int64_t)rows[r] : r;
      const double v = (double)M[row * ld + c] - mu;
      s += v;
      s2 += v * v;
    }
  }
  red[0][g][lane] = s;
  red[1][g][lane] = s2;
  __syncthreads();
  if (g == 0 && c < ncol) {
    sum[c] = ((red[0][0][lane] + red[0][1][lane]) + red[0][2][lane]) + red[0][3][lane];
    ssq[c] = ((red[1][0][lane] + red[1][1][lane]) + red[1][2][lane]) + red[1][3][lane];
  }
}

// ------------------------------------------------------------------------------------
// one fold: training statistics, the cross-covariance, J
// ------------------------------------------------------------------------------------
// stats [F][2][m]: [f][0][c] the sum, [f][1][c] the sum of squares of column c (X columns, then
// Y columns) over segment f. Training rows of fold f = every other segment, added in order.
__global__ void k_fold_stats(const double* __restrict__ stats, int F, int64_t m, int f, double n_tr,
                             const double* __restrict__ mx, const double* __restrict__ my, int64_t p,
                             double* __restrict__ trm, double* __restrict__ trs, double* __restrict__ trabs) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= m) return;
  double s = 0.0, s2 = 0.0;
  for (int g = 0; g < F; ++g) {
    if (g == f) continue;
    s += stats[((int64_t)g * 2 + 0) * m + c];
    s2 += stats[((int64_t)g * 2 + 1) * m + c];
  }
  const double mean = s / n_tr;
  const double var = (s2 - n_tr * mean * mean) / (n_tr - 1.0);
  double sd = sqrt(var);
  if (var <= 0.0) sd = 1.0;  // a constant column: _center_scale_xy's std == 0 -> 1 (NaN stays NaN)
  trm[c] = mean;
  trs[c] = sd;
  trabs[c] = (c < p ? mx[c] : my[c - p]) + mean;
}

// T = sum_f S_f in fold order
__global__ void k_seg_total(const double* __restrict__ S, int F, int64_t pq, double* __restrict__ T) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= pq) return;
  double s = 0.0;
  for (int g = 0; g < F; ++g) s += S[(int64_t)g * pq + e];
  T[e] = s;
}

__device__ inline double fold_c(const double* T, const double* Sf, const double* trm, const double* trs,
                                double n_tr, int64_t p, int64_t q, int64_t i, int64_t j) {
  const double num = (T[i * q + j] - Sf[i * q + j]) - n_tr * trm[i] * trm[p + j];
  return num / (trs[i] * trs[p + j]);
}

// C_f alone (p x q): the test hook of the moment algebra
__global__ void k_fold_xcov(const double* __restrict__ T, const double* __restrict__ Sf,
                            const double* __restrict__ trm, const double* __restrict__ trs, double n_tr,
                            int64_t p, int64_t q, double* __restrict__ C) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= p * q) return;
  C[e] = fold_c(T, Sf, trm, trs, n_tr, p, q, e / q, e % q);
}

// J = [[0, C], [C^T, 0]] ((p + q)^2): entry and mirror come from the same expression
__global__ void k_fold_assemble(const double* __restrict__ T, const double* __restrict__ Sf,
                                const double* __restrict__ trm, const double* __restrict__ trs, double n_tr,
                                int64_t p, int64_t q, double* __restrict__ J) {
  const int64_t m = p + q;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= m * m) return;
  const int64_t a = e / m, b = e % m;
  double v = 0.0;
  if (a < p && b >= p)
    v = fold_c(T, Sf, trm, trs, n_tr, p, q, a, b - p);
  else if (a >= p && b < p)
    v = fold_c(T, Sf, trm, trs, n_tr, p, q, b, a - p);
  J[e] = v;
}

// ------------------------------------------------------------------------------------
// two-operand NT product
// ------------------------------------------------------------------------------------
template <typename TB>
struct XgemmParams {
  const float* A;
  const TB* B;
  int64_t M, N, K, lda, ldb;
  const int32_t* a_rows;  // nullable: row i of the product reads row a_rows[i] of A
  const double* a_mean;   // nullable, length K
  double* partial;        // [S][ntile][T64 * T64]
  int TJ, ntile, S;
  int64_t kslice;         // contraction entries per slice (multiple of T64_K)
  bool veca, vecb;
};

// this thread's 4 consecutive k of one row: row c = tid >> 2, k offset 4 (tid & 3)
__device__ inline f64x4 xg_load(const float* A, int64_t lda, int64_t nrow, bool vec, const int32_t* a_rows,
                                int64_t row0, int64_t k, int64_t k1) {
  const int c = threadIdx.x >> 2, kq = (threadIdx.x & 3) * 4;
  f64x4 v = {0.0, 0.0, 0.0, 0.0};
  const int64_t i = row0 + c, r = k + kq;
  if (i >= nrow || r >= k1) return v;
  const int64_t row = a_rows != nullptr ? (int64_t)a_rows[i] : i;
  const float* src = A + row * lda + r;
  if (vec && r + 4 <= k1) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(src);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (double)t[e];
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (r + e < k1) ? (double)src[e] : 0.0;
  }
  return v;
}

__device__ inline f64x4 xg_load(const double* B, int64_t ldb, int64_t nrow, bool vec, const int32_t*,
                                int64_t row0, int64_t k, int64_t k1) {
  const int c = threadIdx.x >> 2, kq = (threadIdx.x & 3) * 4;
  f64x4 v = {0.0, 0.0, 0.0, 0.0};
  const int64_t i = row0 + c, r = k + kq;
  if (i >= nrow || r >= k1) return v;
  const double* src = B + i * ldb + r;
  if (vec && r + 4 <= k1) {
    const f64x2 t0 = *reinterpret_cast<const f64x2*>(src);
    const f64x2 t1 = *reinterpret_cast<const f64x2*>(src + 2);
    v = f64x4{t0[0], t0[1], t1[0], t1[1]};
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (r + e < k1) ? src[e] : 0.0;
  }
  return v;
}

// scatter the 4 k down the LDS column of row c; out-of-range entries stay exact zeros
__device__ inline void xg_store(double* lds, const f64x4 v, const double* mean, bool row_in, int64_t k,
                                int64_t k1) {
  const int c = threadIdx.x >> 2, kq = (threadIdx.x & 3) * 4;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int64_t r = k + kq + e;
    double x = v[e];
    if (mean != nullptr) x = (row_in && r < k1) ? x - mean[r] : 0.0;
    lds[(kq + e) * T64_LD + c] = x;
  }
}

template <typename TB>
__global__ __launch_bounds__(T64_THREADS, 2) void k_xgemm_nt(XgemmParams<TB> P) {
  __shared__ __attribute__((aligned(16))) double lds[2][2][T64_STAGE];  // [buf][A/B]
  const int id = (int)xcd_remap(blockIdx.x, gridDim.x);
  const int tile = id / P.S, slice = id % P.S;
  const int bi = tile / P.TJ, bj = tile % P.TJ;
  const int64_t ri = (int64_t)bi * T64, rj = (int64_t)bj * T64;
  const int64_t k0 = min(P.K, (int64_t)slice * P.kslice);
  const int64_t k1 = min(P.K, k0 + P.kslice);
  const int nk = (int)((k1 - k0 + T64_K - 1) / T64_K);
  const bool a_in = ri + (threadIdx.x >> 2) < P.M;

  // both operands hold double4s of 4 consecutive k of one row (see tile64.h on why these stay here)
  auto load = [&](int side, int64_t k) {
    return side ? xg_load(P.B, P.ldb, P.N, P.vecb, nullptr, rj, k, k1)
                : xg_load(P.A, P.lda, P.M, P.veca, P.a_rows, ri, k, k1);
  };
  auto store = [&](int side, double* dst, const f64x4 v, int64_t k) {
    xg_store(dst, v, side ? nullptr : P.a_mean, side || a_in, k, k1);
  };
    tile_pipeline(lds, k0, nk, false, load, store, P.partial + ((int64_t)slice * P.ntile + tile) * (T64 * T64));
}

// G = sum of the split-K slices in slice order, rounded once to the output type
template <typename TO>
__global__ __launch_bounds__(256) void k_xgemm_reduce(const double* __restrict__ partial, int S, int ntile, int TJ,
                                                      int64_t M, int64_t N, TO* __restrict__ G, int64_t ldg) {
  const int tile = blockIdx.x;
  const int bi = tile / TJ, bj = tile % TJ;
  for (int e = threadIdx.x; e < T64 * T64; e += blockDim.x) {
    const int64_t i = (int64_t)bi * T64 + e / T64, j = (int64_t)bj * T64 + e % T64;
    if (i >= M || j >= N) continue;
    G[i * ldg + j] = (TO)slice_sum(partial, S, ntile, tile, e);
  }
}

// ------------------------------------------------------------------------------------
// weights from the eigenvectors of J, and the paired column statistics of the scores
// ------------------------------------------------------------------------------------
// One workgroup per component j. V row j = [u; v] / sqrt(2) up to sign and rounding.
//   Wu [k][m] (nullable)  unit u then unit v, svd_flip's sign
//   Wp [k][m]             the same divided by the training standard deviations
//   sigma, null, imb (nullable: |2 |u|^2 - 1| before normalisation) [k]
// A null component's weights are NaN.
__global__ __launch_bounds__(256) void k_svd_extract(const double* __restrict__ w, const double* __restrict__ V,
                                                     int64_t ldv, int64_t p, int64_t q,
                                                     const double* __restrict__ trs, double* __restrict__ Wu,
                                                     double* __restrict__ Wp, double* __restrict__ sigma,
                                                     int32_t* __restrict__ null, double* __restrict__ imb) {
  __shared__ double r_u[256], r_v[256], r_a[256];
  __shared__ int64_t r_i[256];
  const int64_t j = blockIdx.x, m = p + q;
  const double* row = V + j * ldv;
  const int t = threadIdx.x;
  double su = 0.0, sv = 0.0, best = -1.0;
  int64_t bidx = 0;
  for (int64_t i = t; i < m; i += 256) {
    const double x = row[i];
    if (i < p) {
      su += x * x;
      const double a = fabs(x);
      if (a > best) {  // ascending i: the lowest index of a tie stays
        best = a;
        bidx = i;
      }
    } else {
      sv += x * x;
    }
  }
  r_u[t] = su;
  r_v[t] = sv;
  r_a[t] = best;
  r_i[t] = bidx;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {  // fixed tree
    if (t < o) {
      r_u[t] += r_u[t + o];
      r_v[t] += r_v[t + o];
      const double a = r_a[t + o];
      const int64_t ia = r_i[t + o];
      if (a > r_a[t] || (a == r_a[t] && ia < r_i[t])) {
        r_a[t] = a;
        r_i[t] = ia;
      }
    }
    __syncthreads();
  }
  const double nu2 = r_u[0], nv2 = r_v[0];
  const double s1 = w[0], sj = w[j];
  const bool is_null = !(sj > 64.0 * (double)m * DBL_EPSILON * s1) || !(nu2 > 0.0) || !(nv2 > 0.0);
  const double sign = row[r_i[0]] < 0.0 ? -1.0 : 1.0;
  const double fu = sign / sqrt(nu2), fv = sign / sqrt(nv2);
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  for (int64_t i = t; i < m; i += 256) {
    const double unit = is_null ? nan : row[i] * (i < p ? fu : fv);
    if (Wu != nullptr) Wu[j * m + i] = unit;
    Wp[j * m + i] = unit / trs[i];
  }
  if (t == 0) {
    sigma[j] = sj;
    null[j] = is_null ? 1 : 0;
    if (imb != nullptr) imb[j] = fabs(2.0 * nu2 - 1.0);
  }
}

// One thread per paired column: means, then centred sums, in row order. corr is clipped to
// [-1, 1] as np.corrcoef; fewer than 2 rows, or a null component, give NaN.
__global__ void k_col_corr_cov(const double* __restrict__ SX, const double* __restrict__ SY, int64_t nt, int64_t k,
                               int64_t ld, double* __restrict__ corr, double* __restrict__ cov) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= k) return;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  if (nt < 2) {
    corr[j] = nan;
    cov[j] = nan;
    return;
  }
  double ax = 0.0, ay = 0.0;
  for (int64_t r = 0; r < nt; ++r) {
    ax += SX[r * ld + j];
    ay += SY[r * ld + j];
  }
  ax /= (double)nt;
  ay /= (double)nt;
  double sxx = 0.0, syy = 0.0, sxy = 0.0;
  for (int64_t r = 0; r < nt; ++r) {
    const double dx = SX[r * ld + j] - ax, dy = SY[r * ld + j] - ay;
    sxx += dx * dx;
    syy += dy * dy;
    sxy += dx * dy;
  }
  double r = sxy / sqrt(sxx) / sqrt(syy);
  r = r > 1.0 ? 1.0 : (r < -1.0 ? -1.0 : r);  // NaN passes through both comparisons
  corr[j] = r;
  cov[j] = sxy / (double)(nt - 1);
}

// ------------------------------------------------------------------------------------
// host geometry
// ------------------------------------------------------------------------------------
struct XGeom {
  int TI, TJ, ntile, S;
  int64_t kslice;
};

// tiles of an M x N rectangle; the contraction of length K cut into S slices of kslice (a
// multiple of T64_K) so that ~4 workgroups per CU exist where K allows, each slice >= min_stages stages
static XGeom x_geometry(int64_t M, int64_t N, int64_t K, int64_t groups, int min_stages) {
  XGeom g;
  g.TI = (int)((M + T64 - 1) / T64);
  g.TJ = (int)((N + T64 - 1) / T64);
  g.ntile = g.TI * g.TJ;
  const int64_t wgs = std::max<int64_t>(1, (int64_t)g.ntile * std::max<int64_t>(groups, 1));
  const int64_t want = std::max<int64_t>(1, (4LL * num_cus() + wgs - 1) / wgs);
  const int64_t maxs = std::max<int64_t>(1, K / ((int64_t)min_stages * T64_K));
  const int64_t S = std::min<int64_t>({want, maxs, 64});
  g.kslice = ((std::max<int64_t>(K, 1) + S - 1) / S + T64_K - 1) / T64_K * T64_K;
  g.S = (int)std::max<int64_t>(1, (std::max<int64_t>(K, 1) + g.kslice - 1) / g.kslice);
  return g;
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <typename TB, typename TO>
static int xgemm_launch(const float* A, int64_t M, int64_t K, int64_t lda, const int32_t* a_rows,
                        const double* a_mean, const TB* B, int64_t N, int64_t ldb, TO* G, int64_t ldg, void* ws,
                        hipStream_t st) {
  if (M == 0 || N == 0) return VR_OK;
  const XGeom g = x_geometry(M, N, K, 1, 16);
  XgemmParams<TB> P;
  P.A = A;
  P.B = B;
  P.M = M;
  P.N = N;
  P.K = K;
  P.lda = lda;
  P.ldb = ldb;
  P.a_rows = a_rows;
  P.a_mean = a_mean;
  Carver c(ws);
  P.partial = c.take<double>((size_t)g.S * g.ntile * T64 * T64);
  P.TJ = g.TJ;
  P.ntile = g.ntile;
  P.S = g.S;
  P.kslice = g.kslice;
  P.veca = (lda % 4 == 0) && aligned16(A);
  P.vecb = (ldb % (16 / (int64_t)sizeof(TB)) == 0) && aligned16(B);
  k_xgemm_nt<TB><<<(unsigned)(g.ntile * g.S), T64_THREADS, 0, st>>>(P);
  VR_CHECK_LAUNCH();
  k_xgemm_reduce<TO><<<(unsigned)g.ntile, 256, 0, st>>>(P.partial, g.S, g.ntile, g.TJ, M, N, G, ldg);
  VR_CHECK_LAUNCH();
  return VR_OK;
}

static size_t xgemm_ws(int64_t M, int64_t N, int64_t K) {
  if (M <= 0 || N <= 0) return 256;
  const XGeom g = x_geometry(M, N, K, 1, 16);
  Carver c(nullptr);
  c.take<double>((size_t)g.S * g.ntile * T64 * T64);
  return c.bytes();
}

struct FoldsLayout {
  double *T, *trm, *trs, *trabs, *J, *w, *V, *Wp, *SX, *SY;
  void* eig;
  size_t eig_bytes;
  void* gemm;
  size_t gemm_bytes;
  size_t bytes;
};

static FoldsLayout folds_layout(void* ws, int64_t p, int64_t q, int64_t k, int64_t max_test) {
  FoldsLayout L;
  const int64_t m = p + q;
  Carver c(ws);
  L.T = c.take<double>((size_t)(p * q));
  L.trm = c.take<double>((size_t)m);
  L.trs = c.take<double>((size_t)m);
  L.trabs = c.take<double>((size_t)m);
  L.J = c.take<double>((size_t)(m * m));
  L.w = c.take<double>((size_t)std::max<int64_t>(k, 1));
  L.V = c.take<double>((size_t)(std::max<int64_t>(k, 1) * m));
  L.Wp = c.take<double>((size_t)(std::max<int64_t>(k, 1) * m));
  L.SX = c.take<double>((size_t)(std::max<int64_t>(max_test, 1) * std::max<int64_t>(k, 1)));
  L.SY = c.take<double>((size_t)(std::max<int64_t>(max_test, 1) * std::max<int64_t>(k, 1)));
  L.eig_bytes = vr_eigh_top_workspace(m, k);
  L.eig = c.take<char>(L.eig_bytes);
  // the score products of every fold (nt <= max_test rows): S <= ceil(4 CUs / ntile), so a
  // launch's S ntile partial tiles number at most 4 CUs + ntile, ntile largest at max_test
  const int64_t tmax = ((std::max<int64_t>(max_test, 1) + T64 - 1) / T64) * ((std::max<int64_t>(k, 1) + T64 - 1) / T64);
  L.gemm_bytes = (size_t)(4LL * num_cus() + tmax) * T64 * T64 * sizeof(double) + 256;
  L.gemm = c.take<char>(L.gemm_bytes);
  L.bytes = c.bytes();
  return L;
}

static bool seg_ok(const int64_t* seg, int64_t F) {
  if (seg == nullptr || F < 1 || seg[0] != 0) return false;
  for (int64_t f = 0; f < F; ++f)
    if (seg[f + 1] < seg[f]) return false;
  return seg[F] <= INT32_MAX;
}

static int64_t seg_max(const int64_t* seg, int64_t F) {
  int64_t mx = 0;
  for (int64_t f = 0; f < F; ++f) mx = std::max(mx, seg[f + 1] - seg[f]);
  return mx;
}

// The Jacobi path's k_svd_extract: component j of one fold from vr_svd_jacobi_f64's unit rows
// U [r][p], Vt [r][q] (sign and NaN fill already applied there). One workgroup per component.
//   Wu [k][m] (nullable)  u then v;  Wp [k][m]  the same divided by the training standard deviations
__global__ __launch_bounds__(256) void k_svd_weights(const double* __restrict__ U, const double* __restrict__ Vt,
                                                     const double* __restrict__ S, const int32_t* __restrict__ nl,
                                                     int64_t p, int64_t q, const double* __restrict__ trs,
                                                     double* __restrict__ Wu, double* __restrict__ Wp,
                                                     double* __restrict__ sigma, int32_t* __restrict__ null,
                                                     double* __restrict__ imb) {
  const int64_t j = blockIdx.x, m = p + q;
  for (int64_t i = threadIdx.x; i < m; i += 256) {
    const double unit = i < p ? U[j * p + i] : Vt[j * q + (i - p)];
    if (Wu != nullptr) Wu[j * m + i] = unit;
    Wp[j * m + i] = unit / trs[i];
  }
  if (threadIdx.x == 0) {
    sigma[j] = S[j];
    null[j] = nl[j];
    if (imb != nullptr) imb[j] = 0.0;
  }
}

struct FoldsSvdLayout {
  double *T, *trm, *trs, *trabs, *C, *Sv, *U, *Vt, *Wp, *SX, *SY;
  int32_t *nl, *sweeps;
  void* svd;
  size_t svd_bytes;
  void* gemm;
  size_t gemm_bytes;
  size_t bytes;
};

static FoldsSvdLayout folds_svd_layout(void* ws, int64_t p, int64_t q, int64_t k, int64_t max_test, int64_t n_run) {
  FoldsSvdLayout L;
  const int64_t m = p + q, r = std::min(p, q), nr = std::max<int64_t>(n_run, 1), kk = std::max<int64_t>(k, 1);
  Carver c(ws);
  L.T = c.take<double>((size_t)(p * q));
  L.trm = c.take<double>((size_t)(nr * m));
  L.trs = c.take<double>((size_t)(nr * m));
  L.trabs = c.take<double>((size_t)(nr * m));
  L.C = c.take<double>((size_t)(nr * p * q));
  L.Sv = c.take<double>((size_t)(nr * r));
  L.U = c.take<double>((size_t)(nr * r * p));
  L.Vt = c.take<double>((size_t)(nr * r * q));
  L.nl = c.take<int32_t>((size_t)(nr * r));
  L.sweeps = c.take<int32_t>((size_t)nr);
  L.Wp = c.take<double>((size_t)(kk * m));
  L.SX = c.take<double>((size_t)(std::max<int64_t>(max_test, 1) * kk));
  L.SY = c.take<double>((size_t)(std::max<int64_t>(max_test, 1) * kk));
  L.svd_bytes = vr_svd_jacobi_workspace(nr, p, q);
  L.svd = c.take<char>(L.svd_bytes);
  // as folds_layout: a score product's partial tiles number at most 4 CUs + ntile
  const int64_t tmax = ((std::max<int64_t>(max_test, 1) + T64 - 1) / T64) * ((kk + T64 - 1) / T64);
  L.gemm_bytes = (size_t)(4LL * num_cus() + tmax) * T64 * T64 * sizeof(double) + 256;
  L.gemm = c.take<char>(L.gemm_bytes);
  L.bytes = c.bytes();
  return L;
}

}  // namespace vr

using namespace vr;

extern "C" {

size_t vr_xgemm_nt_workspace(int64_t M, int64_t N, int64_t K) { return xgemm_ws(M, N, K); }

int vr_xgemm_nt_f32(const float* A, int64_t M, int64_t K, int64_t lda, const int32_t* a_rows,
                    const double* a_mean, const void* B, int b_f64, int64_t N, int64_t ldb, void* G, int g_f64,
                    int64_t ldg, void* ws, size_t ws_bytes, void* stream) {
  clear_error();
  VR_REQUIRE(M >= 0 && N >= 0 && K >= 1 && lda >= K && ldb >= K && ldg >= N,
             "vr_xgemm_nt_f32: bad shape M=%lld N=%lld K=%lld lda=%lld ldb=%lld ldg=%lld", (long long)M,
             (long long)N, (long long)K, (long long)lda, (long long)ldb, (long long)ldg);
  VR_REQUIRE(M <= INT32_MAX && N <= INT32_MAX && ((M + T64 - 1) / T64) * ((N + T64 - 1) / T64) <= (1 << 24),
             "vr_xgemm_nt_f32: M=%lld N=%lld too large", (long long)M, (long long)N);
  if (M == 0 || N == 0) return VR_OK;
  VR_REQUIRE(A != nullptr && B != nullptr && G != nullptr, "vr_xgemm_nt_f32: null pointer");
  if (ws == nullptr || ws_bytes < xgemm_ws(M, N, K)) {
    set_error("vr_xgemm_nt_f32: workspace too small");
    return VR_EWORKSPACE;
  }
  hipStream_t st = as_stream(stream);
  if (b_f64 && g_f64)
    return xgemm_launch(A, M, K, lda, a_rows, a_mean, (const double*)B, N, ldb, (double*)G, ldg, ws, st);
  if (b_f64) return xgemm_launch(A, M, K, lda, a_rows, a_mean, (const double*)B, N, ldb, (float*)G, ldg, ws, st);
  if (g_f64) return xgemm_launch(A, M, K, lda, a_rows, a_mean, (const float*)B, N, ldb, (double*)G, ldg, ws, st);
  return xgemm_launch(A, M, K, lda, a_rows, a_mean, (const float*)B, N, ldb, (float*)G, ldg, ws, st);
}

size_t vr_xcov_segments_workspace(int64_t p, int64_t q, int64_t F, int64_t max_seg) {
  if (p <= 0 || q <= 0 || F <= 0) return 256;
  const XGeom g = x_geometry(p, q, max_seg, F, 4);
  Carver c(nullptr);
  c.take<double>((size_t)F * g.S * g.ntile * T64 * T64);
  return c.bytes();
}

int vr_xcov_segments_f32(const float* X, int64_t ldx, const float* Y, int64_t ldy, int64_t p, int64_t q,
                         const int32_t* rows, const int64_t* seg, int64_t F, const double* mean_x,
                         const double* mean_y, double* S, double* stats, void* ws, size_t ws_bytes,
                         void* stream) {
  clear_error();
  VR_REQUIRE(p >= 1 && q >= 1 && ldx >= p && ldy >= q, "vr_xcov_segments_f32: bad shape p=%lld q=%lld",
             (long long)p, (long long)q);
  VR_REQUIRE(seg_ok(seg, F) && F <= 65535, "vr_xcov_segments_f32: bad segments");
  VR_REQUIRE(((p + T64 - 1) / T64) * ((q + T64 - 1) / T64) <= (1 << 20), "vr_xcov_segments_f32: p, q too large");
  VR_REQUIRE(S != nullptr && mean_x != nullptr && mean_y != nullptr && (seg[F] == 0 || (X != nullptr && Y != nullptr)),
             "vr_xcov_segments_f32: null pointer");
  const int64_t max_seg = seg_max(seg, F);
  if (ws == nullptr || ws_bytes < vr_xcov_segments_workspace(p, q, F, max_seg)) {
    set_error("vr_xcov_segments_f32: workspace too small");
    return VR_EWORKSPACE;
  }
  hipStream_t st = as_stream(stream);
  const XGeom g = x_geometry(p, q, max_seg, F, 4);
  Carver c(ws);
  double* partial = c.take<double>((size_t)F * g.S * g.ntile * T64 * T64);
  XcovParams P;
  P.X = X;
  P.Y = Y;
  P.p = p;
  P.q = q;
  P.ldx = ldx;
  P.ldy = ldy;
  P.rows = rows;
  P.mx = mean_x;
  P.my = mean_y;
  P.TJ = g.TJ;
  P.ntile = g.ntile;
  P.S = g.S;
  P.kslice = g.kslice;
  P.vecx = (ldx % 4 == 0) && aligned16(X);
  P.vecy = (ldy % 4 == 0) && aligned16(Y);
  const int64_t m = p + q;
  for (int64_t f = 0; f < F; ++f) {
    P.k0 = seg[f];
    P.k1 = seg[f + 1];
    P.partial = partial + f * (int64_t)g.S * g.ntile * T64 * T64;
    k_xcov<<<(unsigned)(g.ntile * g.S), T64_THREADS, 0, st>>>(P);
    VR_CHECK_LAUNCH();
    if (stats != nullptr) {
      double* sum = stats + (f * 2 + 0) * m;
      double* ssq = stats + (f * 2 + 1) * m;
      k_seg_colstats<<<(unsigned)((p + 63) / 64), 256, 0, st>>>(X, ldx, p, rows, mean_x, seg[f], seg[f + 1], sum,
                                                              ssq);
      VR_CHECK_LAUNCH();
      k_seg_colstats<<<(unsigned)((q + 63) / 64), 256, 0, st>>>(Y, ldy, q, rows, mean_y, seg[f], seg[f + 1],
                                                              sum + p, ssq + p);
      VR_CHECK_LAUNCH();
    }
  }
  k_xcov_reduce<<<dim3((unsigned)g.ntile, (unsigned)F), 256, 0, st>>>(partial, g.S, g.ntile, g.TJ, p, q, S);
  VR_CHECK_LAUNCH();
  return VR_OK;
}

size_t vr_fold_xcov_workspace(int64_t p, int64_t q) {
  if (p <= 0 || q <= 0) return 256;
  Carver c(nullptr);
  c.take<double>((size_t)(p * q));
  c.take<double>((size_t)(p + q));
  c.take<double>((size_t)(p + q));
  c.take<double>((size_t)(p + q));
  return c.bytes();
}

int vr_fold_xcov_f64(const double* S, const double* stats, const int64_t* seg, int64_t F, int64_t p, int64_t q,
                     const double* mean_x, const double* mean_y, double* C, void* ws, size_t ws_bytes,
                     void* stream) {
  clear_error();
  VR_REQUIRE(p >= 1 && q >= 1 && seg_ok(seg, F) && F <= INT32_MAX, "vr_fold_xcov_f64: bad shape");
  VR_REQUIRE(S != nullptr && stats != nullptr && C != nullptr && mean_x != nullptr && mean_y != nullptr,
             "vr_fold_xcov_f64: null pointer");
  for (int64_t f = 0; f < F; ++f)
    VR_REQUIRE(seg[F] - (seg[f + 1] - seg[f]) >= 2, "vr_fold_xcov_f64: fold %lld leaves fewer than 2 training rows",
               (long long)f);
  if (ws == nullptr || ws_bytes < vr_fold_xcov_workspace(p, q)) {
    set_error("vr_fold_xcov_f64: workspace too small");
    return VR_EWORKSPACE;
  }
  hipStream_t st = as_stream(stream);
  const int64_t m = p + q, pq = p * q;
  Carver c(ws);
  double* T = c.take<double>((size_t)pq);
  double* trm = c.take<double>((size_t)m);
  double* trs = c.take<double>((size_t)m);
  double* trabs = c.take<double>((size_t)m);
  k_seg_total<<<(unsigned)((pq + 255) / 256), 256, 0, st>>>(S, (int)F, pq, T);
  VR_CHECK_LAUNCH();
  for (int64_t f = 0; f < F; ++f) {
    const double n_tr = (double)(seg[F] - (seg[f + 1] - seg[f]));
    k_fold_stats<<<(unsigned)((m + 255) / 256), 256, 0, st>>>(stats, (int)F, m, (int)f, n_tr, mean_x, mean_y, p, trm,
                                                            trs, trabs);
    VR_CHECK_LAUNCH();
    k_fold_xcov<<<(unsigned)((pq + 255) / 256), 256, 0, st>>>(T, S + f * pq, trm, trs, n_tr, p, q, C + f * pq);
    VR_CHECK_LAUNCH();
  }
  return VR_OK;
}

size_t vr_plssvd_folds_workspace(int64_t p, int64_t q, int64_t k, int64_t max_test) {
  if (p <= 0 || q <= 0 || k < 0 || max_test < 0) return 256;
  return folds_layout(nullptr, p, q, k, max_test).bytes;
}

int vr_plssvd_folds_f64(const float* X, int64_t ldx, const float* Y, int64_t ldy, int64_t p, int64_t q,
                        const int32_t* rows, const int64_t* seg, int64_t F, int64_t n_run, const double* mean_x,
                        const double* mean_y, const double* S, const double* stats, int64_t k, double* corr,
                        double* cov, double* sigma, int32_t* null, double* imbalance, int64_t wfold,
                        double* weights, double* wmean, double* wstd, void* ws, size_t ws_bytes, void* stream) {
  clear_error();
  VR_REQUIRE(p >= 1 && q >= 1 && ldx >= p && ldy >= q && p + q <= 65536, "vr_plssvd_folds_f64: bad shape p=%lld q=%lld",
             (long long)p, (long long)q);
  VR_REQUIRE(seg_ok(seg, F) && F <= INT32_MAX && n_run >= 0 && n_run <= F, "vr_plssvd_folds_f64: bad segments");
  VR_REQUIRE(k >= 1 && k <= std::min(p, q), "vr_plssvd_folds_f64: k=%lld outside [1, min(p, q)]", (long long)k);
  VR_REQUIRE(X != nullptr && Y != nullptr && S != nullptr && stats != nullptr && mean_x != nullptr &&
                 mean_y != nullptr && corr != nullptr && cov != nullptr && sigma != nullptr && null != nullptr,
             "vr_plssvd_folds_f64: null pointer");
  VR_REQUIRE(weights == nullptr || (wfold >= 0 && wfold < n_run && wmean != nullptr && wstd != nullptr),
             "vr_plssvd_folds_f64: bad weights request");
  int64_t max_test = 0;
  for (int64_t f = 0; f < n_run; ++f) {
    VR_REQUIRE(seg[F] - (seg[f + 1] - seg[f]) >= 2,
               "vr_plssvd_folds_f64: fold %lld leaves fewer than 2 training rows", (long long)f);
    max_test = std::max(max_test, seg[f + 1] - seg[f]);
  }
  if (ws == nullptr || ws_bytes < vr_plssvd_folds_workspace(p, q, k, max_test)) {
    set_error("vr_plssvd_folds_f64: workspace too small");
    return VR_EWORKSPACE;
  }
  hipStream_t st = as_stream(stream);
  const int64_t m = p + q, pq = p * q;
  const FoldsLayout L = folds_layout(ws, p, q, k, max_test);
  k_seg_total<<<(unsigned)((pq + 255) / 256), 256, 0, st>>>(S, (int)F, pq, L.T);
  VR_CHECK_LAUNCH();
  for (int64_t f = 0; f < n_run; ++f) {
    const int64_t nt = seg[f + 1] - seg[f];
    const double n_tr = (double)(seg[F] - nt);
    const bool keep = weights != nullptr && f == wfold;
    k_fold_stats<<<(unsigned)((m + 255) / 256), 256, 0, st>>>(stats, (int)F, m, (int)f, n_tr, mean_x, mean_y, p,
                                                            L.trm, keep ? wstd : L.trs, keep ? wmean : L.trabs);
    VR_CHECK_LAUNCH();
    const double* trs = keep ? wstd : L.trs;
    const double* trabs = keep ? wmean : L.trabs;
    k_fold_assemble<<<(unsigned)((m * m + 255) / 256), 256, 0, st>>>(L.T, S + f * pq, L.trm, trs, n_tr, p, q, L.J);
    VR_CHECK_LAUNCH();
    VR_TRY(vr_eigh_top_f64(L.J, m, m, k, L.w, L.V, m, L.eig, L.eig_bytes, stream));
    k_svd_extract<<<(unsigned)k, 256, 0, st>>>(L.w, L.V, m, p, q, trs, keep ? weights : nullptr, L.Wp,
                                               sigma + f * k, null + f * k,
                                               imbalance != nullptr ? imbalance + f * k : nullptr);
    VR_CHECK_LAUNCH();
    if (nt > 0) {  // scores of the test rows: (z - training mean) . u / s
      const int32_t* tr = rows != nullptr ? rows + seg[f] : nullptr;
      const float* Xt = rows != nullptr ? X : X + seg[f] * ldx;
      const float* Yt = rows != nullptr ? Y : Y + seg[f] * ldy;
      VR_TRY((xgemm_launch<double, double>(Xt, nt, p, ldx, tr, trabs, L.Wp, k, m, L.SX, k, L.gemm, st)));
      VR_TRY((xgemm_launch<double, double>(Yt, nt, q, ldy, tr, trabs + p, L.Wp + p, k, m, L.SY, k, L.gemm, st)));
    }
    k_col_corr_cov<<<(unsigned)((k + 255) / 256), 256, 0, st>>>(L.SX, L.SY, nt, k, k, corr + f * k, cov + f * k);
    VR_CHECK_LAUNCH();
  }
  return VR_OK;
}

size_t vr_plssvd_folds_svd_workspace(int64_t p, int64_t q, int64_t k, int64_t max_test, int64_t n_run) {
  if (p <= 0 || q <= 0 || k < 0 || max_test < 0 || n_run < 0) return 256;
  return folds_svd_layout(nullptr, p, q, k, max_test, n_run).bytes;
}

int vr_plssvd_folds_svd_f64(const float* X, int64_t ldx, const float* Y, int64_t ldy, int64_t p, int64_t q,
                            const int32_t* rows, const int64_t* seg, int64_t F, int64_t n_run,
                            const double* mean_x, const double* mean_y, const double* S, const double* stats,
                            int64_t k, double* corr, double* cov, double* sigma, int32_t* null,
                            double* imbalance, int64_t wfold, double* weights, double* wmean, double* wstd,
                            void* ws, size_t ws_bytes, void* stream) {
  clear_error();
  VR_REQUIRE(p >= 1 && q >= 1 && ldx >= p && ldy >= q && std::max(p, q) <= 4096,
             "vr_plssvd_folds_svd_f64: bad shape p=%lld q=%lld (max(p, q) <= 4096)", (long long)p, (long long)q);
  VR_REQUIRE(seg_ok(seg, F) && F <= INT32_MAX && n_run >= 0 && n_run <= F && n_run <= 65535,
             "vr_plssvd_folds_svd_f64: bad segments");
  VR_REQUIRE(k >= 1 && k <= std::min(p, q), "vr_plssvd_folds_svd_f64: k=%lld outside [1, min(p, q)]", (long long)k);
  VR_REQUIRE(X != nullptr && Y != nullptr && S != nullptr && stats != nullptr && mean_x != nullptr &&
                 mean_y != nullptr && corr != nullptr && cov != nullptr && sigma != nullptr && null != nullptr,
             "vr_plssvd_folds_svd_f64: null pointer");
  VR_REQUIRE(weights == nullptr || (wfold >= 0 && wfold < n_run && wmean != nullptr && wstd != nullptr),
             "vr_plssvd_folds_svd_f64: bad weights request");
  int64_t max_test = 0;
  for (int64_t f = 0; f < n_run; ++f) {
    VR_REQUIRE(seg[F] - (seg[f + 1] - seg[f]) >= 2,
               "vr_plssvd_folds_svd_f64: fold %lld leaves fewer than 2 training rows", (long long)f);
    max_test = std::max(max_test, seg[f + 1] - seg[f]);
  }
  if (ws == nullptr || ws_bytes < vr_plssvd_folds_svd_workspace(p, q, k, max_test, n_run)) {
    set_error("vr_plssvd_folds_svd_f64: workspace too small");
    return VR_EWORKSPACE;
  }
  if (n_run == 0) return VR_OK;
  hipStream_t st = as_stream(stream);
  const int64_t m = p + q, pq = p * q, r = std::min(p, q);
  const FoldsSvdLayout L = folds_svd_layout(ws, p, q, k, max_test, n_run);
  k_seg_total<<<(unsigned)((pq + 255) / 256), 256, 0, st>>>(S, (int)F, pq, L.T);
  VR_CHECK_LAUNCH();
  // every run fold's statistics and C, then all their SVDs in one batch
  for (int64_t f = 0; f < n_run; ++f) {
    const double n_tr = (double)(seg[F] - (seg[f + 1] - seg[f]));
    const bool keep = weights != nullptr && f == wfold;
    double* trs = keep ? wstd : L.trs + f * m;
    k_fold_stats<<<(unsigned)((m + 255) / 256), 256, 0, st>>>(stats, (int)F, m, (int)f, n_tr, mean_x, mean_y, p,
                                                            L.trm + f * m, trs, keep ? wmean : L.trabs + f * m);
    VR_CHECK_LAUNCH();
    k_fold_xcov<<<(unsigned)((pq + 255) / 256), 256, 0, st>>>(L.T, S + f * pq, L.trm + f * m, trs, n_tr, p, q,
                                                            L.C + f * pq);
    VR_CHECK_LAUNCH();
  }
  VR_TRY(vr_svd_jacobi_f64(L.C, n_run, p, q, q, pq, L.Sv, L.U, L.Vt, L.nl, L.sweeps, L.svd, L.svd_bytes, stream));
  for (int64_t f = 0; f < n_run; ++f) {
    const int64_t nt = seg[f + 1] - seg[f];
    const bool keep = weights != nullptr && f == wfold;
    const double* trs = keep ? wstd : L.trs + f * m;
    const double* trabs = keep ? wmean : L.trabs + f * m;
    k_svd_weights<<<(unsigned)k, 256, 0, st>>>(L.U + f * r * p, L.Vt + f * r * q, L.Sv + f * r, L.nl + f * r, p, q,
                                               trs, keep ? weights : nullptr, L.Wp, sigma + f * k, null + f * k,
                                               imbalance != nullptr ? imbalance + f * k : nullptr);
    VR_CHECK_LAUNCH();
    if (nt > 0) {  // scores of the test rows: (z - training mean) . u / s
      const int32_t* tr = rows != nullptr ? rows + seg[f] : nullptr;
      const float* Xt = rows != nullptr ? X : X + seg[f] * ldx;
      const float* Yt = rows != nullptr ? Y : Y + seg[f] * ldy;
      VR_TRY((xgemm_launch<double, double>(Xt, nt, p, ldx, tr, trabs, L.Wp, k, m, L.SX, k, L.gemm, st)));
      VR_TRY((xgemm_launch<double, double>(Yt, nt, q, ldy, tr, trabs + p, L.Wp + p, k, m, L.SY, k, L.gemm, st)));
    }
    k_col_corr_cov<<<(unsigned)((k + 255) / 256), 256, 0, st>>>(L.SX, L.SY, nt, k, k, corr + f * k, cov + f * k);
    VR_CHECK_LAUNCH();
  }
  return VR_OK;
}

}  // extern "C"
