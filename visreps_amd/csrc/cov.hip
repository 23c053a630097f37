// PCA covariance of extracted features: replaces batched_pca's
// mean and covariance, scripts/coarsegrain/compute_eigenvectors.py:23-36,
//   mean = X.mean(axis=0)                                 numpy, X float32 C-order (n, p)
//   cov  = sum over batches of (X[b].astype(f64) - mean)^T (X[b].astype(f64) - mean)
//   cov /= n - 1                                          (p, p) float64
//
// k_col_sum   numpy's float32 mean along axis 0 of a C-order array adds whole rows in row
//             order (the inner loop runs over columns), so every column is a sequential
//             float32 sum. One workgroup per 64 columns keeps that order exactly: 15
//             waves stream rows into an LDS ring, wave 0 adds them in order. Bit-identical
//             to numpy; `init` continues a sum (the multi-GPU chain over row shards).
// k_cov       upper-triangle 64 x 64 tiles of the centred Gram in fp64 on tile64.h's pipeline
//             (fp64 MFMA, 16-row stages, double-buffered LDS, row slices): both column panels
//             are centred in fp64 ((double)x - (double)mean, exact, as astype(float64) - mean)
//             while they are staged; a diagonal tile stages one panel for both operands.
//             k_cov_reduce adds the slices in fixed order, divides by the denominator and
//             writes each entry and its mirror (the result is exactly symmetric, like the
//             reference's batch.T @ batch).
//             k_cov<.., true> centres about an fp64 mean instead (the eigenspectrum's Gram,
//             vr_centred_gram64_f32): per column as above, or, read transposed, per contraction
//             index for the n x n form.
// Roofline: fp64 MFMA, algorithmic FLOPs = n p (p + 1) (the unique entries i <= j).
#include "tile64.h"

namespace vr {

// ------------------------------------------------------------------------------------
// column sums in numpy's order
// ------------------------------------------------------------------------------------
constexpr int MS_THREADS = 1024;        // 16 waves: wave 0 adds, waves 1..15 load
constexpr int MS_COLS = 64;             // columns per workgroup (one per lane of wave 0)
constexpr int MS_HALF = 240;            // rows per ring half (15 loader waves x 16 rows)

__global__ __launch_bounds__(MS_THREADS) void k_col_sum(const float* __restrict__ X, int64_t n, int64_t p,
                                                        int64_t ldx, const float* __restrict__ init,
                                                        float* __restrict__ sum) {
  __shared__ float ring[2][MS_HALF][MS_COLS];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t col = (int64_t)blockIdx.x * MS_COLS + lane;
  const bool cin = col < p;
  const int64_t nh = (n + MS_HALF - 1) / MS_HALF;
  // loader wave w (1..15) fills rows [16 (w - 1), 16 w) of a half
  auto fill = [&](int64_t h, int buf) {
    const int64_t r0 = h * MS_HALF + 16 * (wid - 1);
    float v[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = (cin && r0 + i < n) ? X[(r0 + i) * ldx + col] : 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) ring[buf][16 * (wid - 1) + i][lane] = v[i];
  };
  float s = (init != nullptr && cin) ? init[col] : 0.f;
  if (wid > 0 && nh > 0) fill(0, 0);
  __syncthreads();
  for (int64_t h = 0; h < nh; ++h) {
    const int buf = (int)(h & 1);
    if (wid > 0) {
      if (h + 1 < nh) fill(h + 1, buf ^ 1);
    } else {
      const int rows = (int)min<int64_t>(MS_HALF, n - h * MS_HALF);
      for (int i = 0; i < rows; ++i) s = s + ring[buf][i][lane];  // row order, float32
    }
    __syncthreads();
  }
  if (wid == 0 && cin) sum[col] = s;
}

// mean = sum / n in float32 (numpy's true_divide of the float32 sum by the count)
__global__ void k_col_div(const float* __restrict__ sum, int64_t p, float cnt, float* __restrict__ mean) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < p) mean[i] = sum[i] / cnt;
}

// ------------------------------------------------------------------------------------
// fp64 covariance tiles (tile64.h)
// ------------------------------------------------------------------------------------
struct CovParams {
  const float* X;
  int64_t n, p, ldx;
  const float* mean;  // null: uncentred (the ridge Grams)
  double* partial;  // [S][ntile][T64 * T64]
  int T;            // tile rows
  int ntile;        // T (T + 1) / 2
  int S;            // row slices
  int64_t kslice;   // rows per slice (multiple of T64_K)
  bool vec;         // 16-B aligned rows: float4 panel loads
  const double* mean64;  // k_cov<.., true>: the fp64 mean (length p, or n of the contraction when TRANS)
};

// TRANS (the kernel-form ridge Gram X X^T of a row-major (p, n) X): the contraction runs
// along X's rows, so panel entry (k, c) is X[c * ldx + k]. Each thread loads 4 consecutive
// k of one column c (one float4 when aligned) and scatters them down the LDS column.
__device__ inline f32x4 cov_load_t(const CovParams& P, int64_t col0, int64_t k, int64_t k1) {
  const int c = threadIdx.x >> 2, kq = (threadIdx.x & 3) * 4;
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  const int64_t col = col0 + c, r = k + kq;
  if (col >= P.p || r >= k1) return v;
  const float* src = P.X + col * P.ldx + r;
  if (P.vec && r + 4 <= k1) {
    v = *reinterpret_cast<const f32x4*>(src);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (r + e < k1) ? src[e] : 0.f;
  }
  return v;
}

__device__ inline void cov_store_t(double* lds, const f32x4 v) {
  const int c = threadIdx.x >> 2, kq = (threadIdx.x & 3) * 4;
#pragma unroll
  for (int e = 0; e < 4; ++e) lds[(kq + e) * T64_LD + c] = (double)v[e];  // out-of-range entries are 0
}

// ... centred about the fp64 mean of the contraction index (the rows-side centred Gram)
__device__ inline void cov_store_t64(const CovParams& P, double* lds, const f32x4 v, int64_t col0, int64_t k,
                                     int64_t k1) {
  const int c = threadIdx.x >> 2, kq = (threadIdx.x & 3) * 4;
  const bool cin = col0 + c < P.p;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int64_t r = k + kq + e;
    lds[(kq + e) * T64_LD + c] = (cin && r < k1) ? (double)v[e] - P.mean64[r] : 0.0;
  }
}

// tile t of the upper triangle (row-major: (0,0), (0,1), .., (0,T-1), (1,1), ..)
__device__ inline void cov_tile(int t, int T, int& bi, int& bj) {
  int r = 0, start = 0;
  while (start + (T - r) <= t) {
    start += T - r;
    ++r;
  }
  bi = r;
  bj = r + (t - start);
}

// M64: centre about P.mean64 (fp64) instead of P.mean (fp32)
template <bool TRANS, bool M64 = false>
__global__ __launch_bounds__(T64_THREADS, 2) void k_cov(CovParams P) {
  __shared__ __attribute__((aligned(16))) double lds[2][2][T64_STAGE];  // [buf][A/B]
  const int id = (int)xcd_remap(blockIdx.x, gridDim.x);
  const int tile = id / P.S, slice = id % P.S;
  int bi, bj;
  cov_tile(tile, P.T, bi, bj);
  const bool diag = bi == bj;
  const int64_t ci = (int64_t)bi * T64, cj = (int64_t)bj * T64;
  const int64_t k0 = (int64_t)slice * P.kslice;
  const int64_t k1 = min(P.n, k0 + P.kslice);
  const int nk = k1 > k0 ? (int)((k1 - k0 + T64_K - 1) / T64_K) : 0;

  double mA[4], mB[4];
  {
    const int c = (threadIdx.x & 15) * 4;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if constexpr (M64) {
        mA[e] = (!TRANS && ci + c + e < P.p) ? P.mean64[ci + c + e] : 0.0;
        mB[e] = (!TRANS && cj + c + e < P.p) ? P.mean64[cj + c + e] : 0.0;
      } else {
        mA[e] = (P.mean && ci + c + e < P.p) ? (double)P.mean[ci + c + e] : 0.0;
        mB[e] = (P.mean && cj + c + e < P.p) ? (double)P.mean[cj + c + e] : 0.0;
      }
    }
  }
  // TRANS loads hold float4s of 4 consecutive k of one column (see tile64.h on why these stay here)
  auto load = [&](int side, int64_t k) {
    const int64_t col0 = side ? cj : ci;
    return TRANS ? cov_load_t(P, col0, k, k1) : panel_load(P.X, P.ldx, P.p, P.vec, nullptr, col0, k, k1);
  };
  auto store = [&](int side, double* dst, const f32x4 v, int64_t k) {
    if constexpr (TRANS && M64)
      cov_store_t64(P, dst, v, side ? cj : ci, k, k1);
    else if constexpr (TRANS)
      cov_store_t(dst, v);
    else
      panel_store(dst, v, side ? mB : mA, k, k1);
  };
  tile_pipeline(lds, k0, nk, diag, load, store, P.partial + ((int64_t)slice * P.ntile + tile) * (T64 * T64));
}

// sum of the slices in slice order, / denom, into cov (entry and mirror)
__global__ __launch_bounds__(256) void k_cov_reduce(const double* __restrict__ partial, int S, int ntile,
                                                    int T, int64_t p, double denom, double* __restrict__ cov,
                                                    int64_t ldc) {
  const int tile = blockIdx.x;
  int bi, bj;
  cov_tile(tile, T, bi, bj);
  const int64_t ci = (int64_t)bi * T64, cj = (int64_t)bj * T64;
  for (int e = threadIdx.x; e < T64 * T64; e += blockDim.x) {
    const int li = e / T64, lj = e % T64;
    const int64_t i = ci + li, j = cj + lj;
    if (i >= p || j >= p || (bi == bj && li > lj)) continue;
    const double s = slice_sum(partial, S, ntile, tile, e) / denom;
    cov[i * ldc + j] = s;
    if (i != j) cov[j * ldc + i] = s;
  }
}

static void cov_geometry(int64_t n, int64_t p, int& T, int& ntile, int& S, int64_t& kslice) {
  T = (int)((p + T64 - 1) / T64);
  ntile = T * (T + 1) / 2;
  // enough workgroups for ~4 per CU, each slice at least 64 stages of rows
  const int64_t want = std::max<int64_t>(1, (4LL * num_cus() + ntile - 1) / ntile);
  const int64_t maxs = std::max<int64_t>(1, n / (64 * T64_K));
  S = (int)std::min<int64_t>(want, maxs);
  kslice = ((n + S - 1) / S + T64_K - 1) / T64_K * T64_K;
  if (kslice == 0) kslice = T64_K;
  S = (int)std::max<int64_t>(1, (n + kslice - 1) / kslice);
}

// The geometry of a launch, for the workspace size and for cov_launch alike. An empty row
// set (n = 0: a rank with an empty shard) runs as one slice of zero stages, and its
// workgroups still store their all-zero tiles, so it needs one slice of partials.
static void cov_launch_geometry(int64_t n, int64_t p, int& T, int& ntile, int& S, int64_t& kslice) {
  cov_geometry(std::max<int64_t>(n, 1), p, T, ntile, S, kslice);
}

}  // namespace vr

using namespace vr;

extern "C" {

int vr_col_sum_f32(const float* X, int64_t n, int64_t p, int64_t ldx, const float* init, float* sum,
                   void* stream) {
  clear_error();
  VR_REQUIRE(n >= 0 && p >= 0 && ldx >= p, "vr_col_sum_f32: bad shape n=%lld p=%lld ldx=%lld",
             (long long)n, (long long)p, (long long)ldx);
  if (p == 0) return VR_OK;
  VR_REQUIRE(sum != nullptr && (n == 0 || X != nullptr), "vr_col_sum_f32: null pointer");
  const unsigned grid = (unsigned)((p + MS_COLS - 1) / MS_COLS);
  k_col_sum<<<grid, MS_THREADS, 0, as_stream(stream)>>>(X, n, p, ldx, init, sum);
  VR_CHECK_LAUNCH();
  return VR_OK;
}

int vr_col_mean_f32(const float* X, int64_t n, int64_t p, int64_t ldx, float* mean, void* stream) {
  VR_TRY(vr_col_sum_f32(X, n, p, ldx, nullptr, mean, stream));
  if (p == 0) return VR_OK;
  k_col_div<<<(unsigned)((p + 255) / 256), 256, 0, as_stream(stream)>>>(mean, p, (float)n, mean);
  VR_CHECK_LAUNCH();
  return VR_OK;
}

int vr_mean_from_sum_f32(const float* sum, int64_t p, int64_t n, float* mean, void* stream) {
  clear_error();
  VR_REQUIRE(p >= 0 && n >= 0, "vr_mean_from_sum_f32: bad shape");
  if (p == 0) return VR_OK;
  k_col_div<<<(unsigned)((p + 255) / 256), 256, 0, as_stream(stream)>>>(sum, p, (float)n, mean);
  VR_CHECK_LAUNCH();
  return VR_OK;
}

size_t vr_pca_cov_workspace(int64_t n, int64_t p) {
  if (n < 0 || p <= 0) return 256;
  int T, ntile, S;
  int64_t kslice;
  cov_launch_geometry(n, p, T, ntile, S, kslice);
  Carver c(nullptr);
  c.take<double>((size_t)S * ntile * T64 * T64);
  return c.bytes();
}

// (n = contraction length, p = output order) -> k_cov + k_cov_reduce
static int cov_launch(bool trans, const float* X, int64_t n, int64_t p, int64_t ldx, const float* mean,
                      double denom, double* cov, int64_t ldc, void* ws, hipStream_t st,
                      const double* mean64 = nullptr) {
  CovParams P;
  P.mean64 = mean64;
  P.X = X;
  P.n = n;
  P.p = p;
  P.ldx = ldx;
  P.mean = mean;
  cov_launch_geometry(n, p, P.T, P.ntile, P.S, P.kslice);
  Carver c(ws);
  P.partial = c.take<double>((size_t)P.S * P.ntile * T64 * T64);
  P.vec = (ldx % 4 == 0) && ((reinterpret_cast<uintptr_t>(X) & 15) == 0);
  {
    KtScope kt(KT_COV, (double)n * (double)p * (double)(p + 1), st);  // algorithmic FLOPs
    if (mean64 != nullptr && trans)
      k_cov<true, true><<<(unsigned)(P.ntile * P.S), T64_THREADS, 0, st>>>(P);
    else if (mean64 != nullptr)
      k_cov<false, true><<<(unsigned)(P.ntile * P.S), T64_THREADS, 0, st>>>(P);
    else if (trans)
      k_cov<true><<<(unsigned)(P.ntile * P.S), T64_THREADS, 0, st>>>(P);
    else
      k_cov<false><<<(unsigned)(P.ntile * P.S), T64_THREADS, 0, st>>>(P);
    VR_CHECK_LAUNCH();
  }
  k_cov_reduce<<<(unsigned)P.ntile, 256, 0, st>>>(P.partial, P.S, P.ntile, P.T, p, denom, cov, ldc);
  VR_CHECK_LAUNCH();
  return VR_OK;
}

int vr_pca_cov_f64(const float* X, int64_t n, int64_t p, int64_t ldx, const float* mean, double denom,
                   double* cov, int64_t ldc, void* ws, size_t ws_bytes, void* stream) {
  clear_error();
  VR_REQUIRE(n >= 0 && p >= 1 && ldx >= p && ldc >= p, "vr_pca_cov_f64: bad shape n=%lld p=%lld",
             (long long)n, (long long)p);
  VR_REQUIRE(mean != nullptr && cov != nullptr && (n == 0 || X != nullptr), "vr_pca_cov_f64: null pointer");
  VR_REQUIRE(ws_bytes >= vr_pca_cov_workspace(n, p), "vr_pca_cov_f64: workspace too small");
  return cov_launch(false, X, n, p, ldx, mean, denom, cov, ldc, ws, as_stream(stream));
}

size_t vr_gram64_workspace(int64_t n, int64_t p, int rows) {
  return rows ? vr_pca_cov_workspace(p, n) : vr_pca_cov_workspace(n, p);
}

int vr_gram64_f32(const float* X, int64_t n, int64_t p, int64_t ldx, int rows, double* G, int64_t ldg,
                  void* ws, size_t ws_bytes, void* stream) {
  clear_error();
  VR_REQUIRE(n >= 1 && p >= 0 && ldx >= p, "vr_gram64_f32: bad shape n=%lld p=%lld ldx=%lld", (long long)n,
             (long long)p, (long long)ldx);
  VR_REQUIRE(ldg >= (rows ? n : p), "vr_gram64_f32: ldg %lld too small", (long long)ldg);
  VR_REQUIRE(G != nullptr && (p == 0 || X != nullptr), "vr_gram64_f32: null pointer");
  VR_REQUIRE(ws_bytes >= vr_gram64_workspace(n, p, rows), "vr_gram64_f32: workspace too small");
  if (rows) {  // X X^T (n x n): contraction over the p columns, X read transposed
    VR_REQUIRE(p >= 1, "vr_gram64_f32: rows Gram of zero-width X");
    return cov_launch(true, X, p, n, ldx, nullptr, 1.0, G, ldg, ws, as_stream(stream));
  }
  VR_REQUIRE(p >= 1, "vr_gram64_f32: columns Gram of zero-width X");
  return cov_launch(false, X, n, p, ldx, nullptr, 1.0, G, ldg, ws, as_stream(stream));
}

int vr_col_mean_f64(const float* X, int64_t n, int64_t p, int64_t ldx, double* mean, void* stream) {
  clear_error();
  VR_REQUIRE(n >= 1 && p >= 0 && ldx >= p, "vr_col_mean_f64: bad shape n=%lld p=%lld ldx=%lld", (long long)n,
             (long long)p, (long long)ldx);
  if (p == 0) return VR_OK;
  VR_REQUIRE(X != nullptr && mean != nullptr, "vr_col_mean_f64: null pointer");
  return knn_col_mean_f64(X, n, p, ldx, mean, as_stream(stream));
}

size_t vr_centred_gram64_workspace(int64_t n, int64_t p, int rows) { return vr_gram64_workspace(n, p, rows); }

int vr_centred_gram64_f32(const float* X, int64_t n, int64_t p, int64_t ldx, const double* mean, int rows,
                          double denom, double* G, int64_t ldg, void* ws, size_t ws_bytes, void* stream) {
  clear_error();
  VR_REQUIRE(n >= 1 && p >= 1 && ldx >= p, "vr_centred_gram64_f32: bad shape n=%lld p=%lld ldx=%lld",
             (long long)n, (long long)p, (long long)ldx);
  VR_REQUIRE(ldg >= (rows ? n : p), "vr_centred_gram64_f32: ldg %lld too small", (long long)ldg);
  VR_REQUIRE(X != nullptr && mean != nullptr && G != nullptr, "vr_centred_gram64_f32: null pointer");
  if (ws == nullptr || ws_bytes < vr_centred_gram64_workspace(n, p, rows)) {
    set_error("vr_centred_gram64_f32: workspace too small");
    return VR_EWORKSPACE;
  }
  if (rows)  // (X - mean)(X - mean)^T: contraction over the p columns, the mean indexed along it
    return cov_launch(true, X, p, n, ldx, nullptr, denom, G, ldg, ws, as_stream(stream), mean);
  return cov_launch(false, X, n, p, ldx, nullptr, denom, G, ldg, ws, as_stream(stream), mean);
}

}  // extern "C"
