// Internal (non-ABI) declarations shared between the .hip translation units.
#pragma once

#include "common.h"

namespace vr {

// ---- device-wide exclusive scan of uint32 (scan.hip) -------------------------------
constexpr int SCAN_BS = 256;
constexpr int SCAN_IPT = 16;
constexpr int SCAN_TILE = SCAN_BS * SCAN_IPT;
size_t scan_ws_elems(int64_t n);  // uint32 elements of scratch
// out[i] = sum(in[0:i]); *total_dev (if non-null) = sum(in). in may alias out.
int scan_exclusive_u32(const uint32_t* in, uint32_t* out, int64_t n, uint32_t* total_dev,
                       uint32_t* ws, hipStream_t st);

// ---- LSD radix sort of (uint32 key, uint32 value) pairs (sort.hip) -----------------
constexpr int RS_BS = 256;
constexpr int RS_IPT = 16;
constexpr int RS_TILE = RS_BS * RS_IPT;
// One LSD pass (8-bit digit at `shift`) of (ki, vi) into (ko, vo): the building block of
// radix_sort_kv, also the engine's partition of (B position, A position) pairs.
int radix_pass_kv(const uint32_t* ki, const uint32_t* vi, uint32_t* ko, uint32_t* vo, int64_t n,
                  int shift, uint32_t* ws, hipStream_t st);
size_t radix_ws_elems(int64_t n);  // uint32 elements of scratch (histograms + scan)
// An upper bound of radix_ws_elems(n) that is non-decreasing in n, for workspace queries that
// promise monotone sizes.
size_t radix_ws_elems_bound(int64_t n);
// The pass's offsets alone: ws[tile * 256 + d] = output position of tile `tile`'s first key
// of digit d (tiles of RS_TILE keys), for kernels that scatter their own records.
int radix_offsets(const uint32_t* ki, int64_t n, int shift, uint32_t* ws, hipStream_t st);
// One pass on keys alone (no values).
int radix_pass_k(const uint32_t* ki, uint32_t* ko, int64_t n, int shift, uint32_t* ws, hipStream_t st);
// Sorts ascending by key, stable. keys/vals hold the result; *_alt are ping-pong
// buffers of the same length.
int radix_sort_kv(uint32_t* keys, uint32_t* vals, uint32_t* keys_alt, uint32_t* vals_alt,
                  int64_t n, uint32_t* ws, hipStream_t st);

// ---- two-pass fp64 Pearson of two RDM triangles (pearson.hip) ----------------------
// idx == nullptr: the full n_or_k x n_or_k triangle; else the sub-RDM of the n_or_k stimuli
// idx[0..n_or_k), read in place. part: 5 n_or_k doubles, mu: 2 doubles, out: 1 double.
int pearson_two_pass(const float* A, const float* B, int64_t n_or_k, int64_t ld, const int32_t* idx,
                     double* out, double* part, double* mu, hipStream_t st);

// After the call part still holds the second pass's per-row sums, 5 doubles per row:
// [.., .., sum dx dy, sum dx dx, sum dy dy] (mantel.hip re-adds the last two).

// ---- symmetric copy of a strict upper triangle (mantel.hip) --------------------------
// out (n x n, leading dimension ldo) = A's strict upper triangle mirrored, diagonal 0; 32-bit
// entries moved as bit patterns (fp32 or u32). A's diagonal and lower triangle are not read.
// out may be A.
int mirror_upper_u32(const uint32_t* A, int64_t n, int64_t ld, uint32_t* out, int64_t ldo, hipStream_t st);

// ---- two-pass fp64 CKA traces of two kernel matrices (cka_boot.hip) -----------------
// idx == nullptr: the full n_or_k x n_or_k matrices; else K[idx][:, idx], L[idx][:, idx] read in
// place. part: 5 n_or_k doubles, mu: 2 doubles. out: n_out doubles, 1 (the CKA) or 4 (CKA,
// tr(KHLH), tr(KHKH), tr(LHLH)).
int cka_two_pass(const float* K, const float* L, int64_t n_or_k, int64_t ld, const int32_t* idx,
                 double* out, int n_out, double* part, double* mu, hipStream_t st);

// ---- fp64 column means of fp32 rows (knn.hip: k_knn_colsum / k_knn_colmean) ----------
// mean[c] = (sum over rows, in row order, of (double)X[r][c]) / n for c < d. No workspace.
int knn_col_mean_f64(const float* X, int64_t n, int64_t d, int64_t ldx, double* mean, hipStream_t st);

// ---- block-level helpers -----------------------------------------------------------
// Exclusive scan across a block of BS threads (BS multiple of 64, <= 1024).
// lds must hold BS/64 + 1 uint32. Returns this thread's exclusive prefix; total = sum.
template <int BS>
__device__ inline uint32_t block_exclusive_scan(uint32_t v, uint32_t* lds, uint32_t& total) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  uint32_t x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    uint32_t y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  if (lane == 63) lds[wid] = x;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t s = 0;
    for (int w = 0; w < BS / 64; ++w) {
      uint32_t t = lds[w];
      lds[w] = s;
      s += t;
    }
    lds[BS / 64] = s;
  }
  __syncthreads();
  uint32_t r = x - v + lds[wid];
  total = lds[BS / 64];
  __syncthreads();
  return r;
}

// Vector registers of the fp64-MFMA engines (tile64.h, subset_gemm.h).
typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// Block sum of Q doubles per thread, 256 threads, red[Q][4] in LDS: a shuffle tree per wave,
// then the four wave sums in wave order. The sums feed fp64 results, so each caller keeps the
// association it has always had: PAIRS adds (r0 + r1) + (r2 + r3), else r0 + r1 + r2 + r3.
// block_sum_waves leaves the wave sums in red (barrier included) for callers where one thread
// per quantity finishes; block_sum hands every thread every total.
template <int Q>
__device__ inline void block_sum_waves(const double (&v)[Q], double (*red)[4]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    double t = v[q];
    for (int o = 32; o > 0; o >>= 1) t += __shfl_down(t, o, 64);
    if (lane == 0) red[q][w] = t;
  }
  __syncthreads();
}

template <bool PAIRS>
__device__ inline double block_sum_total(const double (&r)[4]) {
  return PAIRS ? (r[0] + r[1]) + (r[2] + r[3]) : r[0] + r[1] + r[2] + r[3];
}

template <int Q, bool PAIRS>
__device__ inline void block_sum(const double (&v)[Q], double (*red)[4], double (&out)[Q]) {
  block_sum_waves<Q>(v, red);
#pragma unroll
  for (int q = 0; q < Q; ++q) out[q] = block_sum_total<PAIRS>(red[q]);
}

// Padded LDS index for tiles read both striped (lane-contiguous) and blocked (16
// consecutive per thread): one pad dword per 32 keeps both patterns conflict-free.
// Block -> work item for a 1-D grid of nb items such that the blocks one XCD receives
// (blockIdx % 8 equal, as the dispatcher deals them) take consecutive items: neighbouring
// items' partial-line writes then meet in one L2.
__device__ inline int64_t xcd_item(int64_t nb) {
  const int64_t b = blockIdx.x, x = b & 7, k = b >> 3, per = nb >> 3, rem = nb & 7;
  return x * per + (x < rem ? x : rem) + k;
}

__device__ inline int lds_pad(int p) { return p + (p >> 5); }

// Sortable transform of an fp32 value: ascending uint32 order == ascending float order,
// -0.0 canonicalised to +0.0 so the two tie (scipy.stats.rankdata semantics).
__device__ inline uint32_t f32_sort_key(float f) {
  uint32_t u = __float_as_uint(f);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

}  // namespace vr

// ---- kernel-level HIP-event timing of the hot kernels (ktimer.cpp) -----------------
// Off by default (vr_ktimer_enable). A KtScope records an event on the launch stream
// before and after the one launch it brackets; vr_ktimer_read resolves them.
namespace vr {
enum KtKernel : int {
  KT_RANKB_EST = 0,   // k_rankB, EST forms over bootstrap subsets (EST 3; the table form EST 1)
  KT_RANKB_EXACT = 1, // k_rankB, exact chunk-base form (VISREPS_ENGINE_EST=0, flagged reruns)
  KT_RANKA = 2,       // k_rankA (both forms)
  KT_JOIN = 3,        // k_join: a unit's A positions (and, for the exact form, A chunks)
  KT_GRAM_WIDE = 4,   // k_gram3e (256^2 super-tiles)
  KT_GRAM_TILE = 5,   // k_gram3 / k_gram (128^2 tiles)
  KT_COUNTA = 6,      // k_countA
  KT_RANKB_FULL = 7,  // k_rankB on the pass holding the full stimulus set (EST 4 A side: EST 3 B walks)
  KT_KWALK = 8,       // k_kwalk: one Kendall stream walk (inversion level or tie stream) of one pass
  KT_COV = 9,         // k_cov: fp64 MFMA covariance / Gram tiles (PCA covariance, ridge kernel matrix)
  KT_JOIN4 = 10,      // k_join4: shared join of one B plan to up to 4 A plans (units = algorithmic bytes)
  KT_FULL_CORR = 11,  // k_full_corr: lane 0's shift sums of an EST 4 pass, per unit (4 B / pair streamed)
  KT_RANKB_GRID = 12,  // k_rankB_grid: one B plan x up to 4 regions, EST 3 (units: pairs x regions)
  KT_KNN_STAGE = 13,  // knn.hip: column means, centred copy, norms (units: bytes of X read)
  KT_KNN_CAND = 14,   // k_knn_cand (units: fp32 FLOPs of the tiles walked)
  KT_KNN_RERANK = 15, // k_knn_merge + k_knn_rerank (units: candidate pairs)
  KT_KNN_EXACT = 16,  // k_knn_exact_rows (units: pairs scanned)
  KT_EIG_TRIDIAG = 17,  // eigvals.hip stage A: all Householder steps of one call (units: bytes of A22 moved)
  KT_EIG_BISECT = 18,   // eigvals.hip stage B: bounds + bisection (units: Sturm terms)
  KT_EIG_INVIT = 19,    // eigvals.hip stage C: shifts, start, inverse iterations + Gram-Schmidt (units: solve steps)
  KT_EIG_BACK = 20,     // eigvals.hip stage D: k_eigv_back (units: bytes of reflectors read)
  KT_SVD_STAGE = 21,    // svd.hip: transpose staging, R = I, the first row norms, setup (units: bytes moved)
  KT_SVD_STEP = 22,     // svd.hip: the k_svd_step launches of one sweep, R replay included (units: 3 n^2 L FLOPs per member)
  KT_SVD_FINISH = 23,   // svd.hip: final row norms + k_svd_finish (units: bytes moved)
  KT_N = 24
};
bool ktimer_on();
struct KtScope {
  KtScope(int kernel, double units, hipStream_t st);  // units: pairs (engine) or FLOPs (Gram)
  ~KtScope();
  int kernel;
  double units;
  hipStream_t st;
  hipEvent_t e0 = nullptr;
};
}  // namespace vr
