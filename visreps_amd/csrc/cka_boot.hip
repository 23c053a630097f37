// Bootstrapped linear CKA (the reference's analysis/metrics/_cka.py: hsic, cka) of two kernel
// matrices over many stimulus subsets,
//   for s in range(n_bootstrap):
//       idx = rng.choice(n, int(0.9 n), replace=False)
//       scores[s] = cka(K[idx][:, idx], L[idx][:, idx])
// as one masked GEMM on the fp64 MFMA, and the two-pass form of one subset.
//
// With H = I - 1 1^T / k, CKA_s = tr(K_s H L_s H) / sqrt(tr(K_s H K_s H) tr(L_s H L_s H)): the
// (k - 1)^2 of hsic cancels. For symmetric K, L, w the 0/1 indicator of a subset of size k,
// u = K w and v = L w,
//   tr(K_s H L_s H) = w^T (K o L) w - (2 / k) sum_i w_i u_i v_i + (w^T u)(w^T v) / k^2,
// and the other two traces with (K, K) and (L, L). Every trace is unchanged by K -> K - c, so
// with fixed shifts cK, cL the engine works on x = (double)K[i][j] - cK, y = (double)L[i][j] - cL:
// the shifts are the means of the finite entries of the whole matrices rounded to float32 (0 if
// that is not finite), so x and y are exact in fp64 and only condition the sums.
//
// The masked GEMM itself (tiling, W staging, the six staged quantities, the fixed-order tail),
// the W kernels, the shift's division and the host driver are subset_gemm.h / pearson_boot.hip,
// shared with the Pearson engine.
//
// k_cka_shift_rows   per-row sums of the finite entries (the shift's numerator).
// k_ckaboot   subset_gemm.h's full walk: all column panels 0 .. n, no j > i mask (u and v need
//             the whole row, and the product forms take the diagonal and both triangles). Six
//             quantities per (row, subset): sum_j w_j {x, y, x^2, y^2, x y, non-finite}. A
//             non-finite entry of K or L is counted: a subset scores NaN iff some (i, j) with i
//             and j in it, the diagonal included, is non-finite.
//             Epilogue: for a row i in the subset, u = acc x, v = acc y; nine partials u, v,
//             u v, u^2, v^2, sum x^2, sum y^2, sum x y, count; the tail adds them over the 64
//             rows in a fixed order, one fp64 partial per (row tile, quantity, subset).
// k_ckaboot_reduce   adds the row tiles in tile order, forms the traces and the score (not
//             clamped: the reference's is not) or the recompute flag. No floating-point
//             atomics anywhere: scores are bit-identical run to run.
//
// Degenerate subsets. The reference gives NaN (0 / 0) when a centred sub-matrix is exactly
// zero; the one-pass trace T = Sxx - (2 / k) Suu + Su^2 / k^2 (Sxx = sum x^2 over the k^2
// entries, Suu = sum u_i^2, Su = sum u_i) cannot decide that. With e = 2^-53 a sum of m terms in
// any order carries an error <= m e sum|term|:
//   err(Sxx) <= k^2 e Sxx;
//   err(u_i) <= k e sum_j |x_ij|, so err(u_i^2) <= 2 k e (sum_j |x_ij|)^2 <= 2 k^2 e sum_j x_ij^2
//   (Cauchy-Schwarz), the sum over i adds k e Suu <= k^2 e Sxx: err((2 / k) Suu) <= 6 k e Sxx;
//   err(Su) <= k^2 e sum |x|, (sum |x|)^2 <= k^2 Sxx: err(Su^2 / k^2) <= 2 k^2 e Sxx.
// A sub-matrix with centred part zero therefore yields |T| <= (3 k^2 + 6 k) e Sxx <= 6 k^2 e Sxx
// (k >= 2) plus a few e (Sxx + (2 / k) Suu + Su^2 / k^2) from the last operations. Every subset with
//   T <= 8 k^2 2^-53 (Sxx + (2 / k) Suu + Su^2 / k^2 + k^2 c^2)
// for K or L is flagged and recomputed with the two passes below. The last term, the energy of
// the shift over the sub-matrix, is not needed by the bound above; it widens the guard to what
// the unshifted one-pass form would need, so that a sub-matrix constant up to a few float32
// ulps (where the shift makes the one-pass sums nearly exact) also takes the two-pass path and
// every near-degenerate score comes from one piece of code, bit-equal to vr_cka_subset_f32.
// For Grams of centred features the shift is ~0 and the term vanishes. The flags are read back
// once per call, after all the work is enqueued.
//
// Two-pass form (cka_two_pass, vr_cka_subset_f32): pass 1 the fp64 row means of K[idx][:, idx]
// and L[idx][:, idx] read in place and their grand means (the mean of the row means); pass 2
// the three sums of products of the double-centred entries ((x - r_i) - r_j) + g. For a constant
// sub-matrix every centred entry is exactly 0 (k copies of one fp32 value sum exactly in fp64
// while k < 2^29 and the quotient by k gives the value back), so the trace is exactly 0 and the
// score NaN. Non-finite entries propagate to NaN. Fixed summation order throughout.
//
// Preconditions as vr_bootstrap_pearson_f32: the rows of idx hold distinct indices in [0, n)
// (an index outside is skipped by the scatter, never written; the two-pass kernels read
// unchecked), and K, L are symmetric (row sums stand for column sums).
#include <algorithm>
#include <cmath>
#include <vector>

#include "subset_gemm.h"

namespace vr {

constexpr int CB_P = 9;      // u, v, u v, u^2, v^2, sum x^2, sum y^2, sum x y, count

// per-row sums of the finite entries of the whole rows: part[2 a + {0, 1}]
__global__ __launch_bounds__(256) void k_cka_shift_rows(const float* __restrict__ K, const float* __restrict__ L,
                                                        int64_t n, int64_t ld, double* __restrict__ part) {
  __shared__ double red[2][4];
  const int64_t a = blockIdx.x;
  double v[2] = {0.0, 0.0}, s[2];
  for (int64_t b = threadIdx.x; b < n; b += 256) {
    const float x = K[a * ld + b], y = L[a * ld + b];
    if (finite_f32(x)) v[0] += (double)x;
    if (finite_f32(y)) v[1] += (double)y;
  }
  block_sum<2, true>(v, red, s);
  if (threadIdx.x < 2) part[a * 2 + threadIdx.x] = s[threadIdx.x];
}

__global__ __launch_bounds__(SG_THREADS) void k_ckaboot(SubsetParams P) {
  __shared__ __attribute__((aligned(16))) double Ws[2][SG_K * SG_WLD];
  __shared__ double red[4][CB_P][SG_T];
  const int bi = blockIdx.x / P.ST, bs = blockIdx.x % P.ST;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int fm = lane & 15, fk = lane >> 4;
  const int64_t i0 = (int64_t)bi * SG_T, s0 = (int64_t)bs * SG_T;
  f64x4 acc[SG_Q][4];
  subset_walk<false>(P, Ws, i0, s0, wid, fm, fk, acc);

  // the nine partials of the rows that are in the subset
  double t[4][CB_P];
#pragma unroll
  for (int sb = 0; sb < 4; ++sb) {
#pragma unroll
    for (int q = 0; q < CB_P; ++q) t[sb][q] = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t row = i0 + wid * 16 + fk + 4 * r;  // < n_pad
      if (P.W[row * P.s_pad + s0 + sb * 16 + fm] != 0) {
        const double u = acc[0][sb][r], v = acc[1][sb][r];
        t[sb][0] += u;
        t[sb][1] += v;
        t[sb][2] += u * v;
        t[sb][3] += u * u;
        t[sb][4] += v * v;
        t[sb][5] += acc[2][sb][r];
        t[sb][6] += acc[3][sb][r];
        t[sb][7] += acc[4][sb][r];
        t[sb][8] += acc[5][sb][r];
      }
    }
  }
  subset_tail<CB_P>(P, red, bi, s0, wid, fm, fk, t);
}

// one thread per subset: row tiles added in tile order, then the score or the recompute flag
__global__ __launch_bounds__(256) void k_ckaboot_reduce(const double* __restrict__ partial, int T, int64_t s_pad,
                                                        int64_t total, int full_first, double k_full, double k_sub,
                                                        const double* __restrict__ shift,
                                                        double* __restrict__ scores, int32_t* __restrict__ flags) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= total) return;
  double v[CB_P] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int b = 0; b < T; ++b)
#pragma unroll
    for (int q = 0; q < CB_P; ++q) v[q] += partial[((int64_t)b * CB_P + q) * s_pad + s];
  const double k = (full_first && s == 0) ? k_full : k_sub;
  double r = __builtin_nan("");
  int flag = 0;
  if (k >= 2.0 && v[8] == 0.0) {
    const double su = v[0], sv = v[1], suv = v[2], suu = v[3], svv = v[4], sxx = v[5], syy = v[6], sxy = v[7];
    const double k2 = k * k;
    const double ax = 2.0 * suu / k, bx = su * su / k2;
    const double ay = 2.0 * svv / k, by = sv * sv / k2;
    const double tx = (sxx - ax) + bx, ty = (syy - ay) + by;
    const double g = 8.0 * k2 * 0x1p-53;  // the guard bound of the file header
    const double ck = shift[0], cl = shift[1];
    if (!(tx > g * (sxx + ax + bx + k2 * ck * ck)) || !(ty > g * (syy + ay + by + k2 * cl * cl))) {
      flag = 1;  // within rounding of a zero centred sub-matrix: the two-pass recompute decides
    } else {
      r = ((sxy - 2.0 * suv / k) + su * sv / k2) / sqrt(tx * ty);
    }
  }
  scores[s] = r;
  flags[s] = flag;
}

// ---- two-pass form ----------------------------------------------------------------------
// SUB: row a and column b are positions in idx (k of them, n = k). rs[2 a + {0, 1}] = row sums.
template <bool SUB>
__global__ __launch_bounds__(256) void k_cka_rowsum(const float* __restrict__ K, const float* __restrict__ L,
                                                    int64_t n, int64_t ld, const int32_t* __restrict__ idx,
                                                    double* __restrict__ rs) {
  __shared__ double red[2][4];
  const int64_t a = blockIdx.x;
  const int64_t ia = SUB ? (int64_t)idx[a] : a;
  double v[2] = {0.0, 0.0}, s[2];
  for (int64_t b = threadIdx.x; b < n; b += 256) {
    const int64_t at = ia * ld + (SUB ? (int64_t)idx[b] : b);
    v[0] += (double)K[at];
    v[1] += (double)L[at];
  }
  block_sum<2, true>(v, red, s);
  if (threadIdx.x < 2) rs[a * 2 + threadIdx.x] = s[threadIdx.x];
}

// row sums -> row means in place; mu[q] = mean of the row means
__global__ __launch_bounds__(256) void k_cka_means(double* __restrict__ rs, int64_t n, double* __restrict__ mu) {
  __shared__ double red[2][4];
  const double k = (double)n;
  double v[2] = {0.0, 0.0}, s[2];
  for (int64_t a = threadIdx.x; a < n; a += 256) {
    const double m0 = rs[a * 2] / k, m1 = rs[a * 2 + 1] / k;
    rs[a * 2] = m0;
    rs[a * 2 + 1] = m1;
    v[0] += m0;
    v[1] += m1;
  }
  block_sum<2, true>(v, red, s);
  if (threadIdx.x < 2) mu[threadIdx.x] = s[threadIdx.x] / k;
}

// sums over row a of the products of the double-centred entries: p3[3 a + {0, 1, 2}] = KL, KK, LL
template <bool SUB>
__global__ __launch_bounds__(256) void k_cka_centred(const float* __restrict__ K, const float* __restrict__ L,
                                                     int64_t n, int64_t ld, const int32_t* __restrict__ idx,
                                                     const double* __restrict__ rm, const double* __restrict__ mu,
                                                     double* __restrict__ p3) {
  __shared__ double red[3][4];
  const int64_t a = blockIdx.x;
  const int64_t ia = SUB ? (int64_t)idx[a] : a;
  const double rka = rm[a * 2], rla = rm[a * 2 + 1], gk = mu[0], gl = mu[1];
  double v[3] = {0.0, 0.0, 0.0}, s[3];
  for (int64_t b = threadIdx.x; b < n; b += 256) {
    const int64_t at = ia * ld + (SUB ? (int64_t)idx[b] : b);
    const double dx = (((double)K[at] - rka) - rm[b * 2]) + gk;
    const double dy = (((double)L[at] - rla) - rm[b * 2 + 1]) + gl;
    v[0] += dx * dy;
    v[1] += dx * dx;
    v[2] += dy * dy;
  }
  block_sum<3, true>(v, red, s);
  if (threadIdx.x < 3) p3[a * 3 + threadIdx.x] = s[threadIdx.x];
}

__global__ __launch_bounds__(256) void k_cka_final(const double* __restrict__ p3, int64_t n, double* __restrict__ out,
                                                   int n_out) {
  __shared__ double red[3][4];
  double v[3] = {0.0, 0.0, 0.0}, s[3];
  for (int64_t a = threadIdx.x; a < n; a += 256)
#pragma unroll
    for (int q = 0; q < 3; ++q) v[q] += p3[a * 3 + q];
  block_sum<3, true>(v, red, s);
  if (threadIdx.x == 0) {
    // an exactly zero centred sub-matrix or non-finite input: undefined, as the reference's 0 / 0
    const bool ok = n >= 2 && s[1] > 0 && s[2] > 0;
    out[0] = ok ? s[0] / sqrt(s[1] * s[2]) : __builtin_nan("");
    if (n_out == 4) {
      out[1] = s[0];
      out[2] = s[1];
      out[3] = s[2];
    }
  }
}

int cka_two_pass(const float* K, const float* L, int64_t n_or_k, int64_t ld, const int32_t* idx, double* out,
                 int n_out, double* part, double* mu, hipStream_t st) {
  const int64_t n = n_or_k;
  double* rm = part;           // 2 n
  double* p3 = part + 2 * n;   // 3 n
  if (idx)
    k_cka_rowsum<true><<<(unsigned)n, 256, 0, st>>>(K, L, n, ld, idx, rm);
  else
    k_cka_rowsum<false><<<(unsigned)n, 256, 0, st>>>(K, L, n, ld, nullptr, rm);
  VR_CHECK_LAUNCH();
  k_cka_means<<<1, 256, 0, st>>>(rm, n, mu);
  VR_CHECK_LAUNCH();
  if (idx)
    k_cka_centred<true><<<(unsigned)n, 256, 0, st>>>(K, L, n, ld, idx, rm, mu, p3);
  else
    k_cka_centred<false><<<(unsigned)n, 256, 0, st>>>(K, L, n, ld, nullptr, rm, mu, p3);
  VR_CHECK_LAUNCH();
  k_cka_final<<<1, 256, 0, st>>>(p3, n, out, n_out);
  VR_CHECK_LAUNCH();
  return VR_OK;
}

static size_t cka_subset_ws(int64_t k, double** part, double** mu, void* ws) {
  Carver c(ws);
  double* p = c.take<double>((size_t)std::max<int64_t>(k, 1) * 5);
  double* m = c.take<double>(2);
  if (part) *part = p;
  if (mu) *mu = m;
  return c.bytes();
}

static const SubsetEngine CKA_BOOT = {
    "vr_bootstrap_cka_f32",
    CB_P,
    [](const float* K, const float* L, int64_t n, int64_t ld, double* part, hipStream_t st) -> int {
      k_cka_shift_rows<<<(unsigned)n, 256, 0, st>>>(K, L, n, ld, part);
      VR_CHECK_LAUNCH();
      return VR_OK;
    },
    [](int64_t n) { return (double)n * (double)n; },
    [](const SubsetParams& P, int T, hipStream_t st) -> int {
      k_ckaboot<<<(unsigned)(T * P.ST), SG_THREADS, 0, st>>>(P);
      VR_CHECK_LAUNCH();
      return VR_OK;
    },
    [](const SubsetLayout& Y, int64_t n, int64_t k, int64_t total, int full_first, double* scores,
       hipStream_t st) -> int {
      k_ckaboot_reduce<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(
          Y.partial, Y.T, Y.s_pad, total, full_first, (double)n, (double)k, Y.shift, scores, Y.flags);
      VR_CHECK_LAUNCH();
      return VR_OK;
    },
    [](const float* K, const float* L, int64_t n_or_k, int64_t ld, const int32_t* idx, double* out, double* part,
       double* mu, hipStream_t st) -> int { return cka_two_pass(K, L, n_or_k, ld, idx, out, 1, part, mu, st); },
};

}  // namespace vr

using namespace vr;

extern "C" {

size_t vr_bootstrap_cka_workspace(int64_t n, int64_t n_sets) {
  return subset_layout(nullptr, n, std::max<int64_t>(n_sets, 0) + 1, CKA_BOOT.np).bytes;
}

int vr_bootstrap_cka_f32(const float* K, const float* L, int64_t n, int64_t ld, const int32_t* idx, int64_t k,
                         int64_t n_sets, int full_first, double* scores, void* ws, size_t ws_bytes, void* stream) {
  return subset_bootstrap(CKA_BOOT, K, L, n, ld, idx, k, n_sets, full_first, scores, ws, ws_bytes, stream);
}

size_t vr_cka_subset_workspace(int64_t k) { return cka_subset_ws(k, nullptr, nullptr, nullptr); }

int vr_cka_subset_f32(const float* K, const float* L, int64_t n, int64_t ld, const int32_t* idx, int64_t k,
                      double* out, void* ws, size_t ws_bytes, void* stream) {
  clear_error();
  VR_REQUIRE(n >= 0 && ld >= n && k >= 0 && k <= n && (idx != nullptr || k == n),
             "vr_cka_subset_f32: bad shape n=%lld ld=%lld k=%lld", (long long)n, (long long)ld, (long long)k);
  const size_t need = vr_cka_subset_workspace(k);
  if (ws_bytes < need || ws == nullptr) {
    set_error("vr_cka_subset_f32: workspace %zu < %zu", ws_bytes, need);
    return VR_EWORKSPACE;
  }
  VR_REQUIRE(out != nullptr, "vr_cka_subset_f32: null pointer");
  hipStream_t st = as_stream(stream);
  if (k < 2) {  // a single stimulus centres to zero: 0 / 0
    const double nan = std::nan("");
    const double four[4] = {nan, nan, nan, nan};
    VR_CHECK_HIP(hipMemcpyAsync(out, four, sizeof(four), hipMemcpyHostToDevice, st));
    VR_CHECK_HIP(hipStreamSynchronize(st));
    return VR_OK;
  }
  VR_REQUIRE(K != nullptr && L != nullptr, "vr_cka_subset_f32: null pointer");
  double *part, *mu;
  cka_subset_ws(k, &part, &mu, ws);
  return cka_two_pass(K, L, k, ld, idx, out, 4, part, mu, st);
}

}  // extern "C"
