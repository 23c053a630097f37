// Bootstrapped Pearson RSA: the loop of rsa.py:233-261 / evals.py:355-373 with
// compare_method="pearson",
//   for s in range(n_bootstrap):
//       idx = rng.choice(n, int(0.9 n), replace=False)
//       scores[s] = pearsonr(triu(A[idx][:, idx]), triu(B[idx][:, idx]))
// as one masked GEMM on the fp64 MFMA instead of one gather + reduction per draw.
//
// W is the n x S 0/1 indicator matrix of the subsets (W[i][s] = 1 iff stimulus i is in subset
// s; column 0 all ones for the full set when full_first). With fixed shifts ca, cb and, for
// every pair i < j of the strict upper triangle, x = (double)A[i][j] - ca,
// y = (double)B[i][j] - cb, the five sums of a subset are quadratic forms in its column of W,
//   S_v[s] = sum_i W[i][s] sum_{j > i} v(i, j) W[j][s],   v in {x, y, x^2, y^2, x y},
// and r[s] = (S_xy - S_x S_y / m) / sqrt((S_xx - S_x^2 / m)(S_yy - S_y^2 / m)), m = k(k-1)/2.
// Pearson is shift-invariant; the shifts only condition the sums. They are the full-triangle
// means of the finite values rounded to float32, so x and y are exact in fp64.
//
// The masked GEMM itself (tiling, W staging, the six staged quantities, the fixed-order tail) is
// subset_gemm.h, shared with cka_boot.hip; so are the W kernels, the shift and the host driver
// below, which both engines run.
//
// k_pboot_fill / k_pboot_scatter   W as bytes (n_pad x s_pad, both padded to 64 and zero
//             there), plain byte / dword stores.
// k_pboot_shift_rows / k_pboot_shift   the two shifts (sums over finite values only, so a NaN
//             in an RDM does not poison them).
// k_pboot     subset_gemm.h's triangle walk: column panels from the workgroup's own row block
//             to n, only upper-triangle tiles are visited, j > i is masked per element inside
//             the diagonal block. The sixth quantity counts non-finite pairs: a subset whose
//             count is non-zero scores NaN, as scipy and vr_pearson_triu_f32 do for NaN / Inf
//             input. Epilogue: rows not in the subset are dropped (W[i][s]), the tail adds the
//             64 rows in a fixed order, one fp64 partial per (row tile, quantity, subset).
// k_pboot_reduce   adds the row tiles in tile order and forms r; no floating-point atomics
//             anywhere, so scores are bit-identical run to run.
// Row tile bi walks T - bi column blocks, so workgroups are numbered heaviest first.
//
// Degenerate subsets. The reference returns NaN for an exactly constant sub-triangle; the
// one-pass variance S_vv - S_v^2 / m cannot decide that. With u = 2^-53, a sum of m terms in
// any order carries an error <= m u sum|v|, so err(S_vv) <= m u S_vv, and with
// |S_v| <= sqrt(m S_vv) (Cauchy-Schwarz) err(S_v^2 / m) <= 2 m u S_vv: a constant sub-triangle
// yields |S_vv - S_v^2 / m| <= 3 m u S_vv plus a few u (S_vv + S_v^2 / m) from the last three
// operations. Every subset with  S_vv - S_v^2/m <= 8 m 2^-53 (S_vv + S_v^2/m)  for v = x or y
// is flagged and recomputed with the two passes of pearson.hip on the sub-RDM read in place
// (exact for constants: sums of one repeated fp32 value are exact in fp64 while m < 2^29).
// The flags are read back once per call, after all the work is enqueued.
//
// Preconditions, as for the rank-plan engines: the rows of idx hold distinct indices in
// [0, n) (an index outside is skipped by the scatter, never written), and the RDMs are
// symmetric: the engine reads the upper triangle whatever the order of idx. There are no
// 16-bit pair codes here, so no n <= 65,535 limit.
#include <algorithm>
#include <cmath>
#include <vector>

#include "subset_gemm.h"

namespace vr {

// W words: 1 in column 0 of the rows < n when full_first, else 0
__global__ void k_pboot_fill(uint32_t* __restrict__ W, int64_t n, int64_t n_pad, int64_t s_pad, int full_first) {
  const int64_t wpr = s_pad / 4;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_pad * wpr) return;
  const int64_t row = i / wpr, w = i % wpr;
  W[i] = (full_first && w == 0 && row < n) ? 1u : 0u;
}

__global__ void k_pboot_scatter(uint8_t* __restrict__ W, const int32_t* __restrict__ idx, int64_t n, int64_t k,
                                int64_t n_sets, int64_t s_pad, int off) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_sets * k) return;
  const int64_t s = t / k;
  const int64_t i = idx[t];
  if (i < 0 || i >= n) return;  // outside the precondition: never written
  W[i * s_pad + off + s] = 1;
}

// per-row sums of the finite values of the strict upper triangle: part[2 a + {0, 1}]
__global__ __launch_bounds__(256) void k_pboot_shift_rows(const float* __restrict__ A, const float* __restrict__ B,
                                                          int64_t n, int64_t ld, double* __restrict__ part) {
  __shared__ double red[2][4];
  const int64_t a = blockIdx.x;
  double v[2] = {0.0, 0.0};
  for (int64_t b = a + 1 + threadIdx.x; b < n; b += 256) {
    const float x = A[a * ld + b], y = B[a * ld + b];
    if (finite_f32(x)) v[0] += (double)x;
    if (finite_f32(y)) v[1] += (double)y;
  }
  block_sum_waves<2>(v, red);
  if (threadIdx.x < 2) part[a * 2 + threadIdx.x] = block_sum_total<false>(red[threadIdx.x]);
}

// shift[q] = float32(sum / M), 0 if that is not finite
__global__ __launch_bounds__(256) void k_pboot_shift(const double* __restrict__ part, int64_t n, double M,
                                                     double* __restrict__ shift) {
  __shared__ double red[2][4];
  double v[2] = {0.0, 0.0};
  for (int64_t a = threadIdx.x; a < n; a += 256) {
    v[0] += part[a * 2];
    v[1] += part[a * 2 + 1];
  }
  block_sum_waves<2>(v, red);
  if (threadIdx.x < 2) {
    const float m = (float)(block_sum_total<false>(red[threadIdx.x]) / M);
    shift[threadIdx.x] = finite_f32(m) ? (double)m : 0.0;
  }
}

// W: n_pad x s_pad bytes (both multiples of 64), W[i][off + s] = 1 iff stimulus i is in row s of
// idx (n_sets x k), column 0 all ones over the rows < n when off == 1, 0 elsewhere.
static int pboot_build_w(uint8_t* W, const int32_t* idx, int64_t n, int64_t k, int64_t n_sets, int64_t n_pad,
                  int64_t s_pad, int off, hipStream_t st) {
  const int64_t words = n_pad * (s_pad / 4);
  k_pboot_fill<<<(unsigned)((words + 255) / 256), 256, 0, st>>>(reinterpret_cast<uint32_t*>(W), n, n_pad, s_pad, off);
  VR_CHECK_LAUNCH();
  if (n_sets * k > 0) {
    k_pboot_scatter<<<(unsigned)((n_sets * k + 255) / 256), 256, 0, st>>>(W, idx, n, k, n_sets, s_pad, off);
    VR_CHECK_LAUNCH();
  }
  return VR_OK;
}

// shift[q] = float32((sum_a part[2 a + q]) / M) as a double, 0 if that is not finite (q = 0, 1)
static int pboot_shift(const double* part, int64_t n, double M, double* shift, hipStream_t st) {
  k_pboot_shift<<<1, 256, 0, st>>>(part, n, M, shift);
  VR_CHECK_LAUNCH();
  return VR_OK;
}

__global__ __launch_bounds__(SG_THREADS) void k_pboot(SubsetParams P) {
  __shared__ __attribute__((aligned(16))) double Ws[2][SG_K * SG_WLD];
  __shared__ double red[4][SG_Q][SG_T];
  const int bi = blockIdx.x / P.ST, bs = blockIdx.x % P.ST;  // bi ascending: heaviest first
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int fm = lane & 15, fk = lane >> 4;
  const int64_t i0 = (int64_t)bi * SG_T, s0 = (int64_t)bs * SG_T;
  f64x4 acc[SG_Q][4];
  subset_walk<true>(P, Ws, i0, s0, wid, fm, fk, acc);

  // keep the rows that are in the subset
  double t[4][SG_Q];
#pragma unroll
  for (int sb = 0; sb < 4; ++sb) {
    bool keep[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t row = i0 + wid * 16 + fk + 4 * r;  // < n_pad
      keep[r] = P.W[row * P.s_pad + s0 + sb * 16 + fm] != 0;
    }
#pragma unroll
    for (int q = 0; q < SG_Q; ++q) {
      t[sb][q] = 0.0;
#pragma unroll
      for (int r = 0; r < 4; ++r) t[sb][q] += keep[r] ? acc[q][sb][r] : 0.0;
    }
  }
  subset_tail<SG_Q>(P, red, bi, s0, wid, fm, fk, t);
}

// one thread per subset: row tiles added in tile order, then the score or the recompute flag
__global__ __launch_bounds__(256) void k_pboot_reduce(const double* __restrict__ partial, int T, int64_t s_pad,
                                                      int64_t total, int full_first, double m_full, double m_sub,
                                                      double* __restrict__ scores, int32_t* __restrict__ flags) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= total) return;
  double v[SG_Q] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int b = 0; b < T; ++b)
#pragma unroll
    for (int q = 0; q < SG_Q; ++q) v[q] += partial[((int64_t)b * SG_Q + q) * s_pad + s];
  const double m = (full_first && s == 0) ? m_full : m_sub;
  double r = __builtin_nan("");
  int flag = 0;
  if (m >= 2.0 && v[5] == 0.0) {
    const double ex = v[0] * v[0] / m, ey = v[1] * v[1] / m;
    const double vx = v[2] - ex, vy = v[3] - ey;
    const double g = 8.0 * m * 0x1p-53;  // the guard bound of the file header
    if (!(vx > g * (v[2] + ex)) || !(vy > g * (v[3] + ey))) {
      flag = 1;  // within rounding of constant: the two-pass recompute decides
    } else {
      r = (v[4] - v[0] * v[1] / m) / sqrt(vx * vy);
      r = r > 1.0 ? 1.0 : (r < -1.0 ? -1.0 : r);
    }
  }
  scores[s] = r;
  flags[s] = flag;
}

__global__ void k_pboot_nan(double* __restrict__ scores, int64_t total) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s < total) scores[s] = __builtin_nan("");
}

SubsetLayout subset_layout(void* ws, int64_t n, int64_t total, int np) {
  SubsetLayout L;
  const int64_t nn = std::max<int64_t>(n, 1), tt = std::max<int64_t>(total, 1);
  L.n_pad = (nn + SG_T - 1) / SG_T * SG_T;
  L.s_pad = (tt + SG_T - 1) / SG_T * SG_T;
  L.T = (int)(L.n_pad / SG_T);
  L.ST = (int)(L.s_pad / SG_T);
  Carver c(ws);
  L.W = c.take<uint8_t>((size_t)L.n_pad * L.s_pad);
  L.partial = c.take<double>((size_t)L.T * np * L.s_pad);
  L.part = c.take<double>((size_t)nn * 5);
  L.mu = c.take<double>(2);
  L.shift = c.take<double>(2);
  L.flags = c.take<int32_t>((size_t)L.s_pad);
  L.bytes = c.bytes();
  return L;
}

int subset_bootstrap(const SubsetEngine& E, const float* A, const float* B, int64_t n, int64_t ld,
                     const int32_t* idx, int64_t k, int64_t n_sets, int full_first, double* scores, void* ws,
                     size_t ws_bytes, void* stream) {
  clear_error();
  VR_REQUIRE(n >= 0 && ld >= n && n_sets >= 0 && k >= 0 && k <= n, "%s: bad shape n=%lld ld=%lld k=%lld n_sets=%lld",
             E.name, (long long)n, (long long)ld, (long long)k, (long long)n_sets);
  const int off = full_first ? 1 : 0;
  const int64_t total = n_sets + off;
  // every call fits the workspace of its (n, n_sets): the layout is monotone in both
  const size_t need = subset_layout(nullptr, n, total, E.np).bytes;
  if (ws_bytes < need || ws == nullptr) {
    set_error("%s: workspace %zu < %zu", E.name, ws_bytes, need);
    return VR_EWORKSPACE;
  }
  if (total == 0) return VR_OK;
  VR_REQUIRE(scores != nullptr && (n_sets == 0 || idx != nullptr) && (n < 2 || (A != nullptr && B != nullptr)),
             "%s: null pointer", E.name);
  hipStream_t st = as_stream(stream);
  if (n < 2) {  // no pair at all; a single stimulus centres to zero
    k_pboot_nan<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(scores, total);
    VR_CHECK_LAUNCH();
    return VR_OK;
  }
  const SubsetLayout L = subset_layout(ws, n, total, E.np);
  VR_TRY(pboot_build_w(L.W, idx, n, k, n_sets, L.n_pad, L.s_pad, off, st));
  VR_TRY(E.shift_rows(A, B, n, ld, L.part, st));
  VR_TRY(pboot_shift(L.part, n, E.shift_denom(n), L.shift, st));
  SubsetParams P;
  P.A = A;
  P.B = B;
  P.n = n;
  P.ld = ld;
  P.W = L.W;
  P.s_pad = L.s_pad;
  P.shift = L.shift;
  P.partial = L.partial;
  P.ST = L.ST;
  P.vec = (ld % 4 == 0) && ((reinterpret_cast<uintptr_t>(A) & 15) == 0) && ((reinterpret_cast<uintptr_t>(B) & 15) == 0);
  VR_TRY(E.walk(P, L.T, st));
  VR_TRY(E.reduce(L, n, k, total, off, scores, st));
  // the one read-back of the call: which subsets the one-pass sums could not decide
  std::vector<int32_t> flags((size_t)total);
  VR_CHECK_HIP(hipMemcpyAsync(flags.data(), L.flags, (size_t)total * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  VR_CHECK_HIP(hipStreamSynchronize(st));
  for (int64_t s = 0; s < total; ++s) {
    if (!flags[(size_t)s]) continue;
    if (off && s == 0)
      VR_TRY(E.two_pass(A, B, n, ld, nullptr, scores, L.part, L.mu, st));
    else
      VR_TRY(E.two_pass(A, B, k, ld, idx + (s - off) * k, scores + s, L.part, L.mu, st));
  }
  return VR_OK;
}

static const SubsetEngine PEARSON_BOOT = {
    "vr_bootstrap_pearson_f32",
    SG_Q,
    [](const float* A, const float* B, int64_t n, int64_t ld, double* part, hipStream_t st) -> int {
      k_pboot_shift_rows<<<(unsigned)n, 256, 0, st>>>(A, B, n, ld, part);
      VR_CHECK_LAUNCH();
      return VR_OK;
    },
    [](int64_t n) { return (double)pairs_of(n); },
    [](const SubsetParams& P, int T, hipStream_t st) -> int {
      k_pboot<<<(unsigned)(T * P.ST), SG_THREADS, 0, st>>>(P);
      VR_CHECK_LAUNCH();
      return VR_OK;
    },
    [](const SubsetLayout& L, int64_t n, int64_t k, int64_t total, int full_first, double* scores,
       hipStream_t st) -> int {
      k_pboot_reduce<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(
          L.partial, L.T, L.s_pad, total, full_first, (double)pairs_of(n), (double)pairs_of(k), scores, L.flags);
      VR_CHECK_LAUNCH();
      return VR_OK;
    },
    pearson_two_pass,
};

}  // namespace vr

using namespace vr;

extern "C" {

size_t vr_bootstrap_pearson_workspace(int64_t n, int64_t n_sets) {
  return subset_layout(nullptr, n, std::max<int64_t>(n_sets, 0) + 1, PEARSON_BOOT.np).bytes;
}

int vr_bootstrap_pearson_f32(const float* A, const float* B, int64_t n, int64_t ld, const int32_t* idx, int64_t k,
                             int64_t n_sets, int full_first, double* scores, void* ws, size_t ws_bytes,
                             void* stream) {
  return subset_bootstrap(PEARSON_BOOT, A, B, n, ld, idx, k, n_sets, full_first, scores, ws, ws_bytes, stream);
}

}  // extern "C"
