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
// k_pboot_fill / k_pboot_scatter   W as bytes (n_pad x s_pad, both padded to 64 and zero
//             there), plain byte / dword stores. pboot_build_w / pboot_shift launch them and
//             k_pboot_shift for cka_boot.hip too.
// k_pboot_shift_rows / k_pboot_shift   the two shifts (sums over finite values only, so a NaN
//             in an RDM does not poison them).
// k_pboot     a workgroup owns 64 rows i x 64 subsets and walks the columns j in panels of 16
//             from its own row block to n: only upper-triangle tiles are visited, j > i is
//             masked per element inside the diagonal block. Wave w owns rows 16 w .. 16 w + 15
//             against all 64 subsets: v_mfma_f64_16x16x4_f64 with A operand v(i, j) (lane l:
//             row l & 15, one float4 of A and of B along j per panel straight from global
//             memory, each element used by exactly one lane, so A and B need no LDS), B operand
//             the W panel widened to 0.0 / 1.0 in LDS (double-buffered, shared by the four
//             waves). Six quantities x 4 subset blocks = 24 accumulators of 4 doubles per lane
//             (192 registers; one wave per SIMD). The sixth quantity counts non-finite pairs:
//             a non-finite value is staged as 0 (0 x NaN in the MFMA would leak it into every
//             subset) and a subset whose count is non-zero scores NaN, as scipy and
//             vr_pearson_triu_f32 do for NaN / Inf input.
//             Epilogue (C/D of the f64 MFMA: col = lane & 15, row = (lane >> 4) + 4 reg):
//             rows not in the subset are dropped (W[i][s]), the 64 rows are added in a fixed
//             order, one fp64 partial per (row tile, quantity, subset).
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

#include "internal.h"

namespace vr {

typedef double pf64x4 __attribute__((ext_vector_type(4)));
typedef float pf32x4 __attribute__((ext_vector_type(4)));

constexpr int PB_T = 64;     // rows per workgroup, and subsets per workgroup
constexpr int PB_K = 16;     // columns j per panel
constexpr int PB_WLD = 68;   // LDS pitch of a W panel row (doubles): rows 4 apart fall 32 banks apart
constexpr int PB_Q = 6;      // x, y, x^2, y^2, x y, non-finite count
constexpr int PB_THREADS = 256;

__device__ inline bool pb_finite(float f) { return (__float_as_uint(f) & 0x7f800000u) != 0x7f800000u; }

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
    if (pb_finite(x)) v[0] += (double)x;
    if (pb_finite(y)) v[1] += (double)y;
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    double t = v[q];
    for (int o = 32; o > 0; o >>= 1) t += __shfl_down(t, o, 64);
    if (lane == 0) red[q][w] = t;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    const int q = threadIdx.x;
    part[a * 2 + q] = red[q][0] + red[q][1] + red[q][2] + red[q][3];
  }
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
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    double t = v[q];
    for (int o = 32; o > 0; o >>= 1) t += __shfl_down(t, o, 64);
    if (lane == 0) red[q][w] = t;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    const int q = threadIdx.x;
    const float m = (float)((red[q][0] + red[q][1] + red[q][2] + red[q][3]) / M);
    shift[q] = pb_finite(m) ? (double)m : 0.0;
  }
}

int pboot_build_w(uint8_t* W, const int32_t* idx, int64_t n, int64_t k, int64_t n_sets, int64_t n_pad,
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

int pboot_shift(const double* part, int64_t n, double M, double* shift, hipStream_t st) {
  k_pboot_shift<<<1, 256, 0, st>>>(part, n, M, shift);
  VR_CHECK_LAUNCH();
  return VR_OK;
}

struct PbParams {
  const float* A;
  const float* B;
  int64_t n, ld;
  const uint8_t* W;  // n_pad x s_pad bytes
  int64_t s_pad;
  const double* shift;
  double* partial;  // [T][PB_Q][s_pad]
  int ST;           // subset tiles
  bool vec;         // 16-B aligned rows: float4 loads
};

__global__ __launch_bounds__(PB_THREADS) void k_pboot(PbParams P) {
  __shared__ __attribute__((aligned(16))) double Ws[2][PB_K * PB_WLD];
  __shared__ double red[4][PB_Q][PB_T];
  const int bi = blockIdx.x / P.ST, bs = blockIdx.x % P.ST;  // bi ascending: heaviest first
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int fm = lane & 15, fk = lane >> 4;
  const int64_t n = P.n;
  const int64_t i0 = (int64_t)bi * PB_T, s0 = (int64_t)bs * PB_T;
  const int64_t i = i0 + wid * 16 + fm;  // the row this lane supplies to the A operand
  const bool iin = i < n;
  const float* ra = P.A + (iin ? i : 0) * P.ld;
  const float* rb = P.B + (iin ? i : 0) * P.ld;
  const double ca = P.shift[0], cb = P.shift[1];
  const int np = (int)((n - i0 + PB_K - 1) / PB_K);  // >= 1: i0 < n

  pf64x4 acc[PB_Q][4];
#pragma unroll
  for (int q = 0; q < PB_Q; ++q)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[q][b] = pf64x4{0.0, 0.0, 0.0, 0.0};

  // this lane's 4 consecutive columns of a panel: j0 + 4 fk + e (entries outside [0, n) are 0)
  auto load_ab = [&](int64_t j0, pf32x4& va, pf32x4& vb) {
    const int64_t j = j0 + fk * 4;
    va = pf32x4{0.f, 0.f, 0.f, 0.f};
    vb = va;
    if (!iin || j >= n) return;
    if (P.vec && j + 4 <= n) {
      va = *reinterpret_cast<const pf32x4*>(ra + j);
      vb = *reinterpret_cast<const pf32x4*>(rb + j);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        va[e] = (j + e < n) ? ra[j + e] : 0.f;
        vb[e] = (j + e < n) ? rb[j + e] : 0.f;
      }
    }
  };
  // W panel: thread t stages row t >> 4, subsets 4 (t & 15) .. + 3 (rows up to n_pad exist)
  const int wr = threadIdx.x >> 4, wc = (threadIdx.x & 15) * 4;
  auto load_w = [&](int64_t j0) {
    return *reinterpret_cast<const uint32_t*>(P.W + (j0 + wr) * P.s_pad + s0 + wc);
  };
  auto store_w = [&](double* dst, uint32_t w) {
#pragma unroll
    for (int e = 0; e < 4; ++e) dst[wr * PB_WLD + wc + e] = (double)((w >> (8 * e)) & 0xffu);
  };

  pf32x4 va, vb, na, nb;
  load_ab(i0, va, vb);
  store_w(Ws[0], load_w(i0));
  __syncthreads();
  for (int p = 0; p < np; ++p) {
    const int cur = p & 1;
    const int64_t j0 = i0 + (int64_t)p * PB_K;
    const bool more = p + 1 < np;
    uint32_t nw = 0;
    if (more) {
      load_ab(j0 + PB_K, na, nb);
      nw = load_w(j0 + PB_K);
    }
    // the wave's rows start at i0 + 16 wid: a panel that ends at or before it holds no j > i
    if (j0 + PB_K - 1 > i0 + wid * 16) {
      const double* Wp = Ws[cur];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        // K position (fk, e) of this step is column j0 + 4 fk + e for both operands
        const int64_t j = j0 + fk * 4 + e;
        const float a = va[e], b = vb[e];
        const bool in = iin && j > i && j < n;
        const bool fin = pb_finite(a) && pb_finite(b);
        const bool use = in && fin;
        const double x = use ? (double)a - ca : 0.0;
        const double y = use ? (double)b - cb : 0.0;
        const double qv[PB_Q] = {x, y, x * x, y * y, x * y, (in && !fin) ? 1.0 : 0.0};
#pragma unroll
        for (int sb = 0; sb < 4; ++sb) {
          const double w = Wp[(fk * 4 + e) * PB_WLD + sb * 16 + fm];
#pragma unroll
          for (int q = 0; q < PB_Q; ++q)
            acc[q][sb] = __builtin_amdgcn_mfma_f64_16x16x4f64(qv[q], w, acc[q][sb], 0, 0, 0);
        }
      }
    }
    if (more) {
      store_w(Ws[cur ^ 1], nw);
      va = na;
      vb = nb;
    }
    __syncthreads();
  }

  // C/D of the f64 MFMA: col (subset) = lane & 15, row = (lane >> 4) + 4 r. Keep the rows that
  // are in the subset, add the wave's 16 rows, then the four waves in wave order.
#pragma unroll
  for (int sb = 0; sb < 4; ++sb) {
    bool keep[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t row = i0 + wid * 16 + fk + 4 * r;  // < n_pad
      keep[r] = P.W[row * P.s_pad + s0 + sb * 16 + fm] != 0;
    }
#pragma unroll
    for (int q = 0; q < PB_Q; ++q) {
      double t = 0.0;
#pragma unroll
      for (int r = 0; r < 4; ++r) t += keep[r] ? acc[q][sb][r] : 0.0;
      t += __shfl_xor(t, 16, 64);
      t += __shfl_xor(t, 32, 64);
      if (fk == 0) red[wid][q][sb * 16 + fm] = t;
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < PB_Q * PB_T; e += PB_THREADS) {
    const int q = e / PB_T, s = e % PB_T;
    P.partial[((int64_t)bi * PB_Q + q) * P.s_pad + s0 + s] = (red[0][q][s] + red[1][q][s]) + (red[2][q][s] + red[3][q][s]);
  }
}

// one thread per subset: row tiles added in tile order, then the score or the recompute flag
__global__ __launch_bounds__(256) void k_pboot_reduce(const double* __restrict__ partial, int T, int64_t s_pad,
                                                      int64_t total, int full_first, double m_full, double m_sub,
                                                      double* __restrict__ scores, int32_t* __restrict__ flags) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= total) return;
  double v[PB_Q] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int b = 0; b < T; ++b)
#pragma unroll
    for (int q = 0; q < PB_Q; ++q) v[q] += partial[((int64_t)b * PB_Q + q) * s_pad + s];
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

struct PbLayout {
  int64_t n_pad, s_pad;
  int T, ST;
  uint8_t* W;
  double* partial;
  double* part;
  double* mu;
  double* shift;
  int32_t* flags;
  size_t bytes;
};

// total: subsets including the full set
static PbLayout pb_layout(void* ws, int64_t n, int64_t total) {
  PbLayout L;
  const int64_t nn = std::max<int64_t>(n, 1), tt = std::max<int64_t>(total, 1);
  L.n_pad = (nn + PB_T - 1) / PB_T * PB_T;
  L.s_pad = (tt + PB_T - 1) / PB_T * PB_T;
  L.T = (int)(L.n_pad / PB_T);
  L.ST = (int)(L.s_pad / PB_T);
  Carver c(ws);
  L.W = c.take<uint8_t>((size_t)L.n_pad * L.s_pad);
  L.partial = c.take<double>((size_t)L.T * PB_Q * L.s_pad);
  L.part = c.take<double>((size_t)nn * 5);
  L.mu = c.take<double>(2);
  L.shift = c.take<double>(2);
  L.flags = c.take<int32_t>((size_t)L.s_pad);
  L.bytes = c.bytes();
  return L;
}

}  // namespace vr

using namespace vr;

extern "C" {

size_t vr_bootstrap_pearson_workspace(int64_t n, int64_t n_sets) {
  return pb_layout(nullptr, n, std::max<int64_t>(n_sets, 0) + 1).bytes;
}

int vr_bootstrap_pearson_f32(const float* A, const float* B, int64_t n, int64_t ld, const int32_t* idx, int64_t k,
                             int64_t n_sets, int full_first, double* scores, void* ws, size_t ws_bytes,
                             void* stream) {
  clear_error();
  VR_REQUIRE(n >= 0 && ld >= n && n_sets >= 0 && k >= 0 && k <= n,
             "vr_bootstrap_pearson_f32: bad shape n=%lld ld=%lld k=%lld n_sets=%lld", (long long)n, (long long)ld,
             (long long)k, (long long)n_sets);
  const int off = full_first ? 1 : 0;
  const int64_t total = n_sets + off;
  // every call fits the workspace of its (n, n_sets): the layout is monotone in both
  const size_t need = pb_layout(nullptr, n, total).bytes;
  if (ws_bytes < need || ws == nullptr) {
    set_error("vr_bootstrap_pearson_f32: workspace %zu < %zu", ws_bytes, need);
    return VR_EWORKSPACE;
  }
  if (total == 0) return VR_OK;
  VR_REQUIRE(scores != nullptr && (n_sets == 0 || idx != nullptr) && (n < 2 || (A != nullptr && B != nullptr)),
             "vr_bootstrap_pearson_f32: null pointer");
  hipStream_t st = as_stream(stream);
  if (n < 2) {  // no pair at all
    k_pboot_nan<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(scores, total);
    VR_CHECK_LAUNCH();
    return VR_OK;
  }
  const PbLayout L = pb_layout(ws, n, total);
  VR_TRY(pboot_build_w(L.W, idx, n, k, n_sets, L.n_pad, L.s_pad, off, st));
  const double m_full = (double)pairs_of(n), m_sub = (double)pairs_of(k);
  k_pboot_shift_rows<<<(unsigned)n, 256, 0, st>>>(A, B, n, ld, L.part);
  VR_CHECK_LAUNCH();
  VR_TRY(pboot_shift(L.part, n, m_full, L.shift, st));
  PbParams P;
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
  k_pboot<<<(unsigned)(L.T * L.ST), PB_THREADS, 0, st>>>(P);
  VR_CHECK_LAUNCH();
  k_pboot_reduce<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(L.partial, L.T, L.s_pad, total, off, m_full, m_sub,
                                                                 scores, L.flags);
  VR_CHECK_LAUNCH();
  // the one read-back of the call: which subsets the one-pass sums could not decide
  std::vector<int32_t> flags((size_t)total);
  VR_CHECK_HIP(hipMemcpyAsync(flags.data(), L.flags, (size_t)total * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  VR_CHECK_HIP(hipStreamSynchronize(st));
  for (int64_t s = 0; s < total; ++s) {
    if (!flags[(size_t)s]) continue;
    if (off && s == 0)
      VR_TRY(pearson_two_pass(A, B, n, ld, nullptr, scores, L.part, L.mu, st));
    else
      VR_TRY(pearson_two_pass(A, B, k, ld, idx + (s - off) * k, scores + s, L.part, L.mu, st));
  }
  return VR_OK;
}

}  // extern "C"
