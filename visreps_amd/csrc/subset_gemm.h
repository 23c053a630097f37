// The masked subset-GEMM of the bootstrap engines (pearson_boot.hip, cka_boot.hip): every
// subset's sums over a symmetric n x n pair (A, B) as one GEMM against W, the n x S 0/1
// indicator matrix of the subsets, on the fp64 MFMA.
//
// A workgroup owns 64 rows i x 64 subsets and walks the columns j in panels of 16. Wave w owns
// rows 16 w .. 16 w + 15 against all 64 subsets: v_mfma_f64_16x16x4_f64 with A operand v(i, j)
// (lane l: row l & 15, one float4 of A and of B along j per panel straight from global memory,
// each element used by exactly one lane, so A and B need no LDS), B operand the W panel widened
// to 0.0 / 1.0 in LDS (double-buffered, shared by the four waves). With fixed shifts ca, cb and
// x = (double)A[i][j] - ca, y = (double)B[i][j] - cb, six quantities per (row, subset),
//   sum_j W[j][s] {x, y, x^2, y^2, x y, non-finite},
// in 6 x 4 subset blocks = 24 accumulators of 4 doubles per lane (192 registers; one wave per
// SIMD). A non-finite value of A or B is staged as 0 in both (0 x NaN in the MFMA would leak it
// into every subset) and counted instead.
//
// subset_walk   the loads, the W staging, the double-buffer loop and the MFMA block, for the
//               triangle walk (panels from the workgroup's own row block to n, j > i masked,
//               panels before a wave's rows skipped) or the full walk (panels 0 .. n, no mask).
// subset_tail   a kernel's per-row epilogue leaves NP partials per lane and subset block (C/D
//               of the f64 MFMA: col = lane & 15, row = (lane >> 4) + 4 reg, so a lane holds 4
//               rows of one subset); the tail adds the wave's 16 rows, then the four waves in a
//               fixed order: one fp64 partial per (row tile, partial, subset), no atomics.
// subset_bootstrap   the host driver of both engines.
#pragma once

#include "internal.h"

namespace vr {

constexpr int SG_T = 64;     // rows per workgroup, and subsets per workgroup
constexpr int SG_K = 16;     // columns j per panel
constexpr int SG_WLD = 68;   // LDS pitch of a W panel row (doubles): rows 4 apart fall 32 banks apart
constexpr int SG_Q = 6;      // x, y, x^2, y^2, x y, non-finite count
constexpr int SG_THREADS = 256;

__device__ inline bool finite_f32(float f) { return (__float_as_uint(f) & 0x7f800000u) != 0x7f800000u; }

struct SubsetParams {
  const float* A;
  const float* B;
  int64_t n, ld;
  const uint8_t* W;  // n_pad x s_pad bytes
  int64_t s_pad;
  const double* shift;
  double* partial;  // [T][partials][s_pad]
  int ST;           // subset tiles
  bool vec;         // 16-B aligned rows: float4 loads
};

struct SubsetLayout {
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

// total: subsets including the full set; np: partials per (row tile, subset)
SubsetLayout subset_layout(void* ws, int64_t n, int64_t total, int np);

// What an engine adds to the shared driver. Each launch goes on stream st.
struct SubsetEngine {
  const char* name;  // the entry point, for messages
  int np;            // partials per (row tile, subset)
  // per-row sums of the finite values the shift averages: part[2 a + {0, 1}]
  int (*shift_rows)(const float* A, const float* B, int64_t n, int64_t ld, double* part, hipStream_t st);
  double (*shift_denom)(int64_t n);  // how many values that is
  int (*walk)(const SubsetParams& P, int T, hipStream_t st);
  // row tiles -> scores[total] and the recompute flags
  int (*reduce)(const SubsetLayout& L, int64_t n, int64_t k, int64_t total, int full_first, double* scores,
                hipStream_t st);
  // the flagged subset again, exactly: idx == nullptr the full set
  int (*two_pass)(const float* A, const float* B, int64_t n_or_k, int64_t ld, const int32_t* idx, double* out,
                  double* part, double* mu, hipStream_t st);
};

// The body of vr_bootstrap_pearson_f32 / vr_bootstrap_cka_f32 (pearson_boot.hip).
int subset_bootstrap(const SubsetEngine& E, const float* A, const float* B, int64_t n, int64_t ld,
                     const int32_t* idx, int64_t k, int64_t n_sets, int full_first, double* scores, void* ws,
                     size_t ws_bytes, void* stream);

// TRI: the strict upper triangle from the workgroup's own row block i0; else every column.
// wid: the wave; fm = lane & 15, fk = lane >> 4: the lane's place in the MFMA fragments.
// Ws: the two W panel buffers. acc[q][sb]: quantity q against subsets s0 + 16 sb .. + 15.
template <bool TRI>
__device__ inline void subset_walk(const SubsetParams& P, double (&Ws)[2][SG_K * SG_WLD], int64_t i0, int64_t s0,
                                   int wid, int fm, int fk, f64x4 (&acc)[SG_Q][4]) {
  const int64_t n = P.n;
  const int64_t i = i0 + wid * 16 + fm;  // the row this lane supplies to the A operand
  const bool iin = i < n;
  const float* ra = P.A + (iin ? i : 0) * P.ld;
  const float* rb = P.B + (iin ? i : 0) * P.ld;
  const double ca = P.shift[0], cb = P.shift[1];
  const int64_t jb = TRI ? i0 : 0;                    // the first panel's column
  const int np = (int)((n - jb + SG_K - 1) / SG_K);  // >= 1: i0 < n; 16 np <= n_pad rows of W exist

#pragma unroll
  for (int q = 0; q < SG_Q; ++q)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[q][b] = f64x4{0.0, 0.0, 0.0, 0.0};

  // this lane's 4 consecutive columns of a panel: j0 + 4 fk + e (entries outside [0, n) are 0)
  auto load_ab = [&](int64_t j0, f32x4& va, f32x4& vb) {
    const int64_t j = j0 + fk * 4;
    va = f32x4{0.f, 0.f, 0.f, 0.f};
    vb = va;
    if (!iin || j >= n) return;
    if (P.vec && j + 4 <= n) {
      va = *reinterpret_cast<const f32x4*>(ra + j);
      vb = *reinterpret_cast<const f32x4*>(rb + j);
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
    for (int e = 0; e < 4; ++e) dst[wr * SG_WLD + wc + e] = (double)((w >> (8 * e)) & 0xffu);
  };

  f32x4 va, vb, na, nb;
  load_ab(jb, va, vb);
  store_w(Ws[0], load_w(jb));
  __syncthreads();
  for (int p = 0; p < np; ++p) {
    const int cur = p & 1;
    const int64_t j0 = jb + (int64_t)p * SG_K;
    const bool more = p + 1 < np;
    uint32_t nw = 0;
    if (more) {
      load_ab(j0 + SG_K, na, nb);
      nw = load_w(j0 + SG_K);
    }
    // TRI: the wave's rows start at i0 + 16 wid: a panel that ends at or before it holds no j > i
    if (!TRI || j0 + SG_K - 1 > i0 + wid * 16) {
      const double* Wp = Ws[cur];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        // K position (fk, e) of this step is column j0 + 4 fk + e for both operands
        const int64_t j = j0 + fk * 4 + e;
        const float a = va[e], b = vb[e];
        const bool in = iin && (!TRI || j > i) && j < n;
        const bool fin = finite_f32(a) && finite_f32(b);
        const bool use = in && fin;
        const double x = use ? (double)a - ca : 0.0;
        const double y = use ? (double)b - cb : 0.0;
        const double qv[SG_Q] = {x, y, x * x, y * y, x * y, (in && !fin) ? 1.0 : 0.0};
#pragma unroll
        for (int sb = 0; sb < 4; ++sb) {
          const double w = Wp[(fk * 4 + e) * SG_WLD + sb * 16 + fm];
#pragma unroll
          for (int q = 0; q < SG_Q; ++q)
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
}

// t[sb][q]: this lane's sum over its 4 rows of partial q for subset s0 + 16 sb + (lane & 15).
// The two shuffles add the wave's 16 rows, red[wave] then the four waves in wave order.
template <int NP>
__device__ inline void subset_tail(const SubsetParams& P, double (&red)[4][NP][SG_T], int bi, int64_t s0, int wid,
                                   int fm, int fk, const double (&t)[4][NP]) {
#pragma unroll
  for (int sb = 0; sb < 4; ++sb)
#pragma unroll
    for (int q = 0; q < NP; ++q) {
      double z = t[sb][q];
      z += __shfl_xor(z, 16, 64);
      z += __shfl_xor(z, 32, 64);
      if (fk == 0) red[wid][q][sb * 16 + fm] = z;
    }
  __syncthreads();
  for (int e = threadIdx.x; e < NP * SG_T; e += SG_THREADS) {
    const int q = e / SG_T, s = e % SG_T;
    P.partial[((int64_t)bi * NP + q) * P.s_pad + s0 + s] = (red[0][q][s] + red[1][q][s]) + (red[2][q][s] + red[3][q][s]);
  }
}

}  // namespace vr
