// Batched one-sided (Hestenes) Jacobi SVD in fp64: vr_svd_jacobi_f64, the dense solver behind
// PLS-SVD's solver="jacobi" (analysis/cross_decomposition.py). Replaces the scipy.linalg.svd of
// sklearn.cross_decomposition.PLSSVD.fit for every fold at once.
//
// Each member is a p x q matrix C. B = C (p <= q) or C^T (p > q, k_svd_stage) has n = min(p, q)
// rows of length L = max(p, q). Plane rotations of row pairs drive the rows of B to mutual
// orthogonality; the same rotations accumulate in R (n x n, starts as I), so R B = Sigma Q^T:
// row j of B ends as sigma_j times a unit singular vector of the long side, row j of R is the
// matching vector of the short side. No Gram matrix is ever formed: the three dots of a pair come
// from the current rows, so the conditioning is never squared, and the vectors come out
// orthogonal to working precision however the singular values are spaced.
//
// k_svd_stage     B <- C or C^T through a 32 x 32 LDS tile; the caller's matrix is never written.
// k_svd_eye       R <- I.
// k_svd_rownorm   two-pass row norms of B (max |x|, then the scaled sum of squares); NaN marks a
//                 row with a non-finite entry. Run before the sweeps (the null-row floor, the
//                 non-finite members) and after them (the singular values).
// k_svd_setup     per member: floor^2 = (64 (p + q) eps max row norm)^2, done = 2 if non-finite.
// k_svd_step<b>   one workgroup (4 waves) per block pair (P, Q) of one member: the 2 b rows of B
//                 in dynamic LDS (2 b L 8 bytes <= 128 KiB: b = 8 to L = 1024, 4 to 2048, 2 to
//                 4096), b rounds of b disjoint cross pairs (i, (i + r) mod b), a wave per pair in
//                 a fixed assignment, a barrier between rounds; on the first step of a sweep the
//                 b - 1 round-robin rounds of within-block pairs of P and Q come first. A wave
//                 forms a = b_i.b_i, c = b_j.b_j, g = b_i.b_j (strided, in order, xor butterfly:
//                 every lane holds the same bits), skips if |g| <= L eps sqrt(a) sqrt(c), else
//                 rotates by zeta = (c - a) / 2g, t = sign(zeta) / (|zeta| + sqrt(1 + zeta^2));
//                 then swaps the two rows if the higher slot holds the larger norm (de Rijk). In
//                 the skip test a norm below the floor counts as the floor, so rows that can only
//                 become null components are orthogonalised to absolute, not relative, accuracy.
//                 (Leaving pairs of such rows alone altogether stalls: a row just above the floor
//                 is then rotated for ever against rows below it that are not orthogonal to each
//                 other; measured) Every rotation
//                 and swap goes to a list in LDS, one fixed entry per (round, pair); after B is
//                 written back the list is replayed on the 2 b rows of R, a thread holding the 2 b
//                 values of its columns in registers (the slots of an entry are compile-time).
// k_svd_sweep_end counters -> done flags, sweep counts.
// k_svd_finish    one workgroup per member row: rank by (sigma descending, slot ascending),
//                 normalise the long-side vector, svd_flip's u-based sign, null rule, NaN fill.
// The block pairs of a step come from vr_jacobi_schedule (host, a round-robin tournament), one
// launch per step in stream order; the host reads the done flags once per sweep.
// Roofline: LDS bandwidth (6 L fp64 LDS accesses per pair against 6 L FLOPs). No floating-point
// atomics: a member's result is bit-identical run to run and in any batch.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <vector>

#include "internal.h"

namespace vr {

constexpr int SV_THREADS = 256;
constexpr int SV_WAVES = SV_THREADS / 64;
constexpr int SV_MAX_SWEEPS = 60;
constexpr int64_t SV_MAX_L = 4096;
constexpr size_t SV_LDS_BYTES = 128 * 1024;

enum : int { SV_NONE = 0, SV_ROT = 1, SV_ROT_SWAP = 2, SV_SWAP = 3 };

// Rounds 0 .. b - 2 pair the slots within P (pairs 0 .. b/2 - 1) and within Q (the rest) by the
// circle method; rounds b - 1 .. 2 b - 2 are the cross pairs (i, b + (i + r) mod b). Slots
// 0 .. b - 1 are P's rows, b .. 2 b - 1 are Q's. si < sj always. List entry = round * b + pair.
template <int b>
__host__ __device__ constexpr void sv_pair_slots(int round, int pair, int& si, int& sj) {
  if (round < b - 1) {
    const int blk = pair / (b / 2), k = pair % (b / 2);
    int x = b - 1, y = round;
    if (k != 0) {
      x = (round + k) % (b - 1);
      y = (round - k + (b - 1)) % (b - 1);
    }
    si = blk * b + (x < y ? x : y);
    sj = blk * b + (x < y ? y : x);
  } else {
    si = pair;
    sj = b + (pair + (round - (b - 1))) % b;
  }
}

// fixed-tree reductions over the 256 threads of a workgroup; every thread gets the result
__device__ inline double block_max(double v, double* red) {
  const int t = threadIdx.x;
  red[t] = v;
  __syncthreads();
  for (int o = SV_THREADS / 2; o > 0; o >>= 1) {
    if (t < o) red[t] = fmax(red[t], red[t + o]);
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

__device__ inline double block_sum(double v, double* red) {
  const int t = threadIdx.x;
  red[t] = v;
  __syncthreads();
  for (int o = SV_THREADS / 2; o > 0; o >>= 1) {
    if (t < o) red[t] += red[t + o];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

__device__ inline double sv_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

// B[mem][i][j] = tr ? A[mem][j][i] : A[mem][i][j]; grid (ceil(L / 32), ceil(n / 32), batch)
__global__ __launch_bounds__(SV_THREADS) void k_svd_stage(const double* __restrict__ A, int64_t lda,
                                                          int64_t stride_a, int64_t n, int64_t L, int tr,
                                                          double* __restrict__ B) {
  __shared__ double tile[32][33];
  const double* a = A + (int64_t)blockIdx.z * stride_a;
  double* o = B + (int64_t)blockIdx.z * n * L;
  const int64_t i0 = (int64_t)blockIdx.y * 32, j0 = (int64_t)blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  if (!tr) {
    for (int r = ty; r < 32; r += 8)
      if (i0 + r < n && j0 + tx < L) o[(i0 + r) * L + j0 + tx] = a[(i0 + r) * lda + j0 + tx];
    return;
  }
  for (int r = ty; r < 32; r += 8)  // A row j0 + r, column i0 + tx
    if (j0 + r < L && i0 + tx < n) tile[r][tx] = a[(j0 + r) * lda + i0 + tx];
  __syncthreads();
  for (int r = ty; r < 32; r += 8)
    if (i0 + r < n && j0 + tx < L) o[(i0 + r) * L + j0 + tx] = tile[tx][r];
}

__global__ void k_svd_eye(double* __restrict__ R, int64_t n, int64_t count) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= count) return;
  const int64_t w = e % (n * n);
  R[e] = (w / n == w % n) ? 1.0 : 0.0;
}

// norm[mem][row] = |B[mem][row]|_2 in two passes, NaN if the row has a non-finite entry (or its
// scaled sum of squares is not finite); grid (n, batch)
__global__ __launch_bounds__(SV_THREADS) void k_svd_rownorm(const double* __restrict__ B, int64_t n, int64_t L,
                                                            double* __restrict__ norm) {
  __shared__ double red[SV_THREADS];
  const int64_t row = blockIdx.x, mem = blockIdx.y;
  const double* x = B + (mem * n + row) * L;
  double mx = 0.0, bad = 0.0;
  for (int64_t k = threadIdx.x; k < L; k += SV_THREADS) {
    const double v = fabs(x[k]);
    if (!(v <= DBL_MAX)) bad = 1.0;
    mx = fmax(mx, v);  // fmax drops a NaN: `bad` carries it
  }
  bad = block_max(bad, red);
  mx = block_max(mx, red);
  double s = 0.0;
  if (mx > 0.0) {
    for (int64_t k = threadIdx.x; k < L; k += SV_THREADS) {
      const double v = x[k] / mx;
      s = fma(v, v, s);
    }
  }
  s = block_sum(s, red);
  if (threadIdx.x == 0) norm[mem * n + row] = bad != 0.0 ? sv_nan() : mx * sqrt(s);
}

// per member: the null-pair floor, the non-finite flag, cleared counters; grid (batch)
__global__ __launch_bounds__(SV_THREADS) void k_svd_setup(const double* __restrict__ norm, int64_t n, double m_eps64,
                                                          double* __restrict__ floor2, int32_t* __restrict__ done,
                                                          int32_t* __restrict__ count,
                                                          int32_t* __restrict__ sweeps) {
  __shared__ double red[SV_THREADS];
  const int64_t mem = blockIdx.x;
  double mx = 0.0, bad = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += SV_THREADS) {
    const double v = norm[mem * n + i];
    if (!(v <= DBL_MAX)) bad = 1.0;
    mx = fmax(mx, v);
  }
  bad = block_max(bad, red);
  mx = block_max(mx, red);
  if (threadIdx.x == 0) {
    const double fl = m_eps64 * mx;
    const double fl2 = fl * fl;
    floor2[mem] = fl2;
    // a floor^2 that overflows would make every pair skip: such a member is not solvable in
    // fp64 dots either and is treated as non-finite
    done[mem] = (bad != 0.0 || !(fl2 <= DBL_MAX) || !(mx * mx * (double)n <= DBL_MAX)) ? 2 : 0;
    count[mem] = 0;
    sweeps[mem] = 0;
  }
}

struct SvdStepParams {
  double* B;             // batch x n x L
  double* R;             // batch x n x n
  int64_t n, L;
  const int32_t* pairs;  // this step's npair x 2 block ids, the second -1 for a bye
  const int32_t* done;   // per member: 0 running, 1 converged, 2 non-finite
  int32_t* count;        // per member: rotations of this sweep
  const double* floor2;  // per member
  double tol;            // L eps
  int first;             // the first step of a sweep: within-block pairs too
};

template <int b>
__global__ __launch_bounds__(SV_THREADS) void k_svd_step(SvdStepParams P) {
  constexpr int NE = (2 * b - 1) * b;  // b (b - 1) within-block entries, then b^2 cross entries
  extern __shared__ __attribute__((aligned(16))) double sv_rows[];  // 2 b x L
  __shared__ double l_cs[NE], l_sn[NE];
  __shared__ int l_op[NE];
  const int64_t mem = blockIdx.y;
  if (P.done[mem] != 0) return;
  const int64_t bp = P.pairs[2 * blockIdx.x], bq = P.pairs[2 * blockIdx.x + 1];
  if (bp < 0 || (bq < 0 && !P.first)) return;
  const int64_t n = P.n, L = P.L;
  double* Bm = P.B + mem * n * L;
  double* Rm = P.R + mem * n * n;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  // global row of a slot; n marks a row that does not exist (ragged last block, bye)
  int64_t grow[2 * b];
#pragma unroll
  for (int s = 0; s < 2 * b; ++s) {
    const int64_t g = s < b ? bp * b + s : (bq < 0 ? n : bq * b + (s - b));
    grow[s] = g < n ? g : n;
  }

#pragma unroll
  for (int s = 0; s < 2 * b; ++s) {
    if (grow[s] >= n) continue;
    const double* src = Bm + grow[s] * L;
    for (int64_t k = tid; k < L; k += SV_THREADS) sv_rows[s * L + k] = src[k];
  }
  for (int e = tid; e < NE; e += SV_THREADS) l_op[e] = SV_NONE;
  __syncthreads();

  const double fl2 = P.floor2[mem];
  int cnt = 0;
  for (int rd = P.first ? 0 : b - 1; rd < 2 * b - 1; ++rd) {
    for (int pr = wid; pr < b; pr += SV_WAVES) {
      int si = 0, sj = 0;
      sv_pair_slots<b>(rd, pr, si, sj);
      const int64_t gi = si < b ? bp * b + si : (bq < 0 ? n : bq * b + (si - b));
      const int64_t gj = sj < b ? bp * b + sj : (bq < 0 ? n : bq * b + (sj - b));
      if (gi >= n || gj >= n) continue;  // wave-uniform
      double* x = sv_rows + (int64_t)si * L;
      double* y = sv_rows + (int64_t)sj * L;
      double a = 0.0, c = 0.0, g = 0.0;
      for (int64_t k = lane; k < L; k += 64) {
        const double xi = x[k], yj = y[k];
        a = fma(xi, xi, a);
        c = fma(yj, yj, c);
        g = fma(xi, yj, g);
      }
      for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o, 64);
        c += __shfl_xor(c, o, 64);
        g += __shfl_xor(g, o, 64);
      }
      // a row below the floor counts with the floor as its norm: relative accuracy above the
      // floor, absolute accuracy below it, with no edge between rows that are rotated and rows
      // that are not
      const bool swap = c > a;
      double cs = 1.0, sn = 0.0;
      int op;
      if (fabs(g) <= P.tol * sqrt(fmax(a, fl2)) * sqrt(fmax(c, fl2))) {
        op = swap ? SV_SWAP : SV_NONE;
      } else {
        const double zeta = (c - a) / (2.0 * g);
        const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        cs = 1.0 / sqrt(1.0 + t * t);
        sn = cs * t;
        op = swap ? SV_ROT_SWAP : SV_ROT;
        ++cnt;
      }
      if (op == SV_SWAP) {
        for (int64_t k = lane; k < L; k += 64) {
          const double xi = x[k], yj = y[k];
          x[k] = yj;
          y[k] = xi;
        }
      } else if (op != SV_NONE) {
        for (int64_t k = lane; k < L; k += 64) {
          const double xi = x[k], yj = y[k];
          const double ni = cs * xi - sn * yj, nj = sn * xi + cs * yj;
          x[k] = swap ? nj : ni;
          y[k] = swap ? ni : nj;
        }
      }
      if (lane == 0) {
        const int e = rd * b + pr;
        l_cs[e] = cs;
        l_sn[e] = sn;
        l_op[e] = op;
      }
    }
    __syncthreads();
  }
  if (lane == 0 && cnt > 0) atomicAdd(P.count + mem, cnt);

#pragma unroll
  for (int s = 0; s < 2 * b; ++s) {
    if (grow[s] >= n) continue;
    double* dst = Bm + grow[s] * L;
    for (int64_t k = tid; k < L; k += SV_THREADS) dst[k] = sv_rows[s * L + k];
  }

  // the same list on the rows of R, column by column in registers
  const bool first = P.first != 0;
  for (int64_t col = tid; col < n; col += SV_THREADS) {
    double v[2 * b];
#pragma unroll
    for (int s = 0; s < 2 * b; ++s) v[s] = grow[s] < n ? Rm[grow[s] * n + col] : 0.0;
#pragma unroll
    for (int rd = 0; rd < 2 * b - 1; ++rd) {
      if (rd < b - 1 && !first) continue;
#pragma unroll
      for (int pr = 0; pr < b; ++pr) {
        int si = 0, sj = 0;
        sv_pair_slots<b>(rd, pr, si, sj);
        const int op = l_op[rd * b + pr];
        if (op == SV_NONE) continue;
        const double vi = v[si], vj = v[sj];
        if (op == SV_SWAP) {
          v[si] = vj;
          v[sj] = vi;
        } else {
          const double cs = l_cs[rd * b + pr], sn = l_sn[rd * b + pr];
          const double ni = cs * vi - sn * vj, nj = sn * vi + cs * vj;
          v[si] = op == SV_ROT_SWAP ? nj : ni;
          v[sj] = op == SV_ROT_SWAP ? ni : nj;
        }
      }
    }
#pragma unroll
    for (int s = 0; s < 2 * b; ++s)
      if (grow[s] < n) Rm[grow[s] * n + col] = v[s];
  }
}

// after a sweep: a running member counts it and is done if it made no rotation
__global__ void k_svd_sweep_end(int64_t batch, int32_t* __restrict__ count, int32_t* __restrict__ done,
                                int32_t* __restrict__ sweeps) {
  const int64_t mem = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (mem >= batch) return;
  if (done[mem] == 0) {
    sweeps[mem] += 1;
    if (count[mem] == 0) done[mem] = 1;
  }
  count[mem] = 0;
}

// One workgroup per member row (slot): its component index is its rank by (sigma descending,
// slot ascending). tr = 0: u = the row of R (length p = n), v = the row of B / sigma (length q);
// tr = 1: u = the row of B / sigma (length p = L), v = the row of R (length q = n).
__global__ __launch_bounds__(SV_THREADS) void k_svd_finish(const double* __restrict__ B, const double* __restrict__ R,
                                                           const double* __restrict__ norm,
                                                           const int32_t* __restrict__ done, int64_t n, int64_t L,
                                                           int tr, double m_eps64, double* __restrict__ S,
                                                           double* __restrict__ U, double* __restrict__ Vt,
                                                           int32_t* __restrict__ null) {
  __shared__ double red[SV_THREADS];
  __shared__ double r_a[SV_THREADS];
  __shared__ int64_t r_i[SV_THREADS];
  const int64_t slot = blockIdx.x, mem = blockIdx.y;
  const int t = threadIdx.x;
  const int64_t p = tr ? L : n, q = tr ? n : L;
  const double nan = sv_nan();
  if (done[mem] == 2) {  // a non-finite member: NaN everywhere, every component null
    for (int64_t i = t; i < p; i += SV_THREADS) U[(mem * n + slot) * p + i] = nan;
    for (int64_t i = t; i < q; i += SV_THREADS) Vt[(mem * n + slot) * q + i] = nan;
    if (t == 0) {
      S[mem * n + slot] = nan;
      null[mem * n + slot] = 1;
    }
    return;
  }
  const double* sig = norm + mem * n;
  const double sj = sig[slot];
  double before = 0.0, mx = 0.0;  // counts below 2^53 are exact in fp64
  for (int64_t i = t; i < n; i += SV_THREADS) {
    const double v = sig[i];
    mx = fmax(mx, v);
    if (v > sj || (v == sj && i < slot)) before += 1.0;
  }
  const double s1 = block_max(mx, red);
  const int64_t j = (int64_t)block_sum(before, red);
  const bool is_null = !(sj > m_eps64 * s1);
  const double* brow = B + (mem * n + slot) * L;
  const double* rrow = R + (mem * n + slot) * n;
  const double* urow = tr ? brow : rrow;
  double best = -1.0;
  int64_t bidx = 0;
  for (int64_t i = t; i < p; i += SV_THREADS) {
    const double a = fabs(urow[i]);
    if (a > best) {  // ascending i: the lowest index of a tie stays
      best = a;
      bidx = i;
    }
  }
  r_a[t] = best;
  r_i[t] = bidx;
  __syncthreads();
  for (int o = SV_THREADS / 2; o > 0; o >>= 1) {  // fixed tree
    if (t < o) {
      const double a = r_a[t + o];
      const int64_t ia = r_i[t + o];
      if (a > r_a[t] || (a == r_a[t] && ia < r_i[t])) {
        r_a[t] = a;
        r_i[t] = ia;
      }
    }
    __syncthreads();
  }
  const double sign = urow[r_i[0]] < 0.0 ? -1.0 : 1.0;
  const double fb = sign / sj, fr = sign;
  double* uo = U + (mem * n + j) * p;
  double* vo = Vt + (mem * n + j) * q;
  for (int64_t i = t; i < p; i += SV_THREADS) uo[i] = is_null ? nan : (tr ? brow[i] * fb : rrow[i] * fr);
  for (int64_t i = t; i < q; i += SV_THREADS) vo[i] = is_null ? nan : (tr ? rrow[i] * fr : brow[i] * fb);
  if (t == 0) {
    S[mem * n + j] = sj;
    null[mem * n + j] = is_null ? 1 : 0;
  }
}

// ------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------
static int sv_block(int64_t L) { return L <= 1024 ? 8 : (L <= 2048 ? 4 : 2); }

struct SvdGeom {
  int64_t n, L, nb, nbe, nsteps, npair;
  int b, tr;
};

static SvdGeom sv_geometry(int64_t p, int64_t q) {
  SvdGeom g;
  g.tr = p > q ? 1 : 0;
  g.n = std::min(p, q);
  g.L = std::max(p, q);
  g.b = sv_block(g.L);
  g.nb = (g.n + g.b - 1) / g.b;
  g.nbe = g.nb + (g.nb & 1);
  g.nsteps = g.nbe - 1;
  g.npair = g.nbe / 2;
  return g;
}

struct SvdLayout {
  double *B, *R, *norm, *floor2;
  int32_t *count, *done, *pairs;
  size_t bytes;
};

static SvdLayout sv_layout(void* ws, int64_t batch, const SvdGeom& g) {
  SvdLayout W;
  Carver c(ws);
  W.B = c.take<double>((size_t)(batch * g.n * g.L));
  W.R = c.take<double>((size_t)(batch * g.n * g.n));
  W.norm = c.take<double>((size_t)(batch * g.n));
  W.floor2 = c.take<double>((size_t)batch);
  W.count = c.take<int32_t>((size_t)batch);
  W.done = c.take<int32_t>((size_t)batch);
  W.pairs = c.take<int32_t>((size_t)(g.nsteps * g.npair * 2));
  W.bytes = c.bytes();
  return W;
}

template <int b>
static int sv_sweeps(const SvdStepParams& base, const SvdGeom& g, const SvdLayout& W, int64_t batch,
                     int32_t* sweeps, std::vector<int32_t>& flags, bool& all_done, hipStream_t st) {
  const size_t lds = (size_t)2 * b * g.L * sizeof(double);
  VR_ONCE(VR_CHECK_HIP(hipFuncSetAttribute((const void*)k_svd_step<b>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)SV_LDS_BYTES)));
  for (int sweep = 0; sweep < SV_MAX_SWEEPS && !all_done; ++sweep) {
    {
      KtScope kt(KT_SVD_STEP, (double)batch * (double)g.n * (double)g.n * (double)g.L * 3.0, st);
      for (int64_t s = 0; s < g.nsteps; ++s) {
        SvdStepParams P = base;
        P.pairs = W.pairs + s * g.npair * 2;
        P.first = s == 0 ? 1 : 0;
        k_svd_step<b><<<dim3((unsigned)g.npair, (unsigned)batch), SV_THREADS, lds, st>>>(P);
        VR_CHECK_LAUNCH();
      }
    }
    k_svd_sweep_end<<<(unsigned)((batch + 255) / 256), 256, 0, st>>>(batch, W.count, W.done, sweeps);
    VR_CHECK_LAUNCH();
    VR_CHECK_HIP(hipMemcpyAsync(flags.data(), W.done, (size_t)batch * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    VR_CHECK_HIP(hipStreamSynchronize(st));
    all_done = std::all_of(flags.begin(), flags.end(), [](int32_t f) { return f != 0; });
  }
  return VR_OK;
}

}  // namespace vr

using namespace vr;

extern "C" {

int vr_jacobi_schedule(int64_t nb, int32_t* pairs) {
  clear_error();
  VR_REQUIRE(nb >= 1 && nb <= (1 << 20) && pairs != nullptr, "vr_jacobi_schedule: nb=%lld outside [1, 2^20] or null pairs",
             (long long)nb);
  const int64_t nbe = nb + (nb & 1), half = nbe / 2;
  std::vector<int64_t> idx((size_t)nbe);
  for (int64_t i = 0; i < nbe; ++i) idx[(size_t)i] = i;
  for (int64_t r = 0; r < nbe - 1; ++r) {
    for (int64_t i = 0; i < half; ++i) {
      int64_t a = idx[(size_t)i], c = idx[(size_t)(nbe - 1 - i)];
      if (a > c) std::swap(a, c);
      int32_t* out = pairs + (r * half + i) * 2;
      out[0] = (int32_t)a;
      out[1] = c >= nb ? -1 : (int32_t)c;  // only the padding block nb_even - 1 can be the bye
    }
    // the circle method: block 0 stays, the others rotate by one place
    const int64_t last = idx[(size_t)(nbe - 1)];
    for (int64_t i = nbe - 1; i >= 2; --i) idx[(size_t)i] = idx[(size_t)(i - 1)];
    if (nbe >= 2) idx[1] = last;
  }
  return VR_OK;
}

size_t vr_svd_jacobi_workspace(int64_t batch, int64_t p, int64_t q) {
  if (batch <= 0 || p <= 0 || q <= 0 || std::max(p, q) > SV_MAX_L) return 256;
  return sv_layout(nullptr, batch, sv_geometry(p, q)).bytes;
}

int vr_svd_jacobi_f64(const double* A, int64_t batch, int64_t p, int64_t q, int64_t lda, int64_t stride_a,
                      double* S, double* U, double* Vt, int32_t* null, int32_t* sweeps, void* ws, size_t ws_bytes,
                      void* stream) {
  clear_error();
  VR_REQUIRE(batch >= 0 && batch <= 65535 && p >= 1 && q >= 1 && lda >= q && stride_a >= 0,
             "vr_svd_jacobi_f64: bad shape batch=%lld p=%lld q=%lld lda=%lld", (long long)batch, (long long)p,
             (long long)q, (long long)lda);
  VR_REQUIRE(std::max(p, q) <= SV_MAX_L,
             "vr_svd_jacobi_f64: max(p, q) = %lld is above %lld (two rows of the long side must fit 128 KiB of LDS)",
             (long long)std::max(p, q), (long long)SV_MAX_L);
  if (batch == 0) return VR_OK;
  VR_REQUIRE(A != nullptr && S != nullptr && U != nullptr && Vt != nullptr && null != nullptr && sweeps != nullptr,
             "vr_svd_jacobi_f64: null pointer");
  VR_REQUIRE(batch == 1 || stride_a >= (p - 1) * lda + q, "vr_svd_jacobi_f64: stride_a=%lld overlaps the members",
             (long long)stride_a);
  if (ws == nullptr || ws_bytes < vr_svd_jacobi_workspace(batch, p, q)) {
    set_error("vr_svd_jacobi_f64: workspace too small");
    return VR_EWORKSPACE;
  }
  hipStream_t st = as_stream(stream);
  const SvdGeom g = sv_geometry(p, q);
  const SvdLayout W = sv_layout(ws, batch, g);
  const double m_eps64 = 64.0 * (double)(p + q) * DBL_EPSILON;

  std::vector<int32_t> sched((size_t)(g.nsteps * g.npair * 2));
  VR_TRY(vr_jacobi_schedule(g.nb, sched.data()));
  VR_CHECK_HIP(hipMemcpyAsync(W.pairs, sched.data(), sched.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
  {
    KtScope kt(KT_SVD_STAGE, (double)batch * (double)g.n * (double)g.L * 16.0, st);
    k_svd_stage<<<dim3((unsigned)((g.L + 31) / 32), (unsigned)((g.n + 31) / 32), (unsigned)batch), SV_THREADS, 0, st>>>(
        A, lda, stride_a, g.n, g.L, g.tr, W.B);
    VR_CHECK_LAUNCH();
    const int64_t rn = batch * g.n * g.n;
    k_svd_eye<<<(unsigned)((rn + 255) / 256), 256, 0, st>>>(W.R, g.n, rn);
    VR_CHECK_LAUNCH();
    k_svd_rownorm<<<dim3((unsigned)g.n, (unsigned)batch), SV_THREADS, 0, st>>>(W.B, g.n, g.L, W.norm);
    VR_CHECK_LAUNCH();
    k_svd_setup<<<(unsigned)batch, SV_THREADS, 0, st>>>(W.norm, g.n, m_eps64, W.floor2, W.done, W.count, sweeps);
    VR_CHECK_LAUNCH();
  }
  std::vector<int32_t> flags((size_t)batch);
  VR_CHECK_HIP(hipMemcpyAsync(flags.data(), W.done, (size_t)batch * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  VR_CHECK_HIP(hipStreamSynchronize(st));  // also: the schedule has left the host vector
  bool all_done = std::all_of(flags.begin(), flags.end(), [](int32_t f) { return f != 0; });

  SvdStepParams P;
  P.B = W.B;
  P.R = W.R;
  P.n = g.n;
  P.L = g.L;
  P.pairs = W.pairs;
  P.done = W.done;
  P.count = W.count;
  P.floor2 = W.floor2;
  P.tol = (double)g.L * DBL_EPSILON;
  P.first = 0;
  if (g.b == 8)
    VR_TRY(sv_sweeps<8>(P, g, W, batch, sweeps, flags, all_done, st));
  else if (g.b == 4)
    VR_TRY(sv_sweeps<4>(P, g, W, batch, sweeps, flags, all_done, st));
  else
    VR_TRY(sv_sweeps<2>(P, g, W, batch, sweeps, flags, all_done, st));
  {
    KtScope kt(KT_SVD_FINISH, (double)batch * (double)g.n * (double)(g.n + g.L) * 16.0, st);
    k_svd_rownorm<<<dim3((unsigned)g.n, (unsigned)batch), SV_THREADS, 0, st>>>(W.B, g.n, g.L, W.norm);
    VR_CHECK_LAUNCH();
    k_svd_finish<<<dim3((unsigned)g.n, (unsigned)batch), SV_THREADS, 0, st>>>(W.B, W.R, W.norm, W.done, g.n, g.L, g.tr,
                                                                             m_eps64, S, U, Vt, null);
    VR_CHECK_LAUNCH();
  }
  if (!all_done) {
    int64_t left = 0;
    for (int32_t f : flags) left += f == 0;
    set_error("vr_svd_jacobi_f64: %lld of %lld members still rotated in sweep %d (outputs hold the last iterate)",
              (long long)left, (long long)batch, SV_MAX_SWEEPS);
    return VR_ENOCONV;
  }
  return VR_OK;
}

}  // extern "C"
