// Eigenvalues of a dense symmetric fp64 matrix (the PCA eigenspectrum of
// analysis/compute_eigenspectra.py): Householder tridiagonalisation, then Sturm-sequence
// bisection; and the eigenvectors of the k largest (vr_eigh_top_f64, below). Deterministic: every
// reduction has a fixed order, there are no float atomics, and every loop's trip count depends on
// m (and k) alone, so the call always returns.
//
// Stage A, m - 2 steps. A is kept as a full, exactly symmetric matrix, so column k below the
// diagonal is read as row k (contiguous) and every row product of A22 reads contiguous memory.
// Step k (trailing size s = m - k - 1) is two launches; its rank-2 update stays pending and is
// applied by step k + 1's sweep, so A is read and written once per step:
//   k_eig_house  one workgroup: alpha = tau (p . v) / 2 and w = fma(-alpha, v, p) of step k - 1,
//                that update on row k alone, then the Householder vector of the updated row k right
//                of the diagonal: LAPACK's dlarfg with v[0] = 1, scaled by the row's max-abs so
//                entries of 2^+-200 neither overflow nor flush; tau, d[k], e[k]. A zero sub-column
//                writes tau = 0 and e[k] = the element (the sweep then only applies what is pending).
//   k_eig_sweep  one wave per EIG_R rows of A22, lanes along the row: a -= v_i w_j + w_i v_j of step
//                k - 1 with both products rounded and no contraction (the sum is commutative, so
//                (i, j) and (j, i) receive bit-identical values and A stays exactly symmetric), the
//                entry is stored, and p = tau A22 v of step k accumulates from the updated entries;
//                a shuffle tree per row.
// A last k_eig_house applies the update still pending on the final 2 x 2 block.
// Stage B:
//   k_eig_bounds one workgroup: the last 2 x 2 block into d, e; e^2; Gershgorin bounds widened
//                by 2 m eps span; pivmin = DBL_MIN max(1, max e^2) as LAPACK's dstebz.
//   k_eig_bisect one lane per eigenvalue index, EIG_HALVINGS halvings of [lo, hi] on the count
//                of negative q in q = d_i - x - e^2_{i-1} / q; d and e^2 are wave-uniform reads.
// k_eig_scan flags a non-finite entry of A before stage A; k_eig_bounds flags a non-finite d or
// e; a flagged call writes NaN to all of w.
//
// vr_eigh_top_f64, the k largest eigenpairs: stage A with k_eig_house<true>, which leaves every
// Householder vector in the row it annihilated and tau in the workspace; stage B for the top k
// indices (k_eig_bisect_top); then
// Stage C: k_eigv_shifts, k_eigv_start, and EIGV_ITERS times k_eigv_solve (inverse iteration on the
//          tridiagonal, one lane per vector) + k_eigv_orth (Gram-Schmidt inside clusters, in order);
// Stage D: k_eigv_back, one workgroup per vector: V <- Q V, EIGV_NB reflectors per block sum, then
//          the sign (largest-magnitude entry positive) and NaN for a flagged call.
#include <cfloat>
#include <cmath>

#include "internal.h"

namespace vr {

constexpr int64_t EIG_MMAX = 65536;
constexpr int EIG_HT = 1024;       // threads of the one-workgroup kernels
constexpr int EIG_WAVES = 4;       // waves per workgroup of k_eig_sweep
constexpr int EIG_R = 2;           // rows per wave
constexpr int EIG_ROWS = EIG_WAVES * EIG_R;  // 8 rows per workgroup
constexpr int EIG_U = 4;           // columns per lane per trip: 256 columns per wave trip
constexpr int EIG_HALVINGS = 60;   // (hi - lo) 2^-60 < eps span for hi - lo <= 2 span (1 + 2 m eps)
// scal[]: 1 lo, 2 hi, 3 pivmin, 4 + (k & 1) tau of step k
constexpr int EIG_NSCAL = 8;
// Inverse iterations of vr_eigh_top_f64. The shift is within a few eps span of its eigenvalue, so
// one solve grows the wanted direction by about 1 / eps against everything 1e-3 span away (nearer
// vectors are the cluster's, which the Gram-Schmidt walk handles): from the hashed start, whose
// component along any direction is about m^-1/2, two solves already reach every bound of
// tests/test_eigh_top.py; the third is spare for a start vector that happens to be deficient.
constexpr int EIGV_ITERS = 3;

// sum over a block of NW waves: lane partials by a shuffle tree, then the waves in order
template <int NW>
__device__ inline double eig_block_sum(double v, double* red) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  if (lane == 0) red[w] = v;
  __syncthreads();
  double s = 0.0;
  for (int i = 0; i < NW; ++i) s += red[i];
  __syncthreads();
  return s;
}

template <int NW>
__device__ inline double eig_block_max(double v, double* red) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_down(v, o, 64));
  if (lane == 0) red[w] = v;
  __syncthreads();
  double s = red[0];
  for (int i = 1; i < NW; ++i) s = fmax(s, red[i]);
  __syncthreads();
  return s;
}

__global__ __launch_bounds__(256) void k_eig_scan(const double* __restrict__ A, int64_t m, int64_t lda,
                                                  int* __restrict__ flag) {
  bool bad = false;
  for (int64_t r = blockIdx.x; r < m; r += gridDim.x) {
    const double* a = A + r * lda;
    for (int64_t j = threadIdx.x; j < m; j += 256) bad |= !isfinite(a[j]);
  }
  if (bad) *flag = 1;  // every writer stores the same value
}

__device__ inline double eig_w(double p, double v, double alpha) { return fma(-alpha, v, p); }

// the rank-2 term of one entry: v_i w_j + w_i v_j with two rounded products, so (i, j) and (j, i)
// receive the same bits
__device__ inline double eig_r2(double vi, double wi, double vj, double wj) {
#pragma clang fp contract(off)
  const double t1 = vi * wj, t2 = wi * vj;
  return t1 + t2;
}

// Step k, one workgroup. The update of step k - 1 is still pending on A[k.., k..] (vectors of
// length sp = m - k, entry 0 is row k): form w = p - alpha v of that step, apply it to row k alone,
// then form step k's Householder vector from the updated row. last: no step k; rows k and k + 1
// (the final 2 x 2 block) take the pending update.
// KEEP (vr_eigh_top_f64): row k right of the diagonal is dead once the vector is formed (no later
// launch reads it), so the vector the step used is stored back over it, v[0] = 1 at column k + 1,
// and tau at scal[EIG_NSCAL + k]; KEEP = false is the code vr_eigvalsh_f64 has always launched.
template <bool KEEP>
__global__ __launch_bounds__(EIG_HT) void k_eig_house(double* __restrict__ A, int64_t m, int64_t lda, int64_t k,
                                                      int last, double* __restrict__ vbuf,
                                                      const double* __restrict__ p, double* __restrict__ w,
                                                      double* __restrict__ d, double* __restrict__ e,
                                                      double* __restrict__ scal) {
  __shared__ double red[EIG_HT / 64];
  __shared__ double first;
  const int64_t sp = m - k;
  const double* vp = vbuf + ((k + 1) & 1) * m;  // step k - 1's vector
  double* vc = vbuf + (k & 1) * m;
  double* row = A + k * lda + k;
  const double tau_p = k > 0 ? scal[4 + ((k + 1) & 1)] : 0.0;
  if (tau_p != 0.0) {
    double dot = 0.0;
    for (int64_t j = threadIdx.x; j < sp; j += EIG_HT) dot = fma(p[j], vp[j], dot);
    dot = eig_block_sum<EIG_HT / 64>(dot, red);
    const double alpha = 0.5 * tau_p * dot;
    const double v0 = vp[0], w0 = eig_w(p[0], v0, alpha);
    const double v1 = vp[1], w1 = eig_w(p[1], v1, alpha);
    for (int64_t j = threadIdx.x; j < sp; j += EIG_HT) {
      const double vj = vp[j], wj = eig_w(p[j], vj, alpha);
      w[j] = wj;
      row[j] = row[j] - eig_r2(v0, w0, vj, wj);
      if (last) row[lda + j] = row[lda + j] - eig_r2(v1, w1, vj, wj);
    }
  }
  if (last) return;
  // each thread reads back only the entries of row k it wrote itself (j = tid + 1024 t)
  double mx = 0.0;
  for (int64_t j = threadIdx.x; j < sp; j += EIG_HT)
    if (j >= 1) mx = fmax(mx, fabs(row[j]));
  if (threadIdx.x == 1) first = row[1];
  if (threadIdx.x == 0) d[k] = row[0];
  mx = eig_block_max<EIG_HT / 64>(mx, red);
  const double x0 = first;
  double sig = 0.0;
  if (mx > 0.0)
    for (int64_t j = threadIdx.x; j < sp; j += EIG_HT)
      if (j >= 2) {
        const double t = row[j] / mx;
        sig = fma(t, t, sig);
      }
  sig = eig_block_sum<EIG_HT / 64>(sig, red);
  if (!(mx > 0.0) || sig == 0.0) {
    if (threadIdx.x == 0) {
      e[k] = x0;
      scal[4 + (k & 1)] = 0.0;
      if constexpr (KEEP) scal[EIG_NSCAL + k] = 0.0;
    }
    return;
  }
  const double as = x0 / mx;
  const double beta = -copysign(sqrt(fma(as, as, sig)), as);
  const double den = as - beta;
  for (int64_t j = threadIdx.x; j < sp; j += EIG_HT)
    if (j >= 1) {
      const double t = j == 1 ? 1.0 : (row[j] / mx) / den;
      vc[j - 1] = t;
      if constexpr (KEEP) row[j] = t;
    }
  if (threadIdx.x == 0) {
    e[k] = beta * mx;
    scal[4 + (k & 1)] = (beta - as) / beta;
    if constexpr (KEEP) scal[EIG_NSCAL + k] = (beta - as) / beta;
  }
}

// Step k, the one sweep over A22 = A[k + 1.., k + 1..]: apply step k - 1's pending update to every
// row and form p = tau A22 v of step k from the updated entries. A is read and written once.
__global__ __launch_bounds__(EIG_WAVES * 64) void k_eig_sweep(double* __restrict__ A, int64_t m, int64_t lda,
                                                              int64_t k, const double* __restrict__ vbuf,
                                                              const double* __restrict__ w,
                                                              const double* __restrict__ scal,
                                                              double* __restrict__ p) {
  const double tau_p = k > 0 ? scal[4 + ((k + 1) & 1)] : 0.0;
  const double tau_c = scal[4 + (k & 1)];
  if (tau_p == 0.0 && tau_c == 0.0) return;
  const bool upd = tau_p != 0.0, mv = tau_c != 0.0;
  const int64_t s = m - k - 1;
  const double* vp = vbuf + ((k + 1) & 1) * m + 1;  // entry of row k + 1 + i: vp[i], wp[i]
  const double* wp = w + 1;
  const double* vc = vbuf + (k & 1) * m;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t r0 = ((int64_t)blockIdx.x * EIG_WAVES + wid) * EIG_R;
  if (r0 >= s) return;
  const int nr = (int)min<int64_t>(EIG_R, s - r0);
  double vi[EIG_R], wi[EIG_R];
#pragma unroll
  for (int r = 0; r < EIG_R; ++r) {
    const int64_t i = min(r0 + r, s - 1);
    vi[r] = upd ? vp[i] : 0.0;
    wi[r] = upd ? wp[i] : 0.0;
  }
  double* ar[EIG_R];  // rows past the last are clamped: loaded, never stored
#pragma unroll
  for (int r = 0; r < EIG_R; ++r) ar[r] = A + (k + 1 + min(r0 + r, s - 1)) * lda + k + 1;
  double acc[EIG_R][EIG_U];
#pragma unroll
  for (int r = 0; r < EIG_R; ++r)
#pragma unroll
    for (int u = 0; u < EIG_U; ++u) acc[r][u] = 0.0;
  for (int64_t j0 = 0; j0 < s; j0 += 64 * EIG_U) {
    // every load of the trip is issued before its first store: the rows' addresses differ by a
    // run-time lda, so a store between them would order the loads behind it
    double a[EIG_R][EIG_U], vj[EIG_U], wj[EIG_U], cj[EIG_U];
#pragma unroll
    for (int u = 0; u < EIG_U; ++u) {
      const int64_t j = j0 + u * 64 + lane;
      const bool in = j < s;
      vj[u] = (in && upd) ? vp[j] : 0.0;
      wj[u] = (in && upd) ? wp[j] : 0.0;
      cj[u] = (in && mv) ? vc[j] : 0.0;
#pragma unroll
      for (int r = 0; r < EIG_R; ++r) a[r][u] = in ? ar[r][j] : 0.0;
    }
    if (upd) {
#pragma unroll
      for (int u = 0; u < EIG_U; ++u)
#pragma unroll
        for (int r = 0; r < EIG_R; ++r) a[r][u] = a[r][u] - eig_r2(vi[r], wi[r], vj[u], wj[u]);
#pragma unroll
      for (int u = 0; u < EIG_U; ++u) {
        const int64_t j = j0 + u * 64 + lane;
#pragma unroll
        for (int r = 0; r < EIG_R; ++r)
          if (j < s && r < nr) ar[r][j] = a[r][u];
      }
    }
#pragma unroll
    for (int u = 0; u < EIG_U; ++u)
#pragma unroll
      for (int r = 0; r < EIG_R; ++r) acc[r][u] = fma(a[r][u], cj[u], acc[r][u]);
  }
  if (!mv) return;
#pragma unroll
  for (int r = 0; r < EIG_R; ++r) {
    double t = acc[r][0];
#pragma unroll
    for (int u = 1; u < EIG_U; ++u) t += acc[r][u];
    for (int o = 32; o > 0; o >>= 1) t += __shfl_down(t, o, 64);
    if (lane == 0 && r < nr) p[r0 + r] = tau_c * t;
  }
}

__global__ __launch_bounds__(EIG_HT) void k_eig_bounds(const double* __restrict__ A, int64_t m, int64_t lda,
                                                       double* __restrict__ d, double* __restrict__ e,
                                                       double* __restrict__ e2, double* __restrict__ scal,
                                                       int* __restrict__ flag) {
  __shared__ double red[EIG_HT / 64];
  // the last 2 x 2 block is already tridiagonal
  auto dv = [&](int64_t i) { return i >= m - 2 ? A[i * lda + i] : d[i]; };
  auto ev = [&](int64_t i) { return i == m - 2 ? A[(m - 1) * lda + m - 2] : e[i]; };  // i in [0, m - 2]
  double lo = INFINITY, hi = -INFINITY, emax = 0.0;
  bool bad = false;
  for (int64_t i = threadIdx.x; i < m; i += EIG_HT) {
    const double di = dv(i);
    const double el = i > 0 ? ev(i - 1) : 0.0, er = i + 1 < m ? ev(i) : 0.0;
    const double r = fabs(el) + fabs(er);
    bad |= !isfinite(di) || !isfinite(er);
    lo = fmin(lo, di - r);
    hi = fmax(hi, di + r);
    emax = fmax(emax, er * er);
    if (i >= m - 2) d[i] = di;
    if (i + 1 < m) {
      if (i == m - 2) e[i] = er;
      e2[i] = er * er;
    }
  }
  lo = -eig_block_max<EIG_HT / 64>(-lo, red);
  hi = eig_block_max<EIG_HT / 64>(hi, red);
  emax = eig_block_max<EIG_HT / 64>(emax, red);
  if (bad) *flag = 1;
  if (threadIdx.x == 0) {
    const double span = fmax(fabs(lo), fabs(hi));
    const double wide = 2.0 * (double)m * DBL_EPSILON * span;
    scal[1] = lo - wide;
    scal[2] = hi + wide;
    scal[3] = DBL_MIN * fmax(1.0, emax);
  }
}

// eigenvalue idx (ascending, from 0) of the tridiagonal lies in [lo, hi] after EIG_HALVINGS
// halvings of [scal[1], scal[2]]
__device__ inline void eig_bisect_one(const double* __restrict__ d, const double* __restrict__ e2,
                                      const double* __restrict__ scal, int64_t m, int64_t idx, double& lo,
                                      double& hi) {
  lo = scal[1], hi = scal[2];
  const double pivmin = scal[3];
  for (int h = 0; h < EIG_HALVINGS; ++h) {
    const double x = 0.5 * (lo + hi);
    // eigenvalues below x: the negative terms of the Sturm sequence
    double q = d[0] - x;
    if (fabs(q) < pivmin) q = -pivmin;
    int64_t c = q < 0.0 ? 1 : 0;
    int64_t i = 1;
    for (; i + 8 <= m; i += 8) {  // the uniform d, e^2 of 8 terms are fetched ahead of the dependent chain
      double dd[8], ee[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) dd[u] = d[i + u], ee[u] = e2[i - 1 + u];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        q = dd[u] - x - ee[u] / q;
        if (fabs(q) < pivmin) q = -pivmin;
        c += q < 0.0 ? 1 : 0;
      }
    }
    for (; i < m; ++i) {
      q = d[i] - x - e2[i - 1] / q;
      if (fabs(q) < pivmin) q = -pivmin;
      c += q < 0.0 ? 1 : 0;
    }
    if (c > idx)
      hi = x;
    else
      lo = x;
  }
}

__global__ __launch_bounds__(64) void k_eig_bisect(const double* __restrict__ d, const double* __restrict__ e2,
                                                   const double* __restrict__ scal, const int* __restrict__ flag,
                                                   int64_t m, double* __restrict__ w) {
  const int64_t idx = (int64_t)blockIdx.x * 64 + threadIdx.x;
  double lo, hi;
  eig_bisect_one(d, e2, scal, m, idx, lo, hi);
  if (idx < m) w[idx] = *flag ? (double)NAN : 0.5 * (lo + hi);
}

// the k largest, descending: w[j] is eigenvalue m - 1 - j, the same halvings as k_eig_bisect
__global__ __launch_bounds__(64) void k_eig_bisect_top(const double* __restrict__ d, const double* __restrict__ e2,
                                                       const double* __restrict__ scal, const int* __restrict__ flag,
                                                       int64_t m, int64_t k, double* __restrict__ w) {
  const int64_t j = (int64_t)blockIdx.x * 64 + threadIdx.x;
  double lo, hi;
  eig_bisect_one(d, e2, scal, m, m - 1 - j, lo, hi);
  if (j < k) w[j] = *flag ? (double)NAN : 0.5 * (lo + hi);
}

// ---- stage C: inverse iteration on the tridiagonal, one lane per eigenvector -------------------
// Z, U1, U2, U3 are m x kp (kp = k rounded up to 64), entry (i, j) at [i * kp + j]: the lanes of a
// wave read and write contiguously.

// |x| raised to at least piv, the sign kept (+ for 0)
__device__ inline double eig_floor(double x, double piv) { return fabs(x) < piv ? copysign(piv, x) : x; }

// the start vector: a fixed hash of (i, j), magnitude in [0.5, 1.5), either sign
__global__ __launch_bounds__(256) void k_eigv_start(double* __restrict__ Z, int64_t m, int64_t kp) {
  const int64_t n = m * kp;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n; t += (int64_t)gridDim.x * 256) {
    uint64_t x = (uint64_t)(t / kp) * 0x9E3779B97F4A7C15ull + (uint64_t)(t % kp) * 0xBF58476D1CE4E5B9ull +
                 0x94D049BB133111EBull;  // splitmix64's finaliser
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    const double r = 0.5 + (double)(x >> 12) * 0x1p-52;
    Z[t] = (x & 1) ? -r : r;
  }
}

// One thread walks the k eigenvalues in order. lam[j]: the shift of vector j, the eigenvalue moved
// down where it would come within sep = 4 eps span of its predecessor's shift (dstein separates
// coincident eigenvalues the same way: two equal shifts would give two parallel vectors).
// cs[j]: the first vector of j's cluster; j joins j - 1's when their eigenvalues lie within
// 1e-3 span (dstein's ORTOL); span is the larger magnitude of the widened Gershgorin bounds.
__global__ __launch_bounds__(64) void k_eigv_shifts(const double* __restrict__ w, const double* __restrict__ scal,
                                                    int64_t k, double* __restrict__ lam, int64_t* __restrict__ cs) {
  if (threadIdx.x != 0) return;
  const double span = fmax(fabs(scal[1]), fabs(scal[2]));
  const double sep = 4.0 * DBL_EPSILON * span, ortol = 1e-3 * span;
  double lp = w[0], wp = w[0];
  int64_t c = 0;
  lam[0] = lp;
  cs[0] = 0;
  for (int64_t j = 1; j < k; ++j) {
    const double wj = w[j];
    double l = wj;
    if (lp - l < sep) l = lp - sep;
    if (!(wp - wj <= ortol)) c = j;
    lam[j] = l;
    cs[j] = c;
    lp = l;
    wp = wj;
  }
}

// One inverse iteration of every vector: (T - lam_j I) x = z_j by Gaussian elimination with
// partial pivoting (dlagtf's row interchanges), the right-hand side eliminated as the rows are, so
// only U (diagonal U1, superdiagonals U2, U3) is kept for the back-substitution. A pivot below
// piv = max(eps span, pivmin) in magnitude is replaced by +-piv: a change of T within its rounding
// (dlagts perturbs such pivots; pivmin is k_eig_bounds', as dstebz). x is scaled by its max-abs,
// which also keeps matrices of 2^+-200 finite, then to unit length (8 partial sums in index
// order), so only the vectors of a cluster need k_eigv_orth. Both chains of m - 1 dependent steps
// fetch what EIGV_F steps need ahead of them, as k_eig_bisect does; no trip depends on the data.
constexpr int EIGV_F = 8;

__global__ __launch_bounds__(64) void k_eigv_solve(const double* __restrict__ d, const double* __restrict__ e,
                                                   const double* __restrict__ scal, const double* __restrict__ lamv,
                                                   int64_t m, int64_t k, int64_t kp, double* __restrict__ Z,
                                                   double* __restrict__ U1, double* __restrict__ U2,
                                                   double* __restrict__ U3) {
  const int64_t j = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (j >= k) return;
  const double lam = lamv[j];
  const double piv = fmax(DBL_EPSILON * fmax(fabs(scal[1]), fabs(scal[2])), scal[3]);
  double* z = Z + j;
  double* u1 = U1 + j;
  double* u2 = U2 + j;
  double* u3 = U3 + j;
  double a = d[0] - lam, b = m > 1 ? e[0] : 0.0, y = z[0];
  // row i against row i + 1 = (c, dn, en | yn)
  auto step = [&](int64_t i, double c, double dn, double en, double yn) {
    // row i stays, or rows i and i + 1 change places; selects, so the lanes of a wave do not diverge
    const bool stay = fabs(a) >= fabs(c);
    const double p1 = stay ? eig_floor(a, piv) : c;
    const double mult = (stay ? c : a) / p1;
    const double p2 = stay ? b : dn, p3 = stay ? 0.0 : en, yi = stay ? y : yn;
    a = fma(-mult, p2, stay ? dn : b);
    b = stay ? en : -mult * en;
    y = fma(-mult, yi, stay ? yn : y);
    u1[i * kp] = p1;
    u2[i * kp] = p2;
    u3[i * kp] = p3;
    z[i * kp] = yi;
  };
  // The loads of the next EIGV_F steps are issued before this group's stores: loads and stores
  // complete in order, so a load behind the stores would wait for all of them.
  double dd[EIGV_F], ee[EIGV_F + 1], yy[EIGV_F];
  auto fetch = [&](int64_t i0) {  // rows i0 + 1 .. i0 + EIGV_F, clamped: what lies past m - 1 is never used
#pragma unroll
    for (int u = 0; u < EIGV_F; ++u) {
      const int64_t r = min(i0 + 1 + u, m - 1);
      dd[u] = d[r], yy[u] = z[r * kp];
    }
#pragma unroll
    for (int u = 0; u <= EIGV_F; ++u) ee[u] = e[min(i0 + u, m - 1)];
  };
  int64_t i = 0;
  fetch(0);
  for (; i + EIGV_F < m; i += EIGV_F) {  // rows i + 1 .. i + EIGV_F <= m - 1
    double cd[EIGV_F], ce[EIGV_F + 1], cy[EIGV_F];
#pragma unroll
    for (int u = 0; u < EIGV_F; ++u) cd[u] = dd[u], cy[u] = yy[u];
#pragma unroll
    for (int u = 0; u <= EIGV_F; ++u) ce[u] = ee[u];
    fetch(i + EIGV_F);
#pragma unroll
    for (int u = 0; u < EIGV_F; ++u) step(i + u, ce[u], cd[u] - lam, i + u + 2 < m ? ce[u + 1] : 0.0, cy[u]);
  }
  for (; i + 1 < m; ++i) step(i, e[i], d[i + 1] - lam, i + 2 < m ? e[i + 1] : 0.0, z[(i + 1) * kp]);
  // back-substitution, x over z
  double x1 = y / eig_floor(a, piv), x2 = 0.0;  // x[i + 1], x[i + 2]
  double mx = fabs(x1);
  z[(m - 1) * kp] = x1;
  auto back = [&](int64_t r, double p1, double p2, double p3, double yr) {
    const double x = fma(-p3, x2, fma(-p2, x1, yr)) / eig_floor(p1, piv);
    z[r * kp] = x;
    mx = fmax(mx, fabs(x));
    x2 = x1;
    x1 = x;
  };
  double q1[EIGV_F], q2[EIGV_F], q3[EIGV_F];
  auto fetch_back = [&](int64_t i0) {  // rows i0 .. i0 - (EIGV_F - 1), clamped at 0
#pragma unroll
    for (int u = 0; u < EIGV_F; ++u) {
      const int64_t r = max(i0 - u, (int64_t)0) * kp;
      q1[u] = u1[r], q2[u] = u2[r], q3[u] = u3[r], yy[u] = z[r];
    }
  };
  i = m - 2;
  if (i >= 0) fetch_back(i);
  for (; i - (EIGV_F - 1) >= 0; i -= EIGV_F) {
    double c1[EIGV_F], c2[EIGV_F], c3[EIGV_F], cy[EIGV_F];
#pragma unroll
    for (int u = 0; u < EIGV_F; ++u) c1[u] = q1[u], c2[u] = q2[u], c3[u] = q3[u], cy[u] = yy[u];
    fetch_back(i - EIGV_F);
#pragma unroll
    for (int u = 0; u < EIGV_F; ++u) back(i - u, c1[u], c2[u], c3[u], cy[u]);
  }
  for (; i >= 0; --i) back(i, u1[i * kp], u2[i * kp], u3[i * kp], z[i * kp]);
  // x / max|x| (1 / mx may be subnormal, so a division), then to unit length; EIGV_W independent
  // loads in flight per trip, rows past the end clamped and not stored
  constexpr int EIGV_W = 32;
  double ss[EIGV_F];
#pragma unroll
  for (int u = 0; u < EIGV_F; ++u) ss[u] = 0.0;
  for (i = 0; i < m; i += EIGV_W) {
    double x[EIGV_W];
#pragma unroll
    for (int u = 0; u < EIGV_W; ++u) x[u] = z[min(i + u, m - 1) * kp];
#pragma unroll
    for (int u = 0; u < EIGV_W; ++u) {
      const double t = i + u < m ? x[u] / mx : 0.0;
      ss[u % EIGV_F] = fma(t, t, ss[u % EIGV_F]);
    }
  }
  const double nrm = sqrt(((ss[0] + ss[1]) + (ss[2] + ss[3])) + ((ss[4] + ss[5]) + (ss[6] + ss[7])));
  for (i = 0; i < m; i += EIGV_W) {
    double x[EIGV_W];
#pragma unroll
    for (int u = 0; u < EIGV_W; ++u) x[u] = z[min(i + u, m - 1) * kp];
#pragma unroll
    for (int u = 0; u < EIGV_W; ++u)
      if (i + u < m) z[(i + u) * kp] = (x[u] / mx) / nrm;
  }
}

// One workgroup walks the vectors in order: a vector j behind the first of its cluster is
// orthogonalised against the cluster's earlier members by modified Gram-Schmidt, twice (the second
// pass restores what cancellation in the first lost: two shifts in one cluster can give nearly
// parallel vectors), then normalised again. Vectors alone in their cluster leave k_eigv_solve
// finished. A thread owns the entries i = tid + 1024 t of every vector, so only the sums synchronise.
__global__ __launch_bounds__(EIG_HT) void k_eigv_orth(double* __restrict__ Z, const int64_t* __restrict__ cs,
                                                      int64_t m, int64_t k, int64_t kp) {
  __shared__ double red[EIG_HT / 64];
  for (int64_t j = 1; j < k; ++j) {
    const int64_t c0 = cs[j];
    if (c0 == j) continue;
    for (int pass = 0; pass < 2; ++pass)
      for (int64_t c = c0; c < j; ++c) {
        double dot = 0.0;
        for (int64_t i = threadIdx.x; i < m; i += EIG_HT) dot = fma(Z[i * kp + c], Z[i * kp + j], dot);
        dot = eig_block_sum<EIG_HT / 64>(dot, red);
        for (int64_t i = threadIdx.x; i < m; i += EIG_HT) Z[i * kp + j] = fma(-dot, Z[i * kp + c], Z[i * kp + j]);
      }
    double ss = 0.0;
    for (int64_t i = threadIdx.x; i < m; i += EIG_HT) ss = fma(Z[i * kp + j], Z[i * kp + j], ss);
    ss = eig_block_sum<EIG_HT / 64>(ss, red);
    const double nrm = sqrt(ss);
    for (int64_t i = threadIdx.x; i < m; i += EIG_HT) Z[i * kp + j] = Z[i * kp + j] / nrm;
  }
}

// ---- stage D: back-transformation, one workgroup per eigenvector ---------------------------------
// Row j of V takes column j of Z, then z <- H_r z for r = m - 3 .. 0 (Q = H_0 .. H_{m-3}), H_r =
// I - tau_r v_r v_r^T on the entries r + 1 .. m - 1, v_r in row r of A as k_eig_house<true> left
// it. EIGV_NB reflectors r_0 > r_1 > .. are applied per block sum: with g_t = v_t . z and
// G_ts = v_t . v_s of the z before the block (all in one reduction),
//   c_t = tau_t (g_t - sum_{s < t} c_s G_ts),   z <- z - sum_t c_t v_t,
// which is H_{r_3} H_{r_2} H_{r_1} H_{r_0} z (the compact WY form, in registers). Reflectors below
// 0 (the last block) and those with tau = 0 (H = I, their row holds no vector) enter as v = 0.
// A thread owns the entries c = tid + 1024 t of z. Then the sign: the largest-magnitude entry
// positive, the lowest index winning a tie. A flagged call (a non-finite input) writes NaN.
constexpr int EIGV_NB = 4;
constexpr int EIGV_NG = EIGV_NB + EIGV_NB * (EIGV_NB - 1) / 2;  // the g and the G below the diagonal

__global__ __launch_bounds__(EIG_HT) void k_eigv_back(const double* __restrict__ A, int64_t m, int64_t lda,
                                                      const double* __restrict__ tauv, const double* __restrict__ Z,
                                                      int64_t kp, const int* __restrict__ flag,
                                                      double* __restrict__ V, int64_t ldv) {
  __shared__ double red[EIG_HT / 64][EIGV_NG];
  __shared__ double tot[EIGV_NG];
  __shared__ int64_t redi[EIG_HT / 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t j = blockIdx.x;
  double* z = V + j * ldv;
  for (int64_t c = threadIdx.x; c < m; c += EIG_HT) z[c] = Z[c * kp + j];
  for (int64_t r0 = m - 3; r0 >= 0; r0 -= EIGV_NB) {
    double tau[EIGV_NB];
    const double* v[EIGV_NB];  // v_t's entry of index c is v[t][c], c >= r_t + 1
    int64_t lo[EIGV_NB];       // v_t = 0 below lo[t]
#pragma unroll
    for (int t = 0; t < EIGV_NB; ++t) {
      const int64_t r = r0 - t;
      tau[t] = r >= 0 ? tauv[r] : 0.0;
      v[t] = A + (r >= 0 ? r : 0) * lda;
      lo[t] = tau[t] != 0.0 ? r + 1 : m;
    }
    const int64_t first = (r0 - (EIGV_NB - 1) >= 0 ? r0 - (EIGV_NB - 1) : 0) + 1;  // the lowest entry touched
    const int64_t over = first - (int64_t)threadIdx.x;
    const int64_t c0 = threadIdx.x + (over > 0 ? (over + EIG_HT - 1) / EIG_HT * EIG_HT : 0);
    double acc[EIGV_NG];
#pragma unroll
    for (int q = 0; q < EIGV_NG; ++q) acc[q] = 0.0;
#pragma unroll 4
    for (int64_t c = c0; c < m; c += EIG_HT) {
      const double zc = z[c];
      double vc[EIGV_NB];
#pragma unroll
      for (int t = 0; t < EIGV_NB; ++t) vc[t] = c >= lo[t] ? v[t][c] : 0.0;
      int q = EIGV_NB;
#pragma unroll
      for (int t = 0; t < EIGV_NB; ++t) {
        acc[t] = fma(vc[t], zc, acc[t]);
#pragma unroll
        for (int s = 0; s < t; ++s, ++q) acc[q] = fma(vc[t], vc[s], acc[q]);
      }
    }
    // all EIGV_NG sums in one reduction: lanes by a shuffle tree, then thread q adds the waves of
    // sum q in order
#pragma unroll
    for (int q = 0; q < EIGV_NG; ++q) {
      double s = acc[q];
      for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
      if (lane == 0) red[wv][q] = s;
    }
    __syncthreads();
    if (threadIdx.x < EIGV_NG) {
      double s = 0.0;
      for (int w = 0; w < EIG_HT / 64; ++w) s += red[w][threadIdx.x];
      tot[threadIdx.x] = s;
    }
    // red is next written after this barrier and tot after the next block's first one, which no
    // thread passes before every thread has read tot here
    __syncthreads();
#pragma unroll
    for (int q = 0; q < EIGV_NG; ++q) acc[q] = tot[q];
    double cf[EIGV_NB];
    {
      int q = EIGV_NB;
#pragma unroll
      for (int t = 0; t < EIGV_NB; ++t) {
        double g = acc[t];
#pragma unroll
        for (int s = 0; s < t; ++s, ++q) g = fma(-cf[s], acc[q], g);
        cf[t] = tau[t] * g;
      }
    }
#pragma unroll 4
    for (int64_t c = c0; c < m; c += EIG_HT) {
      double zc = z[c];
#pragma unroll
      for (int t = 0; t < EIGV_NB; ++t) zc = fma(-cf[t], c >= lo[t] ? v[t][c] : 0.0, zc);
      z[c] = zc;
    }
  }
  // argmax |z|, lowest index on ties: per thread in increasing c, then lanes, then waves
  double best = -1.0;
  int64_t bi = 0;
  for (int64_t c = threadIdx.x; c < m; c += EIG_HT) {
    const double t = fabs(z[c]);
    if (t > best) best = t, bi = c;
  }
  for (int o = 32; o > 0; o >>= 1) {
    const double ob = __shfl_down(best, o, 64);
    const int64_t oi = __shfl_down(bi, o, 64);
    if (ob > best || (ob == best && oi < bi)) best = ob, bi = oi;
  }
  if (lane == 0) red[wv][0] = best, redi[wv] = bi;
  __syncthreads();  // also orders every write of z before the read of z[bi] below
  best = red[0][0], bi = redi[0];
  for (int i = 1; i < EIG_HT / 64; ++i)
    if (red[i][0] > best || (red[i][0] == best && redi[i] < bi)) best = red[i][0], bi = redi[i];
  const bool neg = z[bi] < 0.0;
  const bool bad = *flag != 0;
  __syncthreads();
  if (neg || bad)
    for (int64_t c = threadIdx.x; c < m; c += EIG_HT) z[c] = bad ? (double)NAN : -z[c];
}

struct EigLayout {
  double *v, *p, *w, *d, *e, *e2, *scal;
  int* flag;
  size_t bytes;
};

static EigLayout eig_layout(void* ws, int64_t m) {
  const size_t mm = (size_t)std::max<int64_t>(m, 1);
  EigLayout L;
  Carver c(ws);
  L.v = c.take<double>(2 * mm);
  L.p = c.take<double>(mm);
  L.w = c.take<double>(mm);
  L.d = c.take<double>(mm);
  L.e = c.take<double>(mm);
  L.e2 = c.take<double>(mm);
  L.scal = c.take<double>(EIG_NSCAL);
  L.flag = c.take<int>(1);
  L.bytes = c.bytes();
  return L;
}

// the non-finite scan and stage A (m >= 1); KEEP as k_eig_house
template <bool KEEP>
static int eig_scan_tridiag(double* A, int64_t m, int64_t lda, const EigLayout& L, hipStream_t st) {
  VR_CHECK_HIP(hipMemsetAsync(L.flag, 0, sizeof(int), st));
  k_eig_scan<<<(unsigned)std::min<int64_t>(m, 4096), 256, 0, st>>>(A, m, lda, L.flag);
  VR_CHECK_LAUNCH();
  // bytes of A22 moved: read and written once per step by k_eig_sweep
  double bytes = 0.0;
  for (int64_t k = 0; k + 2 < m; ++k) bytes += 16.0 * (double)(m - k - 1) * (double)(m - k - 1);
  KtScope kt(KT_EIG_TRIDIAG, bytes, st);
  for (int64_t k = 0; k + 2 < m; ++k) {
    const int64_t s = m - k - 1;
    const unsigned grid = (unsigned)((s + EIG_ROWS - 1) / EIG_ROWS);
    k_eig_house<KEEP><<<1, EIG_HT, 0, st>>>(A, m, lda, k, 0, L.v, L.p, L.w, L.d, L.e, L.scal);
    k_eig_sweep<<<grid, EIG_WAVES * 64, 0, st>>>(A, m, lda, k, L.v, L.w, L.scal, L.p);
  }
  if (m >= 3) k_eig_house<KEEP><<<1, EIG_HT, 0, st>>>(A, m, lda, m - 2, 1, L.v, L.p, L.w, L.d, L.e, L.scal);
  VR_CHECK_LAUNCH();
  return VR_OK;
}

// vr_eigh_top_f64: the layout above with tau of every step behind scal (scal[EIG_NSCAL + k]), then
// the shifts, the cluster starts and the four m x kp arrays of stage C
struct EigTopLayout {
  EigLayout base;
  double *lam, *Z, *U1, *U2, *U3;
  int64_t* cs;
  int64_t kp;
  size_t bytes;
};

static EigTopLayout eig_top_layout(void* ws, int64_t m, int64_t k) {
  const size_t mm = (size_t)std::max<int64_t>(m, 1);
  EigTopLayout T;
  T.kp = (std::max<int64_t>(k, 1) + 63) / 64 * 64;
  const size_t zk = mm * (size_t)T.kp;
  EigLayout& L = T.base;
  Carver c(ws);
  L.v = c.take<double>(2 * mm);
  L.p = c.take<double>(mm);
  L.w = c.take<double>(mm);
  L.d = c.take<double>(mm);
  L.e = c.take<double>(mm);
  L.e2 = c.take<double>(mm);
  L.scal = c.take<double>(EIG_NSCAL + mm);
  L.flag = c.take<int>(1);
  T.lam = c.take<double>((size_t)T.kp);
  T.cs = c.take<int64_t>((size_t)T.kp);
  T.Z = c.take<double>(zk);
  T.U1 = c.take<double>(zk);
  T.U2 = c.take<double>(zk);
  T.U3 = c.take<double>(zk);
  L.bytes = T.bytes = c.bytes();
  return T;
}

}  // namespace vr

using namespace vr;

extern "C" {

size_t vr_eigvalsh_workspace(int64_t m) {
  return eig_layout(nullptr, std::min<int64_t>(std::max<int64_t>(m, 0), EIG_MMAX)).bytes;
}

int vr_eigvalsh_f64(double* A, int64_t m, int64_t lda, double* w, void* ws, size_t ws_bytes, void* stream) {
  clear_error();
  VR_REQUIRE(m >= 0 && m <= EIG_MMAX && lda >= m, "vr_eigvalsh_f64: bad shape m=%lld lda=%lld (m <= %lld)",
             (long long)m, (long long)lda, (long long)EIG_MMAX);
  VR_REQUIRE(m == 0 || (A != nullptr && w != nullptr), "vr_eigvalsh_f64: null pointer");
  const size_t need = eig_layout(nullptr, m).bytes;
  if (ws_bytes < need || ws == nullptr) {
    set_error("vr_eigvalsh_f64: workspace %zu < %zu", ws_bytes, need);
    return VR_EWORKSPACE;
  }
  if (m == 0) return VR_OK;
  hipStream_t st = as_stream(stream);
  const EigLayout L = eig_layout(ws, m);
  VR_TRY(eig_scan_tridiag<false>(A, m, lda, L, st));
  {
    KtScope kt(KT_EIG_BISECT, (double)EIG_HALVINGS * (double)m * (double)m, st);
    k_eig_bounds<<<1, EIG_HT, 0, st>>>(A, m, lda, L.d, L.e, L.e2, L.scal, L.flag);
    k_eig_bisect<<<(unsigned)((m + 63) / 64), 64, 0, st>>>(L.d, L.e2, L.scal, L.flag, m, w);
    VR_CHECK_LAUNCH();
  }
  return VR_OK;
}

size_t vr_eigh_top_workspace(int64_t m, int64_t k) {
  m = std::min<int64_t>(std::max<int64_t>(m, 0), EIG_MMAX);
  return eig_top_layout(nullptr, m, std::min<int64_t>(std::max<int64_t>(k, 0), m)).bytes;
}

int vr_eigh_top_f64(double* A, int64_t m, int64_t lda, int64_t k, double* w, double* V, int64_t ldv, void* ws,
                    size_t ws_bytes, void* stream) {
  clear_error();
  VR_REQUIRE(m >= 0 && m <= EIG_MMAX && k >= 0 && k <= m && lda >= m && ldv >= m,
             "vr_eigh_top_f64: bad shape m=%lld k=%lld lda=%lld ldv=%lld (k <= m <= %lld)", (long long)m,
             (long long)k, (long long)lda, (long long)ldv, (long long)EIG_MMAX);
  VR_REQUIRE(m == 0 || A != nullptr, "vr_eigh_top_f64: null pointer");
  VR_REQUIRE(k == 0 || (w != nullptr && V != nullptr), "vr_eigh_top_f64: null pointer");
  const size_t need = eig_top_layout(nullptr, m, k).bytes;
  if (ws_bytes < need || ws == nullptr) {
    set_error("vr_eigh_top_f64: workspace %zu < %zu", ws_bytes, need);
    return VR_EWORKSPACE;
  }
  if (m == 0 || k == 0) return VR_OK;
  hipStream_t st = as_stream(stream);
  const EigTopLayout T = eig_top_layout(ws, m, k);
  const EigLayout& L = T.base;
  const unsigned kwaves = (unsigned)((k + 63) / 64);
  VR_TRY(eig_scan_tridiag<true>(A, m, lda, L, st));
  {
    KtScope kt(KT_EIG_BISECT, (double)EIG_HALVINGS * (double)m * (double)k, st);
    k_eig_bounds<<<1, EIG_HT, 0, st>>>(A, m, lda, L.d, L.e, L.e2, L.scal, L.flag);
    k_eig_bisect_top<<<kwaves, 64, 0, st>>>(L.d, L.e2, L.scal, L.flag, m, k, w);
    VR_CHECK_LAUNCH();
  }
  {
    KtScope kt(KT_EIG_INVIT, (double)EIGV_ITERS * (double)m * (double)k, st);
    k_eigv_shifts<<<1, 64, 0, st>>>(w, L.scal, k, T.lam, T.cs);
    k_eigv_start<<<(unsigned)std::min<int64_t>((m * T.kp + 255) / 256, 4096), 256, 0, st>>>(T.Z, m, T.kp);
    for (int it = 0; it < EIGV_ITERS; ++it) {
      k_eigv_solve<<<kwaves, 64, 0, st>>>(L.d, L.e, L.scal, T.lam, m, k, T.kp, T.Z, T.U1, T.U2, T.U3);
      k_eigv_orth<<<1, EIG_HT, 0, st>>>(T.Z, T.cs, m, k, T.kp);
    }
    VR_CHECK_LAUNCH();
  }
  {
    // bytes of reflectors read: every vector reads all of them
    KtScope kt(KT_EIG_BACK, 4.0 * (double)k * (double)m * (double)m, st);
    k_eigv_back<<<(unsigned)k, EIG_HT, 0, st>>>(A, m, lda, L.scal + EIG_NSCAL, T.Z, T.kp, L.flag, V, ldv);
    VR_CHECK_LAUNCH();
  }
  return VR_OK;
}

}  // extern "C"
