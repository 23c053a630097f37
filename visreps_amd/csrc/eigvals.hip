// Eigenvalues of a dense symmetric fp64 matrix, no vectors (the PCA eigenspectrum of
// analysis/compute_eigenspectra.py): Householder tridiagonalisation, then Sturm-sequence
// bisection. Deterministic: every reduction has a fixed order, there are no float atomics, and
// every loop's trip count depends on m alone, so the call always returns.
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
    }
    return;
  }
  const double as = x0 / mx;
  const double beta = -copysign(sqrt(fma(as, as, sig)), as);
  const double den = as - beta;
  for (int64_t j = threadIdx.x; j < sp; j += EIG_HT)
    if (j >= 1) vc[j - 1] = j == 1 ? 1.0 : (row[j] / mx) / den;
  if (threadIdx.x == 0) {
    e[k] = beta * mx;
    scal[4 + (k & 1)] = (beta - as) / beta;
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

__global__ __launch_bounds__(64) void k_eig_bisect(const double* __restrict__ d, const double* __restrict__ e2,
                                                   const double* __restrict__ scal, const int* __restrict__ flag,
                                                   int64_t m, double* __restrict__ w) {
  const int64_t idx = (int64_t)blockIdx.x * 64 + threadIdx.x;
  double lo = scal[1], hi = scal[2];
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
  if (idx < m) w[idx] = *flag ? (double)NAN : 0.5 * (lo + hi);
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
  VR_CHECK_HIP(hipMemsetAsync(L.flag, 0, sizeof(int), st));
  k_eig_scan<<<(unsigned)std::min<int64_t>(m, 4096), 256, 0, st>>>(A, m, lda, L.flag);
  VR_CHECK_LAUNCH();
  {
    // bytes of A22 moved: read and written once per step by k_eig_sweep
    double bytes = 0.0;
    for (int64_t k = 0; k + 2 < m; ++k) bytes += 16.0 * (double)(m - k - 1) * (double)(m - k - 1);
    KtScope kt(KT_EIG_TRIDIAG, bytes, st);
    for (int64_t k = 0; k + 2 < m; ++k) {
      const int64_t s = m - k - 1;
      const unsigned grid = (unsigned)((s + EIG_ROWS - 1) / EIG_ROWS);
      k_eig_house<<<1, EIG_HT, 0, st>>>(A, m, lda, k, 0, L.v, L.p, L.w, L.d, L.e, L.scal);
      k_eig_sweep<<<grid, EIG_WAVES * 64, 0, st>>>(A, m, lda, k, L.v, L.w, L.scal, L.p);
    }
    if (m >= 3) k_eig_house<<<1, EIG_HT, 0, st>>>(A, m, lda, m - 2, 1, L.v, L.p, L.w, L.d, L.e, L.scal);
    VR_CHECK_LAUNCH();
  }
  {
    KtScope kt(KT_EIG_BISECT, (double)EIG_HALVINGS * (double)m * (double)m, st);
    k_eig_bounds<<<1, EIG_HT, 0, st>>>(A, m, lda, L.d, L.e, L.e2, L.scal, L.flag);
    k_eig_bisect<<<(unsigned)((m + 63) / 64), 64, 0, st>>>(L.d, L.e2, L.scal, L.flag, m, w);
    VR_CHECK_LAUNCH();
  }
  return VR_OK;
}

}  // extern "C"
