// Label-conditioned statistics of an (n, d) fp32 activation matrix: per-class, per-feature fp64
// sums and sums of squares (vr_class_moments_f32), each row's distance to its class centre
// (vr_class_dist_f32) and per-row L1 / L2 / active counts (vr_row_sparsity_f32).
//
// Moments. The summation order is the contract: a class's rows in ascending row index, cut into
// chunks of CM_R rows, added one after the other inside a chunk, the chunk partials added in
// ascending order. Nothing else enters a class's result, so it does not depend on the grid or on
// where the rows of other classes lie, and there is no floating-point atomic.
//   k_cm_keys     key = label (C for a label outside [0, C)), value = row
//   radix passes  stable LSD order of (key, row): as many 8-bit digits as C needs (sort.hip)
//   k_cm_bounds   each class's first position in that order (binary search): counts, chunks, skipped
//   scan          chunk offsets per class (scan.hip)
//   k_cm_chunk    one wave per (chunk, column tile): lanes own columns, CM_U rows' loads in flight,
//                 partials to the workspace; n / CM_R x d / tile waves whatever C is
//   k_cm_fold     one thread per (class, column): its partials in order, then the one add of
//                 `accumulate`
// Rows in bucket C come last in the order and are never read.
//
// Row passes. One wave per row. Lane l adds the column groups g = l, l + 64, ... (a group = 4
// consecutive columns) in ascending order, CM_G groups' loads in flight, then the 64 lane partials
// meet in a fixed xor tree.
// The aligned form reads a group as one 16-byte load, the other form as four scalars: the order
// of additions, and so every bit of the result, is the same in both.
#include "internal.h"

#include <cmath>

namespace vr {

constexpr int CM_R = 128;  // rows per chunk (vr_class_moments_chunk_rows)
constexpr int CM_U = 8;    // rows whose loads are in flight together
constexpr int CM_BS = 64;  // one wave per (chunk, column tile)
constexpr int CM_G = 4;    // row passes: column groups of a lane whose loads are in flight together

__global__ __launch_bounds__(256) void k_cm_keys(const int32_t* __restrict__ labels, int64_t n, int64_t C,
                                                 uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int32_t l = labels[i];
  keys[i] = (l >= 0 && (int64_t)l < C) ? (uint32_t)l : (uint32_t)C;
  vals[i] = (uint32_t)i;
}

// First position of the sorted keys that holds a key >= v (n if none).
__device__ inline uint32_t cm_lower_bound(const uint32_t* __restrict__ keys, uint32_t n, uint32_t v) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(256) void k_cm_bounds(const uint32_t* __restrict__ keys, int64_t n, int64_t C,
                                                   uint32_t* __restrict__ cstart, uint32_t* __restrict__ nch,
                                                   int64_t* __restrict__ counts, int64_t* __restrict__ skipped,
                                                   int accumulate) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  const uint32_t lo = cm_lower_bound(keys, (uint32_t)n, (uint32_t)c);
  const uint32_t hi = cm_lower_bound(keys, (uint32_t)n, (uint32_t)c + 1u);
  cstart[c] = lo;
  nch[c] = (hi - lo + (CM_R - 1)) / CM_R;
  counts[c] = (accumulate ? counts[c] : 0) + (int64_t)(hi - lo);
  if (c == C - 1) {
    cstart[C] = hi;
    *skipped = (accumulate ? *skipped : 0) + (n - (int64_t)hi);
  }
}

// Up to four consecutive columns of one row from column j on; entries past d are not read.
template <bool VEC>
__device__ inline void cm_load4(const float* __restrict__ row, int64_t j, int64_t d, float (&v)[4]) {
  if constexpr (VEC) {
    const float4 q = *reinterpret_cast<const float4*>(row + j);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = j + q < d ? row[j + q] : 0.f;
  }
}

// The same columns of a centre row (doubles); VEC: two 16-byte loads.
template <bool VEC>
__device__ inline void cm_centre4(const double* __restrict__ mu, int64_t j, int64_t d, double (&m)[4]) {
  if constexpr (VEC) {
    const double2 lo = *reinterpret_cast<const double2*>(mu + j);
    const double2 hi = *reinterpret_cast<const double2*>(mu + j + 2);
    m[0] = lo.x; m[1] = lo.y; m[2] = hi.x; m[3] = hi.y;
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) m[q] = j + q < d ? mu[j + q] : 0.0;
  }
}

// W = 4 (16-byte loads: d, ldx multiples of 4 and X 16-byte aligned) or 1 columns per lane.
template <int W>
__global__ __launch_bounds__(CM_BS) void k_cm_chunk(
    const float* __restrict__ X, int64_t d, int64_t ldx, const uint32_t* __restrict__ rows,
    const uint32_t* __restrict__ cstart, const uint32_t* __restrict__ chstart, int64_t C,
    const double* __restrict__ centre, double* __restrict__ psum, double* __restrict__ psq) {
  const uint32_t chunk = blockIdx.x;
  if (chunk >= chstart[C]) return;
  // the class of this chunk: the last c with chstart[c] <= chunk (an empty class shares its
  // offset with the next class, which comes later)
  int64_t lo = 0, hi = C;
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (chstart[mid] <= chunk) lo = mid; else hi = mid;
  }
  const int64_t c = lo;
  const int64_t col = ((int64_t)blockIdx.y * CM_BS + threadIdx.x) * W;
  if (col >= d) return;
  const uint32_t r0 = cstart[c] + (chunk - chstart[c]) * CM_R;
  const uint32_t rend = cstart[c + 1];
  const uint32_t r1 = rend - r0 > (uint32_t)CM_R ? r0 + CM_R : rend;

  double mu[W], s[W], ss[W];
#pragma unroll
  for (int q = 0; q < W; ++q) {
    mu[q] = centre ? centre[c * d + col + q] : 0.0;
    s[q] = 0.0;
    ss[q] = 0.0;
  }
  const float* __restrict__ Xc = X + col;
  uint32_t r = r0;
  for (; r + CM_U <= r1; r += CM_U) {
    float v[CM_U][W];
#pragma unroll
    for (int u = 0; u < CM_U; ++u) {
      const float* p = Xc + (int64_t)rows[r + u] * ldx;
      if constexpr (W == 4) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[u][0] = q.x; v[u][1] = q.y; v[u][2] = q.z; v[u][3] = q.w;
      } else {
        v[u][0] = *p;
      }
    }
#pragma unroll
    for (int u = 0; u < CM_U; ++u) {
#pragma unroll
      for (int q = 0; q < W; ++q) {
        const double x = (double)v[u][q] - mu[q];
        s[q] += x;
        ss[q] = fma(x, x, ss[q]);
      }
    }
  }
  for (; r < r1; ++r) {
    const float* p = Xc + (int64_t)rows[r] * ldx;
#pragma unroll
    for (int q = 0; q < W; ++q) {
      const double x = (double)p[q] - mu[q];
      s[q] += x;
      ss[q] = fma(x, x, ss[q]);
    }
  }
  const int64_t o = (int64_t)chunk * d + col;
#pragma unroll
  for (int q = 0; q < W; ++q) {
    psum[o + q] = s[q];
    if (psq) psq[o + q] = ss[q];
  }
}

// blockIdx.y = 0: sum, 1: sumsq. One thread per (class, column).
__global__ __launch_bounds__(256) void k_cm_fold(const double* __restrict__ psum, const double* __restrict__ psq,
                                                 const uint32_t* __restrict__ chstart, int64_t C, int64_t d,
                                                 double* __restrict__ sum, double* __restrict__ sumsq,
                                                 int accumulate) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= C * d) return;
  const int64_t c = e / d, j = e - c * d;
  const double* __restrict__ part = blockIdx.y ? psq : psum;
  double* __restrict__ out = blockIdx.y ? sumsq : sum;
  const uint32_t k0 = chstart[c], k1 = chstart[c + 1];
  if (k0 == k1) {
    if (!accumulate) out[e] = 0.0;
    return;
  }
  double t = part[(int64_t)k0 * d + j];
  uint32_t k = k0 + 1;
  for (; k + 8 <= k1; k += 8) {  // eight loads in flight, the adds still one after the other
    double p[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) p[u] = part[(int64_t)(k + u) * d + j];
#pragma unroll
    for (int u = 0; u < 8; ++u) t += p[u];
  }
  for (; k < k1; ++k) t += part[(int64_t)k * d + j];
  out[e] = accumulate ? out[e] + t : t;
}

// The 64 lane partials of a wave in a fixed tree; every lane ends with the total.
__device__ inline double cm_wave_sum(double t) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
  return t;
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_class_dist(const float* __restrict__ X, int64_t n, int64_t d, int64_t ldx,
                                                    const int32_t* __restrict__ labels, int64_t C,
                                                    const double* __restrict__ centre, double* __restrict__ dist) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const int32_t l = labels[i];
  if (l < 0 || (int64_t)l >= C) {
    if (lane == 0) dist[i] = __builtin_nan("");
    return;
  }
  const float* __restrict__ row = X + i * ldx;
  const double* __restrict__ mu = centre + (int64_t)l * d;
  double t = 0.0;
  int64_t j = (int64_t)lane * 4;
  for (; j + 256 * (CM_G - 1) < d; j += 256 * CM_G) {  // CM_G groups' loads in flight, added in order
    float v[CM_G][4];
    double m[CM_G][4];
#pragma unroll
    for (int u = 0; u < CM_G; ++u) {
      cm_load4<VEC>(row, j + 256 * u, d, v[u]);
      cm_centre4<VEC>(mu, j + 256 * u, d, m[u]);
    }
#pragma unroll
    for (int u = 0; u < CM_G; ++u) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (VEC || j + 256 * u + q < d) {
          const double x = (double)v[u][q] - m[u][q];
          t = fma(x, x, t);
        }
      }
    }
  }
  for (; j < d; j += 256) {
    float v[4];
    double m[4];
    cm_load4<VEC>(row, j, d, v);
    cm_centre4<VEC>(mu, j, d, m);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (VEC || j + q < d) {
        const double x = (double)v[q] - m[q];
        t = fma(x, x, t);
      }
    }
  }
  t = cm_wave_sum(t);
  if (lane == 0) dist[i] = sqrt(t);
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_row_sparsity(const float* __restrict__ X, int64_t n, int64_t d, int64_t ldx,
                                                      float threshold, double* __restrict__ l1,
                                                      double* __restrict__ l2, int64_t* __restrict__ active) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const float* __restrict__ row = X + i * ldx;
  double a = 0.0, b = 0.0;
  uint32_t cnt = 0;  // a lane sees at most d / 64 + 4 entries
  const auto add = [&](float f) {
    const float m = fabsf(f);
    const double x = (double)m;
    a += x;
    b = fma(x, x, b);
    cnt += m > threshold ? 1u : 0u;  // false for NaN
  };
  int64_t j = (int64_t)lane * 4;
  for (; j + 256 * (CM_G - 1) < d; j += 256 * CM_G) {
    float v[CM_G][4];
#pragma unroll
    for (int u = 0; u < CM_G; ++u) cm_load4<VEC>(row, j + 256 * u, d, v[u]);
#pragma unroll
    for (int u = 0; u < CM_G; ++u) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (VEC || j + 256 * u + q < d) add(v[u][q]);
      }
    }
  }
  for (; j < d; j += 256) {
    float v[4];
    cm_load4<VEC>(row, j, d, v);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (VEC || j + q < d) add(v[q]);
    }
  }
  a = cm_wave_sum(a);
  b = cm_wave_sum(b);
  uint64_t total = cnt;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) total += __shfl_xor(total, o, 64);
  if (lane == 0) {
    l1[i] = a;
    l2[i] = sqrt(b);
    active[i] = (int64_t)total;
  }
}

namespace {

constexpr int64_t CM_NMAX = 2147483647;  // rows are uint32 values of the pairs sort; labels are int32

bool cm_vec_ok(const float* X, int64_t d, int64_t ldx) {
  return d % 4 == 0 && ldx % 4 == 0 && (reinterpret_cast<uintptr_t>(X) & 15) == 0;
}

int64_t cm_chunk_cap(int64_t n, int64_t C) { return n / CM_R + (C < n ? C : n); }

struct CmLayout {
  uint32_t *keys, *vals, *keys_alt, *vals_alt, *radix, *cstart, *chstart, *scan;
  double *psum, *psq;
  size_t bytes;
};

CmLayout cm_layout(void* ws, int64_t n, int64_t d, int64_t C) {
  Carver cv(ws);
  CmLayout L;
  L.keys = cv.take<uint32_t>((size_t)n);
  L.vals = cv.take<uint32_t>((size_t)n);
  L.keys_alt = cv.take<uint32_t>((size_t)n);
  L.vals_alt = cv.take<uint32_t>((size_t)n);
  L.radix = cv.take<uint32_t>(radix_ws_elems_bound(n));
  L.cstart = cv.take<uint32_t>((size_t)C + 1);
  L.chstart = cv.take<uint32_t>((size_t)C + 1);
  L.scan = cv.take<uint32_t>(scan_ws_elems(C));
  const size_t part = (size_t)cm_chunk_cap(n, C) * (size_t)d;
  L.psum = cv.take<double>(part);
  L.psq = cv.take<double>(part);
  L.bytes = cv.bytes();
  return L;
}

bool cm_shape_ok(int64_t n, int64_t d, int64_t C) {
  // grid limits: chunks on x, column tiles of 64 on y, the fold's C d / 256 blocks on x
  return n >= 0 && n <= CM_NMAX && d >= 1 && C >= 1 && C <= CM_NMAX - 1 && d <= (int64_t)1 << 21 &&
         cm_chunk_cap(n, C) <= CM_NMAX && (C * d + 255) / 256 <= CM_NMAX;
}

}  // namespace
}  // namespace vr

using namespace vr;

extern "C" int64_t vr_class_moments_chunk_rows(void) { return CM_R; }

extern "C" size_t vr_class_moments_workspace(int64_t n, int64_t d, int64_t C) {
  if (!cm_shape_ok(n, d, C)) return 0;
  return cm_layout(nullptr, n, d, C).bytes;
}

extern "C" int vr_class_moments_f32(const float* X, int64_t n, int64_t d, int64_t ldx, const int32_t* labels,
                                    int64_t C, const double* centre, int64_t* counts, double* sum,
                                    double* sumsq, int64_t* skipped, int accumulate, void* ws, size_t ws_bytes,
                                    void* stream) {
  clear_error();
  VR_REQUIRE(cm_shape_ok(n, d, C), "vr_class_moments_f32: bad shape n=%lld d=%lld C=%lld", (long long)n,
             (long long)d, (long long)C);
  VR_REQUIRE(ldx >= d, "vr_class_moments_f32: ldx=%lld < d=%lld", (long long)ldx, (long long)d);
  VR_REQUIRE(counts && sum && skipped, "vr_class_moments_f32: null output");
  VR_REQUIRE(n == 0 || (X && labels), "vr_class_moments_f32: null input");
  hipStream_t st = as_stream(stream);
  if (n == 0) {
    if (!accumulate) {
      VR_CHECK_HIP(hipMemsetAsync(counts, 0, (size_t)C * sizeof(int64_t), st));
      VR_CHECK_HIP(hipMemsetAsync(skipped, 0, sizeof(int64_t), st));
      VR_CHECK_HIP(hipMemsetAsync(sum, 0, (size_t)C * d * sizeof(double), st));
      if (sumsq) VR_CHECK_HIP(hipMemsetAsync(sumsq, 0, (size_t)C * d * sizeof(double), st));
    }
    return VR_OK;
  }
  const CmLayout L = cm_layout(ws, n, d, C);
  if (!ws || ws_bytes < L.bytes) {
    set_error("vr_class_moments_f32: workspace %zu < %zu", ws_bytes, L.bytes);
    return VR_EWORKSPACE;
  }
  k_cm_keys<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(labels, n, C, L.keys, L.vals);
  VR_CHECK_LAUNCH();
  uint32_t *ki = L.keys, *vi = L.vals, *ko = L.keys_alt, *vo = L.vals_alt;
  for (int shift = 0; shift < 32 && ((uint64_t)C >> shift) != 0; shift += 8) {  // the digits of keys <= C
    VR_TRY(radix_pass_kv(ki, vi, ko, vo, n, shift, L.radix, st));
    uint32_t* t = ki; ki = ko; ko = t;
    t = vi; vi = vo; vo = t;
  }
  k_cm_bounds<<<(unsigned)((C + 255) / 256), 256, 0, st>>>(ki, n, C, L.cstart, L.chstart, counts, skipped,
                                                          accumulate);
  VR_CHECK_LAUNCH();
  VR_TRY(scan_exclusive_u32(L.chstart, L.chstart, C, L.chstart + C, L.scan, st));
  double* psq = sumsq ? L.psq : nullptr;
  const int64_t cap = cm_chunk_cap(n, C);
  if (cm_vec_ok(X, d, ldx)) {
    const dim3 grid((unsigned)cap, (unsigned)((d + CM_BS * 4 - 1) / (CM_BS * 4)));
    k_cm_chunk<4><<<grid, CM_BS, 0, st>>>(X, d, ldx, vi, L.cstart, L.chstart, C, centre, L.psum, psq);
  } else {
    const dim3 grid((unsigned)cap, (unsigned)((d + CM_BS - 1) / CM_BS));
    k_cm_chunk<1><<<grid, CM_BS, 0, st>>>(X, d, ldx, vi, L.cstart, L.chstart, C, centre, L.psum, psq);
  }
  VR_CHECK_LAUNCH();
  const dim3 fgrid((unsigned)((C * d + 255) / 256), sumsq ? 2u : 1u);
  k_cm_fold<<<fgrid, 256, 0, st>>>(L.psum, psq, L.chstart, C, d, sum, sumsq, accumulate);
  VR_CHECK_LAUNCH();
  return VR_OK;
}

extern "C" int vr_class_dist_f32(const float* X, int64_t n, int64_t d, int64_t ldx, const int32_t* labels,
                                 int64_t C, const double* centre, double* dist, void* stream) {
  clear_error();
  VR_REQUIRE(n >= 0 && n <= CM_NMAX && d >= 1 && C >= 1, "vr_class_dist_f32: bad shape n=%lld d=%lld C=%lld",
             (long long)n, (long long)d, (long long)C);
  VR_REQUIRE(ldx >= d, "vr_class_dist_f32: ldx=%lld < d=%lld", (long long)ldx, (long long)d);
  VR_REQUIRE(centre && (n == 0 || (X && labels && dist)), "vr_class_dist_f32: null pointer");
  if (n == 0) return VR_OK;
  hipStream_t st = as_stream(stream);
  const unsigned grid = (unsigned)((n + 3) / 4);
  if (cm_vec_ok(X, d, ldx) && (reinterpret_cast<uintptr_t>(centre) & 15) == 0)
    k_class_dist<true><<<grid, 256, 0, st>>>(X, n, d, ldx, labels, C, centre, dist);
  else
    k_class_dist<false><<<grid, 256, 0, st>>>(X, n, d, ldx, labels, C, centre, dist);
  VR_CHECK_LAUNCH();
  return VR_OK;
}

extern "C" int vr_row_sparsity_f32(const float* X, int64_t n, int64_t d, int64_t ldx, float threshold, double* l1,
                                   double* l2, int64_t* active, void* stream) {
  clear_error();
  VR_REQUIRE(n >= 0 && n <= CM_NMAX && d >= 1, "vr_row_sparsity_f32: bad shape n=%lld d=%lld", (long long)n,
             (long long)d);
  VR_REQUIRE(ldx >= d, "vr_row_sparsity_f32: ldx=%lld < d=%lld", (long long)ldx, (long long)d);
  VR_REQUIRE(n == 0 || (X && l1 && l2 && active), "vr_row_sparsity_f32: null pointer");
  if (n == 0) return VR_OK;
  hipStream_t st = as_stream(stream);
  const unsigned grid = (unsigned)((n + 3) / 4);
  if (cm_vec_ok(X, d, ldx))
    k_row_sparsity<true><<<grid, 256, 0, st>>>(X, n, d, ldx, threshold, l1, l2, active);
  else
    k_row_sparsity<false><<<grid, 256, 0, st>>>(X, n, d, ldx, threshold, l1, l2, active);
  VR_CHECK_LAUNCH();
  return VR_OK;
}
