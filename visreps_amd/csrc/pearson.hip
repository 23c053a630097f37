// Pearson of two RDMs' strict upper triangles in fp64, replacing
// compute_rdm_correlation(.., correlation="Pearson") -> scipy.stats.pearsonr
// (visreps/analysis/rsa.py:43-47,121-122). Two passes (means, then centred sums) with
// fixed-order reductions, so the result is deterministic.
//
// The same two passes over a sub-RDM A[idx][:, idx] read in place (k_pearson_rows<true>,
// vr_pearson_triu_subset_f32): one bootstrap draw of rsa.py:233-261 with
// compare_method="pearson". The bootstrap engine over many draws is pearson_boot.hip; it
// falls back on these two passes for the draws its one-pass sums cannot decide.
#include "internal.h"

namespace vr {

// SUB: row a and column b are positions in idx (k of them, n = k); the pair is read at the
// upper-triangle entry [min(idx[a], idx[b]), max(..)] whatever the order of idx.
template <bool SUB>
__global__ __launch_bounds__(256) void k_pearson_rows(const float* __restrict__ A,
                                                      const float* __restrict__ B, int64_t n,
                                                      int64_t ld, const int32_t* __restrict__ idx,
                                                      const double* __restrict__ mu,
                                                      double* __restrict__ part) {
  __shared__ double red[5][4];
  const int64_t a = blockIdx.x;
  double s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0;
  const double ma = mu ? mu[0] : 0.0, mb = mu ? mu[1] : 0.0;
  const int64_t ia = SUB ? (int64_t)idx[a] : a;
  for (int64_t b = a + 1 + threadIdx.x; b < n; b += 256) {
    int64_t at = a * ld + b;
    if constexpr (SUB) {
      const int64_t ib = idx[b];
      at = ia < ib ? ia * ld + ib : ib * ld + ia;
    }
    const double x = (double)A[at], y = (double)B[at];
    if (!mu) {
      s0 += x;
      s1 += y;
    } else {
      const double dx = x - ma, dy = y - mb;
      s2 += dx * dy;
      s3 += dx * dx;
      s4 += dy * dy;
    }
  }
  const double v[5] = {s0, s1, s2, s3, s4};
  block_sum_waves<5>(v, red);
  if (threadIdx.x < 5) part[a * 5 + threadIdx.x] = block_sum_total<false>(red[threadIdx.x]);
}

__global__ __launch_bounds__(256) void k_pearson_reduce(const double* __restrict__ part,
                                                        int64_t n, double* __restrict__ mu,
                                                        double* __restrict__ out, int stage,
                                                        double M) {
  __shared__ double red[5][4];
  double v[5] = {0, 0, 0, 0, 0};
  for (int64_t a = threadIdx.x; a < n; a += 256)
    for (int q = 0; q < 5; ++q) v[q] += part[a * 5 + q];
  block_sum_waves<5>(v, red);
  if (threadIdx.x == 0) {
    double s[5];
    for (int q = 0; q < 5; ++q) s[q] = block_sum_total<false>(red[q]);
    if (stage == 0) {
      mu[0] = s[0] / M;
      mu[1] = s[1] / M;
    } else {
      double r;
      if (M < 2 || !(s[3] > 0) || !(s[4] > 0)) {  // constant or NaN input: undefined
        r = __builtin_nan("");
      } else {
        r = s[2] / sqrt(s[3] * s[4]);
        r = r > 1.0 ? 1.0 : (r < -1.0 ? -1.0 : r);
      }
      out[0] = r;
    }
  }
}

// The two passes on stream st: idx == nullptr the full n x n triangle, else the k x k
// sub-RDM (n_or_k = k). part: 5 n_or_k doubles, mu: 2 doubles.
int pearson_two_pass(const float* A, const float* B, int64_t n_or_k, int64_t ld, const int32_t* idx,
                     double* out, double* part, double* mu, hipStream_t st) {
  const int64_t n = n_or_k;
  const double M = (double)pairs_of(n);
  for (int stage = 0; stage < 2; ++stage) {
    if (idx)
      k_pearson_rows<true><<<(unsigned)n, 256, 0, st>>>(A, B, n, ld, idx, stage ? mu : nullptr, part);
    else
      k_pearson_rows<false><<<(unsigned)n, 256, 0, st>>>(A, B, n, ld, nullptr, stage ? mu : nullptr, part);
    VR_CHECK_LAUNCH();
    k_pearson_reduce<<<1, 256, 0, st>>>(part, n, mu, out, stage, M);
    VR_CHECK_LAUNCH();
  }
  return VR_OK;
}

}  // namespace vr

using namespace vr;

extern "C" {

size_t vr_pearson_triu_workspace(int64_t n) {
  Carver c(nullptr);
  c.take<double>((size_t)std::max<int64_t>(n, 1) * 5);
  c.take<double>(2);
  return c.bytes();
}

int vr_pearson_triu_f32(const float* A, const float* B, int64_t n, int64_t ld, double* out,
                        void* ws, size_t ws_bytes, void* stream) {
  VR_REQUIRE(n >= 0 && ld >= n && out != nullptr, "vr_pearson_triu_f32: bad arguments");
  const size_t need = vr_pearson_triu_workspace(n);
  if (ws_bytes < need || ws == nullptr) {
    set_error("vr_pearson_triu_f32: workspace %zu < %zu", ws_bytes, need);
    return VR_EWORKSPACE;
  }
  hipStream_t st = as_stream(stream);
  const int64_t M = pairs_of(n);
  if (M < 2) {
    const double nan = std::nan("");
    VR_CHECK_HIP(hipMemcpyAsync(out, &nan, sizeof(double), hipMemcpyHostToDevice, st));
    VR_CHECK_HIP(hipStreamSynchronize(st));
    return VR_OK;
  }
  Carver c(ws);
  double* part = c.take<double>((size_t)n * 5);
  double* mu = c.take<double>(2);
  return pearson_two_pass(A, B, n, ld, nullptr, out, part, mu, st);
}

size_t vr_pearson_triu_subset_workspace(int64_t k) { return vr_pearson_triu_workspace(k); }

int vr_pearson_triu_subset_f32(const float* A, const float* B, int64_t n, int64_t ld,
                               const int32_t* idx, int64_t k, double* out, void* ws,
                               size_t ws_bytes, void* stream) {
  clear_error();
  VR_REQUIRE(n >= 0 && ld >= n && k >= 0 && k <= n && out != nullptr,
             "vr_pearson_triu_subset_f32: bad arguments");
  const size_t need = vr_pearson_triu_subset_workspace(k);
  if (ws_bytes < need || ws == nullptr) {
    set_error("vr_pearson_triu_subset_f32: workspace %zu < %zu", ws_bytes, need);
    return VR_EWORKSPACE;
  }
  hipStream_t st = as_stream(stream);
  if (pairs_of(k) < 2) {
    const double nan = std::nan("");
    VR_CHECK_HIP(hipMemcpyAsync(out, &nan, sizeof(double), hipMemcpyHostToDevice, st));
    VR_CHECK_HIP(hipStreamSynchronize(st));
    return VR_OK;
  }
  VR_REQUIRE(A != nullptr && B != nullptr && idx != nullptr, "vr_pearson_triu_subset_f32: null pointer");
  Carver c(ws);
  double* part = c.take<double>((size_t)k * 5);
  double* mu = c.take<double>(2);
  return pearson_two_pass(A, B, k, ld, idx, out, part, mu, st);
}

}  // extern "C"
