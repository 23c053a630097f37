// Mantel permutation test of two RDMs: for P joint row/column permutations pi_p of one
// matrix, the sum over unordered pairs {i, j}, i != j, of X[pi_p(i), pi_p(j)] * Y[i, j].
// Replaces the loop
//     for perm in perms: compute_rdm_correlation(A[perm][:, perm], B, correlation=...)
// (rsa.py:96-129 per permutation; the permuted matrix is never materialised). A joint
// permutation maps unordered pairs to unordered pairs one-to-one, so the triangle's mean,
// variance and full-triangle midranks do not depend on pi; only the cross sum is new:
//   Pearson   r_p = S_p / sqrt(SS_a SS_b), S_p = sum (A[pi i, pi j] - ma)(B[i, j] - mb) in fp64
//   Spearman  the same sum over two doubled-midrank matrices (vr_triu_midranks_u32): exact
//             integers, u128 per permutation; rho from the sums on the host (_rho_from_sums)
//
// k_mantel_rows: one workgroup owns row i of the fixed matrix Y and stages it in LDS once for a
// batch of MANTEL_PB permutations. Each wave takes permutations of the batch in turn: it streams
// row pi_p(i) of X coalesced from HBM together with the inverse permutation (uint16, shared by
// all rows, L2-resident), and column c of that row meets the LDS entry Y[i, pi_p^-1(c)]. The full
// square is summed (every unordered pair twice, all rows equal work) and halved at the end. A
// wave's sum runs over the columns in lane-strided order and a shuffle tree, so it depends on the
// permutation alone: not on the batch, the wave or the other permutations of the call. Rows
// longer than lds_cols are staged in chunks of lds_cols columns; each chunk streams the X row
// again and takes the columns whose partner lies in the chunk. One partial per (permutation,
// row); k_mantel_reduce_* adds them in row order. No atomics.
//
// Both matrices are read as full symmetric squares with a zero diagonal. The Pearson entry
// mirrors each RDM's strict upper triangle into such a workspace copy once (mirror_upper_u32:
// the diagonal and lower triangle of the inputs are never read); vr_triu_midranks_u32 writes
// its rank matrix in that form.
#include "window.h"

namespace vr {

constexpr int MANTEL_BS = 1024;         // 16 waves: permutations of a batch, 2 rounds
constexpr int MANTEL_PB = 32;           // permutations per workgroup
constexpr int MANTEL_U = 8;             // columns per lane and step: 8 x 256 B of X in flight per wave
constexpr int MANTEL_LDS_COLS = 36864;  // default lds_cols: 144 of the CU's 160 KiB
constexpr int MANTEL_MIN_COLS = 64;

// out (n x n, leading dimension ldo) = the symmetric matrix whose strict upper triangle is A's,
// diagonal 0. 64 x 64 tiles of the upper triangle are read once (coalesced) and written twice,
// the second time transposed through LDS. out may be A itself (a block reads only its own upper
// tile, and writes after reading it). Values are moved as bit patterns: fp32 or u32.
__global__ __launch_bounds__(256) void k_mirror_upper(const uint32_t* A, int64_t n, int64_t ld,
                                                      uint32_t* out, int64_t ldo) {
  __shared__ uint32_t tile[64][65];
  const int64_t tj = blockIdx.x, ti = blockIdx.y;
  if (tj < ti) return;
  const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
  for (int r = ly; r < 64; r += 4) {
    const int64_t i = ti * 64 + r, j = tj * 64 + lx;
    tile[r][lx] = (i < n && j < n && i < j) ? A[i * ld + j] : 0u;
  }
  __syncthreads();
  for (int r = ly; r < 64; r += 4) {
    const int64_t i = ti * 64 + r, j = tj * 64 + lx;
    if (i < n && j < n) out[i * ldo + j] = (ti != tj || r < lx) ? tile[r][lx] : tile[lx][r];
    const int64_t i2 = tj * 64 + r, j2 = ti * 64 + lx;
    if (ti != tj && i2 < n && j2 < n) out[i2 * ldo + j2] = tile[lx][r];
  }
}

int mirror_upper_u32(const uint32_t* A, int64_t n, int64_t ld, uint32_t* out, int64_t ldo, hipStream_t st) {
  if (n <= 0) return VR_OK;
  const unsigned nt = (unsigned)((n + 63) / 64);
  k_mirror_upper<<<dim3(nt, nt), 256, 0, st>>>(A, n, ld, out, ldo);
  VR_CHECK_LAUNCH();
  return VR_OK;
}

// inv[p][perms[p][j]] = j. inv is zeroed first, so whatever perms holds every entry of inv is a
// column of the matrix; entries outside [0, n) are dropped.
__global__ void k_mantel_inverse(const int32_t* __restrict__ perms, int64_t n, int64_t total,
                                 uint16_t* __restrict__ inv) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int64_t p = e / n, j = e - p * n;
  const uint32_t v = (uint32_t)perms[e];
  if (v < (uint32_t)n) inv[p * n + v] = (uint16_t)j;
}

__device__ inline void wave_sum_u128(uint64_t& lo, uint64_t& hi) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const uint64_t l2 = shfl_xor64(lo, o), h2 = shfl_xor64(hi, o);
    const uint64_t s = lo + l2;
    hi += h2 + (s < lo ? 1u : 0u);
    lo = s;
  }
}

// RANKS: X, Y hold u32 doubled midranks, part is n_perms x n u128 {lo, hi}; else fp32 bit
// patterns, mu = {mean of X's triangle, mean of Y's}, part is n_perms x n doubles.
// grid (n rows, batches of MANTEL_PB permutations); dynamic LDS: min(n, L) words.
template <bool RANKS>
__global__ __launch_bounds__(MANTEL_BS) void k_mantel_rows(
    const uint32_t* __restrict__ X, int64_t ldx, const uint32_t* __restrict__ Y, int64_t ldy, int n,
    const int32_t* __restrict__ perms, const uint16_t* __restrict__ inv, int n_perms, int L,
    const double* __restrict__ mu, void* __restrict__ part) {
  extern __shared__ uint32_t yrow[];
  const int i = blockIdx.x;
  const int p0 = blockIdx.y * MANTEL_PB;
  const int p1 = p0 + MANTEL_PB < n_perms ? p0 + MANTEL_PB : n_perms;
  const int lane = threadIdx.x & 63;
  const int w = (int)wave_uniform(threadIdx.x >> 6);
  double ma = 0.0, mb = 0.0;
  if constexpr (!RANKS) {
    ma = mu[0];
    mb = mu[1];
  }
  for (int c0 = 0; c0 < n; c0 += L) {
    const int len = n - c0 < L ? n - c0 : L;
    __syncthreads();  // the previous chunk's readers
    for (int t = threadIdx.x; t < len; t += MANTEL_BS) yrow[t] = Y[(int64_t)i * ldy + c0 + t];
    __syncthreads();
    for (int p = p0 + w; p < p1; p += MANTEL_BS / 64) {
      uint32_t pi = (uint32_t)sload(perms + (int64_t)p * n + i);
      pi = pi < (uint32_t)n ? pi : (uint32_t)n - 1u;
      const uint32_t* __restrict__ xr = X + (int64_t)pi * ldx;
      const uint16_t* __restrict__ iv = inv + (int64_t)p * n;
      double accf = 0.0;
      u128 acci = 0;
      for (int cb = 0; cb < n; cb += 64 * MANTEL_U) {
        uint32_t xs[MANTEL_U];
        int js[MANTEL_U];
#pragma unroll
        for (int u = 0; u < MANTEL_U; ++u) {  // every load issued before the first use: no branches
          const int c = cb + u * 64 + lane;
          const int cc = c < n ? c : n - 1;
          xs[u] = xr[cc];
          const int jv = (int)iv[cc];
          js[u] = c < n ? jv : -1;
        }
#pragma unroll
        for (int u = 0; u < MANTEL_U; ++u) {
          const uint32_t jj = (uint32_t)(js[u] - c0);  // column of Y's row, within the chunk
          const bool ok = jj < (uint32_t)len;
          const uint32_t y = yrow[ok ? jj : 0u];  // read whatever ok says: the gathers stay in flight together
          if constexpr (RANKS) {
            acci += (u128)((uint64_t)(ok ? xs[u] : 0u) * y);  // the diagonals hold 0
          } else {
            const double t = ((double)__uint_as_float(xs[u]) - ma) * ((double)__uint_as_float(y) - mb);
            accf += (ok && js[u] != i) ? t : 0.0;
          }
        }
      }
      const int64_t o = (int64_t)p * n + i;
      if constexpr (RANKS) {
        uint64_t lo = (uint64_t)acci, hi = (uint64_t)(acci >> 64);
        wave_sum_u128(lo, hi);
        if (lane == 0) {
          uint64_t* q = static_cast<uint64_t*>(part) + 2 * o;
          u128 s = ((u128)hi << 64) | lo;
          if (c0) s += ((u128)q[1] << 64) | q[0];
          q[0] = (uint64_t)s;
          q[1] = (uint64_t)(s >> 64);
        }
      } else {
        for (int s = 32; s > 0; s >>= 1) accf += __shfl_down(accf, s, 64);
        if (lane == 0) {
          double* q = static_cast<double*>(part) + o;
          q[0] = c0 ? q[0] + accf : accf;
        }
      }
    }
  }
}

// sums[p] = (sum over rows, in row order per thread then a fixed tree, of part[p][.]) / 2
__global__ __launch_bounds__(256) void k_mantel_reduce_u128(const uint64_t* __restrict__ part, int64_t n,
                                                            uint64_t* __restrict__ sums) {
  __shared__ uint64_t slo[4], shi[4];
  const int64_t p = blockIdx.x;
  u128 s = 0;
  for (int64_t a = threadIdx.x; a < n; a += 256) {
    const uint64_t* q = part + 2 * (p * n + a);
    s += ((u128)q[1] << 64) | q[0];
  }
  uint64_t lo = (uint64_t)s, hi = (uint64_t)(s >> 64);
  wave_sum_u128(lo, hi);
  if ((threadIdx.x & 63) == 0) {
    slo[threadIdx.x >> 6] = lo;
    shi[threadIdx.x >> 6] = hi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    u128 t = 0;
    for (int q = 0; q < 4; ++q) t += ((u128)shi[q] << 64) | slo[q];
    t >>= 1;  // every unordered pair was met twice
    sums[2 * p] = (uint64_t)t;
    sums[2 * p + 1] = (uint64_t)(t >> 64);
  }
}

// ss = the centred sums of squares of the two triangles, from the per-row partials the second
// pass of pearson_two_pass left in mom (5 doubles per row: [.., .., s_ab, s_aa, s_bb])
__global__ __launch_bounds__(256) void k_mantel_ss(const double* __restrict__ mom, int64_t n,
                                                   double* __restrict__ ss) {
  __shared__ double red[2][4];
  double v[2] = {0, 0};
  for (int64_t a = threadIdx.x; a < n; a += 256) {
    v[0] += mom[a * 5 + 3];
    v[1] += mom[a * 5 + 4];
  }
  block_sum_waves<2>(v, red);
  if (threadIdx.x < 2) ss[threadIdx.x] = block_sum_total<false>(red[threadIdx.x]);
}

__global__ __launch_bounds__(256) void k_mantel_reduce_f64(const double* __restrict__ part, int64_t n,
                                                           const double* __restrict__ ss,
                                                           double* __restrict__ scores) {
  __shared__ double red[1][4];
  const int64_t p = blockIdx.x;
  double v[1] = {0};
  for (int64_t a = threadIdx.x; a < n; a += 256) v[0] += part[p * n + a];
  block_sum_waves<1>(v, red);
  if (threadIdx.x == 0) {
    const double s = 0.5 * block_sum_total<false>(red[0]);  // every unordered pair was met twice
    double r;
    if (!(ss[0] > 0) || !(ss[1] > 0)) {  // constant or non-finite triangle: undefined
      r = __builtin_nan("");
    } else {
      r = s / sqrt(ss[0] * ss[1]);
      r = r > 1.0 ? 1.0 : (r < -1.0 ? -1.0 : r);
    }
    scores[p] = r;
  }
}

__global__ void k_mantel_fill_nan(double* out, int64_t count) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) out[i] = __builtin_nan("");
}

static int mantel_cols(int64_t lds_cols) { return lds_cols == 0 ? MANTEL_LDS_COLS : (int)lds_cols; }

template <bool RANKS>
static int mantel_rows(const uint32_t* X, int64_t ldx, const uint32_t* Y, int64_t ldy, int64_t n,
                       const int32_t* perms, uint16_t* inv, int64_t n_perms, int L, const double* mu,
                       void* part, hipStream_t st) {
  VR_ONCE(VR_CHECK_HIP(hipFuncSetAttribute((const void*)k_mantel_rows<RANKS>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize,
                                           MANTEL_LDS_COLS * (int)sizeof(uint32_t))));
  const int64_t total = n_perms * n;
  VR_CHECK_HIP(hipMemsetAsync(inv, 0, (size_t)total * sizeof(uint16_t), st));
  k_mantel_inverse<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(perms, n, total, inv);
  VR_CHECK_LAUNCH();
  const size_t lds = (size_t)std::min<int64_t>(n, L) * sizeof(uint32_t);
  const dim3 grid((unsigned)n, (unsigned)((n_perms + MANTEL_PB - 1) / MANTEL_PB));
  k_mantel_rows<RANKS><<<grid, MANTEL_BS, lds, st>>>(X, ldx, Y, ldy, (int)n, perms, inv, (int)n_perms, L, mu, part);
  VR_CHECK_LAUNCH();
  return VR_OK;
}

// shared argument checks of the two entry points
static int mantel_check(const char* fn, int64_t n, int64_t ld, int64_t n_perms, int64_t lds_cols) {
  VR_REQUIRE(n >= 0 && ld >= n && n_perms >= 0, "%s: bad shape n=%lld ld=%lld n_perms=%lld", fn, (long long)n,
             (long long)ld, (long long)n_perms);
  VR_REQUIRE(n <= 65535, "%s: n=%lld > 65535 (doubled midranks up to n(n-1) must fit 32 bits)", fn, (long long)n);
  VR_REQUIRE(n_perms <= (int64_t)65535 * MANTEL_PB && n_perms * std::max<int64_t>(n, 1) < ((int64_t)1 << 40),
             "%s: n_perms=%lld too large", fn, (long long)n_perms);
  VR_REQUIRE(lds_cols == 0 || (lds_cols >= MANTEL_MIN_COLS && lds_cols <= MANTEL_LDS_COLS),
             "%s: lds_cols=%lld outside 0 or [%d, %d]", fn, (long long)lds_cols, MANTEL_MIN_COLS, MANTEL_LDS_COLS);
  return VR_OK;
}

struct MantelWs {
  uint32_t *xa, *xb;  // symmetric copies (Pearson)
  uint16_t* inv;
  double *part, *mom, *mu, *ss, *r0;
  uint64_t* ipart;
};

static MantelWs mantel_layout(Carver& c, int64_t n, int64_t n_perms, bool ranks) {
  MantelWs w{};
  const size_t nn = (size_t)std::max<int64_t>(n, 1), np = (size_t)std::max<int64_t>(n_perms, 1);
  w.inv = c.take<uint16_t>(np * nn);
  if (ranks) {
    w.ipart = c.take<uint64_t>(np * nn * 2);
  } else {
    w.xa = c.take<uint32_t>(nn * nn);
    w.xb = c.take<uint32_t>(nn * nn);
    w.part = c.take<double>(np * nn);
    w.mom = c.take<double>(nn * 5);
    w.mu = c.take<double>(2);
    w.ss = c.take<double>(2);
    w.r0 = c.take<double>(1);
  }
  return w;
}

}  // namespace vr

using namespace vr;

extern "C" {

size_t vr_mantel_pearson_workspace(int64_t n, int64_t n_perms) {
  Carver c(nullptr);
  mantel_layout(c, n, n_perms, false);
  return c.bytes();
}

int vr_mantel_pearson_f32(const float* A, const float* B, int64_t n, int64_t ld, const int32_t* perms,
                          int64_t n_perms, int64_t lds_cols, double* scores, void* ws, size_t ws_bytes,
                          void* stream) {
  clear_error();
  VR_TRY(mantel_check("vr_mantel_pearson_f32", n, ld, n_perms, lds_cols));
  if (n_perms == 0) return VR_OK;
  VR_REQUIRE(scores != nullptr, "vr_mantel_pearson_f32: null scores");
  hipStream_t st = as_stream(stream);
  if (pairs_of(n) < 2) {  // scipy: fewer than two pairs
    k_mantel_fill_nan<<<(unsigned)((n_perms + 255) / 256), 256, 0, st>>>(scores, n_perms);
    VR_CHECK_LAUNCH();
    return VR_OK;
  }
  VR_REQUIRE(A && B && perms, "vr_mantel_pearson_f32: null pointer");
  const size_t need = vr_mantel_pearson_workspace(n, n_perms);
  if (ws_bytes < need || ws == nullptr) {
    set_error("vr_mantel_pearson_f32: workspace %zu < %zu", ws_bytes, need);
    return VR_EWORKSPACE;
  }
  Carver c(ws);
  const MantelWs w = mantel_layout(c, n, n_perms, false);
  // means and centred sums of squares: the two fixed-order passes of vr_pearson_triu_f32
  VR_TRY(pearson_two_pass(A, B, n, ld, nullptr, w.r0, w.mom, w.mu, st));
  k_mantel_ss<<<1, 256, 0, st>>>(w.mom, n, w.ss);
  VR_CHECK_LAUNCH();
  VR_TRY(mirror_upper_u32(reinterpret_cast<const uint32_t*>(A), n, ld, w.xa, n, st));
  VR_TRY(mirror_upper_u32(reinterpret_cast<const uint32_t*>(B), n, ld, w.xb, n, st));
  VR_TRY(mantel_rows<false>(w.xa, n, w.xb, n, n, perms, w.inv, n_perms, mantel_cols(lds_cols), w.mu, w.part, st));
  k_mantel_reduce_f64<<<(unsigned)n_perms, 256, 0, st>>>(w.part, n, w.ss, scores);
  VR_CHECK_LAUNCH();
  return VR_OK;
}

size_t vr_mantel_ranks_workspace(int64_t n, int64_t n_perms) {
  Carver c(nullptr);
  mantel_layout(c, n, n_perms, true);
  return c.bytes();
}

int vr_mantel_ranks_u32(const uint32_t* YA, const uint32_t* YB, int64_t n, int64_t ld, const int32_t* perms,
                        int64_t n_perms, int64_t lds_cols, uint64_t* sums, void* ws, size_t ws_bytes,
                        void* stream) {
  clear_error();
  VR_TRY(mantel_check("vr_mantel_ranks_u32", n, ld, n_perms, lds_cols));
  if (n_perms == 0) return VR_OK;
  VR_REQUIRE(sums != nullptr, "vr_mantel_ranks_u32: null sums");
  hipStream_t st = as_stream(stream);
  if (n < 2) {  // no pairs
    VR_CHECK_HIP(hipMemsetAsync(sums, 0, (size_t)n_perms * 2 * sizeof(uint64_t), st));
    return VR_OK;
  }
  VR_REQUIRE(YA && YB && perms, "vr_mantel_ranks_u32: null pointer");
  const size_t need = vr_mantel_ranks_workspace(n, n_perms);
  if (ws_bytes < need || ws == nullptr) {
    set_error("vr_mantel_ranks_u32: workspace %zu < %zu", ws_bytes, need);
    return VR_EWORKSPACE;
  }
  Carver c(ws);
  const MantelWs w = mantel_layout(c, n, n_perms, true);
  VR_TRY(mantel_rows<true>(YA, ld, YB, ld, n, perms, w.inv, n_perms, mantel_cols(lds_cols), nullptr, w.ipart, st));
  k_mantel_reduce_u128<<<(unsigned)n_perms, 256, 0, st>>>(w.ipart, n, sums);
  VR_CHECK_LAUNCH();
  return VR_OK;
}

}  // extern "C"
