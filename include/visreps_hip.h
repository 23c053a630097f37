/*
 * visreps_hip.h — C ABI of libvisreps_hip.so, the MI355X (gfx950) implementation of
 * the visreps RSA eval hot path: N×N Pearson RDM → upper-triangle midrank Spearman →
 * bootstrapped Spearman RSA.
 *
 * The reference (yashsmehta/visreps) has no FFI: its boundary is the Python module API
 * (visreps/analysis/rsa.py). Each entry point below names the reference function or
 * loop it replaces; the Python mirror in visreps_amd/analysis/rsa.py binds them with
 * ctypes.
 *
 * Conventions
 *  - Every function returns int status: VR_OK (0) or a negative VR_E* code; the
 *    message of the last failure on the calling thread is vr_last_error().
 *  - Array pointers marked [dev] are caller-owned device pointers (hipMalloc /
 *    torch.Tensor.data_ptr()); [host] pointers are host memory.
 *  - Scratch memory comes from a caller-provided workspace whose size is given by the
 *    matching *_workspace() query. The library never allocates caller-visible memory.
 *  - `stream` is a hipStream_t passed as void*; device work is enqueued on it. Calls whose
 *    launch geometry depends on device data (plan headers, key ranges, level counts)
 *    synchronise it once before returning; INTEGRATION.md lists them.
 *    Functions are reentrant across distinct streams and workspaces.
 *  - A statistic that is undefined (constant input, NaN input, fewer than two pairs)
 *    is returned as NaN in the output value, never as an error status — the same
 *    contract as compute_rdm_correlation (rsa.py:106-109,123-129).
 */
#ifndef VISREPS_HIP_H
#define VISREPS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VR_OK 0
#define VR_EINVAL (-1)    /* invalid argument (shape, pointer, size) */
#define VR_EHIP (-2)      /* HIP runtime error */
#define VR_EWORKSPACE (-3) /* workspace smaller than the *_workspace() query */
#define VR_EINTERNAL (-4)  /* an exact-arithmetic invariant of the result failed (a bug) */
#define VR_ENOCONV (-5)    /* an iteration hit its cap before converging; outputs hold the last iterate */

/* Library version (major*10000 + minor*100 + patch). */
int vr_version(void);
/* Message of the last failing call on this thread ("" if none). */
const char* vr_last_error(void);

/* ------------------------------------------------------------------------------
 * RDM: replaces compute_rdm(X, correlation="Pearson", correction)
 *      visreps/analysis/rsa.py:59-93 (x.float(); x -= mean; std = sqrt(mean(x^2)+c);
 *      zero-variance guard; cov = x@x.T/D; corr = cov/(std_i std_j + c); clamp; diag=1;
 *      rdm = 1 - corr).
 * X [dev] fp32 row-major (n, d) with leading dimension ldx >= d.
 * rdm [dev] fp32 row-major (n, n) with leading dimension ldr >= n. Exactly symmetric,
 * diagonal exactly 0.
 * -------------------------------------------------------------------------- */
size_t vr_rdm_pearson_workspace(int64_t n, int64_t d);
int vr_rdm_pearson_f32(const float* X, int64_t n, int64_t d, int64_t ldx, float* rdm,
                       int64_t ldr, float correction, void* ws, size_t ws_bytes,
                       void* stream);

/* Block-distributed form (multi-GPU): the upper-triangle tiles of 128x128 are numbered
 * row-major (tile (bi,bj), bi <= bj); this computes tiles [tile_begin, tile_end) only and
 * writes each tile and its mirror into rdm. Entries of other tiles are not touched, so
 * ranks that each own a tile range and start from a zeroed rdm can combine with a sum
 * all-reduce. vr_rdm_tile_count(n) = number of tiles, vr_rdm_tile_cost(n, t) = distinct
 * (i <= j) entries of tile t, for balancing ranges. */
int64_t vr_rdm_tile_count(int64_t n);
// Super-tile rows R of the wide kernel in the full n x n launch at width d (0: the wide
// kernel is not used), and whether the 128-tile range [tile_begin, tile_end) is cut only at
// aligned boundaries (tri_start(2r, T), r <= R, or the end of the triangle): such a range's
// tiles are bit-identical to the full launch's (multi-GPU RDM pieces, pipeline.py).
int64_t vr_rdm_wide_rows(int64_t n, int64_t d);
int vr_rdm_range_aligned(int64_t n, int64_t d, int64_t tile_begin, int64_t tile_end);
int64_t vr_rdm_tile_cost(int64_t n, int64_t tile);
/* Rectangle of upper-triangle tile `tile`: rows [row0, row0+rows) x cols
 * [col0, col0+cols), col0 >= row0 (a diagonal tile covers its upper half). Host only;
 * for planners that place tile ranges on ranks (multi-GPU block-distributed RDM). */
int vr_rdm_tile_rect(int64_t n, int64_t tile, int64_t* row0, int64_t* col0, int64_t* rows,
                     int64_t* cols);
size_t vr_rdm_tiles_workspace(int64_t n, int64_t d, int64_t tile_begin, int64_t tile_end);
int vr_rdm_pearson_tiles_f32(const float* X, int64_t n, int64_t d, int64_t ldx, float* rdm,
                             int64_t ldr, float correction, int64_t tile_begin,
                             int64_t tile_end, void* ws, size_t ws_bytes, void* stream);

/* bf16 features (X holds the 16-bit patterns of torch.bfloat16, row-major with leading
 * dimension ldx): the same RDM as vr_rdm_pearson_f32 of X.float() (rsa.py:76 widens any
 * dtype to fp32), computed on the split bf16 MFMA Gram without an fp32 copy of X; the
 * row statistics and the centring read the bf16 values directly (cfg5: ViT / CLIP
 * features at N = 50k). Tile ranges as vr_rdm_pearson_tiles_f32. */
size_t vr_rdm_bf16_workspace(int64_t n, int64_t d, int64_t tile_begin, int64_t tile_end);
int vr_rdm_pearson_bf16(const uint16_t* X, int64_t n, int64_t d, int64_t ldx, float* rdm,
                        int64_t ldr, float correction, void* ws, size_t ws_bytes, void* stream);
int vr_rdm_pearson_tiles_bf16(const uint16_t* X, int64_t n, int64_t d, int64_t ldx, float* rdm,
                              int64_t ldr, float correction, int64_t tile_begin, int64_t tile_end,
                              void* ws, size_t ws_bytes, void* stream);

/* Plain symmetric Gram G = X X^T (fp32 out; the same MFMA kernels, tiling and accuracy
 * as the RDM, without centring or the correlation epilogue). The kernel matrix of the
 * encoding score's ridge regression: replaces the SVD inside himalaya 0.4.9's
 * RidgeCV(solver="svd") as called from visreps/analysis/encoding_score.py:47-62
 * (kernel form: X_val X_tr^T and X_tr X_tr^T are blocks of one Gram of the stacked rows).
 * Always the exact-fp32 kernel, at any n^2 d (the split kernel's records hold centred rows).
 * Workspace: vr_gram_workspace(n, d), which equals vr_rdm_pearson_workspace(n, d) wherever
 * the RDM takes the fp32 kernel too. G is exactly symmetric. */
size_t vr_gram_workspace(int64_t n, int64_t d);
int vr_gram_f32(const float* X, int64_t n, int64_t d, int64_t ldx, float* G, int64_t ldg,
                void* ws, size_t ws_bytes, void* stream);

/* Encoding-score statistic (visreps/analysis/encoding_score.py:206-224): for each of
 * `draws` row subsets (idx [dev] int32 draws x k; null = all n rows, draws = 1) the mean
 * over the v columns of the per-column Pearson r between Y and P (himalaya 0.4.9
 * correlation_score: zscore products, population std), in fp64. An exactly constant column
 * of Y or P, whatever its value, or a non-finite entry among a draw's rows gives NaN for
 * that column and for the draw's score.
 * Y, P [dev] fp32 (n, v) row-major with leading dimension ld. voxel_r [dev] fp64
 * (draws, v) or null. Workspace: vr_corr_score_workspace(v, draws). */
size_t vr_corr_score_workspace(int64_t v, int64_t draws);
int vr_corr_score_f32(const float* Y, const float* P, int64_t n, int64_t v, int64_t ld,
                      const int32_t* idx, int64_t k, int64_t draws, double* scores,
                      double* voxel_r, void* ws, size_t ws_bytes, void* stream);

/* Row statistics of the same RDM (rsa.py:80-87): mean[i] (fp32) and
 * std[i] = sqrt(mean((x-mean)^2) + correction) with std < 10*correction -> 1.
 * Exposed so extraction can emit them alongside the feature rows. */
int vr_row_stats_f32(const float* X, int64_t n, int64_t d, int64_t ldx, float* mean,
                     float* stdv, float correction, void* stream);

/* ------------------------------------------------------------------------------
 * Rank plans: the one-time per-RDM precompute behind every Spearman on that RDM.
 * The strict upper triangle (torch.triu_indices(n, n, 1) order, rsa.py:111) is
 * sorted by value once (LSD radix sort, -0.0 == +0.0), tie groups (equal fp32 values)
 * are marked, and the positions are cut into chunks aligned to group boundaries.
 * Replaces the per-call scipy.stats.rankdata(.., 'average') inside
 * scipy.stats.spearmanr (rsa.py:43-47,121-122).
 * plan [dev]: vr_rank_plan_bytes(n) bytes, owned by the caller, reused across calls.
 * -------------------------------------------------------------------------- */
size_t vr_rank_plan_bytes(int64_t n);
size_t vr_rank_plan_workspace(int64_t n);
int vr_rank_plan_build_f32(const float* rdm, int64_t n, int64_t ld, void* plan,
                           size_t plan_bytes, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------
 * Spearman of two RDMs' upper triangles: replaces
 * compute_rdm_correlation(rdm1, rdm2, correlation="Spearman") (rsa.py:96-129).
 * out [dev] one double. NaN if n<=1, any NaN value, or a constant triangle.
 * -------------------------------------------------------------------------- */
size_t vr_spearman_triu_workspace(int64_t n);
int vr_spearman_triu_f32(const float* A, const float* B, int64_t n, int64_t ld,
                         double* out, void* ws, size_t ws_bytes, void* stream);

/* Pearson of the two upper triangles (fp64), replacing
 * compute_rdm_correlation(.., correlation="Pearson") -> scipy.stats.pearsonr. */
size_t vr_pearson_triu_workspace(int64_t n);
int vr_pearson_triu_f32(const float* A, const float* B, int64_t n, int64_t ld,
                        double* out, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------
 * Bootstrapped Spearman RSA: replaces the loop
 *   for i in range(n_bootstrap):
 *       idx = rng.choice(n, int(0.9n), replace=False)
 *       scores[i] = compute_rdm_correlation(A[idx][:, idx], B[idx][:, idx], "Spearman")
 * visreps/evals.py:355-373 (identical copies evals.py:506-522, rsa.py:233-261).
 *
 * The engine evaluates 64 subsets per pass (one bit per subset in a per-stimulus
 * 64-bit inclusion mask); every score is exact integer midrank arithmetic on the
 * pre-sorted plans, so results do not depend on pass grouping or GPU count.
 *
 * idx [dev] int32 (n_sets, k): stimulus indices of each subset (distinct, in [0,n)).
 *   If full_first != 0 an extra first subset = all n stimuli is evaluated and its
 *   score written to scores[0] (the point estimate, evals.py:347-349), followed by the
 *   n_sets subset scores. scores [dev] double (n_sets + (full_first?1:0)).
 * -------------------------------------------------------------------------- */
size_t vr_bootstrap_workspace(int64_t n);
int vr_bootstrap_spearman_plans(const void* planA, const void* planB, int64_t n,
                                const int32_t* idx, int64_t k, int64_t n_sets,
                                int full_first, double* scores, void* ws,
                                size_t ws_bytes, void* stream);

/* Units that share one RDM: the bootstrap loop of evals.py:323-373 runs every model
 * layer against the same neural RDM with the same RandomState(42) subsets. plan_a (the
 * shared RDM) against each of the n_b plans in planBs [host array of device pointers].
 * Per pass of 64 subsets the rank walk of plan_a runs once for all n_b units. Row j of
 * scores [dev] double (n_b rows, leading dimension ld_scores >= n_sets + full_first)
 * equals vr_bootstrap_spearman_plans(planBs[j], plan_a, ...) bit for bit (Spearman is
 * symmetric and every sum is an exact integer). Workspace grows by 8 bytes per pair for
 * every B plan after the first. */
size_t vr_bootstrap_multi_workspace(int64_t n, int64_t n_b);
int vr_bootstrap_spearman_multi(const void* plan_a, const void* const* planBs, int64_t n_b,
                                int64_t n, const int32_t* idx, int64_t k, int64_t n_sets,
                                int full_first, double* scores, int64_t ld_scores, void* ws,
                                size_t ws_bytes, void* stream);
/* Shared joins for units that share their B plan across up to 4 A plans (the neural RDMs of
 * the regions one model layer is scored against; the per-unit joins of
 * vr_bootstrap_spearman_multi, evals.py:355-373's loop over regions). vr_engine_posmap4
 * interleaves the A plans' pair -> position maps into 16-B records (posmap4: workspace of
 * vr_engine_posmap4_bytes(n)); vr_engine_join4 then gives, for one B plan, posA[i][q] = the
 * position in A plan i of B's pair at position q (M u32 each) with one 16-B gather per pair,
 * where one join per unit gathers a random line per pair for each A plan. */
size_t vr_engine_posmap4_bytes(int64_t n);
int vr_engine_posmap4(const void* const* plan_as, int64_t n_a, int64_t n, void* posmap4, void* stream);
int vr_engine_join4(const void* posmap4, int64_t n_a, const void* plan_b, int64_t n, uint32_t* const* posA,
                    void* stream);
/* vr_bootstrap_spearman_multi with every unit's A positions already joined (posA[j], M u32,
 * from vr_engine_join4 against this call's A plan): the EST passes read them and skip the
 * per-unit joins. posA is in/out: an exact-form pass (a flagged EST pass re-run, or
 * VISREPS_ENGINE_EST=0) rewrites posA[j] in place, with the same values, beside its A chunks.
 * Workspace vr_bootstrap_multi_joined_workspace(n, n_b): 4 B per pair and unit less than
 * vr_bootstrap_multi_workspace (no posA arrays carved for units after the first). */
size_t vr_bootstrap_multi_joined_workspace(int64_t n, int64_t n_b);
int vr_bootstrap_spearman_multi_joined(const void* plan_a, const void* const* planBs, int64_t n_b, int64_t n,
                                       const int32_t* idx, int64_t k, int64_t n_sets, int full_first,
                                       double* scores, int64_t ld_scores, uint32_t* const* posA, void* ws,
                                       size_t ws_bytes, void* stream);
/* The units of n_a <= 4 A plans (regions) x n_b B plans (model layers) on the same subsets,
 * every unit pre-joined: posA[i * n_b + j] = B plan j's pairs in A plan i (vr_engine_join4);
 * unit (j, i)'s scores at scores + (i * n_b + j) * ld_scores. Equal bit for bit to n_a
 * vr_bootstrap_spearman_multi_joined calls (evals.py:323-373's region x layer loop, whose
 * RandomState(42) gives every region the same index sets): the EST passes walk each B plan
 * once for all regions (their window inclusion bits, group flags and B counts are the same),
 * the regions' rank tables resident together; anything off that path (exact form, masks
 * beyond LDS, giant tie groups, a flagged pass) runs the per-region calls. Workspace
 * vr_bootstrap_grid_joined_workspace(n, n_a, n_b) = n_a x the per-region joined workspace. */
size_t vr_bootstrap_grid_joined_workspace(int64_t n, int64_t n_a, int64_t n_b);
int vr_bootstrap_spearman_grid_joined(const void* const* plan_as, int64_t n_a, const void* const* planBs,
                                      int64_t n_b, int64_t n, const int32_t* idx, int64_t k, int64_t n_sets,
                                      int full_first, double* scores, int64_t ld_scores, uint32_t* const* posA,
                                      void* ws, size_t ws_bytes, void* stream);

/* Passes of the bootstrap engines run in a one-gather-per-pair form (absolute ranks kept
 * modulo 2^16 and recovered against a count estimate). A pass whose ranks the estimate
 * cannot recover (very large tie groups, adversarial orders) -- flagged by the A walk's
 * window checks, or by the tail's invariants (B-side included pairs == M', sum of the
 * gathered A ranks == M'(M'+1)) -- is re-run in the exact chunk-base form; this counter is
 * the number of such re-runs in the process so far (scores never depend on it).
 * VISREPS_ENGINE_EST=0 forces the chunk-base form; an exact-form pass that breaks the
 * invariants fails the call with VR_EINTERNAL. */
int64_t vr_engine_est_reruns(void);
/* Of those re-runs, the passes only the tail invariants flagged: the A walk's window checks
 * passed, so the B side recovered a wrong rank (0 unless a bug or a fault injection). */
int64_t vr_engine_est_tail_flags(void);
/* Test hook, not for product use: from the next engine call on, after the A walk of EST
 * pass `pass` one TB row's lanes 1..63 are corrupted (a B-side error the A walk cannot
 * see), so the tail invariants and the exact re-run can be tested. -1 (the default) = off. */
int vr_test_engine_inject(int64_t pass);
/* Engine calls whose first pass's A counts (a count pre-pass before any EST pass) already
 * put some subset's ranks outside the EST 3 window, so the call left EST 3 without spending
 * a flagged EST pass (VISREPS_ENGINE_EST_PREDICT=0 disables the check). */
int64_t vr_engine_est_predicted(void);
/* Of those, the calls run in EST 1 (per-lane count tables) instead of the exact form
 * (VISREPS_ENGINE_EST1_FALLBACK=0: exact form). */
int64_t vr_engine_est1_fallbacks(void);

// Kernel-level HIP-event timing of the hot kernels, for pricing the dominant kernel against
// its roofline on the stream it runs on (bench.py). Off by default; enabling clears the
// totals. kernel: 0 k_rankB EST forms over bootstrap subsets, 1 k_rankB exact form, 2 k_rankA,
// 3 k_join, 4 k_gram3e (256^2 super-tiles), 5 k_gram3/k_gram (128^2 tiles),
// 6 k_countA, 7 k_rankB EST 4 (the full-set pass: point estimates, phase-1 selections), 8 k_kwalk
// (one Kendall stream walk of one pass), 9 k_cov (fp64 MFMA covariance / ridge Gram tiles),
// 13 .. 16 the nearest-neighbour search of vr_knn2_f32: staging, k_knn_cand (units: FLOPs of the
// tiles walked), merge + rerank, k_knn_exact_rows; 17 .. 20 the symmetric eigensolver: stage A
// (units: bytes of A22 moved), bounds + bisection, and for vr_eigh_top_f64 the inverse iterations
// (stage C) and the back-transformation (stage D); 21 .. 23 the Jacobi SVD of vr_svd_jacobi_f64:
// staging (transpose, R = I, first row norms), all the step launches of one sweep (units: FLOPs
// of a full sweep, 3 n^2 L per member; the replay on R runs inside the step kernel), finish.
// units: pairs walked (engine kernels) or tile FLOPs 2 d x tile elements (Gram kernels).
// No reference counterpart (the reference has no native kernels).
int vr_ktimer_enable(int on);
int vr_ktimer_read(int kernel, double* ms, int64_t* launches, double* units);
// Trace marker: launches an empty kernel (k_trace_mark_begin if begin, else
// k_trace_mark_end) on `stream`, to bracket a region in a rocprofv3 kernel trace.
int vr_trace_mark(int begin, int tag, void* stream);

/* One-shot form: builds both plans in the workspace, then runs the engine. */
size_t vr_bootstrap_spearman_workspace(int64_t n);
int vr_bootstrap_spearman_f32(const float* A, const float* B, int64_t n, int64_t ld,
                              const int32_t* idx, int64_t k, int64_t n_sets,
                              int full_first, double* scores, void* ws, size_t ws_bytes,
                              void* stream);

/* ------------------------------------------------------------------------------
 * Kendall tau-a of two RDMs' upper triangles: replaces
 * compute_rdm_correlation(rdm1, rdm2, correlation="Kendall") -> _kendall_tau_a
 * (visreps/analysis/rsa.py:22-40,96-129): scipy.stats.kendalltau tau-b from exact
 * discordant / tie counts, converted to tau-a = tau_b sqrt((n0-tx)(n0-ty)) / n0.
 * out [dev] one double; NaN for n <= 1, NaN input or a constant triangle.
 * -------------------------------------------------------------------------- */
size_t vr_kendall_triu_workspace(int64_t n);
int vr_kendall_triu_f32(const float* A, const float* B, int64_t n, int64_t ld, double* out,
                        void* ws, size_t ws_bytes, void* stream);

/* Kendall tau-a of two plain fp64 vectors of length m: replaces `_kendall_tau_a(x, y)`
 * itself (visreps/analysis/rsa.py:22-40; imported by the reference's
 * tests/test_rsa_bootstrap.py:46). Every unordered pair compared in fp64, exact integer
 * discordant / tie counts, then the same tau-b -> tau-a conversion as vr_kendall_triu_f32.
 * x, y, out [dev]; out = NaN for m < 2, a NaN element or a constant vector. m <= 2^22
 * (O(m^2) pair work; RDM triangles go through vr_kendall_triu_f32). */
size_t vr_kendall_vec_workspace(int64_t m);
int vr_kendall_tau_a_f64(const double* x, const double* y, int64_t m, double* out, void* ws,
                         size_t ws_bytes, void* stream);

/* The same statistic in O(m log m) for any m < 2^32 (the reference's `_kendall_tau_a` has no
 * size cap: scipy.stats.kendalltau's merge-sort counting, rsa.py:28): both vectors to dense
 * ranks (radix sorts), the (x, y)-lexicographic order, then the discordant pairs as the
 * inversions of the y ranks counted one rank bit per level (kendall_full.hip). Exact integer
 * counts, so equal bit for bit to vr_kendall_tau_a_f64 where both run. x, y, out [dev]. */
size_t vr_kendall_full_vec_workspace(int64_t m);
int vr_kendall_full_vec_f64(const double* x, const double* y, int64_t m, double* out, void* ws,
                            size_t ws_bytes, void* stream);

/* Kendall tau-a of the strict upper triangles of two RDMs beyond the rank plans' 16-bit
 * stimulus indices (compute_rdm_correlation(.., "Kendall"), rsa.py:96-129 -> rsa.py:22-40, at
 * n > 65,535): the kendall_full.hip pipeline on the M = n(n-1)/2 < 2^32 triangle elements
 * (n <= 92,681; configs[2]'s 73k RDM). A, B [dev] (n, n) row-major fp32, leading dimension
 * ld; out [dev] one double (NaN for M < 2, NaN input, a constant triangle). */
size_t vr_kendall_full_workspace(int64_t n);
int vr_kendall_full_f32(const float* A, const float* B, int64_t n, int64_t ld, double* out, void* ws,
                        size_t ws_bytes, void* stream);
/* ... of the sub-RDMs A[idx][:, idx], B[idx][:, idx] (k rows idx [dev] int32 into the n x n
 * RDMs, never materialised): one bootstrap draw of evals.py:361-369 with compare_method=kendall
 * beyond the rank plans. Workspace: vr_kendall_full_workspace(k). */
int vr_kendall_full_subset_f32(const float* A, const float* B, int64_t n, int64_t ld, const int32_t* idx,
                               int64_t k, double* out, void* ws, size_t ws_bytes, void* stream);

/* Bootstrapped Kendall RSA on two rank plans: the bootstrap loop of evals.py:355-373 /
 * rsa.py:233-261 with compare_method="kendall". Arguments as
 * vr_bootstrap_spearman_plans; the workspace depends on the number of subsets:
 * vr_bootstrap_kendall_workspace(n, n_sets) covers up to n_sets subsets plus the full set. */
size_t vr_bootstrap_kendall_workspace(int64_t n, int64_t n_sets);
int vr_bootstrap_kendall_plans(const void* planA, const void* planB, int64_t n,
                               const int32_t* idx, int64_t k, int64_t n_sets, int full_first,
                               double* scores, void* ws, size_t ws_bytes, void* stream);

/* Pearson of the sub-RDMs A[idx][:, idx], B[idx][:, idx] (k rows idx [dev] int32 into the
 * n x n RDMs, read in place at the upper-triangle entry of each pair): one bootstrap draw of
 * rsa.py:233-261 with compare_method="pearson", the two fp64 passes of vr_pearson_triu_f32.
 * out [dev] one double (NaN for k <= 2, non-finite input, a constant sub-triangle).
 * idx must lie in [0, n): the kernels read unchecked. */
size_t vr_pearson_triu_subset_workspace(int64_t k);
int vr_pearson_triu_subset_f32(const float* A, const float* B, int64_t n, int64_t ld,
                               const int32_t* idx, int64_t k, double* out,
                               void* ws, size_t ws_bytes, void* stream);

/* Bootstrapped Pearson RSA on the RDMs themselves: the bootstrap loop of evals.py:355-373 /
 * rsa.py:233-261 with compare_method="pearson" as one masked fp64-MFMA GEMM over all
 * subsets (csrc/pearson_boot.hip). idx, k, n_sets, full_first and the scores layout as
 * vr_bootstrap_spearman_plans (idx may be null when n_sets == 0); A, B [dev] (n, n) row-major
 * fp32 with leading dimension ld. Preconditions as for the rank-plan engines: the rows of
 * idx hold distinct indices in [0, n), and the RDMs are symmetric (the upper triangle is
 * read whatever the order of idx). No n <= 65,535 limit. A subset scores NaN for k <= 2, when
 * it contains a non-finite pair (and only then) or when a sub-triangle is constant; scores
 * are bit-identical run to run. Synchronises the stream once (the flags of the subsets that
 * the two-pass kernels recompute). Workspace: vr_bootstrap_pearson_workspace(n, n_sets)
 * covers up to n_sets subsets plus the full set. */
size_t vr_bootstrap_pearson_workspace(int64_t n, int64_t n_sets);
int vr_bootstrap_pearson_f32(const float* A, const float* B, int64_t n, int64_t ld,
                             const int32_t* idx, int64_t k, int64_t n_sets, int full_first,
                             double* scores, void* ws, size_t ws_bytes, void* stream);

/* Linear CKA (analysis/metrics/_cka.py:10-22) of the sub-matrices K[idx][:, idx], L[idx][:, idx]
 * (k rows idx [dev] int32 into the n x n kernel matrices, read in place; idx null with k == n:
 * the whole matrices): two fp64 passes, row and grand means, then the sums of products of the
 * double-centred entries. out [dev] 4 doubles: CKA, tr(KHLH), tr(KHKH), tr(LHLH) with
 * H = I - 11^T / k (hsic is tr / (k - 1)^2). CKA is NaN for k < 2, non-finite input or a
 * sub-matrix whose centred part is exactly zero (a constant one). K, L symmetric; idx must lie
 * in [0, n): the kernels read unchecked. Bit-identical run to run. */
size_t vr_cka_subset_workspace(int64_t k);
int vr_cka_subset_f32(const float* K, const float* L, int64_t n, int64_t ld,
                      const int32_t* idx, int64_t k, double* out,
                      void* ws, size_t ws_bytes, void* stream);

/* Bootstrapped linear CKA: the CKA of every subset as one masked fp64-MFMA GEMM over all
 * subsets (csrc/cka_boot.hip). idx, k, n_sets, full_first, the scores layout, the error codes
 * and the preconditions as vr_bootstrap_pearson_f32: distinct indices in [0, n) per row of
 * idx, symmetric K and L ([dev] (n, n) row-major fp32, leading dimension ld). A subset scores
 * NaN for k < 2, when some (i, j) with i and j in it (the diagonal included) is non-finite in K
 * or L (and only then), or when a centred sub-matrix is zero; n < 2 gives all NaN without
 * reading K or L. Scores are not clamped and are bit-identical run to run. Synchronises the
 * stream once (the flags of the subsets that the two-pass kernels recompute). Workspace:
 * vr_bootstrap_cka_workspace(n, n_sets) covers up to n_sets subsets plus the full set. */
size_t vr_bootstrap_cka_workspace(int64_t n, int64_t n_sets);
int vr_bootstrap_cka_f32(const float* K, const float* L, int64_t n, int64_t ld,
                         const int32_t* idx, int64_t k, int64_t n_sets, int full_first,
                         double* scores, void* ws, size_t ws_bytes, void* stream);

/* Two nearest neighbours of every row, exact (csrc/knn.hip): the search behind the Facco Two-NN
 * intrinsic dimensionality (analysis/compute_twoNN_ID.py:27-78). X [dev] (n, d) row-major fp32,
 * leading dimension ldx >= d, finite, never written. r [dev] (n, 2) doubles: r1 <= r2, the two
 * smallest Euclidean distances from the row to the other rows, each the square root of the fp64
 * sum of the squared (exact) differences; nn [dev] (n, 2) int32 their rows (nullable), ties to
 * the lower index. An fp32-MFMA candidate pass on a centred scratch copy keeps 4 candidates and
 * a cut per row and never forms the n x n matrix; a row whose error bound cannot separate its
 * second distance from the cut is scanned against all rows in fp64. Bit-identical run to run.
 * n < 3 writes NaN distances and -1 indices; n = 0 writes nothing. VR_EINVAL for n < 0,
 * n > 2^20, d < 1, ldx < d or a null X or r; VR_EWORKSPACE for ws_bytes below
 * vr_knn2_workspace(n, d) (linear in n, non-decreasing in n and d). Synchronises the stream once
 * (the number of rows to scan). vr_knn2_last_fallback_rows: rows of the last call on this
 * thread that took the exact scan. */
size_t vr_knn2_workspace(int64_t n, int64_t d);
int vr_knn2_f32(const float* X, int64_t n, int64_t d, int64_t ldx, double* r, int32_t* nn,
                void* ws, size_t ws_bytes, void* stream);
int64_t vr_knn2_last_fallback_rows(void);
/* Two-NN estimate from r [dev] (n, 2): out [dev] 2 doubles, [1 / mean log(r2 / r1), kept] over
 * the rows with r1 > 0 (kept), added in a fixed order; NaN when no row is kept, inf when the
 * mean is zero. */
int vr_twonn_id_f64(const double* r, int64_t n, double* out, void* stream);

/* k nearest neighbours of every row, exact, 1 <= k <= 16: vr_knn2_f32's candidate pass,
 * certificate and exact scan with the list length a parameter. X as there. r [dev] (n, k) doubles,
 * row j the k smallest Euclidean distances from row j to the other rows (fp64 sums of the exact
 * squared differences, then sqrt), ascending by (squared distance, index); nn [dev] (n, k) int32
 * their rows (nullable). A row with fewer than k other rows (n - 1 < k) has NaN and -1 from slot
 * n - 1 on; n = 0 writes nothing. vr_knn_candidates(k): the candidates C(k) >= k + 2 the fp32 pass
 * keeps and the rerank measures per row (-1 for k outside [1, 16]); a row is proven iff all C are
 * rows and r_k^2 + E < cut - E, every other row (and every row when n <= C + 1) is scanned
 * against all rows. Bit-identical run to run; at k = 2 the bits of vr_knn2_f32 for n >= 3.
 * VR_EINVAL for k outside [1, 16] and as vr_knn2_f32; VR_EWORKSPACE below
 * vr_knn_workspace(n, d, k) (0 for a bad k). Synchronises the stream once.
 * vr_knn_last_fallback_rows: rows of the last vr_knn_f32 call on this thread that took the scan. */
int vr_knn_candidates(int k);
size_t vr_knn_workspace(int64_t n, int64_t d, int k);
int vr_knn_f32(const float* X, int64_t n, int64_t d, int64_t ldx, int k, double* r, int32_t* nn,
               void* ws, size_t ws_bytes, void* stream);
int64_t vr_knn_last_fallback_rows(void);
/* Levina-Bickel maximum-likelihood dimension (MacKay and Ghahramani's form) from r [dev] (n, k),
 * 2 <= k <= 16: a row counts iff r_1 > 0 and r_k is finite, s_i = (1 / (k - 1)) sum_{j < k}
 * log(r_k / r_j); out [dev] 2 doubles, [1 / mean s_i, counted], added in the fixed order of
 * vr_twonn_id_f64, whose bits it gives at k = 2. NaN when no row counts, inf when the mean is 0. */
int vr_mle_id_f64(const double* r, int64_t n, int k, double* out, void* stream);
/* Overlap of two neighbour lists nnA, nnB [dev] (n, k) int32 (entries -1 ignored), 1 <= k <= 16.
 * counts [dev] n int32 (nullable): indices common to row i of both lists; totals [dev] 1 + P
 * int64: totals[0] their sum, totals[1 + p] the sum over i of #{a in N_A(i): perm_p[a] in
 * N_B(perm_p[i])} for row p of perms [dev] (P, n) int32, each a permutation of 0..n-1 (the
 * overlap after B's rows are relabelled; P = 0: perms unused). Integer sums. P <= 2^18. */
int vr_mutual_knn_i32(const int32_t* nnA, const int32_t* nnB, int64_t n, int k,
                      const int32_t* perms, int64_t P, int32_t* counts, int64_t* totals,
                      void* stream);

/* ------------------------------------------------------------------------------
 * Phase-1 sparse random projection (extraction side).
 * Replaces torch.sparse.mm(P, flat.t()).t() (visreps/models/utils.py:334-336) with P the
 * CSR (k x D) components_ of sklearn SparseRandomProjection
 * (visreps/models/utils.py:297-322, visreps/analysis/sparse_random_projection.py:83-150).
 * indptr (k+1) / indices (nnz) int32, values (nnz) fp32, X (B x D, row stride ldx) fp32,
 * out (B x k, row stride ldo) fp32 -- all device. fp32 fma in CSR order per output.
 * -------------------------------------------------------------------------- */
size_t vr_srp_workspace(int64_t B, int64_t D);
int vr_srp_csr_f32(const int32_t* indptr, const int32_t* indices, const float* values,
                   int64_t k, int64_t D, const float* X, int64_t B, int64_t ldx, float* out,
                   int64_t ldo, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------
 * Full-triangle Spearman of two RDMs with up to 2^32 - 1 pairs (n <= 92681), no rank plan:
 * the compute_rdm_correlation(.., "Spearman") path above the engine's 16-bit stimulus
 * indices (rsa.py:96-129 at configs[2]'s 73k stimuli). Average ranks from per-key counts
 * of each triangle's fp32 keys (count tables over the key range, no sort) or, when the key
 * range does not fit the workspace, a radix sort of (key, triangle index); exact u128 sums
 * either way; out [device] one double. vr_spearman_full_workspace(n) covers every RDM whose
 * values span at most 2^30 + 1 fp32 keys (all correlation-distance RDMs: values in [0, 2]);
 * on a wider range the call returns VR_EWORKSPACE and vr_spearman_full_sort_workspace(n)
 * is the size that always suffices.
 * -------------------------------------------------------------------------- */
size_t vr_spearman_full_workspace(int64_t n);
size_t vr_spearman_full_sort_workspace(int64_t n);
/* Form the last vr_spearman_full_* call took: 0 bucketed count tables, 1 plain count tables,
 * 2 radix sort (-1 before any call). */
int vr_spearman_full_last_form(void);
int vr_spearman_full_f32(const float* A, const float* B, int64_t n, int64_t ld, double* out,
                         void* ws, size_t ws_bytes, void* stream);
/* ... of the sub-RDMs A[idx][:, idx], B[idx][:, idx] (k rows idx [dev] int32, never
 * materialised): one bootstrap draw of evals.py:361-369 beyond the rank plans' n <= 65,535
 * (the bootstrap engine's per-pass TB rows would need 128 B per pair: 341 GB at 73k).
 * Workspace: vr_spearman_full_workspace(k). */
int vr_spearman_full_subset_f32(const float* A, const float* B, int64_t n, int64_t ld, const int32_t* idx,
                                int64_t k, double* out, void* ws, size_t ws_bytes, void* stream);
/* Local pieces of the distributed global rank (sample sort over ranks,
 * visreps_amd/analysis/distributed_spearman.py): sortable keys of fp32 values, an in-place
 * (key, value) radix sort, doubled midranks (+ 2 base) of a sorted key run with its tie
 * term sum (k^3 - k) as a u128 {lo, hi}, and an exact u64 dot product (u128 {lo, hi}). */
/* Count-table form of the same global rank (no sort, no key exchange): per-key counts of a
 * rank's sortable keys in [kmin, kmin + bins) into cnt[bins + 1] (zeroed by the caller;
 * atomics), which the caller sums over ranks; then, on the summed table, the tie term sum
 * (c^3 - c) as a u128 {lo, hi}, the table turned into exclusive starts in place, and the
 * doubled midranks cnt[k] + cnt[k + 1] + 1 of this rank's keys. */
int vr_key_counts_u32(const uint32_t* keys, int64_t m, uint32_t kmin, int64_t bins, uint32_t* cnt, void* stream);
size_t vr_key_table_workspace(int64_t bins);
int vr_key_table_midranks(const uint32_t* keys, int64_t m, uint32_t kmin, uint32_t* cnt, int64_t bins, uint64_t* y,
                          uint64_t* tie, void* ws, size_t ws_bytes, void* stream);
int vr_f32_sort_keys(const float* v, int64_t m, uint32_t* keys, void* stream);
size_t vr_sort_pairs_workspace(int64_t m);
int vr_sort_pairs_u32(uint32_t* keys, uint32_t* vals, int64_t m, void* ws, size_t ws_bytes,
                      void* stream);
size_t vr_midranks_workspace(int64_t m);
int vr_midranks_sorted(const uint32_t* keys, int64_t m, uint64_t base, uint64_t* y, uint64_t* tie,
                       void* ws, size_t ws_bytes, void* stream);
size_t vr_dot_u64_workspace(void);
int vr_dot_u64(const uint64_t* a, const uint64_t* b, int64_t m, uint64_t* out, void* ws,
               size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------
 * Mantel permutation test of two RDMs (csrc/mantel.hip): replaces the loop
 *     for perm in perms: compute_rdm_correlation(A[perm][:, perm], B, correlation=...)
 * (rsa.py:96-129 once per permutation, with one n x n gather each). A joint row/column
 * permutation maps unordered pairs to unordered pairs one-to-one, so the triangle's mean,
 * variance and full-triangle midranks do not depend on it: per permutation only the sum over
 * pairs of A[perm i, perm j] * B[i, j] is new, and the permuted matrix is never formed.
 * perms [dev] (n_perms, n) int32; every row MUST be a permutation of 0..n-1: the kernels stay
 * inside their buffers whatever it holds, but the sums of a row that is not one mean nothing
 * (the Python wrapper rejects such rows on the host before any launch). A result depends on its
 * own permutation alone: not on n_perms, nor on the other rows of perms; the same call twice is
 * bit-identical (fixed-order sums, no atomics). n <= 65535 (VR_EINVAL above: doubled midranks
 * up to n(n-1) must fit 32 bits). lds_cols: the most entries of a matrix row a workgroup holds
 * in LDS at once, 0 (the default, 36864 = 144 KiB) or 64 .. 36864; longer rows are walked in
 * chunks of lds_cols, each streaming the permuted row again. n_perms = 0 writes nothing.
 * -------------------------------------------------------------------------- */
/* Y [dev] (n, n) u32, leading dimension ldy >= n, symmetric: Y[i][j] = Y[j][i] = the doubled
 * midrank (2 .. 2M, M = n(n-1)/2; average ranks for ties) of A[min(i,j)][max(i,j)] among A's
 * strict upper triangle, diagonal 0. Only A's strict upper triangle is read. tie [dev] the term
 * sum (t^3 - t) over tie groups as u128 {lo, hi}; nan_flag [dev] one u32, non-zero if the
 * triangle holds a NaN (the ranks then follow the key order and mean nothing to scipy). Key order
 * and tie groups are vr_f32_sort_keys's (-0.0 == +0.0). The radix sort and midrank kernels of
 * vr_spearman_full_f32's sort form. */
size_t vr_triu_midranks_workspace(int64_t n);
int vr_triu_midranks_u32(const float* A, int64_t n, int64_t ld, uint32_t* Y, int64_t ldy, uint64_t* tie,
                         uint32_t* nan_flag, void* ws, size_t ws_bytes, void* stream);
/* Pearson: scores [dev] n_perms doubles, scores[p] = clamp(S_p / sqrt(SS_a SS_b), -1, 1) with
 * S_p = sum over i < j of (A[perm i, perm j] - mean_a)(B[i, j] - mean_b) in fp64; the means and
 * SS come from the two fixed-order passes of vr_pearson_triu_f32. Only the strict upper
 * triangles of A and B are read ([min, max] of each pair): the diagonal and the lower triangle
 * may hold anything. NaN in every score for n(n-1)/2 < 2, a constant triangle, or a non-finite
 * value in either strict upper triangle (vr_pearson_triu_f32's cases). */
size_t vr_mantel_pearson_workspace(int64_t n, int64_t n_perms);
int vr_mantel_pearson_f32(const float* A, const float* B, int64_t n, int64_t ld, const int32_t* perms,
                          int64_t n_perms, int64_t lds_cols, double* scores, void* ws, size_t ws_bytes,
                          void* stream);
/* Spearman: YA, YB [dev] two rank matrices as vr_triu_midranks_u32 writes them (symmetric,
 * zero diagonal, both with leading dimension ld). sums [dev] n_perms x u128 {lo, hi}:
 * sums[p] = sum over i < j of YA[perm i, perm j] * YB[i, j], exact integers, no floating point
 * and so no NaN rule (the caller turns a nan_flag into NaN scores). */
size_t vr_mantel_ranks_workspace(int64_t n, int64_t n_perms);
int vr_mantel_ranks_u32(const uint32_t* YA, const uint32_t* YB, int64_t n, int64_t ld, const int32_t* perms,
                        int64_t n_perms, int64_t lds_cols, uint64_t* sums, void* ws, size_t ws_bytes,
                        void* stream);

/* ------------------------------------------------------------------------------
 * Multi-GPU RDM pieces (stimulus-sharded rows); replace the
 * block-distributed use of vr_rdm_pearson_tiles_f32 + a sum all-reduce:
 *  - each rank splits its own rows (row stats + centred bf16 hi/lo plane records);
 *  - the planes and stats are all-gathered (the only feature exchange);
 *  - each rank computes its tile range from the gathered planes;
 *  - the ranges are exchanged packed (vr_rdm_tiles_pack -> all-gather -> unpack, which
 *    also writes the mirror), instead of a zero-filled n x n sum all-reduce.
 * Plane buffers hold vr_rdm_plane_rows(n) rows of vr_rdm_plane_row_bytes(d) bytes, rows
 * >= n zero. A packed tile range holds 128 x 128 floats per tile, in tile order.
 * -------------------------------------------------------------------------- */
int64_t vr_rdm_plane_rows(int64_t n);
size_t vr_rdm_plane_row_bytes(int64_t d);
int vr_rdm_split_rows_f32(const float* X, int64_t rows, int64_t d, int64_t ldx, float correction,
                          float* mean, float* stdv, uint16_t* planes, void* stream);
/* The same split for the same `rows` rows of npts points (<= 32) in one launch (rows x npts
 * blocks): X[p] (rows, d[p]) with row stride ldx[p], outputs mean[p], stdv[p], planes[p].
 * Host arrays of device pointers. Used by bench.extract_split on each extraction batch. */
int vr_rdm_split_rows_multi_f32(int npts, const float* const* X, const int64_t* d, const int64_t* ldx,
                                int64_t rows, float correction, float* const* mean, float* const* stdv,
                                uint16_t* const* planes, void* stream);
/* Rows src[i] (host array, nrows entries) of every point's X[p] (row stride ldx[p], d[p]
 * floats) to rows dst[i] of out[p] (row stride ldo[p]): one launch per 64 rows for all
 * npts (<= 32) points. bench.extract_split keeps the phase-1 selection rows of each
 * extraction batch with it (the rows `RandomState(42).choice` picks, evals.py:259-263). */
int vr_gather_rows_multi_f32(int npts, const float* const* X, const int64_t* d, const int64_t* ldx,
                             int nrows, const int32_t* src, const int32_t* dst, float* const* out,
                             const int64_t* ldo, void* stream);
size_t vr_rdm_planes_tiles_workspace(int64_t n, int64_t d, int64_t tile_begin, int64_t tile_end);
int vr_rdm_pearson_tiles_planes(const uint16_t* planes, const float* mean, const float* stdv,
                                int64_t n, int64_t d, float* rdm, int64_t ldr, float correction,
                                int64_t tile_begin, int64_t tile_end, void* ws, size_t ws_bytes,
                                void* stream);
int vr_rdm_tiles_pack(const float* rdm, int64_t ldr, int64_t n, int64_t tile_begin,
                      int64_t tile_end, float* packed, void* stream);
int vr_rdm_tiles_unpack(const float* packed, int64_t n, int64_t tile_begin, int64_t tile_end,
                        float* rdm, int64_t ldr, void* stream);

/* One RDM over stimulus-sharded rows behind the C ABI (SURVEY §8(b),(e)): rank `rank` of an
 * RCCL communicator `comm` (ncclComm_t) holds rows_local <= ceil(n / world) consecutive
 * stimulus rows X_local [dev] fp32 (row stride ldx), the ranks' blocks in rank order make
 * the n rows. Block sizes, the split bf16 hi/lo plane records (+ row statistics) and the
 * packed tile ranges are all-gathered over RCCL; each rank computes one tile range cut at
 * the wide kernel's aligned boundaries (vr_rdm_sharded_range: bit-identical tiles to the
 * one-GPU split-Gram launch), and every rank ends with the full RDM in rdm [dev] (ldr >= n).
 * Collective: every rank calls it with the same n, d, world. RCCL is bound at run time
 * (librccl.so.1, the copy torch loaded if any); vr_rccl_* create a communicator from it for
 * callers without their own RCCL binding. No reference counterpart (single-GPU reference). */
int vr_rccl_available(void);
int vr_rccl_unique_id(void* out /* 128 bytes (ncclUniqueId) */);
int vr_rccl_comm_init(void** comm, int world, const void* unique_id, int rank);
int vr_rccl_comm_destroy(void* comm);
int vr_rdm_sharded_range(int64_t n, int64_t d, int world, int rank, int64_t* tile_begin, int64_t* tile_end);
size_t vr_rdm_sharded_workspace(int64_t n, int64_t d, int world);
int vr_rdm_pearson_sharded(const float* X_local, int64_t rows_local, int64_t n, int64_t d, int64_t ldx, float* rdm,
                           int64_t ldr, float correction, void* comm, int rank, int world, void* ws, size_t ws_bytes,
                           void* stream);

/* The collective behind the sharded entry points, as a table: all_gather(send, recv, bytes,
 * user, stream) must leave rank r's `bytes` of send at recv + r * bytes on every rank, ordered
 * on `stream`, and return 0 (non-zero fails the call with VR_EHIP). vr_comm_rccl fills the table
 * with RCCL's ncclAllGather over `nccl_comm` (what vr_rdm_pearson_sharded uses); a caller with
 * another transport (MPI, a host loopback in tests) fills it itself. */
typedef int (*vr_allgather_fn)(const void* send, void* recv, size_t bytes, void* user, void* stream);
typedef struct vr_comm {
  int world;
  int rank;
  vr_allgather_fn all_gather;
  void* user;
} vr_comm;
int vr_comm_rccl(vr_comm* out, void* nccl_comm, int world, int rank);
int vr_rdm_pearson_sharded_comm(const float* X_local, int64_t rows_local, int64_t n, int64_t d, int64_t ldx,
                                float* rdm, int64_t ldr, float correction, const vr_comm* comm, void* ws,
                                size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------
 * Image preprocessing: the eval loaders' get_transform (visreps/dataloaders/obj_cls.py:
 * 27-45) = torchvision Resize(resize, BILINEAR) on a PIL image (Pillow's ImagingResample:
 * antialiased separable bilinear, 22-bit fixed point, uint8 intermediate) ->
 * CenterCrop(crop) -> ToTensor -> Normalize(mean, std), bit-exact.
 * src [device] B x H x W x 3 uint8 (RGB, same size images); out [device] B x 3 x crop x
 * crop float32; mean, std [host] 3 floats each. crop must not exceed the resized image.
 * -------------------------------------------------------------------------- */
size_t vr_transform_workspace(int64_t B, int64_t H, int64_t W, int64_t resize, int64_t crop,
                              int filter);
/* filter: 0 = BILINEAR (get_transform), 1 = BICUBIC (the CLIP and timm DINOv3 loaders,
 * clip_representations.py:27, dino_representations.py:31-32) */
int vr_transform_u8(const uint8_t* src, int64_t B, int64_t H, int64_t W, int64_t resize,
                    int64_t crop, int filter, const float* mean, const float* std, float* out,
                    void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------
 * PCA covariance for the coarse-grained PCA labels: replaces
 * batched_pca's mean and covariance, scripts/coarsegrain/compute_eigenvectors.py:23-36
 *   mean = X.mean(axis=0);  cov = sum_b (X[b].astype(f64) - mean)^T (..) / (n - 1).
 * X [dev] fp32 row-major (n, p), leading dimension ldx >= p.
 * -------------------------------------------------------------------------- */
/* Column sums in numpy's float32 order (rows added in row order, one float32 running sum
 * per column), continued from init [dev] p (nullable: 0). sum [dev] p. Bit-identical to
 * numpy's X.sum(axis=0) on a C-order float32 array; chained over row shards it is the
 * same sum (the multi-GPU form passes the previous shard's sum as init). */
int vr_col_sum_f32(const float* X, int64_t n, int64_t p, int64_t ldx, const float* init,
                   float* sum, void* stream);
/* X.mean(axis=0) as numpy: the column sums / float32(n). mean [dev] p. */
int vr_col_mean_f32(const float* X, int64_t n, int64_t p, int64_t ldx, float* mean, void* stream);
/* mean [dev] p = sum [dev] p / float32(n) (may alias). */
int vr_mean_from_sum_f32(const float* sum, int64_t p, int64_t n, float* mean, void* stream);
/* cov [dev] fp64 (p, p), leading dimension ldc: sum over rows of
 * ((double)x - (double)mean)^T ((double)x - (double)mean) / denom, exactly symmetric, on
 * the fp64 MFMA. mean [dev] fp32 p. denom = n - 1 for the reference's covariance, 1 for a
 * rank's partial sum (multi-GPU: all-reduce, then divide). n = 0 (a rank with an empty
 * shard) is accepted: cov is all zeros, and vr_pca_cov_workspace(0, p) is the size of that
 * launch, as for every accepted (n, p). */
size_t vr_pca_cov_workspace(int64_t n, int64_t p);
int vr_pca_cov_f64(const float* X, int64_t n, int64_t p, int64_t ldx, const float* mean,
                   double denom, double* cov, int64_t ldc, void* ws, size_t ws_bytes,
                   void* stream);

/* Uncentred fp64 Grams of fp32 features on the same fp64 MFMA tiles (the encoding score's
 * ridge): replaces the fp64 X^T X / X X^T that himalaya 0.4.9's
 * RidgeCV(solver="svd") needs, called from visreps/analysis/encoding_score.py:47-62.
 * X [dev] fp32 row-major (n, p), leading dimension ldx >= p. rows = 0: G = X^T X (p x p,
 * the primal form, p < n); rows = 1: G = X X^T (n x n, the kernel form, p >= n). Products
 * of two fp32 values are exact in fp64, sums fp64. G [dev] fp64, leading dimension ldg,
 * exactly symmetric. Workspace: vr_gram64_workspace(n, p, rows). */
size_t vr_gram64_workspace(int64_t n, int64_t p, int rows);
int vr_gram64_f32(const float* X, int64_t n, int64_t p, int64_t ldx, int rows, double* G, int64_t ldg,
                  void* ws, size_t ws_bytes, void* stream);

/* Centred fp64 Grams about an fp64 mean (the eigenspectrum's covariance on its smaller side,
 * analysis/compute_eigenspectra.py): the tiles of vr_pca_cov_f64 / vr_gram64_f32 with
 * (double)x - mean formed while staging. vr_col_mean_f64: mean [dev] p doubles, the fp64 sum of
 * each column in row order / n (n >= 1; the column-sum kernels of csrc/knn.hip, no workspace).
 * vr_centred_gram64_f32: rows = 0: G = (X - mean)^T (X - mean) / denom (p x p); rows = 1:
 * G = (X - mean)(X - mean)^T / denom (n x n), the mean indexed along the contraction. mean [dev]
 * p doubles either way. G [dev] fp64, leading dimension ldg, exactly symmetric. n >= 1, p >= 1.
 * VR_EWORKSPACE below vr_centred_gram64_workspace(n, p, rows). */
int vr_col_mean_f64(const float* X, int64_t n, int64_t p, int64_t ldx, double* mean, void* stream);
size_t vr_centred_gram64_workspace(int64_t n, int64_t p, int rows);
int vr_centred_gram64_f32(const float* X, int64_t n, int64_t p, int64_t ldx, const double* mean,
                          int rows, double denom, double* G, int64_t ldg, void* ws,
                          size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------
 * Eigenvalues of a dense symmetric fp64 matrix, no vectors (csrc/eigvals.hip): unblocked
 * Householder tridiagonalisation, then Sturm-sequence bisection, one lane per eigenvalue.
 * Replaces the eigenvalue half of sklearn PCA(svd_solver="full") in
 * visreps/analysis/compute_eigenspectra.py:11-37 and np.linalg.eigvalsh in
 * experiments/representation_analysis/dimensionality/metrics.py:12-33.
 * A [dev] m x m, symmetric with both triangles filled, leading dimension lda >= m; its
 * contents are destroyed. w [dev] m doubles, ascending. m = 0 writes nothing; m = 1 and m = 2
 * skip the reduction. A non-finite entry anywhere in A gives all-NaN w. Backward stable:
 * |w - lambda| <= c m eps max|lambda|. Bit-identical run to run (fixed-order reductions, no
 * float atomics); no host synchronisation, every launch on the caller's stream; every loop's
 * trip count depends on m alone. VR_EINVAL for m < 0, m > 65536, lda < m or a null A or w;
 * VR_EWORKSPACE for ws_bytes below vr_eigvalsh_workspace(m) (O(m), non-decreasing in m).
 * -------------------------------------------------------------------------- */
size_t vr_eigvalsh_workspace(int64_t m);
int vr_eigvalsh_f64(double* A, int64_t m, int64_t lda, double* w, void* ws, size_t ws_bytes,
                    void* stream);

/* The k algebraically largest eigenpairs of the same kind of matrix, 0 <= k <= m <= 65536, on the
 * same solver (csrc/eigvals.hip); replaces the full torch.linalg.eigh of
 * analysis/reconstruct_from_pcs.py and scripts/coarsegrain/compute_eigenvectors.py where a few
 * leading vectors are kept. A as above, destroyed. w [dev] k doubles, descending: w[j] is bit for
 * bit vr_eigvalsh_f64's w[m - 1 - j]. V [dev] k x m row-major, leading dimension ldv >= m: row j
 * is the unit eigenvector of w[j], its largest-magnitude entry positive (the lowest index on a
 * tie); entries past column m of a row are not written.
 *   stage A  the tridiagonalisation of vr_eigvalsh_f64, each Householder vector stored back over
 *            the row it annihilated and its tau in the workspace
 *   stage B  bisection of the top k indices only
 *   stage C  a fixed number of inverse iterations on the tridiagonal, one lane per vector
 *            (partial pivoting, small pivots replaced, max-abs scaling); coincident eigenvalues
 *            separated by 4 eps span; after each iteration vectors whose eigenvalues chain
 *            within 1e-3 span are orthogonalised in order (modified Gram-Schmidt, two passes)
 *   stage D  V <- Q V, one workgroup per vector applying the m - 2 reflectors in turn
 * Residual ||A v - w v||_2 and orthogonality max|V V^T - I| are of order m eps ||A||_2 and m eps.
 * k = 0 or m = 0 writes nothing; m = 1 gives V = [[1]]. A non-finite entry of A gives NaN in all
 * of w and V; a zero matrix gives w = 0 exactly and k orthonormal vectors. Bit-identical run to
 * run; no host synchronisation; every loop's trip count depends on m and k alone. VR_EINVAL for
 * m < 0, m > 65536, k < 0, k > m, lda < m, ldv < m or a null A, w or V that would be used;
 * VR_EWORKSPACE for ws_bytes below vr_eigh_top_workspace(m, k) (O(m k), non-decreasing in both). */
size_t vr_eigh_top_workspace(int64_t m, int64_t k);
int vr_eigh_top_f64(double* A, int64_t m, int64_t lda, int64_t k, double* w, double* V, int64_t ldv,
                    void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------
 * PLS-SVD cross-decomposition (csrc/xcov.hip; analysis/cross_decomposition.py). Replaces, in
 * visreps/analysis/cross_decomposition.py, GaussianRandomProjection.fit_transform (30-34, 46),
 * the per-fold PLSSVD(..).fit / .transform of the shuffled KFold (49, 60-75) and the
 * per-component np.corrcoef / np.cov of the test scores (78-79). Every kernel runs on the fp64
 * MFMA or in fp64, adds in a fixed order (no float atomics: bit-identical run to run), launches
 * on the caller's stream and never synchronises with the host; trip counts depend on shapes and
 * segment lengths alone.
 * -------------------------------------------------------------------------- */
/* G[i, j] = sum_k ((double)A[a_rows[i], k] - a_mean[k]) * B[j, k]: both operands K-contiguous
 * (NT). A [dev] fp32 with leading dimension lda >= K; a_rows [dev] M int32 (nullable: row i);
 * a_mean [dev] K doubles (nullable: 0). B [dev] N x K, leading dimension ldb >= K, fp32
 * (b_f64 = 0) or fp64 (b_f64 = 1). G [dev] M x N, leading dimension ldg >= N, fp64 (g_f64 = 1)
 * or fp32 (g_f64 = 0: the fp64 sum rounded once). Products of two fp32 values are exact in
 * fp64. Split-K partials are added in slice order. Rows of A or B that are not 16-byte
 * aligned (pointer or leading dimension) take scalar loads. The projection Z = X R^T of
 * GaussianRandomProjection.transform is b_f64 = 0, g_f64 = 0 with R cast to fp32 (the cast
 * scikit-learn applies for float32 X). M = 0 or N = 0 writes nothing; K >= 1. VR_EINVAL for
 * a bad shape or a null pointer, VR_EWORKSPACE below vr_xgemm_nt_workspace(M, N, K). */
size_t vr_xgemm_nt_workspace(int64_t M, int64_t N, int64_t K);
int vr_xgemm_nt_f32(const float* A, int64_t M, int64_t K, int64_t lda, const int32_t* a_rows,
                    const double* a_mean, const void* B, int b_f64, int64_t N, int64_t ldb, void* G,
                    int g_f64, int64_t ldg, void* ws, size_t ws_bytes, void* stream);

/* Segmented cross-moments: the one pass over the data that every fold's training
 * cross-covariance follows from (cross_decomposition.py:62-72 reads 7/8 of the rows K times).
 * X [dev] fp32 (., p) ldx >= p and Y [dev] fp32 (., q) ldy >= q share their rows; rows [dev]
 * int32 (nullable: the identity) lists them in fold order, seg [host] F + 1 offsets into that
 * order with seg[0] = 0 (segment f = positions seg[f] .. seg[f + 1]); mean_x, mean_y [dev]
 * fp64 column means over all rows (vr_col_mean_f64). Writes
 *   S     [dev] F x p x q doubles, S[f] = sum over segment f of (x - mean_x)^T (y - mean_y)
 *   stats [dev] F x 2 x (p + q) doubles (nullable): [f][0] the column sums, [f][1] the sums of
 *         squares of the same centred values, X's columns then Y's.
 * An empty segment gives all zeros. 1 <= F <= 65535. VR_EWORKSPACE below
 * vr_xcov_segments_workspace(p, q, F, longest segment). */
size_t vr_xcov_segments_workspace(int64_t p, int64_t q, int64_t F, int64_t max_seg);
int vr_xcov_segments_f32(const float* X, int64_t ldx, const float* Y, int64_t ldy, int64_t p, int64_t q,
                         const int32_t* rows, const int64_t* seg, int64_t F, const double* mean_x,
                         const double* mean_y, double* S, double* stats, void* ws, size_t ws_bytes,
                         void* stream);

/* The standardised training cross-covariance of every fold from the segment moments (what
 * PLSSVD.fit forms as X_s^T Y_s after _center_scale_xy): with T = sum_f S[f], n_tr = n - n_f,
 * m and s the training mean (about the global mean) and ddof=1 standard deviation from stats
 * (s = 0 replaced by 1),  C[f] = (T - S[f] - n_tr m_x m_y^T) / (s_x s_y^T).  C [dev] F x p x q
 * doubles. Every fold must leave at least 2 training rows. */
size_t vr_fold_xcov_workspace(int64_t p, int64_t q);
int vr_fold_xcov_f64(const double* S, const double* stats, const int64_t* seg, int64_t F, int64_t p,
                     int64_t q, const double* mean_x, const double* mean_y, double* C, void* ws,
                     size_t ws_bytes, void* stream);

/* PLS-SVD of folds 0 .. n_run - 1 (n_run <= F): for each, C[f] as above is written as the
 * symmetric J = [[0, C], [C^T, 0]] of order p + q <= 65536, whose k largest eigenpairs
 * (vr_eigh_top_f64) are sigma_j and [u_j; v_j] / sqrt(2); each half is normalised in fp64, given
 * svd_flip's u-based sign (largest |u| entry positive, lowest index on a tie) and divided by the
 * training standard deviation; the fold's test rows are scored, (z - training mean) . u / s,
 * and each paired score column gives Pearson r and the ddof=1 covariance (two passes). Arguments
 * as vr_xcov_segments_f32, S and stats from it; 1 <= k <= min(p, q). Outputs, [dev]:
 *   corr, cov, sigma  n_run x k doubles;  null  n_run x k int32: 1 where
 *         sigma_j <= 64 (p + q) eps sigma_1 (a component past the rank of C, whose vectors
 *         LAPACK leaves arbitrary): its corr and cov are NaN
 *   imbalance (nullable) n_run x k doubles: |2 |u|^2 - 1| before normalisation
 *   weights (nullable) k x (p + q) doubles: fold wfold's unit u_j then unit v_j per row, with
 *         wmean and wstd (p + q doubles each) its training means and standard deviations.
 * A test fold of fewer than 2 rows gives NaN corr and cov; a non-finite input gives NaN
 * everywhere. VR_EINVAL if a fold leaves fewer than 2 training rows; VR_EWORKSPACE below
 * vr_plssvd_folds_workspace(p, q, k, longest test fold among those run). */
size_t vr_plssvd_folds_workspace(int64_t p, int64_t q, int64_t k, int64_t max_test);
int vr_plssvd_folds_f64(const float* X, int64_t ldx, const float* Y, int64_t ldy, int64_t p, int64_t q,
                        const int32_t* rows, const int64_t* seg, int64_t F, int64_t n_run,
                        const double* mean_x, const double* mean_y, const double* S, const double* stats,
                        int64_t k, double* corr, double* cov, double* sigma, int32_t* null,
                        double* imbalance, int64_t wfold, double* weights, double* wmean, double* wstd,
                        void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------
 * Batched one-sided (Hestenes) Jacobi SVD in fp64 (csrc/svd.hip): the dense solver of PLS-SVD's
 * solver="jacobi". Replaces the scipy.linalg.svd inside PLSSVD.fit
 * (visreps/analysis/cross_decomposition.py:66) for all folds in one call.
 * -------------------------------------------------------------------------- */
/* The thin SVD of `batch` matrices. A [dev] member b at A + b stride_a, p x q row-major with
 * leading dimension lda >= q; never written. With r = min(p, q), outputs [dev]:
 *   S      batch x r doubles, descending (equal values in the order of their rows)
 *   U      batch x r x p doubles, row j = the unit left vector u_j
 *   Vt     batch x r x q doubles, row j = the unit right vector v_j
 *   null   batch x r int32: 1 where sigma_j <= 64 (p + q) eps sigma_1; both vectors of such a
 *          component are NaN
 *   sweeps batch int32: sweeps the member ran, the last one (no rotation) included
 * Signs follow svd_flip's u-based rule: the largest |u_j| entry is positive, the lowest index on
 * a tie. Rotations work on the rows of B = A (p <= q) or A^T, in LDS, in blocks of 8 rows (4
 * above a long side of 1024, 2 above 2048); max(p, q) > 4096 is VR_EINVAL. One launch per step
 * of the block-pair schedule (vr_jacobi_schedule), and after every sweep the host reads the
 * members' done flags with one blocking copy on `stream`: the call synchronises with the host.
 * A member stops at its first sweep without a rotation; a member that still rotates in sweep 60
 * makes the call return VR_ENOCONV after writing the last iterate. A member with a non-finite
 * entry (or whose squared norms overflow) runs no sweep: NaN in S, U and Vt, null = 1,
 * sweeps = 0; the others are unaffected. No floating-point atomics: a member's result is
 * bit-identical run to run and does not depend on the batch it is solved in. sigma is accurate
 * to order (p + q) eps sigma_1, U U^T and Vt Vt^T to order (p + q) eps over the non-null
 * components, whatever the spacing of the singular values. batch = 0 writes nothing; batch <=
 * 65535. VR_EWORKSPACE below vr_svd_jacobi_workspace(batch, p, q). */
size_t vr_svd_jacobi_workspace(int64_t batch, int64_t p, int64_t q);
int vr_svd_jacobi_f64(const double* A, int64_t batch, int64_t p, int64_t q, int64_t lda, int64_t stride_a,
                      double* S, double* U, double* Vt, int32_t* null, int32_t* sweeps, void* ws,
                      size_t ws_bytes, void* stream);
/* Host. The block-pair schedule of one sweep over nb >= 1 blocks: a round-robin tournament
 * (circle method) over nb_even = nb + (nb odd) blocks. pairs [host]
 * (nb_even - 1) x (nb_even / 2) x 2 int32: step s, pair i = the two block ids, lower first; the
 * second is -1 where the block meets the padding block (a bye: nb odd only). Every step's pairs
 * are disjoint and every unordered pair of blocks occurs in exactly one step. */
int vr_jacobi_schedule(int64_t nb, int32_t* pairs);

/* vr_plssvd_folds_f64 on the Jacobi solver: the same arguments and outputs, with every run
 * fold's C formed at once (the arithmetic of vr_fold_xcov_f64), one batched vr_svd_jacobi_f64
 * over the n_run folds, then per fold the first k components divided by the training standard
 * deviation and scored as there. Differences: sigma and null come from the Jacobi solve; u and v
 * are unit vectors on their own, so imbalance (where requested) is written as 0.0; the call
 * synchronises with the host (vr_svd_jacobi_f64) and returns VR_ENOCONV where that does.
 * max(p, q) <= 4096. VR_EWORKSPACE below vr_plssvd_folds_svd_workspace(p, q, k, longest test
 * fold among those run, n_run). */
size_t vr_plssvd_folds_svd_workspace(int64_t p, int64_t q, int64_t k, int64_t max_test, int64_t n_run);
int vr_plssvd_folds_svd_f64(const float* X, int64_t ldx, const float* Y, int64_t ldy, int64_t p, int64_t q,
                            const int32_t* rows, const int64_t* seg, int64_t F, int64_t n_run,
                            const double* mean_x, const double* mean_y, const double* S, const double* stats,
                            int64_t k, double* corr, double* cov, double* sigma, int32_t* null,
                            double* imbalance, int64_t wfold, double* weights, double* wmean, double* wstd,
                            void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------
 * Label-conditioned statistics (csrc/class_stats.hip): the per-class, per-feature sums behind the
 * Fisher ratio, class selectivity and centroid analyses, and two per-row reductions.
 * Replaces the per-batch host copy + np.add.at of class_selectivity_index.py:130-173 and the
 * boolean-mask loops of task_brain_alignment.py:126-195 and variance_ratio.py:31-42.
 * -------------------------------------------------------------------------- */
/* Per-class moments of X [dev] (n, d) fp32 row-major, ldx >= d, under labels [dev] int32 (n):
 * sum[c][j] = sum over the rows i of class c of (x_ij - centre[c][j]), sumsq[c][j] the same of
 * the squares; the subtraction and the product in fp64 (the square enters by one fused
 * multiply-add). centre [dev] (C, d) doubles, null = 0;
 * counts [dev] int64 (C); sum [dev] (C, d) doubles; sumsq the same, nullable; skipped [dev] one
 * int64: rows whose label is outside [0, C), which are counted there and never read.
 * Summation order (the contract): a class's rows in ascending row index, cut into chunks of
 * R = vr_class_moments_chunk_rows() rows, added one after the other inside a chunk, chunk
 * partials added in ascending order. The result is a function of X and of each class's own row
 * order alone: bit-identical run to run, no floating-point atomics. accumulate = 0 overwrites
 * every output (an empty class gets 0); accumulate = 1 adds this call's totals onto counts, sum,
 * sumsq and skipped, one fp64 add per entry of a class that has rows. n = 0 writes zeros (nothing
 * when accumulating). A NaN or inf entry reaches its own (class, column) entries only.
 * VR_EINVAL for n < 0, n > 2^31 - 1, d < 1, d > 2^21, C < 1, ldx < d or a null pointer;
 * VR_EWORKSPACE for ws_bytes below vr_class_moments_workspace(n, d, C): the pairs sort plus
 * (n / R + min(C, n)) d chunk partials of 16 bytes, non-decreasing in n, d and C (0 for a bad
 * shape). No host synchronisation. */
int64_t vr_class_moments_chunk_rows(void);
size_t vr_class_moments_workspace(int64_t n, int64_t d, int64_t C);
int vr_class_moments_f32(const float* X, int64_t n, int64_t d, int64_t ldx, const int32_t* labels,
                         int64_t C, const double* centre, int64_t* counts, double* sum, double* sumsq,
                         int64_t* skipped, int accumulate, void* ws, size_t ws_bytes, void* stream);
/* dist [dev] n doubles: dist[i] = || x_i - centre[labels[i]] ||_2 in fp64, NaN for a label outside
 * [0, C). One wave per row: lane l adds the 4-column groups l, l + 64, ... in ascending order, the
 * 64 partials meet in a fixed tree; the bits do not depend on ldx or alignment. centre non-null. */
int vr_class_dist_f32(const float* X, int64_t n, int64_t d, int64_t ldx, const int32_t* labels,
                      int64_t C, const double* centre, double* dist, void* stream);
/* Per row of X: l1 [dev] n doubles = sum |x|, l2 = sqrt(sum x^2), both in fp64 in the order of
 * vr_class_dist_f32; active [dev] n int64 = #{j: |x_ij| > threshold} (a NaN entry is not counted). */
int vr_row_sparsity_f32(const float* X, int64_t n, int64_t d, int64_t ldx, float threshold, double* l1,
                        double* l2, int64_t* active, void* stream);

/* ------------------------------------------------------------------------------
 * Host: legacy numpy RandomState (MT19937) index streams, bit-exact.
 * Replaces np.random.RandomState(seed) + .choice(n, k, replace=False) / .permutation(n)
 * (evals.py:260-261,356,362-364; rsa.py:169,176,248-250; evals.py:111-113).
 * -------------------------------------------------------------------------- */
/* Opaque generator state (caller-allocated, vr_rng_state_bytes() bytes). */
size_t vr_rng_state_bytes(void);
int vr_rng_seed(void* state, uint32_t seed);                /* RandomState(seed) */
int vr_rng_permutation(void* state, int64_t n, int32_t* out); /* .permutation(n) */
int vr_rng_choice(void* state, int64_t n, int64_t k, int32_t* out); /* .choice(n,k,replace=False) */
int vr_rng_random_u32(void* state, int64_t count, uint32_t* out);   /* raw MT19937 draws */
/* .normal(loc, scale, count), bit for bit (legacy_gauss: the polar method on pairs of 53-bit
 * doubles ((a >> 5) 2^26 + (b >> 6)) / 2^53, x = 2 u - 1, r2 >= 1 or r2 == 0 rejected,
 * f = sqrt(-2 log(r2) / r2); a call returns f x2 and the state keeps f x1 for the next, cleared
 * by vr_rng_seed; the value is loc + scale g). The stream behind scikit-learn's
 * _gaussian_random_matrix (GaussianRandomProjection, cross_decomposition.py:30-31). out [host]. */
int vr_rng_normal_f64(void* state, int64_t count, double loc, double scale, double* out);
/* Convenience: fresh RandomState(seed), then n_draws successive choice(n, k) calls
 * into out (n_draws, k) [host]. */
int vr_legacy_choice(uint32_t seed, int64_t n, int64_t k, int64_t n_draws, int32_t* out);

/* numpy.percentile(x, q) with the default 'linear' method (evals.py:371-372),
 * NaN-propagating. x [host] double (n). Returns the percentile (NaN if n == 0). */
double vr_percentile_linear(const double* x, int64_t n, double q);

#ifdef __cplusplus
}
#endif

#endif /* VISREPS_HIP_H */
