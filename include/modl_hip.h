/*
 * modl_hip.h — C-ABI of libmodl_hip.so, the MI355X (gfx950) implementation of
 * MODL's per-minibatch SOMF hot path.
 *
 * This library takes the place of the reference's Cython extensions
 *   modl/decomposition/dict_fact_fast.pyx, modl/utils/math/enet.pyx,
 *   modl/utils/randomkit/{random_fast,sampler}.pyx (+ randomkit.c, distributions.c),
 *   modl/decomposition/recsys_fast.pyx
 * and of the numpy/BLAS calls of modl/decomposition/dict_fact.py:495-715.
 * Each entry point cites the reference interface it replaces (paths relative to
 * the reference repository).
 *
 * Conventions
 *  - every function returns int: 0 = ok, < 0 = MODL_E* (bad argument / state),
 *    > 0 = hipError_t of a failed HIP call.  No exceptions cross the ABI.
 *  - `_f32` / `_f64` suffixes mirror Cython's fused `floating` type.
 *  - pointers named d_* are DEVICE pointers (hipMalloc'd or torch CUDA tensors),
 *    h_* are HOST pointers.  `stream` is a hipStream_t passed as void*
 *    (NULL = default stream).  Calls are asynchronous w.r.t. the host unless
 *    stated otherwise; the caller owns all buffers.
 *  - matrices are row-major (C order), leading dimension = number of columns
 *    unless an explicit ld is given.
 *  - the dictionary and the surrogate statistic B are held FEATURE-MAJOR on the
 *    device: d_Dt[p][k] = components_.T, d_Bt[p][k] = B_.T, so that a sampled
 *    feature is one contiguous k-vector (coalesced gather of subsampled columns).
 */
#ifndef MODL_HIP_H
#define MODL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MODL_ABI_VERSION 5

/* The largest dictionary (n_components, k) any entry point takes.  Up to 1024 atoms the tuned solvers keep a sample's
 * coefficients in registers; 1024 < k <= 4096 runs the wide route (csrc/cd_wide.hip: the solver's four k-vectors in
 * LDS, 128 KiB in f64 at 4096; csrc/bcd.hip: dict_update_wide).  A larger k is MODL_EINVAL. */
#define MODL_MAX_COMPONENTS 4096

#define MODL_OK 0
#define MODL_EINVAL (-1)   /* bad argument */
#define MODL_ENOMEM (-2)   /* workspace too small / allocation failed */
#define MODL_ESTATE (-3)   /* object used in the wrong state */
#define MODL_ENOGPU (-4)   /* no HIP device available, or not a gfx950-class part (160 KiB of LDS per compute unit) */
#define MODL_ENORCCL (-5)  /* librccl.so could not be loaded (modl_comm_*) */
#define MODL_ERCCL (-6)    /* an RCCL call failed */
#define MODL_ETIMEOUT (-7) /* a persistent dictionary-update launch gave up half-way (the update is incomplete): modl_somf_status */

#define MODL_F32 0
#define MODL_F64 1

#define MODL_AGG_MASKED 0
#define MODL_AGG_FULL 1
#define MODL_AGG_AVERAGE 2

#define MODL_OPT_VARIATIONAL 0
#define MODL_OPT_SGD 1

/* modl_somf_desc.flags (diagnostics; 0 in production) */
#define MODL_FLAG_NO_RIDER 1      /* the B_ update of the rows that were not sampled runs as its own launch */
#define MODL_FLAG_GEMM_STAMPS 2   /* the head statistics product leaves shader-clock stamps (modl_somf_debug_gemm_stamps) */

int modl_abi_version(void);
/* MODL_MAX_COMPONENTS, for callers that do not read this header */
int modl_max_components(void);
/* number of visible HIP devices (0 without a GPU); never fails */
int modl_device_count(void);
const char *modl_error_string(int code);
/* process-wide diagnostics switches (the test-suite forces code paths with them; nothing reads the environment; every
 * switch of the product library selects between CORRECT code paths).
 * MODL_DEBUG_CD_SPARSE_PCT: value >= 0 = share of active coordinates (percent) below which a sweep of the one-wavefront
 * coordinate-descent kernel runs as an active-set sweep (0: always dense, 100: always sparse), -1 = the default rule.
 * MODL_DEBUG_CD_SPLIT: 1 (default) = shared-Gram solves with 32 <= k <= 1024 run the four-wavefront solver
 * (cd_split_impl.hpp), 0 = the one-wavefront solver (cd_solver.hip: the reference's operation order; the two agree to
 * rounding, the tests compare them).  Its variants for k > 256 spill registers and are only built into the
 * diagnostics library (libmodl_hip_diag.so, -DMODL_DIAG): the product library keeps the four-wavefront solver there.
 * MODL_DEBUG_CD_STAMPS / MODL_DEBUG_ATOM_STAMPS (shader-clock stamps written to a caller-supplied device buffer) exist
 * in the diagnostics library only: the product library answers MODL_EINVAL. */
#define MODL_DEBUG_CD_SPARSE_PCT 1
#define MODL_DEBUG_CD_SPLIT 2
#define MODL_DEBUG_CD_STAMPS 3        /* (diagnostics library) value = device pointer to 1024 uint64 (0: off): shader-clock stamps of sample 0 of the four-wavefront solver */
#define MODL_DEBUG_BCD_ACC 5          /* 1 (default): the blocked dictionary update sums its Gram contributions with integer atomics into one fixed-point record; 0: one record per workgroup, summed by every workgroup of the next launch */
#define MODL_DEBUG_ATOM_STAMPS 6      /* (diagnostics library) value = device pointer to 64 uint64, zeroed by the caller (0: off): cycle sums of the projecting workgroup of the grouped atom update (bcd.hip: atom_project_group_kernel) */
#define MODL_DEBUG_BCD_TINY 7         /* 1 (default): the f64 blocked dictionary update of at most 192 sampled features runs as ONE one-workgroup launch; 0: five launches per block of 32 atoms */
#define MODL_DEBUG_STAGE_AHEAD 8      /* 1 (default): inside modl_somf_partial_fit_chunk the next minibatch's parameters are copied to HBM by a workgroup of the dictionary update's last launch; 0: a staging launch at the head of every step */
#define MODL_DEBUG_BCD_PERSIST 9      /* 1 (default): the f32 blocked dictionary update runs as ONE persistent launch (a resolver workgroup + one workgroup per 32 / 64 sampled rows resident in LDS, look-ahead Gram matrices: csrc/bcd_persist.hip) whenever its workgroups fit the chip (hipOccupancyMaxActiveBlocksPerMultiprocessor for the kernel's own footprint); 0: one launch per block of 32 atoms.  Diagnostics library only (the product library treats them as 1): 3 = the resolver waits for a workgroup that never comes before the first block (the launch cannot run: the resolver completes the update alone, modl_somf_persist_recoveries counts it), 4 = the same from the second block on (the update is incomplete: MODL_ETIMEOUT) */
#define MODL_DEBUG_STATS_RESIDENT 10  /* 1 (default): the f32 statistics product X^T code over at least 4096 features and at most 256 atoms runs on persistent workgroups that keep the code matrix in registers (csrc/gemm_resident.hpp, tiles of 16 features); 0: the 32 x 32 tiles or the k-wide tiles of rounds 2-4 */
#define MODL_DEBUG_RECSYS_FUSED 11    /* 1 (default): a masked minibatch of RecsysDictFact with at most 64 (f64: 56) atoms and 64 rows runs its codes (rating chunks of 128, ticketed fixed-order sums, Cholesky) and C_ as ONE launch (csrc/recsys.hip: recsys_fused_kernel), B_ and the blocked dictionary update as launches of their own behind it; 0: the separate launches of rounds 2-5 for everything.  Any other value is rejected (MODL_EINVAL) */
#define MODL_DEBUG_ATOM_MWG 12        /* the l1 projection of an atom with more than 6144 and at most 16 384 sampled features (one launch per atom: the reference's HCP configuration).  1 (default): by the launch's last workgroup with the vector in registers, 40 or 64 elements per thread (csrc/bcd.hip: atom_project_regs; needs MODL_DEBUG_ATOM_PIPE != 0, else as 3); 3: spread over the launch's workgroups - an element or two per thread, a memory round trip per Michelot pass (mwg_l1_project: measured slower, kept selectable and tested); 0: the last workgroup projects from an LDS copy; diagnostics library: 2 = as 3 with a workgroup that withholds its sums (the attempt gives up and the last workgroup projects: the fallback path) */
#define MODL_DEBUG_BCD_FEW 13         /* 1 (default): the f64 blocked dictionary update of 193 to 2048 sampled features runs as ONE launch on up to sixteen workgroups of 128 features that exchange a block's Gram record through memory (csrc/bcd.hip: bcd_few_kernel); 0: four launches per block of 32 atoms */
#define MODL_DEBUG_ATOM_PIPE 14       /* 1 (default): in the per-atom sweep of MODL_DEBUG_ATOM_MWG the gradient rows of the NEXT group of four atoms are formed by workgroups riding on the launches of this group's atoms (against the dictionary as it is then; what this group changes is subtracted afterwards from its compact rows - csrc/bcd.hip: atom_corr_project_kernel, GradRide); 0: a gradient launch of its own between two groups */
int modl_debug_set(int what, int64_t value);
/* 1 in libmodl_hip_diag.so (built with -DMODL_DIAG: the same sources plus the A/B-only kernel variants and the stamp
 * switches), 0 in the product library */
int modl_is_diag_build(void);

/* ------------------------------------------------------------------------- *
 * Host-side RNG — replaces modl/utils/randomkit/random_fast.pyx (RandomState,
 * :49-150) over randomkit.c / distributions.c.  Streams are bit-identical to
 * the reference for the same seed.  Pure host code: usable without a GPU.
 * ------------------------------------------------------------------------- */
typedef struct modl_rk modl_rk;
int modl_rk_create(uint64_t seed, modl_rk **out);            /* RandomState(seed), rk_seed randomkit.c:138 */
void modl_rk_destroy(modl_rk *rk);
int modl_rk_seed(modl_rk *rk, uint64_t seed);                 /* random_fast.pyx:64 */
int modl_rk_random(modl_rk *rk, uint32_t *out);               /* rk_random, randomkit.c:212 */
int modl_rk_randint(modl_rk *rk, uint64_t high, int64_t *out);/* random_fast.pyx:76 -> rk_interval :260 */
int modl_rk_double(modl_rk *rk, double *out);                 /* rk_double, randomkit.c:292 */
int modl_rk_binomial(modl_rk *rk, int64_t n, double p, int64_t *out); /* random_fast.pyx:146 -> distributions.c:442 */
int modl_rk_permutation(modl_rk *rk, int64_t n, int64_t *h_out);      /* random_fast.pyx:79 */
/* raw MT19937 state (key[624], pos), the layout of numpy's legacy RandomState.get_state()[1:3]: a modl_rk loaded with
 * numpy's state continues numpy's stream (legacy permutation(n) == modl_rk_permutation: dict_fact.py:672) */
int modl_rk_get_mt_state(const modl_rk *rk, uint32_t *h_key624, int32_t *pos);
int modl_rk_set_mt_state(modl_rk *rk, const uint32_t *h_key624, int32_t pos);
int modl_rk_shuffle_i64(modl_rk *rk, int64_t *h_x, int64_t n);        /* random_fast.pyx:87 (1-D) */
/* random_fast.pyx:127: draws one swap sequence; h_trace[n] receives the
 * permutation, h_swaps[n] the swap targets to replay on other arrays. */
int modl_rk_shuffle_trace(modl_rk *rk, int64_t n, int64_t *h_trace, int64_t *h_swaps);
/* replays a swap sequence on the rows of a host array (random_fast.pyx:105-119); a target outside 0..i is refused with
 * MODL_EINVAL before any row moves (the device version too, which also wants row_bytes % 4 == 0) */
int modl_apply_swaps_rows(void *h_base, int64_t n, size_t row_bytes, const int64_t *h_swaps);
/* same on a DEVICE array (epoch shuffle of code_ / averages, dict_fact.py:359-379) */
int modl_apply_swaps_rows_device(void *d_base, int64_t n, size_t row_bytes, const int64_t *h_swaps,
                                 void *stream);

/* Feature sampler — replaces modl/utils/randomkit/sampler.pyx:9-70 */
typedef struct modl_sampler modl_sampler;
int modl_sampler_create(int64_t range, int rand_size, int replacement, uint64_t seed, modl_sampler **out);
void modl_sampler_destroy(modl_sampler *s);
/* yield_subset(reduction), sampler.pyx:41.  h_out must hold `range` entries;
 * *n_out receives the subset length.  Indices are unsorted, as in the reference. */
int modl_sampler_yield_subset(modl_sampler *s, double reduction, int64_t *h_out, int64_t *n_out);
/* public attributes of the reference class (sampler.pxd:4-14) */
int modl_sampler_get(modl_sampler *s, int64_t *range, int64_t *lim_inf, int64_t *lim_sup, int64_t *h_box);
/* full state save / restore (box, limits, MT key + position, binomial cache) */
size_t modl_sampler_state_bytes(const modl_sampler *s);
int modl_sampler_get_state(const modl_sampler *s, void *h_buf, size_t bytes);
int modl_sampler_set_state(modl_sampler *s, const void *h_buf, size_t bytes);

/* _batch_weight, dict_fact_fast.pyx:115-122 */
int modl_batch_weight(int64_t count, int64_t batch_size, double learning_rate, double offset, double *out);

/* ------------------------------------------------------------------------- *
 * Fine-grained device entry points, 1:1 with the Cython functions
 * (used by the parity tests and by transform()).
 * ------------------------------------------------------------------------- */

/* _enet_regression_single_gram, dict_fact_fast.pyx:125-215.
 * d_G[k][k], d_Dx[b][k] (overwritten by the solution when l1_ratio == 0, as in
 * the reference), d_X[b][ldx] (only the squared row norms are used, :334),
 * d_code[n][k] (rows d_indices[ii] are warm starts and results), d_indices[b]
 * int64 (NULL = 0..b-1).  d_sweeps (optional, int32[b]) receives the number of
 * coordinate-descent sweeps per sample.  d_ws / ws_bytes: scratch, see
 * modl_enet_regression_workspace().  1 <= k <= MODL_MAX_COMPONENTS. */
size_t modl_enet_regression_workspace(int dtype, int64_t b, int64_t k, int multi_gram);
int modl_enet_regression_single_gram_f32(const float *d_G, float *d_Dx, const float *d_X, int64_t ldx,
                                         int64_t p, float *d_code, const int64_t *d_indices, int64_t b,
                                         int64_t k, float l1_ratio, float alpha, int positive, float tol,
                                         int max_iter, int32_t *d_sweeps, void *d_ws, size_t ws_bytes,
                                         void *stream);
int modl_enet_regression_single_gram_f64(const double *d_G, double *d_Dx, const double *d_X, int64_t ldx,
                                         int64_t p, double *d_code, const int64_t *d_indices, int64_t b,
                                         int64_t k, double l1_ratio, double alpha, int positive, double tol,
                                         int max_iter, int32_t *d_sweeps, void *d_ws, size_t ws_bytes,
                                         void *stream);
/* _enet_regression_multi_gram, dict_fact_fast.pyx:33-113: d_G[b][k][k] */
int modl_enet_regression_multi_gram_f32(const float *d_G, float *d_Dx, const float *d_X, int64_t ldx,
                                        int64_t p, float *d_code, const int64_t *d_indices, int64_t b,
                                        int64_t k, float l1_ratio, float alpha, int positive, float tol,
                                        int max_iter, int32_t *d_sweeps, void *d_ws, size_t ws_bytes,
                                        void *stream);
int modl_enet_regression_multi_gram_f64(const double *d_G, double *d_Dx, const double *d_X, int64_t ldx,
                                        int64_t p, double *d_code, const int64_t *d_indices, int64_t b,
                                        int64_t k, double l1_ratio, double alpha, int positive, double tol,
                                        int max_iter, int32_t *d_sweeps, void *d_ws, size_t ws_bytes,
                                        void *stream);
/* _update_G_average, dict_fact_fast.pyx:217-228: d_G_average[b][k][k] in place */
int modl_update_G_average_f32(float *d_G_average, const float *d_G, const float *d_w_sample, int64_t b,
                              int64_t k, void *stream);
int modl_update_G_average_f64(double *d_G_average, const double *d_G, const double *d_w_sample, int64_t b,
                              int64_t k, void *stream);

/* enet_norm / enet_projection / enet_scale, modl/utils/math/enet.pyx:125,38,150,
 * batched over `rows` vectors of length n laid out with element stride `inc`
 * and vector stride `ld` (so atoms can be rows of D or columns of Dt).
 * d_radius[rows] (projection; scale takes one radius for every row), d_out_norm[rows] (norm).
 * inc < 1 is refused with MODL_EINVAL.  The projection's d_out may be d_v.  A row whose enet norm is not finite (a
 * NaN or an infinity among its entries) comes out NaN throughout from the projection and the scale, and as that norm
 * (NaN or +inf) from the norm; no other row is touched. */
int modl_enet_norm_f32(const float *d_v, int64_t rows, int64_t n, int64_t ld, int64_t inc, float l1_ratio,
                       float *d_out_norm, void *stream);
int modl_enet_norm_f64(const double *d_v, int64_t rows, int64_t n, int64_t ld, int64_t inc, double l1_ratio,
                       double *d_out_norm, void *stream);
int modl_enet_projection_f32(const float *d_v, float *d_out, int64_t rows, int64_t n, int64_t ld, int64_t inc,
                             const float *d_radius, float l1_ratio, void *stream);
int modl_enet_projection_f64(const double *d_v, double *d_out, int64_t rows, int64_t n, int64_t ld,
                             int64_t inc, const double *d_radius, double l1_ratio, void *stream);
int modl_enet_scale_f32(float *d_v, int64_t rows, int64_t n, int64_t ld, int64_t inc, float l1_ratio,
                        float radius, void *stream);
int modl_enet_scale_f64(double *d_v, int64_t rows, int64_t n, int64_t ld, int64_t inc, double l1_ratio,
                        double radius, void *stream);

/* _predict, recsys_fast.pyx:10-38: d_data[nnz] = (P Q) at the CSR pattern;
 * P[n_rows][k], Q[k][n_cols] (f64, int32 CSR as in the reference). */
int modl_predict_csr(double *d_data, const int32_t *d_indices, const int32_t *d_indptr, const double *d_P,
                     int64_t n_rows, int64_t k, const double *d_Q, int64_t n_cols, void *stream);

/* ------------------------------------------------------------------------- *
 * Masked (missing-data) path — RecsysDictFact, modl/decomposition/recsys.py.
 * CSR pieces are int32 as in the reference (recsys_fast.pyx:11-13).
 * ------------------------------------------------------------------------- */
/* Ridge codes on the observed columns of b CSR rows (recsys.py:168-181 and _refit :254-265):
 * code = (D_S D_S^T + alpha |S| / p I)^-1 D_S x_S.  d_row_ids[b] selects rows of the CSR matrix
 * (NULL = rows 0..b-1), d_code_rows[b] the destination rows of d_code (NULL = the CSR row id).
 * Rows without entries keep their code.
 * k is NOT bounded by MODL_MAX_COMPONENTS here: a row's k x k system, its right-hand side and 32 staged dictionary rows share
 * the 160 KiB of LDS of one workgroup.  f32: 1 <= k <= 186 (k <= 64 and k <= 128 factor with one / two rows of the system per
 * lane, 129 .. 186 with the whole workgroup); f64: 1 <= k <= 127 (k <= 64, k <= 121, 122 .. 127 likewise).  A larger k is
 * MODL_EINVAL and nothing is written.  The same limits hold for modl_recsys_minibatch_* and modl_recsys_fit_batches_*, whose
 * minibatches of more than 64 (f64: 56) atoms, more than 64 rows or more than 64 chunks of 128 ratings solve their codes here.
 * Those two do NOT refuse a larger k up front: modl_recsys_plan_create takes any k, and the minibatch answers MODL_EINVAL only
 * when it reaches the code solve, after it has taken a staging slot of the plan and enqueued the staging copy (no state array
 * is written; the plan counts the call as a split one).  Callers check k against these limits themselves, as
 * RecsysDictFact.fit does. */
int modl_recsys_codes_f32(const float *d_Dt, int64_t p, int k, const int32_t *d_indptr, const int32_t *d_indices,
                          const float *d_data, const int64_t *d_row_ids, const int64_t *d_code_rows, int64_t b,
                          double alpha, float *d_code, void *stream);
int modl_recsys_codes_f64(const double *d_Dt, int64_t p, int k, const int32_t *d_indptr, const int32_t *d_indices,
                          const double *d_data, const int64_t *d_row_ids, const int64_t *d_code_rows, int64_t b,
                          double alpha, double *d_code, void *stream);
/* Per-feature weighted B_ update of one minibatch (recsys.py:175,182-185).  d_subset[u]: the features
 * touched by the batch; d_fptr[u+1] / d_entry_sample / d_entry_val: for each of them its entries IN
 * BATCH ORDER (position of the row in the batch, rating); d_code_b[b][k]: the batch's codes;
 * w_times_n_iter = w * n_iter_.  Updates d_feature_n_iter (int64[p]) too. */
int modl_recsys_update_B_f32(float *d_Bt, int k, int64_t *d_feature_n_iter, const int32_t *d_subset,
                             const int32_t *d_fptr, const int32_t *d_entry_sample, const float *d_entry_val,
                             const float *d_code_b, double w_times_n_iter, int64_t u, void *stream);
int modl_recsys_update_B_f64(double *d_Bt, int k, int64_t *d_feature_n_iter, const int32_t *d_subset,
                             const int32_t *d_fptr, const int32_t *d_entry_sample, const double *d_entry_val,
                             const double *d_code_b, double w_times_n_iter, int64_t u, void *stream);
/* _predict (recsys_fast.pyx:10-38) against the feature-major dictionary: d_out[nnz] (double) */
int modl_recsys_predict_f32(double *d_out, const int32_t *d_indices, const int32_t *d_indptr, const float *d_code,
                            int64_t n_rows, int k, const float *d_Dt, void *stream);
int modl_recsys_predict_f64(double *d_out, const int32_t *d_indices, const int32_t *d_indptr, const double *d_code,
                            int64_t n_rows, int k, const double *d_Dt, void *stream);
/* Recommendation: the n_top best items of b queries, without ever writing the b x p scores (csrc/recsys_topn.hip).
 *   score[ii][f] = sum_c code[c] Dt[f][c] (+ d_item_bias[f]) over every item f of 0 .. p-1 that is not excluded for query ii;
 *   d_items[ii * n_top + j] = the item with the j-th largest score, d_scores[...] that score: descending, equal scores by
 *   ascending item id.  The result is a function of the inputs alone (run-to-run identical, whatever the number of slabs the
 *   items are cut into).  Fewer than n_top items left: the tail is item -1 with score -inf.  Inputs are assumed finite.
 * Query ii: its code is row d_code_rows[ii] of d_code[.][k] (NULL: row ii); its excluded items are the entries of row
 * d_ex_rows[ii] (NULL: row ii) of the CSR pattern d_ex_indptr / d_ex_indices, whose column indices may be unsorted and may
 * repeat; d_ex_indptr NULL: nothing is excluded.  d_Dt[p][k]: the feature-major dictionary.  d_item_bias: double[p] or NULL
 * (f32: the sum is formed in double and rounded once).
 * MODL_EINVAL before any device work: a NULL d_code / d_Dt / d_items / d_scores (or d_ex_indices with d_ex_indptr given),
 * b < 0, p < 1 or p >= 2^31, n_top outside 1 .. MODL_RECSYS_MAX_TOPN, k < 1 or k beyond the limit of modl_recsys_codes_* (f32
 * 186, f64 127).  b == 0 does nothing.  d_ws NULL or smaller than modl_recsys_topn_workspace(...): MODL_ENOMEM; no device:
 * MODL_ENOGPU.  The workspace holds a bitmask of p bits per query and, for calls with few queries (the items are then cut into
 * slabs over workgroups), one list per query and slab.  Asynchronous on `stream`. */
#define MODL_RECSYS_MAX_TOPN 128
/* bytes of d_ws for a call with these arguments; 0 for arguments the call refuses (and for b == 0) */
size_t modl_recsys_topn_workspace(int dtype, int64_t p, int k, int64_t b, int n_top);
int modl_recsys_topn_f32(const float *d_code, const int64_t *d_code_rows, int64_t b, int k, const float *d_Dt, int64_t p,
                         const int32_t *d_ex_indptr, const int32_t *d_ex_indices, const int64_t *d_ex_rows,
                         const double *d_item_bias, int n_top, int32_t *d_items, float *d_scores, void *d_ws,
                         size_t ws_bytes, void *stream);
int modl_recsys_topn_f64(const double *d_code, const int64_t *d_code_rows, int64_t b, int k, const double *d_Dt, int64_t p,
                         const int32_t *d_ex_indptr, const int32_t *d_ex_indices, const int64_t *d_ex_rows,
                         const double *d_item_bias, int n_top, int32_t *d_items, double *d_scores, void *d_ws,
                         size_t ws_bytes, void *stream);
/* Ranks of held-out items: where given items stand among the items a query has not excluded, without ever writing the b x p
 * scores (csrc/recsys_rank.hip).  Queries, exclusions, d_Dt and d_item_bias are those of modl_recsys_topn_*, and score[ii][f]
 * is that call's score bit for bit.  The targets of query ii are the entries d_t_indptr[ii] .. d_t_indptr[ii + 1] - 1 of
 * d_t_indices (d_t_indptr: int32[b + 1]); t_max is the caller's promise of the longest target row.
 *   d_ranks[e], for entry e of query ii with item t = d_t_indices[e]: the number of items c != t of 0 .. p-1 that are not
 *   excluded for ii and beat t: a higher score, or an equal score and a smaller id.  With t not excluded that is the
 *   position of t in the query's top-N list.  Whether t itself is excluded plays no part; the other targets of the query are
 *   ordinary candidates; a repeated target gets its rank at every occurrence.  t outside 0 .. p-1: -1.  Entries of a row
 *   beyond its first t_max: -2 (they are not otherwise read).  d_ranks is indexed as d_t_indices is.
 *   d_n_candidates[ii] (int32[b], may be NULL): p minus the number of distinct in-range excluded items of query ii.
 * The result is a function of the inputs alone (counts are summed as integers: no order enters).
 * MODL_EINVAL before any device work: a NULL d_code / d_Dt / d_t_indptr / d_t_indices / d_ranks (or d_ex_indices with
 * d_ex_indptr given), b < 0, p < 1 or p >= 2^31, t_max outside 1 .. MODL_RECSYS_MAX_RANK_TARGETS, k as for the top-N call.
 * b == 0 does nothing.  d_ws NULL or smaller than modl_recsys_ranks_workspace(...): MODL_ENOMEM; no device: MODL_ENOGPU.
 * Every refusal leaves the outputs untouched.  The workspace holds two bitmasks of p bits per query (exclusions, targets),
 * t_max + 1 counters and t_max scores per query.  Asynchronous on `stream`. */
#define MODL_RECSYS_MAX_RANK_TARGETS 64
/* bytes of d_ws for a call with these arguments; 0 for arguments the call refuses (and for b == 0) */
size_t modl_recsys_ranks_workspace(int dtype, int64_t p, int k, int64_t b, int t_max);
int modl_recsys_ranks_f32(const float *d_code, const int64_t *d_code_rows, int64_t b, int k, const float *d_Dt, int64_t p,
                          const int32_t *d_ex_indptr, const int32_t *d_ex_indices, const int64_t *d_ex_rows,
                          const double *d_item_bias, const int32_t *d_t_indptr, const int32_t *d_t_indices, int t_max,
                          int32_t *d_ranks, int32_t *d_n_candidates, void *d_ws, size_t ws_bytes, void *stream);
int modl_recsys_ranks_f64(const double *d_code, const int64_t *d_code_rows, int64_t b, int k, const double *d_Dt, int64_t p,
                          const int32_t *d_ex_indptr, const int32_t *d_ex_indices, const int64_t *d_ex_rows,
                          const double *d_item_bias, const int32_t *d_t_indptr, const int32_t *d_t_indices, int t_max,
                          int32_t *d_ranks, int32_t *d_n_candidates, void *d_ws, size_t ws_bytes, void *stream);
/* One minibatch of RecsysDictFact._single_batch_fit (recsys.py:147-165, 168-213) in ONE call: the batch's ratings are
 * grouped by item on the host (batch order kept inside an item), staged through a pinned slot of the plan, and the
 * codes, the per-item B_ update, the C_ update and the dictionary update on the union of the batch's items are
 * launched on `stream`.  Asynchronous; the plan owns its staging slots and scratch.
 *   h_* : the CSR matrix in host memory (int32 / T, as d_*), n_rows its number of rows;
 *   h_rows[b] : the batch (row ids, in batch order);  h_order[k] : the atom order (numpy permutation, recsys.py:196);
 *   w : _batch_weight;  n_iter : n_iter_ after this batch (w_B = min(1, w n_iter / feature_n_iter), :182).
 * max_entries: the largest number of ratings one batch may hold. */
typedef struct modl_recsys_plan modl_recsys_plan;
int modl_recsys_plan_create(int dtype, int64_t p, int k, int64_t max_batch, int64_t max_entries, modl_recsys_plan **out);
void modl_recsys_plan_destroy(modl_recsys_plan *plan);
int modl_recsys_minibatch_f32(modl_recsys_plan *plan, const int32_t *h_indptr, const int32_t *h_indices, const float *h_data,
                              int64_t n_rows, const int32_t *d_indptr, const int32_t *d_indices, const float *d_data,
                              const int64_t *h_rows, int64_t b, const int64_t *h_order, double alpha, double w,
                              double n_iter, float *d_Dt, float *d_Bt, float *d_C, float *d_code, float *d_comp_norm,
                              int64_t *d_feature_n_iter, void *stream);
int modl_recsys_minibatch_f64(modl_recsys_plan *plan, const int32_t *h_indptr, const int32_t *h_indices, const double *h_data,
                              int64_t n_rows, const int32_t *d_indptr, const int32_t *d_indices, const double *d_data,
                              const int64_t *h_rows, int64_t b, const int64_t *h_order, double alpha, double w,
                              double n_iter, double *d_Dt, double *d_Bt, double *d_C, double *d_code,
                              double *d_comp_norm, int64_t *d_feature_n_iter, void *stream);
/* The per-minibatch host loop of RecsysDictFact.fit (recsys.py:135-139, 147-165) for a run of minibatches in ONE call:
 * h_rows[n_rows_fit] = the (permuted) row ids of the run, cut into minibatches of batch_size (the last one ragged).  Per
 * minibatch: n_iter += its rows, w = _batch_weight(n_iter, rows, learning_rate, 0) (:154), order = the legacy permutation(k)
 * of `order_rng` (:196; load it with numpy's state, modl_rk_set_mt_state), then the minibatch as modl_recsys_minibatch_*.
 * *n_iter is advanced; *n_done (optional) = minibatches enqueued - on an error the ones before the failing minibatch, with
 * n_iter and the generator left behind the last enqueued one.  Asynchronous. */
int modl_recsys_fit_batches_f32(modl_recsys_plan *plan, const int32_t *h_indptr, const int32_t *h_indices, const float *h_data,
                                int64_t n_rows, const int32_t *d_indptr, const int32_t *d_indices, const float *d_data,
                                const int64_t *h_rows, int64_t n_rows_fit, int64_t batch_size, modl_rk *order_rng, double alpha,
                                double learning_rate, int64_t *n_iter, float *d_Dt, float *d_Bt, float *d_C, float *d_code,
                                float *d_comp_norm, int64_t *d_feature_n_iter, void *stream, int64_t *n_done);
int modl_recsys_fit_batches_f64(modl_recsys_plan *plan, const int32_t *h_indptr, const int32_t *h_indices, const double *h_data,
                                int64_t n_rows, const int32_t *d_indptr, const int32_t *d_indices, const double *d_data,
                                const int64_t *h_rows, int64_t n_rows_fit, int64_t batch_size, modl_rk *order_rng, double alpha,
                                double learning_rate, int64_t *n_iter, double *d_Dt, double *d_Bt, double *d_C, double *d_code,
                                double *d_comp_norm, int64_t *d_feature_n_iter, void *stream, int64_t *n_done);
/* Synchronises `stream`; MODL_ETIMEOUT if a dictionary-update launch of this plan gave up in a cross-workgroup wait since the last
 * call (csrc/bcd.hip: bcd_few_kernel on up to sixteen workgroups; the update is incomplete, the flag is cleared), MODL_OK otherwise.
 * While the flag is up every further minibatch of the plan is refused with MODL_ETIMEOUT. */
int modl_recsys_plan_status(modl_recsys_plan *plan, void *stream);
/* diagnostics: minibatches of this plan that ran as ONE launch (csrc/recsys.hip: recsys_fused_kernel: at most 64 atoms, 64 rows
 * and 8192 ratings per minibatch) / as the separate launches */
int modl_recsys_plan_counts(const modl_recsys_plan *plan, int64_t *fused, int64_t *split);
/* diagnostics: on = 1 makes the last workgroup of every one-launch minibatch leave 100 MHz wall-clock stamps ([0] entry, [1] ids,
 * [2] Gram chunk, [3] records summed, [4] factor, [5] ticket, [6] last phase, [7] C_, [10] end (the same stamp as [7]), [11] items;
 * [8], [9], [12] and beyond are not written); h_out[16] (may be NULL) receives the last launch's (synchronises the device); on = 0
 * frees them */
int modl_recsys_plan_stamps(modl_recsys_plan *plan, int on, unsigned long long *h_out);
/* diagnostics: host time (ms) the plan has spent waiting for the device to read a staging slot (eight minibatches of lead) */
int modl_recsys_plan_wait_ms(const modl_recsys_plan *plan, double *ms);
/* C = beta C + alpha rows^T rows, rows[b][k]  (recsys.py:159-160: beta = 1 - w, alpha = w / b) */
int modl_gram_axpby_f32(const float *d_rows, int64_t b, int k, float *d_C, float beta, float alpha, void *stream);
int modl_gram_axpby_f64(const double *d_rows, int64_t b, int k, double *d_C, double beta, double alpha, void *stream);
/* _update_dict on device-resident state (dict_fact.py:650-715, recsys.py:187-213): block-coordinate
 * update of the rows d_subset[s] (int32, NULL = all rows 0..s-1) of d_Dt[p][k].  d_order / h_order: the
 * atom order on the device (int32) and on the host (int64).  Scratch: modl_dict_update_workspace().
 * k <= MODL_MAX_COMPONENTS; beyond 1024 atoms every optimizer but sgd runs one launch pair per atom.
 * This direct call carries no plan: where the f32 update runs as one persistent launch (MODL_DEBUG_BCD_PERSIST) and that
 * launch cannot complete because its workgroups are not all resident (another process holds compute units), the call cannot
 * report it - it returns MODL_OK when the launch was queued.  Only the plan-based entry points (modl_somf_partial_fit*)
 * read the launch's flags back, recover, and return MODL_ETIMEOUT for an incomplete update. */
size_t modl_dict_update_workspace(int dtype, int64_t s_max, int k);
int modl_dict_update_f32(float *d_Dt, const float *d_Bt, const float *d_C, float *d_comp_norm,
                         const int32_t *d_subset, int64_t s, const int32_t *d_order, const int64_t *h_order, int k,
                         int optimizer, int comp_pos, double comp_l1_ratio, double w, double step_size, void *d_ws,
                         size_t ws_bytes, void *stream);
int modl_dict_update_f64(double *d_Dt, const double *d_Bt, const double *d_C, double *d_comp_norm,
                         const int32_t *d_subset, int64_t s, const int32_t *d_order, const int64_t *h_order, int k,
                         int optimizer, int comp_pos, double comp_l1_ratio, double w, double step_size, void *d_ws,
                         size_t ws_bytes, void *stream);
/* Which kernels modl_dict_update_* would run for these arguments under the current modl_debug_set switches, written to
 * buf[cap] as "family/parameter/..." ("persist/RT1", "block/RT2/GPW8/acc1/shards4", "grouped/EPT20/G8/KPL4/enet", "wide",
 * ...: csrc/bcd.hip, du_route).  Read-only: nothing is launched, no device memory is written.  ncu > 0: the route on a
 * device of that many compute units, one workgroup of the persistent launch resident on each - no device is touched, so
 * this works without a GPU; ncu == 0: the current device is asked, as modl_dict_update_* asks it.  MODL_EINVAL for a bad
 * dtype, k outside 1 .. MODL_MAX_COMPONENTS, s <= 0, ncu < 0 or a buffer too small (64 bytes hold every route). */
int modl_dict_update_route(int dtype, int k, int64_t s, int optimizer, int comp_pos, double comp_l1_ratio, int ncu,
                           char *buf, size_t cap);

/* ------------------------------------------------------------------------- *
 * Fused, device-resident minibatch step = DictFact._single_batch_fit,
 * dict_fact.py:495-533 (+ _compute_code :577-648, _update_C/_update_B :559-575,
 * _update_dict :650-715).  The host keeps drawing `subset` (modl_sampler),
 * `order` (numpy legacy RandomState.permutation, dict_fact.py:672) and `w`
 * (modl_batch_weight) exactly as the reference does and passes them in.
 * ------------------------------------------------------------------------- */
typedef struct modl_somf_desc {
    int32_t dtype;          /* MODL_F32 / MODL_F64 */
    int32_t k;              /* n_components, 1 .. MODL_MAX_COMPONENTS */
    int64_t p;              /* n_features */
    int64_t n_samples;      /* rows of code_ (and of the averages) */
    int32_t G_agg;          /* MODL_AGG_* (dict_fact.py:132-133) */
    int32_t Dx_agg;
    int32_t optimizer;      /* MODL_OPT_* */
    int32_t code_pos;
    int32_t comp_pos;
    int32_t max_iter;
    double code_alpha;
    double code_l1_ratio;
    double comp_l1_ratio;
    double tol;
    double step_size;
    int32_t max_batch;      /* largest minibatch this plan will see */
    int32_t flags;          /* MODL_FLAG_* (diagnostics), 0 otherwise */
} modl_somf_desc;

/* device state of one estimator (allocated by the caller; all T = dtype) */
typedef struct modl_somf_state {
    void *d_Dt;          /* [p][k]  components_.T */
    void *d_Bt;          /* [p][k]  B_.T  (several GPUs: this rank's partial sum, B_ = sum over ranks) */
    void *d_C;           /* [k][k]  C_    (several GPUs: this rank's partial sum) */
    void *d_code;        /* [n_samples][k] code_ */
    void *d_comp_norm;   /* [k] comp_norm_ */
    void *d_G;           /* [k][k] G_ (G_agg == full), else NULL */
    void *d_Dx_average;  /* [n_samples][k] (Dx_agg == average), else NULL */
    void *d_G_average;   /* [n_samples][k][k] (G_agg == average), else NULL */
} modl_somf_state;

/* one minibatch; h_* arrays are copied to the device by the call */
typedef struct modl_somf_batch {
    const void *d_X;            /* [b][ldx] minibatch rows, device */
    int64_t ldx;
    int32_t b;                  /* rows in this rank's minibatch */
    int32_t s;                  /* subset length; s == p with h_subset == NULL means all features */
    const int64_t *h_sample_idx;/* [b] rows of code_ (NULL = 0..b-1) */
    const int64_t *h_subset;    /* [s] feature subset (unsorted ok) */
    const int64_t *h_order;     /* [k] atom order of the dictionary update */
    const void *h_w_sample;     /* [b] T, w_sample (only for *_agg == average; may be NULL otherwise) */
    double w;                   /* minibatch weight (_batch_weight) */
    double reduction;           /* self.reduction (scales Dx and G, dict_fact.py:595,604) */
    int64_t b_global;           /* sum of b over all ranks (== b on one GPU) */
} modl_somf_batch;

typedef struct modl_somf_plan modl_somf_plan;
/* allocates the per-estimator scratch (device workspace, pinned staging) on the
 * current device. */
int modl_somf_plan_create(const modl_somf_desc *desc, modl_somf_plan **out);
void modl_somf_plan_destroy(modl_somf_plan *plan);
/* update solver / aggregation parameters between minibatches (set_params,
 * dict_fact.py:339-357).  k, p, dtype, n_samples, max_batch must not change. */
int modl_somf_plan_update(modl_somf_plan *plan, const modl_somf_desc *desc);

/* One GPU: the whole minibatch step (codes, C_/B_ update in the epilogues of the increment products, dictionary
 * update).  Asynchronous on `stream`. */
int modl_somf_step(modl_somf_plan *plan, const modl_somf_state *st, const modl_somf_batch *bt, void *stream);

/* One MASKED minibatch in one call: DictFact._single_batch_fit (dict_fact.py:495-533) for dense rows with missing entries,
 * by the algorithm of RecsysDictFact._single_batch_fit (modl/decomposition/recsys.py:147-213) with the elastic-net codes and
 * atom constraints of DictFact.  d_obs[b][ldo] bytes (1 = observed) goes with bt->d_X[b][ldx]; the row's mask takes the
 * place of the random feature subset: bt->h_subset must be NULL and bt->s == p, bt->reduction is not read; h_sample_idx,
 * h_order and w are as in modl_somf_step.  In order, on `stream` (asynchronous):
 *   codes   every row on its own observed entries - G_i, Dx_i of modl_masked_gram_* (dict_fact.py:594-604 with S = M_i),
 *           solved as _enet_regression_multi_gram (dict_fact_fast.pyx:33-113) from the warm start code_[h_sample_idx],
 *           the solver's X being the zero-filled row; chunks of rows keep the Gram matrices under 256 MB (scratch owned
 *           by the plan, allocated on first use); a row without an observed entry gets a zero code;
 *   C_      <- (1 - w) C_ + (w / b) code^T code                  (recsys.py:159-160, as modl_gram_axpby_*);
 *   B_      per feature, as modl_masked_stats_* with n_iter = n_iter_ after this minibatch (recsys.py:175, 182-185);
 *   D       the dictionary update of modl_somf_step over all p features, with the plan's flag word: an update that
 *           gives up is reported by modl_somf_status / MODL_ETIMEOUT and counted by modl_somf_persist_recoveries.
 * MODL_EINVAL before any device work: a plan whose aggregations are not both MODL_AGG_MASKED, optimizer sgd, k > 1024,
 * a NULL pointer, ldo < p, a subset, b outside 1..max_batch, n_iter <= 0. */
int modl_somf_masked_step(modl_somf_plan *plan, const modl_somf_state *st, const modl_somf_batch *bt, const uint8_t *d_obs,
                          int64_t ldo, int64_t *d_feature_n_iter, int64_t n_iter, void *stream);

/* The per-minibatch HOST loop of partial_fit / _single_batch_fit (dict_fact.py:331-337, 495-526) behind the boundary:
 * n_rows rows of d_X in minibatches of batch_size (the last one may be ragged), for each of them
 *   subset  = sampler.yield_subset(reduction)                      (:507)
 *   n_iter += b_global ; w = _batch_weight(n_iter, b_global, learning_rate, 0)   (:510, :515)
 *   order   = the legacy permutation(k) of `order_rng`               (:672; load it with numpy's state, see
 *                                                                     modl_rk_set_mt_state, and read the state back)
 *   modl_somf_step (comm == NULL) or modl_somf_step_dist (comm != NULL)
 * - the same draws in the same order as the Python loop, so the same bits.  h_sample_idx: n_rows rows of code_ or
 * NULL (0 .. n_rows-1); h_b_global: rows of each GLOBAL minibatch (several ranks) or NULL (== this rank's).
 * Plans with *_agg == average need the per-sample weights the caller keeps (sample_n_iter_): MODL_EINVAL - use the
 * per-minibatch calls.  Asynchronous on `stream` (blocks only on the 8-deep staging ring).
 * With a communicator the staging copy of minibatch t + 1 rides on the last launch of step t's dictionary update
 * exactly as on one GPU (ABI 3; before, a multi-GPU step spent a launch on it).
 * Errors (ABI 3): *n_done (may be NULL) receives the number of minibatches that were enqueued completely; when a
 * minibatch fails, *n_iter, `sampler` and `order_rng` are left where the LAST ENQUEUED minibatch left them (the draws
 * of the look-ahead are rewound), so that the caller can correct the input and continue the reference's streams. */
struct modl_comm;
int modl_somf_partial_fit_chunk(modl_somf_plan *plan, const modl_somf_state *st, const void *d_X, int64_t ldx,
                                int64_t n_rows, int32_t batch_size, const int64_t *h_sample_idx, modl_sampler *sampler,
                                modl_rk *order_rng, int64_t *n_iter, double learning_rate, double reduction,
                                const int64_t *h_b_global, struct modl_comm *comm, int64_t *n_done, void *stream);

/* Several GPUs (one process per GPU, the rows of a global minibatch of b_global rows split over the ranks; every
 * rank passes the same subset / order / w).  The recursions C_ <- (1 - w) C_ + (w / b_global) code^T code and
 * B_ <- (1 - w) B_ + (w / b_global) code^T X are linear in the increments, so every rank keeps its own PARTIAL
 * statistics (st->d_C, st->d_Bt: C_ = sum over ranks, B_ likewise) and only what the dictionary update reads is
 * exchanged - the HEAD  [ C_r (k*k) | the rows of B_r of the sampled features, compact (s*k) ]:
 *   1. modl_somf_code_and_partials : codes of the rank's rows, update of its partial statistics, head -> d_head;
 *   2. the caller sums d_head[0 .. modl_somf_head_elems) over the ranks (ncclAllReduce / RCCL, in place);
 *   3. modl_somf_apply_and_update_dict : the dictionary update from the summed head, identical on every rank
 *      (replicas of the dictionary stay bit-identical).
 * d_head holds modl_somf_delta_elems() = k*k + p*k elements of T (a minibatch without a subset array carries all
 * p rows of B_r).  With one rank and no reduction the two calls give the same bits as modl_somf_step. */
int64_t modl_somf_delta_elems(const modl_somf_desc *desc);
int modl_somf_code_and_partials(modl_somf_plan *plan, const modl_somf_state *st, const modl_somf_batch *bt,
                                void *d_head, void *stream);
/* elements of the head written by the LAST modl_somf_code_and_partials (MODL_ESTATE if none is pending) */
int modl_somf_head_elems(const modl_somf_plan *plan, int64_t *head_elems);
int modl_somf_apply_and_update_dict(modl_somf_plan *plan, const modl_somf_state *st,
                                    const modl_somf_batch *bt, const void *d_head, void *stream);

/* The same exchange inside the library: an RCCL communicator (one per process / GPU, as the north star's
 * "RCCL all-reduce of A_ and B_ over xGMI") and the whole multi-GPU minibatch as ONE call, everything enqueued on
 * one stream.  librccl.so is resolved at run time (dlopen), MODL_ENORCCL if it is not there.
 *   rank 0: modl_comm_unique_id(&id); ship the 128 bytes to the other ranks (MPI, a file, torch.distributed ...);
 *   every rank, with its GPU current: modl_comm_create(&id, rank, world, &comm)   (collective);
 *   per minibatch: modl_somf_step_dist(plan, &st, &bt, comm, stream);  bt.b_global = rows of the global minibatch. */
typedef struct { char bytes[128]; } modl_comm_id;          /* ncclUniqueId */
typedef struct modl_comm modl_comm;
int modl_comm_unique_id(modl_comm_id *out);
int modl_comm_create(const modl_comm_id *id, int rank, int world, modl_comm **out);
void modl_comm_destroy(modl_comm *comm);
/* in-place sum over the ranks of n elements (dtype MODL_F32 / MODL_F64) of a device buffer, on `stream` */
int modl_comm_all_reduce_sum(modl_comm *comm, void *d_buf, int64_t n, int dtype, void *stream);
/* ABI 4 - the abort path.  A rank that dies leaves the others inside ncclAllReduce in the middle of a chunk call; a plain
 * stream synchronisation would then wait for ever.  modl_comm_wait waits for `stream` to drain WHILE watching the
 * communicator (ncclCommGetAsyncError) and the clock: an asynchronous RCCL error, or more than timeout_s seconds
 * (<= 0: no limit) without the stream draining, aborts the communicator (ncclCommAbort: the kernels of this rank that wait
 * inside a collective are released) and returns MODL_ERCCL; MODL_OK when the stream is idle.  After an abort every call
 * on the communicator returns MODL_ERCCL; modl_comm_destroy still frees the handle.  modl_comm_abort: the same, at once
 * (a launcher that has seen another rank exit).  The reference has no counterpart (it is a single-process estimator). */
int modl_comm_wait(modl_comm *comm, void *stream, double timeout_s);
int modl_comm_abort(modl_comm *comm);
int modl_somf_step_dist(modl_somf_plan *plan, const modl_somf_state *st, const modl_somf_batch *bt, modl_comm *comm,
                        void *stream);

/* d_dst[r][0..cols) = d_src[d_idx[r]][0..cols): the row permutations around the path (X = X[permutation] after
 * an epoch, dict_fact.py:309-310; masked_data[permutation], fmri.py:541) on device-resident rows. */
int modl_gather_rows_f32(const float *d_src, int64_t src_ld, const int64_t *d_idx, int64_t n_rows, int64_t cols,
                         float *d_dst, int64_t dst_ld, void *stream);
int modl_gather_rows_f64(const double *d_src, int64_t src_ld, const int64_t *d_idx, int64_t n_rows, int64_t cols,
                         double *d_dst, int64_t dst_ld, void *stream);

/* Which matrix-core launches the library would run for a section of the work on a plan of this descriptor, under the current
 * MODL_DEBUG_STATS_RESIDENT switch and desc->flags, written to buf[cap] as "kernel/alignment/tiles/..." ("dense/al/t2x2/edge/
 * s7/kps160/last40/pipe/sym0", "prep+pair/Dx[...]/G[...]", "stats32/al/t7x2/ride:wide128", "resident16/scalar/ride:after[...]",
 * ".../partialG[gather/small/...]": csrc/step_products.hip; the grammar is spelled out in tests/test_product_routes.py).
 * Read-only: nothing is launched, no device memory is written, no plan is needed and no device is touched, so this works
 * without a GPU.  section: MODL_ROUTE_TRANSFORM - Dx of ONE chunk of b rows of modl_somf_transform; MODL_ROUTE_FULL_GRAM -
 * modl_somf_full_gram; MODL_ROUTE_CODE_PRODUCTS - Dx and G in front of the code solve of a step, with the Gram pass of the
 * dictionary update for G_agg = full; MODL_ROUTE_STATS - the C_ and B_ statistics behind it, and how the rows of B_ that were
 * not sampled are updated.  b, s, has_subset, has_idx, ldx: as the minibatch (or chunk) carries them; x_offset: where X
 * starts, in elements from a 16-byte aligned address.  Every other buffer (Dt, code_, what the library allocates) is taken
 * as 16-byte aligned.  MODL_EINVAL for a bad descriptor, section, b, s or ldx, or a buffer too small:
 * MODL_PRODUCT_ROUTE_MAX bytes hold every route whose gather launches of 128 x 32 tiles have at most 256 row tiles (a
 * misaligned p x k product with k <= 32 names the staging of every row tile: one character each). */
#define MODL_ROUTE_TRANSFORM 0
#define MODL_ROUTE_FULL_GRAM 1
#define MODL_ROUTE_CODE_PRODUCTS 2
#define MODL_ROUTE_STATS 3
#define MODL_PRODUCT_ROUTE_MAX 512
int modl_somf_product_route(const modl_somf_desc *desc, int section, int b, int64_t s, int has_subset, int has_idx,
                            int64_t ldx, int64_t x_offset, char *buf, size_t cap);

/* G_ = D D^T (prepare / set_params(G_agg='full'), dict_fact.py:355,477) */
int modl_somf_full_gram(modl_somf_plan *plan, const void *d_Dt, void *d_G, void *stream);

/* CodingMixin.transform, dict_fact.py:47-92: d_code_out[n][k] from ones.
 * d_G may be NULL (computed from d_Dt). */
int modl_somf_transform(modl_somf_plan *plan, const void *d_Dt, const void *d_G, const void *d_X, int64_t ldx,
                        int64_t n, void *d_code_out, void *stream);

/* Orthogonal matching pursuit (Batch-OMP on Gram quantities, csrc/omp.hip; no counterpart in the reference): the code of a
 * row has at most n_nonzero non-zeros, the atoms picked greedily by the largest |correlation| with the residual (equal
 * values: the lowest index), the coefficients the least-squares fit on the picked atoms.  Sample i reads G_i = d_G + i *
 * g_stride (g_stride 0: one shared k x k matrix; k * k: one per row, as modl_enet_regression_multi_gram_*), d_Dx[i][:] and,
 * with tol >= 0, d_xnorm2[i] = |x_i|^2: a row then stops as soon as its squared residual is <= tol (the tol of scikit-learn's
 * orthogonal_mp_gram), n_nonzero still capping the support.  tol < 0 (or NaN): no threshold, d_xnorm2 is not read and may
 * be NULL.  A row also stops when no correlation is left, or when the best atom is numerically in the span of the picked
 * ones (Schur complement d <= 16 eps_T G_jj).  Written in full by the kernel: d_code[b][k] (zeros off the support),
 * d_support[b][n_nonzero] (selection order, -1 beyond the row's count) and d_n_active[b].  All arithmetic in the dtype; no
 * atomics; the result of a row is the same bits from run to run and in any batch.
 * 1 <= n_nonzero <= MODL_OMP_MAX_NONZERO, n_nonzero <= k; k <= MODL_MAX_COMPONENTS with a shared matrix, k <= 1024 with one
 * per row.  MODL_EINVAL before any device work: a NULL pointer (d_xnorm2 with tol < 0 and d_ws apart), b < 0, k or n_nonzero
 * out of range, g_stride neither 0 nor k * k.  b == 0 does nothing.  MODL_ENOMEM: ws_bytes below modl_omp_workspace(...)
 * (which is 0 for every valid call today: a row's state lives in registers and LDS; the pair is there so that this can
 * change without a new signature).  No device: MODL_ENOGPU. */
#define MODL_OMP_MAX_NONZERO 64
size_t modl_omp_workspace(int dtype, int64_t b, int k, int n_nonzero, int multi_gram);
int modl_omp_gram_f32(const float *d_G, int64_t g_stride, const float *d_Dx, const float *d_xnorm2, int64_t b, int k,
                      int n_nonzero, float tol, float *d_code, int32_t *d_support, int32_t *d_n_active, void *d_ws,
                      size_t ws_bytes, void *stream);
int modl_omp_gram_f64(const double *d_G, int64_t g_stride, const double *d_Dx, const double *d_xnorm2, int64_t b, int k,
                      int n_nonzero, double tol, double *d_code, int32_t *d_support, int32_t *d_n_active, void *d_ws,
                      size_t ws_bytes, void *stream);
/* modl_somf_transform with the OMP coder in the place of the elastic-net solve: the same Gram matrix (d_G may be NULL) and
 * Dx = X D^T products, row norms only when tol >= 0, chunks of the plan's max_batch.  d_code_out[n][k]; d_support_out
 * [n][n_nonzero] and d_n_active_out[n] may be NULL.  The plan's code_* settings are not used. */
int modl_somf_transform_omp(modl_somf_plan *plan, const void *d_Dt, const void *d_G, const void *d_X, int64_t ldx,
                            int64_t n, int n_nonzero, double tol, void *d_code_out, int32_t *d_support_out,
                            int32_t *d_n_active_out, void *stream);

/* diagnostics: coordinate-descent sweeps per sample of the last phase-1 call of this plan
 * (0 for the ridge branch).  Synchronises `stream`. */
int modl_somf_last_sweeps(modl_somf_plan *plan, int32_t *h_out, int cap, int *n_out, void *stream);
/* diagnostics: from now on minibatch number t (counted from this call) of this plan leaves its sweep counts in
 * d_buf[(t % cap_minibatches) * max_batch ...] (int32, device memory owned by the caller, cap_minibatches * max_batch
 * entries) - a tolerance-stopped solver may legitimately do a sweep more or less on a sample when its inputs differ in
 * the last bits, and a long-horizon parity test has to know where that happened.  d_buf == NULL: off. */
int modl_somf_sweeps_history(modl_somf_plan *plan, int32_t *d_buf, int64_t cap_minibatches);

/* diagnostics: 48 shader-clock stamps of the last fused dictionary-update block launch (40 ..: the first riding tile),
 * h_out[48] (synchronises the device) */
/* The persistent dictionary-update launch (csrc/bcd_persist.hip) needs all its workgroups resident at once.  The library asks
 * the runtime whether they fit (occupancy of the kernel's own register / LDS footprint on the plan's device); what it cannot
 * ask is whether another process, or a compute-unit mask, holds units of the same GPU.  Every wait inside the launch is
 * bounded, and what a wait that gives up means is decided on the device:
 *  - BEFORE the first block of atoms is resolved nothing has been applied: the row workgroups leave, the resolver workgroup
 *    runs the reference's sweep by itself (milliseconds instead of microseconds) and the stream carries on with a correctly
 *    updated dictionary - no error.  The plan counts the event (modl_somf_persist_recoveries, a plain read of pinned memory,
 *    no synchronisation) and, from the first one on, keeps one launch per block: whatever held the units may still be there.
 *  - LATER the update is incomplete.  The plan raises a flag that the host reads before every enqueue: the next
 *    modl_somf_step / _code_and_partials / _apply_and_update_dict / _partial_fit_chunk of that plan returns MODL_ETIMEOUT
 *    without enqueuing anything, and keeps doing so until modl_somf_status has been called.
 * modl_somf_status synchronises `stream`, returns MODL_ETIMEOUT if an update of this plan was left incomplete since the last
 * call (and clears the flag; the dictionary of that plan is then not to be trusted: DictFact.prepare again), MODL_OK otherwise.
 * The Python estimator checks it whenever it synchronises and warns once per recovery.  (The reference has no counterpart: it
 * is CPU code.) */
int modl_somf_status(modl_somf_plan *plan, void *stream);
int modl_somf_persist_recoveries(modl_somf_plan *plan, int64_t *count);
int modl_somf_debug_stamps(modl_somf_plan *plan, unsigned long long *h_out);
/* diagnostics: 192 shader-clock stamps of the last PERSISTENT dictionary-update launch (csrc/bcd_persist.hip; written by the
 * diagnostics build only): [0] resolver start, [1 + 5 b ..] per block b: arrivals complete, pieces in LDS, Gram matrix
 * formed, recursion done, S published; [96] row workgroup 0 start, [97] block 0 handed over, [98 + 4 b ..] per block b >= 1:
 * S of block b - 2 fetched, applied + corrected, candidates formed, pieces handed over */
int modl_somf_debug_persist_stamps(modl_somf_plan *plan, unsigned long long *h_out);

/* diagnostics (env MODL_GEMM_STAMPS=1): h_out[8] = shader-clock stamps of one tile of the head statistics product:
 * [0] entry, [1] loads issued, [2] first K-tile in LDS, [3] K loop done, [4] epilogue done; [6], [7] = 100 MHz wall
 * clock at entry / exit (synchronises the device) */
int modl_somf_debug_gemm_stamps(modl_somf_plan *plan, unsigned long long *h_out);

/* ------------------------------------------------------------------------- *
 * Either side of the step: the image patch pipeline and the
 * objective value of CodingMixin.score.
 * ------------------------------------------------------------------------- */
/* fill, modl/input_data/image_fast.pyx:59-74: every (pp, qq, rr) of a p x q x r grid in C order, h_out[p*q*r][3]. Host. */
int modl_image_fill(int64_t p, int64_t q, int64_t r, int64_t *h_out);
/* clean_mask, image_fast.pyx:12-57: origins of the x*y*z windows of h_image[H][W][C] that hold no missing (-1)
 * value, in C order; h_out[(H-x+1)(W-y+1)(C-z+1)][3] (may be NULL: count only), *n_out = number of rows.  Host. */
int modl_image_clean_mask_f32(const float *h_image, int64_t H, int64_t W, int64_t C, int64_t x, int64_t y, int64_t z,
                              int64_t *h_out, int64_t *n_out);
int modl_image_clean_mask_f64(const double *h_image, int64_t H, int64_t W, int64_t C, int64_t x, int64_t y, int64_t z,
                              int64_t *h_out, int64_t *n_out);
/* LazyCleanPatchExtractor.partial_transform (modl/feature_extraction/image.py:54-63) + scale_patches
 * (modl/input_data/image.py:4-23, channel-wise) + flattening (modl/decomposition/image.py:190-199) in one launch:
 * d_out[r][:] = window of d_image[H][W][C] at origin d_idx3[r] = (i, j, c0), shape (x, y, z), C order, each channel
 * centred (with_mean) and divided by (its l2 norm or 1 if 0) * sqrt(z) (with_std).  z <= 1024. */
int modl_image_patches_f32(const float *d_image, int64_t H, int64_t W, int64_t C, const int64_t *d_idx3, int64_t n, int x,
                           int y, int z, int with_mean, int with_std, float *d_out, int64_t ldo, void *stream);
int modl_image_patches_f64(const double *d_image, int64_t H, int64_t W, int64_t C, const int64_t *d_idx3, int64_t n, int x,
                           int y, int z, int with_mean, int with_std, double *d_out, int64_t ldo, void *stream);
/* Reconstruction of an image from the codes of its patches (no counterpart in the reference): encode every window of a
 * regular PATCH GRID, decode it, undo the per-patch scaling, average the overlapping windows - all on the device.
 * The grid: along an axis of length L with patch length x and stride s the origins are 0, s, 2 s, ... <= L - x, plus
 * L - x itself when it is not already the last one (the border is always covered): ceil((L - x) / s) + 1 origins,
 * origin(r) = min(r s, L - x).  A patch spans all channels; patches are numbered row-major over (grid row, grid
 * column).  A pass is the contiguous range of grid rows [row0, row0 + nrows): nrows * grid_cols patches.  Every call
 * below checks 1 <= si <= x <= H, 1 <= sj <= y <= W, 1 <= C <= 1024, 0 <= row0, row0 + nrows <= grid_rows, its
 * pointers and leading dimensions before any device work (MODL_EINVAL); none needs scratch, none uses atomics: the
 * results are bit-identical from run to run.
 * modl_image_grid_shape: the number of grid rows and columns.  Host. */
int modl_image_grid_shape(int64_t H, int64_t W, int64_t x, int64_t y, int64_t si, int64_t sj, int64_t *grid_rows,
                          int64_t *grid_cols);
/* modl_image_patches_* on the patches of a pass, origins computed from the grid (no index array): the rows equal those of
 * modl_image_patches_* at the same origins bit for bit.  Also kept, per patch and channel: d_mean[nrows*grid_cols][C]
 * (0 without with_mean) and d_den[..][C], the divisor that was applied (1 where none was). */
int modl_image_grid_patches_f32(const float *d_image, int64_t H, int64_t W, int64_t C, int x, int y, int si, int sj,
                                int64_t row0, int64_t nrows, int with_mean, int with_std, float *d_out, int64_t ldo,
                                float *d_mean, float *d_den, void *stream);
int modl_image_grid_patches_f64(const double *d_image, int64_t H, int64_t W, int64_t C, int x, int y, int si, int sj,
                                int64_t row0, int64_t nrows, int with_mean, int with_std, double *d_out, int64_t ldo,
                                double *d_mean, double *d_den, void *stream);
/* d_out[m][e] = (d_code d_Dt^T)[m][e] * d_den[m][e % C] + d_mean[m][e % C]: the patches of the codes d_code[n][k] on the
 * dictionary d_Dt[P][k] (feature-major, as the plan holds it), put back on the image's scale (P a multiple of C).
 * d_mean and d_den both NULL: the plain product (CodingMixin.inverse_transform; C is then ignored).  Any k >= 1. */
int modl_image_decode_f32(const float *d_code, int64_t n, int k, const float *d_Dt, int64_t P, int C, const float *d_mean,
                          const float *d_den, float *d_out, int64_t ldo, void *stream);
int modl_image_decode_f64(const double *d_code, int64_t n, int k, const double *d_Dt, int64_t P, int C,
                          const double *d_mean, const double *d_den, double *d_out, int64_t ldo, void *stream);
/* d_acc[H][W][C] (f64, zeroed by the caller before the first pass) += the flattened patches d_patches[nrows*grid_cols][ldp]
 * of a pass, each at its window.  A gather: every accumulator adds its covering patches one at a time in grid order, so
 * the sums do not depend on how the grid rows are cut into passes (passes in increasing row0), bit for bit. */
int modl_image_overlap_add_f32(const float *d_patches, int64_t ldp, int64_t H, int64_t W, int64_t C, int x, int y, int si,
                               int sj, int64_t row0, int64_t nrows, double *d_acc, void *stream);
int modl_image_overlap_add_f64(const double *d_patches, int64_t ldp, int64_t H, int64_t W, int64_t C, int x, int y, int si,
                               int sj, int64_t row0, int64_t nrows, double *d_acc, void *stream);
/* d_image_out[H][W][C] = d_acc / (number of grid patches that cover the pixel) */
int modl_image_overlap_finish_f32(const double *d_acc, int64_t H, int64_t W, int64_t C, int x, int y, int si, int sj,
                                  float *d_image_out, void *stream);
int modl_image_overlap_finish_f64(const double *d_acc, int64_t H, int64_t W, int64_t C, int x, int y, int si, int sj,
                                  double *d_image_out, void *stream);
/* Inpainting (no counterpart in the reference's image module).  The estimator is the reference's own: a code is
 * estimated from a subset S of the features with Dx = r X_S D_S^T, G = r D_S D_S^T, r = p / |S|
 * (modl/decomposition/dict_fact.py:594-604); here S is each row's own set of observed entries, so every row has its own
 * Gram matrix and _enet_regression_multi_gram (dict_fact_fast.pyx:33-113, modl_enet_regression_multi_gram_*) solves it.
 *
 * modl_masked_gram_*: for sample ii of b, row i = d_rows[ii] (d_rows NULL: i = ii), M_i = { e : d_obs[i][e] != 0 },
 * m_i = |M_i| (-> d_nobs[ii]; d_nobs may be NULL), r_i = p / m_i:
 *   d_G[ii][a][c] = r_i sum_{e in M_i} d_Dt[e][a] d_Dt[e][c]     (the full k x k matrix, symmetric bit for bit)
 *   d_Dx[ii][a]   = r_i sum_{e in M_i} d_X[i][e] d_Dt[e][a]
 * and zeros when m_i = 0.  d_Dt[p][k] feature-major, d_X[..][ldx], d_obs[..][ldo] bytes.  Values of d_X at unobserved
 * positions never reach the result (they may be NaN).  The products run on the matrix cores in the dtype, the scaling
 * follows the sums; no atomics (bit-identical from run to run), no scratch.  1 <= k <= 1024, p >= 1, b >= 0; a NULL
 * pointer (d_rows and d_nobs apart), k out of range, ldx < p or ldo < p -> MODL_EINVAL before any device work. */
int modl_masked_gram_f32(const float *d_Dt, int64_t p, int k, const float *d_X, int64_t ldx, const uint8_t *d_obs,
                         int64_t ldo, const int64_t *d_rows, int64_t b, float *d_G, float *d_Dx, int32_t *d_nobs,
                         void *stream);
int modl_masked_gram_f64(const double *d_Dt, int64_t p, int k, const double *d_X, int64_t ldx, const uint8_t *d_obs,
                         int64_t ldo, const int64_t *d_rows, int64_t b, double *d_G, double *d_Dx, int32_t *d_nobs,
                         void *stream);
/* The statistic B_ from dense rows with missing entries: the per-feature update of RecsysDictFact
 * (modl/decomposition/recsys.py:175, 182-185) for a minibatch of b dense rows.  Sample ii is row i = d_rows[ii] (d_rows
 * NULL: i = ii) of d_X[..][ldx] / d_obs[..][ldo] (bytes, 1 = observed), d_code_b[b][k] holds the minibatch's codes.  Per
 * feature e with c_e = #{ii : d_obs[i][e] != 0} (-> d_count[e]; d_count may be NULL):
 *   c_e = 0: d_Bt[e][:] and d_feature_n_iter[e] are left untouched, bit for bit;  otherwise
 *   d_feature_n_iter[e] += c_e;   w_e = min(1, w (c_e / b) (n_iter / d_feature_n_iter[e]))     (f64, in that order)
 *   d_Bt[e][:] <- (1 - w_e) d_Bt[e][:] + (w_e / c_e) sum_{ii : e observed} d_X[i][e] d_code_b[ii][:]
 * (b = 1: the reference's w_B; every row observed everywhere: w_e = w, DictFact._update_B, dict_fact.py:567-575).  The
 * product runs on the matrix cores in the dtype; values of d_X at unobserved positions never reach it (they may be
 * NaN).  Two launches: the product launch only reads d_feature_n_iter, the launch behind it writes it; no atomics, no
 * scratch, the same bits from run to run.  1 <= k <= 1024, p >= 1; a NULL pointer (d_rows and d_count apart), k out of
 * range, ldx < p, ldo < p or b < 0 -> MODL_EINVAL before any device work; b = 0 does nothing. */
int modl_masked_stats_f32(const float *d_X, int64_t ldx, const uint8_t *d_obs, int64_t ldo, const int64_t *d_rows,
                          int64_t b, int64_t p, int k, const float *d_code_b, float *d_Bt, int64_t *d_feature_n_iter,
                          int32_t *d_count, double w, int64_t n_iter, void *stream);
int modl_masked_stats_f64(const double *d_X, int64_t ldx, const uint8_t *d_obs, int64_t ldo, const int64_t *d_rows,
                          int64_t b, int64_t p, int k, const double *d_code_b, double *d_Bt, int64_t *d_feature_n_iter,
                          int32_t *d_count, double w, int64_t n_iter, void *stream);
/* modl_image_grid_patches_* on an image with holes: d_obs_image[H][W][C] bytes, 1 = observed.  Per patch, channel c with
 * the observed window elements O_c, n_c = |O_c|, N = x y:  mean_c = (sum_{O_c} v) / n_c (with_mean and n_c > 0, else
 * 0); observed elements are centred, unobserved ones written as 0; with_std: den_c = norm_c sqrt(C) with norm_c =
 * sqrt(sum_{O_c} u^2) sqrt(N / n_c), the estimate of the full window's norm (1 if it is 0 or n_c = 0), else den_c = 1.
 * Also d_obs_out[n][x*y*C] (the window of d_obs_image in row order) and d_nobs[n] (its sum).  A patch with every
 * element observed gives the row, mean and den of modl_image_grid_patches_* bit for bit. */
int modl_image_grid_patches_masked_f32(const float *d_image, int64_t H, int64_t W, int64_t C, int x, int y, int si,
                                       int sj, int64_t row0, int64_t nrows, int with_mean, int with_std, float *d_out,
                                       int64_t ldo, float *d_mean, float *d_den, const uint8_t *d_obs_image,
                                       uint8_t *d_obs_out, int32_t *d_nobs, void *stream);
int modl_image_grid_patches_masked_f64(const double *d_image, int64_t H, int64_t W, int64_t C, int x, int y, int si,
                                       int sj, int64_t row0, int64_t nrows, int with_mean, int with_std, double *d_out,
                                       int64_t ldo, double *d_mean, double *d_den, const uint8_t *d_obs_image,
                                       uint8_t *d_obs_out, int32_t *d_nobs, void *stream);
/* modl_image_grid_patches_masked_* at the origins of an index list instead of a grid (the masked twin of
 * modl_image_patches_*, modl/feature_extraction/image.py:54-63): window r sits at (d_idx3[r][0], d_idx3[r][1]) and spans
 * all channels - z must equal C (MODL_EINVAL otherwise) and the channel origin d_idx3[r][2] must be 0 (it lives on the
 * device and is not read).  d_mean[n][C], d_den[n][C], d_obs_out[n][x*y*C], d_nobs[n] as there.  The per-window device
 * code is the grid kernel's: a window at a grid origin gives that kernel's row, mean, den, mask row and count bit for bit. */
int modl_image_patches_masked_f32(const float *d_image, int64_t H, int64_t W, int64_t C, const int64_t *d_idx3, int64_t n,
                                  int x, int y, int z, int with_mean, int with_std, float *d_out, int64_t ldo,
                                  float *d_mean, float *d_den, const uint8_t *d_obs_image, uint8_t *d_obs_out,
                                  int32_t *d_nobs, void *stream);
int modl_image_patches_masked_f64(const double *d_image, int64_t H, int64_t W, int64_t C, const int64_t *d_idx3, int64_t n,
                                  int x, int y, int z, int with_mean, int with_std, double *d_out, int64_t ldo,
                                  double *d_mean, double *d_den, const uint8_t *d_obs_image, uint8_t *d_obs_out,
                                  int32_t *d_nobs, void *stream);
/* modl_image_overlap_add_* over the patches q of the pass with d_use[q] != 0 only; d_cnt[H][W] (int32, zeroed by the
 * caller before the first pass) counts them per pixel.  The same gather in grid order: sums and counts do not depend
 * on how the grid rows are cut into passes. */
int modl_image_overlap_add_weighted_f32(const float *d_patches, int64_t ldp, int64_t H, int64_t W, int64_t C, int x,
                                        int y, int si, int sj, int64_t row0, int64_t nrows, double *d_acc,
                                        const uint8_t *d_use, int32_t *d_cnt, void *stream);
int modl_image_overlap_add_weighted_f64(const double *d_patches, int64_t ldp, int64_t H, int64_t W, int64_t C, int x,
                                        int y, int si, int sj, int64_t row0, int64_t nrows, double *d_acc,
                                        const uint8_t *d_use, int32_t *d_cnt, void *stream);
/* d_image_out = d_acc / d_cnt where d_cnt > 0, d_image elsewhere; with keep_observed != 0 the observed elements
 * (d_obs_image != 0) take d_image's value unchanged.  H, W >= 1, 1 <= C <= 1024. */
int modl_image_inpaint_finish_f32(const double *d_acc, const int32_t *d_cnt, const float *d_image,
                                  const uint8_t *d_obs_image, int64_t H, int64_t W, int64_t C, int keep_observed,
                                  float *d_image_out, void *stream);
int modl_image_inpaint_finish_f64(const double *d_acc, const int32_t *d_cnt, const double *d_image,
                                  const uint8_t *d_obs_image, int64_t H, int64_t W, int64_t C, int keep_observed,
                                  double *d_image_out, void *stream);
/* The three sums of CodingMixin.score (dict_fact.py:108-114) on device-resident operands:
 * d_out3 = [ sum (X - code D)^2, sum |code|, sum code^2 ] (f64 accumulation, fixed order: run-to-run reproducible).
 * d_X[n][ldx], d_Dt[p][k], d_code[n][k]; scratch of modl_objective_workspace() bytes (any smaller size that holds at
 * least one row of X works too, in more passes). */
size_t modl_objective_workspace(int dtype, int64_t n, int64_t p);
int modl_objective_f32(const float *d_X, int64_t ldx, int64_t n, int64_t p, const float *d_Dt, int k, const float *d_code,
                       void *d_ws, size_t ws_bytes, double *d_out3, void *stream);
int modl_objective_f64(const double *d_X, int64_t ldx, int64_t n, int64_t p, const double *d_Dt, int k, const double *d_code,
                       void *d_ws, size_t ws_bytes, double *d_out3, void *stream);
/* The sums behind CodingMixin.score(X, mask) and held_out_error on rows with missing entries, in one pass over d_X and
 * the selection bytes.  d_X[n][ldx], d_sel[n][lds] (bytes), d_Dt[p][k], d_code[n][k], d_row_w[n] (f64; NULL = all ones).
 * res_ie = d_X[i][e] - sum_j d_code[i][j] d_Dt[e][j]: the product on the matrix cores in the dtype, the difference in
 * the dtype, the square and every sum in f64.  Entry (i, e) belongs to class c in {1, 2} when d_sel[i][e] == c; any
 * other byte selects nothing.  Per class  S_c = sum res^2,  W_c = sum_i w_i sum_e res^2,  N_c = the number of entries:
 *   d_out8 = [ S_1, W_1, N_1, S_2, W_2, N_2, sum |code|, sum code^2 ]     (the code norms over all n rows)
 * An entry of d_X that is not selected is dropped by a select and enters no arithmetic: NaN or Inf there leaves the eight
 * numbers unchanged bit for bit.  Nothing of size n x p is written; every workgroup leaves its partial sums in d_ws
 * (modl_masked_objective_workspace() bytes) and a last one-workgroup launch adds them in a fixed order: no atomics, the
 * same bits from run to run.  n == 0 gives eight zeros.  MODL_EINVAL before any device work: a NULL d_X, d_sel, d_Dt,
 * d_code, d_out8 or d_ws, n < 0, p < 1, k < 1 or k > MODL_MAX_COMPONENTS, ldx < p, lds < p (or more than 2^31 - 1 tiles
 * of 64 x 64); ws_bytes too small: MODL_ENOMEM. */
size_t modl_masked_objective_workspace(int dtype, int64_t n, int64_t p);
int modl_masked_objective_f32(const float *d_X, int64_t ldx, const uint8_t *d_sel, int64_t lds, int64_t n, int64_t p,
                              const float *d_Dt, int k, const float *d_code, const double *d_row_w, void *d_ws,
                              size_t ws_bytes, double *d_out8, void *stream);
int modl_masked_objective_f64(const double *d_X, int64_t ldx, const uint8_t *d_sel, int64_t lds, int64_t n, int64_t p,
                              const double *d_Dt, int k, const double *d_code, const double *d_row_w, void *d_ws,
                              size_t ws_bytes, double *d_out8, void *stream);
/* Rows completed by their reconstruction: d_out[i][e] = d_obs[i][e] != 0 ? d_X[i][e] : sum_j d_code[i][j] d_Dt[e][j]
 * (a select: observed entries carry the bits of d_X, d_X at unobserved positions is never used).  d_out[n][ldout] must
 * not overlap d_X.  One launch, no scratch.  The same checks: a NULL pointer, n < 0, p < 1, k out of range, ldx, ldo or
 * ldout below p -> MODL_EINVAL before any device work; n == 0 does nothing. */
int modl_impute_f32(const float *d_code, int64_t n, int k, const float *d_Dt, int64_t p, const float *d_X, int64_t ldx,
                    const uint8_t *d_obs, int64_t ldo, float *d_out, int64_t ldout, void *stream);
int modl_impute_f64(const double *d_code, int64_t n, int k, const double *d_Dt, int64_t p, const double *d_X, int64_t ldx,
                    const uint8_t *d_obs, int64_t ldo, double *d_out, int64_t ldout, void *stream);

/* Sparse codes as CSR (csrc/sparse_codes.hip; no counterpart in the reference).  A dense chunk d_code[b][ld] (row-major,
 * ld >= k; the padding columns k .. ld-1 are never read) is compacted in two calls.  An element is kept iff its bits with
 * the sign cleared are non-zero: `value != 0`, scipy's csr_matrix(dense) rule - NaN, +-inf and denormals kept, -0.0
 * dropped - decided on the bits, whatever the floating-point mode does with denormals.  No atomics: the result is a pure
 * function of the chunk.  All of these are asynchronous on `stream`.
 * modl_csr_compact_workspace(b): bytes of scratch of modl_csr_count_* for b rows (0 for b < 0). */
size_t modl_csr_compact_workspace(int64_t b);
/* Count + scan: d_indptr[0] = base, d_indptr[i + 1] = base + the number of kept elements of rows 0 .. i (b + 1 int64;
 * base: the non-zeros of the chunks before this one).  Four launches: a count per row (one wavefront per row), sums of
 * tiles of 1024 rows, a one-workgroup scan of the tile sums, a scan of every tile from its offset.  MODL_EINVAL before any
 * device work: a NULL d_code or d_indptr, b < 0 or b > 2^31 - 1, k < 1 or k > 2^31 - 1, ld < k, base < 0.  b == 0 does
 * nothing (nothing is written).  d_ws NULL or ws_bytes below modl_csr_compact_workspace(b): MODL_ENOMEM; no device:
 * MODL_ENOGPU. */
int modl_csr_count_f32(const float *d_code, int64_t ld, int64_t b, int64_t k, int64_t base, int64_t *d_indptr, void *d_ws,
                       size_t ws_bytes, void *stream);
int modl_csr_count_f64(const double *d_code, int64_t ld, int64_t b, int64_t k, int64_t base, int64_t *d_indptr, void *d_ws,
                       size_t ws_bytes, void *stream);
/* Fill: row i's kept elements go to the positions d_indptr[i] - base ... of d_indices (int32, the column) and d_data (the
 * value, bit for bit), in ascending column order.  d_indptr, base: what modl_csr_count_* made of the same chunk; nnz: the
 * length of d_indices and d_data, at least d_indptr[b] - base (a position outside [0, nnz) is never written).  One launch,
 * one wavefront per row, no scratch.  MODL_EINVAL before any device work: the cases of modl_csr_count_*, a NULL
 * d_indices or d_data, nnz < 0.  b == 0 or nnz == 0 does nothing.  No device: MODL_ENOGPU. */
int modl_csr_fill_f32(const float *d_code, int64_t ld, int64_t b, int64_t k, int64_t base, const int64_t *d_indptr,
                      int64_t nnz, int32_t *d_indices, float *d_data, void *stream);
int modl_csr_fill_f64(const double *d_code, int64_t ld, int64_t b, int64_t k, int64_t base, const int64_t *d_indptr,
                      int64_t nnz, int32_t *d_indices, double *d_data, void *stream);
/* modl_csr_decode_workspace(dtype, k, p): bytes of scratch of modl_csr_decode_* - the atom-major copy of the dictionary,
 * k * p elements (0 for bad arguments). */
size_t modl_csr_decode_workspace(int dtype, int64_t k, int64_t p);
/* CSR codes times the dictionary: d_out[i][e] = sum_j d_data[j] * d_Dt[e][d_indices[j]] over j = d_indptr[i] ..
 * d_indptr[i + 1] - 1 in stored order, one fma chain in the dtype per (i, e), for n rows and e < p (d_out[n][ldo], its
 * padding columns untouched).  Unsorted and repeated indices are legal, repeats add up; an empty row gives zeros.  The
 * order of a row's sum depends on that row alone: a row decodes to the same bits in any batch.  d_Dt[p][k] is first
 * transposed into d_ws (an atom's features side by side), then one launch: a wavefront per row and tile of 256 features.
 * Nothing out of range is dereferenced: an entry whose index is outside [0, k) contributes nothing, a row whose d_indptr
 * pair is negative, decreasing or beyond nnz (the length of d_indices and d_data) contributes nothing, and either sets
 * *d_status (int32, may be NULL; zeroed by the call) to 1.  MODL_EINVAL before any device work: a NULL pointer (d_status
 * and d_ws apart), nnz < 0, n < 0, k < 1 or k > 2^31 - 1, p < 1 or p > 32 * 65535 (the transpose's grid), ldo < p.
 * n == 0 does nothing.  d_ws NULL or ws_bytes below modl_csr_decode_workspace(...): MODL_ENOMEM; no device:
 * MODL_ENOGPU. */
int modl_csr_decode_f32(const int64_t *d_indptr, const int32_t *d_indices, const float *d_data, int64_t nnz, int64_t n,
                        int64_t k, const float *d_Dt, int64_t p, float *d_out, int64_t ldo, int32_t *d_status, void *d_ws,
                        size_t ws_bytes, void *stream);
int modl_csr_decode_f64(const int64_t *d_indptr, const int32_t *d_indices, const double *d_data, int64_t nnz, int64_t n,
                        int64_t k, const double *d_Dt, int64_t p, double *d_out, int64_t ldo, int32_t *d_status, void *d_ws,
                        size_t ws_bytes, void *stream);

/* Signal cleaning of a record (csrc/clean.hip; the arithmetic of nilearn.signal.clean that the
 * reference's masker applies to every record, modl/decomposition/fmri.py:525-526).  d_X[T][ldx] holds T time points of V
 * voxels (ldx >= V, the padding is never read); every column x is treated on its own:
 *   r = x - Q (Q^T x),    out = standardize ? r sqrt(T) / |r| : r
 * with d_Q[T][q] (f64, row-major) a basis with orthonormal columns that the caller builds (modl_amd/signal.py:
 * cleaning_basis - constant, linear ramp, confounds).  With standardize a column is FLAT when |r|^2 <= (q T eps64)^2 |x|^2
 * (the worst-case f64 rounding of the projection) and comes out as exact zeros; without it nothing is zeroed.  The
 * coefficients Q^T x, |x|^2 and |r|^2 are summed in f64 for both dtypes, the residual is formed in f64 and rounded once on
 * store.  The order of every sum depends on T alone - not on V, on the column's place in the call, on ldx / ldo or on
 * d_dst_row - so a column has the same bits wherever it stands and from run to run; a column that holds a NaN or Inf (|x|^2 not
 * finite in f64) comes out as NaN throughout and touches no other column.
 * d_dst_row (int64[T], may be NULL): cleaned row t is written to row d_dst_row[t] of d_out[T][ldo]; it has to be a
 * permutation of 0 .. T-1, which the CALLER checks (an entry outside 0 .. T-1 is skipped on the device, nothing more).
 * d_out == d_X (in place) is legal with d_dst_row == NULL and ldo == ldx only; any other overlap of the address ranges
 * of d_X[T][ldx] and d_out[T][ldo] (d_out shifted by rows, a permutation into the input) is refused.  Asynchronous on `stream`: a copy of the
 * basis into d_ws and one launch, no atomics.
 * MODL_EINVAL before any device work: a NULL d_X / d_Q / d_out, T < 1, V < 1, q outside 1 .. min(T, 64), ldx < V,
 * ldo < V, the in-place / overlap rule.  d_ws NULL or ws_bytes below modl_clean_workspace(...): MODL_ENOMEM; no device: MODL_ENOGPU.
 * modl_clean_max_regressors(): 64.  modl_clean_workspace: bytes of scratch (0 for bad arguments). */
int modl_clean_max_regressors(void);
size_t modl_clean_workspace(int dtype, int64_t T, int64_t V, int q);
int modl_clean_f32(const float *d_X, int64_t ldx, int64_t T, int64_t V, const double *d_Q, int q, int standardize,
                   const int64_t *d_dst_row, float *d_out, int64_t ldo, void *d_ws, size_t ws_bytes, void *stream);
int modl_clean_f64(const double *d_X, int64_t ldx, int64_t T, int64_t V, const double *d_Q, int q, int standardize,
                   const int64_t *d_dst_row, double *d_out, int64_t ldo, void *d_ws, size_t ws_bytes, void *stream);

/* Zero-phase Butterworth filtering of a record (csrc/filtfilt.hip; the low_pass / high_pass of
 * nilearn.signal.clean that the reference's masker takes, modl/decomposition/fmri.py:281-299).  d_X[T][ldx] holds T time
 * points of V voxels (ldx >= V, the padding is never read); every column x is treated on its own:
 *   out[d_dst_row[t]] = filtfilt(b, a, detrend ? x - line(x) : x)[t]
 * which is scipy.signal.filtfilt(b, a, x) with its defaults: padlen = 3 n_taps, odd extension at both ends (left
 * 2 x[0] - x[padlen .. 1], right 2 x[T-1] - x[T-2 .. T-padlen-1]), a forward pass in direct form II transposed started
 * from zi ext[0], the same over the reversed forward output started from zi times its first element, the pads trimmed.
 * line(x) is the least-squares line of the column (mean and ramp), summed in f64 in ascending t.
 * b, a (n_taps each, a[0] == 1) and zi (n_taps - 1; scipy.signal.lfilter_zi(b, a)) are HOST pointers, f64: they travel as
 * kernel arguments (modl_amd/signal.py: butterworth_coefficients builds them with scipy.signal.butter).  The filter state
 * is kept in f64 for both dtypes, the forward output crosses the workspace as f64, the result is rounded once on store.
 * The arithmetic order of a column depends on T and the taps alone - not on V, on the column's place in the call, on ldx /
 * ldo or on d_dst_row - so a column has the same bits wherever it stands and from run to run.  A column that holds a NaN
 * or Inf comes out as NaN throughout and touches no other column; an all-zero column comes out as exact zeros.
 * d_dst_row (int64[T], device, may be NULL): filtered row t is written to row d_dst_row[t] of d_out[T][ldo]; it has to be
 * a permutation of 0 .. T-1, which the CALLER checks (an entry outside 0 .. T-1 is skipped on the device, nothing more).
 * d_out == d_X (in place) is legal with d_dst_row == NULL and ldo == ldx only; any other overlap of the address ranges of
 * d_X[T][ldx] and d_out[T][ldo] is refused.  Asynchronous on `stream`: one launch, no atomics.
 * MODL_EINVAL before any device work: a NULL d_X / d_out / b / a / zi, n_taps outside 2 .. modl_filtfilt_max_taps() = 12,
 * a[0] != 1, a non-finite coefficient, T <= 3 n_taps, V < 1, ldx < V, ldo < V, the in-place / overlap rule.  d_ws NULL or
 * ws_bytes below modl_filtfilt_workspace(...) = (T + 3 n_taps) V 8 bytes: MODL_ENOMEM; no device: MODL_ENOGPU.
 * modl_filtfilt_workspace: bytes of scratch (0 for bad arguments). */
int modl_filtfilt_max_taps(void);
size_t modl_filtfilt_workspace(int dtype, int64_t T, int64_t V, int n_taps);
int modl_filtfilt_f32(const float *d_X, int64_t ldx, int64_t T, int64_t V, const double *b, const double *a,
                      const double *zi, int n_taps, int detrend, const int64_t *d_dst_row, float *d_out, int64_t ldo,
                      void *d_ws, size_t ws_bytes, void *stream);
int modl_filtfilt_f64(const double *d_X, int64_t ldx, int64_t T, int64_t V, const double *b, const double *a,
                      const double *zi, int n_taps, int detrend, const int64_t *d_dst_row, double *d_out, int64_t ldo,
                      void *d_ws, size_t ws_bytes, void *stream);

/* Spatial smoothing and masking of a volume (csrc/masker.hip; what the reference's masker does to
 * a 4-D image before signal.clean: nilearn's _smooth_array, i.e. scipy.ndimage.gaussian_filter1d per spatial axis, then the
 * mask).  d_vol holds T frames of a contiguous box [n0][n1][n2] (n2 fastest), frame t at d_vol + t * frame_stride
 * (frame_stride >= n0 n1 n2, in elements; every offset is 64-bit).  Per frame:
 *   1. every non-finite element counts as 0;
 *   2. per axis a with r_a > 0 the frame is correlated with the 2 r_a + 1 weights w_a (HOST, f64, non-negative, sum 1),
 *      boundary 'reflect' of scipy (d c b a | a b c d | d c b a, period 2 n_a: a short axis is reflected repeatedly);
 *      r_a == 0 or w_a == NULL leaves the axis untouched, bit for bit;
 *   3. d_out[dst(t)][d_col[v]] = the smoothed value of voxel v, for every v with d_col[v] >= 0.
 * d_col[n0][n1][n2] (int32) is the output column of a voxel, -1 outside the mask; the caller builds it once per mask, its
 * values lie in 0 .. V-1 and carry the voxel order (the kernel knows three axes of a box and nothing of x / y / z).
 * d_dst_row (int64[T], may be NULL): frame t goes to row d_dst_row[t] of d_out[T][ldo]; the CALLER checks that it is a
 * permutation, an entry outside 0 .. T-1 is skipped on the device.
 * Every axis sum runs in f64 in ascending tap order for both dtypes and is rounded once to the dtype; the bits of an
 * element depend on the volume and the weights alone - not on the mask, V, the voxel's place in its tile, T or d_dst_row.
 * One launch (after the copy of the weights into d_ws), no intermediate volume: a workgroup smooths one tile of one frame
 * in LDS, and a tile without a masked voxel reads no volume data.  All radii 0: the plain masking gather of 1 and 3,
 * exact.  Asynchronous on `stream`, no atomics.
 * MODL_EINVAL before any device work: a NULL d_vol / d_col / d_out, T / n_a / V < 1, n0 n1 n2 > INT32_MAX, V > n0 n1 n2,
 * frame_stride < n0 n1 n2, ldo < V, a radius outside 0 .. modl_smooth_max_radius() = 8, a non-finite or negative weight,
 * weights whose sum differs from 1 by more than 1e-12, any overlap of d_vol and d_out.  d_ws NULL or ws_bytes below
 * modl_smooth_mask_workspace(...): MODL_ENOMEM; no device: MODL_ENOGPU.  modl_smooth_mask_workspace returns 0 for bad
 * arguments.  modl_smooth_tile: the tile (3 ints) that the kernel uses for these radii and this dtype. */
int modl_smooth_max_radius(void);
int modl_smooth_tile(int dtype, int r0, int r1, int r2, int *tile);
size_t modl_smooth_mask_workspace(int dtype, int64_t T, int64_t n0, int64_t n1, int64_t n2, int r0, int r1, int r2);
int modl_smooth_mask_f32(const float *d_vol, int64_t frame_stride, int64_t T, int64_t n0, int64_t n1, int64_t n2,
                         const double *w0, int r0, const double *w1, int r1, const double *w2, int r2, const int32_t *d_col,
                         int64_t V, const int64_t *d_dst_row, float *d_out, int64_t ldo, void *d_ws, size_t ws_bytes,
                         void *stream);
int modl_smooth_mask_f64(const double *d_vol, int64_t frame_stride, int64_t T, int64_t n0, int64_t n1, int64_t n2,
                         const double *w0, int r0, const double *w1, int r1, const double *w2, int r2, const int32_t *d_col,
                         int64_t V, const int64_t *d_dst_row, double *d_out, int64_t ldo, void *d_ws, size_t ws_bytes,
                         void *stream);
/* The inverse of the masking: d_out[n][n0 n1 n2] is zero-filled by the call, then d_out[i][d_vox[c]] = d_rows[i][c] for the
 * V flat voxel indices d_vox (int64, distinct; an index outside the box is skipped).  Asynchronous on `stream`.
 * MODL_EINVAL: a NULL pointer, n / V / n_a < 1, V > n0 n1 n2, ldr < V, any overlap of d_rows and d_out; MODL_ENOGPU. */
int modl_unmask_f32(const float *d_rows, int64_t ldr, int64_t n, int64_t V, const int64_t *d_vox, int64_t n0, int64_t n1,
                    int64_t n2, float *d_out, void *stream);
int modl_unmask_f64(const double *d_rows, int64_t ldr, int64_t n, int64_t V, const int64_t *d_vox, int64_t n0, int64_t n1,
                    int64_t n2, double *d_out, void *stream);

/* Computing a mask (csrc/compute_mask.hip): the steps of nilearn's compute_epi_mask /
 * compute_background_mask that touch every voxel.  A mask on the device is uint8[n0][n1][n2], n2 fastest (the frame order
 * (Z, Y, X) of modl_smooth_mask); any nonzero byte reads as true, the calls write 0 or 1.  n0 n1 n2 <= INT32_MAX.
 * All calls are asynchronous on `stream`; argument checks return MODL_EINVAL before any device work; a NULL or short
 * workspace is MODL_ENOMEM; no device: MODL_ENOGPU.  Workspace and outputs are written only where the call says.
 *
 * modl_frame_mean: d_mean[v] = (sum over t of d_frames[t * ld_frame + v]) / T for v < n.  The sum runs in f64 in ascending
 * t inside one thread, the division is in f64, the result is rounded once to the dtype; plain IEEE, so NaN and inf
 * propagate; with zero_nonfinite = 1 a non-finite RESULT (after the rounding) is stored as 0.  One thread owns 8 bytes
 * of neighbouring voxels (two f32, one f64) and loads them with one instruction per frame, 512 contiguous bytes per
 * wavefront, whatever the alignment of d_frames and ld_frame (frames of an odd box start anywhere); a last single f32
 * voxel loads on its own.  No atomics, no workspace.
 * MODL_EINVAL: a NULL pointer, T / n < 1, ld_frame < n, zero_nonfinite not 0 / 1, a pointer that is not aligned to an
 * element, any overlap of d_frames and d_mean. */
int modl_frame_mean_f32(const float *d_frames, int64_t ld_frame, int64_t T, int64_t n, int zero_nonfinite, float *d_mean,
                        void *stream);
int modl_frame_mean_f64(const double *d_frames, int64_t ld_frame, int64_t T, int64_t n, int zero_nonfinite, double *d_mean,
                        void *stream);
/* scipy.ndimage.binary_erosion (dilate = 0) / binary_dilation (dilate = 1) with the default cross structure,
 * border_value = 0 and `iterations` >= 1 passes: a voxel survives erosion iff every locus within L1 distance `iterations`
 * lies inside the box and is true, it is set by dilation iff a true voxel lies within that distance.  One launch per
 * pass, alternating between d_ws and d_out; passes that can change nothing any more (erosion past (shortest axis + 1) / 2,
 * dilation past n0 + n1 + n2) are not launched, so any `iterations` is legal.  d_in is not written.
 * d_ws: modl_morph_workspace(n0, n1, n2, iterations) bytes (0 for bad arguments).
 * MODL_EINVAL: a NULL d_in / d_out, an extent < 1, a box above INT32_MAX, iterations < 1, dilate not 0 / 1, any overlap of
 * d_in, d_out and d_ws (d_out aliasing d_in included). */
size_t modl_morph_workspace(int64_t n0, int64_t n1, int64_t n2, int64_t iterations);
int modl_binary_morph(const uint8_t *d_in, int64_t n0, int64_t n1, int64_t n2, int64_t iterations, int dilate, uint8_t *d_out,
                      void *d_ws, size_t ws_bytes, void *stream);
/* 6-connected components (scipy.ndimage.label with the default structure) by union-find in global memory: labels within
 * tiles of modl_label_tile() voxels in LDS, a merge across the tile faces (atomicMin links, agent-scope atomic reads, no
 * workgroup waits for another), a flattening pass.  Every loop descends a chain of strictly decreasing indices, so it is
 * bounded by the box.  d_root (int32[n0][n1][n2]): for a true voxel THE SMALLEST FLAT MEMORY INDEX (i0 n1 + i1) n2 + i2 OF
 * ITS COMPONENT - the same for exactly the voxels of one component; -1 for a false voxel.  The result depends on the
 * mask alone.
 * modl_largest_component: d_out = the component with the most voxels; among components of equal size the one whose first
 * voxel comes first in the C order of the caller's (X, Y, Z) = (n2, n1, n0) array, index (i2 n1 + i1) n0 + i0 - that is
 * labels == np.bincount(labels.ravel())[1:].argmax() + 1 of scipy's labels of the (X, Y, Z) array.  d_info (int64[3], device):
 * the number of components, the winner's size, the winner's first voxel as that C index.  No true voxel: zeros in d_info,
 * an all-false d_out, MODL_OK.  Sizes are counted with one integer add per wavefront and distinct root; all atomics are
 * integer min / max / add, so the bits do not depend on the order of arrival.
 * d_ws: modl_label_workspace(n0, n1, n2) bytes for both calls (0 for bad arguments).
 * MODL_EINVAL: a NULL pointer, an extent < 1, a box above INT32_MAX, n0 or n1 above 65535 tiles, any overlap of the
 * arrays. */
int modl_label_tile(int *tile);
size_t modl_label_workspace(int64_t n0, int64_t n1, int64_t n2);
int modl_label_components(const uint8_t *d_mask, int64_t n0, int64_t n1, int64_t n2, int32_t *d_root, void *d_ws, size_t ws_bytes,
                          void *stream);
int modl_largest_component(const uint8_t *d_mask, int64_t n0, int64_t n1, int64_t n2, uint8_t *d_out, int64_t *d_info, void *d_ws,
                           size_t ws_bytes, void *stream);

/* Connected regions of many maps at once (csrc/regions.hip): the device half of nilearn's
 * connected_regions / RegionExtractor.  d_rows holds M maps as rows of V elements (leading dimension ldr >= V), one element
 * per voxel of a mask; d_col (int32[n0][n1][n2], n2 fastest: the `col` of modl_smooth_mask) is the column of a box voxel or
 * -1 (an entry outside 0 .. V-1 reads as -1; the CALLER sees to it that the columns 0 .. V-1 appear once each).
 * modl_region_labels: an element v is foreground iff it is finite, v != 0 and |v| >= cutoff (compared in the dtype).  The
 * foreground of every map is split into its 6-connected components in the box (scipy.ndimage.label, default structure;
 * maps never interact, columns that are neighbours in the row but not in the box are not connected); a component of n voxels
 * is kept iff n > min_voxels; the kept ones are numbered 1, 2, .. within their map in scipy's order, by the component's
 * first voxel in the C order of the caller's (X, Y, Z) = (n2, n1, n0) array, index (i2 n1 + i1) n0 + i0.
 *   d_labels (int32, M rows of V, ldl >= V)   0, or the number of the element's region within its map;
 *   d_counts (int32[M])                        the regions of every map;
 *   d_sizes (int32[M][size_cap], may be NULL with size_cap = 0)   d_sizes[m][j] = the voxels of region j + 1 of map m for
 *                                              j < min(d_counts[m], size_cap); the other entries are not written.
 *                                              size_cap = V / (max(min_voxels, 0) + 1) holds every region.
 * The chunk of M maps is labelled by one set of launches with the map on a grid axis: the predicate is evaluated from
 * d_rows[m][d_col[g]] inside the tile kernel (no volume is unmasked, no byte mask written), then the union-find of
 * modl_label_components (tiles in LDS, merge across faces, flatten), sizes and first voxels with one integer add and one
 * integer min per wavefront and distinct root, and the numbering by a prefix sum over flags at the first voxels.  All
 * atomics are integer min / add: the same input gives the same bits.  d_rows and d_col are not written.
 * d_ws: modl_region_labels_workspace(M, n0, n1, n2) bytes, 16 M n0 n1 n2 and a little (0 for bad arguments);
 * modl_region_max_maps: the largest M <= 65535 whose workspace fits budget_bytes (0: not even one map, or a bad box).
 * modl_region_gather: d_regions (R rows of V, ldo >= V) from the labels of M maps and d_offsets (int64[M + 1], device,
 * ascending, d_offsets[0] = 0, d_offsets[M] = R: the first region row of every map): row d_offsets[m] + j holds d_rows[m][c]
 * where d_labels[m][c] == j + 1, bit for bit, and 0 elsewhere.  One grid row per region, 16 bytes of neighbouring columns
 * per thread, no atomics, no workspace.  R == 0 does nothing.
 * All calls are asynchronous on `stream`.  MODL_EINVAL before any device work: a NULL pointer, M < 1 or M > 65535 (labels),
 * V < 1, V above the box, a leading dimension below V, an extent < 1, a box above INT32_MAX elements or n0 above 65535
 * tiles, a cutoff that is negative or NaN, size_cap < 0, R < 0, a pointer that is not aligned to an element (gather), any
 * overlap of an output with an input, another output or the workspace.  d_ws NULL or short: MODL_ENOMEM; no device:
 * MODL_ENOGPU. */
size_t modl_region_labels_workspace(int64_t M, int64_t n0, int64_t n1, int64_t n2);
int64_t modl_region_max_maps(int64_t n0, int64_t n1, int64_t n2, size_t budget_bytes);
int modl_region_labels_f32(const float *d_rows, int64_t ldr, int64_t M, int64_t V, const int32_t *d_col, int64_t n0, int64_t n1,
                           int64_t n2, float cutoff, int64_t min_voxels, int32_t *d_labels, int64_t ldl, int32_t *d_counts,
                           int32_t *d_sizes, int64_t size_cap, void *d_ws, size_t ws_bytes, void *stream);
int modl_region_labels_f64(const double *d_rows, int64_t ldr, int64_t M, int64_t V, const int32_t *d_col, int64_t n0, int64_t n1,
                           int64_t n2, double cutoff, int64_t min_voxels, int32_t *d_labels, int64_t ldl, int32_t *d_counts,
                           int32_t *d_sizes, int64_t size_cap, void *d_ws, size_t ws_bytes, void *stream);
int modl_region_gather_f32(const float *d_rows, int64_t ldr, int64_t M, int64_t V, const int32_t *d_labels, int64_t ldl,
                           const int64_t *d_offsets, int64_t R, float *d_regions, int64_t ldo, void *stream);
int modl_region_gather_f64(const double *d_rows, int64_t ldr, int64_t M, int64_t V, const int32_t *d_labels, int64_t ldl,
                           const int64_t *d_offsets, int64_t R, double *d_regions, int64_t ldo, void *stream);

/* Resampling of a volume onto another grid (csrc/resample.hip; the masker's first step: nilearn's
 * resample_img, i.e. per frame scipy.ndimage.affine_transform(frame, A, offset=b, output_shape, order, mode='constant',
 * cval=fill)).  d_vol as for modl_smooth_mask: T frames of a box [n0][n1][n2], n2 fastest, frame_stride >= n0 n1 n2.
 * A (9 doubles, row-major) and b (3 doubles) are HOST arrays IN THIS AXIS ORDER: the locus o = (o0, o1, o2) of the target
 * box [m0][m1][m2] reads the source at x_a = b_a + sum_j A[a][j] o_j, formed in f64 with scipy's bits.  (A caller whose
 * arrays are (X, Y, Z) hands over the reversed box, P A P and P b, P the reversal of the axes.)
 *   - non-finite source elements count as 0;
 *   - a locus with any x_a < 0 or x_a > n_a - 1 receives `fill`;
 *   - order 0: the element at floor(x + 0.5), bit for bit;
 *   - order 1: taps floor(x), floor(x) + 1 per axis, weights 1 - t and t;
 *   - order 3: the frame is replaced by its cubic B-spline coefficients first (modl_spline_prefilter: scipy's
 *     spline_filter(order=3, mode='mirror'), separable, state in f64, one rounding to the dtype per axis), then four taps
 *     per axis at floor(x) - 1 .. floor(x) + 2 with the cubic B-spline weights of t;
 *   - tap indices outside 0 .. n - 1 are mirrored (d c b | a b c d | c b a);
 *   - A exactly the identity and b integer: the shifted crop, through the order-0 path whatever `order` says.
 * The taps are summed along n2, then n1, then n0, in f64 for both dtypes, and rounded once.
 * Box mode (d_vox NULL; V is not looked at): d_out holds T frames [m0][m1][m2] with the frame stride ldo >= m0 m1 m2.
 * Rows mode: d_vox (int64[V], device) lists loci as flat indices with AXIS 0 FASTEST, (o2 m1 + o1) m0 + o0 - the C index
 * in the caller's reversed box, the list that modl_unmask takes; locus c goes to d_out[dst(t)][c], ldo >= V; an index
 * outside the box is skipped.  The value of a locus is the same bits in both modes.  d_dst_row as for modl_smooth_mask.
 * d_order (int64[V], device, may be NULL; rows mode only): thread i of the launch takes column d_order[i] (an entry outside
 * 0 .. V-1 is skipped; the CALLER checks that it is a permutation).  It changes no bit of the result, only which loci a
 * wavefront works on together: with the columns sorted by (o0, o1, o2) - np.argsort of the loci's flat indices with axis
 * 2 fastest - neighbouring threads read neighbouring source elements, as they do in box mode.
 * Order 3 needs d_ws of modl_resample_workspace(dtype, T, n0, n1, n2, 3) bytes: the coefficients and the f64 values of
 * the causal walk, T n0 n1 n2 (sizeof(dtype) + 8) bytes (the caller bounds it by calling with chunks of frames); orders
 * 0 and 1 need none, the function returns 0 for them and for bad arguments.  Asynchronous on `stream`, no atomics.
 * MODL_EINVAL before any device work: a NULL d_vol / A / b / d_out, T or an extent < 1, a box above INT32_MAX elements,
 * a non-finite A, b or fill, an order other than 0, 1, 3, V < 1 or V > m0 m1 m2 or ldo < V (rows), ldo < m0 m1 m2 (box),
 * frame_stride < n0 n1 n2, any overlap of d_vol, d_out and d_ws.  Order 3 with d_ws NULL or ws_bytes too small:
 * MODL_ENOMEM; no device: MODL_ENOGPU.
 * modl_spline_prefilter: the coefficients alone, into d_coef with its own frame stride coef_stride >= n0 n1 n2; d_ws as
 * for order 3.  modl_resample_lds_line(): the longest n2 whose lines the prefilter stages in LDS (longer ones are walked
 * in global memory); modl_resample_frames(): the frames one thread of the gather takes, its grid has ceil(T / that) rows. */
int modl_resample_lds_line(void);
int modl_resample_frames(void);
size_t modl_resample_workspace(int dtype, int64_t T, int64_t n0, int64_t n1, int64_t n2, int order);
int modl_spline_prefilter_f32(const float *d_vol, int64_t frame_stride, int64_t T, int64_t n0, int64_t n1, int64_t n2,
                              float *d_coef, int64_t coef_stride, void *d_ws, size_t ws_bytes, void *stream);
int modl_spline_prefilter_f64(const double *d_vol, int64_t frame_stride, int64_t T, int64_t n0, int64_t n1, int64_t n2,
                              double *d_coef, int64_t coef_stride, void *d_ws, size_t ws_bytes, void *stream);
int modl_resample_f32(const float *d_vol, int64_t frame_stride, int64_t T, int64_t n0, int64_t n1, int64_t n2, const double *A,
                      const double *b, int order, double fill, int64_t m0, int64_t m1, int64_t m2, const int64_t *d_vox, int64_t V,
                      const int64_t *d_order, const int64_t *d_dst_row, float *d_out, int64_t ldo, void *d_ws, size_t ws_bytes,
                      void *stream);
int modl_resample_f64(const double *d_vol, int64_t frame_stride, int64_t T, int64_t n0, int64_t n1, int64_t n2, const double *A,
                      const double *b, int order, double fill, int64_t m0, int64_t m1, int64_t m2, const int64_t *d_vox, int64_t V,
                      const int64_t *d_order, const int64_t *d_dst_row, double *d_out, int64_t ldo, void *d_ws, size_t ws_bytes,
                      void *stream);

/* Amari discrepancy between dictionaries (modl/decomposition/stability.py:7-31: amari_discrepency,
 * mean_amari_discrepency).  For the n dictionaries h_d_dicts[i] (device, row-major k_i x p, atoms in rows), every pair
 * a < b in the reference's generator order (a outer, b inner) gets
 *   C[i][j] = (D_a[i] . D_b[j]) / ||D_a[i]|| / ||D_b[j]||,
 *   d_pair[q] = 0.5 * (mean_j (1 - max_i C[i][j]) + mean_i (1 - max_j C[i][j]))     (n (n - 1) / 2 doubles).
 * The maxima are signed and propagate NaN as ndarray.max does (a zero atom gives NaN).  d_rowmax (may be NULL) receives
 * max_j C[i][j] of every pair, concatenated in pair order (sum over pairs of k_a values), d_colmax (may be NULL)
 * max_i C[i][j] (sum of k_b values).  Norms are accumulated in f64, the products run on the matrix cores in the
 * dtype, the means in f64; no atomics: run-to-run bit-identical.  `launches` (may be NULL) receives the number of
 * kernels launched (3, or 4 when the products are split along p), independent of n.  The call returns after its
 * small host tables have reached the device; the kernels are asynchronous.  Arguments are checked before any device
 * work: n < 2, a k_i <= 0, p <= 0 or a NULL pointer -> MODL_EINVAL; d_ws NULL or smaller than
 * modl_amari_workspace() -> MODL_ENOMEM; no device -> MODL_ENOGPU.  modl_amari_workspace returns 0 for bad
 * arguments. */
size_t modl_amari_workspace(int dtype, int n, const int64_t *h_k, int64_t p);
int modl_amari_f32(const float *const *h_d_dicts, const int64_t *h_k, int n, int64_t p, double *d_pair, float *d_rowmax,
                   float *d_colmax, void *d_ws, size_t ws_bytes, void *stream, int *launches);
int modl_amari_f64(const double *const *h_d_dicts, const int64_t *h_k, int n, int64_t p, double *d_pair, double *d_rowmax,
                   double *d_colmax, void *d_ws, size_t ws_bytes, void *stream, int *launches);

/* One sweep of symmetric FastICA for many restarts at once (csrc/ica.hip), all in f64.
 * d_X1: k rows of V whitened values, ldx >= V.  d_W: unmixing matrices, each k x k row-major, one after the other; d_active:
 * R int32 indices of the matrices to sweep (device; every entry indexes a matrix that d_W holds, and no entry repeats).
 * For each listed restart r, with y = W_r x per voxel:
 *   d_M[r]  (k x k) = (1 / V) sum_v g(y_v) x_v^T,        d_gp[r] (k) = (1 / V) sum_v g'(y_{i, v});
 * the slots of d_M and d_gp of restarts that are not listed are not written.  fun: 0 cube (g = y^3, g' = 3 y^2), 1 logcosh
 * (g = tanh(alpha y), g' = alpha (1 - g^2)), 2 exp (g = y exp(-y^2 / 2), g' = (1 - y^2) exp(-y^2 / 2)); alpha is read by
 * logcosh alone.  The k x V sources stay in registers between the two matrix-core products; the sums are per-workgroup
 * partials in d_ws added in a fixed order, no floating-point atomics: the same input gives the same bits, and the voxel
 * chunking depends on V alone, so a restart's outputs are the same bits whichever other restarts are listed with it.  Nothing is read
 * beyond column V of a row.  Asynchronous on `stream`.  MODL_EINVAL before any device work: a NULL pointer (d_ws apart), k < 1
 * or k > modl_ica_max_components() = 128, V < 1, R < 1 or R > 65535, ldx < V, an unknown fun, a pointer that is not aligned
 * to its element.  d_ws NULL or ws_bytes below modl_ica_sweep_workspace(V, k, R) (0 for bad arguments): MODL_ENOMEM; no
 * device: MODL_ENOGPU. */
int modl_ica_max_components(void);
size_t modl_ica_sweep_workspace(int64_t V, int k, int R);
int modl_ica_sweep_f64(const double *d_X1, int64_t ldx, int64_t V, int k, const double *d_W, const int32_t *d_active, int R, int fun,
                       double alpha, double *d_M, double *d_gp, void *d_ws, size_t ws_bytes, void *stream);

/* Functional connectivity (csrc/connectivity.hip).
 *
 * modl_conn_covariance_*: the covariance matrices of S records of R region signals in one call.  d_X: the records stacked,
 * h_offsets[S] rows of R values, ldx >= R; record s is rows h_offsets[s] .. h_offsets[s + 1] - 1 (T_s of them).  h_offsets is
 * HOST memory (S + 1 int64): it is checked here and copied into the workspace, which is what the kernels read.  Per record,
 * all in f64 (f32 is converted on load: an f32 record and its f64 copy give the same bits), with Xc = X - column means (formed
 * first, in a fixed order; the centred values enter the product, there is no raw-moment correction), E = Xc^T Xc / T, p = R:
 *   estimator 0 (empirical):   cov = E, shrinkage 0;
 *   estimator 1 (Ledoit-Wolf): mu = trace(E) / p, delta_ = sum_ij (Xc^T Xc)_ij^2 / T^2, beta_ = sum_t (sum_i Xc_ti^2)^2,
 *                              beta = min((beta_ / T - delta_) / (p T), delta), delta = (delta_ - 2 mu trace(E) + p mu^2) / p,
 *                              shrinkage = beta == 0 ? 0 : beta / delta, cov = (1 - shrinkage) E + shrinkage mu I
 *                              (sklearn.covariance.LedoitWolf; R = 1: shrinkage 0, as sklearn answers);
 *   output 0: d_cov[s] (R x R row-major, one after the other) = cov; output 1: cov_ij / sqrt(cov_ii cov_jj), diagonal exactly 1.
 * d_shrinkage: S doubles.  The product runs on v_mfma_f64_16x16x4_f64, one workgroup per record and 64 x 64 block of the upper
 * triangle over the whole T of the record; the lower triangle is mirrored, so the output is exactly symmetric.  Partial sums
 * are added in a fixed order, no floating-point atomics: the same input gives the same bits, and a record's bits do not depend
 * on which other records are in the call nor on their order.  Nothing is read beyond column R of a row.  Asynchronous on
 * `stream` once the offsets have been handed to the copy.  MODL_EINVAL before any device work: a NULL pointer (d_ws apart),
 * R < 1 or R > modl_conn_max_regions() = 512 (8 x 8 blocks of 64; the finishing kernel keeps a record's diagonal in LDS),
 * S < 1 or S > 65535, h_offsets[0] < 0, offsets not increasing by at least 2 (a record needs two time points), ldx < R, an
 * unknown estimator or output, a pointer that is not aligned to its element.  d_ws NULL or ws_bytes below
 * modl_conn_covariance_workspace(S, R) (0 for bad arguments): MODL_ENOMEM; no device: MODL_ENOGPU.
 *
 * modl_conn_seed_maps_*: the seed-to-voxel correlation maps of one record.  d_X: T rows of V values, ldx >= V; d_seeds: T rows
 * of R PREPARED seeds, contiguous (every column centred and of unit 2-norm, in the record's dtype); d_out: R rows of V, ldo >= V:
 *   d_out[r][v] = clip((sum_t seeds[t][r] X[t][v]) / sqrt(ss_v), -1, 1),   ss_v = sum_t x_tv^2 - (sum_t x_tv)^2 / T,
 * both sums of ss_v in f64, accumulated while X is staged for the product; a voxel with ss_v <= 8 T 2^-53 sum_t x_tv^2 (constant
 * to rounding) gives an exact 0.  The product runs on the matrix cores in the record's dtype (f32: exact FMA chains, t
 * ascending), one workgroup per 64 voxels over the whole T, no K split: deterministic by construction.  For R <= 128 X is read
 * once; beyond, the workgroup's block of X is re-read (from the caches) once per further 128 seeds.  Nothing is read or written
 * beyond column V of a row.  MODL_EINVAL: a NULL pointer, R < 1 or R > modl_conn_max_regions(), T < 2, V < 1, ldx < V, ldo < V,
 * a pointer that is not aligned to its element; no device: MODL_ENOGPU. */
int modl_conn_max_regions(void);
size_t modl_conn_covariance_workspace(int S, int R);
int modl_conn_covariance_f32(const float *d_X, int64_t ldx, const int64_t *h_offsets, int S, int R, int estimator, int output,
                             double *d_cov, double *d_shrinkage, void *d_ws, size_t ws_bytes, void *stream);
int modl_conn_covariance_f64(const double *d_X, int64_t ldx, const int64_t *h_offsets, int S, int R, int estimator, int output,
                             double *d_cov, double *d_shrinkage, void *d_ws, size_t ws_bytes, void *stream);
int modl_conn_seed_maps_f32(const float *d_X, int64_t ldx, int64_t T, int64_t V, const float *d_seeds, int R, float *d_out, int64_t ldo,
                            void *stream);
int modl_conn_seed_maps_f64(const double *d_X, int64_t ldx, int64_t T, int64_t V, const double *d_seeds, int R, double *d_out, int64_t ldo,
                            void *stream);

/* Hard parcellation (csrc/kmeans.hip): the assignment step of Lloyd's k-means for many centre sets at
 * once, and segmented sums over voxels grouped by label.  All calls are asynchronous on `stream`.
 *
 * modl_kmeans_assign_f64.  d_X: d rows of V doubles, ldx >= V.  d_C: n_sets centre sets, each K x d row-major, one after the
 * other; d_active: R int32 indices of the sets to process (device; every entry lies in 0 .. n_sets - 1 and no entry repeats;
 * an entry outside that range is skipped).  For each listed set r and voxel v:
 *   d_score[r][v] = min_c (|C_c|^2 - 2 C_c . x_v),     d_labels[r][v] = the LOWEST c attaining the minimum (int32, 0-based),
 * both arrays n_sets rows of V; the rows of sets that are not listed are not written.  A voxel whose column of X holds a
 * non-finite value gets label -1 and score NaN, and touches no other voxel; the centres are assumed finite.  The product runs on
 * v_mfma_f64_16x16x4_f64, the (min, argmin) is kept in registers over the centres in groups of 32: no V x K array exists, the
 * workspace holds the R K squared centre norms.  No sums across workgroups, no atomics: the same input gives the same bits, and
 * a set's outputs do not depend on which other sets are listed.  Nothing is read beyond column V of a row.
 * MODL_EINVAL before any device work: a NULL pointer (d_ws apart), d < 1 or d > modl_kmeans_max_features() = 128
 * (= modl_ica_max_components()), K < 1 or K > modl_kmeans_max_clusters() = 4096, V < 1, R < 1 or R > 65535, n_sets < R,
 * ldx < V, a pointer that is not aligned to its element, an overlap of d_score or d_labels with each other, an input or the
 * workspace, or of the workspace with an input.  d_ws NULL or ws_bytes below modl_kmeans_assign_workspace(V, d, K, R) (0 for
 * bad arguments): MODL_ENOMEM; no device: MODL_ENOGPU.
 *
 * modl_label_sums_*.  d_X: `rows` rows of V values, ldx >= V.  d_order: n_order int32 voxel indices grouped by label, ascending
 * within a label; d_offsets: int64[K + 1], label c owns d_order[d_offsets[c] .. d_offsets[c + 1] - 1] (the caller builds both
 * with a stable sort of the labels and a count).  d_sums (double, `rows` rows of K, lds >= K):
 *   d_sums[row][c] = sum over j in d_offsets[c] .. d_offsets[c + 1] - 1 of X[row][d_order[j]],
 * accumulated in f64 (f32 is converted on load), an empty label gives 0.  No floating-point atomics; the order of the additions
 * of one (row, label) is a function of the segment's length alone, so the bits of a label's sum do not depend on the other
 * labels, on the other rows or on K.  A label's segment of d_order is staged once per workgroup and reused over a slab of rows;
 * X is read once per element that belongs to a label, voxels in no segment are never read.  An index outside 0 .. V - 1 adds
 * nothing, offsets are clamped to 0 .. n_order.  MODL_EINVAL before any device work: a NULL pointer, K < 1, rows < 0 or
 * rows > 32 * 65535, V < 1 or V > INT32_MAX, n_order < 0, ldx < V, lds < K, a pointer that is not aligned to its element, an
 * overlap of d_sums with an input.  rows == 0 or n_order == 0 does nothing (d_sums is not written) and returns MODL_OK; no
 * device: MODL_ENOGPU. */
int modl_kmeans_max_clusters(void);
int modl_kmeans_max_features(void);
size_t modl_kmeans_assign_workspace(int64_t V, int d, int K, int R);
int modl_kmeans_assign_f64(const double *d_X, int64_t ldx, int64_t V, int d, const double *d_C, int K, int n_sets, const int32_t *d_active,
                           int R, double *d_score, int32_t *d_labels, void *d_ws, size_t ws_bytes, void *stream);
int modl_label_sums_f32(const float *d_X, int64_t ldx, int64_t rows, int64_t V, const int32_t *d_order, int64_t n_order,
                        const int64_t *d_offsets, int K, double *d_sums, int64_t lds, void *stream);
int modl_label_sums_f64(const double *d_X, int64_t ldx, int64_t rows, int64_t V, const int32_t *d_order, int64_t n_order,
                        const int64_t *d_offsets, int K, double *d_sums, int64_t lds, void *stream);

/* layout helpers: out[c][r] = in[r][c]  (components_ <-> Dt).  ceil(rows / 32) is the grid's y extent: more than
 * 32 * 65536 rows (65536: the y limit the MI355X reports) are refused with MODL_EINVAL before any launch. */
int modl_transpose_f32(const float *d_in, float *d_out, int64_t rows, int64_t cols, void *stream);
int modl_transpose_f64(const double *d_in, double *d_out, int64_t rows, int64_t cols, void *stream);

/* per-kernel-class timing of the fused step (HIP events on `stream`).
 * enable: 0 = off, 1 = every section, otherwise a mask: bit (i + 1) times section i of the order
 * {code_gemm, code_solve, stats_gemm, stats_apply, dict_update} — each timed section costs two event
 * records (a few microseconds of stream bubble each).  get: copies up to `cap` entries; names are static. */
#define MODL_PROF_MAX 16
typedef struct modl_prof_entry {
    const char *name;
    double ms_total;     /* accumulated device time */
    int64_t launches;    /* kernel launches accumulated */
    int64_t calls;       /* timed regions accumulated */
} modl_prof_entry;
int modl_somf_prof_enable(modl_somf_plan *plan, int enable);
/* host time (ms) the calls of this plan have spent waiting for a free staging slot, i.e. for the device: the
 * host runs at most 8 minibatches ahead.  Host enqueue time minus this is what the host itself needs. */
int modl_somf_host_wait_ms(modl_somf_plan *plan, double *out, int reset);
/* record the section events on every `every`-th minibatch only (each recorded section costs two event records, a
 * stream bubble of several microseconds: sampling keeps the timed region undisturbed) */
int modl_somf_prof_stride(modl_somf_plan *plan, int every);
int modl_somf_prof_get(modl_somf_plan *plan, modl_prof_entry *out, int cap, int *n_out);
int modl_somf_prof_reset(modl_somf_plan *plan);

#ifdef __cplusplus
}
#endif
#endif /* MODL_HIP_H */
