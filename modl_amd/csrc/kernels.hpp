// Declarations shared between the translation units of libmodl_hip.
#pragma once
#include "common.hpp"
#include "gemm_plan.hpp"

namespace modl {

// ---- cd_solver.hip ----------------------------------------------------------
template <typename T>
struct CdArgs {
    const T *G;            // [k][k] shared, or [b][k][k] when g_stride != 0
    int64_t g_stride;
    const int64_t *g_idx;  // per-sample Gram index (rows of G_average_), or null: sample ii uses G[ii]
    const T *Dx;           // [b][k]
    const T *xnorm2;       // [b] squared norm of the full sample row
    const T *H0;           // [b][k] initial Q w (from a matrix-core product), or null: computed in-kernel
    T *code;               // [n][k]
    const int64_t *idx;    // [b] or null (identity)
    T *code2 = nullptr;    // optional second destination: code2[idx2[i]] = solution i
    int g_pad_rows = 0;    // rows readable behind G (shared Gram only): >= 16 lets the row prefetch run unclamped
    int ldg = 0;           // row stride of G (0: k).  A shared Gram padded with zeros to ldg = 64 * ceil(k / 64 rounded to
                           // a power of two) columns and ldg + 16 rows runs the vectorised kernel whatever k is
                           // (launch_cd_pad_gram / cd_padded_ld)
    const int64_t *idx2 = nullptr;
    int32_t *sweeps;       // [b] or null
    int b, k;
    T alpha, beta, tol;
    int max_iter, positive;
    int sparse_pct = 20;   // a sweep with at most sparse_pct % of the coordinates active runs as a sparse sweep
                           // (measured at k = 256: a sparse step costs 0.23 us, a dense sweep 14.3 us (f32) / 18.9 us (f64))
};
template <typename T> int launch_cd(hipStream_t stream, const CdArgs<T> &a);
// cd_wide.hip: 1024 < k <= MODL_MAX_COMPONENTS, one workgroup per sample, the k-vectors in LDS; any Gram layout (shared or
// per sample, any row stride ldg, any alignment)
template <typename T> int launch_cd_wide(hipStream_t stream, const CdArgs<T> &a);
// cd_split.hip: the same solver with the chain and the k-wide update on two wavefronts (shared Gram, 64 < k <= 512)
template <typename T> bool cd_split_applies(const CdArgs<T> &a);
// ... what it reads: element size, k, the row stride kq of G, g_stride, G on a 16-byte boundary
bool cd_split_takes(size_t tsz, int k, int kq, int64_t g_stride, bool g_aligned16);
template <typename T> int launch_cd_split(hipStream_t stream, const CdArgs<T> &a);
// a Gram matrix PER SAMPLE whose size is not one of the solver's strides: slices of the minibatch through zero-padded
// copies (slots: scratch of cd_per_sample_scratch_bytes, zero outside the k x k corners - zero-filled once per k)
bool cd_split_enabled();
int cd_per_sample_ld(int k);
size_t cd_per_sample_scratch_bytes(size_t tsz, int64_t b, int k);
template <typename T> int launch_cd_per_sample(hipStream_t stream, const CdArgs<T> &a, T *slots, size_t slot_bytes);
bool cd_one_wave_covers(int k);   // the one-wavefront kernel exists for k coefficients (k <= 256; any k in the diagnostics library)
int cd_padded_ld(int k);   // the row stride the vectorised solver wants for k coefficients (k itself when it fits already)
// Gp[ldg + 16][ldg] (zero-filled once by the caller) <- G[k][k]
template <typename T> int launch_cd_pad_gram(hipStream_t stream, const T *G, int k, T *Gp, int ldg);
template <typename T> int launch_row_norm2(hipStream_t stream, const T *X, int64_t ldx, int64_t p, int64_t b, T *out);

// ---- chol.hip ---------------------------------------------------------------
// factor nmat matrices (G[m] + alpha I) into F[m] (symmetric storage of the
// Cholesky factor: F[i][j] = L[max(i,j)][min(i,j)])
template <typename T>
int launch_cholesky(hipStream_t stream, const T *G, int64_t g_stride, const int64_t *g_idx, T *F, int k, T alpha,
                    int nmat);
// solve F[m] F[m]^T x = rhs for b right-hand sides (rows of rhs, in place);
// f_stride == 0: one shared factor.  Results also scattered to code rows.
// k <= 128: factor (G[m] + alpha I) and solve in one launch, the matrix in LDS (shared matrix: all b right-hand sides;
// g_stride != 0: one matrix and one right-hand side per workgroup).  rhs solved in place, also written to the code rows.
template <typename T> bool ridge_small_applies(int k);
template <typename T>
int launch_ridge_small(hipStream_t stream, const T *G, int64_t g_stride, const int64_t *g_idx, T *rhs, int b, int k, T alpha,
                       T *code, const int64_t *idx);
template <typename T>
int launch_chol_solve(hipStream_t stream, const T *F, int64_t f_stride, T *rhs, int b, int k, T *code,
                      const int64_t *idx);

// wide systems (k > 512): blocked factorisation + substitutions on the matrix cores.  G: shared (g_stride == 0) or
// one Gram per sample at G + h_gidx[i] * g_stride (HOST index array, or null = i); F: k*k scratch; Linv:
// chol_wide_scratch_elems(k) scratch; rhs[b][k]: right-hand sides, overwritten by the solutions, which are also
// written to code rows d_idx (device, or null = row i).
size_t chol_wide_scratch_elems(int k);
bool chol_blocked(int k, size_t tsz, bool shared);   // which ridge systems take the blocked factorisation
template <typename T>
int ridge_solve_wide(hipStream_t stream, const T *G, int64_t g_stride, const int64_t *h_gidx, T *F, T *Linv, T *rhs, int b,
                     int k, T alpha, T *code, const int64_t *d_idx);

// ---- code_solve.hip ---------------------------------------------------------
// Which kernels solve for the codes of a minibatch: decided here and nowhere else, for the step (somf_step.hip) and for
// modl_enet_regression_* alike.
enum CodeRoute {                  // (the ridge leaves first: code_solve tells the two families apart by that)
    CODE_RIDGE_BLOCKED,   // ridge_solve_wide: blocked factorisation and substitutions on the matrix cores
    CODE_RIDGE_SMALL,     // launch_ridge_small: factor + substitutions in one launch, in LDS
    CODE_RIDGE_FACTOR,    // launch_cholesky, then launch_chol_solve
    CODE_CD_WIDE,         // k > 1024: launch_cd_wide, shared or per-sample Gram as stored
    CODE_CD_SLOTS,        // a Gram per sample of a size the four-wavefront solver does not take as stored: launch_cd_per_sample
    CODE_CD_PADDED,       // a shared Gram copied into a zero-padded matrix of the vectorised solver's stride, then launch_cd
    CODE_CD_STORED,       // launch_cd on the matrices where they are
};
// pure: tsz = sizeof(T), g_stride = 0 for a shared Gram, g_aligned16 = G sits on a 16-byte boundary, split_enabled /
// one_wave_covers = cd_split_enabled() / cd_one_wave_covers(k) (arguments, so that a size can be asked for whatever the
// diagnostics switch says).  The size of the minibatch plays no part.
CodeRoute code_route(size_t tsz, int k, double l1_ratio, int64_t g_stride, bool g_aligned16, bool split_enabled,
                     bool one_wave_covers);
template <typename T> inline CodeRoute code_route_of(const T *G, int64_t g_stride, int k, double l1_ratio) {
    return code_route(sizeof(T), k, l1_ratio, g_stride, reinterpret_cast<uintptr_t>(G) % 16 == 0, cd_split_enabled(),
                      cd_one_wave_covers(k));
}
// what the leaves need besides the operands; each caller fills it from its own memory
template <typename T>
struct CodeScratch {
    T *F = nullptr, *Linv = nullptr;      // Cholesky factor(s); chol_wide_scratch_elems(k) for the blocked leaf
    T *H0 = nullptr;                      // [b][k]
    T *Gpad = nullptr; int ld_gpad = 0;   // [ld_gpad + 16][ld_gpad], zero outside the k x k corner (null: nothing is padded)
    size_t gpad_zero_bytes = 0;           // != 0: zero-fill that much of Gpad now (0: the caller did, once)
    T *slots = nullptr; size_t slots_bytes = 0;   // launch_cd_per_sample's scratch
    bool slots_zero = false;              // zero-fill it now
    int g_pad_rows = 0;                   // CdArgs::g_pad_rows of a shared Gram that is solved as stored
    // H0 = code G of a shared Gram by a product launch of its own instead of inside the solver.  The wide solver needs it;
    // modl_enet_regression_* also asks for it at every other size, the step does not: the two sum in different orders,
    // and each caller keeps the bits it has always returned.
    bool h0_by_product = false;
};
// a: the operands and tol, max_iter, positive as for launch_cd (code2 / idx2: the optional second destination, written by
// every leaf); Dx, H0, ldg, g_pad_rows, alpha and beta are set here.  Dx [b][k]: the ridge leaves solve in place.  h_gidx:
// g_idx on the host (the blocked ridge leaf walks per-sample matrices from there).  launches: optional counter.
template <typename T>
int code_solve(hipStream_t stream, CdArgs<T> a, T *Dx, T code_alpha, double l1_ratio, const int64_t *h_gidx,
               const CodeScratch<T> &sc, int *launches);

// ---- step_products.hip ------------------------------------------------------
// Which matrix-core launches form the products of a minibatch step - Dx and G in front of the code solve, the C_ and B_
// statistics behind it, the deferred rows of B_ (the rider), the Gram passes of G_agg = full - and of the transform:
// decided by three pure functions (no device, no global: switches and flags are arguments) and nowhere else.  somf_step.hip
// switches on their results; bcd.hip's plan_ride reads rider_route; modl_somf_product_route spells them as strings.
// split-K scratch of a plan, in elements: the largest split product is max(b, k) x k (Dx, Gram, C increment) with up to
// 64 splits; the p x k product (B increment) has >= 512 tiles at p >= 8k and is not split
size_t split_scratch_elems(int64_t max_batch, int k, int64_t p);

// The rider: the B_ update of the rows that were not sampled, deferred to the idle compute units of the dictionary
// update's launches.  Both thresholds live here.
constexpr int64_t kRiderMaxTiles = 1024;      // 64-feature tiles: from this many on (p > 65 472) nothing rides - the p x k
                                              // product runs as its own k-wide launch, and stats_route's wide pair begins
constexpr int64_t kRiderWideRows = 2048;      // features from which the rider takes k-wide tiles (32 x 128) instead of 32 x 32.
// du_route is asked the residency question of the persistent launch with the wide tile's LDS whenever p >= kRiderWideRows,
// even where plan_wide then declines and the rider takes the 32 x 32 tiles after all (p = 2402: not a multiple of 4).
// That is how the update has always been routed; it stays.
inline bool rider_too_tall(int64_t rows) { return cdiv(rows, 64) >= kRiderMaxTiles; }
inline bool rider_asks_wide_lds(int64_t p) { return p >= kRiderWideRows; }
enum RiderKind {
    RIDER_NONE,       // every row of B_ in the statistics launch (why: RiderWhy)
    RIDER_WIDE,       // rides as k-wide tiles of 32 features x 128 atoms
    RIDER_TILES32,    // rides as 32 x 32 tiles
    RIDER_AFTER,      // the dictionary update has no launch that carries it: completed behind the update, by stats_route
};
enum RiderWhy { RIDER_RIDES, RIDER_NO_PROPER_SUBSET, RIDER_DX_FULL, RIDER_FLAG, RIDER_TOO_TALL };
struct RiderRoute { RiderKind kind = RIDER_NONE; RiderWhy why = RIDER_RIDES; };
// proper_subset: a subset array with 0 < s < p that the step gathers; carried: the dictionary update runs the fused f32
// block or persistent launches (du_carries_riders); unal_x / unal_c: X (leading stride ldx) / the code rows (stride k)
// off 16 bytes
bool du_carries_riders(size_t tsz, int k, int optimizer, int comp_pos, double comp_l1_ratio);
RiderRoute rider_route(bool proper_subset, bool dx_full, bool no_rider_flag, bool carried, int64_t p, int k, int b, int64_t ldx,
                       bool unal_x, bool unal_c);

enum StatsKind { STATS_RESIDENT, STATS_WIDE_PAIR, STATS_PAIR32, STATS_DENSE_PAIR, STATS_EACH };
enum StatsEpi { STATS_EPI_VEC4, STATS_EPI_ROWS };       // the epilogue takes 16 bytes at a time / is row-indirected or stamped
struct StatsRoute {
    StatsKind kind = STATS_EACH;
    bool unal = false;            // an operand off 16 bytes
    StatsEpi epi = STATS_EPI_ROWS; // resident: how the second product's epilogue stores
    DensePlan P0, P1;             // dense pair: the two plans (P1 on kStatBM x kStatBN tiles)
    ProductLaunch C, B;           // one launch each (C: only with M0 > 0): stats_pair launches from these plans
};
#ifndef MODL_STAT_BM
#define MODL_STAT_BM 64
#define MODL_STAT_BN 64
#endif
#ifndef MODL_STAT_BK
#define MODL_STAT_BK 0
#endif
constexpr int kStatBM = MODL_STAT_BM, kStatBN = MODL_STAT_BN, kStatBK = MODL_STAT_BK;   // block tile of the p x k increment product
constexpr int64_t kResidentMinRows = 4096;
// code^T code (M0 x N; M0 == 0: none) and X^T code (M1 x N, X's leading stride ld1), both contracted over K samples.
// unal_c / unal_x: operand off 16 bytes; stamps: diagnostics stamps are wanted (32 x 32 tiles only); resident_switch:
// MODL_DEBUG_STATS_RESIDENT; epi: the second product's epilogue
StatsRoute stats_route(size_t tsz, int64_t M0, int64_t N, int64_t M1, int64_t K, bool unal_c, bool unal_x, int64_t ld1, StatsEpi epi,
                       bool stamps, bool resident_switch, size_t ws_elems);

struct CodeProductsRoute {
    bool need_sub = false;        // Ds = Dt[subset] (and Xs = X[:, subset]) are gathered
    int n_norm = 0, n_rows = 0, n_cols = 0, n_code = 0, fuse_cols = 0, gx = 0;   // the prep launch's parts (workgroups)
    int64_t s_pad = 0;
    bool x_gathered = false;      // Dx contracts Xs (leading stride s_pad) instead of X
    int64_t Kdim = 0;             // Dx's contraction length
    bool want_G = false, paired = false;
    DensePlan PD, PG;             // paired: Dx and G in one launch
    ProductLaunch Dx, G;          // else one launch each: phase1 launches from these plans
    bool g_average = false;       // rows of G_average are updated
    bool track_G = false, partial_G = false;   // G_agg = full: G_ -= / += over the sampled rows when s < p / 2, else recomputed
    GatherPlan gram;              // ... that launch (gram_of_rows)
    RiderRoute rider;
};
// G_agg = full: the dictionary update subtracts the sampled rows' Gram before and adds it after (dict_fact.py:667, 711-715)
// while they are fewer than half the features; else G_ is recomputed over all of p
inline bool gram_is_partial(int64_t s, int64_t p) { return (double)s < (double)p / 2.0; }
constexpr int kPrepRows = 8;      // rows per workgroup of prep_kernel's row gathers
struct StepBases { bool x = true, dt = true, code = true; };   // the caller's X, Dt and code_ start on a 16-byte boundary
// has_subset / has_idx: the minibatch carries a subset / sample-index array (with one, the code rows of the statistics
// are the plan's compact copy)
CodeProductsRoute code_products_route(const modl_somf_desc &d, int b, int64_t s, bool has_subset, bool has_idx, int64_t ldx,
                                      const StepBases &al, size_t ws_elems);
// modl_somf_product_route (section: MODL_ROUTE_*): the route as the string tests/test_product_routes.py: expected_route spells
int product_route_name(const modl_somf_desc &d, int section, int b, int64_t s, bool has_subset, bool has_idx, int64_t ldx,
                       int64_t x_offset, bool resident_switch, char *buf, size_t cap);

// ---- enet.hip ---------------------------------------------------------------
template <typename T>
int launch_enet_norm(hipStream_t stream, const T *v, int64_t rows, int64_t n, int64_t ld, int64_t inc, T l1_ratio,
                     T *out);
template <typename T>
int launch_enet_projection(hipStream_t stream, const T *v, T *out, int64_t rows, int64_t n, int64_t ld,
                           int64_t inc, const T *radius, T l1_ratio);
template <typename T>
int launch_enet_scale(hipStream_t stream, T *v, int64_t rows, int64_t n, int64_t ld, int64_t inc, T l1_ratio,
                      T radius);
template <typename T>
int launch_update_G_average(hipStream_t stream, T *G_average, const int64_t *idx, const T *G, const T *w_sample,
                            int64_t b, int64_t k);
template <typename T>
int launch_transpose(hipStream_t stream, const T *in, T *out, int64_t rows, int64_t cols);

// ---- masked_stats.hip -------------------------------------------------------
// B_ from dense rows with missing entries (modl_masked_stats_*), and the two small launches around the per-row solve of
// a masked minibatch: squared norms of the zero-filled rows; zero codes for the rows nobody observed + the minibatch's
// codes compact in codeb[b][k]
template <typename T>
int launch_masked_stats(hipStream_t stream, const T *X, int64_t ldx, const uint8_t *obs, int64_t ldo, const int64_t *rows,
                        int64_t b, int64_t p, int k, const T *code_b, T *Bt, int64_t *fni, int32_t *count, double w,
                        int64_t n_iter);
template <typename T>
int launch_masked_row_norm2(hipStream_t stream, const T *X, int64_t ldx, const uint8_t *obs, int64_t ldo, int64_t p, int b,
                            T *out);
template <typename T>
int launch_masked_codes_finish(hipStream_t stream, T *code, const int64_t *idx, const int32_t *nobs, int b, int k,
                               T *codeb);

// ---- omp.hip ----------------------------------------------------------------
// Batch-OMP on Gram quantities, one wavefront per sample: at most s atoms (1 <= s <= MODL_OMP_MAX_NONZERO, s <= k <=
// MODL_MAX_COMPONENTS), and with tol >= 0 only until the squared residual, started from xnorm2, is <= tol.  G shared
// (g_stride == 0) or one per sample (g_stride == k * k).  code[b][k], support[b][s] (-1 beyond n_active) and n_active[b]
// are written in full; support and n_active may be null.
bool omp_args_ok(int64_t b, int k, int n_nonzero, bool multi_gram);
template <typename T>
int launch_omp(hipStream_t stream, const T *G, int64_t g_stride, const T *Dx, const T *xnorm2, int64_t b, int k, int s, T tol,
               T *code, int32_t *support, int32_t *n_active);

// ---- bcd.hip ----------------------------------------------------------------
// Work that rides along the block launches of the fused dictionary update, on the compute units that update
// leaves idle: the statistics update of the rows of Bt that were NOT sampled,
//   Bt[f] <- beta Bt[f] + wt (X^T code)[f] / bdiv   for stamp[f] != step,
// a p x k x b product whose result the dictionary update does not need.  dict_update sets `consumed` when it
// took the work; otherwise the caller runs it on its own.
struct StatsRider {
    const void *X; int64_t ldx;           // minibatch rows [b][ldx]
    const void *code;                     // [b][k] the minibatch's code rows (compact)
    int b; int64_t p;
    void *Bt;                             // [p][k]
    const int32_t *stamp; int32_t step;
    double beta, wt, bdiv; int replace;
    int consumed;
};

// The parameter block of the NEXT minibatch (sample indices, subset, order, sample weights: a few KB of a pinned host
// slot) copied to HBM by one extra workgroup of the dictionary update's last launch instead of a launch of its own at
// the head of the next step (4.4 us of PCIe round trip on an otherwise idle chip, every step).  off16 / n16: up to four
// ranges of 16-byte words; the acknowledgement word tells the host the slot may be refilled.
struct StageRide {
    const uint4 *src = nullptr;
    uint4 *dst = nullptr;
    unsigned int off16[4] = {0, 0, 0, 0}, n16[4] = {0, 0, 0, 0};
    unsigned long long *ack = nullptr;
    unsigned long long use = 0;
    int consumed = 0;
};
// the copy itself, by `nthr` threads of ONE workgroup (every load of a round requested before the first store: the
// reads cross the host link)
__device__ __forceinline__ void stage_copy(const uint4 *__restrict__ src, uint4 *__restrict__ dst, const unsigned int (&off16)[4],
                                           const unsigned int (&n16)[4], unsigned long long *ack, unsigned long long use,
                                           int tid, int nthr) {
    constexpr int kMax = 4;
    const size_t c1 = n16[0], c2 = c1 + n16[1], c3 = c2 + n16[2], total = c3 + n16[3];
    for (size_t base = 0; base < total; base += (size_t)kMax * nthr) {
        uint4 v[kMax];
        size_t at[kMax];
#pragma unroll
        for (int u = 0; u < kMax; ++u) {
            size_t e = base + tid + (size_t)u * nthr;
            e = e < total ? e : total - 1;                        // (clamped, no branch around the load)
            at[u] = e < c1 ? off16[0] + e : (e < c2 ? off16[1] + (e - c1) : (e < c3 ? off16[2] + (e - c2) : off16[3] + (e - c3)));
            v[u] = src[at[u]];
        }
#pragma unroll
        for (int u = 0; u < kMax; ++u)
            if (base + tid + (size_t)u * nthr < total) dst[at[u]] = v[u];
    }
    __syncthreads();
    if (tid == 0) __hip_atomic_store(ack, use, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

template <typename T>
struct DictUpdateArgs {
    T *Dt;                    // [p][k] dictionary, feature-major, updated in place on the subset rows
    const T *Bt;              // [p][k]
    const T *C;               // [k][k] (bitwise symmetric)
    T *comp_norm;             // [k]
    const int32_t *subset;    // [s] device, or null = rows 0..s-1
    const int32_t *order;     // [k] device
    const int64_t *h_order;   // [k] host copy (the generic path issues one launch pair per atom)
    int64_t s;
    int k;
    int optimizer, comp_pos;
    double comp_l1_ratio, w, step_size;
    void *ws;                 // scratch, dict_update_workspace() bytes
    size_t ws_bytes;
    StatsRider *rider = nullptr;   // optional (f32 fused path only)
    StageRide *stage = nullptr;    // optional (f32 fused path only): rides the last launch; `consumed` says whether it did
    unsigned int *persist_flags = nullptr;   // optional, pinned host memory, PERSISTENT across calls (zero-initialised), BcdPersistArgs::flags:
                                   // [0] a persistent launch gave up half-way (update incomplete), [1] launches that could not
                                   // run and were completed by one workgroup
    bool allow_persist = true;     // false: one launch per block (a plan whose persistent launch could not run once)
    double *level_hint = nullptr;  // optional [k], PERSISTENT across calls (zero-initialised): the soft-threshold level
                                   // each atom's l1 / elastic-net projection ended with, warm start of the next one
};
// Which kernels take a dictionary update and the parameters their launches need: decided by du_route (bcd.hip) and nowhere
// else; dict_update switches on the family.
enum DuFamily {                   // (the families that walk h_order last: dict_update tells them apart by that)
    DU_SGD,       // du_sgd: col_norm_* + product + sgd_project_kernel
    DU_WIDE,      // dict_update_wide: k > 1024
    DU_TINY,      // du_unfused: bcd_prepare_kernel + bcd_tiny_kernel
    DU_FEW,       // du_unfused: bcd_prepare_kernel + bcd_few_kernel
    DU_UNFUSED,   // du_unfused: bcd_prepare_kernel, then apply / product / bcd_gram_kernel / bcd_resolve_kernel per block
    DU_BLOCK,     // du_block: bcd_setup_kernel, then bcd_block_kernel<RT, GPW> per block
    DU_PERSIST,   // du_persist: bcd_setup_kernel + the persistent launch (bcd_persist.hip)
    DU_SWEEP,     // du_sweep: atom_sweep_kernel
    DU_GROUPED,   // du_grouped: atom_grad_group_kernel<KPL, G> + atom_project_group_kernel<EPT, G, L1> per group
    DU_STAGED,    // du_staged: atom_grad4_kernel<KPL> per group + atom_corr_project_kernel per atom
    DU_STEP,      // du_step: atom_step_kernel<KPL> per atom
};
struct DuRoute {
    DuFamily family = DU_STEP;
    // block, persist: 32 RT sampled rows per workgroup, GPW contraction groups per worker wave, nslab workgroups, the
    // accumulator's shards, acc: bcd_block_kernel sums into the fixed-point accumulator (the persistent launch always does).
    // sgd, unfused: nslab slabs of kGramRows rows.  tiny, few, unfused: nfew = workgroups of bcd_few_kernel
    int RT = 1, GPW = 8, nslab = 0, shards = 1, nfew = 0;
    bool acc = false;
    // the per-atom families: KPL atoms per lane of the gradient kernels, groups of G atoms, EPT elements per thread of the
    // grouped projection, l1: comp_l1_ratio == 1
    int KPL = 1, G = 0, EPT = 0;
    bool l1 = false;
    // staged: the pipelined sweep or a gradient launch per group; spread: the exchange buffers of mwg_l1_project are armed
    // (not pipelined: it projects); pipelined: regs = 40 / 64 elements per thread of atom_project_regs, or 0: the spread
    // projection with ept elements per thread
    bool pipelined = false, spread = false;
    int regs = 0, ept = 1;
    bool lds = false;             // staged, step: the vector's copy in LDS (step: else in global memory)
};
// the route of a direct call as the string tests/test_dict_update_routes.py: expected_route spells (modl_dict_update_route)
int dict_update_route(int dtype, int k, int64_t s, int optimizer, int comp_pos, double comp_l1_ratio, int ncu, char *buf,
                      size_t cap);
int device_cu_count();            // compute units of the current device (one process per GPU: queried once)
size_t dict_update_workspace(int dtype, int64_t s_max, int k);
size_t dict_update_stamps_offset(int dtype, int64_t s_max, int k);
size_t dict_update_persist_stamps_offset(int dtype, int64_t s_max, int k);
template <typename T> int dict_update(hipStream_t stream, const DictUpdateArgs<T> &a, int *launches);

}  // namespace modl
