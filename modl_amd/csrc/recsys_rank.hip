// Ranks of held-out items for RecsysDictFact: where the targets of b queries stand among the items the query has not excluded.
//
//   score[ii][f] = sum_c code[ii][c] * Dt[f][c] (+ item_bias[f])        the score of recsys_topn_kernel, bit for bit: both kernels
//                                                                             get it from topn_score_tile (recsys_topn.hpp)
//   ranks[e]     = #{ c != t : c not excluded for ii, (score[ii][c], c) beats (score[ii][t], t) }     t = t_indices[e] of query ii
//
// The b x p scores are never written.  The launches:
//   1. a memset of the two bitmasks and of the counters; the top-N file's recsys_mask_kernel twice (launch_recsys_mask): the
//      exclusion pattern and the first t_max entries of every target row, each ORed into a bitmask of p bits per query.
//   2. recsys_rank_sweep_kernel<T, false> ("capture"): the tile product of the top-N kernel (a workgroup owns 32 queries and
//      one slab of items; tiles of 128 / 64 items, K in chunks of 64: topn_score_tile).  A score whose bit is set in
//      the target mask is written to every entry of the query's target row that names the item (the row's ids are in LDS;
//      a hit is rare and the hitting lane scans the row).
//   3. recsys_rank_sweep_kernel<T, true> ("count"): the workgroup first sorts the (score, item) pairs of each of its queries'
//      target rows in LDS by counting (in-range targets under topn_beats, equal pairs by entry index; out-of-range ones
//      last).  Then the same product; every score that is not excluded finds by binary search how many of the query's
//      sorted targets beat it (they are a prefix) and adds one to that bin of the query's histogram in LDS.  At the end of
//      the slab the histograms are added to the global ones: integer adds, no order enters.
//   4. recsys_rank_finalize_kernel: one wavefront per query repeats the sort, takes the prefix sum of the histogram (the
//      candidates that beat or are the target at sorted position q are those of the bins 0 .. q), subtracts the target
//      itself where it is a candidate, and writes ranks, the -1 / -2 entries and n_candidates.
#include "recsys_topn.hpp"

namespace modl {

// the position of entry j in the sorted target row (n entries): in-range items first, under topn_beats and then by entry
// index (a repeated item has the same score at every occurrence), the others behind them by entry index.  The scores of
// out-of-range entries are never looked at (nothing wrote them).
template <typename T> __device__ __forceinline__ int rank_sorted_pos(const T *rs, const int *ri, int n, int j, int64_t p) {
    const int ij = ri[j];
    const T sj = rs[j];
    const bool vj = ij >= 0 && ij < p;
    int pos = 0;
    for (int l = 0; l < n; ++l) {
        const int il = ri[l];
        const T sl = rs[l];
        const bool vl = il >= 0 && il < p;
        const bool before = vl ? (!vj || topn_beats(sl, il, sj, ij) || (sl == sj && il == ij && l < j)) : (!vj && l < j);
        pos += before ? 1 : 0;
    }
    return pos;
}

struct RankLds : TopnTileLds { size_t ths, raws, thi, rawi, hist, nn, nv; int ldt, ldh; };
template <typename T> static RankLds rank_lds(int k, int t_max) {
    const int ldt = t_max | 1, ldh = (t_max + 1) | 1;
    const size_t rows = (size_t)kTopnUsers * ldt, hist = (size_t)kTopnUsers * ldh;
    RankLds L;
    static_cast<TopnTileLds &>(L) = topn_tile_lds<T>(k, 2 * rows, 2 * rows + hist + 2 * kTopnUsers, &L.ths, &L.thi);
    L.ldt = ldt;
    L.ldh = ldh;
    L.raws = L.ths + sizeof(T) * rows;
    L.rawi = L.thi + sizeof(int) * rows;
    L.hist = L.rawi + sizeof(int) * rows;
    L.nn = L.hist + sizeof(int) * hist;
    L.nv = L.nn + sizeof(int) * kTopnUsers;
    return L;
}

// COUNT = false: capture the scores of the targets (mask = the target mask); COUNT = true: count (mask = the exclusion mask)
template <typename T, bool COUNT>
__global__ __launch_bounds__(256) void recsys_rank_sweep_kernel(const T *code, const int64_t *code_rows, int64_t b, int k,
                                                                const T *Dt, int64_t p, const unsigned int *mask, int64_t W,
                                                                const double *item_bias, const int32_t *t_indptr,
                                                                const int32_t *t_indices, int t_max, int top_step,
                                                                int64_t slab_items, T *tscore, int32_t *g_hist, RankLds L) {
    using MT = Mma<T>;
    using CF = TopnCfg<T>;
    constexpr int WN = CF::WN, RM = CF::RM, IT = 4 * WN, MW = IT / 32;
    static_assert(RM * MT::TM == kTopnUsers && MT::TN == WN, "one tile column of items per wavefront");
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    T *Cs = reinterpret_cast<T *>(smem_raw + L.cs);
    T *Ds = reinterpret_cast<T *>(smem_raw + L.ds);
    T *th_s = reinterpret_cast<T *>(smem_raw + L.ths);         // capture: unused; count: the sorted targets' scores
    T *raw_s = reinterpret_cast<T *>(smem_raw + L.raws);
    double *bs = reinterpret_cast<double *>(smem_raw + L.bs);
    int *th_i = reinterpret_cast<int *>(smem_raw + L.thi);     // capture: the target rows' ids; count: the sorted targets' ids
    int *raw_i = reinterpret_cast<int *>(smem_raw + L.rawi);
    int *hist = reinterpret_cast<int *>(smem_raw + L.hist);
    int *nn = reinterpret_cast<int *>(smem_raw + L.nn);        // entries of the row (at most t_max)
    int *nv = reinterpret_cast<int *>(smem_raw + L.nv);        // in-range ones among them
    unsigned int *mk = reinterpret_cast<unsigned int *>(smem_raw + L.mk);
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int ldt = L.ldt, ldh = L.ldh;
    const int64_t u0 = (int64_t)blockIdx.x * kTopnUsers;
    const int slab = blockIdx.y;
    const int64_t f_begin = (int64_t)slab * slab_items;
    const int64_t f_end = f_begin + slab_items < p ? f_begin + slab_items : p;

    topn_stage_codes(Cs, L.ldc, code, code_rows, u0, b, k);
    // the target rows
    if (tid < kTopnUsers) {
        int n = 0;
        if (u0 + tid < b) {
            const int64_t len = (int64_t)t_indptr[u0 + tid + 1] - t_indptr[u0 + tid];
            n = (int)(len < 0 ? 0 : (len < t_max ? len : t_max));
        }
        nn[tid] = n;
        nv[tid] = 0;
    }
    __syncthreads();
    for (int e = tid; e < kTopnUsers * t_max; e += 256) {
        const int m = e / t_max, j = e % t_max;
        const bool in = j < nn[m];
        const int64_t ii = u0 + m < b ? u0 + m : b - 1;
        const int id = in ? t_indices[(int64_t)t_indptr[ii] + j] : -1;
        if (COUNT) {
            raw_i[m * ldt + j] = id;
            raw_s[m * ldt + j] = (in && id >= 0 && id < p) ? tscore[ii * t_max + j] : (T)0;
        } else {
            th_i[m * ldt + j] = id;
        }
    }
    if (COUNT) {
        for (int e = tid; e < kTopnUsers * ldh; e += 256) hist[e] = 0;
        __syncthreads();
        for (int e = tid; e < kTopnUsers * t_max; e += 256) {
            const int m = e / t_max, j = e % t_max;
            if (j < nn[m]) {
                const int id = raw_i[m * ldt + j];
                const int pos = rank_sorted_pos(raw_s + m * ldt, raw_i + m * ldt, nn[m], j, p);
                th_s[m * ldt + pos] = raw_s[m * ldt + j];
                th_i[m * ldt + pos] = id;
                if (id >= 0 && id < p) atomicAdd(&nv[m], 1);
            }
        }
    }

    const TopnSplit sp = topn_split<T>(k);
    for (int64_t item0 = f_begin; item0 < f_end; item0 += IT) {
        typename MT::acc_t acc[RM];                          // (its first barrier: the sorted rows are written)
        topn_score_tile(acc, Cs, Ds, mk, bs, L.ldc, L.ldd, Dt, p, k, mask, W, item_bias, item0, f_end, u0, b, sp);
        {
            const int col = wid * WN + MT::acc_col(lane, 0);
            const int64_t f = item0 + col;
            const double bias = bs[col];
            const bool f_ok = f < f_end;
#pragma unroll
            for (int i = 0; i < RM; ++i)
#pragma unroll
                for (int r = 0; r < MT::NACC; ++r) {
                    const int m = i * MT::TM + MT::acc_row(lane, r);
                    const bool bit = (mk[m * MW + (col >> 5)] >> (col & 31)) & 1u;
                    const T s = item_bias ? (T)((double)acc[i][r] + bias) : acc[i][r];
                    if (!f_ok || u0 + m >= b) continue;
                    if (COUNT) {
                        if (bit) continue;                       // excluded
                        const T *ts = th_s + m * ldt;
                        const int *ti = th_i + m * ldt;
                        const int n = nv[m];
                        int pos = 0;                             // the sorted targets that beat (s, f) are a prefix: its length
                        for (int st = top_step; st >= 1; st >>= 1) {
                            const int q = pos + st;
                            if (q <= n && topn_beats(ts[q - 1], ti[q - 1], s, (int)f)) pos = q;
                        }
                        atomicAdd(&hist[m * ldh + pos], 1);
                    } else if (bit) {
                        const int n = nn[m];
                        for (int j = 0; j < n; ++j)
                            if (th_i[m * ldt + j] == (int)f) tscore[(u0 + m) * t_max + j] = s;
                    }
                }
        }
    }
    if (COUNT) {
        __syncthreads();
        for (int e = tid; e < kTopnUsers * (t_max + 1); e += 256) {
            const int m = e / (t_max + 1), q = e % (t_max + 1);
            const int c = hist[m * ldh + q];
            if (u0 + m < b && c) atomicAdd(&g_hist[(u0 + m) * (t_max + 1) + q], c);
        }
    }
}

template <typename T>
__global__ __launch_bounds__(64) void recsys_rank_finalize_kernel(const int32_t *t_indptr, const int32_t *t_indices, int t_max,
                                                                  int64_t p, const unsigned int *ex_mask, int64_t W,
                                                                  const T *tscore, const int32_t *g_hist, int32_t *ranks,
                                                                  int32_t *n_candidates) {
    __shared__ T rs[MODL_RECSYS_MAX_RANK_TARGETS];
    __shared__ int ri[MODL_RECSYS_MAX_RANK_TARGETS];
    const int lane = threadIdx.x;
    const int64_t ii = blockIdx.x;
    const int64_t e0 = t_indptr[ii];
    const int64_t len = (int64_t)t_indptr[ii + 1] - e0;
    const int n = (int)(len < 0 ? 0 : (len < t_max ? len : t_max));
    int id = -1;
    if (lane < n) {
        id = t_indices[e0 + lane];
        ri[lane] = id;
        rs[lane] = (id >= 0 && id < p) ? tscore[ii * t_max + lane] : (T)0;
    }
    __syncthreads();
    // inclusive prefix sum of the histogram over the lanes (bin t_max holds what every target beats: no rank needs it)
    int h = (lane <= t_max && lane < 64) ? g_hist[ii * (t_max + 1) + lane] : 0;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(h, d);
        if (lane >= d) h += o;
    }
    const bool valid = id >= 0 && id < p;
    const int pos = lane < n ? rank_sorted_pos(rs, ri, n, lane, p) : 0;
    const int upto = __shfl(h, pos);
    if (lane < n) {
        int self = 0;
        if (valid) self = ex_mask ? 1 - (int)((ex_mask[ii * W + (id >> 5)] >> (id & 31)) & 1u) : 1;
        ranks[e0 + lane] = valid ? upto - self : -1;
    }
    for (int64_t e = (int64_t)t_max + lane; e < len; e += 64) ranks[e0 + e] = -2;
    if (n_candidates) {
        int c = 0;
        if (ex_mask)
            for (int64_t w = lane; w < W; w += 64) c += __popc(ex_mask[ii * W + w]);
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) c += __shfl_xor(c, d);
        if (lane == 0) n_candidates[ii] = (int32_t)(p - c);
    }
}

struct RankWs { size_t ex_mask, t_mask, hist, tscore, zeroed, total; int64_t W; };
template <typename T> static RankWs rank_ws(int64_t p, int64_t b, int t_max) {
    RankWs w;
    w.W = cdiv(p, 32);
    size_t o = 0;
    w.ex_mask = o; o += align_up(sizeof(unsigned int) * (size_t)b * w.W, 256);
    w.t_mask = o; o += align_up(sizeof(unsigned int) * (size_t)b * w.W, 256);
    w.hist = o; o += align_up(sizeof(int32_t) * (size_t)b * (t_max + 1), 256);
    w.zeroed = o;                                             // masks and counters: one memset
    w.tscore = o; o += align_up(sizeof(T) * (size_t)b * t_max, 256);
    w.total = o;
    return w;
}

template <typename T> static bool rank_args_ok(int64_t p, int k, int64_t b, int t_max) {
    return b >= 0 && p >= 1 && p < ((int64_t)1 << 31) && t_max >= 1 && t_max <= MODL_RECSYS_MAX_RANK_TARGETS && k >= 1 &&
           k <= TopnCfg<T>::KMAX;
}

template <typename T> static size_t rank_workspace(int64_t p, int k, int64_t b, int t_max) {
    if (!rank_args_ok<T>(p, k, b, t_max) || b == 0) return 0;
    return rank_ws<T>(p, b, t_max).total;
}

template <typename T>
static int recsys_ranks(const T *code, const int64_t *code_rows, int64_t b, int k, const T *Dt, int64_t p,
                        const int32_t *ex_indptr, const int32_t *ex_indices, const int64_t *ex_rows, const double *item_bias,
                        const int32_t *t_indptr, const int32_t *t_indices, int t_max, int32_t *ranks, int32_t *n_candidates,
                        void *ws, size_t ws_bytes, hipStream_t st) {
    if (!code || !Dt || !t_indptr || !t_indices || !ranks || (ex_indptr && !ex_indices) || !rank_args_ok<T>(p, k, b, t_max))
        return MODL_EINVAL;
    if (b == 0) return MODL_OK;
    const RankWs w = rank_ws<T>(p, b, t_max);
    if (!ws || ws_bytes < w.total) return MODL_ENOMEM;
    if (modl_device_count() <= 0) return MODL_ENOGPU;
    int64_t slab_items;
    const int S = topn_slabs<T>(p, b, &slab_items);
    char *base = static_cast<char *>(ws);
    unsigned int *ex_mask = ex_indptr ? reinterpret_cast<unsigned int *>(base + w.ex_mask) : nullptr;
    unsigned int *t_mask = reinterpret_cast<unsigned int *>(base + w.t_mask);
    int32_t *hist = reinterpret_cast<int32_t *>(base + w.hist);
    T *tscore = reinterpret_cast<T *>(base + w.tscore);
    const size_t z0 = ex_indptr ? w.ex_mask : w.t_mask;
    MODL_HIP(hipMemsetAsync(base + z0, 0, w.zeroed - z0, st));
    if (ex_indptr) MODL_TRY(launch_recsys_mask(st, ex_indptr, ex_indices, ex_rows, b, p, w.W, INT32_MAX, ex_mask));
    MODL_TRY(launch_recsys_mask(st, t_indptr, t_indices, nullptr, b, p, w.W, t_max, t_mask));
    const RankLds L = rank_lds<T>(k, t_max);
    int top_step = 1;                                         // the largest power of two not above t_max
    while (top_step * 2 <= t_max) top_step *= 2;
    const dim3 grid((unsigned)cdiv(b, kTopnUsers), (unsigned)S);
    MODL_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&recsys_rank_sweep_kernel<T, false>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    hipLaunchKernelGGL((recsys_rank_sweep_kernel<T, false>), grid, dim3(256), L.total, st, code, code_rows, b, k, Dt, p,
                       (const unsigned int *)t_mask, w.W, item_bias, t_indptr, t_indices, t_max, top_step, slab_items, tscore,
                       hist, L);
    MODL_LAUNCH_CHECK();
    MODL_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&recsys_rank_sweep_kernel<T, true>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    hipLaunchKernelGGL((recsys_rank_sweep_kernel<T, true>), grid, dim3(256), L.total, st, code, code_rows, b, k, Dt, p,
                       (const unsigned int *)ex_mask, w.W, item_bias, t_indptr, t_indices, t_max, top_step, slab_items, tscore,
                       hist, L);
    MODL_LAUNCH_CHECK();
    hipLaunchKernelGGL((recsys_rank_finalize_kernel<T>), dim3((unsigned)b), dim3(64), 0, st, t_indptr, t_indices, t_max, p,
                       (const unsigned int *)ex_mask, w.W, (const T *)tscore, (const int32_t *)hist, ranks, n_candidates);
    MODL_LAUNCH_CHECK();
    return MODL_OK;
}

}  // namespace modl

using namespace modl;

extern "C" {

size_t modl_recsys_ranks_workspace(int dtype, int64_t p, int k, int64_t b, int t_max) {
    if (dtype == MODL_F32) return rank_workspace<float>(p, k, b, t_max);
    if (dtype == MODL_F64) return rank_workspace<double>(p, k, b, t_max);
    return 0;
}

#define ABI_RANKS(SFX, T)                                                                                                 \
    int modl_recsys_ranks_##SFX(const T *d_code, const int64_t *d_code_rows, int64_t b, int k, const T *d_Dt, int64_t p,     \
                                const int32_t *d_ex_indptr, const int32_t *d_ex_indices, const int64_t *d_ex_rows,         \
                                const double *d_item_bias, const int32_t *d_t_indptr, const int32_t *d_t_indices,          \
                                int t_max, int32_t *d_ranks, int32_t *d_n_candidates, void *d_ws, size_t ws_bytes,         \
                                void *stream) {                                                                            \
        return recsys_ranks<T>(d_code, d_code_rows, b, k, d_Dt, p, d_ex_indptr, d_ex_indices, d_ex_rows, d_item_bias,     \
                               d_t_indptr, d_t_indices, t_max, d_ranks, d_n_candidates, d_ws, ws_bytes,                   \
                               (hipStream_t)stream);                                                                      \
    }
ABI_RANKS(f32, float)
ABI_RANKS(f64, double)
#undef ABI_RANKS

}  // extern "C"
