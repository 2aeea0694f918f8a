// Recommendation for RecsysDictFact: the n_top best unseen items of b users in one pass over the dictionary.
//
//   score[ii][f] = sum_c code[ii][c] * Dt[f][c] (+ item_bias[f])        for every item f that is not excluded for query ii
//   items[ii][j] = the item with the j-th largest score; equal scores by ascending item id
//
// The b x p scores are never written.  Three launches:
//   1. recsys_mask_kernel (only with an exclusion pattern; launch_recsys_mask serves the rank kernels too): one wavefront per
//      query ORs the items of its CSR row into a bitmask of p bits (zeroed by a memset before it).
//   2. recsys_topn_kernel: a workgroup owns 32 queries and one slab of items.  The 32 codes stay in LDS; the slab is streamed
//      in tiles of IT items (f32: 128, f64: 64; a tile of the feature-major dictionary is one contiguous block), K in chunks
//      of 64.  Each of the four wavefronts multiplies the 32 codes with its quarter of the tile on the matrix cores (Mma<T> of
//      gemm.hpp: one 32 x 32 x 2 tile in f32, two 16 x 16 x 4 tiles in f64; topn_score_tile of recsys_topn.hpp, shared with
//      the rank kernels), and every lane tests its scores against the
//      query's exclusion word (staged in LDS with the tile: O(1) per score) and the query's threshold, the n_top-th best so
//      far.  Scores that beat it go to the query's candidate buffer in LDS; when a buffer holds kMergeMin candidates the
//      wavefront that owns the query merges it into the query's sorted list by ranking (every element counts the elements
//      that beat it: pairs (score, item) are distinct, so the ranks are a permutation) and the threshold rises.  The slot a
//      candidate takes in the buffer comes from an LDS counter, but the merge orders by (score, item) alone, and the threshold
//      only ever rejects what n_top earlier elements beat: the list is a function of the inputs, not of the arrival order.
//   3. recsys_topn_merge_kernel (only with more than one slab): one wavefront per query merges the slabs' sorted lists under
//      the same total order.  The order is total, so the result does not depend on the slab count.
#include "recsys_topn.hpp"
#include <limits>

namespace modl {

__global__ __launch_bounds__(256) void recsys_mask_kernel(const int32_t *indptr, const int32_t *indices,
                                                          const int64_t *rows, int64_t b, int64_t p, int64_t W, int limit,
                                                          unsigned int *mask) {
    const int lane = threadIdx.x & 63;
    const int64_t ii = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ii >= b) return;
    const int64_t r = rows ? rows[ii] : ii;
    unsigned int *row = mask + ii * W;
    const int32_t e0 = indptr[r];
    const int64_t len = (int64_t)indptr[r + 1] - e0;
    const int32_t e1 = e0 + (int32_t)(len < limit ? len : limit);
    for (int32_t e = e0 + lane; e < e1; e += 64) {
        const int32_t f = indices[e];
        if (f >= 0 && f < p) atomicOr(row + (f >> 5), 1u << (f & 31));
    }
}

int launch_recsys_mask(hipStream_t st, const int32_t *indptr, const int32_t *indices, const int64_t *rows, int64_t b,
                       int64_t p, int64_t W, int limit, unsigned int *mask) {
    hipLaunchKernelGGL(recsys_mask_kernel, dim3((unsigned)cdiv(b, 4)), dim3(256), 0, st, indptr, indices, rows, b, p, W,
                       limit, mask);
    MODL_LAUNCH_CHECK();
    return MODL_OK;
}

struct TopnLds : TopnTileLds { size_t tops, topi, cands, candi, cnt; };
template <typename T> static TopnLds topn_lds(int k, int n_top) {
    constexpr int IT = 4 * TopnCfg<T>::WN, CB = IT + kTopnMergeMin;
    const size_t lists = (size_t)kTopnUsers * n_top, bufs = (size_t)kTopnUsers * CB;
    TopnLds L;
    static_cast<TopnTileLds &>(L) = topn_tile_lds<T>(k, lists + bufs, lists + bufs + kTopnUsers, &L.tops, &L.topi);
    L.cands = L.tops + sizeof(T) * lists;
    L.candi = L.topi + sizeof(int) * lists;
    L.cnt = L.candi + sizeof(int) * bufs;
    return L;
}

// the query's sorted list and its candidates -> the n_top best of both, sorted; one wavefront
template <typename T, int CB>
__device__ __forceinline__ void topn_merge_wave(T *ts, int *ti, const T *cs, const int *ci, int n_top, int c) {
    constexpr int NS = (MODL_RECSYS_MAX_TOPN + CB + 63) / 64;
    const int lane = threadIdx.x & 63;
    const int M = n_top + c;
    T es[NS];
    int ei[NS], rk[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int e = s * 64 + lane;
        const bool in_top = e < n_top, in = e < M;
        const int et = in_top ? e : 0, ec = (in && !in_top) ? e - n_top : 0;
        const T vt = ts[et], vc = cs[ec];
        const int it = ti[et], ic = ci[ec];
        es[s] = in ? (in_top ? vt : vc) : -std::numeric_limits<T>::infinity();
        ei[s] = in ? (in_top ? it : ic) : 0x7fffffff;
        rk[s] = 0;
    }
#pragma unroll
    for (int sj = 0; sj < NS; ++sj) {
        if (sj * 64 < M) {                                   // wavefront-uniform
            const int nj = M - sj * 64 < 64 ? M - sj * 64 : 64;
            for (int l = 0; l < nj; ++l) {
                const T s_j = bcast_lane(es[sj], l);
                const int i_j = bcast_lane(ei[sj], l);
#pragma unroll
                for (int s = 0; s < NS; ++s)
                    if (s * 64 < M) rk[s] += topn_beats(s_j, i_j, es[s], ei[s]) ? 1 : 0;
            }
        }
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int s = 0; s < NS; ++s)
        if (s * 64 + lane < M && rk[s] < n_top) {
            ts[rk[s]] = es[s];
            ti[rk[s]] = ei[s];
        }
}

template <typename T>
__global__ __launch_bounds__(256) void recsys_topn_kernel(const T *code, const int64_t *code_rows, int64_t b, int k,
                                                          const T *Dt, int64_t p, const unsigned int *mask, int64_t W,
                                                          const double *item_bias, int n_top, int64_t slab_items, int S,
                                                          int32_t *out_items, T *out_scores, TopnLds L) {
    using MT = Mma<T>;
    using CF = TopnCfg<T>;
    constexpr int WN = CF::WN, RM = CF::RM, IT = 4 * WN, CB = IT + kTopnMergeMin, MW = IT / 32;
    static_assert(RM * MT::TM == kTopnUsers && MT::TN == WN, "one tile column of items per wavefront");
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    T *Cs = reinterpret_cast<T *>(smem_raw + L.cs);
    T *Ds = reinterpret_cast<T *>(smem_raw + L.ds);
    T *top_s = reinterpret_cast<T *>(smem_raw + L.tops);
    T *cand_s = reinterpret_cast<T *>(smem_raw + L.cands);
    double *bs = reinterpret_cast<double *>(smem_raw + L.bs);
    int *top_i = reinterpret_cast<int *>(smem_raw + L.topi);
    int *cand_i = reinterpret_cast<int *>(smem_raw + L.candi);
    int *cnt = reinterpret_cast<int *>(smem_raw + L.cnt);
    unsigned int *mk = reinterpret_cast<unsigned int *>(smem_raw + L.mk);
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int64_t u0 = (int64_t)blockIdx.x * kTopnUsers;
    const int slab = blockIdx.y;
    const int64_t f_begin = (int64_t)slab * slab_items;
    const int64_t f_end = f_begin + slab_items < p ? f_begin + slab_items : p;
    const T ninf = -std::numeric_limits<T>::infinity();

    // the codes of the tile's queries (zero beyond b and beyond k), the empty lists
    topn_stage_codes(Cs, L.ldc, code, code_rows, u0, b, k);
    for (int e = tid; e < kTopnUsers * n_top; e += 256) {
        top_s[e] = ninf;
        top_i[e] = -1 - e % n_top;                            // (distinct: every pair (score, item) of a list differs)
    }
    if (tid < kTopnUsers) cnt[tid] = 0;

    const TopnSplit sp = topn_split<T>(k);
    for (int64_t item0 = f_begin; item0 < f_end; item0 += IT) {
        typename MT::acc_t acc[RM];                          // (its first barrier: the merges of the tile before are done)
        topn_score_tile(acc, Cs, Ds, mk, bs, L.ldc, L.ldd, Dt, p, k, mask, W, item_bias, item0, f_end, u0, b, sp);
        // selection: this lane's item against the threshold of each of its queries
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
                    const unsigned int word = mk[m * MW + (col >> 5)];
                    const T s = item_bias ? (T)((double)acc[i][r] + bias) : acc[i][r];
                    const T th_s = top_s[m * n_top + n_top - 1];
                    const int th_i = top_i[m * n_top + n_top - 1];
                    if (f_ok && u0 + m < b && !((word >> (col & 31)) & 1u) && topn_beats(s, (int)f, th_s, th_i)) {
                        const int pos = atomicAdd(&cnt[m], 1);
                        if (pos < CB) {                          // (always: a tile adds at most IT candidates to fewer than kTopnMergeMin)
                            cand_s[m * CB + pos] = s;
                            cand_i[m * CB + pos] = (int)f;
                        }
                    }
                }
        }
        __syncthreads();
        const bool last = item0 + IT >= f_end;
        for (int m = wid * (kTopnUsers / 4); m < (wid + 1) * (kTopnUsers / 4); ++m) {
            int c = cnt[m];
            c = c < CB ? c : CB;
            if (c >= kTopnMergeMin || (last && c > 0)) {     // wavefront-uniform
                topn_merge_wave<T, CB>(top_s + m * n_top, top_i + m * n_top, cand_s + m * CB, cand_i + m * CB, n_top, c);
                if (lane == 0) cnt[m] = 0;
            }
        }
    }
    __syncthreads();
    for (int e = tid; e < kTopnUsers * n_top; e += 256) {
        const int m = e / n_top, j = e % n_top;
        if (u0 + m >= b) continue;
        const int it = top_i[e];
        const int64_t o = S == 1 ? (u0 + m) * n_top + j : ((u0 + m) * S + slab) * n_top + j;
        out_items[o] = it < 0 ? -1 : it;
        out_scores[o] = it < 0 ? ninf : top_s[e];
    }
}

// the slabs' sorted lists of one query -> its list: n_top rounds, each takes the best head (one list per lane)
template <typename T>
__global__ __launch_bounds__(64) void recsys_topn_merge_kernel(const int32_t *part_items, const T *part_scores, int S,
                                                               int n_top, int32_t *items, T *scores) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    T *ls = reinterpret_cast<T *>(smem_raw);
    int *li = reinterpret_cast<int *>(ls + (size_t)S * n_top);
    const int lane = threadIdx.x;
    const int64_t q = blockIdx.x;
    const int tot = S * n_top;
    const T ninf = -std::numeric_limits<T>::infinity();
    for (int e = lane; e < tot; e += 64) {
        ls[e] = part_scores[q * tot + e];
        li[e] = part_items[q * tot + e];
    }
    __syncthreads();
    int h = 0;
    T cur_s = lane < S ? ls[lane * n_top] : ninf;
    int cur_i = lane < S ? li[lane * n_top] : -1;
    for (int j = 0; j < n_top; ++j) {
        T bs = cur_s;
        int bi = cur_i, bl = lane;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const T os = __shfl_xor(bs, d);
            const int oi = __shfl_xor(bi, d), ol = __shfl_xor(bl, d);
            const bool take = os > bs || (os == bs && (oi < bi || (oi == bi && ol < bl)));
            bs = take ? os : bs;
            bi = take ? oi : bi;
            bl = take ? ol : bl;
        }
        if (lane == 0) {
            items[q * n_top + j] = bi < 0 ? -1 : bi;
            scores[q * n_top + j] = bi < 0 ? ninf : bs;
        }
        if (lane == bl) {
            ++h;
            const int e = (lane < S && h < n_top) ? lane * n_top + h : 0;
            const T ns = ls[e];
            const int ni = li[e];
            cur_s = (lane < S && h < n_top) ? ns : ninf;
            cur_i = (lane < S && h < n_top) ? ni : -1;
        }
    }
}

struct TopnWs { size_t mask, part_items, part_scores, total; int64_t W; };
template <typename T> static TopnWs topn_ws(int64_t p, int64_t b, int n_top, int S) {
    TopnWs w;
    w.W = cdiv(p, 32);
    size_t o = 0;
    w.mask = o; o += align_up(sizeof(unsigned int) * (size_t)b * w.W, 256);
    const size_t lists = S > 1 ? (size_t)b * S * n_top : 0;
    w.part_scores = o; o += align_up(sizeof(T) * lists, 256);
    w.part_items = o; o += align_up(sizeof(int32_t) * lists, 256);
    w.total = o;
    return w;
}

template <typename T> static bool topn_args_ok(int64_t p, int k, int64_t b, int n_top) {
    return b >= 0 && p >= 1 && p < ((int64_t)1 << 31) && n_top >= 1 && n_top <= MODL_RECSYS_MAX_TOPN && k >= 1 &&
           k <= TopnCfg<T>::KMAX;
}

template <typename T> static size_t topn_workspace(int64_t p, int k, int64_t b, int n_top) {
    if (!topn_args_ok<T>(p, k, b, n_top) || b == 0) return 0;
    int64_t slab_items;
    const int S = topn_slabs<T>(p, b, &slab_items);
    return topn_ws<T>(p, b, n_top, S).total;
}

template <typename T>
static int recsys_topn(const T *code, const int64_t *code_rows, int64_t b, int k, const T *Dt, int64_t p,
                       const int32_t *ex_indptr, const int32_t *ex_indices, const int64_t *ex_rows, const double *item_bias,
                       int n_top, int32_t *items, T *scores, void *ws, size_t ws_bytes, hipStream_t st) {
    if (!code || !Dt || !items || !scores || (ex_indptr && !ex_indices) || !topn_args_ok<T>(p, k, b, n_top)) return MODL_EINVAL;
    if (b == 0) return MODL_OK;
    int64_t slab_items;
    const int S = topn_slabs<T>(p, b, &slab_items);
    const TopnWs w = topn_ws<T>(p, b, n_top, S);
    if (!ws || ws_bytes < w.total) return MODL_ENOMEM;
    if (modl_device_count() <= 0) return MODL_ENOGPU;
    char *base = static_cast<char *>(ws);
    unsigned int *mask = nullptr;
    if (ex_indptr) {
        mask = reinterpret_cast<unsigned int *>(base + w.mask);
        MODL_HIP(hipMemsetAsync(mask, 0, sizeof(unsigned int) * (size_t)b * w.W, st));
        MODL_TRY(launch_recsys_mask(st, ex_indptr, ex_indices, ex_rows, b, p, w.W, INT32_MAX, mask));
    }
    const TopnLds L = topn_lds<T>(k, n_top);
    int32_t *o_items = S == 1 ? items : reinterpret_cast<int32_t *>(base + w.part_items);
    T *o_scores = S == 1 ? scores : reinterpret_cast<T *>(base + w.part_scores);
    MODL_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&recsys_topn_kernel<T>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    hipLaunchKernelGGL((recsys_topn_kernel<T>), dim3((unsigned)cdiv(b, kTopnUsers), (unsigned)S), dim3(256), L.total, st,
                       code, code_rows, b, k, Dt, p, (const unsigned int *)mask, w.W, item_bias, n_top, slab_items, S,
                       o_items, o_scores, L);
    MODL_LAUNCH_CHECK();
    if (S > 1) {
        const size_t lds = (sizeof(T) + sizeof(int)) * (size_t)S * n_top;
        MODL_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&recsys_topn_merge_kernel<T>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        hipLaunchKernelGGL((recsys_topn_merge_kernel<T>), dim3((unsigned)b), dim3(64), lds, st,
                           (const int32_t *)o_items, (const T *)o_scores, S, n_top, items, scores);
        MODL_LAUNCH_CHECK();
    }
    return MODL_OK;
}

}  // namespace modl

using namespace modl;

extern "C" {

size_t modl_recsys_topn_workspace(int dtype, int64_t p, int k, int64_t b, int n_top) {
    if (dtype == MODL_F32) return topn_workspace<float>(p, k, b, n_top);
    if (dtype == MODL_F64) return topn_workspace<double>(p, k, b, n_top);
    return 0;
}

#define ABI_TOPN(SFX, T)                                                                                                  \
    int modl_recsys_topn_##SFX(const T *d_code, const int64_t *d_code_rows, int64_t b, int k, const T *d_Dt, int64_t p,      \
                               const int32_t *d_ex_indptr, const int32_t *d_ex_indices, const int64_t *d_ex_rows,          \
                               const double *d_item_bias, int n_top, int32_t *d_items, T *d_scores, void *d_ws,            \
                               size_t ws_bytes, void *stream) {                                                            \
        return recsys_topn<T>(d_code, d_code_rows, b, k, d_Dt, p, d_ex_indptr, d_ex_indices, d_ex_rows, d_item_bias,      \
                              n_top, d_items, d_scores, d_ws, ws_bytes, (hipStream_t)stream);                              \
    }
ABI_TOPN(f32, float)
ABI_TOPN(f64, double)
#undef ABI_TOPN

}  // extern "C"
