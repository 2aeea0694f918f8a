// What the top-N kernel (recsys_topn.hip) and the rank kernels (recsys_rank.hip) share: the tile geometry, the total order
// of (score, item) pairs, the cut of the items into slabs - and the score itself: both files form score[ii][f] by calling
// topn_score_tile below on codes staged by topn_stage_codes, so a rank counted there is a position in the list made here.
#pragma once
#include "gemm.hpp"

namespace modl {

constexpr int kTopnUsers = 32;        // queries of a workgroup
constexpr int kTopnKC = 64;           // contraction chunk staged at a time
constexpr int kTopnMergeMin = 32;     // candidates of a query that trigger a merge
constexpr int kTopnMaxSlabs = 64;     // one list per lane of the merging wavefront
constexpr int kTopnMinSlab = 256;     // items: the shortest slab
constexpr int kTopnTargetWgs = 512;

template <typename T> struct TopnCfg;
template <> struct TopnCfg<float> { static constexpr int WN = 32, RM = 1, KMAX = 186; };     // items per wavefront and tile
template <> struct TopnCfg<double> { static constexpr int WN = 16, RM = 2, KMAX = 127; };

template <typename T> __device__ __forceinline__ bool topn_beats(T sa, int ia, T sb, int ib) {
    return sa > sb || (sa == sb && ia < ib);
}

// the dispatch: slabs of a call (stages of IT items per slab)
template <typename T> static int topn_slabs(int64_t p, int64_t b, int64_t *slab_items) {
    constexpr int IT = 4 * TopnCfg<T>::WN;
    const int64_t tiles = cdiv(b, kTopnUsers);
    int64_t want = kTopnTargetWgs / tiles;
    want = want < 1 ? 1 : (want > kTopnMaxSlabs ? kTopnMaxSlabs : want);
    const int64_t nst = cdiv(p, IT);
    int64_t sps = cdiv(nst, want);
    if (sps < kTopnMinSlab / IT) sps = kTopnMinSlab / IT;
    *slab_items = sps * IT;
    return (int)cdiv(nst, sps);
}

// The head of a sweep kernel's dynamic LDS: codes and dictionary tile, `t_elems` elements of T of the kernel's own (from
// *t0), the tile's biases (8-aligned), `i_elems` ints of the kernel's own (from *i0), the tile's exclusion words.
struct TopnTileLds { size_t cs, ds, bs, mk, total; int ldc, ldd; };
template <typename T> static TopnTileLds topn_tile_lds(int k, size_t t_elems, size_t i_elems, size_t *t0, size_t *i0) {
    constexpr int IT = 4 * TopnCfg<T>::WN, TK = Mma<T>::TK;
    const int kp = (k + TK - 1) / TK * TK;
    TopnTileLds L;
    L.ldc = kp | 1;
    L.ldd = (kp < kTopnKC ? kp : kTopnKC) | 1;
    size_t o = 0;
    L.cs = o; o += sizeof(T) * (size_t)kTopnUsers * L.ldc;
    L.ds = o; o += sizeof(T) * (size_t)IT * L.ldd;
    *t0 = o; o += sizeof(T) * t_elems;
    o = align_up(o, 8);
    L.bs = o; o += sizeof(double) * IT;
    *i0 = o; o += sizeof(int) * i_elems;
    L.mk = o; o += sizeof(unsigned int) * kTopnUsers * (IT / 32);
    L.total = align_up(o, 16);
    return L;
}

// one wavefront per query ORs the first `limit` entries of its CSR row into the query's bitmask of p bits (W words, zeroed
// before).  An OR commutes: duplicates and unsorted indices cost nothing and no order depends on an atomic.
int launch_recsys_mask(hipStream_t st, const int32_t *indptr, const int32_t *indices, const int64_t *rows, int64_t b,
                       int64_t p, int64_t W, int limit, unsigned int *mask);

// the codes of the workgroup's queries u0 .. u0 + 31 into Cs[m * ldc + c] (zero beyond b and beyond k)
template <typename T>
__device__ __forceinline__ void topn_stage_codes(T *Cs, int ldc, const T *code, const int64_t *code_rows, int64_t u0,
                                                 int64_t b, int k) {
    for (int e = threadIdx.x; e < kTopnUsers * ldc; e += 256) {
        const int m = e / ldc, c = e % ldc;
        const int64_t ii = u0 + m < b ? u0 + m : b - 1;
        const int64_t row = code_rows ? code_rows[ii] : ii;
        const T v = code[row * k + (c < k ? c : 0)];
        Cs[e] = (u0 + m < b && c < k) ? v : (T)0;
    }
}

// how the 256 threads share the staging of a tile of Dt: lpr lanes walk one dictionary row (kp = k rounded up to the MFMA's
// K), rpp rows per pass; this thread starts at row `sub`, column c0
struct TopnSplit { int kp, lpr, rpp, sub, c0; };
template <typename T> __device__ __forceinline__ TopnSplit topn_split(int k) {
    TopnSplit s;
    s.kp = (k + Mma<T>::TK - 1) / Mma<T>::TK * Mma<T>::TK;
    s.lpr = s.kp > 32 ? 64 : (s.kp > 16 ? 32 : 16);
    s.rpp = 256 / s.lpr;
    s.sub = threadIdx.x / s.lpr;
    s.c0 = threadIdx.x % s.lpr;
    return s;
}

// The score tile of a workgroup: its 32 queries against the IT items from item0, without the bias.  Wavefront wid holds
// acc[i][r] = sum_c code[u0 + i TM + acc_row(lane, r)][c] * Dt[item0 + wid WN + acc_col(lane, 0)][c], one accumulator
// chain, c ascending.  K in chunks of kTopnKC through Ds (split `sp` of the staging, formed once per kernel by topn_split:
// its divisions stay out of the tile loop; clamped loads, zeros selected
// for items beyond f_end and c beyond k); with the first chunk the tile's exclusion words go to mk[m * IT / 32 + w] and
// its biases to bs[IT].  Each chunk begins with a barrier (the workgroup is done with the tile before, and with whatever
// the caller wrote to LDS) and has one between staging and product; none follows the last product.
template <typename T>
__device__ __forceinline__ void topn_score_tile(typename Mma<T>::acc_t (&acc)[TopnCfg<T>::RM], const T *Cs, T *Ds,
                                                unsigned int *mk, double *bs, int ldc, int ldd, const T *Dt, int64_t p,
                                                int k, const unsigned int *mask, int64_t W, const double *item_bias,
                                                int64_t item0, int64_t f_end, int64_t u0, int64_t b, const TopnSplit &sp) {
    using MT = Mma<T>;
    constexpr int WN = TopnCfg<T>::WN, RM = TopnCfg<T>::RM, IT = 4 * WN, MW = IT / 32;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int kp = sp.kp, lpr = sp.lpr, rpp = sp.rpp, sub = sp.sub, c0 = sp.c0;
#pragma unroll
    for (int i = 0; i < RM; ++i)
#pragma unroll
        for (int r = 0; r < MT::NACC; ++r) acc[i][r] = 0;
    for (int kc0 = 0; kc0 < kp; kc0 += kTopnKC) {
        const int kcn = kp - kc0 < kTopnKC ? kp - kc0 : kTopnKC;
        __syncthreads();
        if (kc0 == 0) {
            if (tid < kTopnUsers * MW) {
                const int m = tid / MW, w = tid % MW;
                const int64_t ii = u0 + m < b ? u0 + m : b - 1;
                const int64_t word = item0 / 32 + w;
                mk[tid] = (mask && word < W) ? mask[ii * W + word] : 0u;
            }
            if (tid < IT) {
                const int64_t f = item0 + tid < p ? item0 + tid : p - 1;
                bs[tid] = item_bias ? item_bias[f] : 0.0;
            }
        }
        for (int c = c0; c < kcn; c += lpr) {
            const int cc = kc0 + c;
            for (int it0 = sub; it0 < IT; it0 += 8 * rpp) {
                int64_t off[8];                              // all eight addresses, then all eight loads: one round trip
                T v[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const int64_t f = item0 + it0 + q * rpp;
                    off[q] = (f < p ? f : p - 1) * k + (cc < k ? cc : 0);
                }
#pragma unroll
                for (int q = 0; q < 8; ++q) v[q] = Dt[off[q]];
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const int item = it0 + q * rpp;
                    if (item < IT) Ds[item * ldd + c] = (item0 + item < f_end && cc < k) ? v[q] : (T)0;
                }
            }
        }
        __syncthreads();
        for (int kk = 0; kk < kcn; kk += MT::TK) {
            const int kr = kk + MT::frag_k(lane);
            const T bf = Ds[(wid * WN + MT::frag_i(lane)) * ldd + kr];
#pragma unroll
            for (int i = 0; i < RM; ++i) {
                const T af = Cs[(i * MT::TM + MT::frag_i(lane)) * ldc + kc0 + kr];
                acc[i] = MT::mma(af, bf, acc[i]);
            }
        }
    }
}

}  // namespace modl
