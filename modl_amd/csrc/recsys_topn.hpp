// What the top-N kernel (recsys_topn.hip) and the rank kernels (recsys_rank.hip) share: the tile geometry, the total order
// of (score, item) pairs and the cut of the items into slabs.  Both files form score[ii][f] with the same Mma<T> chain over
// these tiles, so a rank counted there is a position in the list made here.
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

}  // namespace modl
