// What the matrix-core products decide before they launch, as plain host functions of sizes, the element size, alignment
// facts and scratch: no epilogue, no pointer, no device.  The templates of gemm.hpp, gemm_dense.hpp and gemm_wide.hpp copy
// these results into their problem structs and attach the epilogue; the route functions of step_products.hip ask the same
// functions "what would you do".
#pragma once
#include "common.hpp"

namespace modl {

// ---- the dense kernels (gemm_dense.hpp) ---------------------------------------------------------------------------
constexpr int dense_bk(size_t tsz) { return tsz == 4 ? 32 : 16; }     // K-tile of the dense kernels
constexpr int kDenseRkTiles = 8;          // gemm_dense_tile_auto: a split of at most this many K-tiles stays resident (f32)

struct DensePlan {
    bool ok = false;                      // eligible for the dense kernels
    bool unal_a = false, unal_b = false;  // operand staged element by element (base or leading stride off 16 bytes)
    int tm = 0, tn = 0, splits = 1, sym = 0;
    int64_t kps = 0;
    int tiles() const { return sym ? tm * (tm + 1) / 2 : tn * tm; }
};

// contiguous: both operands have a unit stride; unal_*: operand not on a 16-byte base or leading stride not a multiple of
// 16 bytes; same_operand: A and B are the same array with the same strides; has_ws / ws_elems: split-K scratch
inline DensePlan plan_dense_sizes(size_t tsz, bool contiguous, bool unal_a, bool unal_b, bool same_operand, int64_t M, int64_t N,
                                  int64_t K, bool has_ws, size_t ws_elems, int target_wgs = 512, int max_splits = 64, int bm = 64,
                                  int bn = 64, bool symmetric = false) {
    DensePlan P;
    P.ok = contiguous && K > 0 && M > 0 && N > 0;
    if (!P.ok) return P;
    P.unal_a = unal_a;
    P.unal_b = unal_b;
    // (small misaligned products stay with the gather kernel: nothing to gain, and the toy-sized golden trajectories
    //  recorded from the reference keep the summation order they were validated with)
    if ((unal_a || unal_b) && M * N * K < (int64_t)1 << 22) { P.ok = false; return P; }
    const int BK = dense_bk(tsz);
    const int64_t tm = cdiv(M, bm), tn = cdiv(N, bn);
    const bool sym = symmetric && M == N && bm == bn && same_operand;
    const int64_t ntile = sym ? tm * (tm + 1) / 2 : tm * tn;
    int64_t splits = 1;
    if (ntile < target_wgs && max_splits > 1 && has_ws) {
        splits = target_wgs / ntile;
        const int64_t max_by_k = K / (4 * BK) > 0 ? K / (4 * BK) : 1;       // >= 4 k-tiles per split
        if (splits > max_by_k) splits = max_by_k;
        if (splits > max_splits) splits = max_splits;
        const int64_t max_by_ws = (int64_t)ws_elems / (M * N);
        if (splits > max_by_ws) splits = max_by_ws;
        if (splits < 1) splits = 1;
    }
    P.kps = cdiv(cdiv(K, splits), BK) * BK;
    P.splits = (int)cdiv(K, P.kps);
    P.tn = (int)tn; P.tm = (int)tm;
    P.sym = (sym && P.splits > 1) ? 1 : 0;              // (a direct store would need the mirrored epilogue: split-K only)
    return P;
}

// Which tile a planned product runs (the device decides it split by split in gemm_dense_tile_auto; launch_gemm_dense's own
// kernel is always pipelined): the pipelined tile, the resident-K tile, or pipelined tiles with a short last split resident.
enum DenseTile { TILE_PIPE, TILE_RK, TILE_PIPE_RK_LAST };
inline DenseTile dense_tile_of(size_t tsz, int bm, int bn, int64_t K, const DensePlan &P, bool paired) {
    if (!paired || tsz != 4 || bm > 64 || bn > 64) return TILE_PIPE;
    const int64_t rk = (int64_t)kDenseRkTiles * dense_bk(tsz);
    if (P.kps <= rk) return TILE_RK;
    return (P.splits > 1 && K - (int64_t)(P.splits - 1) * P.kps <= rk) ? TILE_PIPE_RK_LAST : TILE_PIPE;
}

// ---- the statistics tiles (gemm_dense.hpp: plan_stats) and the k-wide tiles (gemm_wide.hpp: plan_wide), f32 ----------------
constexpr int kStatsTile = 32, kStatsBK = 64, kStatsNKT = 4;
constexpr int kWideBK = 32, kWideKmax = 256;
// rows_contiguous: both operands contiguous along their rows (si == 1)
inline bool plan_stats_ok(bool rows_contiguous, bool unal_a, bool unal_b, int64_t M, int64_t N, int64_t K) {
    if (M <= 0 || N <= 0) return true;
    return plan_dense_sizes(4, true, unal_a, unal_b, false, M, N, K, false, 0, 512, 1, kStatsTile, kStatsTile).ok && rows_contiguous &&
           K <= (int64_t)kStatsNKT * kStatsBK;
}
// lda / ldb: leading strides; base_*_aligned: the operand starts on a 16-byte boundary
inline bool plan_wide_ok(bool rows_contiguous, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, bool base_a_aligned,
                         bool base_b_aligned) {
    return rows_contiguous && M > 0 && N > 0 && K > 0 && K <= kWideKmax && M % 4 == 0 && N % 4 == 0 && lda % 4 == 0 && ldb % 4 == 0 &&
           base_a_aligned && base_b_aligned;
}

// ---- the gather kernel (gemm.hpp: launch_gemm) --------------------------------------------------------------------
constexpr int kGatherBK = 16, kGatherBKTall = 32;   // (TileCfg<T>::BK, BKT: the same for both types)
enum GatherCfg { GATHER_BIG = 0, GATHER_SMALL = 1, GATHER_TALL = 2 };   // 128 x 128, 64 x 64, 128 x 32
struct GatherPlan {
    int cfg = GATHER_SMALL, bm = 64, bn = 64, bk = kGatherBK;
    int64_t tm = 0, tn = 0, splits = 1, kps = 0;
};
inline GatherPlan plan_gather(int64_t M, int64_t N, int64_t K, bool has_ws, size_t ws_elems, int target_wgs = 512, int max_splits = 64) {
    GatherPlan P;
    if (N <= 32) { P.cfg = GATHER_TALL; P.bm = 128; P.bn = 32; }
    else if (cdiv(M, 128) * cdiv(N, 128) >= 512) { P.cfg = GATHER_BIG; P.bm = 128; P.bn = 128; }
    else { P.cfg = GATHER_SMALL; P.bm = 64; P.bn = 64; }
    P.tm = cdiv(M, P.bm); P.tn = cdiv(N, P.bn);
    int64_t splits = 1;
    if (K > 0 && P.tm * P.tn < target_wgs && max_splits > 1 && has_ws) {
        splits = target_wgs / (P.tm * P.tn);
        const int64_t max_by_k = K / (8 * kGatherBK) > 0 ? K / (8 * kGatherBK) : 1;   // >= 8 k-tiles per split
        if (splits > max_by_k) splits = max_by_k;
        if (splits > max_splits) splits = max_splits;
        const int64_t max_by_ws = (int64_t)ws_elems / (M * N);
        if (splits > max_by_ws) splits = max_by_ws;
        if (splits < 1) splits = 1;
    }
    const int64_t Kp = K > 0 ? K : 1;
    P.bk = (P.cfg == GATHER_TALL) ? kGatherBKTall : kGatherBK;
    P.kps = cdiv(cdiv(Kp, splits), P.bk) * P.bk;
    P.splits = cdiv(Kp, P.kps);
    return P;
}

// launch_gemm_dense: the dense kernel where plan_dense_sizes takes the product, else the gather kernel (M, N > 0)
struct ProductLaunch {
    bool dense = false;
    DensePlan d;
    GatherPlan g;
    int splits() const { return dense ? d.splits : (int)g.splits; }
};
inline ProductLaunch plan_product(size_t tsz, bool contiguous, bool unal_a, bool unal_b, int64_t M, int64_t N, int64_t K, bool has_ws,
                                  size_t ws_elems, int target_wgs = 512, int max_splits = 64) {
    ProductLaunch L;
    L.d = plan_dense_sizes(tsz, contiguous, unal_a, unal_b, false, M, N, K, has_ws, ws_elems, target_wgs, max_splits);
    L.dense = L.d.ok;
    if (!L.dense) L.g = plan_gather(M, N, K, has_ws, ws_elems, target_wgs, max_splits);
    return L;
}

}  // namespace modl
