// The matrix-core products of the minibatch step and of the transform, routed: three pure host functions say which launches
// form them (kernels.hpp), somf_step.hip launches what they say, bcd.hip's plan_ride reads rider_route, and
// product_route_name spells a route as the string of tests/test_product_routes.py: expected_route.  Nothing here touches a
// device or reads a global: switches and flags are arguments.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>

#include "kernels.hpp"

namespace modl {

size_t split_scratch_elems(int64_t max_batch, int k, int64_t p) {
    const size_t b = (size_t)max_batch, kk = (size_t)k, pp = (size_t)p;
    size_t e = std::max(b, kk) * kk * 64;
    if (pp * kk < e) e = std::max(e, pp * kk * 8);
    return e;
}

// launch_gemm_dense's plan for operands with a unit stride and the plan's split-K scratch
static ProductLaunch product_launch(size_t tsz, bool unal_a, bool unal_b, int64_t M, int64_t N, int64_t K, size_t ws_elems) {
    return plan_product(tsz, true, unal_a, unal_b, M, N, K, ws_elems > 0, ws_elems);
}

// du_route's families DU_BLOCK and DU_PERSIST (bcd.hip), the only ones whose launches call plan_ride
bool du_carries_riders(size_t tsz, int k, int optimizer, int comp_pos, double comp_l1_ratio) {
    return optimizer != MODL_OPT_SGD && comp_l1_ratio == 0.0 && !comp_pos && tsz == 4 && k <= 512;
}

RiderRoute rider_route(bool proper_subset, bool dx_full, bool no_rider_flag, bool carried, int64_t p, int k, int b, int64_t ldx,
                       bool unal_x, bool unal_c) {
    RiderRoute r;
    // only the sampled rows of B_ are needed by the dictionary update -> the rest of the B_ update is deferred and rides
    // along its launches; the sampled features are stamped so that the rider leaves them alone
    // (not for very large feature counts: at p = 200 000 the p x k product is 26 GFLOP, the launches of the dictionary update
    // would wait for their riders - it runs as its own k-wide launch instead, X read once: 0.39 + 0.39 ms against 0.94 ms
    // riding, measured)
    r.why = !proper_subset ? RIDER_NO_PROPER_SUBSET : dx_full ? RIDER_DX_FULL : no_rider_flag ? RIDER_FLAG :
            rider_too_tall(p) ? RIDER_TOO_TALL : RIDER_RIDES;
    if (r.why != RIDER_RIDES) return r;
    // wide tiles (gemm_wide.hpp) keep their X tile in LDS for 128 atoms: X is fetched twice instead of eight times, and a
    // tile is still short enough for the shadow of a block step
    if (carried && p >= kRiderWideRows && plan_wide_ok(true, p, k, b, ldx, k, !unal_x, !unal_c))
        r.kind = RIDER_WIDE;
    else if (carried && p > 0 && plan_stats_ok(true, unal_x, unal_c, p, k, b))
        r.kind = RIDER_TILES32;
    else
        r.kind = RIDER_AFTER;
    return r;
}

StatsRoute stats_route(size_t tsz, int64_t M0, int64_t N, int64_t M1, int64_t K, bool unal_c, bool unal_x, int64_t ld1, StatsEpi epi,
                       bool stamps, bool resident_switch, size_t ws_elems) {
    StatsRoute r;
    r.unal = unal_c || unal_x;
    r.epi = epi;
    if (tsz == 4) {
        const bool p0 = plan_stats_ok(true, unal_c, unal_c, M0, N, K);
        // f32 operands: "off 16 bytes" is a misaligned base or a leading stride that is no multiple of 4 - plan_wide's conditions
        const bool wide = plan_wide_ok(true, M1, N, K, ld1, N, !unal_x, !unal_c);
        // a TALL second problem (the whole p x k product: reduction 1, or 200 000 features) with at most 256 atoms: persistent
        // workgroups with the code matrix resident in registers (gemm_resident.hpp)
        if (p0 && M1 >= kResidentMinRows && N <= 256 && K % 4 == 0 && !stamps && resident_switch && wide) { r.kind = STATS_RESIDENT; return r; }
        // a VERY tall second problem (where nothing rides any more): k-wide tiles, X read once (gemm_wide.hpp)
        if (p0 && rider_too_tall(M1) && !stamps && wide) { r.kind = STATS_WIDE_PAIR; return r; }
        if (p0 && plan_stats_ok(true, unal_x, unal_c, M1, N, K)) { r.kind = STATS_PAIR32; return r; }
    }
    bool ok0 = true;
    if (M0 > 0) {
        r.P0 = plan_dense_sizes(tsz, true, unal_c, unal_c, true, M0, N, K, false, 0);
        ok0 = r.P0.ok;
    }
    r.P1 = plan_dense_sizes(tsz, true, unal_x, unal_c, false, M1, N, K, false, 0, 512, 1, kStatBM, kStatBN);
    if (ok0 && r.P1.ok) { r.kind = STATS_DENSE_PAIR; return r; }
    r.kind = STATS_EACH;
    if (M0 > 0) r.C = product_launch(tsz, unal_c, unal_c, M0, N, K, ws_elems);
    r.B = product_launch(tsz, unal_x, unal_c, M1, N, K, ws_elems);
    return r;
}

CodeProductsRoute code_products_route(const modl_somf_desc &d, int b, int64_t s, bool has_subset, bool has_idx, int64_t ldx,
                                      const StepBases &al, size_t ws_elems) {
    CodeProductsRoute r;
    const size_t tsz = d.dtype == MODL_F32 ? 4 : 8;
    const int64_t vn = 16 / (int64_t)tsz, p = d.p;
    const int k = d.k;
    const bool dx_full = d.Dx_agg == MODL_AGG_FULL;
    // compaction: gather once, contract dense.  Ds = Dt[subset] (whole feature rows), Xs = X[:, subset].  With every feature
    // sampled nothing is copied.  One launch for the row norms and every gather.
    r.need_sub = has_subset && (!dx_full || d.G_agg != MODL_AGG_FULL);
    r.s_pad = (s + 3) / 4 * 4;
    r.n_norm = (d.code_l1_ratio != 0.0) ? b : 0;
    r.n_rows = r.need_sub ? (int)cdiv(s, kPrepRows) : 0;
    r.gx = (int)std::min<int64_t>(cdiv(r.s_pad, 256), 64);
    r.n_cols = (r.need_sub && !dx_full) ? r.gx * b : 0;
    // the column gather rides with the row norms when a row fits in LDS next to nothing else (<= 64 KB) and the rows are
    // 16-byte aligned
    r.fuse_cols = (r.n_cols > 0 && r.n_norm == b && tsz * (size_t)p <= 64 * 1024 && al.x && (ldx * tsz) % 16 == 0) ? 1 : 0;
    if (r.fuse_cols) r.n_cols = 0;
    const bool cd_on_compact = d.code_l1_ratio != 0.0 && d.G_agg != MODL_AGG_AVERAGE;
    r.n_code = (cd_on_compact && has_idx) ? (int)cdiv(b, kPrepRows) : 0;
    r.rider = rider_route(r.need_sub && s > 0 && s < p, dx_full, (d.flags & MODL_FLAG_NO_RIDER) != 0,
                          du_carries_riders(tsz, k, d.optimizer, d.comp_pos, d.comp_l1_ratio), p, k, b, ldx,
                          !al.x || ldx % vn != 0, !(has_idx || al.code) || k % vn != 0);
    // Dx = X . D^T over all of p, or X[:, subset] . D[:, subset]^T * reduction over the gathered (or given) columns
    r.x_gathered = r.need_sub && !dx_full;
    r.Kdim = dx_full ? p : s;
    const bool unal_a = r.x_gathered ? r.s_pad % vn != 0 : (!al.x || ldx % vn != 0);
    const bool unal_dt = !al.dt || k % vn != 0;
    const bool unal_d = r.need_sub ? k % vn != 0 : unal_dt;      // (Ds is the plan's; rows of k elements)
    const bool unal_b = dx_full ? unal_dt : unal_d;              // Dx's second operand: Dt over all of p, else the Gram's
    // the Dx product and the Gram product are independent: one launch (+ one for both split-K sums)
    r.want_G = d.G_agg != MODL_AGG_FULL;
    if (r.want_G && (r.x_gathered ? r.s_pad : ldx) != 1) {       // (the pair kernel takes A contiguous along the contraction only)
        const size_t half = ws_elems / 2;
        // the two products share the chip: 2 workgroups per compute unit in total (256 each) - with 512 each the split-K
        // partials double and the minibatch at reduction 1 takes 0.352 instead of 0.344 ms (same box), with 192 or 384 each
        // 0.354 / 0.358 ms
        constexpr int kPairTarget = 256;
        // (the Gram matrix is symmetric: only its tiles on and above the diagonal are computed, plan_dense `symmetric`)
        r.PG = plan_dense_sizes(tsz, true, unal_d, unal_d, true, k, k, s, ws_elems > 0, ws_elems - half, kPairTarget, 64, 64, 64, true);
        r.PD = plan_dense_sizes(tsz, true, unal_a, unal_b, false, b, k, r.Kdim, ws_elems > 0, half, kPairTarget);
        r.paired = r.PD.ok && r.PG.ok;
    }
    if (!r.paired) {
        r.Dx = product_launch(tsz, unal_a, unal_b, b, k, r.Kdim, ws_elems);
        if (r.want_G) r.G = product_launch(tsz, unal_d, unal_d, k, k, s, ws_elems);
    }
    r.g_average = d.G_agg == MODL_AGG_AVERAGE;
    r.track_G = d.G_agg == MODL_AGG_FULL;
    r.partial_G = r.track_G && gram_is_partial(s, p);
    if (r.track_G) r.gram = plan_gather(k, k, r.partial_G ? s : p, ws_elems > 0, ws_elems);
    return r;
}

// ---- the routes as strings --------------------------------------------------------------------------------------------
namespace {
std::string fmt(const char *f, long long a = 0, long long b = 0, long long c = 0) {
    char t[96];
    snprintf(t, sizeof t, f, a, b, c);
    return t;
}
std::string splits_str(int64_t K, int64_t splits, int64_t kps) {
    return fmt("s%lld/kps%lld/last%lld", (long long)splits, (long long)kps, (long long)(K - (splits - 1) * kps));
}
const char *tile_str(DenseTile t) { return t == TILE_RK ? "rk" : t == TILE_PIPE_RK_LAST ? "pipe+rk_last" : "pipe"; }
std::string dense_str(size_t tsz, const DensePlan &P, int64_t M, int64_t N, int64_t K, bool paired, int bm = 64, int bn = 64) {
    const int BK = dense_bk(tsz);
    const int64_t last = K - (int64_t)(P.splits - 1) * P.kps;
    const bool edge = M % bm || N % bn || P.kps % BK || last % BK;
    std::string s = "dense/";
    s += !(P.unal_a || P.unal_b) ? "al" : std::string("unal") + (P.unal_a ? "A" : "") + (P.unal_b ? "B" : "");
    s += fmt("/t%lldx%lld/", P.tm, P.tn) + (edge ? "edge/" : "interior/") + splits_str(K, P.splits, P.kps) + "/" +
         tile_str(dense_tile_of(tsz, bm, bn, K, P, paired));
    return s + (P.sym ? fmt("/sym1/ut%lld", P.tiles()) : std::string("/sym0"));
}
// (gemm_kernel: a tile of the tall configuration at least half full is staged densely, unless the operand is gathered on K)
std::string gather_str(const GatherPlan &G, int64_t M, int64_t N, int64_t K, bool gather_k) {
    static const char *names[] = {"big", "small", "tall"};
    std::string sa = "g", sb = "g";
    if (G.cfg == GATHER_TALL && !gather_k) {
        sa.clear(); sb.clear();
        for (int64_t m0 = 0; m0 < M; m0 += G.bm) sa += 2 * (M - m0) >= G.bm ? 'd' : 'g';
        for (int64_t n0 = 0; n0 < N; n0 += G.bn) sb += 2 * (N - n0) >= G.bn ? 'd' : 'g';
    }
    return std::string("gather/") + names[G.cfg] + fmt("/t%lldx%lld/", G.tm, G.tn) + splits_str(K, G.splits, G.kps) + "/A" + sa + "/B" + sb;
}
std::string launch_str(size_t tsz, const ProductLaunch &L, int64_t M, int64_t N, int64_t K) {
    return L.dense ? dense_str(tsz, L.d, M, N, K, false) : gather_str(L.g, M, N, K, false);
}
std::string stats_str(size_t tsz, const StatsRoute &r, int64_t M0, int64_t N, int64_t M1, int64_t K) {
    const char *al = r.unal ? "unal" : "al";
    switch (r.kind) {
    case STATS_RESIDENT: return std::string("resident16/") + (r.epi == STATS_EPI_VEC4 ? "vec4" : "scalar");
    case STATS_WIDE_PAIR: return fmt("wide32/c%lld", cdiv(N, 256));
    case STATS_PAIR32: return std::string("stats32/") + al + fmt("/t%lldx%lld", cdiv(M1, kStatsTile), cdiv(N, kStatsTile));
    case STATS_DENSE_PAIR: return std::string("densepair/") + al + "/" + tile_str(dense_tile_of(tsz, kStatBM, kStatBN, K, r.P1, true));
    case STATS_EACH: break;
    }
    std::string s = "each/";
    if (M0 > 0) s += "C[" + launch_str(tsz, r.C, M0, N, K) + "]/";
    return s + "B[" + launch_str(tsz, r.B, M1, N, K) + "]";
}
}  // namespace

int product_route_name(const modl_somf_desc &d, int section, int b, int64_t s, bool has_subset, bool has_idx, int64_t ldx,
                       int64_t x_offset, bool resident_switch, char *buf, size_t cap) {
    if (section < MODL_ROUTE_TRANSFORM || section > MODL_ROUTE_STATS || !buf) return MODL_EINVAL;
    const size_t tsz = d.dtype == MODL_F32 ? 4 : 8;
    const int64_t vn = 16 / (int64_t)tsz, p = d.p;
    const int k = d.k;
    const size_t ws = split_scratch_elems(d.max_batch, k, p);
    StepBases al;                                 // (buffers that the library or torch allocates are taken as aligned)
    al.x = (x_offset * (int64_t)tsz) % 16 == 0;
    const bool x_al = al.x;
    const bool unal_x = !x_al || ldx % vn != 0, unal_c = k % vn != 0;
    std::string out;
    if (section == MODL_ROUTE_FULL_GRAM) {
        out = gather_str(plan_gather(k, k, p, true, ws), k, k, p, false);
    } else {
        if (b <= 0 || b > d.max_batch || ldx < p) return MODL_EINVAL;
        if (section == MODL_ROUTE_TRANSFORM) {
            out = launch_str(tsz, product_launch(tsz, unal_x, unal_c, b, k, p, ws), b, k, p);
        } else {
            if (s < 0 || s > p || (!has_subset && s != p)) return MODL_EINVAL;
            const CodeProductsRoute c = code_products_route(d, b, s, has_subset, has_idx, ldx, al, ws);
            if (section == MODL_ROUTE_CODE_PRODUCTS) {
                out = c.need_sub ? "prep+" : "";
                if (c.paired) {
                    out += "pair/Dx[" + dense_str(tsz, c.PD, b, k, c.Kdim, true) + "]/G[" + dense_str(tsz, c.PG, k, k, s, true) + "]";
                } else {
                    out += "each/Dx[" + launch_str(tsz, c.Dx, b, k, c.Kdim) + "]";
                    if (c.want_G) out += "/G[" + launch_str(tsz, c.G, k, k, s) + "]";
                }
                if (c.track_G)
                    out += (c.partial_G ? "/partialG[" : "/fullG[") +
                           gather_str(c.gram, k, k, c.partial_G ? s : p, c.partial_G && has_subset) + "]";
            } else if (c.rider.kind != RIDER_NONE) {
                // C_ and the SAMPLED rows of B_ now (over the gathered columns of X), the other rows with the dictionary update
                const StatsRoute h = stats_route(tsz, k, k, s, b, unal_c, c.s_pad % vn != 0, c.s_pad, STATS_EPI_ROWS, (d.flags & MODL_FLAG_GEMM_STAMPS) != 0,
                                                 resident_switch, ws);
                out = stats_str(tsz, h, k, k, s, b) + "/ride:";
                if (c.rider.kind == RIDER_WIDE) out += "wide128";
                else if (c.rider.kind == RIDER_TILES32) out += std::string("stats32/") + (unal_x || unal_c ? "unal" : "al");
                else out += "after[" + stats_str(tsz, stats_route(tsz, 0, k, p, b, unal_c, unal_x, ldx, STATS_EPI_ROWS, false, resident_switch, ws),
                                                 0, k, p, b) + "]";
            } else {
                out = stats_str(tsz, stats_route(tsz, k, k, p, b, unal_c, unal_x, ldx, STATS_EPI_VEC4, false, resident_switch, ws), k, k, p, b) +
                      "/noride";
            }
        }
    }
    if (out.size() + 1 > cap) return MODL_EINVAL;
    std::memcpy(buf, out.c_str(), out.size() + 1);
    return MODL_OK;
}

}  // namespace modl
