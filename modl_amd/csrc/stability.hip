// Amari discrepancy between dictionaries (the reference's modl/decomposition/stability.py:7-31).
//
// For dictionaries D_a (k_a x p) and D_b (k_b x p), atoms in rows:
//   C[i, j] = (D_a[i] . D_b[j]) / ||D_a[i]|| / ||D_b[j]||
//   d(a, b) = 0.5 * ( mean_j (1 - max_i C[i, j]) + mean_i (1 - max_j C[i, j]) )
// for every pair a < b of a list, in the reference's generator order (a outer, b inner).
//
// Three launches, four with a K split, whatever the number of dictionaries:
//   1. amari_norm_kernel    every atom norm of every dictionary, once (f64 accumulation, one wavefront per atom);
//   2. amari_pair_kernel    a flat work list of (pair, tile row, tile column, K split) built on the host: a C tile
//                           D_a-tile . D_b-tile^T on the matrix cores (gemm_dense.hpp's pipelined K-contiguous tile);
//                           unsplit, the tile is scaled in LDS and reduced to its per-row and per-column maxima;
//                           split, the raw partial tile goes to the workspace;
//   3. amari_combine_kernel (split only) sums the partial tiles of a tile in split order, scales, reduces;
//   4. amari_reduce_kernel  per pair: maxima over the tile records, the two means in f64 -> d.
// The k_a x k_b matrix itself never reaches HBM.  No atomics, no cross-workgroup waits: every sum has a fixed order
// and the result is bit-identical from run to run.
//
// NaN: the maxima propagate NaN (ndarray.max does; an fmax would drop it), so a zero atom (0 / 0) or a NaN in an
// input reaches the row / column maxima and d exactly as in numpy.  A maximum that is NaN is its own flag.
#include "gemm_dense.hpp"
#include <algorithm>
#include <cstring>
#include <vector>

namespace modl {
namespace {

struct AmDict { const void *ptr; int64_t k; int64_t noff; int64_t unal; };   // noff: first atom in the norm vector
struct AmPair { int a, b, tr, tc; int64_t tile0, roff, coff; };               // tr x tc tiles from tile0 on
struct AmTile { int pair, ti, tj, pad; };

template <typename T> struct AmCfg;
// f32: 128 x 128 tiles (4 wavefronts, each 2 x 2 v_mfma_f32_32x32x2_f32 tiles): 32 flop per byte of operand
// traffic; LDS 2 x 2 x 32 x 132 x 4 B = 66 KiB -> two workgroups per CU.
template <> struct AmCfg<float> { static constexpr int BM = 128, BK = 32; };
// f64: 64 x 64 tiles (each wavefront 2 x 2 v_mfma_f64_16x16x4_f64 tiles); the 128-tile would need 132 KiB of LDS.
template <> struct AmCfg<double> { static constexpr int BM = 64, BK = 32; };

constexpr int kStripRows = 4;          // rows of a tile per workgroup of the combine kernel
constexpr int kTargetItems = 512;      // the work list is K-split until it has about this many items (2 per CU)
constexpr int64_t kMinSplitK = 4096;   // ... but no split is shorter than this (the image example, p = 3 072: unsplit)
constexpr int64_t kMaxPartialBytes = (int64_t)256 << 20;

template <typename T> __device__ __forceinline__ T amax(T a, T b) {   // NaN-propagating maximum (ndarray.max)
    return (a != a) ? a : ((b != b) ? b : (b > a ? b : a));
}

// ---- 1. norms ----------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void amari_norm_kernel(const AmDict *__restrict__ dicts, int n, int64_t total,
                                                         int64_t p, T *__restrict__ norms) {
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= total) return;                                  // wavefront-uniform
    int lo = 0, hi = n - 1;                                  // the dictionary holding atom g
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (dicts[mid].noff <= g) lo = mid; else hi = mid - 1;
    }
    const T *row = static_cast<const T *>(dicts[lo].ptr) + (g - dicts[lo].noff) * p;
    double s[4] = {0, 0, 0, 0};
    int64_t e = lane;
    for (; e + 192 < p; e += 256) {
#pragma unroll
        for (int u = 0; u < 4; ++u) { const double x = (double)row[e + 64 * u]; s[u] += x * x; }
    }
    for (; e < p; e += 64) { const double x = (double)row[e]; s[0] += x * x; }
    const double t = wave_sum((s[0] + s[1]) + (s[2] + s[3]));
    if (lane == 0) norms[g] = (T)sqrt(t);
}

// ---- 2. pair tiles -----------------------------------------------------------------------------------------------
// Epilogue of the tile: unsplit, the scaled value goes to the LDS tile (row stride BM + 1); split, the raw partial sum
// to the workspace.  Called for in-range elements only.
template <typename T, int BM> struct AmEpi {
    T *lds = nullptr, *part = nullptr;
    const T *na = nullptr, *nb = nullptr;
    int64_t m0 = 0, n0 = 0;
    __device__ __forceinline__ void operator()(int64_t m, int64_t n, T v) const {
        const int r = (int)(m - m0), c = (int)(n - n0);
        if (part) part[r * BM + c] = v;
        else lds[r * (BM + 1) + c] = (v / na[m]) / nb[n];      // the reference's order: / ||D_a[i]||, then / ||D_b[j]||
    }
};

template <typename T>
__global__ __launch_bounds__(256) void amari_pair_kernel(const AmDict *__restrict__ dicts, const AmPair *__restrict__ pairs,
                                                         const AmTile *__restrict__ tiles, const T *__restrict__ norms,
                                                         int64_t p, int64_t kps, int nsplit, T *__restrict__ rowrec,
                                                         T *__restrict__ colrec, T *__restrict__ partial) {
    constexpr int BM = AmCfg<T>::BM, BK = AmCfg<T>::BK;
    constexpr size_t kOpBytes = sizeof(T) * 2 * BK * (BM + 4);
    static_assert(sizeof(T) * BM * (BM + 1) <= 2 * kOpBytes, "the C tile reuses the operand tiles' LDS");
    __shared__ __attribute__((aligned(16))) char smem[2 * kOpBytes];
    const int64_t tile = (int64_t)blockIdx.x / nsplit;
    const int s = (int)((int64_t)blockIdx.x % nsplit);
    const AmTile t = tiles[tile];
    const AmPair pr = pairs[t.pair];
    const AmDict da = dicts[pr.a], db = dicts[pr.b];
    DenseOperand A, B;
    A.ptr = da.ptr; A.si = p; A.sk = 1; A.unal = da.unal != 0;
    B.ptr = db.ptr; B.si = p; B.sk = 1; B.unal = db.unal != 0;
    const int64_t m0 = (int64_t)t.ti * BM, n0 = (int64_t)t.tj * BM;
    AmEpi<T, BM> epi;
    epi.m0 = m0; epi.n0 = n0;
    if (nsplit > 1) {
        epi.part = partial + (tile * nsplit + s) * (int64_t)(BM * BM);
    } else {
        epi.lds = reinterpret_cast<T *>(smem);
        epi.na = norms + da.noff;
        epi.nb = norms + db.noff;
    }
    // the tile loop ends with a barrier: the epilogue may overwrite the operand tiles
    gemm_dense_tile<T, false, false, AmEpi<T, BM>, BM, BM, BK>(
        A, B, da.k, db.k, p, kps, nullptr, epi, t.tj, t.ti, s, 1, reinterpret_cast<T(*)[BK][BM + 4]>(smem),
        reinterpret_cast<T(*)[BK][BM + 4]>(smem + kOpBytes));
    if (nsplit > 1) return;
    __syncthreads();
    const int mr = (int)std::min<int64_t>(BM, da.k - m0), nc = (int)std::min<int64_t>(BM, db.k - n0);
    const T *S = reinterpret_cast<const T *>(smem);
    const int x = threadIdx.x;
    T m = -INFINITY;
    if (x < BM) {                         // row maxima: thread x walks row x (stride BM + 1: conflict-free)
        if (x < mr) {
            for (int c = 0; c < nc; ++c) m = amax(m, S[x * (BM + 1) + c]);
            rowrec[tile * BM + x] = m;
        }
    } else if (x < 2 * BM) {              // column maxima
        const int c = x - BM;
        if (c < nc) {
            for (int r = 0; r < mr; ++r) m = amax(m, S[r * (BM + 1) + c]);
            colrec[tile * BM + c] = m;
        }
    }
}

// ---- 3. split combine: one workgroup of BM threads per kStripRows rows of a tile ---------------------------------
template <typename T>
__global__ __launch_bounds__(128) void amari_combine_kernel(const AmDict *__restrict__ dicts, const AmPair *__restrict__ pairs,
                                                            const AmTile *__restrict__ tiles, const T *__restrict__ norms,
                                                            int nsplit, const T *__restrict__ partial,
                                                            T *__restrict__ rowrec, T *__restrict__ colrec) {
    constexpr int BM = AmCfg<T>::BM, R = kStripRows, NS = BM / R;
    __shared__ T vals[R][BM + 1];
    const int64_t tile = (int64_t)blockIdx.x / NS;
    const int strip = (int)((int64_t)blockIdx.x % NS);
    const AmTile t = tiles[tile];
    const AmPair pr = pairs[t.pair];
    const AmDict da = dicts[pr.a], db = dicts[pr.b];
    const int64_t m0 = (int64_t)t.ti * BM, n0 = (int64_t)t.tj * BM;
    const int mr = (int)std::min<int64_t>(BM, da.k - m0), nc = (int)std::min<int64_t>(BM, db.k - n0);
    const int r0 = strip * R;
    if (r0 >= mr) return;                                    // workgroup-uniform
    const int c = threadIdx.x;
    const int nr = std::min(R, mr - r0);
    if (c < nc) {
        T acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = 0;
        const T *src = partial + tile * nsplit * (int64_t)(BM * BM) + (int64_t)r0 * BM + c;
        for (int q = 0; q < nsplit; ++q)                     // split order: fixed
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (r < nr) acc[r] += src[(int64_t)q * BM * BM + r * BM];
        const T nb = norms[db.noff + n0 + c];
        T m = -INFINITY;
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (r < nr) {
                const T v = (acc[r] / norms[da.noff + m0 + r0 + r]) / nb;
                vals[r][c] = v;
                m = amax(m, v);
            }
        colrec[(tile * NS + strip) * BM + c] = m;
    }
    __syncthreads();
    if (c < nr) {
        T m = -INFINITY;
        for (int j = 0; j < nc; ++j) m = amax(m, vals[c][j]);
        rowrec[tile * BM + r0 + c] = m;
    }
}

// ---- 4. per-pair discrepancy -------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void amari_reduce_kernel(const AmDict *__restrict__ dicts, const AmPair *__restrict__ pairs,
                                                           int nstrip, const T *__restrict__ rowrec,
                                                           const T *__restrict__ colrec, double *__restrict__ d_pair,
                                                           T *__restrict__ rowmax, T *__restrict__ colmax) {
    constexpr int BM = AmCfg<T>::BM;
    __shared__ double red[2][256];
    const AmPair pr = pairs[blockIdx.x];
    const int64_t ka = dicts[pr.a].k, kb = dicts[pr.b].k;
    double sr = 0, sc = 0;
    for (int64_t i = threadIdx.x; i < ka; i += 256) {        // max over j: the tile records of row band i / BM
        const int64_t ti = i / BM;
        T m = -INFINITY;
        for (int tj = 0; tj < pr.tc; ++tj) m = amax(m, rowrec[(pr.tile0 + ti * pr.tc + tj) * BM + i % BM]);
        if (rowmax) rowmax[pr.roff + i] = m;
        sr += 1.0 - (double)m;
    }
    for (int64_t j = threadIdx.x; j < kb; j += 256) {        // max over i: the tile records (and strips) of column band j / BM
        const int64_t tj = j / BM;
        T m = -INFINITY;
        for (int ti = 0; ti < pr.tr; ++ti) {
            const int mr = (int)std::min<int64_t>(BM, ka - (int64_t)ti * BM);
            const int ns = nstrip == 1 ? 1 : (mr + kStripRows - 1) / kStripRows;
            const T *rec = colrec + (pr.tile0 + ti * pr.tc + tj) * nstrip * BM + j % BM;
            for (int q = 0; q < ns; ++q) m = amax(m, rec[q * BM]);
        }
        if (colmax) colmax[pr.coff + j] = m;
        sc += 1.0 - (double)m;
    }
    red[0][threadIdx.x] = sr;
    red[1][threadIdx.x] = sc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {                      // fixed tree
        if ((int)threadIdx.x < w) {
            red[0][threadIdx.x] += red[0][threadIdx.x + w];
            red[1][threadIdx.x] += red[1][threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) d_pair[blockIdx.x] = 0.5 * (red[1][0] / (double)kb + red[0][0] / (double)ka);
}

// ---- host plan ---------------------------------------------------------------------------------------------------
struct AmPlan {
    int64_t npairs = 0, ntiles = 0, sum_k = 0, nsplit = 1, kps = 0, nstrip = 1;
    size_t off_pairs = 0, off_tiles = 0, off_norms = 0, off_row = 0, off_col = 0, off_part = 0, bytes = 0;
};

int am_plan(int dtype, int n, const int64_t *h_k, int64_t p, AmPlan &pl, std::vector<AmPair> *pairs,
            std::vector<AmTile> *tiles) {
    if ((dtype != MODL_F32 && dtype != MODL_F64) || n < 2 || !h_k || p <= 0) return MODL_EINVAL;
    for (int i = 0; i < n; ++i)
        if (h_k[i] <= 0 || h_k[i] > INT32_MAX) return MODL_EINVAL;
    const int BM = dtype == MODL_F32 ? AmCfg<float>::BM : AmCfg<double>::BM;
    const int BK = dtype == MODL_F32 ? AmCfg<float>::BK : AmCfg<double>::BK;
    const size_t es = dtype == MODL_F32 ? 4 : 8;
    pl = AmPlan();
    for (int i = 0; i < n; ++i) pl.sum_k += h_k[i];
    int64_t roff = 0, coff = 0;
    for (int a = 0; a + 1 < n; ++a)
        for (int b = a + 1; b < n; ++b) {
            AmPair q;
            q.a = a; q.b = b;
            q.tr = (int)cdiv(h_k[a], BM); q.tc = (int)cdiv(h_k[b], BM);
            q.tile0 = pl.ntiles; q.roff = roff; q.coff = coff;
            if (tiles)
                for (int ti = 0; ti < q.tr; ++ti)
                    for (int tj = 0; tj < q.tc; ++tj) tiles->push_back(AmTile{(int)pl.npairs, ti, tj, 0});
            if (pairs) pairs->push_back(q);
            pl.ntiles += (int64_t)q.tr * q.tc;
            roff += h_k[a]; coff += h_k[b];
            ++pl.npairs;
        }
    // K split: only when the tiles alone leave the chip idle, never below kMinSplitK per split, partials capped
    int64_t ns = 1;
    if (pl.ntiles < kTargetItems) {
        ns = std::min<int64_t>(cdiv(kTargetItems, pl.ntiles), p / kMinSplitK);
        // (a guard that cannot bind at these constants: t < 512 tiles take at most ceil(512 / t) splits, under 1 023
        //  tile-splits of BM * BM * es = 64 KiB (f32) or 32 KiB (f64), 64 MiB in all, and floor(4096 / t) >= ceil(512 / t) for
        //  every such t - tests/test_stability_routes.py::test_partial_cap_cannot_bind enumerates them.  It stays for the day
        //  kTargetItems, the tile size or the cap changes.)
        ns = std::min<int64_t>(ns, kMaxPartialBytes / (pl.ntiles * BM * BM * (int64_t)es));
        ns = std::max<int64_t>(ns, 1);
    }
    pl.kps = cdiv(cdiv(p, ns), BK) * BK;
    pl.nsplit = cdiv(p, pl.kps);                             // every split non-empty
    pl.nstrip = pl.nsplit > 1 ? BM / kStripRows : 1;
    if (pl.ntiles * pl.nsplit > INT32_MAX || pl.ntiles * (BM / kStripRows) > INT32_MAX) return MODL_EINVAL;
    size_t off = align_up(sizeof(AmDict) * (size_t)n, 256);
    pl.off_pairs = off; off = align_up(off + sizeof(AmPair) * (size_t)pl.npairs, 256);
    pl.off_tiles = off; off = align_up(off + sizeof(AmTile) * (size_t)pl.ntiles, 256);
    pl.off_norms = off; off = align_up(off + es * (size_t)pl.sum_k, 256);
    pl.off_row = off;   off = align_up(off + es * (size_t)(pl.ntiles * BM), 256);
    pl.off_col = off;   off = align_up(off + es * (size_t)(pl.ntiles * pl.nstrip * BM), 256);
    pl.off_part = off;
    if (pl.nsplit > 1) off = align_up(off + es * (size_t)(pl.ntiles * pl.nsplit * BM * BM), 256);
    pl.bytes = off;
    return MODL_OK;
}

template <typename T>
int amari_run(const T *const *h_d_dicts, const int64_t *h_k, int n, int64_t p, double *d_pair, T *d_rowmax,
              T *d_colmax, void *d_ws, size_t ws_bytes, void *stream, int *launches) {
    constexpr int BM = AmCfg<T>::BM;
    const int dtype = sizeof(T) == 4 ? MODL_F32 : MODL_F64;
    AmPlan pl;
    std::vector<AmPair> pairs;
    std::vector<AmTile> tiles;
    if (launches) *launches = 0;
    if (!h_d_dicts || !d_pair) return MODL_EINVAL;
    MODL_TRY(am_plan(dtype, n, h_k, p, pl, nullptr, nullptr));
    for (int i = 0; i < n; ++i)
        if (!h_d_dicts[i]) return MODL_EINVAL;
    if (!d_ws || ws_bytes < pl.bytes) return MODL_ENOMEM;
    if (modl_device_count() <= 0) return MODL_ENOGPU;
    am_plan(dtype, n, h_k, p, pl, &pairs, &tiles);
    // the host tables: dictionaries, pairs, tiles, copied in one transfer
    std::vector<char> host(pl.off_norms, 0);
    int64_t noff = 0;
    for (int i = 0; i < n; ++i) {
        const bool unal = (p * (int64_t)sizeof(T)) % 16 != 0 || ((uintptr_t)h_d_dicts[i] & 15) != 0;
        AmDict d{h_d_dicts[i], h_k[i], noff, unal ? 1 : 0};
        memcpy(host.data() + sizeof(AmDict) * i, &d, sizeof d);
        noff += h_k[i];
    }
    memcpy(host.data() + pl.off_pairs, pairs.data(), sizeof(AmPair) * pairs.size());
    memcpy(host.data() + pl.off_tiles, tiles.data(), sizeof(AmTile) * tiles.size());
    char *ws = static_cast<char *>(d_ws);
    const AmDict *dd = reinterpret_cast<const AmDict *>(ws);
    const AmPair *dp = reinterpret_cast<const AmPair *>(ws + pl.off_pairs);
    const AmTile *dt = reinterpret_cast<const AmTile *>(ws + pl.off_tiles);
    T *norms = reinterpret_cast<T *>(ws + pl.off_norms);
    T *rowrec = reinterpret_cast<T *>(ws + pl.off_row), *colrec = reinterpret_cast<T *>(ws + pl.off_col);
    T *partial = reinterpret_cast<T *>(ws + pl.off_part);
    hipStream_t st = (hipStream_t)stream;
    MODL_HIP(hipMemcpyAsync(ws, host.data(), host.size(), hipMemcpyHostToDevice, st));
    MODL_HIP(hipStreamSynchronize(st));                      // `host` is released on return
    hipLaunchKernelGGL(amari_norm_kernel<T>, dim3((unsigned)cdiv(pl.sum_k, 4)), dim3(256), 0, st, dd, n, pl.sum_k, p,
                       norms);
    MODL_LAUNCH_CHECK();
    hipLaunchKernelGGL(amari_pair_kernel<T>, dim3((unsigned)(pl.ntiles * pl.nsplit)), dim3(256), 0, st, dd, dp, dt,
                       (const T *)norms, p, pl.kps, (int)pl.nsplit, rowrec, colrec, partial);
    MODL_LAUNCH_CHECK();
    int nl = 3;
    if (pl.nsplit > 1) {
        hipLaunchKernelGGL(amari_combine_kernel<T>, dim3((unsigned)(pl.ntiles * (BM / kStripRows))), dim3(BM), 0, st,
                           dd, dp, dt, (const T *)norms, (int)pl.nsplit, (const T *)partial, rowrec, colrec);
        MODL_LAUNCH_CHECK();
        ++nl;
    }
    hipLaunchKernelGGL(amari_reduce_kernel<T>, dim3((unsigned)pl.npairs), dim3(256), 0, st, dd, dp, (int)pl.nstrip,
                       (const T *)rowrec, (const T *)colrec, d_pair, d_rowmax, d_colmax);
    MODL_LAUNCH_CHECK();
    if (launches) *launches = nl;
    return MODL_OK;
}

}  // namespace
}  // namespace modl

extern "C" {

size_t modl_amari_workspace(int dtype, int n, const int64_t *h_k, int64_t p) {
    modl::AmPlan pl;
    if (modl::am_plan(dtype, n, h_k, p, pl, nullptr, nullptr) != MODL_OK) return 0;
    return pl.bytes;
}

int modl_amari_f32(const float *const *h_d_dicts, const int64_t *h_k, int n, int64_t p, double *d_pair,
                   float *d_rowmax, float *d_colmax, void *d_ws, size_t ws_bytes, void *stream, int *launches) {
    return modl::amari_run<float>(h_d_dicts, h_k, n, p, d_pair, d_rowmax, d_colmax, d_ws, ws_bytes, stream, launches);
}

int modl_amari_f64(const double *const *h_d_dicts, const int64_t *h_k, int n, int64_t p, double *d_pair,
                   double *d_rowmax, double *d_colmax, void *d_ws, size_t ws_bytes, void *stream, int *launches) {
    return modl::amari_run<double>(h_d_dicts, h_k, n, p, d_pair, d_rowmax, d_colmax, d_ws, ws_bytes, stream, launches);
}

}  // extern "C"
