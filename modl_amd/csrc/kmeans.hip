// Hard parcellation: the two kernels of Lloyd's k-means on (d, V) components and of label signals.
//
// kmeans_assign_kernel.  For every listed centre set r and voxel v,
//     score[r][v] = min_c (|C_c|^2 - 2 C_c . x_v),      labels[r][v] = the lowest c attaining it,
// all in f64.  No V x K array exists: a wavefront forms the 16 voxels x 16 centres tile of X^T C^T on the matrix cores
// (v_mfma_f64_16x16x4_f64) and folds it into a running (min, argmin) in registers - register r of a lane holds voxel
// 4 r + lane / 16 against centre lane % 16, so a lane compares one centre column per tile, centres ascending, with a strict
// `<`: the first (lowest) centre of a tie stays.  The 16 lanes of a voxel are merged at the end by four exchanges that
// prefer the smaller score and, on equal scores, the smaller index.
//
// Placement.  A workgroup takes 64 voxels (blockIdx.x) of one set (blockIdx.y); each of its four wavefronts owns 16 voxels,
// whose d values live in REGISTERS as the DQ * 4 A-fragments of the product (64 VGPRs at d = 128), loaded once.  The centres
// pass through LDS in groups of 32 (rows padded to DQ * 16 with zeros, row stride + 2 doubles: the 16 rows x 2 phases of a
// half-wavefront's fragment read fall into distinct banks), shared by the four wavefronts; the next group is fetched into
// registers while the current one is consumed.  |C_c|^2 comes from kmeans_cnorm_kernel (one thread per centre, features
// ascending) through the workspace: R K doubles.  Centres past K are staged with |C|^2 = +inf and never win.
// A voxel with a non-finite value enters the product as zeros (a row of A only reaches its own row of the tile) and is
// written as label -1, score NaN.
//
// Determinism.  No sums across workgroups or wavefronts, no atomics: a voxel's result is a function of its column, the
// set's centres and d alone, whichever other sets are listed.
//
// label_sums_kernel.  sums[row][c] = sum over j in offsets[c] .. offsets[c + 1] - 1 of X[row][order[j]], in f64.  A
// workgroup takes one label (blockIdx.x) and a slab of 4 RW rows (blockIdx.y); it stages the label's segment of `order` in
// LDS, 2048 indices at a time, once for the whole slab; a wavefront owns RW rows, lane l adds the segment's elements
// l, l + 64, l + 128, ... of each of its rows in that order (RW independent gathers per index), and the 64 lane sums are
// added by the fixed tree of wave_sum.  The order of additions of a (row, label) is a function of the segment's length
// alone: its bits do not depend on the other labels, the other rows, K or RW.  Only listed voxels are read, each once per
// row; an index outside 0 .. V - 1 adds nothing.
#include <algorithm>
#include <cmath>

#include "gemm.hpp"

namespace modl {

constexpr int kKmMaxD = 128;
constexpr int kKmMaxK = 4096;
constexpr int kKmVox = 64;                                  // voxels per workgroup: 16 per wavefront
constexpr int kKmGroup = 32;                                // centres per LDS stage
constexpr int kLsChunk = 2048;                              // indices of a segment staged at a time (a multiple of 64)

static inline bool km_overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

// grid (ceil(K / 256), R): cn[listed set][c] = sum_j C[c][j]^2, j ascending
__global__ __launch_bounds__(256) void kmeans_cnorm_kernel(const double *__restrict__ C, int d, int K, const int32_t *__restrict__ active,
                                                           int n_sets, double *__restrict__ cn) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    const int set = active[blockIdx.y];
    if (c >= K || set < 0 || set >= n_sets) return;
    const double *p = C + ((int64_t)set * K + c) * d;
    double s = 0.0;
    for (int j = 0; j < d; ++j) s = fma(p[j], p[j], s);
    cn[(int64_t)blockIdx.y * K + c] = s;
}

// grid (ceil(V / 64), R), 256 threads; d <= DQ * 16
template <int DQ>
__global__ __launch_bounds__(256) void kmeans_assign_kernel(const double *__restrict__ X, int64_t ldx, int64_t V, int d,
                                                            const double *__restrict__ C, int K, const int32_t *__restrict__ active,
                                                            int n_sets, const double *__restrict__ cn, double *__restrict__ score,
                                                            int32_t *__restrict__ labels) {
    typedef Mma<double> MT;
    constexpr int DP = DQ * 16, NJ = DQ * 4, LD = DP + 2, NF = kKmGroup * DP / 256;
    __shared__ double Cs[kKmGroup][LD];
    __shared__ double cns[kKmGroup];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int i = MT::frag_i(lane), q = MT::frag_k(lane);
    const int set = active[blockIdx.y];
    if (set < 0 || set >= n_sets) return;                   // (the whole workgroup)
    const double *Cr = C + (int64_t)set * K * d;
    const double *cnr = cn + (int64_t)blockIdx.y * K;
    const int64_t v0 = (int64_t)blockIdx.x * kKmVox + w * 16;

    double xf[NJ];                                          // X[4 js + q][v0 + i]
    int bad = 0;
    {
        const int64_t v = v0 + i;
#pragma unroll
        for (int js = 0; js < NJ; ++js) {
            const int j = 4 * js + q;
            double x = (j < d && v < V) ? X[(int64_t)j * ldx + v] : 0.0;
            if (!(fabs(x) <= 1.7976931348623157e308)) {
                bad = 1;
                x = 0.0;
            }
            xf[js] = x;
        }
    }
    bad |= __shfl_xor(bad, 16);                             // the four feature phases of a voxel
    bad |= __shfl_xor(bad, 32);

    double nxt[NF], nxt_cn = 0.0;
    auto fetch = [&](int c0) {
#pragma unroll
        for (int n = 0; n < NF; ++n) {
            const int e = t + n * 256, row = e / DP, col = e % DP;
            const int c = c0 + row;
            nxt[n] = (c < K && col < d) ? Cr[(int64_t)c * d + col] : 0.0;
        }
        if (t < kKmGroup) nxt_cn = (c0 + t < K) ? cnr[c0 + t] : INFINITY;
    };

    double best[4];
    int bidx[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        best[r] = INFINITY;
        bidx[r] = 0;
    }
    fetch(0);
    for (int c0 = 0; c0 < K; c0 += kKmGroup) {
        __syncthreads();                                    // the previous group has been consumed
#pragma unroll
        for (int n = 0; n < NF; ++n) {
            const int e = t + n * 256;
            Cs[e / DP][e % DP] = nxt[n];
        }
        if (t < kKmGroup) cns[t] = nxt_cn;
        __syncthreads();
        if (c0 + kKmGroup < K) fetch(c0 + kKmGroup);
#pragma unroll
        for (int ct = 0; ct < kKmGroup / 16; ++ct) {
            MT::acc_t acc = {0.0, 0.0, 0.0, 0.0};           // register r: voxel 4 r + q against centre c0 + ct * 16 + i
#pragma unroll
            for (int js = 0; js < NJ; ++js) acc = MT::mma(xf[js], Cs[ct * 16 + i][4 * js + q], acc);
            const int c = c0 + ct * 16 + MT::acc_col(lane, 0);
            const double cnc = cns[ct * 16 + MT::acc_col(lane, 0)];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double s = fma(-2.0, acc[r], cnc);
                if (s < best[r]) {
                    best[r] = s;
                    bidx[r] = c;
                }
            }
        }
    }
    // the 16 centre columns of a voxel: smaller score, then smaller index
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int m = 1; m < 16; m <<= 1) {
            const double s2 = __shfl_xor(best[r], m);
            const int i2 = __shfl_xor(bidx[r], m);
            if (s2 < best[r] || (s2 == best[r] && i2 < bidx[r])) {
                best[r] = s2;
                bidx[r] = i2;
            }
        }
    // lane l < 16 writes voxel v0 + l = 4 r + q with r = l / 4, q = l % 4: from register r of the lanes 16 q ..
    double out_s = 0.0;
    int out_l = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const double s = __shfl(best[r], 16 * (lane & 3));
        const int l = __shfl(bidx[r], 16 * (lane & 3));
        if (((lane >> 2) & 3) == r) {
            out_s = s;
            out_l = l;
        }
    }
    const int64_t v = v0 + lane;
    if (lane < 16 && v < V) {
        score[(int64_t)set * V + v] = bad ? __longlong_as_double(0x7ff8000000000000ll) : out_s;
        labels[(int64_t)set * V + v] = bad ? -1 : out_l;
    }
}

template <int DQ>
static void kmeans_launch(dim3 grid, hipStream_t stream, const double *X, int64_t ldx, int64_t V, int d, const double *C, int K,
                          const int32_t *active, int n_sets, const double *cn, double *score, int32_t *labels) {
    hipLaunchKernelGGL((kmeans_assign_kernel<DQ>), grid, dim3(256), 0, stream, X, ldx, V, d, C, K, active, n_sets, cn, score, labels);
}

// grid (K, ceil(rows / (4 RW))), 256 threads
template <typename T, int RW>
__global__ __launch_bounds__(256) void label_sums_kernel(const T *__restrict__ X, int64_t ldx, int64_t rows, int64_t V,
                                                         const int32_t *__restrict__ order, int64_t n_order,
                                                         const int64_t *__restrict__ offsets, double *__restrict__ sums, int64_t lds) {
    __shared__ int32_t ord[kLsChunk];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int64_t c = blockIdx.x;
    int64_t lo = offsets[c], hi = offsets[c + 1];
    lo = lo < 0 ? 0 : (lo > n_order ? n_order : lo);
    hi = hi < lo ? lo : (hi > n_order ? n_order : hi);
    const int64_t row0 = (int64_t)blockIdx.y * (4 * RW) + w * RW;
    const T *xr[RW];
    bool live[RW];
    double acc[RW];
#pragma unroll
    for (int r = 0; r < RW; ++r) {
        live[r] = row0 + r < rows;
        xr[r] = X + (live[r] ? row0 + r : 0) * ldx;
        acc[r] = 0.0;
    }
    for (int64_t p = lo; p < hi; p += kLsChunk) {
        const int m = hi - p < kLsChunk ? (int)(hi - p) : kLsChunk;
        __syncthreads();                                    // the previous piece has been consumed
        for (int e = t; e < m; e += 256) {
            const int32_t v = order[p + e];
            ord[e] = (v >= 0 && (int64_t)v < V) ? v : -1;
        }
        __syncthreads();
#pragma unroll 2
        for (int e = lane; e < m; e += 64) {
            const int32_t v = ord[e];
            if (v >= 0) {
#pragma unroll
                for (int r = 0; r < RW; ++r)
                    if (live[r]) acc[r] += (double)xr[r][v];
            }
        }
    }
#pragma unroll
    for (int r = 0; r < RW; ++r) {
        const double s = wave_sum(acc[r]);
        if (lane == 0 && live[r]) sums[(row0 + r) * lds + c] = s;
    }
}

template <typename T>
static int label_sums_impl(const T *d_X, int64_t ldx, int64_t rows, int64_t V, const int32_t *d_order, int64_t n_order,
                           const int64_t *d_offsets, int K, double *d_sums, int64_t lds, void *stream_) {
    if (!d_X || !d_order || !d_offsets || !d_sums) return MODL_EINVAL;
    if (K < 1 || rows < 0 || V < 1 || V > INT32_MAX || n_order < 0 || ldx < V || lds < K) return MODL_EINVAL;
    if (rows > (int64_t)65535 * 32 || (rows > 0 && (ldx > INT64_MAX / (int64_t)sizeof(T) / rows || lds > INT64_MAX / 8 / rows)))
        return MODL_EINVAL;
    if ((uintptr_t)d_X % sizeof(T) != 0 || (uintptr_t)d_order % 4 != 0 || (uintptr_t)d_offsets % 8 != 0 || (uintptr_t)d_sums % 8 != 0)
        return MODL_EINVAL;
    if (rows > 0) {
        const size_t xb = (size_t)((rows - 1) * ldx + V) * sizeof(T), sb = (size_t)((rows - 1) * lds + K) * 8;
        if (km_overlap(d_sums, sb, d_X, xb) || km_overlap(d_sums, sb, d_offsets, (size_t)(K + 1) * 8) ||
            (n_order > 0 && km_overlap(d_sums, sb, d_order, (size_t)n_order * 4)))
            return MODL_EINVAL;
    }
    if (rows == 0 || n_order == 0) return MODL_OK;
    if (modl_device_count() <= 0) return MODL_ENOGPU;
    hipStream_t stream = (hipStream_t)stream_;
    if (rows >= 128)
        hipLaunchKernelGGL((label_sums_kernel<T, 8>), dim3((unsigned)K, (unsigned)cdiv(rows, 32)), dim3(256), 0, stream, d_X, ldx, rows, V,
                           d_order, n_order, d_offsets, d_sums, lds);
    else
        hipLaunchKernelGGL((label_sums_kernel<T, 1>), dim3((unsigned)K, (unsigned)cdiv(rows, 4)), dim3(256), 0, stream, d_X, ldx, rows, V,
                           d_order, n_order, d_offsets, d_sums, lds);
    MODL_LAUNCH_CHECK();
    return MODL_OK;
}

}  // namespace modl

using namespace modl;

extern "C" {

int modl_kmeans_max_clusters(void) { return kKmMaxK; }
int modl_kmeans_max_features(void) { return kKmMaxD; }

size_t modl_kmeans_assign_workspace(int64_t V, int d, int K, int R) {
    if (V < 1 || d < 1 || d > kKmMaxD || K < 1 || K > kKmMaxK || R < 1 || R > 65535) return 0;
    return (size_t)R * (size_t)K * sizeof(double);
}

int modl_kmeans_assign_f64(const double *d_X, int64_t ldx, int64_t V, int d, const double *d_C, int K, int n_sets, const int32_t *d_active,
                           int R, double *d_score, int32_t *d_labels, void *d_ws, size_t ws_bytes, void *stream_) {
    if (!d_X || !d_C || !d_active || !d_score || !d_labels) return MODL_EINVAL;
    if (d < 1 || d > kKmMaxD || K < 1 || K > kKmMaxK || V < 1 || R < 1 || R > 65535 || n_sets < R || ldx < V || ldx > INT64_MAX / 8 / d ||
        V > INT64_MAX / 8 / n_sets || cdiv(V, kKmVox) > INT32_MAX)
        return MODL_EINVAL;
    if ((uintptr_t)d_X % 8 != 0 || (uintptr_t)d_C % 8 != 0 || (uintptr_t)d_score % 8 != 0 || (uintptr_t)d_labels % 4 != 0 ||
        (uintptr_t)d_active % 4 != 0 || (uintptr_t)d_ws % 8 != 0)
        return MODL_EINVAL;
    const size_t need = (size_t)R * (size_t)K * sizeof(double);
    {
        const size_t xb = (size_t)((int64_t)(d - 1) * ldx + V) * 8, cb = (size_t)n_sets * K * d * 8, ab = (size_t)R * 4;
        const size_t sb = (size_t)n_sets * V * 8, lb = (size_t)n_sets * V * 4;
        const void *outs[2] = {d_score, d_labels};
        const size_t outb[2] = {sb, lb};
        for (int o = 0; o < 2; ++o)
            if (km_overlap(outs[o], outb[o], d_X, xb) || km_overlap(outs[o], outb[o], d_C, cb) || km_overlap(outs[o], outb[o], d_active, ab) ||
                (d_ws && km_overlap(outs[o], outb[o], d_ws, need)))
                return MODL_EINVAL;
        if (km_overlap(d_score, sb, d_labels, lb)) return MODL_EINVAL;
        if (d_ws && (km_overlap(d_ws, need, d_X, xb) || km_overlap(d_ws, need, d_C, cb) || km_overlap(d_ws, need, d_active, ab))) return MODL_EINVAL;
    }
    if (!d_ws || ws_bytes < need) return MODL_ENOMEM;
    if (modl_device_count() <= 0) return MODL_ENOGPU;
    hipStream_t stream = (hipStream_t)stream_;
    double *cn = (double *)d_ws;
    hipLaunchKernelGGL(kmeans_cnorm_kernel, dim3((unsigned)cdiv(K, 256), (unsigned)R), dim3(256), 0, stream, d_C, d, K, d_active, n_sets, cn);
    MODL_LAUNCH_CHECK();
    const dim3 grid((unsigned)cdiv(V, kKmVox), (unsigned)R);
    switch ((d + 15) / 16) {
    case 1: kmeans_launch<1>(grid, stream, d_X, ldx, V, d, d_C, K, d_active, n_sets, cn, d_score, d_labels); break;
    case 2: kmeans_launch<2>(grid, stream, d_X, ldx, V, d, d_C, K, d_active, n_sets, cn, d_score, d_labels); break;
    case 3: kmeans_launch<3>(grid, stream, d_X, ldx, V, d, d_C, K, d_active, n_sets, cn, d_score, d_labels); break;
    case 4: kmeans_launch<4>(grid, stream, d_X, ldx, V, d, d_C, K, d_active, n_sets, cn, d_score, d_labels); break;
    case 5: kmeans_launch<5>(grid, stream, d_X, ldx, V, d, d_C, K, d_active, n_sets, cn, d_score, d_labels); break;
    case 6: kmeans_launch<6>(grid, stream, d_X, ldx, V, d, d_C, K, d_active, n_sets, cn, d_score, d_labels); break;
    case 7: kmeans_launch<7>(grid, stream, d_X, ldx, V, d, d_C, K, d_active, n_sets, cn, d_score, d_labels); break;
    default: kmeans_launch<8>(grid, stream, d_X, ldx, V, d, d_C, K, d_active, n_sets, cn, d_score, d_labels); break;
    }
    MODL_LAUNCH_CHECK();
    return MODL_OK;
}

int modl_label_sums_f32(const float *d_X, int64_t ldx, int64_t rows, int64_t V, const int32_t *d_order, int64_t n_order,
                        const int64_t *d_offsets, int K, double *d_sums, int64_t lds, void *stream) {
    return label_sums_impl<float>(d_X, ldx, rows, V, d_order, n_order, d_offsets, K, d_sums, lds, stream);
}

int modl_label_sums_f64(const double *d_X, int64_t ldx, int64_t rows, int64_t V, const int32_t *d_order, int64_t n_order,
                        const int64_t *d_offsets, int K, double *d_sums, int64_t lds, void *stream) {
    return label_sums_impl<double>(d_X, ldx, rows, V, d_order, n_order, d_offsets, K, d_sums, lds, stream);
}

}  // extern "C"
