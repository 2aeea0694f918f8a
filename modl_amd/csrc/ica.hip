// One sweep of symmetric FastICA for many restarts at once: for every listed restart r, with
// y = W_r x per voxel of the whitened maps X1 (k rows of V),
//     M_r = (1 / V) sum_v g(y_v) x_v^T   (k x k),      gp_r[i] = (1 / V) sum_v g'(y_{i, v}),
// all in f64.  The k x V sources are never written: a wavefront forms a 16 x 16 tile of Y^T = X1^T W_r^T on the matrix
// cores (v_mfma_f64_16x16x4_f64), and the accumulator layout of that instruction - register r of a lane holds voxel
// 4 r + lane / 16 of component lane % 16 - is exactly the A-fragment layout of the second product, whose contraction
// index is the voxel: g(Y) goes from the accumulators of the first product into the operands of the second without
// leaving the registers and without a lane exchange.
//
// Placement.  A workgroup takes one restart (blockIdx.x) and one chunk of voxels (blockIdx.y); it has KT = ceil(k / 16)
// wavefronts, and wavefront `it` owns the 16 components it * 16 .. it * 16 + 15: its 16 rows of W_r live in REGISTERS as
// the KT * 4 B-fragments of the first product (64 VGPRs at k = 128), its 16 rows of M as KT accumulator tiles (another
// 64), loaded / zeroed once per workgroup.  W never touches LDS; LDS only holds the stage of X1 (k rows padded to KT * 16
// with zeros, kStage = 32 voxels, row stride 34 doubles so that the 16 rows x 4 voxels of a second-product fragment fall
// into distinct banks), which every wavefront reads for both products.  The next stage is fetched into registers while the
// current one is consumed.  Voxels past V are staged as zeros: g(0) = 0 for the three non-linearities, so they add
// nothing to M; g' is masked.
//
// Determinism.  A workgroup writes its partial M and gp to the workspace ([restart][chunk][k k + k]); ica_reduce_kernel
// sums the chunks in ascending order and scales by 1 / V.  No floating-point atomics; the chunking depends on V alone,
// so a restart's bits are the same whichever other restarts are listed with it.
#include <algorithm>
#include <cmath>

#include "gemm.hpp"

namespace modl {

constexpr int kIcaMaxK = 128;
constexpr int kIcaStage = 32;                               // voxels per LDS stage
constexpr int kIcaLd = kIcaStage + 2;                       // row stride of the stage in doubles
constexpr int kIcaFetch = 16 * kIcaStage / kWave;           // doubles a thread stages: KT * 16 rows over KT wavefronts
enum { kIcaCube = 0, kIcaLogcosh = 1, kIcaExp = 2 };

// Voxel chunks per restart: a function of V ALONE (at most kIcaChunks chunks of a multiple of kIcaStage voxels), so that the
// order in which a restart's partial sums are added - its bits - does not depend on how many other restarts are listed.
constexpr int64_t kIcaChunks = 96;
static inline int64_t ica_chunk_voxels(int64_t V) { return cdiv(cdiv(V, kIcaChunks), kIcaStage) * kIcaStage; }
static inline int64_t ica_chunks(int64_t V) { return cdiv(V, ica_chunk_voxels(V)); }
static inline size_t ica_ws_bytes(int64_t V, int k, int R) {
    return (size_t)R * (size_t)ica_chunks(V) * ((size_t)k * k + k) * sizeof(double);
}

template <int FUN> __device__ __forceinline__ void ica_nonlinearity(double y, double alpha, double &g, double &gp) {
    if (FUN == kIcaCube) {
        const double y2 = y * y;
        g = y2 * y;
        gp = 3.0 * y2;
    } else if (FUN == kIcaLogcosh) {
        g = tanh(alpha * y);
        gp = alpha * (1.0 - g * g);
    } else {
        const double y2 = y * y, e = exp(-y2 / 2.0);
        g = y * e;
        gp = (1.0 - y2) * e;
    }
}

// grid (R, chunks), KT * 64 threads
template <int KT, int FUN>
__global__ __launch_bounds__(KT * kWave) void ica_sweep_kernel(const double *__restrict__ X, int64_t ldx, int64_t V, int k,
                                                               const double *__restrict__ W, const int32_t *__restrict__ active,
                                                               double alpha, int64_t chunk_voxels, double *__restrict__ part) {
    typedef Mma<double> MT;
    constexpr int KP = KT * 16, NT = KT * kWave;
    __shared__ double Xs[KP][kIcaLd];
    const int t = threadIdx.x, lane = t & 63, it = t >> 6;
    const int c = MT::frag_i(lane), q = MT::frag_k(lane);
    const double *Wr = W + (int64_t)active[blockIdx.x] * k * k;
    const int64_t v_lo = (int64_t)blockIdx.y * chunk_voxels, v_hi = v_lo + chunk_voxels < V ? v_lo + chunk_voxels : V;

    double wf[KT * 4];                                      // W_r[it * 16 + c][4 js + q]
    {
        const int i = it * 16 + c;
#pragma unroll
        for (int js = 0; js < KT * 4; ++js) {
            const int j = 4 * js + q;
            wf[js] = (i < k && j < k) ? Wr[(int64_t)i * k + j] : 0.0;
        }
    }
    MT::acc_t macc[KT];
#pragma unroll
    for (int jt = 0; jt < KT; ++jt)
#pragma unroll
        for (int r = 0; r < 4; ++r) macc[jt][r] = 0.0;
    double gp_acc = 0.0;

    double nxt[kIcaFetch];
    auto fetch = [&](int64_t v0) {
#pragma unroll
        for (int n = 0; n < kIcaFetch; ++n) {
            const int e = t + n * NT, row = e / kIcaStage, col = e % kIcaStage;
            const int64_t v = v0 + col;
            nxt[n] = (row < k && v < v_hi) ? X[(int64_t)row * ldx + v] : 0.0;
        }
    };
    fetch(v_lo);
    for (int64_t v0 = v_lo; v0 < v_hi; v0 += kIcaStage) {
        __syncthreads();                                    // the previous stage has been consumed
#pragma unroll
        for (int n = 0; n < kIcaFetch; ++n) {
            const int e = t + n * NT;
            Xs[e / kIcaStage][e % kIcaStage] = nxt[n];
        }
        __syncthreads();
        if (v0 + kIcaStage < v_hi) fetch(v0 + kIcaStage);
#pragma unroll 1                                            // (unrolled, the two tiles' fragment loads are hoisted and k = 128 spills)
        for (int vt = 0; vt < kIcaStage / 16; ++vt) {
            MT::acc_t y = {0.0, 0.0, 0.0, 0.0};             // Y^T: register r = voxel vt * 16 + 4 r + q, component it * 16 + c
#pragma unroll
            for (int js = 0; js < KT * 4; ++js) y = MT::mma(Xs[4 * js + q][vt * 16 + c], wf[js], y);
            double gy[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                double gp;
                ica_nonlinearity<FUN>(y[r], alpha, gy[r], gp);
                if (v0 + vt * 16 + 4 * r + q < v_hi) gp_acc += gp;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int jt = 0; jt < KT; ++jt) macc[jt] = MT::mma(gy[r], Xs[jt * 16 + c][vt * 16 + 4 * r + q], macc[jt]);
        }
    }

    double *P = part + ((int64_t)blockIdx.x * gridDim.y + blockIdx.y) * ((int64_t)k * k + k);
#pragma unroll
    for (int jt = 0; jt < KT; ++jt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = it * 16 + MT::acc_row(lane, r), j = jt * 16 + MT::acc_col(lane, r);
            if (i < k && j < k) P[(int64_t)i * k + j] = macc[jt][r];
        }
    gp_acc += __shfl_xor(gp_acc, 16);                       // the four voxel phases of a component, in a fixed order
    gp_acc += __shfl_xor(gp_acc, 32);
    if (q == 0 && it * 16 + c < k) P[(int64_t)k * k + it * 16 + c] = gp_acc;
}

// grid (ceil((k k + k) / 256), R): the chunks in ascending order, times 1 / V
__global__ __launch_bounds__(256) void ica_reduce_kernel(const double *__restrict__ part, int64_t chunks, int k, int64_t V,
                                                         const int32_t *__restrict__ active, double *__restrict__ M,
                                                         double *__restrict__ gp) {
    const int64_t per = (int64_t)k * k + k, e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= per) return;
    const double *p = part + (int64_t)blockIdx.y * chunks * per + e;
    double s = 0.0;
    for (int64_t ch = 0; ch < chunks; ++ch) s += p[ch * per];
    s /= (double)V;
    const int64_t r = active[blockIdx.y];
    if (e < (int64_t)k * k) M[r * k * k + e] = s;
    else gp[r * k + (e - (int64_t)k * k)] = s;
}

template <int KT, int FUN>
static void ica_launch(dim3 grid, hipStream_t stream, const double *X, int64_t ldx, int64_t V, int k, const double *W,
                       const int32_t *active, double alpha, int64_t chunk_voxels, double *part) {
    hipLaunchKernelGGL((ica_sweep_kernel<KT, FUN>), grid, dim3(KT * kWave), 0, stream, X, ldx, V, k, W, active, alpha, chunk_voxels,
                       part);
}

template <int FUN>
static void ica_launch_kt(int KT, dim3 grid, hipStream_t stream, const double *X, int64_t ldx, int64_t V, int k, const double *W,
                          const int32_t *active, double alpha, int64_t chunk_voxels, double *part) {
    switch (KT) {
    case 1: return ica_launch<1, FUN>(grid, stream, X, ldx, V, k, W, active, alpha, chunk_voxels, part);
    case 2: return ica_launch<2, FUN>(grid, stream, X, ldx, V, k, W, active, alpha, chunk_voxels, part);
    case 3: return ica_launch<3, FUN>(grid, stream, X, ldx, V, k, W, active, alpha, chunk_voxels, part);
    case 4: return ica_launch<4, FUN>(grid, stream, X, ldx, V, k, W, active, alpha, chunk_voxels, part);
    case 5: return ica_launch<5, FUN>(grid, stream, X, ldx, V, k, W, active, alpha, chunk_voxels, part);
    case 6: return ica_launch<6, FUN>(grid, stream, X, ldx, V, k, W, active, alpha, chunk_voxels, part);
    case 7: return ica_launch<7, FUN>(grid, stream, X, ldx, V, k, W, active, alpha, chunk_voxels, part);
    default: return ica_launch<8, FUN>(grid, stream, X, ldx, V, k, W, active, alpha, chunk_voxels, part);
    }
}

}  // namespace modl

using namespace modl;

extern "C" {

int modl_ica_max_components(void) { return kIcaMaxK; }

size_t modl_ica_sweep_workspace(int64_t V, int k, int R) {
    if (V < 1 || k < 1 || k > kIcaMaxK || R < 1 || R > 65535) return 0;
    return ica_ws_bytes(V, k, R);
}

int modl_ica_sweep_f64(const double *d_X1, int64_t ldx, int64_t V, int k, const double *d_W, const int32_t *d_active, int R, int fun,
                       double alpha, double *d_M, double *d_gp, void *d_ws, size_t ws_bytes, void *stream_) {
    if (!d_X1 || !d_W || !d_active || !d_M || !d_gp) return MODL_EINVAL;
    if (k < 1 || k > kIcaMaxK || V < 1 || R < 1 || R > 65535 || ldx < V || ldx > INT64_MAX / 8 / k) return MODL_EINVAL;
    if (fun != kIcaCube && fun != kIcaLogcosh && fun != kIcaExp) return MODL_EINVAL;
    if ((uintptr_t)d_X1 % 8 != 0 || (uintptr_t)d_W % 8 != 0 || (uintptr_t)d_M % 8 != 0 || (uintptr_t)d_gp % 8 != 0 ||
        (uintptr_t)d_active % 4 != 0 || (uintptr_t)d_ws % 8 != 0)
        return MODL_EINVAL;
    const size_t need = ica_ws_bytes(V, k, R);
    if (!d_ws || ws_bytes < need) return MODL_ENOMEM;
    if (modl_device_count() <= 0) return MODL_ENOGPU;
    hipStream_t stream = (hipStream_t)stream_;
    const int64_t chunk_voxels = ica_chunk_voxels(V), chunks = ica_chunks(V);
    const int KT = (k + 15) / 16;
    const dim3 grid((unsigned)R, (unsigned)chunks);
    double *part = (double *)d_ws;
    if (fun == kIcaCube) ica_launch_kt<kIcaCube>(KT, grid, stream, d_X1, ldx, V, k, d_W, d_active, alpha, chunk_voxels, part);
    else if (fun == kIcaLogcosh) ica_launch_kt<kIcaLogcosh>(KT, grid, stream, d_X1, ldx, V, k, d_W, d_active, alpha, chunk_voxels, part);
    else ica_launch_kt<kIcaExp>(KT, grid, stream, d_X1, ldx, V, k, d_W, d_active, alpha, chunk_voxels, part);
    MODL_LAUNCH_CHECK();
    const int64_t per = (int64_t)k * k + k;
    hipLaunchKernelGGL(ica_reduce_kernel, dim3((unsigned)cdiv(per, 256), (unsigned)R), dim3(256), 0, stream, part, chunks, k, V, d_active,
                       d_M, d_gp);
    MODL_LAUNCH_CHECK();
    return MODL_OK;
}

}  // extern "C"
