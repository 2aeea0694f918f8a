// Signal cleaning of an fMRI record (the arithmetic of nilearn.signal.clean that the reference's masker
// runs on every record before partial_fit, modl/decomposition/fmri.py:525-526): for every column x of X (T x V),
//
//   r = x - Q (Q^T x)                      Q: T x q, orthonormal columns, built on the host in f64 (modl_amd/signal.py)
//   out = standardize ? r sqrt(T) / |r| : r        a FLAT column (|r|^2 <= (q T eps64)^2 |x|^2) standardizes to exact zeros
//
// A workgroup of kCleanWaves wavefronts takes 64 * C adjacent columns, a thread the C columns lane, lane + 64, ...: a
// wavefront reads row t of 64 columns as one contiguous segment (coalesced), wavefront w takes the rows t = w,
// w + kCleanWaves, ...  Row t of Q is the same for the whole wavefront, so it travels through the scalar cache into scalar
// registers, and with C columns per thread one such row serves C * 64 elements.  The coefficients Q^T x, |x|^2 and |r|^2
// are summed in f64 for both dtypes: per wavefront in ascending t, then over the wavefronts in ascending w through LDS.
// That order depends on T alone - not on V, on the column's place in the call, on C, on the leading dimensions or on
// d_dst_row - so a column comes out with the same bits wherever it stands.  A column that holds a NaN or Inf (|x|^2 not
// finite) comes out as NaN throughout and touches no other column.
//
//   sweep 1   c = Q^T x, |x|^2                                         reads X
//   sweep 2   r = x - Q c (f64), |r|^2; without standardize: stores r   reads X (writes out)
//   sweep 3   (standardize) r again, scaled, rounded once, stored       reads X, writes out
//
// The q <= 64 coefficients of a column stay in registers: the kernel is instantiated for the widths of clean_width(),
// the basis is copied into the workspace with its rows padded by zero columns to that width (a zero column changes no
// bit: its coefficient is +0 and r - 0 * 0 = r).  No atomics, no scratch.
#include <algorithm>

#include "common.hpp"

namespace modl {

constexpr int kCleanMaxQ = 64;
constexpr int kCleanWaves = 4;                   // wavefronts of a workgroup: the split of T
constexpr int64_t kCleanMaxGrid = (int64_t)1 << 20;   // workgroups of a launch; the kernel strides over what is beyond

// the instantiated widths: multiples of 4 up to 32, then 48 and 64
static inline int clean_width(int q) { return q <= 32 ? (q + 3) / 4 * 4 : q <= 48 ? 48 : 64; }
// columns per thread: two while the kernel is bound by memory (measured), one once the f64 fma count binds
constexpr int clean_cols(int nq) { return nq <= 8 ? 2 : 1; }

// Qp[t][0 .. nq) = Q[t][0 .. q), 0 beyond
__global__ __launch_bounds__(256) void clean_pad_kernel(const double *Q, int64_t T, int q, int nq, double *Qp) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= T * nq) return;
    const int64_t t = i / nq;
    const int j = (int)(i - t * nq);
    Qp[i] = j < q ? Q[t * q + j] : 0.0;
}

// the sum over the wavefronts of a workgroup, in ascending wavefront order; every wavefront gets it.  part: [waves][64]
__device__ __forceinline__ double clean_combine(double v, double (*part)[64], int wid, int lane) {
    __syncthreads();                             // (part may still be read by the previous call)
    part[wid][lane] = v;
    __syncthreads();
    double s = part[0][lane];
#pragma unroll
    for (int w = 1; w < kCleanWaves; ++w) s += part[w][lane];
    return s;
}

template <typename T, int C> struct CleanCols {
    const T *x;                                  // this thread's first column, row 0; column k is rel[k] elements further
    T *o;
    int rel[C];                                  // 64 k; 0 for a column beyond V, which repeats a live one and is never stored
    bool live[C];
};

// R rows from t (stride kCleanWaves) of the C columns: MODE 1 coefficients and |x|^2 (acc), MODE 2 |r|^2 (acc) and, with
// STORE, the residual; MODE 3 the scaled residual.  The R * C loads are issued before anything is computed.
template <typename T, int NQ, int C, int R, int MODE, bool STORE>
__device__ __forceinline__ void clean_rows(const CleanCols<T, C> &cols, int64_t ldx, int64_t ldo, int64_t n_t, int64_t t,
                                           const double *__restrict__ Qp, const int64_t *__restrict__ dst_row,
                                           double (&c)[C][NQ], double (&acc)[C], const double (&scale)[C],
                                           const bool (&flat)[C]) {
    double x[R][C];
#pragma unroll
    for (int u = 0; u < R; ++u)
#pragma unroll
        for (int k = 0; k < C; ++k) x[u][k] = (double)cols.x[(t + u * kCleanWaves) * ldx + cols.rel[k]];
#pragma unroll
    for (int u = 0; u < R; ++u) {
        const int64_t tu = t + u * kCleanWaves;
        const double *qr = Qp + tu * NQ;
        if (MODE == 1) {
#pragma unroll
            for (int k = 0; k < C; ++k) acc[k] = __builtin_fma(x[u][k], x[u][k], acc[k]);
#pragma unroll
            for (int j = 0; j < NQ; ++j) {
                const double qv = qr[j];
#pragma unroll
                for (int k = 0; k < C; ++k) c[k][j] = __builtin_fma(qv, x[u][k], c[k][j]);
            }
        } else {
            double r[C];
#pragma unroll
            for (int k = 0; k < C; ++k) r[k] = x[u][k];
#pragma unroll
            for (int j = 0; j < NQ; ++j) {
                const double qv = -qr[j];
#pragma unroll
                for (int k = 0; k < C; ++k) r[k] = __builtin_fma(qv, c[k][j], r[k]);
            }
            if (MODE == 2) {
#pragma unroll
                for (int k = 0; k < C; ++k) acc[k] = __builtin_fma(r[k], r[k], acc[k]);
            }
            if (MODE == 3 || STORE) {
                const int64_t d = dst_row ? dst_row[tu] : tu;
                if ((uint64_t)d < (uint64_t)n_t) {
#pragma unroll
                    for (int k = 0; k < C; ++k)
                        if (cols.live[k])
                            cols.o[d * ldo + cols.rel[k]] = MODE == 3 ? (flat[k] ? (T)0 : (T)(r[k] * scale[k])) : (T)r[k];
                }
            }
        }
    }
}

template <typename T, int NQ, int C, int MODE, bool STORE>
__device__ __forceinline__ void clean_sweep(const CleanCols<T, C> &cols, int64_t ldx, int64_t ldo, int64_t n_t, int wid,
                                            const double *__restrict__ Qp, const int64_t *__restrict__ dst_row,
                                            double (&c)[C][NQ], double (&acc)[C], const double (&scale)[C],
                                            const bool (&flat)[C]) {
    constexpr int R = C >= 4 ? 1 : 4 / C;        // rows in flight: four loads per thread
    int64_t t = wid;
    for (; t + (R - 1) * kCleanWaves < n_t; t += R * kCleanWaves)
        clean_rows<T, NQ, C, R, MODE, STORE>(cols, ldx, ldo, n_t, t, Qp, dst_row, c, acc, scale, flat);
    if (R > 1)
        for (; t < n_t; t += kCleanWaves)
            clean_rows<T, NQ, C, 1, MODE, STORE>(cols, ldx, ldo, n_t, t, Qp, dst_row, c, acc, scale, flat);
}

template <typename T, int NQ, int C>
__global__ __launch_bounds__(64 * kCleanWaves) void clean_kernel(const T *X, int64_t ldx, int64_t n_t, int64_t V,
                                                                  const double *__restrict__ Qp, int q, int standardize,
                                                                  const int64_t *__restrict__ dst_row, T *out,
                                                                  int64_t ldo) {
    constexpr int G = NQ < 16 ? NQ : 16;         // coefficients that cross the LDS per round
    __shared__ double part[G][kCleanWaves][64];
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t blocks = (V + 64 * C - 1) / (64 * C);
    for (int64_t cb = blockIdx.x; cb < blocks; cb += gridDim.x) {
        CleanCols<T, C> cols;
        const int64_t col0 = cb * C * 64 + lane;
        cols.x = X + (col0 < V ? col0 : 0);
        cols.o = out + (col0 < V ? col0 : 0);
#pragma unroll
        for (int k = 0; k < C; ++k) {
            cols.live[k] = col0 + 64 * k < V;
            cols.rel[k] = cols.live[k] ? 64 * k : 0;
        }
        double c[C][NQ], xx[C], rr[C], scale[C];
        bool flat[C];
#pragma unroll
        for (int k = 0; k < C; ++k) {
            xx[k] = rr[k] = scale[k] = 0.0;
            flat[k] = false;
#pragma unroll
            for (int j = 0; j < NQ; ++j) c[k][j] = 0.0;
        }
        // ---- sweep 1: c = Q^T x, xx = |x|^2
        clean_sweep<T, NQ, C, 1, false>(cols, ldx, ldo, n_t, wid, Qp, dst_row, c, xx, scale, flat);
#pragma unroll
        for (int k = 0; k < C; ++k) {
#pragma unroll
            for (int g0 = 0; g0 < NQ; g0 += G) {
                __syncthreads();                 // (part may still be read by the previous round)
#pragma unroll
                for (int j = 0; j < G && g0 + j < NQ; ++j) part[j][wid][lane] = c[k][g0 + j];
                __syncthreads();
#pragma unroll
                for (int j = 0; j < G && g0 + j < NQ; ++j) {
                    double s = part[j][0][lane];
#pragma unroll
                    for (int w = 1; w < kCleanWaves; ++w) s += part[j][w][lane];
                    c[k][g0 + j] = s;
                }
            }
            xx[k] = clean_combine(xx[k], part[0], wid, lane);
            if (!(xx[k] < __builtin_inf())) c[k][0] = __builtin_nan("");     // a NaN or Inf in the column: NaN throughout
        }
        // ---- sweep 2: rr = |r|^2; the residual itself is the result when nothing is standardized
        if (!standardize) {                      // (uniform: a kernel argument)
            clean_sweep<T, NQ, C, 2, true>(cols, ldx, ldo, n_t, wid, Qp, dst_row, c, rr, scale, flat);
            continue;
        }
        clean_sweep<T, NQ, C, 2, false>(cols, ldx, ldo, n_t, wid, Qp, dst_row, c, rr, scale, flat);
        // ---- sweep 3: the residual again, scaled to population variance 1; a flat column to exact zeros
        const double thr = (double)q * (double)n_t * 2.220446049250313e-16;
#pragma unroll
        for (int k = 0; k < C; ++k) {
            rr[k] = clean_combine(rr[k], part[0], wid, lane);
            flat[k] = rr[k] <= thr * thr * xx[k];            // (false for a NaN: a poisoned column stays NaN)
            scale[k] = __builtin_sqrt((double)n_t) / __builtin_sqrt(rr[k]);
        }
        clean_sweep<T, NQ, C, 3, true>(cols, ldx, ldo, n_t, wid, Qp, dst_row, c, rr, scale, flat);
    }
}

template <typename T, int NQ>
static int clean_launch(const T *X, int64_t ldx, int64_t n_t, int64_t V, const double *Qp, int q, int standardize,
                        const int64_t *dst_row, T *out, int64_t ldo, hipStream_t stream) {
    constexpr int C = clean_cols(NQ);
    const unsigned grid = (unsigned)std::min(cdiv(V, 64 * C), kCleanMaxGrid);
    hipLaunchKernelGGL((clean_kernel<T, NQ, C>), dim3(grid), dim3(64 * kCleanWaves), 0, stream, X, ldx, n_t, V, Qp, q,
                       standardize, dst_row, out, ldo);
    MODL_LAUNCH_CHECK();
    return MODL_OK;
}

template <typename T>
static int clean_abi(const T *X, int64_t ldx, int64_t n_t, int64_t V, const double *Q, int q, int standardize,
                     const int64_t *dst_row, T *out, int64_t ldo, void *ws, size_t ws_bytes, void *stream_) {
    if (!X || !Q || !out || n_t < 1 || V < 1 || q < 1 || q > kCleanMaxQ || (int64_t)q > n_t || ldx < V || ldo < V ||
        ldx > INT64_MAX / 8 / n_t || ldo > INT64_MAX / 8 / n_t)
        return MODL_EINVAL;
    // d_out may share bytes with d_X only as the very same array, and then without a row permutation
    const uintptr_t x0 = (uintptr_t)X, o0 = (uintptr_t)out;
    const uintptr_t x1 = x0 + (uintptr_t)((n_t - 1) * ldx + V) * sizeof(T), o1 = o0 + (uintptr_t)((n_t - 1) * ldo + V) * sizeof(T);
    if (x0 < o1 && o0 < x1 && (x0 != o0 || dst_row || ldo != ldx)) return MODL_EINVAL;
    const size_t need = modl_clean_workspace(DType<T>::id, n_t, V, q);
    if (need == 0) return MODL_EINVAL;
    if (!ws || ws_bytes < need) return MODL_ENOMEM;
    if (modl_device_count() <= 0) return MODL_ENOGPU;
    hipStream_t stream = (hipStream_t)stream_;
    const int nq = clean_width(q);
    double *Qp = (double *)ws;
    hipLaunchKernelGGL(clean_pad_kernel, dim3((unsigned)cdiv(n_t * nq, 256)), dim3(256), 0, stream, Q, n_t, q, nq, Qp);
    MODL_LAUNCH_CHECK();
    const int s = standardize ? 1 : 0;
#define MODL_CLEAN_CASE(NQ) \
    case NQ: return clean_launch<T, NQ>(X, ldx, n_t, V, Qp, q, s, dst_row, out, ldo, stream)
    switch (nq) {
        MODL_CLEAN_CASE(4);
        MODL_CLEAN_CASE(8);
        MODL_CLEAN_CASE(12);
        MODL_CLEAN_CASE(16);
        MODL_CLEAN_CASE(20);
        MODL_CLEAN_CASE(24);
        MODL_CLEAN_CASE(28);
        MODL_CLEAN_CASE(32);
        MODL_CLEAN_CASE(48);
        MODL_CLEAN_CASE(64);
    }
#undef MODL_CLEAN_CASE
    return MODL_EINVAL;
}

}  // namespace modl

using namespace modl;

extern "C" {

int modl_clean_max_regressors(void) { return kCleanMaxQ; }

size_t modl_clean_workspace(int dtype, int64_t T, int64_t V, int q) {
    if ((dtype != MODL_F32 && dtype != MODL_F64) || T < 1 || V < 1 || q < 1 || q > kCleanMaxQ || (int64_t)q > T ||
        T > ((int64_t)1 << 31) * 256 / kCleanMaxQ)                 // (the grid of the padding launch)
        return 0;
    return (size_t)T * (size_t)clean_width(q) * sizeof(double);
}

int modl_clean_f32(const float *d_X, int64_t ldx, int64_t T, int64_t V, const double *d_Q, int q, int standardize,
                   const int64_t *d_dst_row, float *d_out, int64_t ldo, void *d_ws, size_t ws_bytes, void *stream) {
    return clean_abi<float>(d_X, ldx, T, V, d_Q, q, standardize, d_dst_row, d_out, ldo, d_ws, ws_bytes, stream);
}

int modl_clean_f64(const double *d_X, int64_t ldx, int64_t T, int64_t V, const double *d_Q, int q, int standardize,
                   const int64_t *d_dst_row, double *d_out, int64_t ldo, void *d_ws, size_t ws_bytes, void *stream) {
    return clean_abi<double>(d_X, ldx, T, V, d_Q, q, standardize, d_dst_row, d_out, ldo, d_ws, ws_bytes, stream);
}

}  // extern "C"
