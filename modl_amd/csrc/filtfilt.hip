// Zero-phase Butterworth filtering of an fMRI record (the `low_pass` / `high_pass` of nilearn.signal.clean
// that the reference's masker takes, modl/decomposition/fmri.py:281-299): for every column x of X (T x V),
//
//   out = filtfilt(b, a, detrend ? x - line(x) : x)           scipy.signal.filtfilt with its defaults
//
// that is: padlen = 3 n_taps, the column extended at both ends by odd reflection (left 2 x[0] - x[padlen .. 1], right
// 2 x[T-1] - x[T-2 .. T-padlen-1]), a forward pass in direct form II transposed started from zi ext[0], the same over the
// reversed forward output started from zi times its first element, the pads trimmed.
//
// The recurrence is sequential in t and independent per column: ONE THREAD OWNS ONE COLUMN from start to finish, a
// wavefront reads row t of 64 adjacent columns as one contiguous segment.  b, -a and zi are kernel arguments, uniform
// across the launch, so they are scalar operands of the f64 fmas; the n_taps - 1 state values are f64 registers for both
// dtypes.  The kernel is instantiated for the widths of filtfilt_width() and the coefficients are padded with trailing
// zeros to that width (a zero tap changes no bit of a finite column); padlen always comes from the true n_taps.
//
//   sweep 0   (detrend) sum x, sum (t - (T-1)/2) x in f64, ascending t                           reads X
//   forward   left pad (outputs dropped), the T samples, right pad; the T + padlen outputs from   reads X, writes ws
//             sample 0 on go to the workspace as f64, [T + padlen][V]
//   backward  from the far end of the right pad down to sample 0, rounded once on store            reads ws, writes out
//
// A thread loads kFiltRows rows ahead of the row it computes (two register buffers), so the sequential loop is fed
// although V columns give few wavefronts.  The arithmetic order of a column depends on T and the taps alone - not on V, on
// the column's place in the call, on the leading dimensions or on d_dst_row.  A column that holds a NaN or Inf comes out
// as NaN throughout (a flag per thread, set in the forward pass) and touches no other column; an all-zero column comes
// out as exact zeros.  No atomics, no scratch, no LDS.
#include <algorithm>
#include <cmath>

#include "common.hpp"

#ifndef MODL_FILTFILT_ROWS
#define MODL_FILTFILT_ROWS 8                     // rows a thread has in flight (measured)
#endif
#ifndef MODL_FILTFILT_BLOCK
#define MODL_FILTFILT_BLOCK 64                   // threads of a workgroup (measured)
#endif

namespace modl {

constexpr int kFiltMaxTaps = 12;                 // a band of order 5 has 11
constexpr int kFiltRows = MODL_FILTFILT_ROWS;
constexpr int kFiltBlock = MODL_FILTFILT_BLOCK;
constexpr int64_t kFiltMaxGrid = (int64_t)1 << 20;   // workgroups of a launch; the kernel strides over what is beyond

// the instantiated widths (taps)
static inline int filtfilt_width(int n_taps) { return n_taps <= 2 ? 2 : n_taps <= 8 ? (n_taps + 1) / 2 * 2 : 12; }

template <int NT> struct FiltCoef {
    double b[NT];                                // numerator
    double na[NT];                               // MINUS the denominator (na[0] is not used)
    double zi[NT - 1];                           // steady state of a unit step
};

// one step of direct form II transposed
template <int NT> __device__ __forceinline__ double filt_step(const FiltCoef<NT> &c, double (&z)[NT - 1], double x) {
    const double y = __builtin_fma(c.b[0], x, z[0]);
#pragma unroll
    for (int i = 0; i + 2 < NT; ++i) z[i] = __builtin_fma(c.na[i + 1], y, __builtin_fma(c.b[i + 1], x, z[i + 1]));
    z[NT - 2] = __builtin_fma(c.na[NT - 1], y, c.b[NT - 1] * x);
    return y;
}

// the row of X that element e of the extended column (0 .. T + 2 pad) is made of
__device__ __forceinline__ int64_t filt_ext_row(int64_t e, int64_t n_t, int64_t pad) {
    if (e < pad) return pad - e;
    e -= pad;
    return e < n_t ? e : 2 * n_t - 2 - e;
}

template <typename T, int NT>
__global__ __launch_bounds__(kFiltBlock) void filtfilt_kernel(const T *X, int64_t ldx, int64_t n_t, int64_t V, int pad_,
                                                              const FiltCoef<NT> c, int detrend,
                                                              const int64_t *__restrict__ dst_row, T *out, int64_t ldo,
                                                              double *ws) {
    constexpr int R = kFiltRows;
    const int64_t pad = pad_;
    const int64_t n_e = n_t + 2 * pad;           // the extended column
    const int64_t n_w = n_t + pad;               // rows of the workspace: forward outputs from sample 0 on
    const double mid = 0.5 * (double)(n_t - 1);
    for (int64_t col = (int64_t)blockIdx.x * kFiltBlock + threadIdx.x; col < V; col += (int64_t)gridDim.x * kFiltBlock) {
        const T *x = X + col;
        double *w = ws + col;
        double cur[R], nxt[R];
        // ---- sweep 0: the least-squares line  mean + slope (t - mid)
        double mean = 0.0, slope = 0.0;
        if (detrend) {                           // (uniform: a kernel argument)
            double s0 = 0.0, s1 = 0.0;
#pragma unroll
            for (int u = 0; u < R; ++u) cur[u] = (double)x[std::min<int64_t>(u, n_t - 1) * ldx];
            for (int64_t t0 = 0; t0 < n_t; t0 += R) {
#pragma unroll
                for (int u = 0; u < R; ++u) nxt[u] = (double)x[std::min<int64_t>(t0 + R + u, n_t - 1) * ldx];
#pragma unroll
                for (int u = 0; u < R; ++u)
                    if (t0 + u < n_t) {
                        s0 += cur[u];
                        s1 = __builtin_fma((double)(t0 + u) - mid, cur[u], s1);
                    }
#pragma unroll
                for (int u = 0; u < R; ++u) cur[u] = nxt[u];
            }
            const double n = (double)n_t;
            mean = s0 / n;
            slope = s1 / (n * (n * n - 1.0) / 12.0);
        }
        // with mean = slope = 0 the subtraction below changes no bit
        const double first = (double)x[0] - __builtin_fma(slope, -mid, mean);
        const double last = (double)x[(n_t - 1) * ldx] - __builtin_fma(slope, mid, mean);
        // ---- forward
        double z[NT - 1];
        {
            const double e0 = 2.0 * first - ((double)x[pad * ldx] - __builtin_fma(slope, (double)pad - mid, mean));
#pragma unroll
            for (int i = 0; i < NT - 1; ++i) z[i] = c.zi[i] * e0;
        }
        bool bad = false;
#pragma unroll
        for (int u = 0; u < R; ++u) cur[u] = (double)x[filt_ext_row(std::min<int64_t>(u, n_e - 1), n_t, pad) * ldx];
        for (int64_t e0 = 0; e0 < n_e; e0 += R) {
#pragma unroll
            for (int u = 0; u < R; ++u)
                nxt[u] = (double)x[filt_ext_row(std::min<int64_t>(e0 + R + u, n_e - 1), n_t, pad) * ldx];
#pragma unroll
            for (int u = 0; u < R; ++u) {
                const int64_t e = e0 + u;
                if (e < n_e) {                   // (uniform)
                    const int64_t row = filt_ext_row(e, n_t, pad);
                    const double xd = cur[u] - __builtin_fma(slope, (double)row - mid, mean);
                    const bool inside = e >= pad && e < pad + n_t;
                    if (inside) bad = bad || !(__builtin_fabs(cur[u]) < __builtin_inf());
                    // odd reflection: 2 edge - x, one rounding as in 2 x[0] - x[k]
                    const double v = inside ? xd : __builtin_fma(-1.0, xd, 2.0 * (e < pad ? first : last));
                    const double y = filt_step<NT>(c, z, v);
                    if (e >= pad) w[(e - pad) * V] = y;
                }
            }
#pragma unroll
            for (int u = 0; u < R; ++u) cur[u] = nxt[u];
        }
        // ---- backward: over the forward output from its far end, started from zi times that end
#pragma unroll
        for (int u = 0; u < R; ++u) cur[u] = w[std::max<int64_t>(n_w - 1 - u, 0) * V];
#pragma unroll
        for (int i = 0; i < NT - 1; ++i) z[i] = c.zi[i] * cur[0];
        T *o = out + col;
        for (int64_t r0 = n_w - 1; r0 >= 0; r0 -= R) {
#pragma unroll
            for (int u = 0; u < R; ++u) nxt[u] = w[std::max<int64_t>(r0 - R - u, 0) * V];
#pragma unroll
            for (int u = 0; u < R; ++u) {
                const int64_t r = r0 - u;
                if (r >= 0) {                    // (uniform)
                    const double y = filt_step<NT>(c, z, cur[u]);
                    if (r < n_t) {
                        const int64_t d = dst_row ? dst_row[r] : r;
                        if ((uint64_t)d < (uint64_t)n_t) o[d * ldo] = bad ? (T)__builtin_nan("") : (T)y;
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < R; ++u) cur[u] = nxt[u];
        }
    }
}

template <typename T, int NT>
static int filtfilt_launch(const T *X, int64_t ldx, int64_t n_t, int64_t V, const double *b, const double *a,
                           const double *zi, int n_taps, int detrend, const int64_t *dst_row, T *out, int64_t ldo,
                           double *ws, hipStream_t stream) {
    FiltCoef<NT> c;
    for (int i = 0; i < NT; ++i) {
        c.b[i] = i < n_taps ? b[i] : 0.0;
        c.na[i] = i < n_taps ? -a[i] : 0.0;
        if (i < NT - 1) c.zi[i] = i < n_taps - 1 ? zi[i] : 0.0;
    }
    const unsigned grid = (unsigned)std::min(cdiv(V, kFiltBlock), kFiltMaxGrid);
    hipLaunchKernelGGL((filtfilt_kernel<T, NT>), dim3(grid), dim3(kFiltBlock), 0, stream, X, ldx, n_t, V, 3 * n_taps, c,
                       detrend, dst_row, out, ldo, ws);
    MODL_LAUNCH_CHECK();
    return MODL_OK;
}

template <typename T>
static int filtfilt_abi(const T *X, int64_t ldx, int64_t n_t, int64_t V, const double *b, const double *a,
                        const double *zi, int n_taps, int detrend, const int64_t *dst_row, T *out, int64_t ldo, void *ws,
                        size_t ws_bytes, void *stream_) {
    if (!X || !out || !b || !a || !zi || n_taps < 2 || n_taps > kFiltMaxTaps || V < 1 || n_t <= 3 * (int64_t)n_taps ||
        ldx < V || ldo < V || ldx > INT64_MAX / 8 / n_t || ldo > INT64_MAX / 8 / n_t)
        return MODL_EINVAL;
    if (a[0] != 1.0) return MODL_EINVAL;
    for (int i = 0; i < n_taps; ++i)
        if (!std::isfinite(b[i]) || !std::isfinite(a[i]) || (i < n_taps - 1 && !std::isfinite(zi[i]))) return MODL_EINVAL;
    // d_out may share bytes with d_X only as the very same array, and then without a row permutation
    const uintptr_t x0 = (uintptr_t)X, o0 = (uintptr_t)out;
    const uintptr_t x1 = x0 + (uintptr_t)((n_t - 1) * ldx + V) * sizeof(T), o1 = o0 + (uintptr_t)((n_t - 1) * ldo + V) * sizeof(T);
    if (x0 < o1 && o0 < x1 && (x0 != o0 || dst_row || ldo != ldx)) return MODL_EINVAL;
    const size_t need = modl_filtfilt_workspace(DType<T>::id, n_t, V, n_taps);
    if (need == 0) return MODL_EINVAL;
    if (!ws || ws_bytes < need) return MODL_ENOMEM;
    if (modl_device_count() <= 0) return MODL_ENOGPU;
    hipStream_t stream = (hipStream_t)stream_;
    const int d = detrend ? 1 : 0;
#define MODL_FILTFILT_CASE(NT) \
    case NT: return filtfilt_launch<T, NT>(X, ldx, n_t, V, b, a, zi, n_taps, d, dst_row, out, ldo, (double *)ws, stream)
    switch (filtfilt_width(n_taps)) {
        MODL_FILTFILT_CASE(2);
        MODL_FILTFILT_CASE(4);
        MODL_FILTFILT_CASE(6);
        MODL_FILTFILT_CASE(8);
        MODL_FILTFILT_CASE(12);
    }
#undef MODL_FILTFILT_CASE
    return MODL_EINVAL;
}

}  // namespace modl

using namespace modl;

extern "C" {

int modl_filtfilt_max_taps(void) { return kFiltMaxTaps; }

size_t modl_filtfilt_workspace(int dtype, int64_t T, int64_t V, int n_taps) {
    if ((dtype != MODL_F32 && dtype != MODL_F64) || n_taps < 2 || n_taps > kFiltMaxTaps || V < 1 ||
        T <= 3 * (int64_t)n_taps || T > INT64_MAX / 16 / V)
        return 0;
    return (size_t)(T + 3 * (int64_t)n_taps) * (size_t)V * sizeof(double);
}

int modl_filtfilt_f32(const float *d_X, int64_t ldx, int64_t T, int64_t V, const double *b, const double *a,
                      const double *zi, int n_taps, int detrend, const int64_t *d_dst_row, float *d_out, int64_t ldo,
                      void *d_ws, size_t ws_bytes, void *stream) {
    return filtfilt_abi<float>(d_X, ldx, T, V, b, a, zi, n_taps, detrend, d_dst_row, d_out, ldo, d_ws, ws_bytes, stream);
}

int modl_filtfilt_f64(const double *d_X, int64_t ldx, int64_t T, int64_t V, const double *b, const double *a,
                      const double *zi, int n_taps, int detrend, const int64_t *d_dst_row, double *d_out, int64_t ldo,
                      void *d_ws, size_t ws_bytes, void *stream) {
    return filtfilt_abi<double>(d_X, ldx, T, V, b, a, zi, n_taps, detrend, d_dst_row, d_out, ldo, d_ws, ws_bytes, stream);
}

}  // extern "C"
