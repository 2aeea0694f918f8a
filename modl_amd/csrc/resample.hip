// Resampling of an fMRI volume onto another grid (the first step of the reference's masker: nilearn's
// resample_img, i.e. scipy.ndimage.affine_transform per frame with mode 'constant').  Frames are [T][n0][n1][n2], n2
// fastest - the layout of masker.hip; a target locus o reads the source at x = A o + b (A, b in this axis order).
//
//   prefilter   d_vol[T][n0][n1][n2] -> coefficients[T][n0][n1][n2]: non-finite -> 0, then per axis the cubic B-spline
//               filter of scipy.ndimage.spline_filter1d(order 3, mode 'mirror'): gain 6, a causal and an anticausal
//               recursion with the pole z = sqrt(3) - 2, the causal start value being the mirror sum
//               (c_0 + z^(n-1) c_(n-1) + sum_i z^i (c_i + z^(n-1) c_(n-1-i))) / (1 - z^(2n-2)) cut after kPrefTerms = 64
//               terms (|z|^64 = 2.6e-37), the anticausal one (z c+_(n-2) + c+_(n-1)) z / (z^2 - 1).  An axis of length 1 is
//               left alone.  The state of both recursions and the causal values c+ are f64; an element is rounded to the
//               volume's dtype once per axis, when the anticausal walk stores it.
//   resample    out = sum over (order + 1)^3 taps of weight * (source at order 0 / 1, coefficients at order 3)
//
// The prefilter runs along n2 first (the pass that reads d_vol), then in place along n1 and n0.  Along n1 and n0 one
// thread owns one line and neighbouring threads own neighbouring n2, so every access of a wavefront is coalesced: the
// thread walks forward, writing c+ as f64 into a scratch volume, then backward, writing the coefficients.  Along n2 a
// line is contiguous and that mapping would be uncoalesced: a workgroup stages a slab of R lines as f64 in LDS with
// coalesced loads (rows padded to an odd number of doubles: the walks of a half wavefront fall on 32 distinct bank
// pairs), one thread walks one row in place, and the slab is stored coalesced.  R = 256, 128 or 64 rows within 80 KiB
// (two workgroups per CU), which bounds the line at modl_resample_lds_line() = 159 elements; longer lines take the
// direct walk of the other axes with stride 1.
//
// The gather: one thread owns one output locus.  Its three coordinates x_a = b_a + sum_j A_aj o_j (f64, the products
// and sums in scipy's order and unfused, so a coordinate has scipy's bits), the inside test 0 <= x_a <= n_a - 1, the
// mirrored tap offsets (d c b | a b c d | c b a) and the weights per axis are formed once and reused for the frames
// f = y, y + gridDim.y, ... of the thread; gridDim.y = ceil(T / 4), so a small mask still fills the device.  Sums are
// separable - along n2, then n1, then n0 - and ACCUMULATE IN F64 for both dtypes; the result is rounded once.  Order 0
// copies the element at floor(x + 0.5): bit for bit.  Box mode writes every locus of the target box as frames, rows mode
// only the loci of d_vox, as out[dst(t)][c].  In box mode neighbouring threads take neighbouring n2, so their taps share
// cache lines.  The columns of a mask are numbered with axis 0 fastest, the axis along which the source is slowest: in rows
// mode thread i takes column d_order[i], and with d_order the columns sorted by (o0, o1, o2) the threads of a wavefront
// are neighbours along n2 again (the reads are 64 per locus, the scattered store is one).  No atomics, no waits between
// workgroups.
#include <cmath>

#include "common.hpp"

namespace modl {

constexpr int kPrefTerms = 64;                               // terms of the causal start value
constexpr int kPrefThreads = 256;
constexpr size_t kPrefLds = 80 * 1024;                       // the slab of the n2 pass: two workgroups per CU
constexpr int kPrefLdsLine = 159;                            // 64 rows of 159 doubles
constexpr int kResampleThreads = 256;
constexpr int kResampleFrames = 4;                           // frames of one thread (when T allows)
constexpr int64_t kResampleMaxEdge = ((int64_t)1 << 30) - 1;   // (2 n - 2 of the mirror stays an int)

struct PrefPole {
    double z;                                                // sqrt(3) - 2
    double zn1;                                              // z^(n-1), 0 once the sum is cut before it matters
    double den;                                              // 1 - z^(2n-2)
    double za;                                               // z / (z^2 - 1)
    int k;                                                   // min(n - 2, kPrefTerms)
};

struct ResampleGeom {
    double A[9], b[3];
    int n[3], m[3];
};

static PrefPole pref_pole(int n) {
    PrefPole p;
    p.z = std::sqrt(3.0) - 2.0;
    p.zn1 = n - 1 <= kPrefTerms ? std::pow(p.z, (double)(n - 1)) : 0.0;
    p.den = 1.0 - p.zn1 * p.zn1;
    p.za = p.z / (p.z * p.z - 1.0);
    p.k = std::max(0, std::min(n - 2, kPrefTerms));
    return p;
}

template <typename T> __device__ __forceinline__ T finite_or_0(T v) { return std::fabs(v) < (T)__builtin_inf() ? v : (T)0; }

// one line of n >= 2 doubles in LDS, in place
__device__ __forceinline__ void prefilter_row(double *c, int n, const PrefPole &p) {
    double zi = p.z;
    double s = 6.0 * c[0] + p.zn1 * (6.0 * c[n - 1]);
    for (int i = 1; i <= p.k; ++i) {
        s += zi * (6.0 * c[i] + p.zn1 * (6.0 * c[n - 1 - i]));
        zi *= p.z;
    }
    s /= p.den;
    c[0] = s;
    for (int i = 1; i < n; ++i) {
        s = 6.0 * c[i] + p.z * s;
        c[i] = s;
    }
    s = (p.z * c[n - 2] + s) * p.za;
    c[n - 1] = s;
    for (int i = n - 2; i >= 0; --i) {
        s = p.z * (s - c[i]);
        c[i] = s;
    }
}

// the n2 pass out of LDS: workgroup x takes the rows [x R, x R + R) of the n0 n1 lines of a frame, frames y, y + gridDim.y, ...
template <typename T>
__global__ __launch_bounds__(kPrefThreads) void prefilter_lds_kernel(const T *__restrict__ src, int64_t sfs, T *__restrict__ dst,
                                                                     int64_t dfs, int64_t n_frames, int64_t lines, int n, int R,
                                                                     int pitch, PrefPole p) {
    extern __shared__ __attribute__((aligned(16))) char pref_smem[];
    double *slab = (double *)pref_smem;
    const int tid = threadIdx.x;
    const int64_t l0 = (int64_t)blockIdx.x * R;
    const int rows = lines - l0 < R ? (int)(lines - l0) : R;
    const int cnt = rows * n;                                // <= 256 * 159
    for (int64_t f = blockIdx.y; f < n_frames; f += gridDim.y) {
        const T *s = src + f * sfs + l0 * n;
        for (int e = tid; e < cnt; e += kPrefThreads) {
            const int r = e / n;
            slab[r * pitch + (e - r * n)] = (double)finite_or_0(s[e]);
        }
        __syncthreads();
        if (tid < rows && n >= 2) prefilter_row(slab + tid * pitch, n, p);
        __syncthreads();
        T *d = dst + f * dfs + l0 * n;
        for (int e = tid; e < cnt; e += kPrefThreads) {
            const int r = e / n;
            d[e] = (T)slab[r * pitch + (e - r * n)];
        }
        __syncthreads();                                     // (the next frame overwrites the slab)
    }
}

// One thread, one line of n elements `sa` apart; line j of a frame starts at (j / sa) sa n + j % sa.  src and dst may be
// the same array (a thread reads all of its line before it writes any of it); `scr` holds c+ at the element's own index.
template <typename T, bool FIRST>
__global__ __launch_bounds__(kPrefThreads) void prefilter_walk_kernel(const T *src, int64_t sfs, T *dst, int64_t dfs,
                                                                      double *__restrict__ scr, int64_t box, int64_t n_frames,
                                                                      int64_t lines, int64_t sa, int n, PrefPole p) {
    const int64_t j = (int64_t)blockIdx.x * kPrefThreads + threadIdx.x;
    if (j >= lines) return;
    const int64_t base = (j / sa) * (sa * n) + j % sa;
    for (int64_t f = blockIdx.y; f < n_frames; f += gridDim.y) {
        const T *s = src + f * sfs + base;
        T *d = dst + f * dfs + base;
        double *q = scr + f * box + base;
        auto ld = [&](int i) -> double { return (double)(FIRST ? finite_or_0(s[i * sa]) : s[i * sa]); };
        if (n < 2) {
            if (FIRST) d[0] = finite_or_0(s[0]);
            continue;
        }
        double zi = p.z;
        double acc = 6.0 * ld(0);
        if (p.zn1 != 0.0) acc += p.zn1 * (6.0 * ld(n - 1));
        for (int i = 1; i <= p.k; ++i) {
            double v = 6.0 * ld(i);
            if (p.zn1 != 0.0) v += p.zn1 * (6.0 * ld(n - 1 - i));
            acc += zi * v;
            zi *= p.z;
        }
        acc /= p.den;
        q[0] = acc;
#pragma unroll 4
        for (int i = 1; i < n; ++i) {
            acc = 6.0 * ld(i) + p.z * acc;
            q[i * sa] = acc;
        }
        acc = (p.z * q[(n - 2) * sa] + acc) * p.za;
        d[(n - 1) * sa] = (T)acc;
#pragma unroll 4
        for (int i = n - 2; i >= 0; --i) {
            acc = p.z * (acc - q[i * sa]);
            d[i * sa] = (T)acc;
        }
    }
}

__device__ __forceinline__ int mirror_tap(int i, int n) {      // d c b | a b c d | c b a, period 2 n - 2
    if (n == 1) return 0;
    while (i < 0 || i > n - 1) i = i < 0 ? -i : 2 * (n - 1) - i;
    return i;
}

template <typename T, int ORDER>
__global__ __launch_bounds__(kResampleThreads) void resample_kernel(const T *__restrict__ src, int64_t sfs, int64_t n_frames,
                                                                    ResampleGeom g, double fill,
                                                                    const int64_t *__restrict__ vox, int64_t n_loci,
                                                                    const int64_t *__restrict__ order,
                                                                    const int64_t *__restrict__ dst_row, T *__restrict__ out,
                                                                    int64_t ldo) {
    constexpr int K = ORDER + 1;
    int64_t c = (int64_t)blockIdx.x * kResampleThreads + threadIdx.x;
    if (c >= n_loci) return;
    if (vox && order) {                                      // rows mode: the column this thread takes
        c = order[c];
        if ((uint64_t)c >= (uint64_t)n_loci) return;
    }
    const int64_t mbox = (int64_t)g.m[0] * g.m[1] * g.m[2];
    int o[3];
    if (vox) {                                               // axis 0 fastest: the C index of the caller's (m2, m1, m0) box
        const int64_t v = vox[c];
        if ((uint64_t)v >= (uint64_t)mbox) return;
        const int64_t q = v / g.m[0];
        o[0] = (int)(v - q * g.m[0]);
        o[2] = (int)(q / g.m[1]);
        o[1] = (int)(q - (int64_t)o[2] * g.m[1]);
    } else {
        const int64_t q = c / g.m[2];
        o[2] = (int)(c - q * g.m[2]);
        o[0] = (int)(q / g.m[1]);
        o[1] = (int)(q - (int64_t)o[0] * g.m[1]);
    }
    bool inside = true;
    int off[3][K];
    double w[3][K];
    const int stride[3] = {g.n[1] * g.n[2], g.n[2], 1};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        // scipy: tmp = shift; tmp += coordinate[l] * matrix[l] for its axes l = 0, 1, 2, which are the axes 2, 1, 0 here
        double x = g.b[a];
        x = __dadd_rn(x, __dmul_rn((double)o[2], g.A[3 * a + 2]));
        x = __dadd_rn(x, __dmul_rn((double)o[1], g.A[3 * a + 1]));
        x = __dadd_rn(x, __dmul_rn((double)o[0], g.A[3 * a + 0]));
        const int n = g.n[a];
        if (!(x >= 0.0 && x <= (double)(n - 1))) {           // (also a NaN)
            inside = false;
#pragma unroll
            for (int k = 0; k < K; ++k) off[a][k] = 0, w[a][k] = 0.0;
            continue;
        }
        if constexpr (ORDER == 0) {
            const int i = (int)std::floor(x + 0.5);
            off[a][0] = (i < n ? i : n - 1) * stride[a];
            w[a][0] = 1.0;
        } else {
            const double fl = std::floor(x);
            const int i0 = (int)fl;
            const double y = x - fl;
            if constexpr (ORDER == 1) {
                w[a][0] = 1.0 - y;
                w[a][1] = y;
            } else {                                         // the cubic B-spline, in scipy's arrangement
                const double z = 1.0 - y;
                w[a][1] = (y * y * (y - 2.0) * 3.0 + 4.0) / 6.0;
                w[a][2] = (z * z * (z - 2.0) * 3.0 + 4.0) / 6.0;
                w[a][0] = z * z * z / 6.0;
                w[a][3] = 1.0 - w[a][0] - w[a][1] - w[a][2];
            }
#pragma unroll
            for (int k = 0; k < K; ++k) off[a][k] = mirror_tap(i0 - ORDER / 2 + k, n) * stride[a];
        }
    }
    const int64_t col = c;                                   // box mode: the locus' flat index; rows mode: its column
    for (int64_t f = blockIdx.y; f < n_frames; f += gridDim.y) {
        const int64_t row = dst_row ? dst_row[f] : f;
        if ((uint64_t)row >= (uint64_t)n_frames) continue;
        T *dst = out + row * ldo + col;
        if (!inside) {
            *dst = (T)fill;
            continue;
        }
        const T *s = src + f * sfs;
        if (ORDER == 0) {
            *dst = finite_or_0(s[off[0][0] + off[1][0] + off[2][0]]);
            continue;
        }
        double a0 = 0.0;
#pragma unroll
        for (int k0 = 0; k0 < K; ++k0) {
            double a1 = 0.0;
#pragma unroll
            for (int k1 = 0; k1 < K; ++k1) {
                const T *line = s + (off[0][k0] + off[1][k1]);
                T v[K];
#pragma unroll
                for (int k2 = 0; k2 < K; ++k2) v[k2] = line[off[2][k2]];
                double a2 = 0.0;
#pragma unroll
                for (int k2 = 0; k2 < K; ++k2)
                    a2 = __builtin_fma(w[2][k2], (double)(ORDER == 1 ? finite_or_0(v[k2]) : v[k2]), a2);
                a1 = __builtin_fma(w[1][k1], a2, a1);
            }
            a0 = __builtin_fma(w[0][k0], a1, a0);
        }
        *dst = (T)a0;
    }
}

static inline bool resample_box_ok(int64_t n0, int64_t n1, int64_t n2) {
    return n0 >= 1 && n1 >= 1 && n2 >= 1 && n0 <= kResampleMaxEdge && n1 <= kResampleMaxEdge && n2 <= kResampleMaxEdge &&
           n0 <= INT32_MAX / n1 && n0 * n1 <= INT32_MAX / n2;
}

static inline bool resample_overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

static inline size_t resample_coef_bytes(size_t es, int64_t T, int64_t box) { return align_up((size_t)(T * box) * es, 256); }

// the three passes; `coef` has the frame stride `cfs`, `scr` is T box doubles.  Everything has been checked.
template <typename T>
static int prefilter_run(const T *vol, int64_t fs, int64_t n_frames, int64_t n0, int64_t n1, int64_t n2, T *coef, int64_t cfs,
                         double *scr, hipStream_t stream) {
    const int64_t box = n0 * n1 * n2;
    const unsigned gy = (unsigned)std::min<int64_t>(n_frames, 65535);
    if (n2 <= kPrefLdsLine) {
        const int pitch = (int)n2 | 1;
        const int R = 256 * pitch * 8 <= (int)kPrefLds ? 256 : 128 * pitch * 8 <= (int)kPrefLds ? 128 : 64;
        const size_t lds = (size_t)R * pitch * sizeof(double);
        if (lds > 64 * 1024)
            MODL_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&prefilter_lds_kernel<T>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPrefLds));
        hipLaunchKernelGGL(prefilter_lds_kernel<T>, dim3((unsigned)cdiv(n0 * n1, R), gy), dim3(kPrefThreads), lds, stream, vol, fs,
                           coef, cfs, n_frames, n0 * n1, (int)n2, R, pitch, pref_pole((int)n2));
    } else {
        hipLaunchKernelGGL((prefilter_walk_kernel<T, true>), dim3((unsigned)cdiv(n0 * n1, kPrefThreads), gy), dim3(kPrefThreads), 0,
                           stream, vol, fs, coef, cfs, scr, box, n_frames, n0 * n1, (int64_t)1, (int)n2, pref_pole((int)n2));
    }
    MODL_LAUNCH_CHECK();
    if (n1 > 1) {
        hipLaunchKernelGGL((prefilter_walk_kernel<T, false>), dim3((unsigned)cdiv(n0 * n2, kPrefThreads), gy), dim3(kPrefThreads), 0,
                           stream, (const T *)coef, cfs, coef, cfs, scr, box, n_frames, n0 * n2, n2, (int)n1, pref_pole((int)n1));
        MODL_LAUNCH_CHECK();
    }
    if (n0 > 1) {
        hipLaunchKernelGGL((prefilter_walk_kernel<T, false>), dim3((unsigned)cdiv(n1 * n2, kPrefThreads), gy), dim3(kPrefThreads), 0,
                           stream, (const T *)coef, cfs, coef, cfs, scr, box, n_frames, n1 * n2, n1 * n2, (int)n0,
                           pref_pole((int)n0));
        MODL_LAUNCH_CHECK();
    }
    return MODL_OK;
}

template <typename T>
static int prefilter_abi(const T *vol, int64_t fs, int64_t n_frames, int64_t n0, int64_t n1, int64_t n2, T *coef, int64_t cfs,
                         void *ws, size_t ws_bytes, void *stream) {
    if (!vol || !coef || n_frames < 1 || !resample_box_ok(n0, n1, n2)) return MODL_EINVAL;
    const int64_t box = n0 * n1 * n2;
    if (fs < box || cfs < box || fs > INT64_MAX / 8 / n_frames || cfs > INT64_MAX / 8 / n_frames) return MODL_EINVAL;
    const size_t vol_bytes = (size_t)((n_frames - 1) * fs + box) * sizeof(T), coef_bytes = (size_t)((n_frames - 1) * cfs + box) * sizeof(T);
    const size_t need = modl_resample_workspace(DType<T>::id, n_frames, n0, n1, n2, 3);
    if (need == 0 || resample_overlap(vol, vol_bytes, coef, coef_bytes)) return MODL_EINVAL;
    if (ws && (resample_overlap(vol, vol_bytes, ws, ws_bytes) || resample_overlap(coef, coef_bytes, ws, ws_bytes))) return MODL_EINVAL;
    if (!ws || ws_bytes < need) return MODL_ENOMEM;
    if (modl_device_count() <= 0) return MODL_ENOGPU;
    double *scr = (double *)((char *)ws + resample_coef_bytes(sizeof(T), n_frames, box));
    return prefilter_run<T>(vol, fs, n_frames, n0, n1, n2, coef, cfs, scr, (hipStream_t)stream);
}

template <typename T>
static int resample_abi(const T *vol, int64_t fs, int64_t n_frames, int64_t n0, int64_t n1, int64_t n2, const double *A,
                        const double *b, int order, double fill, int64_t m0, int64_t m1, int64_t m2, const int64_t *vox, int64_t V,
                        const int64_t *walk, const int64_t *dst_row, T *out, int64_t ldo, void *ws, size_t ws_bytes,
                        void *stream_) {
    if (!vol || !A || !b || !out || n_frames < 1 || !resample_box_ok(n0, n1, n2) || !resample_box_ok(m0, m1, m2)) return MODL_EINVAL;
    if (order != 0 && order != 1 && order != 3) return MODL_EINVAL;
    const int64_t box = n0 * n1 * n2, mbox = m0 * m1 * m2;
    const int64_t width = vox ? V : mbox;                   // elements of an output row / frame
    if (width < 1 || width > mbox || ldo < width || fs < box || fs > INT64_MAX / 8 / n_frames || ldo > INT64_MAX / 8 / n_frames)
        return MODL_EINVAL;
    if (!std::isfinite(fill)) return MODL_EINVAL;
    ResampleGeom g;
    bool shift = true;                                       // A the identity, b integer: the shifted crop, at order 0
    for (int i = 0; i < 9; ++i) {
        if (!std::isfinite(A[i])) return MODL_EINVAL;
        g.A[i] = A[i];
        shift = shift && A[i] == (i % 4 == 0 ? 1.0 : 0.0);
    }
    for (int i = 0; i < 3; ++i) {
        if (!std::isfinite(b[i])) return MODL_EINVAL;
        g.b[i] = b[i];
        shift = shift && b[i] == std::floor(b[i]);
    }
    const size_t vol_bytes = (size_t)((n_frames - 1) * fs + box) * sizeof(T), out_bytes = (size_t)((n_frames - 1) * ldo + width) * sizeof(T);
    if (resample_overlap(vol, vol_bytes, out, out_bytes)) return MODL_EINVAL;
    size_t need = 0;
    if (order == 3) {
        need = modl_resample_workspace(DType<T>::id, n_frames, n0, n1, n2, 3);
        if (need == 0) return MODL_EINVAL;
        if (ws && (resample_overlap(vol, vol_bytes, ws, ws_bytes) || resample_overlap(out, out_bytes, ws, ws_bytes))) return MODL_EINVAL;
        if (!ws || ws_bytes < need) return MODL_ENOMEM;
    }
    if (modl_device_count() <= 0) return MODL_ENOGPU;
    hipStream_t stream = (hipStream_t)stream_;
    g.n[0] = (int)n0, g.n[1] = (int)n1, g.n[2] = (int)n2;
    g.m[0] = (int)m0, g.m[1] = (int)m1, g.m[2] = (int)m2;
    if (shift) order = 0;
    const T *src = vol;
    int64_t sfs = fs;
    if (order == 3) {
        T *coef = (T *)ws;
        MODL_TRY(prefilter_run<T>(vol, fs, n_frames, n0, n1, n2, coef, box, (double *)((char *)ws + resample_coef_bytes(sizeof(T), n_frames, box)),
                                  stream));
        src = coef;
        sfs = box;
    }
    const dim3 grid((unsigned)cdiv(width, kResampleThreads), (unsigned)std::min<int64_t>(cdiv(n_frames, kResampleFrames), 65535));
#define MODL_RESAMPLE_LAUNCH(ORDER)                                                                                              \
    hipLaunchKernelGGL((resample_kernel<T, ORDER>), grid, dim3(kResampleThreads), 0, stream, src, sfs, n_frames, g, fill, vox, width, \
                       walk, dst_row, out, ldo)
    if (order == 0) MODL_RESAMPLE_LAUNCH(0);
    else if (order == 1) MODL_RESAMPLE_LAUNCH(1);
    else MODL_RESAMPLE_LAUNCH(3);
#undef MODL_RESAMPLE_LAUNCH
    MODL_LAUNCH_CHECK();
    return MODL_OK;
}

}  // namespace modl

using namespace modl;

extern "C" {

int modl_resample_lds_line(void) { return kPrefLdsLine; }

int modl_resample_frames(void) { return kResampleFrames; }

size_t modl_resample_workspace(int dtype, int64_t T, int64_t n0, int64_t n1, int64_t n2, int order) {
    if ((dtype != MODL_F32 && dtype != MODL_F64) || T < 1 || !resample_box_ok(n0, n1, n2) || order != 3) return 0;
    const int64_t box = n0 * n1 * n2;
    if (T > INT64_MAX / 32 / box) return 0;
    return resample_coef_bytes(dtype == MODL_F32 ? 4 : 8, T, box) + align_up((size_t)(T * box) * sizeof(double), 256);
}

int modl_spline_prefilter_f32(const float *d_vol, int64_t frame_stride, int64_t T, int64_t n0, int64_t n1, int64_t n2,
                              float *d_coef, int64_t coef_stride, void *d_ws, size_t ws_bytes, void *stream) {
    return prefilter_abi<float>(d_vol, frame_stride, T, n0, n1, n2, d_coef, coef_stride, d_ws, ws_bytes, stream);
}

int modl_spline_prefilter_f64(const double *d_vol, int64_t frame_stride, int64_t T, int64_t n0, int64_t n1, int64_t n2,
                              double *d_coef, int64_t coef_stride, void *d_ws, size_t ws_bytes, void *stream) {
    return prefilter_abi<double>(d_vol, frame_stride, T, n0, n1, n2, d_coef, coef_stride, d_ws, ws_bytes, stream);
}

int modl_resample_f32(const float *d_vol, int64_t frame_stride, int64_t T, int64_t n0, int64_t n1, int64_t n2, const double *A,
                      const double *b, int order, double fill, int64_t m0, int64_t m1, int64_t m2, const int64_t *d_vox, int64_t V,
                      const int64_t *d_order, const int64_t *d_dst_row, float *d_out, int64_t ldo, void *d_ws, size_t ws_bytes,
                      void *stream) {
    return resample_abi<float>(d_vol, frame_stride, T, n0, n1, n2, A, b, order, fill, m0, m1, m2, d_vox, V, d_order, d_dst_row, d_out,
                               ldo, d_ws, ws_bytes, stream);
}

int modl_resample_f64(const double *d_vol, int64_t frame_stride, int64_t T, int64_t n0, int64_t n1, int64_t n2, const double *A,
                      const double *b, int order, double fill, int64_t m0, int64_t m1, int64_t m2, const int64_t *d_vox, int64_t V,
                      const int64_t *d_order, const int64_t *d_dst_row, double *d_out, int64_t ldo, void *d_ws, size_t ws_bytes,
                      void *stream) {
    return resample_abi<double>(d_vol, frame_stride, T, n0, n1, n2, A, b, order, fill, m0, m1, m2, d_vox, V, d_order, d_dst_row, d_out,
                                ldo, d_ws, ws_bytes, stream);
}

}  // extern "C"
