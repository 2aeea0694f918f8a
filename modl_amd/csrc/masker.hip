// Spatial smoothing and masking of an fMRI volume (the masker's arithmetic that precedes signal.clean in
// the reference: nilearn's _smooth_array - scipy.ndimage.gaussian_filter1d per spatial axis, boundary 'reflect' - then the
// boolean mask), and the inverse scatter of masked rows back into a volume.
//
//   smooth_mask   d_vol[T][n0][n1][n2] -> d_out[T][ldo]:  non-finite -> 0, three 1-D correlations, out[t][col[v]] = s[t][v]
//   unmask        d_rows[n][ldr] -> d_out[n][n0 n1 n2]:   zeros, then out[i][vox[c]] = rows[i][c]
//
// The smoothing kernel never writes an intermediate volume.  A workgroup of 512 threads takes a tile t0 x t1 x t2 of one
// frame: it reads the tile's slice of d_col and leaves when no voxel of it is in the mask (before any volume data is
// read), loads the tile plus its halo of r_a voxels per side (indices reflected with period 2 n_a, non-finite values
// zeroed) into LDS, correlates along axis 0 and axis 1 from one LDS buffer into the other and along axis 2 straight into
// d_out, for the masked voxels of the tile only.  The fastest axis of every LDS array is axis 2 and consecutive threads
// take consecutive elements of it in all three passes, so a wavefront always touches 64 consecutive words: no bank
// conflict in any direction (taps along axis 0 / 1 move the whole wavefront by one plane / one line).  Every sum runs in
// f64 in ascending tap order over the same 2 r + 1 addends wherever the voxel lies, and is rounded once to the record's
// dtype when it is stored, so the bits of a voxel depend on the volume and the weights alone.  The tile shrinks with the
// radius and the element size (smooth_tile) so that two workgroups share the 160 KiB of a CU.  No atomics, no scratch.
#include <cmath>

#include "common.hpp"

namespace modl {

constexpr int kSmoothMaxR = 8;
constexpr int kSmoothSlot = 2 * kSmoothMaxR + 1;           // weights of an axis in the workspace
constexpr int kSmoothThreads = 512;                          // eight wavefronts: two workgroups fill half the slots of a CU
constexpr int kSmoothMaxTile = 32;                          // the largest tile edge of smooth_tile
constexpr size_t kSmoothLds = 79 * 1024;                    // dynamic LDS of a workgroup: two of them (and their tables) on a CU
constexpr int64_t kSmoothGrid = 1 << 14;                    // workgroups of a launch aimed at (tiles x frame slots)
constexpr int64_t kSmoothMaxEdge = ((int64_t)1 << 30) - 1;  // (2 n - 1 of the reflection stays an int)

struct SmoothWeights { double w[3][kSmoothSlot]; };
struct SmoothGeom {
    int n[3];                                               // the box
    int r[3];                                               // radius per axis, 0: untouched
    int t[3];                                               // the tile (clipped to the box)
    int nt[3];                                              // tiles per axis
};

static const int kSmoothTiles[][3] = {{8, 16, 32}, {8, 8, 32}, {8, 8, 16}, {4, 8, 16}, {4, 4, 16}, {4, 4, 8}, {2, 4, 8},
                                      {2, 2, 8},   {1, 2, 8},  {1, 1, 8},  {1, 1, 4},  {1, 1, 1}};

// LDS elements of a tile: the halo buffer, and the buffer that the first LDS pass writes
static inline void smooth_lds(const int *t, const int *r, size_t *buf0, size_t *buf1) {
    const size_t d0 = t[0] + 2 * r[0], d1 = t[1] + 2 * r[1], d2 = t[2] + 2 * r[2];
    *buf0 = d0 * d1 * d2;
    *buf1 = r[0] > 0 ? (size_t)t[0] * d1 * d2 : r[1] > 0 ? (size_t)t[0] * t[1] * d2 : 0;
}

// the first tile of the list whose two LDS buffers fit kSmoothLds: a function of the radii and the element size alone
static inline void smooth_tile(size_t es, const int *r, int *t) {
    for (const auto &c : kSmoothTiles) {
        size_t b0, b1;
        smooth_lds(c, r, &b0, &b1);
        t[0] = c[0], t[1] = c[1], t[2] = c[2];
        if ((b0 + b1) * es <= kSmoothLds) return;
    }
}

__global__ void smooth_weights_kernel(SmoothWeights sw, double *ws) {
    const int i = threadIdx.x;
    if (i < 3 * kSmoothSlot) ws[i] = sw.w[i / kSmoothSlot][i % kSmoothSlot];
}

template <typename T> __device__ __forceinline__ T finite_or_zero(T v) { return std::fabs(v) < (T)__builtin_inf() ? v : (T)0; }

// i = q d + rem for 0 <= i < 2^22 and 1 <= d <= 2^11: the float quotient is off by one at most, and is put right.  (The
// integer division of the compiler costs more than the load or the eleven taps it would address.)
struct SmoothDiv {
    int d;
    float inv;
    __device__ __forceinline__ explicit SmoothDiv(int d_) : d(d_), inv(1.0f / (float)d_) {}
    __device__ __forceinline__ int operator()(int i, int &rem) const {
        int q = (int)((float)i * inv);
        rem = i - q * d;
        if (rem < 0) { --q; rem += d; }
        else if (rem >= d) { ++q; rem -= d; }
        return q;
    }
};

// sum_j w[j] src[base + j stride], j = 0 .. 2 R, in f64 in ascending j; the 2 R + 1 LDS reads are issued before the sum
template <typename T, int R>
__device__ __forceinline__ double smooth_taps(const T *src, int base, int stride, const double *__restrict__ w) {
    T x[2 * R + 1];
#pragma unroll
    for (int j = 0; j <= 2 * R; ++j) x[j] = src[base + j * stride];
    double s = 0.0;
#pragma unroll
    for (int j = 0; j <= 2 * R; ++j) s = __builtin_fma(w[j], (double)x[j], s);
    return s;
}

// axis 0: (d0, d1, d2) -> (t0, d1, d2), the same linear index in both
template <typename T, int R>
__device__ __forceinline__ void smooth_pass0(const T *src, T *dst, int n_out, int plane, const double *__restrict__ w) {
    for (int i = threadIdx.x; i < n_out; i += kSmoothThreads) dst[i] = (T)smooth_taps<T, R>(src, i, plane, w);
}

// axis 1: (t0, d1, d2) -> (t0, t1, d2)
template <typename T, int R>
__device__ __forceinline__ void smooth_pass1(const T *src, T *dst, int t0, int t1, int d1, int d2,
                                             const double *__restrict__ w) {
    const SmoothDiv by_d2(d2), by_t1(t1);
    for (int i = threadIdx.x; i < t0 * t1 * d2; i += kSmoothThreads) {
        int p2, p1;
        const int q = by_d2(i, p2), p0 = by_t1(q, p1);
        dst[i] = (T)smooth_taps<T, R>(src, (p0 * d1 + p1) * d2 + p2, d2, w);
    }
}

// axis 2 and the mask: (t0, t1, d2) -> the masked voxels of the tile, straight into the row of d_out
template <typename T, int R>
__device__ __forceinline__ void smooth_store(const T *src, const SmoothGeom &g, int o0, int o1, int o2, int d2,
                                             const double *__restrict__ w, const int32_t *__restrict__ col, int64_t V,
                                             T *out_row) {
    const int t1 = g.t[1], t2 = g.t[2], n1 = g.n[1], n2 = g.n[2];
    const SmoothDiv by_t2(t2), by_t1(t1);
    for (int i = threadIdx.x; i < g.t[0] * t1 * t2; i += kSmoothThreads) {
        int p2, p1;
        const int q = by_t2(i, p2), p0 = by_t1(q, p1);
        if (o0 + p0 >= g.n[0] || o1 + p1 >= n1 || o2 + p2 >= n2) continue;
        const int c = col[((int64_t)(o0 + p0) * n1 + o1 + p1) * n2 + o2 + p2];
        if ((uint64_t)c >= (uint64_t)V) continue;             // outside the mask (-1), or no column of d_out
        const int base = (p0 * t1 + p1) * d2 + p2;
        out_row[c] = R > 0 ? (T)smooth_taps<T, R>(src, base, 1, w) : src[base];
    }
}

// the radius is uniform over the launch: one switch per pass, the taps unrolled inside
#define MODL_SMOOTH_R(r, CALL)                          \
    switch (r) {                                        \
        case 1: { constexpr int R = 1; CALL; } break;   \
        case 2: { constexpr int R = 2; CALL; } break;   \
        case 3: { constexpr int R = 3; CALL; } break;   \
        case 4: { constexpr int R = 4; CALL; } break;   \
        case 5: { constexpr int R = 5; CALL; } break;   \
        case 6: { constexpr int R = 6; CALL; } break;   \
        case 7: { constexpr int R = 7; CALL; } break;   \
        case 8: { constexpr int R = 8; CALL; } break;   \
        default: break;                                 \
    }
static_assert(kSmoothMaxR == 8, "MODL_SMOOTH_R lists the radii");

template <typename T>
__global__ __launch_bounds__(kSmoothThreads) void smooth_mask_kernel(const T *__restrict__ vol, int64_t fs, int64_t n_frames,
                                                                      SmoothGeom g, const double *__restrict__ w,
                                                                      const int32_t *__restrict__ col, int64_t V,
                                                                      const int64_t *__restrict__ dst_row, T *out,
                                                                      int64_t ldo, int buf1_off) {
    extern __shared__ __attribute__((aligned(16))) char smooth_smem[];
    __shared__ int tab[3][kSmoothMaxTile + 2 * kSmoothMaxR];     // the reflected box index of every halo coordinate
    T *buf0 = (T *)smooth_smem, *buf1 = buf0 + buf1_off;
    const int tid = threadIdx.x;
    const int t0 = g.t[0], t1 = g.t[1], t2 = g.t[2];
    const int b2 = blockIdx.x % g.nt[2], bq = blockIdx.x / g.nt[2];
    const int o0 = (bq / g.nt[1]) * t0, o1 = (bq % g.nt[1]) * t1, o2 = b2 * t2;
    const int n1 = g.n[1], n2 = g.n[2];
    // ---- the tile's slice of the column map: nothing of the volume is read for a tile outside the mask
    int any = 0;
    const SmoothDiv by_t2(t2), by_t1(t1);
    for (int i = tid; i < t0 * t1 * t2; i += kSmoothThreads) {
        int p2, p1;
        const int q = by_t2(i, p2), p0 = by_t1(q, p1);
        if (o0 + p0 < g.n[0] && o1 + p1 < n1 && o2 + p2 < n2) any |= col[((int64_t)(o0 + p0) * n1 + o1 + p1) * n2 + o2 + p2] >= 0;
    }
    if (!__syncthreads_or(any)) return;
    const int d0 = t0 + 2 * g.r[0], d1 = t1 + 2 * g.r[1], d2 = t2 + 2 * g.r[2];
    for (int i = tid; i < d0 + d1 + d2; i += kSmoothThreads) {
        const int a = i < d0 ? 0 : i < d0 + d1 ? 1 : 2;
        const int l = i - (a == 0 ? 0 : a == 1 ? d0 : d0 + d1);
        const int n = g.n[a];
        int x = (a == 0 ? o0 : a == 1 ? o1 : o2) + l - g.r[a];
        while (x < 0 || x >= n) x = x < 0 ? -1 - x : 2 * n - 1 - x;      // 'reflect': d c b a | a b c d | d c b a
        tab[a][l] = x;
    }
    __syncthreads();
    const double *w0 = w, *w1 = w + kSmoothSlot, *w2 = w + 2 * kSmoothSlot;
    const int halo = d0 * d1 * d2;
    const SmoothDiv by_d2(d2), by_d1(d1);
    constexpr int U = 8;                                     // loads of a thread in flight
    for (int64_t f = blockIdx.y; f < n_frames; f += gridDim.y) {
        const T *frame = vol + f * fs;
        for (int i0 = tid; i0 < halo; i0 += U * kSmoothThreads) {
            T v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {                    // (an index past the end repeats the last element; not stored)
                const int i = min(i0 + u * kSmoothThreads, halo - 1);
                int l2, l1;
                const int q = by_d2(i, l2), l0 = by_d1(q, l1);
                v[u] = frame[((int64_t)tab[0][l0] * n1 + tab[1][l1]) * n2 + tab[2][l2]];
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (i0 + u * kSmoothThreads < halo) buf0[i0 + u * kSmoothThreads] = finite_or_zero(v[u]);
        }
        __syncthreads();
        T *cur = buf0;
        if (g.r[0] > 0) {
            MODL_SMOOTH_R(g.r[0], (smooth_pass0<T, R>(buf0, buf1, t0 * d1 * d2, d1 * d2, w0)));
            cur = buf1;
            __syncthreads();
        }
        if (g.r[1] > 0) {
            T *dst = cur == buf0 ? buf1 : buf0;
            MODL_SMOOTH_R(g.r[1], (smooth_pass1<T, R>(cur, dst, t0, t1, d1, d2, w1)));
            cur = dst;
            __syncthreads();
        }
        const int64_t row = dst_row ? dst_row[f] : f;
        if ((uint64_t)row < (uint64_t)n_frames) {
            if (g.r[2] > 0) {
                MODL_SMOOTH_R(g.r[2], (smooth_store<T, R>(cur, g, o0, o1, o2, d2, w2, col, V, out + row * ldo)));
            } else {
                smooth_store<T, 0>(cur, g, o0, o1, o2, d2, w2, col, V, out + row * ldo);
            }
        }
        __syncthreads();                                     // (the next frame overwrites both buffers)
    }
}

// all radii 0: out[t][col[v]] = finite_or_zero(vol[t][v])
template <typename T>
__global__ __launch_bounds__(256) void mask_gather_kernel(const T *__restrict__ vol, int64_t fs, int64_t n_frames, int64_t box,
                                                          const int32_t *__restrict__ col, int64_t V,
                                                          const int64_t *__restrict__ dst_row, T *out, int64_t ldo) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= box) return;
    const int c = col[v];
    if ((uint64_t)c >= (uint64_t)V) return;
    for (int64_t f = blockIdx.y; f < n_frames; f += gridDim.y) {
        const int64_t row = dst_row ? dst_row[f] : f;
        if ((uint64_t)row < (uint64_t)n_frames) out[row * ldo + c] = finite_or_zero(vol[f * fs + v]);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void unmask_kernel(const T *__restrict__ rows, int64_t ldr, int64_t n, int64_t V,
                                                     const int64_t *__restrict__ vox, int64_t box, T *out) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= V) return;
    const int64_t v = vox[c];
    if ((uint64_t)v >= (uint64_t)box) return;
    for (int64_t i = blockIdx.y; i < n; i += gridDim.y) out[i * box + v] = rows[i * ldr + c];
}

static inline bool smooth_radii_ok(int r0, int r1, int r2) {
    return r0 >= 0 && r0 <= kSmoothMaxR && r1 >= 0 && r1 <= kSmoothMaxR && r2 >= 0 && r2 <= kSmoothMaxR;
}

static inline bool smooth_box_ok(int64_t n0, int64_t n1, int64_t n2) {
    return n0 >= 1 && n1 >= 1 && n2 >= 1 && n0 <= kSmoothMaxEdge && n1 <= kSmoothMaxEdge && n2 <= kSmoothMaxEdge &&
           n0 <= INT32_MAX / n1 && n0 * n1 <= INT32_MAX / n2;
}

static inline bool ranges_overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

template <typename T>
static int smooth_mask_abi(const T *vol, int64_t fs, int64_t n_frames, int64_t n0, int64_t n1, int64_t n2, const double *w0,
                           int r0, const double *w1, int r1, const double *w2, int r2, const int32_t *col, int64_t V,
                           const int64_t *dst_row, T *out, int64_t ldo, void *ws, size_t ws_bytes, void *stream_) {
    if (!vol || !col || !out || n_frames < 1 || V < 1 || !smooth_box_ok(n0, n1, n2) || !smooth_radii_ok(r0, r1, r2)) return MODL_EINVAL;
    const int64_t box = n0 * n1 * n2;
    if (V > box || ldo < V || fs < box || fs > INT64_MAX / 8 / n_frames || ldo > INT64_MAX / 8 / n_frames) return MODL_EINVAL;
    const double *wa[3] = {w0, w1, w2};
    SmoothGeom g;
    SmoothWeights sw = {};
    const int64_t n[3] = {n0, n1, n2};
    const int rin[3] = {r0, r1, r2};
    for (int a = 0; a < 3; ++a) {
        g.n[a] = (int)n[a];
        g.r[a] = wa[a] ? rin[a] : 0;                        // a NULL pointer: the axis is untouched
        double sum = 0.0;
        for (int j = 0; j <= 2 * g.r[a] && g.r[a] > 0; ++j) {
            const double x = wa[a][j];
            if (!std::isfinite(x) || x < 0.0) return MODL_EINVAL;
            sw.w[a][j] = x;
            sum += x;
        }
        if (g.r[a] > 0 && !(std::fabs(sum - 1.0) <= 1e-12)) return MODL_EINVAL;
    }
    if (ranges_overlap(vol, (size_t)((n_frames - 1) * fs + box) * sizeof(T), out, (size_t)((n_frames - 1) * ldo + V) * sizeof(T)))
        return MODL_EINVAL;
    const size_t need = modl_smooth_mask_workspace(DType<T>::id, n_frames, n0, n1, n2, r0, r1, r2);
    if (need == 0) return MODL_EINVAL;
    if (!ws || ws_bytes < need) return MODL_ENOMEM;
    if (modl_device_count() <= 0) return MODL_ENOGPU;
    hipStream_t stream = (hipStream_t)stream_;
    unsigned gy = (unsigned)std::min<int64_t>(n_frames, 65535);
    if (g.r[0] == 0 && g.r[1] == 0 && g.r[2] == 0) {
        hipLaunchKernelGGL(mask_gather_kernel<T>, dim3((unsigned)cdiv(box, 256), gy), dim3(256), 0, stream, vol, fs, n_frames,
                           box, col, V, dst_row, out, ldo);
        MODL_LAUNCH_CHECK();
        return MODL_OK;
    }
    hipLaunchKernelGGL(smooth_weights_kernel, dim3(1), dim3(64), 0, stream, sw, (double *)ws);
    MODL_LAUNCH_CHECK();
    smooth_tile(sizeof(T), g.r, g.t);
    int64_t tiles = 1;
    for (int a = 0; a < 3; ++a) {
        g.t[a] = std::min(g.t[a], g.n[a]);
        g.nt[a] = (int)cdiv(g.n[a], g.t[a]);
        tiles *= g.nt[a];
    }
    size_t b0, b1;
    smooth_lds(g.t, g.r, &b0, &b1);
    const size_t lds = (b0 + b1) * sizeof(T);
    // a workgroup keeps its tile over the frames f = y, y + gy, ...: enough workgroups to fill the device many times over,
    // few enough that the ones of the tiles outside the mask (which leave at once) stay cheap
    gy = (unsigned)std::min<int64_t>(gy, std::max<int64_t>(1, kSmoothGrid / tiles));
    if (lds > 64 * 1024)
        MODL_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&smooth_mask_kernel<T>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSmoothLds));
    hipLaunchKernelGGL(smooth_mask_kernel<T>, dim3((unsigned)tiles, gy), dim3(kSmoothThreads), lds, stream, vol, fs, n_frames, g,
                       (const double *)ws, col, V, dst_row, out, ldo, (int)b0);
    MODL_LAUNCH_CHECK();
    return MODL_OK;
}

template <typename T>
static int unmask_abi(const T *rows, int64_t ldr, int64_t n, int64_t V, const int64_t *vox, int64_t n0, int64_t n1, int64_t n2,
                      T *out, void *stream_) {
    if (!rows || !vox || !out || n < 1 || V < 1 || !smooth_box_ok(n0, n1, n2)) return MODL_EINVAL;
    const int64_t box = n0 * n1 * n2;
    if (V > box || ldr < V || ldr > INT64_MAX / 8 / n || box > INT64_MAX / 8 / n) return MODL_EINVAL;
    if (ranges_overlap(rows, (size_t)((n - 1) * ldr + V) * sizeof(T), out, (size_t)(n * box) * sizeof(T))) return MODL_EINVAL;
    if (modl_device_count() <= 0) return MODL_ENOGPU;
    hipStream_t stream = (hipStream_t)stream_;
    MODL_HIP(hipMemsetAsync(out, 0, (size_t)(n * box) * sizeof(T), stream));
    hipLaunchKernelGGL(unmask_kernel<T>, dim3((unsigned)cdiv(V, 256), (unsigned)std::min<int64_t>(n, 65535)), dim3(256), 0, stream,
                       rows, ldr, n, V, vox, box, out);
    MODL_LAUNCH_CHECK();
    return MODL_OK;
}

}  // namespace modl

using namespace modl;

extern "C" {

int modl_smooth_max_radius(void) { return kSmoothMaxR; }

int modl_smooth_tile(int dtype, int r0, int r1, int r2, int *tile) {
    if ((dtype != MODL_F32 && dtype != MODL_F64) || !smooth_radii_ok(r0, r1, r2) || !tile) return MODL_EINVAL;
    const int r[3] = {r0, r1, r2};
    smooth_tile(dtype == MODL_F32 ? 4 : 8, r, tile);
    return MODL_OK;
}

size_t modl_smooth_mask_workspace(int dtype, int64_t T, int64_t n0, int64_t n1, int64_t n2, int r0, int r1, int r2) {
    if ((dtype != MODL_F32 && dtype != MODL_F64) || T < 1 || !smooth_box_ok(n0, n1, n2) || !smooth_radii_ok(r0, r1, r2)) return 0;
    return align_up(3 * kSmoothSlot * sizeof(double), 256);
}

int modl_smooth_mask_f32(const float *d_vol, int64_t frame_stride, int64_t T, int64_t n0, int64_t n1, int64_t n2,
                         const double *w0, int r0, const double *w1, int r1, const double *w2, int r2, const int32_t *d_col,
                         int64_t V, const int64_t *d_dst_row, float *d_out, int64_t ldo, void *d_ws, size_t ws_bytes,
                         void *stream) {
    return smooth_mask_abi<float>(d_vol, frame_stride, T, n0, n1, n2, w0, r0, w1, r1, w2, r2, d_col, V, d_dst_row, d_out, ldo,
                                  d_ws, ws_bytes, stream);
}

int modl_smooth_mask_f64(const double *d_vol, int64_t frame_stride, int64_t T, int64_t n0, int64_t n1, int64_t n2,
                         const double *w0, int r0, const double *w1, int r1, const double *w2, int r2, const int32_t *d_col,
                         int64_t V, const int64_t *d_dst_row, double *d_out, int64_t ldo, void *d_ws, size_t ws_bytes,
                         void *stream) {
    return smooth_mask_abi<double>(d_vol, frame_stride, T, n0, n1, n2, w0, r0, w1, r1, w2, r2, d_col, V, d_dst_row, d_out, ldo,
                                   d_ws, ws_bytes, stream);
}

int modl_unmask_f32(const float *d_rows, int64_t ldr, int64_t n, int64_t V, const int64_t *d_vox, int64_t n0, int64_t n1,
                    int64_t n2, float *d_out, void *stream) {
    return unmask_abi<float>(d_rows, ldr, n, V, d_vox, n0, n1, n2, d_out, stream);
}

int modl_unmask_f64(const double *d_rows, int64_t ldr, int64_t n, int64_t V, const int64_t *d_vox, int64_t n0, int64_t n1,
                    int64_t n2, double *d_out, void *stream) {
    return unmask_abi<double>(d_rows, ldr, n, V, d_vox, n0, n1, n2, d_out, stream);
}

}  // extern "C"
