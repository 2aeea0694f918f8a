// what sits either side of the SOMF step.
//   image patch pipeline  : modl/feature_extraction/image.py:54-63 (LazyCleanPatchExtractor.partial_transform: a fancy
//                           index into the sliding-window view of the image) fused with
//                           modl/input_data/image.py:4-23 (scale_patches, channel-wise) and the flattening of
//                           modl/decomposition/image.py:190-199 -- the image stays resident in HBM, a minibatch
//                           buffer of flattened, centred, normalised patches is produced by one launch;
//   fill / clean_mask     : modl/input_data/image_fast.pyx:12-74 (host, integer work);
//   objective terms       : modl/decomposition/dict_fact.py:94-114 (CodingMixin.score) on device-resident X, codes
//                           and dictionary, so that scoring callbacks need no D2H copy of the dictionary.
// Beyond the reference (it has no reconstruction): the way back from codes to an image on a regular PATCH GRID -
// grid patches that keep their scaling, decode with unscale, overlap-add, finish (see "reconstruction" below).
#include "gemm.hpp"
#include "kernels.hpp"
#include <algorithm>
#include <vector>

namespace modl {

// ---- patches ------------------------------------------------------------------------------------------------------
// One wavefront per patch.  A patch is the window image[i : i + x, j : j + y, c0 : c0 + z]; its flattened row is
// (x, y, z) in C order.  Channel statistics are taken over the x * y positions of each channel (numpy: axis=(1, 2)):
//   with_mean: v -= mean_c;   with_std: v /= (sqrt(sum_c v^2) or 1 if 0) * sqrt(z)
// The image (a few MB) is L2-resident; the row is written once, coalesced, in flat element order.
constexpr int kPatchMaxChannels = 1024;

// The row of one patch by one wavefront (the body of both patch kernels, so that their rows agree bit for bit): `base`
// = the window's first element, z channels from there.  s_mean / s_den: this wavefront's z slots of LDS.
template <typename T>
__device__ __forceinline__ void patch_row(const T *__restrict__ base, int64_t W, int64_t C, int x, int y, int z,
                                          int with_mean, int with_std, T sqrt_z, T *s_mean, T *s_den,
                                          T *__restrict__ o) {
    const int lane = threadIdx.x & 63;
    const int xy = x * y;
    if (with_mean || with_std) {
        for (int c = 0; c < z; ++c) {
            T mean = 0;
            if (with_mean) {
                T s = 0;
                for (int pos = lane; pos < xy; pos += 64) s += base[((int64_t)(pos / y) * W + pos % y) * C + c];
                mean = wave_sum(s) / (T)xy;
            }
            T den = 1;
            if (with_std) {
                T s = 0;
                for (int pos = lane; pos < xy; pos += 64) {
                    const T v = base[((int64_t)(pos / y) * W + pos % y) * C + c] - mean;
                    s += v * v;
                }
                T sd = sqrt(wave_sum(s));
                if (sd == (T)0) sd = 1;
                den = sd * sqrt_z;
            }
            if (lane == 0) { s_mean[c] = mean; s_den[c] = den; }
        }
    }
    __builtin_amdgcn_wave_barrier();                          // LDS operations of one wavefront complete in order
    const int P = xy * z;
    const int yz = y * z;
    for (int e = lane; e < P; e += 64) {
        const int xi = e / yz, rem = e - xi * yz;             // rem = yi * z + c: contiguous in the image row
        const int c = rem % z;
        T v = base[(int64_t)xi * W * C + (int64_t)(rem / z) * C + c];
        if (with_mean) v -= s_mean[c];
        if (with_std) v /= s_den[c];
        o[e] = v;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void image_patches_kernel(const T *__restrict__ img, int64_t W, int64_t C,
                                                            const int64_t *__restrict__ idx3, int64_t n, int x, int y,
                                                            int z, int with_mean, int with_std, T sqrt_z,
                                                            T *__restrict__ out, int64_t ldo) {
    __shared__ T s_mean[4][kPatchMaxChannels];
    __shared__ T s_den[4][kPatchMaxChannels];
    const int wid = threadIdx.x >> 6;
    const int64_t row = (int64_t)blockIdx.x * 4 + wid;
    if (row >= n) return;                                     // wave-uniform; no block barrier below
    const int64_t i0 = idx3[row * 3 + 0], j0 = idx3[row * 3 + 1], c0 = idx3[row * 3 + 2];
    patch_row<T>(img + (i0 * W + j0) * C + c0, W, C, x, y, z, with_mean, with_std, sqrt_z, s_mean[wid], s_den[wid],
                 out + row * ldo);
}

template <typename T>
int launch_image_patches(hipStream_t stream, const T *img, int64_t H, int64_t W, int64_t C, const int64_t *idx3,
                         int64_t n, int x, int y, int z, int with_mean, int with_std, T *out, int64_t ldo) {
    if (n <= 0) return MODL_OK;
    hipLaunchKernelGGL((image_patches_kernel<T>), dim3((unsigned)cdiv(n, 4)), dim3(256), 0, stream, img, W, C, idx3, n,
                       x, y, z, with_mean, with_std, (T)sqrt((double)z), out, ldo);
    MODL_LAUNCH_CHECK();
    return MODL_OK;
}

// ---- objective ----------------------------------------------------------------------------------------------------
template <typename T> struct EpiResidual {     // R[m][n] = X[m][n] - v
    const T *X; int64_t ldx; T *R; int64_t ldr;
    __device__ __forceinline__ void operator()(int64_t m, int64_t n, T v) const { R[m * ldr + n] = X[m * ldx + n] - v; }
};

constexpr int kObjBlocks = 1024;

// part[b] = sum over the elements owned by block b of f(a): MODE 0 a^2, 1 |a|.  f64 accumulation, fixed order.
template <typename T, int MODE>
__global__ __launch_bounds__(256) void obj_partial_kernel(const T *a, int64_t rows, int64_t cols, int64_t ld,
                                                          double *part) {
    __shared__ double red[4];
    const int64_t total = rows * cols;
    double s = 0;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const double v = (double)a[(e / cols) * ld + e % cols];
        s += MODE == 0 ? v * v : fabs(v);
    }
    s = block_sum(s, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}
__global__ __launch_bounds__(256) void obj_final_kernel(const double *part, int m, double *out, int accumulate) {
    __shared__ double red[4];
    double s = 0;
    for (int i = threadIdx.x; i < m; i += 256) s += part[i];
    s = block_sum(s, red);
    if (threadIdx.x == 0) *out = accumulate ? *out + s : s;
}

template <typename T>
int objective_impl(hipStream_t stream, const T *X, int64_t ldx, int64_t n, int64_t p, const T *Dt, int k, const T *code,
                   void *ws, size_t ws_bytes, double *out3) {
    if (ws_bytes < sizeof(double) * kObjBlocks + sizeof(T) * (size_t)p) return MODL_ENOMEM;
    double *part = static_cast<double *>(ws);
    T *R = reinterpret_cast<T *>(part + kObjBlocks);
    const int64_t chunk = (int64_t)((ws_bytes - sizeof(double) * kObjBlocks) / (sizeof(T) * (size_t)p));
    MODL_HIP(hipMemsetAsync(out3, 0, 3 * sizeof(double), stream));
    if (n == 0) return MODL_OK;
    for (int64_t r0 = 0; r0 < n; r0 += chunk) {
        const int64_t rows = (n - r0 < chunk) ? n - r0 : chunk;
        Operand A, B;
        A.ptr = code + r0 * k; A.si = k; A.sk = 1;
        B.ptr = Dt; B.si = k; B.sk = 1;
        EpiResidual<T> epi{X + r0 * ldx, ldx, R, p};
        MODL_TRY((launch_gemm<T, EpiResidual<T>>(stream, A, B, rows, p, k, epi, SplitWs{}, nullptr, 512, 1)));
        hipLaunchKernelGGL((obj_partial_kernel<T, 0>), dim3(kObjBlocks), dim3(256), 0, stream, R, rows, p, p, part);
        hipLaunchKernelGGL(obj_final_kernel, dim3(1), dim3(256), 0, stream, part, kObjBlocks, out3, 1);
        MODL_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL((obj_partial_kernel<T, 1>), dim3(kObjBlocks), dim3(256), 0, stream, code, n, (int64_t)k, (int64_t)k, part);
    hipLaunchKernelGGL(obj_final_kernel, dim3(1), dim3(256), 0, stream, part, kObjBlocks, out3 + 1, 0);
    hipLaunchKernelGGL((obj_partial_kernel<T, 0>), dim3(kObjBlocks), dim3(256), 0, stream, code, n, (int64_t)k, (int64_t)k, part);
    hipLaunchKernelGGL(obj_final_kernel, dim3(1), dim3(256), 0, stream, part, kObjBlocks, out3 + 2, 0);
    MODL_LAUNCH_CHECK();
    return MODL_OK;
}

// ---- reconstruction -----------------------------------------------------------------------------------------------
// THE PATCH GRID (stated once, here; modl_hip.h and modl_amd/image.py:grid_origins restate it).  Along an axis of
// length L with patch length x and stride s (1 <= s <= x <= L) the origins are 0, s, 2 s, ... <= L - x, plus L - x
// itself when it is not the last of them, so the border is always covered:
//   count  g = ceil((L - x) / s) + 1,   origin(r) = min(r s, L - x).
// A patch spans all channels (z = C, c0 = 0); patches are numbered row-major over (grid row, grid column).  A PASS is
// the contiguous range of grid rows [row0, row0 + nrows); its patch q sits at grid (row0 + q / gcols, q % gcols).
// Pixel t of the axis is covered by the grid indices [lo, hi]: lo = the first r with r s > t - x, hi = t / s, or the
// clamped last index g - 1 once t >= L - x (every r <= g - 2 has r s < L - x, so only the last origin is clamped).
struct GridAxis {
    int64_t L, g;
    int x, s;
    __host__ __device__ __forceinline__ int64_t origin(int64_t r) const { return r * s < L - x ? r * s : L - x; }
    __host__ __device__ __forceinline__ int64_t lo(int64_t t) const { return t - x + s > 0 ? (t - x + s) / s : 0; }
    __host__ __device__ __forceinline__ int64_t hi(int64_t t) const { return t >= L - x ? g - 1 : t / s; }
};
static inline bool grid_axis(int64_t L, int64_t x, int64_t s, GridAxis *a) {
    if (x <= 0 || s <= 0 || s > x || x > L || x > INT32_MAX) return false;
    a->L = L; a->x = (int)x; a->s = (int)s; a->g = cdiv(L - x, s) + 1;
    return true;
}

// image_patches_kernel on the grid: one wavefront per patch of the pass, the origin computed, no index array; the
// statistics that the scaling applied are kept: mean[q][C] and den[q][C] (the divisor actually applied, 1 where none
// was), so that a decoded patch can be put back on the image's scale.
template <typename T>
__global__ __launch_bounds__(256) void image_grid_patches_kernel(const T *__restrict__ img, int64_t C, GridAxis gi,
                                                                 GridAxis gj, int64_t row0, int64_t n, int with_mean,
                                                                 int with_std, T sqrt_z, T *__restrict__ out,
                                                                 int64_t ldo, T *__restrict__ mean,
                                                                 T *__restrict__ den) {
    __shared__ T s_mean[4][kPatchMaxChannels];
    __shared__ T s_den[4][kPatchMaxChannels];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int64_t q = (int64_t)blockIdx.x * 4 + wid;
    if (q >= n) return;                                       // wave-uniform; no block barrier below
    const int64_t i0 = gi.origin(row0 + q / gj.g), j0 = gj.origin(q % gj.g);
    const int z = (int)C;
    if (!(with_mean || with_std))
        for (int c = lane; c < z; c += 64) { s_mean[wid][c] = 0; s_den[wid][c] = 1; }
    patch_row<T>(img + (i0 * gj.L + j0) * C, gj.L, C, gi.x, gj.x, z, with_mean, with_std, sqrt_z, s_mean[wid],
                 s_den[wid], out + q * ldo);
    for (int c = lane; c < z; c += 64) { mean[q * C + c] = s_mean[wid][c]; den[q * C + c] = s_den[wid][c]; }
}

// decode: R[m][e] = (code D)[m][e] * den[m][e % C] + mean[m][e % C]; without mean / den the plain product
template <typename T> struct EpiUnscale {
    T *R; int64_t ldr; const T *mean, *den; int C;
    __device__ __forceinline__ void operator()(int64_t m, int64_t n, T v) const {
        if (mean) {
            const int64_t s = m * C + (int)n % C;
            v = v * den[s] + mean[s];
        }
        R[m * ldr + n] = v;
    }
};

constexpr int64_t kDecodeChunk = (int64_t)1 << 21;            // rows per product launch: 32 768 row tiles of 64 in gridDim.y

template <typename T>
int decode_impl(hipStream_t stream, const T *code, int64_t n, int k, const T *Dt, int64_t P, int C, const T *mean,
                const T *den, T *out, int64_t ldo) {
    for (int64_t r0 = 0; r0 < n; r0 += kDecodeChunk) {
        const int64_t rows = n - r0 < kDecodeChunk ? n - r0 : kDecodeChunk;
        Operand A, B;
        A.ptr = code + r0 * k; A.si = k; A.sk = 1;
        B.ptr = Dt; B.si = k; B.sk = 1;
        EpiUnscale<T> epi{out + r0 * ldo, ldo, mean ? mean + r0 * C : nullptr, den ? den + r0 * C : nullptr, C};
        MODL_TRY((launch_gemm<T, EpiUnscale<T>>(stream, A, B, rows, P, k, epi, SplitWs{}, nullptr, 512, 1)));
    }
    return MODL_OK;
}

// overlap-add as a GATHER: one thread per (pixel, channel) of the pixel rows [i_begin, i_begin + rows) that the pass
// touches.  The thread loads its f64 accumulator, adds the values of the covering patches of this pass one at a time
// in grid order (grid row outer, grid column inner; their offsets follow from the grid, there is no index), stores it.
// Every accumulator therefore sees the same additions in the same order however the grid rows are cut into passes:
// no atomics, bit-identical from run to run and from partition to partition.  Reads of the patches: for one step of
// the loop, neighbouring pixels read the SAME in-patch position of NEIGHBOURING patches (stride ldp), C contiguous
// channels each - runs of C elements, not coalesced; every element of the pass is read exactly once, and the lines
// are reused from L2 by the later steps of the same wavefront.
template <typename T>
__global__ __launch_bounds__(256) void image_overlap_add_kernel(const T *__restrict__ patches, int64_t ldp, int64_t C,
                                                                GridAxis gi, GridAxis gj, int64_t row0, int64_t nrows,
                                                                int64_t i_begin, int64_t total,
                                                                double *__restrict__ acc) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int64_t WC = gj.L * C;
    const int64_t i = i_begin + e / WC, rem = e % WC, j = rem / C, c = rem % C;
    int64_t r_lo = gi.lo(i), r_hi = gi.hi(i);
    if (r_lo < row0) r_lo = row0;
    if (r_hi > row0 + nrows - 1) r_hi = row0 + nrows - 1;
    const int64_t c_lo = gj.lo(j), c_hi = gj.hi(j);
    double *a = acc + i * WC + rem;
    double s = *a;
    for (int64_t gr = r_lo; gr <= r_hi; ++gr) {
        const int64_t di = i - gi.origin(gr);
        for (int64_t gc = c_lo; gc <= c_hi; ++gc) {
            const int64_t dj = j - gj.origin(gc);
            s += (double)patches[((gr - row0) * gj.g + gc) * ldp + (di * gj.x + dj) * C + c];
        }
    }
    *a = s;
}

// image = accumulator / cover count; the count of a pixel is analytic: (grid rows over i) * (grid columns over j)
template <typename T>
__global__ __launch_bounds__(256) void image_overlap_finish_kernel(const double *__restrict__ acc, int64_t C,
                                                                   GridAxis gi, GridAxis gj, int64_t total,
                                                                   T *__restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int64_t WC = gj.L * C;
    const int64_t i = e / WC, j = e % WC / C;
    const int64_t cnt = (gi.hi(i) - gi.lo(i) + 1) * (gj.hi(j) - gj.lo(j) + 1);
    out[e] = (T)(acc[e] / (double)cnt);
}

// ---- inpainting ---------------------------------------------------------------------------------------------------
// image_grid_patches_kernel on an image with holes (obs[H][W][C], 1 = observed).  A window without a hole takes
// patch_row itself, so its row, mean and den are those of modl_image_grid_patches_* bit for bit.  Otherwise the
// statistics of a channel are taken over its n_c OBSERVED positions: mean_c = sum / n_c; the norm of the centred
// observed values times sqrt(x y / n_c) estimates the norm of the full window (1 if it is 0 or n_c = 0); unobserved
// elements of the row are 0.  obs_out[q][:] is the window of obs in the row's element order, nobs[q] its sum.
// One window of an image with holes, by one wavefront: the device code both masked patch kernels share (the grid
// kernel computes the origin, the index-list kernel reads it), so that the same origin gives the same bits.
template <typename T>
__device__ __forceinline__ void masked_patch_window(const T *__restrict__ base, const uint8_t *__restrict__ obase,
                                                    int64_t W, int64_t C, int x, int y, int with_mean, int with_std,
                                                    T sqrt_z, T *s_mean, T *s_den, T *__restrict__ o,
                                                    uint8_t *__restrict__ oo, int32_t *__restrict__ nobs_q,
                                                    T *__restrict__ mean_q, T *__restrict__ den_q) {
    const int lane = threadIdx.x & 63;
    const int z = (int)C, xy = x * y, yz = y * z, P = xy * z;
    int cnt = 0;
    for (int e = lane; e < P; e += 64) {
        const int xi = e / yz, rem = e - xi * yz;
        const uint8_t on = obase[(int64_t)xi * W * C + rem] != 0;
        oo[e] = on;
        cnt += on;
    }
    cnt = (int)wave_sum((double)cnt);
    if (lane == 0) *nobs_q = cnt;
    if (cnt == P) {                                           // wave-uniform: the clean window
        if (!(with_mean || with_std))
            for (int c = lane; c < z; c += 64) { s_mean[c] = 0; s_den[c] = 1; }
        patch_row<T>(base, W, C, x, y, z, with_mean, with_std, sqrt_z, s_mean, s_den, o);
    } else {
        for (int c = 0; c < z; ++c) {
            T s = 0;
            int nc = 0;
            for (int pos = lane; pos < xy; pos += 64) {
                const int64_t at = ((int64_t)(pos / y) * W + pos % y) * C + c;
                const bool on = obase[at] != 0;
                const T v = base[at];
                s += on ? v : (T)0;
                nc += on;
            }
            nc = (int)wave_sum((double)nc);
            const T m = (with_mean && nc > 0) ? wave_sum(s) / (T)nc : (T)0;
            T d = 1;
            if (with_std) {
                T s2 = 0;
                for (int pos = lane; pos < xy; pos += 64) {
                    const int64_t at = ((int64_t)(pos / y) * W + pos % y) * C + c;
                    const T u = base[at] - m;
                    s2 += obase[at] != 0 ? u * u : (T)0;
                }
                T sd = nc > 0 ? sqrt(wave_sum(s2)) * sqrt((T)xy / (T)nc) : (T)1;
                if (sd == (T)0) sd = 1;
                d = sd * sqrt_z;
            }
            if (lane == 0) { s_mean[c] = m; s_den[c] = d; }
        }
        __builtin_amdgcn_wave_barrier();
        for (int e = lane; e < P; e += 64) {
            const int xi = e / yz, rem = e - xi * yz, c = rem % z;
            const int64_t at = (int64_t)xi * W * C + rem;
            T v = base[at];
            if (with_mean) v -= s_mean[c];
            if (with_std) v /= s_den[c];
            o[e] = obase[at] != 0 ? v : (T)0;
        }
    }
    for (int c = lane; c < z; c += 64) { mean_q[c] = s_mean[c]; den_q[c] = s_den[c]; }
}

template <typename T>
__global__ __launch_bounds__(256) void image_grid_patches_masked_kernel(
    const T *__restrict__ img, const uint8_t *__restrict__ obs, int64_t C, GridAxis gi, GridAxis gj, int64_t row0,
    int64_t n, int with_mean, int with_std, T sqrt_z, T *__restrict__ out, int64_t ldo, T *__restrict__ mean,
    T *__restrict__ den, uint8_t *__restrict__ obs_out, int32_t *__restrict__ nobs) {
    __shared__ T s_mean[4][kPatchMaxChannels];
    __shared__ T s_den[4][kPatchMaxChannels];
    const int wid = threadIdx.x >> 6;
    const int64_t q = (int64_t)blockIdx.x * 4 + wid;
    if (q >= n) return;                                       // wave-uniform; no block barrier below
    const int64_t i0 = gi.origin(row0 + q / gj.g), j0 = gj.origin(q % gj.g), W = gj.L;
    masked_patch_window<T>(img + (i0 * W + j0) * C, obs + (i0 * W + j0) * C, W, C, gi.x, gj.x, with_mean, with_std, sqrt_z,
                           s_mean[wid], s_den[wid], out + q * ldo, obs_out + q * ((int64_t)gi.x * gj.x * C), nobs + q,
                           mean + q * C, den + q * C);
}

// the same at the origins (i, j) of an index list idx3[n][3] (modl_image_patches_masked_*: windows span all channels,
// the third entry of an origin is not read)
template <typename T>
__global__ __launch_bounds__(256) void image_patches_masked_kernel(
    const T *__restrict__ img, const uint8_t *__restrict__ obs, int64_t W, int64_t C, const int64_t *__restrict__ idx3,
    int64_t n, int x, int y, int with_mean, int with_std, T sqrt_z, T *__restrict__ out, int64_t ldo,
    T *__restrict__ mean, T *__restrict__ den, uint8_t *__restrict__ obs_out, int32_t *__restrict__ nobs) {
    __shared__ T s_mean[4][kPatchMaxChannels];
    __shared__ T s_den[4][kPatchMaxChannels];
    const int wid = threadIdx.x >> 6;
    const int64_t q = (int64_t)blockIdx.x * 4 + wid;
    if (q >= n) return;                                       // wave-uniform; no block barrier below
    const int64_t i0 = idx3[q * 3 + 0], j0 = idx3[q * 3 + 1];
    masked_patch_window<T>(img + (i0 * W + j0) * C, obs + (i0 * W + j0) * C, W, C, x, y, with_mean, with_std, sqrt_z,
                           s_mean[wid], s_den[wid], out + q * ldo, obs_out + q * ((int64_t)x * y * C), nobs + q,
                           mean + q * C, den + q * C);
}


// image_overlap_add_kernel over the patches of the pass whose use[q] != 0 only; cnt[H][W] counts them per pixel (by
// the thread of channel 0).  The same gather in grid order: sums and counts do not depend on the cut into passes.
template <typename T>
__global__ __launch_bounds__(256) void image_overlap_add_weighted_kernel(
    const T *__restrict__ patches, int64_t ldp, const uint8_t *__restrict__ use, int64_t C, GridAxis gi, GridAxis gj,
    int64_t row0, int64_t nrows, int64_t i_begin, int64_t total, double *__restrict__ acc, int32_t *__restrict__ cnt) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int64_t WC = gj.L * C;
    const int64_t i = i_begin + e / WC, rem = e % WC, j = rem / C, c = rem % C;
    int64_t r_lo = gi.lo(i), r_hi = gi.hi(i);
    if (r_lo < row0) r_lo = row0;
    if (r_hi > row0 + nrows - 1) r_hi = row0 + nrows - 1;
    const int64_t c_lo = gj.lo(j), c_hi = gj.hi(j);
    double *a = acc + i * WC + rem;
    double s = *a;
    int32_t added = 0;
    for (int64_t gr = r_lo; gr <= r_hi; ++gr) {
        const int64_t di = i - gi.origin(gr);
        for (int64_t gc = c_lo; gc <= c_hi; ++gc) {
            const int64_t q = (gr - row0) * gj.g + gc;
            if (!use[q]) continue;
            const int64_t dj = j - gj.origin(gc);
            s += (double)patches[q * ldp + (di * gj.x + dj) * C + c];
            ++added;
        }
    }
    *a = s;
    if (c == 0) cnt[i * gj.L + j] += added;
}

// out = acc / cnt where a used patch covers the pixel, the input image elsewhere - and, with keep_observed, wherever the
// element was observed
template <typename T>
__global__ __launch_bounds__(256) void image_inpaint_finish_kernel(const double *__restrict__ acc,
                                                                   const int32_t *__restrict__ cnt,
                                                                   const T *__restrict__ img,
                                                                   const uint8_t *__restrict__ obs, int64_t C,
                                                                   int64_t total, int keep_observed,
                                                                   T *__restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int32_t n = cnt[e / C];
    const T v = img[e];
    out[e] = (n > 0 && !(keep_observed && obs[e] != 0)) ? (T)(acc[e] / (double)n) : v;
}

// arguments of every grid entry point: the grid itself, the channel count and a pass inside the grid
static inline bool grid_args(int64_t H, int64_t W, int64_t C, int64_t x, int64_t y, int64_t si, int64_t sj,
                             GridAxis *gi, GridAxis *gj) {
    return C > 0 && C <= kPatchMaxChannels && grid_axis(H, x, si, gi) && grid_axis(W, y, sj, gj) &&
           x * y <= INT32_MAX / C;                            // a flattened row is indexed with int
}

template <typename T>
int grid_patches_impl(hipStream_t stream, const T *img, int64_t H, int64_t W, int64_t C, int x, int y, int si, int sj,
                      int64_t row0, int64_t nrows, int with_mean, int with_std, T *out, int64_t ldo, T *mean, T *den) {
    GridAxis gi, gj;
    if (!img || !out || !mean || !den || !grid_args(H, W, C, x, y, si, sj, &gi, &gj) || row0 < 0 || nrows < 0 ||
        row0 + nrows > gi.g || ldo < (int64_t)x * y * C)
        return MODL_EINVAL;
    const int64_t n = nrows * gj.g;
    if (n == 0) return MODL_OK;
    hipLaunchKernelGGL((image_grid_patches_kernel<T>), dim3((unsigned)cdiv(n, 4)), dim3(256), 0, stream, img, C, gi, gj,
                       row0, n, with_mean, with_std, (T)sqrt((double)C), out, ldo, mean, den);
    MODL_LAUNCH_CHECK();
    return MODL_OK;
}

template <typename T>
int overlap_add_impl(hipStream_t stream, const T *patches, int64_t ldp, int64_t H, int64_t W, int64_t C, int x, int y,
                     int si, int sj, int64_t row0, int64_t nrows, double *acc) {
    GridAxis gi, gj;
    if (!patches || !acc || !grid_args(H, W, C, x, y, si, sj, &gi, &gj) || row0 < 0 || nrows < 0 ||
        row0 + nrows > gi.g || ldp < (int64_t)x * y * C)
        return MODL_EINVAL;
    if (nrows == 0) return MODL_OK;
    const int64_t i_begin = gi.origin(row0), i_end = gi.origin(row0 + nrows - 1) + x;
    const int64_t total = (i_end - i_begin) * W * C;
    hipLaunchKernelGGL((image_overlap_add_kernel<T>), dim3((unsigned)cdiv(total, 256)), dim3(256), 0, stream, patches,
                       ldp, C, gi, gj, row0, nrows, i_begin, total, acc);
    MODL_LAUNCH_CHECK();
    return MODL_OK;
}

template <typename T>
int overlap_finish_impl(hipStream_t stream, const double *acc, int64_t H, int64_t W, int64_t C, int x, int y, int si,
                        int sj, T *out) {
    GridAxis gi, gj;
    if (!acc || !out || !grid_args(H, W, C, x, y, si, sj, &gi, &gj)) return MODL_EINVAL;
    const int64_t total = H * W * C;
    hipLaunchKernelGGL((image_overlap_finish_kernel<T>), dim3((unsigned)cdiv(total, 256)), dim3(256), 0, stream, acc, C,
                       gi, gj, total, out);
    MODL_LAUNCH_CHECK();
    return MODL_OK;
}

template <typename T>
int grid_patches_masked_impl(hipStream_t stream, const T *img, const uint8_t *obs, int64_t H, int64_t W, int64_t C, int x,
                             int y, int si, int sj, int64_t row0, int64_t nrows, int with_mean, int with_std, T *out,
                             int64_t ldo, T *mean, T *den, uint8_t *obs_out, int32_t *nobs) {
    GridAxis gi, gj;
    if (!img || !obs || !out || !mean || !den || !obs_out || !nobs || !grid_args(H, W, C, x, y, si, sj, &gi, &gj) ||
        row0 < 0 || nrows < 0 || row0 + nrows > gi.g || ldo < (int64_t)x * y * C)
        return MODL_EINVAL;
    const int64_t n = nrows * gj.g;
    if (n == 0) return MODL_OK;
    hipLaunchKernelGGL((image_grid_patches_masked_kernel<T>), dim3((unsigned)cdiv(n, 4)), dim3(256), 0, stream, img, obs,
                       C, gi, gj, row0, n, with_mean, with_std, (T)sqrt((double)C), out, ldo, mean, den, obs_out, nobs);
    MODL_LAUNCH_CHECK();
    return MODL_OK;
}

template <typename T>
int patches_masked_impl(hipStream_t stream, const T *img, const uint8_t *obs, int64_t H, int64_t W, int64_t C,
                        const int64_t *idx3, int64_t n, int x, int y, int z, int with_mean, int with_std, T *out,
                        int64_t ldo, T *mean, T *den, uint8_t *obs_out, int32_t *nobs) {
    if (!img || !obs || !idx3 || !out || !mean || !den || !obs_out || !nobs || n < 0 || x <= 0 || y <= 0 || x > H ||
        y > W || C <= 0 || C > kPatchMaxChannels || z != C || (int64_t)x * y > INT32_MAX / C || ldo < (int64_t)x * y * C)
        return MODL_EINVAL;
    if (n == 0) return MODL_OK;
    hipLaunchKernelGGL((image_patches_masked_kernel<T>), dim3((unsigned)cdiv(n, 4)), dim3(256), 0, stream, img, obs, W, C,
                       idx3, n, x, y, with_mean, with_std, (T)sqrt((double)C), out, ldo, mean, den, obs_out, nobs);
    MODL_LAUNCH_CHECK();
    return MODL_OK;
}

template <typename T>
int overlap_add_weighted_impl(hipStream_t stream, const T *patches, int64_t ldp, const uint8_t *use, int64_t H, int64_t W,
                              int64_t C, int x, int y, int si, int sj, int64_t row0, int64_t nrows, double *acc,
                              int32_t *cnt) {
    GridAxis gi, gj;
    if (!patches || !use || !acc || !cnt || !grid_args(H, W, C, x, y, si, sj, &gi, &gj) || row0 < 0 || nrows < 0 ||
        row0 + nrows > gi.g || ldp < (int64_t)x * y * C)
        return MODL_EINVAL;
    if (nrows == 0) return MODL_OK;
    const int64_t i_begin = gi.origin(row0), i_end = gi.origin(row0 + nrows - 1) + x;
    const int64_t total = (i_end - i_begin) * W * C;
    hipLaunchKernelGGL((image_overlap_add_weighted_kernel<T>), dim3((unsigned)cdiv(total, 256)), dim3(256), 0, stream,
                       patches, ldp, use, C, gi, gj, row0, nrows, i_begin, total, acc, cnt);
    MODL_LAUNCH_CHECK();
    return MODL_OK;
}

template <typename T>
int inpaint_finish_impl(hipStream_t stream, const double *acc, const int32_t *cnt, const T *img, const uint8_t *obs,
                        int64_t H, int64_t W, int64_t C, int keep_observed, T *out) {
    if (!acc || !cnt || !img || !obs || !out || H <= 0 || W <= 0 || C <= 0 || C > kPatchMaxChannels) return MODL_EINVAL;
    const int64_t total = H * W * C;
    hipLaunchKernelGGL((image_inpaint_finish_kernel<T>), dim3((unsigned)cdiv(total, 256)), dim3(256), 0, stream, acc, cnt,
                       img, obs, C, total, keep_observed, out);
    MODL_LAUNCH_CHECK();
    return MODL_OK;
}

}  // namespace modl

using namespace modl;

extern "C" {

int modl_image_fill(int64_t p, int64_t q, int64_t r, int64_t *h_out) {
    if (p < 0 || q < 0 || r < 0 || (!h_out && p * q * r > 0)) return MODL_EINVAL;
    int64_t l = 0;
    for (int64_t pp = 0; pp < p; ++pp)
        for (int64_t qq = 0; qq < q; ++qq)
            for (int64_t rr = 0; rr < r; ++rr) {
                h_out[3 * l] = pp; h_out[3 * l + 1] = qq; h_out[3 * l + 2] = rr;
                ++l;
            }
    return MODL_OK;
}

}  // extern "C"

namespace {
// image_fast.pyx:36-56.  A missing pixel (value -1) at (pp, qq, rr) clears every patch origin whose window holds it.
// The third range uses the patch WIDTH y where one would expect the depth z (image_fast.pyx:46): kept, it is what the
// reference selects (no difference whenever the patch spans all channels and z <= y, the only use in the reference).
template <typename T>
int clean_mask_impl(const T *image, int64_t H, int64_t W, int64_t C, int64_t x, int64_t y, int64_t z, int64_t *out,
                    int64_t *n_out) {
    if (!image || !n_out || x <= 0 || y <= 0 || z <= 0 || x > H || y > W || z > C) return MODL_EINVAL;
    const int64_t p = H - x + 1, q = W - y + 1, r = C - z + 1;
    std::vector<unsigned char> take((size_t)(p * q * r), 1);
    for (int64_t pp = 0; pp < H; ++pp)
        for (int64_t qq = 0; qq < W; ++qq)
            for (int64_t rr = 0; rr < C; ++rr) {
                if (image[(pp * W + qq) * C + rr] != (T)-1) continue;
                const int64_t x0 = std::max<int64_t>(0, pp - x + 1), x1 = std::min<int64_t>(p, pp + 1);
                const int64_t y0 = std::max<int64_t>(0, qq - y + 1), y1 = std::min<int64_t>(q, qq + 1);
                const int64_t z0 = std::max<int64_t>(0, rr - y + 1), z1 = std::min<int64_t>(r, rr + 1);
                for (int64_t xx = x0; xx < x1; ++xx)
                    for (int64_t yy = y0; yy < y1; ++yy)
                        for (int64_t zz = z0; zz < z1; ++zz) take[(size_t)((xx * q + yy) * r + zz)] = 0;
            }
    int64_t l = 0;
    for (int64_t pp = 0; pp < p; ++pp)
        for (int64_t qq = 0; qq < q; ++qq)
            for (int64_t rr = 0; rr < r; ++rr)
                if (take[(size_t)((pp * q + qq) * r + rr)]) {
                    if (out) { out[3 * l] = pp; out[3 * l + 1] = qq; out[3 * l + 2] = rr; }
                    ++l;
                }
    *n_out = l;
    return MODL_OK;
}
}  // namespace

extern "C" {

int modl_image_clean_mask_f32(const float *h_image, int64_t H, int64_t W, int64_t C, int64_t x, int64_t y, int64_t z,
                              int64_t *h_out, int64_t *n_out) {
    return clean_mask_impl<float>(h_image, H, W, C, x, y, z, h_out, n_out);
}
int modl_image_clean_mask_f64(const double *h_image, int64_t H, int64_t W, int64_t C, int64_t x, int64_t y, int64_t z,
                              int64_t *h_out, int64_t *n_out) {
    return clean_mask_impl<double>(h_image, H, W, C, x, y, z, h_out, n_out);
}

#define MODL_PATCH_ARGS_OK                                                                                          \
    (d_image && d_idx3 && d_out && n >= 0 && x > 0 && y > 0 && z > 0 && x <= H && y <= W && z <= C &&              \
     z <= kPatchMaxChannels && ldo >= (int64_t)x * y * z)

int modl_image_patches_f32(const float *d_image, int64_t H, int64_t W, int64_t C, const int64_t *d_idx3, int64_t n, int x,
                           int y, int z, int with_mean, int with_std, float *d_out, int64_t ldo, void *stream) {
    if (!MODL_PATCH_ARGS_OK) return MODL_EINVAL;
    return launch_image_patches<float>((hipStream_t)stream, d_image, H, W, C, d_idx3, n, x, y, z, with_mean, with_std, d_out, ldo);
}
int modl_image_patches_f64(const double *d_image, int64_t H, int64_t W, int64_t C, const int64_t *d_idx3, int64_t n, int x,
                           int y, int z, int with_mean, int with_std, double *d_out, int64_t ldo, void *stream) {
    if (!MODL_PATCH_ARGS_OK) return MODL_EINVAL;
    return launch_image_patches<double>((hipStream_t)stream, d_image, H, W, C, d_idx3, n, x, y, z, with_mean, with_std, d_out, ldo);
}

int modl_image_grid_shape(int64_t H, int64_t W, int64_t x, int64_t y, int64_t si, int64_t sj, int64_t *grid_rows,
                          int64_t *grid_cols) {
    GridAxis gi, gj;
    if (!grid_rows || !grid_cols || !grid_axis(H, x, si, &gi) || !grid_axis(W, y, sj, &gj)) return MODL_EINVAL;
    *grid_rows = gi.g; *grid_cols = gj.g;
    return MODL_OK;
}

#define MODL_GRID_EXPORTS(SFX, T)                                                                                     \
    int modl_image_grid_patches_##SFX(const T *d_image, int64_t H, int64_t W, int64_t C, int x, int y, int si, int sj, \
                                      int64_t row0, int64_t nrows, int with_mean, int with_std, T *d_out, int64_t ldo, \
                                      T *d_mean, T *d_den, void *stream) {                                            \
        return grid_patches_impl<T>((hipStream_t)stream, d_image, H, W, C, x, y, si, sj, row0, nrows, with_mean,      \
                                    with_std, d_out, ldo, d_mean, d_den);                                             \
    }                                                                                                                 \
    int modl_image_decode_##SFX(const T *d_code, int64_t n, int k, const T *d_Dt, int64_t P, int C, const T *d_mean,  \
                                const T *d_den, T *d_out, int64_t ldo, void *stream) {                                \
        if (!d_code || !d_Dt || !d_out || n < 0 || k <= 0 || P <= 0 || P > INT32_MAX || ldo < P ||                   \
            (d_mean == nullptr) != (d_den == nullptr) || (d_mean && (C <= 0 || P % C != 0)))                         \
            return MODL_EINVAL;                                                                                       \
        return decode_impl<T>((hipStream_t)stream, d_code, n, k, d_Dt, P, C, d_mean, d_den, d_out, ldo);              \
    }                                                                                                                 \
    int modl_image_overlap_add_##SFX(const T *d_patches, int64_t ldp, int64_t H, int64_t W, int64_t C, int x, int y,  \
                                     int si, int sj, int64_t row0, int64_t nrows, double *d_acc, void *stream) {      \
        return overlap_add_impl<T>((hipStream_t)stream, d_patches, ldp, H, W, C, x, y, si, sj, row0, nrows, d_acc);   \
    }                                                                                                                 \
    int modl_image_overlap_finish_##SFX(const double *d_acc, int64_t H, int64_t W, int64_t C, int x, int y, int si,   \
                                        int sj, T *d_image_out, void *stream) {                                       \
        return overlap_finish_impl<T>((hipStream_t)stream, d_acc, H, W, C, x, y, si, sj, d_image_out);                \
    }                                                                                                                 \
    int modl_image_grid_patches_masked_##SFX(const T *d_image, int64_t H, int64_t W, int64_t C, int x, int y, int si,  \
                                             int sj, int64_t row0, int64_t nrows, int with_mean, int with_std,        \
                                             T *d_out, int64_t ldo, T *d_mean, T *d_den,                              \
                                             const uint8_t *d_obs_image, uint8_t *d_obs_out, int32_t *d_nobs,         \
                                             void *stream) {                                                          \
        return grid_patches_masked_impl<T>((hipStream_t)stream, d_image, d_obs_image, H, W, C, x, y, si, sj, row0,    \
                                           nrows, with_mean, with_std, d_out, ldo, d_mean, d_den, d_obs_out, d_nobs); \
    }                                                                                                                 \
    int modl_image_patches_masked_##SFX(const T *d_image, int64_t H, int64_t W, int64_t C, const int64_t *d_idx3,     \
                                        int64_t n, int x, int y, int z, int with_mean, int with_std, T *d_out,        \
                                        int64_t ldo, T *d_mean, T *d_den, const uint8_t *d_obs_image,                 \
                                        uint8_t *d_obs_out, int32_t *d_nobs, void *stream) {                          \
        return patches_masked_impl<T>((hipStream_t)stream, d_image, d_obs_image, H, W, C, d_idx3, n, x, y, z,         \
                                      with_mean, with_std, d_out, ldo, d_mean, d_den, d_obs_out, d_nobs);             \
    }                                                                                                                 \
    int modl_image_overlap_add_weighted_##SFX(const T *d_patches, int64_t ldp, int64_t H, int64_t W, int64_t C, int x, \
                                              int y, int si, int sj, int64_t row0, int64_t nrows, double *d_acc,      \
                                              const uint8_t *d_use, int32_t *d_cnt, void *stream) {                   \
        return overlap_add_weighted_impl<T>((hipStream_t)stream, d_patches, ldp, d_use, H, W, C, x, y, si, sj, row0,  \
                                            nrows, d_acc, d_cnt);                                                     \
    }                                                                                                                 \
    int modl_image_inpaint_finish_##SFX(const double *d_acc, const int32_t *d_cnt, const T *d_image,                  \
                                        const uint8_t *d_obs_image, int64_t H, int64_t W, int64_t C,                  \
                                        int keep_observed, T *d_image_out, void *stream) {                            \
        return inpaint_finish_impl<T>((hipStream_t)stream, d_acc, d_cnt, d_image, d_obs_image, H, W, C,               \
                                      keep_observed, d_image_out);                                                    \
    }
MODL_GRID_EXPORTS(f32, float)
MODL_GRID_EXPORTS(f64, double)

size_t modl_objective_workspace(int dtype, int64_t n, int64_t p) {
    const size_t e = dtype == MODL_F32 ? 4 : 8;
    int64_t rows = n < 1 ? 1 : n;
    if (rows > 8192) rows = 8192;
    return sizeof(double) * kObjBlocks + e * (size_t)p * (size_t)rows;
}
int modl_objective_f32(const float *d_X, int64_t ldx, int64_t n, int64_t p, const float *d_Dt, int k, const float *d_code,
                       void *d_ws, size_t ws_bytes, double *d_out3, void *stream) {
    if (!d_X || !d_Dt || !d_code || !d_ws || !d_out3 || n < 0 || p <= 0 || k <= 0 || ldx < p) return MODL_EINVAL;
    return objective_impl<float>((hipStream_t)stream, d_X, ldx, n, p, d_Dt, k, d_code, d_ws, ws_bytes, d_out3);
}
int modl_objective_f64(const double *d_X, int64_t ldx, int64_t n, int64_t p, const double *d_Dt, int k, const double *d_code,
                       void *d_ws, size_t ws_bytes, double *d_out3, void *stream) {
    if (!d_X || !d_Dt || !d_code || !d_ws || !d_out3 || n < 0 || p <= 0 || k <= 0 || ldx < p) return MODL_EINVAL;
    return objective_impl<double>((hipStream_t)stream, d_X, ldx, n, p, d_Dt, k, d_code, d_ws, ws_bytes, d_out3);
}

}  // extern "C"
