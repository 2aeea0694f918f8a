// Sparse codes as CSR (no counterpart in the reference): compaction of a dense chunk of codes into
// (indptr int64, indices int32, data T) on the device, and the product of CSR codes with the dictionary.
//
//   count  csr_count_kernel (one wavefront per row: 64 columns per step, __ballot + popcount) writes every row's count,
//          csr_tile_sum_kernel / csr_scan_sums_kernel / csr_tile_scan_kernel turn the counts into indptr: tiles of 1024
//          rows are summed, ONE workgroup scans the tile sums (256 at a time, with a carry), every tile is scanned again
//          from its offset.  No atomics: indptr is a pure function of the chunk.
//   fill   csr_fill_kernel (one wavefront per row): a kept element's slot is the row's start plus the number of kept
//          lanes below it (v_mbcnt on the ballot), so the entries come out in ascending column order.
//   decode csr_decode_kernel: a wavefront per (row, tile of 256 features); the row's entries are loaded 64 at a time and
//          handed round by v_readlane, every lane keeps four features.  The dictionary is read atom-major (a transposed
//          copy made once per call), so that an atom's features are contiguous.  Every (row, feature) sum is one fma
//          chain over the row's entries in stored order: a row decodes to the same bits wherever it stands.
//
// An element is kept iff (bits & ~sign) != 0, which is `value != 0` (scipy's csr_matrix(dense) rule: NaN, +-inf and
// denormals kept, -0.0 dropped) decided on the integer bits, so the floating-point mode's treatment of denormals cannot
// change the answer.  Values are moved as integers, bit for bit.
#include <algorithm>

#include "common.hpp"

namespace modl {

constexpr int kCsrWaves = 4;                     // rows (decode: row tiles) per workgroup, one wavefront each
constexpr int kCsrSteps = 4;                     // steps of 64 columns a wavefront loads before it counts them
constexpr int kCsrScanTile = 1024;               // rows per workgroup of the scan (256 threads x 4)
constexpr int64_t kCsrMaxGrid = (int64_t)1 << 20;   // workgroups of a launch; the kernels stride over what is beyond
constexpr int kDecodeFeat = 4;                   // features per lane of the decode: a wavefront covers 256

template <typename T> struct CsrBits;
template <> struct CsrBits<float> { using U = uint32_t; };
template <> struct CsrBits<double> { using U = uint64_t; };
template <typename U> __device__ __forceinline__ bool csr_keep(U bits) { return (U)(bits << 1) != 0; }   // drops the sign

// number of set bits of m below this lane
__device__ __forceinline__ int lanes_below(uint64_t m) {
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// inclusive prefix sum over the 256 threads of a workgroup (thread order); total = the sum of all.  red: 4 words of LDS
__device__ __forceinline__ int64_t block_scan_incl(int64_t v, int64_t *red, int64_t &total) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    for (int d = 1; d < 64; d <<= 1) {
        const int64_t u = __shfl_up(v, d);
        if (lane >= d) v += u;
    }
    __syncthreads();                             // (red may still be read by the previous call)
    if (lane == 63) red[wid] = v;
    __syncthreads();
    int64_t off = 0;
    total = 0;
    for (int w = 0; w < 4; ++w) {
        if (w < wid) off += red[w];
        total += red[w];
    }
    return v + off;
}

// counts[r] = number of kept elements of row r (counts = indptr + 1)
template <typename U>
__global__ __launch_bounds__(64 * kCsrWaves) void csr_count_kernel(const U *code, int64_t ld, int64_t b, int64_t k,
                                                                    int64_t *counts) {
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int64_t r = (int64_t)blockIdx.x * kCsrWaves + wid; r < b; r += (int64_t)gridDim.x * kCsrWaves) {
        const U *row = code + r * ld;
        int64_t n = 0;
        for (int64_t c0 = lane; c0 < k + lane; c0 += 64 * kCsrSteps) {      // (four loads in flight per lane)
            U v[kCsrSteps];
#pragma unroll
            for (int u = 0; u < kCsrSteps; ++u) v[u] = c0 + 64 * u < k ? row[c0 + 64 * u] : (U)0;
#pragma unroll
            for (int u = 0; u < kCsrSteps; ++u) n += __popcll(__ballot(csr_keep(v[u])));
        }
        if (lane == 0) counts[r] = n;
    }
}

__global__ __launch_bounds__(256) void csr_tile_sum_kernel(const int64_t *counts, int64_t b, int64_t *tile_sum) {
    __shared__ int64_t red[4];
    const int64_t i0 = (int64_t)blockIdx.x * kCsrScanTile + 4 * (int64_t)threadIdx.x;
    int64_t s = 0, total;
    for (int u = 0; u < 4; ++u)
        if (i0 + u < b) s += counts[i0 + u];
    block_scan_incl(s, red, total);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

// tile_sum[t] <- sum of the tiles before t, in place; one workgroup, 256 tiles per round with a carry
__global__ __launch_bounds__(256) void csr_scan_sums_kernel(int64_t *tile_sum, int64_t tiles) {
    __shared__ int64_t red[4];
    int64_t carry = 0;
    for (int64_t t0 = 0; t0 < tiles; t0 += 256) {
        const int64_t t = t0 + threadIdx.x;
        const int64_t v = t < tiles ? tile_sum[t] : 0;
        int64_t total;
        const int64_t incl = block_scan_incl(v, red, total);
        if (t < tiles) tile_sum[t] = carry + incl - v;
        carry += total;
    }
}

// indptr[0] = base, indptr[i + 1] = base + counts[0] + ... + counts[i], in place (counts = indptr + 1)
__global__ __launch_bounds__(256) void csr_tile_scan_kernel(int64_t *indptr, int64_t b, int64_t base,
                                                           const int64_t *tile_off) {
    __shared__ int64_t red[4];
    int64_t *counts = indptr + 1;
    const int64_t i0 = (int64_t)blockIdx.x * kCsrScanTile + 4 * (int64_t)threadIdx.x;
    int64_t c[4], s = 0, total;
    for (int u = 0; u < 4; ++u) {
        c[u] = i0 + u < b ? counts[i0 + u] : 0;
        s += c[u];
    }
    int64_t run = base + tile_off[blockIdx.x] + block_scan_incl(s, red, total) - s;
    for (int u = 0; u < 4; ++u) {
        run += c[u];
        if (i0 + u < b) counts[i0 + u] = run;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) indptr[0] = base;
}

// row r's kept elements, in ascending column order, to the slots indptr[r] - base ...; slots outside [0, nnz) are skipped
// (they cannot occur with the indptr the count made of the same chunk)
template <typename U>
__global__ __launch_bounds__(64 * kCsrWaves) void csr_fill_kernel(const U *code, int64_t ld, int64_t b, int64_t k,
                                                                   int64_t base, const int64_t *indptr, int64_t nnz,
                                                                   int32_t *indices, U *data) {
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int64_t r = (int64_t)blockIdx.x * kCsrWaves + wid; r < b; r += (int64_t)gridDim.x * kCsrWaves) {
        const U *row = code + r * ld;
        int64_t pos = indptr[r] - base;
        for (int64_t c0 = lane; c0 < k + lane; c0 += 64 * kCsrSteps) {
            U v[kCsrSteps];
#pragma unroll
            for (int u = 0; u < kCsrSteps; ++u) v[u] = c0 + 64 * u < k ? row[c0 + 64 * u] : (U)0;
#pragma unroll
            for (int u = 0; u < kCsrSteps; ++u) {
                const bool keep = csr_keep(v[u]);
                const uint64_t m = __ballot(keep);
                const int64_t slot = pos + lanes_below(m);
                if (keep && slot >= 0 && slot < nnz) {
                    indices[slot] = (int32_t)(c0 + 64 * u);
                    data[slot] = v[u];
                }
                pos += __popcll(m);
            }
        }
    }
}

// out[i][e] = sum over row i's entries j, in stored order, of data[j] * D[indices[j]][e]   (D atom-major, [k][p])
template <typename T>
__global__ __launch_bounds__(64 * kCsrWaves) void csr_decode_kernel(const int64_t *indptr, const int32_t *indices,
                                                                     const T *data, int64_t nnz, int64_t n, int64_t k,
                                                                     const T *D, int64_t p, int64_t tiles, T *out,
                                                                     int64_t ldo, int32_t *status) {
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t items = n * tiles;
    for (int64_t w = (int64_t)blockIdx.x * kCsrWaves + wid; w < items; w += (int64_t)gridDim.x * kCsrWaves) {
        const int64_t i = w / tiles, t = w - i * tiles;
        const int64_t e0 = t * (64 * kDecodeFeat) + lane;
        int64_t lo = indptr[i], hi = indptr[i + 1];
        bool bad = lo < 0 || hi < lo || hi > nnz;          // a corrupt row contributes nothing
        if (bad) lo = hi = 0;
        T acc[kDecodeFeat];
#pragma unroll
        for (int u = 0; u < kDecodeFeat; ++u) acc[u] = (T)0;
        for (int64_t j0 = lo; j0 < hi; j0 += 64) {
            const int64_t j = j0 + lane;
            int idx = -1;
            T val = (T)0;
            if (j < hi) {
                idx = indices[j];
                val = data[j];
                if (idx < 0 || (int64_t)idx >= k) {         // an index outside the dictionary contributes nothing
                    idx = -1;
                    bad = true;
                }
            }
            const int cnt = hi - j0 < 64 ? (int)(hi - j0) : 64;
            for (int jj = 0; jj < cnt; ++jj) {
                const int a = bcast_lane(idx, jj);
                if (a < 0) continue;
                const T v = bcast_lane(val, jj);
                const T *atom = D + (int64_t)a * p;
#pragma unroll
                for (int u = 0; u < kDecodeFeat; ++u) {
                    const int64_t e = e0 + 64 * u;
                    if (e < p) acc[u] = __builtin_fma(v, atom[e], acc[u]);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kDecodeFeat; ++u) {
            const int64_t e = e0 + 64 * u;
            if (e < p) out[i * ldo + e] = acc[u];
        }
        if (bad && status) *status = 1;
    }
}

static inline unsigned csr_grid(int64_t items) { return (unsigned)std::min(cdiv(items, kCsrWaves), kCsrMaxGrid); }

static bool compact_args_ok(const void *code, int64_t ld, int64_t b, int64_t k, int64_t base, const void *indptr) {
    return code && indptr && b >= 0 && b <= INT32_MAX && k >= 1 && k <= INT32_MAX && ld >= k && base >= 0 &&
           (b == 0 || ld <= INT64_MAX / b);
}

template <typename T>
static int csr_count_abi(const T *code, int64_t ld, int64_t b, int64_t k, int64_t base, int64_t *indptr, void *ws,
                         size_t ws_bytes, void *stream_) {
    using U = typename CsrBits<T>::U;
    if (!compact_args_ok(code, ld, b, k, base, indptr)) return MODL_EINVAL;
    if (b == 0) return MODL_OK;
    if (!ws || ws_bytes < modl_csr_compact_workspace(b)) return MODL_ENOMEM;
    if (modl_device_count() <= 0) return MODL_ENOGPU;
    hipStream_t stream = (hipStream_t)stream_;
    int64_t *tile_off = (int64_t *)ws;
    const int64_t tiles = cdiv(b, kCsrScanTile);
    hipLaunchKernelGGL((csr_count_kernel<U>), dim3(csr_grid(b)), dim3(64 * kCsrWaves), 0, stream, (const U *)code, ld, b,
                       k, indptr + 1);
    MODL_LAUNCH_CHECK();
    hipLaunchKernelGGL(csr_tile_sum_kernel, dim3((unsigned)tiles), dim3(256), 0, stream, indptr + 1, b, tile_off);
    MODL_LAUNCH_CHECK();
    hipLaunchKernelGGL(csr_scan_sums_kernel, dim3(1), dim3(256), 0, stream, tile_off, tiles);
    MODL_LAUNCH_CHECK();
    hipLaunchKernelGGL(csr_tile_scan_kernel, dim3((unsigned)tiles), dim3(256), 0, stream, indptr, b, base, tile_off);
    MODL_LAUNCH_CHECK();
    return MODL_OK;
}

template <typename T>
static int csr_fill_abi(const T *code, int64_t ld, int64_t b, int64_t k, int64_t base, const int64_t *indptr, int64_t nnz,
                        int32_t *indices, T *data, void *stream) {
    using U = typename CsrBits<T>::U;
    if (!compact_args_ok(code, ld, b, k, base, indptr) || !indices || !data || nnz < 0) return MODL_EINVAL;
    if (b == 0 || nnz == 0) return MODL_OK;
    if (modl_device_count() <= 0) return MODL_ENOGPU;
    hipLaunchKernelGGL((csr_fill_kernel<U>), dim3(csr_grid(b)), dim3(64 * kCsrWaves), 0, (hipStream_t)stream,
                       (const U *)code, ld, b, k, base, indptr, nnz, indices, (U *)data);
    MODL_LAUNCH_CHECK();
    return MODL_OK;
}

// the transpose's grid has one row of workgroups per 32 features
constexpr int64_t kDecodeMaxP = (int64_t)32 * 65535;

template <typename T>
static int csr_decode_abi(const int64_t *indptr, const int32_t *indices, const T *data, int64_t nnz, int64_t n, int64_t k,
                          const T *Dt, int64_t p, T *out, int64_t ldo, int32_t *status, void *ws, size_t ws_bytes,
                          void *stream_) {
    if (!indptr || !indices || !data || !Dt || !out || nnz < 0 || n < 0 || k < 1 || k > INT32_MAX || p < 1 ||
        p > kDecodeMaxP || ldo < p || k > INT64_MAX / (int64_t)sizeof(T) / p || (n > 0 && ldo > INT64_MAX / n))
        return MODL_EINVAL;
    const int64_t tiles = cdiv(p, 64 * kDecodeFeat);
    if (n > INT64_MAX / tiles) return MODL_EINVAL;
    if (n == 0) return MODL_OK;
    if (!ws || ws_bytes < modl_csr_decode_workspace(DType<T>::id, k, p)) return MODL_ENOMEM;
    if (modl_device_count() <= 0) return MODL_ENOGPU;
    hipStream_t stream = (hipStream_t)stream_;
    if (status) MODL_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), stream));
    T *D = (T *)ws;                                          // [k][p]: an atom's features side by side
    if (DType<T>::id == MODL_F32) MODL_TRY(modl_transpose_f32((const float *)Dt, (float *)D, p, k, stream_));
    else MODL_TRY(modl_transpose_f64((const double *)Dt, (double *)D, p, k, stream_));
    hipLaunchKernelGGL((csr_decode_kernel<T>), dim3(csr_grid(n * tiles)), dim3(64 * kCsrWaves), 0, stream, indptr, indices,
                       data, nnz, n, k, D, p, tiles, out, ldo, status);
    MODL_LAUNCH_CHECK();
    return MODL_OK;
}

}  // namespace modl

using namespace modl;

extern "C" {

size_t modl_csr_compact_workspace(int64_t b) {
    return b < 0 ? 0 : (size_t)std::max<int64_t>(cdiv(b, kCsrScanTile), 1) * sizeof(int64_t);
}

size_t modl_csr_decode_workspace(int dtype, int64_t k, int64_t p) {
    const int64_t es = dtype == MODL_F32 ? 4 : dtype == MODL_F64 ? 8 : 0;
    if (es == 0 || k < 1 || p < 1 || k > INT64_MAX / es / p) return 0;
    return (size_t)(k * p * es);
}

#define ABI_CSR(SFX, T)                                                                                                   \
    int modl_csr_count_##SFX(const T *d_code, int64_t ld, int64_t b, int64_t k, int64_t base, int64_t *d_indptr,         \
                             void *d_ws, size_t ws_bytes, void *stream) {                                                 \
        return csr_count_abi<T>(d_code, ld, b, k, base, d_indptr, d_ws, ws_bytes, stream);                                \
    }                                                                                                                     \
    int modl_csr_fill_##SFX(const T *d_code, int64_t ld, int64_t b, int64_t k, int64_t base, const int64_t *d_indptr,    \
                            int64_t nnz, int32_t *d_indices, T *d_data, void *stream) {                                   \
        return csr_fill_abi<T>(d_code, ld, b, k, base, d_indptr, nnz, d_indices, d_data, stream);                         \
    }                                                                                                                     \
    int modl_csr_decode_##SFX(const int64_t *d_indptr, const int32_t *d_indices, const T *d_data, int64_t nnz, int64_t n, \
                              int64_t k, const T *d_Dt, int64_t p, T *d_out, int64_t ldo, int32_t *d_status, void *d_ws,  \
                              size_t ws_bytes, void *stream) {                                                            \
        return csr_decode_abi<T>(d_indptr, d_indices, d_data, nnz, n, k, d_Dt, p, d_out, ldo, d_status, d_ws, ws_bytes,   \
                                 stream);                                                                                 \
    }
ABI_CSR(f32, float)
ABI_CSR(f64, double)
#undef ABI_CSR

}  // extern "C"
