// Computing an fMRI mask on the device: the temporal mean of a record, binary erosion / dilation with
// the cross structure, 6-connected component labelling and the largest component - the steps of nilearn's
// compute_epi_mask / compute_background_mask that touch every voxel.  Masks are uint8 (0 / nonzero) boxes [n0][n1][n2],
// n2 fastest: the frame order (Z, Y, X) of masker.hip.
//
// Labelling is union-find over int32 parents indexed by the flat memory index g = (i0 n1 + i1) n2 + i2, with the invariant
// parent[g] <= g, so every chain descends and is shorter than the box:
//   1. label_tile_kernel   one workgroup labels a tile of kLT0 x kLT1 x kLT2 voxels in LDS and writes parent[g] = the smallest g of
//                          the voxel's component WITHIN the tile;
//   2. label_merge_kernel  every true voxel on the low face of a tile unites with its true neighbour across the face.  All
//                          reads of `parent` are agent-scope relaxed atomic loads or the return value of an atomic, every
//                          write is an atomicMin; no workgroup waits for another;
//   3. label_flatten_kernel root[g] = the root of g's chain = the smallest g of the component, -1 for a false voxel.
// The kernel boundaries are the phase boundaries.  The representative depends on the mask alone.
#include <cmath>

#include "label_uf.hpp"

namespace modl {

constexpr size_t kLabelScalars = 256;                       // bytes: {largest size, components, winner's first user index}

// ------------------------------------------------------------------------------------------------------ the mean
template <typename T> __device__ __forceinline__ T finite_or_zero(T v) { return std::fabs(v) < (T)__builtin_inf() ? v : (T)0; }

// One thread owns VEC neighbouring voxels (8 bytes: two f32, one f64) and walks the frames in ascending t with f64
// accumulators: the order of the sum is t = 0, 1, .., T-1 whatever the launch geometry.  A full group is one 8-byte load per
// frame, 512 contiguous bytes per wavefront; the vector type is declared with the alignment of an ELEMENT, since a frame
// of an odd box starts anywhere.  Measured on a 91 x 109 x 91 x 300 record: 8 and 16 bytes per lane
// run at the same rate in f32, 16 bytes per lane on rows that are not 16-byte multiples cost f64 a fifth, and
// per-element loads for every group run at 0.4 of the rate in f32.  Only the last, partial group loads element by element.
template <typename T, int VEC>
__global__ __launch_bounds__(256) void frame_mean_kernel(const T *__restrict__ frames, int64_t ld, int64_t n_frames, int64_t n,
                                                         int zero_nonfinite, T *__restrict__ mean) {
    typedef T Vec __attribute__((ext_vector_type(VEC), aligned(sizeof(T))));
    const int64_t v0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * VEC;
    if (v0 >= n) return;
    double acc[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) acc[j] = 0.0;
    if (v0 + VEC <= n) {
        const T *p = frames + v0;
#pragma unroll 8
        for (int64_t t = 0; t < n_frames; ++t) {
            const Vec x = *reinterpret_cast<const Vec *>(p + t * ld);
#pragma unroll
            for (int j = 0; j < VEC; ++j) acc[j] += (double)x[j];
        }
    } else {
        for (int64_t t = 0; t < n_frames; ++t) {
#pragma unroll
            for (int j = 0; j < VEC; ++j)
                if (v0 + j < n) acc[j] += (double)frames[t * ld + v0 + j];
        }
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        if (v0 + j >= n) break;
        T r = (T)(acc[j] / (double)n_frames);
        if (zero_nonfinite) r = finite_or_zero(r);
        mean[v0 + j] = r;
    }
}

template <typename T>
static int frame_mean_abi(const T *frames, int64_t ld, int64_t n_frames, int64_t n, int zero_nonfinite, T *mean, void *stream_) {
    constexpr int VEC = 8 / sizeof(T);
    if (!frames || !mean || n_frames < 1 || n < 1 || ld < n || ld > INT64_MAX / 8 / n_frames || n > (int64_t)INT32_MAX * 256)
        return MODL_EINVAL;
    if (zero_nonfinite != 0 && zero_nonfinite != 1) return MODL_EINVAL;
    if ((uintptr_t)frames % sizeof(T) != 0 || (uintptr_t)mean % sizeof(T) != 0) return MODL_EINVAL;
    if (overlap(frames, (size_t)((n_frames - 1) * ld + n) * sizeof(T), mean, (size_t)n * sizeof(T))) return MODL_EINVAL;
    if (modl_device_count() <= 0) return MODL_ENOGPU;
    hipLaunchKernelGGL((frame_mean_kernel<T, VEC>), dim3((unsigned)cdiv(cdiv(n, VEC), 256)), dim3(256), 0, (hipStream_t)stream_,
                       frames, ld, n_frames, n, zero_nonfinite, mean);
    MODL_LAUNCH_CHECK();
    return MODL_OK;
}

// ------------------------------------------------------------------------------------------------ erosion, dilation
// one iteration with the cross structure, border value 0: a voxel survives erosion iff it and its six neighbours are inside
// the box and true; it is set by dilation iff it or one of its neighbours inside the box is true
__global__ __launch_bounds__(256) void morph_kernel(const uint8_t *__restrict__ in, int n0, int n1, int n2, int dilate,
                                                    uint8_t *__restrict__ out) {
    const int64_t box = (int64_t)n0 * n1 * n2;
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= box) return;
    const int i2 = (int)(g % n2), i1 = (int)((g / n2) % n1), i0 = (int)(g / ((int64_t)n2 * n1));
    const int64_t s1 = n2, s0 = (int64_t)n1 * n2;
    const bool lo2 = i2 > 0, hi2 = i2 + 1 < n2, lo1 = i1 > 0, hi1 = i1 + 1 < n1, lo0 = i0 > 0, hi0 = i0 + 1 < n0;
    bool r = in[g] != 0;
    if (dilate) {
        r = r || (lo2 && in[g - 1]) || (hi2 && in[g + 1]) || (lo1 && in[g - s1]) || (hi1 && in[g + s1]) ||
            (lo0 && in[g - s0]) || (hi0 && in[g + s0]);
    } else {
        r = r && lo2 && hi2 && lo1 && hi1 && lo0 && hi0;
        r = r && in[g - 1] && in[g + 1] && in[g - s1] && in[g + s1] && in[g - s0] && in[g + s0];
    }
    out[g] = r ? 1 : 0;
}

// n iterations equal one pass with the L1 ball of radius n.  Erosion leaves nothing once n >= (shortest axis + 1) / 2 (no
// locus is that far from the outside), dilation changes nothing past the L1 diameter: more iterations are not launched.
static inline int64_t morph_launches(int64_t n0, int64_t n1, int64_t n2, int64_t iterations, int dilate) {
    const int64_t cap = dilate ? n0 + n1 + n2 : (std::min(n0, std::min(n1, n2)) + 1) / 2;
    return std::min(iterations, cap);
}

// ------------------------------------------------------------------------------------------------------ labelling
// phase 1.  cnt / scal (may be NULL): the counters of modl_largest_component, reset here.
__global__ __launch_bounds__(kLabelThreads) void label_tile_kernel(const uint8_t *__restrict__ mask, LabelGeom g,
                                                                   int *__restrict__ parent, int *__restrict__ cnt,
                                                                   int *__restrict__ scal) {
    constexpr int T0 = kLT0, T1 = kLT1, T2 = kLT2;
    __shared__ int L[T0 * T1 * T2];
    const int l = threadIdx.x;
    const int c = l % T2, b = (l / T2) % T1, a = l / (T2 * T1);
    const int i0 = blockIdx.z * T0 + a, i1 = blockIdx.y * T1 + b, i2 = blockIdx.x * T2 + c;
    const bool inside = i0 < g.n[0] && i1 < g.n[1] && i2 < g.n[2];
    const int64_t gi = ((int64_t)i0 * g.n[1] + i1) * g.n[2] + i2;
    const bool on = inside && mask[gi] != 0;
    if (scal && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && l < 3) scal[l] = l == 2 ? INT_MAX : 0;
    const int r = uf_label_tile(L, l, on);
    if (!inside) return;
    if (cnt) cnt[gi] = 0;
    if (!on) {
        parent[gi] = -1;
        return;
    }
    const int rc = r % T2, rb = (r / T2) % T1, ra = r / (T2 * T1);
    parent[gi] = (int)(((int64_t)(blockIdx.z * T0 + ra) * g.n[1] + (blockIdx.y * T1 + rb)) * g.n[2] + (blockIdx.x * T2 + rc));
}

// phase 2
__global__ __launch_bounds__(256) void label_merge_kernel(const uint8_t *__restrict__ mask, LabelGeom g, int *parent) {
    const int box = g.n[0] * g.n[1] * g.n[2];
    const int64_t gi = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gi >= box || mask[gi] == 0) return;
    const int i2 = (int)(gi % g.n[2]), i1 = (int)((gi / g.n[2]) % g.n[1]), i0 = (int)(gi / ((int64_t)g.n[2] * g.n[1]));
    const int s1 = g.n[2], s0 = g.n[1] * g.n[2];
    uf_merge_faces(parent, (int)gi, g, i2 > 0 && i2 % kLT2 == 0 && mask[gi - 1], i1 > 0 && i1 % kLT1 == 0 && mask[gi - s1],
                   i0 > 0 && i0 % kLT0 == 0 && mask[gi - s0]);
}

// phase 3: the chains are walked (and halved on the way, for the threads that follow) and the root is written apart
__global__ __launch_bounds__(256) void label_flatten_kernel(int *parent, int box, int *__restrict__ root) {
    const int64_t gi = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gi >= box) return;
    constexpr int AG = __HIP_MEMORY_SCOPE_AGENT;
    root[gi] = uf_load<AG>(parent, (int)gi) < 0 ? -1 : uf_find<AG>(parent, (int)gi, box);
}

// sizes: one add per wavefront and distinct root (a ballot loop over the roots present in the wavefront, at most 64 rounds)
__global__ __launch_bounds__(256) void label_count_kernel(const int *__restrict__ root, int box, int *cnt) {
    const int64_t gi = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int r = gi < box ? root[gi] : -1;
    bool todo = r >= 0;
    for (int it = 0; it < kWave; ++it) {
        const unsigned long long m = __ballot(todo);
        if (m == 0) break;
        const int leader = __ffsll((long long)m) - 1;
        const int r0 = __shfl(r, leader);
        const unsigned long long same = __ballot(todo && r == r0);
        if (lane == leader) atomicAdd(cnt + r0, __popcll(same));
        if (r == r0) todo = false;
    }
}

// scal[0] = the largest size, scal[1] = the number of components (integer max / add: the order does not matter)
__global__ __launch_bounds__(256) void label_max_kernel(const int *__restrict__ root, const int *__restrict__ cnt, int box,
                                                        int *scal) {
    const int64_t gi = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool is_root = gi < box && root[gi] == (int)gi;
    const int m = wave_max_int(is_root ? cnt[gi] : 0);
    const unsigned long long roots = __ballot(is_root);
    if ((threadIdx.x & 63) == 0 && roots) {
        atomicMax(scal + 0, m);
        atomicAdd(scal + 1, __popcll(roots));
    }
}

// scal[2] = the smallest USER index (x (n1 n0) + y n0 + z, the C index of the (X, Y, Z) = (n2, n1, n0) array) among the
// voxels of the components of the largest size: the tie rule of the contract
__global__ __launch_bounds__(256) void label_first_kernel(const int *__restrict__ root, const int *__restrict__ cnt, LabelGeom g,
                                                          int *scal) {
    const int box = g.n[0] * g.n[1] * g.n[2];
    const int64_t gi = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int u = INT_MAX;
    if (gi < box) {
        const int r = root[gi];
        if (r >= 0 && cnt[r] == scal[0]) {
            const int i2 = (int)(gi % g.n[2]), i1 = (int)((gi / g.n[2]) % g.n[1]), i0 = (int)(gi / ((int64_t)g.n[2] * g.n[1]));
            u = (i2 * g.n[1] + i1) * g.n[0] + i0;
        }
    }
    u = wave_min_int(u);
    if ((threadIdx.x & 63) == 0 && u != INT_MAX) atomicMin(scal + 2, u);
}

__global__ __launch_bounds__(256) void label_pick_kernel(const int *__restrict__ root, LabelGeom g, const int *__restrict__ scal,
                                                         uint8_t *__restrict__ out, int64_t *__restrict__ info) {
    const int box = g.n[0] * g.n[1] * g.n[2];
    const int64_t gi = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gi >= box) return;
    const int first = scal[2];
    const bool any = first != INT_MAX;
    int winner = -2;
    if (any) {
        const int i0 = first % g.n[0], i1 = (first / g.n[0]) % g.n[1], i2 = first / (g.n[0] * g.n[1]);
        winner = root[((int64_t)i0 * g.n[1] + i1) * g.n[2] + i2];
    }
    out[gi] = root[gi] == winner ? 1 : 0;
    if (gi == 0) {
        info[0] = any ? scal[1] : 0;
        info[1] = any ? scal[0] : 0;
        info[2] = any ? first : 0;
    }
}

static inline bool label_box_ok(int64_t n0, int64_t n1, int64_t n2) {
    return mask_box_ok(n0, n1, n2) && n0 <= (int64_t)kLT0 * kMaxTilesPerAxis && n1 <= (int64_t)kLT1 * kMaxTilesPerAxis;
}

static inline size_t label_slot(int64_t box) { return align_up((size_t)box * sizeof(int), 256); }

static int label_launch(const uint8_t *mask, const LabelGeom &g, int *parent, int *root, int *cnt, int *scal, hipStream_t stream) {
    const int box = g.n[0] * g.n[1] * g.n[2];
    const dim3 tiles((unsigned)cdiv(g.n[2], kLT2), (unsigned)cdiv(g.n[1], kLT1), (unsigned)cdiv(g.n[0], kLT0));
    const dim3 flat((unsigned)cdiv(box, 256));
    hipLaunchKernelGGL(label_tile_kernel, tiles, dim3(kLabelThreads), 0, stream, mask, g, parent, cnt, scal);
    MODL_LAUNCH_CHECK();
    hipLaunchKernelGGL(label_merge_kernel, flat, dim3(256), 0, stream, mask, g, parent);
    MODL_LAUNCH_CHECK();
    hipLaunchKernelGGL(label_flatten_kernel, flat, dim3(256), 0, stream, parent, box, root);
    MODL_LAUNCH_CHECK();
    return MODL_OK;
}

}  // namespace modl

using namespace modl;

extern "C" {

int modl_frame_mean_f32(const float *d_frames, int64_t ld_frame, int64_t T, int64_t n, int zero_nonfinite, float *d_mean,
                        void *stream) {
    return frame_mean_abi<float>(d_frames, ld_frame, T, n, zero_nonfinite, d_mean, stream);
}

int modl_frame_mean_f64(const double *d_frames, int64_t ld_frame, int64_t T, int64_t n, int zero_nonfinite, double *d_mean,
                        void *stream) {
    return frame_mean_abi<double>(d_frames, ld_frame, T, n, zero_nonfinite, d_mean, stream);
}

size_t modl_morph_workspace(int64_t n0, int64_t n1, int64_t n2, int64_t iterations) {
    if (!mask_box_ok(n0, n1, n2) || iterations < 1) return 0;
    return align_up((size_t)(n0 * n1 * n2), 256);
}

int modl_binary_morph(const uint8_t *d_in, int64_t n0, int64_t n1, int64_t n2, int64_t iterations, int dilate, uint8_t *d_out,
                      void *d_ws, size_t ws_bytes, void *stream_) {
    if (!d_in || !d_out || !mask_box_ok(n0, n1, n2) || iterations < 1 || (dilate != 0 && dilate != 1)) return MODL_EINVAL;
    const size_t box = (size_t)(n0 * n1 * n2);
    if (overlap(d_in, box, d_out, box)) return MODL_EINVAL;
    const size_t need = modl_morph_workspace(n0, n1, n2, iterations);
    if (!d_ws || ws_bytes < need) return MODL_ENOMEM;
    if (overlap(d_in, box, d_ws, need) || overlap(d_out, box, d_ws, need)) return MODL_EINVAL;
    if (modl_device_count() <= 0) return MODL_ENOGPU;
    hipStream_t stream = (hipStream_t)stream_;
    const int64_t launches = morph_launches(n0, n1, n2, iterations, dilate);
    const uint8_t *src = d_in;
    for (int64_t s = 1; s <= launches; ++s) {               // the last launch writes d_out, the ones before alternate
        uint8_t *dst = (launches - s) % 2 == 0 ? d_out : (uint8_t *)d_ws;
        hipLaunchKernelGGL(morph_kernel, dim3((unsigned)cdiv((int64_t)box, 256)), dim3(256), 0, stream, src, (int)n0, (int)n1,
                           (int)n2, dilate, dst);
        MODL_LAUNCH_CHECK();
        src = dst;
    }
    return MODL_OK;
}

int modl_label_tile(int *tile) {
    if (!tile) return MODL_EINVAL;
    tile[0] = kLT0;
    tile[1] = kLT1;
    tile[2] = kLT2;
    return MODL_OK;
}

size_t modl_label_workspace(int64_t n0, int64_t n1, int64_t n2) {
    if (!label_box_ok(n0, n1, n2)) return 0;
    return 3 * label_slot(n0 * n1 * n2) + kLabelScalars;
}

int modl_label_components(const uint8_t *d_mask, int64_t n0, int64_t n1, int64_t n2, int32_t *d_root, void *d_ws, size_t ws_bytes,
                          void *stream) {
    if (!d_mask || !d_root || !label_box_ok(n0, n1, n2)) return MODL_EINVAL;
    const size_t box = (size_t)(n0 * n1 * n2);
    const size_t need = modl_label_workspace(n0, n1, n2);
    if (!d_ws || ws_bytes < need) return MODL_ENOMEM;
    if (overlap(d_mask, box, d_root, box * 4) || overlap(d_mask, box, d_ws, need) || overlap(d_root, box * 4, d_ws, need))
        return MODL_EINVAL;
    if (modl_device_count() <= 0) return MODL_ENOGPU;
    const LabelGeom g = {{(int)n0, (int)n1, (int)n2}};
    return label_launch(d_mask, g, (int *)d_ws, d_root, nullptr, nullptr, (hipStream_t)stream);
}

int modl_largest_component(const uint8_t *d_mask, int64_t n0, int64_t n1, int64_t n2, uint8_t *d_out, int64_t *d_info, void *d_ws,
                           size_t ws_bytes, void *stream_) {
    if (!d_mask || !d_out || !d_info || !label_box_ok(n0, n1, n2)) return MODL_EINVAL;
    const size_t box = (size_t)(n0 * n1 * n2);
    if (overlap(d_mask, box, d_out, box)) return MODL_EINVAL;
    const size_t need = modl_label_workspace(n0, n1, n2);
    if (!d_ws || ws_bytes < need) return MODL_ENOMEM;
    if (overlap(d_mask, box, d_ws, need) || overlap(d_out, box, d_ws, need) || overlap(d_info, 24, d_ws, need) ||
        overlap(d_info, 24, d_out, box) || overlap(d_info, 24, d_mask, box))
        return MODL_EINVAL;
    if (modl_device_count() <= 0) return MODL_ENOGPU;
    hipStream_t stream = (hipStream_t)stream_;
    const LabelGeom g = {{(int)n0, (int)n1, (int)n2}};
    const size_t slot = label_slot((int64_t)box);
    int *parent = (int *)d_ws, *root = (int *)((char *)d_ws + slot), *cnt = (int *)((char *)d_ws + 2 * slot);
    int *scal = (int *)((char *)d_ws + 3 * slot);
    MODL_TRY(label_launch(d_mask, g, parent, root, cnt, scal, stream));
    const dim3 flat((unsigned)cdiv((int64_t)box, 256));
    hipLaunchKernelGGL(label_count_kernel, flat, dim3(256), 0, stream, root, (int)box, cnt);
    MODL_LAUNCH_CHECK();
    hipLaunchKernelGGL(label_max_kernel, flat, dim3(256), 0, stream, root, cnt, (int)box, scal);
    MODL_LAUNCH_CHECK();
    hipLaunchKernelGGL(label_first_kernel, flat, dim3(256), 0, stream, root, cnt, g, scal);
    MODL_LAUNCH_CHECK();
    hipLaunchKernelGGL(label_pick_kernel, flat, dim3(256), 0, stream, root, g, scal, d_out, d_info);
    MODL_LAUNCH_CHECK();
    return MODL_OK;
}

}  // extern "C"
