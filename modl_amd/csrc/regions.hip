// Connected regions of many maps at once: the device half of nilearn's connected_regions /
// RegionExtractor.  The maps are rows (M, V) over the V voxels of a mask; `col` [n0][n1][n2] (n2 fastest: the frame order
// (Z, Y, X) of masker.hip) holds the column of every box voxel or -1.  An element v is foreground iff it is finite, v != 0
// and |v| >= cutoff; the foreground of one map is split into its 6-connected components in the box, components of at most
// `min_voxels` voxels are dropped, and the kept ones are numbered 1, 2, .. per map in scipy.ndimage.label's order: by the
// component's first voxel in the C order of the caller's (X, Y, Z) = (n2, n1, n0) array, u = (i2 n1 + i1) n0 + i0.
//
// One set of launches labels a chunk of M maps, the map on the last grid axis; every array of the workspace is [M][box]:
//   1. region_tile_kernel     the predicate straight from rows[m][col[g]] (no volume, no byte mask), then the union-find of
//                             label_uf.hpp on a tile in LDS: parent[g] = the smallest g of the component WITHIN the tile, -1
//                             for background; cnt = 0, first = INT_MAX at the roots of the tile;
//   2. region_merge_kernel    unions across the low faces of the tiles (a voxel is foreground iff parent[g] >= 0);
//   3. region_flatten_kernel  root[g] = the smallest g of the component; `parent` is dead from here and is zeroed to serve as
//                             the flags of step 5;
//   4. region_count_kernel    cnt[root] += the voxels, first[root] = min u: one integer add and one integer min per
//                             wavefront and distinct root;
//   5. region_mark_kernel     flag[first[r]] = 1 for every root r with cnt[r] > min_voxels: the flags are indexed in USER
//                             order, so that
//   6. region_scan_tile_kernel / region_scan_sums_kernel   their inclusive prefix sum (tiles of kScanTile elements in place,
//                             then the exclusive scan of the tile sums by one workgroup per map) is the region number:
//                             number = scan[first] + sums[first / kScanTile]; the last value is the map's count;
//   7. region_write_kernel    labels[m][col[g]] = the number of g's component or 0, sizes[m][number - 1] = cnt.
// All atomics are integer min / add, so the same input gives the same bits.  The gather (region_gather_kernel) then writes
// one row per region: the map's elements where labels == number, 0 elsewhere.
#include <algorithm>
#include <cmath>

#include "label_uf.hpp"

namespace modl {

constexpr int kScanTile = 1024;                             // elements one workgroup scans: 256 threads x 4
constexpr int64_t kMaxMaps = 65535;                         // grid.z of the tile kernel, grid.y of the others
constexpr int64_t kGatherRows = 65535;                      // region rows per launch of the gather (grid.y)

static inline bool region_box_ok(int64_t n0, int64_t n1, int64_t n2) {
    return mask_box_ok(n0, n1, n2) && n0 <= (int64_t)kLT0 * kMaxTilesPerAxis;
}

template <typename T> __device__ __forceinline__ bool region_foreground(T v, T cutoff) {
    const T a = std::fabs(v);
    return a < (T)__builtin_inf() && v != (T)0 && a >= cutoff;             // (NaN fails the first compare)
}

struct RegionWs {
    int *parent, *root, *cnt, *first, *sums;                // parent doubles as the flags / their scan after step 3
};

static inline size_t region_slot(int64_t M, int64_t box) { return align_up((size_t)M * (size_t)box * sizeof(int), 256); }
static inline int64_t region_scan_tiles(int64_t box) { return cdiv(box, kScanTile); }
static inline size_t region_ws_bytes(int64_t M, int64_t box) {
    return 4 * region_slot(M, box) + align_up((size_t)M * (size_t)region_scan_tiles(box) * sizeof(int), 256);
}

// 1.  grid (tiles along n1 x tiles along n2, tiles along n0, M)
template <typename T>
__global__ __launch_bounds__(kLabelThreads) void region_tile_kernel(const T *__restrict__ rows, int64_t ldr, int V,
                                                                    const int *__restrict__ col, LabelGeom g, int tiles2, T cutoff,
                                                                    RegionWs ws) {
    constexpr int T0 = kLT0, T1 = kLT1, T2 = kLT2;
    __shared__ int L[T0 * T1 * T2];
    const int l = threadIdx.x;
    const int c = l % T2, b = (l / T2) % T1, a = l / (T2 * T1);
    const int t2 = blockIdx.x % tiles2, t1 = blockIdx.x / tiles2;
    const int i0 = blockIdx.y * T0 + a, i1 = t1 * T1 + b, i2 = t2 * T2 + c;
    const bool inside = i0 < g.n[0] && i1 < g.n[1] && i2 < g.n[2];
    const int64_t gi = ((int64_t)i0 * g.n[1] + i1) * g.n[2] + i2;
    const int64_t box = (int64_t)g.n[0] * g.n[1] * g.n[2], at = (int64_t)blockIdx.z * box + gi;
    bool on = false;
    if (inside) {
        const int cv = col[gi];
        if (cv >= 0 && cv < V) on = region_foreground(rows[(int64_t)blockIdx.z * ldr + cv], cutoff);
    }
    const int r = uf_label_tile(L, l, on);
    if (!inside) return;
    if (!on) {
        ws.parent[at] = -1;
        return;
    }
    const int rc = r % T2, rb = (r / T2) % T1, ra = r / (T2 * T1);
    ws.parent[at] = (int)(((int64_t)(blockIdx.y * T0 + ra) * g.n[1] + (t1 * T1 + rb)) * g.n[2] + (t2 * T2 + rc));
    if (r == l) {                                           // cnt and first are only ever looked at where a component has its
        ws.cnt[at] = 0;                                     // root, and the root of a component is the root of its part of a tile
        ws.first[at] = INT_MAX;
    }
}

// 2.  grid (ceil(box / 256), M) here and below
__global__ __launch_bounds__(256) void region_merge_kernel(LabelGeom g, int *parent) {
    constexpr int AG = __HIP_MEMORY_SCOPE_AGENT;
    const int box = g.n[0] * g.n[1] * g.n[2];
    const int64_t gi = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gi >= box) return;
    int *P = parent + (int64_t)blockIdx.y * box;
    const int i2 = (int)(gi % g.n[2]), i1 = (int)((gi / g.n[2]) % g.n[1]), i0 = (int)(gi / ((int64_t)g.n[2] * g.n[1]));
    const bool f2 = i2 > 0 && i2 % kLT2 == 0, f1 = i1 > 0 && i1 % kLT1 == 0, f0 = i0 > 0 && i0 % kLT0 == 0;
    if (!(f2 || f1 || f0) || uf_load<AG>(P, (int)gi) < 0) return;
    const int s1 = g.n[2], s0 = g.n[1] * g.n[2];
    uf_merge_faces(P, (int)gi, g, f2 && uf_load<AG>(P, (int)gi - 1) >= 0, f1 && uf_load<AG>(P, (int)gi - s1) >= 0,
                   f0 && uf_load<AG>(P, (int)gi - s0) >= 0);
}

// 3.
__global__ __launch_bounds__(256) void region_flatten_kernel(int *parent, int box, int *__restrict__ root) {
    constexpr int AG = __HIP_MEMORY_SCOPE_AGENT;
    const int64_t gi = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gi >= box) return;
    int *P = parent + (int64_t)blockIdx.y * box;
    root[(int64_t)blockIdx.y * box + gi] = uf_load<AG>(P, (int)gi) < 0 ? -1 : uf_find<AG>(P, (int)gi, box);
}

// 4.  a ballot loop over the roots present in the wavefront, at most 64 rounds
__global__ __launch_bounds__(256) void region_count_kernel(const int *__restrict__ root, LabelGeom g, int *cnt, int *first) {
    const int box = g.n[0] * g.n[1] * g.n[2];
    const int64_t gi = (int64_t)blockIdx.x * 256 + threadIdx.x, base = (int64_t)blockIdx.y * box;
    const int lane = threadIdx.x & 63;
    const int r = gi < box ? root[base + gi] : -1;
    int u = INT_MAX;
    if (r >= 0) {
        const int i2 = (int)(gi % g.n[2]), i1 = (int)((gi / g.n[2]) % g.n[1]), i0 = (int)(gi / ((int64_t)g.n[2] * g.n[1]));
        u = (i2 * g.n[1] + i1) * g.n[0] + i0;
    }
    bool todo = r >= 0;
    for (int it = 0; it < kWave; ++it) {
        const unsigned long long m = __ballot(todo);
        if (m == 0) break;
        const int leader = __ffsll((long long)m) - 1;
        const int r0 = __shfl(r, leader);
        const bool mine = todo && r == r0;
        const unsigned long long same = __ballot(mine);
        const int u0 = wave_min_int(mine ? u : INT_MAX);
        if (lane == leader) {
            atomicAdd(cnt + base + r0, __popcll(same));
            atomicMin(first + base + r0, u0);
        }
        if (mine) todo = false;
    }
}

// 5.
__global__ __launch_bounds__(256) void region_mark_kernel(const int *__restrict__ root, const int *__restrict__ cnt,
                                                          const int *__restrict__ first, int box, int min_voxels,
                                                          int *__restrict__ flag) {
    const int64_t gi = (int64_t)blockIdx.x * 256 + threadIdx.x, base = (int64_t)blockIdx.y * box;
    if (gi >= box || root[base + gi] != (int)gi || cnt[base + gi] <= min_voxels) return;
    const int f = first[base + gi];
    if (f >= 0 && f < box) flag[base + f] = 1;
}

__device__ __forceinline__ int wave_scan_int(int v, int lane) {                // inclusive
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const int t = __shfl_up(v, o);
        if (lane >= o) v += t;
    }
    return v;
}

// 6a.  grid (tiles, M): the inclusive scan of a tile in place, the tile's sum apart
__global__ __launch_bounds__(256) void region_scan_tile_kernel(int *flag, int box, int tiles, int *__restrict__ sums) {
    __shared__ int wsum[4];
    int *f = flag + (int64_t)blockIdx.y * box;
    const int64_t at = (int64_t)blockIdx.x * kScanTile + threadIdx.x * 4;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = at + j < box ? f[at + j] : 0;
    v[1] += v[0];
    v[2] += v[1];
    v[3] += v[2];
    const int s = wave_scan_int(v[3], lane);
    if (lane == 63) wsum[w] = s;
    __syncthreads();
    int off = s - v[3];
    for (int i = 0; i < w; ++i) off += wsum[i];
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (at + j < box) f[at + j] = v[j] + off;
    if (threadIdx.x == 255) sums[(int64_t)blockIdx.y * tiles + blockIdx.x] = off + v[3];
}

// 6b.  grid (M): the exclusive scan of a map's tile sums in place; counts[m] = their total
__global__ __launch_bounds__(256) void region_scan_sums_kernel(int *sums, int tiles, int *__restrict__ counts) {
    __shared__ int wsum[4];
    int *b = sums + (int64_t)blockIdx.x * tiles;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int carry = 0;
    for (int at = 0; at < tiles; at += 256) {
        const int i = at + threadIdx.x;
        const int x = i < tiles ? b[i] : 0;
        const int s = wave_scan_int(x, lane);
        if (lane == 63) wsum[w] = s;
        __syncthreads();
        int off = carry;
        for (int j = 0; j < w; ++j) off += wsum[j];
        if (i < tiles) b[i] = off + s - x;
        carry += wsum[0] + wsum[1] + wsum[2] + wsum[3];
        __syncthreads();
    }
    if (threadIdx.x == 0) counts[blockIdx.x] = carry;
}

// 7.
__global__ __launch_bounds__(256) void region_write_kernel(const int *__restrict__ col, int V, RegionWs ws, int box, int tiles,
                                                           int min_voxels, int *__restrict__ labels, int64_t ldl, int *__restrict__ sizes,
                                                           int64_t size_cap) {
    const int64_t gi = (int64_t)blockIdx.x * 256 + threadIdx.x, base = (int64_t)blockIdx.y * box;
    if (gi >= box) return;
    const int cv = col[gi];
    if (cv < 0 || cv >= V) return;
    const int r = ws.root[base + gi];
    int number = 0;
    if (r >= 0) {
        const int n = ws.cnt[base + r];
        if (n > min_voxels) {
            const int f = ws.first[base + r];
            if (f >= 0 && f < box) number = ws.parent[base + f] + ws.sums[(int64_t)blockIdx.y * tiles + f / kScanTile];
            if (r == (int)gi && number >= 1 && number <= size_cap) sizes[(int64_t)blockIdx.y * size_cap + number - 1] = n;
        }
    }
    labels[(int64_t)blockIdx.y * ldl + cv] = number;
}

// One region row per grid row: VEC neighbouring columns per thread (16 bytes of the dtype), the vector types declared with
// the alignment of an ELEMENT since a row starts anywhere; only the last, partial group goes element by element.  The map's
// element is loaded only where the label matches.
template <typename T, int VEC>
__global__ __launch_bounds__(256) void region_gather_kernel(const T *__restrict__ rows, int64_t ldr, int64_t M, int64_t V,
                                                            const int *__restrict__ labels, int64_t ldl,
                                                            const int64_t *__restrict__ offsets, int64_t row0, T *__restrict__ out,
                                                            int64_t ldo) {
    typedef T VecT __attribute__((ext_vector_type(VEC), aligned(sizeof(T))));
    typedef int VecI __attribute__((ext_vector_type(VEC), aligned(sizeof(int))));
    const int64_t r = row0 + blockIdx.y;
    int64_t lo = 0, hi = M;                                 // the map m with offsets[m] <= r < offsets[m + 1]
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) / 2;
        if (offsets[mid] <= r) lo = mid; else hi = mid;
    }
    const int number = (int)(r - offsets[lo]) + 1;
    const int64_t c0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * VEC;
    if (c0 >= V) return;
    const int *lab = labels + lo * ldl + c0;
    const T *src = rows + lo * ldr + c0;
    T *dst = out + r * ldo + c0;
    if (c0 + VEC <= V) {
        const VecI lv = *reinterpret_cast<const VecI *>(lab);
        VecT o;
#pragma unroll
        for (int j = 0; j < VEC; ++j) o[j] = lv[j] == number ? src[j] : (T)0;
        *reinterpret_cast<VecT *>(dst) = o;
    } else {
        for (int j = 0; c0 + j < V; ++j) dst[j] = lab[j] == number ? src[j] : (T)0;
    }
}

template <typename T>
static int region_labels_abi(const T *rows, int64_t ldr, int64_t M, int64_t V, const int32_t *col, int64_t n0, int64_t n1, int64_t n2,
                             T cutoff, int64_t min_voxels, int32_t *labels, int64_t ldl, int32_t *counts, int32_t *sizes,
                             int64_t size_cap, void *d_ws, size_t ws_bytes, void *stream_) {
    if (!rows || !col || !labels || !counts || !region_box_ok(n0, n1, n2) || M < 1 || M > kMaxMaps) return MODL_EINVAL;
    const int64_t box = n0 * n1 * n2;
    if (V < 1 || V > box || ldr < V || ldl < V || ldr > INT64_MAX / 8 / M || ldl > INT64_MAX / 8 / M) return MODL_EINVAL;
    if (!(cutoff >= (T)0) || size_cap < 0 || size_cap > INT64_MAX / 8 / M || (size_cap > 0 && !sizes)) return MODL_EINVAL;
    const size_t rows_b = (size_t)((M - 1) * ldr + V) * sizeof(T), lab_b = (size_t)((M - 1) * ldl + V) * 4, col_b = (size_t)box * 4;
    const size_t cnt_b = (size_t)M * 4, siz_b = (size_t)M * (size_t)size_cap * 4;
    const size_t need = region_ws_bytes(M, box);
    if (overlap(rows, rows_b, labels, lab_b) || overlap(col, col_b, labels, lab_b) || overlap(counts, cnt_b, labels, lab_b) ||
        overlap(rows, rows_b, counts, cnt_b) || overlap(col, col_b, counts, cnt_b))
        return MODL_EINVAL;
    if (size_cap > 0 && (overlap(sizes, siz_b, labels, lab_b) || overlap(sizes, siz_b, counts, cnt_b) ||
                         overlap(sizes, siz_b, rows, rows_b) || overlap(sizes, siz_b, col, col_b)))
        return MODL_EINVAL;
    if (!d_ws || ws_bytes < need) return MODL_ENOMEM;
    if (overlap(d_ws, need, rows, rows_b) || overlap(d_ws, need, col, col_b) || overlap(d_ws, need, labels, lab_b) ||
        overlap(d_ws, need, counts, cnt_b) || (size_cap > 0 && overlap(d_ws, need, sizes, siz_b)))
        return MODL_EINVAL;
    if (modl_device_count() <= 0) return MODL_ENOGPU;
    hipStream_t stream = (hipStream_t)stream_;
    const LabelGeom g = {{(int)n0, (int)n1, (int)n2}};
    const size_t slot = region_slot(M, box);
    char *w = (char *)d_ws;
    const RegionWs ws = {(int *)w, (int *)(w + slot), (int *)(w + 2 * slot), (int *)(w + 3 * slot), (int *)(w + 4 * slot)};
    const int minv = (int)std::max<int64_t>(-1, std::min<int64_t>(min_voxels, INT32_MAX));
    const int tiles2 = (int)cdiv(n2, kLT2), scan_tiles = (int)region_scan_tiles(box);
    const dim3 tiles((unsigned)(cdiv(n1, kLT1) * tiles2), (unsigned)cdiv(n0, kLT0), (unsigned)M);
    const dim3 flat((unsigned)cdiv(box, 256), (unsigned)M);
    hipLaunchKernelGGL((region_tile_kernel<T>), tiles, dim3(kLabelThreads), 0, stream, rows, ldr, (int)V, col, g, tiles2, cutoff, ws);
    MODL_LAUNCH_CHECK();
    hipLaunchKernelGGL(region_merge_kernel, flat, dim3(256), 0, stream, g, ws.parent);
    MODL_LAUNCH_CHECK();
    hipLaunchKernelGGL(region_flatten_kernel, flat, dim3(256), 0, stream, ws.parent, (int)box, ws.root);
    MODL_LAUNCH_CHECK();
    MODL_HIP(hipMemsetAsync(ws.parent, 0, (size_t)M * (size_t)box * sizeof(int), stream));
    hipLaunchKernelGGL(region_count_kernel, flat, dim3(256), 0, stream, ws.root, g, ws.cnt, ws.first);
    MODL_LAUNCH_CHECK();
    hipLaunchKernelGGL(region_mark_kernel, flat, dim3(256), 0, stream, ws.root, ws.cnt, ws.first, (int)box, minv, ws.parent);
    MODL_LAUNCH_CHECK();
    hipLaunchKernelGGL(region_scan_tile_kernel, dim3((unsigned)scan_tiles, (unsigned)M), dim3(256), 0, stream, ws.parent, (int)box,
                       scan_tiles, ws.sums);
    MODL_LAUNCH_CHECK();
    hipLaunchKernelGGL(region_scan_sums_kernel, dim3((unsigned)M), dim3(256), 0, stream, ws.sums, scan_tiles, counts);
    MODL_LAUNCH_CHECK();
    hipLaunchKernelGGL(region_write_kernel, flat, dim3(256), 0, stream, col, (int)V, ws, (int)box, scan_tiles, minv, labels, ldl,
                       sizes, size_cap);
    MODL_LAUNCH_CHECK();
    return MODL_OK;
}

template <typename T>
static int region_gather_abi(const T *rows, int64_t ldr, int64_t M, int64_t V, const int32_t *labels, int64_t ldl,
                             const int64_t *offsets, int64_t R, T *out, int64_t ldo, void *stream_) {
    constexpr int VEC = 16 / sizeof(T);
    if (!rows || !labels || !offsets || M < 1 || V < 1 || R < 0 || ldr < V || ldl < V || ldo < V) return MODL_EINVAL;
    if (ldr > INT64_MAX / 8 / M || ldl > INT64_MAX / 8 / M || V > INT32_MAX) return MODL_EINVAL;
    if (R == 0) return MODL_OK;
    if (!out || ldo > INT64_MAX / 8 / R) return MODL_EINVAL;
    const size_t rows_b = (size_t)((M - 1) * ldr + V) * sizeof(T), lab_b = (size_t)((M - 1) * ldl + V) * 4;
    const size_t out_b = (size_t)((R - 1) * ldo + V) * sizeof(T), off_b = (size_t)(M + 1) * 8;
    if ((uintptr_t)rows % sizeof(T) != 0 || (uintptr_t)out % sizeof(T) != 0 || (uintptr_t)labels % 4 != 0 || (uintptr_t)offsets % 8 != 0)
        return MODL_EINVAL;
    if (overlap(out, out_b, rows, rows_b) || overlap(out, out_b, labels, lab_b) || overlap(out, out_b, offsets, off_b)) return MODL_EINVAL;
    if (modl_device_count() <= 0) return MODL_ENOGPU;
    for (int64_t row0 = 0; row0 < R; row0 += kGatherRows) {
        const dim3 grid((unsigned)cdiv(cdiv(V, VEC), 256), (unsigned)std::min(kGatherRows, R - row0));
        hipLaunchKernelGGL((region_gather_kernel<T, VEC>), grid, dim3(256), 0, (hipStream_t)stream_, rows, ldr, M, V, labels, ldl,
                           offsets, row0, out, ldo);
        MODL_LAUNCH_CHECK();
    }
    return MODL_OK;
}

}  // namespace modl

using namespace modl;

extern "C" {

size_t modl_region_labels_workspace(int64_t M, int64_t n0, int64_t n1, int64_t n2) {
    if (!region_box_ok(n0, n1, n2) || M < 1 || M > kMaxMaps) return 0;
    return region_ws_bytes(M, n0 * n1 * n2);
}

int64_t modl_region_max_maps(int64_t n0, int64_t n1, int64_t n2, size_t budget_bytes) {
    if (!region_box_ok(n0, n1, n2)) return 0;
    const int64_t box = n0 * n1 * n2;
    int64_t lo = 0, hi = kMaxMaps + 1;                      // the workspace grows with M: the largest M within the budget
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) / 2;
        if (region_ws_bytes(mid, box) <= budget_bytes) lo = mid; else hi = mid;
    }
    return lo;
}

int modl_region_labels_f32(const float *d_rows, int64_t ldr, int64_t M, int64_t V, const int32_t *d_col, int64_t n0, int64_t n1,
                           int64_t n2, float cutoff, int64_t min_voxels, int32_t *d_labels, int64_t ldl, int32_t *d_counts,
                           int32_t *d_sizes, int64_t size_cap, void *d_ws, size_t ws_bytes, void *stream) {
    return region_labels_abi<float>(d_rows, ldr, M, V, d_col, n0, n1, n2, cutoff, min_voxels, d_labels, ldl, d_counts, d_sizes,
                                    size_cap, d_ws, ws_bytes, stream);
}

int modl_region_labels_f64(const double *d_rows, int64_t ldr, int64_t M, int64_t V, const int32_t *d_col, int64_t n0, int64_t n1,
                           int64_t n2, double cutoff, int64_t min_voxels, int32_t *d_labels, int64_t ldl, int32_t *d_counts,
                           int32_t *d_sizes, int64_t size_cap, void *d_ws, size_t ws_bytes, void *stream) {
    return region_labels_abi<double>(d_rows, ldr, M, V, d_col, n0, n1, n2, cutoff, min_voxels, d_labels, ldl, d_counts, d_sizes,
                                     size_cap, d_ws, ws_bytes, stream);
}

int modl_region_gather_f32(const float *d_rows, int64_t ldr, int64_t M, int64_t V, const int32_t *d_labels, int64_t ldl,
                           const int64_t *d_offsets, int64_t R, float *d_regions, int64_t ldo, void *stream) {
    return region_gather_abi<float>(d_rows, ldr, M, V, d_labels, ldl, d_offsets, R, d_regions, ldo, stream);
}

int modl_region_gather_f64(const double *d_rows, int64_t ldr, int64_t M, int64_t V, const int32_t *d_labels, int64_t ldl,
                           const int64_t *d_offsets, int64_t R, double *d_regions, int64_t ldo, void *stream) {
    return region_gather_abi<double>(d_rows, ldr, M, V, d_labels, ldl, d_offsets, R, d_regions, ldo, stream);
}

}  // extern "C"
