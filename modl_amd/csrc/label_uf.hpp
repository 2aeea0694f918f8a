// Union-find labelling of 6-connected components, shared by compute_mask.hip (one binary box) and regions.hip (many maps at
// once): int32 parents indexed by the flat memory index g = (i0 n1 + i1) n2 + i2 of a box [n0][n1][n2], with the invariant
// parent[g] <= g, so every chain descends and is shorter than the box; the root of a component is its smallest g.
#pragma once
#include <climits>

#include "common.hpp"

namespace modl {

constexpr int kLT0 = 8, kLT1 = 8, kLT2 = 8;                 // the tile labelled in LDS, along n0, n1, n2
constexpr int kMaxTilesPerAxis = 65535;                     // grid.y / grid.z
constexpr int kLabelThreads = 512;                          // one thread per voxel of a tile

static inline bool mask_box_ok(int64_t n0, int64_t n1, int64_t n2) {
    return n0 >= 1 && n1 >= 1 && n2 >= 1 && n0 <= INT32_MAX / n1 && n0 * n1 <= INT32_MAX / n2;
}

static inline bool overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

template <int SCOPE> __device__ __forceinline__ int uf_load(int *P, int x) {
    return __hip_atomic_load(P + x, __ATOMIC_RELAXED, SCOPE);
}

// the root of x with path halving; every store is an atomic min of an ancestor, so parent[x] <= x holds throughout and x
// descends strictly: at most `limit` (the number of elements) steps
template <int SCOPE> __device__ __forceinline__ int uf_find(int *P, int x, int limit) {
    for (int it = 0; it < limit; ++it) {
        const int p = uf_load<SCOPE>(P, x);
        if (p == x) return x;
        const int gp = uf_load<SCOPE>(P, p);
        if (gp == p) return p;
        __hip_atomic_fetch_min(P + x, gp, __ATOMIC_RELAXED, SCOPE);
        x = gp;
    }
    return x;
}

// unite the sets of a and b: the larger root is linked under the smaller by an atomic min; when the min displaces another
// link the loop goes on with the displaced value, so no union is lost.  One of a, b descends every round.
template <int SCOPE> __device__ __forceinline__ void uf_union(int *P, int a, int b, int limit) {
    for (int64_t it = 0; it < 2 * (int64_t)limit; ++it) {
        a = uf_find<SCOPE>(P, a, limit);
        b = uf_find<SCOPE>(P, b, limit);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = __hip_atomic_fetch_min(P + a, b, __ATOMIC_RELAXED, SCOPE);      // a > b
        if (old == a) return;
        a = old;
    }
}

struct LabelGeom {
    int n[3];
};

// One workgroup of kLabelThreads threads labels its tile in L (kLT0 kLT1 kLT2 ints of LDS): thread l owns the voxel
// (l / (kLT2 kLT1), (l / kLT2) % kLT1, l % kLT2) of the tile, `on` says whether it is foreground.  Returns the smallest l of
// the voxel's component WITHIN the tile, -1 for a background voxel.  Every thread of the workgroup calls it.
__device__ __forceinline__ int uf_label_tile(int *L, int l, bool on) {
    constexpr int T0 = kLT0, T1 = kLT1, T2 = kLT2;
    constexpr int WG = __HIP_MEMORY_SCOPE_WORKGROUP;
    const int c = l % T2, b = (l / T2) % T1, a = l / (T2 * T1);
    L[l] = on ? l : -1;
    __syncthreads();
    if (on) {
        if (c > 0 && uf_load<WG>(L, l - 1) >= 0) uf_union<WG>(L, l, l - 1, T0 * T1 * T2);
        if (b > 0 && uf_load<WG>(L, l - T2) >= 0) uf_union<WG>(L, l, l - T2, T0 * T1 * T2);
        if (a > 0 && uf_load<WG>(L, l - T2 * T1) >= 0) uf_union<WG>(L, l, l - T2 * T1, T0 * T1 * T2);
    }
    __syncthreads();
    return on ? uf_find<WG>(L, l, T0 * T1 * T2) : -1;
}

// a true voxel g on the low face of a tile unites with its true neighbour across the face; `parent` holds -1 for a false
// voxel.  All reads of `parent` are agent-scope relaxed atomic loads or the return value of an atomic, every write is an
// atomicMin; no workgroup waits for another.
__device__ __forceinline__ void uf_merge_faces(int *parent, int g, const LabelGeom &geom, bool lo2, bool lo1, bool lo0) {
    constexpr int AG = __HIP_MEMORY_SCOPE_AGENT;
    const int box = geom.n[0] * geom.n[1] * geom.n[2], s1 = geom.n[2], s0 = geom.n[1] * geom.n[2];
    if (lo2) uf_union<AG>(parent, g, g - 1, box);
    if (lo1) uf_union<AG>(parent, g, g - s1, box);
    if (lo0) uf_union<AG>(parent, g, g - s0, box);
}

__device__ __forceinline__ int wave_min_int(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ int wave_max_int(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}

}  // namespace modl
