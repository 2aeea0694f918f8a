// Elastic-net code solver for wide dictionaries, 1024 < k <= MODL_MAX_COMPONENTS: the cyclic coordinate descent of
// enet_coordinate_descent_gram (reference: modl/decomposition/dict_fact_fast.pyx:270-427) with one workgroup per sample.
//
// The solvers of cd_solver.hip / cd_split_impl.hpp keep a sample's coefficients in the registers of one or a few
// wavefronts and stop at 1024.  Here the four k-vectors w, H = Q w, q = Dx and diag(Q) live in LDS (4 k elements:
// 128 KiB in f64 at k = 4096, within the 160 KiB of a gfx950 compute unit) and a Gram row streams from global memory
// only when its coordinate actually moves.  Thread t owns the coordinates t, t + 256, ...: it alone writes their
// slots of H and w, so the search for the next coordinate to move reads only its own slots.
//
// Reference semantics, as in cd_solver.hip: sweep order 0..k-1; a zero diagonal skips the coordinate (:357, its
// coefficient keeps its value and does not count in d_w_max / w_max); a zero coefficient whose update stays zero is a
// no-op of the reference's sweep (nothing written, d_w_max / w_max unaffected) and is not visited; the update formula
// (cd_coordinate), d_w_max / w_max, the duality-gap test (:388-425), max_iter, `positive` and the sweep count are the
// reference's.  Only the float summation order of the initial H and of the gap reductions differs.
//
// A sweep: the block finds the first coordinate that moves (each thread scans its own slots, a min-reduction over the
// block), every thread evaluates its update on the same LDS values (wave-uniform), the k-wide update of H follows, then
// the next search starts behind it.  Two barriers per coordinate that moves, none for one that does not.
#include "kernels.hpp"
#include "cd_common.hpp"
#include <climits>

namespace modl {

constexpr int kWideThreads = 256;
constexpr int kWidePer = MODL_MAX_COMPONENTS / kWideThreads;   // coordinates per thread at the bound

__device__ __forceinline__ int wave_min_int(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int u = __shfl_xor(v, o, 64);
        v = u < v ? u : v;
    }
    return v;
}

template <typename T, bool POSITIVE>
__global__ __launch_bounds__(kWideThreads) void cd_wide_kernel(CdArgs<T> a) {
    extern __shared__ __align__(16) unsigned char cd_wide_smem[];
    __shared__ T red[5][kWideThreads / 64];
    __shared__ int nxt[3];                                   // rotating slots of the min-reduction (see next_move)
    const int k = a.k, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int smp = blockIdx.x;
    T *sw = reinterpret_cast<T *>(cd_wide_smem);
    T *sh = sw + k, *sq = sh + k, *sd = sq + k;
    const int64_t ld = a.ldg ? a.ldg : k;
    const T *__restrict__ Q = a.G + (a.g_idx ? a.g_idx[smp] : (int64_t)smp) * a.g_stride;
    const int64_t row_out = a.idx ? a.idx[smp] : (int64_t)smp;
    T *wptr = a.code + row_out * k;
    const T *qptr = a.Dx + (int64_t)smp * k;
    const T alpha = a.alpha, beta = a.beta;

    for (int j = tid; j < k; j += kWideThreads) {
        sw[j] = wptr[j];
        sq[j] = qptr[j];
        sd[j] = Q[(int64_t)j * ld + j];
    }
    if (tid < 3) nxt[tid] = INT_MAX;
    __syncthreads();
    if (a.H0) {
        const T *hp = a.H0 + (int64_t)smp * k;
        for (int j = tid; j < k; j += kWideThreads) sh[j] = hp[j];
    } else {                                                 // H = Q w (:340), rows of the nonzero coefficients
        T acc[kWidePer];
#pragma unroll
        for (int m = 0; m < kWidePer; ++m) acc[m] = 0;
        for (int i = 0; i < k; ++i) {
            const T wi = sw[i];
            if (wi == (T)0) continue;                        // (uniform)
            const T *row = Q + (int64_t)i * ld;
#pragma unroll
            for (int m = 0; m < kWidePer; ++m) {
                const int j = tid + m * kWideThreads;
                if (j < k) acc[m] = fma(wi, row[j], acc[m]);
            }
        }
#pragma unroll
        for (int m = 0; m < kWidePer; ++m) {
            const int j = tid + m * kWideThreads;
            if (j < k) sh[j] = acc[m];
        }
    }
    __syncthreads();

    // the first coordinate after `after` that moves: a nonzero diagonal and a coefficient that is nonzero or becomes so
    int rno = 0;
    auto next_move = [&](int after) -> int {
        int best = INT_MAX;
        for (int j = tid + ((after + 1 > tid) ? (after + 1 - tid + kWideThreads - 1) / kWideThreads * kWideThreads : 0); j < k;
             j += kWideThreads) {
            const T d = sd[j];
            if (d == (T)0) continue;
            const T wj = sw[j];
            if (wj != (T)0 || cd_coordinate<T, POSITIVE>(sh[j], (T)0, sq[j], (T)1 / (d + beta), d, alpha) != (T)0) {
                best = j;
                break;
            }
        }
        best = wave_min_int(best);
        // slot rno % 3 collects this reduction; slot (rno + 1) % 3 was last read two reductions ago, before the barrier
        // of the previous one, so it is re-armed here for the next
        if (tid == 0) nxt[(rno + 1) % 3] = INT_MAX;
        if (lane == 0) atomicMin(&nxt[rno % 3], best);
        __syncthreads();
        const int r = nxt[rno % 3];
        ++rno;
        return r < k ? r : k;
    };

    const T y_norm2 = a.xnorm2[smp];
    const T tol_abs = a.tol * y_norm2;                       // :336
    const T d_w_tol = a.tol;
    int n_iter = 0;
    for (; n_iter < a.max_iter; ++n_iter) {
        T d_w_max = 0, w_max = 0;
        for (int ii = next_move(-1); ii < k; ii = next_move(ii)) {
            const T *row = Q + (int64_t)ii * ld;
            T rv[kWidePer];
#pragma unroll
            for (int m = 0; m < kWidePer; ++m) {             // the row's loads are in flight while the update is evaluated
                const int j = tid + m * kWideThreads;
                rv[m] = row[j < k ? j : k - 1];
            }
            const T wo = sw[ii], dii = sd[ii];
            const T wn = cd_coordinate<T, POSITIVE>(sh[ii], wo, sq[ii], (T)1 / (dii + beta), dii, alpha);   // :361-373
            __syncthreads();                                 // every thread has read sh[ii] / sw[ii]
#pragma unroll
            for (int m = 0; m < kWidePer; ++m) {             // :361-365, :375-378
                const int j = tid + m * kWideThreads;
                if (j < k) sh[j] = fma(wn, rv[m], fma(-wo, rv[m], sh[j]));
            }
            if (tid == (ii & (kWideThreads - 1))) sw[ii] = wn;
            const T dw = fabs(wn - wo), aw = fabs(wn);       // :380-384
            d_w_max = dw > d_w_max ? dw : d_w_max;
            w_max = aw > w_max ? aw : w_max;
        }
        __syncthreads();
        if (w_max == (T)0 || d_w_max / w_max < d_w_tol || n_iter == a.max_iter - 1) {   // :388
            T s_qw = 0, s_wH = 0, s_ww = 0, s_l1 = 0;
            T xmax = POSITIVE ? -INFINITY : (T)0;
            for (int j = tid; j < k; j += kWideThreads) {
                const T wt = sw[j], hj = sh[j], qj = sq[j];
                s_qw += wt * qj;
                s_wH += wt * hj;
                s_ww += wt * wt;
                s_l1 += fabs(wt);
                const T x = (qj - hj) - beta * wt;           // :397
                const T mx = POSITIVE ? x : fabs(x);
                xmax = mx > xmax ? mx : xmax;
            }
            s_qw = wave_sum(s_qw); s_wH = wave_sum(s_wH); s_ww = wave_sum(s_ww); s_l1 = wave_sum(s_l1);
            xmax = wave_max(xmax);
            if (lane == 0) {
                red[0][wid] = s_qw; red[1][wid] = s_wH; red[2][wid] = s_ww; red[3][wid] = s_l1; red[4][wid] = xmax;
            }
            __syncthreads();
            T q_dot_w = red[0][0], wH = red[1][0], w_norm2 = red[2][0], l1 = red[3][0], dual = red[4][0];
#pragma unroll
            for (int v = 1; v < kWideThreads / 64; ++v) {
                q_dot_w += red[0][v]; wH += red[1][v]; w_norm2 += red[2][v]; l1 += red[3][v];
                dual = red[4][v] > dual ? red[4][v] : dual;
            }
            __syncthreads();                                 // (red is reused by the next gap test)
            const double R_norm2 = (double)(y_norm2 + wH) - 2.0 * (double)q_dot_w;   // :404
            double cst;
            T gap;
            if (dual > alpha) {
                cst = (double)(alpha / dual);
                gap = (T)(0.5 * (R_norm2 + R_norm2 * cst * cst));
            } else {
                cst = 1.0;
                gap = (T)R_norm2;
            }
            gap = (T)((double)gap + (((double)(alpha * l1) - cst * (double)y_norm2) + cst * (double)q_dot_w +
                                     ((0.5 * (double)beta) * (1.0 + cst * cst)) * (double)w_norm2));   // :421-423
            if (gap < tol_abs) { ++n_iter; break; }          // :425
        }
    }
    T *w2 = a.code2 ? a.code2 + (a.idx2 ? a.idx2[smp] : (int64_t)smp) * k : nullptr;
    for (int j = tid; j < k; j += kWideThreads) {
        wptr[j] = sw[j];
        if (w2) w2[j] = sw[j];
    }
    if (a.sweeps && tid == 0) a.sweeps[smp] = n_iter;
}

size_t cd_wide_lds_bytes(size_t tsz, int k) { return 4 * tsz * (size_t)k; }

template <typename T>
int launch_cd_wide(hipStream_t stream, const CdArgs<T> &a) {
    if (a.b <= 0 || a.k <= 0) return MODL_OK;
    if (a.k <= 1024 || a.k > MODL_MAX_COMPONENTS) return MODL_EINVAL;
    const size_t lds = cd_wide_lds_bytes(sizeof(T), a.k);
#define MODL_CD_WIDE(POS)                                                                                              \
    do {                                                                                                               \
        MODL_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&cd_wide_kernel<T, POS>),                          \
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));                           \
        hipLaunchKernelGGL((cd_wide_kernel<T, POS>), dim3((unsigned)a.b), dim3(kWideThreads), lds, stream, a);        \
    } while (0)
    if (a.positive) MODL_CD_WIDE(true);
    else MODL_CD_WIDE(false);
#undef MODL_CD_WIDE
    MODL_LAUNCH_CHECK();
    return MODL_OK;
}

template int launch_cd_wide<float>(hipStream_t, const CdArgs<float> &);
template int launch_cd_wide<double>(hipStream_t, const CdArgs<double> &);

}  // namespace modl

extern "C" int modl_max_components(void) { return MODL_MAX_COMPONENTS; }
