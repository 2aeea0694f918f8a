// Orthogonal matching pursuit on Gram quantities (Batch-OMP: Rubinstein, Zibulevsky, Elad 2008): at most s atoms per row, or
// until the squared residual is below a threshold.  The kernel never reads X or D: sample i works on G_i (shared, or one per
// row), a0 = Dx[i] and, with a threshold, |x_i|^2.
//
//   I = [], alpha = a0, eps_res = xnorm2[i], delta_prev = 0
//   for t in 0 .. s-1:
//       if tol given and eps_res <= tol: stop
//       j = argmax over i not in I of |alpha_i|                  (ties: the lowest index)
//       if |alpha_j| == 0: stop
//       t > 0: w = solve(L[:t,:t], G[I, j]);  d = G[j,j] - w.w;  d <= 16 eps_T G[j,j]: stop;  L[t,:t] = w;  L[t,t] = sqrt(d)
//       t = 0: G[j,j] <= 0: stop;  L[0,0] = sqrt(G[j,j])
//       I.append(j);  gamma = solve(L L^T, a0[I]);  beta = G[:, I] gamma;  alpha = a0 - beta
//       delta = gamma . beta[I];  eps_res = eps_res - delta + delta_prev;  delta_prev = delta
//   code[i, :] = 0;  code[i, I] = gamma
//
// One wavefront per sample, four samples per workgroup; s <= 64 = one lane per selected atom.  Lane m keeps I_m, gamma_m, y_m
// (y = L^-1 a0[I], which only grows by one entry per step) and L[m][m] in registers and hands them to the wavefront with
// v_readlane; the strictly lower triangle of L is packed in LDS (s (s - 1) / 2 elements per sample: at most 63 KiB per
// workgroup, f64 at s = 64).  No k-vector is stored anywhere: alpha is needed once per step, for the selection, and the lane
// that owns index i (i mod 64) forms alpha_i = a0_i - sum_j gamma_j G[I_j][i] on the fly from rows of the symmetric G
// (contiguous; a shared G stays in L2) and keeps its running best; the selected set is one bit per owned index in a 64-bit
// register (k <= 4096 = 64 x 64).  The arg-max is a butterfly on (|alpha|, -index): the order is total, so every lane ends with
// the same winner.  Every sum has a fixed order that depends on the sample alone: the same bits from run to run and in any
// batch.  There is no workgroup barrier (the wavefronts of a workgroup stop at different steps) and no route by k or s.
#include "kernels.hpp"
#include <limits>

namespace modl {

constexpr int kOmpWaves = 4;          // samples of a workgroup

__device__ __forceinline__ float omp_sqrt(float v) { return sqrtf(v); }
__device__ __forceinline__ double omp_sqrt(double v) { return sqrt(v); }
template <typename T> __device__ __forceinline__ T omp_abs(T v) { return v < (T)0 ? -v : v; }     // (NaN stays NaN: never selected)

// the writes to L of one lane, read by another lane of the same wavefront later on
__device__ __forceinline__ void omp_lds_order() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

static inline size_t omp_lds_bytes(size_t tsz, int s) { return tsz * (size_t)kOmpWaves * ((size_t)s * (s - 1) / 2); }

template <typename T>
__global__ __launch_bounds__(64 * kOmpWaves) void omp_gram_kernel(const T *__restrict__ G, int64_t g_stride,
                                                                  const T *__restrict__ Dx, const T *__restrict__ xnorm2,
                                                                  int64_t b, int k, int s, T tol, T *__restrict__ code,
                                                                  int32_t *__restrict__ support,
                                                                  int32_t *__restrict__ n_active) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int64_t ii = (int64_t)blockIdx.x * kOmpWaves + wid;
    if (ii >= b) return;                                          // (the whole wavefront: nothing below waits for another one)
    T *L = reinterpret_cast<T *>(smem_raw) + (size_t)wid * ((size_t)s * (s - 1) / 2);      // L[m][c], c < m, at m (m - 1) / 2 + c
    const T *Gi = G + ii * g_stride;
    const T *a0 = Dx + ii * k;
    const int nchunk = (k + 63) >> 6;
    const bool use_tol = tol >= (T)0;
    const T thr = (T)16 * std::numeric_limits<T>::epsilon();
    T eps_res = use_tol ? xnorm2[ii] : (T)0, delta_prev = 0;
    unsigned long long sel = 0;                                   // bit m: index m * 64 + lane is selected
    int sup = 0;                                                  // lane m < t: I_m
    T gam = 0, y = 0, dg = 1;                                     // lane m < t: gamma_m, y_m, L[m][m]
    int t = 0;
    for (; t < s; ++t) {
        if (use_tol && eps_res <= tol) break;
        // alpha = a0 - G[:, I] gamma at the indices this lane owns, and the best of them that is not selected
        T best = -1;
        int bi = -1;
        for (int m = 0; m < nchunk; ++m) {
            const int i = m * 64 + lane;
            const int ic = i < k ? i : k - 1;
            T beta = 0;
            for (int j = 0; j < t; ++j) beta += bcast_lane(gam, j) * Gi[(int64_t)bcast_lane(sup, j) * k + ic];
            const T a = omp_abs(a0[ic] - beta);
            if (i < k && !((sel >> m) & 1ull) && a > best) {      // (ascending i: the first of equal values stays)
                best = a;
                bi = i;
            }
        }
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const T ob = __shfl_xor(best, d);
            const int oi = __shfl_xor(bi, d);
            const bool take = ob > best || (ob == best && (unsigned int)oi < (unsigned int)bi);
            best = take ? ob : best;
            bi = take ? oi : bi;
        }
        if (!(bcast_lane(best, 0) > (T)0)) break;                 // nothing left to explain (or nothing comparable: NaN)
        const int j = __builtin_amdgcn_readfirstlane(bi);        // 0 <= j < k: a lane's own index
        const T *Gj = Gi + (int64_t)j * k;
        const T gjj = Gj[j];
        T w = 0;
        if (t > 0) {
            T r = lane < t ? Gj[sup] : (T)0;                      // G[I, j], read from row j of the symmetric G
            for (int c = 0; c < t; ++c) {
                const T wc = bcast_lane(r, c) / bcast_lane(dg, c);
                if (lane == c) w = wc;
                if (lane > c && lane < t) r -= L[lane * (lane - 1) / 2 + c] * wc;
            }
            const T d = gjj - wave_sum(lane < t ? w * w : (T)0);
            if (!(gjj > (T)0) || !(d > thr * gjj)) break;         // atom numerically in the span of I
            if (lane < t) L[t * (t - 1) / 2 + lane] = w;
            if (lane == t) dg = omp_sqrt(d);
            omp_lds_order();
        } else {
            if (!(gjj > (T)0)) break;
            if (lane == 0) dg = omp_sqrt(gjj);
        }
        if (lane == t) sup = j;
        if (lane == (j & 63)) sel |= 1ull << (j >> 6);
        // y_t = (a0[j] - w . y[:t]) / L[t][t], then L^T gamma = y from the last row up
        const T wy = wave_sum(lane < t ? w * y : (T)0);
        if (lane == t) y = (a0[j] - wy) / dg;
        T r = lane <= t ? y : (T)0;
        for (int c = t; c >= 0; --c) {
            const T gc = bcast_lane(r, c) / bcast_lane(dg, c);
            if (lane == c) gam = gc;
            if (lane < c) r -= L[c * (c - 1) / 2 + lane] * gc;
        }
        if (use_tol) {
            T bI = 0;                                             // beta[I_m] on lane m
            for (int jj = 0; jj <= t; ++jj) bI += bcast_lane(gam, jj) * Gi[(int64_t)bcast_lane(sup, jj) * k + sup];
            const T delta = wave_sum(lane <= t ? gam * bI : (T)0);
            eps_res = eps_res - delta + delta_prev;
            delta_prev = delta;
        }
    }
    // t atoms were accepted.  Every element of the outputs of this sample is written exactly once, by one lane.
    T *crow = code + ii * k;
    for (int m = 0; m < nchunk; ++m) {
        const int i = m * 64 + lane;
        if (i < k && !((sel >> m) & 1ull)) crow[i] = 0;
    }
    if (lane < t) crow[sup] = gam;
    if (support && lane < s) support[ii * s + lane] = lane < t ? sup : -1;
    if (n_active && lane == 0) n_active[ii] = t;
}

template <typename T>
int launch_omp(hipStream_t stream, const T *G, int64_t g_stride, const T *Dx, const T *xnorm2, int64_t b, int k, int s, T tol,
               T *code, int32_t *support, int32_t *n_active) {
    if (b <= 0) return MODL_OK;
    hipLaunchKernelGGL((omp_gram_kernel<T>), dim3((unsigned)cdiv(b, kOmpWaves)), dim3(64 * kOmpWaves),
                       omp_lds_bytes(sizeof(T), s), stream, G, g_stride, Dx, xnorm2, b, k, s, tol, code, support, n_active);
    MODL_LAUNCH_CHECK();
    return MODL_OK;
}
template int launch_omp<float>(hipStream_t, const float *, int64_t, const float *, const float *, int64_t, int, int, float,
                               float *, int32_t *, int32_t *);
template int launch_omp<double>(hipStream_t, const double *, int64_t, const double *, const double *, int64_t, int, int,
                                double, double *, int32_t *, int32_t *);

// one Gram matrix per row: k <= 1024, the limit of modl_masked_gram_* that makes them
bool omp_args_ok(int64_t b, int k, int n_nonzero, bool multi_gram) {
    return b >= 0 && b <= ((int64_t)1 << 32) && k >= 1 && k <= (multi_gram ? 1024 : MODL_MAX_COMPONENTS) && n_nonzero >= 1 &&
           n_nonzero <= MODL_OMP_MAX_NONZERO && n_nonzero <= k;
}

template <typename T>
static int omp_gram_abi(const T *G, int64_t g_stride, const T *Dx, const T *xnorm2, int64_t b, int k, int s, T tol, T *code,
                        int32_t *support, int32_t *n_active, void *ws, size_t ws_bytes, void *stream) {
    if (!G || !Dx || !code || !support || !n_active || (tol >= (T)0 && !xnorm2)) return MODL_EINVAL;
    if (g_stride != 0 && (k < 1 || g_stride != (int64_t)k * k)) return MODL_EINVAL;
    if (!omp_args_ok(b, k, s, g_stride != 0)) return MODL_EINVAL;
    if (b == 0) return MODL_OK;
    const size_t need = modl_omp_workspace(DType<T>::id, b, k, s, g_stride != 0);
    if (ws_bytes < need || (need && !ws)) return MODL_ENOMEM;
    if (modl_device_count() <= 0) return MODL_ENOGPU;
    return launch_omp<T>((hipStream_t)stream, G, g_stride, Dx, tol >= (T)0 ? xnorm2 : nullptr, b, k, s, tol, code, support,
                         n_active);
}

}  // namespace modl

using namespace modl;

extern "C" {

size_t modl_omp_workspace(int dtype, int64_t b, int k, int n_nonzero, int multi_gram) {
    // the state of a sample lives in registers and LDS: no scratch in device memory for any valid call
    (void)dtype; (void)b; (void)k; (void)n_nonzero; (void)multi_gram;
    return 0;
}

#define ABI_OMP(SFX, T)                                                                                                   \
    int modl_omp_gram_##SFX(const T *d_G, int64_t g_stride, const T *d_Dx, const T *d_xnorm2, int64_t b, int k,           \
                            int n_nonzero, T tol, T *d_code, int32_t *d_support, int32_t *d_n_active, void *d_ws,         \
                            size_t ws_bytes, void *stream) {                                                              \
        return omp_gram_abi<T>(d_G, g_stride, d_Dx, d_xnorm2, b, k, n_nonzero, tol, d_code, d_support, d_n_active, d_ws,  \
                               ws_bytes, stream);                                                                         \
    }
ABI_OMP(f32, float)
ABI_OMP(f64, double)
#undef ABI_OMP

}  // extern "C"
