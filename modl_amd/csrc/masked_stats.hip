// The surrogate statistic B_ from dense rows with missing entries: step 5 of the masked minibatch, the
// dense-row counterpart of RecsysDictFact's per-feature update (modl/decomposition/recsys.py:175, 182-185).  For the
// minibatch rows i = 1..b with observed sets M_i and codes code_i, per feature e with c_e = #{i : e in M_i} > 0:
//   feature_n_iter[e] += c_e
//   w_e = min(1, w (c_e / b) (n_iter / feature_n_iter[e]))                          (f64)
//   Bt[e][:] <- (1 - w_e) Bt[e][:] + (w_e / c_e) sum_{i : e in M_i} x_ie code_i
// and nothing at all for a feature nobody observes.
//
// Two launches.  masked_stats_kernel: one workgroup per tile of BT features x BT atoms of the product (X o obs)^T code,
// K = b, on the matrix cores in the dtype (the tile sweep of gemm.hpp with R x R tiles of 16 x 16 x 4 per wavefront:
// BT = 32 for small outputs - more workgroups -, 64 otherwise).  The rows of X and obs are staged with lanes walking the features,
// the codes with lanes walking the atoms; an unobserved element is replaced by zero by a select on the way in (nothing
// of X at an unobserved position - NaN included - reaches a product; no zero-filled copy of X exists).  Every workgroup
// counts its own features' observers from the bytes it stages anyway (exact integers, the same in every workgroup of
// a feature), READS feature_n_iter and forms the weights in f64; the axpby runs in the epilogue, through LDS, with
// lanes walking the atoms.  masked_counts_kernel follows on the stream: it alone WRITES feature_n_iter (and the
// optional counts) - no workgroup of a launch updates a word another one of the same launch reads.  No atomics, no
// waits between workgroups, no scratch: the same bits from run to run.
#include "gemm.hpp"
#include "kernels.hpp"

namespace modl {

namespace {

constexpr int kMsBK = 16;

template <typename T, int R>
__global__ __launch_bounds__(256) void masked_stats_kernel(const T *__restrict__ X, int64_t ldx,
                                                           const uint8_t *__restrict__ obs, int64_t ldo,
                                                           const int64_t *__restrict__ rows, int b, int64_t p, int k,
                                                           const T *__restrict__ code, T *__restrict__ Bt,
                                                           const int64_t *__restrict__ fni, double w, double n_iter) {
    using MT = typename Mma16<T>::type;
    static_assert(MT::TM == 16 && MT::TN == 16 && MT::TK == 4, "16 x 16 x 4 tiles");
    constexpr int BT = 32 * R, BK = kMsBK, LD = BT + 1, WT = 16 * R;
    static_assert(BT * LD >= 2 * BK * LD, "the output tile reuses the operand buffers");
    __shared__ T smem[BT * LD];
    __shared__ int s_cnt[4][BT];
    __shared__ T s_beta[BT], s_alpha[BT];
    T(*As)[LD] = reinterpret_cast<T(*)[LD]>(smem);
    T(*Bs)[LD] = reinterpret_cast<T(*)[LD]>(smem + BK * LD);
    T(*Ct)[LD] = reinterpret_cast<T(*)[LD]>(smem);

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, wm = wid >> 1, wn = wid & 1;
    const int64_t e0 = (int64_t)blockIdx.y * BT;              // features
    const int a0 = (int)blockIdx.x * BT;                      // atoms

    {   // c_e of the tile's features: BT features x (256 / BT) slices of the rows
        constexpr int NS = 256 / BT;
        const int fl = tid % BT, sl = tid / BT;
        const int64_t e = e0 + fl < p ? e0 + fl : p - 1;
        int c = 0;
        for (int i = sl; i < b; i += NS) c += obs[(rows ? rows[i] : (int64_t)i) * ldo + e] != 0;
        if constexpr (NS == 4) s_cnt[sl][fl] = c;
        else {                                                // NS == 8: lanes l and l + 32 of a wavefront hold the same
            c += __shfl_xor(c, 32);                           // feature, slices 2 wid and 2 wid + 1: summed into s_cnt[wid]
            if ((lane & 32) == 0) s_cnt[sl >> 1][fl] = c;
        }
    }

    typename MT::acc_t acc[R][R];
    sweep_zero<MT>(acc);

    for (int k0 = 0; k0 < b; k0 += BK) {
#pragma unroll
        for (int t = 0; t < BT * BK / 256; ++t) {
            const int el = tid + t * 256, il = el % BT, kl = el / BT;
            const int i = k0 + kl, ic = i < b ? i : b - 1;
            const int64_t row = rows ? rows[ic] : (int64_t)ic;
            const int64_t e = e0 + il, ec = e < p ? e : p - 1;                 // lanes walk the features
            const bool on = obs[row * ldo + ec] != 0;
            const T v = X[row * ldx + ec];
            As[kl][il] = (on && i < b && e < p) ? v : (T)0;
            const int a = a0 + il, ac = a < k ? a : k - 1;                     // lanes walk the atoms
            const T cv = code[(int64_t)ic * k + ac];
            Bs[kl][il] = (i < b && a < k) ? cv : (T)0;
        }
        __syncthreads();
        sweep_ktile<MT, BK>(acc, As, Bs, wm * WT, wn * WT, lane);
        __syncthreads();
    }

    // the weights of the tile's features, in f64 (s_cnt is complete: the loop has at least one barrier, b >= 1)
    if (tid < BT) {
        const int64_t e = e0 + tid < p ? e0 + tid : p - 1;
        const int c = s_cnt[0][tid] + s_cnt[1][tid] + s_cnt[2][tid] + s_cnt[3][tid];
        double we = 0.0, al = 0.0;
        if (c > 0) {
            const double seen = (double)(fni[e] + c);
            we = w * ((double)c / (double)b) * (n_iter / seen);
            we = we < 1.0 ? we : 1.0;
            al = we / (double)c;
        }
        s_beta[tid] = (T)(1.0 - we);
        s_alpha[tid] = (T)al;
        s_cnt[0][tid] = c;
    }
    sweep_store<MT>(Ct, acc, wm * WT, wn * WT, lane);
    __syncthreads();
    for (int el = tid; el < BT * BT; el += 256) {
        const int m = el / BT, n = el % BT;                   // lanes walk the atoms
        const int64_t e = e0 + m;
        const int a = a0 + n;
        if (e < p && a < k && s_cnt[0][m] > 0) {
            T *o = Bt + e * k + a;
            *o = s_beta[m] * (*o) + s_alpha[m] * Ct[m][n];
        }
    }
}

__global__ __launch_bounds__(256) void masked_counts_kernel(const uint8_t *__restrict__ obs, int64_t ldo,
                                                            const int64_t *__restrict__ rows, int b, int64_t p,
                                                            int64_t *__restrict__ fni, int32_t *__restrict__ count) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= p) return;
    int c = 0;
    for (int i = 0; i < b; ++i) c += obs[(rows ? rows[i] : (int64_t)i) * ldo + e] != 0;
    if (c > 0) fni[e] += c;
    if (count) count[e] = c;
}

// squared norms of the zero-filled rows (the solver's tolerance scales with them, dict_fact_fast.pyx:334): one
// wavefront per row
template <typename T>
__global__ __launch_bounds__(256) void masked_row_norm2_kernel(const T *__restrict__ X, int64_t ldx,
                                                               const uint8_t *__restrict__ obs, int64_t ldo, int64_t p,
                                                               int b, T *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int i = (int)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= b) return;
    double s = 0;
    for (int64_t e = lane; e < p; e += 64) {
        const bool on = obs[i * ldo + e] != 0;
        const T v = X[i * ldx + e];
        s += on ? (double)v * (double)v : 0.0;
    }
    s = wave_sum(s);
    if (lane == 0) out[i] = (T)s;
}

// after the solve: a row nobody observed gets a zero code whatever the solver made of its zero system; the
// minibatch's codes are left compact in codeb[b][k]
template <typename T>
__global__ __launch_bounds__(256) void masked_codes_finish_kernel(T *__restrict__ code, const int64_t *__restrict__ idx,
                                                                  const int32_t *__restrict__ nobs, int k,
                                                                  T *__restrict__ codeb) {
    const int i = (int)blockIdx.x;
    T *src = code + (idx ? idx[i] : (int64_t)i) * k;
    const bool empty = nobs[i] == 0;
    for (int c = threadIdx.x; c < k; c += 256) {
        const T v = empty ? (T)0 : src[c];
        if (empty) src[c] = v;
        codeb[(int64_t)i * k + c] = v;
    }
}

}  // namespace

template <typename T>
int launch_masked_stats(hipStream_t stream, const T *X, int64_t ldx, const uint8_t *obs, int64_t ldo, const int64_t *rows,
                        int64_t b, int64_t p, int k, const T *code_b, T *Bt, int64_t *fni, int32_t *count, double w,
                        int64_t n_iter) {
    if (!X || !obs || !code_b || !Bt || !fni || k < 1 || k > 1024 || p < 1 || b < 0 || b > INT32_MAX || ldx < p || ldo < p)
        return MODL_EINVAL;
    if (b == 0) return MODL_OK;
    if (cdiv(p, 64) * cdiv(k, 64) >= 512) {
        if (cdiv(p, 64) > 65535) return MODL_EINVAL;
        hipLaunchKernelGGL((masked_stats_kernel<T, 2>), dim3((unsigned)cdiv(k, 64), (unsigned)cdiv(p, 64)), dim3(256), 0,
                           stream, X, ldx, obs, ldo, rows, (int)b, p, k, code_b, Bt, fni, w, (double)n_iter);
    } else {
        hipLaunchKernelGGL((masked_stats_kernel<T, 1>), dim3((unsigned)cdiv(k, 32), (unsigned)cdiv(p, 32)), dim3(256), 0,
                           stream, X, ldx, obs, ldo, rows, (int)b, p, k, code_b, Bt, fni, w, (double)n_iter);
    }
    MODL_LAUNCH_CHECK();
    hipLaunchKernelGGL(masked_counts_kernel, dim3((unsigned)cdiv(p, 256)), dim3(256), 0, stream, obs, ldo, rows, (int)b, p,
                       fni, count);
    MODL_LAUNCH_CHECK();
    return MODL_OK;
}

template <typename T>
int launch_masked_row_norm2(hipStream_t stream, const T *X, int64_t ldx, const uint8_t *obs, int64_t ldo, int64_t p, int b,
                            T *out) {
    if (b <= 0) return MODL_OK;
    hipLaunchKernelGGL((masked_row_norm2_kernel<T>), dim3((unsigned)cdiv(b, 4)), dim3(256), 0, stream, X, ldx, obs, ldo, p,
                       b, out);
    MODL_LAUNCH_CHECK();
    return MODL_OK;
}

template <typename T>
int launch_masked_codes_finish(hipStream_t stream, T *code, const int64_t *idx, const int32_t *nobs, int b, int k,
                               T *codeb) {
    if (b <= 0) return MODL_OK;
    hipLaunchKernelGGL((masked_codes_finish_kernel<T>), dim3((unsigned)b), dim3(256), 0, stream, code, idx, nobs, k, codeb);
    MODL_LAUNCH_CHECK();
    return MODL_OK;
}

#define MODL_MS_INST(T)                                                                                                 \
    template int launch_masked_stats<T>(hipStream_t, const T *, int64_t, const uint8_t *, int64_t, const int64_t *,    \
                                        int64_t, int64_t, int, const T *, T *, int64_t *, int32_t *, double, int64_t); \
    template int launch_masked_row_norm2<T>(hipStream_t, const T *, int64_t, const uint8_t *, int64_t, int64_t, int,   \
                                            T *);                                                                      \
    template int launch_masked_codes_finish<T>(hipStream_t, T *, const int64_t *, const int32_t *, int, int, T *);
MODL_MS_INST(float)
MODL_MS_INST(double)
#undef MODL_MS_INST

}  // namespace modl

extern "C" {

int modl_masked_stats_f32(const float *d_X, int64_t ldx, const uint8_t *d_obs, int64_t ldo, const int64_t *d_rows,
                          int64_t b, int64_t p, int k, const float *d_code_b, float *d_Bt, int64_t *d_feature_n_iter,
                          int32_t *d_count, double w, int64_t n_iter, void *stream) {
    return modl::launch_masked_stats<float>((hipStream_t)stream, d_X, ldx, d_obs, ldo, d_rows, b, p, k, d_code_b, d_Bt,
                                            d_feature_n_iter, d_count, w, n_iter);
}
int modl_masked_stats_f64(const double *d_X, int64_t ldx, const uint8_t *d_obs, int64_t ldo, const int64_t *d_rows,
                          int64_t b, int64_t p, int k, const double *d_code_b, double *d_Bt, int64_t *d_feature_n_iter,
                          int32_t *d_count, double w, int64_t n_iter, void *stream) {
    return modl::launch_masked_stats<double>((hipStream_t)stream, d_X, ldx, d_obs, ldo, d_rows, b, p, k, d_code_b, d_Bt,
                                             d_feature_n_iter, d_count, w, n_iter);
}

}  // extern "C"
