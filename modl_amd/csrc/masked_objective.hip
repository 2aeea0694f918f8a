// Evaluating a dictionary on rows with missing entries: squared residuals over selected entries, and
// rows completed by their reconstruction.  Both are one product code Dt^T whose n x p result never leaves the chip.
//
// masked_tile_kernel: one workgroup per tile of 64 rows x 64 features, K = k, on the matrix cores in the dtype (4
// wavefronts in a 2 x 2 grid, 2 x 2 tiles of 16 x 16 x 4 each: the tile sweep of gemm.hpp).  Both operands are
// k-contiguous, so lanes walk k when staging.  The finished tile goes through LDS (the operand buffers, reused), from
// where lanes walk the features: the epilogue's reads of X and of the selection bytes - their only reads - and the
// stores of the imputed rows are whole cache lines, and the epilogue does not depend on the C/D lane map of the
// instruction (sweep_store resolves it once, where the tile is written to LDS).
//
//   objective: res = X - (code Dt^T) in the dtype where sel is 1 or 2 - by a select, an entry that is not selected
//     (NaN included) reaches no arithmetic -, the square and every sum in f64.  A workgroup leaves its eight partial
//     sums (class 1: S, W, N; class 2: S, W, N; the workgroups of the first feature tile also sum |code| and code^2 of
//     their rows from the operand they stage anyway) in its own 64 bytes of the workspace;
//     masked_objective_final_kernel, one workgroup, adds them in a fixed order.  No atomics: the same bits from run
//     to run.
//   impute: out = obs ? X : code Dt^T, again by a select, so observed entries keep the bits of X.
#include "gemm.hpp"

namespace modl {

namespace {

constexpr int kMoBT = 64, kMoBK = 32, kMoLD = kMoBT + 1;
constexpr size_t kMoSlot = 8 * sizeof(double);                // a workgroup's partial sums

template <typename T, bool IMPUTE>
__global__ __launch_bounds__(256) void masked_tile_kernel(const T *__restrict__ X, int64_t ldx,
                                                          const uint8_t *__restrict__ sel, int64_t lds, int64_t n,
                                                          int64_t p, const T *__restrict__ Dt, int k,
                                                          const T *__restrict__ code, const double *__restrict__ row_w,
                                                          double *__restrict__ part, T *__restrict__ out, int64_t ldout,
                                                          int64_t tiles_p) {
    using MT = typename Mma16<T>::type;
    static_assert(MT::TM == 16 && MT::TN == 16 && MT::TK == 4, "16 x 16 x 4 tiles");
    constexpr int BT = kMoBT, BK = kMoBK, LD = kMoLD, R = 2, WT = 16 * R;
    static_assert(BT * LD >= 2 * BK * LD, "the output tile reuses the operand buffers");
    __shared__ T smem[BT * LD];
    __shared__ double s_red[4][8];
    T(*As)[LD] = reinterpret_cast<T(*)[LD]>(smem);            // codes:    As[kk][row]
    T(*Bs)[LD] = reinterpret_cast<T(*)[LD]>(smem + BK * LD);  // Dt:       Bs[kk][feature]
    T(*Ct)[LD] = reinterpret_cast<T(*)[LD]>(smem);            // product:  Ct[row][feature]

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, wm = wid >> 1, wn = wid & 1;
    const int64_t tile_i = (int64_t)blockIdx.x / tiles_p, tile_e = (int64_t)blockIdx.x % tiles_p;
    const int64_t i0 = tile_i * BT, e0 = tile_e * BT;
    const bool norms = !IMPUTE && tile_e == 0;                // workgroup-uniform

    typename MT::acc_t acc[R][R];
    sweep_zero<MT>(acc);

    double c_abs = 0.0, c_sq = 0.0;
    for (int k0 = 0; k0 < k; k0 += BK) {
        T cv[BT * BK / 256], dv[BT * BK / 256];
#pragma unroll
        for (int t = 0; t < BT * BK / 256; ++t) {             // lanes walk k; clamped coordinates, zeros selected below
            const int el = tid + t * 256, kl = el % BK, il = el / BK;
            const int kk = k0 + kl, kc = kk < k ? kk : k - 1;
            const int64_t i = i0 + il, ic = i < n ? i : n - 1;
            const int64_t e = e0 + il, ec = e < p ? e : p - 1;
            cv[t] = code[ic * k + kc];
            dv[t] = Dt[ec * k + kc];
        }
#pragma unroll
        for (int t = 0; t < BT * BK / 256; ++t) {
            const int el = tid + t * 256, kl = el % BK, il = el / BK;
            const bool in_k = k0 + kl < k;
            const T c = (in_k && i0 + il < n) ? cv[t] : (T)0;
            As[kl][il] = c;
            Bs[kl][il] = in_k ? dv[t] : (T)0;
            if (norms) {
                c_abs += fabs((double)c);
                c_sq += (double)c * (double)c;
            }
        }
        __syncthreads();
        sweep_ktile<MT, BK>(acc, As, Bs, wm * WT, wn * WT, lane);
        __syncthreads();
    }

    sweep_store<MT>(Ct, acc, wm * WT, wn * WT, lane);
    __syncthreads();

    // lanes walk the features: thread tid owns feature e0 + (tid & 63) of the rows i0 + (tid >> 6) + 4 t
    constexpr int NE = BT * BT / 256;
    const int fl = tid & 63;
    const int64_t e = e0 + fl, ec = e < p ? e : p - 1;
    T xv[NE];
    uint8_t sv[NE];
#pragma unroll
    for (int t = 0; t < NE; ++t) {
        const int64_t i = i0 + wid + 4 * t, ic = i < n ? i : n - 1;
        xv[t] = X[ic * ldx + ec];
        sv[t] = sel[ic * lds + ec];
    }
    if constexpr (IMPUTE) {
#pragma unroll
        for (int t = 0; t < NE; ++t) {
            const int m = wid + 4 * t;
            const int64_t i = i0 + m;
            if (i < n && e < p) out[i * ldout + e] = sv[t] != 0 ? xv[t] : Ct[m][fl];
        }
    } else {
        double w[NE];
#pragma unroll
        for (int t = 0; t < NE; ++t) {
            const int64_t i = i0 + wid + 4 * t, ic = i < n ? i : n - 1;
            w[t] = row_w ? row_w[ic] : 1.0;
        }
        double s1 = 0.0, w1 = 0.0, s2 = 0.0, w2 = 0.0;
        int n1 = 0, n2 = 0;
#pragma unroll
        for (int t = 0; t < NE; ++t) {
            const int m = wid + 4 * t;
            const bool in = i0 + m < n && e < p;
            const bool is1 = in && sv[t] == 1, is2 = in && sv[t] == 2;
            const T x = (is1 || is2) ? xv[t] : (T)0;          // the select: nothing unselected reaches the subtraction
            const T res = x - Ct[m][fl];
            const double r2 = (double)res * (double)res;
            const double wr2 = w[t] * r2;
            s1 += is1 ? r2 : 0.0;
            w1 += is1 ? wr2 : 0.0;
            s2 += is2 ? r2 : 0.0;
            w2 += is2 ? wr2 : 0.0;
            n1 += is1;
            n2 += is2;
        }
        double v[8] = {s1, w1, (double)n1, s2, w2, (double)n2, c_abs, c_sq};   // counts <= 4096: exact
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = wave_sum(v[q]);
        if (lane == 0) {
#pragma unroll
            for (int q = 0; q < 8; ++q) s_red[wid][q] = v[q];
        }
        __syncthreads();
        if (tid < 8) part[(int64_t)blockIdx.x * 8 + tid] = ((s_red[0][tid] + s_red[1][tid]) + s_red[2][tid]) + s_red[3][tid];
    }
}

// out8[q] = the sum of the workgroups' partial sums: thread t adds the slots t / 8, t / 8 + 32, ... of quantity t % 8 in
// index order (a wavefront reads 64 consecutive doubles), then thread q adds the 32 sums of its quantity in index order.
// The counts are sums of integers below 2^53 in f64: exact in any order.
__global__ __launch_bounds__(256) void masked_objective_final_kernel(const double *__restrict__ part, int64_t m,
                                                                     double *__restrict__ out8) {
    __shared__ double red[256];
    const int tid = threadIdx.x, q = tid & 7;
    double s = 0.0;
#pragma unroll 4
    for (int64_t g = tid >> 3; g < m; g += 32) s += part[g * 8 + q];
    red[tid] = s;
    __syncthreads();
    if (tid < 8) {
        double t = 0.0;
#pragma unroll
        for (int j = 0; j < 32; ++j) t += red[j * 8 + tid];
        out8[tid] = t;
    }
}

bool masked_tile_args_ok(int64_t n, int64_t p, int k) {
    return n >= 0 && p >= 1 && k >= 1 && k <= MODL_MAX_COMPONENTS;
}
// the number of workgroups; 0 when the grid would not fit its 31 bits
int64_t masked_tile_count(int64_t n, int64_t p, int64_t *tiles_p) {
    *tiles_p = cdiv(p, kMoBT);
    const int64_t tn = cdiv(n, kMoBT);
    if (tn > 0 && *tiles_p > (int64_t)INT32_MAX / tn) return 0;
    return tn * *tiles_p;
}

template <typename T>
int masked_objective_impl(hipStream_t stream, const T *X, int64_t ldx, const uint8_t *sel, int64_t lds, int64_t n,
                          int64_t p, const T *Dt, int k, const T *code, const double *row_w, void *ws, size_t ws_bytes,
                          double *out8) {
    if (!X || !sel || !Dt || !code || !out8 || !ws || !masked_tile_args_ok(n, p, k) || ldx < p || lds < p)
        return MODL_EINVAL;
    int64_t tiles_p;
    const int64_t wgs = masked_tile_count(n, p, &tiles_p);
    if (n > 0 && wgs == 0) return MODL_EINVAL;
    if (ws_bytes < modl_masked_objective_workspace(DType<T>::id, n, p)) return MODL_ENOMEM;
    double *part = static_cast<double *>(ws);
    if (wgs > 0) {
        hipLaunchKernelGGL((masked_tile_kernel<T, false>), dim3((unsigned)wgs), dim3(256), 0, stream, X, ldx, sel, lds, n,
                           p, Dt, k, code, row_w, part, (T *)nullptr, (int64_t)0, tiles_p);
        MODL_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(masked_objective_final_kernel, dim3(1), dim3(256), 0, stream, part, wgs, out8);
    MODL_LAUNCH_CHECK();
    return MODL_OK;
}

template <typename T>
int impute_impl(hipStream_t stream, const T *code, int64_t n, int k, const T *Dt, int64_t p, const T *X, int64_t ldx,
                const uint8_t *obs, int64_t ldo, T *out, int64_t ldout) {
    if (!code || !Dt || !X || !obs || !out || !masked_tile_args_ok(n, p, k) || ldx < p || ldo < p || ldout < p)
        return MODL_EINVAL;
    int64_t tiles_p;
    const int64_t wgs = masked_tile_count(n, p, &tiles_p);
    if (n > 0 && wgs == 0) return MODL_EINVAL;
    if (wgs == 0) return MODL_OK;
    hipLaunchKernelGGL((masked_tile_kernel<T, true>), dim3((unsigned)wgs), dim3(256), 0, stream, X, ldx, obs, ldo, n, p,
                       Dt, k, code, (const double *)nullptr, (double *)nullptr, out, ldout, tiles_p);
    MODL_LAUNCH_CHECK();
    return MODL_OK;
}

}  // namespace

}  // namespace modl

extern "C" {

size_t modl_masked_objective_workspace(int dtype, int64_t n, int64_t p) {
    (void)dtype;                                              // the partial sums are f64 in both dtypes
    const int64_t tn = modl::cdiv(n < 1 ? 1 : n, modl::kMoBT), tp = modl::cdiv(p < 1 ? 1 : p, modl::kMoBT);
    return (size_t)tn * (size_t)tp * modl::kMoSlot;
}
int modl_masked_objective_f32(const float *d_X, int64_t ldx, const uint8_t *d_sel, int64_t lds, int64_t n, int64_t p,
                              const float *d_Dt, int k, const float *d_code, const double *d_row_w, void *d_ws,
                              size_t ws_bytes, double *d_out8, void *stream) {
    return modl::masked_objective_impl<float>((hipStream_t)stream, d_X, ldx, d_sel, lds, n, p, d_Dt, k, d_code, d_row_w,
                                              d_ws, ws_bytes, d_out8);
}
int modl_masked_objective_f64(const double *d_X, int64_t ldx, const uint8_t *d_sel, int64_t lds, int64_t n, int64_t p,
                              const double *d_Dt, int k, const double *d_code, const double *d_row_w, void *d_ws,
                              size_t ws_bytes, double *d_out8, void *stream) {
    return modl::masked_objective_impl<double>((hipStream_t)stream, d_X, ldx, d_sel, lds, n, p, d_Dt, k, d_code, d_row_w,
                                               d_ws, ws_bytes, d_out8);
}
int modl_impute_f32(const float *d_code, int64_t n, int k, const float *d_Dt, int64_t p, const float *d_X, int64_t ldx,
                    const uint8_t *d_obs, int64_t ldo, float *d_out, int64_t ldout, void *stream) {
    return modl::impute_impl<float>((hipStream_t)stream, d_code, n, k, d_Dt, p, d_X, ldx, d_obs, ldo, d_out, ldout);
}
int modl_impute_f64(const double *d_code, int64_t n, int k, const double *d_Dt, int64_t p, const double *d_X, int64_t ldx,
                    const uint8_t *d_obs, int64_t ldo, double *d_out, int64_t ldout, void *stream) {
    return modl::impute_impl<double>((hipStream_t)stream, d_code, n, k, d_Dt, p, d_X, ldx, d_obs, ldo, d_out, ldout);
}

}  // extern "C"
