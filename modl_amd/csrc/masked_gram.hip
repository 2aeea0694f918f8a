// Per-row masked Gram matrix and Dx: the estimator of modl/decomposition/dict_fact.py:594-604
//   Dx = r X_S D_S^T,  G = r D_S D_S^T,  r = p / |S|
// with S the set of OBSERVED entries of each row instead of one random subset per minibatch, so that every row has a
// Gram matrix of its own - the input of _enet_regression_multi_gram (dict_fact_fast.pyx:33-113).
//
// One workgroup per (sample, 64 x 64 tile of the upper triangle of G): 4 wavefronts in a 2 x 2 grid, each owning a
// 32 x 32 block of the tile (f32: one v_mfma_f32_32x32x2_f32 accumulator; f64: 2 x 2 v_mfma_f64_16x16x4_f64; the tile
// sweep of gemm.hpp).  The rows of Dt stream through LDS once per workgroup, 16 at a time, masked-out rows replaced by
// zeros on the way in (a select, so nothing of X at an unobserved position - NaN included - reaches a product).  The
// tiles of the first tile row also carry the sample's row of X as a 65th operand row: one more MFMA per K-step on
// their two upper wavefronts (the hook of sweep_ktile, on the B fragments the step has read anyway) gives
// Dx[c0 : c0 + 64].  After the K loop the tile, scaled by r, goes through LDS (the operand buffers are free by then)
// and is written twice, both times with lanes walking a row of G: as G[a0 + m][c0 + n] and, off the diagonal, mirrored
// as G[c0 + n][a0 + m].  A diagonal tile writes its upper half to both sides.  G is therefore symmetric bit for bit;
// no atomics, no scratch: the result is the same bits from run to run.
// LDS: 64 * 65 elements (16.3 KB f32, 32.5 KB f64) + 16 of X.
#include "gemm.hpp"
#include "kernels.hpp"

namespace modl {

namespace {

constexpr int kMgTile = 64, kMgBK = 16;

template <typename T>
__global__ __launch_bounds__(256) void masked_gram_kernel(const T *__restrict__ Dt, int64_t p, int k, int ntile,
                                                          const T *__restrict__ X, int64_t ldx,
                                                          const uint8_t *__restrict__ obs, int64_t ldo,
                                                          const int64_t *__restrict__ rows, int64_t ii0,
                                                          T *__restrict__ G, T *__restrict__ Dx,
                                                          int32_t *__restrict__ nobs) {
    using MT = Mma<T>;
    constexpr int BT = kMgTile, BK = kMgBK, LD = BT + 1;
    constexpr int R = 32 / MT::TM;                            // MFMA tiles per wavefront and direction
    __shared__ T smem[BT * LD];
    __shared__ T Xs[BK];
    __shared__ int s_cnt[4];
    T(*As)[LD] = reinterpret_cast<T(*)[LD]>(smem);
    T(*Bs)[LD] = reinterpret_cast<T(*)[LD]>(smem + BK * LD);
    T(*Ct)[LD] = reinterpret_cast<T(*)[LD]>(smem);

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, wm = wid >> 1, wn = wid & 1;
    const int64_t ii = ii0 + blockIdx.y;
    const int64_t i = rows ? rows[ii] : ii;
    const uint8_t *o = obs + i * ldo;
    const T *x = X + i * ldx;

    int ta = 0, tc = (int)blockIdx.x;                         // tile (ta, tc), ta <= tc, numbered row by row
    while (tc >= ntile - ta) { tc -= ntile - ta; ++ta; }
    tc += ta;
    const int a0 = ta * BT, c0 = tc * BT;
    const bool diag = ta == tc, with_dx = ta == 0;            // workgroup-uniform

    int cnt = 0;                                              // m_i: every workgroup of the sample counts it the same way
    for (int64_t e = tid; e < p; e += 256) cnt += o[e] != 0;
    cnt = (int)wave_sum((double)cnt);                         // (exact)
    if (lane == 0) s_cnt[wid] = cnt;

    typename MT::acc_t acc[R][R], accx[1][R];
    sweep_zero<MT>(acc);
    sweep_zero<MT>(accx);

    for (int64_t k0 = 0; k0 < p; k0 += BK) {
        // staging: lanes walk the atoms (contiguous in Dt), 4 rows of Dt per round
#pragma unroll
        for (int t = 0; t < BT * BK / 256; ++t) {
            const int el = tid + t * 256, il = el % BT, kl = el / BT;
            const int64_t e = k0 + kl;
            const bool on = e < p && o[e < p ? e : p - 1] != 0;
            const int64_t ec = e < p ? e : p - 1;
            const int ia = a0 + il < k ? a0 + il : k - 1, ic = c0 + il < k ? c0 + il : k - 1;
            const T va = Dt[ec * k + ia], vc = Dt[ec * k + ic];
            As[kl][il] = (on && a0 + il < k) ? va : (T)0;
            Bs[kl][il] = (on && c0 + il < k) ? vc : (T)0;
        }
        if (with_dx && tid < BK) {
            const int64_t e = k0 + tid;
            const int64_t ec = e < p ? e : p - 1;
            const T v = x[ec];
            Xs[tid] = (e < p && o[ec] != 0) ? v : (T)0;
        }
        __syncthreads();
        sweep_ktile<MT, BK>(acc, As, Bs, wm * 32, wn * 32, lane, [&](int kr, const T(&bf)[R]) {
            if (with_dx && wm == 0) {                         // the row of X as row 0 of one more operand tile
                const T xf = MT::frag_i(lane) == 0 ? Xs[kr] : (T)0;
#pragma unroll
                for (int c = 0; c < R; ++c) accx[0][c] = MT::mma(xf, bf[c], accx[0][c]);
            }
        });
        __syncthreads();
    }

    const int m_i = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    const T r_i = m_i > 0 ? (T)p / (T)m_i : (T)0;
    if (blockIdx.x == 0 && tid == 0 && nobs) nobs[ii] = m_i;

    if (with_dx && wm == 0) {
#pragma unroll
        for (int c = 0; c < R; ++c)
#pragma unroll
            for (int r = 0; r < MT::NACC; ++r) {
                const int n = c0 + wn * 32 + c * MT::TN + MT::acc_col(lane, r);
                if (MT::acc_row(lane, r) == 0 && n < k) Dx[ii * k + n] = r_i * accx[0][c][r];
            }
    }

    // the tile through LDS (free after the loop's last barrier), scaled
    sweep_store<MT, true>(Ct, acc, wm * 32, wn * 32, lane, r_i);
    __syncthreads();
    T *Gi = G + ii * (int64_t)k * k;
    for (int el = tid; el < BT * BT; el += 256) {
        const int m = el / BT, n = el % BT;
        if (a0 + m < k && c0 + n < k)
            Gi[(int64_t)(a0 + m) * k + c0 + n] = (diag && m > n) ? Ct[n][m] : Ct[m][n];
    }
    if (!diag)
        for (int el = tid; el < BT * BT; el += 256) {
            const int n = el / BT, m = el % BT;
            if (a0 + m < k && c0 + n < k) Gi[(int64_t)(c0 + n) * k + a0 + m] = Ct[m][n];
        }
}

template <typename T>
int masked_gram_impl(const T *Dt, int64_t p, int k, const T *X, int64_t ldx, const uint8_t *obs, int64_t ldo,
                     const int64_t *rows, int64_t b, T *G, T *Dx, int32_t *nobs, void *stream) {
    if (!Dt || !X || !obs || !G || !Dx || k < 1 || k > 1024 || p < 1 || b < 0 || ldx < p || ldo < p) return MODL_EINVAL;
    if (b == 0) return MODL_OK;
    const int ntile = (int)cdiv(k, kMgTile);
    constexpr int64_t kMaxY = 65535;                          // samples per launch (gridDim.y)
    for (int64_t ii0 = 0; ii0 < b; ii0 += kMaxY) {
        const int64_t nb = b - ii0 < kMaxY ? b - ii0 : kMaxY;
        hipLaunchKernelGGL((masked_gram_kernel<T>), dim3((unsigned)(ntile * (ntile + 1) / 2), (unsigned)nb), dim3(256),
                           0, (hipStream_t)stream, Dt, p, k, ntile, X, ldx, obs, ldo, rows, ii0, G, Dx, nobs);
        MODL_LAUNCH_CHECK();
    }
    return MODL_OK;
}

}  // namespace

}  // namespace modl

extern "C" {

int modl_masked_gram_f32(const float *d_Dt, int64_t p, int k, const float *d_X, int64_t ldx, const uint8_t *d_obs,
                         int64_t ldo, const int64_t *d_rows, int64_t b, float *d_G, float *d_Dx, int32_t *d_nobs,
                         void *stream) {
    return modl::masked_gram_impl<float>(d_Dt, p, k, d_X, ldx, d_obs, ldo, d_rows, b, d_G, d_Dx, d_nobs, stream);
}
int modl_masked_gram_f64(const double *d_Dt, int64_t p, int k, const double *d_X, int64_t ldx, const uint8_t *d_obs,
                         int64_t ldo, const int64_t *d_rows, int64_t b, double *d_G, double *d_Dx, int32_t *d_nobs,
                         void *stream) {
    return modl::masked_gram_impl<double>(d_Dt, p, k, d_X, ldx, d_obs, ldo, d_rows, b, d_G, d_Dx, d_nobs, stream);
}

}  // extern "C"
