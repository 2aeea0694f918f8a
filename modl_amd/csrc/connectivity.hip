// Functional connectivity: the covariance (or correlation) matrices of a list of region-signal
// records in one call, and the seed-to-voxel correlation maps of one record.
//
// Covariance.  Per record s with T rows (time points) of R regions, Xc = X - column means, E = Xc^T Xc / T, all in f64
// (an f32 record is converted on load, so an f32 record and its f64 copy give the same bits).  Three launches:
//   conn_mean_kernel    grid (ceil(R / 64), S): the column means, four phases of time points per column added in a fixed
//                       order;
//   conn_gram_kernel    grid (S * pairs): a workgroup owns one record and one 64 x 64 block (bi <= bj) of the upper
//                       triangle of Xc^T Xc and goes over the whole T of its record, 16 time points a stage, on
//                       v_mfma_f64_16x16x4_f64 through the shared tile sweep (sweep_zero / sweep_ktile / sweep_store); the
//                       CENTRED values are what is staged, rows past T and columns past R as zeros.  The staging is this
//                       file's own (stage_tile neither centres nor converts).  From the staged tiles the workgroup also
//                       forms, per time point, q_a = sum of squares over its row block and q_b over its column block and
//                       accumulates sum_t q_a q_b: summed over all blocks of the square that is
//                       sum_t (sum_i Xc_ti^2)^2, the beta_ of Ledoit-Wolf, without a second product.  It leaves the raw
//                       block in the output, the diagonal in the workspace, and three partial sums (sum of squares of its
//                       block's elements, trace, sum_t q_a q_b) in the workspace;
//   conn_finish_kernel  grid (chunks, S): every workgroup adds the record's partials in ascending block order (off-diagonal
//                       blocks count twice), forms mu, the shrinkage, then for its elements i <= j applies the shrinkage,
//                       optionally divides by the diagonal's square roots, and writes [i][j] and [j][i] from one value:
//                       the output is exactly symmetric.  The diagonal is read from the workspace, never from the output
//                       another workgroup may be writing.
// No floating-point atomics; nothing a record's workgroups compute depends on another record.
//
// Seed maps.  out[r][v] = (sum_t s_tr x_tv) / sqrt(ss_v) with s the prepared seeds (centred, unit norm: sum_t s_tr = 0,
// so the record is never centred).  A workgroup owns 64 voxels and the whole of T; the product runs on the matrix cores in
// the record's dtype (f32: v_mfma_f32_32x32x2_f32, exact FMA chains, t ascending; f64: v_mfma_f64_16x16x4_f64), 128 seeds a
// pass.  While the stage of X passes through the registers of the staging threads they add x and x^2 per voxel in f64
// (first pass only).  By the shapes: for R <= 128 there is one pass and X is read once, from HBM; beyond, pass 2.. re-read
// the workgroup's T x 64 block (T = 1200, f32: 300 KB), which then comes from L2 / the Infinity Cache, not from LDS (160
// KB would not hold it).  There is no K split: one accumulator chain per output.  The epilogue divides, applies the
// constant-voxel rule (ss <= 8 T 2^-53 sum x^2 gives an exact 0) and clips to [-1, 1].
#include <algorithm>
#include <cmath>

#include "gemm.hpp"

namespace modl {

constexpr int kConnMaxRegions = 512;
constexpr int kConnBlk = 64;                                // block of the covariance a workgroup owns (2 x 2 waves, 2 x 2 tiles)
constexpr int kConnBK = 16;                                 // time points per stage
constexpr int kConnLd = kConnBlk + 16;                      // row stride 80 doubles = 32 banks mod 64: the four k-rows of a
                                                            // fragment read fall into distinct banks
constexpr int kSeedBM = 128, kSeedBN = 64;                  // seeds per pass, voxels per workgroup
enum { kConnEmpirical = 0, kConnLedoitWolf = 1 };
enum { kConnCovariance = 0, kConnCorrelation = 1 };

static inline int64_t conn_blocks(int R) { return cdiv(R, kConnBlk); }
static inline int64_t conn_pairs(int R) { return conn_blocks(R) * (conn_blocks(R) + 1) / 2; }
// per record: R means, R diagonal elements, 3 partial sums per block pair; in front of the records the S + 1 offsets
static inline int64_t conn_ws_doubles(int R) { return 2 * (int64_t)R + 3 * conn_pairs(R); }
static inline size_t conn_ws_bytes(int S, int R) { return ((size_t)S + 1) * 8 + (size_t)S * (size_t)conn_ws_doubles(R) * sizeof(double); }

// grid (ceil(R / 64), S), 256 threads: thread (phase, column) adds rows phase, phase + 4, ..; the phases in ascending order
template <typename T>
__global__ __launch_bounds__(256) void conn_mean_kernel(const T *__restrict__ X, int64_t ldx, const int64_t *__restrict__ off,
                                                        int R, double *__restrict__ ws, int64_t ws_rec) {
    __shared__ double part[4][kConnBlk];
    const int s = blockIdx.y, cl = threadIdx.x & 63, ph = threadIdx.x >> 6;
    const int col = blockIdx.x * kConnBlk + cl;
    const int64_t t0 = off[s], Ts = off[s + 1] - t0;
    double acc = 0.0;
    if (col < R)
        for (int64_t t = ph; t < Ts; t += 4) acc += (double)X[(t0 + t) * ldx + col];
    part[ph][cl] = acc;
    __syncthreads();
    if (ph == 0 && col < R) ws[(int64_t)s * ws_rec + col] = (((part[0][cl] + part[1][cl]) + part[2][cl]) + part[3][cl]) / (double)Ts;
}

// grid (S * pairs), 256 threads
template <typename T>
__global__ __launch_bounds__(256) void conn_gram_kernel(const T *__restrict__ X, int64_t ldx, const int64_t *__restrict__ off,
                                                        int R, int pairs, double *__restrict__ cov, double *__restrict__ ws,
                                                        int64_t ws_rec) {
    typedef Mma<double> MT;
    __shared__ double As[kConnBK][kConnLd];
    __shared__ double Bs[kConnBK][kConnLd];
    __shared__ double Ct[kConnBlk][kConnBlk + 1];
    __shared__ double red[4];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, wm = wid >> 1, wn = wid & 1;
    const int s = blockIdx.x / pairs;
    int pr = blockIdx.x % pairs, bi = 0, nb = (R + kConnBlk - 1) / kConnBlk;
    while (pr >= nb - bi) { pr -= nb - bi; ++bi; }          // pairs in the order (0,0) (0,1) .. (1,1) (1,2) ..
    const int bj = bi + pr;
    const int64_t t0 = off[s], Ts = off[s + 1] - t0;
    double *wsr = ws + (int64_t)s * ws_rec;

    // a thread stages column cl of both blocks at the time points rl, rl + 4, rl + 8, rl + 12 of a stage
    const int cl = tid & 63, rl = tid >> 6;
    const int ca = bi * kConnBlk + cl, cb = bj * kConnBlk + cl;
    const double ma = ca < R ? wsr[ca] : 0.0, mb = cb < R ? wsr[cb] : 0.0;
    double na[4], nbv[4];
    auto fetch = [&](int64_t k0) {
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const int64_t t = k0 + rl + 4 * n;
            const bool in = t < Ts;
            const T *row = X + (t0 + (in ? t : 0)) * ldx;
            na[n] = (in && ca < R) ? (double)row[ca] - ma : 0.0;
            nbv[n] = (in && cb < R) ? (double)row[cb] - mb : 0.0;
        }
    };

    MT::acc_t acc[2][2];
    sweep_zero<MT>(acc);
    double qq = 0.0;                                        // sum_t q_a(t) q_b(t) of the time points this thread owns
    fetch(0);
    for (int64_t k0 = 0; k0 < Ts; k0 += kConnBK) {
        __syncthreads();                                    // the previous stage has been consumed
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            As[rl + 4 * n][cl] = na[n];
            Bs[rl + 4 * n][cl] = nbv[n];
        }
        __syncthreads();
        if (k0 + kConnBK < Ts) fetch(k0 + kConnBK);
        sweep_ktile<MT, kConnBK>(acc, As, Bs, wm * 32, wn * 32, lane);
        {   // 16 threads per time point: 4 columns each, then a butterfly over the 16 lanes (every lane the same bits)
            const int kk = tid >> 4, c4 = tid & 15;
            double qa = 0.0, qb = 0.0;
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                const double a = As[kk][c4 + 16 * n], b = Bs[kk][c4 + 16 * n];
                qa += a * a;
                qb += b * b;
            }
#pragma unroll
            for (int m = 1; m < 16; m <<= 1) {
                qa += __shfl_xor(qa, m);
                qb += __shfl_xor(qb, m);
            }
            if (c4 == 0) qq += qa * qb;
        }
    }

    __syncthreads();
    sweep_store<MT>(Ct, acc, wm * 32, wn * 32, lane);
    __syncthreads();
    // the raw block (upper triangle blocks only; the diagonal block whole) to the output, the diagonal to the workspace
    double *C = cov + (int64_t)s * R * R;
    double sq = 0.0, tr = 0.0;
    for (int e = tid; e < kConnBlk * kConnBlk; e += 256) {
        const int il = e >> 6, jl = e & 63, i = bi * kConnBlk + il, j = bj * kConnBlk + jl;
        if (i < R && j < R) {
            const double v = Ct[il][jl];
            C[(int64_t)i * R + j] = v;
            sq += v * v;
            if (i == j) {
                tr += v;
                wsr[R + i] = v;
            }
        }
    }
    sq = block_sum(sq, red);
    tr = block_sum(tr, red);
    qq = block_sum(qq, red);
    if (tid == 0) {
        double *P = wsr + 2 * (int64_t)R + 3 * (blockIdx.x % pairs);
        P[0] = sq;
        P[1] = tr;
        P[2] = qq;
    }
}

// grid (chunks, S), 256 threads
__global__ __launch_bounds__(256) void conn_finish_kernel(const int64_t *__restrict__ off, int R, int pairs, int estimator,
                                                          int output, double *__restrict__ cov, double *__restrict__ shrinkage,
                                                          const double *__restrict__ ws, int64_t ws_rec) {
    __shared__ double dg[kConnMaxRegions];
    const int s = blockIdx.y, tid = threadIdx.x;
    const double *wsr = ws + (int64_t)s * ws_rec, *P = wsr + 2 * (int64_t)R;
    const double Td = (double)(off[s + 1] - off[s]);
    // every thread the same additions in the same order
    double sq = 0.0, tr = 0.0, qq = 0.0;
    {
        const int nb = (R + kConnBlk - 1) / kConnBlk;
        int bi = 0, left = nb;
        for (int p = 0; p < pairs; ++p) {
            const double w = (left == nb - bi) ? 1.0 : 2.0; // the first pair of a row of blocks is its diagonal block
            sq += w * P[3 * p];
            tr += P[3 * p + 1];
            qq += w * P[3 * p + 2];
            if (--left == 0) { ++bi; left = nb - bi; }
        }
    }
    const double p_ = (double)R, trE = tr / Td, mu = trE / p_;
    double shr = 0.0;
    if (estimator == kConnLedoitWolf && R > 1) {            // (one region: nothing to shrink towards, 0 as sklearn answers)
        const double delta_ = sq / (Td * Td);
        double beta = (qq / Td - delta_) / (p_ * Td);
        const double delta = (delta_ - 2.0 * mu * trE + p_ * mu * mu) / p_;
        beta = beta < delta ? beta : delta;
        shr = beta == 0.0 ? 0.0 : beta / delta;
    }
    if (blockIdx.x == 0 && tid == 0) shrinkage[s] = shr;
    for (int i = tid; i < R; i += 256) dg[i] = (1.0 - shr) * (wsr[R + i] / Td) + shr * mu;
    __syncthreads();
    double *C = cov + (int64_t)s * R * R;
    const int64_t n = (int64_t)R * R;
    for (int64_t e = (int64_t)blockIdx.x * 256 + tid; e < n; e += (int64_t)gridDim.x * 256) {
        const int i = (int)(e / R), j = (int)(e % R);
        if (i > j) continue;
        double v;
        if (i == j) v = output == kConnCorrelation ? 1.0 : dg[i];
        else {
            v = (1.0 - shr) * (C[e] / Td);
            if (output == kConnCorrelation) v = v / sqrt(dg[i] * dg[j]);
        }
        C[e] = v;
        C[(int64_t)j * R + i] = v;
    }
}

// ---- seed maps
template <typename T> struct SeedCfg;
template <> struct SeedCfg<float> { static constexpr int RM = 2, RN = 1, PAD = 1; };        // wave: 64 seeds x 32 voxels
template <> struct SeedCfg<double> { static constexpr int RM = 4, RN = 2, PAD = 16; };

// grid (ceil(V / 64)), 256 threads = 2 x 2 waves
template <typename T>
__global__ __launch_bounds__(256) void conn_seed_kernel(const T *__restrict__ X, int64_t ldx, int64_t Tn, int64_t V,
                                                        const T *__restrict__ Sd, int R, T *__restrict__ out, int64_t ldo) {
    typedef Mma<T> MT;
    typedef SeedCfg<T> Cfg;
    constexpr int LDA = kSeedBM + Cfg::PAD, LDB = kSeedBN + Cfg::PAD;
    __shared__ T As[kConnBK][LDA];
    __shared__ T Bs[kConnBK][LDB];
    __shared__ double st[2][4][kSeedBN];
    __shared__ double scale[kSeedBN];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, wm = wid >> 1, wn = wid & 1;
    const int64_t v0 = (int64_t)blockIdx.x * kSeedBN;
    // staging: a thread carries voxel column cl at the time points rl + 4 n and seed column al at the time points ar + 2 n
    const int cl = tid & 63, rl = tid >> 6;
    const int al = tid & 127, ar = tid >> 7;
    const bool vin = v0 + cl < V;
    double sx = 0.0, sxx = 0.0;

    for (int r0 = 0; r0 < R; r0 += kSeedBM) {
        T nb[4], na[8];
        auto fetch = [&](int64_t k0) {
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                const int64_t t = k0 + rl + 4 * n;
                nb[n] = (vin && t < Tn) ? X[t * ldx + v0 + cl] : (T)0;
            }
#pragma unroll
            for (int n = 0; n < 8; ++n) {
                const int64_t t = k0 + ar + 2 * n;
                na[n] = (r0 + al < R && t < Tn) ? Sd[t * R + r0 + al] : (T)0;
            }
        };
        typename MT::acc_t acc[Cfg::RM][Cfg::RN];
        sweep_zero<MT>(acc);
        fetch(0);
        for (int64_t k0 = 0; k0 < Tn; k0 += kConnBK) {
            __syncthreads();
#pragma unroll
            for (int n = 0; n < 4; ++n) Bs[rl + 4 * n][cl] = nb[n];
#pragma unroll
            for (int n = 0; n < 8; ++n) As[ar + 2 * n][al] = na[n];
            if (r0 == 0) {
#pragma unroll
                for (int n = 0; n < 4; ++n) {
                    const double x = (double)nb[n];
                    sx += x;
                    sxx += x * x;
                }
            }
            __syncthreads();
            if (k0 + kConnBK < Tn) fetch(k0 + kConnBK);
            sweep_ktile<MT, kConnBK>(acc, As, Bs, wm * (kSeedBM / 2), wn * (kSeedBN / 2), lane);
        }
        if (r0 == 0) {                                      // the four phases of a voxel in ascending order
            st[0][rl][cl] = sx;
            st[1][rl][cl] = sxx;
            __syncthreads();
            if (tid < kSeedBN) {
                const double a = ((st[0][0][tid] + st[0][1][tid]) + st[0][2][tid]) + st[0][3][tid];
                const double b = ((st[1][0][tid] + st[1][1][tid]) + st[1][2][tid]) + st[1][3][tid];
                const double ss = b - a * a / (double)Tn;
                scale[tid] = ss > 8.0 * (double)Tn * 0x1p-53 * b ? 1.0 / sqrt(ss) : 0.0;
            }
            __syncthreads();
        }
#pragma unroll
        for (int i = 0; i < Cfg::RM; ++i)
#pragma unroll
            for (int j = 0; j < Cfg::RN; ++j)
#pragma unroll
                for (int q = 0; q < MT::NACC; ++q) {
                    const int m = r0 + wm * (kSeedBM / 2) + i * MT::TM + MT::acc_row(lane, q);
                    const int nl = wn * (kSeedBN / 2) + j * MT::TN + MT::acc_col(lane, q);
                    if (m < R && v0 + nl < V) {
                        double c = (double)acc[i][j][q] * scale[nl];
                        c = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);
                        out[(int64_t)m * ldo + v0 + nl] = (T)c;
                    }
                }
    }
}

template <typename T>
static int conn_seed_maps(const T *X, int64_t ldx, int64_t Tn, int64_t V, const T *Sd, int R, T *out, int64_t ldo, void *stream_) {
    if (!X || !Sd || !out) return MODL_EINVAL;
    if (R < 1 || R > kConnMaxRegions || Tn < 2 || V < 1 || ldx < V || ldo < V) return MODL_EINVAL;
    if (V > (int64_t)INT32_MAX * kSeedBN || ldx > INT64_MAX / (int64_t)sizeof(T) / Tn || ldo > INT64_MAX / (int64_t)sizeof(T) / R)
        return MODL_EINVAL;
    if ((uintptr_t)X % sizeof(T) != 0 || (uintptr_t)Sd % sizeof(T) != 0 || (uintptr_t)out % sizeof(T) != 0) return MODL_EINVAL;
    if (modl_device_count() <= 0) return MODL_ENOGPU;
    hipLaunchKernelGGL((conn_seed_kernel<T>), dim3((unsigned)cdiv(V, kSeedBN)), dim3(256), 0, (hipStream_t)stream_, X, ldx, Tn, V, Sd,
                       R, out, ldo);
    MODL_LAUNCH_CHECK();
    return MODL_OK;
}

template <typename T>
static int conn_covariance_entry(const T *X, int64_t ldx, const int64_t *h_off, int S, int R, int estimator, int output, double *cov,
                                 double *shrinkage, void *ws, size_t ws_bytes, void *stream_) {
    if (!X || !h_off || !cov || !shrinkage) return MODL_EINVAL;
    if (R < 1 || R > kConnMaxRegions || S < 1 || S > 65535 || ldx < R) return MODL_EINVAL;
    if (estimator != kConnEmpirical && estimator != kConnLedoitWolf) return MODL_EINVAL;
    if (output != kConnCovariance && output != kConnCorrelation) return MODL_EINVAL;
    if (h_off[0] < 0) return MODL_EINVAL;
    for (int s = 0; s < S; ++s)
        if (h_off[s + 1] < h_off[s] + 2) return MODL_EINVAL;
    if (ldx > INT64_MAX / (int64_t)sizeof(T) / h_off[S]) return MODL_EINVAL;
    if ((uintptr_t)X % sizeof(T) != 0 || (uintptr_t)cov % 8 != 0 || (uintptr_t)shrinkage % 8 != 0 || (uintptr_t)ws % 8 != 0)
        return MODL_EINVAL;
    const int64_t ws_rec = conn_ws_doubles(R);
    if (!ws || ws_bytes < conn_ws_bytes(S, R)) return MODL_ENOMEM;
    if (modl_device_count() <= 0) return MODL_ENOGPU;
    hipStream_t stream = (hipStream_t)stream_;
    // the offsets the kernels read are the ones just checked: they travel in the workspace
    int64_t *d_off = (int64_t *)ws;
    double *w = (double *)ws + (S + 1);
    MODL_HIP(hipMemcpyAsync(d_off, h_off, ((size_t)S + 1) * 8, hipMemcpyHostToDevice, stream));
    const int pairs = (int)conn_pairs(R);
    hipLaunchKernelGGL((conn_mean_kernel<T>), dim3((unsigned)conn_blocks(R), (unsigned)S), dim3(256), 0, stream, X, ldx, d_off, R, w, ws_rec);
    MODL_LAUNCH_CHECK();
    hipLaunchKernelGGL((conn_gram_kernel<T>), dim3((unsigned)((int64_t)S * pairs)), dim3(256), 0, stream, X, ldx, d_off, R, pairs, cov, w,
                       ws_rec);
    MODL_LAUNCH_CHECK();
    const unsigned chunks = (unsigned)std::min<int64_t>(cdiv((int64_t)R * R, 256 * 8), 64);
    hipLaunchKernelGGL(conn_finish_kernel, dim3(chunks, (unsigned)S), dim3(256), 0, stream, d_off, R, pairs, estimator, output, cov,
                       shrinkage, w, ws_rec);
    MODL_LAUNCH_CHECK();
    return MODL_OK;
}

}  // namespace modl

using namespace modl;

extern "C" {

int modl_conn_max_regions(void) { return kConnMaxRegions; }

size_t modl_conn_covariance_workspace(int S, int R) {
    if (S < 1 || S > 65535 || R < 1 || R > kConnMaxRegions) return 0;
    return conn_ws_bytes(S, R);
}

int modl_conn_covariance_f32(const float *d_X, int64_t ldx, const int64_t *h_offsets, int S, int R, int estimator, int output,
                             double *d_cov, double *d_shrinkage, void *d_ws, size_t ws_bytes, void *stream) {
    return conn_covariance_entry<float>(d_X, ldx, h_offsets, S, R, estimator, output, d_cov, d_shrinkage, d_ws, ws_bytes,
                                        stream);
}
int modl_conn_covariance_f64(const double *d_X, int64_t ldx, const int64_t *h_offsets, int S, int R, int estimator, int output,
                             double *d_cov, double *d_shrinkage, void *d_ws, size_t ws_bytes, void *stream) {
    return conn_covariance_entry<double>(d_X, ldx, h_offsets, S, R, estimator, output, d_cov, d_shrinkage, d_ws, ws_bytes,
                                         stream);
}

int modl_conn_seed_maps_f32(const float *d_X, int64_t ldx, int64_t T, int64_t V, const float *d_seeds, int R, float *d_out, int64_t ldo,
                            void *stream) {
    return conn_seed_maps<float>(d_X, ldx, T, V, d_seeds, R, d_out, ldo, stream);
}
int modl_conn_seed_maps_f64(const double *d_X, int64_t ldx, int64_t T, int64_t V, const double *d_seeds, int R, double *d_out, int64_t ldo,
                            void *stream) {
    return conn_seed_maps<double>(d_X, ldx, T, V, d_seeds, R, d_out, ldo, stream);
}

}  // extern "C"
