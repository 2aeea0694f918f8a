// The code solve (dict_fact.py:636-648; dict_fact_fast.pyx:82-94, 174-197): which kernels take a minibatch's systems is
// decided in one place (code_route) and launched in one place (code_solve), for the entry points modl_enet_regression_*
// below and, with scratch from their plan, for the minibatch step, the transform and the masked step (somf_step.hip).
#include "gemm_dense.hpp"
#include "kernels.hpp"

namespace modl {

CodeRoute code_route(size_t tsz, int k, double l1_ratio, int64_t g_stride, bool g_aligned16, bool split_enabled,
                     bool one_wave_covers) {
    const bool shared = g_stride == 0;
    if (l1_ratio == 0.0) {                                            // ridge: dict_fact_fast.pyx:82-94, 174-197
        if (chol_blocked(k, tsz, shared)) return CODE_RIDGE_BLOCKED;
        return (tsz == 4 ? ridge_small_applies<float>(k) : ridge_small_applies<double>(k)) ? CODE_RIDGE_SMALL : CODE_RIDGE_FACTOR;
    }
    if (k > 1024) return CODE_CD_WIDE;
    // any k on the vectorised kernel (cd_solver.hip: cd_padded_ld).  Also k = 512 / 1024 when the matrix is not 16-byte
    // aligned: beyond 256 coefficients only the four-wavefront solver exists in the product build, and it wants aligned rows
    if (shared) return (cd_padded_ld(k) != k || (k > 256 && !g_aligned16)) ? CODE_CD_PADDED : CODE_CD_STORED;
    if (k >= 32 && (split_enabled || !one_wave_covers) && !cd_split_takes(tsz, k, k, g_stride, g_aligned16))
        return CODE_CD_SLOTS;
    return CODE_CD_STORED;
}

template <typename T>
int code_solve(hipStream_t st, CdArgs<T> a, T *Dx, T code_alpha, double l1_ratio, const int64_t *h_gidx,
               const CodeScratch<T> &sc, int *launches) {
    const int b = a.b, k = a.k;
    int uncounted = 0;
    int *nl = launches ? launches : &uncounted;
    CodeRoute route = code_route_of<T>(a.G, a.g_stride, k, l1_ratio);
    if (route <= CODE_RIDGE_FACTOR) {
        const T *solved = a.code;                                     // (compact rows where there is a second destination)
        if (route == CODE_RIDGE_BLOCKED) {
            if (a.g_stride && a.g_idx && !h_gidx) return MODL_EINVAL; // per-sample Grams are walked from the host
            MODL_TRY(ridge_solve_wide<T>(st, a.G, a.g_stride, h_gidx, sc.F, sc.Linv, Dx, b, k, code_alpha, a.code, a.idx));
            *nl += 2;
            solved = Dx;                                              // (this leaf scatters what it left in Dx)
        } else if (route == CODE_RIDGE_SMALL) {
            MODL_TRY(launch_ridge_small<T>(st, a.G, a.g_stride, a.g_idx, Dx, b, k, code_alpha, a.code, a.idx));
            *nl += 1;
        } else {
            MODL_TRY(launch_cholesky<T>(st, a.G, a.g_stride, a.g_idx, sc.F, k, code_alpha, a.g_stride ? b : 1));
            MODL_TRY(launch_chol_solve<T>(st, sc.F, a.g_stride ? (int64_t)k * k : 0, Dx, b, k, a.code, a.idx));
            *nl += 2;
        }
        if (a.code2) {
            hipLaunchKernelGGL((scatter_rows_T_kernel<T, int64_t>), dim3((unsigned)b), dim3(256), 0, st, a.code2, (int64_t)k,
                               a.idx2, (int64_t)b, (int64_t)k, solved, (int64_t)k);
            MODL_LAUNCH_CHECK();
            ++*nl;
        }
        return MODL_OK;
    }
    const T l1 = (T)l1_ratio;
    a.Dx = Dx; a.H0 = nullptr; a.ldg = 0; a.g_pad_rows = sc.g_pad_rows;
    a.alpha = (T)(code_alpha * l1);
    a.beta = (T)((double)code_alpha * (1.0 - (double)l1));
    if (sc.h0_by_product && !a.g_stride) {       // H0 = code G on the matrix cores: k rows per sample, not streamed by one CU
        Operand A, B;
        A.ptr = a.code; A.si = k; A.sk = 1; A.gi = gather64(a.idx);
        B.ptr = a.G; B.si = k; B.sk = 1;
        EpiStore<T> epi{sc.H0, k, (T)1};
        SplitWs none;
        MODL_TRY((launch_gemm<T, EpiStore<T>>(st, A, B, b, k, k, epi, none, nl, 512, 1)));
        a.H0 = sc.H0;
    }   // otherwise H0 = Q w is formed inside the solver (rows stream through its prefetch ring: ~6 us at k = 256, less
        // than the launch of a separate 256 x 256 x 256 product that only occupies 16 workgroups)
    if (route == CODE_CD_WIDE) {
        a.g_pad_rows = 0;
        MODL_TRY(launch_cd_wide<T>(st, a));
        ++*nl;
        return MODL_OK;
    }
    if (route == CODE_CD_SLOTS) {                // zero-padded copies, a slice of the minibatch at a time
        if (sc.slots_zero) MODL_HIP(hipMemsetAsync(sc.slots, 0, sc.slots_bytes, st));
        MODL_TRY(launch_cd_per_sample<T>(st, a, sc.slots, sc.slots_bytes));
        *nl += 2;
        return MODL_OK;
    }
    if (route == CODE_CD_PADDED && sc.Gpad) {    // (a caller without the buffer: as stored, launch_cd decides)
        if (sc.gpad_zero_bytes) MODL_HIP(hipMemsetAsync(sc.Gpad, 0, sc.gpad_zero_bytes, st));
        MODL_TRY(launch_cd_pad_gram<T>(st, a.G, k, sc.Gpad, sc.ld_gpad));
        ++*nl;
        a.G = sc.Gpad; a.ldg = sc.ld_gpad; a.g_pad_rows = 16;
    }
    MODL_TRY(launch_cd<T>(st, a));
    ++*nl;
    return MODL_OK;
}
template int code_solve<float>(hipStream_t, CdArgs<float>, float *, float, double, const int64_t *, const CodeScratch<float> &, int *);
template int code_solve<double>(hipStream_t, CdArgs<double>, double *, double, double, const int64_t *, const CodeScratch<double> &, int *);

namespace {

// workspace: xnorm [b] | H0 [b][k] | F (+ Linv behind the first k*k) | padded copy or slots at the tail, zero-filled per
// call (the workspace is the caller's)
template <typename T>
int enet_regression_abi(const T *G, int64_t g_stride, T *Dx, const T *X, int64_t ldx, int64_t p, T *code,
                        const int64_t *d_indices, int64_t b, int64_t k, T l1_ratio, T alpha, int positive, T tol,
                        int max_iter, int32_t *d_sweeps, void *d_ws, size_t ws_bytes, void *stream) {
    if (!G || !Dx || !X || !code || b < 0 || k <= 0 || k > MODL_MAX_COMPONENTS || p < 0 || ldx < p) return MODL_EINVAL;
    if (!(l1_ratio >= 0 && l1_ratio <= 1)) return MODL_EINVAL;
    if (b == 0) return MODL_OK;
    const size_t need = modl_enet_regression_workspace(DType<T>::id, b, k, g_stride != 0);
    if (!d_ws || ws_bytes < need) return MODL_ENOMEM;
    hipStream_t st = (hipStream_t)stream;
    char *w = static_cast<char *>(d_ws);
    T *xnorm = reinterpret_cast<T *>(w);
    CodeScratch<T> sc;
    sc.H0 = reinterpret_cast<T *>(w + align_up(sizeof(T) * (size_t)b, 256));
    sc.F = reinterpret_cast<T *>(w + align_up(sizeof(T) * (size_t)b, 256) + align_up(sizeof(T) * (size_t)b * k, 256));
    sc.Linv = sc.F + (size_t)k * k;
    sc.h0_by_product = g_stride == 0;
    const CodeRoute route = code_route_of<T>(G, g_stride, (int)k, (double)l1_ratio);
    if (route == CODE_CD_PADDED) {
        sc.ld_gpad = cd_padded_ld((int)k);
        sc.gpad_zero_bytes = align_up(sizeof(T) * ((size_t)sc.ld_gpad + 16) * sc.ld_gpad, 256);
        sc.Gpad = reinterpret_cast<T *>(w + need - sc.gpad_zero_bytes);
    } else if (route == CODE_CD_SLOTS) {
        sc.slots_bytes = cd_per_sample_scratch_bytes(sizeof(T), b, (int)k);
        sc.slots = reinterpret_cast<T *>(w + need - align_up(sc.slots_bytes, 256));
        sc.slots_zero = true;
    }
    if (l1_ratio != 0) MODL_TRY(launch_row_norm2<T>(st, X, ldx, p, b, xnorm));
    CdArgs<T> a;
    a.G = G; a.g_stride = g_stride; a.g_idx = nullptr; a.xnorm2 = xnorm; a.code = code; a.idx = d_indices;
    a.sweeps = d_sweeps; a.b = (int)b; a.k = (int)k;
    a.tol = tol; a.max_iter = max_iter; a.positive = positive;
    return code_solve<T>(st, a, Dx, alpha, (double)l1_ratio, nullptr, sc, nullptr);
}

}  // namespace
}  // namespace modl

using namespace modl;

extern "C" {

// the tail: what a call's route can take, whatever the caller's alignment and the diagnostics switch - asked for a
// misaligned matrix (k > 256: such a shared matrix is copied too) and with the four-wavefront solver enabled
size_t modl_enet_regression_workspace(int dtype, int64_t b, int64_t k, int multi_gram) {
    const size_t t = dtype == MODL_F32 ? 4 : 8;
    if (b < 0 || k < 0) return 0;
    size_t tail = 0;
    if (k > 0 && k <= 1024) {                    // (the wide solver wants neither)
        const CodeRoute route = code_route(t, (int)k, 1.0, multi_gram ? k * k : 0, false, true, cd_one_wave_covers((int)k));
        const size_t kq = (size_t)cd_padded_ld((int)k);
        if (route == CODE_CD_PADDED) tail = align_up(t * (kq + 16) * kq, 256);
        if (route == CODE_CD_SLOTS) tail = align_up(cd_per_sample_scratch_bytes(t, b, (int)k), 256);
    }
    return align_up(t * (size_t)b, 256) + align_up(t * (size_t)b * k, 256) +
           align_up(t * ((size_t)k * k * ((multi_gram && k <= 512) ? (size_t)b : 1) + chol_wide_scratch_elems((int)k)), 256) + tail;
}

#define ABI_REG(NAME, T, G_STRIDE)                                                                                        \
    int NAME(const T *d_G, T *d_Dx, const T *d_X, int64_t ldx, int64_t p, T *d_code, const int64_t *d_indices, int64_t b,  \
             int64_t k, T l1_ratio, T alpha, int positive, T tol, int max_iter, int32_t *d_sweeps, void *d_ws,            \
             size_t ws_bytes, void *stream) {                                                                             \
        return enet_regression_abi<T>(d_G, G_STRIDE, d_Dx, d_X, ldx, p, d_code, d_indices, b, k, l1_ratio, alpha, positive, \
                                      tol, max_iter, d_sweeps, d_ws, ws_bytes, stream);                                   \
    }
ABI_REG(modl_enet_regression_single_gram_f32, float, 0)
ABI_REG(modl_enet_regression_single_gram_f64, double, 0)
ABI_REG(modl_enet_regression_multi_gram_f32, float, k * k)
ABI_REG(modl_enet_regression_multi_gram_f64, double, k * k)
#undef ABI_REG

}  // extern "C"
