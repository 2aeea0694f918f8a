// Dense, software-pipelined matrix-core contraction (no gathers):
//
//   out(m, n) = epilogue( sum_kk A(m, kk) * B(n, kk) ),   X(i, kk) = ptr[i * si + kk * sk], si == 1 or sk == 1
//
// This is the fast path of the SOMF step: the step first compacts what it
// gathers (sampled dictionary rows, sampled columns of the minibatch, the
// minibatch's code rows), then every product is a plain strided GEMM.
//
// gfx950 mapping: 64x64 block tile, BK = 32, 4 wavefronts (2x2) each owning one
// 32x32 v_mfma_f32_32x32x2_f32 tile (f64: 2x2 v_mfma_f64_16x16x4_f64 tiles).
// Global -> register -> LDS staging with 16-byte loads along the contiguous
// dimension; the loads of K-tile t+1 are issued before the MFMA loop of tile t
// and written to the other LDS buffer afterwards (one barrier per K-tile).
// Operands are k-major in LDS (row stride BI + 4: 16-byte aligned vector stores,
// conflict-free fragment reads).  Split-K partial tiles are reduced in a fixed
// order (gemm_reduce_kernel) -> deterministic results.
#pragma once
#include "gemm.hpp"
#include <type_traits>

namespace modl {

struct DenseOperand {
    const void *ptr = nullptr;
    int64_t si = 0, sk = 0;
    bool unal = false;      // set by plan_dense: base or leading stride not a multiple of 16 bytes (k % 4 != 0 ...): every
                            // tile is staged element by element like an edge tile - still the tiled matrix-core kernel,
                            // not the gather kernel of gemm.hpp
};

// Epilogues that read what they overwrite declare `static constexpr bool rmw = true` and split into
// load(m, n) -> old value and store(m, n, v, old); operator() stays (split-K reduction, generic kernel).
template <class E, class = void> struct EpiIsRmw : std::false_type {};
template <class E> struct EpiIsRmw<E, std::void_t<decltype(E::rmw)>> : std::true_type {};
// what load() hands to store(): the old value, or a struct carrying more (EpiStatsSkip: the row's stamp, so that store()
// has nothing left to fetch - a load inside store() was a memory round trip per element)
template <class E, typename T, class = void> struct EpiOldT { typedef T type; };
template <class E, typename T> struct EpiOldT<E, T, std::void_t<typename E::Old>> { typedef typename E::Old type; };
template <class E, typename T> using EpiOld = typename EpiOldT<E, T>::type;

// Column swizzle of the k-major LDS tiles: element (k-row kl, column il) lives at column il ^ gd_swz(kl).  The operand that is
// contiguous along K is written TRANSPOSED - a thread's 16-byte vector becomes four scalar stores to four consecutive k-rows - and
// with the plain layout (row stride BI + 4 words: 4 banks) the eight threads that hold one operand row hit two banks, four-way
// conflicts (SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE = 0.235, round 5's counters).  XOR-ing bits 2-4 of the
// column with bits 2-4 of the k-row spreads them over eight banks; a fragment read (32 consecutive columns of one k-row) and a
// 16-byte vector store along the columns are permuted in whole groups of four: both stay conflict-free and aligned.
#ifndef MODL_GEMM_SWZ
#define MODL_GEMM_SWZ 1
#endif
__device__ __forceinline__ int gd_swz(int kl) { return MODL_GEMM_SWZ ? (((kl >> 2) & 7) << 2) : 0; }

template <typename T> struct Vec4;   // 16-byte vector of T
template <> struct Vec4<float> { typedef float4 type; static constexpr int N = 4; };
template <> struct Vec4<double> { typedef double2 type; static constexpr int N = 2; };

// Stage one BI x BK operand tile global -> registers (16-byte vectors along the contiguous dim).
// NV vectors per thread.  FAST = tile fully inside the matrix; otherwise element-wise guarded.
template <typename T, int BI, int BK, bool IFAST>
struct TileLoader {
    static constexpr int VN = Vec4<T>::N;
    static constexpr int NV = BI * BK / VN / 256;
    typedef typename Vec4<T>::type V;
    V r[NV];
    unsigned msk = 0;                                 // elements outside the operand (edge tiles): stored as zeros

    // Requests the tile; nothing waits here.  A tile that lies fully inside the operand (a workgroup-uniform test)
    // is fetched with plain 16-byte loads; an edge tile element by element from clamped addresses, selecting zeros
    // afterwards — no per-thread branches either way: a branch around a load makes the compiler wait for that
    // load right behind it, which serialises every memory round trip of the tile.
    __device__ __forceinline__ void load(const DenseOperand &op, int64_t i0, int64_t I, int64_t k0, int64_t k_end) {
        const T *base = static_cast<const T *>(op.ptr);
        const bool interior = !op.unal && (i0 + BI <= I) && (k0 + BK <= k_end);
        if (interior) {
            msk = 0;
#pragma unroll
            for (int q = 0; q < NV; ++q) {
                const int e = threadIdx.x + 256 * q;
                int il, kl;
                if (IFAST) { il = (e % (BI / VN)) * VN; kl = e / (BI / VN); }
                else { kl = (e % (BK / VN)) * VN; il = e / (BK / VN); }
                r[q] = *reinterpret_cast<const V *>(base + (i0 + il) * op.si + (k0 + kl) * op.sk);
            }
        } else {
            msk = 0;
#pragma unroll
            for (int q = 0; q < NV; ++q) {
                const int e = threadIdx.x + 256 * q;
                int il, kl;
                if (IFAST) { il = (e % (BI / VN)) * VN; kl = e / (BI / VN); }
                else { kl = (e % (BK / VN)) * VN; il = e / (BK / VN); }
                const int64_t i = i0 + il, kk = k0 + kl;
                const T *p = base + i * op.si + kk * op.sk;
                T *vp = reinterpret_cast<T *>(&r[q]);
#pragma unroll
                for (int c = 0; c < VN; ++c) {
                    const bool in = IFAST ? (i + c < I && kk < k_end) : (i < I && kk + c < k_end);
                    vp[c] = *(in ? p + c : base);             // the zeros are selected in store(): nothing waits here
                    msk |= (in ? 0u : 1u) << (q * VN + c);
                }
            }
        }
    }
    __device__ __forceinline__ void store(T (*S)[BI + 4]) const {
#pragma unroll
        for (int q = 0; q < NV; ++q) {
            const int e = threadIdx.x + 256 * q;
            V v = r[q];
            T *t = reinterpret_cast<T *>(&v);
#pragma unroll
            for (int c = 0; c < VN; ++c) t[c] = ((msk >> (q * VN + c)) & 1u) ? (T)0 : t[c];
            if (IFAST) {
                const int il = (e % (BI / VN)) * VN, kl = e / (BI / VN);
                *reinterpret_cast<V *>(&S[kl][il ^ gd_swz(kl)]) = v;
            } else {
                const int kl = (e % (BK / VN)) * VN, il = e / (BK / VN);
#pragma unroll
                for (int c = 0; c < VN; ++c) S[kl + c][il ^ gd_swz(kl + c)] = t[c];
            }
        }
    }
};

// Epilogue of one tile: the accumulators of this thread go through `epi` (or to the split-K partial buffer).
template <typename T, class Epi, int BM, int BN, int RM, int RN, class MT = Mma<T>>
__device__ __forceinline__ void gemm_tile_epilogue(typename MT::acc_t (&acc)[RM][RN], int64_t M, int64_t N, T *partial,
                                                   const Epi &epi, int64_t m0, int64_t n0, int bz, int nsplit) {
    constexpr int WM = BM / 2, WN = BN / 2;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int wm = wid >> 1, wn = wid & 1;
    const bool direct = (nsplit == 1);
    if constexpr (EpiIsRmw<Epi>::value) {
        // read-modify-write epilogues: ALL the old values are requested first, then everything is stored (element by
        // element the compiler has to keep each load behind the previous store, which might alias it)
        if (direct) {
            EpiOld<Epi, T> old[RM][RN][MT::NACC];
#pragma unroll
            for (int i = 0; i < RM; ++i)
#pragma unroll
                for (int j = 0; j < RN; ++j)
#pragma unroll
                    for (int r = 0; r < MT::NACC; ++r) {
                        const int64_t m = m0 + wm * WM + i * MT::TM + MT::acc_row(lane, r);
                        const int64_t n = n0 + wn * WN + j * MT::TN + MT::acc_col(lane, r);
                        // never a branch around a load (the compiler would wait for it right there): edge elements
                        // read a clamped, valid address and are simply not stored
                        old[i][j][r] = epi.load(m < M ? m : M - 1, n < N ? n : N - 1);
                    }
#pragma unroll
            for (int i = 0; i < RM; ++i)
#pragma unroll
                for (int j = 0; j < RN; ++j)
#pragma unroll
                    for (int r = 0; r < MT::NACC; ++r) {
                        const int64_t m = m0 + wm * WM + i * MT::TM + MT::acc_row(lane, r);
                        const int64_t n = n0 + wn * WN + j * MT::TN + MT::acc_col(lane, r);
                        if (m < M && n < N) epi.store(m, n, acc[i][j][r], old[i][j][r]);
                    }
            return;
        }
    }
#pragma unroll
    for (int i = 0; i < RM; ++i)
#pragma unroll
        for (int j = 0; j < RN; ++j)
#pragma unroll
            for (int r = 0; r < MT::NACC; ++r) {
                const int64_t m = m0 + wm * WM + i * MT::TM + MT::acc_row(lane, r);
                const int64_t n = n0 + wn * WN + j * MT::TN + MT::acc_col(lane, r);
                if (m < M && n < N) {
                    if (direct) epi(m, n, acc[i][j][r]);
                    else partial[((int64_t)bz * M + m) * N + n] = acc[i][j][r];
                }
            }
}

// One output tile of one (possibly K-split) product.  (bx, by, bz) = tile column, tile row, split index.
template <typename T, bool AIFAST, bool BIFAST, class Epi, int BM, int BN, int BK>
__device__ __forceinline__ void gemm_dense_tile(const DenseOperand &A, const DenseOperand &B, int64_t M, int64_t N,
                                                int64_t K, int64_t k_per_split, T *partial, const Epi &epi, int bx, int by,
                                                int bz, int nsplit, T (*As)[BK][BM + 4], T (*Bs)[BK][BN + 4]) {
    using MT = Mma<T>;
    constexpr int WM = BM / 2, WN = BN / 2;               // 2 x 2 waves
    constexpr int RM = WM / MT::TM, RN = WN / MT::TN;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int wm = wid >> 1, wn = wid & 1;
    const int64_t m0 = (int64_t)by * BM, n0 = (int64_t)bx * BN;
    const int64_t k_begin = (int64_t)bz * k_per_split;
    const int64_t k_end = (k_begin + k_per_split < K) ? k_begin + k_per_split : K;

    typename MT::acc_t acc[RM][RN];
#pragma unroll
    for (int i = 0; i < RM; ++i)
#pragma unroll
        for (int j = 0; j < RN; ++j)
#pragma unroll
            for (int r = 0; r < MT::NACC; ++r) acc[i][j][r] = 0;

    TileLoader<T, BM, BK, AIFAST> la;
    TileLoader<T, BN, BK, BIFAST> lb;
    la.load(A, m0, M, k_begin, k_end);
    lb.load(B, n0, N, k_begin, k_end);
    la.store(As[0]);
    lb.store(Bs[0]);
    __syncthreads();
    int cur = 0;
    for (int64_t k0 = k_begin; k0 < k_end; k0 += BK) {
        const bool more = k0 + BK < k_end;
        if (more) {
            la.load(A, m0, M, k0 + BK, k_end);
            lb.load(B, n0, N, k0 + BK, k_end);
        }
#pragma unroll
        for (int kk = 0; kk < BK; kk += MT::TK) {
            T af[RM], bf[RN];
            const int kr = kk + MT::frag_k(lane);
#pragma unroll
            for (int i = 0; i < RM; ++i) af[i] = As[cur][kr][(wm * WM + i * MT::TM + MT::frag_i(lane)) ^ gd_swz(kr)];
#pragma unroll
            for (int j = 0; j < RN; ++j) bf[j] = Bs[cur][kr][(wn * WN + j * MT::TN + MT::frag_i(lane)) ^ gd_swz(kr)];
#pragma unroll
            for (int i = 0; i < RM; ++i)
#pragma unroll
                for (int j = 0; j < RN; ++j) acc[i][j] = MT::mma(af[i], bf[j], acc[i][j]);
        }
        if (more) {
            la.store(As[cur ^ 1]);
            lb.store(Bs[cur ^ 1]);
        }
        __syncthreads();
        cur ^= 1;
    }

    gemm_tile_epilogue<T, Epi, BM, BN, RM, RN>(acc, M, N, partial, epi, m0, n0, bz, nsplit);
}

// Workgroup barrier that orders LDS traffic only (__syncthreads() also waits for every outstanding global load).
__device__ __forceinline__ void gemm_lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// The same tile for a SHORT contraction (K <= NKT * BK, no split): every K-tile of both operands is requested from
// memory at once and waits in registers (NKT * 16 VGPRs for f32 64 x 64 x 32 tiles), so the tile costs ONE memory
// round trip instead of one per K-tile.  With K = 256 (the minibatch) the pipelined tile above spends ~3 us per
// K-tile waiting for its single prefetch: 26 us for a tile whose matrix-core work is 3.4 us.
template <typename T, bool AIFAST, bool BIFAST, class Epi, int BM, int BN, int BK, int NKT, class MT = Mma<T>>
__device__ __forceinline__ void gemm_dense_tile_rk(const DenseOperand &A, const DenseOperand &B, int64_t M, int64_t N,
                                                   int64_t k_begin, int64_t k_end, T *partial, const Epi &epi, int bx, int by,
                                                   int bz, int nsplit, T (*As)[BK][BM + 4], T (*Bs)[BK][BN + 4],
                                                   unsigned long long *dbg = nullptr) {
    const int64_t K = k_end - k_begin;               // at most NKT * BK
    if (dbg && threadIdx.x == 0) { dbg[0] = clock64(); dbg[6] = wall_clock64(); }
    constexpr int WM = BM / 2, WN = BN / 2;
    constexpr int RM = WM / MT::TM, RN = WN / MT::TN;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int wm = wid >> 1, wn = wid & 1;
    const int64_t m0 = (int64_t)by * BM, n0 = (int64_t)bx * BN;
    typename MT::acc_t acc[RM][RN];
#pragma unroll
    for (int i = 0; i < RM; ++i)
#pragma unroll
        for (int j = 0; j < RN; ++j)
#pragma unroll
            for (int r = 0; r < MT::NACC; ++r) acc[i][j][r] = 0;
    typename MT::acc_t acc2[RM][RN];
#pragma unroll
    for (int i = 0; i < RM; ++i)
#pragma unroll
        for (int j = 0; j < RN; ++j)
#pragma unroll
            for (int r = 0; r < MT::NACC; ++r) acc2[i][j][r] = 0;
    TileLoader<T, BM, BK, AIFAST> la[NKT];
    TileLoader<T, BN, BK, BIFAST> lb[NKT];
    // the common case — a tile inside both operands, whole K-tiles — as straight-line code: one pointer per thread and
    // operand, every load at a constant multiple of a stride
    const int nkt = (int)((K + BK - 1) / BK);
    const bool plain = !A.unal && !B.unal && m0 + BM <= M && n0 + BN <= N && K % BK == 0;
    if (plain) {
        constexpr int VN = Vec4<T>::N;
        typedef typename Vec4<T>::type V;
        constexpr int NVA = TileLoader<T, BM, BK, AIFAST>::NV, NVB = TileLoader<T, BN, BK, BIFAST>::NV;
        // thread -> (row il, k kl) of its first vector; one pass of the 256 threads covers PA k-rows (row-contiguous
        // operand) or PA rows (k-contiguous operand)
        constexpr int PA = AIFAST ? 256 / (BM / VN) : 256 / (BK / VN), PB = BIFAST ? 256 / (BN / VN) : 256 / (BK / VN);
        const int ila = AIFAST ? (threadIdx.x % (BM / VN)) * VN : threadIdx.x / (BK / VN);
        const int kla = AIFAST ? threadIdx.x / (BM / VN) : (threadIdx.x % (BK / VN)) * VN;
        const int ilb = BIFAST ? (threadIdx.x % (BN / VN)) * VN : threadIdx.x / (BK / VN);
        const int klb = BIFAST ? threadIdx.x / (BN / VN) : (threadIdx.x % (BK / VN)) * VN;
        const T *pa = static_cast<const T *>(A.ptr) + (m0 + ila) * A.si + (k_begin + kla) * A.sk;
        const T *pb = static_cast<const T *>(B.ptr) + (n0 + ilb) * B.si + (k_begin + klb) * B.sk;
        const int64_t qa = AIFAST ? (int64_t)PA * A.sk : (int64_t)PA * A.si, ta = (int64_t)BK * A.sk;
        const int64_t qb = BIFAST ? (int64_t)PB * B.sk : (int64_t)PB * B.si, tb = (int64_t)BK * B.sk;
#pragma unroll
        for (int t = 0; t < NKT; ++t)
            if (t < nkt) {
#pragma unroll
                for (int q = 0; q < NVA; ++q) la[t].r[q] = *reinterpret_cast<const V *>(pa + t * ta + q * qa);
#pragma unroll
                for (int q = 0; q < NVB; ++q) lb[t].r[q] = *reinterpret_cast<const V *>(pb + t * tb + q * qb);
                la[t].msk = 0;
                lb[t].msk = 0;
            }
    } else {
#pragma unroll
        for (int t = 0; t < NKT; ++t)
            if (t < nkt) {
                la[t].load(A, m0, M, k_begin + (int64_t)t * BK, k_end);
                lb[t].load(B, n0, N, k_begin + (int64_t)t * BK, k_end);
            }
    }
    // a read-modify-write epilogue's old values do not depend on the product: requested now, with the operands
    constexpr bool kRmw = EpiIsRmw<Epi>::value;
    EpiOld<Epi, T> old[RM][RN][MT::NACC];
    if constexpr (kRmw) {
        if (nsplit == 1) {
#pragma unroll
            for (int i = 0; i < RM; ++i)
#pragma unroll
                for (int j = 0; j < RN; ++j)
#pragma unroll
                    for (int r = 0; r < MT::NACC; ++r) {
                        const int64_t m = m0 + wm * WM + i * MT::TM + MT::acc_row(lane, r);
                        const int64_t n = n0 + wn * WN + j * MT::TN + MT::acc_col(lane, r);
                        old[i][j][r] = epi.load(m < M ? m : M - 1, n < N ? n : N - 1);
                    }
        }
    }
    if (dbg && threadIdx.x == 0) dbg[1] = clock64();
    la[0].store(As[0]);
    lb[0].store(Bs[0]);
    gemm_lds_barrier();
    if (dbg && threadIdx.x == 0) dbg[2] = clock64();
#pragma unroll
    for (int t = 0; t < NKT; ++t)
        if (t < nkt) {
            // the next K-tile goes to the other buffer (last read in step t - 1, before that step's barrier) while the
            // matrix cores work on this one; all fragments of a K-tile are read before its first MFMA
            if (t + 1 < NKT && t + 1 < nkt) {
                la[(t + 1) % NKT].store(As[(t + 1) & 1]);
                lb[(t + 1) % NKT].store(Bs[(t + 1) & 1]);
            }
            constexpr int NS = BK / MT::TK;
            T af[NS][RM], bf[NS][RN];
#pragma unroll
            for (int u = 0; u < NS; ++u) {
                const int kr = u * MT::TK + MT::frag_k(lane);
#pragma unroll
                for (int i = 0; i < RM; ++i) af[u][i] = As[t & 1][kr][(wm * WM + i * MT::TM + MT::frag_i(lane)) ^ gd_swz(kr)];
#pragma unroll
                for (int j = 0; j < RN; ++j) bf[u][j] = Bs[t & 1][kr][(wn * WN + j * MT::TN + MT::frag_i(lane)) ^ gd_swz(kr)];
            }
            // two accumulators (even / odd k-steps): a matrix-core instruction that accumulates onto the result of
            // the previous one waits for it (~2x its issue time, measured), two independent chains do not
#pragma unroll
            for (int u = 0; u < NS; ++u)
#pragma unroll
                for (int i = 0; i < RM; ++i)
#pragma unroll
                    for (int j = 0; j < RN; ++j) {
                        if (u & 1) acc2[i][j] = MT::mma(af[u][i], bf[u][j], acc2[i][j]);
                        else acc[i][j] = MT::mma(af[u][i], bf[u][j], acc[i][j]);
                    }
            gemm_lds_barrier();
        }
#pragma unroll
    for (int i = 0; i < RM; ++i)
#pragma unroll
        for (int j = 0; j < RN; ++j)
#pragma unroll
            for (int r = 0; r < MT::NACC; ++r) acc[i][j][r] += acc2[i][j][r];
    if (dbg && threadIdx.x == 0) dbg[3] = clock64();
    bool stored = false;
    if constexpr (kRmw) {
        if (nsplit == 1) {
#pragma unroll
            for (int i = 0; i < RM; ++i)
#pragma unroll
                for (int j = 0; j < RN; ++j)
#pragma unroll
                    for (int r = 0; r < MT::NACC; ++r) {
                        const int64_t m = m0 + wm * WM + i * MT::TM + MT::acc_row(lane, r);
                        const int64_t n = n0 + wn * WN + j * MT::TN + MT::acc_col(lane, r);
                        if (m < M && n < N) epi.store(m, n, acc[i][j][r], old[i][j][r]);
                    }
            stored = true;
        }
    }
    if (!stored) gemm_tile_epilogue<T, Epi, BM, BN, RM, RN, MT>(acc, M, N, partial, epi, m0, n0, bz, nsplit);
    if (dbg && threadIdx.x == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        dbg[4] = clock64();
        dbg[7] = wall_clock64();
    }
}

// tile of a planned problem: the resident-K variant when the contraction is short (f32)
template <typename T, bool AI, bool BI, class Epi, int BM, int BN, int BK>
__device__ __forceinline__ void gemm_dense_tile_auto(const DenseOperand &A, const DenseOperand &B, int64_t M, int64_t N,
                                                     int64_t K, int64_t kps, T *partial, const Epi &epi, int bx, int by, int bz,
                                                     int nsplit, T (*As)[BK][BM + 4], T (*Bs)[BK][BN + 4],
                                                     unsigned long long *dbg = nullptr) {
    constexpr int NKT = kDenseRkTiles;                       // (dense_tile_of, gemm_plan.hpp, names the same choice on the host)
    if constexpr (sizeof(T) == 4 && BM <= 64 && BN <= 64) {      // (128 x 128 tiles: 256 registers of operands - the pipelined tile only)
        const int64_t k_begin = (int64_t)bz * kps, k_end = (k_begin + kps < K) ? k_begin + kps : K;
        if (k_end - k_begin <= (int64_t)NKT * BK) {
            gemm_dense_tile_rk<T, AI, BI, Epi, BM, BN, BK, NKT>(A, B, M, N, k_begin, k_end, partial, epi, bx, by, bz, nsplit,
                                                                As, Bs, dbg);
            return;
        }
    }
    gemm_dense_tile<T, AI, BI, Epi, BM, BN, BK>(A, B, M, N, K, kps, partial, epi, bx, by, bz, nsplit, As, Bs);
}

template <typename T, bool AIFAST, bool BIFAST, class Epi>
__global__ __launch_bounds__(256) void gemm_dense_kernel(DenseOperand A, DenseOperand B, int64_t M, int64_t N, int64_t K,
                                                         int64_t k_per_split, T *partial, Epi epi) {
    constexpr int BM = 64, BN = 64, BK = (sizeof(T) == 4) ? 32 : 16;
    __shared__ __attribute__((aligned(16))) T As[2][BK][BM + 4];
    __shared__ __attribute__((aligned(16))) T Bs[2][BK][BN + 4];
    gemm_dense_tile<T, AIFAST, BIFAST, Epi, BM, BN, BK>(A, B, M, N, K, k_per_split, partial, epi, (int)blockIdx.x,
                                                        (int)blockIdx.y, (int)blockIdx.z, (int)gridDim.z, As, Bs);
}

// ---- two independent products in ONE launch (and their split-K reductions in one more) -------------
// At the metric's shape the products of a minibatch are tiny (0.1 GFLOP): a launch costs more than the
// arithmetic, so the independent ones travel together.
template <typename T, class Epi> struct DenseProblem {
    DenseOperand A, B;
    int64_t M = 0, N = 0, K = 0, kps = 0;
    T *partial = nullptr;
    Epi epi;
    int tn = 0, tm = 0, splits = 1;
    int sym = 0;                                      // 1: out = A A^T (same operand twice, square tiles) with split-K - only the
                                                      // tiles on and above the diagonal are computed, the split-K sum mirrors them
                                                      // (bitwise symmetric, as the full product was: same k-ordered fma chain)
    __host__ __device__ int tiles() const { return sym ? tm * (tm + 1) / 2 : tn * tm; }
    bool ok = false;                                  // aligned: eligible for the dense kernels
    unsigned long long *dbg = nullptr;                // diagnostics: shader-clock stamps of the FIRST tile (resident-K variant)
};

// the sizes and the split are plan_dense_sizes' (gemm_plan.hpp); here the operands, the scratch and the epilogue are attached
template <typename T, class Epi>
DenseProblem<T, Epi> dense_problem(const DensePlan &d, const DenseOperand &A, const DenseOperand &B, int64_t M, int64_t N, int64_t K,
                                   const Epi &epi, T *ws) {
    DenseProblem<T, Epi> P;
    P.A = A; P.B = B; P.M = M; P.N = N; P.K = K; P.epi = epi;
    P.A.unal = d.unal_a; P.B.unal = d.unal_b;
    P.ok = d.ok;
    if (!P.ok) return P;
    P.kps = d.kps; P.splits = d.splits; P.tn = d.tn; P.tm = d.tm; P.sym = d.sym;
    P.partial = ws;
    return P;
}
template <typename T> bool dense_unaligned(const DenseOperand &o) {
    const int64_t ld = (o.si == 1) ? o.sk : o.si;
    return !((reinterpret_cast<uintptr_t>(o.ptr) % 16 == 0) && (ld % Vec4<T>::N == 0));
}
inline bool dense_contiguous(const DenseOperand &o) { return o.si == 1 || o.sk == 1; }

template <typename T, class Epi>
DenseProblem<T, Epi> plan_dense(const DenseOperand &A, const DenseOperand &B, int64_t M, int64_t N, int64_t K, const Epi &epi,
                                T *ws, size_t ws_elems, int target_wgs = 512, int max_splits = 64, int bm = 64, int bn = 64,
                                bool symmetric = false) {
    const bool same = A.ptr == B.ptr && A.si == B.si && A.sk == B.sk;
    return dense_problem<T, Epi>(plan_dense_sizes(sizeof(T), dense_contiguous(A) && dense_contiguous(B), dense_unaligned<T>(A),
                                                  dense_unaligned<T>(B), same, M, N, K, ws != nullptr, ws_elems, target_wgs, max_splits,
                                                  bm, bn, symmetric),
                                 A, B, M, N, K, epi, ws);
}

template <typename T, bool AI0, bool BI0, class Epi0, bool AI1, bool BI1, class Epi1, int BM1 = 64, int BN1 = 64, int BK1 = 0, int BM0 = 64,
          int BN0 = 64>
__global__ __launch_bounds__(256) void gemm_dense_pair_kernel(DenseProblem<T, Epi0> P0, DenseProblem<T, Epi1> P1) {
    constexpr int BM = BM0, BN = BN0, BK = (sizeof(T) == 4) ? 32 : 16;
    extern __shared__ __attribute__((aligned(16))) char gd_smem[];   // sized for the larger of the two tilings
    int id = (int)blockIdx.x;
    // tile number -> (column tile, row tile, split); a symmetric problem only has the tiles with bx >= by
    auto tile_of = [](int tid_, int tn_, int tm_, int sym_, int &bx_, int &by_, int &bz_) {
        if (sym_) {
            const int ut = tm_ * (tm_ + 1) / 2;
            bz_ = tid_ / ut;
            int rem = tid_ % ut, r = 0;
            while (rem >= tn_ - r) { rem -= tn_ - r; ++r; }
            by_ = r;
            bx_ = r + rem;
        } else {
            bx_ = tid_ % tn_;
            by_ = (tid_ / tn_) % tm_;
            bz_ = tid_ / (tn_ * tm_);
        }
    };
    const int t0 = P0.tiles() * P0.splits;
    if (id < t0) {
        T (*As)[BK][BM + 4] = reinterpret_cast<T (*)[BK][BM + 4]>(gd_smem);
        T (*Bs)[BK][BN + 4] = reinterpret_cast<T (*)[BK][BN + 4]>(gd_smem + sizeof(T) * 2 * BK * (BM + 4));
        int bx, by, bz;
        tile_of(id, P0.tn, P0.tm, P0.sym, bx, by, bz);
        gemm_dense_tile_auto<T, AI0, BI0, Epi0, BM, BN, BK>(P0.A, P0.B, P0.M, P0.N, P0.K, P0.kps, P0.partial, P0.epi, bx, by,
                                                            bz, P0.splits, As, Bs);
    } else {
        id -= t0;
        // XCD-aware order for the large problem: workgroups are dealt round-robin to the 8 XCDs (each with its
        // own L2), so the tiles that share an A row-tile are renumbered to land on ONE XCD and fetch it once
        const int t1 = P1.tiles() * P1.splits, chunk = (t1 + 7) / 8;
        id = (id % 8) * chunk + id / 8;
        if (id >= t1) return;
        constexpr int BKB = BK1 > 0 ? BK1 : BK;
        T (*As)[BKB][BM1 + 4] = reinterpret_cast<T (*)[BKB][BM1 + 4]>(gd_smem);
        T (*Bs)[BKB][BN1 + 4] = reinterpret_cast<T (*)[BKB][BN1 + 4]>(gd_smem + sizeof(T) * 2 * BKB * (BM1 + 4));
        int bx, by, bz;
        tile_of(id, P1.tn, P1.tm, P1.sym, bx, by, bz);
        gemm_dense_tile_auto<T, AI1, BI1, Epi1, BM1, BN1, BKB>(P1.A, P1.B, P1.M, P1.N, P1.K, P1.kps, P1.partial, P1.epi, bx,
                                                               by, bz, P1.splits, As, Bs, id == 0 ? P1.dbg : nullptr);
    }
}

// The sum of `splits` partial tiles at element e, in the order of the splits (the same bits as a plain loop), with the loads
// of eight splits in flight at once: as `v += partial[z]` in a loop every load was waited for before the next was requested -
// eight dependent round trips, the whole duration of the reduce launch of the code step (5 us for 2 x 256 x 256 outputs).
template <typename T>
__device__ __forceinline__ T sum_partials(const T *partial, int splits, int64_t stride, int64_t e) {
    T v = 0;
    int z = 0;
    for (; z + 8 <= splits; z += 8) {
        T x[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) x[u] = partial[(int64_t)(z + u) * stride + e];
#pragma unroll
        for (int u = 0; u < 8; ++u) v += x[u];
    }
    if (z < splits) {
        T x[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) x[u] = partial[(int64_t)((z + u < splits) ? z + u : splits - 1) * stride + e];
#pragma unroll
        for (int u = 0; u < 8; ++u) v += (z + u < splits) ? x[u] : (T)0;
    }
    return v;
}

template <typename T, class Epi0, class Epi1>
__global__ __launch_bounds__(256) void gemm_reduce_pair_kernel(const T *partial0, int splits0, int64_t M0, int64_t N0, Epi0 epi0,
                                                               int nblk0, const T *partial1, int splits1, int64_t M1,
                                                               int64_t N1, Epi1 epi1, int sym0, int sym1, int sh0 = 6,
                                                               int sh1 = 6) {
    // (a symmetric problem has partial sums only in its tiles on and above the diagonal, 2^sh x 2^sh: the element of a tile
    //  above the diagonal is summed once, with coalesced reads, and stored to both sides - bitwise symmetric)
    if ((int)blockIdx.x < nblk0) {
        const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
        if (e >= M0 * N0) return;
        const int64_t m = e / N0, n = e % N0;
        if (sym0 && (m >> sh0) > (n >> sh0)) return;
        const T v = sum_partials(partial0, splits0, M0 * N0, e);
        epi0(m, n, v);
        if (sym0 && (m >> sh0) < (n >> sh0)) epi0(n, m, v);
    } else {
        const int64_t e = (int64_t)((int)blockIdx.x - nblk0) * 256 + threadIdx.x;
        if (e >= M1 * N1) return;
        const int64_t m = e / N1, n = e % N1;
        if (sym1 && (m >> sh1) > (n >> sh1)) return;
        const T v = sum_partials(partial1, splits1, M1 * N1, e);
        epi1(m, n, v);
        if (sym1 && (m >> sh1) < (n >> sh1)) epi1(n, m, v);
    }
}

// Both problems must be `ok` (see plan_dense) and their operand orientations known statically; the second
// problem may use a larger block tile (BM1 x BN1, planned with the same values).
template <typename T, bool AI0, bool BI0, class Epi0, bool AI1, bool BI1, class Epi1, int BM1 = 64, int BN1 = 64, int BK1 = 0, int BM0 = 64,
          int BN0 = 64>
int launch_gemm_dense_pair(hipStream_t stream, const DenseProblem<T, Epi0> &P0, const DenseProblem<T, Epi1> &P1,
                           int *launches = nullptr) {
    constexpr int BK = (sizeof(T) == 4) ? 32 : 16;
    constexpr int BKB = BK1 > 0 ? BK1 : BK;
    constexpr size_t lds0 = sizeof(T) * 2 * BK * ((BM0 + 4) + (BN0 + 4)), lds1 = sizeof(T) * 2 * BKB * ((BM1 + 4) + (BN1 + 4));
    constexpr size_t lds = lds0 > lds1 ? lds0 : lds1;
    const int total = P0.tiles() * P0.splits + 8 * ((P1.tiles() * P1.splits + 7) / 8);   // second problem padded to 8 XCD chunks
    auto kern = gemm_dense_pair_kernel<T, AI0, BI0, Epi0, AI1, BI1, Epi1, BM1, BN1, BK1, BM0, BN0>;
    if (lds > 64 * 1024)
        MODL_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)total), dim3(256), lds, stream, P0, P1);
    MODL_LAUNCH_CHECK();
    if (launches) ++*launches;
    const int nb0 = P0.splits > 1 ? (int)cdiv(P0.M * P0.N, 256) : 0, nb1 = P1.splits > 1 ? (int)cdiv(P1.M * P1.N, 256) : 0;
    if (nb0 + nb1 > 0) {
        hipLaunchKernelGGL((gemm_reduce_pair_kernel<T, Epi0, Epi1>), dim3((unsigned)(nb0 + nb1)), dim3(256), 0, stream,
                           P0.partial, P0.splits, P0.M, P0.N, P0.epi, nb0, P1.partial, P1.splits, P1.M, P1.N, P1.epi, P0.sym, P1.sym,
                           BM0 == 128 ? 7 : 6, BM1 == 128 ? 7 : 6);
        MODL_LAUNCH_CHECK();
        if (launches) ++*launches;
    }
    return MODL_OK;
}

// ---- the statistics products (f32, K = minibatch <= 256, both operands contiguous along their rows) ------------
// 32 x 32 workgroup tiles of v_mfma_f32_16x16x4 (one 16 x 16 tile per wavefront) through the resident-K tile: four
// times the workgroups of the 64 x 64 tiling and a quarter of the matrix-core work per wavefront.  These products
// are latency-bound per tile, not throughput-bound (the head of the increment is 80 tiles of 64 x 64 on a
// 256-CU chip), so the tile's critical path is what counts.  Same pairing / XCD renumbering as above.

template <class Epi>
__device__ __forceinline__ void gemm_stats_tile(const DenseProblem<float, Epi> &P, int id, char *smem,
                                                unsigned long long *dbg = nullptr) {
    constexpr int B = kStatsTile, BK = kStatsBK;
    float (*As)[BK][B + 4] = reinterpret_cast<float (*)[BK][B + 4]>(smem);
    float (*Bs)[BK][B + 4] = reinterpret_cast<float (*)[BK][B + 4]>(smem + sizeof(float) * 2 * BK * (B + 4));
    const int bx = id % P.tn, by = id / P.tn;
    gemm_dense_tile_rk<float, true, true, Epi, B, B, BK, kStatsNKT, Mma16f>(P.A, P.B, P.M, P.N, 0, P.K, nullptr, P.epi, bx, by,
                                                                            0, 1, As, Bs, dbg);
}
constexpr size_t kStatsLds = sizeof(float) * 2 * kStatsBK * (kStatsTile + 4) * 2;

template <class Epi0, class Epi1>
__global__ __launch_bounds__(256) void gemm_stats_pair_kernel(DenseProblem<float, Epi0> P0, DenseProblem<float, Epi1> P1) {
    __shared__ __attribute__((aligned(16))) char smem[kStatsLds];
    int id = (int)blockIdx.x;
    const int t0 = P0.tn * P0.tm;
    if (id < t0) {
        gemm_stats_tile<Epi0>(P0, id, smem);
    } else {
        id -= t0;
        const int t1 = P1.tn * P1.tm, chunk = (t1 + 7) / 8;               // XCD-aware order, as in gemm_dense_pair_kernel
        id = (id % 8) * chunk + id / 8;
        if (id >= t1) return;
        gemm_stats_tile<Epi1>(P1, id, smem, id == 0 ? P1.dbg : nullptr);
    }
}

// eligible: f32 (the only instantiation), K <= 256, both operands row-contiguous and aligned (plan with 32 x 32 tiles)
template <class Epi>
DenseProblem<float, Epi> plan_stats(const DenseOperand &A, const DenseOperand &B, int64_t M, int64_t N, int64_t K,
                                    const Epi &epi) {
    DenseProblem<float, Epi> P;
    if (M > 0 && N > 0) P = plan_dense<float, Epi>(A, B, M, N, K, epi, nullptr, 0, 512, 1, kStatsTile, kStatsTile);
    P.epi = epi;
    P.ok = plan_stats_ok(A.si == 1 && B.si == 1, dense_unaligned<float>(A), dense_unaligned<float>(B), M, N, K);
    return P;
}

template <class Epi0, class Epi1>
int launch_gemm_stats_pair(hipStream_t stream, const DenseProblem<float, Epi0> &P0, const DenseProblem<float, Epi1> &P1,
                           int *launches = nullptr) {
    const int total = P0.tn * P0.tm + 8 * ((P1.tn * P1.tm + 7) / 8);
    if (total <= 0) return MODL_OK;
    hipLaunchKernelGGL((gemm_stats_pair_kernel<Epi0, Epi1>), dim3((unsigned)total), dim3(256), 0, stream, P0, P1);
    MODL_LAUNCH_CHECK();
    if (launches) ++*launches;
    return MODL_OK;
}

// Dense launcher.  Requires 16-byte aligned bases and leading strides that keep every vector
// aligned; otherwise falls back to the generic gather kernel (gemm.hpp).
// ... as plan_product (gemm_plan.hpp) planned it with this scratch: a caller that has the plan already launches from it
template <typename T, class Epi>
int launch_product(hipStream_t stream, const ProductLaunch &L, const DenseOperand &A, const DenseOperand &B, int64_t M, int64_t N,
                   int64_t K, const Epi &epi, const SplitWs &ws, int *launches = nullptr) {
    if (M <= 0 || N <= 0) return MODL_OK;
    if (!L.dense) {
        Operand a, b;
        a.ptr = A.ptr; a.si = A.si; a.sk = A.sk;
        b.ptr = B.ptr; b.si = B.si; b.sk = B.sk;
        return launch_gemm_planned<T, Epi>(stream, L.g, a, b, M, N, K, epi, ws, launches);
    }
    const DenseProblem<T, Epi> P = dense_problem<T, Epi>(L.d, A, B, M, N, K, epi, static_cast<T *>(ws.ptr));
    dim3 grid((unsigned)P.tn, (unsigned)P.tm, (unsigned)P.splits);
    const bool ai = A.si == 1, bi = B.si == 1;
#define MODL_GD(AI, BI) \
    hipLaunchKernelGGL((gemm_dense_kernel<T, AI, BI, Epi>), grid, dim3(256), 0, stream, P.A, P.B, M, N, K, P.kps, P.partial, epi)
    if (ai && bi) MODL_GD(true, true);
    else if (ai) MODL_GD(true, false);
    else if (bi) MODL_GD(false, true);
    else MODL_GD(false, false);
#undef MODL_GD
    MODL_LAUNCH_CHECK();
    if (launches) ++*launches;
    if (P.splits > 1) {
        hipLaunchKernelGGL((gemm_reduce_kernel<T, Epi>), dim3((unsigned)cdiv(M * N, 256)), dim3(256), 0, stream,
                           P.partial, P.splits, M, N, epi);
        MODL_LAUNCH_CHECK();
        if (launches) ++*launches;
    }
    return MODL_OK;
}
template <typename T, class Epi>
int launch_gemm_dense(hipStream_t stream, const DenseOperand &A, const DenseOperand &B, int64_t M, int64_t N, int64_t K,
                      const Epi &epi, const SplitWs &ws, int *launches = nullptr, int target_wgs = 512,
                      int max_splits = 64) {
    if (M <= 0 || N <= 0) return MODL_OK;
    return launch_product<T, Epi>(stream,
                                  plan_product(sizeof(T), dense_contiguous(A) && dense_contiguous(B), dense_unaligned<T>(A),
                                               dense_unaligned<T>(B), M, N, K, ws.ptr != nullptr, ws.bytes / sizeof(T), target_wgs, max_splits),
                                  A, B, M, N, K, epi, ws, launches);
}

// ---- compaction kernels -------------------------------------------------------
// dst[r][0..cols) = src[idx[r]][0..cols)   (rows r >= n_rows of the padded destination are zero)
template <typename T, typename I>
__global__ __launch_bounds__(256) void gather_rows_T_kernel(const T *src, int64_t src_ld, const I *idx, int64_t n_rows,
                                                            int64_t n_rows_pad, int64_t cols, T *dst, int64_t dst_ld) {
    const int64_t r = blockIdx.x;
    if (r >= n_rows_pad) return;
    T *d = dst + r * dst_ld;
    if (r < n_rows) {
        const T *s = src + (int64_t)idx[r] * src_ld;
        for (int64_t c = threadIdx.x; c < cols; c += 256) d[c] = s[c];
    } else {
        for (int64_t c = threadIdx.x; c < cols; c += 256) d[c] = 0;
    }
}
// src[idx[r]][0..cols) = dst-compact[r][0..cols)
template <typename T, typename I>
__global__ __launch_bounds__(256) void scatter_rows_T_kernel(T *dst, int64_t dst_ld, const I *idx, int64_t n_rows,
                                                             int64_t cols, const T *src, int64_t src_ld) {
    const int64_t r = blockIdx.x;
    if (r >= n_rows) return;
    T *d = dst + (int64_t)idx[r] * dst_ld;
    const T *s = src + r * src_ld;
    for (int64_t c = threadIdx.x; c < cols; c += 256) d[c] = s[c];
}
}  // namespace modl
