"""The matrix-core products (modl_amd/csrc/gemm.hpp, gemm_dense.hpp, gemm_wide.hpp, gemm_resident.hpp and their dispatch in
modl_amd/csrc/somf_step.hip) route by route, through three probes that expose a product from outside the C ABI (modl_amd._lib:
SomfDesc, SomfState, SomfBatch on torch device tensors, plans created and destroyed here), against the same product in
np.longdouble, element by element.

PROBES
  T  modl_somf_transform with a caller's G = 0, code_l1_ratio = 0, code_alpha = 1: the ridge system is the identity, code_out is
     Dx = X D^T of launch_gemm_dense<EpiStore> (M = b, N = k, K = p; A contiguous along K, B = Dt along N).
     `test_probe_is_transparent`: on the integer scene the codes ARE the integers, so the solve adds nothing there; the
     Gaussian judge allows the probe 4 eps |Dx| on top of the product's bound.
  G  modl_somf_full_gram: G = D D^T by the gather kernel (A = B = Dt, K = p, split-K through the plan's scratch).
  S  one modl_somf_step (three in a row where stated) from a state written here (C0 a random symmetric positive definite
     matrix - the dictionary update divides by its diagonal -, B0, code rows and averages random, finite, non-zero):
     S-code/average  G_agg = Dx_agg = average, ridge codes, n_samples = b + 3, h_sample_idx a permutation, w_sample 1 on
                     half the rows and 0.25 on the others:  Dx_average[idx[i]] = (1 - ws_i) old + ws_i reduction X_S D_S^T
                     (EpiDxAverage), G_average[idx[i]] = (1 - ws_i) old_i + ws_i reduction D_S D_S^T - the paired launch, the
                     prep_kernel gathers and the mirrored symmetric Gram read from outside.  D is the dictionary before the step.
     S-code/full     G_agg = Dx_agg = full, s < p / 2:  G_ = G0 - D0_S D0_S^T + D1_S D1_S^T (gram_of_rows with the subset on
                     the contraction index, EpiAxpby, the split-K reduce); D0, D1 read from the device before / after.
     S-stats         default aggregation (masked), ridge (dense) codes, w = 0.37, b_global = b:  C_ = (1 - w) C0 + (w / b)
                     code^T code and every row f of B_ = (1 - w) B0[f] + (w / b) sum_i code_i X[i, f], from the device's
                     own code_[idx] after the step - the solve is not under test, the product is.

ROUTES (`ROUTES`; `test_route_table` holds every point to `expected_route`, a restatement of the planners, and every leaf of
the restated cascade to at least one point; the same table is in DESIGN.md, section 22).  A leaf is a branch of the
restatement, marked where it is taken by a call of `_leaf`; the list of all leaves is read out of this file's own text, so a
branch cannot be written down and left out.  A probe vouches only for the section whose result it judges: the statistics
section of an S-code point does not count.  `UNREACHED` lists, with the reason, the branches that no point takes.  The restatement
is held, whole string by whole string, against the library's own answer (modl_somf_product_route: the planners of gemm_plan.hpp and
the three route functions of step_products.hip, which somf_step.hip and bcd.hip launch from), at every point and on both sides of
every numeric boundary (`test_route_table`, `test_route_boundaries`), on the CPU.  Functions are cited by name, in modl_amd/csrc.
  plan_dense_sizes       operand misaligned = base % 16 bytes or leading stride % (16 / sizeof T) (dense_unaligned); misaligned and
                         M N K < 2^22 -> not ok, the gather kernel; tiles bm x bn, BK = 32 (f32) / 16 (f64);
                         splits = min(target / tiles, max(1, K / (4 BK)), max_splits, scratch / (M N)) when tiles < target and
                         there is scratch; kps = ceil(ceil(K / splits) / BK) BK, splits = ceil(K / kps); sym = same operand
                         twice, square, and splits > 1: tm (tm + 1) / 2 tiles, the reduce mirrors them (gemm_reduce_pair_kernel)
  dense_tile_of          paired launches only: the resident-K tile when sizeof(T) == 4, tiles <= 64 x 64 and the split's
                         length <= 8 BK, else the pipelined tile - decided split by split (gemm_dense_tile_auto), so a short last split
                         of a long contraction takes the resident-K tile next to pipelined ones ("pipe+rk_last");
                         launch_gemm_dense's own kernel is always pipelined (gemm_dense_kernel)
  TileLoader             a tile inside an aligned operand by 16-byte loads, every other (edge, K tail, misaligned operand)
                         element by element, a lane outside the operand from element [0, 0], zeros selected afterwards
  plan_gather            tall 128 x 32 (BK 32) when N <= 32, big 128 x 128 when ceil(M/128) ceil(N/128) >= 512, else small
                         64 x 64 (BK 16); splits = min(target / tiles, max(1, K / 128), max_splits, scratch / (M N)); tall tiles at
                         least half full, no gather on K: "dense" staging from clamped coordinates (gemm_kernel, stage_tile)
  plan_stats_ok          f32, 32 x 32 tiles of 16x16x4, K <= 256, no split (resident-K tile, 4 K-tiles of 64)
  plan_wide_ok           16-byte aligned operands, M, N, leading strides % 4 == 0, K <= 256
  stats_route            f32: resident (plan_stats(C) ok, rows >= 4096, k <= 256, b % 4 == 0, switch on, plan_wide ok; the
                         epilogue by 16 bytes for EpiStats, element by element for the row-indirected EpiStatsRows), else
                         wide pair (ceil(rows / 64) >= 1024, plan_wide ok: 32 features x 256 atoms per tile), else stats pair
                         (both plan_stats ok); any type: dense pair (both plan_dense ok, no split), else one launch each
                         (launch_gemm_dense: dense kernel, or gather kernel below 2^22)
  code_products_route    need_sub = subset and not (G_agg == Dx_agg == full): prep_kernel gathers Ds = Dt[subset], Xs = X[:, subset]
                         (s_pad = ceil(s / 4) 4 columns); paired = G wanted and both plan_dense ok with 256 workgroups and
                         half the scratch each, the Gram symmetric; else one launch_gemm_dense each
  rider_route            a proper subset, Dx_agg != full, no MODL_FLAG_NO_RIDER, ceil(p / 64) < 1024: C_ and the sampled rows
                         of B_ (EpiStatsRows) now, the others under the dictionary update
                         the update's launches carry it (du_carries_riders: f32, k <= 512, no l1, not sgd): wide tiles 32 x 128 when p >= 2048 and plan_wide ok, else the 32 x 32 tiles of
                         plan_stats, shared out over the carrier launches; otherwise completed after the update (phase2)
                         through stats_pair with EpiStatsSkip
The launches of the code-product and statistics sections (modl_somf_prof_get: code_gemm, stats_gemm) are asserted against the
restated count on every S point: paired or not, split or not.  A rider that the dictionary update did not consume is completed
behind it and counted under dict_update: on the f64 riding points that section has exactly stats_pair's launches for B_ alone
more than the same step under MODL_FLAG_NO_RIDER (asserted).  The tiles of an f32 rider run inside the dictionary update's
launches and are not counted: that they ran is seen in the rows of B_, which tile they took rests on `test_route_table`.

  T dense interior              b 64 k 64 p 96                      T dense edge, K tail, no split   b 70 k 68 p 200
  T dense split-K               b 70 k 68 p 1000 (7 x 160, last 40) T f64 dense split                b 70 k 66 p 500 (7 x 80, last 20)
  T misaligned Dt stride        b 128 k 130 p 260 (B.unal, 2 splits; f64 k 129 p 257)
  T misaligned ldx / base       b 128 k 128 p 257, ldx 258 / a view one element into a buffer with ldx 260 (f64: base)
  T gather small, split         b 64 k 70 p 300 (160 + 140)         T gather tall                    b 200 / 130 k 30 p 333 (f64 k 31)
  T chunks                      max_batch 64, n 67                  T minimal                        b = k = p = 1
  G tall general / half / full  k 12 p 50, k 16 p 300, k 32 p 300   G small K tail / deep split      k 33 p 40, k 70 p 3000 (20 x 144 + 120)
  G big 128 x 128 (f32)         k 2820 p 24 (23 x 23 tiles)         G f64                            k 12, 33, 70
  S-code paired                 b 64 k 64 p 512 s 256; b 50 k 132 p 700 s 600 / 597 / 100; f64 b 50 k 66 p 400 s 300
  S-code paired, long splits    b 50 k 132 p 9600 s 9000 (32 x 288, last 72: pipelined tiles, the last split resident-K, mirrored),
                                s 9200 (last 272: pipelined throughout) - the tiles a production-sized subset takes in f32
  S-code unpaired (gather)      b 20 k 30 p 120 s 60                S-code reduction 1               no subset array, ldx > p
  S-code full                   k 70 p 900 s 300; k 24 p 200 s 64
  S-stats 32 x 32               (b, k, p) = (64, 64, 300), (50, 64, 300), (256, 64, 300), (64, 68, 300)
  S-stats dense pair / gather   b 260; k 30; k 30 p 3000 (misaligned dense kernel for B_)
  S-stats riding                p 600 s 200 (32 x 32 rider), p 2400 s 800 (wide rider), p 2402 (32 x 32 again), NO_RIDER,
                                p 65476 s 800 (ceil(p / 64) = 1024: no rider, resident)
  S-stats resident              p 4096, p 4100, k 36, b 20, p 16416 s 5472 (row-indirected), b 22 (not resident), switch off
  S-stats wide pair             p 65476 k 260 b 24 (two atom chunks), k 32 b 50, p 65474 (32 x 32, misaligned)
  S-stats f64                   dense pair b 50 k 66 p 300; riding p 600 s 200 (completed after the update; k 31: by the gather
                                kernel); k 31 gather
  S-stats sgd; three steps      p 600 s 200 (and p 2400 s 800, the wide rider), overlapping subsets, judged after each step
Not reachable from the ABI: the big configuration in f64 (k > 2048 would need 8 k^2 64 bytes of scratch - run in f32 only, as the
issue lists it); the "dense" staging of the A operand in probe G (M = N <= 32 there; probe T's b = 200 covers it).
Not reached by these probes (`UNREACHED`): a subset with Dx_agg = full and G_agg != full (rider_route then denies the rider); the
probes set G_agg = Dx_agg, which their formulas assume.

SCENES
  integers   X, D uniform in {-3 .. 3}, old averages integer multiples of 4, reduction 2 or 4 passed as given: every partial sum
             is exact in either type in any order.  T, G and S-code/average return the exact integers bitwise (but for the sign of
             zero); G and every G_average row are bitwise symmetric.  S-code/full: D1 is not integer; there the scene asserts the
             bitwise symmetry of G_ and the bound.  Every point of those probes.
  gaussian   the control, every point.
  scales     rows of X and atoms of D scaled by 10^U(-3, 3) (f64: 10^U(-6, 6)); representative points (`rep`).
  poison     NaN in the ldx - p padding columns of X, the rows behind the batch in the X buffer, the rows of code_ and of the
             averages outside idx, a row behind Dt: the bits of the same call without the poison (those places then hold
             finite values); rows outside idx keep their bits.  Every point.
  nan_row    (T, S-code/average) one row of X NaN: only that row of the result is non-finite, every other row keeps its bits.
             It is row 0: element [0, 0] is what the dense TileLoader fetches for a lane outside the operand, so every
             K-tail lane of every other row loads a NaN that must be selected away - the poison cannot reach that loader.
  Every case: a second identical call (a fresh plan, the same state) gives identical bits.

JUDGES
  exact   as above.
  bound   |got - ref| <= (K + S + 6) eps A per element: ref in np.longdouble from the inputs as given, K the contraction
          length, S the number of splits, A the same expression with every term replaced by its absolute value (sum |a||b| |scale|,
          plus |beta old| for the read-modify-write epilogues).  The a-priori bound of a floating-point sum in any order (K - 1
          additions of the chain or tree, S - 1 of the split sum, and at most six roundings of scale factors and the epilogue);
          nothing of the code under test enters it.  S-code/full is two passes over G_, K = s and S the splits of one pass:
          every term of G0 - D0_S D0_S^T + D1_S D1_S^T sees s - 1 + S - 1 additions of its own product and two roundings in
          each epilogue.
  `test_judges_on_the_oracle` (CPU): numpy's same-dtype product stays under 1 / 8 of the bound on every scene, and one dropped
  term (the largest of each element) exceeds it at every K of the table.  Only the largest: at K = 3000 or 9000 in f32 a
  typical term, A / K, is already below the bound, which grows with K.  What catches ONE dropped term at a large K is the
  integer scene, exact at every K; the bound catches a dropped tile, split or K tail.

MEASURED (largest |got - ref| / bound per route on the MI355X, f32 / f64, from this file's own run - `_report` prints them;
recorded, not asserted; a point with a rider is filed under the route of its head launch).  69 GPU cases in 16 s.
  T dense 0.016 / 0.0013              T misaligned 0.0076 / 0.0031          T gather 0.016 / 0.021       G gather 0.089 (big tiles) / 0.049
  S-code paired Dx 0.010 / 0.0031, G 0.022 / 0.0080 (the long splits no worse)   S-code unpaired Dx 0.020, G 0.041   S-code full 0.027 / 0.026
  S-stats 32 x 32 (and its riders) B 0.060, C 0.046                      S-stats dense pair B 0.013 / 0.066, C 0.018 / 0.058
  S-stats gather B 0.061 / 0.016, C 0.057 / 0.0082                       S-stats misaligned dense B 0.057, C 0.037
  S-stats resident B 0.073, C 0.033                                      S-stats wide pair B 0.135, C 0.065
  numpy's same-dtype product on the CPU (`test_judges_on_the_oracle`): at most 0.053 / 0.053 of the bound.

MUTANTS (`test_mutants`, on `tiled_product` and `stats_step`, numpy restatements of the tile / split / mirror loops and of the
riding statistics update).  Mutant -> the scene and judge that reject it:
  K tail of the last split dropped                    integers (exact)
  last split read as a full split                     integers (exact: the columns behind K hold other numbers), poison
  edge tile rows wrapped instead of zero-filled       gaussian (bound) under a read-modify-write epilogue: the wrapped row is
                                                      updated twice.  INVISIBLE under a plain store (asserted)
  zeros multiplied instead of selected                poison.  INVISIBLE while the places hold finite values (asserted), and in a
                                                      loader that fetches its outside lanes from element [0, 0] (asserted): there
                                                      nan_row with the NaN in row 0
  a tile below the diagonal left unmirrored           integers (exact)
  mirror written from the wrong split sum             gaussian (bitwise symmetry).  INVISIBLE on integers (asserted)
  one split's partial added twice                     integers (exact)
  a stamped row updated twice                         gaussian (bound), three steps
  an unstamped row skipped                            gaussian (bound)
  rows[m] ignored in the row-indirected epilogue      gaussian (bound)
  (1 - w) old dropped                                 gaussian (bound) at w = 0.37.  INVISIBLE at w = 1 (asserted)
"""
import zlib
from types import SimpleNamespace

import numpy as np
import pytest

DT = {'f32': np.float32, 'f64': np.float64}
LD = np.longdouble
TSZ = {'f32': 4, 'f64': 8}
VN = {'f32': 4, 'f64': 2}                      # elements of a 16-byte vector (Vec4<T>::N)
BKD = {'f32': 32, 'f64': 16}                   # K-tile of the dense kernels (dense_bk)
FILL = 7.5
NO_RIDER = 1                                   # MODL_FLAG_NO_RIDER
GEMM_STAMPS = 2                                # MODL_FLAG_GEMM_STAMPS


def cdiv(a, b):
    return -(-a // b)


HIT = set()                                    # the branches of the restated dispatch taken since the last HIT.clear()


def _leaf(name):
    """Marks a branch of the restatement.  `all_leaves` reads the names out of this file's own text, so a branch that is
    written down here cannot be left out of the completeness assertion of `test_route_table`."""
    HIT.add(name)
    return name


def all_leaves():
    import re
    with open(__file__.replace('.pyc', '.py')) as f:
        return set(re.findall(r"_leaf\('([^']+)'\)", f.read()))


# ---------------------------------------------------------------------------------------------------- the dispatch, restated
def split_scratch_elems(mb, k, p):             # split_scratch_elems
    e = max(mb, k) * k * 64
    if p * k < e:
        e = max(e, p * k * 8)
    return e


def misaligned(dt, ld, base=0):                # dense_unaligned (base: offset of the operand in elements from an aligned address)
    return (base * TSZ[dt]) % 16 != 0 or ld % VN[dt] != 0


def plan_dense(dt, unal_a, unal_b, M, N, K, ws, target=512, max_splits=64, bm=64, bn=64, symmetric=False):
    """plan_dense_sizes.  ws: elements of split-K scratch (0: none)."""
    P = SimpleNamespace(ok=K > 0 and M > 0 and N > 0, unal_a=unal_a, unal_b=unal_b, M=M, N=N, K=K, splits=1, kps=0, sym=0, tm=0,
                        tn=0, bm=bm, bn=bn)
    if not P.ok:
        return P
    if (unal_a or unal_b) and M * N * K < 1 << 22:
        _leaf('plan_dense: misaligned below 2^22, not ok')
        P.ok = False
        return P
    _leaf('plan_dense: misaligned at or above 2^22') if unal_a or unal_b else _leaf('plan_dense: aligned')
    BK = BKD[dt]
    tm, tn = cdiv(M, bm), cdiv(N, bn)
    sym = symmetric and M == N and bm == bn
    ntile = tm * (tm + 1) // 2 if sym else tm * tn
    splits = 1
    if ntile < target and max_splits > 1 and ws > 0:
        splits = min(target // ntile, max(1, K // (4 * BK)), max_splits, ws // (M * N))
        splits = max(splits, 1)
    P.kps = cdiv(cdiv(K, splits), BK) * BK
    P.splits = cdiv(K, P.kps)
    P.tm, P.tn = tm, tn
    P.sym = 1 if sym and P.splits > 1 else 0
    _leaf('plan_dense: split-K') if P.splits > 1 else _leaf('plan_dense: one split')
    if sym:
        _leaf('plan_dense: symmetric, upper tiles mirrored') if P.sym else _leaf('plan_dense: symmetric but unsplit, every tile computed')
    P.tiles = tm * (tm + 1) // 2 if P.sym else tm * tn
    return P


def dense_tile(dt, P, paired):                 # dense_tile_of; launch_gemm_dense's own kernel is pipelined
    if not paired:
        _leaf('tile: pipelined (a launch of its own)')
        return 'pipe'
    if dt != 'f32' or P.bm > 64 or P.bn > 64:
        _leaf('tile: pipelined (paired, f64)')
        return 'pipe'
    last = P.K - (P.splits - 1) * P.kps
    if P.kps <= 8 * BKD[dt]:
        _leaf('tile: resident-K (paired, f32, splits of at most 8 BK)')
        return 'rk'
    if P.splits > 1 and last <= 8 * BKD[dt]:                              # gemm_dense_tile_auto decides split by split
        _leaf('tile: pipelined, the short last split resident-K (paired, f32)')
        return 'pipe+rk_last'
    _leaf('tile: pipelined (paired, f32, every split longer than 8 BK)')
    return 'pipe'


def splits_str(K, splits, kps):
    return 's%d/kps%d/last%d' % (splits, kps, K - (splits - 1) * kps)


def dense_str(dt, P, paired):
    al = 'al' if not (P.unal_a or P.unal_b) else 'unal' + ('A' if P.unal_a else '') + ('B' if P.unal_b else '')
    last = P.K - (P.splits - 1) * P.kps
    edge = P.M % P.bm or P.N % P.bn or P.kps % BKD[dt] or last % BKD[dt]
    _leaf('dense: edge tiles or a K tail') if edge else _leaf('dense: interior tiles only')
    if P.unal_a:
        _leaf('dense: A staged element by element')
    if P.unal_b:
        _leaf('dense: B staged element by element')
    s = 'dense/%s/t%dx%d/%s/%s/%s' % (al, P.tm, P.tn, 'edge' if edge else 'interior', splits_str(P.K, P.splits, P.kps),
                                      dense_tile(dt, P, paired))
    return s + ('/sym1/ut%d' % P.tiles if P.sym else '/sym0')


def launch_gemm(dt, M, N, K, ws, target=512, max_splits=64, gather_k=False):
    """plan_gather and the staging predicate of gemm_kernel: (route string, launches, splits)."""
    if N <= 32:
        cfg, bm, bn, bk = 'tall', 128, 32, 32
    elif cdiv(M, 128) * cdiv(N, 128) >= 512:
        cfg, bm, bn, bk = 'big', 128, 128, 16
    else:
        cfg, bm, bn, bk = 'small', 64, 64, 16
    _leaf('gather: tall') if cfg == 'tall' else _leaf('gather: big') if cfg == 'big' else _leaf('gather: small')
    tm, tn = cdiv(M, bm), cdiv(N, bn)
    splits = 1
    if K > 0 and tm * tn < target and max_splits > 1 and ws > 0:
        splits = max(1, min(target // (tm * tn), max(1, K // (8 * 16)), max_splits, ws // (M * N)))
    kps = cdiv(cdiv(max(K, 1), splits), bk) * bk
    splits = cdiv(max(K, 1), kps)
    _leaf('gather: split-K') if splits > 1 else _leaf('gather: one split')
    if kps % bk or (K - (splits - 1) * kps) % bk:
        _leaf('gather: K tail')
    if cfg == 'tall' and not gather_k:
        sa = ''.join('d' if 2 * (M - m0) >= bm else 'g' for m0 in range(0, M, bm))
        sb = ''.join('d' if 2 * (N - n0) >= bn else 'g' for n0 in range(0, N, bn))
        _leaf('tall: A tile dense') if 'd' in sa else None
        _leaf('tall: A tile general') if 'g' in sa else None
        _leaf('tall: B tile dense') if 'd' in sb else None
        _leaf('tall: B tile general') if 'g' in sb else None
    elif cfg == 'tall':
        _leaf('tall: gather on K, general staging')
        sa, sb = 'g', 'g'
    else:
        _leaf('small / big: general staging')
        sa, sb = 'g', 'g'
    s = 'gather/%s/t%dx%d/%s/A%s/B%s' % (cfg, tm, tn, splits_str(K, splits, kps), sa, sb)
    return s, 1 + (splits > 1), splits


def launch_gemm_dense(dt, unal_a, unal_b, M, N, K, ws, target=512, max_splits=64):
    """launch_gemm_dense / product_launch: (route string, launches, splits)"""
    P = plan_dense(dt, unal_a, unal_b, M, N, K, ws, target, max_splits)
    if not P.ok:
        _leaf('launch_gemm_dense: gather kernel')
        return launch_gemm(dt, M, N, K, ws, target, max_splits)
    _leaf('launch_gemm_dense: dense kernel')
    return dense_str(dt, P, False), 1 + (P.splits > 1), P.splits


def plan_stats_ok(dt, unal_a, unal_b, M, N, K):                           # plan_stats_ok (both operands row-contiguous here)
    if M <= 0 or N <= 0:
        return True
    return plan_dense(dt, unal_a, unal_b, M, N, K, 0, 512, 1, 32, 32).ok and K <= 256


def plan_wide_ok(M, N, K, ld_a, ld_b, base_a=0):                          # plan_wide_ok
    return M > 0 and N > 0 and 0 < K <= 256 and M % 4 == 0 and N % 4 == 0 and ld_a % 4 == 0 and ld_b % 4 == 0 and \
        (base_a * 4) % 16 == 0


def stats_pair(dt, k, M1, ld1, base1, K, ws, epi='stats', M0=None, resident=True, stamps=False):
    """stats_route: the products code^T code (M0 = k rows; 0: none) and X^T code (M1 rows of leading stride ld1) -> (route, launches)"""
    M0 = k if M0 is None else M0
    unal_c, unal_x = misaligned(dt, k), misaligned(dt, ld1, base1)
    if dt == 'f32':
        p0 = plan_stats_ok(dt, unal_c, unal_c, M0, k, K)
        if p0 and M1 >= 4096 and k <= 256 and K % 4 == 0 and not stamps and resident and plan_wide_ok(M1, k, K, ld1, k, base1):
            _leaf('resident: vec4 epilogue') if epi == 'stats' else _leaf('resident: scalar row-indirected epilogue')
            return 'resident16/%s' % ('vec4' if epi == 'stats' else 'scalar'), 1
        if p0 and cdiv(M1, 64) >= 1024 and not stamps and plan_wide_ok(M1, k, K, ld1, k, base1):
            _leaf('wide pair: one atom chunk') if k <= 256 else _leaf('wide pair: several atom chunks')
            return 'wide32/c%d' % cdiv(k, 256), 1
        if p0 and plan_stats_ok(dt, unal_x, unal_c, M1, k, K):
            _leaf('stats pair: misaligned') if unal_x or unal_c else _leaf('stats pair: aligned')
            return 'stats32/%s/t%dx%d' % ('unal' if unal_x or unal_c else 'al', cdiv(M1, 32), cdiv(k, 32)), 1
    ok0 = True
    if M0 > 0:
        ok0 = plan_dense(dt, unal_c, unal_c, M0, k, K, 0).ok
    P1 = plan_dense(dt, unal_x, unal_c, M1, k, K, 0, 512, 1, 64, 64)
    if ok0 and P1.ok:
        _leaf('dense pair: C and B') if M0 > 0 else _leaf('dense pair: B alone (after the update)')
        return 'densepair/%s/%s' % ('unal' if unal_x or unal_c else 'al', dense_tile(dt, P1, True)), 1
    n, parts = 0, []
    _leaf('one launch each: C and B') if M0 > 0 else _leaf('one launch each: B alone (after the update)')
    if M0 > 0:
        s, l, _ = launch_gemm_dense(dt, unal_c, unal_c, M0, k, K, ws)
        parts.append('C[%s]' % s)
        n += l
    s, l, _ = launch_gemm_dense(dt, unal_x, unal_c, M1, k, K, ws)
    parts.append('B[%s]' % s)
    return 'each/' + '/'.join(parts), n + l


def phase1(dt, b, k, p, s, subset, G_agg, Dx_agg, ldx, mb, flags=0, xbase=0, resident=True, has_idx=True, judged=('code', 'stats'),
           optimizer='variational'):
    """code_products_route and phase1's statistics section for ridge codes (no row norms, codes solved in place): the code-product and statistics sections.  Only the
    branches of the sections in `judged` count as taken (HIT): a probe vouches for the section whose result it judges."""
    taken, mine = set(HIT), {}
    HIT.clear()
    ws = split_scratch_elems(mb, k, p)
    full = G_agg == 'full' and Dx_agg == 'full'
    need_sub = subset and not full
    s_pad = cdiv(s, 4) * 4
    n = 0
    if need_sub and s > 0:                                                   # (n_norm = n_code = 0 for ridge codes)
        _leaf('phase1: prep_kernel gathers Ds and Xs')
        n += 1
    unal_d = misaligned(dt, k)
    if Dx_agg == 'full':
        _leaf('phase1: Dx over all of p')
        unal_a, Kdim = misaligned(dt, ldx, xbase), p
    elif need_sub:
        _leaf('phase1: Dx over the gathered columns')
        unal_a, Kdim = misaligned(dt, s_pad), s
    else:
        _leaf('phase1: Dx over X as given (no subset)')
        unal_a, Kdim = misaligned(dt, ldx, xbase), s
    want_G, paired = G_agg != 'full', False
    if want_G:
        half = ws // 2
        PG = plan_dense(dt, unal_d, unal_d, k, k, s, ws - half, 256, 64, 64, 64, True)
        PD = plan_dense(dt, unal_a, unal_d, b, k, Kdim, half, 256)
        if PD.ok and PG.ok:
            _leaf('phase1: Dx and G paired')
            paired = True
            code = 'pair/Dx[%s]/G[%s]' % (dense_str(dt, PD, True), dense_str(dt, PG, True))
            n += 1 + (PD.splits > 1 or PG.splits > 1)
            splits = (PD.splits, PG.splits)
    if not paired:
        sd, ld, spd = launch_gemm_dense(dt, unal_a, unal_d, b, k, Kdim, ws)
        code, splits = 'each/Dx[%s]' % sd, (spd, 1)
        n += ld
        _leaf('phase1: Dx and G one launch each') if want_G else _leaf('phase1: Dx alone (G is the state\'s)')
        if want_G:
            sg, lg, spg = launch_gemm_dense(dt, unal_d, unal_d, k, k, s, ws)
            code += '/G[%s]' % sg
            n += lg
            splits = (spd, spg)
    if G_agg == 'average':
        _leaf('phase1: G_average rows updated')
        n += 1
    if need_sub:
        code = 'prep+' + code
    out = SimpleNamespace(code=code, code_launches=n, splits=splits)
    mine['code'] = set(HIT)
    HIT.clear()
    # ---- statistics (phase1, rider_route)
    m = 1 if has_idx else 0                                                  # the gather of code_[idx] (ridge: not solved on compact rows)
    proper = need_sub and 0 < s < p
    ride = proper and Dx_agg != 'full' and not (flags & NO_RIDER) and cdiv(p, 64) < 1024      # rider_route
    if not proper:
        _leaf('no rider: no proper subset')
    elif Dx_agg == 'full':
        _leaf('no rider: Dx over all of p with a subset')
    elif flags & NO_RIDER:
        _leaf('no rider: MODL_FLAG_NO_RIDER')
    elif not ride:
        _leaf('no rider: p of 65472 or more')
    if ride:
        r, l = stats_pair(dt, k, s, s_pad, 0, b, ws, 'rows', resident=resident, stamps=bool(flags & GEMM_STAMPS))   # (the head launch alone)
        fused = dt == 'f32' and k <= 512 and optimizer != 'sgd'              # du_carries_riders (the probes' updates have no l1 term)
        if dt == 'f32' and k <= 512 and not fused:
            _leaf('rider: the sgd update carries none')
        unal_c, unal_x = misaligned(dt, k), misaligned(dt, ldx, xbase)
        if fused and p >= 2048 and plan_wide_ok(p, k, b, ldx, k, xbase):     # rider_route
            _leaf('rider: wide128')
            rider = 'wide128'
        elif fused and plan_stats_ok(dt, unal_x, unal_c, p, k, b):           # rider_route
            _leaf('rider: stats32 unal') if unal_x or unal_c else _leaf('rider: stats32 al')
            rider = 'stats32/' + ('unal' if unal_x or unal_c else 'al')
        else:                                                                # phase2 completes it
            _leaf('rider: completed after the update')
            rider = 'after[%s]' % stats_pair(dt, k, p, ldx, xbase, b, ws, 'skip', M0=0, resident=resident)[0]
        out.stats = r + '/ride:' + rider
    else:
        r, l = stats_pair(dt, k, p, ldx, xbase, b, ws, 'stats', resident=resident)
        out.stats = r + '/noride'
    out.stats_launches = m + l
    mine['stats'] = set(HIT)
    HIT.clear()
    HIT.update(taken, *(mine[sec] for sec in judged))
    return out


def partial_gram(dt, k, s, mb, p):             # phase2 -> gram_of_rows with the subset on K
    return launch_gemm(dt, k, k, s, split_scratch_elems(mb, k, p), gather_k=True)


def expected_route(probe, dt, **sh):
    """The code path of a probe at a shape, as a string (see the module docstring for the lines restated)."""
    if probe == 'T':
        n, k, p, mb = sh['b'], sh['k'], sh['p'], sh.get('mb', sh['b'])
        ldx, base = sh.get('ldx', p), sh.get('base', 0)
        ws = split_scratch_elems(mb, k, p)
        chunks = []
        for r0 in range(0, n, mb):                                           # transform_chunks
            b = min(mb, n - r0)
            _leaf('transform: a full chunk') if b == mb else _leaf('transform: a short last chunk')
            chunks.append(launch_gemm_dense(dt, misaligned(dt, ldx, base + r0 * ldx), misaligned(dt, k), b, k, p, ws)[0])
        return 'T:' + '|'.join(chunks)
    if probe == 'G':
        k, p = sh['k'], sh['p']
        return 'G:' + launch_gemm(dt, k, k, p, split_scratch_elems(sh.get('mb', 64), k, p))[0]      # modl_somf_full_gram
    agg = sh.get('agg', 'masked')
    r = phase1(dt, sh['b'], sh['k'], sh['p'], sh.get('s', sh['p']), sh.get('s') is not None, agg, agg, sh.get('ldx', sh['p']),
               sh['b'], sh.get('flags', 0), resident=sh.get('resident', True), judged=('code',) if probe == 'S-code' else ('stats',),
               optimizer=sh.get('optimizer', 'variational'))
    if probe == 'S-code':
        tail = ''
        if agg == 'full' and 2 * sh.get('s', sh['p']) < sh['p']:             # phase2, gram_is_partial: s < p / 2
            _leaf('phase2: G_ -= and += the Gram of the sampled rows')
            tail = '/partialG[%s]' % partial_gram(dt, sh['k'], sh['s'], sh['b'], sh['p'])[0]
        elif agg == 'full':
            _leaf('phase2: G_ recomputed over all of p')
            tail = '/fullG[%s]' % launch_gemm(dt, sh['k'], sh['k'], sh['p'], split_scratch_elems(sh['b'], sh['k'], sh['p']))[0]
        return 'S-code:' + r.code + tail
    return 'S-stats:' + r.stats


SECTION = {'T': 0, 'G': 1, 'S-code': 2, 'S-stats': 3}                        # MODL_ROUTE_*
ROUTE_MAX = 512                                                             # MODL_PRODUCT_ROUTE_MAX


def product_route(dt, section, k, p, n, mb, b, s=None, ldx=None, base=0, agg='masked', optimizer='variational', flags=0, has_idx=True,
                  cap=ROUTE_MAX, rc=False):
    """modl_somf_product_route for a plan of `Plan`'s descriptor: the library's own answer, no plan and no device involved"""
    import ctypes as C
    from modl_amd._lib import lib, check, SomfDesc, AGG, OPT
    d = SomfDesc()
    d.dtype, d.k, d.p, d.n_samples = (0 if dt == 'f32' else 1), k, p, n
    d.G_agg = d.Dx_agg = AGG[agg]
    d.optimizer, d.code_pos, d.comp_pos, d.max_iter = OPT[optimizer], 0, 0, 100
    d.code_alpha, d.code_l1_ratio, d.comp_l1_ratio, d.tol, d.step_size = 1.0, 0.0, 0.0, 1e-3, 1e-3
    d.max_batch, d.flags = mb, flags
    buf = C.create_string_buffer(max(cap, 1))
    code = lib.modl_somf_product_route(C.byref(d), section, b, p if s is None else s, int(s is not None), int(has_idx), p if ldx is None else ldx,
                                       base, buf, cap)
    if rc:
        return code
    check(code, 'modl_somf_product_route')
    return buf.value.decode()


def _resident(on):
    from modl_amd._lib import lib, check, DEBUG_STATS_RESIDENT
    check(lib.modl_debug_set(DEBUG_STATS_RESIDENT, 1 if on else 0))


def library_route(probe, dt, **sh):
    """the same string as `expected_route`, from the library (the transform: one call per chunk)"""
    k, p = sh['k'], sh['p']
    if probe == 'T':
        n, mb, ldx, base = sh['b'], sh.get('mb', sh['b']), sh.get('ldx', p), sh.get('base', 0)
        return 'T:' + '|'.join(product_route(dt, 0, k, p, n, mb, min(mb, n - r0), ldx=ldx, base=base + r0 * ldx) for r0 in range(0, n, mb))
    if probe == 'G':
        return 'G:' + product_route(dt, 1, k, p, 1, sh.get('mb', 64), 1)
    try:
        _resident(sh.get('resident', True))
        return probe + ':' + product_route(dt, SECTION[probe], k, p, sh['b'] + 3, sh['b'], sh['b'], sh.get('s'), sh.get('ldx'), 0,
                                           sh.get('agg', 'masked'), sh.get('optimizer', 'variational'), sh.get('flags', 0))
    finally:
        _resident(True)


# ---------------------------------------------------------------------------------------------------- the table
ROUTES = []


def _route(probe, name, want, dts=('f32',), rep=False, gpu=True, **sh):
    """gpu=False: a point of the route table alone (`test_route_table`); no probe on the device judges it"""
    ROUTES.append(SimpleNamespace(probe=probe, name='%s-%s' % (probe, name), want=want, dts=dts, rep=rep, gpu=gpu, sh=sh))


BOTH = ('f32', 'f64')
_route('T', 'interior', ('dense/al/t1x1/interior/s1/',), rep=True, b=64, k=64, p=96)
_route('T', 'edge_ktail', ('dense/al/t2x2/edge/s1/kps224/last200',), b=70, k=68, p=200)
_route('T', 'split', ('dense/al/t2x2/edge/s7/kps160/last40',), rep=True, b=70, k=68, p=1000)
_route('T', 'split64', ('dense/al/t2x2/edge/s7/kps80/last20',), dts=('f64',), rep=True, b=70, k=66, p=500)
_route('T', 'unal_dt', ('dense/unalB/t2x3/edge/s2/kps160/last100',), rep=True, b=128, k=130, p=260)
_route('T', 'unal_ldx', ('dense/unalA/t2x2/edge/s2/',), b=128, k=128, p=257, ldx=258)
_route('T', 'unal_base', ('dense/unalA/t2x2/edge/',), dts=BOTH, b=128, k=128, p=257, ldx=260, base=1)
_route('T', 'unal_dt64', ('dense/unalB/t2x3/edge/s4/',), dts=('f64',), rep=True, b=128, k=129, p=257, ldx=258)
_route('T', 'gather_small', ('gather/small/t1x2/s2/kps160/last140',), rep=True, b=64, k=70, p=300)
_route('T', 'gather_tall_dense', ('gather/tall/t2x1/s2/', '/Add/Bd'), rep=True, b=200, k=30, p=333)
_route('T', 'gather_tall_general', ('gather/tall/t2x1/s2/', '/Adg/Bd'), b=130, k=30, p=333)
_route('T', 'gather_tall64', ('gather/tall/t2x1/s2/', '/Add/Bd'), dts=('f64',), rep=True, b=200, k=31, p=333)
_route('T', 'chunks', ('dense/al/t1x1/interior/s1/', '|dense/al/t1x1/edge/s1/'), b=67, k=64, p=96, mb=64)
_route('T', 'minimal', ('gather/tall/t1x1/s1/kps32/last1/Ag/Bg',), dts=BOTH, b=1, k=1, p=1)
_route('G', 'tall_general', ('gather/tall/t1x1/s1/kps64/last50/Ag/Bg',), dts=BOTH, rep=True, k=12, p=50)
_route('G', 'tall_half', ('gather/tall/t1x1/s2/kps160/last140/Ag/Bd',), k=16, p=300)
_route('G', 'tall_full', ('gather/tall/t1x1/s2/kps160/last140/Ag/Bd',), k=32, p=300)
_route('G', 'small_ktail', ('gather/small/t1x1/s1/kps48/last40',), dts=BOTH, k=33, p=40)
_route('G', 'small_deep', ('gather/small/t2x2/s21/kps144/last120',), dts=BOTH, rep=True, k=70, p=3000)
_route('G', 'big', ('gather/big/t23x23/s1/kps32/last24',), k=2820, p=24)
_route('S-code', 'pair_rk', ('prep+pair/Dx[dense/al/t1x1/interior/s2/kps128/last128/rk', 'G[dense/al/t1x1/interior/s2/kps128/last128/rk/sym1/ut1]'),
       rep=True, agg='average', b=64, k=64, p=512, s=256)
_route('S-code', 'pair_mirror', ('prep+pair/', 'G[dense/al/t3x3/edge/s4/kps160/last120/rk/sym1/ut6]'), rep=True, agg='average', b=50, k=132,
       p=700, s=600)
_route('S-code', 'pair_spad', ('prep+pair/', 'G[dense/al/t3x3/edge/s4/kps160/last117/rk/sym1/ut6]'), agg='average', b=50, k=132, p=700, s=597)
_route('S-code', 'pair_nosplit', ('prep+pair/', 'G[dense/al/t3x3/edge/s1/kps128/last100/rk/sym0]'), agg='average', b=50, k=132, p=700, s=100)
_route('S-code', 'pair64', ('prep+pair/', 'G[dense/al/t2x2/edge/s4/kps80/last60/pipe/sym1/ut3]'), dts=('f64',), rep=True, agg='average', b=50,
       k=66, p=400, s=300)
_route('S-code', 'pair_long_rk_last', ('prep+pair/', 'G[dense/al/t3x3/edge/s32/kps288/last72/pipe+rk_last/sym1/ut6]'), rep=True, agg='average', b=50,
       k=132, p=9600, s=9000)
_route('S-code', 'pair_long', ('prep+pair/', 'G[dense/al/t3x3/edge/s32/kps288/last272/pipe/sym1/ut6]'), agg='average', b=50, k=132, p=9600, s=9200)
_route('S-code', 'unpaired', ('prep+each/Dx[gather/tall/', '/G[gather/tall/'), rep=True, agg='average', b=20, k=30, p=120, s=60)
_route('S-code', 'reduction1', ('pair/Dx[dense/unalA/',), agg='average', b=128, k=128, p=257, ldx=258)
_route('S-code', 'full_split', ('each/Dx[', 'partialG[gather/small/t2x2/s2/kps160/last140/Ag/Bg]'), dts=BOTH, rep=True, agg='full',
       b=16, k=70, p=900, s=300)
_route('S-code', 'full_tall', ('each/Dx[', 'partialG[gather/tall/t1x1/s1/kps64/last64/Ag/Bg]'), dts=BOTH, agg='full', b=16, k=24, p=200, s=64)
# s = p / 2 is no longer "fewer than half": G_ is recomputed over all of p (the judge of S-code/full assumes the partial passes)
_route('S-code', 'full_regram', ('each/Dx[', 'fullG[gather/tall/t1x1/s1/kps224/last200/Ag/Bd]'), dts=BOTH, gpu=False, agg='full', b=16, k=24, p=200,
       s=100)
_route('S-stats', 'sgd_ride_after', ('stats32/al/t7x2/ride:after[stats32/al/t19x2]',), gpu=False, b=64, k=64, p=600, s=200, optimizer='sgd')
for _b, _k in ((64, 64), (50, 64), (256, 64), (64, 68)):
    _route('S-stats', 'tiles32_b%d_k%d' % (_b, _k), ('stats32/al/t10x%d/noride' % cdiv(_k, 32),), rep=(_b, _k) == (50, 64), b=_b, k=_k, p=300)
_route('S-stats', 'densepair_b260', ('densepair/al/pipe/noride',), rep=True, b=260, k=64, p=300)
_route('S-stats', 'gather_k30', ('each/C[gather/tall/', '/B[gather/tall/', 'noride'), rep=True, b=64, k=30, p=300)
_route('S-stats', 'unal_dense_k30', ('each/C[gather/tall/', '/B[dense/unalB/', 'noride'), rep=True, b=64, k=30, p=3000)
_route('S-stats', 'ride32', ('stats32/al/t7x2/ride:stats32/al',), rep=True, b=64, k=64, p=600, s=200)
_route('S-stats', 'ride_wide', ('stats32/al/t25x2/ride:wide128',), rep=True, b=64, k=64, p=2400, s=800)
_route('S-stats', 'ride32_p2402', ('stats32/al/t25x2/ride:stats32/unal',), b=64, k=64, p=2402, s=800)
_route('S-stats', 'norider', ('stats32/unal/t76x2/noride',), b=64, k=64, p=2402, s=800, flags=NO_RIDER)
_route('S-stats', 'norider_p65476', ('resident16/vec4/noride',), b=64, k=64, p=65476, s=800)
_route('S-stats', 'resident', ('resident16/vec4/noride',), rep=True, b=64, k=64, p=4096)
_route('S-stats', 'resident_p4100', ('resident16/vec4/noride',), b=64, k=64, p=4100)
_route('S-stats', 'resident_k36', ('resident16/vec4/noride',), b=64, k=36, p=4096)
_route('S-stats', 'resident_b20', ('resident16/vec4/noride',), b=20, k=64, p=4096)
_route('S-stats', 'resident_rows', ('resident16/scalar/ride:wide128',), rep=True, b=64, k=64, p=16416, s=5472)
_route('S-stats', 'not_resident_b22', ('stats32/al/t128x2/noride',), b=22, k=64, p=4096)
_route('S-stats', 'resident_off', ('stats32/al/t128x2/noride',), b=64, k=64, p=4096, resident=False)
_route('S-stats', 'wide_2chunks', ('wide32/c2/noride',), rep=True, b=24, k=260, p=65476)
_route('S-stats', 'wide_k32', ('wide32/c1/noride',), b=50, k=32, p=65476)
_route('S-stats', 'wide_p65474', ('stats32/unal/t2047x1/noride',), b=50, k=32, p=65474)
_route('S-stats', 'densepair64', ('densepair/al/pipe/noride',), dts=('f64',), rep=True, b=50, k=66, p=300)
_route('S-stats', 'ride_after64', ('densepair/al/pipe/ride:after[densepair/al/pipe]',), dts=('f64',), rep=True, b=50, k=66, p=600, s=200)
_route('S-stats', 'ride_after64_gather', ('each/C[gather/tall/', 'ride:after[each/B[gather/tall/t5x1/'), dts=('f64',), b=50, k=31, p=600, s=200)
_route('S-stats', 'gather64_k31', ('each/C[gather/tall/', '/B[gather/tall/', 'noride'), dts=('f64',), b=50, k=31, p=300)
_route('S-stats', 'sgd', ('stats32/al/t10x2/noride',), b=64, k=64, p=300, optimizer='sgd')
_route('S-stats', 'three_steps', ('stats32/al/t7x2/ride:stats32/al',), b=64, k=64, p=600, s=200, steps=3)
_route('S-stats', 'three_steps_wide', ('stats32/al/t25x2/ride:wide128',), b=64, k=64, p=2400, s=800, steps=3)
ROUTE_BY_KEY = {(r.name, dt): r for r in ROUTES for dt in r.dts}
POINTS = sorted(key for key, r in ROUTE_BY_KEY.items() if r.gpu)
LEAVES = ('dense/al/', 'dense/unalA/', 'dense/unalB/', '/interior/', '/edge/', 'gather/tall/', 'gather/small/', 'gather/big/', '/Add/', '/Adg/', '/Ag/Bg',
          '/Ag/Bd', '/rk', '/pipe', '/sym1/', '/sym0', '/rk/sym1', '/rk/sym0', '/pipe+rk_last/sym1', 'last272/pipe/sym1', 'pair/Dx[', 'each/Dx[', 'prep+', 'partialG[gather/small/', 'partialG[gather/tall/', 'fullG[gather/tall/',
          'resident16/vec4', 'resident16/scalar', 'wide32/c1', 'wide32/c2', 'stats32/al/', 'stats32/unal/', 'densepair/al/pipe', 'each/C[gather/',
          '/B[gather/', '/B[dense/unalB/', '/noride', 'ride:stats32/al', 'ride:stats32/unal', 'ride:wide128', 'ride:after[densepair/')


# branches of the restatement that no point takes, each with the reason; `test_route_table` holds them to NOT being taken
UNREACHED = {
    'no rider: Dx over all of p with a subset': 'needs Dx_agg = full with G_agg != full; the three probes set G_agg = Dx_agg, as their formulas assume',
}


def route_of(r, dt):
    sh = {a: v for a, v in r.sh.items() if a != 'steps'}
    return expected_route(r.probe, dt, **sh)


def family(r, dt):
    """the route family a figure is recorded under"""
    s = route_of(r, dt)
    if r.probe == 'T':
        return 'T ' + ('gather' if 'gather' in s else 'misaligned' if 'unal' in s else 'dense') + ' ' + dt
    if r.probe == 'G':
        return 'G gather ' + dt
    if r.probe == 'S-code':
        return 'S-code ' + ('full' if 'partialG' in s else 'paired' if 'pair/' in s else 'unpaired') + ' ' + dt
    head = s.split(':', 1)[1].split('/')[0]
    return 'S-stats ' + ('gather' if 'B[gather' in s else 'misaligned dense' if 'B[dense/unal' in s else head) + ' ' + dt


# ---------------------------------------------------------------------------------------------------- scenes
def _seed(*what):
    return zlib.crc32(('products-' + '-'.join(str(w) for w in what)).encode()) % 100000


def draw(scene, rs, rows, cols, dt):
    """(rows, cols) operand of a scene, as float64 values that the dtype holds exactly after the cast"""
    if scene == 'integers':
        return rs.randint(-3, 4, size=(rows, cols)).astype(np.float64)
    a = rs.randn(rows, cols)
    if scene == 'scales':
        span = 3 if dt == 'f32' else 6
        a = a * (10.0 ** rs.uniform(-span, span, rows))[:, None]
    return a.astype(DT[dt]).astype(np.float64)


def spd(rs, k, integers):
    """a random symmetric positive definite matrix without a zero entry (integers: positive multiples of 4, exact)"""
    if integers:
        R = rs.randint(-1, 2, size=(k, 8)).astype(np.float64)
        return 4 * (R.dot(R.T) + 12) + 4 * np.diag(rs.randint(1, 4, size=k).astype(np.float64))
    R = rs.randn(k, k + 8)
    return R.dot(R.T) / k + np.diag(rs.uniform(0.5, 1.5, k))


def make_case(r, dt, scene):
    """The inputs of one call of a probe at a point, as float64 arrays holding values exact in the dtype."""
    sh = r.sh
    rs = np.random.RandomState(_seed(r.name, dt, scene))
    ints = scene == 'integers'
    k, p = sh['k'], sh['p']
    c = SimpleNamespace(probe=r.probe, dt=dt, scene=scene, k=k, p=p, D=draw(scene, rs, k, p, dt), sh=sh)
    if r.probe == 'G':
        return c
    b = sh['b']
    c.b, c.ldx, c.base, c.mb = b, sh.get('ldx', p), sh.get('base', 0), sh.get('mb', b)
    c.X = draw(scene, rs, b, p, dt)
    if r.probe == 'T':
        return c
    c.agg, c.flags, c.optimizer, c.resident = sh.get('agg', 'masked'), sh.get('flags', 0), sh.get('optimizer', 'variational'), sh.get('resident', True)
    c.n = b + 3
    c.idx = rs.permutation(c.n)[:b].astype(np.int64)
    c.steps = sh.get('steps', 1)
    s = sh.get('s')
    c.subsets = [None if s is None else rs.permutation(p)[:s].astype(np.int64) for _ in range(c.steps)]       # unsorted
    c.orders = [rs.permutation(k).astype(np.int64) for _ in range(c.steps)]
    c.reduction = float(rs.choice([2, 4])) if ints else (1.0 if s is None else p / float(s))
    c.w = 0.37
    c.ws = np.where(rs.permutation(b) < b // 2, 1.0, 0.25)
    q = (lambda a: a.astype(DT[dt]).astype(np.float64))
    c.C0 = spd(rs, k, ints)
    nonzero = lambda shape: 4.0 * rs.choice([-3, -2, -1, 1, 2, 3], size=shape)          # noqa: E731
    c.B0 = nonzero((p, k)) if ints else q(rs.randn(p, k))                                  # feature-major, as Bt
    c.code0 = q(rs.randn(c.n, k)) if not ints else rs.randint(1, 4, size=(c.n, k)).astype(np.float64)
    c.G0 = None
    if c.agg == 'full':                                                     # arbitrary symmetric (positive definite: the ridge solve reads it)
        E = spd(rs, k, ints)
        c.G0 = E if ints else np.maximum(q(E), q(E).T)
    c.Dxa0 = c.Ga0 = None
    if c.agg == 'average':
        c.Dxa0 = nonzero((c.n, k)) if ints else q(rs.randn(c.n, k))
        base = spd(rs, k, ints)
        mult = rs.randint(1, 3, size=c.n).astype(np.float64) if ints else rs.uniform(0.5, 2.0, c.n)
        c.Ga0 = q(mult[:, None, None] * base[None])
        c.Ga0 = np.maximum(c.Ga0, c.Ga0.transpose(0, 2, 1))                  # (bitwise symmetric after the cast)
    return c


# ---------------------------------------------------------------------------------------------------- the judges
FIGURES = {}


def _note(what, value):
    if np.isfinite(value):
        FIGURES[what] = max(FIGURES.get(what, 0.0), float(value))


def _report():
    print('largest |got - ref| / bound so far: ' + '; '.join('%s = %.3g' % kv for kv in sorted(FIGURES.items())))


def eps_of(dt):
    return float(np.finfo(DT[dt]).eps)


def bound_of(dt, K, S, A, extra=0.0):
    return (K + S + 6) * eps_of(dt) * np.asarray(A, dtype=np.float64) + extra


def judge_bound(dt, got, ref, A, K, S, who=None, extra=0.0):
    got = np.asarray(got)
    assert np.all(np.isfinite(got)), ('non-finite result', np.argwhere(~np.isfinite(got))[:4])
    err = np.abs(np.asarray(got, dtype=LD) - ref).astype(np.float64)
    bound = bound_of(dt, K, S, A, extra)
    with np.errstate(invalid='ignore', divide='ignore'):
        ratio = np.where(err == 0, 0.0, err / np.where(bound == 0, 1e-300, bound))
    if who:
        _note(who, ratio.max() if ratio.size else 0.0)
    bad = np.argwhere(ratio > 1)
    assert bad.size == 0, ('over the bound', who, float(ratio.max()), bad[:4], len(bad))


def judge_exact(got, ref):
    """the exact integers, bitwise apart from the sign of zero"""
    got = np.asarray(got, dtype=np.float64)
    bad = np.argwhere(~(got == ref))
    assert bad.size == 0, ('not the exact result', bad[:4], len(bad), got[tuple(bad[0])], ref[tuple(bad[0])])


def bits_symmetric(G):
    G = np.ascontiguousarray(G)
    return (G == 0).all() or np.array_equal(G + 0.0, np.swapaxes(G, -1, -2) + 0.0)


def prod_ref(A, B, scale=1.0):
    """(scale A B^T in longdouble, |scale| |A| |B|^T in float64: its own rounding, K 2^-53 of it, is nothing to a bound)"""
    ref = LD(scale) * np.asarray(A, dtype=LD).dot(np.asarray(B, dtype=LD).T)
    return ref, abs(scale) * np.abs(A).dot(np.abs(B).T)


def same_bits(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


# ---- what each probe should return
def judge_T(c, got, S, who=None):
    if c.scene == 'integers':
        judge_exact(got, c.X.dot(c.D.T))
        return
    ref, A = prod_ref(c.X, c.D)
    judge_bound(c.dt, got, ref, A, c.p, S, who, extra=4 * eps_of(c.dt) * np.abs(ref).astype(np.float64))


def judge_G(c, got, S, who=None):
    assert bits_symmetric(got), 'G is not bitwise symmetric'
    if c.scene == 'integers':
        judge_exact(got, c.D.dot(c.D.T))
        return
    ref, A = prod_ref(c.D, c.D)
    judge_bound(c.dt, got, ref, A, c.p, S, who)


def judge_code_average(c, before, after, subset, splits, who=None):
    """Dx_average and G_average rows idx after a step of the average aggregation; rows outside idx keep their bits."""
    cols = np.arange(c.p) if subset is None else subset
    Xs, Ds, red, ws, idx = c.X[:, cols], c.D[:, cols], c.reduction, c.ws, c.idx
    outside = np.setdiff1d(np.arange(c.n), idx)
    assert same_bits(after.Dx_average[outside], before.Dx_average[outside]) and same_bits(after.G_average[outside], before.G_average[outside]), \
        'rows of the averages outside idx were written'
    old_dx, old_g = before.Dx_average[idx].astype(np.float64), before.G_average[idx].astype(np.float64)
    assert bits_symmetric(after.G_average[idx]), 'a row of G_average is not bitwise symmetric'
    if c.scene == 'integers':
        judge_exact(after.Dx_average[idx], (1 - ws)[:, None] * old_dx + ws[:, None] * red * Xs.dot(Ds.T))
        judge_exact(after.G_average[idx], (1 - ws)[:, None, None] * old_g + (ws * red)[:, None, None] * Ds.dot(Ds.T)[None])
        return
    K = len(cols)
    pd, Ad = prod_ref(Xs, Ds, red)
    ref = LD(1) * (1 - ws)[:, None] * old_dx + ws[:, None] * pd
    judge_bound(c.dt, after.Dx_average[idx], ref, np.abs((1 - ws)[:, None] * old_dx) + ws[:, None] * Ad, K, splits[0], who and who + ' Dx')
    pg, Ag = prod_ref(Ds, Ds, red)
    ref = LD(1) * (1 - ws)[:, None, None] * old_g + ws[:, None, None] * pg[None]
    judge_bound(c.dt, after.G_average[idx], ref, np.abs((1 - ws)[:, None, None] * old_g) + ws[:, None, None] * Ag[None], K, splits[1],
                who and who + ' G')


def judge_code_full(c, before, after, subset, S, who=None):
    """G_ = G0 - D0_S D0_S^T + D1_S D1_S^T: two read-modify-write passes of gram_of_rows over the state's G.  Every term of
    the expression goes through at most s - 1 additions of its own product, S - 1 of its split sum and two roundings in each
    of the two epilogues (scale, add), the old value through those four alone: (s + S + 6) eps on every term's size."""
    assert bits_symmetric(after.G), 'G_ is not bitwise symmetric'
    D0, D1 = before.Dt[subset].astype(np.float64), after.Dt[subset].astype(np.float64)          # (s, k), feature-major
    p0, A0 = prod_ref(D0.T, D0.T)
    p1, A1 = prod_ref(D1.T, D1.T)
    G0 = before.G.astype(np.float64)
    judge_bound(c.dt, after.G, LD(1) * G0 - p0 + p1, np.abs(G0) + A0 + A1, len(subset), S, who)


def judge_stats(c, before, after, who=None):
    """C_ and every row of B_ against the update formulas, from the device's own codes"""
    code = after.code[c.idx].astype(np.float64)
    assert np.all(np.isfinite(code)), 'the device returned non-finite codes'
    w, b = c.w, c.b
    beta, wt = (0.0, 1.0) if c.optimizer == 'sgd' else (1 - w, w)
    pc, Ac = prod_ref(code.T, code.T, wt / b)
    C0, B0 = before.C.astype(np.float64), before.Bt.astype(np.float64)
    judge_bound(c.dt, after.C, LD(beta) * C0 + pc, np.abs(beta * C0) + Ac, b, 1, who and who + ' C')
    pb, Ab = prod_ref(c.X.T, code.T, wt / b)
    judge_bound(c.dt, after.Bt, LD(beta) * B0 + pb, np.abs(beta * B0) + Ab, b, 1, who and who + ' B')


# ---------------------------------------------------------------------------------------------------- the loops, restated (mutants)
def tiled_product(A, B, K, bm, bn, bk, kps, sym, dt, out, mut=(), rmw=None, fetch='clamp'):
    """out = epilogue(A[:, :K] B[:, :K]^T) as the tiled kernels form it: tiles of bm x bn, splits of kps, K-tiles of bk staged
    with zeros SELECTED outside the operand, partial sums added in split order, tiles below the diagonal mirrored (sym).  A, B
    hold columns behind K (what the memory behind an operand row holds).  rmw = (beta, alpha): out = beta out + alpha v.
    fetch: what a lane outside the operand loads before the select - 'clamp' the nearest element inside or behind the row (the
    gather kernel's clamped coordinates), 'base' element [0, 0] of the operand (the dense TileLoader)."""
    T = DT[dt]
    M, N = A.shape[0], B.shape[0]
    splits = cdiv(K, kps)
    acc = np.zeros((splits, cdiv(M, bm) * bm, cdiv(N, bn) * bn), dtype=T)

    def stage(Op, i0, bi, k0, k_end):
        I = Op.shape[0]
        ii = np.arange(i0, i0 + bi)
        kk = np.arange(k0, k0 + bk)
        inside = (ii < I)[:, None] & (kk < k_end)[None, :]
        ic = ii % I if 'wrap_rows' in mut else np.minimum(ii, I - 1)
        raw = Op[ic][:, np.minimum(kk, Op.shape[1] - 1)].astype(T)
        if fetch == 'base' and 'wrap_rows' not in mut:
            raw = np.where(inside, raw, Op[0, 0].astype(T))
        if 'wrap_rows' in mut:
            inside = np.ones_like(inside) & (kk < k_end)[None, :]
        if 'multiply_zeros' in mut:
            with np.errstate(invalid='ignore'):
                return raw * inside.astype(T)
        return np.where(inside, raw, T(0))
    for z in range(splits):
        k_begin = z * kps
        k_end = min(k_begin + kps, K)
        if 'last_split_full' in mut and z == splits - 1:
            k_end = k_begin + kps
        for m0 in range(0, M, bm):
            for n0 in range(0, N, bn):
                if sym and m0 > n0:
                    continue
                for k0 in range(k_begin, k_end, bk):
                    if 'drop_k_tail' in mut and z == splits - 1 and k0 + bk > k_end:
                        continue
                    with np.errstate(invalid='ignore'):
                        acc[z, m0:m0 + bm, n0:n0 + bn] += stage(A, m0, bm, k0, k_end).dot(stage(B, n0, bn, k0, k_end).T)
    def store(mm, nn, val):
        if rmw is None:
            out[mm, nn] = val
        else:
            out[mm, nn] = T(rmw[0]) * out[mm, nn] + T(rmw[1]) * val
    # wrap_rows: the rows of an edge tile behind M hold row m % M again, and are stored there again
    for mp in range(acc.shape[1] if 'wrap_rows' in mut else M):
        m, m0 = mp % M, mp // bm * bm
        for n0 in range(0, N, bn):
            if sym and m0 > n0:
                continue
            n1 = min(n0 + bn, N)
            v = np.zeros(n1 - n0, dtype=T)
            for z in range(splits):
                v = v + acc[z, mp, n0:n1]
            if 'split_twice' in mut and splits > 1:
                v = v + acc[splits - 1, mp, n0:n1]
            store(m, slice(n0, n1), v)
            if sym and m0 < n0 and 'unmirrored' not in mut:
                vm = v
                if 'mirror_wrong_split' in mut and splits > 1:
                    vm = np.zeros_like(v)
                    for z in reversed(range(splits)):
                        vm = vm + acc[z, mp, n0:n1]
                for j, n in enumerate(range(n0, n1)):
                    store(n, m, vm[j])
    return out


def stats_step(Bt, X, code, w, subset, stamp, step, dt, mut=()):
    """The riding update of B_ (feature-major Bt) restated: the sampled rows through the row-indirected epilogue, the others
    by the rider, which leaves the rows stamped `step` alone."""
    T = DT[dt]
    b = X.shape[0]
    beta, wt = T(0 if 'beta_dropped' in mut else 1 - w), T(w)
    upd = lambda old, v: (old * beta + (wt * v) / T(b)).astype(T)          # noqa: E731
    V = X.T.astype(T).dot(code.astype(T))                                   # (p, k)
    rows = np.arange(len(subset)) if 'rows_ignored' in mut else subset
    Bt[rows] = upd(Bt[rows], V[subset])
    stamp[subset] = step
    for f in range(Bt.shape[0]):
        stamped = stamp[f] == step
        if stamped and 'stamped_twice' not in mut:
            continue
        if not stamped and 'unstamped_skipped' in mut and f % 7 == 3:
            continue
        Bt[f] = upd(Bt[f], V[f])
    return Bt


# ---------------------------------------------------------------------------------------------------- CPU tests
def test_route_table():
    """ROUTES names what the restated dispatch does at every point, the library's own route (modl_somf_product_route, no device)
    is that string at every point, and every leaf of the cascade is hit."""
    got = {}
    HIT.clear()
    longest = 0
    for (name, dt), r in ROUTE_BY_KEY.items():
        s = got[name, dt] = route_of(r, dt)
        for want in r.want:
            assert want in s, (name, dt, want, s)
        lib_s = library_route(r.probe, dt, **{a: v for a, v in r.sh.items() if a != 'steps'})
        assert lib_s == s, ('the library routes this point otherwise', name, dt, lib_s, s)
        longest = max([longest] + [len(part) for part in s.split(':', 1)[1].split('|')])
    assert longest + 1 <= ROUTE_MAX, ('MODL_PRODUCT_ROUTE_MAX does not hold the longest route of the table', longest)
    hit = set(HIT)
    # every branch that the restatement marks with _leaf(...) - read from this file's text, not from a list kept by hand - is
    # taken by a point, but for those listed, with the reason, in UNREACHED
    assert len(all_leaves()) > 50 and set(UNREACHED) <= all_leaves()
    assert all_leaves() - hit == set(UNREACHED), ('no point reaches', sorted(all_leaves() - hit - set(UNREACHED)), 'reached after all', sorted(hit & set(UNREACHED)))
    everything = ' '.join(got.values())
    for leaf in LEAVES:                       # and the combinations that matter, as they show in the route strings
        assert leaf in everything, ('no point reaches', leaf)
    f32_code = ' '.join(v for (name, dt), v in got.items() if dt == 'f32' and name.startswith('S-code'))
    for leaf in ('/rk/sym1', '/rk/sym0', '/pipe+rk_last/sym1', '/pipe/sym1'):     # the f32 paired Gram under each tile
        assert leaf in f32_code, ('no f32 paired point reaches', leaf)
    assert '/rk' in got['S-code-pair_rk', 'f32'] and 'pipe' in got['S-code-pair64', 'f64']
    for dt in BOTH:
        for fam in ('T dense', 'T gather', 'G gather', 'S-code paired', 'S-code full'):
            assert any(r.rep and dt in r.dts and family(r, dt).startswith(fam) for r in ROUTES), (fam, dt)
    # the thresholds, on either side
    assert not plan_dense('f32', False, True, 128, 130, 252, 1 << 20).ok and plan_dense('f32', False, True, 128, 130, 253, 1 << 20).ok
    assert 128 * 130 * 252 < 1 << 22 <= 128 * 130 * 253
    assert launch_gemm('f32', 64, 32, 64, 0)[0].startswith('gather/tall') and launch_gemm('f32', 64, 33, 64, 0)[0].startswith('gather/small')
    assert launch_gemm('f32', 2816, 2816, 24, 0)[0].startswith('gather/small') and launch_gemm('f32', 2817, 2817, 24, 0)[0].startswith('gather/big')
    assert stats_pair('f32', 64, 4095, 4096, 0, 64, 0)[0].startswith('stats32') and stats_pair('f32', 64, 4096, 4096, 0, 64, 0)[0].startswith('resident')
    assert stats_pair('f32', 260, 65472, 65472, 0, 24, 0)[0].startswith('stats32') and stats_pair('f32', 260, 65476, 65476, 0, 24, 0)[0].startswith('wide')
    assert stats_pair('f32', 64, 300, 300, 0, 256, 0)[0].startswith('stats32') and stats_pair('f32', 64, 300, 300, 0, 257, 0)[0].startswith('densepair')
    assert dense_tile('f32', plan_dense('f32', False, False, 64, 64, 256, 0), True) == 'rk'
    assert dense_tile('f32', plan_dense('f32', False, False, 64, 64, 257, 0), True) == 'pipe'
    assert phase1('f32', 64, 64, 2047 * 4, 800, True, 'masked', 'masked', 2047 * 4, 64).stats.endswith('ride:wide128')
    assert phase1('f32', 64, 64, 2044, 800, True, 'masked', 'masked', 2044, 64).stats.endswith('ride:stats32/al')
    assert phase1('f32', 64, 64, 65472, 800, True, 'masked', 'masked', 65472, 64).stats.endswith('ride:wide128')
    assert phase1('f32', 64, 64, 65476, 800, True, 'masked', 'masked', 65476, 64).stats.endswith('noride')
    assert split_scratch_elems(64, 64, 512) == 262144 and split_scratch_elems(50, 132, 700) == 1115136
    assert len(ROUTE_BY_KEY) == sum(len(r.dts) for r in ROUTES)


def test_route_boundaries():
    """The library against the restatement on both sides of every numeric boundary of the dispatch (pure function calls, no
    device), and the two sides on different routes where the boundary says so."""
    def both(probe, dt, starts=None, has=None, **sh):
        e, g = expected_route(probe, dt, **sh), library_route(probe, dt, **sh)
        assert g == e, ('the library routes this otherwise', probe, dt, sh, g, e)
        body = e.split(':', 1)[1]
        assert starts is None or body.startswith(starts), (probe, dt, sh, e, starts)
        assert has is None or has in body, (probe, dt, sh, e, has)
        return body
    n = 0
    for dt in BOTH:
        # misaligned operands: M N K = 2^22 - 1 (3 * 23 * 89 * 683) stays with the gather kernel, 2^22 takes the dense one
        assert 69 * 89 * 683 == (1 << 22) - 1 and 128 * 128 * 256 == 1 << 22
        both('T', dt, 'gather/', b=69, k=89, p=683)
        both('T', dt, 'dense/unalA/', b=128, k=128, p=256, ldx=257)
        # N = 32 | 33: the tall and the small tiles of the gather kernel
        both('G', dt, 'gather/tall/', k=32, p=40)
        both('G', dt, 'gather/small/', k=33, p=40)
        # a split of 8 BK | 8 BK + 1 (and the short last split of the longer one), paired
        tile = {'f32': ('/rk/', '/pipe+rk_last/', '/pipe/'), 'f64': ('/pipe/',) * 3}[dt]
        s8 = 32 * 8 * BKD[dt]                                                # 32 splits (the scratch's bound) of 8 BK
        both('S-code', dt, has='kps%d/last%d%ssym1' % (8 * BKD[dt], 8 * BKD[dt], tile[0]), agg='average', b=64, k=64, p=2 * s8, s=s8)
        both('S-code', dt, has='kps%d/last%d%ssym1' % (9 * BKD[dt], 4 * BKD[dt] + 1, tile[1]), agg='average', b=64, k=64, p=2 * s8, s=s8 + 1)
        both('S-code', dt, has='kps%d/last%d%ssym1' % (9 * BKD[dt], 9 * BKD[dt] - 8, tile[2]), agg='average', b=64, k=64, p=2 * s8,
             s=30 * 9 * BKD[dt] + 9 * BKD[dt] - 8)                           # (31 splits of 9 BK, the last 8 short of one)
        # s = p / 2 for G_agg = full: fewer than half the features -> the partial passes
        both('S-code', dt, has='/partialG[', agg='full', b=16, k=24, p=200, s=99)
        both('S-code', dt, has='/fullG[', agg='full', b=16, k=24, p=200, s=100)
        both('S-code', dt, has='/fullG[', agg='full', b=16, k=24, p=200, s=101)
        both('S-code', dt, has='/partialG[', agg='full', b=16, k=24, p=201, s=100)
        n += 11
    # the big tiles of the gather kernel from ceil(M / 128) ceil(N / 128) = 512: 511 | 512 tiles of 128 x 128 in a tall
    # misaligned product below 2^22 (k = 33: one column tile), as B_ of the statistics and as Dx of a transform chunk
    assert cdiv(65408, 128) == 511 and cdiv(65409, 128) == 512 and 65409 * 33 < 1 << 22
    both('S-stats', 'f32', has='/B[gather/small/t1022x1/', b=1, k=33, p=65408)
    both('S-stats', 'f32', has='/B[gather/big/t512x1/', b=1, k=33, p=65409)
    both('T', 'f32', 'gather/small/t1022x1/', b=65408, k=33, p=1)
    both('T', 'f32', 'gather/big/t512x1/', b=65409, k=33, p=1)
    both('T', 'f64', 'gather/small/t1022x1/', b=65408, k=33, p=1)
    both('T', 'f64', 'gather/big/t512x1/', b=65409, k=33, p=1)
    both('G', 'f32', 'gather/small/t44x44/', k=2816, p=24)               # (and square: 22 x 22 | 23 x 23)
    both('G', 'f32', 'gather/big/t23x23/', k=2817, p=24)
    st = dict(b=64, k=64, p=300)
    both('S-stats', 'f32', 'stats32/', **dict(st, b=256))                    # statistics K = b: 256 | 257
    both('S-stats', 'f32', 'densepair/', **dict(st, b=257))
    both('S-stats', 'f32', 'stats32/al/', **dict(st, p=4092))                # resident rows: 4096 (4095: also misaligned)
    both('S-stats', 'f32', 'stats32/unal/', **dict(st, p=4095))
    both('S-stats', 'f32', 'stats32/al/', **dict(st, p=4095, ldx=4096))
    both('S-stats', 'f32', 'resident16/', **dict(st, p=4096))
    both('S-stats', 'f32', 'resident16/', **dict(st, p=4096, k=256))         # resident k: 256 | 260
    both('S-stats', 'f32', 'stats32/al/', **dict(st, p=4096, k=260))
    both('S-stats', 'f32', 'resident16/', **dict(st, p=4096, b=20))          # resident K % 4: b = 20 | 22
    both('S-stats', 'f32', 'stats32/al/', **dict(st, p=4096, b=22))
    both('S-stats', 'f32', 'resident16/', **dict(st, p=4096, resident=True)) # the resident switch
    both('S-stats', 'f32', 'stats32/al/', **dict(st, p=4096, resident=False))
    both('S-stats', 'f32', 'stats32/al/', **dict(st, p=65472, k=260, b=24))  # 1023 | 1024 tiles of 64 features: the wide pair ...
    both('S-stats', 'f32', 'stats32/unal/', **dict(st, p=65473, k=260, b=24))
    both('S-stats', 'f32', 'wide32/c2', **dict(st, p=65476, k=260, b=24))
    both('S-stats', 'f32', has='/ride:wide128', **dict(st, p=65472, s=800))  # ... and the end of the rider
    both('S-stats', 'f32', has='/noride', **dict(st, p=65473, s=800))
    both('S-stats', 'f32', has='/noride', **dict(st, p=65476, s=800))
    both('S-stats', 'f32', has='/ride:stats32/al', **dict(st, p=2044, s=800))          # the rider's tiles: p = 2044 | 2048
    both('S-stats', 'f32', has='/ride:wide128', **dict(st, p=2048, s=800))
    both('S-stats', 'f32', has='/ride:wide128', **dict(st, p=2400, s=800, k=512))       # a launch that carries it: k = 512 | 516
    both('S-stats', 'f32', has='/ride:after[', **dict(st, p=2400, s=800, k=516))
    both('S-stats', 'f32', has='/ride:after[', **dict(st, p=2400, s=800, optimizer='sgd'))
    both('S-stats', 'f64', has='/ride:after[', **dict(st, p=2400, s=800))
    both('S-stats', 'f32', has='/noride', **dict(st, p=2400, s=800, flags=NO_RIDER))    # the flags
    both('S-stats', 'f32', 'resident16/scalar/ride:wide128', **dict(st, p=16416, s=5472))
    both('S-stats', 'f32', 'stats32/al/t171x2/ride:wide128', **dict(st, p=16416, s=5472, flags=GEMM_STAMPS))
    both('S-stats', 'f32', 'resident16/vec4/noride', **dict(st, p=16416, s=5472, flags=GEMM_STAMPS | NO_RIDER))
    print('%d boundary points agree' % (n + 39))


def test_product_route_errors():
    """modl_somf_product_route: MODL_EINVAL for a buffer one byte too small, a bad section, a bad descriptor or minibatch"""
    kw = dict(k=68, p=1000, n=70, mb=70, b=70)
    route = product_route('f32', 0, **kw)
    assert route == 'dense/al/t2x2/edge/s7/kps160/last40/pipe/sym0'
    assert product_route('f32', 0, cap=len(route) + 1, **kw) == route
    assert product_route('f32', 0, cap=len(route), rc=True, **kw) == -1               # no room for the terminator
    for section in (-1, 4):
        assert product_route('f32', section, rc=True, **kw) == -1
    assert product_route('f32', 0, rc=True, **dict(kw, k=0)) == -1 and product_route('f32', 0, rc=True, **dict(kw, k=4097)) == -1
    assert product_route('f32', 0, rc=True, **dict(kw, b=71)) == -1 and product_route('f32', 0, rc=True, **dict(kw, b=0)) == -1
    assert product_route('f32', 0, rc=True, ldx=999, **kw) == -1 and product_route('f32', 0, rc=True, base=-1, **kw) == -1
    assert product_route('f32', 2, rc=True, s=1001, **kw) == -1
    import ctypes as C
    from modl_amd._lib import lib
    assert lib.modl_somf_product_route(None, 0, 70, 1000, 0, 0, 1000, 0, C.create_string_buffer(64), 64) == -1


K_CODE = {r.sh.get('s', r.sh['p']) for r in ROUTES if r.probe == 'S-code' and r.gpu}          # contraction lengths of the probes
K_STATS = {r.sh['b'] for r in ROUTES if r.probe == 'S-stats' and r.gpu}
K_TABLE = sorted({r.sh['p'] for r in ROUTES if r.probe in ('T', 'G')} | K_CODE | K_STATS)


@pytest.mark.parametrize('dt', BOTH)
def test_judges_on_the_oracle(dt):
    """numpy's product in the dtype stays under 1 / 8 of the bound on every scene at every contraction length of the table
    (S = 1: the tightest bound), one dropped term per element - its largest - is
    over the bound at every K, so the bound is not vacuous."""
    T = DT[dt]
    worst = 0.0
    for K in K_TABLE:
        for scene in ('gaussian', 'scales', 'integers'):
            rs = np.random.RandomState(_seed('oracle', K, scene))
            A, B = draw(scene, rs, 5, K, dt), draw(scene, rs, 7, K, dt)
            got = A.astype(T).dot(B.astype(T).T)
            ref, Aabs = prod_ref(A, B)
            if scene == 'integers':
                judge_exact(got, A.dot(B.T))
                continue
            err = np.abs(got.astype(LD) - ref).astype(np.float64)
            assert np.all(err <= bound_of(dt, K, 1, Aabs) / 8), (K, scene, (err / bound_of(dt, K, 1, Aabs)).max())
            worst = max(worst, (err / bound_of(dt, K, 1, Aabs)).max())
            if K > 1:
                drop = np.abs(A[:, None, :] * B[None, :, :]).max(axis=2)
                assert np.all(drop > bound_of(dt, K, 64, Aabs)), (K, scene, 'a dropped term hides under the bound')
                # the read-modify-write epilogues, each at the contraction lengths it runs at: the statistics (K = b) with
                # (1 - w, w / b), the averages (K = s) with their smaller weight (0.75, 0.25 reduction, reduction >= 1)
                # (under `scales` a small increment is below the rounding of the old value: nothing could see it)
                for Ks, beta, alpha in ((K_STATS, 0.63, 0.37 / K), (K_CODE, 0.75, 0.25)):
                    if scene == 'gaussian' and K in Ks:
                        old = rs.randn(5, 7).astype(T).astype(np.float64)
                        Ar = np.abs(beta * old) + alpha * Aabs
                        assert np.all(alpha * drop > bound_of(dt, K, 1, Ar)), (K, 'a dropped term hides under the read-modify-write bound')
    print('%s: numpy same-dtype product / bound, largest: %.3g' % (dt, worst))


def _tp(A, B, K, dt, sym=False, mut=(), fill=FILL, **kw):
    M, N = A.shape[0], B.shape[0]
    out = np.full((M, N), fill, dtype=DT[dt])
    if kw.get('rmw'):
        out[:] = kw['old']
    return tiled_product(A, B, K, 8, 8, 4, 12, sym, dt, out, mut, kw.get('rmw'), kw.get('fetch', 'clamp'))


def test_mutants():
    """Every mutant of the restated loops is rejected by its named scene and judge; where one cannot show, that is asserted."""
    dt = 'f32'
    rs = np.random.RandomState(5)
    K, M, N = 29, 19, 13                                   # three splits of 12, the last of 5; K tail 1; edge tiles 3 and 5 rows

    def operands(scene, behind, sym=False):
        A = np.concatenate([draw(scene, rs, M, K, dt), np.full((M, 16), behind)], axis=1)
        B = A if sym else np.concatenate([draw(scene, rs, N, K, dt), np.full((N, 16), behind)], axis=1)
        return A, B

    def exact_ok(A, B, got):
        try:
            judge_exact(got, A[:, :K].dot(B[:, :K].T))
        except AssertionError:
            return False
        return True

    def bound_ok(A, B, got, old=None, rmw=None):
        ref, Aabs = prod_ref(A[:, :K], B[:, :K])
        if rmw:
            ref, Aabs = LD(rmw[0]) * old + LD(rmw[1]) * ref, np.abs(rmw[0] * old) + abs(rmw[1]) * Aabs
        try:
            judge_bound(dt, got, ref, Aabs, K, 3)
        except AssertionError:
            return False
        return True
    # integers, exact
    A, B = operands('integers', 5.0)
    assert exact_ok(A, B, _tp(A, B, K, dt))
    for mut in ('drop_k_tail', 'last_split_full', 'split_twice'):
        assert not exact_ok(A, B, _tp(A, B, K, dt, mut=(mut,))), mut
    As, _ = operands('integers', 5.0, sym=True)
    assert exact_ok(As, As, _tp(As, As, K, dt, sym=True))
    assert not exact_ok(As, As, _tp(As, As, K, dt, sym=True, mut=('unmirrored',)))
    assert exact_ok(As, As, _tp(As, As, K, dt, sym=True, mut=('mirror_wrong_split',)))             # INVISIBLE on integers
    # gaussian
    A, B = operands('gaussian', 0.5)
    good = _tp(A, B, K, dt)
    assert bound_ok(A, B, good)
    Ag, _ = operands('gaussian', 0.5, sym=True)
    assert bits_symmetric(_tp(Ag, Ag, K, dt, sym=True)) and bound_ok(Ag, Ag, _tp(Ag, Ag, K, dt, sym=True))
    assert not bits_symmetric(_tp(Ag, Ag, K, dt, sym=True, mut=('mirror_wrong_split',)))
    # poison: the columns behind K hold NaN
    Ap, Bp = A.copy(), B.copy()
    Ap[:, K:] = np.nan
    Bp[:, K:] = np.nan
    assert same_bits(_tp(Ap, Bp, K, dt), good)
    assert not same_bits(_tp(Ap, Bp, K, dt, mut=('multiply_zeros',)), good)
    assert not same_bits(_tp(Ap, Bp, K, dt, mut=('last_split_full',)), good)
    assert same_bits(_tp(A, B, K, dt, mut=('multiply_zeros',)), good)                               # INVISIBLE without the poison
    # a loader that fetches its outside lanes from element [0, 0] never looks behind the operand: there the poison is
    # INVISIBLE (asserted), and nan_row with the NaN in row 0 is what rejects the mutant - every other row changes
    assert same_bits(_tp(Ap, Bp, K, dt, fetch='base'), good)
    assert same_bits(_tp(Ap, Bp, K, dt, mut=('multiply_zeros',), fetch='base'), good)
    An = A.copy()
    An[0] = np.nan
    clean = _tp(An, B, K, dt, fetch='base')
    assert same_bits(clean[1:], good[1:]) and not np.isfinite(clean[0]).any()
    assert not same_bits(_tp(An, B, K, dt, mut=('multiply_zeros',), fetch='base')[1:], good[1:])
    # wrapped edge rows: invisible under a plain store, a second update under a read-modify-write epilogue
    assert same_bits(_tp(A, B, K, dt, mut=('wrap_rows',)), good)
    old = rs.randn(M, N).astype(np.float32)
    rmw = (0.63, 0.37)
    assert bound_ok(A, B, _tp(A, B, K, dt, rmw=rmw, old=old), old.astype(np.float64), rmw)
    assert not bound_ok(A, B, _tp(A, B, K, dt, rmw=rmw, old=old, mut=('wrap_rows',)), old.astype(np.float64), rmw)
    # the riding statistics update
    p, k, b, s = 40, 6, 9, 12
    X, code = rs.randn(b, p).astype(np.float32), rs.randn(b, k).astype(np.float32)

    def run(mut, w, nsteps=1):
        Bt, stamp = rs_b0.copy(), np.zeros(p, dtype=np.int64)
        ok = True
        for t in range(nsteps):
            sub = subsets[t]
            before = Bt.copy()
            Bt = stats_step(Bt, X, code, w, sub, stamp, t + 1, dt, mut)
            pb, Ab = prod_ref(X.T, code.T, w / b)
            try:
                judge_bound(dt, Bt, LD(1 - w) * before.astype(np.float64) + pb, np.abs((1 - w) * before.astype(np.float64)) + Ab, b, 1)
            except AssertionError:
                ok = False
        return ok
    rs_b0 = rs.randn(p, k).astype(np.float32)
    subsets = [rs.permutation(p)[:s] for _ in range(3)]
    assert set(subsets[0]) - set(subsets[1]), 'a feature sampled in step 1 and not in step 2'
    assert run((), 0.37, 3)
    for mut in ('stamped_twice', 'unstamped_skipped', 'rows_ignored', 'beta_dropped'):
        assert not run((mut,), 0.37, 3), mut
    assert run(('beta_dropped',), 1.0)                                                              # INVISIBLE at w = 1


# ---------------------------------------------------------------------------------------------------- the probes on the device
@pytest.fixture(scope='module')
def gpu():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    return torch.device('cuda', 0)


class Plan:
    """a modl_somf plan of this test's own (ridge codes, code_alpha = 1)"""
    def __init__(self, dt, k, p, n, mb, agg='masked', optimizer='variational', flags=0):
        import ctypes as C
        from modl_amd._lib import lib, check, SomfDesc, AGG, OPT
        d = SomfDesc()
        d.dtype, d.k, d.p, d.n_samples = (0 if dt == 'f32' else 1), k, p, n
        d.G_agg = d.Dx_agg = AGG[agg]
        d.optimizer, d.code_pos, d.comp_pos, d.max_iter = OPT[optimizer], 0, 0, 100
        d.code_alpha, d.code_l1_ratio, d.comp_l1_ratio, d.tol, d.step_size = 1.0, 0.0, 0.0, 1e-3, 1e-3
        d.max_batch, d.flags = mb, flags
        self.h = C.c_void_p()
        check(lib.modl_somf_plan_create(C.byref(d), C.byref(self.h)), 'modl_somf_plan_create')

    def __enter__(self):
        return self.h

    def __exit__(self, *exc):
        from modl_amd._lib import lib
        lib.modl_somf_plan_destroy(self.h)
        self.h = None


def _td(dt):
    import torch
    return torch.float32 if dt == 'f32' else torch.float64


def _dev(a, dt, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=DT[dt])).to(dev)


def x_buffer(c, dev, X, poison):
    """X as a view of leading stride ldx, `base` elements into a buffer; two more rows behind the batch; the padding columns and
    those rows hold NaN (poison) or 0.5"""
    import torch
    rows = X.shape[0] + 2
    buf = torch.full((c.base + rows * c.ldx + 8,), float('nan') if poison else 0.5, dtype=_td(c.dt), device=dev)
    view = buf[c.base:c.base + rows * c.ldx].view(rows, c.ldx)
    view[:X.shape[0], :c.p] = _dev(X, c.dt, dev)
    assert view.data_ptr() % 16 == (c.base * TSZ[c.dt]) % 16
    return buf, view


def dt_buffer(c, dev, poison):
    import torch
    Dt = torch.full((c.p + 1, c.k), float('nan') if poison else 0.5, dtype=_td(c.dt), device=dev)
    Dt[:c.p] = _dev(c.D.T, c.dt, dev)
    assert Dt.data_ptr() % 16 == 0
    return Dt


def run_T(c, dev, poison=False, X=None):
    import torch
    from modl_amd._lib import lib, check
    from modl_amd.device import ptr, stream_ptr
    X = c.X if X is None else X
    n = X.shape[0]
    buf, view = x_buffer(c, dev, X, poison)
    Dt = dt_buffer(c, dev, poison)
    G = torch.zeros((c.k, c.k), dtype=_td(c.dt), device=dev)
    out = torch.full((n + 1, c.k), FILL, dtype=_td(c.dt), device=dev)
    with Plan(c.dt, c.k, c.p, n, c.mb) as plan:
        check(lib.modl_somf_transform(plan, ptr(Dt), ptr(G), ptr(view), c.ldx, n, ptr(out), stream_ptr(dev)), 'modl_somf_transform')
        torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert np.all(out[n] == FILL), 'the row behind code_out was written'
    return out[:n]


def run_G(c, dev, poison=False):
    import torch
    from modl_amd._lib import lib, check
    from modl_amd.device import ptr, stream_ptr
    Dt = dt_buffer(c, dev, poison)
    G = torch.full((c.k + 1, c.k), FILL, dtype=_td(c.dt), device=dev)
    with Plan(c.dt, c.k, c.p, 1, 64) as plan:
        check(lib.modl_somf_full_gram(plan, ptr(Dt), ptr(G), stream_ptr(dev)), 'modl_somf_full_gram')
        torch.cuda.synchronize()
    G = G.cpu().numpy()
    assert np.all(G[c.k] == FILL), 'the row behind G was written'
    return G[:c.k]


def run_S(c, dev, poison=False, X=None):
    """c.steps calls of modl_somf_step from the case's state: the list of the state (numpy) before the first and after each
    step, each with the launches of the code-product and statistics sections of that step."""
    import ctypes as C
    import torch
    from modl_amd._lib import lib, check, SomfState, SomfBatch, ProfEntry
    from modl_amd.device import ptr, stream_ptr
    X = c.X if X is None else X
    nan = float('nan')
    outside = np.setdiff1d(np.arange(c.n), c.idx)
    buf, view = x_buffer(c, dev, X, poison)
    st = SimpleNamespace(Dt=dt_buffer(c, dev, poison), Bt=_dev(c.B0, c.dt, dev), C=_dev(c.C0, c.dt, dev), code=_dev(c.code0, c.dt, dev),
                         comp_norm=torch.zeros(c.k, dtype=_td(c.dt), device=dev), G=None, Dx_average=None, G_average=None)
    if c.agg == 'full':
        st.G = _dev(c.G0, c.dt, dev)
    if c.agg == 'average':
        st.Dx_average, st.G_average = _dev(c.Dxa0, c.dt, dev), _dev(c.Ga0, c.dt, dev)
    if poison:
        st.code[torch.from_numpy(outside).to(dev)] = nan
        if c.agg == 'average':
            st.Dx_average[torch.from_numpy(outside).to(dev)] = nan
            st.G_average[torch.from_numpy(outside).to(dev)] = nan
    s = SomfState()
    s.d_Dt, s.d_Bt, s.d_C, s.d_code, s.d_comp_norm = ptr(st.Dt), ptr(st.Bt), ptr(st.C), ptr(st.code), ptr(st.comp_norm)
    s.d_G, s.d_Dx_average, s.d_G_average = ptr(st.G), ptr(st.Dx_average), ptr(st.G_average)

    def snap(launches=None):
        get = lambda t: None if t is None else t.cpu().numpy()               # noqa: E731
        return SimpleNamespace(Dt=get(st.Dt)[:c.p], Bt=get(st.Bt), C=get(st.C), code=get(st.code), G=get(st.G),
                               Dx_average=get(st.Dx_average), G_average=get(st.G_average), launches=launches)
    snaps = [snap()]
    wsample = np.ascontiguousarray(c.ws, dtype=DT[c.dt])
    with Plan(c.dt, c.k, c.p, c.n, c.b, c.agg, c.optimizer, c.flags) as plan:
        check(lib.modl_somf_prof_enable(plan, 1))
        for t in range(c.steps):
            bt = SomfBatch()
            bt.d_X, bt.ldx, bt.b = ptr(view), c.ldx, c.b
            sub, order = c.subsets[t], c.orders[t]
            bt.h_sample_idx, bt.h_order = c.idx.ctypes.data, order.ctypes.data
            bt.s, bt.h_subset = (c.p, None) if sub is None else (len(sub), sub.ctypes.data)
            bt.h_w_sample = wsample.ctypes.data
            bt.w, bt.reduction, bt.b_global = c.w, c.reduction, c.b
            check(lib.modl_somf_prof_reset(plan))
            check(lib.modl_somf_step(plan, C.byref(s), C.byref(bt), stream_ptr(dev)), 'modl_somf_step')
            check(lib.modl_somf_status(plan, stream_ptr(dev)), 'modl_somf_status')
            torch.cuda.synchronize()
            arr, n = (ProfEntry * 16)(), C.c_int(0)
            check(lib.modl_somf_prof_get(plan, arr, 16, C.byref(n)))
            snaps.append(snap({arr[i].name.decode(): int(arr[i].launches) for i in range(n.value)}))
    return snaps


def state_bits(snaps, c, rows_in_idx_only=False):
    """the bytes of everything a step may write, over the steps (poison: the rows inside idx only)"""
    out = []
    for sn in snaps[1:]:
        for name in ('Dt', 'Bt', 'C', 'G'):
            a = getattr(sn, name)
            out.append(b'' if a is None else a.tobytes())
        for name in ('code', 'Dx_average', 'G_average'):
            a = getattr(sn, name)
            out.append(b'' if a is None else (a[c.idx] if rows_in_idx_only else a).tobytes())
    return out


def outside_kept(snaps, c):
    outside = np.setdiff1d(np.arange(c.n), c.idx)
    for sn in snaps[1:]:
        for name in ('code', 'Dx_average', 'G_average'):
            a, a0 = getattr(sn, name), getattr(snaps[0], name)
            if a is not None and not same_bits(a[outside], a0[outside]):
                return False
    return True


def judge_S(r, c, snaps, who=None):
    dt = c.dt
    want = phase1(dt, c.b, c.k, c.p, r.sh.get('s', c.p), r.sh.get('s') is not None, c.agg, c.agg, c.ldx, c.b, c.flags, resident=c.resident, optimizer=c.optimizer)
    for t in range(c.steps):
        before, after = snaps[t], snaps[t + 1]
        assert after.launches['code_gemm'] == want.code_launches and after.launches['stats_gemm'] == want.stats_launches, \
            ('launches of the sections', after.launches, want.code_launches, want.stats_launches)
        if r.probe == 'S-stats':
            judge_stats(c, before, after, who)
        elif c.agg == 'average':
            judge_code_average(c, before, after, c.subsets[t], want.splits, who)
        else:
            judge_code_full(c, before, after, c.subsets[t], partial_gram(dt, c.k, len(c.subsets[t]), c.b, c.p)[2], who)
    assert outside_kept(snaps, c), 'rows outside idx were written'


def _split_T(r, dt):
    sh = r.sh
    mb = sh.get('mb', sh['b'])
    return max(launch_gemm_dense(dt, misaligned(dt, sh.get('ldx', sh['p']), sh.get('base', 0)), misaligned(dt, sh['k']), min(mb, sh['b']), sh['k'],
                                 sh['p'], split_scratch_elems(mb, sh['k'], sh['p']))[2], 1)


def _split_G(r, dt):
    return launch_gemm(dt, r.sh['k'], r.sh['k'], r.sh['p'], split_scratch_elems(64, r.sh['k'], r.sh['p']))[2]


def _with_resident_switch(c, f):
    from modl_amd._lib import lib, check, DEBUG_STATS_RESIDENT
    if c.probe != 'S-stats' or c.resident:
        return f()
    try:
        check(lib.modl_debug_set(DEBUG_STATS_RESIDENT, 0))
        return f()
    finally:
        check(lib.modl_debug_set(DEBUG_STATS_RESIDENT, 1))


SMALL_POINTS = [c for c in POINTS if c[0] != 'G-big']


def NAN_ROWS(b):
    """nan_row: row 0, so that element [0, 0] - what the K-tail and edge lanes of the dense TileLoader fetch for every row
    before they select zeros - is NaN.  (A NaN fetched for a ROW outside the operand lands in a tile row that is never
    stored, whatever the loader does: only the K direction can leak, and the poison behind each row covers the clamped fetch.)"""
    return (0,)


def _scenes_of(r):
    scenes = ['gaussian']
    if r.probe in ('T', 'G', 'S-code'):
        scenes.append('integers')
    if r.rep:
        scenes.append('scales')
    return scenes


def _run_point(r, dt, dev):
    who = family(r, dt)
    lib_s = library_route(r.probe, dt, **{a: v for a, v in r.sh.items() if a != 'steps'})
    assert lib_s == route_of(r, dt), ('the library, next to the device, routes this point otherwise', lib_s, route_of(r, dt))
    for scene in _scenes_of(r):
        c = make_case(r, dt, scene)
        if r.probe == 'T':
            got = run_T(c, dev)
            judge_T(c, got, _split_T(r, dt), who)
            assert same_bits(got, run_T(c, dev)), ('a second identical call gave other bits', scene)
            if scene == 'gaussian':
                assert same_bits(got, run_T(c, dev, poison=True)), 'the poison changed the result'
                for row in NAN_ROWS(c.b):
                    Xn = c.X.copy()
                    Xn[row] = np.nan
                    bad = run_T(c, dev, X=Xn)
                    others = np.delete(np.arange(c.b), row)
                    assert not np.isfinite(bad[row]).any() and same_bits(bad[others], got[others]), ('a NaN row of X left its row', row)
        elif r.probe == 'G':
            got = run_G(c, dev)
            judge_G(c, got, _split_G(r, dt), who)
            assert same_bits(got, run_G(c, dev)), ('a second identical call gave other bits', scene)
            if scene == 'gaussian':
                assert same_bits(got, run_G(c, dev, poison=True)), 'the poison changed the result'
        else:
            snaps = _with_resident_switch(c, lambda: run_S(c, dev))
            judge_S(r, c, snaps, who)
            again = _with_resident_switch(c, lambda: run_S(c, dev))
            assert state_bits(snaps, c) == state_bits(again, c), ('a second identical call gave other bits', scene)
            if 'ride:after[' in route_of(r, dt) and scene == 'gaussian':
                # the rider that no launch of the dictionary update consumed is completed behind it (phase2), counted under
                # dict_update: as many launches more than the same step without a rider as stats_pair takes for B_ alone
                extra = stats_pair(dt, c.k, c.p, c.ldx, c.base, c.b, split_scratch_elems(c.b, c.k, c.p), 'skip', M0=0)[1]
                c.flags |= NO_RIDER
                plain = run_S(c, dev)
                c.flags &= ~NO_RIDER
                assert snaps[1].launches['dict_update'] == plain[1].launches['dict_update'] + extra, \
                    ('launches of the dictionary update with and without the rider', snaps[1].launches, plain[1].launches, extra)
                judge_stats(c, plain[0], plain[1])
            if scene == 'gaussian':
                poisoned = _with_resident_switch(c, lambda: run_S(c, dev, poison=True))
                assert state_bits(snaps, c, True) == state_bits(poisoned, c, True), 'the poison changed the result'
                assert outside_kept(poisoned, c), 'poisoned rows outside idx were written'
                if r.probe == 'S-code' and c.agg == 'average':
                    for row in NAN_ROWS(c.b):
                        Xn = c.X.copy()
                        Xn[row] = np.nan
                        bad = run_S(c, dev, X=Xn)[1]
                        others = np.delete(np.arange(c.b), row)
                        assert not np.isfinite(bad.Dx_average[c.idx[row]]).any(), ('the NaN row came back finite', row)
                        assert same_bits(bad.Dx_average[c.idx[others]], snaps[1].Dx_average[c.idx[others]]), \
                            ('a NaN row of X left its row of Dx_average', row)
                        assert same_bits(bad.G_average, snaps[1].G_average), ('a NaN row of X reached G_average', row)
    _report()


@pytest.mark.gpu
@pytest.mark.parametrize('name,dt', SMALL_POINTS, ids=['%s-%s' % c for c in SMALL_POINTS])
def test_route(gpu, name, dt):
    _run_point(ROUTE_BY_KEY[name, dt], dt, gpu)


@pytest.mark.gpu
def test_route_big_tiles(gpu):
    """G at k = 2820, p = 24: 23 x 23 tiles of 128 x 128, no split (its plan holds 2 GB of split-K scratch: a test of its own)."""
    _run_point(ROUTE_BY_KEY['G-big', 'f32'], 'f32', gpu)


@pytest.mark.gpu
@pytest.mark.parametrize('dt', BOTH)
def test_probe_is_transparent(gpu, dt):
    """Probe T on the integer scene returns the exact integers at a dense, a misaligned and a gather point: the ridge solve of
    the identity system adds no rounding there, so what probe T shows elsewhere is the product."""
    for name in ('T-split' if dt == 'f32' else 'T-split64', 'T-unal_base', 'T-minimal'):
        r = ROUTE_BY_KEY[name, dt]
        c = make_case(r, dt, 'integers')
        judge_exact(run_T(c, gpu), c.X.dot(c.D.T))
