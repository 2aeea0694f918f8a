"""The masked-row kernels route by route: modl_masked_gram_* (modl_amd/csrc/masked_gram.hip), modl_masked_stats_*
(modl_amd/csrc/masked_stats.hip), the chunk loop of modl_somf_masked_step (modl_amd/csrc/somf_step.hip) and its two Python twins,
HipBackend.transform_masked and the masked branch of HipBackend.omp (modl_amd/dict_fact.py).  Every result is compared element by
element with the same expression in np.longdouble, or bit by bit with the same kernels called on other row ranges.

ROUTES (`GRAM_POINTS`, `STATS_POINTS`, `STEP_POINTS`; `test_route_table` holds every point to `expected_route`, a restatement of
the dispatch, and every leaf of the restatement to at least one point; the same table is in DESIGN.md, section 24).  A leaf is a
branch of the restatement, marked where it is taken by a call of `_leaf`; the list of all leaves is read out of this file's own
text.  `UNREACHED` lists, with the reason, the leaves that no point takes.  Lines as of this commit, in modl_amd/csrc:
G = masked_gram.hip, M = masked_stats.hip; somf_step.hip is cited by function name.
  G:49-53    tile        ntile = ceil(k / 64); ntile (ntile + 1) / 2 workgroups per sample, the upper triangle numbered row by row:
                         `while (tc >= ntile - ta)`; closed form ta = floor((2 ntile + 1 - sqrt((2 ntile + 1)^2 - 8 t)) / 2),
                         tc = t - ta ntile + ta (ta - 1) / 2 + ta (`gram_tile`, checked against the loop for ntile = 1 .. 16);
                         ta == tc: diagonal (upper half written to both sides, G:115), else mirrored (G:117-121); ta == 0: the
                         tile carries Dx (G:77-82, 85-89, 98-106)
  G:55-58    count       m_i over e < p (never the ldo padding), r_i = p / m_i in the dtype, 0 for an empty row (G:94-96)
  G:64-83    staging     K-steps of 16 rows of Dt, zeros selected for an unobserved row, for e >= p (K tail p % 16) and for an
                         atom >= k (edge tile k % 64)
  G:129-136  launches    ceil(b / 65535), the later ones with ii0 into rows, G, Dx and nobs
  M:167-174  stats       R = 2 (64 x 64 tiles) iff ceil(p / 64) ceil(k / 64) >= 512, else R = 1 (32 x 32); grid ceil(k / BT) x
                         ceil(p / BT); refusal ceil(p / 64) > 65535 on the R = 2 branch (M:168)
  M:49-60    observers   NS = 256 / BT row slices: 8 for R = 1 (lanes l and l + 32 folded by the cross-lane exchange), 4 for R = 2
  M:65-79    staging     K-steps of 16 samples; zeros selected for an unobserved element, a sample >= b (K tail b % 16), a
                         feature >= p, an atom >= k
  M:85-98    weights    seen = feature_n_iter[e] + c_e (read, never written here), w_e = min(1, w (c_e / b) (n_iter / seen)),
                         alpha = w_e / c_e, beta = 1 - w_e in f64, rounded to the dtype; c_e = 0: the row is not touched
  M:112-121  counts      feature_n_iter[e] += c_e where c_e > 0, count[e] = c_e when given, after the product on the stream
  masked_chunk_rows      clamp(256 MiB / (k k sizeof T), 1, 4096) - HipBackend.masked_chunk_rows in Python
  masked_step            workspace: crows = min(chunk rows, max_batch); need_F = ridge codes and 128 < k <= 512 (neither the blocked nor the
                         one-launch factorisation): a second block of crows k k for the factors
  masked_step            chunks: ceil(b / crows); chunk r0 uses X + r0 ldx, obs + r0 ldo, Dx + r0 k, nobs + r0, xnorm + r0, d_sweeps + r0
                         and d_idx + r0 (or code + r0 k without h_sample_idx)

  gram k       (k, p) = (1, 33) (63, 17) (64, 16) (65, 36) (127, 15) (128, 200) (129, 20) (5, 1) (1023, 17) (1024, 36): ntile 1, 1,
               1, 2, 2, 2, 3, 1, 16, 16; p % 16 in {0, 1, 4, 8, 15}; p < 16; k = 1023, 1024 with b = 2
  gram layout  tight: rows NULL, ldx = ldo = p; loose: rows a permutation with a repeat into a larger X, ldx = p + 3, ldo = p + 5
               (k 65 and k 128 both ways)
  gram launch  k 2 p 5, b = 65 535 (one launch), 65 536, 65 540 (two) through rows cycling over eight rows, 65 540 with rows NULL
  stats R = 1  (k, p, b) = (1, 1, 1) (31, 33, 15) (32, 32, 16) (33, 65, 17) (70, 193, 33) (1024, 1984, 9: 496 tiles of 64 x 64)
               (64, 32704, 5: 511)
  stats R = 2  (1024, 2048, 9) (961, 1985, 17: edge tiles both ways) (64, 32705, 5: 512) and, f32, (1, 4194240, 1): the
               largest grid, ceil(p / 64) = 65 535
  stats layout tight: rows NULL, ldx = ldo = p; loose: rows a permutation, ldx = p + 3, ldo = p + 1; d_count NULL or given
               ((70, 193, 33) and (961, 1985, 17) in every combination)
  stats refusal (1, 4194241, 1): MODL_EINVAL before any device work (`test_stats_refusal`, host pointers, no GPU)
  step         k 1024 p 64: f64 b = max_batch = 35 (32 + 3 rows) ridge with h_sample_idx / without, and with code_l1_ratio 1;
               f32 b = 70 (64 + 6) ridge; f64 b = 32 and 33 (one chunk / 32 + 1); max_batch = b = 10 (crows = max_batch); k 256
               ridge, b = 10 (the factor block behind the Gram block)
  twins        Coder at k 1024 p 64 f64: masked_chunk_rows() + 3 = 35 holed rows between clean and empty ones, enet and omp

SCENES
  integers   Dt, X and code uniform in {-3 .. 3}.  Gram: masks with p / m_i a power of two (m_i in {p, p / 2, p / 4} where p
             divides, an empty row always; one more mask per other divisor m_i of p, r_i an integer - all an odd p has): G and
             Dx are the exact integers bitwise, G bitwise symmetric.  Stats: c_e a power of
             two or 0 and the weight forced to the clamp (n_iter = 10^6): Bt is bitwise sum / c_e where observed, bit-unchanged
             where c_e = 0; at (32, 32, 16) once more with the raw weight exactly 1 (w = 0.5, everybody observes, seen = n_iter / 2).
  gaussian   the control, judged by the bound element by element.  Its masks ARE the adversarial patterns (`masks` of the
             issue): per row fully observed, empty, only element 0, only element p - 1, only the K tail, all but the K tail, a
             16-block unobserved between observed ones, alternating, then Bernoulli(1/2) rows; for stats per feature: nobody,
             everybody, one observer for every row residue mod 8 and for row b - 1, observers in the last K-step only.
  scales     rows of X and atoms scaled by 10^U(-3, 3) (f64: 10^U(-6, 6)); representative points (`rep`).  Stats: the weight
             at the clamp, as under integers (an increment far below the rounding of the old value would be judged by nothing).
  bytes      the observed bytes drawn from {1, 2, 0x80, 0xFF}: the bits of the gaussian call (all of nobs, G, Dx; d_count,
             feature_n_iter, Bt).
  poison     NaN and Inf alternating at every unobserved position of X: the bits of the gaussian call (finite values there).
  nan_row    a NaN at an observed entry of one row.  Gram: that sample's Dx is non-finite throughout, its G and every other
             sample keep their bits.  Stats: the rows of Bt of the features where the NaN is observed are non-finite, every
             other row keeps its bits.
  Every call is made twice and gives identical bits.  Canaries that keep their bits on every call: one sample slot behind G, Dx
  and nobs, one row behind Bt, entries behind feature_n_iter and d_count; the inputs themselves, with NaN in the ldx - p padding
  of X, 1 in the ldo - p padding of obs, and NaN / 1 in the rows of X / obs outside `rows`.

JUDGES (ref in np.longdouble from the inputs as given, eps the dtype's machine epsilon; nothing of the code under test enters)
  exact   as above.
  gram    |G - ref| <= (m_i + 4) eps A, A = r_i sum_{e in M_i} |Dt[e][a]| |Dt[e][c]|; Dx with |X[i][e]| for one factor: m_i - 1
          additions (zeros selected in add exactly), one rounding of each product, of r_i and of the scaling.
  stats   |Bt - ref| <= (c_e + 6) eps (|beta_e| |Bt0[e][a]| + |alpha_e| sum_{i observes e} |x_ie| |code_i[a]|), beta_e and alpha_e
          in f64 in the header's order of operations.
  `test_judges_on_the_oracle` (CPU): numpy's same-dtype restatement (product in the dtype, scaling after the sum, beta / alpha
  rounded to the dtype) is within the bound on every scene and shape of the table; no constant had to grow.  Dropping the
  single largest term of an element leaves the bound: in every element (that has a non-zero term) of the Gram scenes and of
  the statistics where beta = 0 (integers, scales), since the largest of m terms is at least A / m and 1 / m > (m + 6) eps at
  every m of the table.  Next to an old value (gaussian statistics) an element whose terms are all below the rounding of
  beta Bt0 shows a dropped term to no judge; there the dropped term is over the product's share of the bound, (c_e + 6) eps
  |alpha_e| sum |x||code|, in every element, and over the whole bound somewhere in every feature row (k >= 8).

LAYER 3
  step    the codes of every non-empty row are, bit for bit, those of modl_masked_gram_* + modl_enet_regression_multi_gram_* called
          here on the same two row ranges with the same arguments (X + r0 ldx, obs + r0 ldo, rows NULL, the warm start code_[idx]).
          The one argument that is not the same is the solver's squared row norm under code_l1_ratio = 1 (the step:
          masked_row_norm2_kernel, the ABI: row_norm2_kernel on the zero-filled rows, other orders of summation); the scene
          makes both exact - X in multiples of 1 / 4, sums of squares exact in f64 - so the bits must match there too, sweep
          counts included.  An empty row's code is exactly zero (its warm start overwritten), rows of code_ outside the batch
          keep their bits, feature_n_iter is exact, C_ and every row of B_ are within the bound from the device's own codes
          (C_: (b + 6) eps on (1 - w) |C0| + (w / b) |code|^T |code|), modl_somf_last_sweeps returns b counts.
  twins   every holed row of Coder.transform(X, mask) and of algorithm='omp' equals the row obtained when its chunk's rows are
          submitted alone.

MEASURED (largest |got - ref| / bound per route on the MI355X, f32 / f64, from this file's own run - `_report` prints them;
recorded, not asserted).  73 GPU cases in 13 s, none above 1.6 s.
  gram ntile 1   G 0.179 / 0.171, Dx 0.162 / 0.156        gram ntile 2   G 0.184 / 0.189, Dx 0.154 / 0.162
  gram ntile 3   G 0.175 / 0.179, Dx 0.150 / 0.172        gram ntile 16  G 0.214 / 0.210, Dx 0.186 / 0.171
  stats R = 1    0.218 / 0.178                            stats R = 2    0.217 / 0.202
  step           B_ 0.053 / 0.101, C_ 0.016 / 0.082
  numpy's same-dtype restatement on the CPU (`test_judges_on_the_oracle`): gram 0.214 / 0.210, stats 0.218 / 0.202 of the bound.
  The device's largest ratios are the restatement's: they belong to elements of one or two terms (`only element 0`, a single
  observer), whose few roundings do not depend on the order of a sum.

MUTANTS (`test_mutants`, on `gram_restated`, `stats_restated` and `chunked`, numpy restatements of the tile loops at 8 x 8 tiles,
K-steps of 4 and eight observer slices).  Mutant -> the scene and judge that reject it:
  a tile below the diagonal left unmirrored         integers (exact)
  a diagonal tile mirrored from its lower half      INVISIBLE (asserted): both operands of a diagonal tile are the same rows, so
                                                    the lower half holds the same products summed in the same order
  the K tail (p % 16, b % 16) dropped               integers (exact), gaussian (bound): masks `only the K tail`, `last K-step only`
  the K tail read past the end                      integers (exact: the rows behind hold other numbers) and the NaN padding of X
  m_i counted over the ldo padding                  integers (exact) in the loose layout.  INVISIBLE at ldo = p (asserted)
  Dx taken from accumulator row 1                   integers (exact), gaussian (bound): it is zero
  Dx written by every tile row                      INVISIBLE (asserted): every tile row forms the same sum from the same operand
                                                    tile; the same bits are written again
  zeros multiplied instead of selected              poison.  INVISIBLE while the places hold finite values (asserted)
  one observer slice lost; the odd slices lost      gaussian (bound) and integers (exact) through the one-observer features, one
                                                    per residue mod 8: the row keeps its old bits
  c_e from rows 0 .. b-1, the product from rows[]   gaussian (bound) in the loose layout.  INVISIBLE with rows NULL (asserted)
  feature_n_iter written before it is read          gaussian (bound) where the clamp does not bind.  INVISIBLE where it binds
                                                    (asserted: the integer scene)
  the clamp min(1, .) left out                      integers (exact).  INVISIBLE where the raw weight is below 1 (asserted)
  w_e / b instead of w_e / c_e                      integers (exact), gaussian (bound).  INVISIBLE on a feature that everybody
                                                    observes (asserted)
  a byte of 2 read as unobserved by one kernel      bytes (the product, the count or the counts kernel alone: other bits than with
                                                    bytes of 1); on the device the step under code_l1_ratio = 1 adds the row norms
  the second chunk reading rows 0 .. c-1 again      gaussian (bound), integers (exact) on the rows of the second chunk
"""
import ctypes as C
import re
import zlib
from types import SimpleNamespace

import numpy as np
import pytest

DT = {'f32': np.float32, 'f64': np.float64}
LD = np.longdouble
BOTH = ('f32', 'f64')
FILL = 7.5
EINVAL = -1
MAX_Y = 65535                                  # samples per launch of masked_gram (G:130), tile rows of masked_stats (M:168)


def cdiv(a, b):
    return -(-a // b)


HIT = set()                                    # the branches of the restated dispatch taken since the last HIT.clear()


def _leaf(name):
    """Marks a branch of the restatement.  `all_leaves` reads the names out of this file's own text, so a branch that is
    written down here cannot be left out of the completeness assertion of `test_route_table`."""
    HIT.add(name)
    return name


def all_leaves():
    with open(__file__.replace('.pyc', '.py')) as f:
        return set(re.findall(r"_leaf\('([^']+)'\)", f.read()))


# ---------------------------------------------------------------------------------------------------- the dispatch, restated
def gram_tile_loop(t, ntile):                  # G:49-51, as written there
    ta, tc = 0, t
    while tc >= ntile - ta:
        tc -= ntile - ta
        ta += 1
    return ta, tc + ta


def _isqrt_up(n):
    s = int(np.sqrt(float(n)))
    while s * s > n:
        s -= 1
    while s * s < n:
        s += 1
    return s


def gram_tile(t, ntile):
    """tile t of the upper triangle numbered row by row, in closed form: row ta starts at ta ntile - ta (ta - 1) / 2"""
    ta = (2 * ntile + 1 - _isqrt_up((2 * ntile + 1) ** 2 - 8 * t)) // 2
    return ta, t - (ta * ntile - ta * (ta - 1) // 2) + ta


def gram_route(k, p, b, rows):
    if k < 1 or k > 1024 or p < 1 or b < 0:                                  # G:127
        return SimpleNamespace(s=_leaf('gram/einval'), launches=0)
    ntile = cdiv(k, 64)                                                      # G:129
    wg = ntile * (ntile + 1) // 2
    kinds = []
    for t in range(wg):
        ta, tc = gram_tile(t, ntile)
        if ta == tc:
            kinds.append(_leaf('gram/diag+dx') if ta == 0 else _leaf('gram/diag'))
        else:
            kinds.append(_leaf('gram/mirrored+dx') if ta == 0 else _leaf('gram/mirrored'))
    launches = cdiv(b, MAX_Y)                                                # G:131-136
    s = 'gram/ntile%d/wg%d/diag%d/dx%d/' % (ntile, wg, sum('diag' in x for x in kinds), sum('+dx' in x for x in kinds))
    s += _leaf('gram/relaunch') if launches > 1 else _leaf('gram/one_launch')
    s += '%d/' % launches
    s += (_leaf('gram/rows') if rows else _leaf('gram/rows_null')) + '/'
    s += (_leaf('gram/ktail') if p % 16 else _leaf('gram/kfull')) + '/'
    s += _leaf('gram/edge') if k % 64 else _leaf('gram/interior')
    return SimpleNamespace(s=s, launches=launches, ntile=ntile, wg=wg)


def stats_route(k, p, b, rows, count):
    if k < 1 or k > 1024 or p < 1 or b < 0:                                  # M:164
        return SimpleNamespace(s=_leaf('stats/einval'), rc=EINVAL)
    if cdiv(p, 64) * cdiv(k, 64) >= 512:                                     # M:167
        if cdiv(p, 64) > MAX_Y:                                              # M:168
            return SimpleNamespace(s=_leaf('stats/R2/refused'), rc=EINVAL)
        R, s = 2, _leaf('stats/R2')
    else:
        R, s = 1, _leaf('stats/R1')
    BT = 32 * R
    grid = (cdiv(k, BT), cdiv(p, BT))                                        # M:169, 172
    NS = 256 // BT                                                           # M:50
    s += '/grid%dx%d/' % grid
    s += (_leaf('stats/NS8') if NS == 8 else _leaf('stats/NS4')) + '/'
    s += (_leaf('stats/rows') if rows else _leaf('stats/rows_null')) + '/'
    s += (_leaf('stats/count') if count else _leaf('stats/count_null')) + '/'
    s += (_leaf('stats/ktail') if b % 16 else _leaf('stats/kfull')) + '/'
    s += (_leaf('stats/edge_p') if p % BT else _leaf('stats/full_p')) + '/'
    s += _leaf('stats/edge_k') if k % BT else _leaf('stats/full_k')
    return SimpleNamespace(s=s, rc=0, R=R, BT=BT, grid=grid, NS=NS)


def masked_chunk_rows(k, tsz):                                               # masked_chunk_rows
    r = (256 << 20) // (k * k * tsz)
    return 1 if r < 1 else (4096 if r > 4096 else r)


def step_route(dt, k, b, max_batch, l1_ratio, has_idx):
    tsz = 4 if dt == 'f32' else 8
    full = masked_chunk_rows(k, tsz)
    crows = min(full, max_batch)                                             # masked_step
    s = (_leaf('step/crows=chunk_rows') if crows == full else _leaf('step/crows=max_batch')) + '%d/' % crows
    # need_F (masked_step) as far as the workspace needs it: ridge codes whose systems take neither the blocked factorisation
    # (chol_blocked, per-sample matrices: k > 512) nor the one-launch one (ridge_small_applies: k <= 128 in both types)
    need_F = l1_ratio == 0 and not k > 512 and not k <= 128
    s += (_leaf('step/ws2') if need_F else _leaf('step/ws1')) + '/'
    chunks = cdiv(b, crows)                                                  # masked_step's chunk loop
    s += (_leaf('step/chunks') if chunks > 1 else _leaf('step/one_chunk')) + '%d/' % chunks
    if need_F and chunks > 1:
        s += _leaf('step/chunks+ws2') + '/'
    s += (_leaf('step/xnorm') if l1_ratio != 0 else _leaf('step/ridge')) + '/'
    s += _leaf('step/idx') if has_idx else _leaf('step/code+r0k')
    ws = (2 if need_F else 1) * cdiv(tsz * crows * k * k, 256) * 256 + cdiv(4 * max_batch, 256) * 256      # masked_step
    return SimpleNamespace(s=s, crows=crows, chunks=chunks, ws=ws, ranges=[(r0, min(crows, b - r0)) for r0 in range(0, b, crows)])


def expected_route(probe, dt, **sh):
    if probe == 'gram':
        return gram_route(sh['k'], sh['p'], sh['b'], sh['layout'] != 'tight').s
    if probe == 'stats':
        return stats_route(sh['k'], sh['p'], sh['b'], sh['layout'] != 'tight', sh['count']).s
    return step_route(dt, sh['k'], sh['b'], sh['mb'], sh['l1'], sh['idx']).s


POINTS = []


def _point(probe, name, want, dts=BOTH, rep=False, **sh):
    POINTS.append(SimpleNamespace(probe=probe, name=name, want=want, dts=dts, rep=rep, sh=sh))


def _g(name, k, p, layout, want, b=None, **kw):
    _point('gram', name, want, k=k, p=p, layout=layout, b=b or 10, **kw)


_g('g-k1', 1, 33, 'tight', ('ntile1/wg1/diag1/dx1', 'ktail', 'edge', 'rows_null'))
_g('g-k63', 63, 17, 'loose', ('ntile1/', 'ktail', 'edge', 'gram/rows/'))
_g('g-k64', 64, 16, 'tight', ('ntile1/', 'kfull', 'interior'))
_g('g-k65', 65, 36, 'tight', ('ntile2/wg3/diag2/dx2', 'edge'), rep=True)
_g('g-k65-loose', 65, 36, 'loose', ('ntile2/wg3/diag2/dx2', 'gram/rows/'))
_g('g-k127', 127, 15, 'loose', ('ntile2/', 'ktail', 'edge'))
_g('g-k128', 128, 200, 'tight', ('ntile2/', 'ktail', 'interior'), rep=True)
_g('g-k128-loose', 128, 200, 'loose', ('ntile2/', 'interior', 'gram/rows/'))
_g('g-k129', 129, 20, 'loose', ('ntile3/wg6/diag3/dx3', 'edge'))
_g('g-p1', 5, 1, 'tight', ('ntile1/', 'ktail'))
_g('g-k1023', 1023, 17, 'loose', ('ntile16/wg136/diag16/dx16', 'edge'), b=2)
_g('g-k1024', 1024, 36, 'tight', ('ntile16/wg136/diag16/dx16', 'interior'), b=2)
_g('g-launch-65535', 2, 5, 'cycle', ('one_launch1/',), b=65535, launch=True)
_g('g-launch-65536', 2, 5, 'cycle', ('relaunch2/',), b=65536, launch=True)
_g('g-launch-65540', 2, 5, 'cycle', ('relaunch2/', 'gram/rows/'), b=65540, launch=True)
_g('g-launch-65540-null', 2, 5, 'tight', ('relaunch2/', 'rows_null'), b=65540, launch=True)


def _s(name, k, p, b, layout, count, want, **kw):
    _point('stats', name, want, k=k, p=p, b=b, layout=layout, count=count, **kw)


_s('s-1', 1, 1, 1, 'tight', False, ('stats/R1/grid1x1/', 'NS8'))
_s('s-31', 31, 33, 15, 'loose', True, ('stats/R1/grid1x2/', 'ktail', 'edge_p', 'edge_k'))
_s('s-32', 32, 32, 16, 'tight', True, ('stats/R1/grid1x1/', 'kfull', 'full_p', 'full_k'))
_s('s-33', 33, 65, 17, 'loose', False, ('stats/R1/grid2x3/', 'ktail'))
_s('s-70', 70, 193, 33, 'loose', True, ('stats/R1/grid3x7/', 'stats/rows/', 'stats/count/'), rep=True)
_s('s-70-tight', 70, 193, 33, 'tight', False, ('stats/R1/grid3x7/', 'rows_null', 'count_null'))
_s('s-70-tight-count', 70, 193, 33, 'tight', True, ('stats/R1/', 'rows_null', 'stats/count/'))
_s('s-70-loose-nocount', 70, 193, 33, 'loose', False, ('stats/R1/', 'stats/rows/', 'count_null'))
_s('s-496', 1024, 1984, 9, 'tight', True, ('stats/R1/grid32x62/',), big=True)
_s('s-511', 64, 32704, 5, 'loose', True, ('stats/R1/grid2x1022/',), big=True)
_s('s-512', 64, 32705, 5, 'loose', True, ('stats/R2/grid1x512/', 'NS4', 'edge_p', 'full_k'), big=True)
_s('s-R2', 1024, 2048, 9, 'tight', False, ('stats/R2/grid16x32/', 'full_p', 'full_k', 'rows_null', 'count_null'), big=True)
_s('s-R2-edge', 961, 1985, 17, 'loose', True, ('stats/R2/grid16x32/', 'edge_p', 'edge_k', 'stats/rows/', 'stats/count/'), big=True, rep=True)
_s('s-R2-edge-tight', 961, 1985, 17, 'tight', True, ('stats/R2/grid16x32/', 'rows_null', 'stats/count/'), big=True)
_s('s-R2-edge-nocount', 961, 1985, 17, 'loose', False, ('stats/R2/grid16x32/', 'stats/rows/', 'count_null'), big=True)
_s('s-R2-maxgrid', 1, MAX_Y * 64, 1, 'tight', False, ('stats/R2/grid1x65535/',), dts=('f32',), big=True, only_gaussian=True)
_s('s-refused', 1, MAX_Y * 64 + 1, 1, 'tight', False, ('stats/R2/refused',), host=True)


def _t(name, dt, b, want, l1=0.0, idx=True, mb=35, k=1024):
    _point('step', name, want, dts=(dt,), k=k, p=64, b=b, mb=mb, l1=l1, idx=idx)


_t('t-ridge', 'f64', 35, ('crows=chunk_rows32/', 'ws1', 'chunks2/', 'step/ridge', 'step/idx'))
_t('t-ridge-noidx', 'f64', 35, ('chunks2/', 'step/ridge', 'code+r0k'), idx=False)
_t('t-l1', 'f64', 35, ('chunks2/', 'step/xnorm', 'step/idx'), l1=1.0)
_t('t-ridge32', 'f32', 70, ('crows=chunk_rows64/', 'chunks2/', 'step/ridge'), mb=70)
_t('t-one', 'f64', 32, ('one_chunk1/',))
_t('t-33', 'f64', 33, ('chunks2/',))
_t('t-max-batch', 'f64', 10, ('crows=max_batch10/', 'one_chunk1/'), mb=10)
_t('t-factors', 'f64', 10, ('crows=max_batch10/', 'ws2', 'one_chunk1/'), mb=10, k=256)

POINT_BY_KEY = {(r.name, dt): r for r in POINTS for dt in r.dts}
UNREACHED = {
    'gram/einval': 'k, p, b outside the entry point\'s domain: MODL_EINVAL before any launch, covered by the EINVAL tests of tests/test_inpaint.py',
    'stats/einval': 'as above, tests/test_masked_fit.py::test_masked_entry_points_are_einval_before_any_device_work',
    'step/chunks+ws2': 'a second chunk next to the factor block needs b > masked_chunk_rows(k <= 512) >= 128 rows with a Gram matrix and a '
                       'factor of up to 2 MiB each; the factor block is indexed by the sample within the chunk, not by r0, so a second '
                       'chunk adds no address to it that t-factors (one chunk) does not use',
}


def route_of(r, dt):
    return expected_route(r.probe, dt, **{k: v for k, v in r.sh.items() if k in ('k', 'p', 'b', 'layout', 'count', 'mb', 'l1', 'idx')})


# ---------------------------------------------------------------------------------------------------- scenes
def _seed(*what):
    return zlib.crc32(('masked-' + '-'.join(str(w) for w in what)).encode()) % 100000


def draw(scene, rs, rows, cols, dt):
    """(rows, cols) operand of a scene, as float64 values that the dtype holds exactly after the cast"""
    if scene == 'integers':
        return rs.randint(-3, 4, size=(rows, cols)).astype(np.float64)
    a = rs.randn(rows, cols)
    if scene == 'scales':
        span = 3 if dt == 'f32' else 6
        a = a * (10.0 ** rs.uniform(-span, span, rows))[:, None]
    return a.astype(DT[dt]).astype(np.float64)


def gram_patterns(p):
    """the adversarial rows of a mask over p features, each a bool vector"""
    e = np.arange(p)
    t0 = 16 * (p // 16) if p % 16 else max(p - 16, 0)                        # the last K-step: the tail, or the last full one
    tail = e >= t0
    hole = ~((e >= 16) & (e < 32)) if p > 32 else ~(e < min(16, p // 2))      # a whole 16-block out between observed ones
    return [np.ones(p, bool), np.zeros(p, bool), e == 0, e == p - 1, tail, ~tail, hole, e % 2 == 0]


def gram_int_masks(p, rs):
    """masks with p / m a power of two: m in {p, p / 2, p / 4} where p divides, structured and random; one empty row; and one
    mask per other divisor m of p (an odd p has no other exact ratio), element p - 1 always among its entries"""
    e = np.arange(p)
    out = [np.ones(p, bool), np.zeros(p, bool)]
    for q in (2, 4):
        if p % q == 0:
            out.append(e % q == q - 1)                                       # (holds element p - 1: inside the K tail)
            for _ in range(2):
                m = np.zeros(p, bool)
                m[rs.permutation(p)[:p // q]] = True
                out.append(m)
    for m_ in (d for d in range(1, p) if p % d == 0 and p // d not in (2, 4)):
        m = np.zeros(p, bool)                                                # and any other divisor: r = p / m is an integer, as exact
        m[np.append(rs.permutation(p - 1)[:m_ - 1], p - 1).astype(int)] = True
        out.append(m)
    out.append(np.ones(p, bool))
    return out


def make_gram_case(r, dt, scene):
    sh = r.sh
    k, p, layout = sh['k'], sh['p'], sh['layout']
    rs = np.random.RandomState(_seed(r.name, dt, scene))
    Dt = draw(scene, rs, k, p, dt).T.copy()                                  # (p, k); `scales` scales the atoms
    if sh.get('launch'):                                                     # eight source rows, b samples cycling over them
        masks = [m for m in gram_patterns(p)]
        src = 8
        b = sh['b']
        n = src + 2 if layout == 'cycle' else b + 1
    elif scene == 'integers':
        masks = gram_int_masks(p, rs)
        src = len(masks)
    else:
        masks = gram_patterns(p) + [rs.rand(p) < 0.5, rs.rand(p) < 0.5]
        src = len(masks)
    if not sh.get('launch'):
        if sh['b'] < src:                                                    # the big dictionaries: two rows, holed ones
            pick = [4, 6] if scene != 'integers' else [len(masks) - 2, 0]
            masks = [masks[i] for i in pick]
            src = len(masks)
        b = src + (1 if layout == 'loose' else 0)                            # loose: one source row twice
        n = src + 2
    c = SimpleNamespace(probe='gram', dt=dt, scene=scene, k=k, p=p, b=b, Dt=Dt, layout=layout)
    c.ldx, c.ldo = (p + 3, p + 5) if layout == 'loose' else (p, p)
    X = draw(scene, rs, n, p, dt)
    obs = np.ones((n, p), dtype=np.uint8)
    if layout == 'tight' and sh.get('launch'):
        obs[:] = np.array([masks[i % 8] for i in range(n)], dtype=np.uint8)
        X[:] = X[np.arange(n) % 8]
        c.rows = None
        c.src_of = np.arange(b) % 8
    elif layout == 'cycle':
        obs[:src] = np.array(masks, dtype=np.uint8)
        c.rows = (np.arange(b) % 8).astype(np.int64)
        c.src_of = c.rows
    elif layout == 'loose':
        at = rs.permutation(n)[:src]                                         # where the source rows lie in the X buffer
        obs[at] = np.array(masks, dtype=np.uint8)
        order = rs.permutation(src)
        c.rows = np.concatenate([at[order], at[order[:1]]]).astype(np.int64)
    else:
        obs[:src] = np.array(masks, dtype=np.uint8)
        c.rows = None
    c.X, c.obs, c.n = X, obs, n
    c.samples = np.arange(b) if c.rows is None else c.rows
    return c


def launch_source(r, dt):
    """(the eight source rows of a long batch as a case of their own, the long batch)"""
    c, small = make_gram_case(r, dt, 'gaussian'), make_gram_case(r, dt, 'gaussian')
    small.b = 8
    small.rows = None if c.rows is None else np.arange(8, dtype=np.int64)
    small.samples = np.arange(8)
    return small, c


def stats_masks(b, p, rs, scene):
    """(b, p) bool: column patterns.  integers: c_e a power of two (or 0); else the adversarial features and Bernoulli(1/2)"""
    on = np.zeros((b, p), dtype=bool)
    if scene == 'integers':
        sizes = [0] + [1 << j for j in range(0, 8) if (1 << j) <= b]
        for e in range(p):
            c = sizes[e % len(sizes)] if e < 2 * len(sizes) else sizes[rs.randint(len(sizes))]
            on[rs.permutation(b)[:c], e] = True
        if p >= 16:
            for i in range(min(b, 8)):                                       # one observer per residue (c_e = 1 is a power of two)
                on[:, 8 + i] = False
                on[i, 8 + i] = True
        return on
    on[:] = rs.rand(b, p) < 0.5
    if p >= 32:
        on[:, 0] = False                                                     # nobody
        on[:, 1] = True                                                      # everybody
        f = 2
        for i in sorted(set(range(min(b, 8))) | {b - 1}):                    # one observer: every residue mod 8, and row b - 1
            on[:, f] = False
            on[i, f] = True
            f += 1
        last = 16 * ((b - 1) // 16)                                          # observers in the last K-step only
        on[:, f] = False
        on[last:, f] = True
        on[:, p - 1] = False
        on[b - 1, p - 1] = True
    if p == 1:
        on[:] = True
    return on


def make_stats_case(r, dt, scene, variant=None):
    sh = r.sh
    k, p, b, layout = sh['k'], sh['p'], sh['b'], sh['layout']
    rs = np.random.RandomState(_seed(r.name, dt, scene))
    c = SimpleNamespace(probe='stats', dt=dt, scene=scene, k=k, p=p, b=b, layout=layout, count=sh['count'])
    c.ldx, c.ldo = (p + 3, p + 1) if layout == 'loose' else (p, p)
    c.n = b + (3 if layout == 'loose' else 1)
    c.rows = rs.permutation(c.n)[:b].astype(np.int64) if layout == 'loose' else None
    c.samples = np.arange(b) if c.rows is None else c.rows
    c.X = np.zeros((c.n, p))
    c.X[c.samples] = draw(scene, rs, b, p, dt)
    c.obs = np.ones((c.n, p), dtype=np.uint8)
    c.obs[c.samples] = stats_masks(b, p, rs, scene)
    c.code = draw('integers' if scene == 'integers' else 'gaussian', rs, b, k, dt)
    c.Bt0 = draw(scene if scene != 'scales' else 'gaussian', rs, p, k, dt)
    if scene in ('integers', 'scales'):                                      # the clamp binds on every observed feature
        c.w, c.n_iter, c.fni0 = 0.9, 10 ** 6, rs.randint(0, 10, size=p).astype(np.int64)
    else:
        c.w, c.n_iter = 0.35, 1000
        c.fni0 = rs.randint(1, 4000, size=p).astype(np.int64)                # uneven: the clamp binds for the rarely seen features
    if variant == 'raw1':                                                    # the raw weight exactly 1: 0.5 (b / b) (n_iter / (n_iter / 2))
        c.obs[c.samples] = 1
        c.w, c.n_iter, c.fni0 = 0.5, 4 * b, np.full(p, b, dtype=np.int64)
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


def same_bits(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def bits_symmetric(G):
    G = np.ascontiguousarray(G)
    return np.array_equal(G + 0.0, np.swapaxes(G, -1, -2) + 0.0)


def judge_exact(got, ref, what=''):
    """the exact values, bitwise apart from the sign of zero"""
    got = np.asarray(got, dtype=np.float64)
    bad = np.argwhere(~(got == ref))
    assert bad.size == 0, ('not the exact result', what, bad[:4], len(bad), got[tuple(bad[0])], ref[tuple(bad[0])])


def judge_bound(got, ref, bound, who=None, what=''):
    got = np.asarray(got)
    assert np.all(np.isfinite(got)), ('non-finite result', what, np.argwhere(~np.isfinite(got))[:4])
    err = np.abs(np.asarray(got, dtype=LD) - ref).astype(np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        ratio = np.where(err == 0, 0.0, err / np.where(bound == 0, 1e-300, bound))
    if who:
        _note(who, ratio.max() if ratio.size else 0.0)
    bad = np.argwhere(ratio > 1)
    assert bad.size == 0, ('over the bound', who, what, float(ratio.max()), bad[:4], len(bad))
    return float(ratio.max()) if ratio.size else 0.0


def gram_ref(c, want_drop=False):
    """per sample of the case: ref G, Dx in longdouble, the bounds, m_i; (want_drop: the largest term of every element)"""
    if getattr(c, '_ref', None) is not None and (c._ref[0] or not want_drop):
        return c._ref[1]
    eps = eps_of(c.dt)
    out = {}
    for i in np.unique(c.samples):
        M = np.flatnonzero(c.obs[i] != 0)
        m = len(M)
        if m == 0:
            out[i] = SimpleNamespace(m=0)
            continue
        DM, x = c.Dt[M], c.X[i, M]
        r = LD(c.p) / LD(m)
        o = SimpleNamespace(m=m)
        o.G = r * np.asarray(DM, dtype=LD).T.dot(np.asarray(DM, dtype=LD))
        o.Dx = r * np.asarray(x, dtype=LD).dot(np.asarray(DM, dtype=LD))
        o.bG = (m + 4) * eps * float(r) * np.abs(DM).T.dot(np.abs(DM))
        o.bDx = (m + 4) * eps * float(r) * np.abs(x).dot(np.abs(DM))
        if want_drop:
            dG, dDx = np.zeros((c.k, c.k)), np.zeros(c.k)
            for e in range(m):
                dG = np.maximum(dG, np.abs(np.outer(DM[e], DM[e])))
                dDx = np.maximum(dDx, np.abs(x[e] * DM[e]))
            o.dG, o.dDx = float(r) * dG, float(r) * dDx
        out[i] = o
    c._ref = (want_drop, out)
    return out


def judge_gram(c, G, Dx, nobs, who=None):
    ref = gram_ref(c)
    assert bits_symmetric(G), 'G is not bitwise symmetric'
    seen = {}
    for ii, i in enumerate(c.samples):
        o = ref[i]
        assert nobs[ii] == o.m, ('nobs', ii, i, nobs[ii], o.m)
        if i in seen:                                                        # a repeated row: the same bits
            assert same_bits(G[ii], G[seen[i]]) and same_bits(Dx[ii], Dx[seen[i]]), ('a repeated row gave other bits', ii, seen[i])
            continue
        seen[i] = ii
        if o.m == 0:
            assert not G[ii].any() and not Dx[ii].any(), ('an empty row is not zero', ii)
        elif c.scene == 'integers':
            judge_exact(G[ii], o.G.astype(np.float64), ('G', ii))
            judge_exact(Dx[ii], o.Dx.astype(np.float64), ('Dx', ii))
        else:
            judge_bound(G[ii], o.G, o.bG, who and who + ' G', ii)
            judge_bound(Dx[ii], o.Dx, o.bDx, who and who + ' Dx', ii)


def stats_weights(c_e, fni0, w, n_iter, b):
    """beta_e, alpha_e in f64, the operations in the order of M:90-93"""
    c_e = c_e.astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        seen = (fni0 + c_e.astype(np.int64)).astype(np.float64)
        we = w * (c_e / float(b)) * (float(n_iter) / seen)
        we = np.where(we < 1.0, we, 1.0)
        al = we / c_e
    we, al = np.where(c_e > 0, we, 0.0), np.where(c_e > 0, al, 0.0)
    return 1.0 - we, al, we


def stats_ref(c, code=None, want_drop=False):
    code = c.code if code is None else code
    on = c.obs[c.samples] != 0
    Xz = np.where(on, c.X[c.samples], 0.0)
    ce = on.sum(axis=0)
    beta, al, we = stats_weights(ce, c.fni0, c.w, c.n_iter, c.b)
    o = SimpleNamespace(c=ce, beta=beta, alpha=al, we=we, Xz=Xz, fni=c.fni0 + ce)
    o.ref = LD(1) * beta[:, None] * c.Bt0 + al[:, None] * np.asarray(Xz, dtype=LD).T.dot(np.asarray(code, dtype=LD))
    o.bound = (ce + 6)[:, None] * eps_of(c.dt) * (np.abs(beta)[:, None] * np.abs(c.Bt0) + np.abs(al)[:, None] * np.abs(Xz).T.dot(np.abs(code)))
    if want_drop:
        d = np.zeros((c.p, c.k))
        for i in range(c.b):
            d = np.maximum(d, np.abs(np.outer(Xz[i], code[i])))
        o.drop = np.abs(al)[:, None] * d
    return o


def judge_stats(c, Bt, fni, cnt, who=None, code=None):
    o = stats_ref(c, code)
    T = DT[c.dt]
    np.testing.assert_array_equal(fni, o.fni)
    if cnt is not None:
        np.testing.assert_array_equal(cnt, o.c)
    dead = o.c == 0
    assert same_bits(Bt[dead], c.Bt0.astype(T)[dead]), 'a row of Bt that nobody observes was written'
    live = ~dead
    if c.scene == 'integers':
        assert np.all(o.we[live] == 1.0), 'the scene does not force the clamp'
        sums = o.Xz.T.dot(c.code if code is None else code)
        judge_exact(Bt[live], (sums / np.maximum(o.c, 1)[:, None])[live], 'Bt')
    else:
        judge_bound(Bt[live], o.ref[live], o.bound[live], who, 'Bt')


# ---------------------------------------------------------------------------------------------------- the loops, restated (mutants)
def gram_restated(c, dt, mut=(), BT=8, BK=4, rows=None, X=None, obs=None, behind=None):
    """G, Dx, nobs as masked_gram_kernel forms them, at tiles of BT x BT and K-steps of BK: the triangle numbering, zeros
    SELECTED on the way in, the row of X as one more operand row whose accumulator row 0 is Dx, the scaled tile written as
    it is and mirrored.  The buffers carry the case's padding (X: NaN, obs: 1); `behind` is what follows Dt in memory."""
    T = DT[dt]
    k, p = c.k, c.p
    rows = c.samples if rows is None else rows
    X = c.X if X is None else X
    obs = c.obs if obs is None else obs
    n = X.shape[0]
    Xb = np.full((n, c.ldx), np.nan, dtype=T)
    Xb[:, :p] = X
    ob = np.ones((n, c.ldo), dtype=np.uint8)
    ob[:, :p] = obs
    De = np.vstack([c.Dt, np.full((BK, k), 5.0) if behind is None else behind]).astype(T)
    b, ntile = len(rows), cdiv(k, BT)
    G, Dx, nobs = np.full((b, k, k), FILL, dtype=T), np.full((b, k), FILL, dtype=T), np.full(b, -7, dtype=np.int32)
    seen = (lambda v: v == 1) if 'byte2_product' in mut else (lambda v: v != 0)
    counted = (lambda v: v == 1) if 'byte2_count' in mut else (lambda v: v != 0)
    M_, N_ = np.meshgrid(np.arange(BT), np.arange(BT), indexing='ij')
    with np.errstate(invalid='ignore'):
        for ii, i in enumerate(rows):
            o, x = ob[i], Xb[i]
            m = int(counted(o[:c.ldo if 'count_padding' in mut else p]).sum())
            r = T(p) / T(m) if m else T(0)
            nobs[ii] = m
            for t in range(ntile * (ntile + 1) // 2):
                ta, tc = gram_tile(t, ntile)
                a0, c0 = ta * BT, tc * BT
                diag, with_dx = ta == tc, ta == 0 or 'dx_every_row' in mut
                va, vc = a0 + np.arange(BT) < k, c0 + np.arange(BT) < k
                ia, ic = np.minimum(a0 + np.arange(BT), k - 1), np.minimum(c0 + np.arange(BT), k - 1)
                acc, accx = np.zeros((BT, BT), dtype=T), np.zeros((2, BT), dtype=T)
                for k0 in range(0, p, BK):
                    e = k0 + np.arange(BK)
                    if 'drop_ktail' in mut and k0 + BK > p:
                        continue
                    if 'read_past' in mut:
                        ec, on = e, seen(o[e])
                    else:
                        ec = np.minimum(e, p - 1)
                        on = (e < p) & seen(o[ec])
                    A, B, xs = De[ec][:, ia], De[ec][:, ic], x[ec]
                    if 'multiply_zeros' in mut:
                        A, B, xs = A * (on[:, None] & va[None]).astype(T), B * (on[:, None] & vc[None]).astype(T), xs * on.astype(T)
                    else:
                        A, B, xs = np.where(on[:, None] & va[None], A, T(0)), np.where(on[:, None] & vc[None], B, T(0)), np.where(on, xs, T(0))
                    acc = acc + A.T.dot(B)
                    if with_dx:
                        Xop = np.zeros((BK, 2), dtype=T)
                        Xop[:, 0] = xs
                        accx = accx + np.stack([(Xop[:, j, None] * B).sum(axis=0) for j in (0, 1)])
                if with_dx:
                    Dx[ii, c0 + np.flatnonzero(vc)] = (r * accx[1 if 'dx_row1' in mut else 0])[vc]
                Ct = r * acc
                ok = va[:, None] & vc[None]
                upper = np.where(diag & ((M_ < N_) if 'diag_from_lower' in mut else (M_ > N_)), Ct.T, Ct)
                G[ii][(a0 + M_)[ok], (c0 + N_)[ok]] = upper[ok]
                if not diag and 'no_mirror' not in mut:
                    G[ii][(c0 + N_)[ok], (a0 + M_)[ok]] = Ct[ok]
    return G, Dx, nobs


def chunked(c, dt, crows, mut=()):
    """the chunk loop of masked_step around the restated gram: chunk r0 reads rows r0 .. r0 + c - 1 and writes there"""
    parts = []
    for r0 in range(0, c.b, crows):
        n = min(crows, c.b - r0)
        parts.append(gram_restated(c, dt, rows=c.samples[0:n] if 'chunk_restart' in mut else c.samples[r0:r0 + n]))
    return tuple(np.concatenate([q[j] for q in parts]) for j in range(3))


def stats_restated(c, dt, mut=(), BT=8, BK=4, NS=8, obs=None, X=None, code_behind=None):
    """Bt, feature_n_iter, counts as masked_stats_kernel + masked_counts_kernel form them, at tiles of BT x BT, K-steps of BK
    and NS observer slices (the odd ones arrive through the cross-lane fold)."""
    T = DT[dt]
    k, p, b = c.k, c.p, c.b
    X = c.X if X is None else X
    obs = c.obs if obs is None else obs
    n = X.shape[0]
    Xb = np.full((n + BK, c.ldx), 3.0, dtype=T)                              # (rows behind the buffer: other numbers, observed)
    Xb[:n, p:] = np.nan
    Xb[:n, :p] = X
    ob = np.ones((n + BK, c.ldo), dtype=np.uint8)
    ob[:n, :p] = obs
    code = np.vstack([c.code, np.full((BK, k), 2.0) if code_behind is None else code_behind]).astype(T)
    rr = np.concatenate([c.samples, n + np.arange(BK)])                      # (what `read_past` finds behind rows / behind row b - 1)
    Bt, fni0 = c.Bt0.astype(T).copy(), c.fni0
    seen = (lambda v: v == 1) if 'byte2_product' in mut else (lambda v: v != 0)
    counted = (lambda v: v == 1) if 'byte2_count' in mut else (lambda v: v != 0)
    lost = {int(m[len('lose_slice'):]) for m in mut if m.startswith('lose_slice')} | ({1, 3, 5, 7} if 'lose_odd' in mut else set())
    with np.errstate(invalid='ignore', divide='ignore'):
        for e0 in range(0, p, BT):
            fe, ve = np.minimum(e0 + np.arange(BT), p - 1), e0 + np.arange(BT) < p
            cnt = np.zeros(BT, dtype=np.int64)
            for sl in range(NS):
                if sl in lost:
                    continue
                src = np.arange(b)[sl::NS] if 'c_first_rows' in mut else rr[:b][sl::NS]
                cnt += counted(ob[src][:, fe]).sum(axis=0)
            for a0 in range(0, k, BT):
                fa, va = np.minimum(a0 + np.arange(BT), k - 1), a0 + np.arange(BT) < k
                acc = np.zeros((BT, BT), dtype=T)
                for k0 in range(0, b, BK):
                    i = k0 + np.arange(BK)
                    if 'drop_ktail' in mut and k0 + BK > b:
                        continue
                    ic, vi = (i, np.ones(BK, bool)) if 'read_past' in mut else (np.minimum(i, b - 1), i < b)
                    row = rr[ic]
                    on = seen(ob[row][:, fe]) & vi[:, None] & ve[None]
                    A = np.where(on, Xb[row][:, fe], T(0))
                    if 'multiply_zeros' in mut:
                        A = Xb[row][:, fe] * on.astype(T)
                    B = np.where(vi[:, None] & va[None], code[ic][:, fa], T(0))
                    acc = acc + A.T.dot(B)
                seen_n = (fni0[fe] + cnt + (cnt if 'fni_first' in mut else 0)).astype(np.float64)
                we = c.w * (cnt / float(b)) * (float(c.n_iter) / seen_n)
                if 'no_clamp' not in mut:
                    we = np.where(we < 1.0, we, 1.0)
                al = we / (float(b) if 'w_over_b' in mut else cnt.astype(np.float64))
                we, al = np.where(cnt > 0, we, 0.0), np.where(cnt > 0, al, 0.0)
                beta, alpha = (1.0 - we).astype(T), al.astype(T)
                ok = (ve & (cnt > 0))[:, None] & va[None]
                old = Bt[np.ix_(fe, fa)]
                new = beta[:, None] * old + alpha[:, None] * acc
                Bt[(e0 + np.arange(BT))[:, None].repeat(BT, 1)[ok], (a0 + np.arange(BT))[None].repeat(BT, 0)[ok]] = new[ok]
    tally = (lambda v: v == 1) if 'byte2_counts_kernel' in mut else (lambda v: v != 0)
    ce = tally(ob[rr[:b]][:, :p]).sum(axis=0)                                # masked_counts_kernel (M:112-121)
    return Bt, fni0 + ce, ce.astype(np.int32)


# ---------------------------------------------------------------------------------------------------- CPU tests
def test_route_table():
    """Every point names what the restated dispatch does there, every leaf of the restatement is hit, both neighbours of
    every numeric boundary are present, and the restatements agree with the kernel's loop and with the Python twin."""
    HIT.clear()
    for (name, dt), r in POINT_BY_KEY.items():
        s = route_of(r, dt)
        for want in r.want:
            assert want in s, (name, dt, want, s)
    hit = set(HIT)
    assert len(all_leaves()) > 30 and set(UNREACHED) <= all_leaves()
    assert all_leaves() - hit == set(UNREACHED), ('no point reaches', sorted(all_leaves() - hit - set(UNREACHED)),
                                                  'reached after all', sorted(hit & set(UNREACHED)))
    # the triangle numbering: the closed form against the kernel's loop, and the tiles of a triangle are its upper half
    for ntile in range(1, 17):
        tiles = [gram_tile(t, ntile) for t in range(ntile * (ntile + 1) // 2)]
        assert tiles == [gram_tile_loop(t, ntile) for t in range(len(tiles))], ntile
        assert tiles == [(a, c) for a in range(ntile) for c in range(a, ntile)], ntile
    # the numeric boundaries, on either side, among the points
    ks = {r.sh['k'] for r in POINTS if r.probe == 'gram'}
    assert {1, 63, 64, 65, 127, 128, 129, 1023, 1024} <= ks
    assert {1, 15, 16, 17, 33, 200} <= {r.sh['p'] for r in POINTS if r.probe == 'gram'}
    assert {MAX_Y, MAX_Y + 1, MAX_Y + 5} <= {r.sh['b'] for r in POINTS if r.probe == 'gram'}
    assert gram_route(2, 5, MAX_Y, True).launches == 1 and gram_route(2, 5, MAX_Y + 1, True).launches == 2
    prods = {cdiv(r.sh['p'], 64) * cdiv(r.sh['k'], 64) for r in POINTS if r.probe == 'stats'}
    assert {496, 511, 512} <= prods
    assert stats_route(64, 32704, 5, True, True).R == 1 and stats_route(64, 32705, 5, True, True).R == 2
    assert stats_route(1024, 1984, 9, False, True).R == 1 and stats_route(1024, 2048, 9, False, False).R == 2
    assert stats_route(1, MAX_Y * 64, 1, False, False).rc == 0 and stats_route(1, MAX_Y * 64 + 1, 1, False, False).rc == EINVAL
    assert stats_route(1, MAX_Y * 64, 1, False, False).grid == (1, MAX_Y)
    assert stats_route(32, 32, 16, False, True).NS == 8 and stats_route(1024, 2048, 9, False, False).NS == 4
    for dt, b_one, b_two in (('f64', 32, 33), ('f32', 64, 65)):
        assert step_route(dt, 1024, b_one, 128, 0.0, True).chunks == 1 and step_route(dt, 1024, b_two, 128, 0.0, True).chunks == 2
    assert step_route('f64', 1024, 35, 35, 0.0, True).ranges == [(0, 32), (32, 3)]
    assert step_route('f32', 1024, 70, 70, 0.0, True).ranges == [(0, 64), (64, 6)]
    assert 'ws2' in step_route('f64', 129, 4, 4, 0.0, True).s and 'ws1' in step_route('f64', 128, 4, 4, 0.0, True).s
    assert 'ws2' in step_route('f64', 512, 4, 4, 0.0, True).s and 'ws1' in step_route('f64', 513, 4, 4, 0.0, True).s
    assert 'ws1' in step_route('f64', 256, 4, 4, 1.0, True).s
    assert step_route('f64', 1024, 35, 35, 0.0, True).ws == 32 * 1024 * 1024 * 8 + 256
    # the Python twin of the chunk rows
    from modl_amd.dict_fact import HipBackend
    for k in (1, 64, 520, 830, 1024):
        for dt in BOTH:
            twin = HipBackend.masked_chunk_rows(SimpleNamespace(k=k, dtype=np.dtype(DT[dt])))
            assert twin == masked_chunk_rows(k, np.dtype(DT[dt]).itemsize), (k, dt, twin)
    assert masked_chunk_rows(1024, 8) == 32 and masked_chunk_rows(1024, 4) == 64 and masked_chunk_rows(1, 4) == 4096
    assert len(POINT_BY_KEY) == sum(len(r.dts) for r in POINTS)


def test_stats_refusal():
    """ceil(p / 64) > 65535 on the 64 x 64 route is MODL_EINVAL before any device work (host pointers, no GPU); its neighbour
    below passes the argument check of a b = 0 call"""
    from modl_amd._lib import lib
    buf = np.zeros(64)
    q = buf.ctypes.data_as(C.c_void_p)
    r = POINT_BY_KEY['s-refused', 'f32']
    p, k = r.sh['p'], r.sh['k']
    assert stats_route(k, p, 1, False, False).rc == EINVAL and stats_route(k, p - 1, 1, False, False).rc == 0
    for sfx in BOTH:
        ms = getattr(lib, 'modl_masked_stats_' + sfx)
        assert ms(q, p, q, p, None, 1, p, k, q, q, q, None, 0.5, 10, None) == EINVAL
        assert ms(q, p * 16, q, p * 16, None, 1, p * 16, 1024, q, q, q, None, 0.5, 10, None) == EINVAL
        assert ms(q, p, q, p, None, 0, p, k, q, q, q, None, 0.5, 10, None) == 0          # b = 0: nothing to do, no refusal


def _scenes_of(r):
    if r.sh.get('only_gaussian') or r.sh.get('launch'):
        return ['gaussian']
    return ['gaussian', 'integers'] + (['scales'] if r.rep else [])


@pytest.mark.parametrize('dt', BOTH)
def test_judges_on_the_oracle(dt):
    """The same-dtype numpy restatement is within the bound on every scene and shape of the table, and dropping the single
    largest term of an element leaves it."""
    T = DT[dt]
    worst = {'gram': 0.0, 'stats': 0.0}
    shapes = set()
    for r in POINTS:
        shape = (r.probe, r.sh['k'], r.sh['p'], r.sh.get('b') if r.probe == 'stats' else None)
        if dt not in r.dts or r.probe == 'step' or r.sh.get('host') or shape in shapes:
            continue                                                         # (a shape once: the layouts do not enter a bound)
        shapes.add(shape)
        for scene in _scenes_of(r):
            if r.probe == 'gram':
                c = launch_source(r, dt)[0] if r.sh.get('launch') else make_gram_case(r, dt, scene)
                ref = gram_ref(c, want_drop=True)
                for i, o in ref.items():
                    if o.m == 0:
                        continue
                    M = np.flatnonzero(c.obs[i])
                    DM, x = c.Dt[M].astype(T), c.X[i, M].astype(T)
                    rT = T(c.p) / T(o.m)
                    G, Dx = rT * DM.T.dot(DM), rT * x.dot(DM)
                    assert G.dtype == T and Dx.dtype == T
                    if scene == 'integers':
                        judge_exact(G, o.G.astype(np.float64)), judge_exact(Dx, o.Dx.astype(np.float64))
                    else:
                        worst['gram'] = max(worst['gram'], judge_bound(G, o.G, o.bG), judge_bound(Dx, o.Dx, o.bDx))
                    for dropped, bound in ((o.dG, o.bG), (o.dDx, o.bDx)):
                        assert np.all(dropped[dropped > 0] > bound[dropped > 0]), (r.name, scene, 'a dropped term hides under the bound')
            else:
                c = make_stats_case(r, dt, scene)
                o = stats_ref(c, want_drop=True)
                S = o.Xz.astype(T).T.dot(c.code.astype(T))
                Bt = o.beta.astype(T)[:, None] * c.Bt0.astype(T) + o.alpha.astype(T)[:, None] * S
                assert Bt.dtype == T
                live = o.c > 0
                if scene == 'integers':
                    judge_exact(Bt[live], (o.Xz.T.dot(c.code) / np.maximum(o.c, 1)[:, None])[live])
                else:
                    worst['stats'] = max(worst['stats'], judge_bound(Bt[live], o.ref[live], o.bound[live]))
                # the product's share of the bound, element by element: (c_e + 6) eps alpha sum <= (c_e + 6) c_e eps alpha max
                share = (o.c + 6)[:, None] * eps_of(dt) * np.abs(o.alpha)[:, None] * np.abs(o.Xz).T.dot(np.abs(c.code))
                assert np.all(o.drop[o.drop > 0] > share[o.drop > 0]), (r.name, scene, 'a dropped term hides under the bound')
                if scene != 'gaussian':                                      # beta = 0: that share is the whole bound
                    assert np.all(o.beta[live] == 0) and np.allclose(share[live], o.bound[live], rtol=1e-12, atol=0)
                elif c.k >= 8:                                               # next to an old value: every feature row is rejected
                    assert np.all((o.drop > o.bound)[live].any(axis=1)), (r.name, scene, 'a row of dropped terms hides under the bound')
    print('%s: numpy same-dtype restatement / bound, largest: gram %.3g, stats %.3g' % (dt, worst['gram'], worst['stats']))
    assert worst['gram'] > 0 and worst['stats'] > 0


def _small_gram(scene, layout, k=19, p=10, dt='f64'):
    r = SimpleNamespace(name='mut-g-%s-%s' % (scene, layout), sh=dict(k=k, p=p, layout=layout, b=99))
    return make_gram_case(r, dt, scene)


def _small_stats(scene, layout, k=11, p=37, b=14, dt='f64', variant=None):
    r = SimpleNamespace(name='mut-s-%s-%s' % (scene, layout), sh=dict(k=k, p=p, b=b, layout=layout, count=True))
    return make_stats_case(r, dt, scene, variant)


def _rejects(f, *a):
    try:
        f(*a)
    except AssertionError:
        return True
    return False


def test_mutants():
    """Every mutant of the restated loops is rejected by the scene and judge the docstring names; where a scene cannot see a
    mutant, that is asserted too."""
    def gram_ok(c, mut=(), **kw):
        G, Dx, nobs = gram_restated(c, c.dt, mut, **kw)
        assert not np.any(G == FILL) or 'no_mirror' in mut, 'an element of G was not written'
        judge_gram(c, G, Dx, nobs)
        return G, Dx, nobs

    ints, gauss = _small_gram('integers', 'loose', p=12), _small_gram('gaussian', 'loose')
    ints_tight = _small_gram('integers', 'tight', p=12)
    for c in (ints, gauss, ints_tight, _small_gram('gaussian', 'tight'), _small_gram('scales', 'loose'), _small_gram('integers', 'tight', k=1, p=1)):
        gram_ok(c)                                                           # the restatement itself passes
    assert _rejects(gram_ok, ints, ('no_mirror',))
    G0 = gram_ok(gauss)
    for c in (ints, gauss):                                                  # INVISIBLE: see the docstring
        gram_ok(c, ('diag_from_lower',))
        assert all(same_bits(a, b) for a, b in zip(gram_ok(c, ('dx_every_row',)), gram_ok(c)))
    tail = _small_gram('integers', 'tight', p=10)                            # p % BK = 2: a K tail
    assert _rejects(gram_ok, tail, ('drop_ktail',)) and _rejects(gram_ok, gauss, ('drop_ktail',))
    tail_loose = _small_gram('integers', 'loose', p=10)
    assert _rejects(gram_ok, tail_loose, ('read_past',))                      # (NaN from the padding of X, other numbers behind Dt)
    zeros_behind = np.zeros((4, tail_loose.k))
    G, Dx, nobs = gram_restated(tail_loose, 'f64', ('read_past',), behind=zeros_behind)
    assert not np.all(np.isfinite(Dx)), 'the NaN padding of X does not reach a loader that reads past the K tail'
    assert _rejects(gram_ok, ints, ('count_padding',))
    gram_ok(ints_tight, ('count_padding',))                                  # INVISIBLE at ldo = p
    assert _rejects(gram_ok, ints, ('dx_row1',)) and _rejects(gram_ok, gauss, ('dx_row1',))
    gram_ok(gauss, ('multiply_zeros',))                                      # INVISIBLE while the places hold finite values
    Xp = gauss.X.copy()
    Xp[gauss.obs == 0] = np.nan
    assert all(same_bits(a, b) for a, b in zip(gram_restated(gauss, 'f64', X=Xp), G0))
    assert not all(same_bits(a, b) for a, b in zip(gram_restated(gauss, 'f64', ('multiply_zeros',), X=Xp), G0))
    by = np.where(gauss.obs != 0, 2, 0).astype(np.uint8)
    assert all(same_bits(a, b) for a, b in zip(gram_restated(gauss, 'f64', obs=by), G0))
    for m in ('byte2_product', 'byte2_count'):
        assert not all(same_bits(a, b) for a, b in zip(gram_restated(gauss, 'f64', (m,), obs=by), G0)), m
    for c in (ints_tight, _small_gram('gaussian', 'tight')):                  # the chunk loop: 8 + 3 rows
        assert c.b > 8
        G, Dx, nobs = chunked(c, 'f64', 8)
        judge_gram(c, G, Dx, nobs)
        G, Dx, nobs = chunked(c, 'f64', 8, ('chunk_restart',))
        assert _rejects(judge_gram, c, G, Dx, nobs)

    def stats_ok(c, mut=(), **kw):
        Bt, fni, cnt = stats_restated(c, c.dt, mut, **kw)
        judge_stats(c, Bt, fni, cnt)
        return Bt, fni, cnt

    si, sg = _small_stats('integers', 'loose'), _small_stats('gaussian', 'loose')
    sg_tight = _small_stats('gaussian', 'tight')
    for c in (si, sg, sg_tight, _small_stats('integers', 'tight'), _small_stats('scales', 'loose'), _small_stats('gaussian', 'tight', 1, 1, 1),
              _small_stats('integers', 'tight', b=16, variant='raw1')):
        stats_ok(c)
    assert _rejects(stats_ok, si, ('drop_ktail',)) and _rejects(stats_ok, sg, ('drop_ktail',))       # b % BK = 2
    assert _rejects(stats_ok, _small_stats('integers', 'tight'), ('read_past',)) and _rejects(stats_ok, sg_tight, ('read_past',))
    for sl in range(8):
        assert _rejects(stats_ok, sg, ('lose_slice%d' % sl,)) and _rejects(stats_ok, si, ('lose_slice%d' % sl,)), sl
    assert _rejects(stats_ok, sg, ('lose_odd',)) and _rejects(stats_ok, si, ('lose_odd',))
    assert _rejects(stats_ok, sg, ('c_first_rows',))
    stats_ok(sg_tight, ('c_first_rows',))                                    # INVISIBLE with rows NULL
    assert _rejects(stats_ok, sg, ('fni_first',))
    stats_ok(si, ('fni_first',))                                             # INVISIBLE where the clamp binds
    assert _rejects(stats_ok, si, ('no_clamp',))
    low = _small_stats('gaussian', 'tight')
    low.fni0 = low.fni0 + 100000                                             # every raw weight far below 1
    stats_ok(low)
    stats_ok(low, ('no_clamp',))                                             # INVISIBLE there
    assert _rejects(stats_ok, si, ('w_over_b',)) and _rejects(stats_ok, sg, ('w_over_b',))
    stats_ok(_small_stats('integers', 'tight', b=16, variant='raw1'), ('w_over_b',))      # INVISIBLE: everybody observes
    stats_ok(sg, ('multiply_zeros',))
    Xp = sg.X.copy()
    Xp[sg.obs == 0] = np.inf
    B0 = stats_restated(sg, 'f64')
    assert all(same_bits(a, b) for a, b in zip(stats_restated(sg, 'f64', X=Xp), B0))
    assert not all(same_bits(a, b) for a, b in zip(stats_restated(sg, 'f64', ('multiply_zeros',), X=Xp), B0))
    by = np.where(sg.obs != 0, 2, 0).astype(np.uint8)
    assert all(same_bits(a, b) for a, b in zip(stats_restated(sg, 'f64', obs=by), B0))
    for m in ('byte2_product', 'byte2_count', 'byte2_counts_kernel'):
        assert not all(same_bits(a, b) for a, b in zip(stats_restated(sg, 'f64', (m,), obs=by), B0)), m


# ---------------------------------------------------------------------------------------------------- layer 2: the ABI on the device
@pytest.fixture(scope='module')
def gpu():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    return torch.device('cuda', 0)


def _td(dt):
    import torch
    return torch.float32 if dt == 'f32' else torch.float64


def _dev(a, dt, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=DT[dt])).to(dev)


def _bytes(t):
    return t.cpu().numpy().tobytes()


def _buffers(c, dev, X=None, obs=None):
    """X and obs as the case lays them out: NaN in the ldx - p columns, 1 in the ldo - p columns, NaN / 1 in the rows that
    are not samples of the call"""
    import torch
    X = c.X if X is None else X
    obs = c.obs if obs is None else obs
    Xh = np.full((c.n, c.ldx), np.nan, dtype=DT[c.dt])
    oh = np.ones((c.n, c.ldo), dtype=np.uint8)
    Xh[:, :c.p], oh[:, :c.p] = X, obs
    outside = np.setdiff1d(np.arange(c.n), c.samples)
    Xh[outside], oh[outside] = np.nan, 1
    rows = None if c.rows is None else torch.from_numpy(c.rows).to(dev)
    return torch.from_numpy(Xh).to(dev), torch.from_numpy(oh).to(dev), rows


def run_gram(c, dev, X=None, obs=None):
    """modl_masked_gram_* twice on the case: (G, Dx, nobs) of the b samples; the canaries and the inputs keep their bits,
    the second call gives the bits of the first"""
    import torch
    from modl_amd._lib import lib
    from modl_amd.device import ptr
    f = getattr(lib, 'modl_masked_gram_' + c.dt)
    Xb, ob, rows = _buffers(c, dev, X, obs)
    Dt = torch.full((c.p + 1, c.k), float('nan'), dtype=_td(c.dt), device=dev)               # (a NaN row behind Dt)
    Dt[:c.p] = _dev(c.Dt, c.dt, dev)
    before = [_bytes(t) for t in (Xb, ob, Dt)]
    b, k, outs = c.b, c.k, []
    for _ in range(2):
        G = torch.full((b + 1, k, k), FILL, dtype=_td(c.dt), device=dev)
        Dx = torch.full((b + 1, k), FILL, dtype=_td(c.dt), device=dev)
        nobs = torch.full((b + 1,), -7, dtype=torch.int32, device=dev)
        assert f(ptr(Dt), c.p, k, ptr(Xb), c.ldx, ptr(ob), c.ldo, ptr(rows), b, ptr(G), ptr(Dx), ptr(nobs), None) == 0
        torch.cuda.synchronize()
        outs.append([t.cpu().numpy() for t in (G, Dx, nobs)])
    G, Dx, nobs = outs[0]
    assert np.all(G[b] == FILL) and np.all(Dx[b] == FILL) and nobs[b] == -7, 'the slot behind the last sample was written'
    assert before == [_bytes(t) for t in (Xb, ob, Dt)], 'an input was written'
    assert all(same_bits(x, y) for x, y in zip(outs[0], outs[1])), 'a second identical call gave other bits'
    return G[:b], Dx[:b], nobs[:b]


def run_stats(c, dev, X=None, obs=None):
    import torch
    from modl_amd._lib import lib
    from modl_amd.device import ptr
    f = getattr(lib, 'modl_masked_stats_' + c.dt)
    Xb, ob, rows = _buffers(c, dev, X, obs)
    code = _dev(c.code, c.dt, dev)
    before = [_bytes(t) for t in (Xb, ob, code)]
    p, k, outs = c.p, c.k, []
    for _ in range(2):
        Bt = torch.full((p + 1, k), FILL, dtype=_td(c.dt), device=dev)
        Bt[:p] = _dev(c.Bt0, c.dt, dev)
        fni = torch.full((p + 3,), 77, dtype=torch.int64, device=dev)
        fni[:p] = torch.from_numpy(c.fni0).to(dev)
        cnt = torch.full((p + 3,), -7, dtype=torch.int32, device=dev) if c.count else None
        assert f(ptr(Xb), c.ldx, ptr(ob), c.ldo, ptr(rows), c.b, p, k, ptr(code), ptr(Bt), ptr(fni), ptr(cnt), c.w, c.n_iter, None) == 0
        torch.cuda.synchronize()
        outs.append([None if t is None else t.cpu().numpy() for t in (Bt, fni, cnt)])
    Bt, fni, cnt = outs[0]
    assert np.all(Bt[p] == FILL), 'the row behind Bt was written'
    assert np.all(fni[p:] == 77) and (cnt is None or np.all(cnt[p:] == -7)), 'entries behind feature_n_iter / d_count were written'
    assert before == [_bytes(t) for t in (Xb, ob, code)], 'an input was written'
    assert all(x is None or same_bits(x, y) for x, y in zip(outs[0], outs[1])), 'a second identical call gave other bits'
    return Bt[:p], fni[:p], None if cnt is None else cnt[:p]


def _bytes_scene(c, rs):
    obs = c.obs.copy()
    obs[obs != 0] = rs.choice(np.array([1, 2, 0x80, 0xFF], dtype=np.uint8), size=int((obs != 0).sum()))
    assert {1, 2, 0x80, 0xFF} <= set(np.unique(obs)) or obs.size < 16
    return obs


def _poison(c):
    X = c.X.copy()
    hole = np.argwhere(c.obs == 0)
    X[tuple(hole[0::2].T)] = np.nan
    X[tuple(hole[1::2].T)] = np.inf
    return X


def _who(r, dt):
    s = route_of(r, dt)
    if r.probe == 'gram':
        return 'gram ntile %s %s' % (s.split('ntile')[1].split('/')[0], dt)
    return 'stats %s %s' % ('R2' if '/R2' in s else 'R1', dt)


def _run_gram_point(r, dt, dev):
    who = _who(r, dt)
    for scene in _scenes_of(r):
        c = make_gram_case(r, dt, scene)
        got = run_gram(c, dev)
        judge_gram(c, *got, who=who)
        if scene != 'gaussian':
            continue
        rs = np.random.RandomState(_seed(r.name, dt, 'bytes'))
        assert all(same_bits(x, y) for x, y in zip(run_gram(c, dev, obs=_bytes_scene(c, rs)), got)), 'bytes other than 1 changed the result'
        assert all(same_bits(x, y) for x, y in zip(run_gram(c, dev, X=_poison(c)), got)), 'the poison changed the result'
        ms = [int((c.obs[i] != 0).sum()) for i in c.samples]
        j = int(np.argmax([m if m < c.p or c.p == 1 else 0 for m in ms]))    # a holed row (p = 1: the observed one)
        if ms[j] > 0:
            i = c.samples[j]
            Xn = c.X.copy()
            Xn[i, np.flatnonzero(c.obs[i])[0]] = np.nan
            G, Dx, nobs = run_gram(c, dev, X=Xn)
            hit = c.samples == i
            assert not np.isfinite(Dx[hit]).any(), 'a NaN at an observed entry left Dx finite'
            assert same_bits(G, got[0]) and same_bits(Dx[~hit], got[1][~hit]) and same_bits(nobs, got[2]), 'a NaN of one row reached another result'
    _report()


def _run_launch_point(r, dt, dev):
    """b beyond one launch: every sample is the bits of its source row's result from a call of eight samples"""
    small, c = launch_source(r, dt)
    want = run_gram(small, dev)
    judge_gram(small, *want, who='gram ntile 1 ' + dt)
    G, Dx, nobs = run_gram(c, dev)
    assert len(c.src_of) == c.b and (c.b <= MAX_Y or c.src_of[MAX_Y] == MAX_Y % 8)
    assert same_bits(G, want[0][c.src_of]) and same_bits(Dx, want[1][c.src_of]) and same_bits(nobs, want[2][c.src_of]), \
        ('a sample of a long batch is not its source row\'s result', np.flatnonzero((Dx != want[1][c.src_of]).any(axis=1))[:4])


def _run_stats_point(r, dt, dev):
    who = _who(r, dt)
    for scene in _scenes_of(r):
        c = make_stats_case(r, dt, scene)
        got = run_stats(c, dev)
        judge_stats(c, *got, who=who)
        if scene == 'integers' and r.name == 's-32':
            c1 = make_stats_case(r, dt, scene, 'raw1')
            beta, al, we = stats_weights(np.full(c1.p, c1.b), c1.fni0, c1.w, c1.n_iter, c1.b)
            assert np.all(c1.w * 1.0 * (c1.n_iter / (c1.fni0 + c1.b)) == 1.0) and np.all(we == 1.0)
            judge_stats(c1, *run_stats(c1, dev))
        if scene != 'gaussian' or r.sh.get('only_gaussian'):
            continue
        same = lambda a, b: all(x is None or same_bits(x, y) for x, y in zip(a, b))          # noqa: E731
        rs = np.random.RandomState(_seed(r.name, dt, 'bytes'))
        assert same(run_stats(c, dev, obs=_bytes_scene(c, rs)), got), 'bytes other than 1 changed the result'
        assert same(run_stats(c, dev, X=_poison(c)), got), 'the poison changed the result'
        on = c.obs[c.samples] != 0
        at = np.argwhere(on)
        i, e = at[len(at) // 2]
        Xn = c.X.copy()
        Xn[c.samples[i], e] = np.nan
        Bt, fni, cnt = run_stats(c, dev, X=Xn)
        others = np.arange(c.p) != e
        assert not np.isfinite(Bt[e]).any(), 'a NaN at an observed entry left its row of Bt finite'
        assert same_bits(Bt[others], got[0][others]) and same_bits(fni, got[1]), 'a NaN of one feature reached another row of Bt'
    _report()


GPU_POINTS = [(r.name, dt) for r in POINTS for dt in r.dts if r.probe in ('gram', 'stats') and not r.sh.get('host')]


@pytest.mark.gpu
@pytest.mark.parametrize('name,dt', GPU_POINTS, ids=['%s-%s' % c for c in GPU_POINTS])
def test_route(gpu, name, dt):
    r = POINT_BY_KEY[name, dt]
    if r.sh.get('launch'):
        _run_launch_point(r, dt, gpu)
    elif r.probe == 'gram':
        _run_gram_point(r, dt, gpu)
    else:
        _run_stats_point(r, dt, gpu)


# ---------------------------------------------------------------------------------------------------- layer 3: the chunk loops
class Plan:
    """a masked modl_somf plan of this test's own"""
    def __init__(self, dt, k, p, n, mb, l1_ratio, alpha, tol, max_iter):
        from modl_amd._lib import lib, check, SomfDesc, AGG, OPT
        d = SomfDesc()
        d.dtype, d.k, d.p, d.n_samples = (0 if dt == 'f32' else 1), k, p, n
        d.G_agg = d.Dx_agg = AGG['masked']
        d.optimizer, d.code_pos, d.comp_pos, d.max_iter = OPT['variational'], 0, 0, max_iter
        d.code_alpha, d.code_l1_ratio, d.comp_l1_ratio, d.tol, d.step_size = alpha, l1_ratio, 0.0, tol, 1e-3
        d.max_batch, d.flags = mb, 0
        self.h = C.c_void_p()
        check(lib.modl_somf_plan_create(C.byref(d), C.byref(self.h)), 'modl_somf_plan_create')

    def __enter__(self):
        return self.h

    def __exit__(self, *exc):
        from modl_amd._lib import lib
        lib.modl_somf_plan_destroy(self.h)
        self.h = None


def step_masks(b, p, r0, rs):
    """the second chunk (rows r0 ..) holds an empty row, a fully observed row and holed rows; the first the same"""
    on = rs.rand(b, p) < 0.6
    on[1], on[2] = False, True
    on[r0] = False
    if r0 + 1 < b:
        on[r0 + 1] = True
    if r0 + 2 < b:
        on[r0 + 2, :p // 2] = False
    return on


def make_step_case(r, dt):
    sh = r.sh
    k, p, b = sh['k'], sh['p'], sh['b']
    rs = np.random.RandomState(_seed(r.name, dt))
    q = lambda a: a.astype(DT[dt]).astype(np.float64)                       # noqa: E731
    c = SimpleNamespace(dt=dt, k=k, p=p, b=b, mb=sh['mb'], l1=sh['l1'], has_idx=sh['idx'], scene='gaussian')
    c.route = step_route(dt, k, b, c.mb, c.l1, c.has_idx)
    c.n = b + 3
    c.idx = rs.permutation(c.n)[:b].astype(np.int64) if c.has_idx else None
    c.code_rows = c.idx if c.has_idx else np.arange(b)
    c.ldx, c.ldo = p + 3, p + 1
    c.X = np.round(rs.randn(b, p) * 4) / 4                                   # multiples of 1 / 4: squared row norms exact in any order
    r0 = c.route.ranges[-1][0]
    c.obs = step_masks(b, p, r0, rs).astype(np.uint8)
    c.Dt = q(rs.randn(p, k) / np.sqrt(p))
    R = rs.randn(k, 16)
    c.C0 = q(R.dot(R.T) / 16 + np.diag(rs.uniform(0.5, 1.5, k)))
    c.C0 = np.maximum(c.C0, c.C0.T)
    c.Bt0, c.code0 = q(rs.randn(p, k)), q(rs.randn(c.n, k))
    c.fni0 = rs.randint(1, 4000, size=p).astype(np.int64)
    c.w, c.n_iter = 0.37, 1000
    c.alpha, c.tol, c.max_iter = (0.5, 1e-3, 100) if c.l1 == 0 else (0.05, 1e-3, 60)
    c.order = rs.permutation(k).astype(np.int64)
    c.samples, c.rows, c.count = np.arange(b), None, False
    return c


def run_step(c, dev, obs=None):
    """one modl_somf_masked_step from the case's state: code_, C_, Bt, feature_n_iter and the sweep counts afterwards"""
    obs = c.obs if obs is None else obs
    import torch
    from modl_amd._lib import lib, check, SomfState, SomfBatch
    from modl_amd.device import ptr, stream_ptr
    td = _td(c.dt)
    Xb = torch.full((c.b + 1, c.ldx), float('nan'), dtype=td, device=dev)
    Xb[:c.b, :c.p] = _dev(c.X, c.dt, dev)
    Xb[:c.b, :c.p][torch.from_numpy(obs == 0).to(dev)] = float('nan')        # nothing of X at an unobserved position is used
    ob = torch.ones((c.b + 1, c.ldo), dtype=torch.uint8, device=dev)
    ob[:c.b, :c.p] = torch.from_numpy(obs).to(dev)
    st = SimpleNamespace(Dt=_dev(c.Dt, c.dt, dev), Bt=_dev(c.Bt0, c.dt, dev), C=_dev(c.C0, c.dt, dev), code=_dev(c.code0, c.dt, dev),
                         comp_norm=torch.zeros(c.k, dtype=td, device=dev), fni=torch.from_numpy(c.fni0).to(dev))
    s = SomfState()
    s.d_Dt, s.d_Bt, s.d_C, s.d_code, s.d_comp_norm = ptr(st.Dt), ptr(st.Bt), ptr(st.C), ptr(st.code), ptr(st.comp_norm)
    out = SimpleNamespace(Xb=Xb, ob=ob)
    with Plan(c.dt, c.k, c.p, c.n, c.mb, c.l1, c.alpha, c.tol, c.max_iter) as plan:
        bt = SomfBatch()
        bt.d_X, bt.ldx, bt.b, bt.s = ptr(Xb), c.ldx, c.b, c.p
        bt.h_sample_idx = None if c.idx is None else c.idx.ctypes.data
        bt.h_subset, bt.h_w_sample, bt.h_order = None, None, c.order.ctypes.data
        bt.w, bt.reduction, bt.b_global = c.w, 1.0, c.b
        check(lib.modl_somf_masked_step(plan, C.byref(s), C.byref(bt), ptr(ob), c.ldo, ptr(st.fni), c.n_iter, stream_ptr(dev)),
              'modl_somf_masked_step')
        check(lib.modl_somf_status(plan, stream_ptr(dev)), 'modl_somf_status')
        torch.cuda.synchronize()
        sw, n = (C.c_int32 * (c.b + 4))(), C.c_int(0)
        check(lib.modl_somf_last_sweeps(plan, sw, c.b + 4, C.byref(n), stream_ptr(dev)), 'modl_somf_last_sweeps')
        out.n_sweeps, out.sweeps = n.value, np.array(sw[:n.value])
    out.code, out.C, out.Bt, out.fni = (t.cpu().numpy() for t in (st.code, st.C, st.Bt, st.fni))
    return out


def direct_codes(c, dev, Xb, ob):
    """the codes of the batch by modl_masked_gram_* + modl_enet_regression_multi_gram_* on the step's own row ranges, with the
    step's arguments; (code_ afterwards, sweeps, nobs)"""
    import torch
    from modl_amd._lib import lib, check
    from modl_amd.device import ptr, stream_ptr
    td = _td(c.dt)
    gram = getattr(lib, 'modl_masked_gram_' + c.dt)
    solve = getattr(lib, 'modl_enet_regression_multi_gram_' + c.dt)
    Dt = _dev(c.Dt, c.dt, dev)
    code = _dev(c.code0, c.dt, dev)
    Xz = torch.where(ob[:, :c.p] != 0, Xb[:, :c.p], torch.zeros((), dtype=td, device=dev)).contiguous()
    idx = None if c.idx is None else torch.from_numpy(c.idx).to(dev)
    sweeps = torch.full((c.b,), -1, dtype=torch.int32, device=dev)
    nobs = torch.full((c.b,), -1, dtype=torch.int32, device=dev)
    for r0, n in c.route.ranges:
        G = torch.empty((n, c.k, c.k), dtype=td, device=dev)
        Dx = torch.empty((n, c.k), dtype=td, device=dev)
        check(gram(ptr(Dt), c.p, c.k, ptr(Xb[r0:]), c.ldx, ptr(ob[r0:]), c.ldo, None, n, ptr(G), ptr(Dx), ptr(nobs[r0:]), stream_ptr(dev)),
              'modl_masked_gram')
        nbytes = lib.modl_enet_regression_workspace(0 if c.dt == 'f32' else 1, n, c.k, 1)
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        check(solve(ptr(G), ptr(Dx), ptr(Xz[r0:]), c.p, c.p, ptr(code if idx is not None else code[r0:]),
                    None if idx is None else ptr(idx[r0:]), n, c.k, c.l1, c.alpha, 0, c.tol, c.max_iter, ptr(sweeps[r0:]), ptr(ws), nbytes,
                    stream_ptr(dev)), 'modl_enet_regression_multi_gram')
        torch.cuda.synchronize()
    return code.cpu().numpy(), sweeps.cpu().numpy(), nobs.cpu().numpy()


STEP_POINTS = [(r.name, dt) for r in POINTS for dt in r.dts if r.probe == 'step']


@pytest.mark.gpu
@pytest.mark.parametrize('name,dt', STEP_POINTS, ids=['%s-%s' % c for c in STEP_POINTS])
def test_step_chunks(gpu, name, dt):
    """modl_somf_masked_step across the chunk boundary: see LAYER 3 in the module docstring"""
    r = POINT_BY_KEY[name, dt]
    c = make_step_case(r, dt)
    T = DT[dt]
    got = run_step(c, gpu)
    want_code, want_sweeps, nobs = direct_codes(c, gpu, got.Xb, got.ob)
    m = (c.obs != 0).sum(axis=1)
    np.testing.assert_array_equal(nobs, m)
    r0 = c.route.ranges[-1][0]
    assert m[r0] == 0 and (c.b < r0 + 2 or m[r0 + 1] == c.p) and (c.b < r0 + 3 or 0 < m[r0 + 2] < c.p)
    rows, live = c.code_rows, m > 0
    assert np.all(np.isfinite(got.code[rows]))
    assert not got.code[rows[~live]].any(), 'an empty row kept its warm start'
    assert c.code0[rows[~live]].all()
    bad = np.flatnonzero((got.code[rows[live]] != want_code[rows[live]]).any(axis=1))
    assert same_bits(got.code[rows[live]], want_code[rows[live]]), ('rows whose codes are not those of the direct calls', np.flatnonzero(live)[bad])
    assert np.count_nonzero(got.code[rows[live]]) > 0
    outside = np.setdiff1d(np.arange(c.n), rows)
    assert same_bits(got.code[outside], c.code0.astype(T)[outside]), 'rows of code_ outside the batch were written'
    assert got.n_sweeps == c.b
    if c.l1 != 0:
        np.testing.assert_array_equal(got.sweeps[live], want_sweeps[live])
        assert np.all(got.sweeps[live] >= 1)
    # the statistics from the device's own codes
    code = got.code[rows].astype(np.float64)
    c.code = code
    who = 'step %s' % dt
    judge_stats(c, got.Bt, got.fni, None, who=who + ' B', code=code)
    ref = LD(1 - c.w) * c.C0 + LD(c.w / c.b) * np.asarray(code, dtype=LD).T.dot(np.asarray(code, dtype=LD))
    bound = (c.b + 6) * eps_of(dt) * ((1 - c.w) * np.abs(c.C0) + (c.w / c.b) * np.abs(code).T.dot(np.abs(code)))
    judge_bound(got.C, ref, bound, who + ' C', 'C_')
    again = run_step(c, gpu)
    assert all(same_bits(getattr(got, f), getattr(again, f)) for f in ('code', 'C', 'Bt', 'fni')), 'a second identical step gave other bits'
    if c.l1 != 0:
        # bytes: the step's four readers of the mask (the Gram, the statistics, the counts and - under code_l1_ratio != 0 only -
        # the squared row norms) agree on 2, 0x80 and 0xFF
        other = run_step(c, gpu, obs=_bytes_scene(c, np.random.RandomState(_seed(name, 'bytes'))))
        assert all(same_bits(getattr(got, f), getattr(other, f)) for f in ('code', 'C', 'Bt', 'fni', 'sweeps')), 'bytes other than 1 changed the step'
    _report()


@pytest.mark.gpu
@pytest.mark.parametrize('algorithm', ['enet', 'omp'])
def test_python_chunk_loops(gpu, algorithm):
    """HipBackend.transform_masked / the masked branch of HipBackend.omp across masked_chunk_rows(): every holed row equals,
    bit for bit, the row obtained when the rows of its chunk are submitted alone"""
    from modl_amd import Coder
    k, p = 1024, 64
    rs = np.random.RandomState(_seed('twins', algorithm))
    D = rs.randn(k, p)
    D /= np.sqrt((D ** 2).sum(axis=1))[:, None]
    coder = Coder(D, code_alpha=0.05)
    kw = dict(algorithm='omp', n_nonzero_coefs=4) if algorithm == 'omp' else {}
    step = masked_chunk_rows(k, 8)
    n_holed = step + 3
    kinds = []                                                               # holed rows between clean and empty ones
    while kinds.count('holed') < n_holed:
        kinds += ['holed', 'clean', 'empty'] if len(kinds) % 2 else ['holed']
    n = len(kinds)
    X = rs.randn(n, 8).dot(rs.randn(8, p)) + 0.3 * rs.randn(n, p)
    mask = rs.rand(n, p) < 0.6
    for i, kind in enumerate(kinds):
        if kind != 'holed':
            mask[i] = kind == 'clean'
        else:
            mask[i, i % p], mask[i, (i + 1) % p] = True, False
    X[~mask] = np.nan
    code = coder.transform(X, mask=mask, **kw)
    assert coder._backend.masked_chunk_rows() == step and code.dtype == np.float64
    holed = np.flatnonzero([x == 'holed' for x in kinds])
    assert len(holed) == step + 3 and np.all(np.isfinite(code))
    assert not code[[x == 'empty' for x in kinds]].any()
    for part in (holed[:step], holed[step:]):
        alone = coder.transform(X[part], mask=mask[part], **kw)
        bad = np.flatnonzero((alone != code[part]).any(axis=1))
        assert same_bits(alone, code[part]), ('rows that differ when their chunk is submitted alone', part[bad])
        assert np.count_nonzero(alone) > 0
    assert same_bits(coder.transform(X, mask=mask, **kw), code)

