"""The elastic-net code solve (l1_ratio > 0) route by route, through modl_amd.dict_fact_fast._enet_regression_{single,multi}_gram
(and modl_enet_regression_* directly where the shim cannot express a layout), against the CPU oracle's
enet_regression_*_gram on inputs built to leave the main branch of enet_coordinate_descent_gram.

ROUTES (`ROUTES`, checked against `expected_route`, a restatement of the dispatch; the same table is in DESIGN.md, section 19).
Lines: A = csrc/code_solve.hip (code_route, code_solve), S = csrc/cd_solver.hip, P = csrc/cd_split.hip, as of this commit.

  shared Gram, product library, default switches
    k = 5, 31, 32, 33   one wavefront (cd_kernel, 1 coefficient per lane), 64-stride padded copy, padded-vector loader:
                        A:19, A:81-85 copies (cd_padded_ld = 64, S:568); P:20 refuses a stride of 64, so S:545 falls
                        through to S:547; S:496-498 picks VEC and PAD.  (The four-wavefront solver starts at k = 65 for a shared
                        matrix: 32 <= k <= 64 is padded to 64, not to 128.  A per-sample matrix of that size is padded to 128,
                        S:600.)
    k = 70, 128         four wavefronts at stride 128 (P:33): 128 in place (A:19 false), 70 through the padded copy
    k = 129, 256        four wavefronts at stride 256 (P:34); 129 through the copy, 256 in place
    k = 257, 512        stride 512 (P:35)
    k = 513, 1024       stride 1024 (P:36)
    k = 1025            the wide solver (A:16, csrc/cd_wide.hip)
  misaligned shared matrix (a view one element into a buffer), k = 128, 256: A:19 makes no copy (k <= 256), P:23 refuses,
                        S:547-549 + S:496 (not VEC): cd_kernel with the element-wise loader, 2 / 4 coefficients per lane
  per-sample Gram
    k = 128             in place on the four-wavefront solver (A:20: cd_split_applies holds, A:87 -> S:545)
    k = 70              through zero-padded slots of stride 128 (A:20-21, A:75-79, S:617-640)
    k = 513, f64, b = 9 slots of 1024 x 1024 x 8 B = 8 MiB: eight per 64 MiB slice (S:589, S:601-607), so two slices (S:623)
    k = 20, b = 5       cd_kernel, element-wise loader (A:20 needs k >= 32; S:547); the second workgroup holds one sample
    k = 1025            the wide solver with a matrix per sample (A:16)
  MODL_DEBUG_CD_SPLIT = 0 (S:543-545), shared, k = 70, 128, 200, 256: cd_kernel with 2 / 4 coefficients per lane; 70 and 200 through
                        the padded copy with the padded-vector loader (S:498), 128 and 256 in place with the vector loader
  MODL_DEBUG_CD_SPARSE_PCT = 0 / 100 (S:533-534) on those four: dense / active-set sweeps only
Routing cannot be observed from outside; `test_workspace_table` pins what can be: the padded-copy and slot terms of
modl_enet_regression_workspace for every (k, b) of the table.

SCENES (`make_case`; seeded RandomState; D (k x p) Gaussian, rows normalised; X = (randn * (rand < 0.1)) D + 0.1 randn;
G = D D^T symmetrised and Dx = X D^T in the dtype; idx a permutation into a code array with three extra rows, which hold 7.5;
p = k + 80; b = 20 up to k = 513, 6 beyond; defaults l1_ratio 0.9, alpha 0.3, tol 1e-2, max_iter 100, start ones).
Special positions: 0, k-1, k//3, k//3 + 1 and, for k > 64, 63 and 64.
  generic           the control
  dead_ones         the atoms at the special positions zeroed (zero rows / columns of G, zero Dx); max_iter 20.  Every sample
                    runs all 20 sweeps (the dead ones stay in the gap's l1 term) and the dead coefficients come back 1
  dead_zero_start   same matrix, start 0 at the dead positions: stops on the gap, dead coefficients come back 0
  dead_q            as dead_zero_start with Dx = 3 alpha at the dead positions: they enter the dual norm
  duplicate         atom 5 = atom 4, atom k-1 = atom 0 (k < 7: atom 2 = atom 1), signal planted on the first of each pair;
                    l1_ratio 1.0 (singular) and 0.7
  all_zero          alpha = 1.5 max|Dx|, l1_ratio 1: one sweep, zero codes, the `dual <= alpha` branch, the w_max == 0 exit
  positive_none     positive, D = |randn| normalised, X = -|randn|: Dx < 0, one sweep, zero codes
  zero_row          row 1 of X and Dx zero (tol ||x||^2 = 0), from ones and from zeros; max_iter 30: that row runs 30 sweeps
                    and ends at zero, its neighbours in the workgroup follow the oracle
  limits            (max_iter, tol) = (0, 1e-2), (1, 1e-2), (2, 1e-2), (25, 0), (100, 1e9): 0, 1, 2, 25, 1 sweeps; max_iter 0
                    returns the input bits
  warm_at_solution  start from the oracle's code at tol 1e-6: one sweep
  tight             tol 1e-4 / 1e-6, max_iter 1000, l1_ratio 1.0 / 0.5, positive or not
  x_layout          shared, k = 70, direct ABI call: ldx = p + 3 with NaN padding and ldx = p + 1, p in {1, 3, 1027, 4101} (rows
                    alternately 16-byte misaligned in one of the two for every p); row 2's only non-zero is element p - 1
Every route runs generic, dead_ones, dead_zero_start, duplicate and zero_row; the others run on shared 31, 70, 256, 513, 1025
and per-sample 70.  f64 everywhere, f32 on every route but the two-slice one (in f32 its nine slots fit one slice).

JUDGES
  A (f64, the numbers of test_gpu_kernels.py): sweep counts identical, rel_fro < 1e-10, identical support, rows outside idx
    bit-identical, dead coefficients equal to the input (zeros by value: the reference itself produces -0.0).
    EXACT TIES.  Where atoms are copies of one another and there is no ridge to split the weight (`duplicate` at l1_ratio 1,
    and x_layout at p = 1, where all 70 atoms are one atom up to sign), the copy's soft-threshold argument equals the threshold
    in exact arithmetic once the original has moved, so whether the copy comes back 0 or +-1e-16 depends on the rounding
    order of H - between two CPU implementations already: at k = 257 the oracle returns 0.0 for coefficient 5 of sample 9
    where `restated_cd` (numpy's dot for H = G w) returns 1.7e-16, and the same step in the four-wavefront solver's order
    flips 36 coefficients of x_layout at p = 1 (`test_exact_ties_are_a_matter_of_rounding_order`).  On those coordinates alone
    (`case.ties`) a zero and a non-zero agree when both are within k eps max(1, |q|_max, |w|_max) of zero; every other
    coordinate and every other scene compares supports literally.
  B (f32): where the scene forces the count (dead_ones, all_zero, positive_none, limits, the zero row) counts identical;
    elsewhere equal on >= 90 % of the samples and rel_fro < 2e-5 on those (p < k: 1e-4 through the fit w D).
    Rows outside idx and dead coefficients as in A.
    One exception, rooted in the reference's own f32 behaviour and shown with the oracle (F32_NOISE_SCENES = tight): where a
    tight case misses the 90 % and the oracle's own f32 run leaves its f64 run on more than 10 % of the same samples (asserted;
    k = 1025, b = 6, tol 1e-6: one sample of six), the codes are held to conftest.assert_within_f32_noise on every sample.
  C (both dtypes; tight, and generic at tol 1e-2), independent of the oracle: P(w) = |x|^2 / 2 - w.q + w G w / 2 + a |w|_1 +
    beta |w|^2 / 2 in f64 on the inputs as given, w* from `solve_star` (plain numpy coordinate descent to a KKT residual
    < 1e-13).  For every sample that stopped before max_iter: P(w) - P(w*) <= tol |x|^2 (the accepted duality gap bounds
    the suboptimality) and, with mu = lambda_min(G) + beta > 0, |w - w*|^2 <= 2 tol |x|^2 / mu (strong convexity).
    `test_judge_c_on_the_oracle` asserts that the oracle alone stays below ORACLE_SHARE_OF_C of either bound on every case C is
    applied to.

MUTANTS (`test_mutants`, on `restated_cd`, the sweep in plain f64 numpy, which `test_restatement` holds to the oracle: same
sweeps, 1e-12).  Mutant -> the scene that rejects it under A (or C):
  dead coefficient zeroed on output                  dead_ones
  dead coefficient counted in w_max                  INVISIBLE in every scene here: a dead coefficient that is not zero keeps
                                                     the gap above tol |x|^2 by its own a |w| term, so an earlier gap TEST
                                                     never becomes an earlier EXIT (asserted: no scene rejects it)
  dead coefficient left out of |w|_1 and |w|^2       dead_ones (the gap passes: fewer than max_iter sweeps)
  dead coordinate left out of the dual norm          dead_q
  |.| in the dual norm when positive                 positive_none
  gap not evaluated at n_iter == max_iter - 1        INVISIBLE by construction: n_iter ends at max_iter and the code is the same
                                                     whether that last test is made, passes or fails (asserted on limits)
  tol not scaled by |x|^2                            zero_row
  |x|^2 taken over ldx                               x_layout
  sweep count off by one on the gap exit             generic
  w_max == 0 exit missing                            all_zero
  soft threshold with alpha, not alpha l1_ratio      generic
  beta missing from the step denominator             generic
  duplicates visited in reverse order                duplicate
"""
import ctypes as C
import functools
import zlib
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import somf_oracle as _orc

from .conftest import assert_within_f32_noise, rel_fro

DT = {'f32': np.float32, 'f64': np.float64}
FILL = 7.5                       # rows of the code array outside idx
SWITCH_DEFAULTS = {'CD_SPLIT': 1, 'CD_SPARSE_PCT': -1}
ORACLE_SHARE_OF_C = 0.015        # the issue's figure: the reference alone uses at most 1.5 % of either bound of judge C
FORCED = ('dead_ones', 'all_zero', 'positive_none', 'limits')
EVERY_ROUTE = ('generic', 'dead_ones', 'dead_zero_start', 'duplicate', 'zero_row')
REPRESENTATIVE = ('dead_q', 'all_zero', 'positive_none', 'limits', 'warm_at_solution')
# f32 scenes that fall back to the reference's own f32 noise (conftest.assert_within_f32_noise) where the oracle's f32 run itself
# leaves its f64 run on more than 10 % of the samples (judge_b)
F32_NOISE_SCENES = ('tight',)


# ---------------------------------------------------------------------------------------------------- the dispatch, restated
def padded_ld(k):                # csrc/cd_solver.hip:568
    return 64 if k <= 64 else 128 if k <= 128 else 256 if k <= 256 else 512 if k <= 512 else 1024


def _au(x):
    return -(-x // 256) * 256


def slot_count(tsz, b, k):       # csrc/cd_solver.hip:600-607
    ld = max(128, padded_ld(k))
    return min(max(1, (64 << 20) // (ld * ld * tsz)), max(b, 1)), ld


def expected_workspace(dt, b, k, multi):
    """modl_enet_regression_workspace restated (csrc/code_solve.hip:142-154): (total, padded-copy term, slot term)."""
    t = 4 if dt == 'f32' else 8
    chol = -(-k // 64) * 64 * 64 if k > 128 else 0                      # csrc/chol.hip:512
    base = _au(t * b) + _au(t * b * k) + _au(t * (k * k * (b if multi and k <= 512 else 1) + chol))
    copy = slots = 0
    if not multi and 0 < k <= 1024 and (padded_ld(k) != k or k > 256):
        copy = _au(t * (padded_ld(k) + 16) * padded_ld(k))
    if multi and 32 <= k <= 1024:
        n, ld = slot_count(t, b, k)
        slots = _au(n * ld * ld * t)
    return base + copy + slots, copy, slots


def expected_route(dt, k, b, multi=False, misaligned=False, split=1):
    """The route of the product library (see the module docstring for the lines restated)."""
    t = 4 if dt == 'f32' else 8
    if k > 1024:
        return 'wide'
    split_wanted = split != 0 or k > 256
    if multi:
        in_place = k in (128, 256, 512, 1024)
        if k >= 32 and (split != 0 or k > 256) and not in_place:
            n, ld = slot_count(t, b, k)
            return 'split%d/slots/slices%d' % (ld, -(-b // n))
        if split_wanted and in_place:
            return 'split%d/in_place' % k
        kpl = 1 if k <= 64 else 2 if k <= 128 else 4
        return 'one_wave/kpl%d/%s' % (kpl, 'vector' if k == 64 * kpl else 'element')
    copied = padded_ld(k) != k or (k > 256 and misaligned)
    ld = padded_ld(k)
    aligned = copied or not misaligned
    if split_wanted and ld >= 128 and k >= 32 and aligned:
        return 'split%d/%s' % (ld, 'copy' if copied else 'in_place')
    kpl = 1 if k <= 64 else 2 if k <= 128 else 4
    return 'one_wave/kpl%d/%s' % (kpl, 'padded' if copied else ('vector' if aligned else 'element'))


def batch_of(k):
    return 20 if k <= 513 else 6


ROUTES = []


def _route(name, k, want, cite, b=None, multi=False, misaligned=False, sw=None, dts=('f64', 'f32'), extra=False):
    ROUTES.append(SimpleNamespace(name=name, k=k, b=b or batch_of(k), multi=multi, misaligned=misaligned, sw=dict(sw or {}),
                                  dts=dts, want=want, cite=cite, extra=extra))


for _k, _want, _cite in ((5, 'one_wave/kpl1/padded', 'A:19 S:545 P:20 S:547 S:498'), (31, 'one_wave/kpl1/padded', 'A:19 P:22 S:547 S:498'),
                         (32, 'one_wave/kpl1/padded', 'A:19 P:20 S:547'), (33, 'one_wave/kpl1/padded', 'A:19 P:20 S:547'),
                         (70, 'split128/copy', 'A:19 S:545 P:33'), (128, 'split128/in_place', 'A:19 S:545 P:33'),
                         (129, 'split256/copy', 'A:19 P:34'), (256, 'split256/in_place', 'P:34'), (257, 'split512/copy', 'A:19 P:35'),
                         (512, 'split512/in_place', 'P:35'), (513, 'split1024/copy', 'A:19 P:36'), (1024, 'split1024/in_place', 'P:36'),
                         (1025, 'wide', 'A:16')):
    _route('shared-k%d' % _k, _k, _want, _cite, extra=_k in (31, 70, 256, 513, 1025))
_route('misaligned-k128', 128, 'one_wave/kpl2/element', 'A:19 P:23 S:548 S:496', misaligned=True)
_route('misaligned-k256', 256, 'one_wave/kpl4/element', 'A:19 P:23 S:549 S:496', misaligned=True)
_route('multi-k128', 128, 'split128/in_place', 'A:20 A:87 S:545', multi=True)
_route('multi-k70', 70, 'split128/slots/slices1', 'A:20-21 A:75-79 S:617', multi=True, extra=True)
_route('multi-k513-two-slices', 513, 'split1024/slots/slices2', 'A:20-21 A:75-79 S:589 S:601-607 S:623', b=9, multi=True, dts=('f64',))
_route('multi-k20', 20, 'one_wave/kpl1/element', 'A:20 S:547 S:496', b=5, multi=True)
_route('multi-k1025', 1025, 'wide', 'A:16', multi=True)
for _pct in (-1, 0, 100):
    for _k, _want in ((70, 'one_wave/kpl2/padded'), (128, 'one_wave/kpl2/vector'), (200, 'one_wave/kpl4/padded'),
                      (256, 'one_wave/kpl4/vector')):
        _sw = {'CD_SPLIT': 0}
        if _pct >= 0:
            _sw['CD_SPARSE_PCT'] = _pct
        _route('split0%s-k%d' % ('' if _pct < 0 else '-pct%d' % _pct, _k), _k, _want, 'S:543-545 S:533 S:548-549 S:498', sw=_sw)
ROUTE_BY_NAME = {r.name: r for r in ROUTES}


# ---------------------------------------------------------------------------------------------------- scenes
def special_positions(k):
    pos = {0, k - 1, k // 3, k // 3 + 1}
    if k > 64:
        pos |= {63, 64}
    return sorted(pos)


def duplicate_pairs(k):
    """(original, copy) pairs of the `duplicate` scene"""
    return [(4, 5), (0, k - 1)] if k >= 7 else [(1, 2), (0, k - 1)]


@functools.lru_cache(maxsize=3)
def _draws(k, b, p, multi, seed):
    rs = np.random.RandomState(seed)
    Ds = []
    for _ in range(b if multi else 1):
        D = rs.randn(k, p)
        Ds.append(D / np.sqrt((D ** 2).sum(1))[:, None])
    Z = rs.randn(b, k) * (rs.rand(b, k) < 0.1)
    noise = 0.1 * rs.randn(b, p)
    idx = rs.permutation(b + 3)[:b].astype(np.int64)
    return Ds, Z, noise, idx


VARIANTS = {
    'generic': [dict()],
    'dead_ones': [dict(max_iter=20)],
    'dead_zero_start': [dict()],
    'dead_q': [dict(max_iter=30)],
    'duplicate': [dict(l1_ratio=1.0), dict(l1_ratio=0.7)],
    'all_zero': [dict(l1_ratio=1.0)],
    'positive_none': [dict(positive=True)],
    'zero_row': [dict(max_iter=30, start='ones'), dict(max_iter=30, start='zeros')],
    'limits': [dict(max_iter=0), dict(max_iter=1), dict(max_iter=2), dict(max_iter=25, tol=0.0), dict(tol=1e9)],
    'warm_at_solution': [dict()],
    'tight': [dict(tol=tol, max_iter=1000, l1_ratio=l1, positive=pos) for l1 in (1.0, 0.5) for pos in (False, True)
              for tol in (1e-4, 1e-6)],
}
LIMITS_SWEEPS = (0, 1, 2, 25, 1)
ZERO_ROW = 1


def make_case(dt, k, b, scene, variant=None, multi=False, p=None, seed=None):
    """One call's inputs: G (k, k) or (b, k, k), Dx (b, k), X (b, p), code0 (b + 3, k), idx, the scalar arguments, `dead`."""
    dtn = dt if isinstance(dt, str) else [n for n, d in DT.items() if d == dt][0]
    dt = DT[dtn]
    v = dict(l1_ratio=0.9, alpha=0.3, positive=False, tol=1e-2, max_iter=100, start='ones')
    v.update(variant or {})
    p = p if p is not None else k + 80
    if seed is None:
        seed = zlib.crc32(('%d-%d-%d-%d' % (k, b, p, multi)).encode()) % 100000
    Ds, Z, noise, idx = _draws(k, b, p, bool(multi), seed)
    dead, pairs = [], []
    if scene == 'positive_none':
        Ds = [np.abs(D) / np.sqrt((D ** 2).sum(1))[:, None] for D in Ds]
    elif scene.startswith('dead'):
        dead = special_positions(k)
        Ds = [D.copy() for D in Ds]
        for D in Ds:
            D[dead] = 0
    elif scene == 'duplicate':
        pairs = duplicate_pairs(k)
        Ds = [D.copy() for D in Ds]
        Z = Z.copy()
        for D in Ds:
            for src, cp in pairs:
                D[cp] = D[src]
        Z[:, [cp for _, cp in pairs]] = 0               # (the signal is on the originals alone)
        Z[:, pairs[0][0]] = 1.0
        Z[:, 0] = -1.5
    if scene == 'positive_none':
        X = -np.abs(noise) * 10
    elif multi:
        X = np.stack([Z[i].dot(Ds[i]) for i in range(b)]) + noise
    else:
        X = Z.dot(Ds[0]) + noise
    X = np.ascontiguousarray(X.astype(dt))
    Dd = [D.astype(dt) for D in Ds]
    Gs = []
    for D in Dd:
        G = D.dot(D.T).astype(dt)
        Gs.append((G + G.T) / 2)
    if multi:
        G = np.ascontiguousarray(np.stack(Gs))
        Dx = np.ascontiguousarray(np.stack([X[i].dot(Dd[i].T) for i in range(b)]).astype(dt))
    else:
        G = np.ascontiguousarray(Gs[0])
        Dx = np.ascontiguousarray(X.dot(Dd[0].T).astype(dt))
    assert G.dtype == dt and Dx.dtype == dt
    start = np.ones((b, k), dtype=dt) if v['start'] == 'ones' else np.zeros((b, k), dtype=dt)
    if scene in ('dead_zero_start', 'dead_q'):
        start[:, dead] = 0
    if scene == 'dead_q':
        Dx[:, dead] = 3 * v['alpha']
    if scene == 'zero_row':
        X[ZERO_ROW] = 0
        Dx[ZERO_ROW] = 0
    if scene == 'all_zero':
        v['alpha'] = 1.5 * float(np.abs(Dx).max())
    ties = sorted(c for pr in pairs for c in pr) if v['l1_ratio'] == 1.0 else []
    case = SimpleNamespace(dt=dt, dtn=dtn, k=k, b=b, p=p, multi=bool(multi), scene=scene, G=G, Dx=Dx, X=X, idx=idx, dead=dead,
                           pairs=pairs, ties=ties, D=Dd, Xbuf=None, ldx=p, **{n: v[n] for n in ('l1_ratio', 'alpha', 'positive', 'tol', 'max_iter')})
    if scene == 'warm_at_solution':
        cold = SimpleNamespace(**vars(case))
        cold.code0 = _code0(b, k, idx, start, dt)
        cold.tol, cold.max_iter = 1e-6, 1000
        start = run_oracle(cold)[0][idx]
    case.code0 = _code0(b, k, idx, start, dt)
    return case


def _code0(b, k, idx, start, dt):
    code0 = np.full((b + 3, k), FILL, dtype=dt)
    code0[idx] = start
    return code0


X_LAYOUT = [(p, pad) for p in (1, 3, 1027, 4101) for pad in (3, 1)]
LAST_ONLY_ROW = 2


def make_x_layout_case(dt, p, pad, k=70, b=20):
    """`x_layout`: the generic scene at p features with X in a (b, p + pad) buffer whose padding is NaN; row 2's only
    non-zero is its last element."""
    case = make_case(dt, k, b, 'generic', dict(max_iter=30), p=p)
    case.scene = 'x_layout'
    case.ties = list(range(k)) if p == 1 else []        # (one feature: every atom is a copy of every other, up to its sign)
    case.X[LAST_ONLY_ROW] = 0
    case.X[LAST_ONLY_ROW, p - 1] = 1.0
    case.Dx[LAST_ONLY_ROW] = case.X[LAST_ONLY_ROW].dot(case.D[0].T)
    case.ldx = p + pad
    case.Xbuf = np.full((b, p + pad), np.nan, dtype=case.dt)
    case.Xbuf[:, :p] = case.X
    return case


# ---------------------------------------------------------------------------------------------------- the three solvers on a case
def run_oracle(case, dt=None):
    """(code (b + 3, k), sweeps) of the CPU oracle, on the case's arrays as type dt"""
    dt = case.dt if dt is None else dt
    code = case.code0.astype(dt)
    sw = np.zeros(case.b, dtype=np.int32)
    f = _orc.enet_regression_multi_gram if case.multi else _orc.enet_regression_single_gram
    f(case.G.astype(dt), case.Dx.astype(dt), case.X.astype(dt), code, case.idx, case.l1_ratio, case.alpha, case.positive, case.tol,
      case.max_iter, sweeps=sw)
    return code, sw


def restated_cd(w, a, beta, Q, q, y2, max_iter, tol, positive, mut=(), alpha_full=None, order=None):
    """enet_coordinate_descent_gram (the reference's dict_fact_fast.pyx:270-427, as oracle/somf_oracle_impl.inc states it) for one
    sample in f64 numpy, with the hooks of the mutants.  Returns (w, sweeps)."""
    w = np.array(w, dtype=np.float64)
    k = len(w)
    diag = np.diag(Q).copy()
    live = diag != 0
    tol_abs = tol if 'tol_unscaled' in mut else tol * y2
    H = Q.dot(w)
    order = range(k) if order is None else order
    n_iter = 0
    while n_iter < max_iter:
        w_max = d_w_max = 0.0
        for ii in order:
            Qii = diag[ii]
            if Qii == 0.0:
                if 'dead_in_w_max' in mut:
                    w_max = max(w_max, abs(w[ii]))
                continue
            w_ii = w[ii]
            if 'fused_order' in mut:       # not a mutant: the step as the four-wavefront solver orders it (csrc/cd_split_impl.hpp)
                z = (q[ii] + Qii * w_ii) - H[ii]
                cl = min(z, a) if positive else min(max(z, -a), a)
                w[ii] = (z - cl) * (1.0 / (Qii + beta))
                H += w[ii] * Q[ii] - w_ii * Q[ii]
                d_w_max = max(d_w_max, abs(w[ii] - w_ii))
                w_max = max(w_max, abs(w[ii]))
                continue
            if w_ii != 0.0:
                H -= w_ii * Q[ii]
            tmp = q[ii] - H[ii]
            if positive and tmp < 0.0:
                w[ii] = 0.0
            else:
                thr = alpha_full if 'alpha_not_l1' in mut else a
                den = Qii if 'no_beta_in_step' in mut else Qii + beta
                w[ii] = np.sign(tmp) * max(abs(tmp) - thr, 0.0) / den
            if w[ii] != 0.0:
                H += w[ii] * Q[ii]
            d_w_max = max(d_w_max, abs(w[ii] - w_ii))
            w_max = max(w_max, abs(w[ii]))
        last = n_iter == max_iter - 1 and 'no_gap_at_last' not in mut
        zero_exit = w_max == 0.0 and 'no_w_max_exit' not in mut
        if zero_exit or (w_max != 0.0 and d_w_max / w_max < tol) or last:
            wn = np.where(live, w, 0.0) if 'dead_out_of_norms' in mut else w
            q_dot_w = w.dot(q)
            XtA = q - H - beta * w
            if 'dead_out_of_dual' in mut:
                XtA = XtA[live]
            dual = (np.abs(XtA).max() if 'abs_dual_positive' in mut else XtA.max()) if positive else np.abs(XtA).max()
            R = y2 + w.dot(H) - 2.0 * q_dot_w
            if dual > a:
                cst = a / dual
                gap = 0.5 * (R + R * cst * cst)
            else:
                cst = 1.0
                gap = R
            gap += a * np.abs(wn).sum() - cst * y2 + cst * q_dot_w + 0.5 * beta * (1.0 + cst * cst) * wn.dot(wn)
            if gap < tol_abs:
                if 'count_off_by_one' not in mut:
                    n_iter += 1
                break
        n_iter += 1
    if 'dead_zeroed' in mut:
        w[~live] = 0.0
    return w, n_iter


def run_restated(case, mut=()):
    """`restated_cd` on every sample of the case (f64): (code, sweeps)"""
    code = case.code0.astype(np.float64)
    sw = np.zeros(case.b, dtype=np.int32)
    a, beta = case.alpha * case.l1_ratio, case.alpha * (1.0 - case.l1_ratio)
    Xn = case.X.astype(np.float64)
    if 'ynorm_over_ldx' in mut and case.Xbuf is not None:
        Xn = case.Xbuf.astype(np.float64)
    order = None
    if 'reverse_duplicates' in mut and case.pairs:
        order = list(range(case.k))
        for src, cp in case.pairs:
            i, j = order.index(src), order.index(cp)
            order[i], order[j] = order[j], order[i]
    for i in range(case.b):
        Q = (case.G[i] if case.multi else case.G).astype(np.float64)
        w, sw[i] = restated_cd(code[case.idx[i]], a, beta, Q, case.Dx[i].astype(np.float64), float(Xn[i].dot(Xn[i])), case.max_iter,
                               case.tol, case.positive, mut, alpha_full=case.alpha, order=order)
        code[case.idx[i]] = w
    return code, sw


def solve_star(case):
    """w* (b, k): the minimiser of P on the case's inputs as given (cast to f64), by plain coordinate descent in numpy - all
    samples at once, sweeps over the coordinates that are non-zero or violate their optimality condition - until the KKT
    residual of every coordinate of every sample is below 1e-13.  Nothing here comes from the oracle."""
    G, q = case.G.astype(np.float64), case.Dx.astype(np.float64)
    b, k = q.shape
    a, beta, pos = case.alpha * case.l1_ratio, case.alpha * (1.0 - case.l1_ratio), case.positive
    diag = np.einsum('bjj->bj', G) if case.multi else np.diag(G)[None, :].repeat(b, 0)
    assert np.all(diag > 0)
    w = np.zeros((b, k))
    for _ in range(400):
        H = np.einsum('bj,bjk->bk', w, G) if case.multi else w.dot(G)
        g = q - H - beta * w
        if pos:
            r = np.where(w > 0, np.abs(g - a), np.maximum(g - a, 0.0))
        else:
            r = np.where(w != 0, np.abs(g - a * np.sign(w)), np.maximum(np.abs(g) - a, 0.0))
        if r.max() < 1e-13:
            return w
        cand = np.nonzero(((w != 0) | (r > 0)).any(axis=0))[0]
        for _ in range(25):
            for j in cand:
                Gj = G[:, j, :] if case.multi else G[j]
                dj, wj = diag[:, j], w[:, j]
                tmp = q[:, j] - H[:, j] + dj * wj
                new = np.maximum(tmp - a, 0.0) if pos else np.sign(tmp) * np.maximum(np.abs(tmp) - a, 0.0)
                new /= dj + beta
                d = new - wj
                if d.any():
                    H += d[:, None] * Gj
                    w[:, j] = new
    raise AssertionError('solve_star did not reach a KKT residual of 1e-13: %.3e' % r.max())


_STAR = {}


def star_of(case, key):
    """w*, mu = lambda_min(G) + beta and |x|^2 per sample, cached per (route, dtype, l1_ratio, positive): tol and max_iter do
    not enter"""
    key = key + (case.dtn, case.l1_ratio, case.positive)
    if key not in _STAR:
        G = case.G.astype(np.float64)
        lam = np.array([np.linalg.eigvalsh(g)[0] for g in G]) if case.multi else np.full(case.b, np.linalg.eigvalsh(G)[0])
        X = case.X.astype(np.float64)
        _STAR[key] = (solve_star(case), lam + case.alpha * (1.0 - case.l1_ratio), (X * X).sum(1))
    return _STAR[key]


def primal(case, w):
    """P(w) per sample, f64, on the inputs as given"""
    G, q, w = case.G.astype(np.float64), case.Dx.astype(np.float64), np.asarray(w, dtype=np.float64)
    a, beta = case.alpha * case.l1_ratio, case.alpha * (1.0 - case.l1_ratio)
    X = case.X.astype(np.float64)
    Gw = np.einsum('bj,bjk->bk', w, G) if case.multi else w.dot(G)
    return 0.5 * (X * X).sum(1) - (w * q).sum(1) + 0.5 * (w * Gw).sum(1) + a * np.abs(w).sum(1) + 0.5 * beta * (w * w).sum(1)


# ---------------------------------------------------------------------------------------------------- the judges
FIGURES = {}                     # judge -> the largest error / bound seen (printed, recorded in DESIGN.md, not asserted)


def _note(judge, value):
    FIGURES[judge] = max(FIGURES.get(judge, 0.0), float(value))


def _untouched(case, code):
    outside = np.setdiff1d(np.arange(case.b + 3), case.idx)
    assert code[outside].tobytes() == case.code0[outside].tobytes(), 'rows of the code array outside idx were written'
    if case.dead:
        np.testing.assert_array_equal(code[case.idx][:, case.dead], case.code0[case.idx][:, case.dead],
                                      err_msg='a dead coefficient (zero diagonal) changed')


def support_mismatch(w, ref, ties=(), scale=None):
    """(sample, coordinate) pairs where one of w, ref is zero and the other is not.  Not counted: a coordinate of `ties`
    (copies of one atom: see EXACT TIES in the module docstring) where both values are within k eps max(1, |q|_max, |w|_max) of
    zero - the soft threshold's argument sits ON the threshold there and its sign is a matter of rounding order."""
    w, ref = np.asarray(w, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    ne = (w != 0) != (ref != 0)
    if len(ties):
        scale = np.maximum(1.0, np.maximum(np.abs(ref).max(1), 0.0 if scale is None else scale))
        lim = (w.shape[1] * np.finfo(np.float64).eps * scale)[:, None]
        tie = np.zeros_like(ne)
        tie[:, list(ties)] = True
        ne &= ~(tie & (np.abs(w) <= lim) & (np.abs(ref) <= lim))
    return np.argwhere(ne)


def judge_a(case, got, ref):
    (code, sw), (rcode, rsw) = got, ref
    np.testing.assert_array_equal(sw, rsw, err_msg='sweep counts')
    err = rel_fro(code[case.idx], rcode[case.idx])
    _note('A rel_fro / 1e-10', err / 1e-10)
    assert err < 1e-10, ('rel_fro', err)
    bad = support_mismatch(code[case.idx], rcode[case.idx], case.ties, np.abs(case.Dx).max(1))
    assert len(bad) == 0, ('support', [(i, j, code[case.idx][i, j], rcode[case.idx][i, j]) for i, j in bad[:8]])
    _untouched(case, code)
    if case.max_iter == 0:
        assert code.tobytes() == case.code0.tobytes(), 'max_iter = 0 changed the code'


def judge_b(case, got, ref, ref64=None):
    """ref64: a callable giving the oracle's f64 run on the same (f32) inputs, for F32_NOISE_SCENES"""
    (code, sw), (rcode, rsw) = got, ref
    w, rw = code[case.idx].astype(np.float64), rcode[case.idx].astype(np.float64)
    if case.scene in FORCED:
        np.testing.assert_array_equal(sw, rsw, err_msg='sweep counts (forced by the scene)')
        same = np.ones(case.b, dtype=bool)
    else:
        if case.scene == 'zero_row':
            assert sw[ZERO_ROW] == rsw[ZERO_ROW] == case.max_iter, (sw[ZERO_ROW], rsw[ZERO_ROW])
            assert np.all(w[ZERO_ROW] == 0)
        same = sw == rsw
        if same.mean() < 0.9 and case.scene in F32_NOISE_SCENES:
            # the rule cannot be met where the reference's own f32 run leaves its f64 run on more than 10 % of the samples
            # (at tol 1e-6 the gap's f32 rounding is within a factor of ten of tol |x|^2): shown here with the oracle, and the
            # codes are then held to the reference's own f32 noise instead, on every sample
            code64, sw64 = ref64()
            assert (rsw == sw64).mean() < 0.9, ('the reference keeps its sweep counts in f32, the kernel does not', sw, rsw, sw64)
            err, noise = assert_within_f32_noise(w, rw, code64[case.idx], case.scene)
            _note('B (f32 noise rule) err / (2 noise + 1e-5)', err / (2 * noise + 1e-5))
            _untouched(case, code)
            return
        _note('B share of samples with other sweep counts / 0.1', (1.0 - same.mean()) / 0.1)
        assert same.mean() >= 0.9, ('sweep counts differ on more than 10 % of the samples', sw, rsw)
    if case.p < case.k:            # no unique minimiser: through the fit w D
        D = case.D[0].astype(np.float64)
        err = rel_fro(w[same].dot(D), rw[same].dot(D))
        _note('B rel_fro of the fit / 1e-4', err / 1e-4)
        assert err < 1e-4, ('rel_fro of the fit', err)
    else:
        err = rel_fro(w[same], rw[same])
        _note('B rel_fro / 2e-5', err / 2e-5)
        assert err < 2e-5, ('rel_fro', err)
    _untouched(case, code)
    if case.max_iter == 0:
        assert code.tobytes() == case.code0.tobytes(), 'max_iter = 0 changed the code'


def judge_c(case, got, key, who='C'):
    """Returns the largest share of either bound that a stopped sample used."""
    code, sw = got
    wstar, mu, y2 = star_of(case, key)
    w = code[case.idx].astype(np.float64)
    stopped = sw < case.max_iter
    assert stopped.any(), 'judge C is vacuous here: no sample stopped before max_iter'
    assert np.all(mu > 0)
    bound = case.tol * y2
    sub = (primal(case, w) - primal(case, wstar)) / bound
    dist = ((w - wstar) ** 2).sum(1) / (2.0 * bound / mu)
    share = max(sub[stopped].max(), dist[stopped].max())
    _note(who + ' suboptimality / bound', sub[stopped].max())
    _note(who + ' distance / bound', dist[stopped].max())
    assert sub[stopped].max() <= 1.0, ('P(w) - P(w*) over tol |x|^2', sub)
    assert dist[stopped].max() <= 1.0, ('|w - w*|^2 over 2 tol |x|^2 / mu', dist)
    return share


def accepts(judge, *args):
    kept = dict(FIGURES)             # (a mutant's figures are not the kernels')
    try:
        judge(*args)
    except AssertionError:
        return False
    finally:
        FIGURES.clear()
        FIGURES.update(kept)
    return True


# ---------------------------------------------------------------------------------------------------- CPU tests
CPU_K = (70, 31)


def _cpu_cases(dt, k, b=8):
    for scene, variants in VARIANTS.items():
        for v in variants:
            yield make_case(dt, k, b, scene, v)
    yield make_case(dt, k, b, 'generic', multi=True)
    yield make_x_layout_case(dt, 3, 3, k=k, b=b)


@pytest.mark.parametrize('k', CPU_K)
def test_restatement(k):
    """`restated_cd` equals the oracle on every scene: same sweeps, 1e-12."""
    for case in _cpu_cases('f64', k):
        if case.scene == 'tight' and case.tol < 1e-5:
            continue                                   # (the same code path as tol 1e-4, five times the sweeps in Python)
        code, sw = run_restated(case)
        rcode, rsw = run_oracle(case)
        np.testing.assert_array_equal(sw, rsw, err_msg=case.scene)
        assert rel_fro(code, rcode) < 1e-12, (case.scene, rel_fro(code, rcode))


@pytest.mark.parametrize('dt', ['f32', 'f64'])
@pytest.mark.parametrize('k', CPU_K)
def test_scenes_are_what_they_claim(dt, k):
    b = 20
    run = lambda scene, i=0: (lambda c: (c,) + run_oracle(c))(make_case(dt, k, b, scene, VARIANTS[scene][i]))   # noqa: E731
    case, code, sw = run('generic')
    assert sw.min() > 1 and sw.max() < case.max_iter and len(set(case.idx.tolist())) == b and case.code0.shape[0] == b + 3
    case, code, sw = run('dead_ones')
    assert case.dead == special_positions(k) and np.all(np.diag(case.G)[case.dead] == 0) and np.all(case.Dx[:, case.dead] == 0)
    assert np.all(case.G[case.dead] == 0) and np.all(case.G[:, case.dead] == 0)
    assert np.all(sw == case.max_iter) and np.all(code[case.idx][:, case.dead] == 1)
    where = special_positions(200)
    assert 63 in where and 64 in where and 0 in where and 199 in where and any(b_ - a_ == 1 for a_, b_ in zip(where, where[1:]))
    case, code, sw = run('dead_zero_start')
    assert np.all(sw < case.max_iter) and np.all(code[case.idx][:, case.dead] == 0)
    case, code, sw = run('dead_q')
    assert np.all(case.Dx[:, case.dead] == case.dt(3 * case.alpha)) and np.all(code[case.idx][:, case.dead] == 0)
    plain = run_oracle(make_case(dt, k, b, 'dead_zero_start', dict(max_iter=30)))[1]
    assert np.any(sw != plain), 'the dead right-hand sides do not reach the stopping rule'
    for i in (0, 1):
        case, code, sw = run('duplicate', i)
        for src, cp in case.pairs:
            np.testing.assert_array_equal(case.D[0][src], case.D[0][cp])
            np.testing.assert_allclose(case.G[src], case.G[cp], rtol=0, atol=1e-6)   # (as the product forms it: equal to rounding)
            assert np.all((code[case.idx][:, src] != 0) | (code[case.idx][:, cp] != 0))
    for scene in ('all_zero', 'positive_none'):
        case, code, sw = run(scene)
        assert np.all(sw == 1) and np.all(code[case.idx] == 0), (scene, sw)
    assert np.all(case.Dx < 0)
    for i in (0, 1):
        case, code, sw = run('zero_row', i)
        assert not case.X[ZERO_ROW].any() and sw[ZERO_ROW] == case.max_iter and not code[case.idx[ZERO_ROW]].any()
        assert np.all(np.delete(sw, ZERO_ROW) < case.max_iter)
    for i, want in enumerate(LIMITS_SWEEPS):
        case, code, sw = run('limits', i)
        assert np.all(sw == want), (i, sw)
        if case.max_iter == 0:
            assert code.tobytes() == case.code0.tobytes()
    case, code, sw = run('warm_at_solution')
    assert np.all(sw == 1)
    case = make_x_layout_case(dt, 1027, 3)
    assert np.isnan(case.Xbuf[:, case.p:]).all() and np.count_nonzero(case.X[LAST_ONLY_ROW]) == 1 and case.X[LAST_ONLY_ROW, -1] == 1
    assert run_oracle(case)[1][LAST_ONLY_ROW] < case.max_iter


def test_exact_ties_are_a_matter_of_rounding_order():
    """EXACT TIES (module docstring): `fused_order`, the same step in the operation order of the four-wavefront solver, passes
    judge A on every scene - and, compared literally, flips the support of the oracle where atoms are copies of each other."""
    flips = 0
    for case in list(_cpu_cases('f64', 70, b=20)) + [make_x_layout_case('f64', 1, 3), make_case('f64', 257, 20, 'duplicate', dict(l1_ratio=1.0))]:
        if case.scene == 'tight' and case.tol < 1e-5:
            continue
        ref = run_oracle(case)
        for got in (run_restated(case, ('fused_order',)), run_restated(case)):
            judge_a(case, got, ref)
            literal = support_mismatch(got[0][case.idx], ref[0][case.idx])
            assert len(literal) == 0 or case.ties, case.scene
            assert all(j in case.ties for _, j in literal)
            flips += len(literal)
    print('%d coefficients at an exact tie differ from the oracle in being zero' % flips)
    assert flips > 0


MUTANTS = {
    'dead_zeroed': 'dead_ones', 'dead_in_w_max': None, 'dead_out_of_norms': 'dead_ones', 'dead_out_of_dual': 'dead_q',
    'abs_dual_positive': 'positive_none', 'no_gap_at_last': None, 'tol_unscaled': 'zero_row', 'ynorm_over_ldx': 'x_layout',
    'count_off_by_one': 'generic', 'no_w_max_exit': 'all_zero', 'alpha_not_l1': 'generic', 'no_beta_in_step': 'generic',
    'reverse_duplicates': 'duplicate',
}


def _mutant_cases(scene, k=70, b=8):
    if scene == 'x_layout':
        return [make_x_layout_case('f64', 1027, 3, k=k, b=b)]
    return [make_case('f64', k, b, scene, v) for v in VARIANTS[scene]]


def test_mutants():
    """Every mutant of the sweep is rejected by its named scene under judge A; the two invisible ones by none."""
    refs = {}

    def rejected(mut, scene):
        out = False
        for i, case in enumerate(_mutant_cases(scene)):
            if (scene, i) not in refs:
                refs[scene, i] = run_oracle(case)
                judge_a(case, run_restated(case), refs[scene, i])      # (the unmutated restatement passes)
            out = out or not accepts(judge_a, case, run_restated(case, (mut,)), refs[scene, i])
        return out
    for mut, scene in MUTANTS.items():
        if scene is not None:
            assert rejected(mut, scene), '%s survives %s' % (mut, scene)
    for scene in ('dead_ones', 'dead_zero_start', 'dead_q', 'all_zero', 'limits', 'generic'):
        assert not rejected('dead_in_w_max', scene), scene
    for scene in ('limits', 'generic', 'dead_ones'):
        assert not rejected('no_gap_at_last', scene), scene


def _judge_c_cases(route, dt):
    yield make_case(dt, route.k, route.b, 'generic', multi=route.multi)
    for v in VARIANTS['tight']:
        yield make_case(dt, route.k, route.b, 'tight', v, multi=route.multi)


@pytest.mark.parametrize('dt', ['f32', 'f64'])
@pytest.mark.parametrize('name', [r.name for r in ROUTES if r.extra])
def test_judge_c_on_the_oracle(name, dt):
    """Judge C is neither vacuous nor unreachable: on every case it is applied to, samples stop before max_iter and the
    oracle alone uses at most ORACLE_SHARE_OF_C of either bound."""
    route = ROUTE_BY_NAME[name]
    worst = 0.0
    for case in _judge_c_cases(route, dt):
        share = judge_c(case, run_oracle(case), (name,), who='C (oracle)')
        worst = max(worst, share)
        assert share <= ORACLE_SHARE_OF_C, (case.tol, case.l1_ratio, case.positive, share)
    print('%s %s: the oracle uses %.3f %% of judge C at most' % (name, dt, 100 * worst))


def test_judge_c_rejects_a_wrong_objective():
    """A solver that stops on a gap ten thousand times too wide, or minimises with alpha in place of alpha l1_ratio, fails C."""
    case = make_case('f64', 70, 8, 'tight', dict(tol=1e-6, max_iter=1000, l1_ratio=0.5))
    loose = SimpleNamespace(**vars(case))
    loose.tol = 1e-1
    code, sw = run_oracle(loose)
    assert not accepts(judge_c, case, (code, np.minimum(sw, 1)), ('mutant',))
    assert not accepts(judge_c, case, run_restated(case, ('alpha_not_l1',)), ('mutant',))
    assert accepts(judge_c, case, run_oracle(case), ('mutant',))


def test_route_table():
    """ROUTES names what the dispatch does; every route runs the five common scenes, the representatives all of them."""
    for r in ROUTES:
        for dt in r.dts:
            assert expected_route(dt, r.k, r.b, r.multi, r.misaligned, r.sw.get('CD_SPLIT', 1)) == r.want, (r.name, dt)
    want = {'one_wave/kpl1/padded', 'one_wave/kpl2/padded', 'one_wave/kpl4/padded', 'one_wave/kpl2/vector', 'one_wave/kpl4/vector',
            'one_wave/kpl1/element', 'one_wave/kpl2/element', 'one_wave/kpl4/element', 'split128/copy', 'split128/in_place',
            'split256/copy', 'split256/in_place', 'split512/copy', 'split512/in_place', 'split1024/copy', 'split1024/in_place',
            'split128/slots/slices1', 'split1024/slots/slices2', 'wide'}
    assert want <= set(r.want for r in ROUTES)
    assert expected_route('f32', 513, 9, True) == 'split1024/slots/slices1'        # (why the two-slice route is f64 only)
    assert sorted(r.k for r in ROUTES if r.extra and not r.multi) == [31, 70, 256, 513, 1025]
    assert [r.k for r in ROUTES if r.extra and r.multi] == [70]
    assert set(k for r in ROUTES for k in (r.k,)) >= {31, 32, 33, 129, 257, 513}
    assert len(set(r.name for r in ROUTES)) == len(ROUTES)


def test_workspace_table():
    """modl_enet_regression_workspace against the padded-copy and slot terms recomputed from cd_padded_ld and the 64 MiB rule."""
    from modl_amd._lib import lib
    for r in ROUTES:
        for dt in ('f32', 'f64'):
            got = lib.modl_enet_regression_workspace(0 if dt == 'f32' else 1, r.b, r.k, int(r.multi))
            total, copy, slots = expected_workspace(dt, r.b, r.k, r.multi)
            assert got == total, (r.name, dt, got, total, copy, slots)
    assert expected_workspace('f32', 20, 128, False)[1] == 0
    assert expected_workspace('f32', 20, 129, False)[1] == _au(4 * (256 + 16) * 256)
    assert expected_workspace('f64', 20, 512, False)[1] == _au(8 * (512 + 16) * 512)       # (for a misaligned caller's matrix)
    assert expected_workspace('f64', 9, 513, True)[2] == 8 * 1024 * 1024 * 8 and slot_count(8, 9, 513) == (8, 1024)
    assert expected_workspace('f32', 9, 513, True)[2] == 9 * 1024 * 1024 * 4
    assert expected_workspace('f64', 20, 70, True)[2] == 20 * 128 * 128 * 8
    assert expected_workspace('f64', 5, 20, True)[1:] == (0, 0) and expected_workspace('f64', 6, 1025, True)[1:] == (0, 0)


def test_refusals_before_any_device_work():
    """Bad arguments are answered before anything touches a device (the pointers here are never dereferenced)."""
    from modl_amd._lib import lib
    EINVAL, ENOMEM, OK = -1, -2, 0
    fake = C.c_void_p(4096)
    kmax = lib.modl_max_components()
    for sfx, multi in (('f32', 0), ('f64', 0), ('f32', 1), ('f64', 1)):
        f = getattr(lib, 'modl_enet_regression_%s_gram_%s' % ('multi' if multi else 'single', sfx))

        def call(b=4, k=70, p=10, ldx=10, l1=0.5, ws=None):
            need = lib.modl_enet_regression_workspace(0 if sfx == 'f32' else 1, b, k, multi)
            return f(fake, fake, fake, ldx, p, fake, fake, b, k, l1, 0.3, 0, 1e-2, 10, None, fake, need if ws is None else need + ws,
                     None)
        assert call(k=0) == EINVAL and call(k=kmax + 1) == EINVAL and call(ldx=9) == EINVAL
        assert call(l1=-0.1) == EINVAL and call(l1=1.5) == EINVAL and call(l1=float('nan')) == EINVAL
        assert call(ws=-1) == ENOMEM and call(k=kmax, ws=-1) == ENOMEM
        assert call(b=0) == OK


# ---------------------------------------------------------------------------------------------------- GPU tests
@pytest.fixture(scope='module')
def fast():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    from modl_amd import dict_fact_fast
    return dict_fact_fast


@pytest.fixture
def switches():
    """sets the code solve's debug switches; the defaults are back when the test ends, however it ends"""
    from modl_amd import _lib

    def put(values):
        for name, v in values.items():
            _lib.check(_lib.lib.modl_debug_set(getattr(_lib, 'DEBUG_' + name), int(v)), 'modl_debug_set')
    try:
        yield put
    finally:
        put(SWITCH_DEFAULTS)


def run_gpu(fast, case, misaligned=False):
    """The case through the shim (numpy in, numpy out); a misaligned shared matrix as a device view one element into a buffer."""
    import torch
    code = case.code0.copy()
    sw = np.zeros(case.b, dtype=np.int32)
    f = fast._enet_regression_multi_gram if case.multi else fast._enet_regression_single_gram
    args = (case.idx, case.l1_ratio, case.alpha, case.positive, case.tol, case.max_iter)
    if not misaligned:
        f(case.G.copy(), case.Dx.copy(), case.X, code, *args, sweeps=sw)
        return code, sw
    dev = torch.device('cuda', 0)
    buf = torch.empty(case.k * case.k + 1, dtype=torch.float32 if case.dtn == 'f32' else torch.float64, device=dev)
    G = buf[1:].view(case.k, case.k)
    G.copy_(torch.from_numpy(case.G))
    assert G.data_ptr() % 16 == case.dt().itemsize and G.is_contiguous()
    dcode = torch.from_numpy(code).to(dev)
    f(G, torch.from_numpy(case.Dx).to(dev), torch.from_numpy(case.X).to(dev), dcode, *args, sweeps=sw)
    return dcode.cpu().numpy(), sw


def run_gpu_direct(case):
    """modl_enet_regression_single_gram_* with X in its (b, ldx) buffer"""
    import torch
    from modl_amd._lib import lib, check
    from modl_amd.device import dtype_id, sfx, ptr, stream_ptr
    dev = torch.device('cuda', 0)
    G, Dx, Xb, code, idx = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (case.G, case.Dx, case.Xbuf, case.code0, case.idx))
    assert Xb.stride(0) == case.ldx and Xb.data_ptr() % 16 == 0
    sw = torch.zeros(case.b, dtype=torch.int32, device=dev)
    nbytes = lib.modl_enet_regression_workspace(dtype_id(case.dt), case.b, case.k, 0)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    f = getattr(lib, 'modl_enet_regression_single_gram_' + sfx(case.dt))
    check(f(ptr(G), ptr(Dx), ptr(Xb), case.ldx, case.p, ptr(code), ptr(idx), case.b, case.k, case.l1_ratio, case.alpha, int(case.positive),
            case.tol, case.max_iter, ptr(sw), ptr(ws), nbytes, stream_ptr(dev)), 'modl_enet_regression_single_gram')
    torch.cuda.synchronize()
    return code.cpu().numpy(), sw.cpu().numpy()


def judge_ab(case, got):
    if case.dtn == 'f64':
        judge_a(case, got, run_oracle(case))
    else:
        judge_b(case, got, run_oracle(case), lambda: run_oracle(case, np.float64))


def _report():
    print('figures so far: ' + '; '.join('%s = %.3g' % kv for kv in sorted(FIGURES.items())))


GPU_CASES = [(r.name, dt, scene) for r in ROUTES for dt in r.dts for scene in EVERY_ROUTE + (REPRESENTATIVE if r.extra else ())]


@pytest.mark.gpu
@pytest.mark.parametrize('name,dt,scene', GPU_CASES, ids=['%s-%s-%s' % c for c in GPU_CASES])
def test_route(fast, switches, name, dt, scene):
    route = ROUTE_BY_NAME[name]
    cases = [make_case(dt, route.k, route.b, scene, v, multi=route.multi) for v in VARIANTS[scene]]
    switches(route.sw)
    for case in cases:
        got = run_gpu(fast, case, route.misaligned)
        judge_ab(case, got)
        if scene == 'generic':
            judge_c(case, got, (name,))
        if route.misaligned:             # the aligned call (the four-wavefront solver): f32 agreement rule / 1e-10 with equal sweeps
            aligned = run_gpu(fast, case)
            if dt == 'f64':
                np.testing.assert_array_equal(got[1], aligned[1])
                assert rel_fro(got[0], aligned[0]) < 1e-10
            else:
                same = got[1] == aligned[1]
                assert same.mean() >= 0.9 and rel_fro(got[0][case.idx][same], aligned[0][case.idx][same]) < 2e-5
    _report()


TIGHT_CASES = [(r.name, dt, l1, pos) for r in ROUTES if r.extra for dt in r.dts for l1 in (1.0, 0.5) for pos in (False, True)]


@pytest.mark.gpu
@pytest.mark.parametrize('name,dt,l1,pos', TIGHT_CASES, ids=['%s-%s-l1_%g-%s' % (n, d, l, 'pos' if s else 'any') for n, d, l, s in TIGHT_CASES])
def test_tight(fast, name, dt, l1, pos):
    route = ROUTE_BY_NAME[name]
    for v in VARIANTS['tight']:
        if v['l1_ratio'] == l1 and v['positive'] == pos:
            case = make_case(dt, route.k, route.b, 'tight', v, multi=route.multi)
            got = run_gpu(fast, case)
            judge_ab(case, got)
            judge_c(case, got, (name,))
    _report()


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'f64'])
@pytest.mark.parametrize('p,pad', X_LAYOUT, ids=['p%d-ldx+%d' % c for c in X_LAYOUT])
def test_x_layout(fast, p, pad, dt):
    case = make_x_layout_case(dt, p, pad)
    got = run_gpu_direct(case)
    ref = run_oracle(case)
    assert got[1][LAST_ONLY_ROW] == ref[1][LAST_ONLY_ROW], '|x|^2 of the row whose only non-zero is its last element'
    judge_ab(case, got)
    _report()


@pytest.mark.gpu
@pytest.mark.parametrize('k', [70, 300])
def test_coder_transform_with_a_zero_and_a_duplicated_atom(fast, k):
    """Coder.transform (the plan's own padded Gram, ld_gpad) in f64 against the oracle's transform under judge A (transform
    returns no sweep counts: codes, support and the dead coefficient, which keeps the solver's start value of one)."""
    from modl_amd import Coder
    rs = np.random.RandomState(k)
    n, p = 24, k + 80
    D = rs.randn(k, p)
    D /= np.sqrt((D ** 2).sum(1))[:, None]
    dead, (src, cp) = k // 2, (4, 5)
    D[dead] = 0
    D[cp] = D[src]
    Z = rs.randn(n, k) * (rs.rand(n, k) < 0.1)
    Z[:, src], Z[:, cp] = 1.0, 0.0
    X = Z.dot(D) + 0.1 * rs.randn(n, p)
    for l1 in (1.0, 0.7):
        kw = dict(code_alpha=0.3, code_l1_ratio=l1, tol=1e-3, max_iter=100)
        got = Coder(D, **kw).transform(X)
        ref = _orc.transform(_orc.SomfParams(n_components=k, **kw), D, X)
        err = rel_fro(got, ref)
        _note('A rel_fro / 1e-10', err / 1e-10)
        assert err < 1e-10, err
        bad = support_mismatch(got, ref, (src, cp) if l1 == 1.0 else (), np.abs(X.dot(D.T)).max(1))
        assert len(bad) == 0, [(i, j, got[i, j], ref[i, j]) for i, j in bad[:8]]
        np.testing.assert_array_equal(got[:, dead], ref[:, dead])
        assert np.all(ref[:, dead] == 1) and np.all((ref[:, src] != 0) | (ref[:, cp] != 0))
