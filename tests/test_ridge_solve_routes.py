"""The ridge code solve (l1_ratio = 0: (G + alpha I) code = Dx, csrc/chol.hip) route by route, through
modl_amd.dict_fact_fast._enet_regression_{single,multi}_gram (and modl_enet_regression_* directly to read the device's own Dx
buffer), against a Cholesky solve in np.longdouble written here and against LAPACK posv (the CPU oracle), row by row.

ROUTES (`ROUTES`, checked against `expected_route`, a restatement of the dispatch; the same table is in DESIGN.md, section 19b).
Lines: A = csrc/code_solve.hip (code_route, code_solve), C = csrc/chol.hip, as of this commit.

  A:13 + C:516-518    chol_blocked: k > 512, or a shared matrix with k > 160 or k k sizeof(T) > kCholLdsBytes = 160 KiB - 512
                      (C:31): shared f32 k >= 161, shared f64 k >= 143.  Blocks of kCholNB = 64 columns (C:336), the last of
                      nb = k - 64 (ceil(k / 64) - 1) (C:454)
  A:14 + C:286-288    ridge_small_applies: k <= 128 (C:211) and ((k | 1) k + ((k + 3) & ~3) + 3 (k <= 64 ? 4 : 8) 64) sizeof(T)
                      <= 150 KiB (every k <= 128 in both types).  RPL = 1 for k <= 64, else 2 (C:309); per_wave = 1 for a
                      matrix per sample, else ceil(b / 4) (C:306); NR = min(6, per_wave) (C:310-322); a shared matrix takes
                      ceil(b / (4 NR)) passes of the right-hand-side loop (C:264), a matrix per sample one workgroup each
  A:43-44             cholesky_kernel<LDS> while k k sizeof(T) <= kCholLdsBytes (C:91: f32 k <= 202, f64 k <= 142), else
                      cholesky_kernel<global>; chol_solve_kernel<KPL>, KPL = 4 for 129 <= k <= 256, 8 beyond (C:190-193)

  small, shared, RPL 1      k = 7, b in {1, 2, 4, 5, 8, 9, 12, 13, 16, 17, 20, 21, 24, 25, 49}: NR 1 1 1 2 2 3 3 4 4 5 5 6 6 6 6,
                            25 in two passes, 49 in three; b = 9 at k in {1, 2, 3, 4, 5, 63, 64}
  small, shared, RPL 2      k = 70, the same b; b = 9 at k in {65, 66, 67, 127, 128}
  small, per sample         b = 5, k in {1, 3, 64, 65, 128}; b = 1 at k = 70
  one workgroup, shared     f32 k in {129, 160}, f64 k in {129, 142}; b in {1, 4, 5}
  one workgroup, per sample f32 k in {129, 202, 203, 256, 257, 512}, f64 k in {129, 142, 143, 256, 257, 512}; b = 5 (k = 512: 3)
  blocked, shared           f32 k in {161, 192, 193, 513, 1025}, f64 k in {143, 160, 193, 513}; b in {1, 9, 33} (k >= 513: 9)
  blocked, per sample       k in {513, 577}, b = 2
  misaligned shared G       a view one element into a buffer, k in {70, 160, 193}, b = 9
Routing cannot be observed from outside; `test_workspace_table` pins what can be: the F and Linv terms of
modl_enet_regression_workspace at every point, chol_wide_scratch_elems through them, and the k = 128 / 129 boundary.

SCENES (`make_case`; seeded RandomState; D (k x p) Gaussian, rows normalised; X = (randn * (rand < 0.1)) D + 0.1 randn; G = D D^T
symmetrised and Dx = X D^T in the dtype; idx a permutation into a code array with three extra rows, which hold 7.5; codes
start at ones; p = k + 80; alpha 0.1 unless stated).  Special positions: 0, k-1, k//3, k//3 + 1 and, for k > 64, 63 and 64.
  generic         the control
  rank_def        D of rank max(1, k // 2), alpha 1e-3
  duplicate       atom 5 = atom 4, atom k-1 = atom 0 (k < 7: atom 2 = atom 1), alpha 1e-3
  dead            the atoms at the special positions zeroed: those coefficients come back 0 by value, nothing is NaN
  row_scales      rows of X scaled by 10^U(-6, 6): a whole-batch norm would hide an error in the small rows
  diagonal        G = diag(g), g in 10^U(-3, 3), and G = 0: code = Dx / (g + alpha) element by element (judge E)
  atom_scales     atom j scaled by 10^U(-3, 3): cond ~ 1e7 at a small backward error.  f64 under R and F, f32 under R alone
  zero_row        row min(1, b - 1) of Dx zero: that code row is zero by value, its neighbours follow the judges
  non_finite_row  one row of Dx NaN, then one element +Inf; per-sample routes also a NaN in one sample's matrix.  Only that
                  row of code and Dx is non-finite, every other row has the bits of the same call without the poison
  ignored_arguments  positive = True, tol = 1e9, max_iter = 0 give the bits of the defaults
  alpha_zero      alpha = 0 on a full-rank G (p = 4 k)
Every point runs the first six; the rest run on the representative points (`rep`) of each route.  Systems that are not positive
definite are out of scope (chol.hip's header: NaNs, unreported).

JUDGES, each per row.  c* = `truth`: Cholesky in np.longdouble, one vectorised column step per j (`chol_ld`, `solve_ld`),
which `test_restatement` holds to the oracle's f64 posv on every scene (k cond eps64 per row).
  E  (diagonal, zero G): zeros by value, elsewhere |code - c*| <= 16 eps |c*| per element: one addition, one square root, and per
     substitution direction at most one reciprocal or division and two products - under ten roundings.  The zeros by value
     also hold for the dead coefficients and the zero row; the other coefficients of those scenes are general solves (R and F).
  R  eta_r = |A c_r - q_r|_inf / (|A|_inf |c_r|_inf + |q_r|_inf) in longdouble on the inputs as given <= R_MARGIN eta_oracle,
     R_MARGIN = 8, eta_oracle = ETA_ORACLE eps: the largest eta_r of the oracle's posv in the same dtype over every scene and
     every point of the table, measured by `test_judges_on_the_oracle` of this file (its own run: 1.278 eps in f32, at `duplicate`
     k = 128, and 1.036 eps in f64, at `dead` k = 7 b = 24; no growth with k; ETA_ORACLE = 1.28 and 1.04).  On the blocked routes the bound is multiplied by
     1 + sqrt(cond_2(A)): they apply explicit inverses of the 64 x 64 diagonal blocks of L, conditionally stable with
     cond(L_jj) <= sqrt(cond(A)).
  F  |c_r - c*_r| / |c*_r| <= F_MARGIN max_r'(the oracle's same-dtype error on that case) + 4 eps, F_MARGIN = 8.
  Bookkeeping, every case: rows of code outside idx keep the bits of 7.5; Dx on return has the bits of code[idx]
  (`test_dx_on_the_device` reads the device buffer after a direct ABI call); a second identical call gives identical bits.
`test_judges_on_the_oracle` asserts that the oracle alone stays under 1 / 8 of the R and F bounds on every case they are applied
to, and that the F bound is not vacuous (< 0.05).

MEASURED (this file's own runs; recorded, not asserted, except where a judge above says so).
  Oracle on the CPU, largest over every point, in eps (f32 / f64): eta 1.278 / 1.036 (ETA_ORACLE); forward error generic 14 / 12,
  dead 12 / 11, row_scales 13 / 11, zero_row 11 / 9, alpha_zero 2.9 / 2.8, atom_scales 9e2 / 1.1e3, duplicate 5.4e3 / 1.7e3,
  rank_def 6.5e3 / 6.1e3.
  Device on the MI355X, largest per route:    eta in eps (f32 / f64)   eta / R bound   forward error / oracle's   / F bound   E / 16 eps
    small, shared                             1.00 / 1.20              0.14            3.4                        0.35        0.16
    small, per sample                         0.70 / 0.80              0.10            4.2                        0.53        0.13
    one workgroup, shared                     0.72 / 1.58              0.19            4.2                        0.45        0.12
    one workgroup, per sample                 1.05 / 1.31              0.16            3.5                        0.39        0.11
    blocked, shared                           0.62 / 0.60              0.011           2.0                        0.25        0.15
    blocked, per sample                       0.26 / 0.44              0.008           1.2                        0.13        0.14
    Coder.transform (k = 70, 193)             0.90 / 0.90              0.11            1.9                        0.20
  No route needs more than F_MARGIN = 8 times the oracle's forward error (4.2 at most); the blocked routes stay below one
  eps of backward error, so their sqrt(cond) allowance is not used by these scenes.

MUTANTS (`test_mutants`, on `restated`: the whole call in longdouble numpy).  Mutant -> the scene that rejects it:
  alpha added to every entry of G                           generic (R)
  alpha missing on diagonal element k-1                     dead (position k-1 is dead: a zero pivot, NaN)
  last right-hand side takes its neighbour's solution       row_scales (R; under a batch-wide rel_fro the small row vanishes)
  rows written at r, not idx[r]                             generic (bookkeeping: the rows that hold 7.5)
  backward substitution stops before element 0              generic (R)
  solution not written back to Dx                           generic (bookkeeping)
  sample i uses matrix i-1                                  generic, per sample (R)
  ragged last block read as a full block                    generic at k = 70 in blocks of 64 (a last block of 6).  INVISIBLE where
                                                            the last block is one column (k = 193, 513, 1025: element 0 of the
                                                            inverse is in place under either stride; asserted at k = 65)
  result clipped at zero when `positive` is set             ignored_arguments
  a dead coefficient set to Dx / alpha of its neighbour     dead (zeros by value)
  one step of the four-column pass skipped at k % 4 == 1    generic at k = 5.  INVISIBLE at k = 7 (k % 4 = 3; asserted)
"""
import functools
import zlib
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import somf_oracle as _orc

from .conftest import assert_within_f32_noise, rel_fro
from .test_code_solve_routes import expected_workspace as _enet_workspace, _au

DT = {'f32': np.float32, 'f64': np.float64}
LD = np.longdouble
FILL = 7.5
R_MARGIN = 8.0
F_MARGIN = 8.0
ETA_ORACLE = {'f32': 1.28, 'f64': 1.04}        # in eps; measured by test_judges_on_the_oracle (module docstring, judge R)
E_ULPS = 16
NB = 64                                      # csrc/chol.hip:336
EVERY_ROUTE = ('generic', 'rank_def', 'duplicate', 'dead', 'row_scales', 'diagonal')
REPRESENTATIVE = ('atom_scales', 'zero_row', 'alpha_zero')
VARIANTS = {'diagonal': (0, 1)}
B_LIST = (1, 2, 4, 5, 8, 9, 12, 13, 16, 17, 20, 21, 24, 25, 49)
B_NR_PASSES = {1: (1, 1), 2: (1, 1), 4: (1, 1), 5: (2, 1), 8: (2, 1), 9: (3, 1), 12: (3, 1), 13: (4, 1), 16: (4, 1), 17: (5, 1),
               20: (5, 1), 21: (6, 1), 24: (6, 1), 25: (6, 2), 49: (6, 3), 33: (6, 2)}


# ---------------------------------------------------------------------------------------------------- the dispatch, restated
def chol_lds_bytes():                        # csrc/chol.hip:31
    return 160 * 1024 - 512


def chol_blocked(t, k, shared):              # csrc/chol.hip:516-518
    return k > 512 or (shared and (k > 160 or k * k * t > chol_lds_bytes()))


def ridge_small_lds(t, k):                   # csrc/chol.hip:286
    return ((k | 1) * k + ((k + 3) & ~3) + 3 * (4 if k <= 64 else 8) * 64) * t


def ridge_small_applies(t, k):               # csrc/chol.hip:211, 288
    return k <= 128 and ridge_small_lds(t, k) <= 150 * 1024


def chol_wide_scratch_elems(k):              # csrc/chol.hip:512
    return -(-k // NB) * NB * NB if k > 128 else 0


def expected_route(dt, k, b, multi):
    """The code path of a ridge call (see the module docstring for the lines restated)."""
    t = 4 if dt == 'f32' else 8
    if chol_blocked(t, k, not multi):                                    # A:13
        nblk = -(-k // NB)
        return 'blocked/%s/blocks%d/last%d' % ('per_sample' if multi else 'shared', nblk, k - NB * (nblk - 1))
    if ridge_small_applies(t, k):                                        # A:14
        per_wave = 1 if multi else -(-b // 4)                            # C:306
        nr = min(6, per_wave)                                            # C:310-322
        count = 1 if multi else b                                        # C:229
        return 'small/%s/rpl%d/nr%d/passes%d' % ('per_sample' if multi else 'shared', 1 if k <= 64 else 2, nr, -(-count // (4 * nr)))
    return 'one_wg/%s/%s/kpl%d' % ('per_sample' if multi else 'shared', 'lds' if k * k * t <= chol_lds_bytes() else 'global',
                                   4 if k <= 256 else 8)                 # A:43-44, C:91, C:190-193


def ridge_workspace_terms(dt, b, k, multi):
    """(F elements, Linv elements) of modl_enet_regression_workspace (csrc/code_solve.hip:152-153)"""
    return k * k * (b if multi and k <= 512 else 1), chol_wide_scratch_elems(k)


ROUTES = []


def _route(k, b, want, dts=('f32', 'f64'), multi=False, misaligned=False, rep=False):
    name = '%s-k%d-b%d' % ('misaligned' if misaligned else 'multi' if multi else 'shared', k, b)
    ROUTES.append(SimpleNamespace(name=name, k=k, b=b, multi=multi, misaligned=misaligned, dts=dts, want=want, rep=rep))


for _k, _rpl in ((7, 1), (70, 2)):
    for _b in B_LIST:
        _route(_k, _b, 'small/shared/rpl%d/nr%d/passes%d' % ((_rpl,) + B_NR_PASSES[_b]), rep=_b == 25)
for _k in (1, 2, 3, 4, 5, 63, 64):
    _route(_k, 9, 'small/shared/rpl1/nr3/passes1')
for _k in (65, 66, 67, 127, 128):
    _route(_k, 9, 'small/shared/rpl2/nr3/passes1')
for _k in (1, 3, 64, 65, 128):
    _route(_k, 5, 'small/per_sample/rpl%d/nr1/passes1' % (1 if _k <= 64 else 2), multi=True, rep=_k == 65)
_route(70, 1, 'small/per_sample/rpl2/nr1/passes1', multi=True)
for _b in (1, 4, 5):
    _route(129, _b, 'one_wg/shared/lds/kpl4')
    _route(160, _b, 'one_wg/shared/lds/kpl4', dts=('f32',), rep=_b == 5)
    _route(142, _b, 'one_wg/shared/lds/kpl4', dts=('f64',), rep=_b == 5)
_route(129, 5, 'one_wg/per_sample/lds/kpl4', multi=True, rep=True)
_route(202, 5, 'one_wg/per_sample/lds/kpl4', dts=('f32',), multi=True)
_route(203, 5, 'one_wg/per_sample/global/kpl4', dts=('f32',), multi=True, rep=True)
_route(142, 5, 'one_wg/per_sample/lds/kpl4', dts=('f64',), multi=True)
_route(143, 5, 'one_wg/per_sample/global/kpl4', dts=('f64',), multi=True, rep=True)
_route(256, 5, 'one_wg/per_sample/global/kpl4', multi=True)
_route(257, 5, 'one_wg/per_sample/global/kpl8', multi=True, rep=True)
_route(512, 3, 'one_wg/per_sample/global/kpl8', multi=True)
for _b in (1, 9, 33):
    _route(161, _b, 'blocked/shared/blocks3/last33', dts=('f32',))
    _route(192, _b, 'blocked/shared/blocks3/last64', dts=('f32',))
    _route(143, _b, 'blocked/shared/blocks3/last15', dts=('f64',))
    _route(160, _b, 'blocked/shared/blocks3/last32', dts=('f64',))
    _route(193, _b, 'blocked/shared/blocks4/last1', rep=_b == 9)
_route(513, 9, 'blocked/shared/blocks9/last1')
_route(1025, 9, 'blocked/shared/blocks17/last1', dts=('f32',))
_route(513, 2, 'blocked/per_sample/blocks9/last1', multi=True, rep=True)
_route(577, 2, 'blocked/per_sample/blocks10/last1', multi=True)
_route(70, 9, 'small/shared/rpl2/nr3/passes1', misaligned=True, rep=True)
_route(160, 9, 'one_wg/shared/lds/kpl4', dts=('f32',), misaligned=True)
_route(160, 9, 'blocked/shared/blocks3/last32', dts=('f64',), misaligned=True)
_route(193, 9, 'blocked/shared/blocks4/last1', misaligned=True)
ROUTE_BY_KEY = {(r.name, dt): r for r in ROUTES for dt in r.dts}
POINTS = sorted(ROUTE_BY_KEY)


def is_blocked(route, dt):
    return route.want.startswith('blocked') and expected_route(dt, route.k, route.b, route.multi).startswith('blocked')


# ---------------------------------------------------------------------------------------------------- scenes
def special_positions(k):
    pos = {0, k - 1, k // 3, min(k // 3 + 1, k - 1)}
    if k > 64:
        pos |= {63, 64}
    return sorted(pos)


def duplicate_pairs(k):
    """(original, copy) pairs of the `duplicate` scene (k = 1: none)"""
    pairs = [(4, 5), (0, k - 1)] if k >= 7 else [(1, 2), (0, k - 1)]
    return [(s, c) for s, c in pairs if s < c < k]


def zero_row_of(b):
    return min(1, b - 1)


def _normalised(D):
    return D / np.sqrt((D ** 2).sum(1))[:, None]


@functools.lru_cache(maxsize=2)
def _draws(k, b, p, multi, seed):
    rs = np.random.RandomState(seed)
    Ds = [_normalised(rs.randn(k, p)) for _ in range(b if multi else 1)]
    Z = rs.randn(b, k) * (rs.rand(b, k) < 0.1)
    noise = 0.1 * rs.randn(b, p)
    idx = rs.permutation(b + 3)[:b].astype(np.int64)
    return Ds, Z, noise, idx


def make_case(dt, k, b, scene, variant=0, multi=False):
    """One call's inputs: G (k, k) or (b, k, k), Dx (b, k), X (b, p), code0 (b + 3, k), idx, alpha and what the scene marks."""
    dtn = dt if isinstance(dt, str) else [n for n, d in DT.items() if d == dt][0]
    dt = DT[dtn]
    p = 4 * k if scene == 'alpha_zero' else k + 80
    seed = zlib.crc32(('ridge-%d-%d-%d-%d' % (k, b, p, multi)).encode()) % 100000
    Ds, Z, noise, idx = _draws(k, b, p, bool(multi), seed)
    rs = np.random.RandomState(seed + 7)
    alpha, dead, pairs, zero_row = 0.1, [], [], None
    if scene == 'rank_def':
        r = max(1, k // 2)
        Ds = [_normalised(rs.randn(k, r).dot(rs.randn(r, p))) for _ in Ds]
        alpha = 1e-3
    elif scene == 'duplicate':
        pairs = duplicate_pairs(k)
        Ds = [D.copy() for D in Ds]
        for D in Ds:
            for src, cp in pairs:
                D[cp] = D[src]
        alpha = 1e-3
    elif scene == 'dead':
        dead = special_positions(k)
        Ds = [D.copy() for D in Ds]
        for D in Ds:
            D[dead] = 0
    elif scene == 'atom_scales':
        Ds = [D * (10.0 ** rs.uniform(-3, 3, k))[:, None] for D in Ds]
    elif scene == 'alpha_zero':
        alpha = 0.0
    X = np.stack([Z[i].dot(Ds[i]) for i in range(b)]) + noise if multi else Z.dot(Ds[0]) + noise
    if scene == 'row_scales':
        X = X * (10.0 ** rs.uniform(-6, 6, b))[:, None]
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
    if scene == 'diagonal':
        G = np.zeros_like(G)
        if variant == 0:
            for g in (G if multi else [G]):
                g.flat[::k + 1] = (10.0 ** rs.uniform(-3, 3, k)).astype(dt)
    if scene == 'zero_row':
        zero_row = zero_row_of(b)
        X[zero_row] = 0
        Dx[zero_row] = 0
    assert G.dtype == dt and Dx.dtype == dt
    code0 = np.full((b + 3, k), FILL, dtype=dt)
    code0[idx] = 1
    return SimpleNamespace(dt=dt, dtn=dtn, k=k, b=b, p=p, multi=bool(multi), scene=scene, variant=variant, G=G, Dx=Dx, X=X, idx=idx,
                           code0=code0, alpha=alpha, dead=dead, pairs=pairs, zero_row=zero_row, positive=False, tol=1e-2, max_iter=100)


def cases_of(route, dt, scenes):
    for scene in scenes:
        for v in VARIANTS.get(scene, (0,)):
            yield make_case(dt, route.k, route.b, scene, v, multi=route.multi)


# ---------------------------------------------------------------------------------------------------- the truth in longdouble
def chol_ld(A, mut=()):
    """Lower Cholesky factor of A in longdouble, left-looking, one vectorised column step per j."""
    A = np.asarray(A, dtype=LD)
    k = A.shape[0]
    L = np.zeros((k, k), dtype=LD)
    with np.errstate(invalid='ignore', divide='ignore'):
        for j in range(k):
            if 'skip_pass_k4_1' in mut and k % 4 == 1 and j == k - 1:
                L[j, j] = A[j, j]
                continue
            v = A[j:, j] - L[j:, :j].dot(L[j, :j])
            d = np.sqrt(v[0])
            L[j, j] = d
            L[j + 1:, j] = v[1:] / d
    return L


def solve_ld(L, Q, mut=()):
    """L L^T x = q for the rows q of Q (b, k): returns (b, k) in longdouble."""
    k = L.shape[0]
    Y = np.array(Q, dtype=LD).T.copy()
    with np.errstate(invalid='ignore', divide='ignore'):
        for j in range(k):
            Y[j] = (Y[j] - L[j, :j].dot(Y[:j])) / L[j, j]
        for j in range(k - 1, 0 if 'backward_stops_at_1' in mut else -1, -1):
            Y[j] = (Y[j] - L[j + 1:, j].dot(Y[j + 1:])) / L[j, j]
    return Y.T.copy()


def tri_inv_ld(L):
    n = L.shape[0]
    X = np.zeros((n, n), dtype=LD)
    for i in range(n):
        e = np.zeros(n, dtype=LD)
        e[i] = 1
        X[i] = (e - L[i, :i].dot(X[:i])) / L[i, i]
    return X


def blocked_solve_ld(L, Q, nb_full=NB, mut=()):
    """The substitutions as the blocked route orders them (csrc/chol.hip:477-510): the diagonal blocks applied through their
    explicit inverses.  `ragged_as_full`: the last block's inverse, stored with a row stride of nb, read with a stride of 64."""
    k = L.shape[0]
    Y = np.array(Q, dtype=LD).T.copy()
    blocks = []
    for j0 in range(0, k, nb_full):
        nb = min(nb_full, k - j0)
        Li = tri_inv_ld(L[j0:j0 + nb, j0:j0 + nb])
        if 'ragged_as_full' in mut and nb < nb_full and j0 + nb == k:
            buf = np.zeros(nb_full * nb_full, dtype=LD)
            buf[:nb * nb] = Li.ravel()
            Li = buf.reshape(nb_full, nb_full)[:nb, :nb].copy()
        blocks.append((j0, nb, Li))
    for j0, nb, Li in blocks:
        Y[j0:j0 + nb] = Li.dot(Y[j0:j0 + nb])
        Y[j0 + nb:] -= L[j0 + nb:, j0:j0 + nb].dot(Y[j0:j0 + nb])
    for j0, nb, Li in reversed(blocks):
        Y[j0:j0 + nb] = Li.T.dot(Y[j0:j0 + nb])
        Y[:j0] -= L[j0:j0 + nb, :j0].T.dot(Y[j0:j0 + nb])
    return Y.T.copy()


def system_of(G, alpha, dt):
    """G + alpha I with alpha as the dtype holds it (the inputs as given), in longdouble"""
    A = np.array(G, dtype=LD)
    A.flat[::A.shape[0] + 1] += LD(dt(alpha))
    return A


_FACTORS = {}


def _factor(G, alpha, dt):
    """(A, L, cond_2(A)) cached on the bytes of G: several scenes share a matrix"""
    key = (zlib.crc32(G.tobytes()), G.shape, str(G.dtype), alpha)
    if key not in _FACTORS:
        if len(_FACTORS) > 6:
            _FACTORS.clear()
        A = system_of(G, alpha, dt)
        ev = np.linalg.eigvalsh(A.astype(np.float64))
        _FACTORS[key] = (A, chol_ld(A), float(ev[-1] / ev[0]) if ev[0] > 0 else np.inf)
    return _FACTORS[key]


def truth(case):
    """(c* (b, k) longdouble, per-sample cond_2(A))"""
    if not case.multi:
        A, L, cond = _factor(case.G, case.alpha, case.dt)
        return solve_ld(L, case.Dx), np.full(case.b, cond)
    out, conds = [], []
    for i in range(case.b):
        A, L, cond = _factor(case.G[i], case.alpha, case.dt)
        out.append(solve_ld(L, case.Dx[i:i + 1])[0])
        conds.append(cond)
    return np.stack(out), np.array(conds)


def eta_of(case, sol):
    """Judge R's normwise backward error per row, in longdouble on the inputs as given."""
    c, q = np.asarray(sol, dtype=LD), np.asarray(case.Dx, dtype=LD)
    out = np.zeros(case.b)
    with np.errstate(invalid='ignore', over='ignore'):
        for i in range(case.b if case.multi else 1):
            A = system_of(case.G[i] if case.multi else case.G, case.alpha, case.dt)
            rows = slice(i, i + 1) if case.multi else slice(None)
            num = np.abs(c[rows].dot(A) - q[rows]).max(1)            # (A is symmetric)
            den = np.abs(A).sum(1).max() * np.abs(c[rows]).max(1) + np.abs(q[rows]).max(1)
            out[rows] = np.where(num == 0, LD(0), num / np.where(den == 0, LD(1), den)).astype(np.float64)
    return out


def forward_error(sol, cstar):
    """|c_r - c*_r| / |c*_r| per row (rows with c* = 0: 0 if c = 0, else inf)"""
    d = np.sqrt(((np.asarray(sol, dtype=LD) - cstar) ** 2).sum(1))
    n = np.sqrt((cstar ** 2).sum(1))
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.where(n == 0, np.where(d == 0, 0.0, np.inf), d / np.where(n == 0, LD(1), n)).astype(np.float64)


def run_oracle(case, dt=None):
    """code (b + 3, k) of the CPU oracle (LAPACK posv), on the case's arrays as type dt"""
    dt = case.dt if dt is None else dt
    code = case.code0.astype(dt)
    f = _orc.enet_regression_multi_gram if case.multi else _orc.enet_regression_single_gram
    f(case.G.astype(dt), case.Dx.astype(dt), case.X.astype(dt), code, case.idx, 0.0, case.alpha, False, 1e-2, 100)
    return code


def restated(case, mut=()):
    """The whole call in longdouble numpy, with the hooks of the mutants: (code, Dx on return), as float64."""
    k, b = case.k, case.b
    sol = np.zeros((b, k), dtype=LD)
    for i in range(b if case.multi else 1):
        src = (i - 1) % b if 'previous_matrix' in mut else i
        G = case.G[src] if case.multi else case.G
        A = system_of(G, case.alpha, case.dt)
        if 'alpha_everywhere' in mut:
            A = np.array(G, dtype=LD) + LD(case.dt(case.alpha))
        if 'alpha_missing_last' in mut:
            A[k - 1, k - 1] -= LD(case.dt(case.alpha))
        L = chol_ld(A, mut)
        rows = slice(i, i + 1) if case.multi else slice(None)
        sol[rows] = blocked_solve_ld(L, case.Dx[rows], mut=mut) if ('blocked' in mut or 'ragged_as_full' in mut) else \
            solve_ld(L, case.Dx[rows], mut)
    if 'last_takes_neighbour' in mut and b > 1:
        sol[b - 1] = sol[b - 2]
    if 'positive_clips' in mut and case.positive:
        sol = np.maximum(sol, 0)
    if 'dead_takes_neighbour' in mut:
        for j in case.dead:
            if j + 1 < k:
                sol[:, j] = np.asarray(case.Dx[:, j + 1], dtype=LD) / LD(case.alpha)
    sol = sol.astype(np.float64)
    code = case.code0.astype(np.float64)
    code[np.arange(b) if 'rows_at_r' in mut else case.idx] = sol
    return code, (case.Dx.astype(np.float64) if 'no_writeback' in mut else sol)


# ---------------------------------------------------------------------------------------------------- the judges
FIGURES = {}                     # figure -> the largest value seen (printed and recorded, not asserted)


def _note(what, value):
    if np.isfinite(value):
        FIGURES[what] = max(FIGURES.get(what, 0.0), float(value))


def _report():
    print('figures so far: ' + '; '.join('%s = %.3g' % kv for kv in sorted(FIGURES.items())))


def bookkeeping(case, got):
    code, dx = got
    outside = np.setdiff1d(np.arange(case.b + 3), case.idx)
    assert code[outside].tobytes() == case.code0[outside].tobytes(), 'rows of the code array outside idx were written'
    assert np.asarray(dx).tobytes() == np.ascontiguousarray(code[case.idx]).tobytes(), 'Dx on return is not code[idx], bit for bit'


def zeros_by_value(case, sol):
    if case.dead:
        assert np.all(sol[:, case.dead] == 0), ('a dead coefficient is not zero', sol[:, case.dead])
    if case.zero_row is not None:
        assert np.all(sol[case.zero_row] == 0), ('the zero row of Dx gave a non-zero code', sol[case.zero_row])


def judge_e(case, sol, who='E'):
    eps = np.finfo(case.dt).eps
    q = np.asarray(case.Dx, dtype=LD)
    diag = np.stack([np.diag(g) for g in case.G]) if case.multi else np.diag(case.G)[None, :]
    cstar = q / (np.asarray(diag, dtype=LD) + LD(case.dt(case.alpha)))
    s = np.asarray(sol, dtype=LD)
    assert np.all(s[cstar == 0] == 0), 'a zero of the exact solution is not zero'
    with np.errstate(invalid='ignore', divide='ignore'):
        err = np.where(cstar == 0, LD(0), np.abs(s - cstar) / np.abs(cstar)).astype(np.float64) / eps
    _note('%s ulps / %d' % (who, E_ULPS), np.nanmax(err) / E_ULPS)
    assert np.all(err <= E_ULPS), ('element-wise error in eps', np.nanmax(err), np.argwhere(~(err <= E_ULPS))[:4])


def r_bound(case, conds, blocked):
    bound = R_MARGIN * ETA_ORACLE[case.dtn] * np.finfo(case.dt).eps
    return bound * (1 + np.sqrt(conds)) if blocked else np.full(case.b, bound)


def judge_r(case, sol, conds, blocked, who='R'):
    eta = eta_of(case, sol)
    bound = r_bound(case, conds, blocked)
    _note('%s eta / bound' % who, (eta / bound).max())
    _note('%s eta / eps %s' % (who, case.dtn), eta.max() / np.finfo(case.dt).eps)
    assert np.all(eta <= bound), ('backward error over its bound, per row', case.scene, (eta / bound).round(3))
    return eta


def f_bound(case, cstar, oracle_sol):
    return F_MARGIN * forward_error(oracle_sol, cstar).max() + 4 * np.finfo(case.dt).eps


def judge_f(case, sol, cstar, oracle_sol, who='F'):
    err = forward_error(sol, cstar)
    oerr = forward_error(oracle_sol, cstar).max()
    bound = f_bound(case, cstar, oracle_sol)
    _note('%s error / bound' % who, err.max() / bound)
    if oerr > 0:
        _note('%s error / oracle error' % who, err.max() / oerr)
    assert np.all(err <= bound), ('forward error over its bound, per row', case.scene, (err / bound).round(3), oerr)


def f_applies(case):
    return not (case.scene == 'atom_scales' and case.dtn == 'f32')


def judge(case, got, blocked, who=''):
    """Everything that holds for one finished call: bookkeeping, zeros by value, E or R (+ F)."""
    bookkeeping(case, got)
    sol = got[0][case.idx]
    assert np.all(np.isfinite(sol)), ('non-finite codes', case.scene, np.argwhere(~np.isfinite(sol))[:4])
    zeros_by_value(case, sol)
    if case.scene == 'diagonal':
        judge_e(case, sol, who + 'E')
        return
    cstar, conds = truth(case)
    judge_r(case, sol, conds, blocked, who + 'R')
    if f_applies(case):
        judge_f(case, sol, cstar, run_oracle(case)[case.idx], who + 'F')


def accepts(*args, **kw):
    kept = dict(FIGURES)             # (a mutant's figures are not the kernels')
    try:
        judge(*args, **kw)
    except AssertionError:
        return False
    finally:
        FIGURES.clear()
        FIGURES.update(kept)
    return True


# ---------------------------------------------------------------------------------------------------- CPU tests
CPU_POINTS = [(5, 9, False), (70, 9, False), (65, 5, True), (193, 4, False)]
ALL_SCENES = EVERY_ROUTE + REPRESENTATIVE


def _cpu_cases(dt, k, b, multi):
    route = SimpleNamespace(k=k, b=b, multi=multi)
    return cases_of(route, dt, ALL_SCENES)


@pytest.mark.parametrize('k,b,multi', CPU_POINTS)
def test_restatement(k, b, multi):
    """`chol_ld` + `solve_ld` (and the blocked ordering of the substitutions) against the oracle's f64 posv on every scene:
    k cond eps per row, the forward error a backward-stable solve may show."""
    eps = np.finfo(np.float64).eps
    for case in _cpu_cases('f64', k, b, multi):
        cstar, conds = truth(case)
        ref = run_oracle(case)[case.idx]
        err = forward_error(ref, cstar)
        assert np.all(err <= k * conds * eps), (case.scene, err, conds)
        code, dx = restated(case)
        np.testing.assert_array_equal(code[case.idx], cstar.astype(np.float64))
        bookkeeping(case, (code.astype(case.dt), dx.astype(case.dt)))
        blocked = restated(case, ('blocked',))[0][case.idx]
        assert np.all(forward_error(blocked, cstar) <= k * conds * eps), case.scene


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_scenes_are_what_they_claim(dt):
    k, b = 70, 9
    eps = np.finfo(DT[dt]).eps
    mk = lambda scene, v=0, multi=False, k=k: make_case(dt, k, b, scene, v, multi=multi)   # noqa: E731
    cond = lambda c: truth(c)[1].max()                                                         # noqa: E731
    rank = lambda G: int((np.linalg.eigvalsh(G.astype(np.float64)) > 1e-4).sum())             # noqa: E731
    case = mk('generic')
    assert 5 < cond(case) < 60 and rank(case.G) == k and case.alpha == 0.1
    assert len(set(case.idx.tolist())) == b and case.code0.shape == (b + 3, k) and np.all(case.code0[case.idx] == 1)
    assert np.all(case.code0[np.setdiff1d(np.arange(b + 3), case.idx)] == FILL)
    assert np.array_equal(case.G, case.G.T)
    case = mk('rank_def')
    assert rank(case.G) == k // 2 and case.alpha == 1e-3 and 1e3 < cond(case) < 1e5
    case = mk('duplicate')
    assert case.pairs == [(4, 5), (0, k - 1)] and rank(case.G) == k - 2
    for src, cp in case.pairs:
        np.testing.assert_allclose(case.G[src], case.G[cp], rtol=0, atol=8 * eps)
    assert duplicate_pairs(5) == [(1, 2), (0, 4)] and duplicate_pairs(1) == [] and duplicate_pairs(2) == [(0, 1)]
    case = mk('dead')
    assert case.dead == [0, 23, 24, 63, 64, 69] and special_positions(200) == [0, 63, 64, 66, 67, 199]
    assert not case.G[case.dead].any() and not case.G[:, case.dead].any() and not case.Dx[:, case.dead].any()
    assert np.all(truth(case)[0][:, case.dead] == 0)
    assert special_positions(1) == [0] and special_positions(3) == [0, 1, 2]
    case = mk('row_scales')
    norms = np.sqrt((case.Dx.astype(np.float64) ** 2).sum(1))
    assert norms.max() / norms.min() > 1e6                 # (a batch-wide norm sees the largest row alone)
    case = mk('diagonal')
    g = np.diag(case.G)
    assert np.array_equal(case.G, np.diag(g)) and g.max() / g.min() > 1e4 and g.min() > 0
    assert not mk('diagonal', 1).G.any()
    case = mk('diagonal', 0, multi=True, k=65)
    assert case.G.shape == (b, 65, 65) and not np.array_equal(case.G[0], case.G[1])
    case = mk('atom_scales')
    assert cond(case) > 1e6
    case = mk('zero_row')
    assert case.zero_row == 1 and not case.Dx[1].any() and case.Dx[0].any() and case.Dx[2].any()
    assert not truth(case)[0][1].any() and zero_row_of(1) == 0
    case = mk('alpha_zero')
    assert case.alpha == 0 and case.p == 4 * k and cond(case) < 60
    case = mk('generic', multi=True, k=65)
    assert case.G.shape == (b, 65, 65) and not np.array_equal(case.G[0], case.G[1])


def test_route_table():
    """ROUTES names what the dispatch does at every point, and every path of the issue's table is there."""
    for (name, dt), r in ROUTE_BY_KEY.items():
        assert expected_route(dt, r.k, r.b, r.multi) == r.want, (name, dt, expected_route(dt, r.k, r.b, r.multi))
    wants = set(r.want for r in ROUTES)
    for rpl in (1, 2):
        for nr, passes in set(B_NR_PASSES.values()):
            assert 'small/shared/rpl%d/nr%d/passes%d' % (rpl, nr, passes) in wants
        assert 'small/per_sample/rpl%d/nr1/passes1' % rpl in wants
    assert {'one_wg/shared/lds/kpl4', 'one_wg/per_sample/lds/kpl4', 'one_wg/per_sample/global/kpl4', 'one_wg/per_sample/global/kpl8',
            'blocked/shared/blocks3/last64', 'blocked/shared/blocks4/last1', 'blocked/per_sample/blocks9/last1'} <= wants
    # the boundaries, on either side
    assert [ridge_small_applies(t, k) for t in (4, 8) for k in (128, 129)] == [True, False, True, False]
    assert ridge_small_lds(8, 128) == 145408 and ridge_small_lds(4, 70) == 26312 and ridge_small_lds(4, 7) == 3300
    assert [chol_blocked(4, k, True) for k in (160, 161)] == [False, True]
    assert [chol_blocked(8, k, True) for k in (142, 143)] == [False, True]
    assert [chol_blocked(t, k, False) for t in (4, 8) for k in (512, 513)] == [False, True, False, True]
    assert expected_route('f32', 202, 5, True).split('/')[2] == 'lds' and expected_route('f32', 203, 5, True).split('/')[2] == 'global'
    assert expected_route('f64', 142, 5, True).split('/')[2] == 'lds' and expected_route('f64', 143, 5, True).split('/')[2] == 'global'
    assert expected_route('f64', 256, 5, True).endswith('kpl4') and expected_route('f64', 257, 5, True).endswith('kpl8')
    # the left-looking pass of four columns: every tail length among the small points
    assert {r.k % 4 for r in ROUTES if r.want.startswith('small/shared')} == {0, 1, 2, 3}
    # one representative per route family and dtype
    for fam in ('small/shared/rpl1', 'small/shared/rpl2', 'small/per_sample', 'one_wg/shared', 'one_wg/per_sample/lds',
                'one_wg/per_sample/global/kpl4', 'one_wg/per_sample/global/kpl8', 'blocked/shared', 'blocked/per_sample'):
        for dt in ('f32', 'f64'):
            assert any(r.rep and dt in r.dts and r.want.startswith(fam) for r in ROUTES), (fam, dt)
    assert len(ROUTE_BY_KEY) == sum(len(r.dts) for r in ROUTES)


def test_workspace_table():
    """modl_enet_regression_workspace: the F term (k k, times b for a matrix per sample up to k = 512) and the Linv term
    (chol_wide_scratch_elems) at every point of the table; the elastic-net file's restatement supplies the other terms."""
    from modl_amd._lib import lib
    for (name, dt), r in ROUTE_BY_KEY.items():
        t = 4 if dt == 'f32' else 8
        got = lib.modl_enet_regression_workspace(0 if dt == 'f32' else 1, r.b, r.k, int(r.multi))
        total, copy, slots = _enet_workspace(dt, r.b, r.k, r.multi)
        F, Linv = ridge_workspace_terms(dt, r.b, r.k, r.multi)
        assert got == total, (name, dt, got, total)
        assert got - copy - slots - _au(t * r.b) - _au(t * r.b * r.k) == _au(t * (F + Linv)), (name, dt)
    assert chol_wide_scratch_elems(128) == 0 and chol_wide_scratch_elems(129) == 3 * 4096 and chol_wide_scratch_elems(192) == 3 * 4096
    assert chol_wide_scratch_elems(193) == 4 * 4096 and chol_wide_scratch_elems(1025) == 17 * 4096
    base = lambda k: lib.modl_enet_regression_workspace(1, 9, k, 0) - sum(_enet_workspace('f64', 9, k, False)[1:])   # noqa: E731
    assert base(128) == _au(72) + _au(72 * 128) + _au(8 * 128 * 128)
    assert base(129) == _au(72) + _au(72 * 129) + _au(8 * (129 * 129 + 3 * 4096))
    assert ridge_workspace_terms('f64', 3, 512, True)[0] == 3 * 512 * 512 and ridge_workspace_terms('f64', 2, 513, True)[0] == 513 * 513


MUTANTS = {
    'alpha_everywhere': ('generic', 70, False), 'alpha_missing_last': ('dead', 70, False), 'last_takes_neighbour': ('row_scales', 70, False),
    'rows_at_r': ('generic', 70, False), 'backward_stops_at_1': ('generic', 70, False), 'no_writeback': ('generic', 70, False),
    'previous_matrix': ('generic', 65, True), 'ragged_as_full': ('generic', 70, False), 'positive_clips': ('ignored_arguments', 70, False),
    'dead_takes_neighbour': ('dead', 70, False), 'skip_pass_k4_1': ('generic', 5, False),
}
INVISIBLE = {'ragged_as_full': ('generic', 65, False), 'skip_pass_k4_1': ('generic', 7, False)}


def _mutant_case(scene, k, multi, b=9):
    if scene == 'ignored_arguments':
        case = make_case('f64', k, b, 'generic', multi=multi)
        case.positive, case.tol, case.max_iter = True, 1e9, 0
        return case
    return make_case('f64', k, b, scene, multi=multi)


def _judge_restated(case, got):
    got = (got[0].astype(case.dt), got[1].astype(case.dt))
    if case.positive:                                  # ignored_arguments: the bits of the defaults
        plain = restated(case)
        assert got[0].tobytes() == plain[0].astype(case.dt).tobytes()
    judge(case, got, blocked=False)


def test_mutants():
    """Every mutant of the call is rejected by its named scene; where a mutant cannot show, that is asserted too."""
    def rejected(mut, scene, k, multi):
        case = _mutant_case(scene, k, multi)
        _judge_restated(case, restated(case))                        # (the unmutated restatement passes)
        try:
            kept = dict(FIGURES)
            _judge_restated(case, restated(case, (mut,)))
        except AssertionError:
            return True
        finally:
            FIGURES.clear()
            FIGURES.update(kept)
        return False
    for mut, where in MUTANTS.items():
        assert rejected(mut, *where), '%s survives %s' % (mut, where)
    for mut, where in INVISIBLE.items():
        assert not rejected(mut, *where), '%s shows at %s' % (mut, where)
    # a batch-wide norm does not see the row that took its neighbour's solution when that row is small
    case = make_case('f64', 70, 9, 'row_scales')
    big = np.abs(case.Dx).max()
    for r in (7, 8):                                                   # (the last row and its neighbour small)
        case.Dx[r] *= 1e-10 * big / np.abs(case.Dx[r]).max()
    good, bad = restated(case), restated(case, ('last_takes_neighbour',))
    assert rel_fro(bad[0][case.idx], good[0][case.idx]) < 1e-9
    assert accepts(case, tuple(a.astype(case.dt) for a in good), False) and not accepts(case, tuple(a.astype(case.dt) for a in bad), False)


@pytest.mark.parametrize('name,dt', POINTS, ids=['%s-%s' % c for c in POINTS])
def test_judges_on_the_oracle(name, dt):
    """The oracle's posv alone, on every case of this point: eta below ETA_ORACLE eps (R_MARGIN times that is judge R's
    bound, so the reference uses at most 1 / 8 of it), its forward error at most 1 / 8 of judge F's bound, and that bound
    not vacuous.  Prints the figures the module docstring records."""
    route = ROUTE_BY_KEY[name, dt]
    eps = np.finfo(DT[dt]).eps
    blocked = is_blocked(route, dt)
    worst = {}
    for case in cases_of(route, dt, ALL_SCENES if route.rep else EVERY_ROUTE):
        sol = run_oracle(case)[case.idx]
        assert np.all(np.isfinite(sol)), case.scene
        eta = eta_of(case, sol)
        assert np.all(eta <= ETA_ORACLE[dt] * eps), (case.scene, eta / eps)
        if case.scene == 'diagonal':
            judge_e(case, sol, 'oracle E')
            continue
        cstar, conds = truth(case)
        assert np.all(eta <= r_bound(case, conds, blocked) / 8)
        worst[case.scene] = (eta.max() / eps, forward_error(sol, cstar).max() / eps)
        if f_applies(case):
            bound = f_bound(case, cstar, sol)
            assert np.all(forward_error(sol, cstar) <= bound / 8) and bound < 0.05, (case.scene, bound)
    print('%s %s oracle (eta, forward error) in eps: %s' % (name, dt, '; '.join('%s %.2f %.3g' % ((s,) + v) for s, v in worst.items())))


def test_refusals_before_any_device_work():
    """Bad arguments of a ridge call are answered before anything touches a device (the pointers are never dereferenced)."""
    import ctypes as C
    from modl_amd._lib import lib
    EINVAL, ENOMEM, OK = -1, -2, 0
    fake = C.c_void_p(4096)
    kmax = lib.modl_max_components()
    for sfx, multi in (('f32', 0), ('f64', 0), ('f32', 1), ('f64', 1)):
        f = getattr(lib, 'modl_enet_regression_%s_gram_%s' % ('multi' if multi else 'single', sfx))

        def call(b=4, k=70, p=10, ldx=10, ws=0, G=fake, Dx=fake, code=fake):
            need = lib.modl_enet_regression_workspace(0 if sfx == 'f32' else 1, b, k, multi)
            return f(G, Dx, fake, ldx, p, code, fake, b, k, 0.0, 0.1, 0, 1e-2, 10, None, fake, need + ws, None)
        assert call(k=0) == EINVAL and call(k=kmax + 1) == EINVAL and call(ldx=9) == EINVAL and call(b=-1) == EINVAL
        assert call(G=None) == EINVAL and call(Dx=None) == EINVAL and call(code=None) == EINVAL
        for k in (70, 150, 193, 600):
            assert call(k=k, ws=-1) == ENOMEM
        assert call(b=0) == OK


# ---------------------------------------------------------------------------------------------------- GPU tests
@pytest.fixture(scope='module')
def fast():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    from modl_amd import dict_fact_fast
    return dict_fact_fast


def run_gpu(fast, case, misaligned=False):
    """The case through the shim: (code (b + 3, k), Dx on return).  A misaligned shared matrix is a device view one element
    into a buffer."""
    import torch
    f = fast._enet_regression_multi_gram if case.multi else fast._enet_regression_single_gram
    args = (case.idx, 0.0, case.alpha, case.positive, case.tol, case.max_iter)
    if not misaligned:
        code, dx = case.code0.copy(), case.Dx.copy()
        f(case.G.copy(), dx, case.X, code, *args)
        return code, dx
    dev = torch.device('cuda', 0)
    buf = torch.empty(case.k * case.k + 1, dtype=torch.float32 if case.dtn == 'f32' else torch.float64, device=dev)
    G = buf[1:].view(case.k, case.k)
    G.copy_(torch.from_numpy(case.G))
    assert G.data_ptr() % 16 == case.dt().itemsize and G.is_contiguous()
    dcode, ddx = torch.from_numpy(case.code0.copy()).to(dev), torch.from_numpy(case.Dx.copy()).to(dev)
    f(G, ddx, torch.from_numpy(case.X).to(dev), dcode, *args)
    return dcode.cpu().numpy(), ddx.cpu().numpy()


def run_gpu_direct(case):
    """modl_enet_regression_*_gram_* on device buffers of this test's own: (code, Dx) as the device holds them afterwards."""
    import torch
    from modl_amd._lib import lib, check
    from modl_amd.device import dtype_id, sfx, ptr, stream_ptr
    dev = torch.device('cuda', 0)
    G, Dx, X, code, idx = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (case.G, case.Dx, case.X, case.code0, case.idx))
    nbytes = lib.modl_enet_regression_workspace(dtype_id(case.dt), case.b, case.k, int(case.multi))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    f = getattr(lib, 'modl_enet_regression_%s_gram_%s' % ('multi' if case.multi else 'single', sfx(case.dt)))
    check(f(ptr(G), ptr(Dx), ptr(X), case.p, case.p, ptr(code), ptr(idx), case.b, case.k, 0.0, case.alpha, 0, 1e-2, 100, None,
            ptr(ws), nbytes, stream_ptr(dev)), 'modl_enet_regression')
    torch.cuda.synchronize()
    return code.cpu().numpy(), Dx.cpu().numpy()


def same_bits(a, b):
    return all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


def family(route):
    return '/'.join(route.want.split('/')[:2]) + ' '


@pytest.mark.gpu
@pytest.mark.parametrize('name,dt', POINTS, ids=['%s-%s' % c for c in POINTS])
def test_route(fast, name, dt):
    route = ROUTE_BY_KEY[name, dt]
    for case in cases_of(route, dt, EVERY_ROUTE):
        got = run_gpu(fast, case, route.misaligned)
        judge(case, got, is_blocked(route, dt), family(route))
        assert same_bits(got, run_gpu(fast, case, route.misaligned)), ('a second identical call gave other bits', case.scene)
    _report()


REPS = [(n, dt) for (n, dt) in POINTS if ROUTE_BY_KEY[n, dt].rep]


@pytest.mark.gpu
@pytest.mark.parametrize('name,dt', REPS, ids=['%s-%s' % c for c in REPS])
def test_representative_scenes(fast, name, dt):
    """atom_scales, zero_row, alpha_zero, ignored_arguments and non_finite_row on one point per route."""
    route = ROUTE_BY_KEY[name, dt]
    blocked = is_blocked(route, dt)
    for case in cases_of(route, dt, REPRESENTATIVE):
        got = run_gpu(fast, case, route.misaligned)
        judge(case, got, blocked, family(route))
        assert same_bits(got, run_gpu(fast, case, route.misaligned)), case.scene
    case = make_case(dt, route.k, route.b, 'generic', multi=route.multi)
    clean = run_gpu(fast, case, route.misaligned)
    # ignored_arguments
    case.positive, case.tol, case.max_iter = True, 1e9, 0
    assert same_bits(clean, run_gpu(fast, case, route.misaligned)), 'positive / tol / max_iter changed a ridge solve'
    case.positive, case.tol, case.max_iter = False, 1e-2, 100
    # non_finite_row
    r = min(2, case.b - 1)
    others = np.delete(np.arange(case.b), r)
    for what in ('nan_row', 'inf_element') + (('nan_in_matrix',) if route.multi else ()):
        bad = SimpleNamespace(**vars(case))
        bad.Dx, bad.G = case.Dx.copy(), case.G
        if what == 'nan_row':
            bad.Dx[r] = np.nan
        elif what == 'inf_element':
            bad.Dx[r, case.k // 2] = np.inf
        else:
            bad.G = case.G.copy()
            bad.G[r, min(1, case.k - 1), 0] = bad.G[r, 0, min(1, case.k - 1)] = np.nan
        code, dx = run_gpu(fast, bad, route.misaligned)
        bookkeeping_rows = np.setdiff1d(np.arange(case.b + 3), case.idx[r:r + 1])
        assert code[bookkeeping_rows].tobytes() == clean[0][bookkeeping_rows].tobytes(), (what, 'a non-finite value left its row')
        assert dx[others].tobytes() == clean[1][others].tobytes(), (what, 'a non-finite value left its row of Dx')
        assert not np.all(np.isfinite(code[case.idx[r]])), (what, 'the poisoned row came back finite')
        assert dx[r].tobytes() == code[case.idx[r]].tobytes() or (np.isnan(dx[r]) == np.isnan(code[case.idx[r]])).all()
    _report()


ALIGNED_REPS = [c for c in REPS if not ROUTE_BY_KEY[c].misaligned]     # (the misaligned view is a layout of the shim's caller)


@pytest.mark.gpu
@pytest.mark.parametrize('name,dt', ALIGNED_REPS, ids=['%s-%s' % c for c in ALIGNED_REPS])
def test_dx_on_the_device(name, dt):
    """A direct ABI call on buffers of the test's own: the device's Dx holds code[idx] bit for bit, rows outside idx keep 7.5,
    and the codes are those of the shim."""
    route = ROUTE_BY_KEY[name, dt]
    case = make_case(dt, route.k, route.b, 'generic', multi=route.multi)
    got = run_gpu_direct(case)
    judge(case, got, is_blocked(route, dt), family(route))


# ---------------------------------------------------------------------------------------------------- through the plan
@pytest.fixture(scope='module')
def DictFact():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    from modl_amd import DictFact
    return DictFact


PLAN_KW = dict(G_agg='average', Dx_agg='average', code_l1_ratio=0, comp_l1_ratio=1, code_alpha=1e-2)


@pytest.mark.gpu
@pytest.mark.parametrize('dt', [np.float64, np.float32], ids=['f64', 'f32'])
@pytest.mark.parametrize('k', [70, 150])
def test_partial_fit_average_gram_with_ridge_codes(DictFact, oracle, k, dt):
    """G_agg = Dx_agg = 'average' with ridge codes: a minibatch's samples index rows of G_average_ (g_idx): ridge_small_kernel at
    k = 70, cholesky_kernel + chol_solve_kernel at k = 150.  n = k rows (the estimator wants as many rows as atoms) in three
    minibatches, the last one ragged: 30, 30, 10 at k = 70 and 64, 64, 22 at k = 150."""
    from .test_gpu_step import _make_pair
    n, b = (70, 30) if k == 70 else (150, 64)
    assert n % b and -(-n // b) == 3
    est, pr, st, X = _make_pair(DictFact, oracle, dt, n=n, p=k + 60, k=k, b=b, r=2, **PLAN_KW)
    est.partial_fit(X)
    oracle.partial_fit(st, pr, X)
    if dt == np.float64:
        eD, eC = rel_fro(est.components_, st.D), rel_fro(est.code_[:n], st.code[:n])
        assert eD < 1e-9 and eC < 1e-9, (eD, eC)
        last = [rel_fro(est.code_[i], st.code[i]) for i in range(2 * b, n)]      # the ragged minibatch, row by row
        assert max(last) < 1e-9, last
        return
    X64 = X.astype(np.float64)
    st64 = oracle.prepare(pr, n_samples=n, X=X64)
    oracle.partial_fit(st64, pr, X64)
    assert_within_f32_noise(est.components_, st.D, st64.D, 'dictionary')
    assert_within_f32_noise(est.code_[:n], st.code[:n], st64.code[:n], 'codes')
    assert_within_f32_noise(est.code_[2 * b:n], st.code[2 * b:n], st64.code[2 * b:n], 'codes of the ragged minibatch')


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f64', 'f32'])
@pytest.mark.parametrize('k', [70, 193])
def test_coder_transform_ragged_last_batch(fast, k, dt):
    """Coder.transform with ridge codes on 2.5 batches of the transform plan (4096 rows each) against the direct solve of the
    same rows.  D and X are small dyadic rationals, so that G = D D^T and Dx = X D^T are exact in either dtype whatever
    the order of the sums: the plan's solver and the direct call see the same bits, and judge F applies as it stands - on
    every row of the last, partial batch and on the first rows of the full ones."""
    from modl_amd import Coder
    rs = np.random.RandomState(k)
    n, p, alpha = 4096 * 2 + 2048, k + 80, 1.0
    D = (rs.randint(-4, 5, size=(k, p)) / 8.0).astype(DT[dt])
    X = rs.randint(-8, 9, size=(n, p)).astype(DT[dt])
    G, Dx = D.dot(D.T), X.dot(D.T)
    assert np.array_equal(G.astype(np.float64), D.astype(np.float64).dot(D.T.astype(np.float64)))
    assert np.array_equal(Dx.astype(np.float64), X.astype(np.float64).dot(D.T.astype(np.float64)))
    got = Coder(D, code_alpha=alpha, code_l1_ratio=0).transform(X)
    assert got.shape == (n, k) and got.dtype == DT[dt]
    rows = np.concatenate([np.arange(0, 8), np.arange(4096, 4104), np.arange(8192, n)])
    case = SimpleNamespace(dt=DT[dt], dtn=dt, k=k, b=len(rows), p=p, multi=False, scene='transform', variant=0, G=G, Dx=Dx[rows], X=X[rows],
                           idx=np.arange(len(rows), dtype=np.int64), code0=np.ones((len(rows) + 3, k), dtype=DT[dt]), alpha=alpha,
                           dead=[], pairs=[], zero_row=None, positive=False, tol=1e-2, max_iter=100)
    cstar, conds = truth(case)
    osol = run_oracle(case)[:len(rows)]
    blocked = expected_route(dt, k, 4096, False).startswith('blocked')
    judge_f(case, got[rows], cstar, osol, 'transform F')
    judge_r(case, got[rows], conds, blocked, 'transform R')
    # every row against the direct solve of all rows in one call
    direct = np.ones((n, k), dtype=DT[dt])
    fast._enet_regression_single_gram(G.copy(), Dx.copy(), X, direct, np.arange(n, dtype=np.int64), 0.0, alpha, False, 1e-2, 100)
    judge_f(case, direct[rows], cstar, osol, 'direct F')
    bound = 2 * f_bound(case, cstar, osol)                       # (two results, each within the bound of c*)
    num = np.sqrt(((got.astype(np.float64) - direct) ** 2).sum(1))
    den = np.sqrt((direct.astype(np.float64) ** 2).sum(1))
    assert np.all(num <= bound * den), ('transform against the direct solve, per row', (num / den).max(), bound)
    _report()
