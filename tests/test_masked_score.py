"""Scoring, validating and imputing rows with missing entries: modl_masked_objective_* and modl_impute_*
(csrc/masked_objective.hip), `CodingMixin.score(X, mask)`, `held_out_error`, `impute` and `ImageDictFact.held_out_error`.

The reference has no counterpart.  The judge is `restate`, the definitions of include/modl_hip.h in numpy f64, and `judge`,
which holds the eight numbers of a launch to bounds computed from the case's own inputs - no tuned tolerance:

  u = 2^-24 (f32), 2^-53 (f64): unit roundoff of the dtype.
  delta_ie = (k + 2) u (|X_ie| + sum_j |code_ij| |Dt_ej|): the worst case of a k-term FMA chain in any order plus the
      subtraction in the dtype (|X_ie| taken as 0 where X is not used).
  a sum of w_i res_ie^2 over a selection may differ from the restatement by
      sum w_i (2 |res_ie| delta_ie + delta_ie^2)  +  n p 2^-52 sum
      (the second term: the squares, the weights and n p f64 additions in another order, each below 2^-53 relative);
  the code norms, sums of n k exact (f32) or once-rounded (f64) terms in f64, by n k 2^-52 sum; counts are exact;
  an imputed entry by delta_ie (without |X_ie|: X is not used there); an observed one carries the bits of X.

`test_restatement_in_the_dtype_sits_inside_the_bound` checks in numpy that the restatement run in f32 uses less than
0.2 % of this bound and the f64 one less than 1e-6 of it: the bound cannot fail a correct kernel.  It is loose in f32 at
large k (one dropped entry is invisible at k = 256), so every case runs in both dtypes - f64 is the sharp run - and
single-entry selections are added, where the sum must be that one res^2 within 2 |res| delta + delta^2.

`test_judge_rejects_mutants` runs wrong versions of the restatement (MUTANTS) on the CPU cases in both dtypes: the judge
rejects all but those named in INVISIBLE.  'residual_in_f64' (the subtraction rounded in f64 where the dtype is f32)
cannot be seen by any bound that admits the dtype's own rounding; it is listed for that reason."""
import ctypes as C
from collections import namedtuple

import numpy as np
import pytest
from numpy.testing import assert_array_equal

DT = {'f32': np.float32, 'f64': np.float64}
U = {'f32': 2.0 ** -24, 'f64': 2.0 ** -53}
MUTANTS = ('classes_swapped', 'w_unweighted', 'w_of_neighbour_row', 'last_column_dropped', 'last_row_dropped',
           'abs_residual', 'unselected_counted', 'unselected_nan_summed', 'norms_of_selected_rows', 'residual_in_f64')
INVISIBLE = ('residual_in_f64',)

Case = namedtuple('Case', 'dt X sel Dt code w')


# ---- the restatement and the judge ------------------------------------------------------------------------------------
def restate(c, T=np.float64, mutant=None):
    """[S_1, W_1, N_1, S_2, W_2, N_2, sum |code|, sum code^2]: product and difference in T, squares and sums in f64"""
    n, p = c.sel.shape
    sel = c.sel
    w = np.ones(n) if c.w is None else np.asarray(c.w, dtype=np.float64)
    if mutant == 'w_unweighted':
        w = np.ones(n)
    if mutant == 'w_of_neighbour_row':
        w = np.roll(w, 1)
    if mutant == 'classes_swapped':
        sel = np.where(sel == 1, 2, np.where(sel == 2, 1, sel))
    if mutant == 'unselected_counted':
        sel = np.where((sel != 1) & (sel != 2), 1, sel)
    used = (sel == 1) | (sel == 2)
    X = c.X.astype(T) if mutant == 'unselected_nan_summed' else np.where(used, c.X, 0).astype(T)
    prod = c.code.astype(T) @ c.Dt.astype(T).T
    if mutant == 'residual_in_f64':
        res = X.astype(np.float64) - prod.astype(np.float64)
    else:
        res = (X - prod).astype(np.float64)
    r2 = np.abs(res) if mutant == 'abs_residual' else res * res
    # the mutant: a product with zero instead of a select
    pick = (lambda m: r2 * m) if mutant == 'unselected_nan_summed' else (lambda m: np.where(m, r2, 0.0))
    if mutant == 'last_column_dropped':
        sel = sel.copy()
        sel[:, -1] = 0
    if mutant == 'last_row_dropped':
        sel = sel.copy()
        sel[-1, :] = 0
    out = []
    for cls in (1, 2):
        m = sel == cls
        out += [np.sum(pick(m)), np.sum(w * np.sum(pick(m), axis=1)), float(m.sum())]
    code = c.code.astype(np.float64)
    if mutant == 'norms_of_selected_rows':
        code = code[((sel == 1) | (sel == 2)).any(axis=1)]
    return np.array(out + [np.abs(code).sum(), (code * code).sum()])


def entry_bounds(c):
    """(res, delta) per entry in f64; X counts as 0 where it is not used"""
    k = c.code.shape[1]
    used = (c.sel == 1) | (c.sel == 2)
    X = np.where(used, c.X, 0).astype(np.float64)
    code, Dt = c.code.astype(np.float64), c.Dt.astype(np.float64)
    delta = (k + 2) * U[c.dt] * (np.abs(X) + np.abs(code) @ np.abs(Dt).T)
    return X - code @ Dt.T, delta


def bounds(c):
    """how far each of the eight numbers may be from restate(c)"""
    n, p = c.sel.shape
    k = c.code.shape[1]
    res, delta = entry_bounds(c)
    w = np.ones(n) if c.w is None else np.asarray(c.w, dtype=np.float64)
    want = restate(c)
    e = 2 * np.abs(res) * delta + delta * delta
    b = np.zeros(8)
    for q, cls in ((0, 1), (3, 2)):
        m = c.sel == cls
        b[q] = np.sum(np.where(m, e, 0.0)) + n * p * 2.0 ** -52 * want[q]
        b[q + 1] = np.sum(w * np.sum(np.where(m, e, 0.0), axis=1)) + n * p * 2.0 ** -52 * want[q + 1]
    b[6:] = n * k * 2.0 ** -52 * want[6:]
    return want, b


def judge(c, got):
    """True when the eight numbers `got` are within the bounds of the restatement (NaN is outside every bound)"""
    want, b = bounds(c)
    got = np.asarray(got, dtype=np.float64)
    return got.shape == (8,) and bool(np.all(np.abs(got - want) <= b))


def used_fraction(c, got):
    want, b = bounds(c)
    d = np.abs(np.asarray(got) - want)
    return float(np.max(np.where(b > 0, d / np.where(b > 0, b, 1), np.where(d > 0, np.inf, 0.0))))


# ---- cases --------------------------------------------------------------------------------------------------------------
_DATA = {}


def data(dt, n, p, k, seed=0):
    """finite X0 (n, p), Dt (p, k), code (n, k) in the dtype and row weights (n,) f64: X0 = code Dt^T + noise, a third of
    the codes zero, one row of codes zero, weights between 0.5 and 3 (no two neighbours alike).  Computed once, shared."""
    key = (dt, n, p, k, seed)
    if key not in _DATA:
        rs = np.random.RandomState(1000 * seed + n + 7 * p + 13 * k)
        Dt = rs.randn(p, k) / np.sqrt(k)
        code = rs.randn(n, k) * (rs.rand(n, k) > 1 / 3)
        if n > 2:
            code[n // 2] = 0
        X0 = code @ Dt.T + 0.3 * rs.randn(n, p)
        w = 0.5 + 2.5 * rs.rand(n)
        T = DT[dt]
        _DATA[key] = (np.ascontiguousarray(X0.astype(T)), np.ascontiguousarray(Dt.astype(T)),
                      np.ascontiguousarray(code.astype(T)), w)
        for a in _DATA[key]:
            a.setflags(write=False)
    return _DATA[key]


def make_case(dt, n, p, k, sel, weighted, seed=0):
    """X is NaN wherever sel selects nothing"""
    X0, Dt, code, w = data(dt, n, p, k, seed)
    sel = np.ascontiguousarray(sel, dtype=np.uint8)
    X = np.where((sel == 1) | (sel == 2), X0, np.nan).astype(DT[dt])
    return Case(dt, X, sel, Dt, code, w if weighted else None)


def random_sel(n, p, seed=0):
    sel = np.random.RandomState(77 + seed + n + p).randint(0, 4, size=(n, p)).astype(np.uint8)
    return sel


def cpu_cases(dt):
    """'random': 17 x 33, k = 7, every byte value, both classes in the last row and the last column, row 3 (codes not
    zero) entirely unselected, weights;  'plain': the same without weights;  'single': one entry of class 1"""
    n, p, k = 17, 33, 7
    sel = random_sel(n, p)
    sel[3] = 0
    sel[-1, :4] = (1, 2, 0, 3)
    sel[:4, -1] = (2, 1, 3, 0)
    single = np.zeros((n, p), dtype=np.uint8)
    single[15, 16] = 1
    return dict(random=make_case(dt, n, p, k, sel, True), plain=make_case(dt, n, p, k, sel, False),
                single=make_case(dt, n, p, k, single, True))


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_restatement_on_a_case_worked_by_hand():
    """2 x 3, k = 1: code D = [[1, 0, -1], [2, 0, -2]], res = [[0, 2, 4], [2, 5, 8]]; class 1 = {(0,0), (1,1), (1,2)}:
    S = 0 + 25 + 64, W = 2 * 0 + 3 * 89, N = 3; class 2 = {(0,1), (1,0)}: S = 4 + 4, W = 2 * 4 + 3 * 4, N = 2; the entry
    (0, 2) of X, not selected, is NaN"""
    c = Case('f64', np.array([[1., 2., np.nan], [4., 5., 6.]]), np.array([[1, 2, 0], [2, 1, 1]], dtype=np.uint8),
             np.array([[1.], [0.], [-1.]]), np.array([[1.], [2.]]), np.array([2., 3.]))
    assert_array_equal(restate(c), [89., 267., 3., 8., 20., 2., 3., 5.])
    assert_array_equal(restate(c._replace(w=None)), [89., 89., 3., 8., 8., 2., 3., 5.])
    assert_array_equal(restate(c._replace(sel=np.array([[7, 3, 0], [0, 255, 4]], dtype=np.uint8))), [0, 0, 0, 0, 0, 0, 3, 5])
    assert judge(c, restate(c)) and not judge(c, restate(c) + np.eye(8)[0] * 1e-9)


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_restatement_in_the_dtype_sits_inside_the_bound(dt):
    """what a correct kernel computes (product and difference in the dtype, numpy's summation order) on the shapes of the
    GPU tests: inside the bound everywhere; in f64 numpy's matmul and the restatement are the same computation (below 1e-6
    of the bound, in fact 0); in f32 below 0.2 % of it wherever k >= 16 (at most 0.05 %, measured) - the two smallest
    shapes, k = 1 and k = 7, where (k + 2) u is not far above the rounding of a single operation and few entries average
    out, use up to 0.35 % (17 x 33 x 7), still three hundred times inside"""
    for n, p, k in SHAPES:
        for weighted in (True, False):
            c = make_case(dt, n, p, k, random_sel(n, p), weighted)
            frac = used_fraction(c, restate(c, T=DT[dt]))
            print('restatement in', dt, (n, p, k), 'weighted' if weighted else 'plain', 'uses', frac, 'of the bound')
            assert frac < 1
            if dt == 'f64':
                assert frac < 1e-6
            elif k >= 16:
                assert frac < 2e-3


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_judge_rejects_mutants(dt):
    cases = cpu_cases(dt)
    for c in cases.values():
        assert judge(c, restate(c)) and judge(c, restate(c, T=DT[dt]))
    c = cases['random']
    assert c.code[3].any() and not c.sel[3].any() and {1, 2} <= set(c.sel[-1]) and {1, 2} <= set(c.sel[:, -1])
    survivors = [m for m in MUTANTS if judge(c, restate(c, T=DT[dt], mutant=m))]
    assert survivors == list(INVISIBLE), survivors       # (in f64 'residual_in_f64' is the restatement itself)
    # without weights 'w_unweighted' and 'w_of_neighbour_row' are the restatement itself: nothing else survives
    plain = [m for m in MUTANTS if judge(cases['plain'], restate(cases['plain'], T=DT[dt], mutant=m))]
    assert set(plain) == {'w_unweighted', 'w_of_neighbour_row'} | set(INVISIBLE), plain
    # the single entry: the sum is that one res^2
    s = cases['single']
    res, delta = entry_bounds(s)
    got = restate(s, T=DT[dt])
    assert got[2] == 1 and got[5] == 0 and got[3] == 0
    assert abs(got[0] - res[15, 16] ** 2) <= 2 * abs(res[15, 16]) * delta[15, 16] + delta[15, 16] ** 2


def _host_ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_new_entry_points_check_arguments_before_any_device_work():
    """the host-side checks of every new export: no GPU is touched (the pointers are host arrays, never read)"""
    from modl_amd._lib import lib
    buf = np.zeros(4096)
    q = _host_ptr(buf)
    kmax = lib.modl_max_components()
    assert kmax == 4096
    for dtype_id in (0, 1):
        for p in (1, 64, 65, 1000):
            sizes = [lib.modl_masked_objective_workspace(dtype_id, n, p) for n in list(range(0, 300)) + [10 ** 6, 10 ** 8]]
            assert min(sizes) > 0 and all(a <= b for a, b in zip(sizes, sizes[1:]))
    for sfx in ('f32', 'f64'):
        mo = getattr(lib, 'modl_masked_objective_' + sfx)
        need = lib.modl_masked_objective_workspace(0 if sfx == 'f32' else 1, 17, 33)
        ok = dict(X=q, ldx=36, sel=q, lds=38, n=17, p=33, Dt=q, k=7, code=q, w=None, ws=q, wsb=need, out=q)
        call = lambda a: mo(a['X'], a['ldx'], a['sel'], a['lds'], a['n'], a['p'], a['Dt'], a['k'], a['code'], a['w'],
                            a['ws'], a['wsb'], a['out'], None)
        for bad in (dict(X=None), dict(sel=None), dict(Dt=None), dict(code=None), dict(out=None), dict(ws=None),
                    dict(n=-1), dict(p=0), dict(p=-3), dict(k=0), dict(k=-1), dict(k=kmax + 1), dict(ldx=32), dict(lds=32)):
            assert call(dict(ok, **bad)) == -1, bad
        for wsb in (0, need - 1):
            assert call(dict(ok, wsb=wsb)) == -2, wsb
        im = getattr(lib, 'modl_impute_' + sfx)
        ok = dict(code=q, n=17, k=7, Dt=q, p=33, X=q, ldx=36, obs=q, ldo=38, out=q, ldout=34)
        call = lambda a: im(a['code'], a['n'], a['k'], a['Dt'], a['p'], a['X'], a['ldx'], a['obs'], a['ldo'], a['out'],
                            a['ldout'], None)
        for bad in (dict(code=None), dict(Dt=None), dict(X=None), dict(obs=None), dict(out=None), dict(n=-1), dict(p=0),
                    dict(k=0), dict(k=kmax + 1), dict(ldx=32), dict(ldo=32), dict(ldout=32)):
            assert call(dict(ok, **bad)) == -1, bad
        assert call(dict(ok, n=0)) == 0                              # nothing to do, nothing launched


def test_bad_arguments_raise_valueerror_without_gpu():
    from modl_amd import DictFact
    X = np.zeros((5, 60))
    full = np.ones((5, 60), dtype=bool)
    est = DictFact(n_components=7)
    for bad_mask in (np.ones((5, 59), dtype=bool), np.ones((4, 60), dtype=bool), np.ones(60, dtype=bool),
                     np.ones((5, 60, 1), dtype=bool)):
        for call in (lambda: est.score(X, mask=bad_mask), lambda: est.held_out_error(X, mask=bad_mask),
                     lambda: est.impute(X, bad_mask)):
            with pytest.raises(ValueError, match='mask'):
                call()
    with pytest.raises(ValueError, match='n_samples, n_features'):
        est.held_out_error(np.zeros(60))
    for bad in (0.0, 1.0, 1.5, -0.1, float('nan'), np.float32(2), 1, True, 'half', None, np.ones((5, 59), dtype=bool),
                np.ones((4, 60), dtype=bool), np.ones(60, dtype=bool), np.ones((5, 60)), np.ones((5, 60), dtype=np.uint8)):
        for mask in (None, full):
            with pytest.raises(ValueError, match='held_out'):
                est.held_out_error(X, mask=mask, held_out=bad)
    for call in (lambda: est.held_out_error(X, algorithm='lars'), lambda: est.impute(X, full, algorithm='lars'),
                 lambda: est.held_out_error(X, n_nonzero_coefs=3), lambda: est.impute(X, full, residual_tol=0.1)):
        with pytest.raises(ValueError, match='algorithm'):
            call()
    big = DictFact(n_components=1025)
    for call in (lambda: big.score(X, mask=full), lambda: big.held_out_error(X), lambda: big.held_out_error(X, mask=full),
                 lambda: big.impute(X, full)):
        with pytest.raises(ValueError, match='1024'):
            call()


# ---- GPU: the kernels through the ABI, with given codes ---------------------------------------------------------------
SHAPES = [(1, 1, 1), (17, 33, 7), (33, 65, 70), (5, 193, 33), (130, 60, 256), (65, 1000, 17), (40, 200, 1100), (3, 64, 4096),
          (700, 700, 16)]


def _t(a):
    import torch
    return torch.from_numpy(np.array(a, order='C')).cuda()             # (a copy: the shared arrays are read-only)


def _padded(a, ld, fill):
    """the device tensor (n, ld) whose first columns are `a`, the padding `fill`"""
    import torch
    out = torch.full((a.shape[0], ld), fill, dtype=torch.from_numpy(a[:0]).dtype, device='cuda')
    out[:, :a.shape[1]] = _t(a)
    return out


class Device:
    """the operands of one (dtype, shape) on the device, staged once: Dt, code, weights, workspace"""

    def __init__(self, dt, n, p, k):
        import torch
        from modl_amd._lib import lib
        self.dt, self.n, self.p, self.k = dt, n, p, k
        _, Dt, code, w = data(dt, n, p, k)
        self.Dt, self.code, self.w = _t(Dt), _t(code), _t(w)
        self.nbytes = lib.modl_masked_objective_workspace(0 if dt == 'f32' else 1, n, p)
        self.ws = torch.empty(self.nbytes, dtype=torch.uint8, device='cuda')

    def objective(self, c, n=None):
        """the eight numbers of case c: ldx = p + 3, lds = p + 5, NaN and 1 in the padding"""
        import torch
        from modl_amd._lib import lib
        X, sel = _padded(c.X, self.p + 3, float('nan')), _padded(c.sel, self.p + 5, 1)
        out = torch.full((8,), float('nan'), dtype=torch.float64, device='cuda')
        rc = getattr(lib, 'modl_masked_objective_' + self.dt)(
            X.data_ptr(), self.p + 3, sel.data_ptr(), self.p + 5, self.n if n is None else n, self.p, self.Dt.data_ptr(),
            self.k, self.code.data_ptr(), None if c.w is None else self.w.data_ptr(), self.ws.data_ptr(), self.nbytes,
            out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
        return out.cpu().numpy()


def _selections(n, p):
    sel = random_sel(n, p)
    one_row_out = random_sel(n, p, seed=1)
    one_row_out[n // 3] = np.where(one_row_out[n // 3] < 2, 0, 3)
    return dict(random=sel, none=np.zeros((n, p), dtype=np.uint8), all_class_1=np.ones((n, p), dtype=np.uint8),
                class_2_only=np.where(sel == 2, 2, np.where(sel == 1, 3, sel)), one_row_unselected=one_row_out)


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'f64'])
@pytest.mark.parametrize('n,p,k', SHAPES)
def test_masked_objective_through_the_abi(n, p, k, dt):
    dev = Device(dt, n, p, k)
    for name, sel in _selections(n, p).items():
        for weighted in (True, False):
            c = make_case(dt, n, p, k, sel, weighted)
            got = dev.objective(c)
            print('masked objective', dt, (n, p, k), name, 'weighted' if weighted else 'plain', 'uses', used_fraction(c, got),
                  'of the bound')
            assert judge(c, got), (name, weighted, got, bounds(c))
            if name == 'random':
                assert_array_equal(dev.objective(c).view(np.int64), got.view(np.int64))       # the same bits again
            if name == 'none':
                assert_array_equal(got[:6], 0)
            if name == 'all_class_1':
                assert got[2] == n * p and got[5] == 0 and got[3] == 0 and got[4] == 0
            if name == 'class_2_only':
                assert got[2] == 0 and got[0] == 0 and got[1] == 0
    for i, e in ((0, 0), (n - 1, p - 1), (15, 16), (16, 15), (63, 64)):
        if i < n and e < p:
            sel = np.zeros((n, p), dtype=np.uint8)
            sel[i, e] = 1
            c = make_case(dt, n, p, k, sel, False)
            got = dev.objective(c)
            res, delta = entry_bounds(c)
            assert got[2] == 1 and got[5] == 0 and got[3] == 0 and got[4] == 0 and got[0] == got[1], ((i, e), got)
            assert abs(got[0] - res[i, e] ** 2) <= 2 * abs(res[i, e]) * delta[i, e] + delta[i, e] ** 2, ((i, e), got)
            c2 = make_case(dt, n, p, k, 2 * sel, True)                                         # and as class 2, weighted
            got2 = dev.objective(c2)
            assert judge(c2, got2) and got2[3] == got[0] and got2[5] == 1 and got2[0] == 0, ((i, e), got2)
    assert_array_equal(dev.objective(make_case(dt, n, p, k, random_sel(n, p), True), n=0), 0)    # n = 0: eight zeros


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'f64'])
@pytest.mark.parametrize('n,p,k', SHAPES)
def test_impute_through_the_abi(n, p, k, dt):
    """ldx = p + 3, ldo = p + 5, ldout = p + 1; NaN at unobserved X; observed entries keep their bits, the padding of
    the output is not written, imputed entries are within delta of code D"""
    import torch
    from modl_amd._lib import lib
    dev = Device(dt, n, p, k)
    X0, Dt, code, _ = data(dt, n, p, k)
    bits = np.int32 if dt == 'f32' else np.int64
    prod = code.astype(np.float64) @ Dt.astype(np.float64).T
    delta = (k + 2) * U[dt] * (np.abs(code.astype(np.float64)) @ np.abs(Dt.astype(np.float64)).T)
    masks = dict(random=random_sel(n, p) % 3, none=np.zeros((n, p), dtype=np.uint8), all=np.full((n, p), 255, dtype=np.uint8))
    for name, obs in masks.items():
        X = np.where(obs != 0, X0, np.nan).astype(DT[dt])
        dX, dobs = _padded(X, p + 3, float('nan')), _padded(obs.astype(np.uint8), p + 5, 1)
        out = torch.full((n, p + 1), -7.0, dtype=dX.dtype, device='cuda')
        rc = getattr(lib, 'modl_impute_' + dt)(dev.code.data_ptr(), n, k, dev.Dt.data_ptr(), p, dX.data_ptr(), p + 3,
                                               dobs.data_ptr(), p + 5, out.data_ptr(), p + 1,
                                               torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
        got = out.cpu().numpy()
        assert_array_equal(got[:, p], -7.0)
        got = np.ascontiguousarray(got[:, :p])
        o = obs != 0
        assert_array_equal(got.view(bits)[o], np.ascontiguousarray(X).view(bits)[o])
        err = np.abs(got.astype(np.float64) - prod)[~o]
        assert np.all(err <= delta[~o]), (name, float(np.max(err / delta[~o])))
        if name == 'none' and n > 2:
            assert np.count_nonzero(got) > 0


# ---- GPU: the estimators ------------------------------------------------------------------------------------------------
ALPHA = 0.05


def _batch(dtype, seed=3, n=20, p=60, k=12):
    """as test_inpaint._mixed_batch: rows 0, 5, 9, 19 clean, rows 3 and 12 empty, the others half observed"""
    rs = np.random.RandomState(seed)
    D = rs.randn(k, p)
    D /= np.linalg.norm(D, axis=1, keepdims=True)
    X = (rs.randn(n, 4) @ rs.randn(4, p) + 0.3 * rs.randn(n, p)) / np.sqrt(p)
    mask = rs.rand(n, p) < 0.5
    mask[[0, 5, 9, 19]] = True
    mask[[3, 12]] = False
    return D.astype(dtype), X.astype(dtype), mask


_EST = {}


def estimator(kind, dtype):
    from modl_amd import Coder, DictFact
    key = (kind, np.dtype(dtype))
    if key not in _EST:
        D, X, _ = _batch(dtype)
        if kind == 'Coder':
            _EST[key] = Coder(D, code_alpha=ALPHA, code_l1_ratio=0.7)
        else:
            _EST[key] = DictFact(n_components=12, code_alpha=ALPHA, code_l1_ratio=0.7, batch_size=5, n_epochs=2,
                                 random_state=0).fit(_batch(dtype, seed=4, n=40)[1])
    return _EST[key]


def _case_of(est, dt, X, sel, code, w=None):
    T = DT[dt]
    Dt = np.ascontiguousarray(np.asarray(est.components_).T.astype(T))
    return Case(dt, np.asarray(X, dtype=T), np.ascontiguousarray(sel, dtype=np.uint8), Dt, np.asarray(code, dtype=T), w)


def _score_of(est, s):
    return (s[1] / 2 + est.code_alpha * (est.code_l1_ratio * s[6] + (1 - est.code_l1_ratio) / 2 * s[7]))


def _rmse_window(S, b, N):
    """the interval of sqrt(S' / N) over |S' - S| <= b; division and square root are correctly rounded (2^-53 each)"""
    r = 4 * 2.0 ** -53
    return np.sqrt(max(S - b, 0.0) / N) * (1 - r), np.sqrt((S + b) / N) * (1 + r)


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f64', 'f32'])
@pytest.mark.parametrize('kind', ['Coder', 'DictFact'])
def test_estimators_score_validate_and_impute(kind, dt):
    """every figure against the restatement fed with the codes of est.transform(X, coded mask): the solver is not
    re-judged.  The batch has clean, holed and empty rows; the boolean hold-out empties row 1."""
    import torch
    from sklearn.utils import check_random_state
    dtype = DT[dt]
    est = estimator(kind, dtype)
    assert np.asarray(est.components_).dtype == dtype
    _, X, mask = _batch(dtype)
    n, p = X.shape
    Xn = np.where(mask, X, np.nan).astype(dtype)
    m = mask.sum(axis=1)
    assert (m == p).sum() == 4 and (m == 0).sum() == 2

    # score(X, mask)
    code = est.transform(Xn, mask=mask)
    w = np.where(m > 0, p / np.maximum(m, 1), 0.0)
    c = _case_of(est, dt, Xn, mask, code, w)
    want, b = bounds(c)
    got = est.score(Xn, mask=mask)
    bound = _score_of(est, b) / n + 4 * 2.0 ** -53 * _score_of(est, want) / n
    print('score with a mask', kind, dt, got, 'off by', abs(got - _score_of(est, want) / n), 'bound', bound)
    assert abs(got - _score_of(est, want) / n) <= bound
    assert got == est.score(_t(Xn), mask=_t(mask))

    # a full mask: score(X).  Both sides are within their bound of the exact value (score(X) rounds the product and the
    # difference in the dtype as well), so within twice the bound of each other
    full = np.ones((n, p), dtype=bool)
    cf = _case_of(est, dt, X, full, est.transform(X), np.ones(n))
    wantf, bf = bounds(cf)
    plain, masked = est.score(X), est.score(X, mask=full)
    print('score, full mask', kind, dt, plain, masked, 'bound', 2 * _score_of(est, bf) / n)
    assert abs(masked - _score_of(est, wantf) / n) <= _score_of(est, bf) / n + 4 * 2.0 ** -53 * plain
    assert abs(masked - plain) <= 2 * _score_of(est, bf) / n + 8 * 2.0 ** -53 * plain
    assert np.float64(plain).view(np.int64) == np.float64(est.score(X, mask=None)).view(np.int64)

    # held_out_error: a fraction (the draw restated), a boolean array that empties row 1, omp, no mask
    H_frac = check_random_state(5).random_sample((n, p)) < 0.3
    H_bool = np.random.RandomState(9).rand(n, p) < 0.25
    H_bool[1] = True
    assert mask[1].any() and not mask[1].all()
    runs = [(dict(mask=mask, held_out=0.3, random_state=5), mask, H_frac, {}),
            (dict(mask=mask, held_out=H_bool), mask, H_bool, {}),
            (dict(held_out=0.3, random_state=5), full, H_frac, {}),
            (dict(mask=mask, held_out=H_bool, algorithm='omp', n_nonzero_coefs=3), mask, H_bool,
             dict(algorithm='omp', n_nonzero_coefs=3))]
    for kw, obs, H, coder_kw in runs:
        Xin = X if obs is full else Xn
        coded = obs & ~H
        code = est.transform(Xin, mask=coded, **coder_kw)
        if H is H_bool:
            assert not coded[1].any() and not code[1].any() and (obs & H)[1].any()
        sel = obs.astype(np.uint8) * (1 + H.astype(np.uint8))
        c = _case_of(est, dt, Xin, sel, code)
        want, b = bounds(c)
        got = est.held_out_error(Xin, **kw)
        print('held_out_error', kind, dt, sorted(kw), got, 'restated', np.sqrt(want[3] / want[5]), np.sqrt(want[0] / want[2]))
        assert type(got).__name__ == 'HeldOutError' and got._fields == ('rmse', 'rmse_coded', 'n_held_out', 'n_coded')
        assert got.n_held_out == want[5] == (obs & H).sum() and got.n_coded == want[2] == coded.sum()
        lo, hi = _rmse_window(want[3], b[3], want[5])
        assert lo <= got.rmse <= hi, (got.rmse, lo, hi)
        lo, hi = _rmse_window(want[0], b[0], want[2])
        assert lo <= got.rmse_coded <= hi, (got.rmse_coded, lo, hi)
        if 'algorithm' not in kw:                                      # tensors in: the same figures
            kw_t = {key: _t(v) if isinstance(v, np.ndarray) else v for key, v in kw.items()}
            assert est.held_out_error(_t(Xin), **kw_t) == got
    # empty sets give nan, they do not raise
    none = est.held_out_error(Xn, mask=mask, held_out=np.zeros((n, p), dtype=bool))
    assert np.isnan(none.rmse) and none.n_held_out == 0 and none.n_coded == mask.sum() and np.isfinite(none.rmse_coded)
    everything = est.held_out_error(Xn, mask=mask, held_out=np.ones((n, p), dtype=bool))
    assert np.isnan(everything.rmse_coded) and everything.n_coded == 0 and everything.n_held_out == mask.sum()
    assert abs(everything.rmse - np.sqrt(np.mean(X.astype(np.float64)[mask] ** 2))) <= n * p * 2.0 ** -52 * everything.rmse

    # impute
    bits = np.int32 if dt == 'f32' else np.int64
    for coder_kw in ({}, dict(algorithm='omp', n_nonzero_coefs=3)):
        code = est.transform(Xn, mask=mask, **coder_kw).astype(np.float64)
        D = np.asarray(est.components_).astype(np.float64)
        out = est.impute(Xn, mask, **coder_kw)
        assert isinstance(out, np.ndarray) and out.dtype == dtype and out.shape == X.shape
        assert_array_equal(out.view(bits)[mask], Xn.view(bits)[mask])
        delta = (D.shape[0] + 2) * U[dt] * (np.abs(code) @ np.abs(D))
        assert np.all(np.abs(out.astype(np.float64) - code @ D)[~mask] <= delta[~mask])
        assert np.count_nonzero(out[~mask]) > 0 and not out[[3, 12]].any()
        out_t = est.impute(_t(Xn), _t(mask), **coder_kw)
        assert isinstance(out_t, torch.Tensor) and out_t.is_cuda
        assert_array_equal(out_t.cpu().numpy().view(bits), out.view(bits))


# ---- GPU: ImageDictFact.held_out_error ---------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_image_held_out_error_is_inpaint_plus_numpy(dtype):
    """on the 19 x 23 x 3 fixture of test_inpaint.py, strides 1 and (2, 3): the same inpaint call, the error restated in
    numpy f64.  Both sides sum at most 1311 f64 squares of the same bits in different orders: 1311 * 2^-52 relative on the
    sum, half of it on the root; the counts are exact."""
    from sklearn.utils import check_random_state
    from .test_inpaint import STRIDES, SHAPE, fitted, inpaint_image
    est = fitted(dtype, 'dictionary learning')
    img, obs = inpaint_image(dtype)
    H_frac = check_random_state(11).random_sample(SHAPE) < 0.2
    H_2d = np.random.RandomState(12).rand(*SHAPE[:2]) < 0.3
    H_block = np.zeros(SHAPE[:2], dtype=bool)                     # 8 x 10, larger than (2 x - 1) x (2 y - 1): at stride 1 its
    H_block[0:8, 6:16] = True                                     # centre is covered by windows without a coded element only
    for stride in STRIDES:
        for kw, H, mask in ((dict(held_out=0.2, random_state=11), H_frac, None),
                            (dict(held_out=H_block), H_block[:, :, None] & np.ones(SHAPE, dtype=bool), None),
                            (dict(held_out=H_2d, mask=obs), H_2d[:, :, None] & np.ones(SHAPE, dtype=bool), obs),
                            (dict(held_out=H_frac, mask=obs[:, :, 0] & obs[:, :, 1] & obs[:, :, 2]), H_frac,
                             (obs[:, :, 0] & obs[:, :, 1] & obs[:, :, 2])[:, :, None] & np.ones(SHAPE, dtype=bool))):
            o = obs if mask is None else mask
            out, filled = est.inpaint(img, mask=o & ~H, stride=stride, return_filled=True)
            held = o & H
            seen = held & filled[:, :, None]
            d = (out.astype(np.float64) - img.astype(np.float64))[seen]
            got = est.held_out_error(img, stride=stride, **kw)
            print('image held_out_error', np.dtype(dtype), stride, sorted(kw), got)
            assert type(got).__name__ == 'ImageHeldOutError' and got._fields == ('rmse', 'n_held_out', 'n_unfilled')
            assert got.n_held_out == seen.sum() > 0 and got.n_unfilled == held.sum() - seen.sum()
            if H is not H_frac and mask is None and stride == (1, 1):
                assert got.n_unfilled > 0
            want = np.sqrt(np.sum(d * d) / seen.sum())
            assert abs(got.rmse - want) <= 1311 * 2.0 ** -52 * want
    for bad in (1.0, np.ones(SHAPE[:2]), np.ones((19, 22), dtype=bool), np.ones(SHAPE + (1,), dtype=bool)):
        with pytest.raises(ValueError, match='held_out'):
            est.held_out_error(img, held_out=bad)
