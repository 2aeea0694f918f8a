"""CanICA on the device: modl_amd.canica, csrc/ica.hip, fMRIDictFact(dict_init='canica').

The judge is the set of host twins (`*_host`: numpy / scipy and sklearn.decomposition.fastica).  Layer 1 (no GPU) holds the
judge to an independent restatement in plain numpy - the FastICA loop with an explicit loop over voxels for the sweep and
scipy's eigh for the decorrelation -, shows that each mutant of the restatement is rejected by at least one case, checks the
threshold bit for bit against scipy.stats.scoreatpercentile and the two PCA steps against prescribed spectra, and then the
refusals.  Layer 2 (gpu): the sweep kernel through the C-ABI inside guard elements with a NaN-poisoned workspace, then the
Python functions, the pipeline on planted maps and the estimator.

Tolerances, and where each comes from.

W_TOL, for unmixing matrices of the same input and the same w_init computed in two ways (twin against restatement, device
against twin): measured on the CPU as the largest |difference| in W between the twin's run and the twin's run on the same
input with the voxel order reversed - a different, equally valid summation order - over CASES x FUNS: 4.1e-15 (the worst case
is cube on the (5, 1500) maps).  W_TOL = 100 x 4.1e-15 = 4.1e-13; the factor absorbs a third summation order, the device's.
Every case first asserts, on the twin's own lim sequence (fastica_lims_host), that no lim comes within a relative 1e-6 of
tol: an iteration count cannot then flip on rounding.

The sweep, per output element: (8 (V + k) + ULP_fun) u times the sum of the absolute values of its terms, u = 2^-53.  The
terms of M[i][j] are those of (1 / V) sum_v g(sum_l w_il x_lv) x_jv written out: for cube the expanded polynomial, whose
absolute sum is (sum_l |w_il x_lv|)^3 |x_jv| / V; for logcosh and exp |g| plus a first-order image of the inner product's
absolute sum A = sum_l |w_il x_lv|: (|g| + D A) |x_jv| / V with D an upper bound of |dg/dy| - alpha for logcosh (the slope of
tanh(alpha y) is at most alpha), e (1 + y^2) for exp (e = exp(-y^2 / 2): the two terms of dg/dy in absolute value); likewise
for gp: alpha (1 + g^2) + 2 alpha^2 |g| A for logcosh, (1 + y^2) e + e |y| (3 + y^2) A for exp (see abs_terms).  8 counts the
roundings of the formula per accumulated term (product, accumulation, cube / square, scale) with room for the two
products' different association.
ULP_fun: the ulp error of the device's tanh / exp in f64.  The table of HIP's math functions was not at hand where this was
written, so it was measured: the largest ulp difference between the device's function and numpy's over the arguments these
cases produce was 1 for tanh and 1 for exp; twice that, 2, is used for both.

reduce_record, per element of row i: 64 V u s_1^2 / min_gap(s^2) times s_i (eigenvector perturbation of the Gram matrix,
whose entries carry V u s_1^2 of rounding); group_components, per element of the projector C^T C: the same with the gap
between the k-th and (k + 1)-th squared group singular values.

The module imports the new names at the top: no test here can pass without the feature."""
import ctypes as C
import warnings

import numpy as np
import pytest
import scipy.linalg
import scipy.stats
from scipy.optimize import linear_sum_assignment

from modl_amd.canica import (IcaMaps, Canica, reduce_record, group_components, fastica_maps, threshold_maps, canica,  # noqa: F401
                             reduce_record_host, group_components_host, fastica_maps_host, threshold_maps_host, canica_host,
                             fastica_lims_host, FUNS)
from modl_amd._lib import lib

from .test_clean import EINVAL, ENOMEM, same_bits
from .test_compute_mask import _Guarded, GUARD, gpu  # noqa: F401

U = 2.0 ** -53
W_TOL = 4.1e-13
ULP = {'cube': 0, 'logcosh': 2, 'exp': 2}
TOL = 1e-4
MUTANTS = ('gp_y2', 'no_gp', 'sum_not_mean', 'row_decorrelation', 'lim_no_abs', 'select_max', 'percentile_k', 'sign_reversed',
           'centre_components')


# ------------------------------------------------------------------------------------------------------- the phantoms
def sparse_maps(seed, k, V):
    rng = np.random.RandomState(seed)
    return rng.laplace(size=(k, V)) * (rng.rand(k, V) < 0.15)


def phantom(seed, V, T, k, n_records):
    """(planted maps (k, V), records): the phantom of the issue"""
    rng = np.random.RandomState(seed)
    maps = rng.laplace(size=(k, V)) * (rng.rand(k, V) < 0.15)
    records = []
    for _ in range(n_records):
        r = rng.randn(T, k) @ maps + 0.1 * rng.randn(T, V)
        records.append(r - r.mean(axis=0))
    return maps, records


def mixed_case(k, V, n_init=4):
    """sparse Laplace maps mixed by a random orthogonal matrix, and a w_init"""
    rng = np.random.RandomState(100 + k)
    q, _ = np.linalg.qr(rng.randn(k, k))
    return np.ascontiguousarray(q @ sparse_maps(7 + k, k, V)), rng.randn(n_init, k, k)


CASES = {(3, 600): mixed_case(3, 600), (5, 1500): mixed_case(5, 1500)}
PHANTOMS = [(600, 24, 3, 2), (1500, 30, 5, 2)]
_twin_cache = {}


def twin(shape, fun):
    """the judge's run of a case, computed once and shared"""
    if (shape, fun) not in _twin_cache:
        comp, w0 = CASES[shape]
        with warnings.catch_warnings():
            warnings.simplefilter('error')                               # every restart converges
            res = fastica_maps_host(comp, fun=fun, tol=TOL, max_iter=60, w_init=w0)
        lims = fastica_lims_host(comp, w0, fun, n_iter=res.n_iter)
        for seq in lims:                                                # the precondition: no count can flip on rounding
            assert len(seq) and np.all(np.abs(seq - TOL) > 1e-6 * TOL)
        _twin_cache[shape, fun] = res
    return _twin_cache[shape, fun]


def matched_correlations(planted, found):
    """|corr| of every planted map with the distinct recovered map assigned to it"""
    k = planted.shape[0]
    c = np.abs(np.corrcoef(np.vstack([planted, found]))[:k, k:])
    rows, cols = linear_sum_assignment(-c)
    return c[rows, cols]


# ------------------------------------------------------------------------------------------- the restatement (numpy)
def re_nonlinearity(y, fun, alpha, mutant=None):
    if fun == 'cube':
        return y ** 3, (y ** 2 if mutant == 'gp_y2' else 3 * y ** 2)
    if fun == 'logcosh':
        g = np.tanh(alpha * y)
        return g, alpha * (1 - g * g)
    e = np.exp(-y * y / 2)
    return y * e, (1 - y * y) * e


def re_sweep(X1, W, fun, alpha, mutant=None):
    """M = (1 / V) sum_v g(W x_v) x_v^T, gp = (1 / V) sum_v g'(W x_v): one voxel at a time"""
    k, V = X1.shape
    M, gp = np.zeros((k, k)), np.zeros(k)
    for v in range(V):
        x = X1[:, v]
        g, d = re_nonlinearity(W @ x, fun, alpha, mutant)
        M += np.outer(g, x)
        gp += d
    # (the sum replaces the mean in M alone: in both M and gp it would only scale W1's argument, which the symmetric
    # decorrelation undoes - no case could see it)
    return (M if mutant == 'sum_not_mean' else M / V), gp / V


def re_decorrelation(W, mutant=None):
    if mutant == 'row_decorrelation':
        return W / np.linalg.norm(W, axis=1, keepdims=True)
    s, u = scipy.linalg.eigh(W @ W.T)
    s = np.maximum(s, np.finfo(np.float64).tiny)
    return u @ np.diag(1.0 / np.sqrt(s)) @ u.T @ W


def re_whiten(X, mutant=None):
    Xc = X - (X.mean(axis=0, keepdims=True) if mutant == 'centre_components' else X.mean(axis=1, keepdims=True))
    s, u = scipy.linalg.eigh(Xc @ Xc.T / X.shape[1])
    return u @ np.diag(1.0 / np.sqrt(s)) @ u.T @ Xc


def re_fastica(comp, w_init, fun, alpha=1.0, tol=TOL, max_iter=60, mutant=None):
    X1 = re_whiten(comp, mutant)
    n, k = w_init.shape[:2]
    Ws, n_iter, converged, l1 = np.zeros((n, k, k)), np.zeros(n, np.int64), np.zeros(n, bool), np.zeros(n)
    for r in range(n):
        W = re_decorrelation(w_init[r], mutant)
        for it in range(1, max_iter + 1):
            M, gp = re_sweep(X1, W, fun, alpha, mutant)
            W1 = re_decorrelation(M if mutant == 'no_gp' else M - gp[:, None] * W, mutant)
            d = np.diag(W1 @ W.T)
            lim = np.max(np.abs((d if mutant == 'lim_no_abs' else np.abs(d)) - 1))
            W = W1
            n_iter[r] = it
            if lim < tol:
                converged[r] = True
                break
        Ws[r] = W
        l1[r] = np.abs(W @ X1).sum(axis=1).max()
    selected = int(np.argmax(l1) if mutant == 'select_max' else np.argmin(l1))
    return IcaMaps(Ws[selected] @ X1, Ws, n_iter, converged, np.zeros(n, bool), selected)


def re_threshold(maps, ratio, mutant=None):
    m = np.array(maps, dtype=np.float64)
    k = m.shape[0]
    if ratio is not None:
        per = 100.0 - (k * ratio if mutant == 'percentile_k' else 100.0 / k * ratio)
        cut = scipy.stats.scoreatpercentile(np.abs(m).ravel(), per)
        m = np.where(np.abs(m) < cut, 0.0, m)
    for i in range(k):
        hi, lo = m[i].max(), m[i].min()
        if (hi > -lo) if mutant == 'sign_reversed' else (hi < -lo):
            m[i] = -m[i]
    return m


def agrees(a, b):
    """two IcaMaps of the same case: counts, flags and selection equal, W within W_TOL"""
    return (np.array_equal(np.asarray(a.n_iter), np.asarray(b.n_iter)) and np.array_equal(np.asarray(a.converged), np.asarray(b.converged))
            and a.selected == b.selected and bool(np.max(np.abs(np.asarray(a.W) - np.asarray(b.W))) <= W_TOL))


# ----------------------------------------------------------------------------------------------- layer 1: no GPU
@pytest.mark.parametrize('fun', sorted(FUNS))
@pytest.mark.parametrize('shape', sorted(CASES))
def test_the_twin_agrees_with_the_restatement(shape, fun):
    comp, w0 = CASES[shape]
    got, want = twin(shape, fun), re_fastica(comp, w0, fun)
    print(shape, fun, 'n_iter', got.n_iter, want.n_iter, 'max |dW|', np.max(np.abs(got.W - want.W)))
    assert not got.failed.any() and got.converged.all()
    assert agrees(got, want)
    assert np.max(np.abs(got.maps - want.maps)) <= W_TOL * np.abs(want.maps).max() * comp.shape[0]


@pytest.mark.parametrize('fun', sorted(FUNS))
@pytest.mark.parametrize('shape', sorted(CASES))
def test_the_measured_tolerance_holds_for_another_summation_order(shape, fun):
    """the measurement behind W_TOL: the twin on the voxels in reversed order stays within W_TOL / 100"""
    comp, w0 = CASES[shape]
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        rev = fastica_maps_host(np.ascontiguousarray(comp[:, ::-1]), fun=fun, tol=TOL, max_iter=60, w_init=w0)
    got = twin(shape, fun)
    print(shape, fun, 'max |dW| under reversal', np.max(np.abs(got.W - rev.W)))
    assert np.array_equal(got.n_iter, rev.n_iter) and got.selected == rev.selected
    assert np.max(np.abs(got.W - rev.W)) <= W_TOL / 100


def _pipeline(ica, ratio, mutant=None):
    return re_threshold(ica.maps, ratio, mutant)


@pytest.mark.parametrize('mutant', MUTANTS)
def test_the_judge_rejects_the_mutant(mutant):
    """every mutant of the restatement disagrees with the twin on at least one case (fun, or the thresholded maps)"""
    shape = (3, 600)
    comp, w0 = CASES[shape]
    rejected = False
    for fun in ('cube', 'logcosh'):
        if mutant == 'gp_y2' and fun != 'cube':
            continue
        got = twin(shape, fun)
        if mutant in ('percentile_k', 'sign_reversed'):
            # the sign rule is exercised on maps whose first row is negated: its larger side is then the negative one
            maps = got.maps * np.array([-1.0, 1.0, 1.0])[:, None]
            rejected |= not same_bits(threshold_maps_host(maps, 'auto'), re_threshold(maps, 1.0, mutant))
            assert same_bits(threshold_maps_host(maps, 'auto'), re_threshold(maps, 1.0))
        else:
            rejected |= not agrees(got, re_fastica(comp, w0, fun, max_iter=12, mutant=mutant))
        if rejected:
            break
    assert rejected


def _threshold_cases():
    rng = np.random.RandomState(3)
    a = np.round(rng.laplace(size=(4, 50)) * 4) / 4                      # a coarse grid: many ties, also at the cutoff
    b = a.copy()
    b[2] = 0                                                            # an all-zero map
    c = rng.randn(3, 41)
    c[1, 5], c[1, 6] = 7.0, -7.0                                        # max == -min: no flip
    c[0] = -np.abs(c[0])                                                # flips
    return {'ties': a, 'zero_map': b, 'max_equals_minus_min': c}


@pytest.mark.parametrize('name', sorted(_threshold_cases()))
@pytest.mark.parametrize('threshold', ['auto', 0.5, 2.0, None])
def test_threshold_maps_host_is_scipys_percentile_bit_for_bit(name, threshold):
    maps = _threshold_cases()[name]
    k = maps.shape[0]
    got = threshold_maps_host(maps, threshold)
    want = maps.copy()
    if threshold is not None:
        ratio = 1.0 if threshold == 'auto' else threshold
        cut = scipy.stats.scoreatpercentile(np.abs(maps), 100.0 - 100.0 / k * ratio)
        if name == 'ties' and threshold == 'auto':
            assert np.sum(np.abs(maps) == cut) > 1                      # the cutoff sits on a tie, and ties are kept
        want[np.abs(want) < cut] = 0
        assert np.all(np.abs(got[got != 0]) >= cut)
    for i in range(k):
        if want[i].max() < -want[i].min():
            want[i] = -want[i]
    assert same_bits(got, want)
    if name == 'max_equals_minus_min' and threshold is None:
        assert same_bits(got[1], maps[1]) and same_bits(got[0], -maps[0])
    assert same_bits(maps, _threshold_cases()[name])                    # the input is left alone


def svd_record(seed=0, T=12, V=500):
    """a record U diag(s) Vt with prescribed, separated singular values"""
    rng = np.random.RandomState(seed)
    Uq, _ = np.linalg.qr(rng.randn(T, T))
    Vq, _ = np.linalg.qr(rng.randn(V, T))
    s = np.array([12, 10, 8.5, 7, 6, 5, 4.2, 3.5, 3, 2.5, 2, 1.5])[:T]
    return (Uq * s) @ Vq.T, Uq, s, Vq.T


def check_reduced(got, Uq, s, Vt, k):
    V = Vt.shape[1]
    gap = np.min(np.abs(np.diff(s ** 2)))
    for i in range(k):
        sign = 1.0 if Uq[np.argmax(np.abs(Uq[:, i])), i] > 0 else -1.0
        err = np.max(np.abs(got[i] - sign * s[i] * Vt[i]))
        bound = 64 * V * U * s[0] ** 2 / gap * s[i]
        print('row', i, 'error', err, 'bound', bound)
        assert err <= bound


def test_reduce_record_host_recovers_prescribed_singular_vectors():
    rows, Uq, s, Vt = svd_record()
    got = reduce_record_host(rows, 5)
    assert got.shape == (5, 500) and got.dtype == np.float64
    check_reduced(got, Uq, s, Vt, 5)


def group_stack(seed=0, shape=PHANTOMS[0]):
    _, records = phantom(seed, *shape)
    return [reduce_record_host(r, shape[2]) for r in records]


def check_projector(comp, variance, reduced, k):
    X = np.concatenate(reduced)
    X = X / np.linalg.norm(X, axis=1, keepdims=True)
    _, s, Vt = np.linalg.svd(X, full_matrices=False)
    V = X.shape[1]
    bound = 64 * V * U * s[0] ** 2 / (s[k - 1] ** 2 - s[k] ** 2)
    err = np.max(np.abs(comp.T @ comp - Vt[:k].T @ Vt[:k]))
    print('projector error', err, 'bound', bound, 'gap', s[k - 1] ** 2 - s[k] ** 2)
    assert err <= bound
    assert np.max(np.abs(comp @ comp.T - np.eye(k))) <= 64 * V * U
    assert np.max(np.abs(np.sort(variance)[::-1] - s[:k] ** 2)) <= 64 * V * U * s[0] ** 2


def test_group_components_host_spans_the_top_subspace():
    reduced = group_stack()
    comp, variance = group_components_host(reduced, 3)
    assert comp.shape == (3, 600)
    check_projector(comp, variance, reduced, 3)
    zero = [reduced[0], np.zeros((1, 600))]                              # a zero row is left alone
    comp0, _ = group_components_host(zero, 3)
    assert np.all(np.isfinite(comp0))


def _fake():
    return C.c_void_p(4096)


def _sweep_rc(k=3, V=10, R=1, fun=0, ldx=None, ws_bytes=None, ws=True):
    need = lib.modl_ica_sweep_workspace(V, k, R)
    return lib.modl_ica_sweep_f64(_fake(), V if ldx is None else ldx, V, k, _fake(), _fake(), R, fun, 1.0, _fake(), _fake(),
                                  _fake() if ws else None, need if ws_bytes is None else ws_bytes, None)


def test_the_sweep_refuses_bad_arguments_before_any_device_work():
    kmax = lib.modl_ica_max_components()
    assert kmax >= 128
    assert lib.modl_ica_sweep_workspace(1000, 70, 10) >= 10 * (70 * 70 + 70) * 8
    for bad in (dict(k=0), dict(k=kmax + 1), dict(V=0), dict(R=0), dict(fun=3), dict(fun=-1), dict(ldx=9)):
        assert _sweep_rc(**bad) == EINVAL, bad
    assert _sweep_rc(ws_bytes=lib.modl_ica_sweep_workspace(10, 3, 1) - 1) == ENOMEM
    assert _sweep_rc(ws=False) == ENOMEM
    for bad in ((0, 3, 1), (10, 0, 1), (10, kmax + 1, 1), (10, 3, 0)):
        assert lib.modl_ica_sweep_workspace(*bad) == 0
    assert lib.modl_ica_sweep_f64(None, 10, 10, 3, _fake(), _fake(), 1, 0, 1.0, _fake(), _fake(), _fake(), 1 << 20, None) == EINVAL


def test_value_errors_name_the_offender():
    comp, w0 = CASES[(3, 600)]
    with pytest.raises(ValueError, match='n_components = 13'):
        reduce_record_host(np.zeros((12, 40)), 13)
    with pytest.raises(ValueError, match='n_components = 13'):
        reduce_record(np.zeros((12, 40)), 13)
    with pytest.raises(ValueError, match='n_components'):
        group_components_host([np.ones((2, 40))], 3)
    with pytest.raises(ValueError, match='one number of voxels'):
        group_components_host([np.ones((2, 40)), np.ones((2, 41))], 2)
    for f in (fastica_maps_host, fastica_maps):
        with pytest.raises(ValueError, match="'cube', 'logcosh' or 'exp'"):
            f(comp, fun='tanh', w_init=w0)
        with pytest.raises(ValueError, match='w_init must be'):
            f(comp, w_init=w0[:, :2])
        with pytest.raises(ValueError, match='n_init'):
            f(comp, n_init=0)
        with pytest.raises(ValueError, match='max_iter'):
            f(comp, max_iter=0, w_init=w0)
        with pytest.raises(ValueError, match='at most'):
            f(np.zeros((lib.modl_ica_max_components() + 1, 300)), w_init=None, n_init=1)
    with pytest.raises(ValueError, match='every restart'):
        fastica_maps_host(comp, w_init=np.full_like(w0, np.nan))
    with pytest.raises(ValueError, match='alpha'):                       # sklearn's own refusals are errors, not failed restarts
        fastica_maps_host(comp, fun='logcosh', alpha=3.0, w_init=w0)
    for f in (threshold_maps_host, threshold_maps):
        with pytest.raises(ValueError, match='threshold must'):
            f(comp, 'automatic')
        with pytest.raises(ValueError, match=r'\(0, 3\]'):
            f(comp, 3.5)
    for f in (canica_host, canica):
        with pytest.raises(ValueError, match='shortest record'):
            f([np.zeros((8, 50)), np.zeros((4, 50))], n_components=5)


def test_the_seeds_are_drawn_as_nilearn_and_sklearn_draw_them():
    comp, _ = CASES[(3, 600)]
    rs = np.random.RandomState(11)
    seeds = rs.randint(np.iinfo(np.int32).max, size=3)
    w0 = np.stack([np.random.RandomState(s).normal(size=(3, 3)) for s in seeds])
    a = fastica_maps_host(comp, n_init=3, random_state=11, return_all=True)
    b = fastica_maps_host(comp, w_init=w0, return_all=True)
    assert same_bits(a.W, b.W) and a.selected == b.selected and a.maps.shape == (3, 3, 600)
    assert same_bits(a.maps[a.selected], fastica_maps_host(comp, w_init=w0).maps)


def test_a_failed_restart_is_a_state_of_the_twin():
    comp, w0 = CASES[(3, 600)]
    bad = w0.copy()
    bad[1] = np.nan
    got, clean = fastica_maps_host(comp, w_init=bad), twin((3, 600), 'cube')
    assert got.failed.tolist() == [False, True, False, False] and got.n_iter[1] == 0 and np.all(np.isnan(got.W[1]))
    keep = [0, 2, 3]
    assert same_bits(got.W[keep], clean.W[keep]) and got.selected != 1


def _host_fmri():
    from .test_masker import _host_estimators
    return _host_estimators()[0]


def test_dict_init_canica_argument_checks_on_the_oracle_backend():
    est = _host_fmri()
    _, records = phantom(0, 200, 12, 3, 2)
    kw = dict(n_components=3, n_epochs=1, random_state=0, batch_size=6, alpha=0.1)
    with pytest.raises(ValueError, match="goes with dict_init = 'canica'"):
        est(dict_init_args=dict(n_init=2), **kw).fit(records)
    with pytest.raises(ValueError, match="goes with dict_init = 'canica'"):
        est(dict_init=records[0][:3], dict_init_args={}, **kw).fit(records)
    with pytest.raises(ValueError, match='dict_init_args must be'):
        est(dict_init='canica', dict_init_args=dict(restarts=2), **kw).fit(records)
    with pytest.raises(ValueError, match='dict_init_args must be'):
        est(dict_init='canica', dict_init_args=[2], **kw).fit(records)
    with pytest.raises(ValueError, match="'cube', 'logcosh' or 'exp'"):
        est(dict_init='canica', dict_init_args=dict(fun='tanh'), **kw).fit(records)
    with pytest.raises(ValueError, match='threshold must'):
        est(dict_init='canica', dict_init_args=dict(threshold=9), **kw).fit(records)
    short = est(dict_init='canica', **dict(kw, n_components=10))
    with pytest.raises(ValueError, match='time points of record 1'):
        short.fit([records[0], records[1][:9]])
    assert not hasattr(short, 'dict_fact_') and not hasattr(short, 'canica_')     # raised before any record is fitted
    rs_a, rs_b = np.random.RandomState(5), np.random.RandomState(5)
    a = est(dict_init=None, **dict(kw, random_state=rs_a)).fit(records)
    b = est(dict_init=None, dict_init_args=None, **dict(kw, random_state=rs_b)).fit(records)
    assert same_bits(a.components_, b.components_) and rs_a.randint(1 << 30) == rs_b.randint(1 << 30)
    assert not hasattr(a, 'canica_')


# ------------------------------------------------------------------------------------------------ layer 2: the GPU
class _NanWorkspace:
    """`need` bytes of NaN doubles between two guard blocks of NaN"""

    def __init__(self, need):
        import torch
        assert need > 0 and need % 8 == 0
        self.n = need // 8
        self.buf = torch.full((self.n + 64,), float('nan'), dtype=torch.float64, device='cuda')
        self.ptr = C.c_void_p(self.buf.data_ptr() + 32 * 8)

    def check(self):
        w = self.buf.cpu().numpy()
        assert np.all(np.isnan(w[:32])) and np.all(np.isnan(w[32 + self.n:]))


def abs_terms(W, X, fun, alpha):
    """per restart: (the sums of the absolute values of the terms of M (k, k) and of gp (k,), the exact-arithmetic M, gp)"""
    V = X.shape[1]
    y, A = W @ X, np.abs(W) @ np.abs(X)
    if fun == 'cube':
        g, d, ga, da = y ** 3, 3 * y ** 2, A ** 3, 3 * A ** 2
    elif fun == 'logcosh':
        g = np.tanh(alpha * y)
        d = alpha * (1 - g * g)
        ga, da = np.abs(g) + alpha * A, alpha * (1 + g * g) + 2 * alpha * alpha * np.abs(g) * A
    else:
        e = np.exp(-y * y / 2)
        g, d = y * e, (1 - y * y) * e
        ga, da = np.abs(g) + e * (1 + y * y) * A, (1 + y * y) * e + e * np.abs(y) * (3 + y * y) * A
    return ga @ np.abs(X).T / V, da.sum(axis=1) / V, g @ X.T / V, d.sum(axis=1) / V


def sweep_inputs(k, V, R, seed):
    """X (k, V), W (R + 2, k, k) of which restarts 1 and R + 1 are not listed, the list in descending order"""
    rng = np.random.RandomState(seed)
    X = rng.laplace(size=(k, V)) * (rng.rand(k, V) < 0.4) + 0.05 * rng.randn(k, V)
    W = rng.randn(R + 2, k, k) / np.sqrt(k)
    active = np.array([i for i in range(R + 2) if i not in (1, R + 1)][::-1], dtype=np.int32)
    return X, W, active


def run_sweep(torch, X, W, active, fun, alpha):
    """the C-ABI call: ldx = V + 5 with NaN after every row, guarded outputs, a NaN-poisoned workspace"""
    k, V = X.shape
    n, R = W.shape[0], len(active)
    ldx = V + 5
    Xp = np.full((k, ldx), np.nan)
    Xp[:, :V] = X
    dX = torch.full((GUARD + k * ldx + GUARD,), float('nan'), dtype=torch.float64, device='cuda')
    dX[GUARD:GUARD + k * ldx] = torch.from_numpy(Xp.ravel()).cuda()
    dW, dA = torch.from_numpy(np.ascontiguousarray(W)).cuda(), torch.from_numpy(active).cuda()
    M, gp = _Guarded(n * k * k, torch.float64, -777.25), _Guarded(n * k, torch.float64, -777.25)
    need = lib.modl_ica_sweep_workspace(V, k, R)
    ws = _NanWorkspace(need)
    rc = lib.modl_ica_sweep_f64(C.c_void_p(dX.data_ptr() + GUARD * 8), ldx, V, k, C.c_void_p(dW.data_ptr()), C.c_void_p(dA.data_ptr()),
                                R, FUNS[fun], alpha, M.ptr, gp.ptr, ws.ptr, need, None)
    assert rc == 0
    torch.cuda.synchronize()
    ws.check()
    return M.get().reshape(n, k, k), gp.get().reshape(n, k)


def sweep_shapes():
    kmax = lib.modl_ica_max_components()
    return [(1, 1, 1, 'cube'), (1, 64, 3, 'exp'), (3, 63, 3, 'logcosh'), (16, 64, 1, 'exp'), (16, 1000, 10, 'logcosh'),
            (17, 65, 3, 'cube'), (17, 65, 3, 'logcosh'), (17, 65, 3, 'exp'), (70, 1000, 10, 'cube'), (70, 4099, 3, 'exp'),
            (kmax, 4099, 10, 'cube'), (kmax, 4099, 10, 'logcosh'), (kmax, 4099, 10, 'exp'), (kmax, 63, 1, 'cube')]


@pytest.mark.gpu
@pytest.mark.parametrize('k,V,R,fun', sweep_shapes())
def test_gpu_sweep_through_the_c_abi(gpu, k, V, R, fun):
    alpha = 1.5 if fun == 'logcosh' else 1.0
    X, W, active = sweep_inputs(k, V, R, 1000 * k + V + R)
    M, gp = run_sweep(gpu, X, W, active, fun, alpha)
    M2, gp2 = run_sweep(gpu, X, W, active, fun, alpha)
    assert same_bits(M, M2) and same_bits(gp, gp2)                      # the same bits from run to run
    c = (8 * (V + k) + ULP[fun]) * U
    worst = 0.0
    for r in range(R + 2):
        if r not in active:
            assert np.all(M[r] == -777.25) and np.all(gp[r] == -777.25)  # unlisted: the slots keep their poison
            continue
        Ma, gpa, Mw, gpw = abs_terms(W[r], X, fun, alpha)
        assert np.all(np.abs(M[r] - Mw) <= c * Ma) and np.all(np.abs(gp[r] - gpw) <= c * gpa)
        worst = max(worst, np.max(np.abs(M[r] - Mw) / (c * Ma)), np.max(np.abs(gp[r] - gpw) / (c * gpa)))
    print('largest error / bound', worst)


@pytest.mark.gpu
@pytest.mark.parametrize('k,fun', [(17, 'cube'), (70, 'exp'), (70, 'logcosh')])
def test_gpu_a_restart_has_the_same_bits_whoever_is_listed_with_it(gpu, k, fun):
    """V = 4099 is cut into many chunks: a restart swept in a list of 3 and in a list of 10 gives the same bits, in any order
    of the list - the chunking, and with it the order of a restart's partial sums, depends on V alone"""
    V = 4099
    X, W, _ = sweep_inputs(k, V, 10, 77 + k)                           # 12 matrices
    ten = np.array([0, 2, 3, 4, 5, 6, 7, 8, 9, 10], dtype=np.int32)
    three = np.array([9, 3, 6], dtype=np.int32)
    one = np.array([6], dtype=np.int32)
    assert lib.modl_ica_sweep_workspace(V, k, 10) == 10 * lib.modl_ica_sweep_workspace(V, k, 1)
    assert lib.modl_ica_sweep_workspace(V, k, 1) > 8 * (k * k + k) * 8      # more than eight chunks
    M10, gp10 = run_sweep(gpu, X, W, ten, fun, 1.25)
    for listed in (three, one):
        M, gp = run_sweep(gpu, X, W, listed, fun, 1.25)
        for r in listed:
            assert same_bits(M[r], M10[r]) and same_bits(gp[r], gp10[r]), (listed, r)
        assert np.all(M[[r for r in range(12) if r not in listed]] == -777.25)


@pytest.mark.gpu
def test_gpu_sweep_error_returns(gpu):
    torch = gpu
    k, V, R = 3, 40, 2
    X = torch.zeros((k, V), dtype=torch.float64, device='cuda')
    W = torch.zeros((R, k, k), dtype=torch.float64, device='cuda')
    act = torch.arange(R, dtype=torch.int32, device='cuda')
    M, gp = _Guarded(R * k * k, torch.float64, -777.25), _Guarded(R * k, torch.float64, -777.25)
    need = lib.modl_ica_sweep_workspace(V, k, R)
    ws = _NanWorkspace(need)
    p = lambda t: C.c_void_p(t.data_ptr())

    def call(k=k, V=V, R=R, fun=0, ldx=V, ws_bytes=need, wsp=ws.ptr):
        return lib.modl_ica_sweep_f64(p(X), ldx, V, k, p(W), p(act), R, fun, 1.0, M.ptr, gp.ptr, wsp, ws_bytes, None)
    kmax = lib.modl_ica_max_components()
    for bad in (dict(k=0), dict(k=kmax + 1), dict(V=0), dict(R=0), dict(fun=3), dict(ldx=V - 1)):
        assert call(**bad) == EINVAL, bad
    assert call(ws_bytes=need - 8) == ENOMEM and call(wsp=None) == ENOMEM
    torch.cuda.synchronize()
    assert np.all(M.get() == -777.25) and np.all(gp.get() == -777.25)   # a refused call writes nothing
    assert call() == 0
    torch.cuda.synchronize()
    assert np.all(M.get() == 0) and np.all(gp.get() == 0)               # cube of zeros


def _np(x):
    return x.cpu().numpy() if hasattr(x, 'cpu') else np.asarray(x)


@pytest.mark.gpu
@pytest.mark.parametrize('fun', sorted(FUNS))
@pytest.mark.parametrize('shape', sorted(CASES))
@pytest.mark.parametrize('cuda', [False, True])
def test_gpu_fastica_maps_equals_the_twin(gpu, shape, fun, cuda):
    comp, w0 = CASES[shape]
    want = twin(shape, fun)
    got = fastica_maps(gpu.from_numpy(comp).cuda() if cuda else comp, fun=fun, tol=TOL, max_iter=60, w_init=w0)
    assert isinstance(got.maps, gpu.Tensor if cuda else np.ndarray)
    host = IcaMaps(_np(got.maps), _np(got.W), _np(got.n_iter), _np(got.converged), _np(got.failed), got.selected)
    print(shape, fun, 'n_iter', host.n_iter, want.n_iter, 'max |dW|', np.max(np.abs(host.W - want.W)))
    assert not host.failed.any()
    assert agrees(host, want)
    assert np.max(np.abs(host.maps - want.maps)) <= W_TOL * np.abs(want.maps).max() * comp.shape[0]


@pytest.mark.gpu
def test_gpu_a_nan_restart_fails_alone(gpu):
    comp, w0 = CASES[(3, 600)]
    bad = w0.copy()
    bad[1] = np.nan
    clean = fastica_maps(comp, w_init=w0, return_all=True)
    got = fastica_maps(comp, w_init=bad, return_all=True)
    assert got.failed.tolist() == [False, True, False, False] and not clean.failed.any()
    keep = [0, 2, 3]
    assert same_bits(got.W[keep], clean.W[keep]) and np.all(np.isnan(got.W[1])) and np.all(np.isnan(got.maps[1]))
    assert same_bits(got.maps[keep], clean.maps[keep]) and np.array_equal(got.n_iter[keep], clean.n_iter[keep])
    l1 = np.abs(clean.maps[keep]).sum(axis=2).max(axis=1)
    assert got.selected == keep[int(np.argmin(l1))]                     # the selection ignores restart 1
    with pytest.raises(ValueError, match='every restart'):
        fastica_maps(comp, w_init=np.full_like(w0, np.nan))


@pytest.mark.gpu
@pytest.mark.parametrize('cuda', [False, True])
def test_gpu_reduce_group_threshold_equal_their_twins(gpu, cuda):
    give = (lambda a: gpu.from_numpy(np.ascontiguousarray(a)).cuda()) if cuda else (lambda a: a)
    rows, Uq, s, Vt = svd_record()
    got = reduce_record(give(rows), 5)
    assert isinstance(got, gpu.Tensor if cuda else np.ndarray) and tuple(got.shape) == (5, 500)
    check_reduced(_np(got), Uq, s, Vt, 5)
    rows32 = rows.astype(np.float32)                                    # a float32 record: accumulated in f64 all the same
    check_reduced(_np(reduce_record(give(rows32), 5)), *_svd_of(rows32), 5)
    for shape in PHANTOMS:
        reduced = group_stack(0, shape)
        comp, variance = group_components([give(r) for r in reduced], shape[2])
        assert isinstance(comp, gpu.Tensor if cuda else np.ndarray)
        check_projector(_np(comp), _np(variance), reduced, shape[2])
    for name, maps in sorted(_threshold_cases().items()):
        for threshold in ('auto', 0.5, 2.0, None):
            out = threshold_maps(give(maps), threshold)
            assert isinstance(out, gpu.Tensor if cuda else np.ndarray)
            assert same_bits(_np(out), threshold_maps_host(maps, threshold)), (name, threshold)
    big = twin((5, 1500), 'cube').maps
    assert same_bits(_np(threshold_maps(give(big), 'auto')), threshold_maps_host(big, 'auto'))


def _svd_of(rows):
    """the f64 SVD of a record as (U, s, Vt): the yardstick of a float32 record, whose spectrum is no longer the prescribed one"""
    Uq, s, Vt = np.linalg.svd(rows.astype(np.float64), full_matrices=False)
    return Uq, s, Vt


@pytest.mark.gpu
@pytest.mark.parametrize('seed', range(4))
@pytest.mark.parametrize('shape', PHANTOMS)
def test_gpu_canica_recovers_planted_maps(gpu, shape, seed):
    planted, records = phantom(seed, *shape)
    kw = dict(n_components=shape[2], n_init=10, threshold=None, fun='cube', random_state=seed)
    host = canica_host(records, **kw)
    c_host = matched_correlations(planted, host.maps)
    print('twin  ', shape, seed, c_host)
    assert c_host.min() >= 0.97                                         # the precondition
    got = canica(records, **kw)
    c_dev = matched_correlations(planted, got.maps)
    print('device', shape, seed, c_dev)
    assert isinstance(got.maps, np.ndarray) and got.maps.shape == planted.shape and got.variance.shape == (shape[2],)
    assert not got.ica.failed.any()
    assert c_dev.min() >= 0.97
    if seed == 0:                                                       # CUDA tensors in, CUDA tensors out, the same bits
        dev = canica([gpu.from_numpy(r).cuda() for r in records], **kw)
        assert isinstance(dev.maps, gpu.Tensor) and same_bits(_np(dev.maps), got.maps)


@pytest.mark.gpu
def test_gpu_fmri_dict_fact_starts_from_canica(gpu):
    from modl_amd.fmri import fMRIDictFact
    _, records = phantom(0, 1500, 30, 5, 2)
    flat = np.zeros(16 * 10 * 10, dtype=bool)
    flat[:1500] = True
    mask = np.random.RandomState(1).permutation(flat).reshape(16, 10, 10)
    assert mask.sum() == 1500
    kw = dict(n_components=5, n_epochs=2, batch_size=10, alpha=0.1, mask=mask)
    a = fMRIDictFact(dict_init='canica', random_state=3, **kw).fit(records)
    b = fMRIDictFact(dict_init='canica', random_state=3, **kw).fit(records)
    plain = fMRIDictFact(dict_init=None, random_state=3, **kw).fit(records)
    assert isinstance(a.canica_, Canica) and tuple(a.canica_.maps.shape) == (5, 1500) and not hasattr(plain, 'canica_')
    assert all(isinstance(x, np.ndarray) for x in (a.canica_.maps, a.canica_.variance) + tuple(a.canica_.ica[:5]))   # numpy, as the rest
    assert a.components_.shape == (5, 1500) and a.components_img_.shape == (16, 10, 10, 5)
    assert same_bits(a.components_, b.components_)
    s_canica, s_plain = a.score(records), plain.score(records)
    print('score from canica', s_canica, 'from dict_init=None', s_plain)
    assert np.isfinite(s_canica) and s_canica <= s_plain
    rs_a, rs_b = np.random.RandomState(5), np.random.RandomState(5)
    p = fMRIDictFact(dict_init=None, random_state=rs_a, **kw).fit(records)
    q = fMRIDictFact(dict_init=None, dict_init_args=None, random_state=rs_b, **kw).fit(records)
    assert same_bits(p.components_, q.components_) and rs_a.randint(1 << 30) == rs_b.randint(1 << 30)
    few = fMRIDictFact(dict_init='canica', dict_init_args=dict(n_init=3, threshold=None, fun='logcosh', tol=1e-3, max_iter=100),
                       random_state=3, **kw).fit(records)
    assert _np(few.canica_.ica.n_iter).shape == (3,) and few.components_.shape == (5, 1500)
