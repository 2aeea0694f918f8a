"""Signal cleaning of fMRI records: cleaning_basis / clean of modl_amd/signal.py, modl_clean_* of
csrc/clean.hip, and the `standardize` / `detrend` / `confounds` of fMRIDictFact, fMRICoder and rfMRIDictionaryScorer.
nilearn is not available, so nothing is pinned to a run of nilearn.signal.clean: its semantics (linear detrending,
confound regression, z-scoring) are judged against scipy.

Layer 1 (no GPU): this file's own f64 restatement of the projection and the host path `clean_host` are compared with
scipy.signal.detrend, scipy.stats.zscore(ddof=0) and lstsq residuals (<= 1e-11 max-abs); the basis is orthonormal with
the expected number of columns; the judge the GPU tests use rejects planted mutants of a correct answer; argument errors
are raised without a device; the estimators' wiring is checked on the oracle-backed host backend.

The judge, per element:  |got - ref| <= eps_out |ref| + q T eps64 |x_col| s_col,  ref the f64 restatement on the same
input values, s_col = sqrt(T) / |r_col| when standardizing and 1 otherwise: the second term is the worst-case f64
rounding of the projection (q dot products and q updates of length T on a column of norm |x_col|), scaled like the
output; the first is the one rounding on store.  A column that the restatement finds flat must be exact zeros, a column
that holds a NaN / Inf must be NaN throughout.

Layer 2 (GPU): the kernel through the ABI on shapes around the split of T over the four wavefronts, the four rows a
wavefront has in flight and the 64 columns of a workgroup with a q for every instantiated width, adversarial columns, the slice / permutation / run-to-run bit
contracts, `clean()` and the estimators."""
import ctypes as C

import numpy as np
import pytest
import scipy.linalg
import scipy.signal
import scipy.stats

EPS64 = float(np.finfo(np.float64).eps)
DT = {'f32': np.float32, 'f64': np.float64}
EINVAL, ENOMEM, ENOGPU = -1, -2, -4
SENT = -777.25                                   # what the padding and untouched outputs hold
PAD = 3
SHAPES = [(1, 1), (2, 5), (3, 63), (37, 65), (130, 257), (257, 1030)]
QS = (1, 2, 5, 9, 13, 17, 21, 26, 30, 33, 40, 48, 49, 64)      # every instantiated width of the kernel: 4, 8, ..., 32, 48, 64


# ------------------------------------------------------------------------------------------- the restatement (numpy)
def _unit(v):
    return v / np.linalg.norm(v)


def restate_basis(T, detrend, standardize, confounds, skip=None):
    """steps 1 of the semantics, column by column (modified Gram-Schmidt, twice); skip: a confound left out (mutant)"""
    cols = [np.full(T, 1 / np.sqrt(T))]
    ramp = np.arange(T) - (T - 1) / 2
    if detrend and np.linalg.norm(ramp) > 0:
        cols.append(_unit(ramp))

    def residual(v, basis):
        for _ in range(2):
            for b in basis:
                v = v - b * b.dot(v)
        return v
    if confounds is not None:
        conf = np.asarray(confounds, dtype=np.float64)
        conf = conf - conf.mean(axis=0)
        kept = []
        for j in range(conf.shape[1]):
            if j == skip:
                continue
            r = residual(conf[:, j], cols)
            if np.linalg.norm(r) > 100 * EPS64 * np.sqrt(T) * np.linalg.norm(conf[:, j]):
                kept.append(_unit(r))
        if kept:
            Qc, R, _ = scipy.linalg.qr(np.column_stack(kept), mode='economic', pivoting=True)
            for j in range(Qc.shape[1]):
                if abs(R[j, j]) > 100 * EPS64:
                    cols.append(_unit(residual(Qc[:, j], cols)))
    if not (detrend or standardize):
        cols = cols[1:]
    return np.column_stack(cols) if cols else np.zeros((T, 0))


def restate_clean(X, Q, standardize, ddof=0, zero_flat=True):
    """steps 2 and 3 in f64: (out, flat columns, |r| per column)"""
    T, q = Q.shape
    x = np.asarray(X, dtype=np.float64)
    with np.errstate(all='ignore'):
        r = x - Q @ (Q.T @ x)
        rn = np.sqrt(np.sum(r * r, axis=0))
        flat = np.zeros(x.shape[1], dtype=bool)
        if standardize:
            flat = rn ** 2 <= (q * T * EPS64) ** 2 * np.sum(x * x, axis=0)
            r = r * (np.sqrt(T - ddof) / rn)
            if zero_flat:
                r[:, flat] = 0.0
    return r, flat, rn


def judge(got, X, Q, standardize, eps_out):
    """list of the columns of `got` that the judge of the module docstring rejects"""
    T, q = Q.shape
    ref, flat, rn = restate_clean(X, Q, standardize)
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape
    xn = np.sqrt(np.sum(np.asarray(X, dtype=np.float64) ** 2, axis=0))
    bad = []
    for j in range(ref.shape[1]):
        if not np.all(np.isfinite(np.asarray(X)[:, j])):
            ok = bool(np.all(np.isnan(got[:, j])))
        elif flat[j]:
            ok = bool(np.all(got[:, j] == 0))
        else:
            s = np.sqrt(T) / rn[j] if standardize else 1.0
            ok = bool(np.all(np.abs(got[:, j] - ref[:, j]) <= eps_out * np.abs(ref[:, j]) + q * T * EPS64 * xn[j] * s))
        if not ok:
            bad.append(j)
    return bad


def random_basis(T, q, seed):
    """q orthonormal columns: constant, ramp (T > 1), then random directions"""
    rs = np.random.RandomState(seed)
    A = np.column_stack([np.ones(T), np.arange(T) - (T - 1) / 2, rs.randn(T, max(q, 2))])[:, :max(q, 2)]
    if T == 1:
        return np.ones((1, 1))
    Qf, _ = np.linalg.qr(A)
    return np.ascontiguousarray(Qf[:, :q])


def bold(T, V, dtype, seed):
    rs = np.random.RandomState(seed)
    return (100 + 3 * rs.randn(T, V)).astype(dtype)


def confound_set(T, seed=3):
    """three independent columns, a duplicate of the second and one equal to the ramp (up to scale and offset)"""
    c3 = np.random.RandomState(seed).randn(T, 3)
    return np.column_stack([c3, c3[:, 1], 2.0 * np.arange(T) + 5])


# ------------------------------------------------------------------------------------------------ layer 1: no GPU
def _judges(X, conf):
    det = lambda a: scipy.signal.detrend(a, axis=0)
    z = lambda a: scipy.stats.zscore(a, axis=0, ddof=0)
    res = lambda a, c: a - c @ np.linalg.lstsq(c, a, rcond=None)[0]
    cc = conf - conf.mean(axis=0)
    return [((True, False, None), det(X)),
            ((False, True, None), z(X)),
            ((True, True, None), z(det(X))),
            ((True, False, conf), res(det(X), det(conf))),
            ((True, True, conf), z(res(det(X), det(conf)))),
            ((False, False, conf), res(X, cc)),
            ((False, True, conf), z(res(X - X.mean(axis=0), cc)))]


def test_restatement_and_host_path_against_scipy():
    from modl_amd.signal import clean_host, cleaning_basis
    T, V = 37, 9
    X = bold(T, V, np.float64, 0)
    conf = confound_set(T)
    for (detrend, standardize, c), want in _judges(X, conf):
        Q = restate_basis(T, detrend, standardize, c)
        assert Q.shape[1] == {(1, 0): 5, (1, 1): 5, (0, 0): 4, (0, 1): 5}[(detrend, standardize)] if c is not None \
            else Q.shape[1] == 1 + detrend
        assert cleaning_basis(T, detrend, standardize, c).shape == Q.shape
        mine = restate_clean(X, Q, standardize)[0]
        host = clean_host(X, detrend, standardize, c)
        print(detrend, standardize, c is not None, np.abs(mine - want).max(), np.abs(host - want).max())
        assert np.abs(mine - want).max() <= 1e-11
        assert np.abs(host - want).max() <= 1e-11
    # the record's mean survives a confounds-only cleaning
    assert np.allclose(clean_host(X, False, False, conf).mean(axis=0), X.mean(axis=0), rtol=1e-12)


def test_basis():
    from modl_amd.signal import cleaning_basis
    from modl_amd._lib import lib
    assert lib.modl_clean_max_regressors() == 64
    for T in (1, 2, 3, 37):
        conf = confound_set(T)
        for detrend in (False, True):
            for standardize in (False, True):
                for c in (None, conf, np.full((T, 2), 3.7)):
                    Q = cleaning_basis(T, detrend, standardize, c)
                    assert Q.dtype == np.float64 and Q.shape[0] == T
                    q = Q.shape[1]
                    assert np.abs(Q.T @ Q - np.eye(q)).max() <= 1e-14 if q else True
                    base = min(T, 1 + detrend) if (detrend or standardize) else 0
                    if c is None or c is not conf:               # all-constant confounds add nothing
                        assert q == base, (T, detrend, standardize)
                    elif T == 37:
                        assert q == (5 if (detrend or standardize) else 4)
                    else:
                        assert q <= T
                    assert q == restate_basis(T, detrend, standardize, c).shape[1]
    rs = np.random.RandomState(1)
    with pytest.raises(ValueError):
        cleaning_basis(100, True, True, rs.randn(100, 70))
    assert cleaning_basis(100, True, True, rs.randn(100, 62)).shape == (100, 64)
    # the span is what matters: the projector equals the restatement's
    Q, Qr = cleaning_basis(37, True, True, confound_set(37)), restate_basis(37, True, True, confound_set(37))
    assert np.abs(Q @ Q.T - Qr @ Qr.T).max() <= 1e-13


def test_confounds_from_files(tmp_path):
    from modl_amd.signal import clean_host
    X, conf = bold(20, 4, np.float64, 2), np.random.RandomState(5).randn(20, 2)
    np.save(str(tmp_path / 'c.npy'), conf)
    np.savetxt(str(tmp_path / 'c.csv'), conf, delimiter=',')
    want = clean_host(X, True, True, conf)
    assert np.array_equal(clean_host(X, True, True, str(tmp_path / 'c.npy')), want)
    assert np.abs(clean_host(X, True, True, str(tmp_path / 'c.csv')) - want).max() <= 1e-12


def _mutant_case(dtype):
    """a record with a flat column (constant 10000) at index 2, its confounds and the correct answer in `dtype`"""
    T, V = 40, 6
    X = bold(T, V, dtype, 7)
    X[:, 2] = 10000
    conf = confound_set(T)[:, :3]
    Q = restate_basis(T, True, True, conf)
    ref = restate_clean(X, Q, True)[0].astype(dtype)
    return X, conf, Q, ref


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_judge_rejects_mutants(dt):
    dtype = DT[dt]
    eps_out = float(np.finfo(dtype).eps)
    X, conf, Q, ref = _mutant_case(dtype)
    T = X.shape[0]
    assert judge(ref, X, Q, True, eps_out) == []
    mutants = {}
    Qm = restate_basis(T, False, True, conf)                                     # ramp not removed
    mutants['ramp_kept'] = restate_clean(X, Qm, True)[0]
    mutants['ddof1'] = restate_clean(X, Q, True, ddof=1)[0]
    mutants['confound_skipped'] = restate_clean(X, restate_basis(T, True, True, conf, skip=1), True)[0]
    mutants['flat_not_zeroed'] = restate_clean(X, Q, True, zero_flat=False)[0]
    m = ref.copy()
    m[:, 4] = 0
    mutants['standardized_zeroed'] = m
    m = ref.copy()
    m[[5, 17]] = m[[17, 5]]
    mutants['rows_swapped'] = m
    m = ref.copy()
    m[:, 3] = ref[:, 4]
    mutants['column_shifted'] = m
    for name, got in mutants.items():
        assert judge(np.asarray(got).astype(dtype), X, Q, True, eps_out) != [], name
    # without standardization: the ramp, a skipped confound, swapped rows
    Qn = restate_basis(T, True, False, conf)
    refn = restate_clean(X, Qn, False)[0].astype(dtype)
    assert judge(refn, X, Qn, False, eps_out) == []
    assert judge(restate_clean(X, restate_basis(T, False, False, conf), False)[0], X, Qn, False, eps_out) != []
    assert judge(restate_clean(X, restate_basis(T, True, False, conf, skip=0), False)[0], X, Qn, False, eps_out) != []
    m = refn.copy()
    m[[0, 1]] = m[[1, 0]]
    assert judge(m, X, Qn, False, eps_out) != []


def test_flat_rule_figures():
    """the two figures of the flat rule: a constant f32 column of 10000 (q = 64, T = 1200) is under the threshold, the
    same column with one element moved by one f32 ulp is over it"""
    T, q = 1200, 64
    Q = random_basis(T, q, 0)
    x = np.full((T, 1), 10000, dtype=np.float32)
    thr = q * T * EPS64
    _, flat, rn = restate_clean(x, Q, True)
    assert flat[0] and rn[0] / np.linalg.norm(x.astype(np.float64)) < thr
    x[7, 0] = np.nextafter(np.float32(10000), np.float32(np.inf))
    out, flat, rn = restate_clean(x, Q, True)
    assert not flat[0] and rn[0] / np.linalg.norm(x.astype(np.float64)) > thr
    assert abs(out.var() - 1) < 1e-6


def test_clean_argument_errors_without_a_device():
    from modl_amd.signal import clean, clean_host
    X = bold(10, 4, np.float32, 0)
    for f in (clean, clean_host):
        with pytest.raises(ValueError):
            f(X[0])                                                         # rank
        with pytest.raises(ValueError):
            f(X, confounds=np.zeros((9, 2)))                                # T mismatch
        with pytest.raises(ValueError):
            f(X, confounds=np.zeros((10, 2, 2)))                            # rank of the confounds
        bad = np.random.RandomState(0).randn(10, 2)
        bad[3, 1] = np.nan
        with pytest.raises(ValueError):
            f(X, confounds=bad)
        with pytest.raises(ValueError):
            f(bold(100, 4, np.float32, 0), confounds=np.random.RandomState(0).randn(100, 70))
        for perm in ([0] * 10, np.arange(9), np.arange(10) + 1, np.arange(10.0)):
            with pytest.raises(ValueError):
                f(X, permutation=perm)
        with pytest.raises(ValueError):
            f(X, permutation=np.arange(10)[::-1], out=X)                    # out aliases the input
        with pytest.raises(ValueError):
            f(X, out=np.zeros((10, 5), dtype=np.float32))
    # nothing asked: the input itself
    assert clean(X, detrend=False, standardize=False) is X
    # host path: permutation and out
    perm = np.random.RandomState(1).permutation(10)
    want = clean_host(X)
    assert np.array_equal(clean_host(X, permutation=perm), want[perm])
    buf = np.empty_like(X)
    assert clean_host(X, out=buf) is buf and np.array_equal(buf, want)
    Y = X.copy()
    assert clean_host(Y, out=Y) is Y and np.array_equal(Y, want)


def _bad_calls(T, V, ld, q):
    """(name, overrides of the good call's arguments, expected code)"""
    return [('null X', dict(X=None), EINVAL), ('null Q', dict(Q=None), EINVAL), ('null out', dict(out=None), EINVAL),
            ('q = 0', dict(q=0), EINVAL), ('q > T', dict(q=T + 1), EINVAL), ('q > 64', dict(q=65, T=100), EINVAL),
            ('ldx < V', dict(ldx=V - 1), EINVAL), ('ldo < V', dict(ldo=V - 1), EINVAL), ('T = 0', dict(T=0), EINVAL),
            ('V = 0', dict(V=0), EINVAL), ('in place with rows', dict(out='X'), EINVAL),
            ('in place, other ld', dict(out='X', dst=None, ldo=ld + 1), EINVAL),
            ('out overlaps X, a row further', dict(out='X+row', dst=None), EINVAL),
            ('out overlaps X, with rows', dict(out='X+row'), EINVAL),
            ('null ws', dict(ws=None), ENOMEM), ('small ws', dict(ws_bytes='short'), ENOMEM)]


def _call_clean(lib, sx, a):
    vp = lambda v: C.c_void_p(v) if v else C.c_void_p(0)
    return getattr(lib, 'modl_clean_' + sx)(vp(a['X']), a['ldx'], a['T'], a['V'], vp(a['Q']), a['q'], 1, vp(a['dst']),
                                            vp(a['out']), a['ldo'], vp(a['ws']), a['ws_bytes'], None)


def _bad_call_args(lib, dt, ptrs, T, V, ld, q, over):
    need = lib.modl_clean_workspace(0 if dt == 'f32' else 1, T, V, q)
    a = dict(X=ptrs['X'], ldx=ld, T=T, V=V, Q=ptrs['Q'], q=q, dst=ptrs['dst'], out=ptrs['out'], ldo=ld, ws=ptrs['ws'],
             ws_bytes=need)
    a.update(over)
    if a['out'] == 'X':
        a['out'] = a['X']
    if a['out'] == 'X+row':
        a['out'] = a['X'] + ld * (4 if dt == 'f32' else 8)
    if a['ws_bytes'] == 'short':
        a['ws_bytes'] = need - 1
    return a


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_entry_points_refuse_bad_arguments_without_a_device(dt):
    from modl_amd._lib import lib
    T, V, ld, q = 12, 7, 9, 3
    bufs = dict(X=np.zeros((T, ld), DT[dt]), Q=np.zeros((T, q)), dst=np.arange(T, dtype=np.int64),
                out=np.zeros((T, ld), DT[dt]), ws=np.zeros(T * 64))
    ptrs = {k: v.ctypes.data for k, v in bufs.items()}
    assert lib.modl_clean_workspace(0, T, V, q) >= T * q * 8
    for args in ((7, T, V, q), (0, 0, V, q), (0, T, 0, q), (0, T, V, 0), (0, T, V, 65), (0, 3, V, 4)):
        assert lib.modl_clean_workspace(*args) == 0
    for name, over, code in _bad_calls(T, V, ld, q):
        assert _call_clean(lib, dt, _bad_call_args(lib, dt, ptrs, T, V, ld, q, over)) == code, name
    if lib.modl_device_count() == 0:
        assert _call_clean(lib, dt, _bad_call_args(lib, dt, ptrs, T, V, ld, q, {})) == ENOGPU


def _fmri_case(dtype=np.float64):
    rs = np.random.RandomState(11)
    recs = [(100 + 3 * rs.randn(n, 96)).astype(dtype) for n in (40, 33)]
    confs = [rs.randn(n, 3) for n in (40, 33)]
    kw = dict(n_components=4, n_epochs=1, random_state=0, batch_size=10, alpha=0.1, reduction=2)
    return recs, confs, kw


def _check_estimators(fMRIDictFact, fMRICoder, cleaner, dtype):
    """the wiring: cleaning inside the estimators (flags on, confounds passed) equals handing over records cleaned by
    `cleaner` with the flags off, bit for bit - fit (the permutation folded in), transform, score, coder, scorer"""
    from modl_amd.fmri import rfMRIDictionaryScorer
    recs, confs, kw = _fmri_case(dtype)
    pre = [cleaner(r, True, True, c) for r, c in zip(recs, confs)]
    on = fMRIDictFact(standardize=True, detrend=True, **kw).fit(recs, confounds=confs)
    off = fMRIDictFact(**kw).fit(pre)
    assert np.array_equal(on.components_, off.components_)
    assert not np.array_equal(on.components_, fMRIDictFact(**kw).fit(recs).components_)
    for a, b in zip(on.transform(recs, confounds=confs), off.transform(pre)):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    assert on.score(recs, confounds=confs) == off.score(pre)
    # confounds only, one record without any
    pre_c = [cleaner(recs[0], False, False, confs[0]), recs[1]]
    on_c = fMRIDictFact(**kw).fit(recs, confounds=[confs[0], None])
    assert np.array_equal(on_c.components_, fMRIDictFact(**kw).fit(pre_c).components_)
    # flags off, no confounds: the path as it was
    plain = fMRIDictFact(**kw).fit(recs)
    assert np.array_equal(plain.components_, fMRIDictFact(standardize=False, detrend=False, **kw).fit(
        recs, confounds=[None, None]).components_)
    assert plain.score(recs) == plain.score(recs, confounds=None)
    # the coder
    c_on = fMRICoder(on.components_, alpha=0.1, standardize=True, detrend=True).fit()
    c_off = fMRICoder(on.components_, alpha=0.1).fit()
    for a, b in zip(c_on.transform(recs, confounds=confs), c_off.transform(pre)):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    assert c_on.score(recs, confounds=confs) == c_off.score(pre)
    assert np.array_equal(c_on.transform(recs[0], confounds=confs[0])[0], c_off.transform(pre[0])[0])
    # the scorer: flags from its first argument, test_confounds live
    s_on, s_off = rfMRIDictionaryScorer(recs, test_confounds=confs), rfMRIDictionaryScorer(pre)
    s_on(on, on.dict_fact_, 0.0, 0.0)
    s_off(off, off.dict_fact_, 0.0, 0.0)
    assert s_on.score == s_off.score
    with pytest.raises(ValueError):
        on.fit(recs, confounds=confs[:1])


def test_estimators_clean_records_host_logic():
    from modl_amd.fmri import fMRICoder
    from modl_amd.signal import clean_host
    from .test_wrappers import _fmri_estimator, _host_classes

    class HostfMRICoder(fMRICoder):
        _coder_class = _host_classes()[1]
    _check_estimators(_fmri_estimator(True), HostfMRICoder, clean_host, np.float64)


# ------------------------------------------------------------------------------------------------ layer 2: the GPU
@pytest.fixture(scope='module')
def gpu():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    return torch


def gpu_clean(X, Q, standardize, dst=None, inplace=False):
    """modl_clean_* on X padded to ld = V + PAD with sentinels: the (T, V) result; asserts that the padding of the output
    is untouched and, out of place, the input too"""
    import torch
    from modl_amd._lib import lib, check
    from modl_amd.device import ptr
    T, V = X.shape
    q = Q.shape[1]
    sx = 'f32' if X.dtype == np.float32 else 'f64'
    host = np.full((T, V + PAD), SENT, dtype=X.dtype)
    host[:, :V] = X
    d_X = torch.from_numpy(host).to('cuda')
    d_out = d_X if inplace else torch.full((T, V + PAD), SENT, dtype=d_X.dtype, device='cuda')
    d_Q = torch.from_numpy(np.ascontiguousarray(Q, dtype=np.float64)).to('cuda')
    d_dst = None if dst is None else torch.from_numpy(np.ascontiguousarray(dst, dtype=np.int64)).to('cuda')
    need = lib.modl_clean_workspace(0 if sx == 'f32' else 1, T, V, q)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    check(getattr(lib, 'modl_clean_' + sx)(ptr(d_X), V + PAD, T, V, ptr(d_Q), q, int(standardize), ptr(d_dst), ptr(d_out),
                                           V + PAD, ptr(ws), need, None), 'modl_clean')
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert np.all(out[:, V:] == SENT)
    if not inplace:
        assert np.array_equal(d_X.cpu().numpy(), host, equal_nan=True)
    return np.ascontiguousarray(out[:, :V])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_clean_through_the_abi(gpu, dt, shape):
    T, V = shape
    dtype, eps_out = DT[dt], float(np.finfo(DT[dt]).eps)
    X = bold(T, V, dtype, 100 + T)
    perm = np.random.RandomState(T).permutation(T)
    dst = np.empty(T, dtype=np.int64)
    dst[perm] = np.arange(T)
    for q in [q for q in QS if q <= T]:
        Q = random_basis(T, q, q)
        for standardize in (False, True):
            plain = gpu_clean(X, Q, standardize)
            assert judge(plain, X, Q, standardize, eps_out) == [], (q, standardize)
            assert same_bits(gpu_clean(X, Q, standardize, inplace=True), plain), (q, standardize)
            assert same_bits(gpu_clean(X, Q, standardize, dst=dst), plain[perm]), (q, standardize)


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_adversarial_columns(gpu, dt):
    dtype, eps_out = DT[dt], float(np.finfo(DT[dt]).eps)
    T = 130
    rs = np.random.RandomState(4)
    conf = rs.randn(T, 3).astype(np.float32).astype(np.float64)              # exact in f32: a column can EQUAL a confound
    Q = restate_basis(T, True, True, conf)
    assert Q.shape[1] == 5
    X = bold(T, 70, dtype, 5)
    X[:, 0] = 10000                                                          # constant
    X[:, 1] = 0                                                              # zeros
    X[:, 2] = 10000
    X[17, 2] = np.nextafter(np.float32(10000), np.float32(np.inf))           # constant but for one f32 ulp (one f64 ulp
    #                                                                          is below the rounding of the projection)
    X[:, 3] = (0.25 * np.arange(T) - 3).astype(dtype)                        # a ramp (exact in f32)
    X[:, 4] = conf[:, 1].astype(dtype)                                       # a confound
    X[:, 5] = (1e4 + rs.randn(T)).astype(dtype)                              # BOLD-like: mean 1e4, unit noise
    X[:, 66] = X[:, 5]                                                       # ... and in the second wavefront block
    out = gpu_clean(X, Q, True)
    _, flat, _ = restate_clean(X, Q, True)
    assert list(np.flatnonzero(flat)) == [0, 1, 3, 4]
    assert judge(out, X, Q, True, eps_out) == []
    for j in (0, 1, 3, 4):
        assert np.all(out[:, j] == 0), j
    assert abs(out[:, 2].astype(np.float64).var() - 1) < 1e-5 and abs(out[:, 5].astype(np.float64).var() - 1) < 1e-5
    assert same_bits(out[:, 5], out[:, 66])
    plain = gpu_clean(X, Q, False)
    assert judge(plain, X, Q, False, eps_out) == []
    assert np.all(plain[:, 1] == 0) and np.all(np.abs(plain[:, 0]) < 1e-6)   # nothing is zeroed, nothing is large


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_non_finite_columns_stay_in_their_column(gpu, dt):
    dtype, eps_out = DT[dt], float(np.finfo(DT[dt]).eps)
    T, V = 37, 130
    X = bold(T, V, dtype, 8)
    Q = random_basis(T, 5, 2)
    for standardize in (False, True):
        want = gpu_clean(X, Q, standardize)
        Y = X.copy()
        Y[3, 7] = np.nan
        Y[30, 64] = np.inf
        got = gpu_clean(Y, Q, standardize)
        assert judge(got, Y, Q, standardize, eps_out) == []
        assert np.all(np.isnan(got[:, 7])) and np.all(np.isnan(got[:, 64]))
        others = np.setdiff1d(np.arange(V), [7, 64])
        assert same_bits(got[:, others], want[:, others])


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_slice_permutation_and_rerun_bits(gpu, dt):
    import torch
    from modl_amd.signal import clean, cleaning_basis
    T, V = 130, 257
    X = bold(T, V, DT[dt], 9)
    conf = np.random.RandomState(2).randn(T, 4)
    perm = np.random.RandomState(3).permutation(T)
    d_X = torch.from_numpy(X).to('cuda')
    full = clean(d_X, confounds=conf)
    assert full.is_cuda and same_bits(full.cpu().numpy(), clean(d_X, confounds=conf).cpu().numpy())
    assert same_bits(clean(d_X[:, 3:200], confounds=conf).cpu().numpy(), full[:, 3:200].cpu().numpy())
    assert same_bits(clean(d_X, confounds=conf, permutation=perm).cpu().numpy(), full.cpu().numpy()[perm])
    # numpy in, numpy out; both agree with the ABI result
    Q = cleaning_basis(T, True, True, conf)
    abi = gpu_clean(X, Q, True)
    host_in = clean(X, confounds=conf)
    assert isinstance(host_in, np.ndarray) and same_bits(host_in, abi) and same_bits(full.cpu().numpy(), abi)
    # out: a fresh buffer, in place, and the q = 0 short cut
    buf = torch.empty_like(d_X)
    assert clean(d_X, confounds=conf, out=buf) is buf and same_bits(buf.cpu().numpy(), abi)
    work = d_X.clone()
    assert clean(work, confounds=conf, out=work) is work and same_bits(work.cpu().numpy(), abi)
    assert clean(d_X, detrend=False, standardize=False) is d_X
    with pytest.raises(ValueError):
        clean(d_X, permutation=perm, out=d_X)
    with pytest.raises(ValueError):
        clean(d_X, out=d_X[:, :200])
    assert same_bits(d_X.cpu().numpy(), X)


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_entry_points_refuse_bad_arguments(gpu, dt):
    import torch
    from modl_amd._lib import lib
    T, V, ld, q = 12, 7, 9, 3
    tdt = torch.float32 if dt == 'f32' else torch.float64
    bufs = dict(X=torch.full((T, ld), 1.5, dtype=tdt, device='cuda'),
                Q=torch.from_numpy(random_basis(T, q, 0)).to('cuda'),
                dst=torch.arange(T, dtype=torch.int64, device='cuda'),
                out=torch.full((T, ld), SENT, dtype=tdt, device='cuda'),
                ws=torch.zeros(T * 64, dtype=torch.float64, device='cuda'))
    ptrs = {k: v.data_ptr() for k, v in bufs.items()}
    for name, over, code in _bad_calls(T, V, ld, q):
        assert _call_clean(lib, dt, _bad_call_args(lib, dt, ptrs, T, V, ld, q, over)) == code, name
    torch.cuda.synchronize()
    assert bool((bufs['out'] == SENT).all()) and bool((bufs['X'] == 1.5).all())


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_estimators_clean_records_on_the_device(gpu, dt):
    from modl_amd.fmri import fMRICoder, fMRIDictFact
    from modl_amd.signal import clean
    _check_estimators(fMRIDictFact, fMRICoder, clean, DT[dt])
