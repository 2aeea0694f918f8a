"""Temporal filtering of fMRI records: butterworth_coefficients / butterworth / the `low_pass`,
`high_pass`, `t_r` of clean, clean_host and cleaning_basis (modl_amd/signal.py), modl_filtfilt_* of csrc/filtfilt.hip, and
the same arguments of fMRIDictFact, fMRICoder and rfMRIDictionaryScorer.  nilearn is not available, so nothing is pinned
to a run of nilearn.signal.clean: its semantics (current releases: detrend, filter signals and confounds alike, regress,
z-score) are judged against scipy.signal.

The restatement is a plain direct-form-II-transposed filtfilt (odd extension of 3 n_taps, zi scaled by the first sample,
forwards and backwards), run in f64 and in np.longdouble.  Per case (a filter, a T, a set of columns)

    e_case = max over the columns of  max_t |f64 restatement - longdouble restatement| / max|x_col|,
             floored at n_taps (T + 2 padlen) eps64

(the floor is the unamplified rounding of the recurrences; what is above it is the conditioning of the ba form; a single
column's figure is a draw - on the 1030 columns of a case it spreads over a decade - so the case's worst is the measure),
and the judge accepts an element if

    |got - ref| <= n_store eps_out |ref| + 8 e_case max|x_col|,        ref the longdouble restatement,

n_store = 1 for the kernel (one rounding on store) and 2 for the filtered `clean` (temporary plus result).  The factor 8:
fused multiply-adds and another operation order change WHICH roundings happen, not how many; the planted mutants sit many
orders above it.  Where longdouble is no wider than f64, e_case is measured as the change of the f64 restatement under a
relative 1-ulp perturbation of the input, and ref is the f64 restatement.  An all-zero column must be exact zeros, a
column with a NaN / Inf must be NaN throughout.

The n_store = 2 model of the filtered `clean` (each of the two roundings relative to the element itself) is applied in
f64, where both roundings are far below the second term.  In f32 it cannot hold for a temporary of the signals' dtype:
the temporary's rounding is eps32 |F[t]| / 2 of the FILTERED value, and the projection (the mean, the confounds) moves
small elements, so that |ref[t]| is no measure of |F[t]| any more - emulated on the host (f64 filtfilt rounded to f32,
f64 projection rounded to f32; T = 64, V = 257) between 76 and 257 of 257 columns hold an element outside the model for
every filter and flag combination with a non-empty Q2.  There the filtered `clean` is pinned differently and more
sharply: its bits equal those of clean(butterworth(X), basis=Q2), whose two halves are judged on their own (here with
n_store = 1, and in test_clean.py).  That bit identity is asserted for both dtypes and every case.

All figures use the t_r = 2 s filters: in the ba form a band 0.01 - 0.1 Hz at t_r = 0.72 s is conditioned up to 3e-7
(relative to max|x|, f64 against longdouble, in scipy and nilearn alike - §21)."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.signal
import scipy.stats

from .test_clean import SENT, PAD, DT, EINVAL, ENOMEM, ENOGPU, _judges, bold, confound_set, restate_basis, same_bits

EPS64 = float(np.finfo(np.float64).eps)
LD = np.longdouble
WIDE = float(np.finfo(LD).eps) < EPS64            # is longdouble wider than f64 here
T_R = 2.0
# name -> (filter arguments, taps); the kernel's widths are 2, 4, 6, 8, 12 taps
FILTERS = {'hp1': (dict(high_pass=0.01, order=1), 2), 'lp2': (dict(low_pass=0.1, order=2), 3),
           'band2': (dict(high_pass=0.01, low_pass=0.1, order=2), 5), 'lp5': (dict(low_pass=0.1, order=5), 6),
           'hp5': (dict(high_pass=0.01, order=5), 6), 'band3': (dict(high_pass=0.01, low_pass=0.1, order=3), 7),
           'band5': (dict(high_pass=0.01, low_pass=0.1, order=5), 11)}
VS = (1, 63, 65, 257, 1030)


def coefficients(name):
    kw, taps = FILTERS[name]
    nyq = 0.5 / T_R
    lo, hi, order = kw.get('low_pass'), kw.get('high_pass'), kw['order']
    if lo is not None and hi is not None:
        b, a = scipy.signal.butter(order, [hi / nyq, lo / nyq], 'band')
    elif hi is not None:
        b, a = scipy.signal.butter(order, hi / nyq, 'high')
    else:
        b, a = scipy.signal.butter(order, lo / nyq, 'low')
    assert len(b) == taps and a[0] == 1
    return b, a, scipy.signal.lfilter_zi(b, a)


def clean_kwargs(name):
    kw = dict(FILTERS[name][0])
    return dict(low_pass=kw.get('low_pass'), high_pass=kw.get('high_pass'), t_r=T_R, filter_order=kw['order'])


# ------------------------------------------------------------------------------------------- the restatement
def restate_detrend(x):
    """x minus its least-squares line, in the dtype of x"""
    dt = x.dtype.type
    T = x.shape[0]
    tc = np.arange(T).astype(dt) - dt(T - 1) / dt(2)
    x = x - x.sum(axis=0) / dt(T)
    if T > 1:
        x = x - tc[:, None] * ((tc[:, None] * x).sum(axis=0) / (tc * tc).sum())
    return x


def _lfilter(b, a, sig, z):
    """direct form II transposed over axis 0 from the state z (n_taps - 1, V)"""
    n = len(b)
    z = z.copy()
    y = np.empty_like(sig)
    for t in range(sig.shape[0]):
        x = sig[t]
        y[t] = b[0] * x + z[0]
        for i in range(n - 2):
            z[i] = b[i + 1] * x + z[i + 1] - a[i + 1] * y[t]
        z[n - 2] = b[n - 1] * x - a[n - 1] * y[t]
    return y


def restate_filtfilt(coef, X, dtype=np.float64, detrend=False, mutant=None):
    """filtfilt of every column of X (T, V) in `dtype`; mutant: one planted fault"""
    b, a, zi = (np.asarray(c).astype(dtype) for c in coef)
    if mutant == 'b_reversed':
        b = b[::-1].copy()
    x = np.asarray(X).astype(dtype)
    if detrend:
        x = restate_detrend(x)
    two = dtype(2)
    pad = 3 * len(b) + (1 if mutant == 'padlen_plus_one' else 0)
    assert x.shape[0] > pad
    if mutant == 'even_extension':
        ext = np.concatenate([x[pad:0:-1], x, x[-2:-pad - 2:-1]])
    else:
        ext = np.concatenate([two * x[0] - x[pad:0:-1], x, two * x[-1] - x[-2:-pad - 2:-1]])
    first = np.ones_like(ext[0]) if mutant == 'zi_not_scaled' else ext[0]
    fwd = _lfilter(b, a, ext, zi[:, None] * first)
    if mutant == 'forward_only':
        return fwd[pad:-pad]
    rev = fwd[::-1]
    start = np.zeros_like(rev[0]) if mutant == 'backward_state_zero' else rev[0]
    return _lfilter(b, a, rev, zi[:, None] * start)[::-1][pad:-pad]


def reference(coef, X, detrend):
    """(ref, e): the reference (longdouble where it is wider) and e_case, the worst column's figure, once per column"""
    X = np.asarray(X, dtype=np.float64)
    T, n = X.shape[0], len(coef[0])
    f64 = restate_filtfilt(coef, X, np.float64, detrend)
    if WIDE:
        ref = restate_filtfilt(coef, X, LD, detrend)
        diff = np.abs(f64.astype(LD) - ref).max(axis=0).astype(np.float64)
    else:
        sign = np.where(np.random.RandomState(0).rand(*X.shape) < 0.5, -1.0, 1.0)
        ref = f64
        diff = np.abs(restate_filtfilt(coef, X * (1 + EPS64 * sign), np.float64, detrend) - f64).max(axis=0)
    xmax = np.abs(X).max(axis=0)
    with np.errstate(invalid='ignore', divide='ignore'):
        e = np.where(xmax > 0, diff / xmax, 0.0)
    return ref, np.full(X.shape[1], max(float(e.max()), n * (T + 6 * n) * EPS64))


def judge(got, ref, X, e_col, eps_out, n_store=1, factor=8.0):
    """list of the columns of `got` that the judge of the module docstring rejects"""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape
    X = np.asarray(X, dtype=np.float64)
    bad = []
    for j in range(ref.shape[1]):
        if not np.all(np.isfinite(X[:, j])):
            ok = bool(np.all(np.isnan(got[:, j])))
        elif not np.any(X[:, j]):
            ok = bool(np.all(got[:, j] == 0))
        else:
            r = ref[:, j]
            tol = n_store * eps_out * np.abs(r) + factor * e_col[j] * np.abs(X[:, j]).max()
            ok = bool(np.all(np.abs(got[:, j].astype(r.dtype) - r) <= tol))
            if not ok:
                print('judge: column %d, worst |got - ref| / tol = %.3g' % (j, float((np.abs(got[:, j].astype(r.dtype) - r) / tol).max())))
        if not ok:
            bad.append(j)
    return bad


@functools.lru_cache(maxsize=None)
def case(name, T, detrend):
    """the shared case of a filter and a T: (X as f32-exact f64 (T, 1030), ref, e_col); never written to"""
    X = bold(T, VS[-1], np.float32, 1000 + T).astype(np.float64)
    ref, e = reference(coefficients(name), X, detrend)
    for arr in (X, ref, e):
        arr.setflags(write=False)
    return X, ref, e


def lengths(name):
    pad = 3 * FILTERS[name][1]
    return (pad + 1, pad + 2, 64, 257)


# ------------------------------------------------------------------------------------------------ layer 1: no GPU
def test_coefficients_and_their_errors():
    from modl_amd.signal import butterworth_coefficients, butterworth, clean_host, cleaning_basis
    from modl_amd._lib import lib
    assert lib.modl_filtfilt_max_taps() == 12
    for name in FILTERS:
        kw = clean_kwargs(name)
        got = butterworth_coefficients(T_R, kw['low_pass'], kw['high_pass'], kw['filter_order'])
        for g, w in zip(got, coefficients(name)):
            assert g.dtype == np.float64 and np.array_equal(g, w), name
    assert len(butterworth_coefficients(T_R, high_pass=0.01)[0]) == 6                # order 5 is the default
    bad = [dict(t_r=None, high_pass=0.01), dict(t_r=0.0, high_pass=0.01), dict(t_r=-2.0, low_pass=0.1),
           dict(t_r=T_R), dict(t_r=T_R, high_pass=0.0), dict(t_r=T_R, high_pass=-0.01), dict(t_r=T_R, low_pass=0.25),
           dict(t_r=T_R, low_pass=0.3), dict(t_r=T_R, high_pass=0.1, low_pass=0.1), dict(t_r=T_R, high_pass=0.2, low_pass=0.1),
           dict(t_r=T_R, high_pass=0.01, order=0), dict(t_r=T_R, high_pass=0.01, order=12),
           dict(t_r=T_R, high_pass=0.01, low_pass=0.1, order=6)]
    for kw in bad:
        with pytest.raises(ValueError):
            butterworth_coefficients(**kw)
    assert len(butterworth_coefficients(T_R, high_pass=0.01, order=11)[0]) == 12
    X = bold(40, 3, np.float64, 0)
    for f in (clean_host, lambda x, **kw: cleaning_basis(x.shape[0], **kw)):
        with pytest.raises(ValueError):
            f(X, high_pass=0.01)                                                 # a filter without t_r
        with pytest.raises(ValueError):
            f(X, high_pass=0.3, t_r=T_R)
        with pytest.raises(ValueError):
            f(X[:18], high_pass=0.01, t_r=T_R)                                   # T <= padlen = 18
        f(X[:19], high_pass=0.01, t_r=T_R)
    with pytest.raises(ValueError):
        butterworth(X, T_R)
    with pytest.raises(ValueError):
        butterworth(X[:18], T_R, high_pass=0.01)


def test_restatement_against_scipy_filtfilt():
    for name in FILTERS:
        coef = coefficients(name)
        for T in lengths(name)[:3]:
            X, ref, e = case(name, T, False)
            X, ref, e = X[:, :9], ref[:, :9], e[:9]
            want = scipy.signal.filtfilt(coef[0], coef[1], X, axis=0)
            assert judge(want, ref, X, e, 0.0) == [], (name, T)
            assert judge(restate_filtfilt(coef, X), ref, X, e, 0.0) == [], (name, T)


def test_conditioning_figures():
    """the table of §21: scipy's f64 filtfilt against the longdouble restatement, relative to max|x|, on detrended BOLD-like
    columns - small for the t_r = 2 filters that the tests use, up to 3e-7 for the order-5 band at t_r = 0.72.  The figures
    depend on the draw, so each bound is a decade above the table's figure."""
    if not WIDE:
        return                                               # (needs a longdouble wider than f64)
    worst = {}
    for key, t_r, lo, hi, bound in (('hp', 2.0, None, 0.01, 7e-12), ('lp', 2.0, 0.1, None, 5e-16),
                                    ('band', 2.0, 0.1, 0.01, 2e-11), ('band072', 0.72, 0.1, 0.01, 3e-7)):
        from modl_amd.signal import butterworth_coefficients
        coef = butterworth_coefficients(t_r, lo, hi)
        w = 0.0
        for T in (3 * len(coef[0]) + 1, 64, 130, 257):
            X = scipy.signal.detrend(bold(T, 8, np.float64, T), axis=0)
            ref = restate_filtfilt(coef, X, LD)
            got = scipy.signal.filtfilt(coef[0], coef[1], X, axis=0)
            w = max(w, float((np.abs(got - ref).max(axis=0) / np.abs(X).max(axis=0)).max()))
        print(key, w)
        worst[key] = w
        assert w <= 10 * bound, (key, w)
    assert worst['band072'] > 100 * worst['band']            # the conditioning is the method's, and it is the t_r


def _drop_null(conf_f, conf):
    return conf_f[:, np.linalg.norm(conf_f, axis=0) > np.sqrt(EPS64) * np.linalg.norm(conf, axis=0)]


def composition(X, conf, detrend, standardize, coef):
    """the three steps written out with scipy: detrend -> filtfilt on signals and confounds -> lstsq residual -> zscore"""
    det = lambda v: scipy.signal.detrend(v, axis=0)
    filt = lambda v: scipy.signal.filtfilt(coef[0], coef[1], v, axis=0)
    A = filt(det(X) if detrend else X)
    if conf is not None:
        Cf = _drop_null(filt(det(conf) if detrend else conf), conf)
        cc = Cf - Cf.mean(axis=0)
        if standardize:
            A = A - A.mean(axis=0)
        A = A - cc @ np.linalg.lstsq(cc, A, rcond=None)[0]
    return scipy.stats.zscore(A, axis=0, ddof=0) if standardize else A


def test_host_path_against_the_written_out_composition():
    """clean_host with a filter against scipy's detrend / filtfilt / lstsq / zscore for every flag combination of
    test_clean._judges (plus the bare filter) and every kind of filter: two f64 routes through the same filtfilt.
    Measured: worst max-abs difference 2.45e-10 (the order-5 band with detrend, values of size 3: scipy's detrend and the
    closed-form line differ by rounding, which the band's conditioning of 2e-11 max|x| carries on; 7e-11 for the
    high-pass, 9e-14 for the low-pass).  The bound is a decade above."""
    from modl_amd.signal import clean_host
    T, V = 64, 9
    X = bold(T, V, np.float64, 0)
    conf = confound_set(T)
    worst = 0.0
    for name in ('hp5', 'lp5', 'band5', 'hp1'):
        coef = coefficients(name)
        flags = [f for f, _ in _judges(X, conf)] + [(False, False, None)]
        for detrend, standardize, c in flags:
            want = composition(X, c, detrend, standardize, coef)
            got = clean_host(X, detrend, standardize, c, **clean_kwargs(name))
            d = float(np.abs(got - want).max())
            print(name, detrend, standardize, c is not None, d)
            worst = max(worst, d)
    print('worst', worst)
    assert worst <= 2.5e-9
    # permutation, out, basis and dtype on the host path
    kw = clean_kwargs('hp5')
    perm = np.random.RandomState(1).permutation(T)
    want = clean_host(X, True, True, conf, **kw)
    assert np.array_equal(clean_host(X, True, True, conf, permutation=perm, **kw), want[perm])
    from modl_amd.signal import cleaning_basis
    Q2 = cleaning_basis(T, True, True, conf, **kw)
    assert Q2.shape == (T, 4)                        # constant + three confounds: the duplicate and the ramp are gone
    assert np.array_equal(clean_host(X, True, True, basis=Q2, **kw), want)
    buf = np.empty_like(X)
    assert clean_host(X, True, True, conf, out=buf, **kw) is buf and np.array_equal(buf, want)
    X32 = X.astype(np.float32)
    got32 = clean_host(X32, True, True, conf, **kw)
    assert got32.dtype == np.float32 and np.abs(got32 - clean_host(X32.astype(np.float64), True, True, conf, **kw)).max() < 1e-6
    # without a filter nothing changes
    assert np.array_equal(clean_host(X, True, True, conf), clean_host(X, True, True, conf, low_pass=None, high_pass=None,
                                                                      t_r=T_R))


def restate_filtered_clean(X, conf, detrend, standardize, coef, filter_confounds=True):
    """the filtered clean in longdouble (where wider): steps 1-2 by the restatement, the basis Q2 by test_clean's
    restate_basis from the f64-filtered confounds, the projection and the scaling in longdouble"""
    dt = LD if WIDE else np.float64
    F = restate_filtfilt(coef, X, dt, detrend)
    Cf = None
    if conf is not None:
        Cf = restate_filtfilt(coef, conf, np.float64, detrend) if filter_confounds else np.asarray(conf, dtype=np.float64)
        Cf = _drop_null(Cf, conf)
    Q = restate_basis(X.shape[0], False, standardize, Cf).astype(dt)
    if Q.shape[1] == 0:
        return F
    r = F - Q @ (Q.T @ F)
    if standardize:
        r = r * (np.sqrt(dt(X.shape[0])) / np.sqrt((r * r).sum(axis=0)))
    return r


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_judge_rejects_mutants(dt):
    dtype, eps_out = DT[dt], float(np.finfo(DT[dt]).eps)
    for name in ('hp5', 'lp5', 'band5', 'hp1'):
        coef = coefficients(name)
        T = 64
        X, ref, e = case(name, T, False)
        X, ref, e = X[:, :6], ref[:, :6], e[:6]
        assert judge(ref.astype(dtype), ref, X, e, eps_out) == []
        for mutant in ('even_extension', 'padlen_plus_one', 'zi_not_scaled', 'backward_state_zero', 'forward_only',
                       'b_reversed'):
            if mutant == 'b_reversed' and np.allclose(coef[0], coef[0][::-1], rtol=1e-9, atol=0):
                continue                                                 # a low-pass: b is a palindrome, no mutant
            got = restate_filtfilt(coef, X, np.float64, mutant=mutant).astype(dtype)
            assert len(judge(got, ref, X, e, eps_out)) == X.shape[1], (name, mutant)
    # the filtered clean: confounds left unfiltered
    T = 64
    X = bold(T, 6, dtype, 3)
    conf = confound_set(T)[:, :3]
    coef = coefficients('hp5')
    for standardize in (False, True):
        ref = restate_filtered_clean(X, conf, True, standardize, coef)
        _, e = reference(coef, X, True)
        assert judge(ref.astype(dtype), ref, X, e, eps_out, n_store=2) == []
        got = restate_filtered_clean(X, conf, True, standardize, coef, filter_confounds=False).astype(dtype)
        assert len(judge(got, ref, X, e, eps_out, n_store=2)) == X.shape[1], standardize


def _bad_calls(T, V, ld, n):
    """(name, overrides of the good call's arguments, expected code)"""
    return [('null X', dict(X=None), EINVAL), ('null out', dict(out=None), EINVAL), ('null b', dict(b=None), EINVAL),
            ('null a', dict(a=None), EINVAL), ('null zi', dict(zi=None), EINVAL), ('1 tap', dict(n=1), EINVAL),
            ('13 taps', dict(n=13, T=100), EINVAL), ('a[0] != 1', dict(a=('set', 0, 2.0)), EINVAL),
            ('nan in b', dict(b=('set', 1, np.nan)), EINVAL), ('inf in a', dict(a=('set', 2, np.inf)), EINVAL),
            ('nan in zi', dict(zi=('set', 0, np.nan)), EINVAL), ('T = padlen', dict(T=3 * n), EINVAL),
            ('V = 0', dict(V=0), EINVAL), ('ldx < V', dict(ldx=V - 1), EINVAL), ('ldo < V', dict(ldo=V - 1), EINVAL),
            ('in place with rows', dict(out='X'), EINVAL), ('in place, other ld', dict(out='X', dst=None, ldo=ld + 1), EINVAL),
            ('out overlaps X, a row further', dict(out='X+row', dst=None), EINVAL),
            ('null ws', dict(ws=None), ENOMEM), ('small ws', dict(ws_bytes='short'), ENOMEM),
            ('bad pointer and no workspace', dict(X=None, ws=None), EINVAL)]


def _call_filtfilt(lib, dt, ptrs, coef, T, V, ld, over):
    """the good call (d_dst_row given, out of place) with `over` applied"""
    n = len(coef[0])
    a = dict(X=ptrs['X'], ldx=ld, T=T, V=V, b=coef[0].copy(), a=coef[1].copy(), zi=coef[2].copy(), n=n, dst=ptrs['dst'],
             out=ptrs['out'], ldo=ld, ws=ptrs['ws'])
    a['ws_bytes'] = lib.modl_filtfilt_workspace(0 if dt == 'f32' else 1, T, V, n)
    for k, v in over.items():
        if isinstance(v, tuple) and v[0] == 'set':
            a[k][v[1]] = v[2]
        else:
            a[k] = v
    if isinstance(a['out'], str):
        a['out'] = a['X'] + (ld * (4 if dt == 'f32' else 8) if a['out'] == 'X+row' else 0)
    if a['ws_bytes'] == 'short':
        a['ws_bytes'] = lib.modl_filtfilt_workspace(0 if dt == 'f32' else 1, T, V, n) - 1
    vp = lambda v: C.c_void_p(v) if v else C.c_void_p(0)
    hp = lambda v: None if v is None else v.ctypes.data
    return getattr(lib, 'modl_filtfilt_' + dt)(vp(a['X']), a['ldx'], a['T'], a['V'], hp(a['b']), hp(a['a']), hp(a['zi']),
                                               a['n'], 1, vp(a['dst']), vp(a['out']), a['ldo'], vp(a['ws']), a['ws_bytes'],
                                               None)


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_entry_points_refuse_bad_arguments_without_a_device(dt):
    from modl_amd._lib import lib
    coef = coefficients('band2')
    T, V, ld, n = 20, 7, 9, 5
    assert lib.modl_filtfilt_workspace(0, T, V, n) == (T + 3 * n) * V * 8 == lib.modl_filtfilt_workspace(1, T, V, n)
    assert lib.modl_filtfilt_workspace(0, 37, 1, 12) == (37 + 36) * 8
    for args in ((7, T, V, n), (0, 3 * n, V, n), (0, T, 0, n), (0, T, V, 1), (0, 100, V, 13), (0, -1, V, n)):
        assert lib.modl_filtfilt_workspace(*args) == 0, args
    bufs = dict(X=np.zeros((T, ld), DT[dt]), dst=np.arange(T, dtype=np.int64), out=np.zeros((T, ld), DT[dt]),
                ws=np.zeros((T + 3 * n) * V))
    ptrs = {k: v.ctypes.data for k, v in bufs.items()}
    for name, over, code in _bad_calls(T, V, ld, n):
        assert _call_filtfilt(lib, dt, ptrs, coef, T, V, ld, over) == code, name
    if lib.modl_device_count() == 0:
        assert _call_filtfilt(lib, dt, ptrs, coef, T, V, ld, {}) == ENOGPU
        assert _call_filtfilt(lib, dt, ptrs, coef, T, V, ld, dict(ws=None)) == ENOMEM          # ENOMEM before ENOGPU


def _fmri_case(dtype=np.float64):
    rs = np.random.RandomState(11)
    recs = [(100 + 3 * rs.randn(n, 96)).astype(dtype) for n in (40, 33)]
    confs = [rs.randn(n, 3) for n in (40, 33)]
    kw = dict(n_components=4, n_epochs=2, random_state=0, batch_size=10, alpha=0.1, reduction=2)
    return recs, confs, kw


def _check_estimators(fMRIDictFact, fMRICoder, cleaner, dtype):
    """the wiring: filtering inside the estimators equals handing over records cleaned by `cleaner` with everything off,
    bit for bit - fit (the permutation folded in, the per-record basis kept over the epochs), transform, score, coder,
    scorer"""
    from modl_amd.fmri import rfMRIDictionaryScorer
    recs, confs, kw = _fmri_case(dtype)
    filt = dict(high_pass=0.01, t_r=T_R)
    pre = [cleaner(r, True, True, c, **filt) for r, c in zip(recs, confs)]
    on = fMRIDictFact(standardize=True, detrend=True, **filt, **kw).fit(recs, confounds=confs)
    off = fMRIDictFact(**kw).fit(pre)
    assert np.array_equal(on.components_, off.components_)
    assert not np.array_equal(on.components_, fMRIDictFact(standardize=True, detrend=True, **kw).fit(
        recs, confounds=confs).components_)
    for a, b in zip(on.transform(recs, confounds=confs), off.transform(pre)):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    assert on.score(recs, confounds=confs) == off.score(pre)
    # the filter alone (nothing left to project: the filter launch carries the permutation), as a band
    band = dict(high_pass=0.01, low_pass=0.1, t_r=T_R)
    long_recs = [np.concatenate([r, r[::-1]]) for r in recs]                 # a band of order 5 needs T > 33
    pre_b = [cleaner(r, False, False, None, **band) for r in long_recs]
    on_b = fMRIDictFact(**band, **kw).fit(long_recs)
    assert np.array_equal(on_b.components_, fMRIDictFact(**kw).fit(pre_b).components_)
    assert not np.array_equal(on_b.components_, fMRIDictFact(**kw).fit(long_recs).components_)
    # the coder
    c_on = fMRICoder(on.components_, alpha=0.1, standardize=True, detrend=True, **filt).fit()
    c_off = fMRICoder(on.components_, alpha=0.1).fit()
    for a, b in zip(c_on.transform(recs, confounds=confs), c_off.transform(pre)):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    assert c_on.score(recs, confounds=confs) == c_off.score(pre)
    # the scorer: the filter from its first argument
    s_on, s_off = rfMRIDictionaryScorer(recs, test_confounds=confs), rfMRIDictionaryScorer(pre)
    s_on(on, on.dict_fact_, 0.0, 0.0)
    s_off(off, off.dict_fact_, 0.0, 0.0)
    assert s_on.score == s_off.score
    with pytest.raises(ValueError):
        fMRIDictFact(high_pass=0.01, **kw).fit(recs)                         # no t_r
    with pytest.raises(ValueError):
        fMRIDictFact(**band, **kw).fit(recs)                                 # 33 time points: too short for the band


def test_estimators_filter_records_host_logic():
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


def gpu_filtfilt(X, coef, detrend, dst=None, inplace=False):
    """modl_filtfilt_* on X padded to ld = V + PAD with sentinels: the (T, V) result; asserts that the padding of the
    output is untouched and, out of place, the input too"""
    import torch
    from modl_amd._lib import lib, check
    from modl_amd.device import ptr
    T, V = X.shape
    b, a, zi = (np.ascontiguousarray(c, dtype=np.float64) for c in coef)
    sx = 'f32' if X.dtype == np.float32 else 'f64'
    host = np.full((T, V + PAD), SENT, dtype=X.dtype)
    host[:, :V] = X
    d_X = torch.from_numpy(host).to('cuda')
    d_out = d_X if inplace else torch.full((T, V + PAD), SENT, dtype=d_X.dtype, device='cuda')
    d_dst = None if dst is None else torch.from_numpy(np.ascontiguousarray(dst, dtype=np.int64)).to('cuda')
    need = lib.modl_filtfilt_workspace(0 if sx == 'f32' else 1, T, V, len(b))
    assert need == (T + 3 * len(b)) * V * 8
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    check(getattr(lib, 'modl_filtfilt_' + sx)(ptr(d_X), V + PAD, T, V, b.ctypes.data, a.ctypes.data, zi.ctypes.data, len(b),
                                              int(detrend), ptr(d_dst), ptr(d_out), V + PAD, ptr(ws), need, None),
          'modl_filtfilt')
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert np.all(out[:, V:] == SENT)
    if not inplace:
        assert np.array_equal(d_X.cpu().numpy(), host, equal_nan=True)
    return np.ascontiguousarray(out[:, :V])


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(FILTERS))
@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_filtfilt_through_the_abi(gpu, dt, name):
    dtype, eps_out = DT[dt], float(np.finfo(DT[dt]).eps)
    coef = coefficients(name)
    for T in lengths(name):
        for detrend in (False, True):
            X, ref, e = case(name, T, detrend)
            for V in VS:
                Xv = X[:, :V].astype(dtype)
                plain = gpu_filtfilt(Xv, coef, detrend)
                assert judge(plain, ref[:, :V], Xv, e[:V], eps_out) == [], (T, V, detrend)
                assert same_bits(gpu_filtfilt(Xv, coef, detrend, inplace=True), plain), (T, V, detrend)


def adversarial(T, dtype):
    rs = np.random.RandomState(4)
    X = bold(T, 70, dtype, 5)
    X[:, 0] = 0                                                              # zeros
    X[:, 1] = 10000                                                          # a constant
    X[:, 2] = (0.25 * np.arange(T) - 3).astype(dtype)                        # a pure ramp (exact in f32)
    X[:, 3] = (1e6 + rs.randn(T)).astype(dtype)                              # 1e6 + a small signal
    X[:, 4] = 1 - 2.0 * (np.arange(T) % 2)                                   # +-1 alternating: the Nyquist frequency
    X[:, 66] = X[:, 3]                                                       # ... and in the second wavefront
    return X


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_adversarial_columns(gpu, dt):
    dtype, eps_out = DT[dt], float(np.finfo(DT[dt]).eps)
    T = 130
    X = adversarial(T, dtype)
    out = {}
    for name in ('hp5', 'lp5', 'band5'):
        coef = coefficients(name)
        for detrend in (False, True):
            ref, e = reference(coef, X, detrend)
            got = out[name, detrend] = gpu_filtfilt(X, coef, detrend)
            assert judge(got, ref, X, e, eps_out) == [], (name, detrend)
            assert np.all(got[:, 0] == 0)
            assert same_bits(got[:, 3], got[:, 66])
    scale = FILTERS['hp5'][1] * (T + 36) * EPS64 * 8
    assert np.abs(out['hp5', False][:, 1]).max() <= max(scale, 7e-12 * 8) * 10000    # a constant under a high-pass: gone
    assert np.abs(out['lp5', True][:, 2]).max() <= scale * np.abs(X[:, 2]).max()     # a ramp with detrend: gone
    # Nyquist under a low-pass: gone away from the ends (the odd extension breaks the alternation there; scipy: 1.8e-6)
    assert np.abs(out['lp5', False][40:-40, 4]).max() < 1e-5
    assert np.abs(out['hp5', False][:, 3]).max() < 10                                # 1e6 + noise: the 1e6 is gone ...
    assert np.abs(out['hp5', False][:, 3]).std() > 0.1                               # ... and the noise is not


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_non_finite_columns_stay_in_their_column(gpu, dt):
    dtype, eps_out = DT[dt], float(np.finfo(DT[dt]).eps)
    T, V = 64, 130
    X = bold(T, V, dtype, 8)
    for name in ('hp1', 'band5'):
        coef = coefficients(name)
        for detrend in (False, True):
            want = gpu_filtfilt(X, coef, detrend)
            Y = X.copy()
            Y[3, 7] = np.nan
            Y[T - 1, 64] = np.inf
            Y[0, 129] = -np.inf
            got = gpu_filtfilt(Y, coef, detrend)
            for j in (7, 64, 129):
                assert np.all(np.isnan(got[:, j])), (name, detrend, j)
            others = np.setdiff1d(np.arange(V), [7, 64, 129])
            assert same_bits(got[:, others], want[:, others])
            ref, e = reference(coef, np.where(np.isfinite(Y), Y, 0), detrend)
            assert judge(got, ref, Y, e, eps_out) == []


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_slice_permutation_and_rerun_bits(gpu, dt):
    T, V = 64, 257
    X = bold(T, V, DT[dt], 9)
    perm = np.random.RandomState(3).permutation(T)
    dst = np.empty(T, dtype=np.int64)
    dst[perm] = np.arange(T)
    for name in ('hp1', 'lp5', 'band5'):
        coef = coefficients(name)
        for detrend in (False, True):
            full = gpu_filtfilt(X, coef, detrend)
            assert same_bits(gpu_filtfilt(X, coef, detrend), full)
            assert same_bits(gpu_filtfilt(X[:, 3:200].copy(), coef, detrend), full[:, 3:200])
            assert same_bits(gpu_filtfilt(X[:, 70:71].copy(), coef, detrend), full[:, 70:71])
            assert same_bits(gpu_filtfilt(X, coef, detrend, dst=dst), full[perm])


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_entry_points_refuse_bad_arguments(gpu, dt):
    import torch
    from modl_amd._lib import lib
    coef = coefficients('band2')
    T, V, ld, n = 20, 7, 9, 5
    tdt = torch.float32 if dt == 'f32' else torch.float64
    bufs = dict(X=torch.full((T, ld), 1.5, dtype=tdt, device='cuda'), dst=torch.arange(T, dtype=torch.int64, device='cuda'),
                out=torch.full((T, ld), SENT, dtype=tdt, device='cuda'),
                ws=torch.zeros((T + 3 * n) * V, dtype=torch.float64, device='cuda'))
    ptrs = {k: v.data_ptr() for k, v in bufs.items()}
    for name, over, code in _bad_calls(T, V, ld, n):
        assert _call_filtfilt(lib, dt, ptrs, coef, T, V, ld, over) == code, name
    torch.cuda.synchronize()
    assert bool((bufs['out'] == SENT).all()) and bool((bufs['X'] == 1.5).all())
    assert _call_filtfilt(lib, dt, ptrs, coef, T, V, ld, {}) == 0
    torch.cuda.synchronize()
    assert bool((bufs['out'][:, V:] == SENT).all()) and not bool((bufs['out'][:, :V] == SENT).any())


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_butterworth_and_filtered_clean(gpu, dt):
    import torch
    from modl_amd.signal import butterworth, clean, cleaning_basis
    dtype, eps_out = DT[dt], float(np.finfo(DT[dt]).eps)
    T, V = 64, 257
    X = bold(T, V, dtype, 12)
    d_X = torch.from_numpy(X).to('cuda')
    conf = confound_set(T)
    perm = np.random.RandomState(5).permutation(T)
    for name in ('hp5', 'band5'):
        coef, kw = coefficients(name), clean_kwargs(name)
        bkw = dict(low_pass=kw['low_pass'], high_pass=kw['high_pass'], order=kw['filter_order'])
        for detrend in (False, True):
            ref, e = reference(coef, X, detrend)
            abi = gpu_filtfilt(X, coef, detrend)
            # butterworth: CUDA tensor and numpy, out, in place, a strided view, the permutation
            got = butterworth(d_X, T_R, detrend=detrend, **bkw)
            assert got.is_cuda and same_bits(got.cpu().numpy(), abi)
            assert judge(got.cpu().numpy(), ref, X, e, eps_out) == []
            host_in = butterworth(X, T_R, detrend=detrend, **bkw)
            assert isinstance(host_in, np.ndarray) and same_bits(host_in, abi)
            buf = torch.empty_like(d_X)
            assert butterworth(d_X, T_R, detrend=detrend, out=buf, **bkw) is buf and same_bits(buf.cpu().numpy(), abi)
            work = d_X.clone()
            assert butterworth(work, T_R, detrend=detrend, out=work, **bkw) is work and same_bits(work.cpu().numpy(), abi)
            assert same_bits(butterworth(d_X[:, 3:200], T_R, detrend=detrend, **bkw).cpu().numpy(), abi[:, 3:200])
            assert same_bits(butterworth(d_X, T_R, detrend=detrend, permutation=perm, **bkw).cpu().numpy(), abi[perm])
            # Q2 empty: the filtered clean IS the filter, permutation included
            assert same_bits(clean(d_X, detrend, False, permutation=perm, **kw).cpu().numpy(), abi[perm])
            # Q2 not empty
            for standardize, c in ((True, None), (True, conf), (False, conf)):
                Q2 = cleaning_basis(T, detrend, standardize, c, **kw)
                assert Q2.shape[1] == (1 if standardize else 0) + (0 if c is None else 3 if detrend else 4)
                got = clean(d_X, detrend, standardize, c, **kw).cpu().numpy()
                # the composition, bit for bit: the filter's result cleaned without a filter
                assert same_bits(got, clean(torch.from_numpy(abi).to('cuda'), False, standardize, basis=Q2).cpu().numpy())
                assert same_bits(clean(d_X, detrend, standardize, basis=Q2, **kw).cpu().numpy(), got)
                assert same_bits(clean(d_X, detrend, standardize, c, permutation=perm, **kw).cpu().numpy(), got[perm])
                assert same_bits(clean(X, detrend, standardize, c, **kw), got)
                work = d_X.clone()
                assert clean(work, detrend, standardize, c, out=work, **kw) is work and same_bits(work.cpu().numpy(), got)
                # the judge with n_store = 2, in f64 (module docstring: why not in f32)
                if dt == 'f64':
                    want = restate_filtered_clean(X, c, detrend, standardize, coef)
                    assert judge(got, want, X, e, eps_out, n_store=2) == [], (name, detrend, standardize, c is not None)
    with pytest.raises(ValueError):
        clean(d_X, permutation=perm, out=d_X, **clean_kwargs('hp5'))
    with pytest.raises(ValueError):
        butterworth(d_X[:18], T_R, high_pass=0.01)
    assert same_bits(d_X.cpu().numpy(), X)


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_estimators_filter_records_on_the_device(gpu, dt):
    from modl_amd.fmri import fMRICoder, fMRIDictFact
    from modl_amd.signal import clean
    _check_estimators(fMRIDictFact, fMRICoder, clean, DT[dt])
