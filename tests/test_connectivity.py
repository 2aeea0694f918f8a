"""Functional connectivity on the device: modl_amd.connectivity, csrc/connectivity.hip.

Layer 1 (no GPU) holds the numpy / scipy twins to independent judges - sklearn.covariance for the covariances, scipy.linalg.inv /
logm / sqrtm for precision, partial correlation and tangent, np.corrcoef for the seed maps, an index-loop restatement for the
vectorization, the closed form on commuting matrices and the fixed-point property for the geometric mean - then shows that each
mutant of the restatement is rejected by at least one case, and checks the refusals.  Layer 2 (gpu): the kernels through the
C-ABI inside guard elements with a poisoned workspace, then the Python layer and the estimator hook, all against the twins.

Tolerances (derivations in DESIGN.md section 30):
  covariance / correlation elements   C_COV (T + R) u64 sum_t |Xc_ti| |Xc_tj| / T with C_COV = 8: both sides sum T products and a
                                      mean of T values (2 (T + 2) u64 together), the centred operands carry the rounding of the
                                      mean and of the subtraction, each at most (T + 1) u64 (|x| / |Xc|) - the records here have
                                      |mean| <= 3 rms, so another 2 * 3 * ... stays under 8 in all; the trace, the shrinkage and
                                      its application add O(R) roundings.  Ledoit-Wolf adds |(mu I - E)_ij| times the bound of
                                      the shrinkage (two differences of such sums, over delta: its own conditioning).  For the
                                      correlation the element bound t is carried through the normalisation to first order:
                                      t_ij / sqrt(c_ii c_jj) + |corr_ij| (t_ii / (2 c_ii) + t_jj / (2 c_jj)).
  seed maps                           C (T + 2) (u sum_t |s_tr| |x_tv| / sqrt(ss_v) + u64 |out| sxx_v / ss_v): T FMAs and the final
                                      cast in the record's precision u, and the f64 raw-moment difference ss_v whose conditioning
                                      is sxx / ss.  C = 1 for f32 records (the f64 judge's own error is negligible), C = 2 for f64
                                      records (the judge errs as much as the kernel).
  precision, partial correlation,     conditioning decides: 100 times the largest difference between the twin and the twin on the
  tangent, geometric mean             same records with the time order reversed (an equally valid summation order), measured
                                      over the cases of this file when the module is set up, and printed.

The module imports the new names at the top: no test here can pass without the feature."""
import warnings

import numpy as np
import pytest
import scipy.linalg
from sklearn.exceptions import ConvergenceWarning

from modl_amd import connectivity as K
from modl_amd import (covariances, ConnectivityMeasure, geometric_mean, sym_matrix_to_vec, vec_to_sym_matrix,  # noqa: F401
                      seed_correlation, covariances_host, ConnectivityMeasureHost, geometric_mean_host,
                      seed_correlation_host)

from .test_clean import DT, EINVAL, ENOMEM, ENOGPU, same_bits
from .test_compute_mask import _Guarded, _Workspace, gpu  # noqa: F401

U64, U32 = 2.0 ** -53, 2.0 ** -24
C_COV = 8.0
SENT = -777.25
MIX_CASES = [(3, 5, 30), (6, 17, 40), (4, 33, 60), (8, 20, 25)]          # (S, R, T): the geometric mean converges on these
LW_SHAPES = [(5, 3), (19, 17), (40, 33), (7, 20), (2, 4), (3, 1)]        # (T, R)
COV_MUTANTS = ('ddof1', 'no_centre', 'beta_unclipped', 'beta_no_T', 'shrink_I')
VEC_MUTANTS = ('diag_unscaled', 'upper_order')
SEED_MUTANTS = ('no_constant_rule', 'seeds_not_centred')


# ------------------------------------------------------------------------------------------------------- the cases
def mixture_signals(S, R, T, seed=0, dtype=np.float64):
    """S records of a Gaussian mixture with a shared mixing matrix, record s with T + 3 s time points and offset means"""
    rs = np.random.RandomState(seed)
    A = np.eye(R) + rs.randn(R, R) / np.sqrt(R)
    out = []
    for s in range(S):
        Z = rs.randn(T + 3 * s, R) @ (A + 0.3 * rs.randn(R, R) / np.sqrt(R)) + 2.0 * rs.randn(R)
        out.append(Z.astype(dtype))
    return out


def plain_signals(T, R, seed, dtype=np.float64):
    rs = np.random.RandomState(seed)
    return ((rs.randn(T, R) * (0.5 + rs.rand(R))) @ (np.eye(R) + 0.4 * rs.randn(R, R) / np.sqrt(R)) + rs.randn(R)).astype(dtype)


def seed_case(T, V, R, dtype, seed=0):
    """an offset record (mean 1000, std 10: centring or the sum of squares in f32 would be wrong), exactly constant columns and
    a column that is constant to rounding"""
    rs = np.random.RandomState(1000 * T + V + R + seed)
    X = (1000.0 + 10.0 * rs.randn(T, V)).astype(dtype)
    const = sorted({0, V // 2, V - 1}) if V > 2 else [0]
    X[:, const[0]] = 1000.0
    if len(const) > 1:
        X[:, const[1]] = dtype(1000.1)
        X[:, const[2]] = 0.0
    seeds = rs.randn(T, R) + 3.0
    return X, seeds, np.array(const)


# ------------------------------------------------------------------------------------------- the restatement (plain numpy)
def re_cov(X, estimator='ledoit_wolf', mutant=None):
    X = np.asarray(X, np.float64)
    T, p = X.shape
    Xc = X if mutant == 'no_centre' else X - X.sum(axis=0) / T
    n = T - 1 if mutant == 'ddof1' else T
    E = np.einsum('ti,tj->ij', Xc, Xc) / n
    if estimator == 'empirical' or p == 1:
        return E, 0.0
    mu = np.trace(E) / p
    delta_ = np.sum(E ** 2)
    beta_ = sum(float(np.sum(Xc[t] ** 2)) ** 2 for t in range(T))
    beta = ((beta_ if mutant == 'beta_no_T' else beta_ / T) - delta_) / (p * T)
    delta = (delta_ - 2.0 * mu * np.trace(E) + p * mu ** 2) / p
    if mutant != 'beta_unclipped':
        beta = min(beta, delta)
    sh = 0.0 if beta == 0 else beta / delta
    return (1.0 - sh) * E + sh * (1.0 if mutant == 'shrink_I' else mu) * np.eye(p), sh


def cov_bound(X):
    """the forward bound of the module docstring for every covariance element, (R, R)"""
    X = np.asarray(X, np.float64)
    T, R = X.shape
    Xc = np.abs(X - X.mean(axis=0))
    return C_COV * (T + R) * U64 * (Xc.T @ Xc) / T


def lw_shrinkage_bound(X):
    """how far two correct evaluations of the Ledoit-Wolf shrinkage may lie apart: beta and delta are differences of sums of
    (T + R) terms, d(shrinkage) <= (d(beta) + shrinkage d(delta)) / delta with shrinkage <= 1"""
    X = np.asarray(X, np.float64)
    T, p = X.shape
    if p == 1:
        return 0.0
    Xc = X - X.mean(axis=0)
    E = Xc.T @ Xc / T
    mu = np.trace(E) / p
    delta_ = np.sum(E ** 2)
    beta_ = np.sum(np.sum(Xc ** 2, axis=1) ** 2)
    delta = (delta_ - 2 * mu * np.trace(E) + p * mu ** 2) / p
    return C_COV * (T + p) * U64 * ((beta_ / T + delta_) / (p * T) + (delta_ + 3 * p * mu * mu) / p) / delta


def cov_tolerance(X, estimator, correlation=False):
    """the element bound; for Ledoit-Wolf also what the shrinkage's own conditioning may add (it moves element ij by
    (mu I - E)_ij d(shrinkage)); for the correlation that bound carried through c_ij / sqrt(c_ii c_jj) to first order:
    t_ij / sqrt(c_ii c_jj) + |corr_ij| (t_ii / (2 c_ii) + t_jj / (2 c_jj))"""
    cov = covariances_host([X], estimator)[0][0]
    tol = cov_bound(X)
    if estimator == 'ledoit_wolf':
        E = covariances_host([X], 'empirical')[0][0]
        tol = tol + lw_shrinkage_bound(X) * np.abs(np.trace(E) / E.shape[0] * np.eye(E.shape[0]) - E)
    if correlation:
        d = np.diag(cov)
        rel = np.diag(tol) / (2.0 * d)
        tol = (tol + np.abs(cov) * (rel[:, None] + rel[None, :])) / np.sqrt(np.outer(d, d))
    return tol


def re_vec(m, discard_diagonal=False, mutant=None):
    out = []
    n = m.shape[0]
    for i in range(n):
        for j in range(i + 1):
            a, b = (j, i) if mutant == 'upper_order' else (i, j)
            if i == j:
                if not discard_diagonal:
                    out.append(m[i, i] if mutant == 'diag_unscaled' else m[i, i] / np.sqrt(2.0))
            else:
                out.append(m[a, b])
    if mutant == 'upper_order':                             # (0,0) (0,1) .. (0,n-1) (1,1) ..: the upper triangle row-major
        out = [m[i, j] / (np.sqrt(2.0) if i == j else 1.0) for i in range(n) for j in range(i, n) if not (discard_diagonal and i == j)]
    return np.array(out)


def re_partial(cov, mutant=None):
    P = scipy.linalg.inv(cov)
    d = np.sqrt(np.diag(P))
    out = (1.0 if mutant == 'no_sign' else -1.0) * P / np.outer(d, d)
    np.fill_diagonal(out, 1.0)
    return out


def re_tangent(cov, G, mutant=None):
    W = scipy.linalg.inv(G) if mutant == 'whiten_inv' else scipy.linalg.inv(np.real(scipy.linalg.sqrtm(G)))
    return np.real(scipy.linalg.logm(W @ cov @ W))


def re_seed(rows, seeds, mutant=None):
    X = np.asarray(rows, np.float64)
    T = X.shape[0]
    s = np.asarray(seeds, np.float64)
    if mutant != 'seeds_not_centred':
        s = s - s.mean(axis=0)
    s = (s / np.sqrt((s * s).sum(axis=0))).astype(rows.dtype).astype(np.float64)
    sx, sxx = X.sum(axis=0), (X * X).sum(axis=0)
    ss = sxx - sx * sx / T
    with np.errstate(all='ignore'):
        out = (s.T @ X) / np.sqrt(ss)
    if mutant != 'no_constant_rule':
        out[:, ss <= 8 * T * U64 * sxx] = 0.0
    return np.clip(out, -1.0, 1.0)


def seed_bound(X, seeds, out):
    X64 = np.asarray(X, np.float64)
    T = X64.shape[0]
    s = np.abs(K.prepare_seeds_host(seeds).astype(X.dtype).astype(np.float64))
    sx, sxx = X64.sum(axis=0), (X64 * X64).sum(axis=0)
    ss = sxx - sx * sx / T
    ok = ss > 8 * T * U64 * sxx
    ss = np.where(ok, ss, 1.0)
    u, c = (U32, 1.0) if X.dtype == np.float32 else (U64, 2.0)
    b = c * (T + 2) * (u * (s.T @ np.abs(X64)) / np.sqrt(ss) + U64 * np.abs(np.asarray(out, np.float64)) * sxx / ss)
    b[:, ~ok] = 0.0
    return b


# ------------------------------------------------------------------------------------------- layer 1: the twins and judges
@pytest.mark.parametrize('T,R', LW_SHAPES, ids=lambda v: str(v))
def test_covariances_host_is_sklearns(T, R):
    from sklearn.covariance import LedoitWolf, EmpiricalCovariance
    X = plain_signals(T, R, 7 * T + R)
    lw_tol, emp_tol, sh_tol = cov_tolerance(X, 'ledoit_wolf'), cov_tolerance(X, 'empirical'), lw_shrinkage_bound(X)
    cov, sh = covariances_host([X], 'ledoit_wolf')
    lw = LedoitWolf(store_precision=False).fit(X)
    assert abs(sh[0] - lw.shrinkage_) <= sh_tol, (sh[0], lw.shrinkage_, sh_tol)
    assert np.all(np.abs(cov[0] - lw.covariance_) <= lw_tol)
    emp, sh0 = covariances_host([X], 'empirical')
    assert sh0[0] == 0 and np.all(np.abs(emp[0] - EmpiricalCovariance(store_precision=False).fit(X).covariance_) <= emp_tol)
    assert same_bits(cov[0], cov[0].T) and same_bits(emp[0], emp[0].T)
    for est, tol in (('ledoit_wolf', lw_tol), ('empirical', emp_tol)):
        ref, rsh = re_cov(X, est)
        got, gsh = covariances_host([X], est)
        assert np.all(np.abs(got[0] - ref) <= tol) and abs(gsh[0] - rsh) <= sh_tol


def test_covariances_host_takes_records_of_different_lengths_and_both_dtypes():
    sig = mixture_signals(3, 5, 30)
    cov, sh = covariances_host(sig)
    assert cov.shape == (3, 5, 5) and sh.shape == (3,) and cov.dtype == np.float64 and np.all((sh > 0) & (sh < 1))
    for s in range(3):
        one, sh1 = covariances_host([sig[s]])
        assert same_bits(one[0], cov[s]) and sh1[0] == sh[s]
    c32, _ = covariances_host([x.astype(np.float32) for x in sig])
    c64, _ = covariances_host([x.astype(np.float32).astype(np.float64) for x in sig])
    assert same_bits(c32, c64)


@pytest.mark.parametrize('mutant', COV_MUTANTS)
def test_the_covariance_judge_rejects_the_mutant(mutant):
    rejected = 0
    for T, R in LW_SHAPES[:4] + [(30, 5)]:
        X = plain_signals(T, R, 7 * T + R)
        if mutant == 'beta_unclipped' and T > R:            # nearly orthogonal regions of nearly one variance: E is close to
            Q = np.linalg.qr(X - X.mean(axis=0))[0]         # mu I, delta is small and beta exceeds it
            X = np.sqrt(T) * Q * (1.0 + 0.01 * np.arange(R))
        cov = covariances_host([X])[0][0]
        bad = re_cov(X, mutant=mutant)[0]
        rejected += bool(np.any(np.abs(bad - cov) > cov_tolerance(X, 'ledoit_wolf')))
    assert rejected >= 1


def _measures(cases_signals, cls):
    out = {}
    for name, sig in cases_signals.items():
        for kind in K.KINDS:
            m = cls(kind=kind)
            out[name, kind] = (m.fit_transform(sig), m.mean_)
    return out


@pytest.fixture(scope='module')
def mix():
    """the mixture cases, the twin's answers on them, and the tolerance of the conditioned kinds: 100 times the largest
    difference between the twin and the twin on the time-reversed records"""
    signals = {c: mixture_signals(*c) for c in MIX_CASES}
    twin = _measures(signals, ConnectivityMeasureHost)
    rev = _measures({c: [x[::-1].copy() for x in s] for c, s in signals.items()}, ConnectivityMeasureHost)
    seen = {kind: max(max(np.abs(twin[c, kind][i] - rev[c, kind][i]).max() for i in (0, 1)) for c in MIX_CASES) for kind in K.KINDS}
    tol = {kind: 100.0 * v for kind, v in seen.items()}
    print('twin against the twin on time-reversed records, largest difference:', seen)
    assert all(0 < v < 1e-11 for v in seen.values()), seen
    return dict(signals=signals, twin=twin, tol=tol)


@pytest.mark.parametrize('case', MIX_CASES, ids=lambda c: 'S%dR%dT%d' % c)
def test_measures_host_against_scipy(mix, case):
    sig, tol = mix['signals'][case], mix['tol']
    cov = covariances_host(sig)[0]
    got = {kind: mix['twin'][case, kind] for kind in K.KINDS}
    assert same_bits(got['covariance'][0], cov) and same_bits(got['covariance'][1], cov.mean(axis=0))
    for s in range(len(sig)):
        d = np.sqrt(np.diag(cov[s]))
        assert np.all(np.abs(got['correlation'][0][s] - cov[s] / np.outer(d, d)) <= 4 * U64)
        assert np.all(np.diag(got['correlation'][0][s]) == 1.0) and np.all(np.diag(got['partial correlation'][0][s]) == 1.0)
        assert np.abs(got['precision'][0][s] - scipy.linalg.inv(cov[s])).max() <= tol['precision']
        assert np.abs(got['partial correlation'][0][s] - re_partial(cov[s])).max() <= tol['partial correlation']
        assert np.abs(got['partial correlation'][0][s] - re_partial(cov[s], 'no_sign')).max() > 1e3 * tol['partial correlation']
    G = got['tangent'][1]
    m = ConnectivityMeasureHost(kind='tangent').fit(sig)
    assert same_bits(m.mean_, G) and np.abs(m.whitening_ - scipy.linalg.inv(np.real(scipy.linalg.sqrtm(G)))).max() <= tol['tangent']
    for s in range(len(sig)):
        assert np.abs(got['tangent'][0][s] - re_tangent(cov[s], G)).max() <= tol['tangent']
        assert np.abs(got['tangent'][0][s] - re_tangent(cov[s], G, 'whiten_inv')).max() > 1e3 * tol['tangent']
    assert same_bits(got['tangent'][0], np.swapaxes(got['tangent'][0], 1, 2))
    # transform of unseen records uses the fitted whitening
    unseen = mixture_signals(2, case[1], case[2], seed=5)
    t = m.transform(unseen)
    cu = covariances_host(unseen)[0]
    assert all(np.abs(t[s] - re_tangent(cu[s], G)).max() <= tol['tangent'] for s in range(2)) and same_bits(m.mean_, G)
    for kind in K.KINDS:                                    # the vectorized forms are the vectors of the matrices
        full = got[kind][0]
        for discard in (False, True):
            v = ConnectivityMeasureHost(kind=kind, vectorize=True, discard_diagonal=discard).fit_transform(sig)
            R = case[1]
            assert v.shape == (len(sig), R * (R - 1) // 2 if discard else R * (R + 1) // 2)
            assert all(same_bits(v[s], re_vec(full[s], discard)) for s in range(len(sig)))


def test_vectorization_is_the_index_loop():
    rs = np.random.RandomState(1)
    for n in (1, 2, 5, 40):
        m = rs.randn(n, n)
        m = m + m.T
        for discard in (False, True):
            v = sym_matrix_to_vec(m, discard)
            assert same_bits(v, re_vec(m, discard))
            for mutant in VEC_MUTANTS:
                if n >= 5 and not (discard and mutant == 'diag_unscaled'):
                    assert not np.array_equal(v, re_vec(m, discard, mutant)), mutant
        # the round trip: exact off the diagonal, and exact everywhere when the diagonal travels beside the vector; a diagonal
        # element that went through / sqrt(2) * sqrt(2) has been rounded twice and may come back one ulp away
        back = vec_to_sym_matrix(sym_matrix_to_vec(m))
        off = ~np.eye(n, dtype=bool)
        assert same_bits(back[off], m[off]) and np.all(np.abs(np.diag(back) - np.diag(m)) <= np.spacing(np.abs(np.diag(m))))
        assert same_bits(vec_to_sym_matrix(sym_matrix_to_vec(m, True), np.diag(m).copy()), m)
        stack = np.stack([m, 2 * m])
        assert same_bits(sym_matrix_to_vec(stack)[1], sym_matrix_to_vec(2 * m)) and same_bits(
            vec_to_sym_matrix(sym_matrix_to_vec(stack, True), np.stack([np.diag(m), 2 * np.diag(m)])), stack)
    with pytest.raises(ValueError, match='square'):
        sym_matrix_to_vec(np.zeros((3, 4)))
    with pytest.raises(ValueError, match='lower triangle'):
        vec_to_sym_matrix(np.zeros(4))
    with pytest.raises(ValueError, match='diagonal'):
        vec_to_sym_matrix(np.zeros(3), np.zeros(4))


def test_geometric_mean_host_commuting_matrices_have_the_closed_form():
    rs = np.random.RandomState(3)
    R, S = 9, 5
    Q = np.linalg.qr(rs.randn(R, R))[0]
    lam = np.exp(rs.randn(S, R))
    covs = np.stack([(Q * l) @ Q.T for l in lam])
    G, norms = geometric_mean_host(covs, return_norms=True)
    ref = (Q * np.exp(np.log(lam).mean(axis=0))) @ Q.T
    assert len(norms) <= 3 and np.abs(G - ref).max() <= 64 * R * U64 * np.abs(ref).max(), (len(norms), np.abs(G - ref).max())


@pytest.mark.parametrize('case', MIX_CASES, ids=lambda c: 'S%dR%dT%d' % c)
def test_geometric_mean_host_is_a_fixed_point(mix, case):
    cov = covariances_host(mix['signals'][case])[0]
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        G, norms = geometric_mean_host(cov, return_norms=True)
    R = case[1]
    assert 2 <= len(norms) <= 10 and norms[-1] < 1e-7 and np.all(norms[:-1] >= 1e-7)
    assert np.all(np.abs(norms / 1e-7 - 1.0) > 1e-3), norms     # no iteration count can flip on rounding
    W = scipy.linalg.inv(np.real(scipy.linalg.sqrtm(G)))
    L = np.mean([np.real(scipy.linalg.logm(W @ c @ W)) for c in cov], axis=0)
    assert np.linalg.norm(L) / R ** 2 < 1e-7
    assert same_bits(G, G.T) and same_bits(G, mix['twin'][case, 'tangent'][1])
    assert same_bits(geometric_mean_host(list(cov)), G)


def test_geometric_mean_host_warns_at_max_iter_and_refuses():
    cov = covariances_host(mixture_signals(*MIX_CASES[1]))[0]
    with pytest.warns(ConvergenceWarning, match='maximum number of iterations'):
        G, norms = geometric_mean_host(cov, max_iter=2, return_norms=True)
    assert len(norms) == 2 and norms[-1] >= 1e-7 and np.all(np.isfinite(G))
    with pytest.raises(ValueError, match='max_iter'):
        geometric_mean_host(cov, max_iter=0)
    with pytest.raises(ValueError, match='tol'):
        geometric_mean_host(cov, tol=0.0)
    with pytest.raises(ValueError, match=r'\(S, R, R\)'):
        geometric_mean_host(cov[0])
    with pytest.raises(ValueError, match='positive definite'):
        geometric_mean_host(np.stack([np.diag([1.0, -1.0])]))
    bad = cov.copy()
    bad[0] = -bad[0]                                        # a mean that is positive definite, a record that is not
    bad[1:] *= 10
    with pytest.raises(FloatingPointError):
        with np.errstate(all='ignore'):
            geometric_mean_host(bad)


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_seed_correlation_host_is_corrcoef(dt):
    rejected = {m: 0 for m in SEED_MUTANTS}
    for T, V, R in ((2, 5, 1), (5, 63, 3), (37, 130, 17)):
        X, seeds, const = seed_case(T, V, R, DT[dt])
        got = seed_correlation_host(X, seeds)
        assert got.dtype == DT[dt] and got.shape == (R, V) and np.all(np.abs(got) <= 1) and np.all(got[:, const] == 0)
        keep = np.setdiff1d(np.arange(V), const)
        with np.errstate(all='ignore'):
            ref = np.corrcoef(np.asarray(seeds, np.float64).T, X[:, keep].astype(np.float64).T)[:R, R:]
        bound = seed_bound(X, seeds, got)
        # np.corrcoef takes the seeds in f64, the definition casts the prepared seeds to the record's dtype: one more u of the
        # bound's sum; the answer itself is rounded to the record's dtype
        tol = bound * (1.0 + 1.0 / (T + 2)) + (U32 if dt == 'f32' else U64)
        assert np.all(np.abs(got[:, keep] - np.clip(ref, -1, 1)) <= tol[:, keep])
        assert np.all(np.abs(got - re_seed(X, seeds)) <= tol)
        for m in SEED_MUTANTS:
            with np.errstate(all='ignore'):
                bad = re_seed(X, seeds, m)
            rejected[m] += bool(np.any(~(np.abs(bad - got) <= tol)))
    assert all(v >= 1 for v in rejected.values()), rejected


def test_the_offset_record_rejects_sums_of_squares_in_f32():
    """the discriminating power of the offset-mean case, checked before relying on it: a sequential f32 emulation of the kernel's
    product sits well inside the bound, the same with ss formed in f32 is outside it"""
    T, V, R = 37, 4099, 17
    X, seeds, const = seed_case(T, V, R, np.float32)
    ref = seed_correlation_host(X.astype(np.float64), seeds)
    bound = seed_bound(X, seeds, ref)
    sh = K.prepare_seeds_host(seeds).astype(np.float32)
    acc, sx, sxx = np.zeros((R, V), np.float32), np.zeros(V, np.float32), np.zeros(V, np.float32)
    for t in range(T):
        acc = acc + sh[t][:, None] * X[t][None, :]
        sx, sxx = sx + X[t], sxx + X[t] * X[t]
    X64 = X.astype(np.float64)
    ss = (X64 * X64).sum(axis=0) - X64.sum(axis=0) ** 2 / T
    keep = np.setdiff1d(np.arange(V), const)
    good = acc[:, keep].astype(np.float64) / np.sqrt(ss[keep])
    frac = np.max(np.abs(good - ref[:, keep]) / bound[:, keep])
    with np.errstate(all='ignore'):
        mut = acc[:, keep].astype(np.float64) / np.sqrt((sxx - sx * sx / np.float32(T)).astype(np.float64)[keep])
    worst = np.nanmax(np.abs(mut - ref[:, keep]) / bound[:, keep])
    print('f32 emulation: %.3f of the bound (largest bound %.2e); with ss in f32: %.1f of the bound' % (frac, bound.max(), worst))
    assert frac < 1 and (worst > 1 or np.isnan(mut).any())


def test_value_errors_name_the_offender():
    ok = plain_signals(6, 3, 0)
    for fn in (covariances, covariances_host):
        with pytest.raises(ValueError, match='at least 2 time points'):
            fn([ok, ok[:1]])
        with pytest.raises(ValueError, match='one number of regions'):
            fn([ok, ok[:, :2]])
        with pytest.raises(ValueError, match='estimator'):
            fn([ok], estimator='oas')
        with pytest.raises(ValueError, match='at least one record'):
            fn([])
        with pytest.raises(ValueError, match=r'\(time points, regions\)'):
            fn([ok[0]])
    for cls in (ConnectivityMeasure, ConnectivityMeasureHost):
        with pytest.raises(ValueError, match='kind'):
            cls(kind='coherence').fit([ok])
        with pytest.raises(ValueError, match='not fitted'):
            cls().transform([ok])
        with pytest.raises(ValueError, match='regions'):
            cls().fit([ok]).transform([ok[:, :2]])
    X, seeds, _ = seed_case(5, 7, 2, np.float64)
    for fn in (seed_correlation, seed_correlation_host):
        with pytest.raises(ValueError, match='at least 2 time points'):
            fn(X[:1], seeds[:1])
        with pytest.raises(ValueError, match='time points'):
            fn(X, seeds[:4])
        flat = seeds.copy()
        flat[:, 1] = 3.5
        with pytest.raises(ValueError, match='seed 1 is constant'):
            fn(X, flat)
        with pytest.raises(ValueError, match=r'\(time points, voxels\)'):
            fn(X[0], seeds)


def _cov_call(lib, dt, p, over=None):
    a = dict(X=p['X'], ldx=5, off=p['off'], S=2, R=4, est=1, out=0, cov=p['cov'], sh=p['sh'], ws=p['ws'],
             ws_bytes=lib.modl_conn_covariance_workspace(2, 4))
    a.update(over or {})
    return getattr(lib, 'modl_conn_covariance_' + dt)(a['X'], a['ldx'], a['off'], a['S'], a['R'], a['est'], a['out'], a['cov'], a['sh'],
                                                     a['ws'], a['ws_bytes'], None)


def _seed_call(lib, dt, p, over=None):
    a = dict(X=p['X'], ldx=5, T=6, V=5, seeds=p['seeds'], R=2, out=p['out'], ldo=6)
    a.update(over or {})
    return getattr(lib, 'modl_conn_seed_maps_' + dt)(a['X'], a['ldx'], a['T'], a['V'], a['seeds'], a['R'], a['out'], a['ldo'], None)


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_entry_points_refuse_bad_arguments_without_a_device(dt):
    from modl_amd._lib import lib
    maxr = lib.modl_conn_max_regions()
    assert maxr >= 512
    bufs = dict(X=np.ones(6 * 5, DT[dt]), off=np.array([0, 2, 6], np.int64), cov=np.zeros(2 * 16), sh=np.zeros(2), ws=np.zeros(1 << 12, np.uint8),
                seeds=np.ones(6 * 2, DT[dt]), out=np.zeros(2 * 6, DT[dt]),
                off_short=np.array([0, 1, 6], np.int64), off_back=np.array([0, 4, 3], np.int64), off_neg=np.array([-1, 2, 6], np.int64))
    p = {k: v.ctypes.data for k, v in bufs.items()}
    need = lib.modl_conn_covariance_workspace(2, 4)
    assert 0 < need <= bufs['ws'].nbytes and lib.modl_conn_covariance_workspace(1, 4) < need < lib.modl_conn_covariance_workspace(2, 65)
    assert lib.modl_conn_covariance_workspace(1, maxr) > 0
    for S_, R_ in ((0, 4), (-1, 4), (2, 0), (2, -3), (2, maxr + 1)):
        assert lib.modl_conn_covariance_workspace(S_, R_) == 0 and _cov_call(lib, dt, p, dict(S=S_, R=R_, ldx=max(R_, 5))) == EINVAL
    for k in ('X', 'off', 'cov', 'sh'):
        assert _cov_call(lib, dt, p, {k: None}) == EINVAL, k
    for over in (dict(ldx=3), dict(est=2), dict(est=-1), dict(out=2), dict(out=-1), dict(off=p['off_short']), dict(off=p['off_back']),
                 dict(off=p['off_neg']), dict(X=p['X'] + 1), dict(cov=p['cov'] + 4), dict(sh=p['sh'] + 2), dict(ws=p['ws'] + 3)):
        assert _cov_call(lib, dt, p, over) == EINVAL, over
    assert _cov_call(lib, dt, p, dict(ws=None)) == ENOMEM and _cov_call(lib, dt, p, dict(ws_bytes=need - 1)) == ENOMEM
    for k in ('X', 'seeds', 'out'):
        assert _seed_call(lib, dt, p, {k: None}) == EINVAL, k
    for over in (dict(R=0), dict(R=maxr + 1), dict(T=1), dict(T=0), dict(V=0), dict(ldx=4), dict(ldo=4), dict(X=p['X'] + 2),
                 dict(seeds=p['seeds'] + 1), dict(out=p['out'] + 3)):
        assert _seed_call(lib, dt, p, over) == EINVAL, over
    assert all(np.all(bufs[k] == 0) for k in ('cov', 'sh', 'ws', 'out')) and np.all(bufs['X'] == 1)
    if lib.modl_device_count() == 0:
        assert _cov_call(lib, dt, p) == ENOGPU and _seed_call(lib, dt, p) == ENOGPU
        assert _cov_call(lib, dt, p, dict(ws=None)) == ENOMEM                     # ENOMEM before ENOGPU


def test_python_functions_equal_their_host_twins():
    """without a GPU the functions ARE their twins; with one this is the device against the judge"""
    sig = mixture_signals(*MIX_CASES[0])
    cov, sh = covariances(sig)
    ref, rsh = covariances_host(sig)
    assert isinstance(cov, np.ndarray) and all(np.all(np.abs(cov[s] - ref[s]) <= cov_tolerance(sig[s], 'ledoit_wolf'))
                                                for s in range(len(sig)))
    assert all(abs(sh[s] - rsh[s]) <= lw_shrinkage_bound(sig[s]) for s in range(len(sig)))
    # (100 times the geometric mean's time-reversal difference on this case, 8.5e-15 measured on the CPU: the module docstring)
    assert np.abs(geometric_mean(ref) - geometric_mean_host(ref)).max() <= 8.5e-13
    X, seeds, _ = seed_case(5, 63, 3, np.float32)
    got, want = seed_correlation(X, seeds), seed_correlation_host(X, seeds)
    assert got.dtype == np.float32 and np.all(np.abs(got.astype(np.float64) - want) <= seed_bound(X, seeds, want))


# ---------------------------------------------------------------------------------------------------- the estimator hook
def _seed_phantom(dtype):
    rs = np.random.RandomState(11)
    shape, T = (8, 7, 6), 40
    mask = np.zeros(shape, bool)
    mask[1:7, 1:6, :] = True
    mask[3, 3, 2] = False                                    # 179 voxels
    D = rs.randn(3, int(mask.sum())).astype(dtype)
    vol = (100.0 + 10.0 * rs.randn(*shape, T)).astype(dtype)
    flat = (50.0 + 5.0 * rs.randn(T, int(mask.sum()))).astype(dtype)
    flat += (rs.randn(T, 3) @ D).astype(dtype)
    return mask, D, vol, flat


def _check_coder_seed_correlation(fMRICoder, dtype):
    mask, D, vol, flat = _seed_phantom(dtype)
    coder = fMRICoder(D, mask=mask, standardize=True, detrend=True).fit()
    maps = coder.seed_correlation([vol, flat])
    assert len(maps) == 2 and all(isinstance(m, np.ndarray) and m.shape == D.shape and m.dtype == dtype for m in maps)
    for rec, got in zip((vol, flat), maps):
        rows = coder._rows(rec)
        rows = rows.cpu().numpy() if hasattr(rows, 'cpu') else np.asarray(rows)
        codes = coder.transform([rec])[0]
        want = seed_correlation_host(rows, codes)
        assert np.all(np.abs(got.astype(np.float64) - want) <= seed_bound(rows, codes, want)) and np.abs(want).max() > 0.05
    assert coder.seed_maps_img_.shape == mask.shape + (3,) and np.all(coder.seed_maps_img_[~mask] == 0)
    assert same_bits(np.ascontiguousarray(coder.seed_maps_img_[mask].T), maps[1])
    one = coder.seed_correlation(flat)                       # one record as it is
    assert len(one) == 1 and same_bits(one[0], maps[1])
    free = fMRICoder(D).fit()
    assert free.seed_correlation([flat])[0].shape == D.shape and not hasattr(free, 'seed_maps_img_')
    with pytest.raises(ValueError, match='not fitted'):
        fMRICoder(D).seed_correlation([flat])


def test_coder_seed_correlation_host_logic():
    from .test_masker import _host_estimators
    _check_coder_seed_correlation(_host_estimators()[1], np.float64)


# ------------------------------------------------------------------------------------------------ layer 2: the GPU
RECORD_SETS = [(2,), (3, 37, 5), (64, 2, 19, 4)]


def gpu_covariance(sig, ld, est, out, dt):
    """modl_conn_covariance_* on the stacked records inside guards, with a poisoned workspace: (cov (S, R, R), shrinkage (S,))"""
    import torch
    from modl_amd._lib import lib
    R, S = sig[0].shape[1], len(sig)
    stacked = np.full((sum(x.shape[0] for x in sig), ld), SENT, DT[dt])
    stacked[:, :R] = np.concatenate(sig)
    X = torch.from_numpy(stacked).cuda()
    off = np.concatenate([[0], np.cumsum([x.shape[0] for x in sig])]).astype(np.int64)
    cov, sh = _Guarded(S * R * R, torch.float64, SENT), _Guarded(S, torch.float64, SENT)
    ws = _Workspace(lib.modl_conn_covariance_workspace(S, R))
    rc = getattr(lib, 'modl_conn_covariance_' + dt)(X.data_ptr(), ld, off.ctypes.data, S, R, est, out, cov.ptr, sh.ptr, ws.ptr, ws.need, None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    ws.check()
    return cov.get().reshape(S, R, R), sh.get()


def _check_covariance(sig, got, gsh, est, out, fractions):
    name = 'ledoit_wolf' if est else 'empirical'
    ref, rsh = covariances_host(sig, name)
    for s, X in enumerate(sig):
        assert same_bits(got[s], got[s].T)
        want = K._correlation_of(ref[s]) if out else ref[s]
        tol = cov_tolerance(X, name, bool(out))
        assert abs(gsh[s] - rsh[s]) <= (lw_shrinkage_bound(X) if est else 0.0), (gsh[s], rsh[s])
        if out:
            assert np.all(np.diag(got[s]) == 1.0)
        err = np.abs(got[s] - want)
        assert np.all(err <= tol), (err.max(), tol.max())
        with np.errstate(invalid='ignore', divide='ignore'):
            fractions.append(float(np.nanmax(np.where(tol > 0, err / tol, 0.0))))


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'f64'])
@pytest.mark.parametrize('R', [1, 15, 16, 17, 33, 130])
def test_gpu_covariance_kernels_agree_with_the_twin(gpu, R, dt):
    fractions = []
    for lens in RECORD_SETS:
        sig = [plain_signals(T, R, 100 * T + R + i, DT[dt]) for i, T in enumerate(lens)]
        for ld in (R, R + 3):
            for est in (0, 1):
                for out in (0, 1):
                    got, gsh = gpu_covariance(sig, ld, est, out, dt)
                    _check_covariance(sig, got, gsh, est, out, fractions)
    print('R = %d %s: largest seen fraction of the bound %.3f' % (R, dt, max(fractions)))


@pytest.mark.gpu
def test_gpu_covariance_at_the_largest_region_count(gpu):
    from modl_amd._lib import lib
    R = lib.modl_conn_max_regions()
    sig = [plain_signals(8, R, 5, np.float64)]
    fractions = []
    for est, out in ((1, 0), (0, 1)):
        got, gsh = gpu_covariance(sig, R, est, out, 'f64')
        _check_covariance(sig, got, gsh, est, out, fractions)
    print('R = %d: largest seen fraction of the bound %.3f' % (R, max(fractions)))


@pytest.mark.gpu
def test_gpu_covariance_bits(gpu):
    """two calls, a record alone / first of three / last of three, an f32 record and its f64 copy: the same bits"""
    for R in (17, 130):
        a, b, c = (plain_signals(T, R, T + R, np.float32) for T in (37, 5, 64))
        for est, out in ((1, 0), (1, 1), (0, 0)):
            alone, sh_alone = gpu_covariance([a], R, est, out, 'f32')
            again, sh_again = gpu_covariance([a], R, est, out, 'f32')
            first, sh_first = gpu_covariance([a, b, c], R + 3, est, out, 'f32')
            last, sh_last = gpu_covariance([c, b, a], R, est, out, 'f32')
            wide, sh_wide = gpu_covariance([a.astype(np.float64)], R, est, out, 'f64')
            for m, s in ((again[0], sh_again[0]), (first[0], sh_first[0]), (last[2], sh_last[2]), (wide[0], sh_wide[0])):
                assert same_bits(m, alone[0]) and s == sh_alone[0]


def gpu_seed_maps(X, sh, ldx, ldo, dt):
    import torch
    from modl_amd._lib import lib
    T, V = X.shape
    R = sh.shape[1]
    padded = np.full((T, ldx), SENT, DT[dt])
    padded[:, :V] = X
    d_X, d_s = torch.from_numpy(padded).cuda(), torch.from_numpy(np.ascontiguousarray(sh, DT[dt])).cuda()
    out = _Guarded(R * ldo, torch.float32 if dt == 'f32' else torch.float64, SENT)
    rc = getattr(lib, 'modl_conn_seed_maps_' + dt)(d_X.data_ptr(), ldx, T, V, d_s.data_ptr(), R, out.ptr, ldo, None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    got = out.get().reshape(R, ldo)
    assert np.all(got[:, V:] == DT[dt](SENT))
    return got[:, :V]


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'f64'])
@pytest.mark.parametrize('T', [2, 5, 37, 67])
def test_gpu_seed_maps_agree_with_the_twin(gpu, T, dt):
    worst = 0.0
    for V in (1, 63, 64, 65, 4099):
        for R in (1, 17, 33, 70):
            X, seeds, const = seed_case(T, V, R, DT[dt])
            sh = K.prepare_seeds_host(seeds).astype(DT[dt])
            got = gpu_seed_maps(X, sh, V + 5, V + 2, dt)
            want = seed_correlation_host(X, seeds).astype(np.float64)
            bound = seed_bound(X, seeds, want)
            assert got.dtype == DT[dt] and np.all(np.abs(got) <= 1) and np.all(got[:, const] == 0)
            err = np.abs(got.astype(np.float64) - want)
            assert np.all(err <= bound), (V, R, err.max(), bound.max())
            ok = bound > 0
            if ok.any():
                worst = max(worst, float(np.max(err[ok] / bound[ok])))
            if (V, R) in ((65, 17), (4099, 70)):
                assert same_bits(gpu_seed_maps(X, sh, V, V, dt), got)
    print('T = %d %s: largest seen fraction of the bound %.3f' % (T, dt, worst))


@pytest.mark.gpu
def test_gpu_seed_maps_beyond_one_pass_of_seeds(gpu):
    """more than 128 seeds: the workgroup's block of the record is swept once per 128 seeds, the statistics come from the first"""
    X, seeds, const = seed_case(37, 130, 300, np.float32)
    sh = K.prepare_seeds_host(seeds).astype(np.float32)
    got = gpu_seed_maps(X, sh, 131, 130, 'f32')
    want = seed_correlation_host(X, seeds).astype(np.float64)
    assert np.all(np.abs(got.astype(np.float64) - want) <= seed_bound(X, seeds, want)) and np.all(got[:, const] == 0)


@pytest.mark.gpu
@pytest.mark.parametrize('case', MIX_CASES, ids=lambda c: 'S%dR%dT%d' % c)
def test_gpu_connectivity_measure_agrees_with_the_twin(gpu, mix, case):
    torch = gpu
    sig, tol = mix['signals'][case], mix['tol']
    unseen = mixture_signals(2, case[1], case[2], seed=5)
    bounds = np.stack([cov_tolerance(x, 'ledoit_wolf') for x in sig])
    seen = {}
    for kind in K.KINDS:
        want, want_mean = mix['twin'][case, kind]
        for cuda in (False, True):
            records = [torch.from_numpy(x).cuda() for x in sig] if cuda else sig
            m = ConnectivityMeasure(kind=kind)
            got = m.fit_transform(records)
            assert (isinstance(got, torch.Tensor) and got.is_cuda and m.mean_.is_cuda) if cuda else isinstance(got, np.ndarray)
            got, mean = (got.cpu().numpy(), m.mean_.cpu().numpy()) if cuda else (got, m.mean_)
            if kind == 'covariance':
                assert np.all(np.abs(got - want) <= bounds) and np.all(np.abs(mean - want_mean) <= bounds.max(axis=0))
            elif kind == 'correlation':
                cb = np.stack([cov_tolerance(x, 'ledoit_wolf', True) for x in sig])
                assert np.all(np.abs(got - want) <= cb) and np.all(got[:, range(case[1]), range(case[1])] == 1.0)
            else:
                seen[kind] = max(seen.get(kind, 0.0), np.abs(got - want).max(), np.abs(mean - want_mean).max())
                assert np.abs(got - want).max() <= tol[kind] and np.abs(mean - want_mean).max() <= tol[kind], (kind, seen[kind], tol[kind])
            assert same_bits(got, np.swapaxes(got, 1, 2))
            if kind == 'tangent':
                t = m.transform([torch.from_numpy(x).cuda() for x in unseen] if cuda else unseen)
                t = t.cpu().numpy() if cuda else t
                ref = ConnectivityMeasureHost(kind=kind).fit(sig).transform(unseen)
                assert np.abs(t - ref).max() <= tol[kind]
                wh = m.whitening_.cpu().numpy() if cuda else m.whitening_
                assert np.abs(wh - ConnectivityMeasureHost(kind=kind).fit(sig).whitening_).max() <= tol[kind]
            for discard in (False, True):
                v = ConnectivityMeasure(kind=kind, vectorize=True, discard_diagonal=discard).fit_transform(records)
                v = v.cpu().numpy() if cuda else v
                if kind in ('covariance', 'correlation'):   # (the kernels' bits are fixed; the eigensolver's are not promised)
                    assert same_bits(v, sym_matrix_to_vec(got, discard))
                else:
                    assert np.abs(v - sym_matrix_to_vec(got, discard)).max() <= tol[kind]
    G = geometric_mean(torch.from_numpy(mix['twin'][case, 'covariance'][0]).cuda())
    assert G.is_cuda and np.abs(G.cpu().numpy() - mix['twin'][case, 'tangent'][1]).max() <= tol['tangent']
    print('largest difference from the twin on the device:', seen, 'tolerances:', {k: tol[k] for k in seen})


@pytest.mark.gpu
def test_gpu_python_functions(gpu):
    torch = gpu
    sig = [x.astype(np.float32) for x in mixture_signals(*MIX_CASES[2])]
    ref, rsh = covariances_host(sig)
    for est in ('ledoit_wolf', 'empirical'):
        ref, rsh = covariances_host(sig, est)
        cov, sh = covariances([torch.from_numpy(x).cuda() for x in sig], est)
        assert cov.is_cuda and sh.is_cuda and cov.dtype == torch.float64
        host_cov, host_sh = covariances(sig, est)
        assert same_bits(cov.cpu().numpy(), host_cov) and same_bits(sh.cpu().numpy(), host_sh)
        assert all(np.all(np.abs(host_cov[s] - ref[s]) <= cov_tolerance(sig[s], est)) for s in range(len(sig)))
    X, seeds, const = seed_case(37, 4099, 17, np.float32)
    want = seed_correlation_host(X, seeds)
    got = seed_correlation(torch.from_numpy(X).cuda(), torch.from_numpy(seeds).cuda())
    assert got.is_cuda and got.dtype == torch.float32
    assert np.all(np.abs(got.cpu().numpy().astype(np.float64) - want) <= seed_bound(X, seeds, want))
    view = torch.from_numpy(np.concatenate([X, X], axis=1)).cuda()[:, :4099]         # a view with a leading dimension
    assert same_bits(seed_correlation(view, seeds).cpu().numpy(), got.cpu().numpy())
    assert same_bits(seed_correlation(X, seeds), got.cpu().numpy())
    with pytest.raises(ValueError, match='constant'):
        seed_correlation(torch.from_numpy(X).cuda(), np.ones((37, 2)))
    with pytest.raises(ValueError, match='at most'):
        seed_correlation(X, np.random.RandomState(0).randn(37, 513))
    with pytest.raises(ValueError, match='at most'):
        covariances([np.random.RandomState(0).randn(4, 513)])


@pytest.mark.gpu
def test_gpu_fmri_coder_seed_correlation(gpu):
    from modl_amd.fmri import fMRICoder
    _check_coder_seed_correlation(fMRICoder, np.float32)
