"""Dictionaries of 1024 < k <= 4096 atoms (the wide route: csrc/cd_wide.hip, csrc/bcd.hip dict_update_wide) against the
CPU oracle: the code solve through the ABI shims, the dictionary update through modl_dict_update_*, the estimator, Coder,
fMRIDictFact, the bounds and a pickle round trip.  f64: <= 1e-9 with the oracle's sweep counts; f32: within the reference
algorithm's own f32 noise (conftest.assert_within_f32_noise)."""
import pickle

import numpy as np
import pytest

from .conftest import assert_within_f32_noise, rel_fro

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gpu():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    return torch


def _atoms(k, p, seed=0, dt=np.float64):
    rs = np.random.RandomState(seed)
    D = rs.randn(k, p) * (rs.rand(k, p) < 0.5) + 0.05 * rs.randn(k, p)
    return (D / np.linalg.norm(D, axis=1, keepdims=True)).astype(dt)


def _regression_inputs(k, dt, b=24, seed=0):
    rs = np.random.RandomState(seed)
    p = k + 400
    D = _atoms(k, p, seed, np.float64)
    X = rs.randn(b, 24).dot(D[rs.choice(k, 24, replace=False)]) + 0.05 * rs.randn(b, p)
    G = D.dot(D.T)
    Dx = X.dot(D.T)
    n = b + 8
    code = np.zeros((n, k))
    code[rs.rand(n, k) < 0.01] = 0.1
    idx = rs.permutation(n)[:b].astype(np.int64)
    return [np.ascontiguousarray(a.astype(dt)) for a in (G, Dx, X, code)] + [idx]


def _solve_pair(oracle, kind, G, Dx, X, code, idx, l1_ratio, positive, alpha=0.2, tol=1e-3, max_iter=100):
    from modl_amd import dict_fact_fast as dff
    f_gpu = getattr(dff, '_enet_regression_%s_gram' % kind)
    f_orc = getattr(oracle, 'enet_regression_%s_gram' % kind)
    b = Dx.shape[0]
    sw_gpu, sw_orc = np.zeros(b, np.int32), np.zeros(b, np.int32)
    c_gpu, c_orc = code.copy(), code.copy()
    f_gpu(G, Dx.copy(), X, c_gpu, idx, l1_ratio, alpha, positive, tol, max_iter, sweeps=sw_gpu)
    f_orc(G, Dx.copy(), X, c_orc, idx, l1_ratio, alpha, positive, tol, max_iter, sweeps=sw_orc)
    return c_gpu, c_orc, sw_gpu, sw_orc


@pytest.mark.parametrize('k', [1025, 1100, 2048, 4096])
@pytest.mark.parametrize('positive', [False, True])
def test_code_solve_single_gram_f64(gpu, oracle, k, positive):
    G, Dx, X, code, idx = _regression_inputs(k, np.float64)
    c_gpu, c_orc, sw_gpu, sw_orc = _solve_pair(oracle, 'single', G, Dx, X, code, idx, 0.5, positive)
    np.testing.assert_array_equal(sw_gpu, sw_orc)
    assert rel_fro(c_gpu, c_orc) < 1e-9


@pytest.mark.parametrize('k', [1100, 2048])
def test_code_solve_single_gram_f32(gpu, oracle, k):
    ins64 = _regression_inputs(k, np.float64)
    ins32 = [a.astype(np.float32) if a.dtype == np.float64 else a for a in ins64]
    c_gpu, c32, sw_gpu, sw32 = _solve_pair(oracle, 'single', *ins32, 0.5, False)
    _, c64, _, sw64 = _solve_pair(oracle, 'single', *ins64, 0.5, False)
    assert np.sum(sw_gpu != sw64) <= max(1, len(sw64) // 8), (sw_gpu, sw64)
    assert_within_f32_noise(c_gpu, c32, c64, 'codes')


def test_code_solve_unaligned_gram(gpu, oracle):
    """A Gram matrix at an offset of one element (not 16-byte aligned) and a device tensor input: no padded copy."""
    import torch
    k = 1100
    G, Dx, X, code, idx = _regression_inputs(k, np.float64, seed=1)
    from modl_amd import dict_fact_fast as dff
    buf = torch.zeros(k * k + 1, dtype=torch.float64, device='cuda')
    buf[1:] = torch.from_numpy(G.ravel()).cuda()
    dG = buf[1:].view(k, k)
    assert dG.data_ptr() % 16 != 0
    dcode = torch.from_numpy(code.copy()).cuda()
    sw_gpu = np.zeros(len(idx), np.int32)
    out = dff._enet_regression_single_gram(dG, torch.from_numpy(Dx).cuda(), torch.from_numpy(X).cuda(), dcode, idx,
                                           0.5, 0.2, False, 1e-3, 100, sweeps=sw_gpu)
    c_orc, sw_orc = code.copy(), np.zeros(len(idx), np.int32)
    oracle.enet_regression_single_gram(G, Dx.copy(), X, c_orc, idx, 0.5, 0.2, False, 1e-3, 100, sweeps=sw_orc)
    np.testing.assert_array_equal(sw_gpu, sw_orc)
    assert rel_fro(out.cpu().numpy(), c_orc) < 1e-9


@pytest.mark.parametrize('k', [1100, 2048])
def test_code_solve_multi_gram_f64(gpu, oracle, k):
    G, Dx, X, code, idx = _regression_inputs(k, np.float64, b=6)
    rs = np.random.RandomState(3)
    Gm = np.stack([G * (1 + 0.1 * rs.rand()) for _ in range(len(idx))])   # a different Gram per sample
    c_gpu, c_orc, sw_gpu, sw_orc = _solve_pair(oracle, 'multi', Gm, Dx, X, code, idx, 0.5, False)
    np.testing.assert_array_equal(sw_gpu, sw_orc)
    assert rel_fro(c_gpu, c_orc) < 1e-9


@pytest.mark.parametrize('kind', ['single', 'multi'])
def test_ridge_codes_k2048(gpu, oracle, kind):
    G, Dx, X, code, idx = _regression_inputs(2048, np.float64, b=4 if kind == 'multi' else 24)
    if kind == 'multi':
        G = np.stack([G] * len(idx))
    c_gpu, c_orc, _, _ = _solve_pair(oracle, kind, G, Dx, X, code, idx, 0.0, False)
    assert rel_fro(c_gpu[idx], c_orc[idx]) < 1e-9


# ---- the dictionary update through modl_dict_update_* ------------------------------------------------------------
# (the case builder and the call live in test_dict_update_routes.py, which runs them over every route up to 1024 atoms)
from .test_dict_update_routes import dict_update_case as _dict_update_case  # noqa: E402


UPDATE_CASES = [dict(), dict(comp_l1_ratio=1.0), dict(comp_l1_ratio=0.5), dict(comp_l1_ratio=1.0, comp_pos=True),
                dict(optimizer='sgd')]


@pytest.mark.parametrize('case', UPDATE_CASES, ids=lambda c: '-'.join('%s=%s' % kv for kv in c.items()) or 'l2')
@pytest.mark.parametrize('k,s', [(1100, 1000), (1100, 8000), (2048, 1000)])
def test_dict_update_f64(gpu, oracle, case, k, s):
    D, cn, D_orc, cn_orc = _dict_update_case(oracle, k, s, np.float64, **case)
    assert rel_fro(D, D_orc) < 1e-9
    # the norm budgets left after the projections sit at rounding level (~1e-16) when the ball is hit: absolute
    np.testing.assert_allclose(cn, cn_orc, rtol=1e-9, atol=1e-12)


# ---- the estimator ------------------------------------------------------------------------------------------------
def _est_pair(oracle, dt, k, b=16, r=2, n=None, n_samples=None, p=1500, seed=0, **extra):
    from modl_amd import DictFact
    rs = np.random.RandomState(seed)
    n = n or k + 2 * b
    k0 = 32
    X = ((rs.randn(n, k0) * (rs.rand(n, k0) < 0.3)).dot(rs.randn(k0, p)) / np.sqrt(0.3 * k0)
         + 0.1 * rs.randn(n, p)).astype(dt)
    kw = dict(n_components=k, batch_size=b, reduction=r, code_alpha=1.0, learning_rate=0.92, random_state=0)
    kw.update(extra)
    ns = n_samples or n
    est = DictFact(**kw)
    est.prepare(n_samples=ns, X=X)
    pr = oracle.SomfParams(**kw)
    st = oracle.prepare(pr, n_samples=ns, X=X)
    return est, pr, st, X


def _run(est, oracle, pr, st, X, b, path):
    """two minibatches on the estimator (None: the oracle only) and on the oracle; the estimator's sweep counts of the
    per-minibatch path"""
    st.sweeps = []
    sweeps = []
    if path == 'chunk':
        if est is not None:
            est.partial_fit(X[:2 * b])                           # one call, two minibatches (the chunk route)
        oracle.partial_fit(st, pr, X[:2 * b])
    else:
        for t in range(2):
            rows = slice(t * b, (t + 1) * b)
            idx = np.arange(rows.start, rows.stop)
            if est is not None:
                est.partial_fit(X[rows], idx)
                if pr.code_l1_ratio != 0:
                    sweeps.append(est._backend.last_sweeps().copy())
            oracle.partial_fit(st, pr, X[rows], idx)
    return sweeps


def _observables(est, st, b):
    out = [('components_', est.components_, st.D), ('code_', est.code_[:2 * b], st.code[:2 * b]), ('C_', est.C_, st.C),
           ('B_', est.B_, st.B)]
    if getattr(st, 'G', None) is not None and getattr(est, 'G_', None) is not None:
        out.append(('G_', est.G_, st.G))
    return out


EST_CASES = {'default': dict(), 'G_full': dict(G_agg='full'), 'ridge': dict(code_l1_ratio=0.0),
             'l1_pos_atoms': dict(comp_l1_ratio=1.0, comp_pos=True), 'sgd': dict(optimizer='sgd', learning_rate=1.0)}


# every case on both paths at k = 1100; at k = 2048 the chunk route with the default and sgd cases
EST_F64 = ([(1100, c, path) for c in EST_CASES for path in ('step', 'chunk')] + [(2048, c, 'step') for c in EST_CASES] +
           [(2048, 'default', 'chunk'), (2048, 'sgd', 'chunk')])


@pytest.mark.parametrize('k,case,path', EST_F64)
def test_estimator_f64(gpu, oracle, k, case, path):
    b = 16
    est, pr, st, X = _est_pair(oracle, np.float64, k, b=b, **EST_CASES[case])
    sweeps = _run(est, oracle, pr, st, X, b, path)
    for t, sw in enumerate(sweeps):
        np.testing.assert_array_equal(sw, st.sweeps[t])
    for name, got, want in _observables(est, st, b):
        assert rel_fro(got, want) < 1e-9, (name, rel_fro(got, want))


@pytest.mark.parametrize('k', [1100])
def test_estimator_average_f64(gpu, oracle, k):
    """G_agg = Dx_agg = 'average': one Gram per sample (G_average_), few samples so that n k^2 stays small."""
    b = 8
    est, pr, st, X = _est_pair(oracle, np.float64, k, b=b, n_samples=2 * b, G_agg='average', Dx_agg='average')
    sweeps = _run(est, oracle, pr, st, X, b, 'step')
    for t, sw in enumerate(sweeps):
        np.testing.assert_array_equal(sw, st.sweeps[t])
    for name, got, want in _observables(est, st, b):
        assert rel_fro(got, want) < 1e-9, (name, rel_fro(got, want))


@pytest.mark.parametrize('case', ['default', 'l1_pos_atoms'])
@pytest.mark.parametrize('k', [1100, 2048])
def test_estimator_f32(gpu, oracle, k, case):
    b = 16
    est, pr32, s32, X = _est_pair(oracle, np.float32, k, b=b, **EST_CASES[case])
    _, pr64, s64, _ = _est_pair(oracle, np.float64, k, b=b, **EST_CASES[case])
    sweeps = _run(est, oracle, pr32, s32, X, b, 'step')
    _run(None, oracle, pr64, s64, X.astype(np.float64), b, 'step')
    flips = sum(int(np.sum(sw != s64.sweeps[t])) for t, sw in enumerate(sweeps))
    assert flips <= max(1, 0.05 * 2 * b), flips
    for (name, got, want32), (_, _, want64) in zip(_observables(est, s32, b), _observables(est, s64, b)):
        if flips:
            err = rel_fro(got, want64)
            noise = rel_fro(want32, want64)
            assert err <= 2 * noise + 1e-5 + 6e-5, (name, err, noise, flips)
        else:
            assert_within_f32_noise(got, want32, want64, name)


# ---- Coder, fMRI, bounds, pickle ----------------------------------------------------------------------------------
def test_coder_transform_score_k2048(gpu, oracle):
    from modl_amd import Coder
    k, p = 2048, 2400
    D = _atoms(k, p, 5)
    rs = np.random.RandomState(1)
    X = rs.randn(20, 16).dot(D[:16]) + 0.05 * rs.randn(20, p)
    coder = Coder(D, code_alpha=0.2, code_l1_ratio=1.0, tol=1e-3, max_iter=100)
    pr = oracle.SomfParams(n_components=k, code_alpha=0.2, code_l1_ratio=1.0, tol=1e-3, max_iter=100)
    assert rel_fro(coder.transform(X), oracle.transform(pr, D, X)) < 1e-9
    s_gpu, s_orc = coder.score(X), oracle.score(pr, D, X)
    assert abs(s_gpu - s_orc) <= 1e-9 * abs(s_orc)


def test_fmri_dict_fact_k1100(gpu):
    from oracle import wrappers_oracle
    from modl_amd.fmri import fMRIDictFact
    rs = np.random.RandomState(0)
    k, p = 1100, 1300
    maps = _atoms(k, p, 2)
    recs = []
    for _ in range(2):
        x = rs.randn(24, 40).dot(maps[:40]) + 0.01 * rs.randn(24, p)
        recs.append(np.ascontiguousarray((x - x.mean(0)) / x.std(0)))
    common = dict(n_components=k, alpha=1e-2, batch_size=24, learning_rate=0.92, random_state=0, dict_init=maps,
                  method='masked', reduction=2, n_epochs=1)
    est = fMRIDictFact(**common).fit(recs)
    D_ref, st = wrappers_oracle.fmri_fit(recs, **common)
    assert rel_fro(est.components_, D_ref) < 1e-9
    assert rel_fro(est.dict_fact_.code_, st.code) < 1e-9


def test_k4096_one_minibatch_f64(gpu, oracle):
    """The LDS edge of the code solver: 4 x 4096 f64 coefficients per sample."""
    b = 8
    est, pr, st, X = _est_pair(oracle, np.float64, 4096, b=b, p=1200)
    est.partial_fit(X[:b], np.arange(b))
    sw = est._backend.last_sweeps().copy()
    st.sweeps = []
    oracle.partial_fit(st, pr, X[:b], np.arange(b))
    np.testing.assert_array_equal(sw, st.sweeps[0])
    for name, got, want in _observables(est, st, b // 2):
        assert rel_fro(got, want) < 1e-9, (name, rel_fro(got, want))


def test_k4097_rejected(gpu):
    from modl_amd import DictFact
    X = np.random.RandomState(0).randn(4100, 50)
    with pytest.raises(ValueError, match='4096'):
        DictFact(n_components=4097, batch_size=8).prepare(n_samples=4100, X=X)


def test_multi_rank_path_rejected_above_1024(gpu):
    """The two-phase exchange of several ranks (forced here on one rank) is refused beyond 1024 atoms."""
    from modl_amd import DictFact
    X = np.random.RandomState(0).randn(1100, 50)
    est = DictFact(n_components=1025, batch_size=8)
    est._force_reduce = True
    with pytest.raises(ValueError, match='single GPU'):
        est.prepare(n_samples=1100, X=X)


def test_pickle_round_trip_k1100(gpu, oracle):
    b = 16
    est, pr, st, X = _est_pair(oracle, np.float64, 1100, b=b)
    est.partial_fit(X[:b], np.arange(b))
    est2 = pickle.loads(pickle.dumps(est))
    np.testing.assert_array_equal(est2.components_, est.components_)
    np.testing.assert_array_equal(est2.C_, est.C_)
    rows = np.arange(b, 2 * b)
    est.partial_fit(X[rows], rows)
    est2.partial_fit(X[rows], rows)
    np.testing.assert_array_equal(est2.components_, est.components_)
    np.testing.assert_array_equal(est2.code_, est.code_)
