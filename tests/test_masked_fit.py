"""Learning a dictionary from rows and images with missing entries: modl_masked_stats_* (csrc/masked_stats.hip),
modl_image_patches_masked_* (csrc/image.hip), modl_somf_masked_step, `DictFact.partial_fit / fit(X, mask=)` and
`ImageDictFact.fit(image, mask=)`.

The checker is a numpy restatement of the masked minibatch, written here from the estimator's definition; it takes the
solver, the dictionary update, the minibatch weight and `prepare` from the oracle and nothing from the code under test.
Tolerances are those of tests/test_inpaint.py, rel_fro against the f64 checker: products f64 <= 1e-12, f32 <= 1e-5; f64
end to end through the solver <= 1e-9; f32 trajectories by `assert_within_f32_noise` (the restatement in f32 against
itself in f64)."""
import ctypes as C
import pickle

import numpy as np
import pytest
from numpy.testing import assert_array_equal

from .conftest import assert_within_f32_noise, rel_fro

DTYPES = [np.float32, np.float64]
TOL = {np.dtype(np.float32): 1e-5, np.dtype(np.float64): 1e-12}
E2E = 1e-9


# ---- the restatement --------------------------------------------------------------------------------------------------
class Ref:
    """state of the restated estimator: the oracle's SomfState + feature_n_iter"""

    def __init__(self, orc, kw, n, X0, dtype):
        self.orc = orc
        self.pr = orc.SomfParams(**kw)
        self.st = orc.prepare(self.pr, n_samples=n, X=np.asarray(X0, dtype=dtype))
        self.fni = np.zeros(X0.shape[1], dtype=np.int64)

    def step(self, X, obs, idx, order):
        """steps 1 - 6 on the rows X (b, p) with the bool mask obs, code rows idx, atom order `order`"""
        orc, st, pr = self.orc, self.st, self.pr
        dt = st.D.dtype
        b, p = X.shape
        k = st.D.shape[0]
        idx = np.asarray(idx, dtype=np.int64)
        st.n_iter += b
        w = orc.batch_weight(st.n_iter, b, pr.learning_rate, 0)
        Xz = np.where(obs, X, 0).astype(dt)
        G, Dx = np.zeros((b, k, k), dtype=dt), np.zeros((b, k), dtype=dt)
        m = obs.sum(axis=1)
        for i in np.flatnonzero(m):
            M = np.flatnonzero(obs[i])
            r = dt.type(p) / dt.type(len(M))
            DM = st.D[:, M]
            G[i] = r * DM.dot(DM.T)
            Dx[i] = r * DM.dot(Xz[i, M])
        live = np.flatnonzero(m > 0)
        if len(live):
            orc.enet_regression_multi_gram(G[live], Dx[live], Xz[live], st.code, idx[live], pr.code_l1_ratio,
                                           pr.code_alpha, pr.code_pos, pr.tol, pr.max_iter)
        st.code[idx[m == 0]] = 0
        code = st.code[idx]
        st.C *= dt.type(1 - w)
        st.C += dt.type(w / b) * code.T.dot(code)
        c = obs.sum(axis=0)
        for e in np.flatnonzero(c):
            self.fni[e] += c[e]
            we = min(1.0, w * (c[e] / b) * (st.n_iter / self.fni[e]))
            st.B[:, e] = dt.type(1 - we) * st.B[:, e] + dt.type(we / c[e]) * code.T.dot(Xz[:, e])
        orc.update_dict(st, pr, np.arange(p), w, np.asarray(order))

    def partial_fit(self, X, obs, idx, batch_size, rng):
        for s in range(0, X.shape[0], batch_size):
            sl = slice(s, min(s + batch_size, X.shape[0]))
            self.step(X[sl], obs[sl], idx[sl], rng.permutation(self.st.D.shape[0]))


def clone_rng(est):
    rng = np.random.RandomState()
    rng.set_state(est.random_state.get_state())
    return rng


def masked_rows(n, p, seed, frac=0.5, nan=True):
    rs = np.random.RandomState(seed)
    X = rs.randn(n, 8).dot(rs.randn(8, p)) + 0.3 * rs.randn(n, p)
    obs = rs.rand(n, p) < frac
    obs[1] = True                                        # one full row
    obs[2] = False                                       # one empty row
    if nan:
        X[~obs] = np.nan
    return X, obs


def assert_state(est, ref, tol, what=''):
    st = ref.st
    for name, got, want in (('components_', est.components_, st.D), ('C_', est.C_, st.C), ('B_', est.B_, st.B),
                            ('code_', est.code_, st.code), ('comp_norm_', est.comp_norm_, st.comp_norm)):
        assert np.all(np.isfinite(got)), (what, name)
        if name == 'comp_norm_':                          # (the project's rule for it, tests/test_gpu_step.py)
            assert rel_fro(got, want) <= tol or np.allclose(got, want, atol=1e-12), (what, name, rel_fro(got, want))
        else:
            assert rel_fro(got, want) <= tol, (what, name, rel_fro(got, want))
    assert_array_equal(est.feature_n_iter_, ref.fni)
    assert est.n_iter_ == st.n_iter


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


KW = dict(n_components=12, batch_size=10, code_alpha=0.1, learning_rate=0.9, random_state=3, tol=1e-9, max_iter=2000)


# ---- 1. no GPU: argument checking ---------------------------------------------------------------------------------------
def test_masked_entry_points_are_einval_before_any_device_work():
    from modl_amd._lib import lib, SomfState, SomfBatch
    buf = np.zeros(4096)
    p = buf.ctypes.data_as(C.c_void_p)
    for sfx in ('f32', 'f64'):
        ms = getattr(lib, 'modl_masked_stats_' + sfx)
        ok = dict(X=p, ldx=60, obs=p, ldo=60, rows=None, b=3, p=60, k=12, code=p, Bt=p, fni=p, count=None)
        for bad in (dict(X=None), dict(obs=None), dict(code=None), dict(Bt=None), dict(fni=None), dict(k=0), dict(k=1025),
                    dict(ldx=59), dict(ldo=59), dict(b=-1)):
            a = dict(ok, **bad)
            assert ms(a['X'], a['ldx'], a['obs'], a['ldo'], a['rows'], a['b'], a['p'], a['k'], a['code'], a['Bt'],
                      a['fni'], a['count'], 0.5, 10, None) == -1, bad
        assert ms(p, 60, p, 60, None, 0, 60, 12, p, p, p, None, 0.5, 10, None) == 0       # b = 0: nothing to do
        pm = getattr(lib, 'modl_image_patches_masked_' + sfx)
        ok = dict(img=p, H=19, W=23, C=3, idx=p, n=4, x=4, y=5, z=3, out=p, ldo=60, mean=p, den=p, oi=p, oo=p, nobs=p)
        for bad in (dict(z=2), dict(z=1), dict(x=0), dict(y=0), dict(x=20), dict(y=24), dict(C=0), dict(C=1025, z=1025),
                    dict(n=-1), dict(ldo=59), dict(img=None), dict(idx=None), dict(out=None), dict(mean=None),
                    dict(den=None), dict(oi=None), dict(oo=None), dict(nobs=None)):
            a = dict(ok, **bad)
            assert pm(a['img'], a['H'], a['W'], a['C'], a['idx'], a['n'], a['x'], a['y'], a['z'], 1, 1, a['out'], a['ldo'],
                      a['mean'], a['den'], a['oi'], a['oo'], a['nobs'], None) == -1, bad
    st, bt = SomfState(), SomfBatch()
    assert lib.modl_somf_masked_step(None, C.byref(st), C.byref(bt), p, 60, p, 10, None) == -1


def test_masked_fit_value_errors():
    """everything a masked fit does not support is a ValueError before any device work (no GPU here)"""
    from modl_amd import DictFact
    from modl_amd.image import ImageDictFact
    X, m = np.zeros((20, 6)), np.ones((20, 6), dtype=bool)
    for kw in (dict(G_agg='full'), dict(Dx_agg='average'), dict(optimizer='sgd'), dict(n_components=1025)):
        est = DictFact(**kw)
        with pytest.raises(ValueError):
            est.partial_fit(X, mask=m)
        with pytest.raises(ValueError):
            est.fit(X, mask=m)
    for bad in (np.ones((20, 5), dtype=bool), np.ones((19, 6), dtype=bool), np.ones(20, dtype=bool)):
        with pytest.raises(ValueError):
            DictFact().partial_fit(X, mask=bad)
        with pytest.raises(ValueError):
            DictFact().fit(X, mask=bad)
    image = np.zeros((19, 23, 3))
    for method in ('average', 'dictionary only', 'sgd'):
        with pytest.raises(ValueError):
            ImageDictFact(method=method, patch_size=(4, 4), n_components=6).fit(image, mask=image != -1)
    with pytest.raises(ValueError):
        ImageDictFact(patch_size=(4, 4), n_components=6).fit(image, mask=np.ones((19, 22), dtype=bool))


# ---- 2. modl_masked_stats ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('k,p,b', [(7, 37, 1), (33, 60, 5), (70, 193, 17), (130, 60, 100), (256, 65, 33), (1024, 64, 3)])
def test_masked_stats(k, p, b, dtype):
    import torch
    from modl_amd._lib import lib
    from modl_amd.device import ptr
    rs = np.random.RandomState(k + p + b)
    n = b + 7
    X = rs.randn(n, p + 3)                                # ldx > p
    obs = rs.rand(n, p + 1) < 0.5                         # ldo > p
    rows = rs.permutation(n)[:b]
    obs[:, 0] = False                                     # nobody observes feature 0
    obs[:, 1] = True                                      # everybody observes feature 1
    if b > 1:
        obs[rows[0], 2], obs[rows[1:], 2] = True, False   # one observer
    X[:, :p + 1][~obs] = np.nan
    code = rs.randn(b, k)
    Bt0 = rs.randn(p, k)
    n_iter, w = 1000, 0.35
    fni0 = rs.randint(1, 4000, size=p).astype(np.int64)   # uneven: the clamp binds for the rarely seen features
    fni0[1] = 10
    c = obs[rows][:, :p].sum(axis=0)
    fni = fni0 + c
    we = np.where(c > 0, np.minimum(1.0, w * (c / b) * (n_iter / fni)), 0.0)
    raw = w * (c / b) * (n_iter / fni)
    assert np.any((c > 0) & (raw > 1)) and np.any((c > 0) & (raw < 1))      # both classes occur
    Xz = np.where(obs[rows][:, :p], X[rows][:, :p], 0.0)
    want = np.where((c > 0)[:, None], (1 - we)[:, None] * Bt0 + (we / np.maximum(c, 1))[:, None] * Xz.T.dot(code), Bt0)

    f = getattr(lib, 'modl_masked_stats_' + ('f32' if dtype == np.float32 else 'f64'))
    d_X, d_obs, d_rows, d_code = _t(X.astype(dtype)), _t(obs.view(np.uint8)), _t(rows.astype(np.int64)), _t(code.astype(dtype))
    outs = []
    for _ in range(2):
        d_Bt, d_fni = _t(Bt0.astype(dtype)), _t(fni0)
        d_cnt = torch.full((p,), -1, dtype=torch.int32, device='cuda')
        assert f(ptr(d_X), p + 3, ptr(d_obs), p + 1, ptr(d_rows), b, p, k, ptr(d_code), ptr(d_Bt), ptr(d_fni), ptr(d_cnt),
                 w, n_iter, None) == 0
        torch.cuda.synchronize()
        outs.append((d_Bt.cpu().numpy(), d_fni.cpu().numpy(), d_cnt.cpu().numpy()))
    Bt, got_fni, got_c = outs[0]
    assert_array_equal(got_c, c)
    assert_array_equal(got_fni, np.where(c > 0, fni, fni0))
    assert not np.any(np.isnan(Bt))
    assert_array_equal(Bt[c == 0], Bt0.astype(dtype)[c == 0])               # bit-unchanged
    want_t = np.where((c > 0)[:, None], want, Bt0.astype(dtype).astype(np.float64))
    err = rel_fro(Bt, want_t)
    print('masked_stats k=%d p=%d b=%d %s: %.3e' % (k, p, b, np.dtype(dtype).name, err))
    assert err <= TOL[np.dtype(dtype)]
    for a, b2 in zip(outs[0], outs[1]):
        assert_array_equal(a, b2)                                           # the same bits from run to run
    # without rows / counts: rows 0..b-1
    d_Bt, d_fni = _t(Bt0.astype(dtype)), _t(fni0)
    assert f(ptr(d_X), p + 3, ptr(d_obs), p + 1, None, b, p, k, ptr(d_code), ptr(d_Bt), ptr(d_fni), None, w, n_iter,
             None) == 0
    c0 = obs[:b, :p].sum(axis=0)
    assert_array_equal(d_fni.cpu().numpy(), fni0 + c0)


# ---- 3. modl_image_patches_masked --------------------------------------------------------------------------------------
def holed_image(dtype, seed=21):
    """the 19 x 23 x 3 recipe of tests/test_inpaint.py, restated: (image with -1 at the missing elements, obs bool)"""
    shape = (19, 23, 3)
    rs = np.random.RandomState(seed)
    img = rs.rand(*shape) * 2 + np.linspace(0, 1, shape[1])[None, :, None]
    img[0:4, 0:5, :] = 0.75                               # a constant window (zero norm)
    rs = np.random.RandomState(seed + 1)
    obs = rs.rand(*shape) >= 0.3
    obs[6:14, 7:17, :] = False
    obs[15:19, 0:5, 0] = False
    obs[15, 0, 1] = obs[16, 2, 2] = True
    obs[0, 0, :] = True
    obs[1, 1, 0] = False
    img[~obs] = -1
    return np.ascontiguousarray(img.astype(dtype)), obs


def np_masked_scaled(image, obs, origins, patch, with_mean, with_std):
    x, y = patch
    c = image.shape[2]
    n, N = len(origins), x * y
    rows, orows = np.zeros((n, x, y, c)), np.zeros((n, x, y, c), dtype=np.uint8)
    mean, den = np.zeros((n, c)), np.ones((n, c))
    for q, (i, j, _) in enumerate(origins):
        for ch in range(c):
            o = obs[i:i + x, j:j + y, ch].astype(bool)
            v = image[i:i + x, j:j + y, ch].astype(np.float64)
            nc = int(o.sum())
            if with_mean and nc > 0:
                mean[q, ch] = v[o].sum() / nc
            u = np.where(o, v - mean[q, ch], 0.0)
            if with_std:
                norm = np.sqrt(np.square(u).sum()) * np.sqrt(N / nc) if nc > 0 else 1.0
                if norm == 0:
                    norm = 1.0
                den[q, ch] = norm * np.sqrt(c)
            rows[q, :, :, ch] = u / den[q, ch]
            orows[q, :, :, ch] = o
    orows = orows.reshape(n, -1)
    return rows.reshape(n, -1), mean, den, orows, orows.sum(axis=1).astype(np.int32)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', DTYPES)
def test_image_patches_masked(dtype):
    from modl_amd.image import _patches_masked, _grid_patches_masked_pass, _grid, _grid_shape, grid_origins
    img, obs = holed_image(dtype)
    d_img, d_obs = _t(img), _t(obs.view(np.uint8))
    patch = (4, 5)
    g = _grid(img.shape, patch, (2, 3))
    grows, gcols = _grid_shape(g)
    origins = grid_origins(img.shape, patch, (2, 3))
    for wm, ws in ((True, True), (False, True), (True, False)):
        want = _grid_patches_masked_pass(d_img, d_obs, g, gcols, 0, grows, wm, ws)
        got = _patches_masked(d_img, d_obs, origins, patch + (3,), wm, ws)
        for a, b in zip(got, want):
            assert_array_equal(a.cpu().numpy(), b.cpu().numpy())            # the grid kernel's bits
    rs = np.random.RandomState(5)
    H, W = img.shape[:2]
    border = [(0, 0), (H - 4, W - 5), (0, W - 5), (H - 4, 0), (15, 0), (7, 8)]
    pts = border + [(rs.randint(H - 3), rs.randint(W - 4)) for _ in range(31)]
    origins = np.array([(i, j, 0) for i, j in pts], dtype=np.int64)[rs.permutation(len(pts))]
    rows, mean, den, orows, nobs = np_masked_scaled(img, obs, origins, patch, True, True)
    got = [t.cpu().numpy() for t in _patches_masked(d_img, d_obs, origins, patch + (3,), True, True)]
    tol = TOL[np.dtype(dtype)]
    for name, a, b in (('rows', got[0], rows), ('mean', got[1], mean), ('den', got[2], den)):
        assert rel_fro(a, b) <= tol, (name, rel_fro(a, b))
    assert_array_equal(got[3], orows)
    assert_array_equal(got[4], nobs)


# ---- 4. trajectories ---------------------------------------------------------------------------------------------------
def run_both(orc, kw, D0, X, obs, dtype, second=None, check=None):
    """the estimator on the GPU and the restatement side by side, one minibatch at a time, both started from the rows D0;
    `check(est, ref, t)` after every minibatch"""
    from modl_amd import DictFact
    n = X.shape[0] + (0 if second is None else second[0].shape[0])
    est = DictFact(**kw)
    est.prepare(n_samples=n, X=D0.astype(dtype))
    ref = Ref(orc, kw, n, D0, dtype)
    rng = clone_rng(est)
    bs, t, base = kw['batch_size'], 0, 0
    for Xc, oc in ((X, obs),) + ((second,) if second is not None else ()):
        for s in range(0, Xc.shape[0], bs):
            sl = slice(s, min(s + bs, Xc.shape[0]))
            idx = np.arange(base + sl.start, base + sl.stop)
            est.partial_fit(Xc[sl].astype(dtype), idx, mask=oc[sl])
            ref.step(Xc[sl].astype(dtype), oc[sl], idx, rng.permutation(kw['n_components']))
            if check is not None:
                check(est, ref, t)
            t += 1
        base += Xc.shape[0]
    return est, ref


# (k, p, code_l1_ratio, code_pos, comp_l1_ratio, comp_pos); the wide shape (more atoms than observed entries per row: the
# masked Gram matrices are singular) runs once, with the elastic-net codes, whose minimiser is unique.  The last two are
# the other ridge routes of the masked step: one Cholesky factor per row (128 < k <= 512), the blocked factorisation
# (k > 512)
TRAJ = [(12, 60, 1, False, 0, False), (12, 60, 0, False, 0, False), (12, 60, 0.5, False, 1, True),
        (12, 60, 1, True, 0, True), (70, 37, 0.5, False, 1, True), (130, 60, 0, False, 0, False),
        (520, 37, 0, False, 0, False)]


@pytest.mark.gpu
@pytest.mark.parametrize('k,p,code_l1_ratio,code_pos,comp_l1_ratio,comp_pos', TRAJ)
def test_masked_trajectory_f64(oracle, k, p, code_l1_ratio, code_pos, comp_l1_ratio, comp_pos):
    X, obs = masked_rows(25, p, seed=k)
    X2, obs2 = masked_rows(13, p, seed=99)                # a second call with fresh rows continues the trajectory
    D0 = np.random.RandomState(k + 1).randn(k, p)
    kw = dict(KW, n_components=k, code_l1_ratio=code_l1_ratio, code_pos=code_pos, comp_l1_ratio=comp_l1_ratio,
              comp_pos=comp_pos)
    run_both(oracle, kw, D0, X, obs, np.float64, second=(X2, obs2),
             check=lambda est, ref, t: assert_state(est, ref, E2E, 'minibatch %d' % t))


@pytest.mark.gpu
@pytest.mark.parametrize('code_l1_ratio', [0, 1])
def test_masked_trajectory_f32(oracle, code_l1_ratio):
    X, obs = masked_rows(25, 60, seed=12)
    kw = dict(KW, code_l1_ratio=code_l1_ratio, tol=1e-4)
    D0 = np.random.RandomState(13).randn(12, 60)
    refs = {}
    for dt in (np.float32, np.float64):                   # the restatement in f32 against itself in f64
        ref = Ref(oracle, kw, 25, D0, dt)
        rng = ref.st.rng                                  # (the oracle's prepare has drawn what the estimator's draws)
        hist = []
        for s in range(0, 25, 10):
            sl = slice(s, min(s + 10, 25))
            ref.step(X[sl].astype(dt), obs[sl], np.arange(sl.start, sl.stop), rng.permutation(12))
            hist.append({n: np.array(v) for n, v in (('D', ref.st.D), ('C', ref.st.C), ('B', ref.st.B), ('code', ref.st.code),
                                                   ('comp_norm', ref.st.comp_norm))})
        refs[np.dtype(dt)] = hist
    n_check = 3 if code_l1_ratio == 0 else 1              # l1: a tolerance-stopped solve may flip a sweep later

    def check(est, ref, t):
        if t >= n_check:
            return
        h32, h64 = refs[np.dtype(np.float32)][t], refs[np.dtype(np.float64)][t]
        for name, got in (('D', est.components_), ('C', est.C_), ('B', est.B_), ('code', est.code_),
                          ('comp_norm', est.comp_norm_)):
            print('f32 l1=%s t=%d %s: err %.2e noise %.2e' % (code_l1_ratio, t, name, rel_fro(got, h64[name]),
                                                             rel_fro(h32[name], h64[name])))
            assert_within_f32_noise(got, h32[name], h64[name], '%s after minibatch %d' % (name, t))
        assert_array_equal(est.feature_n_iter_, ref.fni)
        assert est.n_iter_ == ref.st.n_iter
    run_both(oracle, kw, D0, X, obs, np.float32, check=check)


# ---- the library's own checks, on real plans -------------------------------------------------------------------------
@pytest.mark.gpu
def test_masked_step_is_einval_on_real_plans():
    """modl_somf_masked_step behind the Python ValueErrors: every bad plan and every bad argument is MODL_EINVAL, nothing
    is enqueued, B_ and feature_n_iter are unchanged"""
    import torch
    from modl_amd import DictFact
    from modl_amd._lib import lib
    from modl_amd.device import ptr, stream_ptr
    X, obs = masked_rows(25, 60, seed=1, nan=False)
    d_obs = _t(obs.view(np.uint8))
    subset = np.arange(60, dtype=np.int64)

    def call(est, check=True, **bad):
        be = est._backend
        Xh = be.stage_X(X)
        bt, keep = be._batch(Xh, slice(0, 10), np.arange(10), None, np.arange(est.n_components), None, 0.5, 1.0, 10)
        a = dict(obs=ptr(d_obs), ldo=60, fni=ptr(be.feature_n_iter), n_iter=10)
        for name, v in bad.items():
            if name in a:
                a[name] = v
            else:
                setattr(bt, name, v)
        st = be._state()
        B0, f0, D0 = be.Bt.clone(), be.feature_n_iter.clone(), be.Dt.clone()
        rc = lib.modl_somf_masked_step(be.plan, C.byref(st), C.byref(bt), a['obs'], a['ldo'], a['fni'], a['n_iter'],
                                       stream_ptr(be.device))
        torch.cuda.synchronize()
        if check:
            assert torch.equal(be.Bt, B0) and torch.equal(be.feature_n_iter, f0) and torch.equal(be.Dt, D0), bad
        return rc

    def prepared(**kw):
        est = DictFact(**dict(KW, **kw))
        est.prepare(n_samples=25, n_features=60, dtype=np.float64)
        est._backend.Bt.normal_()
        est._backend.feature_n_iter += 3
        return est

    for kw in (dict(G_agg='full', Dx_agg='full'), dict(G_agg='full'), dict(Dx_agg='full'), dict(Dx_agg='average'),
               dict(G_agg='average'), dict(optimizer='sgd'), dict(n_components=1025)):
        assert call(prepared(**kw)) == -1, kw
    est = prepared()
    for bad in (dict(obs=None), dict(fni=None), dict(ldo=59), dict(n_iter=0), dict(n_iter=-5), dict(b=0), dict(b=-1),
                dict(b=11), dict(s=59), dict(s=61), dict(h_subset=subset.ctypes.data), dict(ldx=59), dict(d_X=None),
                dict(h_order=None)):
        assert call(est, **bad) == -1, bad
    assert call(est, check=False) == 0                     # the same call with nothing wrong runs
    assert np.all(est.feature_n_iter_ == 3 + obs[:10].sum(axis=0))


# ---- 5. a full mask is the unmasked fit --------------------------------------------------------------------------------
@pytest.mark.gpu
def test_full_mask_is_the_unmasked_fit():
    from modl_amd import DictFact
    rs = np.random.RandomState(0)
    X = rs.randn(30, 8).dot(rs.randn(8, 40)) + 0.3 * rs.randn(30, 40)
    kw = dict(KW, code_l1_ratio=0, reduction=1)
    a, b = DictFact(**kw), DictFact(**kw)
    a.prepare(n_samples=30, X=X)
    b.prepare(n_samples=30, X=X)
    a.partial_fit(X, mask=np.ones(X.shape, dtype=bool))
    b.partial_fit(X)
    for name in ('components_', 'C_', 'B_', 'code_'):
        assert rel_fro(getattr(a, name), getattr(b, name)) <= E2E, name
    assert a.n_iter_ == 30
    assert_array_equal(a.feature_n_iter_, np.full(40, 30))
    assert_array_equal(b.feature_n_iter_, np.zeros(40))
    a.partial_fit(X)                                      # an unmasked call leaves feature_n_iter_ alone
    assert_array_equal(a.feature_n_iter_, np.full(40, 30))


# ---- 6. pickle and fit -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_pickle_continues_a_masked_trajectory():
    from modl_amd import DictFact
    X, obs = masked_rows(25, 60, seed=4)
    X2, obs2 = masked_rows(15, 60, seed=5)
    est = DictFact(**dict(KW, code_l1_ratio=0))
    est.prepare(n_samples=40, X=np.where(obs, X, 0))
    est.partial_fit(X, np.arange(25), mask=obs)
    twin = pickle.loads(pickle.dumps(est))
    assert_array_equal(twin.feature_n_iter_, est.feature_n_iter_)
    for e in (est, twin):
        e.partial_fit(X2, np.arange(25, 40), mask=obs2)
    for name in ('components_', 'C_', 'B_', 'code_', 'comp_norm_', 'feature_n_iter_'):
        assert_array_equal(getattr(twin, name), getattr(est, name))
    state = est.__getstate__()
    del state['_saved']['feature_n_iter']                 # a pickle from before: zeros
    old = DictFact.__new__(DictFact)
    old.__setstate__(state)
    assert_array_equal(old.feature_n_iter_, np.zeros(60))


@pytest.mark.gpu
def test_fit_with_a_mask_two_epochs(oracle):
    from modl_amd import DictFact
    X, obs = masked_rows(25, 60, seed=8)
    kw = dict(KW, n_epochs=2)
    est = DictFact(**kw).fit(X, mask=obs)
    Xz = np.where(obs, X, 0)
    ref = Ref(oracle, kw, 25, Xz, np.float64)
    rng = ref.st.rng                                      # the oracle's prepare has drawn what the estimator's drew
    Xc, oc = X, obs
    for _ in range(2):
        ref.partial_fit(Xc, oc, np.arange(25), 10, rng)
        perm = oracle.shuffle(ref.st, ref.pr)
        Xc, oc = Xc[perm], oc[perm]
    assert_state(est, ref, E2E, 'fit')


# ---- 7. ImageDictFact.fit(image, mask=) --------------------------------------------------------------------------------
@pytest.mark.gpu
def test_image_fit_with_a_mask(oracle):
    from modl_amd.image import ImageDictFact, masked_candidates
    img, obs = holed_image(np.float64)
    x = y = 4
    H, W, Cc = img.shape
    cand = np.array([(i, j, 0) for i in range(H - x + 1) for j in range(W - y + 1)
                     if obs[i:i + x, j:j + y, :].sum() >= 0.25 * x * y * Cc], dtype=np.int64).reshape(-1, 3)
    assert_array_equal(masked_candidates(obs, (x, y), 0.25), cand)
    n_all = (H - x + 1) * (W - y + 1)
    assert 0 < len(cand) < n_all                          # min_observed excludes some windows, not all
    strict = masked_candidates(obs, (x, y), 0.75)
    assert 0 < len(strict) < len(cand)
    assert all(obs[i:i + x, j:j + y, :].mean() >= 0.75 for i, j, _ in strict)

    kw = dict(method='masked', patch_size=(x, y), n_components=6, batch_size=10, buffer_size=40, alpha=0.1, n_epochs=2,
              random_state=7, max_patches=90)
    est = ImageDictFact(**kw).fit(img, mask=obs)
    # the restatement, fed with the numpy masked scaling of the same windows in the same order
    rng = np.random.RandomState(7)
    origins = cand[rng.permutation(len(cand))[:90]]
    rows, _, _, orows, _ = np_masked_scaled(img, obs, origins, (x, y), True, True)
    dkw = dict(n_components=6, batch_size=10, code_alpha=0.1, learning_rate=0.92, reduction=10, tol=1e-2, n_epochs=2,
               random_state=rng, code_l1_ratio=1, comp_l1_ratio=0)
    ref = Ref(oracle, dkw, len(origins), rows, np.float64)
    orows = orows.astype(bool)
    for epoch in range(2):
        if epoch >= 1:
            perm = oracle.shuffle(ref.st, ref.pr)
            rows, orows = rows[perm], orows[perm]
        ref.partial_fit(rows, orows, np.arange(len(origins)), 10, ref.st.rng)
    assert_state(est.dict_fact_, ref, E2E, 'image fit')


@pytest.mark.gpu
def test_image_without_a_clean_window():
    from modl_amd.image import ImageDictFact
    rs = np.random.RandomState(2)
    H, W = 24, 24
    img = (rs.rand(H, W, 1) + np.sin(np.arange(W) / 3.0)[None, :, None]).astype(np.float64)
    obs = np.ones((H, W, 1), dtype=bool)
    obs[np.arange(H)[:, None] % 2 == np.arange(W)[None, :] % 2] = False    # a checkerboard: half missing, no clean window
    damaged = np.where(obs, img, -1.0)
    kw = dict(patch_size=(4, 4), n_components=6, batch_size=10, alpha=0.01, random_state=0, max_patches=200)
    from modl_amd._lib import ModlError
    with pytest.raises(ModlError):                        # today's rule finds no window: the patch launch gets an empty list
        ImageDictFact(**kw).fit(damaged)
    est = ImageDictFact(**kw).fit(damaged, mask=damaged != -1)
    out = est.inpaint(damaged)
    assert out.shape == damaged.shape and np.all(np.isfinite(out))
    assert_array_equal(out[obs], damaged[obs])
    assert not np.any(out[~obs] == -1)


# ---- 8. it learns ------------------------------------------------------------------------------------------------------
def planted(seed=0, n=400, p=40, k=8, nnz=3):
    rs = np.random.RandomState(seed)
    Q = rs.randn(k, p)
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    Z = np.zeros((n, k))
    for i in range(n):
        Z[i, rs.permutation(k)[:nnz]] = rs.randn(nnz)
    obs = rs.rand(n, p) < 0.5
    return Z.dot(Q), obs


LEARN_KW = dict(n_components=8, batch_size=20, code_alpha=0.01, code_l1_ratio=0, learning_rate=0.9, random_state=1,
                n_epochs=6)


def hidden_error(X, obs, code, D):
    R = (X - code.dot(D))[~obs]
    return float(np.sum(R ** 2) / np.sum(X[~obs] ** 2))


def ref_codes(orc, ref, X, obs):
    """codes of the training rows on the restatement's dictionary (the same masked estimator, from ones)"""
    st, pr = ref.st, ref.pr
    n, p = X.shape
    k = st.D.shape[0]
    G, Dx = np.zeros((n, k, k)), np.zeros((n, k))
    for i in range(n):
        M = np.flatnonzero(obs[i])
        DM = st.D[:, M]
        G[i], Dx[i] = p / len(M) * DM.dot(DM.T), p / len(M) * DM.dot(X[i, M])
    code = np.ones((n, k))
    orc.enet_regression_multi_gram(G, Dx, np.where(obs, X, 0), code, np.arange(n), pr.code_l1_ratio, pr.code_alpha,
                                   pr.code_pos, pr.tol, pr.max_iter)
    return code


def learn_reference(orc):
    X, obs = planted()
    ref = Ref(orc, LEARN_KW, X.shape[0], np.where(obs, X, 0), np.float64)
    before = hidden_error(X, obs, ref_codes(orc, ref, X, obs), ref.st.D)
    Xc, oc = X, obs
    for _ in range(LEARN_KW['n_epochs']):
        ref.partial_fit(Xc, oc, np.arange(X.shape[0]), LEARN_KW['batch_size'], ref.st.rng)
        perm = orc.shuffle(ref.st, ref.pr)
        Xc, oc = Xc[perm], oc[perm]
    after = hidden_error(X, obs, ref_codes(orc, ref, X, obs), ref.st.D)
    return X, obs, before, after


def test_planted_problem_is_learnable(oracle):
    """the condition on the inputs (no GPU): the restatement alone halves the error on the hidden entries"""
    _, _, before, after = learn_reference(oracle)
    print('hidden-entry error: prepare %.4f, after the fit %.4f' % (before, after))
    assert after <= 0.5 * before


@pytest.mark.gpu
def test_it_learns(oracle):
    from modl_amd import DictFact
    X, obs, before, after = learn_reference(oracle)
    assert after <= 0.5 * before
    est = DictFact(**LEARN_KW).fit(X, mask=obs)
    code = est.transform(X, mask=obs)
    got = hidden_error(X, obs, code, est.components_)
    print('hidden-entry error: GPU %.4f, restatement %.4f, prepare %.4f' % (got, after, before))
    assert got <= 1.05 * after
