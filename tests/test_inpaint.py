"""Inpainting: the per-row masked Gram / Dx product (csrc/masked_gram.hip), masked grid patches, weighted overlap-add and
finish (csrc/image.hip, "inpainting"), `CodingMixin.transform(X, mask)` and `ImageDictFact.inpaint`.

The checkers are plain numpy in f64, written here: the formulas restated.  Tolerances, rel_fro against
the f64 checker: f64 <= 1e-12, f32 <= 1e-5, f64 end to end through the solver <= 1e-9.  Image 19 x 23 x 3 with patch
(4, 5) as in test_image_reconstruct.py; its holes: 30 % of the elements at random per channel, a fully missing 8 x 10
block at (6, 7) (larger than 2x-1 by 2y-1: at stride 1 some pixels are covered by empty windows only), the window at
(0, 0) constant (zero norm), the window at (15, 0) without any observed element in channel 0."""
import contextlib
import ctypes as C
import io

import numpy as np
import pytest
from numpy.testing import assert_array_equal

from .conftest import rel_fro
from .test_image_reconstruct import PATCH, make_image, restated_origins

SHAPE = (19, 23, 3)
STRIDES = [(1, 1), (2, 3)]
DTYPES = [np.float32, np.float64]
TOL = {np.dtype(np.float32): 1e-5, np.dtype(np.float64): 1e-12}


# ---- the checkers -----------------------------------------------------------------------------------------------------
def np_masked_gram(Dt, X, obs, rows):
    """G[ii] = r sum_{e in M} Dt[e] Dt[e]^T, Dx[ii] = r sum_{e in M} X[i][e] Dt[e], r = p / |M|, zeros when M is empty"""
    Dt = np.asarray(Dt, dtype=np.float64)
    p, k = Dt.shape
    G, Dx, nobs = np.zeros((len(rows), k, k)), np.zeros((len(rows), k)), np.zeros(len(rows), dtype=np.int32)
    for ii, i in enumerate(rows):
        M = np.flatnonzero(obs[i])
        nobs[ii] = len(M)
        if len(M) == 0:
            continue
        r = p / len(M)
        for e in M:
            G[ii] += np.outer(Dt[e], Dt[e])
            Dx[ii] += float(X[i, e]) * Dt[e]
        G[ii] *= r
        Dx[ii] *= r
    return G, Dx, nobs


def np_masked_scaled(image, obs, origins, patch, with_mean, with_std):
    """rows, mean (n, C), den (n, C), obs rows, nobs: the statistics over the observed elements of each channel"""
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


def np_weighted_overlap(patches, use, origins, shape, patch):
    x, y = patch
    acc, cnt = np.zeros(shape), np.zeros(shape[:2], dtype=np.int32)
    for row, u, (i, j, _) in zip(np.asarray(patches, dtype=np.float64), use, origins):
        if u:
            acc[i:i + x, j:j + y, :] += row.reshape(x, y, shape[2])
            cnt[i:i + x, j:j + y] += 1
    return acc, cnt


def np_finish(acc, cnt, image, obs, keep_observed):
    out = np.where(cnt[:, :, None] > 0, acc / np.maximum(cnt, 1)[:, :, None], image.astype(np.float64))
    return np.where(obs.astype(bool), image.astype(np.float64), out) if keep_observed else out


def holed_image(dtype, seed=21):
    """(image with -1 at the missing elements, obs (H, W, C) bool)"""
    img = make_image(SHAPE, np.float64, seed=seed)        # the window at (0, 0) is constant
    rs = np.random.RandomState(seed + 1)
    obs = rs.rand(*SHAPE) >= 0.3
    obs[6:14, 7:17, :] = False
    obs[15:19, 0:5, 0] = False
    obs[15, 0, 1] = obs[16, 2, 2] = True                  # channels 1 - 2 of that window are not wholly missing
    obs[0, 0, :] = True                                   # the constant window keeps observed elements in every channel
    obs[1, 1, 0] = False                                  # ... and a hole
    img[~obs] = -1
    return np.ascontiguousarray(img.astype(dtype)), obs


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- CPU --------------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_einval_before_any_device_work():
    """the host-side checks of every new export: no GPU is touched (the pointers are host arrays, never read)"""
    from modl_amd._lib import lib
    buf = np.zeros(4096)
    p = buf.ctypes.data_as(C.c_void_p)
    for sfx in ('f32', 'f64'):
        mg = getattr(lib, 'modl_masked_gram_' + sfx)
        ok = dict(Dt=p, p=60, k=12, X=p, ldx=60, obs=p, ldo=60, rows=None, b=3, G=p, Dx=p, nobs=None)
        for bad in (dict(Dt=None), dict(X=None), dict(obs=None), dict(G=None), dict(Dx=None), dict(k=0), dict(k=1025),
                    dict(p=0), dict(ldx=59), dict(ldo=59), dict(b=-1)):
            a = dict(ok, **bad)
            assert mg(a['Dt'], a['p'], a['k'], a['X'], a['ldx'], a['obs'], a['ldo'], a['rows'], a['b'], a['G'], a['Dx'],
                      a['nobs'], None) == -1, bad
        assert mg(p, 60, 12, p, 60, p, 60, None, 0, p, p, None, None) == 0          # b = 0: nothing to do
        gp = getattr(lib, 'modl_image_grid_patches_masked_' + sfx)
        ok = dict(H=19, W=23, C=3, x=4, y=5, si=2, sj=3, row0=0, nrows=9, ldo=60, img=p, out=p, mean=p, den=p, oi=p,
                  oo=p, nobs=p)
        for bad in (dict(si=5), dict(sj=6), dict(si=0), dict(H=3), dict(W=4), dict(C=0), dict(C=1025), dict(row0=-1),
                    dict(nrows=10), dict(row0=5, nrows=5), dict(nrows=-1), dict(ldo=59), dict(img=None), dict(out=None),
                    dict(mean=None), dict(den=None), dict(oi=None), dict(oo=None), dict(nobs=None)):
            a = dict(ok, **bad)
            assert gp(a['img'], a['H'], a['W'], a['C'], a['x'], a['y'], a['si'], a['sj'], a['row0'], a['nrows'], 1, 1,
                      a['out'], a['ldo'], a['mean'], a['den'], a['oi'], a['oo'], a['nobs'], None) == -1, bad
        add = getattr(lib, 'modl_image_overlap_add_weighted_' + sfx)
        assert add(p, 60, 19, 23, 3, 4, 5, 5, 3, 0, 9, p, p, p, None) == -1
        assert add(p, 59, 19, 23, 3, 4, 5, 2, 3, 0, 9, p, p, p, None) == -1
        assert add(p, 60, 19, 23, 3, 4, 5, 2, 3, 0, 10, p, p, p, None) == -1
        assert add(p, 60, 19, 23, 3, 4, 5, 2, 3, 0, 9, None, p, p, None) == -1
        assert add(p, 60, 19, 23, 3, 4, 5, 2, 3, 0, 9, p, None, p, None) == -1
        assert add(p, 60, 19, 23, 3, 4, 5, 2, 3, 0, 9, p, p, None, None) == -1
        assert add(None, 60, 19, 23, 3, 4, 5, 2, 3, 0, 9, p, p, p, None) == -1
        fin = getattr(lib, 'modl_image_inpaint_finish_' + sfx)
        assert fin(p, p, p, p, 0, 23, 3, 1, p, None) == -1
        assert fin(p, p, p, p, 19, 0, 3, 1, p, None) == -1
        assert fin(p, p, p, p, 19, 23, 0, 1, p, None) == -1
        assert fin(p, p, p, p, 19, 23, 1025, 1, p, None) == -1
        for hole in range(5):
            a = [p] * 5
            a[hole] = None
            assert fin(a[0], a[1], a[2], a[3], 19, 23, 3, 1, a[4], None) == -1, hole


def test_bad_arguments_raise_valueerror_without_gpu():
    from modl_amd import DictFact
    from .test_wrappers import _image_estimator, synth_image
    X = np.zeros((5, 60))
    for bad_mask in (np.ones((5, 59), dtype=bool), np.ones((4, 60), dtype=bool), np.ones(60, dtype=bool),
                     np.ones((5, 60, 1), dtype=bool)):
        with pytest.raises(ValueError, match='mask'):
            DictFact(n_components=7).transform(X, mask=bad_mask)
    with pytest.raises(ValueError, match='1024'):
        DictFact(n_components=1025).transform(X, mask=np.ones((5, 60), dtype=bool))
    est = _image_estimator(True)(patch_size=PATCH, n_components=5, batch_size=10, alpha=0.1, random_state=0,
                                 max_patches=40, reduction=2)
    with contextlib.redirect_stdout(io.StringIO()):
        est.fit(synth_image(19, 23, 3, seed=2))
    img = np.zeros(SHAPE)
    for kw in (dict(mask=np.ones((19, 22), dtype=bool)), dict(mask=np.ones((19, 23, 2), dtype=bool)),
               dict(mask=np.ones((19, 23, 3, 1), dtype=bool)), dict(mask=np.ones(19, dtype=bool)),
               dict(stride=(5, 1)), dict(stride=(1, 6)), dict(stride=0)):
        with pytest.raises(ValueError):
            est.inpaint(img, **kw)
    for bad_img in (np.zeros((19, 23, 1)), np.zeros((3, 23, 3)), np.zeros((19, 4, 3)), np.zeros((19, 23))):
        with pytest.raises(ValueError):
            est.inpaint(bad_img)
    est.n_components = 1025
    with pytest.raises(ValueError, match='1024'):
        est.inpaint(img)


def test_hole_pattern_has_every_class_of_patch():
    """the fixture itself, on the CPU: clean, holed and empty windows on both grids, and at stride 1 pixels that only
    empty windows cover"""
    img, obs = holed_image(np.float64)
    for stride in STRIDES:
        origins = restated_origins(SHAPE, PATCH, stride)[0]
        nobs = np_masked_scaled(img, obs, origins, PATCH, True, True)[4]
        P = PATCH[0] * PATCH[1] * SHAPE[2]
        assert (nobs == 0).any() and ((nobs > 0) & (nobs < P)).any(), stride
        cnt = np_weighted_overlap(np.zeros((len(origins), P)), nobs > 0, origins, SHAPE, PATCH)[1]
        assert (cnt > 0).any() and (stride != (1, 1) or (cnt == 0).any())
    img2, obs2 = inpaint_image(np.float64)                # adds clean windows: (0, 8) and, on the (2, 3) grid, (0, 9)
    assert_array_equal(np_masked_scaled(img2, obs2, [(0, 8, 0), (0, 9, 0)], PATCH, True, True)[4], 60)
    assert_array_equal(img2 == -1, ~obs2)


# ---- GPU: the masked Gram kernel -------------------------------------------------------------------------------------
def _masked_gram(Dt, X, obs, rows, b):
    import torch
    from modl_amd._lib import lib, check
    from modl_amd.device import ptr, stream_ptr
    k = Dt.shape[1]
    G = torch.full((b, k, k), float('nan'), dtype=Dt.dtype, device=Dt.device)
    Dx = torch.full((b, k), float('nan'), dtype=Dt.dtype, device=Dt.device)
    nobs = torch.full((b,), -7, dtype=torch.int32, device=Dt.device)
    f = getattr(lib, 'modl_masked_gram_' + ('f32' if Dt.dtype == torch.float32 else 'f64'))
    check(f(ptr(Dt), Dt.shape[0], k, ptr(X), X.stride(0), ptr(obs), obs.stride(0), ptr(rows), b, ptr(G), ptr(Dx), ptr(nobs),
            stream_ptr(Dt.device)), 'modl_masked_gram')
    return G.cpu().numpy(), Dx.cpu().numpy(), nobs.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('k,p,b', [(7, 37, 5), (33, 60, 9), (70, 193, 6), (130, 60, 5), (256, 192, 3), (1024, 64, 2)])
def test_masked_gram(k, p, b, dtype):
    import torch
    rs = np.random.RandomState(k + p)
    n = b + 3                                             # rows 0 - 2: fully observed, one entry observed, none
    Dt = rs.randn(p, k).astype(dtype)
    X = rs.randn(n, p).astype(dtype)
    obs = (rs.rand(n, p) < 0.5).astype(np.uint8)
    obs[0], obs[1], obs[2] = 1, 0, 0
    obs[1, p // 3] = 1
    Xn = np.where(obs != 0, X, np.nan).astype(dtype)      # unobserved entries must not reach the result
    tol = TOL[np.dtype(dtype)]
    d_Dt = _t(Dt)

    def run(rows, ldx, ldo):
        """all of X's rows, b at a time"""
        Xp = torch.full((n, ldx), float('nan'), dtype=d_Dt.dtype, device='cuda')
        Op = torch.ones((n, ldo), dtype=torch.uint8, device='cuda')          # the padding says "observed": never read
        Xp[:, :p], Op[:, :p] = _t(Xn), _t(obs)
        for c0 in range(0, len(rows), b):
            chunk = rows[c0:c0 + b]
            d_rows = _t(np.asarray(chunk, dtype=np.int64)) if ldx != p else None
            if d_rows is None:
                assert list(chunk) == list(range(b))
            G, Dx, nobs = _masked_gram(d_Dt, Xp, Op, d_rows, b)
            wG, wDx, wn = np_masked_gram(Dt, X, obs, chunk)
            assert np.isfinite(G).all() and np.isfinite(Dx).all()
            assert_array_equal(nobs, wn)
            assert_array_equal(G, np.swapaxes(G, 1, 2))                      # exactly symmetric
            errs = rel_fro(G, wG), rel_fro(Dx, wDx)
            print('masked gram', (k, p, b), np.dtype(dtype), 'rows' if d_rows is not None else 'identity', errs)
            assert max(errs) <= tol, errs
            for ii, i in enumerate(chunk):
                if i == 2:                                                   # no observed entry
                    assert nobs[ii] == 0
                    assert_array_equal(G[ii], 0)
                    assert_array_equal(Dx[ii], 0)
                if i == 1:
                    assert nobs[ii] == 1
                if i == 0:
                    assert nobs[ii] == p
            G2, Dx2, nobs2 = _masked_gram(d_Dt, Xp, Op, d_rows, b)            # run to run
            assert_array_equal(G2, G)
            assert_array_equal(Dx2, Dx)
            assert_array_equal(nobs2, nobs)

    run(list(range(b)), p, p)                             # d_rows NULL, dense leading dimensions
    perm = list(rs.permutation(n))
    rows = perm + [perm[0]]                               # every row, one of them twice
    rows += [perm[1]] * (-len(rows) % b)
    run(rows, p + 3, p + 5)                               # d_rows, ldx > p, ldo > p


# ---- GPU: the image kernels ------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('stride', STRIDES)
def test_masked_grid_patches(stride, dtype):
    from modl_amd import image as mi
    img, obs = holed_image(dtype)
    origins = restated_origins(SHAPE, PATCH, stride)[0]
    g = mi._grid(SHAPE, PATCH, stride)
    grows, gcols = mi._grid_shape(g)
    d_img = _t(np.where(obs, img, np.nan).astype(dtype))  # missing values must not reach the result
    d_obs = _t(obs.astype(np.uint8))
    clean_img = make_image(SHAPE, dtype, seed=23)
    d_clean, d_all = _t(clean_img), _t(np.ones(SHAPE, dtype=np.uint8))
    for with_mean, with_std in ((True, True), (True, False), (False, True), (False, False)):
        got = [t.cpu().numpy() for t in mi._grid_patches_masked_pass(d_img, d_obs, g, gcols, 0, grows, with_mean, with_std)]
        want = np_masked_scaled(img, obs, origins, PATCH, with_mean, with_std)
        assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all() and np.isfinite(got[2]).all()
        assert_array_equal(got[3], want[3])
        assert_array_equal(got[4], want[4])
        errs = tuple(rel_fro(a, b) for a, b in zip(got[:3], want[:3]))
        print('masked grid patches', stride, np.dtype(dtype), with_mean, with_std, errs)
        assert max(errs) <= TOL[np.dtype(dtype)], errs
        assert_array_equal(got[0][got[3] == 0], 0)        # unobserved elements are written as 0
        if with_mean and with_std:                        # the constant window (0, 0), with a hole: zero norm -> 1
            assert 0 < got[4][0] < 60
            assert_array_equal(got[0][0], 0)
            assert_array_equal(got[1][0], dtype(0.5))
            assert_array_equal(got[2][0], dtype(np.sqrt(np.float64(3))))
        # a pass is the matching slice of the full call
        part = mi._grid_patches_masked_pass(d_img, d_obs, g, gcols, grows // 3, grows - grows // 3, with_mean, with_std)
        for a, b in zip(part, got):
            assert_array_equal(a.cpu().numpy(), b[(grows // 3) * gcols:])
        # an image without holes: modl_image_grid_patches_*'s outputs bit for bit
        m = mi._grid_patches_masked_pass(d_clean, d_all, g, gcols, 0, grows, with_mean, with_std)
        u = mi._grid_patches_pass(d_clean, g, gcols, 0, grows, with_mean, with_std)
        for a, b in zip(m[:3], u):
            assert_array_equal(a.cpu().numpy(), b.cpu().numpy())
        assert_array_equal(m[3].cpu().numpy(), 1)
        assert_array_equal(m[4].cpu().numpy(), 60)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('stride', STRIDES)
def test_weighted_overlap_add_and_finish(stride, dtype):
    import torch
    from modl_amd import image as mi
    img, obs = holed_image(dtype)
    origins, grows, gcols = restated_origins(SHAPE, PATCH, stride)
    g = mi._grid(SHAPE, PATCH, stride)
    rs = np.random.RandomState(5)
    nobs = np_masked_scaled(img, obs, origins, PATCH, False, False)[4]
    use = ((nobs > 0) & (rs.rand(len(origins)) < 0.8)).astype(np.uint8)
    assert (use == 0).any() and use.any()
    patches = rs.randn(len(origins), 60).astype(dtype)
    patches[use == 0] = np.nan                            # rows that are not used are not read
    acc_w, cnt_w = np_weighted_overlap(np.where(use[:, None] != 0, patches, 0), use, origins, SHAPE, PATCH)
    assert (cnt_w == 0).any() and (cnt_w > 0).any()
    d_p, d_use, d_img, d_obs = _t(patches), _t(use), _t(img), _t(obs.astype(np.uint8))
    outs = {}
    for rows_per_pass in (None, 2):
        acc = torch.zeros(SHAPE, dtype=torch.float64, device='cuda')
        cnt = torch.zeros(SHAPE[:2], dtype=torch.int32, device='cuda')
        for row0, nrows in mi._passes(grows, gcols, 60 * patches.itemsize, rows_per_pass):
            sl = slice(row0 * gcols, (row0 + nrows) * gcols)
            mi._overlap_add_weighted(d_p[sl], d_use[sl], g, row0, nrows, acc, cnt)
        assert_array_equal(cnt.cpu().numpy(), cnt_w)
        err = rel_fro(acc.cpu().numpy(), acc_w)
        assert err <= TOL[np.dtype(dtype)], err
        for keep in (True, False):
            out = mi._inpaint_finish(acc, cnt, d_img, d_obs, keep).cpu().numpy()
            want = np_finish(acc_w, cnt_w, img, obs, keep)
            err = rel_fro(out, want)
            print('weighted overlap + finish', stride, np.dtype(dtype), rows_per_pass, keep, err)
            assert out.dtype == dtype and err <= TOL[np.dtype(dtype)], err
            assert_array_equal(out[cnt_w == 0], img[cnt_w == 0])             # uncovered pixels: the input
            if keep:
                assert_array_equal(out[obs], img[obs])
            outs.setdefault(keep, out)
            assert_array_equal(out, outs[keep])                              # whatever the cut into passes


# ---- GPU: transform(X, mask) -----------------------------------------------------------------------------------------
def _mixed_batch(dtype, seed=3, n=20, p=60, k=12):
    rs = np.random.RandomState(seed)
    D = rs.randn(k, p)
    D /= np.linalg.norm(D, axis=1, keepdims=True)
    X = (rs.randn(n, 4) @ rs.randn(4, p) + 0.3 * rs.randn(n, p)) / np.sqrt(p)
    mask = rs.rand(n, p) < 0.5
    mask[[0, 5, 9, 19]] = True                            # clean rows
    mask[[3, 12]] = False                                 # empty rows
    return D.astype(dtype), X.astype(dtype), mask


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', DTYPES)
def test_transform_with_a_full_mask_is_transform(dtype):
    import torch
    from modl_amd import Coder
    D, X, _ = _mixed_batch(dtype)
    coder = Coder(D, code_alpha=0.05)
    want = coder.transform(X)
    assert np.count_nonzero(want) > 0
    got = coder.transform(X, mask=np.ones(X.shape, dtype=bool))
    assert isinstance(got, np.ndarray) and got.dtype == dtype
    assert_array_equal(got, want)
    got_t = coder.transform(_t(X), mask=torch.ones(X.shape, dtype=torch.bool, device='cuda'))
    assert isinstance(got_t, torch.Tensor) and got_t.is_cuda
    assert_array_equal(got_t.cpu().numpy(), want)


@pytest.mark.gpu
@pytest.mark.parametrize('l1_ratio,pos', [(1.0, False), (0.0, False), (1.0, True), (0.5, False)])
def test_transform_with_a_mask_f64(oracle, l1_ratio, pos):
    from modl_amd import Coder
    D, X, mask = _mixed_batch(np.float64)
    n, k = X.shape[0], D.shape[0]
    alpha = 0.05
    coder = Coder(D, code_alpha=alpha, code_l1_ratio=l1_ratio, code_pos=pos)
    code = coder.transform(np.where(mask, X, np.nan), mask=mask)
    assert code.shape == (n, k) and code.dtype == np.float64 and np.isfinite(code).all()
    nobs = mask.sum(axis=1)
    clean, empty = np.flatnonzero(nobs == X.shape[1]), np.flatnonzero(nobs == 0)
    holed = np.flatnonzero((nobs > 0) & (nobs < X.shape[1]))
    assert len(clean) == 4 and len(empty) == 2 and len(holed) == n - 6
    assert_array_equal(code[empty], 0)
    assert_array_equal(code[clean], coder.transform(X[clean]))
    G, Dx, _ = np_masked_gram(D.T, X, mask, holed)
    want = np.ones((len(holed), k))
    oracle.enet_regression_multi_gram(G, Dx, np.ascontiguousarray(np.where(mask, X, 0)[holed]), want,
                                      np.arange(len(holed)), l1_ratio, alpha, pos, coder.tol, coder.max_iter)
    assert np.count_nonzero(want) > 0
    err = rel_fro(code[holed], want)
    print('transform with a mask, f64, l1_ratio', l1_ratio, 'pos', pos, err)
    assert err <= 1e-9, err


@pytest.mark.gpu
def test_transform_with_a_mask_f32_bookkeeping():
    """the device-made G_i / Dx_i of the holed rows through the public solver with the same arguments: the same bits as
    transform's holed rows (chunking and row bookkeeping, independent of a sweep-count flip); several chunks too"""
    import torch
    from modl_amd import Coder
    from modl_amd._lib import lib, check
    from modl_amd.device import ptr, stream_ptr
    from modl_amd.dict_fact import HipBackend
    D, X, mask = _mixed_batch(np.float32)
    n, k, p = X.shape[0], D.shape[0], X.shape[1]
    coder = Coder(D, code_alpha=0.05)
    code = coder.transform(X, mask=mask)
    be = coder._backend
    holed = np.flatnonzero((mask.sum(axis=1) > 0) & (mask.sum(axis=1) < p))
    Xz = _t(np.where(mask, X, 0).astype(np.float32))
    G, Dx, nobs = be.masked_gram(Xz, _t(mask.view(np.uint8)), _t(holed.astype(np.int64)))
    assert_array_equal(nobs.cpu().numpy(), mask.sum(axis=1)[holed])
    Xc = Xz[_t(holed.astype(np.int64))]
    out = torch.ones((len(holed), k), dtype=torch.float32, device='cuda')
    nbytes = lib.modl_enet_regression_workspace(0, len(holed), k, 1)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device='cuda')
    check(lib.modl_enet_regression_multi_gram_f32(ptr(G), ptr(Dx), ptr(Xc), p, p, ptr(out), None, len(holed), k,
                                                  coder.code_l1_ratio, coder.code_alpha, 0, coder.tol, coder.max_iter,
                                                  None, ptr(ws), nbytes, stream_ptr(be.device)))
    assert np.count_nonzero(out.cpu().numpy()) > 0
    assert_array_equal(code[holed], out.cpu().numpy())
    assert_array_equal(code[mask.sum(axis=1) == 0], 0)
    original = HipBackend.masked_chunk_rows
    try:                                                  # 5 rows per masked solve: the same codes, row by row
        HipBackend.masked_chunk_rows = lambda self: 5
        assert_array_equal(coder.transform(X, mask=mask), code)
    finally:
        HipBackend.masked_chunk_rows = original


# ---- GPU: inpaint ----------------------------------------------------------------------------------------------------
_FITTED = {}


def fitted(dtype, setting, k=6):
    """one small estimator per (dtype, setting, k), fitted on a clean 19 x 23 x 3 image, shared by the tests below"""
    from modl_amd.image import ImageDictFact
    from .test_wrappers import synth_image
    key = (np.dtype(dtype), setting, k)
    if key not in _FITTED:
        est = ImageDictFact(patch_size=PATCH, n_components=k, batch_size=20, alpha=0.1, random_state=0, max_patches=100,
                            reduction=2, setting=setting)
        with contextlib.redirect_stdout(io.StringIO()):
            est.fit(synth_image(19, 23, 3, seed=5).astype(dtype))
        _FITTED[key] = est
    return _FITTED[key]


def inpaint_image(dtype):
    """`holed_image` with the elements [0:4, 8:14] observed: the windows at (0, 8) and (0, 9), the latter an origin of
    both grids, are clean"""
    img, obs = holed_image(dtype)
    full = make_image(SHAPE, np.float64, seed=21)
    obs[0:4, 8:14, :] = True                              # holds the windows (0, 8) and (0, 9)
    img = np.where(obs, full, -1).astype(dtype)
    return np.ascontiguousarray(img), obs


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('setting', ['dictionary learning', 'NMF'])
def test_inpaint_without_the_solver(setting, dtype):
    """alpha = 1e6: the first sweep's soft threshold zeroes every coefficient (test_reconstruct_without_the_solver; the
    masked Gram's entries are at most p = 60 times larger), so a used window decodes to its observed-channel means
    ('dictionary learning') or to zero ('NMF') and the image follows exactly in numpy."""
    est = fitted(dtype, setting)
    img, obs = inpaint_image(dtype)
    est.dict_fact_.set_params(code_alpha=1e6)
    try:
        for stride in STRIDES:
            origins = restated_origins(SHAPE, PATCH, stride)[0]
            _, mean, _, _, nobs = np_masked_scaled(img, obs, origins, PATCH, setting != 'NMF', True)
            acc, cnt = np_weighted_overlap(np.tile(mean, PATCH[0] * PATCH[1]), nobs > 0, origins, SHAPE, PATCH)
            for keep in (True, False):
                out, filled = est.inpaint(img, stride=stride, keep_observed=keep, return_filled=True)
                assert out.shape == img.shape and out.dtype == dtype
                assert filled.dtype == bool and filled.shape == SHAPE[:2]
                assert_array_equal(filled, cnt > 0)
                want = np_finish(acc, cnt, img, obs, keep)
                err = rel_fro(out, want)
                print('inpaint, no solver', setting, np.dtype(dtype), stride, keep, err)
                assert err <= TOL[np.dtype(dtype)], err
                assert_array_equal(out[~filled], img[~filled])
                if keep:
                    assert_array_equal(out[obs], img[obs])
    finally:
        est.dict_fact_.set_params(code_alpha=0.1)


@pytest.mark.gpu
def test_inpaint_through_the_solver_f64():
    """k = 12, stride (2, 3), alpha = 0.1.  The checker codes the SAME device-made masked patches through the public
    transform(rows, mask=obs rows); decode, unscale, weighted overlap and finish are numpy."""
    import torch
    from modl_amd import image as mi
    est = fitted(np.float64, 'dictionary learning', k=12)
    img, obs = inpaint_image(np.float64)
    stride = (2, 3)
    g = mi._grid(SHAPE, PATCH, stride)
    grows, gcols = mi._grid_shape(g)
    rows, mean, den, orows, nobs = (t.cpu().numpy() for t in mi._grid_patches_masked_pass(
        _t(img), _t(obs.astype(np.uint8)), g, gcols, 0, grows, True, True))
    assert (nobs == 60).any() and (nobs == 0).any() and ((nobs > 0) & (nobs < 60)).any()
    code = est.dict_fact_.transform(rows, mask=orows != 0)
    assert np.count_nonzero(code[nobs == 60]) > 0 and np.count_nonzero(code[(nobs > 0) & (nobs < 60)]) > 0
    assert_array_equal(code[nobs == 0], 0)
    D = est.components_.reshape(12, -1)
    reps = PATCH[0] * PATCH[1]
    origins = restated_origins(SHAPE, PATCH, stride)[0]
    acc, cnt = np_weighted_overlap((code @ D) * np.tile(den, reps) + np.tile(mean, reps), nobs > 0, origins, SHAPE, PATCH)
    outs = []
    for keep in (True, False):
        want = np_finish(acc, cnt, img, obs, keep)
        for rows_per_pass in (None, 2):
            out, filled = est.inpaint(img, stride=stride, keep_observed=keep, rows_per_pass=rows_per_pass,
                                      return_filled=True)
            err = rel_fro(out, want)
            print('inpaint through the solver, keep', keep, 'rows_per_pass', rows_per_pass, err)
            assert err <= 1e-9, err
            assert_array_equal(filled, cnt > 0)
            assert_array_equal(out[~filled], img[~filled])
            if keep:
                assert_array_equal(out[obs], img[obs])
            outs.append(out)
    # an explicit mask, (H, W, C) or - where all channels of a pixel go together - (H, W); a CUDA tensor in and out
    other = est.inpaint(np.where(obs, img, 7.0), mask=obs, stride=stride)   # what the missing elements hold is not used
    covered = np.repeat((cnt > 0)[:, :, None], 3, axis=2)
    assert_array_equal(other[covered], outs[0][covered])
    assert_array_equal(other[~covered & ~obs], 7.0)
    pix = obs.all(axis=2)
    img_p = np.where(pix[:, :, None], make_image(SHAPE, np.float64, seed=21), -1)
    a = est.inpaint(img_p, mask=pix, stride=stride)
    assert_array_equal(a, est.inpaint(img_p, mask=np.repeat(pix[:, :, None], 3, axis=2), stride=stride))
    assert_array_equal(a, est.inpaint(img_p, stride=stride))
    out_t = est.inpaint(torch.from_numpy(img).cuda(), stride=stride)
    assert isinstance(out_t, torch.Tensor) and out_t.is_cuda and out_t.dtype == torch.float64
    assert_array_equal(out_t.cpu().numpy(), outs[0])


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', DTYPES)
def test_inpaint_without_holes_is_reconstruct(dtype):
    est = fitted(dtype, 'dictionary learning')
    img = make_image(SHAPE, dtype, seed=7)
    for stride in STRIDES:
        want = est.reconstruct(img, stride=stride)
        assert_array_equal(est.inpaint(img, stride=stride, keep_observed=False), want)
        assert_array_equal(est.inpaint(img, stride=stride, keep_observed=False, rows_per_pass=2), want)
        out, filled = est.inpaint(img, stride=stride, return_filled=True)    # keep_observed: the image itself
        assert_array_equal(out, img)
        assert filled.all()
