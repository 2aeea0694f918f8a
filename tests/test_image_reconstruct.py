"""Reconstruction of an image from the codes of its patches: the patch grid, grid patches that keep their scaling,
decode with unscale, overlap-add and finish (csrc/image.hip), `CodingMixin.inverse_transform`, `modl_amd.image`'s
`grid_origins` / `grid_patches` / `reconstruct_from_patches` and `ImageDictFact.reconstruct`.

The checkers are plain numpy in f64, written here: the grid rule restated as a loop, `scale_patches`' arithmetic with
the statistics kept, and a Python overlap loop.  Tolerances, rel_fro against the f64 checker:
f64 <= 1e-12, f32 <= 1e-5, f64 end to end through the solver <= 1e-9.  Shapes: image 19 x 23 x 3 with patch (4, 5) is
the smallest at which every index path can go wrong (sizes that are no multiple of the stride: the last origin is
clamped and rows / columns are double-covered; 304 patches at stride 1: 76 workgroups)."""
import contextlib
import ctypes as C
import io

import numpy as np
import pytest
from numpy.testing import assert_array_equal

from .conftest import rel_fro

PATCH = (4, 5)
# (image shape, stride)
GRIDS = [((19, 23, 3), (1, 1)), ((19, 23, 3), (2, 3)), ((19, 23, 3), (3, 2)),
         ((19, 23, 3), (4, 5)),                         # stride == patch: no overlap except at the clamp
         ((19, 23, 1), (2, 3)), ((19, 23, 5), (3, 2)),
         ((4, 5, 3), (1, 1))]                           # one patch is the whole image
DTYPES = [np.float32, np.float64]
TOL = {np.dtype(np.float32): 1e-5, np.dtype(np.float64): 1e-12}


# ---- the checkers -----------------------------------------------------------------------------------------------------
def axis_origins(L, x, s):
    o, t = [], 0
    while t <= L - x:
        o.append(t)
        t += s
    if o[-1] != L - x:
        o.append(L - x)
    return o


def restated_origins(shape, patch, stride):
    oi, oj = axis_origins(shape[0], patch[0], stride[0]), axis_origins(shape[1], patch[1], stride[1])
    return np.array([(i, j, 0) for i in oi for j in oj], dtype=np.int64).reshape(-1, 3), len(oi), len(oj)


def np_scaled(image, origins, patch, with_mean, with_std):
    """scale_patches' arithmetic in f64 on the windows at `origins`, the statistics kept: rows, mean (n, C), den (n, C)"""
    x, y = patch
    X = np.stack([image[i:i + x, j:j + y, :] for i, j, _ in origins]).astype(np.float64)
    n, c = X.shape[0], X.shape[3]
    mean = X.mean(axis=(1, 2)) if with_mean else np.zeros((n, c))
    X = X - mean[:, None, None, :]
    den = np.ones((n, c))
    if with_std:
        norm = np.sqrt(np.square(X).sum(axis=(1, 2)))
        norm[norm == 0] = 1
        den = norm * np.sqrt(c)
    X = X / den[:, None, None, :]
    return X.reshape(n, -1), mean, den


def np_overlap(patches, origins, shape, patch):
    x, y = patch
    acc, cnt = np.zeros(shape), np.zeros(shape)
    for row, (i, j, _) in zip(np.asarray(patches, dtype=np.float64), origins):
        acc[i:i + x, j:j + y, :] += row.reshape(x, y, shape[2])
        cnt[i:i + x, j:j + y, :] += 1
    assert cnt.min() >= 1
    return acc / cnt


def make_image(shape, dtype, seed=0):
    rs = np.random.RandomState(seed)
    img = rs.rand(*shape)
    if shape[0] >= 8:
        img[0:4, 0:5, :] = 0.5                          # a constant patch at origin (0, 0): exact sums, zero norm
    return np.ascontiguousarray(img.astype(dtype))

# ---- CPU --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,stride', GRIDS)
def test_grid_origins_follow_the_rule(shape, stride):
    from modl_amd import grid_origins
    from modl_amd._lib import lib
    got = grid_origins(shape, PATCH, stride)
    want, grows, gcols = restated_origins(shape, PATCH, stride)
    assert got.dtype == np.int64
    assert_array_equal(got, want)
    cnt = np.zeros(shape[:2], dtype=int)
    for i, j, _ in got:
        cnt[i:i + PATCH[0], j:j + PATCH[1]] += 1
    assert cnt.min() >= 1                                # full coverage, the border included
    assert got[-1, 0] == shape[0] - PATCH[0] and got[-1, 1] == shape[1] - PATCH[1]
    r, c = C.c_int64(), C.c_int64()
    assert lib.modl_image_grid_shape(shape[0], shape[1], PATCH[0], PATCH[1], stride[0], stride[1], C.byref(r), C.byref(c)) == 0
    assert (r.value, c.value) == (grows, gcols)
    assert_array_equal(grid_origins(shape, PATCH, 1), restated_origins(shape, PATCH, (1, 1))[0])     # int stride

def test_bad_arguments_are_einval_before_any_device_work():
    """the host-side checks of every new export: no GPU is touched (the pointers are host arrays, never read)"""
    from modl_amd._lib import lib
    buf = np.zeros(4096)
    p = buf.ctypes.data_as(C.c_void_p)
    r, c = C.c_int64(), C.c_int64()
    gs = lambda *a: lib.modl_image_grid_shape(*a, C.byref(r), C.byref(c))
    assert gs(19, 23, 4, 5, 5, 1) == -1                  # stride > patch
    assert gs(19, 23, 4, 5, 1, 6) == -1
    assert gs(19, 23, 4, 5, 0, 1) == -1                  # stride < 1
    assert gs(3, 23, 4, 5, 1, 1) == -1                   # image smaller than the patch
    assert gs(19, 4, 4, 5, 1, 1) == -1
    assert gs(19, 23, 0, 5, 1, 1) == -1
    assert lib.modl_image_grid_shape(19, 23, 4, 5, 1, 1, None, C.byref(c)) == -1
    for sfx in ('f32', 'f64'):
        gp = getattr(lib, 'modl_image_grid_patches_' + sfx)
        ok = dict(H=19, W=23, C=3, x=4, y=5, si=2, sj=3, row0=0, nrows=9, ldo=60, img=p, out=p, mean=p, den=p)
        for bad in (dict(si=5), dict(sj=6), dict(si=0), dict(H=3), dict(W=4), dict(C=0), dict(C=1025), dict(row0=-1),
                    dict(nrows=10), dict(row0=5, nrows=5), dict(nrows=-1), dict(ldo=59), dict(img=None), dict(out=None),
                    dict(mean=None), dict(den=None)):
            a = dict(ok, **bad)
            assert gp(a['img'], a['H'], a['W'], a['C'], a['x'], a['y'], a['si'], a['sj'], a['row0'], a['nrows'], 1, 1,
                      a['out'], a['ldo'], a['mean'], a['den'], None) == -1, bad
        dec = getattr(lib, 'modl_image_decode_' + sfx)
        assert dec(p, 10, 0, p, 60, 3, p, p, p, 60, None) == -1            # k < 1
        assert dec(p, 10, 7, p, 0, 3, p, p, p, 60, None) == -1             # P < 1
        assert dec(p, 10, 7, p, 60, 3, p, p, p, 59, None) == -1            # ldo < P
        assert dec(p, 10, 7, p, 60, 7, p, p, p, 60, None) == -1            # P no multiple of C
        assert dec(p, 10, 7, p, 60, 0, p, p, p, 60, None) == -1
        assert dec(p, 10, 7, p, 60, 3, p, None, p, 60, None) == -1         # mean without den
        assert dec(p, 10, 7, p, 60, 3, None, p, p, 60, None) == -1
        assert dec(None, 10, 7, p, 60, 3, p, p, p, 60, None) == -1
        assert dec(p, -1, 7, p, 60, 3, p, p, p, 60, None) == -1
        add = getattr(lib, 'modl_image_overlap_add_' + sfx)
        assert add(p, 60, 19, 23, 3, 4, 5, 5, 3, 0, 9, p, None) == -1
        assert add(p, 59, 19, 23, 3, 4, 5, 2, 3, 0, 9, p, None) == -1
        assert add(p, 60, 19, 23, 3, 4, 5, 2, 3, 0, 10, p, None) == -1
        assert add(p, 60, 19, 23, 3, 4, 5, 2, 3, 0, 9, None, None) == -1
        assert add(None, 60, 19, 23, 3, 4, 5, 2, 3, 0, 9, p, None) == -1
        fin = getattr(lib, 'modl_image_overlap_finish_' + sfx)
        assert fin(p, 19, 23, 3, 4, 5, 2, 6, p, None) == -1
        assert fin(p, 3, 23, 3, 4, 5, 2, 3, p, None) == -1
        assert fin(p, 19, 23, 1025, 4, 5, 2, 3, p, None) == -1
        assert fin(None, 19, 23, 3, 4, 5, 2, 3, p, None) == -1
        assert fin(p, 19, 23, 3, 4, 5, 2, 3, None, None) == -1

def test_bad_arguments_raise_valueerror_without_gpu():
    from modl_amd import grid_origins, grid_patches, reconstruct_from_patches
    from modl_amd.image import ImageDictFact
    from .test_wrappers import _image_estimator, synth_image
    img = np.zeros((19, 23, 3))
    for fn in (lambda **k: grid_origins(img.shape, **k), lambda **k: grid_patches(img, **k),
               lambda **k: reconstruct_from_patches(np.zeros((4, 60)), img.shape, **k)):
        for bad in (dict(patch_size=PATCH, stride=(5, 1)), dict(patch_size=PATCH, stride=6), dict(patch_size=PATCH, stride=0),
                    dict(patch_size=(20, 5), stride=1), dict(patch_size=(4, 24), stride=1)):
            with pytest.raises(ValueError):
                fn(**bad)
    with pytest.raises(ValueError):
        grid_origins((19, 23), PATCH, 1)
    with pytest.raises(ValueError):
        ImageDictFact(patch_size=PATCH).reconstruct(img)                   # unfitted
    est = _image_estimator(True)(patch_size=PATCH, n_components=5, batch_size=10, alpha=0.1, random_state=0,
                                 max_patches=40, reduction=2)
    with contextlib.redirect_stdout(io.StringIO()):
        est.fit(synth_image(19, 23, 3, seed=2))
    for bad_img, stride in ((np.zeros((19, 23, 1)), 1),                     # channels differ from the fitted 3
                            (np.zeros((19, 23, 3)), (5, 1)), (np.zeros((19, 23, 3)), (1, 6)),
                            (np.zeros((3, 23, 3)), 1), (np.zeros((19, 4, 3)), 1)):
        with pytest.raises(ValueError):
            est.reconstruct(bad_img, stride=stride)

# ---- GPU --------------------------------------------------------------------------------------------------------------
def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()

@pytest.mark.gpu
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape,stride', GRIDS)
def test_grid_patches(shape, stride, dtype):
    from modl_amd import grid_origins, grid_patches
    from modl_amd import image as mi
    from modl_amd.dict_fact import HipBackend
    img = make_image(shape, dtype)
    origins = grid_origins(shape, PATCH, stride)
    be = HipBackend()
    d_img = be.stage_image(img)
    g = mi._grid(shape, PATCH, stride)
    grows, gcols = mi._grid_shape(g)
    combos = [(True, True), (True, False), (False, True), (False, False)] if shape == (19, 23, 3) and stride == (2, 3) \
        else [(True, True)]
    for with_mean, with_std in combos:
        rows, mean, den = grid_patches(d_img, PATCH, stride, with_mean, with_std)
        assert rows.dtype == d_img.dtype and tuple(rows.shape) == (len(origins), PATCH[0] * PATCH[1] * shape[2])
        assert tuple(mean.shape) == tuple(den.shape) == (len(origins), shape[2])
        # bit-equal to the training path's kernel on the same origins
        old = be.image_patches(d_img, origins, PATCH + (shape[2],), with_mean, with_std)
        assert_array_equal(rows.cpu().numpy(), old.cpu().numpy())
        want_rows, want_mean, want_den = np_scaled(img, origins, PATCH, with_mean, with_std)
        errs = (rel_fro(rows.cpu().numpy(), want_rows), rel_fro(mean.cpu().numpy(), want_mean),
                rel_fro(den.cpu().numpy(), want_den))
        print('grid patches', shape, stride, np.dtype(dtype), with_mean, with_std, errs)
        assert max(errs) <= TOL[np.dtype(dtype)], errs
        if shape[0] >= 8 and with_mean and with_std:      # the constant patch: zero row, divisor 1 * sqrt(C), exact mean
            assert_array_equal(rows[0].cpu().numpy(), 0)
            assert_array_equal(mean[0].cpu().numpy(), dtype(0.5))
            assert_array_equal(den[0].cpu().numpy(), dtype(np.sqrt(np.float64(shape[2]))))
        # a pass is the matching slice of the full call, bit for bit
        for row0, nrows in ((0, 1), (grows - 1, 1), (grows // 3, grows - grows // 3)):
            part = mi._grid_patches_pass(d_img, g, gcols, row0, nrows, with_mean, with_std)
            for a, b in zip(part, (rows, mean, den)):
                assert_array_equal(a.cpu().numpy(), b[row0 * gcols:(row0 + nrows) * gcols].cpu().numpy())

@pytest.mark.gpu
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('k', [7, 300])
def test_decode_and_inverse_transform(k, dtype):
    import torch
    from modl_amd import Coder, DictFact
    rs = np.random.RandomState(k)
    n, P, c = 37, 60, 3
    X = rs.randn(max(k, n), P).astype(dtype)
    code = (rs.randn(n, k) * (rs.rand(n, k) < 0.3)).astype(dtype)
    mean, den = rs.randn(n, c).astype(dtype), (0.5 + rs.rand(n, c)).astype(dtype)
    est = DictFact(n_components=k, random_state=0).prepare(n_samples=X.shape[0], X=X)
    D = est.components_
    assert D.dtype == dtype and D.shape == (k, P)
    tol = TOL[np.dtype(dtype)]
    plain = code.astype(np.float64) @ D.astype(np.float64)
    be = est._backend
    got = be.decode(_t(code)).cpu().numpy()
    got_u = be.decode(_t(code), _t(mean), _t(den)).cpu().numpy()
    want_u = plain * np.tile(den.astype(np.float64), P // c) + np.tile(mean.astype(np.float64), P // c)
    errs = rel_fro(got, plain), rel_fro(got_u, want_u)
    print('decode', k, np.dtype(dtype), errs)
    assert max(errs) <= tol, errs
    coder = Coder(D)
    for e in (est, coder):
        out = e.inverse_transform(code)
        assert isinstance(out, np.ndarray) and out.dtype == dtype and out.shape == (n, P)
        assert_array_equal(out, got)
        out_t = e.inverse_transform(_t(code))
        assert isinstance(out_t, torch.Tensor) and out_t.is_cuda
        assert_array_equal(out_t.cpu().numpy(), got)
    with pytest.raises(ValueError):
        est.inverse_transform(code[:, :-1])

@pytest.mark.gpu
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape,stride', GRIDS)
def test_overlap_add_and_finish(shape, stride, dtype):
    import torch
    from modl_amd import reconstruct_from_patches
    origins, grows, _ = restated_origins(shape, PATCH, stride)
    rs = np.random.RandomState(3)
    patches = rs.randn(len(origins), PATCH[0] * PATCH[1] * shape[2]).astype(dtype)
    want = np_overlap(patches, origins, shape, PATCH)
    one = reconstruct_from_patches(patches, shape, PATCH, stride)
    assert isinstance(one, np.ndarray) and one.dtype == dtype and one.shape == shape
    err = rel_fro(one, want)
    print('overlap', shape, stride, np.dtype(dtype), err)
    assert err <= TOL[np.dtype(dtype)], err
    assert_array_equal(reconstruct_from_patches(patches, shape, PATCH, stride), one)          # run to run
    assert_array_equal(reconstruct_from_patches(patches, shape, PATCH, stride, rows_per_pass=1), one)
    uneven = [r for r in range(2, grows) if grows % r]
    if uneven:                                            # a pass size that does not divide the grid rows
        assert_array_equal(reconstruct_from_patches(patches, shape, PATCH, stride, rows_per_pass=uneven[-1]), one)
    out_t = reconstruct_from_patches(_t(patches), shape, PATCH, stride, rows_per_pass=2)
    assert isinstance(out_t, torch.Tensor) and out_t.is_cuda
    assert_array_equal(out_t.cpu().numpy(), one)

_FITTED = {}

def fitted(dtype, setting, k=6):
    """one small fitted estimator per (dtype, setting, k), shared by the tests below"""
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

@pytest.mark.gpu
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('setting', ['dictionary learning', 'NMF'])
def test_reconstruct_without_the_solver(setting, dtype):
    """alpha = 1e6: from the warm start of ones the first sweep's soft threshold zeroes every coefficient
    (|q_i - sum_j G_ij w_j| <= 1 + k on unit-norm patches and atoms), so the decoded patch is its channel means
    ('dictionary learning') or zero ('NMF', with_mean=False) and the image follows exactly in numpy."""
    est = fitted(dtype, setting)
    img = make_image((19, 23, 3), dtype, seed=7)
    est.dict_fact_.set_params(code_alpha=1e6)
    try:
        for stride in ((1, 1), (2, 3)):
            out = est.reconstruct(img, stride=stride)
            assert out.shape == img.shape and out.dtype == dtype
            if setting == 'NMF':
                assert_array_equal(out, 0)
                continue
            origins = restated_origins(img.shape, PATCH, stride)[0]
            _, mean, _ = np_scaled(img, origins, PATCH, True, True)
            want = np_overlap(np.tile(mean, PATCH[0] * PATCH[1]), origins, img.shape, PATCH)
            err = rel_fro(out, want)
            print('reconstruct, no solver', np.dtype(dtype), stride, err)
            assert err <= TOL[np.dtype(dtype)], err
    finally:
        est.dict_fact_.set_params(code_alpha=0.1)

@pytest.mark.gpu
def test_reconstruct_through_the_solver_f64():
    """k = 12, stride (2, 3), alpha = 0.1.  The checker codes the SAME device-made patches through the public transform,
    so the solver's input bits agree on both sides; decode, unscale and overlap are numpy."""
    from modl_amd import grid_patches
    est = fitted(np.float64, 'dictionary learning', k=12)
    img = make_image((19, 23, 3), np.float64, seed=11)
    stride = (2, 3)
    rows, mean, den = (t.cpu().numpy() for t in grid_patches(img, PATCH, stride, True, True))
    code = est.dict_fact_.transform(rows)
    assert np.count_nonzero(code) > 0                     # the solver really contributes
    D = est.components_.reshape(12, -1)
    reps = PATCH[0] * PATCH[1]
    origins = restated_origins(img.shape, PATCH, stride)[0]
    want = np_overlap((code @ D) * np.tile(den, reps) + np.tile(mean, reps), origins, img.shape, PATCH)
    for rows_per_pass in (None, 2):
        out = est.reconstruct(img, stride=stride, rows_per_pass=rows_per_pass)
        err = rel_fro(out, want)
        print('reconstruct through the solver, rows_per_pass', rows_per_pass, err)
        assert err <= 1e-9, err

@pytest.mark.gpu
def test_reconstruct_shape_and_dtype():
    import torch
    est = fitted(np.float32, 'dictionary learning')
    img64 = make_image((21, 26, 3), np.float64, seed=13)  # another size than the fitted image's
    out = est.reconstruct(img64, stride=3)
    assert isinstance(out, np.ndarray) and out.shape == img64.shape and out.dtype == np.float32
    assert np.isfinite(out).all()
    out_t = est.reconstruct(torch.from_numpy(img64).cuda(), stride=3)
    assert isinstance(out_t, torch.Tensor) and out_t.dtype == torch.float32 and tuple(out_t.shape) == img64.shape
    assert_array_equal(out_t.cpu().numpy(), out)
