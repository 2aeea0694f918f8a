"""Smoothing and masking of fMRI volumes (modl_amd/masker.py, csrc/masker.hip).

nilearn is not installed, so nothing is pinned to a run of it: its smoothing is scipy.ndimage.gaussian_filter1d per spatial
axis (mode 'reflect'), and that is the yardstick.

THE JUDGE.  `ref` is the f64 restatement below: non-finite -> 0, then per axis a with sigma_a = fwhm_a / (sqrt(8 ln 2) v_a) > 0
a correlation with w[j] = exp(-j^2 / (2 sigma_a^2)), j = -r_a .. r_a, r_a = int(4 sigma_a + 0.5), normalised, over the index
reflected with period 2 n; sums in f64, nothing rounded in between.  With M the largest |finite element| of the frame an
element passes if

    |got - ref| <= (3 eps_out / 2 (1 + 4 eps_out) + 2 sum_a (2 r_a + 2) eps64) M

The weights are non-negative and sum to 1, so every pass is a contraction: each of at most three roundings to the output
dtype adds at most eps_out / 2 M, an f64 sum of 2 r + 1 products at most (2 r + 2) eps64 M / 2 per axis, and the bound doubles
that.  With all radii 0 the judge is bit equality with vol[mask].T after zeroing the non-finite elements.  The mutants of
MUTANTS (a wrong boundary, radius, normalisation, sigma, axis, order of mask and smoothing, column order, NaN handling) are
rejected: measured on the cases below they sit at 8e-2 M or more, except the radius int(4 sigma), whose missing outermost
taps weigh 3.7e-5 M - still 200 times the f32 bound of 1.8e-7 M.

Layer 1 (no GPU): the restatement against scipy, the mutants, gaussian_weights, the host path, every ValueError, the refusals
of the entry points, the estimators on the oracle backend.  Layer 2 (gpu): the kernels through the C-ABI, determinism,
modl_unmask, the refusals with the output untouched, the Python functions and the estimators on the device.

The module imports modl_amd.masker at the top, so none of its tests can pass without the feature - also the two that look
only at the yardstick itself (the restatement against scipy, the judge against the mutants)."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.ndimage

from modl_amd import masker as _masker  # noqa: F401  (see the module docstring)

from .test_clean import SENT, DT, EINVAL, ENOMEM, ENOGPU, same_bits

EPS64 = float(np.finfo(np.float64).eps)
F2S = np.sqrt(8.0 * np.log(2.0))
MUTANTS = ('nearest', 'mirror', 'radius', 'unnormalised', 'no_voxel', 'swap_sigmas', 'mask_first', 'keep_nonfinite',
           'fortran_columns')

# (spatial shape, T, fwhm, voxel size): the shapes and widths of the issue; radii up to 20 on axes of length 3
CASES = {'7x5x3': ((7, 5, 3), 4, 6.0, (2.0, 2.0, 2.0)),
         '17x9x2': ((17, 9, 2), 3, 6.0, (2.0, 1.5, 3.0)),
         '1x6x33': ((1, 6, 33), 2, 4.0, (2.0, 2.0, 1.0)),
         '20x19x18': ((20, 19, 18), 2, 8.0, (3.0, 2.0, 2.5)),          # 4 sigma_x = 4.53: int(4 sigma) is another radius
         '5x4x3': ((5, 4, 3), 2, 12.0, (1.0, 1.0, 1.0)),
         'per axis': ((9, 8, 7), 2, (6.0, 0.0, None), (2.0, 2.0, 2.0))}


# ------------------------------------------------------------------------------------------- the restatement (numpy)
def sigmas_of(fwhm, voxel, mutant=None):
    fw = list(fwhm) if np.ndim(fwhm) else [fwhm] * 3
    sig = [0.0 if f is None else float(f) / F2S / (1.0 if mutant == 'no_voxel' else v) for f, v in zip(fw, voxel)]
    if mutant == 'swap_sigmas':
        sig[0], sig[1] = sig[1], sig[0]
    return sig


def radii_of(fwhm, voxel):
    return [int(4.0 * s + 0.5) if s > 0 else 0 for s in sigmas_of(fwhm, voxel)]


def _index(i, n, mutant):
    if mutant == 'nearest':
        return min(max(i, 0), n - 1)
    if mutant == 'mirror':                                # d c b | a b c d | c b a, period 2 n - 2
        if n == 1:
            return 0
        i %= 2 * n - 2
        return i if i < n else 2 * n - 2 - i
    i %= 2 * n                                            # 'reflect': d c b a | a b c d | d c b a, period 2 n
    return i if i < n else 2 * n - 1 - i


def restate_axis(a, sigma, axis, mutant=None):
    r = int(4.0 * sigma) if mutant == 'radius' else int(4.0 * sigma + 0.5)
    if r == 0:
        return a
    j = np.arange(-r, r + 1, dtype=np.float64)
    w = np.exp(-j * j / (2.0 * sigma * sigma))
    if mutant != 'unnormalised':
        w = w / w.sum()
    n = a.shape[axis]
    out = np.zeros_like(a)
    with np.errstate(invalid='ignore'):                   # (the mutant that keeps NaN and Inf)
        for k in range(2 * r + 1):                        # ascending tap order
            idx = [_index(i + k - r, n, mutant) for i in range(n)]
            out += w[k] * np.take(a, idx, axis=axis)
    return out


def restate(vol, fwhm, voxel, mask=None, mutant=None):
    """steps 1-2 on (X, Y, Z, T) in f64: the smoothed volume"""
    a = np.array(vol, dtype=np.float64)
    if mutant != 'keep_nonfinite':
        a[~np.isfinite(a)] = 0.0
    if mutant == 'mask_first':
        a[~mask] = 0.0
    for axis, s in enumerate(sigmas_of(fwhm, voxel, mutant)):
        if s > 0:
            a = restate_axis(a, s, axis, mutant)
    return a


def rows_of(a, mask, mutant=None):
    """step 3: (T, V)"""
    if mutant == 'fortran_columns':
        return a.transpose(2, 1, 0, 3)[mask.transpose(2, 1, 0)].T
    return a[mask].T


def frame_max(vol):
    """M per frame: the largest |finite element|"""
    a = np.abs(np.where(np.isfinite(vol), vol, 0).astype(np.float64))
    return a.reshape(-1, a.shape[3]).max(axis=0)


def bound(eps_out, radii):
    return 3 * eps_out / 2 * (1 + 4 * eps_out) + 2 * sum(2 * r + 2 for r in radii if r > 0) * EPS64


def judge(got, ref, M, eps_out, radii):
    """(passes, worst error over its bound); got, ref (T, V), M (T,)"""
    with np.errstate(invalid='ignore'):
        err = np.abs(np.asarray(got, dtype=np.float64) - ref) / (bound(eps_out, radii) * M[:, None])
    return bool(np.all(err <= 1.0)), float(np.max(np.where(np.isnan(err), np.inf, err)))


def scipy_chain(vol, fwhm, voxel):
    """nilearn's _smooth_array: in place, axis by axis, in the array's dtype"""
    arr = np.array(vol)
    arr[~np.isfinite(arr)] = 0
    for axis, s in enumerate(sigmas_of(fwhm, voxel)):
        if s > 0:
            scipy.ndimage.gaussian_filter1d(arr, s, output=arr, axis=axis)
    return arr


def volume(shape, T, dtype, seed, plant=True):
    rs = np.random.RandomState(seed)
    vol = (100 + 20 * rs.randn(*shape, T)).astype(dtype)
    if plant:                                             # NaN, +Inf, -Inf: some land inside a mask, some outside
        flat = vol.reshape(-1)
        pos = rs.choice(flat.shape[0], size=min(6, flat.shape[0] // 4), replace=False)
        flat[pos] = np.resize(np.array([np.nan, np.inf, -np.inf], dtype=dtype), pos.shape[0])
    return vol


def random_mask(shape, seed, p=0.5):
    rs = np.random.RandomState(seed)
    m = rs.rand(*shape) < p
    m.reshape(-1)[rs.randint(m.size)] = True
    return m


@functools.lru_cache(maxsize=None)
def case(name, dt):
    """(vol, mask, ref rows, M, radii) - computed once, never written to"""
    shape, T, fwhm, voxel = CASES[name]
    vol = volume(shape, T, DT[dt], seed=len(name))
    mask = random_mask(shape, seed=7)
    flat = np.flatnonzero(~np.isfinite(vol.reshape(-1, T)).all(axis=1))
    mask.reshape(-1)[flat[::2]] = True                    # planted elements on both sides of the mask
    mask.reshape(-1)[flat[1::2]] = False
    if not mask.any():
        mask.reshape(-1)[0] = True
    ref = rows_of(restate(vol, fwhm, voxel), mask)
    for a in (vol, mask, ref):
        a.setflags(write=False)
    return vol, mask, ref, frame_max(vol), radii_of(fwhm, voxel)


# ------------------------------------------------------------------------------------------------ layer 1: no GPU
@pytest.mark.parametrize('name', list(CASES))
def test_restatement_against_scipy(name):
    shape, T, fwhm, voxel = CASES[name]
    radii = radii_of(fwhm, voxel)
    vol, mask, ref, M, _ = case(name, 'f64')
    got = rows_of(scipy_chain(vol, fwhm, voxel), mask)
    err = np.abs(got - ref) / M[:, None]
    print(name, 'f64 scipy - restatement: %.3g M' % err.max())
    assert err.max() <= 2 * sum(2 * r + 2 for r in radii if r > 0) * EPS64
    vol32, mask32, ref32, M32, _ = case(name, 'f32')
    ok, worst = judge(rows_of(scipy_chain(vol32, fwhm, voxel), mask32), ref32, M32, float(np.finfo(np.float32).eps), radii)
    print(name, 'f32 scipy: %.3g of the bound' % worst)
    assert ok, worst


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_judge_rejects_mutants(dt):
    eps_out = float(np.finfo(DT[dt]).eps)
    caught = {m: [] for m in MUTANTS}
    for name, (shape, T, fwhm, voxel) in CASES.items():
        vol, mask, ref, M, radii = case(name, dt)
        good = rows_of(restate(vol, fwhm, voxel).astype(DT[dt]), mask)         # the restatement, rounded once: accepted
        assert judge(good, ref, M, eps_out, radii)[0], name
        for m in MUTANTS:
            bad = rows_of(restate(vol, fwhm, voxel, mask, mutant=m), mask, mutant=m).astype(DT[dt])
            if not judge(bad, ref, M, eps_out, radii)[0]:
                caught[m].append(name)
    assert all(caught.values()), {m: c for m, c in caught.items() if not c}
    assert '20x19x18' in caught['radius'] and '17x9x2' in caught['swap_sigmas']


def test_gaussian_weights_against_scipy():
    from modl_amd.masker import gaussian_weights
    for sigma in (0.2548, 0.849, 1.274, 1.1324, 1.699, 2.017, 5.096):
        w, r = gaussian_weights(sigma)
        assert r == int(4 * sigma + 0.5) and w.shape == (2 * r + 1,) and w.dtype == np.float64
        assert abs(w.sum() - 1.0) <= 4 * EPS64 and np.all(w > 0)
        impulse = np.zeros(4 * r + 1)
        impulse[2 * r] = 1.0
        got = scipy.ndimage.gaussian_filter1d(impulse, sigma)[r:3 * r + 1]     # correlating a unit impulse: w reversed,
        assert np.max(np.abs(got - w[::-1])) <= 4 * EPS64                        # and w is symmetric
    for none in (0, 0.0, None, 0.1):                                             # int(4 * 0.1 + 0.5) == 0
        w, r = gaussian_weights(none)
        assert r == 0 and np.array_equal(w, [1.0])
    for bad in (-1.0, np.nan, np.inf):
        with pytest.raises(ValueError):
            gaussian_weights(bad)


def test_host_path_and_round_trip():
    from modl_amd.masker import smooth_mask_host, unmask_host, ArrayMasker
    for name, (shape, T, fwhm, voxel) in CASES.items():
        for dt in ('f32', 'f64'):
            vol, mask, ref, M, radii = case(name, dt)
            got = smooth_mask_host(vol, mask, fwhm, voxel)
            assert got.shape == ref.shape and got.dtype == DT[dt] and got.flags.c_contiguous
            assert judge(got, ref, M, float(np.finfo(DT[dt]).eps), radii)[0], (name, dt)
            plain = smooth_mask_host(vol, mask)                                  # no smoothing: the masking alone, exact
            assert same_bits(plain, np.where(np.isfinite(vol), vol, 0)[mask].T)
            back = unmask_host(plain, mask)
            assert back.shape == shape + (T,) and back.dtype == DT[dt]
            assert np.all(back[~mask] == 0) and same_bits(back[mask].T, plain)
            assert same_bits(smooth_mask_host(back, mask), plain)
            perm = np.random.RandomState(1).permutation(T)
            moved = smooth_mask_host(vol, mask, fwhm, voxel, dst_row=perm)
            assert same_bits(moved[perm], got)
            assert same_bits(smooth_mask_host(np.asfortranarray(vol), mask, fwhm, voxel), got)
    vol, mask, ref, M, radii = case('7x5x3', 'f64')
    assert same_bits(smooth_mask_host(vol[..., 0], mask, 6.0, (2, 2, 2)), smooth_mask_host(vol[..., :1], mask, 6.0, (2, 2, 2)))
    assert smooth_mask_host(np.ones((7, 5, 3, 2), np.int16), mask).dtype == np.float64       # any other dtype: f64


def test_array_masker_on_host_arrays():
    from modl_amd import _lib
    from modl_amd.masker import ArrayMasker, smooth_mask, unmask, smooth_mask_host
    from modl_amd.signal import clean
    shape, T = (6, 5, 4), 40
    vol = volume(shape, T, np.float64, seed=3)
    mask = random_mask(shape, seed=2)
    m = ArrayMasker(mask, voxel_size=(2, 2, 2), smoothing_fwhm=6, standardize=True, detrend=True, high_pass=0.01, t_r=2.0)
    with pytest.raises(ValueError):
        m.transform(vol)                                                         # not fitted
    assert m.fit() is m and m.n_voxels_ == mask.sum()
    rows = smooth_mask(vol, mask, 6, (2, 2, 2))
    assert rows.shape == (T, mask.sum()) and isinstance(rows, np.ndarray)
    if _lib.lib.modl_device_count() == 0:
        assert same_bits(rows, smooth_mask_host(vol, mask, 6, (2, 2, 2)))
    got = m.transform(vol)
    assert same_bits(got, clean(rows, True, True, None, high_pass=0.01, t_r=2.0))
    assert same_bits(ArrayMasker(mask, (2, 2, 2), 6).fit().transform(vol), rows)
    img = m.inverse_transform(got)
    assert img.shape == shape + (T,) and np.all(img[~mask] == 0) and same_bits(img[mask].T, got)
    assert same_bits(img, unmask(got, mask))
    # a 2-D input is taken as masked already: cleaned only; with smoothing_fwhm that is an error
    plain = ArrayMasker(mask, standardize=True).fit()
    pre = np.ascontiguousarray(np.where(np.isfinite(vol), vol, 0)[mask].T)
    assert same_bits(plain.transform(pre), plain.transform(vol))
    assert ArrayMasker(mask).fit().transform(pre) is pre
    with pytest.raises(ValueError, match='already masked'):
        m.transform(pre)
    with pytest.raises(ValueError):
        plain.transform(pre[:, :-1])


def test_value_errors_name_the_offender():
    from modl_amd.masker import smooth_mask, smooth_mask_host, unmask, ArrayMasker, SMOOTH_MAX_RADIUS
    assert SMOOTH_MAX_RADIUS >= 8
    vol = np.ones((4, 3, 2, 2))
    mask = np.ones((4, 3, 2), dtype=bool)
    for f in (smooth_mask, smooth_mask_host):
        with pytest.raises(ValueError, match='boolean'):
            f(vol, mask.astype(np.uint8))
        with pytest.raises(ValueError, match='boolean'):
            f(vol, mask[0])
        with pytest.raises(ValueError, match=r'\(4, 3, 2\).*\(4, 3, 3\)'):
            f(vol, np.ones((4, 3, 3), dtype=bool))
        with pytest.raises(ValueError, match='empty'):
            f(vol, np.zeros((4, 3, 2), dtype=bool))
        with pytest.raises(ValueError, match='voxel_size.*-2'):
            f(vol, mask, 6, (2, -2, 2))
        with pytest.raises(ValueError, match='voxel_size'):
            f(vol, mask, 6, (2, 0, 2))
        with pytest.raises(ValueError, match='smoothing_fwhm.*-6'):
            f(vol, mask, -6)
        with pytest.raises(ValueError, match='smoothing_fwhm'):
            f(vol, mask, (6, np.nan, 6))
        with pytest.raises(ValueError, match='smoothing_fwhm'):
            f(vol, mask, (6, 6))
        with pytest.raises(ValueError, match='permutation'):
            f(vol, mask, dst_row=[0, 0])
        with pytest.raises(ValueError):
            f(vol[0], mask)
    with pytest.raises(ValueError, match='radius of 9 .*at most %d' % SMOOTH_MAX_RADIUS):
        smooth_mask(vol, mask, 10.6, (2, 2, 2))                                   # sigma 2.25: r = 9
    with pytest.raises(ValueError, match='at most %d' % SMOOTH_MAX_RADIUS):
        ArrayMasker(mask, smoothing_fwhm=(0, 0, 30)).fit()
    with pytest.raises(ValueError, match=r'\(n, 24\)'):
        unmask(np.ones((2, 23)), mask)
    with pytest.raises(ValueError, match='boolean'):
        unmask(np.ones((2, 24)), mask.astype(float))


# ---- the refusals of the entry points: the good call, and one argument wrong at a time
def _weights_for(radii):
    from modl_amd.masker import gaussian_weights
    out = []
    for r in radii:
        w = gaussian_weights((r + 0.2) / 4.0)[0] if r else np.ones(1)
        assert w.shape[0] == 2 * r + 1
        out.append(np.ascontiguousarray(w))
    return out


def _bad_smooth_calls(box, V, ld):
    return [('null vol', dict(vol=None), EINVAL), ('null col', dict(col=None), EINVAL), ('null out', dict(out=None), EINVAL),
            ('T = 0', dict(T=0), EINVAL), ('n0 = 0', dict(n0=0), EINVAL), ('n1 < 0', dict(n1=-1), EINVAL),
            ('n2 = 0', dict(n2=0), EINVAL), ('V = 0', dict(V=0), EINVAL), ('ldo < V', dict(ldo=V - 1), EINVAL),
            ('frame stride < box', dict(fs=box - 1), EINVAL), ('radius 9', dict(r0=9), EINVAL), ('radius -1', dict(r2=-1), EINVAL),
            ('nan weight', dict(w1=('set', 1, np.nan)), EINVAL), ('inf weight', dict(w0=('set', 0, np.inf)), EINVAL),
            ('negative weight', dict(w2=('set', 0, -1e-3)), EINVAL), ('sum not 1', dict(w1=('add', 2, 1e-9)), EINVAL),
            ('out inside vol', dict(out='vol'), EINVAL), ('out overlaps the last frame', dict(out='vol+last'), EINVAL),
            ('null ws', dict(ws=None), ENOMEM), ('small ws', dict(ws_bytes='short'), ENOMEM),
            ('bad pointer and no workspace', dict(vol=None, ws=None), EINVAL)]


def _call_smooth(lib, dt, ptrs, T, box3, radii, V, ld, over):
    n0, n1, n2 = box3
    w = _weights_for(radii)
    a = dict(vol=ptrs['vol'], fs=n0 * n1 * n2, T=T, n0=n0, n1=n1, n2=n2, w0=w[0], r0=radii[0], w1=w[1], r1=radii[1], w2=w[2],
             r2=radii[2], col=ptrs['col'], V=V, dst=ptrs['dst'], out=ptrs['out'], ldo=ld, ws=ptrs['ws'])
    a['ws_bytes'] = lib.modl_smooth_mask_workspace(0 if dt == 'f32' else 1, T, n0, n1, n2, *radii)
    for k, v in over.items():
        if isinstance(v, tuple) and v[0] == 'set':
            a[k][v[1]] = v[2]
        elif isinstance(v, tuple) and v[0] == 'add':
            a[k][v[1]] += v[2]
        else:
            a[k] = v
    es = 4 if dt == 'f32' else 8
    if a['out'] == 'vol':
        a['out'] = a['vol']
    elif a['out'] == 'vol+last':
        a['out'] = a['vol'] + (T * n0 * n1 * n2 - 1) * es
    if a['ws_bytes'] == 'short':
        a['ws_bytes'] = lib.modl_smooth_mask_workspace(0 if dt == 'f32' else 1, T, n0, n1, n2, *radii) - 1
    vp = lambda v: C.c_void_p(v) if v else C.c_void_p(0)
    hp = lambda v: None if v is None else v.ctypes.data
    return getattr(lib, 'modl_smooth_mask_' + dt)(vp(a['vol']), a['fs'], a['T'], a['n0'], a['n1'], a['n2'], hp(a['w0']), a['r0'],
                                                  hp(a['w1']), a['r1'], hp(a['w2']), a['r2'], vp(a['col']), a['V'],
                                                  vp(a['dst']), vp(a['out']), a['ldo'], vp(a['ws']), a['ws_bytes'], None)


def _bad_unmask_calls(V):
    return [('null rows', dict(rows=None)), ('null vox', dict(vox=None)), ('null out', dict(out=None)), ('n = 0', dict(n=0)),
            ('V = 0', dict(V=0)), ('n1 = 0', dict(n1=0)), ('ldr < V', dict(ldr=V - 1)), ('V > box', dict(V=10 ** 6, ldr=10 ** 6)),
            ('out is rows', dict(out='rows'))]


def _call_unmask(lib, dt, ptrs, n, V, box3, over):
    a = dict(rows=ptrs['rows'], ldr=V, n=n, V=V, vox=ptrs['vox'], n0=box3[0], n1=box3[1], n2=box3[2], out=ptrs['uout'])
    a.update(over)
    if a['out'] == 'rows':
        a['out'] = a['rows']
    vp = lambda v: C.c_void_p(v) if v else C.c_void_p(0)
    return getattr(lib, 'modl_unmask_' + dt)(vp(a['rows']), a['ldr'], a['n'], a['V'], vp(a['vox']), a['n0'], a['n1'], a['n2'],
                                             vp(a['out']), None)


def _workspace_refusals(lib):
    good = lib.modl_smooth_mask_workspace(0, 3, 5, 4, 3, 2, 0, 8)
    assert good >= 3 * 17 * 8 and good == lib.modl_smooth_mask_workspace(1, 3, 5, 4, 3, 2, 0, 8)
    for args in ((7, 3, 5, 4, 3, 2, 0, 8), (0, 0, 5, 4, 3, 2, 0, 8), (0, 3, 0, 4, 3, 2, 0, 8), (0, 3, 5, -1, 3, 2, 0, 8),
                 (0, 3, 5, 4, 0, 2, 0, 8), (0, 3, 5, 4, 3, 9, 0, 8), (0, 3, 5, 4, 3, 2, -1, 8), (0, 3, 5, 4, 3, 2, 0, 9),
                 (0, 3, 1 << 20, 1 << 20, 4, 1, 1, 1)):
        assert lib.modl_smooth_mask_workspace(*args) == 0, args
    tile = (C.c_int * 3)()
    assert lib.modl_smooth_tile(0, 3, 3, 3, tile) == 0 and all(t >= 1 for t in tile)
    assert lib.modl_smooth_tile(0, 9, 3, 3, tile) == EINVAL and lib.modl_smooth_tile(2, 3, 3, 3, tile) == EINVAL
    assert lib.modl_smooth_tile(0, 3, 3, 3, None) == EINVAL
    assert lib.modl_smooth_max_radius() >= 8


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_entry_points_refuse_bad_arguments_without_a_device(dt):
    from modl_amd._lib import lib
    _workspace_refusals(lib)
    T, box3, radii = 2, (5, 4, 3), (2, 1, 3)
    box = 60
    V, ld = 20, 23
    bufs = dict(vol=np.zeros((T, box), DT[dt]), col=np.zeros(box, np.int32), dst=np.arange(T, dtype=np.int64),
                out=np.zeros((T, ld), DT[dt]), ws=np.zeros(512), rows=np.zeros((T, V), DT[dt]),
                vox=np.arange(V, dtype=np.int64), uout=np.zeros((T, box), DT[dt]))
    ptrs = {k: v.ctypes.data for k, v in bufs.items()}
    for name, over, code in _bad_smooth_calls(box, V, ld):
        assert _call_smooth(lib, dt, ptrs, T, box3, radii, V, ld, over) == code, name
    for name, over in _bad_unmask_calls(V):
        assert _call_unmask(lib, dt, ptrs, T, V, box3, over) == EINVAL, name
    if lib.modl_device_count() == 0:
        assert _call_smooth(lib, dt, ptrs, T, box3, radii, V, ld, {}) == ENOGPU
        assert _call_smooth(lib, dt, ptrs, T, box3, radii, V, ld, dict(ws=None)) == ENOMEM      # ENOMEM before ENOGPU
        assert _call_unmask(lib, dt, ptrs, T, V, box3, {}) == ENOGPU


# ---- the estimators
def _fmri_volumes(dtype):
    shape = (6, 5, 4)
    mask = random_mask(shape, seed=5, p=0.6)
    vols = [volume(shape, 30, dtype, seed=1), np.asfortranarray(volume(shape, 25, dtype, seed=2))]
    kw = dict(n_components=4, n_epochs=2, random_state=0, batch_size=10, alpha=0.1, reduction=2)
    return vols, mask, kw


def _check_masked_estimators(fMRIDictFact, fMRICoder, dtype, tmp_path):
    """the wiring: mask / smoothing_fwhm inside the estimators equal handing over records that an ArrayMasker has smoothed
    and masked, bit for bit - fit, components_img_, dict_init as a volume, transform, score, coder, scorer"""
    from modl_amd.fmri import rfMRIDictionaryScorer
    from modl_amd.masker import ArrayMasker, unmask
    vols, mask, kw = _fmri_volumes(dtype)
    mk = dict(mask=mask, smoothing_fwhm=6, voxel_size=(2, 2, 2))
    masker = ArrayMasker(mask, voxel_size=(2, 2, 2), smoothing_fwhm=6).fit()
    pre = [masker.transform(v) for v in vols]
    on = fMRIDictFact(**mk, **kw).fit(vols)
    off = fMRIDictFact(**kw).fit(pre)
    assert same_bits(on.components_, off.components_)
    assert on.components_img_.shape == mask.shape + (4,) and isinstance(on.components_img_, np.ndarray)
    assert same_bits(on.components_img_, unmask(on.components_, mask))
    assert np.all(on.components_img_[~mask] == 0) and same_bits(on.components_img_[mask].T, on.components_)
    assert not hasattr(off, 'components_img_')
    assert not same_bits(on.components_, fMRIDictFact(mask=mask, **kw).fit(vols).components_)      # the smoothing acts
    # a .npy path of a 4-D volume, a 2-D record next to it, and cleaning on top (the permutation folded into the cleaning)
    path = str(tmp_path / 'vol.npy')
    np.save(path, vols[1])
    cl = dict(standardize=True, detrend=True)
    mixed = fMRIDictFact(**mk, **cl, **kw).fit([vols[0], path])
    assert same_bits(mixed.components_, fMRIDictFact(**cl, **kw).fit(pre).components_)
    assert same_bits(mixed.components_, fMRIDictFact(**mk, **cl, **kw).fit([pre[0], vols[1]]).components_)
    # dict_init as a volume: masked, not smoothed
    init = np.random.RandomState(4).randn(*mask.shape, 4).astype(dtype)
    a = fMRIDictFact(dict_init=init, **mk, **kw).fit(vols)
    b = fMRIDictFact(dict_init=np.ascontiguousarray(init[mask].T), **kw).fit(pre)
    assert same_bits(a.components_, b.components_)
    # transform and score
    for x, y in zip(on.transform(vols), off.transform(pre)):
        assert same_bits(np.asarray(x), np.asarray(y))
    assert on.score(vols) == off.score(pre)
    # the coder
    c_on = fMRICoder(on.components_, alpha=0.1, **mk).fit()
    c_off = fMRICoder(on.components_, alpha=0.1).fit()
    for x, y in zip(c_on.transform(vols), c_off.transform(pre)):
        assert same_bits(np.asarray(x), np.asarray(y))
    assert same_bits(np.asarray(c_on.transform(vols[0])[0]), np.asarray(c_off.transform(pre[0])[0]))     # one record
    assert c_on.score(vols) == c_off.score(pre)
    assert same_bits(c_on.components_img_, on.components_img_)
    assert same_bits(fMRICoder(on.components_img_, alpha=0.1, mask=mask).fit().components_, on.components_)
    # the scorer: the masking arguments come from its first argument
    s_on, s_off = rfMRIDictionaryScorer(vols), rfMRIDictionaryScorer(pre)
    s_on(on, on.dict_fact_, 0.0, 0.0)
    s_off(off, off.dict_fact_, 0.0, 0.0)
    assert s_on.score == s_off.score
    with pytest.raises(ValueError, match='mask'):
        fMRIDictFact(smoothing_fwhm=6, **kw).fit(pre)
    with pytest.raises(ValueError, match='mask'):
        fMRIDictFact(**kw).fit(vols)
    with pytest.raises(ValueError, match='mask'):
        fMRICoder(on.components_, smoothing_fwhm=6).fit()


def _check_legacy(fMRIDictFact, dtype):
    """the three new arguments left at None: the fit of before, bits and draws"""
    from .test_filter import _fmri_case
    recs, confs, kw = _fmri_case(dtype)
    rs_a, rs_b = np.random.RandomState(3), np.random.RandomState(3)
    a = fMRIDictFact(**dict(kw, random_state=rs_a)).fit(recs)
    b = fMRIDictFact(**dict(kw, random_state=rs_b), mask=None, smoothing_fwhm=None, voxel_size=None).fit(recs)
    assert same_bits(a.components_, b.components_)
    assert rs_a.randint(1 << 30) == rs_b.randint(1 << 30)                      # the same number of draws
    assert not hasattr(b, 'components_img_')
    params = fMRIDictFact().get_params()
    assert params['mask'] is None and params['smoothing_fwhm'] is None and params['voxel_size'] is None


def _host_estimators():
    from modl_amd.fmri import fMRICoder
    from .test_wrappers import _fmri_estimator, _host_classes

    class HostfMRICoder(fMRICoder):
        _coder_class = _host_classes()[1]
    return _fmri_estimator(True), HostfMRICoder


def test_estimators_mask_records_host_logic(tmp_path):
    est, coder = _host_estimators()
    _check_masked_estimators(est, coder, np.float64, tmp_path)


def test_legacy_path_unchanged_host_logic():
    _check_legacy(_host_estimators()[0], np.float64)


# ------------------------------------------------------------------------------------------------ layer 2: the GPU
@pytest.fixture(scope='module')
def gpu():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    return torch


GUARD = 64                                               # elements of SENT before and after the output


def column_map(mask):
    col = np.full(mask.shape, -1, dtype=np.int32)
    col[mask] = np.arange(mask.sum(), dtype=np.int32)
    return col


def gpu_smooth_mask(frames, weights, col, V, dst=None, pad=3):
    """modl_smooth_mask_* on frames (T, n0, n1, n2) with d_out[T][V + pad] inside guard elements and the workspace inside
    guard bytes: the (T, V) result; asserts that padding, guards and the input are untouched"""
    import torch
    from modl_amd._lib import lib, check
    from modl_amd.device import ptr
    T, n0, n1, n2 = frames.shape
    sx = 'f32' if frames.dtype == np.float32 else 'f64'
    es = frames.dtype.itemsize
    radii = [(len(w) - 1) // 2 if w is not None else 0 for w in weights]
    d_vol = torch.from_numpy(np.array(frames, order='C')).to('cuda')
    d_col = torch.from_numpy(np.ascontiguousarray(col)).to('cuda')
    ld = V + pad
    d_buf = torch.full((2 * GUARD + T * ld,), SENT, dtype=d_vol.dtype, device='cuda')
    d_dst = None if dst is None else torch.from_numpy(np.ascontiguousarray(dst, dtype=np.int64)).to('cuda')
    need = lib.modl_smooth_mask_workspace(0 if sx == 'f32' else 1, T, n0, n1, n2, *radii)
    assert need > 0
    d_ws = torch.full((need + 512,), 0xA5, dtype=torch.uint8, device='cuda')
    hp = lambda w, r: w.ctypes.data if r else None
    check(getattr(lib, 'modl_smooth_mask_' + sx)(
        ptr(d_vol), n0 * n1 * n2, T, n0, n1, n2, hp(weights[0], radii[0]), radii[0], hp(weights[1], radii[1]), radii[1],
        hp(weights[2], radii[2]), radii[2], ptr(d_col), V, ptr(d_dst), C.c_void_p(d_buf.data_ptr() + GUARD * es), ld,
        C.c_void_p(d_ws.data_ptr() + 256), need, None), 'modl_smooth_mask')
    torch.cuda.synchronize()
    buf = d_buf.cpu().numpy()
    out = buf[GUARD:GUARD + T * ld].reshape(T, ld)
    assert np.all(buf[:GUARD] == SENT) and np.all(buf[GUARD + T * ld:] == SENT) and np.all(out[:, V:] == SENT)
    ws = d_ws.cpu().numpy()
    assert np.all(ws[:256] == 0xA5) and np.all(ws[256 + need:] == 0xA5)
    assert np.array_equal(d_vol.cpu().numpy(), frames, equal_nan=True)
    return np.ascontiguousarray(out[:, :V])


def kernel_weights(fwhm, voxel):
    from modl_amd.masker import gaussian_weights
    return [np.ascontiguousarray(gaussian_weights(s)[0]) if s > 0 else None for s in sigmas_of(fwhm, voxel)]


def kernel_tile(dt, radii):
    from modl_amd._lib import lib
    tile = (C.c_int * 3)()
    assert lib.modl_smooth_tile(0 if dt == 'f32' else 1, *radii, tile) == 0
    return tuple(tile)


# (box, fwhm per axis, voxel size): radii 0 / 1 / 3 / 5 / 8 mixed per axis, an axis shorter than its radius, one untouched
GPU_CASES = {'7x5x3 r555': ((7, 5, 3), (6.0, 6.0, 6.0), (2.0, 2.0, 2.0)),
             '17x9x2 r830': ((17, 9, 2), (9.5, 4.0, None), (2.0, 2.0, 2.0)),
             '1x6x33 r158': ((1, 6, 33), (1.2, 6.0, 9.5), (2.0, 2.0, 2.0)),
             '20x19x18 r351': ((20, 19, 18), (4.0, 6.0, 1.2), (2.0, 2.0, 2.0)),
             '20x19x18 r003': ((20, 19, 18), (None, 0.0, 6.0), (2.0, 2.0, 3.0)),
             'tile + 1 r333': (None, (4.0, 4.0, 4.0), (2.0, 2.0, 2.0)),
             'tile + 1 r888': (None, (9.5, 9.5, 9.5), (2.0, 2.0, 2.0)),
             '7x5x3 r000': ((7, 5, 3), None, (2.0, 2.0, 2.0))}
GPU_RADII = {'7x5x3 r555': (5, 5, 5), '17x9x2 r830': (8, 3, 0), '1x6x33 r158': (1, 5, 8), '20x19x18 r351': (3, 5, 1),
             '20x19x18 r003': (0, 0, 3), 'tile + 1 r333': (3, 3, 3), 'tile + 1 r888': (8, 8, 8), '7x5x3 r000': (0, 0, 0)}


@functools.lru_cache(maxsize=None)
def gpu_case(name, dt, T=3):
    """(frames (T, n0, n1, n2), smoothed reference (n0, n1, n2, T) f64, M, weights, radii, box, tile)"""
    box, fwhm, voxel = GPU_CASES[name]
    fw = [fwhm] * 3 if not np.ndim(fwhm) else fwhm
    radii = tuple(radii_of(fw, voxel))
    assert radii == GPU_RADII[name]
    tile = kernel_tile(dt, radii)
    if box is None:
        box = tuple(t + 1 for t in tile)
    vol = volume(box, T, DT[dt], seed=11)
    ref = restate(vol, fw, voxel)
    frames = np.ascontiguousarray(vol.transpose(3, 0, 1, 2))
    for a in (frames, ref):
        a.setflags(write=False)
    return frames, ref, frame_max(vol), kernel_weights(fw, voxel), radii, box, tile


def masks_of(box, tile, name):
    """(label, mask): all true, one voxel at each corner, a checkerboard, two blobs around an empty tile, V = 1 / 63 / 65"""
    out = [('all', np.ones(box, dtype=bool))]
    for cx in (0, box[0] - 1):
        for cy in (0, box[1] - 1):
            for cz in (0, box[2] - 1):
                m = np.zeros(box, dtype=bool)
                m[cx, cy, cz] = True
                out.append(('corner %d %d %d' % (cx, cy, cz), m))
    i, j, k = np.indices(box)
    out.append(('checkerboard', (i + j + k) % 2 == 0))
    if box[0] > 2 * tile[0]:                                                    # room for a whole tile between two blobs
        m = np.zeros(box, dtype=bool)
        m[:2] = True
        m[2 * tile[0]:, ::2] = True
        assert not m[tile[0]:2 * tile[0]].any()
        out.append(('two blobs', m))
    order = np.random.RandomState(2).permutation(int(np.prod(box)))
    for V in (63, 65):
        if V <= order.shape[0]:
            m = np.zeros(box, dtype=bool)
            m.reshape(-1)[order[:V]] = True
            out.append(('V = %d' % V, m))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(GPU_CASES))
@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_smooth_mask_through_the_abi(gpu, dt, name):
    frames, ref, M, weights, radii, box, tile = gpu_case(name, dt)
    eps_out = float(np.finfo(DT[dt]).eps)
    T = frames.shape[0]
    clean_vol = np.where(np.isfinite(frames), frames, 0).transpose(1, 2, 3, 0)
    labels = []
    for label, mask in masks_of(box, tile, name):
        labels.append(label)
        V = int(mask.sum())
        got = gpu_smooth_mask(frames, weights, column_map(mask), V)
        if not any(radii):
            assert same_bits(got, clean_vol[mask].T), label
            continue
        ok, worst = judge(got, ref[mask].T, M, eps_out, radii)
        print(name, dt, label, 'V = %d: %.3f of the bound' % (V, worst))
        assert ok, (label, worst)
    if name == '20x19x18 r351':
        assert 'two blobs' in labels
    # T = 1, and the rows reversed through d_dst_row
    mask = masks_of(box, tile, name)[9][1]
    V = int(mask.sum())
    full = gpu_smooth_mask(frames, weights, column_map(mask), V)
    rev = gpu_smooth_mask(frames, weights, column_map(mask), V, dst=np.arange(T)[::-1], pad=0)
    assert same_bits(rev[::-1], full)
    one = gpu_smooth_mask(frames[1:2], weights, column_map(mask), V)
    assert same_bits(one, full[1:2])
    skipped = gpu_smooth_mask(frames, weights, column_map(mask), V, dst=np.array([1, T + 5, -1]))
    assert same_bits(skipped[1], full[0]) and np.all(skipped[[0, 2]] == SENT)  # an entry outside 0 .. T-1 is skipped


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_bits_depend_on_volume_and_weights_alone(gpu, dt):
    for name in ('20x19x18 r351', 'tile + 1 r333', '1x6x33 r158'):
        frames, ref, M, weights, radii, box, tile = gpu_case(name, dt)
        rs = np.random.RandomState(8)
        m1, m2 = rs.rand(*box) < 0.5, rs.rand(*box) < 0.3
        m2[0, 0, 0] = m1[0, 0, 0] = True
        full = gpu_smooth_mask(frames, weights, column_map(np.ones(box, dtype=bool)), int(np.prod(box)))
        vol = full.T.reshape(box + (frames.shape[0],))
        a = gpu_smooth_mask(frames, weights, column_map(m1), int(m1.sum()))
        b = gpu_smooth_mask(frames, weights, column_map(m2), int(m2.sum()))
        assert same_bits(a, vol[m1].T) and same_bits(b, vol[m2].T)                # the same voxel under three masks
        assert same_bits(a, gpu_smooth_mask(frames, weights, column_map(m1), int(m1.sum())))        # run to run
        assert same_bits(gpu_smooth_mask(frames[1:2], weights, column_map(m1), int(m1.sum())), a[1:2])
    # untouched axes are untouched: with radii (0, 0, r) a line along the last axis sees nothing of the other two
    frames, ref, M, weights, radii, box, tile = gpu_case('20x19x18 r003', dt)
    col = column_map(np.ones(box, dtype=bool))
    got = gpu_smooth_mask(frames, weights, col, int(np.prod(box))).T.reshape(box + (frames.shape[0],))
    moved = gpu_smooth_mask(np.ascontiguousarray(frames[:, ::-1, ::-1]), weights, col, int(np.prod(box)))
    assert same_bits(moved.T.reshape(box + (frames.shape[0],))[::-1, ::-1], got)  # rows along z do not see x and y


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_unmask_through_the_abi(gpu, dt):
    import torch
    from modl_amd._lib import lib, check
    from modl_amd.device import ptr
    for box in ((7, 5, 3), (1, 6, 33), (20, 19, 18)):
        for label, mask in masks_of(box, (8, 8, 8), ''):
            V, n, pad = int(mask.sum()), 3, 2
            rows = np.random.RandomState(V).randn(n, V + pad).astype(DT[dt])
            rows[0, 0] = np.nan
            d_rows = torch.from_numpy(rows).to('cuda')
            d_vox = torch.from_numpy(np.flatnonzero(mask.ravel()).astype(np.int64)).to('cuda')
            nb = int(np.prod(box))
            d_buf = torch.full((2 * GUARD + n * nb,), SENT, dtype=d_rows.dtype, device='cuda')
            check(getattr(lib, 'modl_unmask_' + dt)(ptr(d_rows), V + pad, n, V, ptr(d_vox), *box,
                                                    C.c_void_p(d_buf.data_ptr() + GUARD * rows.itemsize), None), 'modl_unmask')
            torch.cuda.synchronize()
            buf = d_buf.cpu().numpy()
            assert np.all(buf[:GUARD] == SENT) and np.all(buf[GUARD + n * nb:] == SENT)
            got = buf[GUARD:GUARD + n * nb].reshape((n,) + box)
            want = np.zeros((n,) + box, dtype=DT[dt])
            want[:, mask] = rows[:, :V]
            assert same_bits(got, want), (box, label)


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_entry_points_refuse_bad_arguments(gpu, dt):
    import torch
    from modl_amd._lib import lib
    _workspace_refusals(lib)
    T, box3, radii = 2, (5, 4, 3), (2, 1, 3)
    box, V, ld = 60, 20, 23
    td = torch.float32 if dt == 'f32' else torch.float64
    bufs = dict(vol=torch.ones((T, box), dtype=td, device='cuda'), col=torch.arange(box, dtype=torch.int32, device='cuda') % V,
                dst=torch.arange(T, dtype=torch.int64, device='cuda'), out=torch.full((T, ld), SENT, dtype=td, device='cuda'),
                ws=torch.zeros(512, dtype=torch.uint8, device='cuda'), rows=torch.ones((T, V), dtype=td, device='cuda'),
                vox=torch.arange(V, dtype=torch.int64, device='cuda'), uout=torch.full((T, box), SENT, dtype=td, device='cuda'))
    ptrs = {k: v.data_ptr() for k, v in bufs.items()}
    for name, over, code in _bad_smooth_calls(box, V, ld):
        assert _call_smooth(lib, dt, ptrs, T, box3, radii, V, ld, over) == code, name
    for name, over in _bad_unmask_calls(V):
        assert _call_unmask(lib, dt, ptrs, T, V, box3, over) == EINVAL, name
    torch.cuda.synchronize()
    assert bool((bufs['out'] == SENT).all()) and bool((bufs['uout'] == SENT).all()) and bool((bufs['vol'] == 1).all())
    assert _call_smooth(lib, dt, ptrs, T, box3, radii, V, ld, {}) == 0             # and the good call is one
    assert _call_unmask(lib, dt, ptrs, T, V, box3, {}) == 0
    torch.cuda.synchronize()
    assert bool((bufs['out'][:, :V] == 1).all()) and bool((bufs['out'][:, V:] == SENT).all())


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_python_functions_on_the_device(gpu, dt):
    import torch
    from modl_amd.masker import smooth_mask, unmask, ArrayMasker, unmask_host
    from modl_amd.signal import clean
    shape, T = (11, 9, 10), 40
    vol = volume(shape, T, DT[dt], seed=4)
    mask = random_mask(shape, seed=6, p=0.3)
    fwhm, voxel = (6.0, 4.0, 5.0), (2.0, 2.0, 3.0)
    radii = radii_of(fwhm, voxel)
    ref = restate(vol, fwhm, voxel)[mask].T
    got = smooth_mask(vol, mask, fwhm, voxel)
    assert isinstance(got, np.ndarray) and got.dtype == DT[dt] and got.shape == ref.shape
    assert judge(got, ref, frame_max(vol), float(np.finfo(DT[dt]).eps), radii)[0]
    d_c = torch.from_numpy(vol).to('cuda')                                         # C order: permuted on the device
    d_f = torch.from_numpy(np.ascontiguousarray(vol.T)).to('cuda').permute(3, 2, 1, 0)          # Fortran order: as it is
    assert d_f.shape == d_c.shape and not d_f.is_contiguous()
    g_c, g_f = smooth_mask(d_c, mask, fwhm, voxel), smooth_mask(d_f, mask, fwhm, voxel)
    assert g_c.is_cuda and g_f.is_cuda and g_c.dtype == d_c.dtype
    assert same_bits(g_c.cpu().numpy(), got) and same_bits(g_f.cpu().numpy(), got)
    assert same_bits(smooth_mask(np.asfortranarray(vol), mask, fwhm, voxel), got)
    assert same_bits(smooth_mask(vol[..., 2], mask, fwhm, voxel), got[2:3])        # a 3-D array: one frame
    perm = np.random.RandomState(0).permutation(T)
    assert same_bits(smooth_mask(d_c, mask, fwhm, voxel, dst_row=perm).cpu().numpy()[perm], got)
    assert same_bits(smooth_mask(vol, mask), np.where(np.isfinite(vol), vol, 0)[mask].T)
    # unmask
    img = unmask(got, mask)
    assert isinstance(img, np.ndarray) and same_bits(img, unmask_host(got, mask))
    d_img = unmask(g_c, mask)
    assert d_img.is_cuda and tuple(d_img.shape) == shape + (T,) and same_bits(d_img.cpu().numpy(), img)
    # the masker: smoothing and masking, then the cleaning that exists
    m = ArrayMasker(mask, voxel, fwhm, standardize=True, detrend=True, high_pass=0.01, t_r=2.0).fit()
    want = clean(smooth_mask(d_c, mask, fwhm, voxel), True, True, None, high_pass=0.01, t_r=2.0)
    assert same_bits(m.transform(d_c).cpu().numpy(), want.cpu().numpy())
    assert same_bits(m.transform(vol), want.cpu().numpy())
    assert same_bits(m.inverse_transform(want).cpu().numpy(), unmask_host(want.cpu().numpy(), mask))


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_estimators_mask_records_on_the_device(gpu, dt, tmp_path):
    from modl_amd.fmri import fMRIDictFact, fMRICoder
    _check_masked_estimators(fMRIDictFact, fMRICoder, DT[dt], tmp_path)
    _check_legacy(fMRIDictFact, DT[dt])
