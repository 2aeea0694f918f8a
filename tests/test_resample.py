"""Resampling of fMRI volumes onto the mask's grid (modl_amd/masker.py, csrc/resample.hip).

nilearn is not installed, so nothing is pinned to a run of it: its resample_img is scipy.ndimage.affine_transform per frame
(mode 'constant', order 3 / 1 / 0), and that is the yardstick.

THE JUDGE.  `ref` is scipy itself on the f64 copy of the input with the non-finite elements zeroed: affine_transform for a
resampled frame, spline_filter(order=3, mode='mirror') for the coefficients.  With M the largest |finite element| of the
frame and eps the machine epsilon of the volume's dtype (the coefficients are stored in that dtype) an element passes if

    order 3:                                |got - ref| <= (40.5 eps + 13.5 eps + 3600 eps64) M
    the coefficients alone:                 |got - ref| <= (40.5 eps + 1728 eps64) M
    order 1:                                |got - ref| <= (eps / 2 + 64 eps64) M
    order 0, identity + integer shift:      the same bits

Where this comes from.  The 1-D prefilter has l-infinity gain 3, so the exact coefficients are bounded by 27 M.  The device
rounds to the storage dtype once per axis: after the first axis the values are bounded by 3 M and the error eps / 2 * 3 M
is amplified by the two remaining axes (9), after the second it is eps / 2 * 9 M amplified by 3, after the third
eps / 2 * 27 M - 13.5 eps M each, 40.5 eps M together.  The B-spline and the linear weights are non-negative and sum to 1,
so the gather is a contraction of the coefficients: nothing is amplified, its result is bounded by 27 M and its one
rounding to the output dtype adds at most 13.5 eps M (eps / 2 M at order 1, where the taps are the elements themselves).
Everything else is f64 arithmetic, on the device (the kernels carry the recursions and ACCUMULATE THE TAPS IN F64 for
both dtypes) and in scipy alike: a recursion step rounds twice and forgets with |z| = 0.268, at most 32 eps64 of an
axis' input bound per axis, amplified like the storage roundings: 3 * 288 = 864 eps64 M per implementation; the sum of 64
products of weights that carry a few eps64 each, at most 905 eps64 M per implementation; 2 * (864 + 905) < 3600.  The
causal start value is the mirror sum cut after 64 terms: |z|^64 = 2.6e-37, nothing.  Coordinates need no term: the
kernel forms them with scipy's operations in scipy's order.  f32: 6.4e-6 M, f64: 8.1e-13 M.
Measured on the cases below: f32 storage emulated in numpy at most 1.1 eps32 M; on an MI355X at most 1.3 eps M (f32) and
8.6 eps M (f64) at order 3, 5.4 eps M and 56 eps M for the coefficients alone, 4.2 eps M at order 1.

The inputs leave the judge nothing to skip.  Every case asserts that a quarter of its loci or more fall inside the source
box; the oblique cases assert that no coordinate lies within 1e-9 of 0 or n - 1 and, for order 0, that no x + 0.5 lies within
1e-9 of an integer, so no locus is excluded from the comparison; the exact cases (dyadic A, b in multiples of 0.25) put
loci exactly on 0 and on n - 1, which are inside, as in scipy.

The mutants of MUTANTS are rejected at 100 times the bound or more (test_judge_rejects_mutants asserts the ratio).

Layer 1 (no GPU): the restatement against scipy, the mutants, resample_host, voxel_size_of, every ValueError, the refusals of
the entry points, ArrayMasker and the estimators on the oracle backend.  Layer 2 (gpu): the prefilter, box mode and rows
mode through the C-ABI, determinism, the refusals with output and workspace untouched, the Python functions and the
estimators on the device.

The module imports modl_amd.masker.resample at the top, so none of its tests can pass without the feature."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.ndimage

from modl_amd.masker import resample  # noqa: F401  (see the module docstring)

from .test_clean import SENT, DT, EINVAL, ENOMEM, ENOGPU, same_bits
from .test_masker import random_mask, GUARD, scipy_chain, _host_estimators

EPS64 = float(np.finfo(np.float64).eps)
POLE = np.sqrt(3.0) - 2.0
ORDERS = {'continuous': 3, 'linear': 1, 'nearest': 0}
MUTANTS = ('reflect', 'floor0', 'transposed', 'axes_not_reversed', 'b_not_permuted', 'no_anticausal_init', 'no_gain',
           'bound_n', 'keep_nonfinite', 'prefilter_order1')


def bound(order, eps):
    """the judge's bound in units of M (module docstring)"""
    if order == 3:
        return 54.0 * eps + 3600 * EPS64
    if order == 'coefficients':                           # the three storage roundings and the f64 recursions of both sides
        return 40.5 * eps + 1728 * EPS64
    if order == 1:
        return 0.5 * eps + 64 * EPS64
    return 0.0


def _rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return rx @ ry @ rz


# name: (source shape (X, Y, Z), target shape, A, b, kind) in the USER's axis order; the kernel sees both boxes reversed
CASES = {
    'oblique': ((5, 6, 7), (9, 5, 6), 0.8 * _rot(0.11, -0.07, 0.13) + np.array([[0, 0.05, 0], [0, 0, 0], [0.03, 0, 0]]),
                np.array([0.37, 0.61, 0.83]), 'oblique'),
    '2mm to 3mm': ((13, 15, 13), (9, 10, 9), 1.5 * np.eye(3), np.zeros(3), 'exact'),
    'magnify': ((3, 4, 5), (7, 9, 11), np.diag([0.29, 0.31, 0.37]) + 0.01 * (np.ones((3, 3)) - np.eye(3)),
                np.array([0.043, 0.057, 0.071]), 'oblique'),
    'half': ((5, 6, 7), (9, 13, 14), 0.5 * np.eye(3), np.array([0.0, -0.5, 0.25]), 'exact'),
    'double': ((13, 15, 13), (7, 8, 6), 2.0 * np.eye(3), np.array([0.0, 0.25, 2.0]), 'exact'),
    'flat': ((1, 6, 9), (3, 5, 8), np.array([[0, 0, 0], [0.1031, 0.9017, 0.1313], [0.0707, -0.0503, 1.0719]]),
             np.array([0.0, 0.3137, 0.4391]),
             'oblique'),
    'shift': ((5, 6, 7), (6, 5, 9), np.eye(3), np.array([1.0, -2.0, 0.0]), 'shift'),
    'outside': ((5, 6, 7), (4, 3, 5), 0.5 * np.eye(3), np.array([100.0, 0.0, 0.0]), 'outside'),
}
PREFILTER_BOXES = [(7, 6, 5), (1, 6, 33), (2, 3, 70), (3, 2, 300)]          # the kernel's (n0, n1, n2)


def make_volume(shape, T, dtype, seed, offset=0.0):
    """(X, Y, Z, T): noise (around `offset`), an impulse planted at a corner of every frame, NaN / +Inf / -Inf elements"""
    rs = np.random.RandomState(seed)
    vol = (offset + rs.randn(*shape, T)).astype(dtype)
    vol[-1, -1, -1, :] += 8.0
    vol[0, 0, 0, ::2] -= 8.0
    flat = vol.reshape(-1)
    pos = rs.choice(flat.shape[0], size=max(3, flat.shape[0] // 40), replace=False)
    flat[pos] = np.resize(np.array([np.nan, np.inf, -np.inf], dtype=dtype), pos.shape[0])
    return vol


def frame_max(vol):
    a = np.abs(np.where(np.isfinite(vol), vol, 0).astype(np.float64))
    return a.reshape(-1, a.shape[3]).max(axis=0)


def zeroed64(vol):
    return np.where(np.isfinite(vol), vol, 0).astype(np.float64)


def scipy_resample(vol, A, b, shape, order, fill=0.0):
    """the reference: (X', Y', Z', T) f64"""
    a = zeroed64(vol)
    return np.stack([scipy.ndimage.affine_transform(a[..., t], A, offset=b, output_shape=shape, order=order, mode='constant',
                                                    cval=fill) for t in range(a.shape[3])], axis=-1)


def scipy_coordinates(A, b, shape):
    """(3, loci) in scipy's arithmetic: tmp = shift; tmp += coordinate[l] * matrix[l], l = 0, 1, 2"""
    o = np.indices(shape).reshape(3, -1).astype(np.float64)
    x = np.repeat(np.asarray(b, dtype=np.float64)[:, None], o.shape[1], axis=1)
    for l in range(3):
        x = x + o[l] * np.asarray(A, dtype=np.float64)[:, l:l + 1]
    return x


# ------------------------------------------------------------------------------------------- the restatement (numpy)
def _mirror(i, n, mutant=None):
    i = np.asarray(i)
    if n == 1:
        return np.zeros_like(i)
    if mutant == 'reflect':                               # d c b a | a b c d | d c b a
        i = i % (2 * n)
        return np.where(i < n, i, 2 * n - 1 - i)
    i = i % (2 * n - 2)                                   # d c b | a b c d | c b a
    return np.where(i < n, i, 2 * n - 2 - i)


def restate_prefilter_axis(a, axis, mutant=None, store=None):
    n = a.shape[axis]
    if n == 1:
        return a
    c = np.moveaxis(a, axis, 0).astype(np.float64)        # (a copy)
    if mutant != 'no_gain':
        c *= 6.0
    z, zn = POLE, POLE ** (n - 1)
    s = c[0] + zn * c[n - 1]
    zi = z
    for i in range(1, n - 1):
        s = s + zi * (c[i] + zn * c[n - 1 - i])
        zi *= z
    c[0] = s / (1.0 - zn * zn)
    for i in range(1, n):
        c[i] += z * c[i - 1]
    if mutant != 'no_anticausal_init':
        c[n - 1] = (z * c[n - 2] + c[n - 1]) * z / (z * z - 1.0)
    for i in range(n - 2, -1, -1):
        c[i] = z * (c[i + 1] - c[i])
    if store is not None:
        c = c.astype(store).astype(np.float64)            # one rounding to the storage dtype per axis
    return np.moveaxis(c, 0, axis)


def restate_prefilter(a, mutant=None, store=None, axes=(2, 1, 0)):
    """the coefficients of a 3-D f64 array; axes in the device's order when the array is (X, Y, Z): x (its n2) first"""
    for axis in axes:
        a = restate_prefilter_axis(a, axis, mutant, store)
    return a


def restate(vol, A, b, shape, order, fill=0.0, mutant=None, store=None):
    """the device's arithmetic restated: (X', Y', Z', T) f64.  `store`: the dtype the coefficients are rounded to per axis."""
    a = np.array(vol, dtype=np.float64)
    if mutant != 'keep_nonfinite':
        a[~np.isfinite(a)] = 0.0
    A, b = np.asarray(A, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if mutant == 'transposed':
        A = A.T
    if mutant == 'axes_not_reversed':                     # the kernel's axes are reversed: it needs P A P, and was given A
        A = A[::-1, ::-1]
    if mutant == 'b_not_permuted':
        b = b[::-1]
    x = scipy_coordinates(A, b, shape)
    n = np.array(a.shape[:3], dtype=np.float64)[:, None]
    inside = np.all((x >= 0) & (x <= (n if mutant == 'bound_n' else n - 1)), axis=0)
    xi = np.where(inside[None, :], x, 0.0)
    taps, weights = [], []
    for ax in range(3):
        if order == 0:
            taps.append([np.floor(xi[ax] if mutant == 'floor0' else xi[ax] + 0.5).astype(np.int64)])
            weights.append([np.ones(x.shape[1])])
            continue
        i0 = np.floor(xi[ax])
        y = xi[ax] - i0
        i0 = i0.astype(np.int64)
        if order == 1:
            taps.append([i0, i0 + 1])
            weights.append([1.0 - y, y])
        else:
            zc = 1.0 - y
            w1 = (y * y * (y - 2.0) * 3.0 + 4.0) / 6.0
            w2 = (zc * zc * (zc - 2.0) * 3.0 + 4.0) / 6.0
            w0 = zc * zc * zc / 6.0
            taps.append([i0 - 1, i0, i0 + 1, i0 + 2])
            weights.append([w0, w1, w2, 1.0 - w0 - w1 - w2])
        taps[-1] = [_mirror(t, a.shape[ax], mutant) for t in taps[-1]]
    if order == 0:
        taps = [[np.minimum(t[0], a.shape[ax] - 1)] for ax, t in enumerate(taps)]
    out = np.empty(tuple(shape) + (a.shape[3],))
    with np.errstate(invalid='ignore', over='ignore'):
        for t in range(a.shape[3]):
            f = a[..., t]
            if order == 3 or (order == 1 and mutant == 'prefilter_order1'):
                f = restate_prefilter(f, mutant, store)
            acc0 = 0.0
            for k0 in range(len(taps[0])):                # separable: z (the device's n2) innermost, then y, then x
                acc1 = 0.0
                for k1 in range(len(taps[1])):
                    acc2 = 0.0
                    for k2 in range(len(taps[2])):
                        acc2 = acc2 + weights[2][k2] * f[taps[0][k0], taps[1][k1], taps[2][k2]]
                    acc1 = acc1 + weights[1][k1] * acc2
                acc0 = acc0 + weights[0][k0] * acc1
            out[..., t] = np.where(inside, acc0, fill).reshape(shape)
    return out


def judge(got, ref, M, order, eps):
    """(passes, worst error in units of M); got, ref (..., T), M (T,)"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    with np.errstate(invalid='ignore'):
        err = np.abs(got - ref) / M
    worst = float(np.max(np.where(np.isnan(err), np.inf, err)))
    return worst <= bound(order, eps), worst


@functools.lru_cache(maxsize=None)
def case(name, dt, T=2, offset=0.0):
    """(vol (X, Y, Z, T), A, b, target shape, kind, M, {order: scipy's result}) - computed once, never written to"""
    src, shape, A, b, kind = CASES[name]
    vol = make_volume(src, T, DT[dt], seed=len(name) + T, offset=offset)
    refs = {order: scipy_resample(vol, A, b, shape, order) for order in (0, 1, 3)}
    for a in (vol,) + tuple(refs.values()):
        a.setflags(write=False)
    return vol, A, b, shape, kind, frame_max(vol), refs


def check_inputs(name):
    """what the module docstring promises of the inputs, asserted from scipy's coordinates"""
    src, shape, A, b, kind = CASES[name]
    x = scipy_coordinates(A, b, shape)
    n = np.array(src, dtype=np.float64)[:, None]
    inside = np.all((x >= 0) & (x <= n - 1), axis=0)
    if kind == 'outside':
        assert not inside.any()
        return
    assert inside.mean() >= 0.25, (name, inside.mean())
    if kind == 'oblique':
        live = (np.array(src) > 1)[:, None] & np.ones_like(x, dtype=bool)            # a zero row of A: x = 0 exactly, inside
        assert np.abs(x)[live].min() > 1e-9 and np.abs(x - (n - 1))[live].min() > 1e-9, name
        h = x + 0.5
        assert np.abs(h - np.round(h))[live].min() > 1e-9, name
        flat = ~live[:, 0]
        assert np.all(x[flat] == 0.0) and np.all(np.asarray(A)[flat] == 0) and np.all(np.asarray(b)[flat] == 0)
    if kind == 'exact':
        assert np.all(x * 4 == np.round(x * 4))                                      # every coordinate is exact
        assert np.any(x == 0) and np.any(x == n - 1), name                           # loci exactly on 0 and on n - 1
    if kind == 'shift':
        assert np.array_equal(A, np.eye(3)) and np.array_equal(b, np.floor(b))


def shifted_crop(vol, b, shape, fill=0.0):
    """out[o] = vol[o + b] where that exists, fill elsewhere; non-finite -> 0"""
    out = np.full(tuple(shape) + (vol.shape[3],), fill, dtype=vol.dtype)
    src = np.where(np.isfinite(vol), vol, 0).astype(vol.dtype)
    o = np.indices(shape).reshape(3, -1)
    s = o + np.asarray(b, dtype=np.int64)[:, None]
    ok = np.all((s >= 0) & (s < np.array(vol.shape[:3])[:, None]), axis=0)
    out[o[0][ok], o[1][ok], o[2][ok]] = src[s[0][ok], s[1][ok], s[2][ok]]
    return out


def affine_of(A, b, target_affine):
    """a source affine such that the module's (A, b) come out (up to rounding): affine = target_affine @ inv([[A, b], [0, 1]])"""
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = A, b
    return target_affine @ np.linalg.inv(m)


# ------------------------------------------------------------------------------------------------ layer 1: no GPU
@pytest.mark.parametrize('name', list(CASES))
def test_inputs_leave_nothing_out(name):
    check_inputs(name)


@pytest.mark.parametrize('name', list(CASES))
def test_restatement_against_scipy(name):
    vol, A, b, shape, kind, M, refs = case(name, 'f64')
    for order in (0, 1, 3):
        got = restate(vol, A, b, shape, order)
        if order == 0:
            assert np.array_equal(got, refs[0]), name
            continue
        err = np.abs(got - refs[order]).max() / M.max()
        print(name, order, 'restatement - scipy: %.3g M' % err)
        assert err <= bound(order, 0.0), (name, order, err)
    # the coefficients, in any order of the axes
    f = zeroed64(vol)[..., 0]
    want = scipy.ndimage.spline_filter(f, order=3, mode='mirror', output=np.float64)
    for axes in ((2, 1, 0), (0, 1, 2)):
        assert np.abs(restate_prefilter(f, axes=axes) - want).max() <= bound('coefficients', 0.0) * M[0], name
    # f32 storage of the coefficients, emulated: what the device's f32 path may differ by
    vol32 = vol.astype(np.float32)
    got32 = restate(vol32, A, b, shape, 3, store=np.float32).astype(np.float32)
    ok, worst = judge(got32, scipy_resample(vol32, A, b, shape, 3), frame_max(vol32), 3, float(np.finfo(np.float32).eps))
    print(name, 'f32 storage emulated: %.3g eps32 M' % (worst / float(np.finfo(np.float32).eps)))
    assert ok, (name, worst)
    if kind == 'shift':
        assert np.array_equal(refs[0], shifted_crop(vol, b, shape))


def test_prefilter_gain_is_three():
    n = 33
    alt = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    assert abs(np.abs(scipy.ndimage.spline_filter1d(alt, order=3, mode='mirror')).max() - 3.0) <= 1e-9
    for m in (1, 2, 3, 70, 300):                          # every length the GPU tests use, against scipy
        x = np.random.RandomState(m).randn(m, 2, 2)
        want = scipy.ndimage.spline_filter1d(x, order=3, axis=0, mode='mirror')
        assert np.abs(restate_prefilter_axis(x, 0) - want).max() <= 200 * EPS64 * np.abs(x).max()


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_judge_rejects_mutants(dt):
    eps = float(np.finfo(DT[dt]).eps)
    applies = {'floor0': (0,), 'no_anticausal_init': (3,), 'no_gain': (3,), 'prefilter_order1': (1,)}
    worst_ratio = {m: 0.0 for m in MUTANTS}
    for name in ('oblique', '2mm to 3mm', 'magnify', 'half', 'flat'):
        vol, A, b, shape, kind, M, refs = case(name, dt)
        for order in (0, 1, 3):
            good = restate(vol, A, b, shape, order, store=DT[dt]).astype(DT[dt])           # the restatement: accepted
            ok, worst = judge(good, refs[order], M, order, eps)
            assert ok, (name, order, worst)
            for m in MUTANTS:
                if order not in applies.get(m, (0, 1, 3)):
                    continue
                bad = restate(vol, A, b, shape, order, mutant=m, store=DT[dt]).astype(DT[dt])
                err = judge(bad, refs[order], M, order, eps)[1]
                ref_bound = bound(order, eps) if order else bound(3, eps)       # (bits at order 0: any difference fails)
                worst_ratio[m] = max(worst_ratio[m], err / ref_bound)
    print({m: '%.3g' % r for m, r in worst_ratio.items()})
    assert all(r >= 100.0 for r in worst_ratio.values()), worst_ratio


def test_resample_host_against_scipy():
    from modl_amd.masker import resample_host, resample_mask
    from modl_amd import _lib
    target_affine = np.array([[3.0, 0, 0, -20], [0, 3, 0, -31], [0, 0, 3, 7], [0, 0, 0, 1]])
    from modl_amd.masker import _grid_transform
    for name in CASES:
        if name == 'flat':                                                      # (a singular A is no pair of affines)
            continue
        for dt in ('f32', 'f64'):
            vol, A, b, shape, kind, M, refs = case(name, dt)
            aff = affine_of(A, b, target_affine)
            A2, b2 = _grid_transform(aff, target_affine)
            assert np.abs(A2 - A).max() <= 1e-13 and np.abs(b2 - b).max() <= 1e-12
            crop = np.array_equal(A2, np.eye(3)) and np.array_equal(b2, np.floor(b2))
            for interp, order in ORDERS.items():
                order = 0 if crop else order
                got = resample_host(vol, aff, target_affine, shape, interp)
                assert got.shape == tuple(shape) + (vol.shape[3],) and got.dtype == DT[dt]
                want = scipy_resample(vol, A2, b2, shape, order).astype(DT[dt])
                assert same_bits(got, want), (name, dt, interp)
                assert same_bits(resample_host(np.asfortranarray(vol), aff, target_affine, shape, interp), got)
    # the identity plus an integer shift: the crop, whatever the interpolation; a fill value; a 3-D input; another dtype
    vol, A, b, shape, kind, M, refs = case('shift', 'f32')
    aff = np.eye(4)
    tgt = np.eye(4)
    tgt[:3, 3] = b
    for interp in ORDERS:
        assert same_bits(resample_host(vol, aff, tgt, shape, interp, fill_value=-3.5), shifted_crop(vol, b, shape, -3.5))
    assert same_bits(resample_host(vol[..., 0], aff, tgt, shape), resample_host(vol[..., :1], aff, tgt, shape))
    assert resample_host(np.ones((5, 6, 7), np.int16), aff, tgt, shape).dtype == np.float64
    if _lib.lib.modl_device_count() == 0:                                       # without a GPU: the host path
        assert same_bits(resample(vol, aff, tgt, shape), resample_host(vol, aff, tgt, shape))
        mask = random_mask(shape, seed=3)
        perm = np.random.RandomState(0).permutation(vol.shape[3])
        rows = resample_mask(vol, aff, mask, tgt, dst_row=perm)
        assert same_bits(rows[perm], resample_host(vol, aff, tgt, shape)[mask].T)


def test_voxel_size_of():
    from modl_amd.masker import voxel_size_of
    assert voxel_size_of(np.diag([2.0, 3.0, 1.5, 1.0])) == (2.0, 3.0, 1.5)
    a = np.eye(4)
    a[:3, :3] = 2.5 * _rot(0.3, 0.2, -0.4)
    a[:3, 3] = (-90, -126, -72)
    assert np.allclose(voxel_size_of(a), 2.5, rtol=0, atol=1e-14)
    a[:3, :3] = np.array([[1.0, 2, 0], [2, 1, 0], [2, 2, 4]])
    assert np.allclose(voxel_size_of(a), np.sqrt([9.0, 9.0, 16.0]))
    with pytest.raises(ValueError, match='singular'):
        voxel_size_of(np.diag([2.0, 0.0, 2.0, 1.0]))


def test_value_errors_name_the_offender():
    from modl_amd.masker import resample_host, resample_mask, ArrayMasker
    vol = np.ones((4, 3, 2, 2))
    eye = np.eye(4)
    sing = np.diag([2.0, 2.0, 0.0, 1.0])
    for f in (resample, resample_host):
        with pytest.raises(ValueError, match='^affine is singular'):
            f(vol, sing, eye, (4, 3, 2))
        with pytest.raises(ValueError, match='^target_affine is singular'):
            f(vol, eye, sing, (4, 3, 2))
        with pytest.raises(ValueError, match=r'^affine must be a 4 x 4 matrix.*\(3, 3\)'):
            f(vol, np.eye(3), eye, (4, 3, 2))
        with pytest.raises(ValueError, match='^target_affine has non-finite'):
            f(vol, eye, np.diag([1.0, np.nan, 1.0, 1.0]), (4, 3, 2))
        with pytest.raises(ValueError, match='^affine must have the last row'):
            f(vol, np.arange(16.0).reshape(4, 4), eye, (4, 3, 2))
        with pytest.raises(ValueError, match='target_shape.*-3'):
            f(vol, eye, eye, (4, -3, 2))
        with pytest.raises(ValueError, match='target_shape'):
            f(vol, eye, eye, (4, 3))
        with pytest.raises(ValueError, match='target_shape.*2.5'):
            f(vol, eye, eye, (4, 3, 2.5))
        with pytest.raises(ValueError, match="interpolation.*'cubic'"):
            f(vol, eye, eye, (4, 3, 2), interpolation='cubic')
        with pytest.raises(ValueError, match='fill_value.*nan'):
            f(vol, eye, eye, (4, 3, 2), fill_value=np.nan)
        with pytest.raises(ValueError, match="fill_value.*'x'"):
            f(vol, eye, eye, (4, 3, 2), fill_value='x')
        with pytest.raises(ValueError, match=r'volume must be.*\(4, 3\)'):
            f(vol[..., 0, 0], eye, eye, (4, 3, 2))
    mask = np.ones((4, 3, 2), dtype=bool)
    with pytest.raises(ValueError, match='^mask_affine is singular'):
        resample_mask(vol, eye, mask, sing)
    with pytest.raises(ValueError, match='boolean'):
        resample_mask(vol, eye, mask.astype(np.uint8), eye)
    with pytest.raises(ValueError, match='permutation'):
        resample_mask(vol, eye, mask, eye, dst_row=[0, 0])
    with pytest.raises(ValueError, match='^mask_affine is singular'):
        ArrayMasker(mask, mask_affine=sing).fit()
    with pytest.raises(ValueError, match='no mask_affine'):
        ArrayMasker(mask).fit().transform(vol, affine=eye)
    with pytest.raises(ValueError, match='^affine is singular'):
        ArrayMasker(mask, mask_affine=eye).fit().transform(vol, affine=sing)
    with pytest.raises(ValueError, match=r'\(5, 3, 2\).*\(4, 3, 2\)'):           # another shape and no affine: as before
        ArrayMasker(mask, mask_affine=eye).fit().transform(np.ones((5, 3, 2, 2)))


# ---- the refusals of the entry points: the good call, and one argument wrong at a time
KBOX, KTARGET, KT = (5, 4, 3), (4, 3, 6), 2               # the kernel's boxes of the refusal tests


def _bad_resample_calls(V, ld):
    nan9, inf3 = np.eye(3).ravel(), np.zeros(3)
    nan9[5], inf3[1] = np.nan, np.inf
    return [('null vol', dict(vol=None), EINVAL), ('null A', dict(A=None), EINVAL), ('null b', dict(b=None), EINVAL),
            ('null out', dict(out=None), EINVAL), ('T = 0', dict(T=0), EINVAL), ('n0 = 0', dict(n0=0), EINVAL),
            ('n1 < 0', dict(n1=-1), EINVAL), ('n2 = 0', dict(n2=0), EINVAL), ('m0 = 0', dict(m0=0), EINVAL),
            ('m2 < 0', dict(m2=-4), EINVAL), ('source box above INT32_MAX', dict(n0=1 << 20, n1=1 << 11), EINVAL),
            ('target box above INT32_MAX', dict(m1=1 << 16, m2=1 << 16), EINVAL), ('nan in A', dict(A=nan9), EINVAL),
            ('inf in b', dict(b=inf3), EINVAL), ('nan fill', dict(fill=np.nan), EINVAL), ('inf fill', dict(fill=np.inf), EINVAL),
            ('order 2', dict(order=2), EINVAL), ('order -1', dict(order=-1), EINVAL), ('order 4', dict(order=4), EINVAL),
            ('V = 0', dict(V=0), EINVAL), ('V > box', dict(V=10 ** 6, ldo=10 ** 6), EINVAL), ('ldo < V', dict(ldo=V - 1), EINVAL),
            ('frame stride < box', dict(fs='box-1'), EINVAL), ('out inside vol', dict(out='vol'), EINVAL),
            ('out overlaps the last frame', dict(out='vol+last'), EINVAL), ('ws inside vol', dict(ws='vol'), EINVAL),
            ('ws is out', dict(ws='out'), EINVAL), ('null ws', dict(ws=None), ENOMEM), ('small ws', dict(ws_bytes='short'), ENOMEM),
            ('bad pointer and no workspace', dict(vol=None, ws=None), EINVAL),
            ('box mode: ldo < box', dict(vox=None, ldo=71), EINVAL)]


def _call_resample(lib, dt, ptrs, V, ld, over):
    n0, n1, n2 = KBOX
    m0, m1, m2 = KTARGET
    es = 4 if dt == 'f32' else 8
    a = dict(vol=ptrs['vol'], fs=n0 * n1 * n2, T=KT, n0=n0, n1=n1, n2=n2, A=0.9 * np.eye(3).ravel(), b=np.full(3, 0.25), order=3,
             fill=0.0, m0=m0, m1=m1, m2=m2, vox=ptrs['vox'], V=V, perm=None, dst=ptrs['dst'], out=ptrs['out'], ldo=ld, ws=ptrs['ws'])
    a['ws_bytes'] = lib.modl_resample_workspace(0 if dt == 'f32' else 1, KT, n0, n1, n2, 3)
    a.update(over)
    if a['fs'] == 'box-1':
        a['fs'] = n0 * n1 * n2 - 1
    if a['out'] == 'vol':
        a['out'] = a['vol']
    elif a['out'] == 'vol+last':
        a['out'] = a['vol'] + (KT * n0 * n1 * n2 - 1) * es
    if a['ws'] == 'vol':
        a['ws'] = a['vol']
    elif a['ws'] == 'out':
        a['ws'] = a['out']
    if a['ws_bytes'] == 'short':
        a['ws_bytes'] = lib.modl_resample_workspace(0 if dt == 'f32' else 1, KT, n0, n1, n2, 3) - 1
    vp = lambda v: C.c_void_p(v) if v else C.c_void_p(0)
    hp = lambda v: None if v is None else v.ctypes.data
    return getattr(lib, 'modl_resample_' + dt)(vp(a['vol']), a['fs'], a['T'], a['n0'], a['n1'], a['n2'], hp(a['A']), hp(a['b']),
                                               a['order'], a['fill'], a['m0'], a['m1'], a['m2'], vp(a['vox']), a['V'],
                                               vp(a['perm']), vp(a['dst']), vp(a['out']), a['ldo'], vp(a['ws']), a['ws_bytes'], None)


def _bad_prefilter_calls():
    return [('null vol', dict(vol=None), EINVAL), ('null coef', dict(coef=None), EINVAL), ('T = 0', dict(T=0), EINVAL),
            ('n1 = 0', dict(n1=0), EINVAL), ('frame stride < box', dict(fs=59), EINVAL), ('coef stride < box', dict(cfs=59), EINVAL),
            ('coef is vol', dict(coef='vol'), EINVAL), ('ws is coef', dict(ws='coef'), EINVAL), ('null ws', dict(ws=None), ENOMEM),
            ('small ws', dict(ws_bytes='short'), ENOMEM)]


def _call_prefilter(lib, dt, ptrs, over):
    n0, n1, n2 = KBOX
    a = dict(vol=ptrs['vol'], fs=n0 * n1 * n2, T=KT, n0=n0, n1=n1, n2=n2, coef=ptrs['coef'], cfs=n0 * n1 * n2, ws=ptrs['ws'])
    a['ws_bytes'] = lib.modl_resample_workspace(0 if dt == 'f32' else 1, KT, n0, n1, n2, 3)
    a.update(over)
    if a['coef'] == 'vol':
        a['coef'] = a['vol']
    if a['ws'] == 'coef':
        a['ws'] = a['coef']
    if a['ws_bytes'] == 'short':
        a['ws_bytes'] = lib.modl_resample_workspace(0 if dt == 'f32' else 1, KT, n0, n1, n2, 3) - 1
    vp = lambda v: C.c_void_p(v) if v else C.c_void_p(0)
    return getattr(lib, 'modl_spline_prefilter_' + dt)(vp(a['vol']), a['fs'], a['T'], a['n0'], a['n1'], a['n2'], vp(a['coef']),
                                                       a['cfs'], vp(a['ws']), a['ws_bytes'], None)


def _workspace_refusals(lib):
    for dt, es in ((0, 4), (1, 8)):
        need = lib.modl_resample_workspace(dt, 3, 5, 4, 3, 3)
        assert 3 * 60 * (es + 8) <= need <= 3 * 60 * (es + 8) + 512
        assert lib.modl_resample_workspace(dt, 3, 5, 4, 3, 0) == 0 and lib.modl_resample_workspace(dt, 3, 5, 4, 3, 1) == 0
    for args in ((7, 3, 5, 4, 3, 3), (0, 0, 5, 4, 3, 3), (0, 3, 0, 4, 3, 3), (0, 3, 5, -1, 3, 3), (0, 3, 5, 4, 0, 3),
                 (0, 3, 5, 4, 3, 2), (0, 3, 5, 4, 3, -1), (0, 3, 1 << 20, 1 << 20, 4, 3)):
        assert lib.modl_resample_workspace(*args) == 0, args
    assert 64 <= lib.modl_resample_lds_line() < 300 and lib.modl_resample_frames() >= 1


def _host_buffers(dt, V, ld):
    n = int(np.prod(KBOX))
    return dict(vol=np.ones((KT, n), DT[dt]), vox=np.arange(V, dtype=np.int64), dst=np.arange(KT, dtype=np.int64),
                out=np.full((KT, ld), SENT, DT[dt]), ws=np.zeros(8192, np.uint8), coef=np.full((KT, n), SENT, DT[dt]),
                big=np.full((KT, int(np.prod(KTARGET))), SENT, DT[dt]))


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_entry_points_refuse_bad_arguments_without_a_device(dt):
    from modl_amd._lib import lib
    _workspace_refusals(lib)
    V, ld = 20, 23
    bufs = _host_buffers(dt, V, ld)
    ptrs = {k: v.ctypes.data for k, v in bufs.items()}
    for name, over, code in _bad_resample_calls(V, ld):
        assert _call_resample(lib, dt, ptrs, V, ld, over) == code, name
    for name, over, code in _bad_prefilter_calls():
        assert _call_prefilter(lib, dt, ptrs, over) == code, name
    assert np.all(bufs['out'] == SENT) and np.all(bufs['coef'] == SENT) and np.all(bufs['ws'] == 0)
    if lib.modl_device_count() == 0:
        assert _call_resample(lib, dt, ptrs, V, ld, {}) == ENOGPU
        assert _call_resample(lib, dt, ptrs, V, ld, dict(order=1, ws=None, ws_bytes=0)) == ENOGPU      # no workspace needed
        assert _call_resample(lib, dt, ptrs, V, ld, dict(ws=None)) == ENOMEM                            # ENOMEM before ENOGPU
        assert _call_prefilter(lib, dt, ptrs, {}) == ENOGPU


# ---- ArrayMasker and the estimators
MASK_AFFINE = np.array([[3.0, 0, 0, -12], [0, 3, 0, -15], [0, 0, 3, -9], [0, 0, 0, 1]])     # the mask: 3 mm, (9, 10, 9)
RECORD_AFFINE = np.array([[2.0, 0, 0, -12.5], [0, 2, 0, -14], [0, 0, 2, -10.5], [0, 0, 0, 1]])     # records: 2 mm, (13, 15, 13)


def _fmri_grids(dtype):
    mask = random_mask((9, 10, 9), seed=5, p=0.5)
    rs = np.random.RandomState(1)
    vols = [(100 + 20 * rs.randn(13, 15, 13, 30)).astype(dtype), np.asfortranarray((100 + 20 * rs.randn(13, 15, 13, 25)).astype(dtype))]
    vols[0][3, 4, 5, 6] = np.nan
    atlas = rs.randn(11, 12, 10, 4).astype(dtype)                                # maps on a third grid
    atlas_affine = np.array([[2.5, 0, 0, -13], [0, 2.5, 0, -15.5], [0, 0, 2.5, -10], [0, 0, 0, 1]])
    kw = dict(n_components=4, n_epochs=2, random_state=0, batch_size=10, alpha=0.1, reduction=2)
    return vols, mask, atlas, atlas_affine, kw


def _pre_resampled(vols, dtype):
    """the records resampled beforehand with scipy, 'continuous'"""
    from modl_amd.masker import _grid_transform
    A, b = _grid_transform(RECORD_AFFINE, MASK_AFFINE)
    return [scipy_resample(v, A, b, (9, 10, 9), 3).astype(dtype) for v in vols]


def test_array_masker_other_grid_host_logic():
    from modl_amd import _lib
    from modl_amd.masker import ArrayMasker, resample_host, resample_mask, smooth_mask, voxel_size_of
    vols, mask, atlas, atlas_affine, kw = _fmri_grids(np.float64)
    vol = vols[0]
    m = ArrayMasker(mask, mask_affine=MASK_AFFINE).fit()
    assert m.voxel_size_ == (3.0, 3.0, 3.0) == voxel_size_of(MASK_AFFINE)
    assert ArrayMasker(mask, (2, 2, 2), mask_affine=MASK_AFFINE).fit().voxel_size_ == (2, 2, 2)
    assert ArrayMasker(mask).fit().voxel_size_ == (1, 1, 1)
    # the same grid: today's path, bit for bit (allclose affine, same shape)
    on_grid = np.random.RandomState(2).randn(9, 10, 9, 5)
    near = MASK_AFFINE.copy()
    near[:3] *= 1 + 1e-12
    assert same_bits(m.transform(on_grid, affine=near), ArrayMasker(mask).fit().transform(on_grid))
    assert same_bits(m.transform(on_grid), ArrayMasker(mask).fit().transform(on_grid))
    sm = ArrayMasker(mask, smoothing_fwhm=6, mask_affine=MASK_AFFINE).fit()
    assert same_bits(sm.transform(on_grid, affine=MASK_AFFINE), smooth_mask(on_grid, mask, 6, (3, 3, 3)))
    if _lib.lib.modl_device_count() > 0:
        return                                                                   # (the device's arithmetic: layer 2)
    # another grid: rows mode alone without smoothing; box mode, then the smoothing, with it
    box = resample_host(vol, RECORD_AFFINE, MASK_AFFINE, mask.shape)
    assert same_bits(m.transform(vol, affine=RECORD_AFFINE), box[mask].T)
    assert same_bits(resample_mask(vol, RECORD_AFFINE, mask, MASK_AFFINE), box[mask].T)
    assert same_bits(sm.transform(vol, affine=RECORD_AFFINE), smooth_mask(box, mask, 6, (3, 3, 3)))
    perm = np.random.RandomState(0).permutation(vol.shape[3])
    assert same_bits(m.mask_volume(vol, dst_row=perm, affine=RECORD_AFFINE)[perm], box[mask].T)
    assert same_bits(sm.mask_volume(vol, dst_row=perm, affine=RECORD_AFFINE)[perm], smooth_mask(box, mask, 6, (3, 3, 3)))
    # cleaning on top, and maps: masked, never smoothed
    cl = ArrayMasker(mask, smoothing_fwhm=6, standardize=True, detrend=True, mask_affine=MASK_AFFINE).fit()
    from modl_amd.signal import clean
    assert same_bits(cl.transform(vol, affine=RECORD_AFFINE), clean(smooth_mask(box, mask, 6, (3, 3, 3)), True, True))
    assert same_bits(sm.mask_maps(atlas, affine=atlas_affine), resample_host(atlas, atlas_affine, MASK_AFFINE, mask.shape)[mask].T)


def _check_resampling_estimators(fMRIDictFact, fMRICoder, dtype):
    """the wiring.  Records on another grid, inside the estimators, against the same records resampled beforehand - with
    the library's own function (the same bits) and with scipy (within the judge's bound carried through the coder)."""
    from modl_amd.fmri import rfMRIDictionaryScorer
    from modl_amd.masker import resample, resample_mask
    vols, mask, atlas, atlas_affine, kw = _fmri_grids(dtype)
    mk = dict(mask=mask, mask_affine=MASK_AFFINE)
    own = [np.asarray(resample(v, RECORD_AFFINE, MASK_AFFINE, mask.shape)) for v in vols]
    init = np.ascontiguousarray(resample_mask(atlas, atlas_affine, mask, MASK_AFFINE))
    for extra in (dict(), dict(smoothing_fwhm=6), dict(standardize=True, detrend=True)):
        a = fMRIDictFact(dict_init=(atlas, atlas_affine), **mk, **extra, **kw).fit(vols, affines=RECORD_AFFINE)
        b = fMRIDictFact(dict_init=init, mask=mask, voxel_size=(3, 3, 3), **extra, **kw).fit(own)
        assert a.components_img_.shape == mask.shape + (4,)
        assert same_bits(a.components_, b.components_), extra
    # one affine per record; a record on the mask's grid next to one that is not; transform, score, coder, scorer
    a = fMRIDictFact(**mk, **kw).fit([vols[0], own[1]], affines=[RECORD_AFFINE, MASK_AFFINE])
    b = fMRIDictFact(mask=mask, **kw).fit(own)
    assert same_bits(a.components_, b.components_)
    assert same_bits(a.components_, fMRIDictFact(**mk, **kw).fit([vols[0], own[1]], affines=[RECORD_AFFINE, None]).components_)
    for x, y in zip(a.transform(vols, affines=RECORD_AFFINE), b.transform(own)):
        assert same_bits(np.asarray(x), np.asarray(y))
    assert a.score(vols, affines=[RECORD_AFFINE] * 2) == b.score(own)
    c_on = fMRICoder((atlas, atlas_affine), alpha=0.1, **mk).fit()
    c_off = fMRICoder(init, alpha=0.1, mask=mask).fit()
    assert same_bits(c_on.components_, c_off.components_) and c_on.components_img_.shape == mask.shape + (4,)
    for x, y in zip(c_on.transform(vols, affines=RECORD_AFFINE), c_off.transform(own)):
        assert same_bits(np.asarray(x), np.asarray(y))
    assert c_on.score(vols, affines=RECORD_AFFINE) == c_off.score(own)
    s_on, s_off = rfMRIDictionaryScorer(vols, test_affines=RECORD_AFFINE), rfMRIDictionaryScorer(own)
    s_on(a, a.dict_fact_, 0.0, 0.0)
    s_off(b, b.dict_fact_, 0.0, 0.0)
    assert s_on.score == s_off.score
    # affines=None: what it was
    assert same_bits(fMRIDictFact(mask=mask, **kw).fit(own, affines=None).components_, b.components_)
    # against scipy: the codes of a record move by the resampling error times what the ridge coder amplifies.  The codes
    # are c = (D D' + lambda I)^-1 D x with some lambda >= 0, an operator of norm max s / (s^2 + lambda) <= 1 / s_min(D);
    # ||dx|| <= sqrt(V) bound M, and the solve itself rounds: cond(D D') eps |c|, with a factor 16
    eps = float(np.finfo(dtype).eps)
    pre = _pre_resampled(vols, dtype)
    sv = np.linalg.svd(np.asarray(a.components_, dtype=np.float64), compute_uv=False)
    for x, y, v in zip(a.transform(vols, affines=RECORD_AFFINE), b.transform(pre), vols):
        dx = np.sqrt(a.components_.shape[1]) * (bound(3, eps) + eps) * frame_max(v).max()
        tol = dx / sv.min() + 16 * eps * (sv.max() / sv.min()) ** 2 * np.abs(np.asarray(y)).max()
        assert np.abs(np.asarray(x, dtype=np.float64) - np.asarray(y, dtype=np.float64)).max() <= tol
    with pytest.raises(ValueError, match='affines'):
        fMRIDictFact(**mk, **kw).fit(vols, affines=[RECORD_AFFINE])
    with pytest.raises(ValueError, match='mask_affine'):
        fMRIDictFact(mask=mask, **kw).fit(vols, affines=RECORD_AFFINE)
    with pytest.raises(ValueError, match='mask'):
        fMRIDictFact(dict_init=(atlas, atlas_affine), **kw).fit(own)
    params = fMRIDictFact().get_params()
    assert params['mask_affine'] is None and fMRICoder(init).get_params()['mask_affine'] is None


def test_estimators_resample_records_host_logic():
    est, coder = _host_estimators()
    _check_resampling_estimators(est, coder, np.float64)


# ------------------------------------------------------------------------------------------------ layer 2: the GPU
@pytest.fixture(scope='module')
def gpu():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    return torch


def kernel_args(A, b):
    """P A P and P b: the kernel's axes are the user's reversed"""
    return np.ascontiguousarray(np.asarray(A, dtype=np.float64)[::-1, ::-1]), np.ascontiguousarray(np.asarray(b, dtype=np.float64)[::-1])


def _padded_frames(frames, fs_pad):
    """device copy of (T, n0, n1, n2) with the frame stride box + fs_pad, the padding holding SENT"""
    import torch
    T = frames.shape[0]
    box = int(np.prod(frames.shape[1:]))
    host = np.full((T, box + fs_pad), SENT, dtype=frames.dtype)
    host[:, :box] = frames.reshape(T, box)
    return torch.from_numpy(host).to('cuda'), host


def _guarded(n, dtype):
    import torch
    return torch.full((2 * GUARD + n,), SENT, dtype=dtype, device='cuda')


def _workspace(need):
    import torch
    return torch.full((need + 512,), 0xA5, dtype=torch.uint8, device='cuda')


def _check_workspace(d_ws, need):
    ws = d_ws.cpu().numpy()
    assert np.all(ws[:256] == 0xA5) and np.all(ws[256 + need:] == 0xA5)


def gpu_prefilter(frames, fs_pad=5, cs_pad=3):
    """modl_spline_prefilter_* on frames (T, n0, n1, n2): the coefficients; strides larger than the box, sentinels kept"""
    import torch
    from modl_amd._lib import lib, check
    T, n0, n1, n2 = frames.shape
    box = n0 * n1 * n2
    sx = 'f32' if frames.dtype == np.float32 else 'f64'
    es = frames.dtype.itemsize
    d_vol, host = _padded_frames(frames, fs_pad)
    d_buf = _guarded(T * (box + cs_pad), d_vol.dtype)
    need = lib.modl_resample_workspace(0 if sx == 'f32' else 1, T, n0, n1, n2, 3)
    assert need > 0
    d_ws = _workspace(need)
    check(getattr(lib, 'modl_spline_prefilter_' + sx)(
        C.c_void_p(d_vol.data_ptr()), box + fs_pad, T, n0, n1, n2, C.c_void_p(d_buf.data_ptr() + GUARD * es), box + cs_pad,
        C.c_void_p(d_ws.data_ptr() + 256), need, None), 'modl_spline_prefilter')
    torch.cuda.synchronize()
    buf = d_buf.cpu().numpy()
    out = buf[GUARD:GUARD + T * (box + cs_pad)].reshape(T, box + cs_pad)
    assert np.all(buf[:GUARD] == SENT) and np.all(buf[GUARD + T * (box + cs_pad):] == SENT) and np.all(out[:, box:] == SENT)
    _check_workspace(d_ws, need)
    assert np.array_equal(d_vol.cpu().numpy(), host, equal_nan=True)
    return np.ascontiguousarray(out[:, :box]).reshape(frames.shape)


def gpu_resample(frames, Ak, bk, order, target, fill=0.0, vox=None, dst=None, pad=3, fs_pad=5, perm=None):
    """modl_resample_* on frames (T, n0, n1, n2) in the KERNEL's axis order (Ak, bk and `target` (m0, m1, m2) too): box mode
    (T, m0, m1, m2), rows mode (T, V).  The output has the stride width + pad inside guard elements, the workspace sits inside
    guard bytes: asserts that padding, guards and the input are untouched."""
    import torch
    from modl_amd._lib import lib, check
    from modl_amd.device import ptr
    T, n0, n1, n2 = frames.shape
    box = n0 * n1 * n2
    sx = 'f32' if frames.dtype == np.float32 else 'f64'
    es = frames.dtype.itemsize
    d_vol, host = _padded_frames(frames, fs_pad)
    width = int(np.prod(target)) if vox is None else len(vox)
    ld = width + pad
    d_buf = _guarded(T * ld, d_vol.dtype)
    d_vox = None if vox is None else torch.from_numpy(np.ascontiguousarray(vox, dtype=np.int64)).to('cuda')
    d_dst = None if dst is None else torch.from_numpy(np.ascontiguousarray(dst, dtype=np.int64)).to('cuda')
    d_perm = None if perm is None else torch.from_numpy(np.ascontiguousarray(perm, dtype=np.int64)).to('cuda')
    need = lib.modl_resample_workspace(0 if sx == 'f32' else 1, T, n0, n1, n2, order)
    assert (need > 0) == (order == 3)
    d_ws = _workspace(need)
    Ak, bk = np.ascontiguousarray(Ak, dtype=np.float64), np.ascontiguousarray(bk, dtype=np.float64)
    check(getattr(lib, 'modl_resample_' + sx)(
        C.c_void_p(d_vol.data_ptr()), box + fs_pad, T, n0, n1, n2, Ak.ctypes.data, bk.ctypes.data, order, fill, *target, ptr(d_vox),
        width if vox is not None else 0, ptr(d_perm), ptr(d_dst), C.c_void_p(d_buf.data_ptr() + GUARD * es), ld,
        C.c_void_p(d_ws.data_ptr() + 256) if need else None, need, None), 'modl_resample')
    torch.cuda.synchronize()
    buf = d_buf.cpu().numpy()
    out = buf[GUARD:GUARD + T * ld].reshape(T, ld)
    assert np.all(buf[:GUARD] == SENT) and np.all(buf[GUARD + T * ld:] == SENT) and np.all(out[:, width:] == SENT)
    _check_workspace(d_ws, need)
    assert np.array_equal(d_vol.cpu().numpy(), host, equal_nan=True)
    out = np.ascontiguousarray(out[:, :width])
    return out.reshape((T,) + tuple(target)) if vox is None else out


def to_frames(vol):
    """(X, Y, Z, T) -> (T, Z, Y, X), contiguous"""
    return np.ascontiguousarray(vol.transpose(3, 2, 1, 0))


def from_frames(frames):
    return frames.transpose(3, 2, 1, 0)


@pytest.mark.gpu
@pytest.mark.parametrize('box', PREFILTER_BOXES, ids=lambda b: '%dx%dx%d' % b)
@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_prefilter_through_the_abi(gpu, dt, box):
    from modl_amd._lib import lib
    line = lib.modl_resample_lds_line()
    assert PREFILTER_BOXES[2][2] > 64 and PREFILTER_BOXES[2][2] <= line < PREFILTER_BOXES[3][2]    # LDS slab, and the direct walk
    eps = float(np.finfo(DT[dt]).eps)
    for offset in (0.0, 1e4):
        vol = make_volume(box, 3, DT[dt], seed=sum(box), offset=offset)          # here (X, Y, Z) IS the kernel's (n0, n1, n2)
        frames = np.ascontiguousarray(vol.transpose(3, 0, 1, 2))
        got = gpu_prefilter(frames)
        a = zeroed64(vol)
        want = np.stack([scipy.ndimage.spline_filter(a[..., t], order=3, mode='mirror', output=np.float64) for t in range(3)])
        ok, worst = judge(got.transpose(1, 2, 3, 0), want.transpose(1, 2, 3, 0), frame_max(vol), 'coefficients', eps)
        print(box, dt, offset, 'coefficients: %.3g eps M' % (worst / eps))
        assert ok, worst
        assert same_bits(gpu_prefilter(frames[1:2]), got[1:2])                   # a frame does not see the others
        assert same_bits(gpu_prefilter(frames, fs_pad=0, cs_pad=0), got)


BOX_CASES = ['oblique', '2mm to 3mm', 'magnify', 'half', 'double', 'flat', 'shift', 'outside']


@pytest.mark.gpu
@pytest.mark.parametrize('name', BOX_CASES)
@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_box_mode_through_the_abi(gpu, dt, name):
    from modl_amd._lib import lib
    check_inputs(name)
    eps = float(np.finfo(DT[dt]).eps)
    assert lib.modl_resample_frames() < 5                                       # T = 5: more than one chunk of frames
    for T, offset in ((1, 0.0), (5, 0.0), (2, 1e4)):
        vol, A, b, shape, kind, M, refs = case(name, dt, T, offset)
        Ak, bk = kernel_args(A, b)
        frames = to_frames(vol)
        for order in (0, 1, 3):
            got = from_frames(gpu_resample(frames, Ak, bk, order, shape[::-1]))
            if kind == 'shift':
                assert same_bits(got, shifted_crop(vol, b, shape)), (T, order)  # the crop, whatever the order
            elif kind == 'outside':
                assert np.all(got == 0), (T, order)
            elif order == 0:
                assert same_bits(got, refs[0].astype(DT[dt])), (T, order)
            else:
                ok, worst = judge(got, refs[order], M, order, eps)
                print(name, dt, 'T = %d, offset %g, order %d: %.3g eps M' % (T, offset, order, worst / eps))
                assert ok, (T, order, worst)
    # the fill value; a source of NaN only, entirely outside: all fill, nothing of the source reaches the arithmetic
    vol, A, b, shape, kind, M, refs = case(name, dt, 2)
    Ak, bk = kernel_args(A, b)
    for order in (0, 1, 3):
        got = from_frames(gpu_resample(to_frames(vol), Ak, bk, order, shape[::-1], fill=-2.5))
        x = scipy_coordinates(A, b, shape)
        inside = np.all((x >= 0) & (x <= np.array(vol.shape[:3])[:, None] - 1), axis=0).reshape(shape)
        assert np.all(got[~inside] == -2.5)
        plain = from_frames(gpu_resample(to_frames(vol), Ak, bk, order, shape[::-1]))
        assert same_bits(got[inside], plain[inside])
    if kind == 'outside':
        nans = np.full_like(vol, np.nan)
        for order in (0, 1, 3):
            assert np.all(gpu_resample(to_frames(nans), Ak, bk, order, shape[::-1], fill=7.0) == 7.0)


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_rows_mode_through_the_abi(gpu, dt):
    for name in ('oblique', '2mm to 3mm', 'magnify', 'half', 'shift'):
        vol, A, b, shape, kind, M, refs = case(name, dt, 5)
        T = vol.shape[3]
        Ak, bk = kernel_args(A, b)
        frames = to_frames(vol)
        mask = random_mask(shape, seed=4, p=0.4)
        mask[0, 0, 0] = mask[-1, -1, -1] = True                                   # the first and the last voxel of the box
        one = np.zeros(shape, dtype=bool)
        one[shape[0] // 2, 1, shape[2] - 1] = True
        for order in (0, 1, 3):
            box = from_frames(gpu_resample(frames, Ak, bk, order, shape[::-1]))
            for m in (mask, one):
                vox = np.flatnonzero(m.ravel())                                   # C index in (X', Y', Z'): the kernel's axis 0 fastest
                rows = gpu_resample(frames, Ak, bk, order, shape[::-1], vox=vox, pad=4)
                assert same_bits(rows, box[m].T), (name, order)                   # the box-mode result gathered at the mask
            vox = np.flatnonzero(mask.ravel())
            perm = np.roll(np.arange(T), 2)[::-1].copy()
            assert not np.array_equal(perm, np.arange(T))
            moved = gpu_resample(frames, Ak, bk, order, shape[::-1], vox=vox, dst=perm, pad=0)
            assert same_bits(moved[perm], box[mask].T), (name, order)
            # d_order: which thread takes which column - the sorted order of the Python layer, a random one, one with holes
            xs, ys, zs = np.unravel_index(vox, shape)
            for walk in (np.argsort((zs * shape[1] + ys) * shape[0] + xs), np.random.RandomState(1).permutation(len(vox))):
                assert same_bits(gpu_resample(frames, Ak, bk, order, shape[::-1], vox=vox, perm=walk), box[mask].T), (name, order)
            holes = np.arange(len(vox))
            holes[[0, -1]] = -1, len(vox)
            part = gpu_resample(frames, Ak, bk, order, shape[::-1], vox=vox, perm=holes)
            assert same_bits(part[:, 1:-1], box[mask].T[:, 1:-1]) and np.all(part[:, [0, -1]] == SENT)
            skipped = gpu_resample(frames[:3], Ak, bk, order, shape[::-1], vox=vox, dst=np.array([1, T + 5, -1]))
            assert same_bits(skipped[1], box[mask].T[0]) and np.all(skipped[[0, 2]] == SENT)     # outside 0 .. T-1: skipped
            wild = gpu_resample(frames[:1], Ak, bk, order, shape[::-1], vox=np.array([vox[0], -1, 10 ** 9, vox[-1]]))
            assert same_bits(wild[0, [0, 3]], box[mask].T[0, [0, -1]]) and np.all(wild[0, 1:3] == SENT)     # outside the box: skipped


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_bits_are_reproducible(gpu, dt):
    import torch
    vol, A, b, shape, kind, M, refs = case('oblique', dt, 5)
    Ak, bk = kernel_args(A, b)
    frames = to_frames(vol)
    target_affine = MASK_AFFINE
    aff = affine_of(A, b, target_affine)
    for order, interp in ((3, 'continuous'), (1, 'linear'), (0, 'nearest')):
        a = gpu_resample(frames, Ak, bk, order, shape[::-1])
        assert same_bits(a, gpu_resample(frames, Ak, bk, order, shape[::-1]))                  # run to run
        assert same_bits(gpu_resample(frames[3:4], Ak, bk, order, shape[::-1]), a[3:4])        # whatever the chunk of frames
        assert same_bits(gpu_resample(frames, Ak, bk, order, shape[::-1], fs_pad=0, pad=0), a)
        c = resample(np.ascontiguousarray(vol), aff, target_affine, shape, interp)             # C order and Fortran order
        f = resample(np.asfortranarray(vol), aff, target_affine, shape, interp)
        assert same_bits(c, f)
        d_c = torch.from_numpy(np.ascontiguousarray(vol)).to('cuda')
        d_f = torch.from_numpy(np.ascontiguousarray(vol.T)).to('cuda').permute(3, 2, 1, 0)
        assert not d_f.is_contiguous()
        assert same_bits(resample(d_c, aff, target_affine, shape, interp).cpu().numpy(), c)
        assert same_bits(resample(d_f, aff, target_affine, shape, interp).cpu().numpy(), c)


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_entry_points_refuse_bad_arguments(gpu, dt):
    import torch
    from modl_amd._lib import lib
    _workspace_refusals(lib)
    V, ld = 20, 23
    host = _host_buffers(dt, V, ld)
    host['ws'][:] = 0xA5
    bufs = {k: torch.from_numpy(v).to('cuda') for k, v in host.items()}
    ptrs = {k: v.data_ptr() for k, v in bufs.items()}
    for name, over, code in _bad_resample_calls(V, ld):
        assert _call_resample(lib, dt, ptrs, V, ld, over) == code, name
    for name, over, code in _bad_prefilter_calls():
        assert _call_prefilter(lib, dt, ptrs, over) == code, name
    torch.cuda.synchronize()
    assert bool((bufs['out'] == SENT).all()) and bool((bufs['coef'] == SENT).all()) and bool((bufs['ws'] == 0xA5).all())
    assert bool((bufs['vol'] == 1).all())
    assert _call_resample(lib, dt, ptrs, V, ld, {}) == 0                          # and the good calls are
    assert _call_resample(lib, dt, ptrs, V, ld, dict(order=1, ws=None, ws_bytes=0, out=ptrs['big'], vox=None, ldo=72)) == 0
    torch.cuda.synchronize()
    out = bufs['out'].cpu().numpy()
    assert np.all(out[:, V:] == SENT) and not np.any(out[:, :V] == SENT)
    assert _call_prefilter(lib, dt, ptrs, {}) == 0
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_python_functions_on_the_device(gpu, dt, monkeypatch):
    import torch
    from modl_amd import masker as mk
    from modl_amd.masker import resample_mask, resample_host, ArrayMasker, _grid_transform
    from .test_masker import restate as smooth_restate, judge as smooth_judge, radii_of
    eps = float(np.finfo(DT[dt]).eps)
    vols, mask, atlas, atlas_affine, kw = _fmri_grids(DT[dt])
    vol = vols[0][..., :7]
    shape = mask.shape
    A, b = _grid_transform(RECORD_AFFINE, MASK_AFFINE)
    M = frame_max(vol)
    perm = np.random.RandomState(0).permutation(vol.shape[3])
    boxes = {}
    for interp, order in ORDERS.items():
        ref = scipy_resample(vol, A, b, shape, order)
        got = resample(vol, RECORD_AFFINE, MASK_AFFINE, shape, interp)
        assert isinstance(got, np.ndarray) and got.dtype == DT[dt] and got.shape == ref.shape
        if order == 0:
            assert same_bits(got, ref.astype(DT[dt]))
        else:
            ok, worst = judge(got, ref, M, order, eps)
            print(dt, interp, '%.3g eps M' % (worst / eps))
            assert ok, worst
        boxes[interp] = got
        d = resample(torch.from_numpy(vol).to('cuda'), RECORD_AFFINE, MASK_AFFINE, shape, interp)
        assert d.is_cuda and tuple(d.shape) == ref.shape and same_bits(d.cpu().numpy(), got)
        assert same_bits(resample(vol[..., 2], RECORD_AFFINE, MASK_AFFINE, shape, interp), got[..., 2:3])
        rows = resample_mask(vol, RECORD_AFFINE, mask, MASK_AFFINE, interp)
        assert isinstance(rows, np.ndarray) and same_bits(rows, got[mask].T)
        d_rows = resample_mask(torch.from_numpy(vol).to('cuda'), RECORD_AFFINE, mask, MASK_AFFINE, interp, dst_row=perm)
        assert d_rows.is_cuda and same_bits(d_rows.cpu().numpy()[perm], rows)
        filled = resample(vol, RECORD_AFFINE, MASK_AFFINE, (11, 10, 9), interp, fill_value=-1.5)
        x = scipy_coordinates(A, b, shape)
        inside = np.all((x >= 0) & (x <= np.array(vol.shape[:3])[:, None] - 1), axis=0).reshape(shape)
        assert np.all(filled[9:] == -1.5) and np.all(filled[:9][~inside] == -1.5)    # x = 1.5 o + 0.25 > 12 from o = 8 on
        assert same_bits(filled[:9][inside], got[inside]) and np.all(got[~inside] == 0)
    # frames in chunks: a workspace bound of two frames gives the same bits, with and without dst_row
    per_frame = mk.lib.modl_resample_workspace(0 if dt == 'f32' else 1, 1, 13, 15, 13, 3)
    monkeypatch.setattr(mk, 'RESAMPLE_WORKSPACE_BYTES', 2 * per_frame + 100)
    assert same_bits(resample(vol, RECORD_AFFINE, MASK_AFFINE, shape), boxes['continuous'])
    assert same_bits(resample_mask(vol, RECORD_AFFINE, mask, MASK_AFFINE, dst_row=perm)[perm], boxes['continuous'][mask].T)
    monkeypatch.undo()
    # the masker: rows mode alone without smoothing; with smoothing, scipy's resampling followed by test_masker's scipy chain
    m = ArrayMasker(mask, mask_affine=MASK_AFFINE).fit()
    assert same_bits(m.transform(vol, affine=RECORD_AFFINE), boxes['continuous'][mask].T)
    assert same_bits(m.mask_volume(vol, dst_row=perm, affine=RECORD_AFFINE)[perm], boxes['continuous'][mask].T)
    fwhm, voxel = 6.0, (3.0, 3.0, 3.0)
    sm = ArrayMasker(mask, smoothing_fwhm=fwhm, mask_affine=MASK_AFFINE).fit()
    got = sm.transform(vol, affine=RECORD_AFFINE)
    d_got = sm.transform(torch.from_numpy(vol).to('cuda'), affine=RECORD_AFFINE)
    assert d_got.is_cuda and same_bits(d_got.cpu().numpy(), got)
    ref_box = scipy_resample(vol, A, b, shape, 3)
    want = scipy_chain(ref_box, fwhm, voxel)[mask].T
    # the smoothing is a contraction, so the resampling error passes through it undamped at most; its own bound is added
    radii = radii_of(fwhm, voxel)
    from .test_masker import bound as smooth_bound
    tol = (bound(3, eps) + smooth_bound(eps, radii) * 27.0) * M[:, None]
    assert np.all(np.abs(got.astype(np.float64) - want) <= tol), float((np.abs(got - want) / M[:, None]).max() / eps)
    assert same_bits(sm.transform(np.asarray(boxes['continuous'][..., :3]), affine=MASK_AFFINE),
                     mk.smooth_mask(boxes['continuous'][..., :3], mask, fwhm, voxel))          # the same grid: today's path
    assert same_bits(sm.mask_maps(atlas, affine=atlas_affine), resample_mask(atlas, atlas_affine, mask, MASK_AFFINE))
    assert same_bits(resample_host(vol, RECORD_AFFINE, MASK_AFFINE, shape, 'nearest'), boxes['nearest'])


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_estimators_resample_records_on_the_device(gpu, dt):
    from modl_amd.fmri import fMRIDictFact, fMRICoder
    _check_resampling_estimators(fMRIDictFact, fMRICoder, DT[dt])
