"""Spatial smoothing and masking of fMRI volumes on the device, and the way back: the arithmetic of the reference's
masker that precedes `signal.clean` (nilearn's NiftiMasker on array data: `_smooth_array`, then the boolean mask;
`inverse_transform` for the learned maps).  DESIGN.md section 23.

For a volume `vol` (X, Y, Z, T), `voxel_size` (vx, vy, vz) in mm and `smoothing_fwhm` in mm (a scalar or one per axis):

    1. every non-finite element is replaced by 0 (the masker's ensure_finite), smoothing or not;
    2. per spatial axis a, sigma_a = fwhm_a / (sqrt(8 ln 2) v_a); when sigma_a > 0 every frame is correlated along that
       axis with w[j] = exp(-j^2 / (2 sigma_a^2)), j = -r_a .. r_a, r_a = int(4 sigma_a + 0.5), built in f64 and normalised
       to sum 1, boundary 'reflect' of scipy (d c b a | a b c d | d c b a) - scipy.ndimage.gaussian_filter1d, which is
       what nilearn calls.  fwhm_a of 0 or None leaves the axis untouched, bit for bit;
    3. out[t, c] = smoothed[x, y, z, t], c counting the true voxels of `mask` (X, Y, Z) in C order: vol[mask].T;
    4. unmask(rows (n, V), mask) is (X, Y, Z, n): the row's values at the mask's true voxels, exact zeros elsewhere.

The smoothing sees the whole volume, so voxels outside the mask bleed in.  On the device steps 1-3 are ONE launch
(csrc/masker.hip) without an intermediate volume; tiles of the box that hold no masked voxel read nothing.  The kernel
works on frames (T, Z, Y, X) - the bytes of a Fortran-ordered (X, Y, Z, T) array, nibabel's layout, which is handed over
as it is; a C-ordered volume is permuted to that layout on the device first, so both give the same bits.

Resampling (csrc/resample.hip) precedes all of this when a volume lies on another grid than the
mask: `resample`, `resample_mask`, and the `affine` argument of ArrayMasker.  With `affine` the source's 4 x 4 voxel-to-world
matrix and `target_affine` / `target_shape` the target grid, A = inv(affine)[:3, :3] @ target_affine[:3, :3] and
b = inv(affine)[:3, :3] @ target_affine[:3, 3] + inv(affine)[:3, 3] are formed in f64 on the host, the target voxel o reads
the source at x = A o + b, and every frame is scipy.ndimage.affine_transform(frame, A, offset=b, output_shape=target_shape,
order=ORDER, mode='constant', cval=fill_value), ORDER = 3 / 1 / 0 for interpolation = 'continuous' / 'linear' / 'nearest' -
the arithmetic of nilearn's resample_img.  Non-finite source elements count as 0 before anything else: that is this
library's rule (step 1 above), NOT nilearn's, which extrapolates around them.  When A is exactly the identity and b is
exactly integer the result is the shifted crop of the source, bit for bit, whatever the interpolation (nilearn's shortcut).

nilearn is not installed where this was written: the steps are judged against scipy (tests/test_masker.py,
tests/test_resample.py).

Computing the mask (csrc/compute_mask.hip) is the step before all of this when none is given:
`compute_epi_mask`, `compute_background_mask`, their `compute_multi_*` forms over several records and `intersect_masks`,
`largest_connected_component` - the arithmetic of nilearn.masking on arrays, judged against scipy.ndimage (label,
binary_erosion, binary_dilation); `ArrayMasker(mask='epi' | 'background')` and the fMRI estimators call them.  Every
function has a `*_host` twin made of numpy and scipy.
Out of scope: NIfTI reading and writing, fwhm='fast', resampling with `clip` or a non-numeric fill, computing a mask across
grids (resample first), the 'template' strategies."""
import numpy as np
import scipy.ndimage
import torch
from sklearn.base import BaseEstimator

from ._lib import lib
from .device import STREAM, call, current_device, dtype_id, have_gpu, scratch
from .signal import clean

SMOOTH_MAX_RADIUS = lib.modl_smooth_max_radius()           # 8: fwhm 8 mm at 2 mm voxels, 6 mm at 1.5 mm
_FWHM_TO_SIGMA = float(np.sqrt(8.0 * np.log(2.0)))
RESAMPLE_WORKSPACE_BYTES = 1 << 28                          # order 3: frames are resampled in chunks within this workspace
_ORDERS = {'continuous': 3, 'linear': 1, 'nearest': 0}

__all__ = ['smooth_mask', 'unmask', 'gaussian_weights', 'smooth_mask_host', 'unmask_host', 'ArrayMasker', 'resample',
           'resample_mask', 'resample_host', 'voxel_size_of', 'compute_epi_mask', 'compute_background_mask',
           'compute_multi_epi_mask', 'compute_multi_background_mask', 'intersect_masks', 'largest_connected_component',
           'compute_epi_mask_host', 'compute_background_mask_host', 'compute_multi_epi_mask_host',
           'compute_multi_background_mask_host', 'intersect_masks_host', 'largest_connected_component_host']


def gaussian_weights(sigma):
    """(w, r): the 2 r + 1 weights exp(-j^2 / (2 sigma^2)), j = -r .. r, r = int(4 sigma + 0.5), f64, normalised to sum 1 -
    the kernel of scipy.ndimage.gaussian_filter1d(., sigma) with its default truncate = 4.  sigma of 0 or None:
    (array([1.]), 0), nothing to do.  ValueError: a negative or non-finite sigma."""
    if sigma is None:
        return np.ones(1), 0
    sigma = float(sigma)
    if not (sigma >= 0 and np.isfinite(sigma)):
        raise ValueError('sigma must be finite and >= 0, got %r' % sigma)
    r = int(4.0 * sigma + 0.5)
    if sigma == 0 or r == 0:
        return np.ones(1), 0
    j = np.arange(-r, r + 1, dtype=np.float64)
    w = np.exp(-0.5 / (sigma * sigma) * j * j)
    return w / w.sum(), r


def _sigmas(smoothing_fwhm, voxel_size):
    """the three sigmas in voxels (0: axis untouched).  ValueError with the offending value."""
    vs = np.asarray(voxel_size, dtype=np.float64)
    if vs.shape != (3,) or not np.all(np.isfinite(vs)) or not np.all(vs > 0):
        raise ValueError('voxel_size must be three positive numbers, got %r' % (voxel_size,))
    if smoothing_fwhm is None:
        return (0.0, 0.0, 0.0)
    if isinstance(smoothing_fwhm, str):
        raise ValueError("smoothing_fwhm must be a number or one per axis, got %r ('fast' is not implemented)" % smoothing_fwhm)
    fw = smoothing_fwhm if np.ndim(smoothing_fwhm) else [smoothing_fwhm] * 3
    if len(fw) != 3:
        raise ValueError('smoothing_fwhm must be a scalar or one value per axis, got %r' % (smoothing_fwhm,))
    out = []
    for f, v in zip(fw, vs):
        f = 0.0 if f is None else float(f)
        if not (f >= 0 and np.isfinite(f)):
            raise ValueError('smoothing_fwhm must be finite and >= 0, got %r' % (smoothing_fwhm,))
        out.append(f / (_FWHM_TO_SIGMA * v))
    return tuple(out)


def _weights(smoothing_fwhm, voxel_size):
    """[(w, r)] per axis x, y, z.  ValueError: a radius above modl_smooth_max_radius()."""
    sigmas = _sigmas(smoothing_fwhm, voxel_size)
    ws = [gaussian_weights(s) for s in sigmas]
    for (w, r), s in zip(ws, sigmas):
        if r > SMOOTH_MAX_RADIUS:
            raise ValueError('smoothing_fwhm = %r at voxel_size = %r gives a radius of %d voxels (sigma %.3g), at most %d '
                             'are supported' % (smoothing_fwhm, voxel_size, r, s, SMOOTH_MAX_RADIUS))
    return ws


def _check_mask(mask, shape=None):
    if isinstance(mask, torch.Tensor):
        mask = mask.detach().cpu().numpy()
    mask = np.asarray(mask)
    if mask.ndim != 3 or mask.dtype != np.bool_:
        raise ValueError('mask must be a 3-D boolean array, got shape %s, dtype %s' % (mask.shape, mask.dtype))
    if shape is not None and tuple(shape) != mask.shape:
        raise ValueError('the volume has spatial shape %s, the mask %s' % (tuple(shape), mask.shape))
    if not mask.any():
        raise ValueError('the mask of shape %s is empty' % (mask.shape,))
    return mask


class _Maps:
    """What a mask becomes once: `col` (Z, Y, X) int32, the output column of a voxel in the kernel's axis order or -1, and
    `vox` (V,) int64, the flat C index in (X, Y, Z) of every column; device copies are kept per device."""

    def __init__(self, mask):
        self.mask = _check_mask(mask)
        self.n_voxels = int(self.mask.sum())
        col = np.full(self.mask.shape, -1, dtype=np.int32)
        col[self.mask] = np.arange(self.n_voxels, dtype=np.int32)            # C order, z fastest: the order of vol[mask]
        self.col = np.ascontiguousarray(col.transpose(2, 1, 0))
        self.vox = np.flatnonzero(self.mask.ravel()).astype(np.int64)
        self._dev = {}
        self._order = {}

    def order_on(self, device):
        """(V,) int64 on `device`: the columns sorted by their voxel's place in a (Z, Y, X) frame - the order in which the
        resampling kernel walks the mask's loci, so that a wavefront reads neighbouring source elements"""
        key = str(device)
        if key not in self._order:
            x, y, z = np.unravel_index(self.vox, self.mask.shape)
            frame_index = (z * self.mask.shape[1] + y) * self.mask.shape[0] + x
            self._order[key] = torch.from_numpy(np.argsort(frame_index, kind='stable').astype(np.int64)).to(device)
        return self._order[key]

    def on(self, device):
        key = str(device)
        if key not in self._dev:
            self._dev[key] = (torch.from_numpy(self.col).to(device), torch.from_numpy(self.vox).to(device))
        return self._dev[key]


def _maps(mask):
    return mask if isinstance(mask, _Maps) else _Maps(mask)


def _check_volume(volume, maps):
    """the volume as (X, Y, Z, T): a numpy array or a CUDA tensor of float32 / float64"""
    cuda = isinstance(volume, torch.Tensor)
    if cuda and not volume.is_cuda:
        raise ValueError('volume must be a numpy array or a CUDA tensor, got a tensor on %s' % volume.device)
    vol = volume if cuda else np.asarray(volume)
    if vol.ndim == 3:
        vol = vol[..., None]
    if vol.ndim != 4 or vol.shape[3] < 1:
        raise ValueError('volume must be (X, Y, Z, T) or (X, Y, Z), got shape %s' % (tuple(volume.shape),))
    if maps is not None and tuple(vol.shape[:3]) != maps.mask.shape:
        raise ValueError('the volume has spatial shape %s, the mask %s' % (tuple(vol.shape[:3]), maps.mask.shape))
    if cuda:
        if vol.dtype not in (torch.float32, torch.float64):
            vol = vol.to(torch.float64)
    elif vol.dtype not in (np.float32, np.float64):
        vol = vol.astype(np.float64)
    return vol


def _check_dst(dst_row, T):
    if dst_row is None:
        return None
    dst = np.asarray(dst_row)
    if dst.ndim != 1 or dst.shape[0] != T or dst.dtype.kind not in 'iu' or not np.array_equal(np.sort(dst), np.arange(T)):
        raise ValueError('dst_row must be a permutation of 0 .. %d' % (T - 1))
    return np.ascontiguousarray(dst, dtype=np.int64)


def _smooth_mask_device(frames, maps, weights, dst):
    """frames: contiguous CUDA tensor (T, Z, Y, X); weights [(w, r)] for x, y, z; dst int64 numpy or None -> (T, V)"""
    T, n0, n1, n2 = frames.shape
    V = maps.n_voxels
    (wx, rx), (wy, ry), (wz, rz) = weights
    wx, wy, wz = (np.ascontiguousarray(w, dtype=np.float64) for w in (wx, wy, wz))
    need = lib.modl_smooth_mask_workspace(dtype_id(frames), T, n0, n1, n2, rz, ry, rx)
    if need == 0:
        raise ValueError('modl_smooth_mask: unsupported shape %s, radii %s' % (tuple(frames.shape), (rz, ry, rx)))
    d_col, _ = maps.on(frames.device)
    d_dst = None if dst is None else torch.from_numpy(dst).to(frames.device)
    out = torch.empty((T, V), dtype=frames.dtype, device=frames.device)
    ws = scratch(need, frames.device)
    call('modl_smooth_mask', frames, n0 * n1 * n2, T, n0, n1, n2, wz if rz else None, rz, wy if ry else None, ry,
         wx if rx else None, rx, d_col, V, d_dst, out, V, ws, need, STREAM, device=frames.device, dtype=frames)
    return out


def _smooth_mask_host(vol, maps, weights, sigmas, dst):
    arr = np.array(vol, copy=True, order='K')
    arr[~np.isfinite(arr)] = 0
    for axis, ((w, r), s) in enumerate(zip(weights, sigmas)):
        if r > 0:
            scipy.ndimage.gaussian_filter1d(arr, s, axis=axis, output=arr, mode='reflect', truncate=4.0)
    rows = np.ascontiguousarray(arr[maps.mask].T)
    if dst is None:
        return rows
    out = np.empty_like(rows)
    out[dst] = rows
    return out


def smooth_mask_host(volume, mask, smoothing_fwhm=None, voxel_size=(1, 1, 1), dst_row=None):
    """`smooth_mask` with scipy.ndimage.gaussian_filter1d and numpy on the host, same semantics (every axis rounded to the
    volume's dtype, as scipy's in-place chain does): what `smooth_mask` runs without a GPU, and the CPU baseline of
    scripts/bench_smooth.py.  Any radius is accepted."""
    if isinstance(volume, torch.Tensor):
        raise ValueError('smooth_mask_host takes a numpy array')
    maps = _maps(mask)
    vol = _check_volume(volume, maps)
    sigmas = _sigmas(smoothing_fwhm, voxel_size)
    return _smooth_mask_host(vol, maps, [gaussian_weights(s) for s in sigmas], sigmas, _check_dst(dst_row, vol.shape[3]))


def smooth_mask(volume, mask, smoothing_fwhm=None, voxel_size=(1, 1, 1), dst_row=None):
    """Smooth a volume and apply a mask (module docstring), in one launch on the device: (T, V).

    volume          (X, Y, Z, T) as img.get_fdata() gives it, or (X, Y, Z) for one frame; float32 or float64 (anything else
                    is converted to float64): a numpy array (a numpy array comes back) or a CUDA tensor (a CUDA tensor
                    comes back).  A Fortran-ordered volume is used as it is, a C-ordered one is permuted on the device.
    mask            (X, Y, Z) boolean array
    smoothing_fwhm  None, a number, or one per axis (None / 0: axis untouched), in mm
    voxel_size      (vx, vy, vz) in mm
    dst_row         None, or a permutation of 0 .. T-1: frame t is written to row dst_row[t]

    Without a GPU a numpy input goes through `smooth_mask_host`.
    ValueError: a mask that is not 3-D boolean, does not match the volume or is empty, a non-positive voxel size, a negative
    or non-finite fwhm, a radius int(4 sigma + 0.5) above modl_smooth_max_radius() = 8, a dst_row that is no permutation."""
    return _smooth_mask(volume, _maps(mask), _weights(smoothing_fwhm, voxel_size), _sigmas(smoothing_fwhm, voxel_size),
                        dst_row)


def _smooth_mask(volume, maps, weights, sigmas, dst_row):
    """`smooth_mask` with the mask's maps and the weights of `_weights` at hand (an ArrayMasker keeps both)"""
    vol = _check_volume(volume, maps)
    dst = _check_dst(dst_row, vol.shape[3])
    if isinstance(vol, torch.Tensor):
        return _smooth_mask_device(_to_frames(vol), maps, weights, dst)
    if not have_gpu():
        return _smooth_mask_host(vol, maps, weights, sigmas, dst)
    device = current_device()
    if vol.flags.f_contiguous:
        frames = torch.from_numpy(vol.T).to(device)                          # (T, Z, Y, X), the same bytes
    else:
        frames = _to_frames(torch.from_numpy(np.ascontiguousarray(vol)).to(device))
    return _smooth_mask_device(frames, maps, weights, dst).cpu().numpy()


def _to_frames(vol):
    """CUDA tensor (X, Y, Z, T) -> contiguous (T, Z, Y, X): a view for Fortran order, a permuting copy otherwise"""
    return vol.permute(3, 2, 1, 0).contiguous()


def unmask_host(rows, mask):
    """`unmask` in numpy: (X, Y, Z, n) with rows[i] at the mask's true voxels of [..., i] and zeros elsewhere"""
    if isinstance(rows, torch.Tensor):
        raise ValueError('unmask_host takes a numpy array')
    maps = _maps(mask)
    rows = _check_rows(rows, maps)
    out = np.zeros(maps.mask.shape + (rows.shape[0],), dtype=rows.dtype)
    out[maps.mask] = rows.T
    return out


def _check_rows(rows, maps):
    cuda = isinstance(rows, torch.Tensor)
    if cuda and not rows.is_cuda:
        raise ValueError('rows must be a numpy array or a CUDA tensor, got a tensor on %s' % rows.device)
    r = rows if cuda else np.asarray(rows)
    if r.ndim == 1:
        r = r[None, :]
    if r.ndim != 2 or r.shape[0] < 1 or r.shape[1] != maps.n_voxels:
        raise ValueError('rows must be (n, %d), one column per voxel of the mask, got shape %s'
                         % (maps.n_voxels, tuple(rows.shape)))
    if cuda:
        if r.dtype not in (torch.float32, torch.float64):
            r = r.to(torch.float64)
        if not (r.shape[1] == 1 or r.stride(1) == 1):
            r = r.contiguous()
    elif r.dtype not in (np.float32, np.float64):
        r = r.astype(np.float64)
    return r


def _unmask_device(rows, maps):
    n, V = rows.shape
    X, Y, Z = maps.mask.shape
    _, d_vox = maps.on(rows.device)
    out = torch.empty((n, X, Y, Z), dtype=rows.dtype, device=rows.device)
    call('modl_unmask', rows, rows.stride(0), n, V, d_vox, X, Y, Z, out, STREAM, device=rows.device, dtype=rows)
    return out.permute(1, 2, 3, 0)


def unmask(rows, mask):
    """Masked rows back into a volume: rows (n, V) (or (V,) for one) -> (X, Y, Z, n), the row's values at the true voxels
    of `mask` in C order, exact zeros elsewhere; the inverse of the masking of `smooth_mask`.  numpy in, numpy out; CUDA
    tensor in, CUDA tensor out (a view with the frame axis last of a frame-major array).  Without a GPU: `unmask_host`.
    ValueError: a bad mask, rows whose width is not the number of voxels of the mask."""
    maps = _maps(mask)
    r = _check_rows(rows, maps)
    if isinstance(r, torch.Tensor):
        return _unmask_device(r, maps)
    if not have_gpu():
        return unmask_host(r, maps)
    return _unmask_device(torch.from_numpy(np.ascontiguousarray(r)).to(current_device()), maps).cpu().numpy()


def _check_affine(affine, name):
    """the 4 x 4 voxel-to-world matrix as f64.  ValueError naming `name`: a wrong shape, a non-finite entry, a last row
    that is not (0, 0, 0, 1), a singular 3 x 3 part."""
    if isinstance(affine, torch.Tensor):
        affine = affine.detach().cpu().numpy()
    try:
        a = np.asarray(affine, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError('%s must be a 4 x 4 matrix, got %r' % (name, affine))
    if a.shape != (4, 4):
        raise ValueError('%s must be a 4 x 4 matrix, got shape %s' % (name, a.shape))
    if not np.all(np.isfinite(a)):
        raise ValueError('%s has non-finite entries: %r' % (name, a.tolist()))
    if not np.array_equal(a[3], [0.0, 0.0, 0.0, 1.0]):
        raise ValueError('%s must have the last row (0, 0, 0, 1), got %r' % (name, a[3].tolist()))
    if np.linalg.matrix_rank(a[:3, :3]) < 3:
        raise ValueError('%s is singular: %r' % (name, a[:3, :3].tolist()))
    return a


def voxel_size_of(affine):
    """(vx, vy, vz) in mm of a 4 x 4 voxel-to-world matrix: sqrt((affine[:3, :3] ** 2).sum(0)), nilearn's rule"""
    a = _check_affine(affine, 'affine')
    return tuple(float(v) for v in np.sqrt((a[:3, :3] ** 2).sum(axis=0)))


def _grid_transform(affine, target_affine, target_name='target_affine'):
    """(A, b) of the module docstring, f64, in the axis order x, y, z"""
    inv = np.linalg.inv(_check_affine(affine, 'affine'))
    ta = _check_affine(target_affine, target_name)
    return inv[:3, :3] @ ta[:3, :3], inv[:3, :3] @ ta[:3, 3] + inv[:3, 3]


def _check_grid(target_shape, interpolation, fill_value):
    try:
        shape = tuple(int(n) for n in target_shape)
        bad = len(shape) != 3 or any(n < 1 for n in shape) or any(n != m for n, m in zip(shape, target_shape))
    except (TypeError, ValueError):
        bad = True
    if bad:
        raise ValueError('target_shape must be three positive integers, got %r' % (target_shape,))
    if not isinstance(interpolation, str) or interpolation not in _ORDERS:
        raise ValueError("interpolation must be 'continuous', 'linear' or 'nearest', got %r" % (interpolation,))
    if isinstance(fill_value, (str, bytes)) or np.ndim(fill_value) != 0 or not np.isfinite(float(fill_value)):
        raise ValueError('fill_value must be a finite number, got %r' % (fill_value,))
    return shape, _ORDERS[interpolation], float(fill_value)


def _is_shift(A, b):
    return bool(np.array_equal(A, np.eye(3)) and np.array_equal(b, np.floor(b)))


def _resample_host(vol, A, b, shape, order, fill):
    """(X, Y, Z, T) numpy -> (X', Y', Z', T), Fortran-ordered, through scipy: what the kernels are judged against"""
    arr = np.where(np.isfinite(vol), vol, 0).astype(vol.dtype, copy=False)
    if _is_shift(A, b):
        order = 0
    out = np.empty(shape + (vol.shape[3],), dtype=vol.dtype, order='F')
    for t in range(vol.shape[3]):
        out[..., t] = scipy.ndimage.affine_transform(arr[..., t], A, offset=b, output_shape=shape, output=vol.dtype,
                                                     order=order, mode='constant', cval=fill)
    return out


def _rows_host(box, maps, dst):
    rows = np.ascontiguousarray(box[maps.mask].T)
    if dst is None:
        return rows
    out = np.empty_like(rows)
    out[dst] = rows
    return out


def _resample_device(frames, A, b, shape, order, fill, maps=None, dst=None):
    """frames: contiguous CUDA tensor (T, Z, Y, X).  Box mode (maps None): (T, Z', Y', X'); rows mode: (T, V).  At order 3 the
    frames go through in chunks whose workspace stays within RESAMPLE_WORKSPACE_BYTES (one frame at least)."""
    T, n0, n1, n2 = frames.shape
    m0, m1, m2 = shape[2], shape[1], shape[0]
    dt = dtype_id(frames)
    if _is_shift(A, b):
        order = 0
    Ak = np.ascontiguousarray(A[::-1, ::-1], dtype=np.float64)           # P A P and P b: the kernel's axes are z, y, x
    bk = np.ascontiguousarray(b[::-1], dtype=np.float64)
    box = n0 * n1 * n2
    chunk = T
    if order == 3:
        per_frame = lib.modl_resample_workspace(dt, 1, n0, n1, n2, 3)
        if per_frame == 0:
            raise ValueError('modl_resample: unsupported shape %s' % (tuple(frames.shape),))
        chunk = max(1, min(T, RESAMPLE_WORKSPACE_BYTES // per_frame))
    with torch.cuda.device(frames.device):
        if maps is None:
            out = torch.empty((T, m0, m1, m2), dtype=frames.dtype, device=frames.device)
            d_vox, d_order, V, ldo = None, None, 0, m0 * m1 * m2
        else:
            _, d_vox = maps.on(frames.device)
            d_order = maps.order_on(frames.device) if order > 0 else None        # (order 0: one read per store, no gain)
            V = ldo = maps.n_voxels
            out = torch.empty((T, V), dtype=frames.dtype, device=frames.device)
        fold = dst is not None and chunk >= T                            # one call: the kernel permutes the rows itself
        d_dst = None if dst is None else torch.from_numpy(dst).to(frames.device)
        target = out if dst is None or fold else torch.empty_like(out)
        ws = None
        for t0 in range(0, T, chunk):
            n = min(chunk, T - t0)
            need = lib.modl_resample_workspace(dt, n, n0, n1, n2, order)
            if need and (ws is None or ws.numel() < need):
                ws = scratch(need, frames.device)
            call('modl_resample', frames[t0:t0 + n], box, n, n0, n1, n2, Ak, bk, order, fill, m0, m1, m2, d_vox, V, d_order,
                 d_dst if fold else None, target[t0:t0 + n], ldo, ws, need, STREAM, device=frames.device, dtype=frames)
        if target is not out:
            out[d_dst] = target
    return out


def _resample(vol, A, b, shape, order, fill, maps=None, dst=None):
    """vol: what _check_volume returned.  Box mode: (X', Y', Z', T); rows mode (maps given): (T, V)."""
    def finish(res):
        return res if maps is not None else res.permute(3, 2, 1, 0)

    if isinstance(vol, torch.Tensor):
        return finish(_resample_device(_to_frames(vol), A, b, shape, order, fill, maps, dst))
    if not have_gpu():
        res = _resample_host(vol, A, b, shape, order, fill)
        return res if maps is None else _rows_host(res, maps, dst)
    return finish(_resample_device(_to_frames(_upload(vol)), A, b, shape, order, fill, maps, dst)).cpu().numpy()


def _upload(vol):
    """numpy (X, Y, Z, T) -> CUDA tensor of that shape on the current device; a Fortran-ordered volume keeps its bytes (its
    frames (T, Z, Y, X) are then a view)"""
    device = current_device()
    if vol.flags.f_contiguous:
        return torch.from_numpy(vol.T).to(device).permute(3, 2, 1, 0)
    return torch.from_numpy(np.ascontiguousarray(vol)).to(device)


def resample_host(volume, affine, target_affine, target_shape, interpolation='continuous', fill_value=0):
    """`resample` through scipy.ndimage.affine_transform on the host, same semantics (the spline arithmetic in f64, one
    rounding to the volume's dtype): what `resample` runs without a GPU, and the CPU baseline of
    scripts/bench_resample.py.  The result is Fortran-ordered."""
    if isinstance(volume, torch.Tensor):
        raise ValueError('resample_host takes a numpy array')
    shape, order, fill = _check_grid(target_shape, interpolation, fill_value)
    A, b = _grid_transform(affine, target_affine)
    return _resample_host(_check_volume(volume, None), A, b, shape, order, fill)


def resample(volume, affine, target_affine, target_shape, interpolation='continuous', fill_value=0):
    """Resample a volume onto another grid (module docstring) on the device: (X', Y', Z', T).

    volume          (X, Y, Z, T) or (X, Y, Z), float32 or float64 (anything else is converted to float64): a numpy array
                    (a numpy array comes back) or a CUDA tensor (a CUDA tensor comes back, a view with the frame axis last
                    of a frame-major array).  A C-ordered and a Fortran-ordered volume give the same bits.
    affine          4 x 4, voxel to world, of the volume
    target_affine   4 x 4 of the target grid; target_shape its (X', Y', Z')
    interpolation   'continuous' (cubic spline), 'linear' or 'nearest'
    fill_value      what a target voxel outside the source box 0 <= x_a <= n_a - 1 receives

    Non-finite elements of the volume count as 0 - this library's rule, not nilearn's (module docstring).
    'continuous' keeps the spline coefficients of the frames in flight in a workspace of (itemsize + 8) bytes per source
    element: the frames go through in chunks so that it stays within RESAMPLE_WORKSPACE_BYTES = 256 MiB (one frame at
    least).  Without a GPU a numpy input goes through `resample_host`.
    ValueError, naming the offender: an affine that is not 4 x 4, not finite, without the last row (0, 0, 0, 1) or
    singular, a bad target_shape, interpolation or fill_value."""
    shape, order, fill = _check_grid(target_shape, interpolation, fill_value)
    A, b = _grid_transform(affine, target_affine)
    return _resample(_check_volume(volume, None), A, b, shape, order, fill)


def resample_mask(volume, affine, mask, mask_affine, interpolation='continuous', dst_row=None):
    """Resample a volume onto a mask's grid and keep the mask's voxels: (T, V), column c being the c-th true voxel of `mask`
    in C order - `resample(volume, affine, mask_affine, mask.shape, interpolation)[mask].T` to the bit, but the target
    volume is never formed: only the V masked loci are gathered.  `dst_row` as for `smooth_mask`; fill value 0."""
    maps = _maps(mask)
    shape, order, fill = _check_grid(maps.mask.shape, interpolation, 0)
    A, b = _grid_transform(affine, mask_affine, 'mask_affine')
    vol = _check_volume(volume, None)
    return _resample(vol, A, b, shape, order, fill, maps, _check_dst(dst_row, vol.shape[3]))


# ------------------------------------------------------------------------------------------- computing a mask (section 27)
def _check_post(connected, opening):
    if isinstance(opening, (str, bytes)) or np.ndim(opening) != 0 or int(opening) != opening or int(opening) < 0:
        raise ValueError('opening must be False or an integer >= 0, got %r' % (opening,))
    return bool(connected), int(opening)


def _check_cutoffs(lower_cutoff, upper_cutoff):
    lo, up = float(lower_cutoff), float(upper_cutoff)
    if not (0 <= lo <= 1 and 0 <= up <= 1 and lo < up):
        raise ValueError('the cutoffs must satisfy 0 <= lower_cutoff < upper_cutoff <= 1, got lower_cutoff = %r, '
                         'upper_cutoff = %r' % (lower_cutoff, upper_cutoff))
    return lo, up


def _check_border(border_size):
    if isinstance(border_size, (bool, np.bool_)) or not isinstance(border_size, (int, np.integer)) or border_size < 1:
        raise ValueError('border_size must be an integer >= 1, got %r' % (border_size,))
    return int(border_size)


def _check_threshold(threshold):
    t = float(threshold)
    if not 0 <= t <= 1:
        raise ValueError('threshold must lie in [0, 1], got %r' % (threshold,))
    return t


def _cut_indices(lo, up, n):
    a, b = int(np.floor(lo * n)), min(int(np.floor(up * n)), n - 1)
    if b <= a:
        raise ValueError('lower_cutoff = %r and upper_cutoff = %r leave no interval among n = %d sorted values'
                         % (lo, up, n))
    return a, b


def _warn_empty(empty, what):
    if empty:
        import warnings
        warnings.warn('%s computed an empty mask' % what, UserWarning, stacklevel=3)


def _bool_mask_host(mask, name='mask'):
    if isinstance(mask, torch.Tensor):
        raise ValueError('the *_host functions take numpy arrays')
    mask = np.asarray(mask)
    if mask.ndim != 3 or mask.dtype != np.bool_:
        raise ValueError('%s must be a 3-D boolean array, got shape %s, dtype %s' % (name, mask.shape, mask.dtype))
    return mask


def largest_connected_component_host(mask):
    """`largest_connected_component` through scipy.ndimage.label: 6-connectivity, the component with the most voxels, ties
    to the one whose first voxel comes first in C order.  ValueError: no true voxel."""
    mask = _bool_mask_host(mask)
    labels, n = scipy.ndimage.label(mask)
    if n == 0:
        raise ValueError('the mask of shape %s has no true voxel: there is no connected component' % (mask.shape,))
    if n == 1:
        return mask.copy()
    return labels == np.bincount(labels.ravel())[1:].argmax() + 1


def _post_host(mask, opening, connected):
    if opening:
        mask = scipy.ndimage.binary_erosion(mask, iterations=opening)
    if connected and mask.any():
        mask = largest_connected_component_host(mask)
    if opening:
        mask = scipy.ndimage.binary_dilation(mask, iterations=2 * opening)
        mask = scipy.ndimage.binary_erosion(mask, iterations=opening)
    return mask


def _mean_host(vol):
    """contract item 1 on (X, Y, Z, T): the f64 sum over t, the f64 division, one rounding to the dtype"""
    return (vol.sum(axis=3, dtype=np.float64) / vol.shape[3]).astype(vol.dtype)


def _host_volume(volume):
    if isinstance(volume, torch.Tensor):
        raise ValueError('the *_host functions take numpy arrays')
    return _check_volume(volume, None)


def _epi_host(vol, lo, up, connected, opening, exclude_zeros):
    mean = _mean_host(vol)
    mean[~np.isfinite(mean)] = 0
    s = np.sort(mean.ravel())
    if exclude_zeros:
        s = s[s != 0]
    a, b = _cut_indices(lo, up, len(s))
    ia = int(np.argmax(s[a + 1:b + 1] - s[a:b]))
    threshold = mean.dtype.type(0.5) * (s[ia + a] + s[ia + a + 1])
    return _post_host(mean >= threshold, opening, connected)


def _border_host(d, b):
    return np.concatenate([x.ravel() for x in (d[:b], d[-b:], d[:, :b], d[:, -b:], d[:, :, :b], d[:, :, -b:])])


def _background_host(vol, border_size, connected, opening):
    mean = _mean_host(vol)
    border = _border_host(mean, border_size)
    if np.isnan(border).any():
        mask = ~np.isnan(mean)
    else:
        mask = mean != np.median(border)
    return _post_host(mask, opening, connected)


def compute_epi_mask_host(volume, lower_cutoff=0.2, upper_cutoff=0.85, connected=True, opening=2, exclude_zeros=False):
    """`compute_epi_mask` composed of numpy and scipy.ndimage: what runs without a GPU, the judge of the kernels and the CPU
    baseline of scripts/bench_mask.py"""
    lo, up = _check_cutoffs(lower_cutoff, upper_cutoff)
    connected, opening = _check_post(connected, opening)
    mask = _epi_host(_host_volume(volume), lo, up, connected, opening, bool(exclude_zeros))
    _warn_empty(not mask.any(), 'compute_epi_mask')
    return mask


def compute_background_mask_host(volume, border_size=2, connected=False, opening=False):
    """`compute_background_mask` composed of numpy and scipy.ndimage (see compute_epi_mask_host)"""
    border_size = _check_border(border_size)
    connected, opening = _check_post(connected, opening)
    mask = _background_host(_host_volume(volume), border_size, connected, opening)
    _warn_empty(not mask.any(), 'compute_background_mask')
    return mask


def _check_masks(masks, name='masks'):
    if isinstance(masks, (np.ndarray, torch.Tensor)) or masks is None:
        raise ValueError('%s must be a list of (X, Y, Z) boolean arrays, got %s' % (name, type(masks).__name__))
    masks = list(masks)
    if not masks:
        raise ValueError('%s is an empty list' % name)
    return masks


def _intersect_count(threshold, n):
    return min(threshold, 1 - 1e-7) * n


def intersect_masks_host(masks, threshold=0.5, connected=True):
    """`intersect_masks` in numpy (the largest component through scipy)"""
    threshold = _check_threshold(threshold)
    masks = [_bool_mask_host(m, 'masks[%d]' % i) for i, m in enumerate(_check_masks(masks))]
    count = np.zeros(masks[0].shape, dtype=np.int64)
    for i, m in enumerate(masks):
        if m.shape != masks[0].shape:
            raise ValueError('masks[%d] has shape %s, masks[0] %s' % (i, m.shape, masks[0].shape))
        count += m
    keep = count > _intersect_count(threshold, len(masks))
    if connected and keep.any():
        keep = largest_connected_component_host(keep)
    return keep


def _check_volumes(volumes):
    if isinstance(volumes, (np.ndarray, torch.Tensor)):
        return [volumes]
    if volumes is None or isinstance(volumes, (str, bytes)):
        raise ValueError('volumes must be a list of (X, Y, Z, T) arrays, got %r' % (volumes,))
    return volumes


def _multi_host(volumes, single, threshold, connected, what):
    masks, shape = [], None
    for i, v in enumerate(_check_volumes(volumes)):
        vol = _host_volume(v)
        if shape is not None and vol.shape[:3] != shape:
            raise ValueError('volumes[%d] has spatial shape %s, volumes[0] %s' % (i, vol.shape[:3], shape))
        shape = vol.shape[:3]
        masks.append(single(vol))
    if not masks:
        raise ValueError('volumes is an empty list')
    mask = intersect_masks_host(masks, threshold, connected)
    _warn_empty(not mask.any(), what)
    return mask


def compute_multi_epi_mask_host(volumes, lower_cutoff=0.2, upper_cutoff=0.85, connected=True, opening=2, threshold=0.5,
                                exclude_zeros=False):
    """`compute_multi_epi_mask` on the host: compute_epi_mask_host of every volume, then intersect_masks_host"""
    lo, up = _check_cutoffs(lower_cutoff, upper_cutoff)
    connected, opening = _check_post(connected, opening)
    threshold = _check_threshold(threshold)
    return _multi_host(volumes, lambda v: _epi_host(v, lo, up, connected, opening, bool(exclude_zeros)), threshold, connected,
                       'compute_multi_epi_mask')


def compute_multi_background_mask_host(volumes, border_size=2, connected=True, opening=2, threshold=0.5):
    """`compute_multi_background_mask` on the host"""
    border_size = _check_border(border_size)
    connected, opening = _check_post(connected, opening)
    threshold = _check_threshold(threshold)
    return _multi_host(volumes, lambda v: _background_host(v, border_size, connected, opening), threshold, connected,
                       'compute_multi_background_mask')


# ---- the device: masks are uint8 tensors (Z, Y, X), the kernels' frame order
def _frame_mean_device(frames, zero_nonfinite):
    """frames: contiguous CUDA tensor (T, Z, Y, X) -> (Z, Y, X), contract item 1 (csrc/compute_mask.hip)"""
    T, n0, n1, n2 = frames.shape
    box = n0 * n1 * n2
    mean = torch.empty((n0, n1, n2), dtype=frames.dtype, device=frames.device)
    call('modl_frame_mean', frames, box, T, box, int(bool(zero_nonfinite)), mean, STREAM, device=frames.device, dtype=frames)
    return mean


def _morph_device(m, iterations, dilate):
    n0, n1, n2 = m.shape
    need = lib.modl_morph_workspace(n0, n1, n2, iterations)
    if need == 0:
        raise ValueError('modl_binary_morph: unsupported box %s, iterations %r' % (tuple(m.shape), iterations))
    out, ws = torch.empty_like(m), scratch(need, m.device)
    call('modl_binary_morph', m, n0, n1, n2, iterations, int(dilate), out, ws, need, STREAM, device=m.device)
    return out


def _largest_device(m):
    """(the largest component (Z, Y, X) uint8, [components, size, first voxel]) - the three numbers come to the host"""
    n0, n1, n2 = m.shape
    need = lib.modl_label_workspace(n0, n1, n2)
    if need == 0:
        raise ValueError('modl_largest_component: unsupported box %s' % (tuple(m.shape),))
    out, ws = torch.empty_like(m), scratch(need, m.device)
    info = torch.empty(3, dtype=torch.int64, device=m.device)
    call('modl_largest_component', m, n0, n1, n2, out, info, ws, need, STREAM, device=m.device)
    return out, info.cpu().tolist()


def _post_device(m, opening, connected):
    if opening:
        m = _morph_device(m, opening, False)
    if connected:
        out, info = _largest_device(m)                                       # (no true voxel: the empty mask stays)
        if info[0] > 1:
            m = out
    if opening:
        m = _morph_device(_morph_device(m, 2 * opening, True), opening, False)
    return m


def _epi_device(frames, lo, up, connected, opening, exclude_zeros):
    mean = _frame_mean_device(frames, True)
    s = torch.sort(mean.reshape(-1)).values
    if exclude_zeros:
        s = s[s != 0]
    a, b = _cut_indices(lo, up, int(s.shape[0]))
    delta = s[a + 1:b + 1] - s[a:b]
    ia = int((delta == delta.max()).nonzero()[0, 0])                         # the FIRST argmax
    pair = s[ia + a:ia + a + 2].cpu().numpy()
    threshold = pair.dtype.type(0.5) * (pair[0] + pair[1])                   # numpy arithmetic in the dtype
    return _post_device((mean >= threshold.item()).to(torch.uint8), opening, connected)


def _background_device(frames, border_size, connected, opening):
    mean = _frame_mean_device(frames, False)
    d, b = mean.permute(2, 1, 0), border_size
    border = torch.cat([x.reshape(-1) for x in (d[:b], d[-b:], d[:, :b], d[:, -b:], d[:, :, :b], d[:, :, -b:])])
    if bool(torch.isnan(border).any()):
        mask = ~torch.isnan(mean)
    else:
        s = torch.sort(border).values
        h = s.shape[0] // 2
        pair = s[h - 1:h + 1].cpu().numpy()
        with np.errstate(all='ignore'):
            median = pair.dtype.type(0.5) * (pair[0] + pair[1])              # np.median: the mean of the two middle values
        mask = mean != median.item()
    return _post_device(mask.to(torch.uint8), opening, connected)


def _device_frames(volume):
    """(frames (T, Z, Y, X) on the device, was the input a CUDA tensor) or (the checked numpy volume, None) without a GPU"""
    vol = _check_volume(volume, None)
    if isinstance(vol, torch.Tensor):
        return _to_frames(vol), True
    if not have_gpu():
        return vol, None
    return _to_frames(_upload(vol)), False


def _mask_out(m, cuda):
    """a device mask (Z, Y, X) uint8 as the caller's (X, Y, Z) boolean: a CUDA view, or a numpy array"""
    out = m.to(torch.bool).permute(2, 1, 0)
    return out if cuda else np.ascontiguousarray(out.cpu().numpy())


def _mask_in(mask, name='mask'):
    """an (X, Y, Z) boolean numpy array or CUDA tensor as (uint8 (Z, Y, X) on the device, was it a CUDA tensor)"""
    cuda = isinstance(mask, torch.Tensor)
    if cuda and not mask.is_cuda:
        raise ValueError('%s must be a numpy array or a CUDA tensor, got a tensor on %s' % (name, mask.device))
    if not cuda:
        mask = np.asarray(mask)
    if mask.ndim != 3 or mask.dtype not in (np.bool_, torch.bool):
        raise ValueError('%s must be a 3-D boolean array, got shape %s, dtype %s' % (name, tuple(mask.shape), mask.dtype))
    if not cuda:
        mask = torch.from_numpy(np.ascontiguousarray(mask)).to(current_device())
    return mask.permute(2, 1, 0).contiguous().to(torch.uint8), cuda


def largest_connected_component(mask):
    """The largest 6-connected component of an (X, Y, Z) boolean mask (scipy.ndimage.label's default structure); among
    components of equal size the one whose first voxel comes first in C order.  numpy in, numpy out; a CUDA tensor in, a
    CUDA tensor out.  On the device: union-find labelling, csrc/compute_mask.hip.  Without a GPU:
    `largest_connected_component_host`.  ValueError: a mask that is not 3-D boolean or has no true voxel."""
    if not isinstance(mask, torch.Tensor) and not have_gpu():
        return largest_connected_component_host(mask)
    m, cuda = _mask_in(mask)
    out, info = _largest_device(m)
    if info[0] == 0:
        raise ValueError('the mask of shape %s has no true voxel: there is no connected component' % (tuple(mask.shape),))
    return _mask_out(out, cuda)


def compute_epi_mask(volume, lower_cutoff=0.2, upper_cutoff=0.85, connected=True, opening=2, exclude_zeros=False):
    """The brain mask of an EPI record, nilearn's compute_epi_mask on an array: (X, Y, Z) boolean.

    The mean over t (f64 sum, rounded once to the dtype), non-finite elements of it set to 0; s = its sorted values (without
    the zeros if `exclude_zeros`), n = len(s), lo = floor(lower_cutoff n), hi = min(floor(upper_cutoff n), n - 1), ia = the
    first argmax of s[lo+1:hi+1] - s[lo:hi], threshold = (s[ia+lo] + s[ia+lo+1]) / 2 in the dtype; mean >= threshold, then
    the post-processing: erosion by `opening` (cross structure, border 0), the largest 6-connected component if `connected`
    and the mask is not empty, dilation by 2 `opening` and erosion by `opening`.
    volume: (X, Y, Z, T) or (X, Y, Z), float32 / float64 (anything else is converted to float64), numpy (numpy comes back) or
    a CUDA tensor (a CUDA tensor comes back, a permuted view); C and Fortran order give the same bits.  The mean, the
    morphology and the labelling are kernels of csrc/compute_mask.hip; the sort runs on the device, two values of it come to
    the host.  Without a GPU a numpy input goes through `compute_epi_mask_host`.
    ValueError naming the offender: cutoffs outside [0, 1] or lower >= upper, hi <= lo, a negative opening.  An empty result
    comes back with a UserWarning."""
    lo, up = _check_cutoffs(lower_cutoff, upper_cutoff)
    connected, opening = _check_post(connected, opening)
    frames, cuda = _device_frames(volume)
    if cuda is None:
        mask = _epi_host(frames, lo, up, connected, opening, bool(exclude_zeros))
        _warn_empty(not mask.any(), 'compute_epi_mask')
        return mask
    m = _epi_device(frames, lo, up, connected, opening, bool(exclude_zeros))
    _warn_empty(not bool(m.any()), 'compute_epi_mask')
    return _mask_out(m, cuda)


def compute_background_mask(volume, border_size=2, connected=False, opening=False):
    """The mask of a record whose background is constant (or NaN), nilearn's compute_background_mask on an array.

    The mean over t; border = the `border_size` outermost planes of every face, as numpy slices them (edges and corners
    count more than once); if it holds a NaN the mask is ~isnan(mean), otherwise mean != np.median(border); then the
    post-processing of `compute_epi_mask`.  Input, output and dispatch as there.
    ValueError: border_size that is not an integer >= 1, a negative opening."""
    border_size = _check_border(border_size)
    connected, opening = _check_post(connected, opening)
    frames, cuda = _device_frames(volume)
    if cuda is None:
        mask = _background_host(frames, border_size, connected, opening)
        _warn_empty(not mask.any(), 'compute_background_mask')
        return mask
    m = _background_device(frames, border_size, connected, opening)
    _warn_empty(not bool(m.any()), 'compute_background_mask')
    return _mask_out(m, cuda)


def _intersect_device(masks, threshold, connected):
    """masks: an iterable of uint8 (Z, Y, X) device tensors; the running count stays on the device"""
    count, n = None, 0
    for i, m in enumerate(masks):
        if count is None:
            count = torch.zeros(m.shape, dtype=torch.int32, device=m.device)
        elif m.shape != count.shape:
            raise ValueError('masks[%d] has shape %s, masks[0] %s' % (i, tuple(m.shape)[::-1], tuple(count.shape)[::-1]))
        count += m != 0
        n += 1
    if count is None:
        raise ValueError('masks is an empty list')
    keep = (count.to(torch.float64) > _intersect_count(threshold, n)).to(torch.uint8)
    if connected:
        out, info = _largest_device(keep)
        if info[0] > 1:
            keep = out
    return keep


def intersect_masks(masks, threshold=0.5, connected=True):
    """The voxels that are true in more than min(threshold, 1 - 1e-7) len(masks) of the (X, Y, Z) boolean `masks` (threshold 0:
    the union, 1: the intersection), then the largest component if `connected` and any voxel is kept - nilearn's
    intersect_masks.  A CUDA tensor comes back if any mask is one.  Without a GPU: `intersect_masks_host`.
    ValueError: a threshold outside [0, 1], an empty list, shapes that differ."""
    threshold = _check_threshold(threshold)
    masks = _check_masks(masks)
    if not have_gpu() and not any(isinstance(m, torch.Tensor) for m in masks):
        return intersect_masks_host(masks, threshold, connected)
    pairs = [_mask_in(m, 'masks[%d]' % i) for i, m in enumerate(masks)]
    return _mask_out(_intersect_device([m for m, _ in pairs], threshold, connected), any(c for _, c in pairs))


def _multi(volumes, single_device, single_host, threshold, connected, what):
    state = {'cuda': False, 'shape': None}

    def masks():
        for i, v in enumerate(_check_volumes(volumes)):
            frames, cuda = _device_frames(v)
            shape = tuple(frames.shape[:3]) if cuda is None else tuple(frames.shape[1:])[::-1]
            if state['shape'] is not None and shape != state['shape']:
                raise ValueError('volumes[%d] has spatial shape %s, volumes[0] %s' % (i, shape, state['shape']))
            state['shape'] = shape
            state['cuda'] = state['cuda'] or bool(cuda)
            yield single_host(frames) if cuda is None else single_device(frames)

    if not have_gpu():
        found = list(masks())
        if not found:
            raise ValueError('volumes is an empty list')
        mask = intersect_masks_host(found, threshold, connected)
        _warn_empty(not mask.any(), what)
        return mask
    try:
        m = _intersect_device(masks(), threshold, connected)
    except ValueError as e:
        if str(e) == 'masks is an empty list':
            raise ValueError('volumes is an empty list')
        raise
    _warn_empty(not bool(m.any()), what)
    return _mask_out(m, state['cuda'])


def compute_multi_epi_mask(volumes, lower_cutoff=0.2, upper_cutoff=0.85, connected=True, opening=2, threshold=0.5,
                           exclude_zeros=False):
    """`compute_epi_mask` of every volume of a list (or any iterable: they are taken one at a time) with these arguments, then
    `intersect_masks(those, threshold, connected)`; the running count stays on the device.  All volumes must have one
    spatial shape.  A CUDA tensor comes back if any volume is one.  ValueError: as `compute_epi_mask` and `intersect_masks`,
    an empty list, shapes that differ."""
    lo, up = _check_cutoffs(lower_cutoff, upper_cutoff)
    connected, opening = _check_post(connected, opening)
    threshold = _check_threshold(threshold)
    ez = bool(exclude_zeros)
    return _multi(volumes, lambda f: _epi_device(f, lo, up, connected, opening, ez),
                  lambda v: _epi_host(v, lo, up, connected, opening, ez), threshold, connected, 'compute_multi_epi_mask')


def compute_multi_background_mask(volumes, border_size=2, connected=True, opening=2, threshold=0.5):
    """`compute_background_mask` of every volume with these arguments, then `intersect_masks(those, threshold, connected)`;
    see `compute_multi_epi_mask`."""
    border_size = _check_border(border_size)
    connected, opening = _check_post(connected, opening)
    threshold = _check_threshold(threshold)
    return _multi(volumes, lambda f: _background_device(f, border_size, connected, opening),
                  lambda v: _background_host(v, border_size, connected, opening), threshold, connected,
                  'compute_multi_background_mask')


MASK_STRATEGIES = {'epi': compute_multi_epi_mask, 'background': compute_multi_background_mask}


def _check_strategy(mask, mask_args):
    if mask not in MASK_STRATEGIES:
        raise ValueError("mask must be a boolean array, 'background' or 'epi', got %r" % (mask,))
    if mask_args is not None and not isinstance(mask_args, dict):
        raise ValueError('mask_args must be None or a dict of arguments of compute_multi_%s_mask, got %r' % (mask, mask_args))
    return MASK_STRATEGIES[mask], dict(mask_args or {})


def _check_same_grid(affine, mask_affine, what):
    """while a mask is computed every volume lies on one grid: an affine that says otherwise is refused"""
    if affine is None:
        return
    a = _check_affine(affine, 'affine')
    if mask_affine is None or not np.allclose(a, _check_affine(mask_affine, 'mask_affine')):
        raise ValueError('%s has affine %r, which is not mask_affine = %r: a mask is computed on one grid - resample first '
                         '(modl_amd.masker.resample)' % (what, a.tolist(),
                                                         None if mask_affine is None else np.asarray(mask_affine).tolist()))


def compute_strategy_mask(mask, mask_args, volumes, affines=None, mask_affine=None):
    """the mask of the strategy `mask` ('background' / 'epi') over `volumes` (an iterable), as a numpy (X, Y, Z) boolean array"""
    fn, args = _check_strategy(mask, mask_args)
    if affines is not None:
        for i, a in enumerate(affines):
            _check_same_grid(a, mask_affine, 'volume %d' % i)
    found = fn(volumes, **args)
    return found.cpu().numpy() if isinstance(found, torch.Tensor) else found


class ArrayMasker(BaseEstimator):
    """The reference's masker on arrays: smooth, mask, clean - and back.

    mask            (X, Y, Z) boolean array, or the strategy 'background' / 'epi': `fit(volumes)` then computes the mask from one
                    volume or a list with compute_multi_background_mask / compute_multi_epi_mask (module docstring, section
                    27) and `mask_args` (None or a dict of their arguments).  `mask_` is the boolean array either way.
                    `fit()` without volumes is then a ValueError, and so is an `affine` of `fit` that is not allclose to
                    `mask_affine`: a mask is computed on one grid, resample first.
    voxel_size      (vx, vy, vz) in mm, what the affine of an image says
    smoothing_fwhm  None, a number or one per axis, in mm
    standardize, detrend, low_pass, high_pass, t_r    the cleaning of every record (modl_amd.signal.clean)

    fit() builds the column map and the voxel list of the mask and the Gaussian weights once (`n_voxels_`).  transform(volume, confounds=None):
    (T, V), smoothed and masked by one launch, then cleaned.  A 2-D (T, V) input is taken as already masked and is only
    cleaned (the reference's MultiRawMasker contract); with `smoothing_fwhm` set that is a ValueError, since nothing can
    be smoothed any more.  inverse_transform(rows): (X, Y, Z, n).

    mask_affine     None, or the mask's 4 x 4 voxel-to-world matrix.  With it, `transform` and `mask_volume` take the
                    `affine` of the volume: when that is allclose to `mask_affine` and the volume has the mask's shape the
                    volume is on the mask's grid and takes the path above, bit for bit; otherwise it is resampled onto the
                    mask's grid first ('continuous', fill 0; module docstring) - into the mask's box and then smoothed when
                    there is smoothing, straight into the (T, V) rows (no target volume) when there is none.  With
                    `voxel_size` left at (1, 1, 1) or None the voxel size is `voxel_size_of(mask_affine)` (`voxel_size_`).
                    An `affine` without `mask_affine`, or a singular one, is a ValueError."""

    def __init__(self, mask, voxel_size=(1, 1, 1), smoothing_fwhm=None, standardize=False, detrend=False, low_pass=None,
                 high_pass=None, t_r=None, mask_affine=None, mask_args=None):
        self.mask = mask
        self.mask_args = mask_args
        self.mask_affine = mask_affine
        self.voxel_size = voxel_size
        self.smoothing_fwhm = smoothing_fwhm
        self.standardize = standardize
        self.detrend = detrend
        self.low_pass = low_pass
        self.high_pass = high_pass
        self.t_r = t_r

    def fit(self, X=None, y=None, affine=None):
        if isinstance(self.mask, str):
            _check_strategy(self.mask, self.mask_args)
            if X is None:
                raise ValueError('mask = %r is computed from volumes: call fit(volumes)' % self.mask)
            volumes = _check_volumes(X)
            affines = None if affine is None else ([affine] * len(volumes) if np.ndim(affine) == 2 else list(affine))
            self.mask_ = compute_strategy_mask(self.mask, self.mask_args, volumes, affines, self.mask_affine)
        else:
            if self.mask_args is not None:
                raise ValueError('mask_args = %r goes with mask = \'background\' or \'epi\', not with an array' % (self.mask_args,))
            self.mask_ = self.mask
        self.maps_ = _Maps(self.mask_)
        self.mask_affine_ = None if self.mask_affine is None else _check_affine(self.mask_affine, 'mask_affine')
        voxel_size = (1, 1, 1) if self.voxel_size is None else self.voxel_size
        if self.mask_affine_ is not None and np.array_equal(np.asarray(voxel_size, dtype=object), (1, 1, 1)):
            voxel_size = voxel_size_of(self.mask_affine_)                    # (left at its default: the affine says it)
        self.voxel_size_ = voxel_size
        self.sigmas_ = _sigmas(self.smoothing_fwhm, voxel_size)              # (the arguments are checked here)
        self.weights_ = _weights(self.smoothing_fwhm, voxel_size)            # built once, used by every transform
        self.n_voxels_ = self.maps_.n_voxels
        return self

    def _other_grid(self, volume, affine):
        """None when the volume lies on the mask's grid, else (A, b) of the resampling onto it"""
        if affine is None:
            return None
        if self.mask_affine_ is None:
            raise ValueError('affine = %r was given, but the masker has no mask_affine to resample onto'
                             % (np.asarray(affine).tolist(),))
        a = _check_affine(affine, 'affine')
        if tuple(volume.shape[:3]) == self.maps_.mask.shape and np.allclose(a, self.mask_affine_):
            return None
        return _grid_transform(a, self.mask_affine_, 'mask_affine')

    def mask_maps(self, volume, affine=None):
        """maps given as a volume (X, Y, Z, k), e.g. an atlas: masked, NEVER smoothed: (k, V).  On another grid (`affine`)
        they are resampled ('continuous') straight into the rows."""
        maps = self._fitted()
        if not isinstance(volume, torch.Tensor):
            volume = np.asarray(volume)
        grid = self._other_grid(volume, affine) if volume.ndim in (3, 4) else None
        if grid is None:
            return _smooth_mask(volume, maps, [(np.ones(1), 0)] * 3, (0.0, 0.0, 0.0), None)
        return _resample(_check_volume(volume, None), grid[0], grid[1], maps.mask.shape, 3, 0.0, maps, None)

    def _fitted(self):
        if not hasattr(self, 'maps_'):
            raise ValueError('ArrayMasker is not fitted: call fit() first')
        return self.maps_

    def _smooths(self):
        return any(r > 0 for _, r in self.weights_)

    def mask_volume(self, volume, dst_row=None, affine=None):
        """the (resampling,) smoothing and masking alone: (T, V); a 2-D input passes as it is"""
        maps = self._fitted()
        if not isinstance(volume, torch.Tensor):
            volume = np.asarray(volume)
        if volume.ndim == 2:
            if self._smooths():
                raise ValueError('a 2-D record of shape %s is already masked and cannot be smoothed (smoothing_fwhm = %r)'
                                 % (tuple(volume.shape), self.smoothing_fwhm))
            if volume.shape[1] != maps.n_voxels:
                raise ValueError('the record has %d voxels, the mask %d' % (volume.shape[1], maps.n_voxels))
            if dst_row is None:
                return volume
            inv = np.empty(len(dst_row), dtype=np.int64)
            inv[np.asarray(dst_row)] = np.arange(len(dst_row))
            return volume[torch.from_numpy(inv).to(volume.device) if isinstance(volume, torch.Tensor) else inv]
        grid = self._other_grid(volume, affine) if volume.ndim in (3, 4) else None
        if grid is None:
            return _smooth_mask(volume, maps, self.weights_, self.sigmas_, dst_row)
        vol = _check_volume(volume, None)
        if self._smooths():                                                  # into the mask's box, then the launch of before
            if not isinstance(vol, torch.Tensor) and have_gpu():
                return self.mask_volume(_upload(vol), dst_row, affine).cpu().numpy()     # (one upload for both steps)
            return _smooth_mask(_resample(vol, grid[0], grid[1], maps.mask.shape, 3, 0.0), maps, self.weights_, self.sigmas_,
                                dst_row)
        return _resample(vol, grid[0], grid[1], maps.mask.shape, 3, 0.0, maps, _check_dst(dst_row, vol.shape[3]))

    def transform(self, volume, confounds=None, affine=None):
        rows = self.mask_volume(volume, affine=affine)
        if not (self.detrend or self.standardize or confounds is not None or self.low_pass is not None
                or self.high_pass is not None):
            return rows
        return clean(rows, self.detrend, self.standardize, confounds, low_pass=self.low_pass, high_pass=self.high_pass,
                     t_r=self.t_r)

    def inverse_transform(self, rows):
        return unmask(rows, self._fitted())
