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

nilearn is not installed where this was written: the steps are judged against scipy (tests/test_masker.py).
Out of scope: computing a mask, resampling, NIfTI reading and writing, fwhm='fast'."""
import numpy as np
import scipy.ndimage
import torch
from sklearn.base import BaseEstimator

from ._lib import lib, check
from .signal import clean

SMOOTH_MAX_RADIUS = lib.modl_smooth_max_radius()           # 8: fwhm 8 mm at 2 mm voxels, 6 mm at 1.5 mm
_FWHM_TO_SIGMA = float(np.sqrt(8.0 * np.log(2.0)))

__all__ = ['smooth_mask', 'unmask', 'gaussian_weights', 'smooth_mask_host', 'unmask_host', 'ArrayMasker']


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
    if tuple(vol.shape[:3]) != maps.mask.shape:
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
    from .device import ptr, stream_ptr
    T, n0, n1, n2 = frames.shape
    V = maps.n_voxels
    sx = 'f32' if frames.dtype == torch.float32 else 'f64'
    (wx, rx), (wy, ry), (wz, rz) = weights
    wx, wy, wz = (np.ascontiguousarray(w, dtype=np.float64) for w in (wx, wy, wz))
    need = lib.modl_smooth_mask_workspace(0 if sx == 'f32' else 1, T, n0, n1, n2, rz, ry, rx)
    if need == 0:
        raise ValueError('modl_smooth_mask: unsupported shape %s, radii %s' % (tuple(frames.shape), (rz, ry, rx)))
    with torch.cuda.device(frames.device):
        d_col, _ = maps.on(frames.device)
        d_dst = None if dst is None else torch.from_numpy(dst).to(frames.device)
        out = torch.empty((T, V), dtype=frames.dtype, device=frames.device)
        ws = torch.empty(need, dtype=torch.uint8, device=frames.device)
        check(getattr(lib, 'modl_smooth_mask_' + sx)(
            ptr(frames), n0 * n1 * n2, T, n0, n1, n2, wz.ctypes.data if rz else None, rz, wy.ctypes.data if ry else None,
            ry, wx.ctypes.data if rx else None, rx, ptr(d_col), V, ptr(d_dst), ptr(out), V, ptr(ws), need,
            stream_ptr(frames.device)), 'modl_smooth_mask')
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
    if lib.modl_device_count() <= 0:
        return _smooth_mask_host(vol, maps, weights, sigmas, dst)
    device = torch.device('cuda', torch.cuda.current_device())
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
    from .device import ptr, stream_ptr
    n, V = rows.shape
    X, Y, Z = maps.mask.shape
    with torch.cuda.device(rows.device):
        _, d_vox = maps.on(rows.device)
        out = torch.empty((n, X, Y, Z), dtype=rows.dtype, device=rows.device)
        check(getattr(lib, 'modl_unmask_' + ('f32' if rows.dtype == torch.float32 else 'f64'))(
            ptr(rows), rows.stride(0), n, V, ptr(d_vox), X, Y, Z, ptr(out), stream_ptr(rows.device)), 'modl_unmask')
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
    if lib.modl_device_count() <= 0:
        return unmask_host(r, maps)
    device = torch.device('cuda', torch.cuda.current_device())
    return _unmask_device(torch.from_numpy(np.ascontiguousarray(r)).to(device), maps).cpu().numpy()


class ArrayMasker(BaseEstimator):
    """The reference's masker on arrays: smooth, mask, clean - and back.

    mask            (X, Y, Z) boolean array
    voxel_size      (vx, vy, vz) in mm, what the affine of an image says
    smoothing_fwhm  None, a number or one per axis, in mm
    standardize, detrend, low_pass, high_pass, t_r    the cleaning of every record (modl_amd.signal.clean)

    fit() builds the column map and the voxel list of the mask and the Gaussian weights once (`n_voxels_`).  transform(volume, confounds=None):
    (T, V), smoothed and masked by one launch, then cleaned.  A 2-D (T, V) input is taken as already masked and is only
    cleaned (the reference's MultiRawMasker contract); with `smoothing_fwhm` set that is a ValueError, since nothing can
    be smoothed any more.  inverse_transform(rows): (X, Y, Z, n)."""

    def __init__(self, mask, voxel_size=(1, 1, 1), smoothing_fwhm=None, standardize=False, detrend=False, low_pass=None,
                 high_pass=None, t_r=None):
        self.mask = mask
        self.voxel_size = voxel_size
        self.smoothing_fwhm = smoothing_fwhm
        self.standardize = standardize
        self.detrend = detrend
        self.low_pass = low_pass
        self.high_pass = high_pass
        self.t_r = t_r

    def fit(self, X=None, y=None):
        self.maps_ = _Maps(self.mask)
        self.sigmas_ = _sigmas(self.smoothing_fwhm, self.voxel_size)         # (the arguments are checked here)
        self.weights_ = _weights(self.smoothing_fwhm, self.voxel_size)       # built once, used by every transform
        self.n_voxels_ = self.maps_.n_voxels
        return self

    def _fitted(self):
        if not hasattr(self, 'maps_'):
            raise ValueError('ArrayMasker is not fitted: call fit() first')
        return self.maps_

    def _smooths(self):
        return any(r > 0 for _, r in self.weights_)

    def mask_volume(self, volume, dst_row=None):
        """the smoothing and masking alone: (T, V); a 2-D input passes as it is"""
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
        return _smooth_mask(volume, maps, self.weights_, self.sigmas_, dst_row)

    def transform(self, volume, confounds=None):
        rows = self.mask_volume(volume)
        if not (self.detrend or self.standardize or confounds is not None or self.low_pass is not None
                or self.high_pass is not None):
            return rows
        return clean(rows, self.detrend, self.standardize, confounds, low_pass=self.low_pass, high_pass=self.high_pass,
                     t_r=self.t_r)

    def inverse_transform(self, rows):
        return unmask(rows, self._fitted())
