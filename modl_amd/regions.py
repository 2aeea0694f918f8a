"""Connected regions of learned maps on the device: the arithmetic of nilearn.regions.connected_regions / RegionExtractor
(extractor='connected_components') on masked rows.  DESIGN.md section 28, csrc/regions.hip.

`components` is (k, V), float32 or float64, a numpy array or a CUDA tensor (which may be non-contiguous); `mask` is (X, Y, Z)
boolean with V true voxels; column c is the c-th true voxel in C order, the order of vol[mask], `unmask` and the masker.

    1. every non-finite element counts as 0 (the rule of `resample`);
    2. the cutoff c >= 0 is a scalar applied to |v|: an element is foreground iff it is finite, v != 0 and |v| >= c, compared
       in the dtype of the components.  thresholding_strategy None: c = 0; 'value': c = threshold; 'ratio_n_voxels' with
       threshold = r, 0 < r <= k: n_keep = min(k V, max(1, floor(r V + 0.5))) and c is the n_keep-th largest |v| over all k V
       elements - an order statistic, not interpolated; ties at c are all kept;
    3. the foreground of ONE map is split into its 6-connected components in the (X, Y, Z) box: scipy.ndimage.label with the
       default structure.  Columns that are neighbours in the row but not in the box are not connected; maps never interact;
    4. a component of n voxels is kept iff n > min_region_size / voxel_volume, a strict float64 compare, with voxel_volume =
       prod(voxel_size), or |det(mask_affine[:3, :3])| when an affine is given;
    5. regions are ordered by map, within a map by scipy's label number: ascending position of the component's first voxel
       in the C order of the (X, Y, Z) array;
    6. `regions` (R, V) in the dtype of the components: row r holds the elements of map index[r] on the voxels of its
       component, bit for bit with their sign, and 0 elsewhere; `index` (R,) int64; `sizes` (R,) int64 in voxels.  R == 0:
       empty arrays and a UserWarning.

Where this differs from nilearn (which is not installed where this was written: scipy.ndimage and the text above are the
yardstick): nilearn's 'ratio_n_voxels' takes an INTERPOLATED percentile (scipy.stats.scoreatpercentile) of |v| over the
whole box, zeros outside the mask included, and keeps |v| > that value; here the cutoff is an order statistic over the
mask's voxels alone and ties are kept.  nilearn's 'percentile' and 'img_value' strategies map onto 'value' with a cutoff
computed by the caller.  nilearn propagates non-finite elements into the threshold; here they are 0.  The extractor
'local_regions' (random walker) is not implemented.

Every function has a `*_host` twin made of numpy and scipy: what runs without a GPU, the judge of the tests and the CPU
baseline of scripts/bench_regions.py."""
import warnings
from collections import namedtuple

import numpy as np
import scipy.ndimage
import torch

from ._lib import lib
from .device import STREAM, call, current_device, have_gpu, scratch
from .masker import _maps, _check_affine

__all__ = ['Regions', 'connected_regions', 'region_labels', 'connected_regions_host', 'region_labels_host']

Regions = namedtuple('Regions', ['regions', 'index', 'sizes'])
STRATEGIES = (None, 'value', 'ratio_n_voxels')
MAX_MAPS_PER_PASS = 65535                                  # a grid axis holds the maps of a pass


# ---- arguments
def _check_components(components, maps):
    """(k, V) float32 / float64: a numpy array, or a CUDA tensor whose rows are contiguous (a copy otherwise)"""
    cuda = isinstance(components, torch.Tensor)
    if cuda and not components.is_cuda:
        raise ValueError('components must be a numpy array or a CUDA tensor, got a tensor on %s' % components.device)
    c = components if cuda else np.asarray(components)
    if c.ndim != 2 or c.shape[0] < 1 or c.shape[1] != maps.n_voxels:
        raise ValueError('components must be (k, %d), one column per voxel of the mask, got shape %s'
                         % (maps.n_voxels, tuple(c.shape)))
    if cuda:
        if c.dtype not in (torch.float32, torch.float64):
            c = c.to(torch.float64)
        if c.stride(1) != 1 or (c.shape[0] > 1 and c.stride(0) < c.shape[1]):
            c = c.contiguous()
    elif c.dtype not in (np.float32, np.float64):
        c = c.astype(np.float64)
    return c


def _size_threshold(min_region_size, voxel_size, mask_affine):
    """min_region_size / voxel_volume in float64: a component of n voxels is kept iff n > this"""
    try:
        size = float(min_region_size)
    except (TypeError, ValueError):
        raise ValueError('min_region_size must be a number (mm^3), got %r' % (min_region_size,))
    if not np.isfinite(size):
        raise ValueError('min_region_size must be finite, got %r' % (min_region_size,))
    if mask_affine is not None:
        volume = abs(float(np.linalg.det(_check_affine(mask_affine, 'mask_affine')[:3, :3])))
    else:
        vs = np.asarray(voxel_size, dtype=np.float64)
        if vs.shape != (3,) or not np.all(np.isfinite(vs)) or not np.all(vs > 0):
            raise ValueError('voxel_size must be three positive numbers, got %r' % (voxel_size,))
        volume = float(np.prod(vs))
    return np.float64(size) / np.float64(volume)


def _check_strategy(threshold, strategy, k):
    if strategy not in STRATEGIES:
        raise ValueError("thresholding_strategy must be None, 'value' or 'ratio_n_voxels', got %r" % (strategy,))
    if strategy is None:
        if threshold is not None:
            raise ValueError('threshold = %r needs a thresholding_strategy (\'value\' or \'ratio_n_voxels\')' % (threshold,))
        return None
    try:
        t = float(threshold)
    except (TypeError, ValueError):
        raise ValueError('thresholding_strategy = %r needs a number as threshold, got %r' % (strategy, threshold))
    if strategy == 'value' and not (t >= 0 and np.isfinite(t)):
        raise ValueError("threshold must be finite and >= 0 with thresholding_strategy = 'value', got %r" % (threshold,))
    if strategy == 'ratio_n_voxels' and not (0 < t <= k):
        raise ValueError("threshold must lie in (0, %d] (the number of maps) with thresholding_strategy = 'ratio_n_voxels', got %r"
                         % (k, threshold))
    return t


def _n_keep(r, k, V):
    return min(k * V, max(1, int(np.floor(r * V + 0.5))))


def _cutoff_host(comp, threshold, strategy):
    """the cutoff as a scalar of the components' dtype"""
    t = _check_strategy(threshold, strategy, comp.shape[0])
    if strategy is None:
        return comp.dtype.type(0)
    if strategy == 'value':
        return comp.dtype.type(t)
    a = np.where(np.isfinite(comp), np.abs(comp), 0).ravel()
    at = a.size - _n_keep(t, *comp.shape)                                    # the n_keep-th largest of a.size values
    return np.partition(a, at)[at]


def _cutoff_device(comp, threshold, strategy):
    """the same on the device: the order statistic through torch.kthvalue, one scalar comes to the host"""
    t = _check_strategy(threshold, strategy, comp.shape[0])
    if strategy is None:
        return 0.0
    np_type = np.float32 if comp.dtype == torch.float32 else np.float64
    if strategy == 'value':
        return float(np_type(t))
    a = torch.where(torch.isfinite(comp), comp.abs(), torch.zeros((), dtype=comp.dtype, device=comp.device)).reshape(-1)
    return float(torch.kthvalue(a, a.numel() - _n_keep(t, *comp.shape) + 1).values.item())


# ---- the host twins
def _labels_host(comp, maps, cutoff, size_threshold):
    """(labels (k, V) int32, counts (k,) int64, sizes [per map: (count,) int64])"""
    k, V = comp.shape
    with np.errstate(invalid='ignore'):
        fg = np.isfinite(comp) & (comp != 0) & (np.abs(comp) >= cutoff)
    labels = np.zeros((k, V), dtype=np.int32)
    counts = np.zeros(k, dtype=np.int64)
    sizes = []
    box = np.zeros(maps.mask.shape, dtype=bool)
    for m in range(k):
        box[maps.mask] = fg[m]
        lab, n = scipy.ndimage.label(box)
        n_vox = np.bincount(lab.ravel(), minlength=n + 1)[1:].astype(np.int64)
        keep = n_vox.astype(np.float64) > size_threshold
        number = np.zeros(n + 1, dtype=np.int32)
        number[1:][keep] = np.arange(1, int(keep.sum()) + 1, dtype=np.int32)
        labels[m] = number[lab[maps.mask]]
        counts[m] = int(keep.sum())
        sizes.append(n_vox[keep])
    return labels, counts, sizes


def _host_args(components, mask, min_region_size, threshold, thresholding_strategy, voxel_size, mask_affine):
    if isinstance(components, torch.Tensor):
        raise ValueError('the *_host functions take numpy arrays')
    maps = _maps(mask)
    comp = _check_components(components, maps)
    return comp, maps, _cutoff_host(comp, threshold, thresholding_strategy), _size_threshold(min_region_size, voxel_size,
                                                                                           mask_affine)


def region_labels_host(components, mask, min_region_size=1350, threshold=None, thresholding_strategy=None,
                       voxel_size=(1, 1, 1), mask_affine=None):
    """`region_labels` through numpy and scipy.ndimage.label, one map at a time: (labels (k, V) int32, counts (k,) int64)"""
    comp, maps, cutoff, size_threshold = _host_args(components, mask, min_region_size, threshold, thresholding_strategy,
                                                    voxel_size, mask_affine)
    labels, counts, _ = _labels_host(comp, maps, cutoff, size_threshold)
    return labels, counts


def _empty_warning():
    warnings.warn('connected_regions: no region is left after the threshold and the size filter; the result is empty',
                  UserWarning, stacklevel=3)


def connected_regions_host(components, mask, min_region_size=1350, threshold=None, thresholding_strategy=None,
                           voxel_size=(1, 1, 1), mask_affine=None):
    """`connected_regions` through numpy and scipy.ndimage.label, same semantics: what runs without a GPU, the judge of the
    tests and the CPU baseline of scripts/bench_regions.py"""
    comp, maps, cutoff, size_threshold = _host_args(components, mask, min_region_size, threshold, thresholding_strategy,
                                                    voxel_size, mask_affine)
    labels, counts, sizes = _labels_host(comp, maps, cutoff, size_threshold)
    R = int(counts.sum())
    regions = np.zeros((R, comp.shape[1]), dtype=comp.dtype)
    index = np.repeat(np.arange(comp.shape[0], dtype=np.int64), counts)
    r = 0
    for m in range(comp.shape[0]):
        for j in range(1, int(counts[m]) + 1):
            at = labels[m] == j
            regions[r, at] = comp[m, at]
            r += 1
    if R == 0:
        _empty_warning()
    return Regions(regions, index, np.concatenate(sizes).astype(np.int64) if sizes else np.zeros(0, np.int64))


# ---- the device
def _memory_error(what, need, device):
    free, total = torch.cuda.mem_get_info(device)
    return MemoryError('connected_regions: %s need %.2f GB of device memory, %.2f GB of %.2f GB are free'
                       % (what, need / 1e9, free / 1e9, total / 1e9))


def _maps_per_pass(maps_per_pass, k, box3, device):
    """the maps one set of launches labels: the argument, or what half of the free device memory holds"""
    if maps_per_pass is not None:
        if isinstance(maps_per_pass, bool) or not isinstance(maps_per_pass, (int, np.integer)) or maps_per_pass < 1:
            raise ValueError('maps_per_pass must be a positive integer or None, got %r' % (maps_per_pass,))
        M = min(int(maps_per_pass), k, MAX_MAPS_PER_PASS)
    free, _ = torch.cuda.mem_get_info(device)
    if maps_per_pass is None:
        M = min(int(lib.modl_region_max_maps(*box3, free // 2)), k)
    need = lib.modl_region_labels_workspace(max(M, 1), *box3)
    if need == 0:
        raise ValueError('modl_region_labels: unsupported box %s' % (box3,))
    if M < 1 or need > free:
        raise _memory_error('the labelling workspace of %d map(s) would' % max(M, 1), need, device)
    return M, need


def _labels_device(comp, maps, cutoff, size_threshold, maps_per_pass):
    """comp: CUDA tensor (k, V) with contiguous rows -> labels (k, V) int32, counts (k,) int32, sizes (k, cap) int32, all on
    the device; nothing comes to the host"""
    k, V = comp.shape
    box3 = tuple(int(n) for n in maps.col.shape)                             # (Z, Y, X): the kernels' axis order
    min_voxels = int(min(max(np.floor(size_threshold), -1), 2 ** 31 - 1))     # n > t  <=>  n > floor(t) for an integer n
    cap = V // (max(min_voxels, 0) + 1)                                      # no map has more regions than this
    with torch.cuda.device(comp.device):
        d_col, _ = maps.on(comp.device)
        labels = torch.empty((k, V), dtype=torch.int32, device=comp.device)
        counts = torch.empty(k, dtype=torch.int32, device=comp.device)
        sizes = torch.zeros((k, max(cap, 1)), dtype=torch.int32, device=comp.device)
        M, need = _maps_per_pass(maps_per_pass, k, box3, comp.device)
        ws = scratch(need, comp.device)
        ldr = comp.stride(0) if k > 1 else V
        for a in range(0, k, M):
            b = min(a + M, k)
            call('modl_region_labels', comp[a:b], ldr, b - a, V, d_col, *box3, cutoff, min_voxels, labels[a:b], V, counts[a:b],
                 sizes[a:b] if cap else None, sizes.shape[1] if cap else 0, ws, need, STREAM, device=comp.device, dtype=comp)
    return labels, counts, sizes


def _device_components(components, maps):
    """(the components on the device, was the input a CUDA tensor); (the checked numpy array, None) without a GPU"""
    comp = _check_components(components, maps)
    if isinstance(comp, torch.Tensor):
        return comp, True
    if not have_gpu():
        return comp, None
    return torch.from_numpy(np.ascontiguousarray(comp)).to(current_device()), False


def region_labels(components, mask, min_region_size=1350, threshold=None, thresholding_strategy=None, voxel_size=(1, 1, 1),
                  mask_affine=None, maps_per_pass=None):
    """The compact form of `connected_regions` (module docstring, same arguments): (labels, counts) with labels (k, V) int32,
    0 or the 1-based number of the element's region within its map, and counts (k,) int64, the regions of every map.  numpy
    in, numpy out; a CUDA tensor in, CUDA tensors out.  Without a GPU: `region_labels_host`."""
    maps = _maps(mask)
    comp, cuda = _device_components(components, maps)
    size_threshold = _size_threshold(min_region_size, voxel_size, mask_affine)
    if cuda is None:
        labels, counts, _ = _labels_host(comp, maps, _cutoff_host(comp, threshold, thresholding_strategy), size_threshold)
        return labels, counts
    labels, counts, _ = _labels_device(comp, maps, _cutoff_device(comp, threshold, thresholding_strategy), size_threshold,
                                       maps_per_pass)
    counts = counts.to(torch.int64)
    return (labels, counts) if cuda else (labels.cpu().numpy(), counts.cpu().numpy())


def connected_regions(components, mask, min_region_size=1350, threshold=None, thresholding_strategy=None,
                      voxel_size=(1, 1, 1), mask_affine=None, maps_per_pass=None):
    """Split every map into its connected regions (module docstring): Regions(regions (R, V), index (R,), sizes (R,)).

    components              (k, V) float32 / float64 (anything else is converted to float64): a numpy array (numpy arrays come
                            back) or a CUDA tensor, contiguous or not (CUDA tensors come back)
    mask                    (X, Y, Z) boolean array with V true voxels
    min_region_size         mm^3; a component of n voxels is kept iff n > min_region_size / voxel_volume
    threshold, thresholding_strategy    None / None: every finite nonzero element; 'value': |v| >= threshold;
                            'ratio_n_voxels': the round(threshold V) largest |v| over all maps, ties kept
    voxel_size, mask_affine the voxel volume is prod(voxel_size), or |det(mask_affine[:3, :3])| when the affine is given
    maps_per_pass           the maps labelled by one set of launches (their workspace is 16 bytes per box voxel and map);
                            None: what half of the free device memory holds.  It changes no bit of the result.

    On the device (csrc/regions.hip) the labelling reads the rows through the mask's column map - no volume is unmasked -,
    the per-map counts come to the host once, and the regions are gathered by one launch.  Without a GPU a numpy input goes
    through `connected_regions_host`.  MemoryError: the regions, or the workspace of one map, do not fit the free device
    memory.  ValueError: a bad mask, components that are not (k, V), an unknown strategy, a threshold out of range, a
    non-positive voxel size, a bad affine.  UserWarning: no region is left (the arrays are empty)."""
    maps = _maps(mask)
    comp, cuda = _device_components(components, maps)
    size_threshold = _size_threshold(min_region_size, voxel_size, mask_affine)
    if cuda is None:
        return connected_regions_host(comp, maps, min_region_size, threshold, thresholding_strategy, voxel_size, mask_affine)
    k, V = comp.shape
    labels, counts, sizes = _labels_device(comp, maps, _cutoff_device(comp, threshold, thresholding_strategy), size_threshold,
                                           maps_per_pass)
    with torch.cuda.device(comp.device):
        counts = counts.to(torch.int64)
        offsets = torch.zeros(k + 1, dtype=torch.int64, device=comp.device)
        torch.cumsum(counts, 0, out=offsets[1:])
        R = int(offsets[-1].item())                                          # the one value that comes to the host
        need = R * V * comp.element_size()
        if need > torch.cuda.mem_get_info(comp.device)[0]:
            raise _memory_error('the %d regions of %d voxels' % (R, V), need, comp.device)
        regions = torch.empty((R, V), dtype=comp.dtype, device=comp.device)
        index = torch.repeat_interleave(torch.arange(k, dtype=torch.int64, device=comp.device), counts, output_size=R)
        kept = torch.arange(sizes.shape[1], device=comp.device)[None, :] < counts[:, None]
        sizes = sizes[kept].to(torch.int64)                                  # row-major: by map, then by number
        if R:
            call('modl_region_gather', comp, comp.stride(0) if k > 1 else V, k, V, labels, V, offsets, R, regions, V, STREAM,
                 device=comp.device, dtype=comp)
    if R == 0:
        _empty_warning()
    if cuda:
        return Regions(regions, index, sizes)
    return Regions(regions.cpu().numpy(), index.cpu().numpy(), sizes.cpu().numpy())
