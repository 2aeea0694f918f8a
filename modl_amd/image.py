"""ImageDictFact: dictionary learning on image patches (reference:
modl/decomposition/image.py:13-224), driving modl_amd.DictFact's
prepare / partial_fit / shuffle / set_params exactly as the reference does
(image.py:96-152).  The image is uploaded once and stays resident in HBM; every
buffer of patches is gathered, centred, normalised and flattened by one HIP launch
(modl_image_patches_*, csrc/image.hip: modl/feature_extraction/image.py:54-63 +
modl/input_data/image.py:4-23 fused) and handed to the SOMF step as a device tensor.
The patch-origin lists (fill / clean_mask, image_fast.pyx:12-74) are integer host
work behind the same C-ABI.  The numpy `scale_patches` below serves the public
transform / score on patches the caller holds in host memory.
The way back (no counterpart in the reference): `ImageDictFact.reconstruct` encodes
every window of a regular patch grid, decodes it, undoes the per-patch scaling and
averages the overlapping windows, all on the device (`grid_origins`, `grid_patches`,
`reconstruct_from_patches`; the kernels are in csrc/image.hip, "reconstruction")."""
import ctypes as C
import time
from collections import namedtuple
from math import sqrt

import numpy as np
import torch
from numpy.lib.stride_tricks import sliding_window_view
from sklearn.base import BaseEstimator
from sklearn.utils import check_random_state, gen_batches
from sklearn.utils.validation import check_is_fitted

from .device import STREAM, call, default_device, to_device
from .dict_fact import DictFact, _held_out_set


ImageHeldOutError = namedtuple('ImageHeldOutError', ['rmse', 'n_held_out', 'n_unfilled'])


def scale_patches(X, with_mean=True, with_std=True, channel_wise=True, copy=True):
    """Centred / l2-normalised patches, X: (n, ph, pw, c).  Same arithmetic, in the same order, as the reference's
    modl/input_data/image.py:4-23 (statistics per patch and channel over the ph x pw positions, the norm times
    sqrt(c); or per patch over everything when not channel_wise) written once over a reduction-axes tuple; the
    training path never calls this - its patches are produced already scaled by modl_image_patches_* on the device."""
    X = np.array(X, copy=True) if copy else X
    axes = (1, 2) if channel_wise else (1, 2, 3)
    if with_mean:
        X -= X.mean(axis=axes, keepdims=True)
    if with_std:
        norm = np.sqrt(np.square(X).sum(axis=axes, keepdims=True))
        norm[norm == 0] = 1
        if channel_wise:
            norm = norm * sqrt(X.shape[3])
        X /= norm
    return X


def fill(p, q, r):
    """All patch coordinates in C order (image_fast.pyx:59-74)."""
    out = np.empty((p * q * r, 3), dtype=np.int64)
    call('modl_image_fill', p, q, r, out, device=None)
    return out


def clean_mask(patches, image):
    """Coordinates of the patches without any missing (-1) pixel (image_fast.pyx:12-57)."""
    x, y, z = patches.shape[3:]
    if image.dtype not in (np.float32, np.float64):
        raise TypeError('clean_mask: float32 or float64 image expected (fused `floating`, image_fast.pyx:12)')
    image = np.ascontiguousarray(image)
    H, W, Cc = image.shape
    out = np.empty(((H - x + 1) * (W - y + 1) * (Cc - z + 1), 3), dtype=np.int64)
    n = C.c_int64()
    call('modl_image_clean_mask', image, H, W, Cc, x, y, z, out, C.byref(n), device=None, dtype=image.dtype)
    return out[:n.value].copy()


# ---- the patch grid of reconstruction ----------------------------------------------------------------------------------
def _grid(image_shape, patch_size, stride):
    """(H, W, C, x, y, si, sj) of a grid, checked: every bad argument is a ValueError here, before any library call"""
    if len(image_shape) != 3:
        raise ValueError('an image of shape (height, width, channels) is expected, got shape %s' % (tuple(image_shape),))
    H, W, Cc = (int(v) for v in image_shape)
    x, y = (int(v) for v in patch_size)
    si, sj = (int(v) for v in (stride if np.ndim(stride) else (stride, stride)))
    if x < 1 or y < 1 or x > H or y > W:
        raise ValueError('patch_size %s does not fit an image of shape %s' % ((x, y), (H, W, Cc)))
    if not (1 <= si <= x and 1 <= sj <= y):
        raise ValueError('stride %s: 1 <= stride <= patch_size %s is needed (a larger one leaves pixels uncovered)'
                         % ((si, sj), (x, y)))
    if not 1 <= Cc <= 1024:
        raise ValueError('1 to 1024 channels are supported, got %d' % Cc)
    return H, W, Cc, x, y, si, sj


def _axis_origins(L, x, s):
    o = np.arange(0, L - x + 1, s, dtype=np.int64)
    return o if o[-1] == L - x else np.append(o, L - x)


def grid_origins(image_shape, patch_size, stride=1):
    """Origins (i, j, 0) of the patch grid of reconstruction, an (n, 3) int64 array in patch order.  The rule: along an
    axis of length L with patch length x and stride s the origins are 0, s, 2 s, ... <= L - x, plus L - x itself when
    it is not already the last one, so that the border is always covered; a patch spans all channels; patches are
    numbered row-major over (grid row, grid column)."""
    H, W, _, x, y, si, sj = _grid(image_shape, patch_size, stride)
    oi, oj = _axis_origins(H, x, si), _axis_origins(W, y, sj)
    out = np.zeros((oi.shape[0] * oj.shape[0], 3), dtype=np.int64)
    out[:, 0], out[:, 1] = np.repeat(oi, oj.shape[0]), np.tile(oj, oi.shape[0])
    return out


def _grid_shape(g):
    H, W, _, x, y, si, sj = g
    rows, cols = C.c_int64(), C.c_int64()
    call('modl_image_grid_shape', H, W, x, y, si, sj, C.byref(rows), C.byref(cols), device=None)
    return rows.value, cols.value


def _grid_patches_pass(d_image, g, gcols, row0, nrows, with_mean, with_std):
    """the patches of the grid rows [row0, row0 + nrows) of a device image: (patches, mean, den)"""
    H, W, Cc, x, y, si, sj = g
    n, kw = nrows * gcols, dict(dtype=d_image.dtype, device=d_image.device)
    out, mean, den = torch.empty((n, x * y * Cc), **kw), torch.empty((n, Cc), **kw), torch.empty((n, Cc), **kw)
    call('modl_image_grid_patches', d_image, H, W, Cc, x, y, si, sj, row0, nrows, int(bool(with_mean)), int(bool(with_std)),
         out, x * y * Cc, mean, den, STREAM, device=d_image.device, dtype=d_image)
    return out, mean, den


def _overlap_add(d_patches, g, row0, nrows, acc):
    H, W, Cc, x, y, si, sj = g
    call('modl_image_overlap_add', d_patches, d_patches.stride(0), H, W, Cc, x, y, si, sj, row0, nrows, acc, STREAM,
         device=acc.device, dtype=d_patches)


def _overlap_finish(acc, g, dtype):
    H, W, Cc, x, y, si, sj = g
    out = torch.empty((H, W, Cc), dtype=dtype, device=acc.device)
    call('modl_image_overlap_finish', acc, H, W, Cc, x, y, si, sj, out, STREAM, device=acc.device, dtype=out)
    return out


def _grid_patches_masked_pass(d_image, d_obs, g, gcols, row0, nrows, with_mean, with_std):
    """`_grid_patches_pass` on an image with holes (d_obs (H, W, C) uint8, 1 = observed): (patches, mean, den, obs rows
    (n, x*y*C) uint8, nobs (n,) int32), the statistics taken over the observed elements (modl_image_grid_patches_masked_*)"""
    H, W, Cc, x, y, si, sj = g
    n, kw = nrows * gcols, dict(dtype=d_image.dtype, device=d_image.device)
    out, mean, den = torch.empty((n, x * y * Cc), **kw), torch.empty((n, Cc), **kw), torch.empty((n, Cc), **kw)
    obs = torch.empty((n, x * y * Cc), dtype=torch.uint8, device=d_image.device)
    nobs = torch.empty(n, dtype=torch.int32, device=d_image.device)
    call('modl_image_grid_patches_masked', d_image, H, W, Cc, x, y, si, sj, row0, nrows, int(bool(with_mean)),
         int(bool(with_std)), out, x * y * Cc, mean, den, d_obs, obs, nobs, STREAM, device=d_image.device, dtype=d_image)
    return out, mean, den, obs, nobs


def _patches_masked(d_image, d_obs, origins, patch_shape, with_mean, with_std):
    """`_grid_patches_masked_pass` at the origins of an index list (n, 3) (modl_image_patches_masked_*): (patches, mean,
    den, obs rows, nobs) of the windows of an image with holes, scaled on their observed elements"""
    H, W, Cc = d_image.shape
    x, y, z = (int(v) for v in patch_shape)
    idx = torch.from_numpy(np.ascontiguousarray(origins, dtype=np.int64)).to(d_image.device)
    n, kw = idx.shape[0], dict(dtype=d_image.dtype, device=d_image.device)
    out, mean, den = torch.empty((n, x * y * z), **kw), torch.empty((n, Cc), **kw), torch.empty((n, Cc), **kw)
    obs = torch.empty((n, x * y * z), dtype=torch.uint8, device=d_image.device)
    nobs = torch.empty(n, dtype=torch.int32, device=d_image.device)
    call('modl_image_patches_masked', d_image, H, W, Cc, idx, n, x, y, z, int(bool(with_mean)), int(bool(with_std)), out,
         x * y * z, mean, den, d_obs, obs, nobs, STREAM, device=d_image.device, dtype=d_image)
    return out, mean, den, obs, nobs


def masked_candidates(mask, patch_size, min_observed):
    """Origins (i, j, 0), in C order, of the windows of an (H, W, C) bool mask whose observed share of their x*y*C
    elements is at least `min_observed` (integer arithmetic on a summed-area table; host work, like clean_mask)"""
    mask = np.asarray(mask) != 0
    H, W, Cc = mask.shape
    x, y = (int(v) for v in patch_size)
    sat = np.zeros((H + 1, W + 1), dtype=np.int64)
    sat[1:, 1:] = mask.sum(axis=2, dtype=np.int64).cumsum(axis=0).cumsum(axis=1)
    cnt = sat[x:, y:] - sat[:-x, y:] - sat[x:, :-y] + sat[:-x, :-y]
    ii, jj = np.nonzero(cnt >= min_observed * (x * y * Cc))
    out = np.zeros((ii.shape[0], 3), dtype=np.int64)
    out[:, 0], out[:, 1] = ii, jj
    return out


def _overlap_add_weighted(d_patches, use, g, row0, nrows, acc, cnt):
    H, W, Cc, x, y, si, sj = g
    call('modl_image_overlap_add_weighted', d_patches, d_patches.stride(0), H, W, Cc, x, y, si, sj, row0, nrows, acc, use,
         cnt, STREAM, device=acc.device, dtype=d_patches)


def _inpaint_finish(acc, cnt, d_image, d_obs, keep_observed):
    H, W, Cc = d_image.shape
    out = torch.empty_like(d_image)
    call('modl_image_inpaint_finish', acc, cnt, d_image, d_obs, H, W, Cc, int(bool(keep_observed)), out, STREAM,
         device=acc.device, dtype=out)
    return out


PASS_BYTES = 256 << 20      # a pass's patch buffer stays under this: a memory bound, not a tuned value


def _passes(grows, gcols, row_bytes, rows_per_pass):
    """(row0, nrows) of every pass over the grid rows, in order"""
    if rows_per_pass is None:
        rows_per_pass = max(1, PASS_BYTES // (gcols * row_bytes))
    rows_per_pass = int(rows_per_pass)
    if rows_per_pass < 1:
        raise ValueError('rows_per_pass >= 1 is needed, got %d' % rows_per_pass)
    return [(r0, min(rows_per_pass, grows - r0)) for r0 in range(0, grows, rows_per_pass)]


def _stage_image(image, device=None, dtype=None):
    """(H, W, C) image, numpy or tensor -> contiguous float32 / float64 device tensor"""
    if isinstance(image, torch.Tensor):
        floating = image.dtype in (torch.float32, torch.float64)
        if device is None and image.is_cuda:
            device = image.device
    else:
        image = np.asarray(image)
        floating = image.dtype in (np.float32, np.float64)
    if dtype is None and not floating:
        dtype = np.float64
    return to_device(image, torch.device(device) if device is not None else default_device(), dtype=dtype)


def grid_patches(image, patch_size, stride=1, with_mean=True, with_std=True, device=None):
    """Every patch of the grid (`grid_origins`) of an (H, W, C) image, flattened and scaled channel-wise as
    `scale_patches` does, with what the scaling removed: the device tensors (patches (n, x*y*C), mean (n, C), den (n, C)),
    den being the divisor that was applied (1 where none was) - `patches * den + mean` per channel is the window again."""
    g = _grid(np.shape(image), patch_size, stride)
    d_image = _stage_image(image, device)
    grows, gcols = _grid_shape(g)
    return _grid_patches_pass(d_image, g, gcols, 0, grows, with_mean, with_std)


def reconstruct_from_patches(patches, image_shape, patch_size, stride=1, rows_per_pass=None):
    """The image whose pixels are the averages of the flattened patches (n, x*y*C) that cover them, the patches lying
    on the grid of `grid_origins` (already on the image's scale).  Sums are accumulated in float64 in grid order by a
    gather on the device: the result does not depend on `rows_per_pass` (grid rows per launch) nor on the run, bit for
    bit.  A numpy array gives a numpy array, a CUDA tensor a CUDA tensor, of the patches' dtype."""
    g = _grid(image_shape, patch_size, stride)
    H, W, Cc, x, y = g[:5]
    on_host = not isinstance(patches, torch.Tensor)
    if on_host:
        patches = np.asarray(patches)
        patches = torch.from_numpy(np.ascontiguousarray(
            patches, dtype=None if patches.dtype in (np.float32, np.float64) else np.float64)).to(default_device())
    grows, gcols = _grid_shape(g)
    if patches.ndim != 2 or tuple(patches.shape) != (grows * gcols, x * y * Cc):
        raise ValueError('patches of shape %s expected on this grid, got %s'
                         % ((grows * gcols, x * y * Cc), tuple(patches.shape)))
    patches = patches.contiguous()
    acc = torch.zeros((H, W, Cc), dtype=torch.float64, device=patches.device)
    for row0, nrows in _passes(grows, gcols, patches.shape[1] * patches.element_size(), rows_per_pass):
        _overlap_add(patches[row0 * gcols:(row0 + nrows) * gcols], g, row0, nrows, acc)
    out = _overlap_finish(acc, g, patches.dtype)
    return out.cpu().numpy() if on_host else out


class LazyCleanPatchExtractor(BaseEstimator):
    """Patch origins of an image, drawn once, patches produced on demand (the estimator surface of
    modl/feature_extraction/image.py:8-83: `fit`, `transform`, `partial_transform`, `shuffle`, `indices_3d`,
    `patches_`).  The state is the (n, 3) array of origins - every window without a missing (-1) pixel
    (`clean_mask`) or simply all of them (`fill`), permuted by the random state and cut to `max_patches`; a batch of
    patches is a fancy index into the strided window view on the host (`_take`) or one launch on the HBM-resident
    image (`partial_transform_scaled`)."""

    def __init__(self, patch_size=None, random_state=None, max_patches=None):
        self.patch_size = patch_size
        self.max_patches = max_patches
        self.random_state = random_state

    def fit(self, X, y=None):
        self.random_state = check_random_state(self.random_state)
        height, width, n_channels = X.shape
        ph, pw = self.patch_size if self.patch_size is not None else (height // 10, width // 10)
        self.image_, self._device_image = X, None
        self.patches_ = sliding_window_view(X, (ph, pw, n_channels))          # every window, as a strided view
        has_holes = bool(np.any(X == -1))
        origins = clean_mask(self.patches_, X) if has_holes else fill(*self.patches_.shape[:3])
        keep = self.random_state.permutation(origins.shape[0])[:self.max_patches]
        self.indices_3d = origins[keep]
        return self

    def _take(self, origins):
        return self.patches_[origins[:, 0], origins[:, 1], origins[:, 2]]

    def transform(self, X=None):
        if X is not None:
            self.fit(X)
        return self._take(self.indices_3d)

    def partial_transform(self, X=None, batch=None):
        if X is not None:
            self.fit(X)
        if batch is None:
            return self._take(self.indices_3d)
        return self._take(self.indices_3d[slice(0, batch) if isinstance(batch, int) else batch])

    def partial_transform_scaled(self, backend, batch, with_mean=True, with_std=True):
        """Device path of partial_transform + scale_patches + flattening: the patches `batch` of the HBM-resident
        image as a (n, patch_size) device tensor (image.py:139-144 in one launch)."""
        if isinstance(batch, int):
            batch = slice(0, batch)
        if self._device_image is None or self._device_image[0] is not backend:
            self._device_image = (backend, backend.stage_image(self.image_))
        return backend.image_patches(self._device_image[1], self.indices_3d[batch], self.patch_shape_, with_mean, with_std)

    def shuffle(self, permutation=None):
        if permutation is None:
            permutation = self.random_state.permutation(self.indices_3d.shape[0])
        self.indices_3d = self.indices_3d[permutation]

    @property
    def n_patches_(self):
        return self.indices_3d.shape[0]

    @property
    def patch_shape_(self):
        return self.patches_.shape[-3:]


def _flatten_patches(patches, with_mean=True, with_std=True, copy=False):
    n_patches = patches.shape[0]
    patches = scale_patches(patches, with_mean=with_mean, with_std=with_std, copy=copy)
    return patches.reshape((n_patches, -1))


class ImageDictFact(BaseEstimator):
    methods = {'masked': {'G_agg': 'masked', 'Dx_agg': 'masked'},
               'dictionary only': {'G_agg': 'full', 'Dx_agg': 'full'},
               'gram': {'G_agg': 'masked', 'Dx_agg': 'masked'},      # first epochs; switched at epoch 4
               'average': {'G_agg': 'average', 'Dx_agg': 'average'},
               'reducing ratio': {'G_agg': 'masked', 'Dx_agg': 'masked'}}

    settings = {'dictionary learning': {'comp_l1_ratio': 0, 'code_l1_ratio': 1, 'comp_pos': False,
                                        'code_pos': False, 'with_std': True, 'with_mean': True},
                'NMF': {'comp_l1_ratio': 0, 'code_l1_ratio': 1, 'comp_pos': True, 'code_pos': True,
                        'with_std': True, 'with_mean': False}}

    def __init__(self, method='masked', setting='dictionary learning', patch_size=(8, 8), batch_size=100,
                 buffer_size=None, step_size=1e-3, n_components=50, alpha=0.1, learning_rate=0.92, reduction=10,
                 n_epochs=1, random_state=None, callback=None, max_patches=None, verbose=0, n_threads=1):
        self.n_threads = n_threads
        self.step_size = step_size
        self.verbose = verbose
        self.callback = callback
        self.random_state = random_state
        self.n_epochs = n_epochs
        self.reduction = reduction
        self.learning_rate = learning_rate
        self.alpha = alpha
        self.n_components = n_components
        self.batch_size = batch_size
        self.method = method
        self.setting = setting
        self.patch_size = patch_size
        self.buffer_size = buffer_size
        self.max_patches = max_patches

    _dict_fact_class = DictFact

    def fit(self, image, y=None, mask=None, min_observed=0.25):
        """image.py:68-153.  With `mask` ((H, W) or (H, W, C), True = observed) the dictionary is learned from the damaged
        image itself: every window whose observed share is at least `min_observed` is a candidate (instead of the clean
        windows only), each buffer of windows is scaled on its observed elements on the device and fitted with its mask
        (`DictFact.partial_fit(..., mask=)`).  The usual call: `est.fit(image, mask=image != -1).inpaint(image)`.
        A masked fit needs G_agg = Dx_agg = 'masked' on every epoch: the methods 'masked' and 'reducing ratio' (whose
        schedule of `reduction` is kept but has no effect, a masked minibatch does not use `reduction`), and 'gram' up to
        n_epochs = 4 - its schedule switches to 'full' / 'average' at the fifth epoch, which a mask does not support."""
        if mask is not None:
            if self.method == 'sgd' or ImageDictFact.methods[self.method] != {'G_agg': 'masked', 'Dx_agg': 'masked'} or \
                    (self.method == 'gram' and self.n_epochs > 4):
                raise ValueError("a fit with a mask needs a method whose aggregations are G_agg = Dx_agg = 'masked' on "
                                 "every epoch ('masked', 'reducing ratio', or 'gram' with n_epochs <= 4: it switches to "
                                 "'full' / 'average' at the fifth), got method=%r, n_epochs=%d" % (self.method, self.n_epochs))
            if np.ndim(image) == 2:
                image = image[:, :, None]
            if len(np.shape(image)) != 3 or tuple(np.shape(mask)) not in (tuple(np.shape(image))[:2], tuple(np.shape(image))):
                raise ValueError('mask of shape %s does not match an image of shape %s'
                                 % (tuple(np.shape(mask)), tuple(np.shape(image))))
            if self.n_components > 1024:
                raise ValueError('a fit with a mask supports at most 1024 components (one Gram matrix per window), got %d'
                                 % self.n_components)
        self.random_state = check_random_state(self.random_state)
        if self.method != 'sgd':
            method = ImageDictFact.methods[self.method]
            G_agg, Dx_agg = method['G_agg'], method['Dx_agg']
            reduction = self.reduction
            optimizer = 'variational'
        else:
            optimizer, reduction, G_agg, Dx_agg = 'sgd', 1, 'full', 'full'
        setting = ImageDictFact.settings[self.setting]
        with_std, with_mean = setting['with_std'], setting['with_mean']
        buffer_size = self.batch_size * 10 if self.buffer_size is None else self.buffer_size

        self.dict_fact_ = self._dict_fact_class(
            n_epochs=self.n_epochs, random_state=self.random_state, n_components=self.n_components,
            comp_l1_ratio=setting['comp_l1_ratio'], learning_rate=self.learning_rate, comp_pos=setting['comp_pos'],
            optimizer=optimizer, step_size=self.step_size, code_pos=setting['code_pos'], batch_size=self.batch_size,
            G_agg=G_agg, Dx_agg=Dx_agg, reduction=reduction, code_alpha=self.alpha,
            code_l1_ratio=setting['code_l1_ratio'], tol=1e-2, callback=self._callback, verbose=self.verbose,
            n_threads=self.n_threads)
        if mask is not None:
            return self._fit_masked(image, mask, min_observed, with_mean, with_std, buffer_size)

        patch_extractor = LazyCleanPatchExtractor(patch_size=self.patch_size, max_patches=self.max_patches,
                                                  random_state=self.random_state)
        patch_extractor.fit(image)
        n_patches = patch_extractor.n_patches_
        self.patch_shape_ = patch_extractor.patch_shape_

        # device pipeline whenever the image is float32 / float64 (the dtype the reference's in-place scale_patches
        # accepts) and the step's backend owns a GPU
        probe = self.dict_fact_._make_backend()
        on_device = hasattr(probe, 'image_patches') and image.dtype in (np.float32, np.float64)

        def scaled(batch):
            if on_device:
                return patch_extractor.partial_transform_scaled(probe, batch, with_mean=with_mean, with_std=with_std)
            return _flatten_patches(patch_extractor.partial_transform(batch=batch), with_mean=with_mean,
                                    with_std=with_std, copy=True)

        self.dict_fact_.prepare(n_samples=n_patches, X=scaled(slice(0, self.n_components)))
        for i in range(self.n_epochs):
            if i >= 1:
                permutation = self.dict_fact_.shuffle()
                patch_extractor.shuffle(permutation)
            buffers = gen_batches(n_patches, buffer_size)
            if self.method == 'gram' and i == 4:
                self.dict_fact_.set_params(G_agg='full', Dx_agg='average')
            if self.method == 'reducing ratio':
                reduction = 1 + (self.reduction - 1) / sqrt(i + 1)
                self.dict_fact_.set_params(reduction=reduction)
            for buffer in buffers:
                self.dict_fact_.partial_fit(scaled(buffer), buffer)
        return self

    def _fit_masked(self, image, mask, min_observed, with_mean, with_std, buffer_size):
        df = self.dict_fact_
        probe = df._make_backend()
        d_image = _stage_image(image, probe.device)
        H, W, Cc = d_image.shape
        m = mask.cpu().numpy() if isinstance(mask, torch.Tensor) else np.asarray(mask)
        m = np.array(np.broadcast_to((m != 0) if m.ndim == 3 else (m != 0)[:, :, None], (H, W, Cc)), order='C')
        d_obs = torch.from_numpy(m.view(np.uint8)).to(d_image.device)
        x, y = (int(v) for v in (self.patch_size if self.patch_size is not None else (H // 10, W // 10)))
        if x < 1 or y < 1 or x > H or y > W:
            raise ValueError('patch_size %s does not fit an image of shape %s' % ((x, y), (H, W, Cc)))
        self.patch_shape_ = (x, y, Cc)
        origins = masked_candidates(m, (x, y), min_observed)
        keep = self.random_state.permutation(origins.shape[0])[:self.max_patches]
        origins = origins[keep]
        n_patches = origins.shape[0]
        if n_patches < self.n_components:
            raise ValueError('%d windows have at least %g of their elements observed: at least n_components = %d are '
                             'needed' % (n_patches, min_observed, self.n_components))

        def scaled(batch):
            out = _patches_masked(d_image, d_obs, origins[batch], self.patch_shape_, with_mean, with_std)
            return out[0], out[3]

        df.prepare(n_samples=n_patches, X=scaled(slice(0, self.n_components))[0])
        for i in range(self.n_epochs):
            if i >= 1:
                origins = origins[df.shuffle()]
            if self.method == 'reducing ratio':
                df.set_params(reduction=1 + (self.reduction - 1) / sqrt(i + 1))
            for buffer in gen_batches(n_patches, buffer_size):
                patches, obs = scaled(buffer)
                df.partial_fit(patches, buffer, mask=obs)
        return self

    def _prep(self, patches):
        s = ImageDictFact.settings[self.setting]
        return _flatten_patches(np.asarray(patches), with_mean=s['with_mean'], with_std=s['with_std'], copy=True)

    def transform(self, patches, sparse=False):
        """codes of the patches; sparse=True: as CSR (`DictFact.transform`)"""
        return self.dict_fact_.transform(self._prep(patches), sparse=sparse)

    def score(self, patches):
        return self.dict_fact_.score(self._prep(patches))

    def reconstruct(self, image, stride=1, rows_per_pass=None, algorithm='enet', n_nonzero_coefs=None,
                    residual_tol=None):
        """The image rebuilt from the sparse codes of its patches: every window of the patch grid (`grid_origins`:
        stride `stride`, an int or a pair, the last window clamped to the border) is scaled as in `fit`, encoded on the
        fitted dictionary, decoded, put back on the image's scale, and the overlapping windows are averaged.  Returns
        an array of the image's shape in the dtype of the fitted dictionary (the input is cast as `transform` casts).
        Image, patches, codes and sums stay on the device, `rows_per_pass` grid rows at a time (default: as many as keep
        the patch buffer under 256 MB); the result does not depend on it.  The value -1 is ordinary data here.
        `algorithm`, `n_nonzero_coefs`, `residual_tol`: the coder, as in `DictFact.transform` ('omp': orthogonal matching
        pursuit).  The threshold applies to the rows as they are coded, that is after the per-patch scaling of `fit`
        (centred and, by the setting, divided by the patch's norm), not to the pixels of the image."""
        check_is_fitted(self, 'dict_fact_')
        omp = self.dict_fact_._omp_params(algorithm, n_nonzero_coefs, residual_tol)
        be = self.dict_fact_._backend
        g = _grid(np.shape(image), self.patch_shape_[:2], stride)
        if g[2] != self.patch_shape_[2]:
            raise ValueError('the image has %d channels, the estimator was fitted on %d' % (g[2], self.patch_shape_[2]))
        on_host = not isinstance(image, torch.Tensor)
        d_image = _stage_image(image, be.device, dtype=be.dtype)
        s = ImageDictFact.settings[self.setting]
        kw = self.dict_fact_._plan_kwargs(4096)
        G = be.G if self.dict_fact_.G_agg == 'full' else None              # as CodingMixin._transform
        grows, gcols = _grid_shape(g)
        acc = torch.zeros(g[:3], dtype=torch.float64, device=be.device)
        for row0, nrows in _passes(grows, gcols, be.p * be.dtype.itemsize, rows_per_pass):
            patches, mean, den = _grid_patches_pass(d_image, g, gcols, row0, nrows, s['with_mean'], s['with_std'])
            if omp is not None:
                code = be.omp(patches, omp[0], omp[1], G, kw=kw)[0]
            else:
                code = be.transform(patches, kw, G, to_host=False)
            _overlap_add(be.decode(code, mean, den), g, row0, nrows, acc)
        out = _overlap_finish(acc, g, d_image.dtype)
        return out.cpu().numpy() if on_host else out

    def inpaint(self, image, mask=None, stride=1, missing=-1, keep_observed=True, rows_per_pass=None,
                return_filled=False, algorithm='enet', n_nonzero_coefs=None, residual_tol=None):
        """The image with its missing elements filled in from the fitted dictionary.  `mask` is a bool array of shape
        (H, W) or (H, W, C), True = observed; None: `image != missing`, element by element (`clean_mask`'s rule).  As
        `reconstruct`, on the same patch grid, but every window is scaled by the statistics of its observed elements
        and coded on them alone (`CodingMixin.transform` with a mask: a window without a hole is coded exactly as
        `reconstruct` codes it, one without an observed element is left out); the decoded windows that were used are
        averaged.  Elements that no used window covers keep their input value, and so do, with `keep_observed`, the
        observed ones.  Shape, dtype, host / device in -> out and the independence from `rows_per_pass` are those of
        `reconstruct`; on an image without holes `inpaint(image, keep_observed=False)` is `reconstruct(image)` bit
        for bit.  With `return_filled` the (H, W) bool array of the pixels that a used window covers comes along.
        Holes wider than a patch are not filled (the method is not iterated).
        `algorithm`, `n_nonzero_coefs`, `residual_tol`: the coder, as in `DictFact.transform` with a mask.  The threshold
        applies to the rows as they are coded, after the per-patch scaling by the statistics of the observed elements:
        a window's residual is r |x_S - code D_S|^2 on its scaled observed elements."""
        check_is_fitted(self, 'dict_fact_')
        omp = self.dict_fact_._omp_params(algorithm, n_nonzero_coefs, residual_tol)
        be = self.dict_fact_._backend
        g = _grid(np.shape(image), self.patch_shape_[:2], stride)
        if g[2] != self.patch_shape_[2]:
            raise ValueError('the image has %d channels, the estimator was fitted on %d' % (g[2], self.patch_shape_[2]))
        if mask is not None and tuple(np.shape(mask)) not in (g[:2], g[:3]):
            raise ValueError('mask of shape %s: %s or %s is expected' % (tuple(np.shape(mask)), g[:2], g[:3]))
        if self.n_components > 1024:
            raise ValueError('inpaint supports at most 1024 components (one Gram matrix per window), got %d'
                             % self.n_components)
        on_host = not isinstance(image, torch.Tensor)
        d_image = _stage_image(image, be.device, dtype=be.dtype)
        if mask is None:
            d_obs = (d_image != missing).to(torch.uint8)
        else:
            m = mask if isinstance(mask, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(mask) != 0))
            m = (m != 0).to(be.device)
            d_obs = (m if m.ndim == 3 else m[:, :, None].expand(g[:3])).to(torch.uint8).contiguous()
        s = ImageDictFact.settings[self.setting]
        kw = self.dict_fact_._plan_kwargs(4096)
        G = be.G if self.dict_fact_.G_agg == 'full' else None              # as CodingMixin._transform
        grows, gcols = _grid_shape(g)
        acc = torch.zeros(g[:3], dtype=torch.float64, device=be.device)
        cnt = torch.zeros(g[:2], dtype=torch.int32, device=be.device)
        for row0, nrows in _passes(grows, gcols, be.p * be.dtype.itemsize, rows_per_pass):
            patches, mean, den, obs, nobs = _grid_patches_masked_pass(d_image, d_obs, g, gcols, row0, nrows,
                                                                      s['with_mean'], s['with_std'])
            if omp is not None:
                code = be.omp(patches, omp[0], omp[1], G, obs=obs, kw=kw, nobs=nobs)[0]
            else:
                code = be.transform_masked(patches, obs, kw, G, nobs=nobs)
            use = (nobs > 0).to(torch.uint8)
            _overlap_add_weighted(be.decode(code, mean, den), use, g, row0, nrows, acc, cnt)
        out = _inpaint_finish(acc, cnt, d_image, d_obs, keep_observed)
        out = out.cpu().numpy() if on_host else out
        if not return_filled:
            return out
        filled = cnt > 0
        return out, (filled.cpu().numpy() if on_host else filled)

    def held_out_error(self, image, mask=None, held_out=0.1, stride=1, missing=-1, random_state=None, algorithm='enet',
                       n_nonzero_coefs=None, residual_tol=None):
        """Error of `inpaint` on elements it was not shown.  The observed elements (`mask`, or `image != missing`) are
        split by `held_out`: a bool array of shape (H, W) or (H, W, C), or a fraction in (0, 1), in which case
        H = check_random_state(random_state).random_sample(image.shape) < held_out.  The image is inpainted from
        observed & ~H (`inpaint(image, mask=observed & ~H, stride=stride, return_filled=True, ...)`) and compared with
        its own values on observed & H.  Returns ImageHeldOutError(rmse, n_held_out, n_unfilled): the root mean squared
        difference over the held-out elements that a used window covered (summed in f64 on the device; nan when there
        is none), their number, and the number of held-out elements that no used window covered.  This is what a
        `callback` of a masked fit calls: fit on mask & ~H, watch H."""
        check_is_fitted(self, 'dict_fact_')
        be = self.dict_fact_._backend
        g = _grid(np.shape(image), self.patch_shape_[:2], stride)
        if mask is not None and tuple(np.shape(mask)) not in (g[:2], g[:3]):
            raise ValueError('mask of shape %s: %s or %s is expected' % (tuple(np.shape(mask)), g[:2], g[:3]))
        if isinstance(held_out, (float, np.floating)):
            H = _held_out_set(held_out, tuple(np.shape(image)), random_state)
        else:
            H = _held_out_set(held_out, g[:2] if len(np.shape(held_out)) == 2 else g[:3], random_state)

        def on_device(m):
            m = m if isinstance(m, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(m) != 0))
            m = (m != 0).to(be.device)
            return m if m.ndim == 3 else m[:, :, None].expand(g[:3])

        d_image = _stage_image(image, be.device, dtype=be.dtype)
        obs = (d_image != missing) if mask is None else on_device(mask)
        H = on_device(H)
        out, filled = self.inpaint(d_image, mask=obs & ~H, stride=stride, return_filled=True, algorithm=algorithm,
                                   n_nonzero_coefs=n_nonzero_coefs, residual_tol=residual_tol)
        held = obs & H
        seen = held & filled[:, :, None]
        diff = torch.where(seen, out.double() - d_image.double(), torch.zeros((), dtype=torch.float64, device=be.device))
        sq, n_seen, n_held = float((diff * diff).sum()), int(seen.sum()), int(held.sum())
        return ImageHeldOutError(sqrt(sq / n_seen) if n_seen else float('nan'), n_seen, n_held - n_seen)

    def stage_test_patches(self, patches):
        """Scaled, flattened test patches as a tensor on the estimator's device: `score_staged` then evaluates the
        objective without any host copy of the test set or of the dictionary (scoring callbacks, image.py:202-225)."""
        return self.dict_fact_._backend.stage_X(self._prep(patches))

    def score_staged(self, staged):
        return self.dict_fact_.score(staged)

    @property
    def n_iter_(self):
        return self.dict_fact_.n_iter_

    @property
    def time_(self):
        return self.dict_fact_.time_

    @property
    def components_(self):
        return self.dict_fact_.components_.reshape((self.n_components,) + tuple(self.patch_shape_))

    def _callback(self, *args):
        if self.callback is not None:
            self.callback(self)


class DictionaryScorer:
    """image.py:202-225 (time.clock is gone from Python 3.8: perf_counter)."""

    def __init__(self, test_data, info=None):
        self.start_time = time.perf_counter()
        self.test_data = test_data
        self.test_time = 0
        self.time, self.cpu_time, self.score, self.iter = [], [], [], []
        self.info = info

    def __call__(self, dict_fact):
        t0 = time.perf_counter()
        if hasattr(dict_fact, 'stage_test_patches'):
            # the test set is scaled and uploaded once per (estimator, setting); every later call scores it in HBM
            key = (id(dict_fact), getattr(dict_fact, 'setting', None))
            if getattr(self, '_staged_key', None) != key:
                self._staged, self._staged_key = dict_fact.stage_test_patches(self.test_data), key
            score = dict_fact.score_staged(self._staged)
        else:
            score = dict_fact.score(self.test_data)
        self.test_time += time.perf_counter() - t0
        self.time.append(time.perf_counter() - self.start_time - self.test_time)
        self.score.append(score)
        self.iter.append(dict_fact.n_iter_)
        self.cpu_time.append(dict_fact.time_)
        if self.info is not None:
            self.info['time'], self.info['score'], self.info['iter'] = self.cpu_time, self.score, self.iter
