"""Stability of dictionaries across runs: the Amari discrepancy.

Port of modl/decomposition/stability.py:7-31 (`amari_discrepency`, `mean_amari_discrepency`, the reference's
spelling).  Every pair of a list is evaluated by ONE call of libmodl_hip (modl_amari_f32 / _f64: three kernel
launches, four when the products are split along the features, whatever the number of dictionaries); torch only
holds device memory.  The mean and the standard deviation over the n (n - 1) / 2 pair values are taken on the host,
with numpy, as the reference does.

Inputs are numpy arrays (memmaps included) or torch tensors of shape (n_components, n_features).  Host inputs are
copied to the device once per call, one copy per dictionary; a C-contiguous CUDA tensor of the computing dtype is used
in place.  All float32 -> float32 products (the reference's sgemm), anything else -> float64, as numpy promotes.
"""
import ctypes as C

import numpy as np
import torch

from . import device as dev
from ._lib import lib

__all__ = ['amari_discrepency', 'mean_amari_discrepency']


def _is_f32(D):
    if isinstance(D, torch.Tensor):
        return D.dtype == torch.float32
    return np.asarray(D).dtype == np.float32


def _shape(D):
    return tuple(D.shape) if isinstance(D, torch.Tensor) else np.shape(D)


def _check(dictionaries):
    shapes = [_shape(D) for D in dictionaries]
    for s in shapes:
        if len(s) != 2:
            raise ValueError('a dictionary must be 2-D (n_components, n_features), got shape %s' % (s,))
        if s[0] == 0 or s[1] == 0:
            raise ValueError('empty dictionary of shape %s' % (s,))
    ps = {s[1] for s in shapes}
    if len(ps) != 1:
        raise ValueError('dictionaries have different numbers of features: %s' % sorted(ps))
    return shapes


def _result_type(np_dtype):
    """the type of the reference's return value for inputs of this dtype, under the installed numpy"""
    z = np.zeros((1, 1), np_dtype)
    return type(.5 * (np.mean(1 - z.max(axis=0)) + np.mean(1 - z.max(axis=1))))


def _stage(D, np_dtype, device):
    tdt = dev.torch_dtype(np_dtype)
    if isinstance(D, torch.Tensor):
        if D.device == device and D.dtype == tdt and D.is_contiguous():
            return D                                          # used in place
        return D.detach().to(device=device, dtype=tdt).contiguous()
    a = np.ascontiguousarray(D, dtype=np_dtype)               # no host copy for a contiguous array of the right dtype
    return torch.from_numpy(a).to(device)


def amari_pairs(dictionaries, maxima=False):
    """Every pair (a < b, a outer) of `dictionaries` on the GPU.  Returns a dict with
    'd' (float64 numpy array of the n (n - 1) / 2 discrepancies), 'dtype' (the computing dtype), 'launches' (kernels
    launched) and, with maxima=True, 'rowmax' / 'colmax': per pair, max_j C[i, j] (length k_a) and max_i C[i, j]
    (length k_b), numpy arrays of the computing dtype."""
    dictionaries = list(dictionaries)
    if len(dictionaries) < 2:
        raise ValueError('at least two dictionaries are needed')
    shapes = _check(dictionaries)
    np_dtype = np.dtype(np.float32) if all(_is_f32(D) for D in dictionaries) else np.dtype(np.float64)
    device = dev.default_device()
    n, p = len(dictionaries), int(shapes[0][1])
    ks = np.array([s[0] for s in shapes], dtype=np.int64)
    ws_bytes = lib.modl_amari_workspace(dev.dtype_id(np_dtype), n, ks.ctypes.data_as(C.c_void_p), p)
    if ws_bytes == 0:
        raise ValueError('modl_amari_workspace rejected n=%d, p=%d, k=%s' % (n, p, ks.tolist()))
    npairs = n * (n - 1) // 2
    pair_ks = [(int(ks[a]), int(ks[b])) for a in range(n - 1) for b in range(a + 1, n)]
    n_row = sum(ka for ka, _ in pair_ks) if maxima else 0
    n_col = sum(kb for _, kb in pair_ks) if maxima else 0
    staged = sum(int(k) * p * np_dtype.itemsize for k, D in zip(ks, dictionaries)
                 if not (isinstance(D, torch.Tensor) and D.device == device))
    need = staged + ws_bytes + (n_row + n_col) * np_dtype.itemsize + 8 * npairs
    free, total = torch.cuda.mem_get_info(device)
    if need > free:
        raise MemoryError('mean_amari_discrepency: the staged dictionaries and the workspace need %.2f GB of device '
                          'memory, %.2f GB of %.2f GB are free; there is no CPU path'
                          % (need / 1e9, free / 1e9, total / 1e9))
    tensors = [_stage(D, np_dtype, device) for D in dictionaries]
    ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in tensors])
    ws = dev.scratch(ws_bytes, device)
    d_pair = torch.empty(npairs, dtype=torch.float64, device=device)
    tdt = dev.torch_dtype(np_dtype)
    rowmax = torch.empty(n_row, dtype=tdt, device=device) if maxima else None
    colmax = torch.empty(n_col, dtype=tdt, device=device) if maxima else None
    launches = C.c_int(0)
    dev.call('modl_amari', ptrs, ks, n, p, d_pair, rowmax, colmax, ws, ws_bytes, dev.STREAM, C.byref(launches),
             device=device, dtype=np_dtype)
    out = {'d': d_pair.cpu().numpy(), 'dtype': np_dtype, 'launches': launches.value}
    if maxima:
        rm, cm = rowmax.cpu().numpy(), colmax.cpu().numpy()
        ro = np.cumsum([0] + [ka for ka, _ in pair_ks])
        co = np.cumsum([0] + [kb for _, kb in pair_ks])
        out['rowmax'] = [rm[ro[q]:ro[q + 1]] for q in range(npairs)]
        out['colmax'] = [cm[co[q]:co[q + 1]] for q in range(npairs)]
    del tensors
    return out


def amari_discrepency(D1, D2):
    """Amari discrepancy of two dictionaries (stability.py:7-22).

    D1: (n_components_1, n_features), D2: (n_components_2, n_features); returns
    0.5 * (mean_j (1 - max_i C[i, j]) + mean_i (1 - max_j C[i, j])) with C the cosines of the atoms (signed).
    NaN (a zero atom, a NaN in an input) propagates as in numpy.
    """
    r = amari_pairs([D1, D2])
    return _result_type(r['dtype'])(r['d'][0])


def mean_amari_discrepency(dictionaries, n_jobs=1):
    """Mean and (population) standard deviation of the Amari discrepancy over every pair of `dictionaries`
    (stability.py:25-31).  `n_jobs` is accepted for the reference's signature and ignored: all pairs are one GPU call.
    Fewer than two dictionaries give (nan, nan) with numpy's RuntimeWarning, as the reference does."""
    dictionaries = list(dictionaries)
    if len(dictionaries) < 2:
        ds = np.array([])
        return np.mean(ds), np.std(ds)
    r = amari_pairs(dictionaries)
    rtype = _result_type(r['dtype'])
    ds = np.array([rtype(v) for v in r['d']])
    return np.mean(ds), np.std(ds)
