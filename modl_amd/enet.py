"""Drop-in for modl/utils/math/enet.pyx (enet_norm :125, enet_projection :38,
enet_scale :150) on the GPU; 1-D vectors or, batched, the rows of a 2-D array."""
import numpy as np
import torch

from .device import STREAM, call, default_device, np_dtype_of, to_device


def _dt(a):
    return a.dtype if isinstance(a, np.ndarray) else np_dtype_of(a)


def enet_norm(v, l1_ratio):
    dev = default_device()
    dv = to_device(v, dev)
    rows = 1 if dv.dim() == 1 else dv.shape[0]
    n = dv.shape[-1]
    out = torch.empty(rows, dtype=dv.dtype, device=dev)
    call('modl_enet_norm', dv, rows, n, n, 1, l1_ratio, out, STREAM, device=dev, dtype=_dt(v))
    res = out.cpu().numpy()
    return float(res[0]) if dv.dim() == 1 else res


def enet_projection(v, out, radius, l1_ratio):
    dev = default_device()
    dv = to_device(v, dev)
    rows = 1 if dv.dim() == 1 else dv.shape[0]
    n = dv.shape[-1]
    dout = torch.empty_like(dv)
    rad = to_device(np.broadcast_to(np.asarray(radius, dtype=_dt(v)), (rows,)).copy(), dev)
    call('modl_enet_projection', dv, dout, rows, n, n, 1, rad, l1_ratio, STREAM, device=dev, dtype=_dt(v))
    if isinstance(out, np.ndarray):
        out[...] = dout.cpu().numpy()
    else:
        out.copy_(dout)


def enet_scale(X, l1_ratio, radius=1):
    dev = default_device()
    dv = to_device(X, dev)
    if isinstance(X, torch.Tensor) and dv.data_ptr() != X.data_ptr():
        raise ValueError('enet_scale works in place: pass a contiguous device tensor or a numpy array')
    rows = 1 if dv.dim() == 1 else dv.shape[0]
    n = dv.shape[-1]
    call('modl_enet_scale', dv, rows, n, n, 1, l1_ratio, radius, STREAM, device=dev, dtype=_dt(X))
    if isinstance(X, np.ndarray):
        X[...] = dv.cpu().numpy()
