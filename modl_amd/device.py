"""Device plumbing: torch is used for device memory, streams and (optionally)
torch.distributed only; all arithmetic runs in libmodl_hip.so."""
import ctypes as C

import numpy as np
import torch

from ._lib import lib, check, require_gpu, MODL_F32, MODL_F64

_TORCH_DT = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}
STREAM = object()              # stands for the device's current stream in the arguments of call()


def dtype_id(dtype):
    """MODL_F32 / MODL_F64 of a numpy dtype, a torch dtype or a tensor"""
    if isinstance(dtype, torch.Tensor):
        dtype = dtype.dtype
    if dtype in (torch.float32, torch.float64):
        return MODL_F32 if dtype == torch.float32 else MODL_F64
    if not isinstance(dtype, torch.dtype):
        dtype = np.dtype(dtype)
        if dtype == np.float32:
            return MODL_F32
        if dtype == np.float64:
            return MODL_F64
    raise TypeError('float32 or float64 expected, got %s' % dtype)


def sfx(dtype):
    """'f32' / 'f64' of a numpy dtype, a torch dtype or a tensor"""
    return 'f32' if dtype_id(dtype) == MODL_F32 else 'f64'


def torch_dtype(np_dtype):
    return _TORCH_DT[np.dtype(np_dtype)]


def np_dtype_of(t):
    return np.dtype(np.float32) if t.dtype == torch.float32 else np.dtype(np.float64)


def have_gpu():
    return lib.modl_device_count() > 0


def current_device():
    return torch.device('cuda', torch.cuda.current_device())


def default_device():
    require_gpu()
    return current_device()


def stream_ptr(device=None):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _arg(a, stream):
    if a is STREAM:
        return stream
    if a is None:
        return C.c_void_p(0)
    if isinstance(a, torch.Tensor):
        return C.c_void_p(a.data_ptr())
    if isinstance(a, np.ndarray):
        return C.c_void_p(a.ctypes.data)
    return a


def call(name, *args, device, dtype=None, lib=lib):
    """lib.<name>[_f32|_f64](*args) with `device` current and STREAM replaced by that device's current stream; ModlError
    when it does not return 0.  `dtype` (a numpy dtype, a torch dtype or a tensor) picks the suffix.  Tensors and numpy
    arrays are passed as their addresses, None as a null pointer, anything else as it is.  device=None (host-only entry
    points): no device is made current and STREAM may not be used."""
    if dtype is not None:
        name += '_' + sfx(dtype)
    f = getattr(lib, name)
    if device is None:
        if any(a is STREAM for a in args):
            raise ValueError('%s: STREAM needs a device' % name)
        rc = f(*[_arg(a, None) for a in args])
    else:
        with torch.cuda.device(device):
            stream = stream_ptr(device)
            rc = f(*[_arg(a, stream) for a in args])
    check(rc, name)


def scratch(nbytes, device):
    """uint8 device tensor of max(nbytes, 8) bytes (an empty tensor has no address)"""
    return torch.empty(max(int(nbytes), 8), dtype=torch.uint8, device=device)


def is_cuda(a):
    if isinstance(a, torch.Tensor):
        if not a.is_cuda:
            raise ValueError('a numpy array or a CUDA tensor is expected, got a tensor on %s' % a.device)
        return True
    return False


def as_float_tensor(a, device=None, dtype=None):
    """a float tensor of a numpy array (copied to `device`, by default the current one) or of a tensor (which stays where
    it is): float32 / float64 as given, anything else as float64, then cast to `dtype` if one is given"""
    if isinstance(a, torch.Tensor):
        if a.dtype not in (torch.float32, torch.float64):
            a = a.to(torch.float64)
    else:
        a = np.asarray(a)
        if a.dtype not in (np.float32, np.float64):
            a = a.astype(np.float64)
        a = torch.from_numpy(np.ascontiguousarray(a)).to(device or current_device())
    return a if dtype is None else a.to(dtype)


def like_input(t, cuda):
    """a result as the caller passed its input: the CUDA tensor, or a numpy array"""
    return t if cuda else t.cpu().numpy()


def to_device(a, device, dtype=None):
    """numpy array / torch tensor -> contiguous device tensor (no copy if already there)."""
    if isinstance(a, torch.Tensor):
        t = a
        if dtype is not None and t.dtype != torch_dtype(dtype):
            t = t.to(torch_dtype(dtype))
        if t.device != device:
            t = t.to(device)
        return t.contiguous()
    a = np.ascontiguousarray(a, dtype=dtype)
    return torch.from_numpy(a).to(device)


def transpose_to(src, rows, cols):
    """out[c][r] = src[r][c] on the device (components_ <-> feature-major Dt)."""
    out = torch.empty((cols, rows), dtype=src.dtype, device=src.device)
    call('modl_transpose', src, out, rows, cols, STREAM, device=src.device, dtype=src)
    return out


def gather_rows(src, perm):
    """src[perm] for a 2-D device tensor with contiguous rows, by the library's gather kernel."""
    idx = torch.from_numpy(np.ascontiguousarray(perm, dtype=np.int64)).to(src.device)
    out = torch.empty((idx.shape[0], src.shape[1]), dtype=src.dtype, device=src.device)
    call('modl_gather_rows', src, src.stride(0), idx, idx.shape[0], src.shape[1], out, out.stride(0), STREAM,
         device=src.device, dtype=src)
    return out
