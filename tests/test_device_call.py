"""modl_amd.device.call / scratch: the one way the Python side calls libmodl_hip.

CPU: a fake library whose entry points record what they were given (suffix, argument conversion, error text, the
STREAM rule).  GPU: two real entry points through `call` - modl_transpose_* (stream last) and modl_amari_* (stream
before the last argument, a count returned through byref) - and, where two devices are visible, a recsys backend on
the device that is not current."""
import ctypes as C

import numpy as np
import pytest
import torch

from modl_amd._lib import ModlError
from modl_amd.device import STREAM, call, scratch, sfx


class FakeLib:
    """every attribute is an entry point that records its arguments and returns `rc`"""

    def __init__(self, rc=0):
        self.rc, self.calls = rc, []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return self.rc
        return entry


# ---- CPU ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype,name', [(np.float32, 'modl_x_f32'), (np.dtype(np.float64), 'modl_x_f64'),
                                        (torch.float64, 'modl_x_f64'), (torch.float32, 'modl_x_f32'),
                                        (torch.zeros(2, dtype=torch.float32), 'modl_x_f32'),
                                        (torch.zeros(2, dtype=torch.float64), 'modl_x_f64'), (None, 'modl_x')])
def test_suffix(dtype, name):
    fake = FakeLib()
    call('modl_x', 1, device=None, dtype=dtype, lib=fake)
    assert [c[0] for c in fake.calls] == [name]


def test_suffix_rejects_other_dtypes():
    for bad in (np.int32, torch.int32, torch.zeros(2, dtype=torch.uint8)):
        with pytest.raises(TypeError, match='float32 or float64 expected'):
            sfx(bad)


def test_argument_conversion():
    fake = FakeLib()
    t = torch.arange(6, dtype=torch.float32)
    a = np.arange(4, dtype=np.int64)
    n = C.c_int(0)
    ref = C.byref(n)
    arr = (C.c_void_p * 2)(1, 2)
    call('modl_x', t, None, a, 7, 2.5, ref, arr, t[2:], device=None, lib=fake)
    (_, got), = fake.calls
    assert isinstance(got[0], C.c_void_p) and got[0].value == t.data_ptr()
    assert isinstance(got[1], C.c_void_p) and not got[1].value                # a null pointer
    assert isinstance(got[2], C.c_void_p) and got[2].value == a.ctypes.data
    assert got[3] == 7 and type(got[3]) is int and got[4] == 2.5 and type(got[4]) is float
    assert got[5] is ref and got[6] is arr
    assert got[7].value == t.data_ptr() + 2 * t.element_size()                # a view: its own address


def test_return_code():
    call('modl_x', 1, device=None, lib=FakeLib(0))                            # silent
    with pytest.raises(ModlError, match=r'modl_x_f64 failed: .* \(code 1\)'):
        call('modl_x', 1, device=None, dtype=np.float64, lib=FakeLib(1))
    with pytest.raises(ModlError, match=r'modl_y failed'):
        call('modl_y', device=None, lib=FakeLib(2))


def test_stream_needs_a_device():
    fake = FakeLib()
    with pytest.raises(ValueError, match='modl_x_f32: STREAM needs a device'):
        call('modl_x', 1, STREAM, device=None, dtype=np.float32, lib=fake)
    assert fake.calls == []


def test_scratch_size():
    for nbytes, size in ((0, 8), (1, 8), (8, 8), (9, 9), (np.int64(4096), 4096)):
        t = scratch(nbytes, 'cpu')
        assert t.dtype == torch.uint8 and t.numel() == size


# ---- GPU ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_scratch_has_an_address():
    t = scratch(0, torch.device('cuda', torch.cuda.current_device()))
    assert t.is_cuda and t.numel() == 8 and t.data_ptr() != 0


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_transpose_through_call(dtype):
    src = torch.arange(15, dtype=dtype, device='cuda').reshape(3, 5)
    out = torch.empty((5, 3), dtype=dtype, device=src.device)
    call('modl_transpose', src, out, 3, 5, STREAM, device=src.device, dtype=src)
    assert torch.equal(out, src.T)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_amari_launch_count_through_byref(dtype):
    """the stream is not the last argument of modl_amari_*; the pair of test_stability.test_signed_maximum_gpu"""
    from modl_amd._lib import lib
    from modl_amd.device import dtype_id
    device = torch.device('cuda', torch.cuda.current_device())
    A = np.eye(3, 5).astype(dtype)
    tensors = [torch.from_numpy(A).to(device), torch.from_numpy(-A).to(device)]
    ptrs = (C.c_void_p * 2)(*[t.data_ptr() for t in tensors])
    ks = np.array([3, 3], dtype=np.int64)
    nbytes = lib.modl_amari_workspace(dtype_id(dtype), 2, ks.ctypes.data_as(C.c_void_p), 5)
    assert nbytes > 0
    ws = scratch(nbytes, device)
    d = torch.empty(1, dtype=torch.float64, device=device)
    launches = C.c_int(0)
    call('modl_amari', ptrs, ks, 2, 5, d, None, None, ws, nbytes, STREAM, C.byref(launches), device=device, dtype=dtype)
    assert launches.value == 3                                                # (unsplit products: three kernels)
    assert float(d.cpu()[0]) == 1.0


@pytest.mark.gpu
@pytest.mark.skipif(torch.cuda.device_count() < 2, reason='needs two visible devices')
def test_recsys_topn_on_the_device_that_is_not_current():
    """a backend built with device='cuda:1' while cuda:0 is current launches on cuda:1: its top items are those of the
    same backend on cuda:0.  p = 5, k = 3, 2 rows, n_top = 2: the smallest shape tests/test_recsys_recommend.py
    writes out (the ABI matrix's minimum p = k = 1 has one item and could not tell two answers apart)."""
    import scipy.sparse as sp
    from modl_amd.recsys import _RecsysDevice
    rs = np.random.RandomState(0)
    X = sp.csr_matrix(rs.rand(2, 5).astype(np.float32))
    D, code = rs.randn(3, 5).astype(np.float32), rs.randn(2, 3).astype(np.float32)
    items = []
    with torch.cuda.device(0):
        for index in (0, 1):
            be = _RecsysDevice(X, 3, np.float32, device='cuda:%d' % index)
            be.set_dictionary(D)
            got = be.topn(torch.from_numpy(code).to(be.device), None, None, None, None, 2)
            assert got.device == be.device and torch.cuda.current_device() == 0
            items.append(got.cpu().numpy())
    assert items[0].shape == (2, 2) and np.array_equal(items[0], items[1])
