"""Sparse codes as CSR: compaction of dense codes on the device (modl_csr_count_* / modl_csr_fill_*), the
product of CSR codes with the dictionary (modl_csr_decode_*), and `transform(..., sparse=True)` / `inverse_transform` of
sparse codes on DictFact and Coder.  The yardstick is scipy.

Layer 1 (no GPU): a numpy restatement of count / scan / fill and of the decode is compared with
scipy.sparse.csr_matrix(dense) and csr @ D; the judges the GPU tests use reject a list of mutants of the restatement; the
entry points refuse bad arguments before any device work; the estimators raise ValueError without a device.

The judge of a compaction is exact: indptr, indices and the BITS of data.  The judge of a decode is the bound
|out - ref| <= (m_i + 1) u sum_j |data_j| |D[idx_j][e]| with ref in np.longdouble, m_i the row's entry count and u = 2^-24
(f32) or 2^-53 (f64); it holds for any order of the sum, fused or not.

Mutants the cases cannot see: none of the listed ones.  Not listed, and invisible by construction: a decode that sums a
row's entries in another fixed order (the bound holds for every order; what the kernel promises instead - the same bits
for the same row in any batch - is tested on the device), and a compaction that differs only in what it writes beyond nnz
or into the padding of indptr (the GPU tests guard those with sentinels).

Layer 2 (GPU): the kernels through the ABI on shapes around the 64-lane step, the four rows of a workgroup, the 1024-row
scan tile and the 256 tiles of one round of the tile-sum scan; the estimators' slice contract, memory cap and round trip.
"""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

DT = {'f32': np.float32, 'f64': np.float64}
UINT = {'f32': np.uint32, 'f64': np.uint64}
U_ROUND = {'f32': 2.0 ** -24, 'f64': 2.0 ** -53}
EINVAL, ENOMEM, ENOGPU = -1, -2, -4
BIG_BASE = 2 ** 31 + 7


def dt_of(a):
    return 'f32' if a.dtype == np.float32 else 'f64'


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(UINT[dt_of(a)])


# ------------------------------------------------------------------------------------------- the restatement (numpy)
def keep(a, mutant=None):
    """the keep rule on the bits: sign cleared, anything left"""
    u = bits(a)
    sign = u.dtype.type(1) << u.dtype.type(8 * u.dtype.itemsize - 1)
    if mutant == 'gt0':
        with np.errstate(invalid='ignore'):
            return a > 0
    if mutant == 'neg_zero_kept':
        return u != 0
    if mutant == 'denormal_dropped':
        mant = 23 if a.dtype == np.float32 else 52
        return ((u & ~sign) >> u.dtype.type(mant)) != 0
    if mutant == 'nan_dropped':
        return ((u & ~sign) != 0) & ~np.isnan(a)
    return (u & ~sign) != 0


def restate_compact(padded, k, base, mutant=None):
    """count / scan / fill of a dense chunk padded[b][ld], ld >= k: (indptr int64, indices int32, data)"""
    b = padded.shape[0]
    dense = padded if mutant == 'padding_read' else padded[:, :k]
    m = keep(dense, mutant)
    if mutant == 'last_col_dropped':
        m[:, k - 1] = False
    if mutant == 'last_row_dropped':
        m[b - 1] = False
    counts = m.sum(axis=1).astype(np.int64)                                  # count
    indptr = np.empty(b + 1, dtype=np.int64)                                # scan
    indptr[0] = 0 if mutant == 'base_ignored' else base
    indptr[1:] = indptr[0] + np.cumsum(counts)
    if mutant == 'indptr_after_empty':
        empty = np.flatnonzero(counts == 0)
        if len(empty):
            indptr[empty[0] + 1:] += 1
    nnz = int(counts.sum())
    indices, data = np.zeros(nnz, dtype=np.int32), np.zeros(nnz, dtype=padded.dtype)
    start = np.concatenate([[0], np.cumsum(counts)])
    for r in range(b):                                                      # fill
        cols = np.flatnonzero(m[r])
        if mutant == 'descending':
            cols = cols[::-1]
        indices[start[r]:start[r + 1]] = cols
        data[start[r]:start[r + 1]] = dense[r, cols]
    return indptr, indices, data


def restate_decode(indptr, indices, data, Dt, n, mutant=None):
    """out[i][e] = sum_j data[j] Dt[e][indices[j]] in stored order, in the dtype; corrupt rows and entries contribute
    nothing and raise the status: (out, status)"""
    p, k = Dt.shape
    D = Dt.ravel().reshape(k, p) if mutant == 'Dt_atom_major' else Dt.T
    out, status, nnz = np.zeros((n, p), dtype=Dt.dtype), 0, len(data)
    for i in range(n):
        r = min(i + 1, n - 1) if mutant == 'neighbour_indptr' else i
        lo, hi = int(indptr[r]), int(indptr[r + 1])
        if lo < 0 or hi < lo or hi > nnz:
            status = 1
            continue
        seen = set()
        for j in range(lo, hi):
            a = int(indices[j])
            if a < 0 or a >= k:
                status = 1
                continue
            if mutant == 'skips_repeat' and a in seen:
                continue
            seen.add(a)
            out[i] = out[i] + data[j] * D[a]
    return out, status


COMPACT_MUTANTS = ('gt0', 'neg_zero_kept', 'denormal_dropped', 'nan_dropped', 'last_col_dropped', 'last_row_dropped',
                   'base_ignored', 'indptr_after_empty', 'descending', 'padding_read')
DECODE_MUTANTS = ('skips_repeat', 'neighbour_indptr', 'Dt_atom_major')


# ------------------------------------------------------------------------------------------------------ the judges
def scipy_compact(padded, k):
    ref = sp.csr_matrix(np.ascontiguousarray(padded[:, :k]))
    assert ref.has_canonical_format
    return ref


def judge_compact(ref, base, got):
    """exact: indptr, indices and the bits of data against scipy's csr_matrix(dense); ref = scipy_compact(...)"""
    indptr, indices, data = got
    assert indptr.dtype == np.int64 and indices.dtype == np.int32 and data.dtype == ref.data.dtype
    np.testing.assert_array_equal(indptr, base + ref.indptr.astype(np.int64))
    np.testing.assert_array_equal(indices, ref.indices)
    np.testing.assert_array_equal(bits(data), bits(ref.data))


def decode_reference(indptr, indices, data, Dt, n):
    """(ref, bound) in np.longdouble; corrupt rows and entries left out as the kernel leaves them out"""
    p, k = Dt.shape
    L = np.longdouble
    DL = np.ascontiguousarray(Dt.T).astype(L)
    ref, bound, u = np.zeros((n, p), dtype=L), np.zeros((n, p), dtype=L), L(U_ROUND[dt_of(Dt)])
    for i in range(n):
        lo, hi = int(indptr[i]), int(indptr[i + 1])
        if lo < 0 or hi < lo or hi > len(data):
            continue
        idx = np.asarray(indices[lo:hi], dtype=np.int64)
        ok = (idx >= 0) & (idx < k)
        terms = data[lo:hi][ok].astype(L)[:, None] * DL[idx[ok]]
        ref[i] = terms.sum(axis=0)
        bound[i] = (hi - lo + 1) * u * np.abs(terms).sum(axis=0)
    return ref, bound


def judge_decode(indptr, indices, data, Dt, n, out):
    """the largest |out - ref| / bound (0 / 0 = 0); asserts it is <= 1"""
    ref, bound = decode_reference(indptr, indices, data, Dt, n)
    assert out.shape == ref.shape and out.dtype == Dt.dtype
    err = np.abs(out.astype(np.longdouble) - ref)
    assert np.all(err <= bound), 'decode misses the bound by up to %.3g (absolute)' % float(np.max(err - bound))
    with np.errstate(invalid='ignore', divide='ignore'):
        return float(np.nanmax(np.where(bound > 0, err / bound, 0), initial=0.0))


def rejects(check, *args):
    try:
        check(*args)
    except AssertionError:
        return True
    return False


# ------------------------------------------------------------------------------------------------------- the cases
PATTERNS = ('zero', 'full', 'd001', 'd03', 'col0', 'col_last', 'alt_rows', 'neg_zero_row', 'denormal', 'nan', 'inf')


def make_dense(dt, b, k, pattern, seed=0):
    T = DT[dt]
    rs = np.random.RandomState(seed)
    vals = rs.randn(b, k).astype(T)
    vals[vals == 0] = 1
    d03 = np.where(rs.rand(b, k) < 0.3, vals, T(0))
    d03[rs.rand(b, k) < 0.05] = T(-0.0)
    r, tiny = b // 2, np.finfo(T).smallest_subnormal
    if pattern == 'zero':
        a = np.zeros((b, k), dtype=T)
    elif pattern == 'full':
        a = vals
    elif pattern == 'd001':
        a = np.where(rs.rand(b, k) < 0.01, vals, T(0))
    elif pattern == 'd03':
        a = d03
    elif pattern in ('col0', 'col_last'):
        a = np.zeros((b, k), dtype=T)
        c = 0 if pattern == 'col0' else k - 1
        a[:, c] = vals[:, c]
    elif pattern == 'alt_rows':
        a = vals
        a[0::2] = 0
    elif pattern == 'neg_zero_row':
        a = d03
        a[r] = T(-0.0)
    elif pattern == 'denormal':
        a = d03
        a[r, k // 2], a[0, 0], a[b - 1, k - 1] = tiny, -tiny, tiny
    elif pattern == 'nan':
        a = d03
        a[r, k - 1], a[0, 0] = np.nan, -np.nan
    elif pattern == 'inf':
        a = d03
        a[r, 0], a[b - 1, k - 1] = np.inf, -np.inf
    else:
        raise KeyError(pattern)
    return np.ascontiguousarray(a, dtype=T)


def pad(a, extra):
    """a[b][k] inside a[b][k + extra], NaN in the padding"""
    out = np.full((a.shape[0], a.shape[1] + extra), np.nan, dtype=a.dtype)
    out[:, :a.shape[1]] = a
    return out


def hand_compact(dt):
    """(padded, k, base, indptr, indices, data) worked by hand: ld = k + 1 with NaN behind, an empty row in the middle,
    -0.0, a negative value, NaN, a denormal, -inf, the last column of the last row"""
    T = DT[dt]
    tiny = np.finfo(T).smallest_subnormal
    a = np.array([[0, 1.5, -0.0, 0, -2],
                  [0, -0.0, 0, 0, 0],
                  [np.nan, 0, tiny, -np.inf, 0],
                  [0, 0, 0, 0, 7]], dtype=T)
    return (pad(a, 1), 5, 10, np.array([10, 12, 12, 15, 16], dtype=np.int64), np.array([1, 4, 0, 2, 3, 4], dtype=np.int32),
            np.array([1.5, -2, np.nan, tiny, -np.inf, 7], dtype=T))


def hand_decode(dt):
    """(indptr, indices, data, Dt, n, out) worked by hand: D = [[1, 2], [3, 4], [5, 6]] (atoms in rows), a repeated and
    unsorted row, an empty row"""
    T = DT[dt]
    Dt = np.array([[1, 3, 5], [2, 4, 6]], dtype=T)
    return (np.array([0, 3, 3, 4], dtype=np.int64), np.array([2, 0, 2, 1], dtype=np.int32),
            np.array([1.0, 2.0, 0.5, -1.0], dtype=T), Dt, 3, np.array([[9.5, 13], [0, 0], [-3, -4]], dtype=T))


def random_csr(dt, n, k, p, seed=0, counts=None):
    """unsorted indices with repeats; row i has counts[i % len(counts)] entries"""
    T = DT[dt]
    rs = np.random.RandomState(seed)
    counts = [(65, 0, 1, 64, k)[i % 5] for i in range(n)] if counts is None else [counts[i % len(counts)] for i in range(n)]
    indptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    indices = rs.randint(0, k, size=int(indptr[-1])).astype(np.int32)
    for i in range(n):
        if counts[i] >= 2:
            indices[indptr[i] + 1] = indices[indptr[i]]                    # a repeat, side by side
            if counts[i] >= 3:
                indices[indptr[i + 1] - 1] = indices[indptr[i]]            # and one far away
    data = rs.randn(len(indices)).astype(T)
    Dt = np.ascontiguousarray(rs.randn(p, k).astype(T))
    return indptr, indices, data, Dt


# ------------------------------------------------------------------------------------------------- layer 1: no GPU
@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_restatement_against_scipy(dt):
    padded, k, base, indptr, indices, data = hand_compact(dt)
    got = restate_compact(padded, k, base)
    np.testing.assert_array_equal(got[0], indptr)
    np.testing.assert_array_equal(got[1], indices)
    np.testing.assert_array_equal(bits(got[2]), bits(data))
    judge_compact(scipy_compact(padded, k), base, got)
    for b, k, extra, base in ((1, 1, 0, 0), (7, 65, 3, BIG_BASE), (33, 130, 0, 5), (5, 64, 3, 0)):
        for pattern in PATTERNS:
            padded = pad(make_dense(dt, b, k, pattern, seed=b + k), extra)
            judge_compact(scipy_compact(padded, k), base, restate_compact(padded, k, base))
    ip, ix, dv, Dt, n, out = hand_decode(dt)
    got, status = restate_decode(ip, ix, dv, Dt, n)
    np.testing.assert_array_equal(got, out)
    assert status == 0 and judge_decode(ip, ix, dv, Dt, n, got) == 0.0
    for n, k, p in ((1, 1, 1), (9, 7, 33), (6, 70, 5)):
        ip, ix, dv, Dt = random_csr(dt, n, k, p, seed=n)
        got, status = restate_decode(ip, ix, dv, Dt, n)
        assert status == 0
        print('%s restated decode (%d, %d, %d): %.3g of the bound' % (dt, n, k, p, judge_decode(ip, ix, dv, Dt, n, got)))
        # scipy's own product (it sums duplicates first, in its own order): inside the same bound
        csr = sp.csr_matrix((dv, ix, ip), shape=(n, k))
        judge_decode(ip, ix, dv, Dt, n, np.asarray(csr @ np.ascontiguousarray(Dt.T), dtype=DT[dt]))


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_judges_reject_mutants(dt):
    padded, k, base = hand_compact(dt)[:3]
    cases = [(padded, k, base)] + [(pad(make_dense(dt, 9, 66, pattern, seed=3), 2), 66, 77) for pattern in PATTERNS]
    for mutant in COMPACT_MUTANTS:
        seen = [rejects(judge_compact, scipy_compact(c[0], c[1]), c[2], restate_compact(*c, mutant=mutant)) for c in cases]
        assert seen[0], 'the case worked by hand does not see the mutant %r' % mutant
        assert any(seen[1:]), 'no random case sees the mutant %r' % mutant
    ip, ix, dv, Dt, n, _ = hand_decode(dt)
    rnd = random_csr(dt, 9, 7, 33, seed=1)
    for mutant in DECODE_MUTANTS:
        assert rejects(judge_decode, ip, ix, dv, Dt, n, restate_decode(ip, ix, dv, Dt, n, mutant)[0]), mutant
        assert rejects(judge_decode, *rnd[:3], rnd[3], 9, restate_decode(*rnd, 9, mutant)[0]), mutant
    # and the corrupt inputs of the GPU test mean what they say in the restatement
    for bad_ix, bad_ip in ((np.array([2, 3, 2, 1], dtype=np.int32), ip), (np.array([2, 0, -1, 1], dtype=np.int32), ip),
                           (ix, np.array([0, 3, 2, 4], dtype=np.int64))):
        out, status = restate_decode(bad_ip, bad_ix, dv, Dt, n)
        assert status == 1
        judge_decode(bad_ip, bad_ix, dv, Dt, n, out)


def _hp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def test_entry_points_refuse_before_any_device_work():
    """host arrays stand in for device buffers: nothing reads them"""
    from modl_amd._lib import lib
    no_gpu = lib.modl_device_count() <= 0
    q = np.zeros(4096)
    assert lib.modl_csr_compact_workspace(-1) == 0
    sizes = [lib.modl_csr_compact_workspace(b) for b in list(range(0, 3000)) + [10 ** 6, 2 ** 31 - 1]]
    assert min(sizes) > 0 and all(a <= b for a, b in zip(sizes, sizes[1:]))
    for dtype_id, es in ((0, 4), (1, 8)):
        assert lib.modl_csr_decode_workspace(dtype_id, 7, 33) == 7 * 33 * es
        assert lib.modl_csr_decode_workspace(dtype_id, 0, 33) == 0 and lib.modl_csr_decode_workspace(dtype_id, 7, 0) == 0
    assert lib.modl_csr_decode_workspace(2, 7, 33) == 0
    for sx in ('f32', 'f64'):
        count, fill, decode = (getattr(lib, 'modl_csr_%s_%s' % (name, sx)) for name in ('count', 'fill', 'decode'))
        need = lib.modl_csr_compact_workspace(5)
        ok = dict(code=q, ld=9, b=5, k=7, base=3, indptr=q, ws=q, wsb=need)
        call = lambda a: count(_hp(a['code']), a['ld'], a['b'], a['k'], a['base'], _hp(a['indptr']), _hp(a['ws']), a['wsb'],
                               None)
        for bad in (dict(code=None), dict(indptr=None), dict(b=-1), dict(b=2 ** 31), dict(k=0), dict(k=-1), dict(k=2 ** 31),
                    dict(ld=6), dict(base=-1), dict(ws=None, k=0), dict(wsb=0, b=-1)):
            assert call(dict(ok, **bad)) == EINVAL, bad
        for bad in (dict(ws=None), dict(wsb=0), dict(wsb=need - 1)):
            assert call(dict(ok, **bad)) == ENOMEM, bad
        assert call(dict(ok, b=0)) == 0 and call(dict(ok, b=0, ws=None, wsb=0)) == 0
        ok = dict(code=q, ld=9, b=5, k=7, base=3, indptr=q, nnz=11, indices=q, data=q)
        call = lambda a: fill(_hp(a['code']), a['ld'], a['b'], a['k'], a['base'], _hp(a['indptr']), a['nnz'],
                              _hp(a['indices']), _hp(a['data']), None)
        for bad in (dict(code=None), dict(indptr=None), dict(indices=None), dict(data=None), dict(b=-1), dict(k=0),
                    dict(ld=6), dict(base=-1), dict(nnz=-1)):
            assert call(dict(ok, **bad)) == EINVAL, bad
        assert call(dict(ok, b=0)) == 0 and call(dict(ok, nnz=0)) == 0
        need = lib.modl_csr_decode_workspace(0 if sx == 'f32' else 1, 7, 33)
        ok = dict(indptr=q, indices=q, data=q, nnz=11, n=5, k=7, Dt=q, p=33, out=q, ldo=36, status=q, ws=q, wsb=need)
        call = lambda a: decode(_hp(a['indptr']), _hp(a['indices']), _hp(a['data']), a['nnz'], a['n'], a['k'], _hp(a['Dt']),
                                a['p'], _hp(a['out']), a['ldo'], _hp(a['status']), _hp(a['ws']), a['wsb'], None)
        for bad in (dict(indptr=None), dict(indices=None), dict(data=None), dict(Dt=None), dict(out=None), dict(nnz=-1),
                    dict(n=-1), dict(k=0), dict(k=2 ** 31), dict(p=0), dict(p=32 * 65535 + 1, ldo=2 ** 22), dict(ldo=32),
                    dict(ws=None, n=-1)):
            assert call(dict(ok, **bad)) == EINVAL, bad
        for bad in (dict(ws=None), dict(wsb=0), dict(wsb=need - 1)):
            assert call(dict(ok, **bad)) == ENOMEM, bad
        assert call(dict(ok, n=0)) == 0 and call(dict(ok, n=0, status=None, ws=None, wsb=0)) == 0
        if no_gpu:                                                            # a valid call gets as far as the device
            assert call(ok) == ENOGPU and call(dict(ok, status=None)) == ENOGPU


def test_bad_arguments_raise_valueerror_without_gpu():
    from modl_amd import DictFact, SparseCodes
    est = DictFact(n_components=7)
    X = np.zeros((5, 12))
    with pytest.raises(ValueError, match='rows_per_chunk belongs to sparse=True'):
        est.transform(X, rows_per_chunk=5)
    with pytest.raises(ValueError, match='rows_per_chunk belongs to sparse=True'):
        est.transform(X, mask=np.ones((5, 12), dtype=bool), algorithm='omp', rows_per_chunk=4096)
    for bad in (0, -3, 2.5):
        with pytest.raises(ValueError, match='rows_per_chunk must be'):
            est.transform(X, sparse=True, rows_per_chunk=bad)
    with pytest.raises(ValueError, match='mask'):
        est.transform(X, mask=np.ones((4, 12), dtype=bool), sparse=True)
    with pytest.raises(ValueError, match='algorithm'):
        est.transform(X, algorithm='lars', sparse=True)
    for wrong in (sp.csr_matrix((3, 6)), sp.csc_matrix((3, 8)), sp.coo_matrix(np.ones((2, 5)))):
        with pytest.raises(ValueError, match='7 components'):
            est.inverse_transform(wrong)
    with pytest.raises(ValueError, match='7 components'):
        est.inverse_transform(SparseCodes(np.zeros(4, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0), (3, 8)))
    for idx in (7, -1):
        out_of_range = sp.csr_matrix((np.ones(2), np.array([0, idx], dtype=np.int32), np.array([0, 1, 2, 2])), shape=(3, 7))
        with pytest.raises(ValueError, match=r'outside \[0, 7\)'):
            est.inverse_transform(out_of_range)


# -------------------------------------------------------------------------------------------------- layer 2: the GPU
@pytest.fixture(scope='module')
def gpu():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    return torch


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to('cuda')


GUARD = 8                                # sentinel elements behind every output
I_SENT, V_SENT = -77, 12345.0


def gpu_compact(d_code, k, base):
    """modl_csr_count_* then modl_csr_fill_* on the device tensor d_code (b, ld); asserts that nothing is written behind
    the b + 1 entries of indptr and the nnz entries of indices and data"""
    import torch
    from modl_amd._lib import lib
    from modl_amd.device import ptr
    sx = 'f32' if d_code.dtype == torch.float32 else 'f64'
    b, ld = d_code.shape[0], d_code.stride(0)
    indptr = torch.full((b + 1 + GUARD,), I_SENT, dtype=torch.int64, device='cuda')
    nbytes = lib.modl_csr_compact_workspace(b)
    ws = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
    assert getattr(lib, 'modl_csr_count_' + sx)(ptr(d_code), ld, b, k, base, ptr(indptr), ptr(ws), nbytes, None) == 0
    torch.cuda.synchronize()
    ip = indptr.cpu().numpy()
    assert np.all(ip[b + 1:] == I_SENT), 'written behind indptr'
    nnz = int(ip[b]) - base
    assert 0 <= nnz <= b * k
    indices = torch.full((nnz + GUARD,), I_SENT, dtype=torch.int32, device='cuda')
    data = torch.full((nnz + GUARD,), V_SENT, dtype=d_code.dtype, device='cuda')
    assert getattr(lib, 'modl_csr_fill_' + sx)(ptr(d_code), ld, b, k, base, ptr(indptr), nnz, ptr(indices), ptr(data), None) == 0
    torch.cuda.synchronize()
    ix, dv = indices.cpu().numpy(), data.cpu().numpy()
    assert np.all(ix[nnz:] == I_SENT) and np.all(dv[nnz:] == V_SENT), 'written behind nnz'
    return ip[:b + 1], ix[:nnz], dv[:nnz]


# every k and every b of the list once (small b with large k), the two pairs named apart, a scan of more than one tile
# (70 000 rows = 69 tiles) and one of more than one round of the tile-sum scan (300 000 rows = 293 tiles > 256)
COMPACT_SHAPES = ((1, 4096), (3, 1000), (4, 256), (5, 127), (255, 65), (257, 64), (1025, 63), (4097, 1), (4097, 65), (5, 4096),
                  (70000, 8), (300000, 1))


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'f64'])
@pytest.mark.parametrize('b,k', COMPACT_SHAPES, ids=['b%d-k%d' % s for s in COMPACT_SHAPES])
def test_compaction_through_the_abi(gpu, dt, b, k):
    for pattern in PATTERNS:
        a = make_dense(dt, b, k, pattern, seed=b + k)
        ref = scipy_compact(a, k)
        tight, padded = _dev(a), _dev(pad(a, 3))
        for d_code in (tight, padded):
            for base in (0, BIG_BASE):
                judge_compact(ref, base, gpu_compact(d_code, k, base))


DECODE_SHAPES = ((1, 1, 1), (17, 7, 33), (5, 33, 193), (33, 70, 65), (3, 4096, 64), (40, 1100, 200), (4, 12, 10000), (2, 256, 70001))
EXTRA = 5                                # ldo = p + EXTRA


def gpu_decode(indptr, indices, data, Dt, n, expect_status=0):
    """modl_csr_decode_* with ldo = p + 5: (out (n, p), the padding asserted untouched)"""
    import torch
    from modl_amd._lib import lib
    from modl_amd.device import ptr
    sx = dt_of(Dt)
    p, k = Dt.shape
    out = torch.full((n, p + EXTRA), V_SENT, dtype=torch.from_numpy(Dt[:0]).dtype, device='cuda')
    status = torch.full((1 + GUARD,), I_SENT, dtype=torch.int32, device='cuda')
    nbytes = lib.modl_csr_decode_workspace(0 if sx == 'f32' else 1, k, p)
    ws = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
    d = [_dev(t) for t in (indptr, indices, data, Dt)]
    rc = getattr(lib, 'modl_csr_decode_' + sx)(ptr(d[0]), ptr(d[1]), ptr(d[2]), len(data), n, k, ptr(d[3]), p, ptr(out),
                                               p + EXTRA, ptr(status), ptr(ws), nbytes, None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    st, o = status.cpu().numpy(), out.cpu().numpy()
    assert st[0] == expect_status and np.all(st[1:] == I_SENT)
    assert np.all(o[:, p:] == V_SENT), 'the padding of the output changed'
    return np.ascontiguousarray(o[:, :p])


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'f64'])
@pytest.mark.parametrize('n,k,p', DECODE_SHAPES, ids=['n%d-k%d-p%d' % s for s in DECODE_SHAPES])
def test_decode_through_the_abi(gpu, dt, n, k, p):
    ip, ix, dv, Dt = random_csr(dt, n, k, p, seed=n + k)
    out = gpu_decode(ip, ix, dv, Dt, n)
    print('%s decode (%d, %d, %d): %.3g of the bound' % (dt, n, k, p, judge_decode(ip, ix, dv, Dt, n, out)))
    # the same rows in another batch (reversed, an empty row and a copy of row 0 in front): the same bits
    order = [0] + list(range(n))[::-1]
    counts = np.diff(ip)
    ip2 = np.concatenate([[0, 0], np.cumsum(counts[order])]).astype(np.int64)
    sel = np.concatenate([np.arange(ip[i], ip[i + 1]) for i in order]).astype(np.int64)
    out2 = gpu_decode(ip2, ix[sel], dv[sel], Dt, n + 2)
    assert not np.any(out2[0])
    np.testing.assert_array_equal(bits(out2[1:]), bits(out[order]))
    np.testing.assert_array_equal(bits(gpu_decode(ip, ix, dv, Dt, n)), bits(out))          # and from run to run


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_decode_of_corrupt_input_is_defined(gpu, dt):
    n, k, p = 6, 9, 70
    ip, ix, dv, Dt = random_csr(dt, n, k, p, seed=5, counts=(3, 0, 66, 5))
    clean = gpu_decode(ip, ix, dv, Dt, n)
    for what in ('index_k', 'index_minus_1', 'decreasing_indptr'):
        ip2, ix2 = ip.copy(), ix.copy()
        if what == 'index_k':
            ix2[ip[2] + 65] = k                                              # in the second round of 64 entries of row 2
        elif what == 'index_minus_1':
            ix2[ip[0] + 1] = -1
        else:
            ip2[4] = ip2[3] - 2                                              # row 3 is (ip[3], ip[3] - 2): decreasing
        out = gpu_decode(ip2, ix2, dv, Dt, n, expect_status=1)
        judge_decode(ip2, ix2, dv, Dt, n, out)                               # the reference leaves the same entries out
        if what == 'decreasing_indptr':
            assert not np.any(out[3])
        untouched = [i for i in range(n) if not (what == 'index_k' and i == 2) and not (what == 'index_minus_1' and i == 0)
                     and not (what == 'decreasing_indptr' and i in (3, 4))]
        np.testing.assert_array_equal(bits(out[untouched]), bits(clean[untouched]))
    # beyond the arrays: the last non-empty row claims more entries than there are
    ip3 = ip.copy()
    ip3[n - 1:] += 1
    out = gpu_decode(ip3, ix, dv, Dt, n, expect_status=1)
    assert not np.any(out[n - 2:])
    np.testing.assert_array_equal(bits(out[:n - 2]), bits(clean[:n - 2]))
    np.testing.assert_array_equal(bits(gpu_decode(ip, ix, dv, Dt, n)), bits(clean))        # and on it goes, status 0 again


# ---- the estimators ------------------------------------------------------------------------------------------------
ALPHA = 0.05
N, P, K, RPC = 17, 12, 7, 5


def _rows(dtype, n=N, p=P, k=K, seed=3):
    """(D, X, mask): rows 0, 5, 9 and 16 clean, row 3 unobserved, the others half observed"""
    rs = np.random.RandomState(seed)
    D = rs.randn(k, p)
    D /= np.linalg.norm(D, axis=1, keepdims=True)
    X = (rs.randn(n, 4) @ rs.randn(4, p) + 0.3 * rs.randn(n, p)) / np.sqrt(p)
    mask = rs.rand(n, p) < 0.5
    mask[[0, 5, 9, n - 1]] = True
    mask[3] = False
    return D.astype(dtype), X.astype(dtype), mask


_EST = {}


def estimator(kind, dt):
    from modl_amd import Coder, DictFact
    if (kind, dt) not in _EST:
        D, X, _ = _rows(DT[dt])
        if kind == 'Coder':
            _EST[kind, dt] = Coder(D, code_alpha=ALPHA, code_l1_ratio=0.7)
        else:
            _EST[kind, dt] = DictFact(n_components=K, code_alpha=ALPHA, code_l1_ratio=0.7, batch_size=5, n_epochs=2,
                                      random_state=0).fit(_rows(DT[dt], n=40, seed=4)[1])
    return _EST[kind, dt]


CODERS = (dict(), dict(algorithm='omp', n_nonzero_coefs=2), dict(algorithm='omp', residual_tol=0.05))


def _assert_same_csr(got, ref):
    np.testing.assert_array_equal(np.diff(got.indptr), np.diff(ref.indptr))
    np.testing.assert_array_equal(got.indices, ref.indices)
    np.testing.assert_array_equal(bits(got.data), bits(ref.data))


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'f64'])
@pytest.mark.parametrize('kind', ['Coder', 'DictFact'])
def test_slice_contract(gpu, kind, dt):
    import torch
    from modl_amd import SparseCodes
    est = estimator(kind, dt)
    _, X, mask = _rows(DT[dt])
    for kw in CODERS:
        for m in (None, mask):
            got = est.transform(X, mask=m, sparse=True, rows_per_chunk=RPC, **kw)
            assert sp.isspmatrix_csr(got) and got.shape == (N, K) and got.dtype == DT[dt]
            assert got.has_canonical_format and np.all(got.data != 0)
            assert got.nnz > 0 and (m is None or got.indptr[3] == got.indptr[4])
            for c0 in range(0, N, RPC):
                sl = slice(c0, c0 + RPC)
                dense = est.transform(X[sl], mask=None if m is None else m[sl], **kw)
                _assert_same_csr(got[sl], sp.csr_matrix(dense))
            dev = est.transform(_dev(X), mask=None if m is None else _dev(m), sparse=True, rows_per_chunk=RPC, **kw)
            assert isinstance(dev, SparseCodes) and tuple(dev.shape) == (N, K)
            assert all(t.is_cuda for t in dev[:3])
            assert (dev.indptr.dtype, dev.indices.dtype, dev.data.dtype) == \
                (torch.int64, torch.int32, torch.float32 if dt == 'f32' else torch.float64)
            assert dev.indptr.shape == (N + 1,) and int(dev.indptr[0]) == 0 and int(dev.indptr[-1]) == dev.data.shape[0]
            host = dev.to_scipy()
            assert host.shape == (N, K)
            _assert_same_csr(host, got)
    # one chunk for everything, and a chunk per row
    whole = est.transform(X, sparse=True, rows_per_chunk=N)
    _assert_same_csr(whole, sp.csr_matrix(est.transform(X)))
    by_row = est.transform(X, mask=mask, sparse=True, rows_per_chunk=1)
    for i in range(N):
        _assert_same_csr(by_row[i:i + 1], sp.csr_matrix(est.transform(X[i:i + 1], mask=mask[i:i + 1])))


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_whole_call_corollary(gpu, dt):
    est = estimator('Coder', dt)
    n = 4096 + 5
    X = _rows(DT[dt], n=n, seed=8)[1]
    for kw in (dict(), dict(algorithm='omp', n_nonzero_coefs=2)):
        got = est.transform(X, sparse=True, **kw)
        assert got.shape == (n, K) and got.has_canonical_format
        assert np.all(np.diff(got.indptr)[4094:4098] > 0), 'the rows around the chunk boundary must not be empty'
        _assert_same_csr(got, sp.csr_matrix(est.transform(X, **kw)))


@pytest.mark.gpu
def test_sparse_route_stays_under_the_memory_cap(gpu):
    """a cap, not a measurement: the sparse route must stay below half of the dense (n, k) codes - a chunk's dense buffer
    is 16.8 MB, the CSR under 0.5 MB, the dense codes 81.9 MB - and the dense route, next to it, must exceed the cap"""
    import torch
    from modl_amd import Coder
    n, p, k = 20000, 16, 1024
    rs = np.random.RandomState(0)
    D = rs.randn(k, p).astype(np.float32)
    D /= np.linalg.norm(D, axis=1, keepdims=True)
    coder = Coder(D)
    X = _dev(rs.randn(n, p).astype(np.float32))
    cap = n * k * 4 / 2
    kw = dict(algorithm='omp', n_nonzero_coefs=2)
    coder.transform(X[:8], **kw)                                              # (the plan of the coders exists)

    def rise(call):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = call()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before, out
    sparse_rise, codes = rise(lambda: coder.transform(X, sparse=True, **kw))
    dense_rise, dense = rise(lambda: coder.transform(X, **kw))
    print('peak device memory over the call: sparse %.1f MB, dense %.1f MB, cap %.1f MB'
          % (sparse_rise / 1e6, dense_rise / 1e6, cap / 1e6))
    assert sparse_rise < cap
    assert dense_rise > cap
    assert codes.data.shape[0] <= 2 * n and codes.data.shape[0] > n
    _assert_same_csr(codes.to_scipy(), sp.csr_matrix(dense.cpu().numpy()))


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'f64'])
@pytest.mark.parametrize('kind', ['Coder', 'DictFact'])
def test_round_trip(gpu, kind, dt):
    import torch
    from modl_amd import SparseCodes
    est = estimator(kind, dt)
    X = _rows(DT[dt])[1]
    Dt = np.ascontiguousarray(np.asarray(est.components_).T.astype(DT[dt]))
    dense, csr = est.transform(X), est.transform(X, sparse=True)
    back_dense, back_csr = est.inverse_transform(dense), est.inverse_transform(csr)
    for back in (back_dense, back_csr):
        assert isinstance(back, np.ndarray) and back.dtype == DT[dt] and back.shape == (N, P)
    # each against the longdouble product of the same codes, within its own bound (the two sums run in different orders)
    full = sp.csr_matrix(dense)
    print('%s %s: dense decode %.3g, csr decode %.3g of the bound' % (
        kind, dt, judge_decode(full.indptr, full.indices, full.data, Dt, N, back_dense),
        judge_decode(csr.indptr, csr.indices, csr.data, Dt, N, back_csr)))
    for other in (csr.tocsc(), csr.tocoo()):                                  # any scipy sparse matrix
        np.testing.assert_array_equal(bits(est.inverse_transform(other)), bits(back_csr))
    dev = est.transform(_dev(X), sparse=True)
    back_dev = est.inverse_transform(dev)
    assert isinstance(back_dev, torch.Tensor) and back_dev.is_cuda and tuple(back_dev.shape) == (N, P)
    np.testing.assert_array_equal(bits(back_dev.cpu().numpy()), bits(back_csr))
    assert not np.any(est.inverse_transform(sp.csr_matrix((3, K), dtype=DT[dt])))       # no entry at all: zeros
    # the kernel's status word: an index outside the dictionary in device input
    bad = SparseCodes(dev.indptr, torch.where(dev.indices == dev.indices[0], K, dev.indices).to(torch.int32), dev.data,
                      dev.shape)
    with pytest.raises(ValueError, match='corrupt'):
        est.inverse_transform(bad)
    with pytest.raises(ValueError, match='%d components' % K):
        est.inverse_transform(SparseCodes(dev.indptr, dev.indices, dev.data, (N, K + 1)))
    np.testing.assert_array_equal(bits(est.inverse_transform(dev).cpu().numpy()), bits(back_csr))


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'f64'])
@pytest.mark.parametrize('kind', ['Coder', 'DictFact'])
def test_nothing_else_moved(gpu, kind, dt, monkeypatch):
    """sparse=False is the call that never mentions `sparse`: the same bits, and no csr_* call"""
    est = estimator(kind, dt)
    _, X, mask = _rows(DT[dt])
    want = [est.transform(X, mask=m, **kw) for kw in CODERS for m in (None, mask)]

    def forbidden(*a, **k):
        raise AssertionError('the dense route touched the CSR kernels')
    monkeypatch.setattr(est._backend, 'compact', forbidden)
    monkeypatch.setattr(est._backend, 'decode_csr', forbidden)
    got = [est.transform(X, mask=m, sparse=False, **kw) for kw in CODERS for m in (None, mask)]
    for g, w in zip(got, want):
        assert isinstance(g, np.ndarray) and g.dtype == DT[dt]
        np.testing.assert_array_equal(bits(g), bits(w))
    np.testing.assert_array_equal(bits(est.inverse_transform(want[0])), bits(est.inverse_transform(got[0])))
    with pytest.raises(AssertionError, match='touched'):
        est.transform(X, sparse=True)


@pytest.mark.gpu
def test_image_transform_passes_the_flag(gpu):
    """ImageDictFact.transform(patches, sparse=True) is csr_matrix of its dense codes (one chunk: no mask, < 4096 rows)"""
    import contextlib
    import io
    from modl_amd.image import ImageDictFact
    from .test_wrappers import synth_image
    img = synth_image(24, 24, 3, seed=2).astype(np.float32)
    est = ImageDictFact(patch_size=(8, 8), n_components=32, batch_size=20, alpha=0.1, random_state=0, max_patches=200)
    with contextlib.redirect_stdout(io.StringIO()):
        est.fit(img)
    rs = np.random.RandomState(0)
    patches = rs.rand(9, 8, 8, 3).astype(np.float32)
    dense = est.transform(patches)
    got = est.transform(patches, sparse=True)
    assert sp.isspmatrix_csr(got) and got.shape == dense.shape == (9, 32) and got.nnz > 0
    _assert_same_csr(got, sp.csr_matrix(dense))
    np.testing.assert_array_equal(bits(est.transform(patches, sparse=False)), bits(dense))
