"""The Amari discrepancy (modl/decomposition/stability.py:7-31 -> modl_amd.stability, modl_amari_*).

The yardstick is a float64 numpy restatement of the reference's formula (`restate` below), itself checked against
tests/golden/stability.npz, which tests/golden/make_golden_stability.py records from the reference's own module."""
import ctypes as C

import numpy as np
import pytest

from .conftest import load_golden

# f32 tolerance (absolute, on cosines and on d): the products run in exact f32 on the matrix cores, the norms in f64.
# Measured on the MI355X against the f64 restatement (scripts/bench_stability.py, profiles/stability_bench.jsonl): the
# largest deviation of a per-pair maximum is 1.8e-7 at the image shape (k = 80, p = 3 072) and 8.8e-9 at k = 70,
# p = 200 000 on independent atoms; the cases below (shared atoms, maxima near 0.8, p up to 200 000) pass under 1e-5.
F32_ATOL = 1e-5


def restate(D1, D2):
    """float64 restatement of stability.py:20-22: (row maxima, column maxima, d)"""
    D1 = np.asarray(D1, dtype=np.float64)
    D2 = np.asarray(D2, dtype=np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        C_ = D1.dot(D2.T) / np.sqrt(np.sum(D1 ** 2, axis=1))[:, None] / np.sqrt(np.sum(D2 ** 2, axis=1))[None, :]
        rmax, cmax = C_.max(axis=1), C_.max(axis=0)
        return rmax, cmax, .5 * (np.mean(1 - cmax) + np.mean(1 - rmax))


def restate_mean(dictionaries):
    ds = [restate(a, b)[2] for i, a in enumerate(dictionaries[:-1]) for b in dictionaries[i + 1:]]
    return np.mean(ds), np.std(ds)


def upstream(n_dictionaries):
    # modl/decomposition/tests/test_stability.py: check_random_state(23), 50 x 100
    rng = np.random.RandomState(23)
    return [rng.randn(50, 100) for _ in range(n_dictionaries)]


def related(ks, p, dtype, seed=0):
    """dictionaries that share atoms (permuted, some negated, plus noise): the maxima are not all noise"""
    rs = np.random.RandomState(seed)
    base = rs.randn(max(ks), p)
    out = []
    for k in ks:
        sel = rs.permutation(max(ks))[:k]
        sign = np.where(rs.rand(k) < 0.2, -1.0, 1.0)[:, None]
        out.append((sign * base[sel] + 0.7 * rs.randn(k, p)).astype(dtype))
    return out


@pytest.fixture(scope='module')
def gold():
    return load_golden('stability')


@pytest.fixture(scope='module')
def lib():
    from modl_amd import _lib
    return _lib.lib


# ---- CPU ----------------------------------------------------------------------------------------------------------

def test_fixture_against_restatement(gold):
    assert abs(restate(*upstream(2))[2] - gold['up_pair_d']) < 1e-12
    assert abs(gold['up_self_d']) < 1e-12
    m, s = restate_mean(upstream(20))
    assert abs(m - gold['up_mean_m']) < 1e-12 and abs(s - gold['up_mean_s']) < 1e-12
    assert abs(restate(gold['ragged_A'], gold['ragged_B'])[2] - gold['ragged_d']) < 1e-12
    assert abs(restate(gold['ragged_B'], gold['ragged_A'])[2] - gold['ragged_d_rev']) < 1e-12
    assert abs(restate(gold['self_A'], gold['self_A'])[2] - gold['self_d']) < 1e-12
    assert np.isnan(restate(gold['zero_A'], gold['zero_B'])[2]) and np.isnan(gold['zero_d'])
    # the reference ran these in f32: its own rounding, against the f64 restatement
    assert abs(restate(gold['f32_A'], gold['f32_B'])[2] - gold['f32_d']) < 1e-6
    m, s = restate_mean([gold['f32_list_%d' % i] for i in range(3)])
    assert abs(m - gold['f32_list_m']) < 1e-6 and abs(s - gold['f32_list_s']) < 1e-6
    assert np.isnan(gold['one_m']) and np.isnan(gold['one_s'])


def test_abi_argument_validation(lib):
    from modl_amd._lib import MODL_F32, MODL_F64
    k2 = np.array([5, 7], dtype=np.int64)
    kp = k2.ctypes.data_as(C.c_void_p)
    assert lib.modl_amari_workspace(MODL_F32, 2, kp, 10) > 0
    assert lib.modl_amari_workspace(MODL_F64, 2, kp, 10) > 0
    assert lib.modl_amari_workspace(7, 2, kp, 10) == 0                 # bad dtype
    assert lib.modl_amari_workspace(MODL_F32, 1, kp, 10) == 0          # n < 2
    assert lib.modl_amari_workspace(MODL_F32, 2, kp, 0) == 0           # p <= 0
    bad = np.array([5, 0], dtype=np.int64)
    assert lib.modl_amari_workspace(MODL_F32, 2, bad.ctypes.data_as(C.c_void_p), 10) == 0
    fake = (C.c_void_p * 2)(16, 32)                                     # never dereferenced: arguments come first
    pair, ws = C.c_void_p(64), C.c_void_p(128)
    big = 1 << 40
    launches = C.c_int(-1)
    f32 = lib.modl_amari_f32
    assert f32(fake, kp, 1, 10, pair, None, None, ws, big, None, C.byref(launches)) == -1
    assert f32(fake, kp, 2, 0, pair, None, None, ws, big, None, None) == -1
    assert f32(fake, bad.ctypes.data_as(C.c_void_p), 2, 10, pair, None, None, ws, big, None, None) == -1
    assert f32(fake, kp, 2, 10, None, None, None, ws, big, None, None) == -1              # no output
    assert f32((C.c_void_p * 2)(16, 0), kp, 2, 10, pair, None, None, ws, big, None, None) == -1
    assert f32(fake, kp, 2, 10, pair, None, None, None, big, None, None) == -2            # MODL_ENOMEM
    assert f32(fake, kp, 2, 10, pair, None, None, ws, 1, None, None) == -2
    assert launches.value == 0
    if lib.modl_device_count() == 0:
        assert f32(fake, kp, 2, 10, pair, None, None, ws, big, None, None) == -4          # MODL_ENOGPU
        assert lib.modl_amari_f64(fake, kp, 2, 10, pair, None, None, ws, big, None, None) == -4


def test_python_argument_errors():
    from modl_amd import amari_discrepency, mean_amari_discrepency
    rs = np.random.RandomState(0)
    with pytest.raises(ValueError):
        amari_discrepency(rs.randn(10), rs.randn(3, 10))                 # not 2-D
    with pytest.raises(ValueError):
        amari_discrepency(rs.randn(4, 10), rs.randn(3, 11))              # p differs
    with pytest.raises(ValueError):
        mean_amari_discrepency([rs.randn(4, 10), rs.randn(4, 10), rs.randn(2, 3, 10)])
    with pytest.raises(ValueError):
        amari_discrepency(np.zeros((0, 10)), rs.randn(3, 10))            # no atoms


def test_fewer_than_two_dictionaries(gold):
    from modl_amd import mean_amari_discrepency
    for dicts in ([], [np.random.RandomState(0).randn(5, 7)]):
        with pytest.warns(RuntimeWarning):
            m, s = mean_amari_discrepency(dicts, n_jobs=4)
        assert np.isnan(m) and np.isnan(s)
        assert type(m).__name__ == str(gold['one_m__type']) and type(s).__name__ == str(gold['one_s__type'])


def test_no_joblib():
    # n_jobs is accepted and ignored: one GPU call, no joblib pool
    import ast
    import modl_amd.stability as st
    tree = ast.parse(open(st.__file__).read())
    names = [a.name for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names]
    names += [n.module for n in ast.walk(tree) if isinstance(n, ast.ImportFrom) and n.module]
    assert not [m for m in names if m.split('.')[0] == 'joblib']


# ---- GPU ----------------------------------------------------------------------------------------------------------

def _check_scalar(value, gold, key, tol):
    ref = gold[key]
    assert type(value).__name__ == str(gold[key + '__type']), (key, type(value))
    if np.isnan(ref):
        assert np.isnan(value), key
    else:
        assert abs(float(value) - float(ref)) <= tol, (key, float(value), float(ref))


@pytest.mark.gpu
def test_fixture_cases_gpu(gold):
    from modl_amd import amari_discrepency, mean_amari_discrepency
    D = upstream(2)
    d = amari_discrepency(D[0], D[1])
    assert d >= 0
    _check_scalar(d, gold, 'up_pair_d', 1e-12)
    _check_scalar(amari_discrepency(D[0], D[0]), gold, 'up_self_d', 1e-12)
    m, s = mean_amari_discrepency(upstream(20), n_jobs=3)
    _check_scalar(m, gold, 'up_mean_m', 1e-12)
    _check_scalar(s, gold, 'up_mean_s', 1e-12)
    _check_scalar(amari_discrepency(gold['ragged_A'], gold['ragged_B']), gold, 'ragged_d', 1e-12)
    _check_scalar(amari_discrepency(gold['ragged_B'], gold['ragged_A']), gold, 'ragged_d_rev', 1e-12)
    _check_scalar(amari_discrepency(gold['self_A'], gold['self_A']), gold, 'self_d', 1e-12)
    _check_scalar(amari_discrepency(gold['zero_A'], gold['zero_B']), gold, 'zero_d', 0)
    # f32: against the f64 restatement to F32_ATOL, and to the reference's own f32 run
    f = amari_discrepency(gold['f32_A'], gold['f32_B'])
    _check_scalar(f, gold, 'f32_d', F32_ATOL)
    assert abs(float(f) - restate(gold['f32_A'], gold['f32_B'])[2]) <= F32_ATOL
    L = [gold['f32_list_%d' % i] for i in range(3)]
    m, s = mean_amari_discrepency(L)
    _check_scalar(m, gold, 'f32_list_m', F32_ATOL)
    _check_scalar(s, gold, 'f32_list_s', F32_ATOL)


@pytest.mark.gpu
def test_nan_propagates_gpu():
    from modl_amd import amari_discrepency
    from modl_amd.stability import amari_pairs
    for dt in (np.float32, np.float64):
        A, B = related([9, 12], 40, dt, seed=3)
        A[2, 5] = np.nan
        assert np.isnan(amari_discrepency(A, B))
        r = amari_pairs([A, B], maxima=True)
        rm, cm, _ = restate(A, B)
        assert np.array_equal(np.isnan(r['rowmax'][0]), np.isnan(rm)) and np.isnan(r['rowmax'][0][2])
        assert np.all(np.isnan(r['colmax'][0])) and np.all(np.isnan(cm))
        B[4] = 0                                                       # a zero atom: one NaN column
        A[2, 5] = 1.0
        r = amari_pairs([A, B], maxima=True)
        assert np.isnan(r['d'][0]) and np.isnan(r['colmax'][0][4]) and np.all(np.isnan(r['rowmax'][0]))
        assert np.sum(np.isnan(r['colmax'][0])) == 1


def test_signed_maximum_gpu_case():
    # anti-correlated atoms are not matched: the restatement (and the kernels) take the signed maximum
    A = np.eye(3, 5)
    rm, cm, d = restate(A, -A)
    assert np.all(rm == 0) and d == 1.0


@pytest.mark.gpu
def test_signed_maximum_gpu():
    from modl_amd import amari_discrepency
    A = np.eye(3, 5)
    assert amari_discrepency(A, -A) == 1.0
    assert amari_discrepency(A.astype(np.float32), -A.astype(np.float32)) == np.float32(1.0)


# (dtype, ks, p): p in {1, 3, 3 072, 200 000}, k in {1, 37, 70, 129, 1 024, 1 500}; the p = 200 000 cases take the K
# split, the p <= 3 072 ones the unsplit tile; 129, 1 500 and 70 leave partial edge tiles of both tile sizes (128 / 64)
MAXIMA_CASES = [
    ('f64', [1, 37], 1),
    ('f32', [37, 1, 70], 3),
    ('f64', [1500, 129], 3),
    ('f64', [37, 70, 129], 3072),
    ('f32', [129, 1024, 1500], 3072),
    ('f32', [70, 70], 200000),
    ('f64', [70, 129], 200000),
    ('f32', [37, 70, 129, 1, 70] * 4, 3072),      # 20 ragged dictionaries: 190 pairs in one launch
]


@pytest.mark.gpu
@pytest.mark.parametrize('dt,ks,p', MAXIMA_CASES)
def test_pair_maxima_against_restatement(dt, ks, p):
    from modl_amd.stability import amari_pairs
    dtype = np.float32 if dt == 'f32' else np.float64
    D = related(ks, p, dtype, seed=len(ks) + p)
    r = amari_pairs(D, maxima=True)
    assert r['dtype'] == dtype
    tol = F32_ATOL if dt == 'f32' else 1e-12
    q = 0
    for a in range(len(D) - 1):
        for b in range(a + 1, len(D)):
            rm, cm, d = restate(D[a], D[b])
            assert r['rowmax'][q].shape == (ks[a],) and r['colmax'][q].shape == (ks[b],)
            assert np.max(np.abs(r['rowmax'][q] - rm)) <= tol, (a, b)
            assert np.max(np.abs(r['colmax'][q] - cm)) <= tol, (a, b)
            assert abs(r['d'][q] - d) <= tol, (a, b)
            q += 1
    assert q == len(r['d'])


@pytest.mark.gpu
def test_three_large_dictionaries_f32():
    from modl_amd import mean_amari_discrepency
    from modl_amd.stability import amari_pairs
    D = related([1024] * 3, 50000, np.float32, seed=5)
    r = amari_pairs(D, maxima=True)
    assert r['launches'] == 4                                          # 192 tiles: split along p
    q = 0
    for a in range(2):
        for b in range(a + 1, 3):
            rm, cm, d = restate(D[a], D[b])
            assert np.max(np.abs(r['rowmax'][q] - rm)) <= F32_ATOL
            assert np.max(np.abs(r['colmax'][q] - cm)) <= F32_ATOL
            assert abs(r['d'][q] - d) <= F32_ATOL
            q += 1
    m, s = mean_amari_discrepency(D)
    assert type(m).__name__ == str(load_golden('stability')['f32_list_m__type'])
    assert abs(m - np.mean(r['d'])) <= F32_ATOL


@pytest.mark.gpu
@pytest.mark.parametrize('dt,ks,p', [('f32', [70, 70], 200000), ('f64', [37, 70, 129], 3072)])
def test_bit_identical_runs(dt, ks, p):
    from modl_amd.stability import amari_pairs
    D = related(ks, p, np.float32 if dt == 'f32' else np.float64, seed=11)
    r1, r2 = amari_pairs(D, maxima=True), amari_pairs(D, maxima=True)
    assert r1['d'].tobytes() == r2['d'].tobytes()
    for a, b in zip(r1['rowmax'] + r1['colmax'], r2['rowmax'] + r2['colmax']):
        assert a.tobytes() == b.tobytes()


@pytest.mark.gpu
def test_launch_count_independent_of_n():
    from modl_amd.stability import amari_pairs
    r2 = amari_pairs(upstream(2))
    r20 = amari_pairs(upstream(20))
    assert r2['launches'] == r20['launches'] == 3
    assert len(r20['d']) == 190


@pytest.mark.gpu
def test_torch_input_matches_numpy():
    import torch
    from modl_amd import amari_discrepency, mean_amari_discrepency
    for dt in (np.float32, np.float64):
        D = related([37, 70, 129], 3072, dt, seed=2)
        T = [torch.from_numpy(x).cuda() for x in D]
        assert mean_amari_discrepency(D) == mean_amari_discrepency(T)
        assert amari_discrepency(D[0], D[2]) == amari_discrepency(T[0], T[2])
    # a mixed list is computed in f64, as numpy promotes
    D = related([20, 30], 64, np.float64, seed=4)
    mixed = amari_discrepency(D[0].astype(np.float32), D[1])
    assert type(mixed) is np.float64
    assert abs(mixed - restate(D[0].astype(np.float32), D[1])[2]) <= 1e-12


@pytest.mark.gpu
def test_image_example_end_to_end():
    # examples/stability_selection.py:90: dictionaries of ImageDictFact fits with different seeds, flattened
    import contextlib
    import io
    from modl_amd import mean_amari_discrepency
    from modl_amd.image import ImageDictFact
    from .test_wrappers import synth_image
    img = synth_image(40, 40, 3, seed=1)
    dicts = []
    for seed in (0, 1):
        est = ImageDictFact(patch_size=(6, 6), n_components=12, batch_size=20, alpha=0.05, random_state=seed,
                            max_patches=300, reduction=2)
        with contextlib.redirect_stdout(io.StringIO()):
            est.fit(img)
        comp = est.components_
        dicts.append(comp.reshape((comp.shape[0], -1)))
    m, s = mean_amari_discrepency(dicts)
    rm, rs = restate_mean(dicts)
    tol = F32_ATOL if all(d.dtype == np.float32 for d in dicts) else 1e-12
    assert abs(m - rm) <= tol and abs(s - rs) <= tol
    assert 0 <= m <= 2
