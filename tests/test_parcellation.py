"""Hard parcellation on the device: modl_amd.parcellation, csrc/kmeans.hip, fMRIParcellation.

The judge is the set of host twins (`*_host`, plain numpy).  Layer 1 (no GPU) holds the k-means twin to
sklearn.cluster.KMeans(init=init, n_init=1, algorithm='lloyd', tol=0) - labels identical, inertia to 1e-12 relative - and to an
independent restatement with explicit loops over voxels, shows that every mutant of the restatement is rejected by at least one
case, checks label_signals_host against scipy.ndimage.mean and kmeans_init_host against its stated rule, and then the refusals.
Layer 2 (gpu): the two kernels through the C-ABI inside guard elements (NaN padding after every row, a NaN-poisoned workspace),
then the Python functions, the pipeline on planted parcels and the estimator.

Why labels are compared EXACTLY.  Every trajectory case asserts on the judge's own run that, over all assignments and voxels,
(second-best score - best score) / max_c(|C_c|^2 + 2 sum_j |C_cj x_jv|) > 1e-9, exact bit ties excluded (a tie is decided by the
index, not by rounding).  The rounding of a score is at most 4 (d + 4) u of that denominator (u = 2^-53: d products and d
accumulations of the dot product in any association, the d of |C|^2, the final fused multiply-add), 6e-14 at d = 128: no label
can flip on summation order.  The same bound, against the winning centre's absolute sum, is the tolerance of the kernel's scores.

Sums and means: (n + 2) u sum |x| for a sum of n terms in any order (n - 1 additions, the conversion, the division of a mean),
against a reference accumulated in extended precision.

The module imports the new names at the top: no test here can pass without the feature."""
import ctypes as C
import warnings

import numpy as np
import pytest
import scipy.ndimage

from modl_amd.parcellation import (KMeansParcels, Parcellation, kmeans_init, kmeans_parcels, label_signals, signals_to_rows,  # noqa: F401
                                   parcellate, kmeans_init_host, kmeans_parcels_host, label_signals_host, signals_to_rows_host,
                                   parcellate_host, kmeans_trace_host, _assign_host)
from modl_amd.fmri import fMRIParcellation
from modl_amd._lib import lib

from .test_clean import EINVAL, ENOMEM, ENOGPU, same_bits
from .test_compute_mask import _Guarded, GUARD, gpu  # noqa: F401
from .test_canica import _NanWorkspace

U = 2.0 ** -53
GAP = 1e-9
TRAJECTORY = [(3, 600, 4), (5, 1500, 7), (17, 1037, 20), (33, 2111, 37), (8, 4099, 130), (16, 3000, 64), (128, 777, 16)]
MUTANTS = ('drop_cnorm', 'highest_on_tie', 'divide_by_V', 'keep_empty', 'no_subtract', 'select_max')
SIGNAL_MUTANTS = ('zero_based', 'label0_is_a_parcel')
PHANTOMS = [(600, 24, 4, 2), (1500, 30, 7, 2)]
SEEDS = {(128, 777, 16): 1}                                 # (the default seed passes through two empty clusters at once there)


# ------------------------------------------------------------------------------------------------------- the phantoms
def blobs(d, V, K, seed=None):
    """K Gaussian blobs (centres 3 randn, unit noise) as (d, V) components, and K distinct voxels as the init"""
    rng = np.random.RandomState(SEEDS.get((d, V, K), 1000 * d + V + K) if seed is None else seed)
    centres = 3 * rng.randn(K, d)
    X = np.ascontiguousarray((centres[rng.randint(K, size=V)] + rng.randn(V, d)).T)
    init = np.ascontiguousarray(X[:, rng.choice(V, K, replace=False)].T)
    return X, init


def duplicated_case(copies=1):
    """(6, 900, 9) with init[5] = init[2] (copies=2: init[7] too): an exact tie that the lower index wins, so the copies start
    empty and are relocated"""
    X, init = blobs(6, 900, 9)
    init[5] = init[2]
    if copies == 2:
        init[7] = init[2]
    return X, init


def abs_sums(X, Cc):
    """(K, V): |C_c|^2 + 2 sum_j |C_cj x_jv|, the absolute sum of the terms of a score"""
    return (Cc * Cc).sum(axis=1)[:, None] + 2.0 * (np.abs(Cc) @ np.abs(X))


def assignment_gap(X, Cc):
    """the smallest (second-best - best) / max_c abs_sum over the voxels, exact ties excluded; inf for K = 1"""
    if Cc.shape[0] < 2:
        return np.inf
    S = (Cc * Cc).sum(axis=1)[:, None] - 2.0 * (Cc @ X)
    two = np.partition(S, 1, axis=0)[:2]
    gap = (two[1] - two[0]) / abs_sums(X, Cc).max(axis=0)
    gap = gap[two[1] != two[0]]
    return gap.min() if gap.size else np.inf


def relocation_gap(X, trace):
    """over the updates with e > 0 empty clusters: the smallest relative difference between successive distances among the
    e + 1 farthest voxels (the e that move and the first that stays)"""
    xn2, worst = (X * X).sum(axis=0), np.inf
    for Cc, e in zip(trace['centers'], trace['empty']):
        if e:
            _, score = _assign_host(X, Cc)
            far = np.sort(score + xn2)[::-1][:e + 1]
            worst = min(worst, np.min((far[:-1] - far[1:]) / far[0]))
    return worst


_judge_cache = {}


def judge(key, X, init, tol=0.0):
    """the twin's run of a case and its trace, computed once and shared; asserts the precondition of exact labels"""
    if key not in _judge_cache:
        res = kmeans_parcels_host(X, init.shape[-2], init=init, tol=tol, max_iter=300)
        traces = kmeans_trace_host(X, init, tol=tol, max_iter=300)
        gaps = [assignment_gap(X, Cc) for tr in traces for Cc in tr['centers']]
        print(key, 'n_iter', res.n_iter, 'smallest assignment gap', min(gaps), 'empty', [max(tr['empty'], default=0) for tr in traces])
        assert min(gaps) > GAP
        assert res.converged.all()
        _judge_cache[key] = (res, traces)
    return _judge_cache[key]


def trajectory(shape):
    X, init = blobs(*shape)
    return (X, init) + judge(shape, X, init)


# ------------------------------------------------------------------------------------------- the restatement (loops)
def re_assign(X, Cc, mutant=None):
    V, K = X.shape[1], Cc.shape[0]
    labels, score = np.zeros(V, dtype=np.int64), np.zeros(V)
    for v in range(V):
        best, at = None, -1
        for c in range(K):
            s = -2.0 * float(Cc[c] @ X[:, v])
            if mutant != 'drop_cnorm':
                s += float(Cc[c] @ Cc[c])
            if best is None or s < best or (mutant == 'highest_on_tie' and s == best):
                best, at = s, c
        labels[v], score[v] = at, best
    return labels, score


def re_lloyd(X, Cc, tol_abs, max_iter, mutant=None):
    d, V = X.shape
    K = Cc.shape[0]
    prev, n_iter, converged, strict = None, 0, False, False
    for it in range(1, max_iter + 1):
        labels, score = re_assign(X, Cc, mutant)
        if prev is not None and list(labels) == list(prev):
            converged = strict = True
            break
        sums, counts = np.zeros((K, d)), np.zeros(K, dtype=np.int64)
        for v in range(V):
            sums[labels[v]] += X[:, v]
            counts[labels[v]] += 1
        if mutant != 'keep_empty':
            empty = [c for c in range(K) if counts[c] == 0]
            dist = [score[v] + float(X[:, v] @ X[:, v]) for v in range(V)]
            far = sorted(range(V), key=lambda v: (-dist[v], v))[:len(empty)]
            for c, v in zip(empty, far):
                if mutant != 'no_subtract':
                    sums[labels[v]] -= X[:, v]
                counts[labels[v]] -= 1
                sums[c], counts[c] = X[:, v], 1
        new = Cc.copy()
        for c in range(K):
            if counts[c] > 0:
                new[c] = sums[c] / (V if mutant == 'divide_by_V' else counts[c])
        shift = float(((new - Cc) ** 2).sum())
        Cc, prev, n_iter = new, labels, it
        if shift <= tol_abs:
            converged = True
            break
    if not strict:
        labels, score = re_assign(X, Cc, mutant)
    inertia = sum(score[v] + float(X[:, v] @ X[:, v]) for v in range(V))
    return labels, Cc, inertia, n_iter, converged


def re_kmeans(X, init, tol=0.0, max_iter=300, mutant=None):
    init = init[None] if init.ndim == 2 else init
    tol_abs = tol * float(np.mean([np.var(row) for row in X]))
    runs = [re_lloyd(X, c.copy(), tol_abs, max_iter, mutant) for c in init]
    inertias = np.array([r[2] for r in runs])
    sel = int(np.argmax(inertias) if mutant == 'select_max' else np.argmin(inertias))
    return KMeansParcels((runs[sel][0] + 1).astype(np.int32), runs[sel][1], float(inertias[sel]), np.array([r[3] for r in runs]),
                         np.array([r[4] for r in runs]), sel, inertias)


def re_label_signals(rows, labels, K, mutant=None):
    T, V = rows.shape
    sums, counts = np.zeros((T, K)), np.zeros(K, dtype=np.int64)
    for v in range(V):
        c = int(labels[v]) - (0 if mutant == 'zero_based' else 1)
        if mutant == 'label0_is_a_parcel':
            c = int(labels[v])
        if 0 <= c < K:
            sums[:, c] += rows[:, v]
            counts[c] += 1
    return np.where(counts > 0, sums / np.maximum(counts, 1), 0.0), counts


def centre_bound(X, labels0, K):
    """(K, d): (n_c + 2) u sum |x| / n_c per element of a centre"""
    out = np.zeros((K, X.shape[0]))
    for c in range(K):
        n = int(np.sum(labels0 == c))
        if n:
            out[c] = (n + 2) * U * np.abs(X[:, labels0 == c]).sum(axis=1) / n
    return out


def agrees(a, b, X):
    """two KMeansParcels of one case: labels, counts, flags and selection equal, the centres within their bound"""
    lab = np.asarray(a.labels)
    if not (np.array_equal(lab, np.asarray(b.labels)) and np.array_equal(np.asarray(a.n_iter), np.asarray(b.n_iter))
            and np.array_equal(np.asarray(a.converged), np.asarray(b.converged)) and a.selected == b.selected):
        return False
    K = np.asarray(a.centers).shape[0]
    return bool(np.all(np.abs(np.asarray(a.centers) - np.asarray(b.centers)) <= centre_bound(X, lab - 1, K)))


# ----------------------------------------------------------------------------------------------- layer 1: no GPU
@pytest.mark.parametrize('shape', TRAJECTORY, ids=str)
def test_the_twin_agrees_with_sklearn(shape):
    from sklearn.cluster import KMeans
    X, init, got, traces = trajectory(shape)
    assert max(traces[0]['empty'], default=0) <= 1                      # sklearn leaves the order among several unspecified
    assert relocation_gap(X, traces[0]) > GAP
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        sk = KMeans(n_clusters=shape[2], init=init, n_init=1, algorithm='lloyd', tol=0, max_iter=300).fit(X.T)
    print(shape, 'inertia', got.inertia, sk.inertia_, 'n_iter', got.n_iter, sk.n_iter_)
    assert got.labels.dtype == np.int32 and got.labels.min() >= 1 and got.labels.max() <= shape[2]
    assert np.array_equal(got.labels - 1, sk.labels_)
    assert abs(got.inertia - sk.inertia_) <= 1e-12 * sk.inertia_
    assert got.n_iter[0] == sk.n_iter_ - 1 and got.selected == 0         # sklearn counts the closing iteration too


def test_a_duplicated_centre_is_an_exact_tie_for_the_lower_index():
    from sklearn.cluster import KMeans
    X, init = duplicated_case()
    got, traces = judge('dup', X, init)
    assert traces[0]['empty'][0] == 1 and max(traces[0]['empty']) == 1
    first, _ = _assign_host(X, init)
    assert np.any(first == 2) and not np.any(first == 5)               # the lower index took every voxel of the tie
    assert relocation_gap(X, traces[0]) > GAP
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        sk = KMeans(n_clusters=9, init=init, n_init=1, algorithm='lloyd', tol=0, max_iter=300).fit(X.T)
    assert np.array_equal(got.labels - 1, sk.labels_) and abs(got.inertia - sk.inertia_) <= 1e-12 * sk.inertia_
    assert len(np.unique(got.labels)) == 9                             # the relocated cluster lives


def test_two_empty_clusters_at_once_follow_the_stated_rule():
    X, init = duplicated_case(copies=2)
    got, traces = judge('dup2', X, init)
    assert traces[0]['empty'][0] == 2
    assert relocation_gap(X, traces[0]) > GAP
    assert agrees(got, re_kmeans(X, init), X)


@pytest.mark.parametrize('shape', TRAJECTORY[:4] + [(128, 777, 16)], ids=str)
def test_the_twin_agrees_with_the_restatement(shape):
    X, init, got, _ = trajectory(shape)
    want = re_kmeans(X, init)
    assert agrees(got, want, X)
    assert abs(got.inertia - want.inertia) <= 1e-12 * want.inertia


def restart_case():
    """the four blobs of (3, 600, 4) cut into six parcels from three inits: the restarts end in different minima"""
    X, _ = blobs(3, 600, 4)
    rng = np.random.RandomState(6)
    return X, np.stack([np.ascontiguousarray(X[:, rng.choice(600, 6, replace=False)].T) for _ in range(3)])


def test_the_restart_with_the_smallest_inertia_is_selected():
    X, inits = restart_case()
    got, _ = judge('restarts', X, inits)
    srt = np.sort(got.inertias)
    print('inertias', got.inertias)
    assert srt[1] - srt[0] > GAP * srt[0]                               # the precondition: the selection cannot flip on rounding
    assert got.selected == int(np.argmin(got.inertias)) == 1 and got.inertia == got.inertias[got.selected]
    assert agrees(got, re_kmeans(X, inits), X)
    tie = kmeans_parcels_host(X, 6, init=np.stack([inits[2], inits[2]]), tol=0)
    assert tie.selected == 0 and tie.inertias[0] == tie.inertias[1]    # ties go to the lower index


@pytest.mark.parametrize('mutant', MUTANTS)
def test_the_judge_rejects_the_mutant(mutant):
    """every mutant of the restatement disagrees with the twin on at least one case"""
    rejected = False
    for key, (X, init) in (('dup', duplicated_case()), ('restarts', restart_case())):
        got, _ = judge(key, X, init)
        assert agrees(got, re_kmeans(X, init, max_iter=40), X)
        rejected |= not agrees(got, re_kmeans(X, init, max_iter=40, mutant=mutant), X)
    X, init = duplicated_case()                                         # one update alone: the centres right after a relocation
    one = kmeans_parcels_host(X, 9, init=init, tol=0, max_iter=1)
    assert not one.converged[0] and agrees(one, re_kmeans(X, init, max_iter=1), X)
    rejected |= not agrees(one, re_kmeans(X, init, max_iter=1, mutant=mutant), X)
    assert rejected


def signal_case(dtype, T=7, V=333, K=20, seed=0):
    rng = np.random.RandomState(seed)
    rows = (rng.randn(T, V) + 3.0).astype(dtype)
    labels = rng.randint(0, K + 3, size=V).astype(np.int32)           # 0, K + 1, K + 2: in no parcel
    labels[labels == 5] = 6                                             # an empty label
    labels[11] = -4
    return rows, labels, K


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
def test_label_signals_host_against_scipy_ndimage_mean(dtype):
    rows, labels, K = signal_case(dtype)
    got, counts = label_signals_host(rows, labels, K)
    assert got.dtype == dtype and got.shape == (7, K) and counts.dtype == np.int64
    safe = np.where((labels >= 1) & (labels <= K), labels, 0)
    assert np.array_equal(counts, np.bincount(safe, minlength=K + 1)[1:])
    assert counts[4] == 0 and np.all(got[:, 4] == 0)                    # an empty label: a column of zeros
    eps_out = np.finfo(dtype).eps if dtype == np.float32 else 0.0
    for t in range(rows.shape[0]):
        want = scipy.ndimage.mean(rows[t].astype(np.float64), safe, index=np.arange(1, K + 1))
        for c in range(K):
            if counts[c]:
                x = np.abs(rows[t, safe == c + 1].astype(np.float64))
                assert abs(got[t, c] - want[c]) <= (counts[c] + 2) * U * x.sum() / counts[c] + eps_out * abs(want[c]), (t, c)
    sums, _ = label_signals_host(rows, labels, K, strategy='sum')
    assert np.allclose(sums[:, counts > 0] / counts[counts > 0], got[:, counts > 0], rtol=1e-6)
    assert label_signals_host(rows, labels)[0].shape == (7, K + 2)      # n_labels=None: the largest label
    want, wc = re_label_signals(rows.astype(np.float64), labels, K)
    assert np.array_equal(counts, wc) and np.allclose(got, want, rtol=1e-6 if dtype == np.float32 else 1e-13)


@pytest.mark.parametrize('mutant', SIGNAL_MUTANTS)
def test_the_judge_rejects_the_label_mutant(mutant):
    rows, labels, K = signal_case(np.float64)
    got, counts = label_signals_host(rows, labels, K)
    want, wc = re_label_signals(rows, labels, K, mutant)
    assert not (np.array_equal(counts, wc) and np.allclose(got, want, rtol=1e-13))


def coarse_signals(T, K, dtype):
    """signals on a grid of 2^-10: n copies of a value add up without rounding in float64 whatever the order, so the mean of a
    piecewise-constant row gives the value back bit for bit"""
    return (np.round(np.random.RandomState(3).randn(T, K) * 1024) / 1024).astype(dtype)


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
def test_signals_to_rows_inverts_label_signals_on_piecewise_constant_rows(dtype):
    _, labels, K = signal_case(dtype)
    signals = coarse_signals(5, K, dtype)
    rows = signals_to_rows_host(signals, labels)
    ok = (labels >= 1) & (labels <= K)
    assert rows.dtype == dtype and rows.shape == (5, 333) and np.all(rows[:, ~ok] == 0)
    assert same_bits(rows[:, ok], signals[:, labels[ok] - 1])
    back, counts = label_signals_host(rows, labels, K)
    assert same_bits(back[:, counts > 0], signals[:, counts > 0])       # the mean of n copies of x is x, bit for bit
    assert same_bits(signals_to_rows_host(back, labels), rows)
    assert same_bits(signals_to_rows(signals, labels), rows)            # numpy in, numpy out: the host path


def init_rule_margin(X, vox, seed):
    """replays kmeans_init's rule from the same RandomState; returns the smallest distance of a draw from a boundary of the
    cumulative sum, relative to the total"""
    rs = np.random.RandomState(seed)
    d, V = X.shape
    worst = np.inf
    for r in range(vox.shape[0]):
        first = rs.randint(V)
        draws = [rs.random_sample() for _ in range(vox.shape[1] - 1)]
        assert vox[r, 0] == first
        closest = ((X - X[:, [first]]) ** 2).sum(axis=0)
        for c, draw in enumerate(draws, start=1):
            cum = np.cumsum(closest)
            val = draw * cum[-1]
            v = int(vox[r, c])
            assert cum[v] > val and (v == 0 or cum[v - 1] <= val)       # the first voxel whose inclusive sum exceeds the draw
            below = val - (cum[v - 1] if v else 0.0)
            worst = min(worst, (cum[v] - val) / cum[-1], below / cum[-1])
            closest = np.minimum(closest, ((X - X[:, [v]]) ** 2).sum(axis=0))
    return worst


@pytest.mark.parametrize('shape', [(3, 600, 4), (17, 1037, 20)], ids=str)
def test_kmeans_init_host_follows_the_stated_rule(shape):
    X, _ = blobs(*shape)
    centers, vox = kmeans_init_host(X, shape[2], n_init=3, random_state=7, return_voxels=True)
    assert centers.shape == (3, shape[2], shape[0]) and vox.shape == (3, shape[2])
    assert same_bits(centers, np.ascontiguousarray(X[:, vox.reshape(-1)].T.reshape(centers.shape)))
    margin = init_rule_margin(X, vox, 7)
    print(shape, 'smallest distance of a draw from a boundary', margin)
    assert margin > GAP
    assert all(len(set(v)) == shape[2] for v in vox)                    # a chosen voxel has distance 0: never drawn again
    assert same_bits(kmeans_init_host(X, shape[2], 3, 7), centers)
    a = kmeans_parcels_host(X, shape[2], n_init=3, tol=0, random_state=7)
    b = kmeans_parcels_host(X, shape[2], init=centers, tol=0)
    assert same_bits(a.labels, b.labels) and a.selected == b.selected


def test_value_errors_name_the_offender():
    X, init = blobs(3, 600, 4)
    kmax, dmax = lib.modl_kmeans_max_clusters(), lib.modl_kmeans_max_features()
    for f in (kmeans_parcels_host, kmeans_parcels):
        with pytest.raises(ValueError, match='n_parcels must be'):
            f(X, 0, init=None)
        with pytest.raises(ValueError, match='larger than the 600 voxels'):
            f(X, 601)
        with pytest.raises(ValueError, match='at most %d parcels' % kmax):
            f(np.zeros((2, kmax + 10)), kmax + 1)
        with pytest.raises(ValueError, match='at most %d components' % dmax):
            f(np.zeros((dmax + 1, 300)), 3)
        with pytest.raises(ValueError, match='max_iter'):
            f(X, 4, init=init, max_iter=0)
        with pytest.raises(ValueError, match='tol must be'):
            f(X, 4, init=init, tol=-1.0)
        with pytest.raises(ValueError, match='n_init'):
            f(X, 4, n_init=0)
        with pytest.raises(ValueError, match=r'init must be \(n_init, 4, 3\)'):
            f(X, 4, init=init[:, :2])
        with pytest.raises(ValueError, match='init holds non-finite'):
            f(X, 4, init=np.full_like(init, np.nan))
        bad = X.copy()
        bad[1, 17] = np.inf
        with pytest.raises(ValueError, match='non-finite'):
            f(bad, 4, init=init)
        with pytest.raises(ValueError, match='2-D'):
            f(X[0], 4)
    for f in (kmeans_init_host, kmeans_init):
        with pytest.raises(ValueError, match='larger than the 600 voxels'):
            f(X, 601)
        with pytest.raises(ValueError, match='n_init'):
            f(X, 4, n_init=0)
    rows, labels, K = signal_case(np.float64)
    for f in (label_signals_host, label_signals):
        with pytest.raises(ValueError, match="'mean' or 'sum'"):
            f(rows, labels, K, strategy='median')
        with pytest.raises(ValueError, match=r'labels must be \(333,\)'):
            f(rows, labels[:-1], K)
        with pytest.raises(ValueError, match='labels must be integers'):
            f(rows, labels.astype(np.float64), K)
        with pytest.raises(ValueError, match='n_labels'):
            f(rows, labels, 0)
    for f in (signals_to_rows_host, signals_to_rows):
        with pytest.raises(ValueError, match='1-D'):
            f(rows[:, :K], labels.reshape(3, 111))
    for f in (parcellate_host, parcellate):
        with pytest.raises(ValueError, match='shortest record'):
            f([np.zeros((8, 50)), np.zeros((4, 50))], 3, n_components=5)
        with pytest.raises(ValueError, match='one number of voxels'):
            f([np.zeros((8, 50)), np.zeros((8, 51))], 3, n_components=5)
        with pytest.raises(ValueError, match='at least one record'):
            f([], 3)


class _Unreadable:
    """a record that must not be processed: it has a shape and a dtype, and nothing else"""
    shape, ndim, dtype = (30, 50), 2, np.dtype(np.float64)

    def __array__(self, *a, **k):
        raise AssertionError('a record was processed before the arguments were refused')


def test_the_estimator_refuses_before_any_record_is_processed():
    recs = [_Unreadable(), np.zeros((9, 50))]
    with pytest.raises(ValueError, match='compute_epi_mask'):
        fMRIParcellation(mask='epi').fit(recs)
    with pytest.raises(ValueError, match='at most %d components' % lib.modl_kmeans_max_features()):
        fMRIParcellation(n_components=lib.modl_kmeans_max_features() + 1).fit(recs)
    est = fMRIParcellation(n_parcels=5, n_components=10)
    with pytest.raises(ValueError, match='n_components = 10 is larger than the 9 time points of record 1'):
        est.fit(recs)
    with pytest.raises(ValueError, match='larger than the 50 voxels'):
        fMRIParcellation(n_parcels=51, n_components=5).fit(recs)
    with pytest.raises(ValueError, match='n_components must be'):
        fMRIParcellation(n_components=0).fit(recs)
    with pytest.raises(ValueError, match='at least one record'):
        fMRIParcellation().fit([])
    assert not hasattr(est, 'labels_')
    with pytest.raises(ValueError, match='not fitted'):
        est.transform([np.zeros((9, 50))])
    with pytest.raises(ValueError, match='not fitted'):
        est.inverse_transform([np.zeros((9, 5))])
    assert fMRIParcellation().get_params()['n_parcels'] == 50


def _at(i):
    """a fake, aligned, far-apart address: the argument checks never follow it"""
    return C.c_void_p((i + 1) << 40)


def _assign_rc(d=3, V=10, K=4, n=2, R=1, ldx=None, ws_bytes=None, ws=True, ptrs=None):
    need = lib.modl_kmeans_assign_workspace(V, d, K, R)
    p = dict(X=_at(0), C=_at(1), active=_at(2), score=_at(3), labels=_at(4), ws=_at(5))
    p.update(ptrs or {})
    return lib.modl_kmeans_assign_f64(p['X'], V if ldx is None else ldx, V, d, p['C'], K, n, p['active'], R, p['score'], p['labels'],
                                      p['ws'] if ws else None, need if ws_bytes is None else ws_bytes, None)


def _sums_rc(sfx='f64', rows=3, V=10, K=4, n_order=10, ldx=None, lds=None, ptrs=None):
    p = dict(X=_at(0), order=_at(1), offsets=_at(2), sums=_at(3))
    p.update(ptrs or {})
    return getattr(lib, 'modl_label_sums_' + sfx)(p['X'], V if ldx is None else ldx, rows, V, p['order'], n_order, p['offsets'], K,
                                                  p['sums'], K if lds is None else lds, None)


def test_the_entry_points_refuse_bad_arguments_before_any_device_work():
    kmax, dmax = lib.modl_kmeans_max_clusters(), lib.modl_kmeans_max_features()
    assert kmax >= 1024 and dmax == 128 == lib.modl_ica_max_components()
    assert lib.modl_kmeans_assign_workspace(300512, 100, 1000, 3) < 300512 * 8          # nothing of size V, let alone V x K
    assert lib.modl_kmeans_assign_workspace(10, 3, 4, 2) >= 2 * 4 * 8
    for bad in ((0, 3, 4, 1), (10, 0, 4, 1), (10, dmax + 1, 4, 1), (10, 3, 0, 1), (10, 3, kmax + 1, 1), (10, 3, 4, 0), (10, 3, 4, 65536)):
        assert lib.modl_kmeans_assign_workspace(*bad) == 0, bad
    for bad in (dict(d=0), dict(d=dmax + 1), dict(K=0), dict(K=kmax + 1), dict(V=0), dict(R=0), dict(R=3, n=2), dict(R=65536, n=65536),
                dict(ldx=9), dict(ptrs=dict(X=None)), dict(ptrs=dict(C=None)), dict(ptrs=dict(active=None)), dict(ptrs=dict(score=None)),
                dict(ptrs=dict(labels=None)), dict(ptrs=dict(X=C.c_void_p((1 << 40) + 4))), dict(ptrs=dict(labels=C.c_void_p((5 << 40) + 2))),
                dict(ptrs=dict(score=_at(0))), dict(ptrs=dict(labels=_at(1))), dict(ptrs=dict(score=_at(5))), dict(ptrs=dict(ws=_at(0))),
                dict(ptrs=dict(labels=C.c_void_p((4 << 40) + 8)))):
        assert _assign_rc(**bad) == EINVAL, bad
    assert _assign_rc(ws=False) == ENOMEM and _assign_rc(ws_bytes=lib.modl_kmeans_assign_workspace(10, 3, 4, 1) - 1) == ENOMEM
    for sfx in ('f32', 'f64'):
        for bad in (dict(K=0), dict(rows=-1), dict(V=0), dict(V=1 << 31, ldx=1 << 31), dict(n_order=-1), dict(ldx=9), dict(lds=3),
                    dict(rows=32 * 65535 + 1), dict(ptrs=dict(X=None)), dict(ptrs=dict(order=None)), dict(ptrs=dict(offsets=None)),
                    dict(ptrs=dict(sums=None)), dict(ptrs=dict(sums=C.c_void_p((4 << 40) + 4))), dict(ptrs=dict(order=C.c_void_p((2 << 40) + 2))),
                    dict(ptrs=dict(sums=_at(0))), dict(ptrs=dict(sums=_at(1))), dict(ptrs=dict(sums=_at(2)))):
            assert _sums_rc(sfx, **bad) == EINVAL, (sfx, bad)
        assert _sums_rc(sfx, rows=0) == 0 and _sums_rc(sfx, n_order=0) == 0          # nothing to do, with or without a device
    if lib.modl_device_count() == 0:
        assert _assign_rc() == ENOGPU and _sums_rc() == ENOGPU


# ------------------------------------------------------------------------------------------------ layer 2: the GPU
LSENT = -77


def run_assign(torch, X, Cs, active):
    """the C-ABI call: ldx = V + 3 with NaN after every row, guarded outputs, a NaN-poisoned workspace"""
    d, V = X.shape
    n, K = Cs.shape[:2]
    R, ldx = len(active), V + 3
    Xp = np.full((d, ldx), np.nan)
    Xp[:, :V] = X
    dX = torch.full((GUARD + d * ldx + GUARD,), float('nan'), dtype=torch.float64, device='cuda')
    dX[GUARD:GUARD + d * ldx] = torch.from_numpy(Xp.ravel()).cuda()
    dC, dA = torch.from_numpy(np.ascontiguousarray(Cs)).cuda(), torch.from_numpy(np.asarray(active, dtype=np.int32)).cuda()
    score, labels = _Guarded(n * V, torch.float64, -777.25), _Guarded(n * V, torch.int32, LSENT)
    need = lib.modl_kmeans_assign_workspace(V, d, K, R)
    assert 0 < need < max(V, 64) * K * 8
    ws = _NanWorkspace(need)
    rc = lib.modl_kmeans_assign_f64(C.c_void_p(dX.data_ptr() + GUARD * 8), ldx, V, d, C.c_void_p(dC.data_ptr()), K, n,
                                    C.c_void_p(dA.data_ptr()), R, score.ptr, labels.ptr, ws.ptr, need, None)
    assert rc == 0
    torch.cuda.synchronize()
    ws.check()
    return score.get().reshape(n, V), labels.get().reshape(n, V)


def check_assignment(X, Cc, score, labels):
    want, _ = _assign_host(X, Cc)
    assert assignment_gap(X, Cc) > GAP
    assert np.array_equal(labels, want)
    d, V = X.shape
    exact = ((Cc * Cc).sum(axis=1)[:, None] - 2.0 * (Cc @ X))[want, np.arange(V)]
    bound = 4 * (d + 4) * U * abs_sums(X, Cc)[want, np.arange(V)]
    print('largest score error / bound', np.max(np.abs(score - exact) / bound))
    assert np.all(np.abs(score - exact) <= bound)


def assign_shapes():
    return [(1, 1, 1)] + [TRAJECTORY[i] for i in (0, 2, 3, 6, 4, 5)] + [(5, 257, lib.modl_kmeans_max_clusters())]


@pytest.mark.gpu
@pytest.mark.parametrize('shape', assign_shapes(), ids=str)
def test_gpu_assignment_through_the_c_abi(gpu, shape):
    d, V, K = shape
    if shape in TRAJECTORY:
        X, _, _, traces = trajectory(shape)
        sets = [traces[0]['centers'][0], traces[0]['centers'][-1]]      # the judge's first and last assignment
    else:
        rng = np.random.RandomState(d + V + K)
        X = 3 * rng.randn(d, V)
        sets = [3 * rng.randn(K, d), 3 * rng.randn(K, d)]
    rng = np.random.RandomState(9)
    Cs = np.stack(sets + [sets[0] + 0.1 * rng.randn(K, d), sets[1] + 0.1 * rng.randn(K, d), sets[1][::-1].copy()])   # five sets
    active = [3, 0, 1]                                                  # a permuted subset of three
    score, labels = run_assign(gpu, X, Cs, active)
    for r in range(5):
        if r in active:
            check_assignment(X, Cs[r], score[r], labels[r])
        else:
            assert np.all(score[r] == -777.25) and np.all(labels[r] == LSENT)     # unlisted: the slots keep their poison
    again = run_assign(gpu, X, Cs, active)
    assert same_bits(score, again[0]) and same_bits(labels, again[1])   # the same bits from call to call
    for r in active:                                                    # and whoever is listed with it
        alone = run_assign(gpu, X, Cs, [r])
        assert same_bits(alone[0][r], score[r]) and same_bits(alone[1][r], labels[r])
        others = [q for q in range(5) if q != r]
        assert np.all(alone[0][others] == -777.25) and np.all(alone[1][others] == LSENT)


@pytest.mark.gpu
def test_gpu_assignment_ties_and_non_finite_voxels(gpu):
    X, init = duplicated_case()
    score, labels = run_assign(gpu, X, init[None], [0])
    check_assignment(X, init, score[0], labels[0])
    assert np.any(labels[0] == 2) and not np.any(labels[0] == 5)       # an exact tie: the lower index
    bad = X.copy()
    bad[3, 7], bad[0, 100], bad[5, 899] = np.nan, np.inf, -np.inf
    s2, l2 = run_assign(gpu, bad, init[None], [0])
    hit = np.zeros(900, dtype=bool)
    hit[[7, 100, 899]] = True
    assert np.all(l2[0][hit] == -1) and np.all(np.isnan(s2[0][hit]))
    assert same_bits(s2[0][~hit], score[0][~hit]) and same_bits(l2[0][~hit], labels[0][~hit])     # that voxel only


@pytest.mark.gpu
def test_gpu_entry_points_refuse_and_write_nothing(gpu):
    torch = gpu
    d, V, K, n = 3, 40, 4, 2
    X = torch.zeros((d, V), dtype=torch.float64, device='cuda')
    Cs = torch.zeros((n, K, d), dtype=torch.float64, device='cuda')
    act = torch.arange(n, dtype=torch.int32, device='cuda')
    score, labels = _Guarded(n * V, torch.float64, -777.25), _Guarded(n * V, torch.int32, LSENT)
    need = lib.modl_kmeans_assign_workspace(V, d, K, n)
    ws = _NanWorkspace(need)
    p = lambda t: C.c_void_p(t.data_ptr())

    def call(d=d, V=V, K=K, R=n, ldx=V, ws_bytes=need, wsp=ws.ptr, sc=score.ptr):
        return lib.modl_kmeans_assign_f64(p(X), ldx, V, d, p(Cs), K, n, p(act), R, sc, labels.ptr, wsp, ws_bytes, None)
    for bad in (dict(d=0), dict(K=0), dict(V=0), dict(R=0), dict(R=3), dict(ldx=V - 1), dict(sc=p(X)), dict(wsp=p(Cs))):
        assert call(**bad) == EINVAL, bad
    assert call(ws_bytes=need - 8) == ENOMEM and call(wsp=None) == ENOMEM
    torch.cuda.synchronize()
    assert np.all(score.get() == -777.25) and np.all(labels.get() == LSENT)     # a refused call writes nothing
    assert call() == 0
    torch.cuda.synchronize()
    assert np.all(score.get() == 0) and np.all(labels.get() == 0)       # all centres equal: the lowest index
    sums = _Guarded(d * K, torch.float64, -777.25)
    order, off = torch.arange(V, dtype=torch.int32, device='cuda'), torch.zeros(K + 1, dtype=torch.int64, device='cuda')
    f = lib.modl_label_sums_f64
    assert f(p(X), V, d, V, p(order), V, p(off), K, p(X), K, None) == EINVAL     # the output over the input
    assert f(p(X), V, 0, V, p(order), V, p(off), K, sums.ptr, K, None) == 0 and f(p(X), V, d, V, p(order), 0, p(off), K, sums.ptr, K, None) == 0
    torch.cuda.synchronize()
    assert np.all(sums.get() == -777.25)                                # no row, or no order: nothing is written
    assert f(p(X), V, d, V, p(order), V, p(off), K, sums.ptr, K, None) == 0
    torch.cuda.synchronize()
    assert np.all(sums.get() == 0)                                      # every label empty: zeros


def run_sums(torch, rows, order, offsets, K, pad=3):
    """modl_label_sums_* with ldx = V + pad (NaN after every row), lds = K + 2 inside guards"""
    T, V = rows.shape
    ldx, lds = V + pad, K + 2
    Xp = np.full((T, ldx), np.nan, dtype=rows.dtype)
    Xp[:, :V] = rows
    dX = torch.from_numpy(Xp).cuda()
    dO, dF = torch.from_numpy(np.asarray(order, dtype=np.int32)).cuda(), torch.from_numpy(np.asarray(offsets, dtype=np.int64)).cuda()
    out = _Guarded(T * lds, torch.float64, -777.25)
    f = lib.modl_label_sums_f32 if rows.dtype == np.float32 else lib.modl_label_sums_f64
    rc = f(C.c_void_p(dX.data_ptr()), ldx, T, V, C.c_void_p(dO.data_ptr()), len(order), C.c_void_p(dF.data_ptr()), K, out.ptr, lds, None)
    assert rc == 0
    torch.cuda.synchronize()
    got = out.get().reshape(T, lds)
    assert np.all(got[:, K:] == -777.25)
    return got[:, :K].copy()


def segments(keys, K):
    """keys in 0 .. K (K: in no segment) -> (order: a stable sort, offsets)"""
    order = np.argsort(keys, kind='stable').astype(np.int32)
    return order, np.concatenate([[0], np.cumsum(np.bincount(keys, minlength=K + 1)[:K])]).astype(np.int64)


def check_sums(got, rows, keys, K):
    worst = 0.0
    for c in range(K):
        x = rows[:, keys == c].astype(np.longdouble)
        n = x.shape[1]
        if n == 0:
            assert np.all(got[:, c] == 0)
            continue
        err, bound = np.abs(got[:, c] - x.sum(axis=1)).astype(np.float64), (n + 2) * U * np.abs(x).sum(axis=1).astype(np.float64)
        assert np.all(err <= bound), c
        worst = max(worst, float(np.max(err / np.maximum(bound, 1e-300))))
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('K', [1, 20, 1024])
@pytest.mark.parametrize('V', [1, 33, 4099])
@pytest.mark.parametrize('T', [1, 7, 130])
def test_gpu_label_sums_through_the_c_abi(gpu, T, V, K, dtype):
    rng = np.random.RandomState(T + V + K)
    rows = (rng.randn(T, V) + 1.0).astype(dtype)
    keys = rng.randint(0, K + 1, size=V)                                # K: in no segment; K > V leaves many labels empty
    if K > 1 and V > 1:
        keys[keys == 1] = 0                                             # an empty label in every case
    rows[:, keys == K] = np.nan                                         # never read into any sum
    order, offsets = segments(keys, K)
    got = run_sums(gpu, rows, order, offsets, K)
    print('largest error / bound', check_sums(got, rows, keys, K))
    assert same_bits(got, run_sums(gpu, rows, order, offsets, K))       # the same bits from call to call
    everything = np.zeros(V, dtype=np.int64)                            # one segment holding everything
    clean = np.where(np.isnan(rows), 1.0, rows).astype(dtype)
    o2, f2 = segments(everything, K)
    check_sums(run_sums(gpu, clean, o2, f2, K), clean, everything, K)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
def test_gpu_a_labels_sum_depends_on_its_own_segment_alone(gpu, dtype):
    """the bits of one label's sums are unchanged when the membership of the other labels, the other rows or K change; the
    segment is longer than one staged piece and the rows take both slab widths"""
    T, V, K, c = 130, 9001, 5, 2
    rng = np.random.RandomState(1)
    rows = rng.randn(T, V).astype(dtype)
    keys = rng.randint(0, K + 1, size=V)
    keys[rng.rand(V) < 0.5] = c                                         # ~ 5000 voxels: three staged pieces
    assert np.sum(keys == c) > 4096
    base = run_sums(gpu, rows, *segments(keys, K), K)
    other = keys.copy()
    moved = other != c
    other[moved] = rng.permutation(other[moved])                        # the other labels trade voxels
    other[moved & (rng.rand(V) < 0.3)] = K
    assert same_bits(run_sums(gpu, rows, *segments(other, K), K)[:, c], base[:, c])
    wide = np.where(keys == K, K + 7, keys)                             # K + 7 labels
    assert same_bits(run_sums(gpu, rows, *segments(wide, K + 7), K + 7)[:, c], base[:, c])
    few = run_sums(gpu, np.ascontiguousarray(rows[40:47]), *segments(keys, K), K)     # 7 rows: the narrow slab
    assert same_bits(few[:, c], base[40:47, c])
    assert same_bits(run_sums(gpu, rows, *segments(keys, K), K, pad=11)[:, c], base[:, c])


def _np(x):
    return x.cpu().numpy() if hasattr(x, 'cpu') else np.asarray(x)


def _host(res):
    return KMeansParcels(_np(res.labels), _np(res.centers), res.inertia, _np(res.n_iter), _np(res.converged), res.selected, _np(res.inertias))


@pytest.mark.gpu
@pytest.mark.parametrize('shape', TRAJECTORY, ids=str)
def test_gpu_kmeans_parcels_equals_the_twin(gpu, shape):
    X, init, want, _ = trajectory(shape)
    cuda = shape[1] % 2 == 0                                            # CUDA tensors in half of the cases
    got = kmeans_parcels(gpu.from_numpy(X).cuda() if cuda else X, shape[2], init=init, tol=0, max_iter=300)
    assert isinstance(got.labels, gpu.Tensor if cuda else np.ndarray)
    got = _host(got)
    print(shape, 'n_iter', got.n_iter, want.n_iter, 'inertia', got.inertia, want.inertia)
    assert got.labels.dtype == np.int32 and agrees(got, want, X)
    assert abs(got.inertia - want.inertia) <= 1e-12 * want.inertia


@pytest.mark.gpu
def test_gpu_kmeans_parcels_restarts_empties_and_tol(gpu):
    for key, (X, init) in (('dup', duplicated_case()), ('dup2', duplicated_case(2)), ('restarts', restart_case())):
        want, _ = judge(key, X, init)
        got = _host(kmeans_parcels(X, init.shape[-2], init=init, tol=0))
        assert agrees(got, want, X), key
        assert np.all(np.abs(got.inertias - want.inertias) <= 1e-12 * want.inertias)
    X, inits = restart_case()
    alone = _host(kmeans_parcels(X, 6, init=inits[2], tol=0))           # a restart does not depend on the others
    assert alone.n_iter[0] == want.n_iter[2] and abs(alone.inertia - want.inertias[2]) <= 1e-12 * alone.inertia
    X, init = blobs(5, 1500, 9, seed=3)                                 # the tolerance stop
    want, traces = judge('tol', X, init, tol=1e-4)
    shifts, thr = np.array(traces[0]['shifts']), traces[0]['tol']
    print('shifts', shifts, 'threshold', thr)
    assert thr > 0 and np.all(np.abs(shifts - thr) > 1e-6 * thr)       # no count can flip on rounding
    assert 0 < shifts[-1] <= thr and np.all(shifts[:-1] > thr)          # and the tolerance is what stopped it
    got = _host(kmeans_parcels(X, 9, init=init, tol=1e-4))
    assert agrees(got, want, X) and abs(got.inertia - want.inertia) <= 1e-12 * want.inertia


@pytest.mark.gpu
@pytest.mark.parametrize('shape', [(3, 600, 4), (17, 1037, 20)], ids=str)
def test_gpu_kmeans_init_equals_the_twin(gpu, shape):
    X, _ = blobs(*shape)
    want_c, want_v = kmeans_init_host(X, shape[2], n_init=3, random_state=7, return_voxels=True)
    assert init_rule_margin(X, want_v, 7) > GAP                         # the precondition
    got_c, got_v = kmeans_init(X, shape[2], n_init=3, random_state=7, return_voxels=True)
    assert np.array_equal(got_v, want_v) and same_bits(got_c, want_c)
    dev = kmeans_init(gpu.from_numpy(X).cuda(), shape[2], n_init=3, random_state=7)
    assert isinstance(dev, gpu.Tensor) and same_bits(_np(dev), want_c)
    a = _host(kmeans_parcels(X, shape[2], n_init=3, tol=0, random_state=7))
    b = kmeans_parcels_host(X, shape[2], n_init=3, tol=0, random_state=7)
    assert np.array_equal(a.labels, b.labels) and a.selected == b.selected


@pytest.mark.gpu
@pytest.mark.parametrize('cuda', [False, True])
@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
def test_gpu_label_signals_and_back(gpu, dtype, cuda):
    give = (lambda a: gpu.from_numpy(np.ascontiguousarray(a)).cuda()) if cuda else (lambda a: a)
    kind = gpu.Tensor if cuda else np.ndarray
    rows, labels, K = signal_case(dtype, T=130, V=4099, K=37)
    safe = np.where((labels >= 1) & (labels <= K), labels, 0)
    for strategy in ('mean', 'sum'):
        got, counts = label_signals(give(rows), give(labels), K, strategy)
        assert isinstance(got, kind) and isinstance(counts, kind)
        got, counts = _np(got), _np(counts)
        want, wc = label_signals_host(rows, labels, K, strategy)
        assert got.dtype == dtype and np.array_equal(counts, wc) and counts.dtype == np.int64
        for c in range(K):
            x = np.abs(rows[:, safe == c + 1].astype(np.float64)).sum(axis=1)
            div = counts[c] if strategy == 'mean' and counts[c] else 1
            # device and twin each lie within (n + 2) u sum |x| (/ n) of the exact value: twice that apart, plus the rounding to f32
            bound = 2 * (counts[c] + 2) * U * x / div + (np.finfo(np.float32).eps * np.abs(want[:, c]) if dtype == np.float32 else 0)
            assert np.all(np.abs(got[:, c].astype(np.float64) - want[:, c]) <= bound), (strategy, c)
    assert _np(label_signals(give(rows), give(labels))[0]).shape == (130, K + 2)
    signals = coarse_signals(5, K, dtype)
    back = signals_to_rows(give(signals), give(labels))
    assert isinstance(back, kind) and same_bits(_np(back), signals_to_rows_host(signals, labels))
    again, counts = label_signals(back, give(labels), K)                # piecewise-constant rows: bit for bit
    assert same_bits(_np(again)[:, _np(counts) > 0], signals[:, _np(counts) > 0])


def planted(seed, V, T, K, n_records):
    """(labels (V,) in 0 .. K - 1, the planted time courses, the records): the phantom of the issue"""
    rng = np.random.RandomState(seed)
    labels = rng.randint(K, size=V)
    courses, records = [], []
    for _ in range(n_records):
        tc = rng.randn(T, K)
        r = tc[:, labels] + 0.3 * rng.randn(T, V)
        r = r - r.mean(axis=0)
        records.append(r / r.std(axis=0))
        courses.append(tc)
    return labels, courses, records


def same_partition(a, b, K):
    """two labelings are one partition up to a permutation of the labels"""
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == K and len({p[0] for p in pairs}) == K and len({p[1] for p in pairs}) == K


@pytest.mark.gpu
@pytest.mark.parametrize('shape', PHANTOMS, ids=str)
def test_gpu_parcellate_recovers_planted_parcels(gpu, shape):
    V, T, K, n_records = shape
    truth, courses, records = planted(0, *shape)
    got = parcellate(records, K, n_components=K, n_init=3, random_state=0)
    assert isinstance(got, Parcellation) and isinstance(got.labels, np.ndarray) and got.labels.dtype == np.int32
    assert got.labels.min() == 1 and got.labels.max() == K and got.variance.shape == (K,)
    assert same_partition(got.labels, truth, K)                         # exactly, up to a permutation of the labels
    assert np.array_equal(got.sizes, np.bincount(got.labels - 1, minlength=K)) and got.kmeans.converged.all()
    for rec, tc in zip(records, courses):
        signals, counts = label_signals(rec, got.labels, K)
        assert np.array_equal(counts, got.sizes)
        for c in range(K):
            planted_label = truth[np.flatnonzero(got.labels == c + 1)[0]]
            assert np.corrcoef(signals[:, c], tc[:, planted_label])[0, 1] > 0.99
    dev = parcellate([gpu.from_numpy(r).cuda() for r in records], K, n_components=K, n_init=3, random_state=0)
    assert isinstance(dev.labels, gpu.Tensor) and np.array_equal(_np(dev.labels), got.labels)


@pytest.mark.gpu
def test_gpu_fmri_parcellation(gpu):
    from modl_amd import ConnectivityMeasure
    from modl_amd.signal import clean
    truth, _, records = planted(1, 600, 24, 4, 2)
    flat = np.zeros(12 * 10 * 8, dtype=bool)
    flat[:600] = True
    mask = np.random.RandomState(1).permutation(flat).reshape(12, 10, 8)
    kw = dict(n_parcels=4, n_components=4, n_init=3, random_state=0, mask=mask, standardize=True, detrend=True)
    est = fMRIParcellation(**kw).fit(records)
    assert est.labels_.shape == (600,) and est.labels_.dtype == np.int32 and same_partition(est.labels_, truth, 4)
    assert np.array_equal(est.parcel_sizes_, np.bincount(est.labels_ - 1, minlength=4)) and est.variance_.shape == (4,)
    assert isinstance(est.kmeans_, KMeansParcels) and isinstance(est.kmeans_.centers, np.ndarray)
    assert est.labels_img_.shape == mask.shape and est.labels_img_.dtype == np.int32
    assert np.all(est.labels_img_[~mask] == 0) and np.array_equal(est.labels_img_[mask], est.labels_)
    assert np.array_equal(fMRIParcellation(**kw).fit(records).labels_, est.labels_)
    signals = est.transform(records)
    for rec, s in zip(records, signals):
        want, _ = label_signals(clean(rec, detrend=True, standardize=True), est.labels_, 4)
        assert s.shape == (24, 4) and same_bits(s, want)
    volume = np.zeros(mask.shape + (24,))
    volume[mask] = records[0].T                                         # a 4-D record under the mask: the same signals
    assert same_bits(est.transform([volume])[0], signals[0])
    back = est.inverse_transform(signals)
    assert back[0].shape == (24, 600)
    for c in range(4):
        assert same_bits(back[0][:, est.labels_ == c + 1], np.repeat(signals[0][:, [c]], est.parcel_sizes_[c], axis=1))
    again = est.transform(back)                                         # piecewise constant with the parcel means
    assert np.allclose(again[0], clean(signals[0], detrend=True, standardize=True), atol=1e-10)
    conn = ConnectivityMeasure(kind='correlation').fit_transform(signals)
    conn = _np(conn)
    assert conn.shape == (2, 4, 4) and np.array_equal(conn, conn.transpose(0, 2, 1)) and np.all(np.diagonal(conn, axis1=1, axis2=2) == 1)
