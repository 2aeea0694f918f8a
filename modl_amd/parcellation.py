"""Hard parcellation on the device: k-means parcels of the group components, and label signals (DESIGN.md section 31,
csrc/kmeans.hip).  Every mask voxel belongs to exactly one of K parcels; the per-parcel mean time series are the region
signals - nilearn's `Parcellations(method='kmeans')` plus `NiftiLabelsMasker`.

    1. kmeans_init       plain k-means++ on the voxels of the (d, V) components;
    2. kmeans_parcels    Lloyd's algorithm, all restarts at once: per iteration one modl_kmeans_assign_f64 over the restarts
                         still running (the V x K scores never exist), one stable sort of the labels, and one
                         modl_label_sums_f64 per running restart for the new centres;
    3. label_signals     the mean (or sum) of the rows over every label, through the same segmented-sum kernel;
       signals_to_rows   its inverse: every voxel gets its parcel's signal;
    4. parcellate        reduce_record -> group_components (modl_amd.canica) -> kmeans_parcels on a list of cleaned records.

The rules of kmeans_parcels.  The first three are those of sklearn's KMeans(algorithm='lloyd'), so sklearn can judge: a restart
stops when its labels equal those of the previous iteration; it also stops when the squared centre shift is at most `tol` times
the mean over features of the variance over voxels, and one final assignment then makes labels and centres agree; empty
clusters, taken in ascending index, are moved onto the voxels farthest from their centres - those in descending
score + |x|^2, ties to the lower voxel index - and each moved voxel is subtracted from the cluster it leaves (sklearn leaves
the order among several empty clusters unspecified).  inertia is the sum over voxels of score + |x|^2 with the score of the
last assignment; the restart with the smallest inertia is selected, ties to the lower index.  n_iter counts the iterations
that changed the labels (sklearn counts the closing iteration too).  Labels are 1 .. K; 0 is "no parcel", as in region_labels.

Where this departs from nilearn (nilearn is not installed where this was written: its Parcellations is described here from
its documented algorithm and has not been run against this): nilearn clusters the same group-PCA basis with
MiniBatchKMeans; this is full-batch Lloyd with restarts, whose fixed point does not depend on a batch order.  The seeding
is plain k-means++, one candidate per step; sklearn's greedy variant tries 2 + log(K) candidates and keeps the best.

Every function takes numpy arrays or CUDA tensors and answers in kind; a numpy input without a GPU goes through the `*_host`
twin: plain numpy, what runs without a GPU, the judge of the tests and the CPU baseline of scripts/bench_parcellation.py."""
from collections import namedtuple

import numpy as np
import torch
from sklearn.utils import check_random_state

from ._lib import lib
from .canica import _check_2d, _check_records, reduce_record, group_components, reduce_record_host, group_components_host
from .device import STREAM, as_float_tensor, call, have_gpu, is_cuda, like_input, scratch

__all__ = ['KMeansParcels', 'Parcellation', 'kmeans_init', 'kmeans_parcels', 'label_signals', 'signals_to_rows', 'parcellate',
           'kmeans_init_host', 'kmeans_parcels_host', 'label_signals_host', 'signals_to_rows_host', 'parcellate_host',
           'kmeans_trace_host', 'kmeans_assign', 'label_sums']

KMeansParcels = namedtuple('KMeansParcels', ['labels', 'centers', 'inertia', 'n_iter', 'converged', 'selected', 'inertias'])
Parcellation = namedtuple('Parcellation', ['labels', 'sizes', 'variance', 'kmeans'])
ASSIGN_CHUNK = 8192                                         # voxels per K x chunk temporary of the host twin


# ---- arguments
def _is_int(x):
    return isinstance(x, (int, np.integer)) and not isinstance(x, bool)


def _check_parcels(n_parcels, V):
    if not _is_int(n_parcels) or n_parcels < 1:
        raise ValueError('n_parcels must be a positive integer, got %r' % (n_parcels,))
    if n_parcels > lib.modl_kmeans_max_clusters():
        raise ValueError('kmeans_parcels takes at most %d parcels, got %d' % (lib.modl_kmeans_max_clusters(), n_parcels))
    if n_parcels > V:
        raise ValueError('n_parcels = %d is larger than the %d voxels' % (n_parcels, V))
    return int(n_parcels)


def _check_kmeans_scalars(d, n_init, tol, max_iter):
    if d > lib.modl_kmeans_max_features():
        raise ValueError('kmeans_parcels takes at most %d components, got %d' % (lib.modl_kmeans_max_features(), d))
    if not _is_int(max_iter) or max_iter < 1:
        raise ValueError('max_iter must be a positive integer, got %r' % (max_iter,))
    if isinstance(tol, (str, bool)) or not tol >= 0:
        raise ValueError('tol must be non-negative, got %r' % (tol,))
    if not _is_int(n_init) or n_init < 1 or n_init > 65535:
        raise ValueError('n_init must be an integer in 1 .. 65535, got %r' % (n_init,))


def _check_init(init, K, d):
    """a given init as a float64 numpy array (n_init, K, d); (K, d) is one restart"""
    if isinstance(init, torch.Tensor):
        init = init.detach().cpu().numpy()
    init = np.array(init, dtype=np.float64)
    if init.ndim == 2:
        init = init[None]
    if init.ndim != 3 or init.shape[0] < 1 or init.shape[1:] != (K, d):
        raise ValueError('init must be (n_init, %d, %d), got shape %s' % (K, d, init.shape))
    if init.shape[0] > 65535:
        raise ValueError('n_init must be an integer in 1 .. 65535, got %d' % init.shape[0])
    if not np.all(np.isfinite(init)):
        raise ValueError('init holds non-finite values')
    return np.ascontiguousarray(init)


def _not_finite():
    return ValueError('components holds non-finite values: k-means needs finite input')


# ---- the kernels on CUDA tensors
def kmeans_assign(X, C, active, score=None, labels=None, ws=None):
    """One launch of modl_kmeans_assign_f64 on CUDA tensors: X (d, V) float64 with contiguous rows, C (n, K, d) float64
    contiguous, active (R,) int32 -> (score (n, V) float64, labels (n, V) int32, 0-based); only the rows of the listed sets are
    written."""
    d, V = X.shape
    n, K = C.shape[:2]
    R = int(active.shape[0])
    if score is None:
        score = torch.zeros((n, V), dtype=torch.float64, device=X.device)
    if labels is None:
        labels = torch.full((n, V), -1, dtype=torch.int32, device=X.device)
    need = lib.modl_kmeans_assign_workspace(V, d, K, R)
    if ws is None:
        ws = scratch(need, X.device)
    elif ws.numel() < need:
        raise ValueError('kmeans_assign: the workspace holds %d bytes, %d sets need %d' % (ws.numel(), R, need))
    call('modl_kmeans_assign_f64', X, X.stride(0) if d > 1 else V, V, d, C, K, n, active, R, score, labels, ws, ws.numel(),
         STREAM, device=X.device)
    return score, labels


def label_sums(rows, order, offsets, sums=None):
    """One launch of modl_label_sums_*: rows (T, V) float32 / float64 CUDA tensor with contiguous rows, order (n,) int32,
    offsets (K + 1,) int64 -> sums (T, K) float64."""
    T, V = rows.shape
    K = int(offsets.shape[0]) - 1
    if sums is None:
        sums = torch.zeros((T, K), dtype=torch.float64, device=rows.device)
    call('modl_label_sums', rows, rows.stride(0) if T > 1 else V, T, V, order, int(order.shape[0]), offsets, K, sums,
         sums.stride(0) if T > 1 else K, STREAM, device=rows.device, dtype=rows)
    return sums


def _segments(keys, K):
    """keys (..., V) int64 in 0 .. K (K: in no segment) -> (order int32 (..., V): a stable sort, counts int64 (..., K),
    offsets int64 (..., K + 1))"""
    order = torch.sort(keys, dim=-1, stable=True).indices.to(torch.int32)
    counts = torch.zeros(keys.shape[:-1] + (K + 1,), dtype=torch.int64, device=keys.device)
    counts.scatter_add_(-1, keys, torch.ones_like(keys))
    counts = counts[..., :K].contiguous()
    offsets = torch.zeros(keys.shape[:-1] + (K + 1,), dtype=torch.int64, device=keys.device)
    offsets[..., 1:] = counts.cumsum(-1)
    return order.contiguous(), counts, offsets


# ---- k-means++
def _init_draws(rs, V, K, n_init):
    """per restart: (the first voxel, the K - 1 uniform draws), in the order the generator is consumed"""
    return [(int(rs.randint(V)), rs.random_sample(K - 1)) for _ in range(n_init)]


def kmeans_init(components, n_parcels, n_init=1, random_state=None, return_voxels=False):
    """Plain k-means++ on the V columns of (d, V) components -> centres (n_init, K, d) float64 (with return_voxels=True also
    the chosen voxels (n_init, K)).  Per restart: the first centre is voxel rng.randint(V); each further centre is the first
    voxel whose inclusive float64 cumulative sum of the current squared distances (to the nearest centre so far) exceeds
    rng.random_sample() * total.  One candidate per step: sklearn's greedy variant tries 2 + log(K) and keeps the best.  On
    the device distances, cumulative sum and search are torch and nothing is transferred until the end; host and device can
    pick different voxels only when a draw falls within rounding of a boundary of the cumulative sum."""
    cuda = is_cuda(components)
    if not cuda and not have_gpu():
        return kmeans_init_host(components, n_parcels, n_init, random_state, return_voxels)
    X = as_float_tensor(components).to(torch.float64)
    _check_2d(X, 'components')
    d, V = X.shape
    K = _check_parcels(n_parcels, V)
    _check_kmeans_scalars(d, n_init, 0.0, 1)
    with torch.cuda.device(X.device):
        if not bool(torch.isfinite(X).all()):
            raise _not_finite()
        vox = torch.empty((n_init, K), dtype=torch.int64, device=X.device)
        for r, (first, draws) in enumerate(_init_draws(check_random_state(random_state), V, K, n_init)):
            vox[r, 0] = first
            closest = ((X - X[:, first:first + 1]) ** 2).sum(dim=0)
            for c in range(1, K):
                cum = closest.cumsum(0)
                v = torch.searchsorted(cum, (cum[-1] * float(draws[c - 1])).reshape(1), right=True).clamp_(max=V - 1)
                vox[r, c] = v[0]
                closest = torch.minimum(closest, ((X - X[:, v]) ** 2).sum(dim=0))
        centers = X[:, vox.reshape(-1)].T.reshape(n_init, K, d).contiguous()
    if return_voxels:
        return like_input(centers, cuda), like_input(vox, cuda)
    return like_input(centers, cuda)


def kmeans_init_host(components, n_parcels, n_init=1, random_state=None, return_voxels=False):
    """`kmeans_init` in numpy"""
    X = np.asarray(components, dtype=np.float64)
    _check_2d(X, 'components')
    d, V = X.shape
    K = _check_parcels(n_parcels, V)
    _check_kmeans_scalars(d, n_init, 0.0, 1)
    if not np.all(np.isfinite(X)):
        raise _not_finite()
    vox = np.empty((n_init, K), dtype=np.int64)
    for r, (first, draws) in enumerate(_init_draws(check_random_state(random_state), V, K, n_init)):
        vox[r, 0] = first
        closest = ((X - X[:, first:first + 1]) ** 2).sum(axis=0)
        for c in range(1, K):
            cum = np.cumsum(closest)
            v = min(int(np.searchsorted(cum, cum[-1] * draws[c - 1], side='right')), V - 1)
            vox[r, c] = v
            closest = np.minimum(closest, ((X - X[:, v:v + 1]) ** 2).sum(axis=0))
    centers = np.ascontiguousarray(X[:, vox.reshape(-1)].T.reshape(n_init, K, d))
    return (centers, vox) if return_voxels else centers


# ---- Lloyd
def _relocate(X, lab, dist, sums, counts):
    """the empty clusters of one restart, in place (module docstring); X (d, V), lab (V,), dist (V,), sums (d, K), counts (K,):
    CUDA tensors.  The rare path: it synchronises."""
    empty = torch.nonzero(counts == 0).flatten().tolist()
    far = torch.sort(dist, descending=True, stable=True).indices[:len(empty)].tolist()
    for cid, v in zip(empty, far):
        old = int(lab[v])
        sums[:, old] -= X[:, v]
        sums[:, cid] = X[:, v]
        counts[old] -= 1
        counts[cid] = 1


def _centers_of(sums, counts, old):
    """sums (.., d, K), counts (.., K), old (.., K, d) -> (.., K, d): the means; a cluster left without a voxel keeps its centre"""
    cnt = counts[..., :, None].to(torch.float64)
    return torch.where(cnt > 0, sums.transpose(-1, -2) / cnt.clamp_min(1.0), old)


def kmeans_parcels(components, n_parcels, n_init=3, init=None, tol=1e-4, max_iter=300, random_state=None):
    """Lloyd's k-means of the V columns of (d, V) components into K = n_parcels parcels, all restarts at once (module
    docstring: the rules).  `components` is converted to float64; non-finite input is a ValueError.  `init` (n_init, K, d) or
    (K, d), or None: `kmeans_init` with `random_state`.

    Returns KMeansParcels(labels (V,) int32 in 1 .. K, centers (K, d), inertia, n_iter (n_init,), converged (n_init,), selected,
    inertias (n_init,)): labels, centres and inertia of the selected restart."""
    cuda = is_cuda(components)
    if not cuda and not have_gpu():
        return kmeans_parcels_host(components, n_parcels, n_init, init, tol, max_iter, random_state)
    X = as_float_tensor(components).to(torch.float64).contiguous()
    _check_2d(X, 'components')
    d, V = X.shape
    K = _check_parcels(n_parcels, V)
    _check_kmeans_scalars(d, n_init if init is None else 1, tol, max_iter)
    dev = X.device
    with torch.cuda.device(dev):
        if not bool(torch.isfinite(X).all()):
            raise _not_finite()
        if init is None:
            C = kmeans_init(X, K, n_init, random_state)
        else:
            C = torch.from_numpy(_check_init(init, K, d)).to(dev)
        n = C.shape[0]
        xn2 = (X * X).sum(dim=0)
        tol_abs = float(X.var(dim=1, unbiased=False).mean()) * tol
        score = torch.zeros((n, V), dtype=torch.float64, device=dev)
        labels = torch.full((n, V), -1, dtype=torch.int32, device=dev)
        prev = torch.full((n, V), -2, dtype=torch.int32, device=dev)
        ws = scratch(lib.modl_kmeans_assign_workspace(V, d, K, n), dev)
        run, strict = np.ones(n, dtype=bool), np.zeros(n, dtype=bool)
        converged, n_iter = np.zeros(n, dtype=bool), np.zeros(n, dtype=np.int64)
        for it in range(1, max_iter + 1):
            idx = np.flatnonzero(run)
            if not len(idx):
                break
            active = torch.from_numpy(idx.astype(np.int32)).to(dev)
            kmeans_assign(X, C, active, score, labels, ws)
            a64 = active.long()
            lab = labels[a64]
            same = (lab == prev[a64]).all(dim=1)
            # every running restart is sorted and summed by itself, and the kernels' orders of addition do not depend on the
            # other restarts: a restart's bits do not depend on which others are still running
            order, counts, offsets = _segments(lab.long(), K)
            sums = torch.zeros((len(idx), d, K), dtype=torch.float64, device=dev)
            for j in range(len(idx)):
                label_sums(X, order[j], offsets[j], sums[j])
            old = C[a64]
            new = _centers_of(sums, counts, old)
            shift = ((new - old) ** 2).sum(dim=(1, 2))
            state = torch.stack([same.to(torch.float64), (counts == 0).sum(dim=1).to(torch.float64), shift]).cpu().numpy()
            for j, r in enumerate(idx):                                 # the one transfer of an iteration, empty clusters apart
                if state[0, j] > 0:
                    run[r], strict[r], converged[r] = False, True, True
                    continue
                if state[1, j] > 0:
                    _relocate(X, lab[j], score[r] + xn2, sums[j], counts[j])
                    new[j] = _centers_of(sums[j], counts[j], old[j])
                    state[2, j] = float(((new[j] - old[j]) ** 2).sum())
                C[r], prev[r], n_iter[r] = new[j], lab[j], it
                if state[2, j] <= tol_abs:
                    run[r], converged[r] = False, True
        last = np.flatnonzero(~strict)
        if len(last):                                                   # labels and centres agree
            kmeans_assign(X, C, torch.from_numpy(last.astype(np.int32)).to(dev), score, labels, ws)
        inertias = (score + xn2).sum(dim=1).cpu().numpy()
        selected = int(np.argmin(inertias))
        out_labels = labels[selected] + 1
        centers = C[selected].clone()
    if cuda:
        return KMeansParcels(out_labels, centers, float(inertias[selected]), torch.from_numpy(n_iter).to(dev),
                             torch.from_numpy(converged).to(dev), selected, torch.from_numpy(inertias).to(dev))
    return KMeansParcels(out_labels.cpu().numpy(), centers.cpu().numpy(), float(inertias[selected]), n_iter, converged, selected,
                         inertias)


def _assign_host(X, C):
    """(labels (V,) int64 0-based: the lowest index of the minimum, score (V,)) of score = min_c |C_c|^2 - 2 C_c . x"""
    V = X.shape[1]
    cn = np.einsum('kj,kj->k', C, C)
    labels, score = np.empty(V, dtype=np.int64), np.empty(V)
    for a in range(0, V, ASSIGN_CHUNK):
        S = cn[:, None] - 2.0 * (C @ X[:, a:a + ASSIGN_CHUNK])
        lab = S.argmin(axis=0)
        labels[a:a + ASSIGN_CHUNK] = lab
        score[a:a + ASSIGN_CHUNK] = S[lab, np.arange(S.shape[1])]
    return labels, score


def _sums_host(X, labels, K):
    """(sums (rows, K) float64, counts (K,)) over the labels 0 .. K - 1; any other label is in no segment"""
    ok = (labels >= 0) & (labels < K)
    lab = np.where(ok, labels, K)
    sums = np.stack([np.bincount(lab, weights=row, minlength=K + 1)[:K] for row in X]) if len(X) else np.zeros((0, K))
    return sums, np.bincount(lab, minlength=K + 1)[:K]


def _lloyd_host(X, xn2, C, tol_abs, max_iter, trace=None):
    prev, n_iter, converged, strict = None, 0, False, False
    for it in range(1, max_iter + 1):
        labels, score = _assign_host(X, C)
        if trace is not None:
            trace['centers'].append(C.copy())
        if prev is not None and np.array_equal(labels, prev):
            converged = strict = True
            break
        sums, counts = _sums_host(X, labels, C.shape[0])
        empty = np.flatnonzero(counts == 0)
        if len(empty):
            far = np.argsort(-(score + xn2), kind='stable')[:len(empty)]
            for cid, v in zip(empty, far):
                old = labels[v]
                sums[:, old] -= X[:, v]
                sums[:, cid] = X[:, v]
                counts[old] -= 1
                counts[cid] = 1
        new = np.where(counts[:, None] > 0, sums.T / np.maximum(counts, 1)[:, None], C)
        shift = float(((new - C) ** 2).sum())
        if trace is not None:
            trace['shifts'].append(shift)
            trace['empty'].append(len(empty))
        C, prev, n_iter = new, labels, it
        if shift <= tol_abs:
            converged = True
            break
    if not strict:
        labels, score = _assign_host(X, C)
        if trace is not None:
            trace['centers'].append(C.copy())
    return labels, C, float((score + xn2).sum()), n_iter, converged


def _kmeans_host(components, n_parcels, n_init, init, tol, max_iter, random_state, traces=None):
    X = np.asarray(components, dtype=np.float64)
    _check_2d(X, 'components')
    d, V = X.shape
    K = _check_parcels(n_parcels, V)
    _check_kmeans_scalars(d, n_init if init is None else 1, tol, max_iter)
    if not np.all(np.isfinite(X)):
        raise _not_finite()
    C0 = kmeans_init_host(X, K, n_init, random_state) if init is None else _check_init(init, K, d)
    xn2 = (X * X).sum(axis=0)
    tol_abs = float(X.var(axis=1).mean()) * tol
    runs = []
    for r in range(C0.shape[0]):
        if traces is not None:
            traces.append({'centers': [], 'shifts': [], 'empty': [], 'tol': tol_abs})
        runs.append(_lloyd_host(X, xn2, C0[r].copy(), tol_abs, max_iter, None if traces is None else traces[-1]))
    inertias = np.array([r[2] for r in runs])
    selected = int(np.argmin(inertias))
    return KMeansParcels((runs[selected][0] + 1).astype(np.int32), runs[selected][1], float(inertias[selected]),
                         np.array([r[3] for r in runs], dtype=np.int64), np.array([r[4] for r in runs], dtype=bool), selected, inertias)


def kmeans_parcels_host(components, n_parcels, n_init=3, init=None, tol=1e-4, max_iter=300, random_state=None):
    """`kmeans_parcels` in numpy, one restart at a time"""
    return _kmeans_host(components, n_parcels, n_init, init, tol, max_iter, random_state)


def kmeans_trace_host(components, init, tol=1e-4, max_iter=300):
    """What `kmeans_parcels_host` passes through on the same arguments: per restart a dict with `centers` (the (K, d) centres of
    every assignment, the closing one included), `shifts` (the squared centre shift of every update), `empty` (the number of
    empty clusters of every update) and `tol` (the absolute threshold the shifts are compared with).  The tests assert on it
    that no assignment comes near a tie and no shift near the threshold."""
    init = np.asarray(init, dtype=np.float64)
    traces = []
    _kmeans_host(components, int(init.shape[-2]), 1, init, tol, max_iter, None, traces)
    return traces


# ---- label signals
def _check_strategy(strategy):
    if strategy not in ('mean', 'sum'):
        raise ValueError("strategy must be 'mean' or 'sum', got %r" % (strategy,))


def _check_labels(labels, V, n_labels):
    if labels.ndim != 1 or labels.shape[0] != V:
        raise ValueError('labels must be (%d,), one per voxel, got shape %s' % (V, tuple(labels.shape)))
    if n_labels is not None and (not _is_int(n_labels) or n_labels < 1):
        raise ValueError('n_labels must be a positive integer, got %r' % (n_labels,))


def label_signals(rows, labels, n_labels=None, strategy='mean'):
    """(T, V) rows and (V,) integer labels -> (signals (T, K) in the dtype of `rows` (float32 / float64), counts (K,) int64):
    column c - 1 is the mean (strategy='sum': the sum) of the voxels labelled c, accumulated in float64 by modl_label_sums_*;
    K = n_labels, or the largest label.  Labels outside 1 .. K are ignored (0 is "no parcel"); an empty label gives a column of
    zeros."""
    _check_strategy(strategy)
    cuda = is_cuda(rows)
    if isinstance(labels, torch.Tensor) and not cuda:
        labels = labels.detach().cpu().numpy()
    if not cuda and not have_gpu():
        return label_signals_host(rows, labels, n_labels, strategy)
    R = as_float_tensor(rows).contiguous()
    _check_2d(R, 'rows')
    lab = labels if isinstance(labels, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(labels)))
    if lab.dtype.is_floating_point or lab.dtype == torch.bool:
        raise ValueError('labels must be integers, got %s' % lab.dtype)
    _check_labels(lab, R.shape[1], n_labels)
    with torch.cuda.device(R.device):
        lab = lab.to(R.device).long()
        K = int(n_labels) if n_labels is not None else max(int(lab.max()), 1)
        keys = torch.where((lab >= 1) & (lab <= K), lab - 1, torch.full_like(lab, K))
        order, counts, offsets = _segments(keys, K)
        sums = label_sums(R, order, offsets)
        if strategy == 'mean':
            sums = torch.where(counts > 0, sums / counts.clamp_min(1).to(torch.float64), torch.zeros_like(sums))
        signals = sums.to(R.dtype)
    return like_input(signals, cuda), like_input(counts, cuda)


def label_signals_host(rows, labels, n_labels=None, strategy='mean'):
    """`label_signals` in numpy: one np.bincount per row, float64 sums"""
    _check_strategy(strategy)
    R = np.asarray(rows)
    if R.dtype not in (np.float32, np.float64):
        R = R.astype(np.float64)
    _check_2d(R, 'rows')
    lab = np.asarray(labels)
    if lab.dtype.kind not in 'iu':
        raise ValueError('labels must be integers, got %s' % lab.dtype)
    _check_labels(lab, R.shape[1], n_labels)
    lab = lab.astype(np.int64)
    K = int(n_labels) if n_labels is not None else max(int(lab.max()), 1)
    sums, counts = _sums_host(R, lab - 1, K)
    if strategy == 'mean':
        sums = np.where(counts > 0, sums / np.maximum(counts, 1), 0.0)
    return sums.astype(R.dtype), counts.astype(np.int64)


def signals_to_rows(signals, labels):
    """The inverse of `label_signals`: (T, K) signals and (V,) labels -> rows (T, V) with rows[t, v] = signals[t, labels[v] - 1],
    0 where the label is outside 1 .. K.  Indexing only: torch on a CUDA tensor, numpy otherwise."""
    if not is_cuda(signals):
        if isinstance(labels, torch.Tensor):
            labels = labels.detach().cpu().numpy()
        return signals_to_rows_host(signals, labels)
    _check_2d(signals, 'signals')
    lab = labels if isinstance(labels, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(labels)))
    if lab.ndim != 1:
        raise ValueError('labels must be 1-D, got shape %s' % (tuple(lab.shape),))
    lab = lab.to(signals.device).long()
    ok = (lab >= 1) & (lab <= signals.shape[1])
    return torch.where(ok, signals[:, torch.where(ok, lab - 1, torch.zeros_like(lab))], torch.zeros((), dtype=signals.dtype, device=signals.device))


def signals_to_rows_host(signals, labels):
    """`signals_to_rows` in numpy"""
    S = np.asarray(signals)
    _check_2d(S, 'signals')
    lab = np.asarray(labels).astype(np.int64)
    if lab.ndim != 1:
        raise ValueError('labels must be 1-D, got shape %s' % (lab.shape,))
    ok = (lab >= 1) & (lab <= S.shape[1])
    return np.where(ok, S[:, np.where(ok, lab - 1, 0)], np.zeros((), dtype=S.dtype))


# ---- the pipeline
def _sizes(labels, K):
    if isinstance(labels, torch.Tensor):
        return torch.bincount(labels.long() - 1, minlength=K)
    return np.bincount(labels.astype(np.int64) - 1, minlength=K)


def parcellate(records, n_parcels, n_components=20, n_init=3, tol=1e-4, max_iter=300, random_state=None):
    """Parcels of a list of cleaned (T_i, V) records: reduce_record on each, group_components (modl_amd.canica: the basis
    nilearn clusters), kmeans_parcels on the (n_components, V) basis.  Returns Parcellation(labels (V,) int32 in 1 .. K,
    sizes (K,), variance (n_components,), kmeans: the KMeansParcels record).  ValueError: n_components larger than the
    shortest record."""
    records = _check_records(records, n_components, 'parcellate', same_width=True)
    cuda = any(is_cuda(r) for r in records)
    if not cuda and not have_gpu():
        return parcellate_host(records, n_parcels, n_components, n_init, tol, max_iter, random_state)
    K = _check_parcels(n_parcels, records[0].shape[1])
    _check_kmeans_scalars(n_components, n_init, tol, max_iter)
    device = next((r.device for r in records if isinstance(r, torch.Tensor)), None)
    reduced = [reduce_record(as_float_tensor(r, device), n_components) for r in records]
    comp, variance = group_components(reduced, n_components)
    del reduced
    km = kmeans_parcels(comp, K, n_init, None, tol, max_iter, random_state)
    if cuda:
        return Parcellation(km.labels, _sizes(km.labels, K), variance, km)
    km = KMeansParcels(km.labels.cpu().numpy(), km.centers.cpu().numpy(), km.inertia, km.n_iter.cpu().numpy(),
                       km.converged.cpu().numpy(), km.selected, km.inertias.cpu().numpy())
    return Parcellation(km.labels, _sizes(km.labels, K), variance.cpu().numpy(), km)


def parcellate_host(records, n_parcels, n_components=20, n_init=3, tol=1e-4, max_iter=300, random_state=None):
    """`parcellate` through the host twins"""
    records = _check_records(records, n_components, 'parcellate', same_width=True)
    K = _check_parcels(n_parcels, records[0].shape[1])
    _check_kmeans_scalars(n_components, n_init, tol, max_iter)
    comp, variance = group_components_host([reduce_record_host(r, n_components) for r in records], n_components)
    km = kmeans_parcels_host(comp, K, n_init, None, tol, max_iter, random_state)
    return Parcellation(km.labels, _sizes(km.labels, K), variance, km)
