"""CanICA on the device: starting maps for fMRIDictFact from nothing but the records (csrc/ica.hip).

    1. reduce_record       every cleaned record (T, V) to its k leading right singular vectors times their singular values
                           (nilearn's per-subject PCA at reduction_ratio='auto'), through the T x T Gram matrix;
    2. group_components    the reductions stacked, every row scaled to unit norm (the CCA step of nilearn's _MultiPCA), the
                           top-k right singular vectors of the stack: an orthonormal basis of the group subspace;
    3. fastica_maps        symmetric FastICA on that basis, `n_init` restarts at once: centring over voxels, SYMMETRIC
                           whitening X1 = C^{-1/2} (X - mean), then per iteration one fused sweep of modl_ica_sweep_f64 (all
                           running restarts; the k x V sources never leave the registers) and sklearn's symmetric
                           decorrelation batched over the restarts with torch; the restart with the smallest
                           max_i sum_v |maps[i, v]| among those that did not fail is selected;
    4. threshold_maps      entries below scipy.stats.scoreatpercentile(|maps|, 100 - 100 / k * ratio) become 0, then every
                           map with max < -min changes sign.

The two Gram products, the projections and the small eigenproblems are library plumbing through torch (f64, chunked over V);
the FastICA sweep is the hand-written kernel.  Every function takes numpy arrays or CUDA tensors and answers in kind; a
numpy input without a GPU goes through the `*_host` twin.

Where this departs from sklearn / nilearn (nilearn is not installed where this was written: its CanICA is described here
from its documented algorithm and has not been run against this): whitening uses the symmetric inverse square root, not
sklearn's PCA whitening - the two differ by a rotation that ICA absorbs, and the symmetric root is a continuous function
of the input also where the covariance has equal eigenvalues, which after the group PCA is the normal case; the PCA steps
use the exact Gram route, not a randomized SVD; a restart whose unmixing matrix turns non-finite is a reported state
(`failed`), not an error, unless every restart fails.

The `*_host` twins are numpy / scipy and sklearn.decomposition.fastica (whiten=False on the symmetrically whitened rows, one
restart at a time): what runs without a GPU, the judge of the tests and the CPU baseline of scripts/bench_canica.py."""
import warnings
from collections import namedtuple

import numpy as np
import scipy.linalg
import scipy.stats
import torch
from sklearn.exceptions import ConvergenceWarning
from sklearn.utils import check_random_state

from ._lib import lib
from .device import STREAM, as_float_tensor, call, have_gpu, is_cuda, like_input, scratch

__all__ = ['IcaMaps', 'Canica', 'reduce_record', 'group_components', 'fastica_maps', 'threshold_maps', 'canica',
           'reduce_record_host', 'group_components_host', 'fastica_maps_host', 'threshold_maps_host', 'canica_host',
           'fastica_lims_host', 'ica_sweep']

IcaMaps = namedtuple('IcaMaps', ['maps', 'W', 'n_iter', 'converged', 'failed', 'selected'])
Canica = namedtuple('Canica', ['maps', 'variance', 'ica'])
FUNS = {'cube': 0, 'logcosh': 1, 'exp': 2}
GRAM_CHUNK = 1 << 16                                        # voxels per f64 temporary of the Gram route


# ---- arguments
def _check_2d(a, what):
    if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError('%s must be a 2-D array with at least one row and one column, got shape %s' % (what, tuple(a.shape)))


def _check_k(n_components, rows, what):
    if isinstance(n_components, bool) or not isinstance(n_components, (int, np.integer)) or n_components < 1:
        raise ValueError('n_components must be a positive integer, got %r' % (n_components,))
    if n_components > rows:
        raise ValueError('n_components = %d is larger than the %d rows of %s' % (n_components, rows, what))
    return int(n_components)


def _check_fun(fun):
    if fun not in FUNS:
        raise ValueError("fun must be 'cube', 'logcosh' or 'exp', got %r" % (fun,))
    return FUNS[fun]


# ---- PCA through the Gram matrix
def _gram_f64(rows):
    """rows rows^T in f64, the voxels in chunks"""
    G = torch.zeros((rows.shape[0], rows.shape[0]), dtype=torch.float64, device=rows.device)
    for a in range(0, rows.shape[1], GRAM_CHUNK):
        c = rows[:, a:a + GRAM_CHUNK].to(torch.float64)
        G.addmm_(c, c.T)
    return G


def _project_f64(Ut, rows):
    """Ut rows in f64, the voxels in chunks"""
    out = torch.empty((Ut.shape[0], rows.shape[1]), dtype=torch.float64, device=rows.device)
    for a in range(0, rows.shape[1], GRAM_CHUNK):
        torch.matmul(Ut, rows[:, a:a + GRAM_CHUNK].to(torch.float64), out=out[:, a:a + GRAM_CHUNK])
    return out


def _top_eigh(G, k):
    """the k leading eigenpairs of a symmetric matrix, descending, every eigenvector signed so that its largest-magnitude
    entry is positive: (eigenvalues (k,), eigenvectors as rows (k, n))"""
    s2, U = torch.linalg.eigh(G)
    s2, Ut = s2.flip(0)[:k], U.flip(1)[:, :k].T.contiguous()
    at = Ut.abs().argmax(dim=1, keepdim=True)
    Ut = Ut * torch.where(Ut.gather(1, at) < 0, -1.0, 1.0)
    return s2.clamp_min(0), Ut


def _top_eigh_host(G, k):
    s2, U = scipy.linalg.eigh(G)
    s2, Ut = s2[::-1][:k], np.ascontiguousarray(U[:, ::-1][:, :k].T)
    at = np.abs(Ut).argmax(axis=1)
    Ut = Ut * np.where(Ut[np.arange(k), at] < 0, -1.0, 1.0)[:, None]
    return np.maximum(s2, 0), Ut


def reduce_record(rows, n_components):
    """(T, V) cleaned rows -> (k, V) float64: S[:k, None] * Vt[:k] of the record's SVD (nilearn's per-subject reduction at
    reduction_ratio='auto'), from the eigenvectors U of the T x T Gram matrix as U[:, :k]^T rows, accumulated in f64 over
    chunks of voxels.  Every row is signed so that the largest-magnitude entry of its temporal vector is positive.
    ValueError: n_components > T."""
    cuda = is_cuda(rows)
    if not cuda and not have_gpu():
        return reduce_record_host(rows, n_components)
    rows = as_float_tensor(rows)
    _check_2d(rows, 'rows')
    k = _check_k(n_components, rows.shape[0], 'the record')
    with torch.cuda.device(rows.device):
        _, Ut = _top_eigh(_gram_f64(rows), k)
        return like_input(_project_f64(Ut, rows), cuda)


def reduce_record_host(rows, n_components):
    """`reduce_record` through numpy's SVD"""
    rows = np.asarray(rows, dtype=np.float64)
    _check_2d(rows, 'rows')
    k = _check_k(n_components, rows.shape[0], 'the record')
    U, S, Vt = np.linalg.svd(rows, full_matrices=False)
    at = np.abs(U[:, :k]).argmax(axis=0)
    sign = np.where(U[at, np.arange(k)] < 0, -1.0, 1.0)
    return (sign * S[:k])[:, None] * Vt[:k]


def _stack(reduced, host):
    if isinstance(reduced, (np.ndarray, torch.Tensor)):
        reduced = [reduced]
    if len(reduced) < 1:
        raise ValueError('group_components needs at least one reduced record')
    for r in reduced:
        _check_2d(r, 'a reduced record')
        if r.shape[1] != reduced[0].shape[1]:
            raise ValueError('the reduced records must have one number of voxels, got %d and %d' % (reduced[0].shape[1], r.shape[1]))
    if host:
        return np.concatenate([np.asarray(r, dtype=np.float64) for r in reduced])
    device = next((r.device for r in reduced if isinstance(r, torch.Tensor)), None)
    return torch.cat([as_float_tensor(r, device).to(torch.float64) for r in reduced])


def group_components(reduced, n_components):
    """A list of (k_i, V) reductions, stacked, every row scaled to unit norm (zero rows are left alone) -> (components (k, V)
    float64 with orthonormal rows: the top-k right singular vectors of the stack; variance (k,): their squared singular
    values).  Same Gram route as `reduce_record`.  The group spectrum is nearly degenerate by construction, so only the
    subspace is defined: any orthonormal basis of it is a correct answer."""
    listed = [reduced] if isinstance(reduced, (np.ndarray, torch.Tensor)) else list(reduced)
    cuda = any(is_cuda(r) for r in listed)
    if not cuda and not have_gpu():
        return group_components_host(listed, n_components)
    X = _stack(listed, False)
    k = _check_k(n_components, X.shape[0], 'the stacked reductions')
    with torch.cuda.device(X.device):
        norm = X.norm(dim=1, keepdim=True)
        X = X / torch.where(norm > 0, norm, torch.ones_like(norm))
        s2, Ut = _top_eigh(_gram_f64(X), k)
        if not bool((s2 > 0).all()):
            raise ValueError('the stacked reductions have rank below n_components = %d' % k)
        comp = _project_f64(Ut / s2.sqrt()[:, None], X)
        return like_input(comp, cuda), like_input(s2, cuda)


def group_components_host(reduced, n_components):
    """`group_components` through numpy / scipy: the same Gram route on the host"""
    X = _stack(reduced, True)
    k = _check_k(n_components, X.shape[0], 'the stacked reductions')
    norm = np.linalg.norm(X, axis=1, keepdims=True)
    X = X / np.where(norm > 0, norm, 1.0)
    s2, Ut = _top_eigh_host(X @ X.T, k)
    if not np.all(s2 > 0):
        raise ValueError('the stacked reductions have rank below n_components = %d' % k)
    return (Ut / np.sqrt(s2)[:, None]) @ X, s2


# ---- FastICA
def _check_ica_scalars(k, n_init, fun, tol, max_iter):
    _check_fun(fun)
    if k > lib.modl_ica_max_components():
        raise ValueError('fastica_maps takes at most %d components, got %d' % (lib.modl_ica_max_components(), k))
    if isinstance(max_iter, bool) or not isinstance(max_iter, (int, np.integer)) or max_iter < 1:
        raise ValueError('max_iter must be a positive integer, got %r' % (max_iter,))
    if isinstance(tol, (str, bool)) or not tol > 0:
        raise ValueError('tol must be positive, got %r' % (tol,))
    if isinstance(n_init, bool) or not isinstance(n_init, (int, np.integer)) or n_init < 1 or n_init > 65535:
        raise ValueError('n_init must be an integer in 1 .. 65535, got %r' % (n_init,))


def _check_ica_args(k, n_init, fun, tol, max_iter, w_init, random_state):
    """the checked arguments' w_init (n_init, k, k): the one given, or drawn from `random_state`"""
    _check_ica_scalars(k, n_init if w_init is None else 1, fun, tol, max_iter)
    if w_init is None:
        rs = check_random_state(random_state)
        seeds = rs.randint(np.iinfo(np.int32).max, size=n_init)            # as nilearn draws them
        return np.stack([check_random_state(int(s)).normal(size=(k, k)) for s in seeds])      # as sklearn draws w_init
    if isinstance(w_init, torch.Tensor):
        w_init = w_init.detach().cpu().numpy()
    w_init = np.array(w_init, dtype=np.float64)
    if w_init.ndim != 3 or w_init.shape[0] < 1 or w_init.shape[1:] != (k, k):
        raise ValueError('w_init must be (n_init, %d, %d), got shape %s' % (k, k, w_init.shape))
    return w_init


def _whiten_host(X):
    """centring over voxels and symmetric whitening: X1 = C^{-1/2} (X - mean), C = (X - mean)(X - mean)^T / V"""
    Xc = X - X.mean(axis=1, keepdims=True)
    s, u = scipy.linalg.eigh(Xc @ Xc.T / X.shape[1])
    if not s[0] > np.finfo(np.float64).eps * s[-1]:
        raise ValueError('the components are linearly dependent after centring: they cannot be whitened')
    return np.ascontiguousarray(((u / np.sqrt(s)) @ u.T) @ Xc)


def _whiten(X):
    Xc = X - X.mean(dim=1, keepdim=True)
    s, u = torch.linalg.eigh(_gram_f64(Xc) / X.shape[1])
    if not bool(s[0] > np.finfo(np.float64).eps * s[-1]):
        raise ValueError('the components are linearly dependent after centring: they cannot be whitened')
    return _project_f64((u / s.sqrt()) @ u.T, Xc)


def _sym_decorrelation(W):
    """sklearn's, batched: (W W^T)^{-1/2} W through eigh, the eigenvalues clipped at finfo.tiny"""
    s, u = torch.linalg.eigh(W @ W.transpose(1, 2))
    s = s.clamp_min(np.finfo(np.float64).tiny)
    return (u * (1.0 / s.sqrt())[:, None, :]) @ u.transpose(1, 2) @ W


def _sym_decorrelation_host(W):
    s, u = scipy.linalg.eigh(W @ W.T)
    s = np.clip(s, a_min=np.finfo(W.dtype).tiny, a_max=None)
    return np.linalg.multi_dot([u * (1.0 / np.sqrt(s)), u.T, W])


def _finite(W):
    return torch.isfinite(W).all(dim=2).all(dim=1)


def _safe(W, ok):
    """the matrices that are not `ok` replaced by the identity, so that a batched eigh sees finite input"""
    eye = torch.eye(W.shape[1], dtype=W.dtype, device=W.device).expand_as(W)
    return torch.where(ok[:, None, None], W, eye)


def ica_sweep(X1, W, active, fun='cube', alpha=1.0, M=None, gp=None, ws=None):
    """One launch of modl_ica_sweep_f64 on CUDA tensors: X1 (k, V) float64 with contiguous rows, W (n, k, k) float64
    contiguous, active (R,) int32 -> (M (n, k, k), gp (n, k)); only the slots of the listed restarts are written."""
    k, V = X1.shape
    R = int(active.shape[0])
    if M is None:
        M = torch.zeros_like(W)
    if gp is None:
        gp = torch.zeros(W.shape[:2], dtype=torch.float64, device=W.device)
    need = lib.modl_ica_sweep_workspace(V, k, R)
    if ws is None:
        ws = scratch(need, W.device)
    elif ws.numel() < need:
        raise ValueError('ica_sweep: the workspace holds %d bytes, %d restarts need %d' % (ws.numel(), R, need))
    call('modl_ica_sweep_f64', X1, X1.stride(0) if k > 1 else V, V, k, W, active, R, _check_fun(fun), float(alpha), M, gp, ws,
         ws.numel(), STREAM, device=X1.device)
    return M, gp


def _warn_not_converged(n):
    warnings.warn('fastica_maps: %d restart(s) did not converge in max_iter iterations; consider a larger max_iter or tol' % n,
                  ConvergenceWarning, stacklevel=3)


def _select(l1, failed):
    """the restart, among those that did not fail, with the smallest max_i sum_v |maps[i, v]| (nilearn's choice)"""
    if failed.all():
        raise ValueError('fastica_maps: every restart ended with a non-finite unmixing matrix')
    return int(np.argmin(np.where(failed, np.inf, l1)))


def fastica_maps(components, n_init=10, fun='cube', alpha=1.0, tol=1e-4, max_iter=200, w_init=None, random_state=None,
                 return_all=False):
    """Symmetric FastICA of (k, V) components with `n_init` restarts swept together (module docstring).

    Centring over voxels, symmetric whitening, then W = sym_decorrelation(w_init) and per iteration, for the restarts still
    running: one fused sweep (M, gp), W1 = sym_decorrelation(M - gp[:, None] * W), lim = max | |diag(W1 W^T)| - 1 |, W = W1,
    converged when lim < tol - sklearn's `_ica_par` for every restart.  `w_init` (n_init, k, k), or None: n_init seeds drawn
    from `random_state` as nilearn draws them, a standard normal k x k from each as sklearn draws it.  A restart whose W turns
    non-finite is marked `failed` and leaves the sweep (n_iter 0); all failed: ValueError.  A restart that reaches max_iter is
    kept, reported as not converged, and one ConvergenceWarning is raised.

    Returns IcaMaps(maps, W (n_init, k, k), n_iter, converged, failed (n_init,), selected): maps (k, V) = W[selected] X1, or
    with return_all=True the stack (n_init, k, V) (n_init k V 8 bytes; rows of failed restarts are NaN)."""
    cuda = is_cuda(components)
    if not cuda and not have_gpu():
        return fastica_maps_host(components, n_init, fun, alpha, tol, max_iter, w_init, random_state, return_all)
    X = as_float_tensor(components).to(torch.float64)
    _check_2d(X, 'components')
    k, V = X.shape
    w0 = _check_ica_args(k, n_init, fun, tol, max_iter, w_init, random_state)
    n = w0.shape[0]
    dev = X.device
    with torch.cuda.device(dev):
        X1 = _whiten(X)
        W = torch.from_numpy(w0).to(dev)
        ok = _finite(W)
        W = _sym_decorrelation(_safe(W, ok))
        ok &= _finite(W)
        running = ok.clone()
        n_iter = np.zeros(n, dtype=np.int64)
        converged = np.zeros(n, dtype=bool)
        M, gp = torch.zeros_like(W), torch.zeros((n, k), dtype=torch.float64, device=dev)
        ws = scratch(lib.modl_ica_sweep_workspace(V, k, n), dev)
        run = running.cpu().numpy()
        for it in range(1, max_iter + 1):
            if not run.any():
                break
            active = torch.from_numpy(np.flatnonzero(run).astype(np.int32)).to(dev)
            ica_sweep(X1, W, active, fun, alpha, M, gp, ws)
            # the decorrelation always runs on the whole batch (idle restarts as the identity), one shape for every call, and
            # the sweep's voxel chunking depends on V alone: a restart's bits do not depend on which others are still running
            new = _safe(M - gp[:, :, None] * W, running)
            fin = _finite(new)
            W1 = _sym_decorrelation(_safe(new, fin))
            fin &= _finite(W1)
            lim = ((W1 * W).sum(dim=2).abs() - 1).abs().amax(dim=1)
            state = torch.stack([fin.to(torch.float64), lim]).cpu().numpy()          # the one transfer of an iteration
            good = run & (state[0] > 0)
            bad = run & ~good
            W = torch.where(torch.from_numpy(good).to(dev)[:, None, None], W1, W)
            n_iter[good] = it
            done = good & (state[1] < tol)
            converged |= done
            run = good & ~done
            if bad.any():
                ok &= torch.from_numpy(~bad).to(dev)
            running = torch.from_numpy(run).to(dev)
        failed = ~ok.cpu().numpy()
        n_iter[failed] = 0
        W = torch.where(ok[:, None, None], W, torch.full_like(W, float('nan')))
        l1 = np.full(n, np.inf)
        stack = torch.full((n, k, V), float('nan'), dtype=torch.float64, device=dev) if return_all else None
        for r in np.flatnonzero(~failed):
            maps = _project_f64(W[r], X1)
            l1[r] = float(maps.abs().sum(dim=1).max())
            if return_all:
                stack[r] = maps
        selected = _select(l1, failed)
        maps = stack if return_all else _project_f64(W[selected], X1)
    if (~converged & ~failed).any():
        _warn_not_converged(int((~converged & ~failed).sum()))
    if cuda:
        return IcaMaps(maps, W, torch.from_numpy(n_iter).to(dev), torch.from_numpy(converged).to(dev),
                       torch.from_numpy(failed).to(dev), selected)
    return IcaMaps(maps.cpu().numpy(), W.cpu().numpy(), n_iter, converged, failed, selected)


def fastica_maps_host(components, n_init=10, fun='cube', alpha=1.0, tol=1e-4, max_iter=200, w_init=None, random_state=None,
                      return_all=False):
    """`fastica_maps` through numpy / scipy and sklearn.decomposition.fastica(whiten=False) on the symmetrically whitened
    rows, one restart at a time; a restart on which sklearn raises (a non-finite W) is `failed`"""
    from sklearn.decomposition import fastica
    X = np.asarray(components, dtype=np.float64)
    _check_2d(X, 'components')
    k, V = X.shape
    w0 = _check_ica_args(k, n_init, fun, tol, max_iter, w_init, random_state)
    n = w0.shape[0]
    X1 = _whiten_host(X)
    X1t = np.ascontiguousarray(X1.T)
    W = np.full((n, k, k), np.nan)
    n_iter, converged, failed = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    l1 = np.full(n, np.inf)
    stack = np.full((n, k, V), np.nan) if return_all else None
    for r in range(n):
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter('always')
            try:
                with np.errstate(all='ignore'):
                    _, Wr, _, it = fastica(X1t, whiten=False, algorithm='parallel', fun=fun,
                                           fun_args={'alpha': alpha} if fun == 'logcosh' else None, tol=tol, max_iter=int(max_iter),
                                           w_init=np.ascontiguousarray(w0[r]), compute_sources=False, return_n_iter=True)
            except ValueError as e:                                      # scipy's eigh on a non-finite W W^T
                if 'infs or NaNs' not in str(e):
                    raise
                failed[r] = True
        for c in caught:                                                 # sklearn's other warnings pass through
            if not issubclass(c.category, ConvergenceWarning):
                warnings.warn_explicit(c.message, c.category, c.filename, c.lineno)
        if failed[r]:
            continue
        if not np.all(np.isfinite(Wr)):
            failed[r] = True
            continue
        W[r], n_iter[r] = Wr, it
        converged[r] = not any(issubclass(c.category, ConvergenceWarning) for c in caught)
        maps = Wr @ X1
        l1[r] = np.abs(maps).sum(axis=1).max()
        if return_all:
            stack[r] = maps
    selected = _select(l1, failed)
    if (~converged & ~failed).any():
        _warn_not_converged(int((~converged & ~failed).sum()))
    return IcaMaps(stack if return_all else W[selected] @ X1, W, n_iter, converged, failed, selected)


def _nonlinearity_host(Y, fun, alpha):
    if fun == 'cube':
        return Y ** 3, (3 * Y ** 2).mean(axis=-1)
    if fun == 'logcosh':
        g = np.tanh(alpha * Y)
        return g, (alpha * (1 - g ** 2)).mean(axis=-1)
    e = np.exp(-(Y ** 2) / 2)
    return Y * e, ((1 - Y ** 2) * e).mean(axis=-1)


def fastica_lims_host(components, w_init, fun='cube', alpha=1.0, n_iter=None, max_iter=200):
    """The sequence lim_1, lim_2, .. of every restart of `fastica_maps_host` on the same arguments, replayed with numpy
    (sklearn does not report it): a list of 1-D arrays, n_iter[r] (or max_iter) values each; empty for a failed restart.
    The tests assert on it that no lim comes near `tol`, so that an iteration count cannot flip on rounding."""
    _check_fun(fun)
    X1 = _whiten_host(np.asarray(components, dtype=np.float64))
    out = []
    for r, w in enumerate(np.asarray(w_init, dtype=np.float64)):
        lims = []
        steps = max_iter if n_iter is None else int(n_iter[r])
        try:
            with np.errstate(all='ignore'):
                W = _sym_decorrelation_host(w) if steps else None
                for _ in range(steps):
                    g, gp = _nonlinearity_host(W @ X1, fun, alpha)
                    W1 = _sym_decorrelation_host(g @ X1.T / X1.shape[1] - gp[:, None] * W)
                    lims.append(max(abs(abs(np.einsum('ij,ij->i', W1, W)) - 1)))
                    W = W1
        except ValueError:
            lims = []
        out.append(np.array(lims))
    return out


# ---- threshold and sign
def _check_ratio(threshold, k):
    if threshold is None:
        return None
    if isinstance(threshold, str):
        if threshold != 'auto':
            raise ValueError("threshold must be 'auto', a number or None, got %r" % (threshold,))
        return 1.0
    try:
        ratio = float(threshold)
    except (TypeError, ValueError):
        raise ValueError("threshold must be 'auto', a number or None, got %r" % (threshold,))
    if not 0 < ratio <= k:
        raise ValueError('threshold must lie in (0, %d] (the number of maps), got %r' % (k, threshold))
    return ratio


def _percentile_weights(n, k, ratio):
    """scipy.stats.scoreatpercentile's position in the sorted values: (i, None, None) when it falls on one, else
    (i, weight of value i, weight of value i + 1)"""
    per = 100.0 - 100.0 / k * ratio
    idx = per / 100.0 * (n - 1)
    i = int(idx)
    if i == idx:
        return i, None, None
    return i, (i + 1) - idx, idx - i


def threshold_maps(maps, threshold='auto'):
    """(k, V) maps -> float64 maps with every entry whose magnitude is below the cutoff set to 0, then every map with
    max < -min negated.  The cutoff is scipy.stats.scoreatpercentile(|maps|, 100 - 100 / k * ratio) over all k V values,
    interpolated as scipy does; ratio = 1 for 'auto', otherwise the number given (0 < ratio <= k).  On the device the two
    order statistics come from torch.kthvalue and the interpolation is scipy's arithmetic on those two numbers, so the
    result equals the twin's bit for bit.  threshold=None only applies the sign rule."""
    cuda = is_cuda(maps)
    if not cuda and not have_gpu():
        return threshold_maps_host(maps, threshold)
    m = as_float_tensor(maps).to(torch.float64)
    _check_2d(m, 'maps')
    ratio = _check_ratio(threshold, m.shape[0])
    with torch.cuda.device(m.device):
        if ratio is not None:
            a = m.abs().reshape(-1)
            i, wa, wb = _percentile_weights(a.numel(), m.shape[0], ratio)
            lo = float(torch.kthvalue(a, i + 1).values.item())
            if wa is None:
                cutoff = lo
            else:
                hi = float(torch.kthvalue(a, i + 2).values.item())
                weights = np.array([wa, wb], float)
                cutoff = np.add.reduce(np.array([lo, hi]) * weights) / weights.sum()
            m = torch.where(m.abs() < float(cutoff), torch.zeros((), dtype=m.dtype, device=m.device), m)
        flip = m.amax(dim=1) < -m.amin(dim=1)
        m = torch.where(flip[:, None], -m, m)
    return like_input(m, cuda)


def threshold_maps_host(maps, threshold='auto'):
    """`threshold_maps` through numpy and scipy.stats.scoreatpercentile"""
    m = np.array(maps, dtype=np.float64)
    _check_2d(m, 'maps')
    ratio = _check_ratio(threshold, m.shape[0])
    if ratio is not None:
        cutoff = scipy.stats.scoreatpercentile(np.abs(m), 100.0 - 100.0 / m.shape[0] * ratio)
        m[np.abs(m) < cutoff] = 0
    flip = m.max(axis=1) < -m.min(axis=1)
    m[flip] = -m[flip]
    return m


# ---- the pipeline
def _check_records(records, n_components, what='canica', same_width=False):
    if isinstance(records, (np.ndarray, torch.Tensor)) and records.ndim == 2:
        records = [records]
    records = list(records)
    if not records:
        raise ValueError('%s needs at least one record' % what)
    for r in records:
        _check_2d(r, 'a record')
        _check_k(n_components, r.shape[0], 'the shortest record')
        if same_width and r.shape[1] != records[0].shape[1]:
            raise ValueError('the records must have one number of voxels, got %d and %d' % (records[0].shape[1], r.shape[1]))
    return records


def canica(records, n_components=20, n_init=10, threshold='auto', fun='cube', tol=1e-4, max_iter=200, random_state=None):
    """CanICA of a list of cleaned (T_i, V) records: reduce_record on each, group_components, fastica_maps, threshold_maps.
    Returns Canica(maps (k, V) float64, variance (k,), ica: the IcaMaps record).  The stacked reductions take
    n_records * k * V * 8 bytes.  ValueError: n_components larger than the shortest record."""
    records = _check_records(records, n_components)
    cuda = any(is_cuda(r) for r in records)
    if not cuda and not have_gpu():
        return canica_host(records, n_components, n_init, threshold, fun, tol, max_iter, random_state)
    _check_ratio(threshold, n_components)
    device = next((r.device for r in records if isinstance(r, torch.Tensor)), None)
    reduced = [reduce_record(as_float_tensor(r, device), n_components) for r in records]
    comp, variance = group_components(reduced, n_components)
    del reduced
    ica = fastica_maps(comp, n_init, fun, 1.0, tol, max_iter, None, random_state)
    maps = threshold_maps(ica.maps, threshold)
    if cuda:
        return Canica(maps, variance, ica)
    return Canica(maps.cpu().numpy(), variance.cpu().numpy(),
                  IcaMaps(ica.maps.cpu().numpy(), ica.W.cpu().numpy(), ica.n_iter.cpu().numpy(), ica.converged.cpu().numpy(),
                          ica.failed.cpu().numpy(), ica.selected))


def canica_host(records, n_components=20, n_init=10, threshold='auto', fun='cube', tol=1e-4, max_iter=200, random_state=None):
    """`canica` through the host twins"""
    records = _check_records(records, n_components)
    _check_ratio(threshold, n_components)
    comp, variance = group_components_host([reduce_record_host(r, n_components) for r in records], n_components)
    ica = fastica_maps_host(comp, n_init, fun, 1.0, tol, max_iter, None, random_state)
    return Canica(threshold_maps_host(ica.maps, threshold), variance, ica)
