"""Functional connectivity on the device (csrc/connectivity.hip): what follows the region signals of
`fMRICoder.transform` in the fMRI chain.

    covariances            the covariance matrix of every record of a list of (T_i, R) signals, empirical or Ledoit-Wolf
                           (sklearn.covariance.LedoitWolf's arithmetic), all records in ONE call of modl_conn_covariance_*;
    ConnectivityMeasure    nilearn's estimator of that name: kinds 'covariance', 'correlation', 'precision',
                           'partial correlation' and 'tangent' (the geometric mean of the fitted covariances, the records
                           whitened by its inverse square root, the matrix logarithm), optionally vectorized;
    geometric_mean         nilearn's fixed-point iteration for the geometric mean of symmetric positive definite matrices;
    sym_matrix_to_vec / vec_to_sym_matrix     the lower triangle, row-major, the diagonal divided by sqrt(2);
    seed_correlation       the Pearson correlation over time of every seed signal with every voxel of a cleaned record
                           (modl_conn_seed_maps_*: one fused pass over the record, nothing centred or normalised in memory).

The two products are the hand-written kernels.  The small dense algebra on R x R matrices (inverse, eigendecompositions for
square roots, logarithms and exponentials) is batched torch.linalg on the device: library plumbing, as in canica.py.  Every
function takes numpy arrays or CUDA tensors and answers in kind (CUDA results are never downloaded); a numpy input without a
GPU goes through the `*_host` twin.  The twins are numpy / scipy: what runs without a GPU, and the judge of the tests.

Departures from nilearn (not installed where this was written: its behaviour is described from its documented algorithm): newer
nilearn versions standardize the signals inside ConnectivityMeasure first - here the caller's cleaning decides
(`fMRICoder(standardize=True)`); there is no `inverse_transform`; Ledoit-Wolf shrinkage is computed in one block, which is
what sklearn's blocked loop sums to."""
import warnings

import numpy as np
import scipy.linalg
import torch
from sklearn.base import BaseEstimator
from sklearn.exceptions import ConvergenceWarning

from ._lib import lib
from .device import STREAM, as_float_tensor, call, current_device, have_gpu, is_cuda, scratch

__all__ = ['covariances', 'covariances_host', 'ConnectivityMeasure', 'ConnectivityMeasureHost', 'geometric_mean',
           'geometric_mean_host', 'sym_matrix_to_vec', 'vec_to_sym_matrix', 'seed_correlation', 'seed_correlation_host',
           'prepare_seeds_host', 'KINDS', 'ESTIMATORS']

ESTIMATORS = {'empirical': 0, 'ledoit_wolf': 1}
KINDS = ('covariance', 'correlation', 'precision', 'partial correlation', 'tangent')
U64 = 2.0 ** -53


# ---- arguments
def _check_estimator(estimator):
    if estimator not in ESTIMATORS:
        raise ValueError("estimator must be 'empirical' or 'ledoit_wolf', got %r" % (estimator,))
    return ESTIMATORS[estimator]


def _check_signals(signals):
    """the list of records, each 2-D (T_i >= 2, R), one R for all"""
    if isinstance(signals, (np.ndarray, torch.Tensor)):
        signals = [signals] if signals.ndim == 2 else list(signals)
    signals = list(signals)
    if not signals:
        raise ValueError('at least one record of signals is needed')
    for s in signals:
        if s.ndim != 2 or s.shape[1] < 1:
            raise ValueError('a record of signals must be (time points, regions), got shape %s' % (tuple(s.shape),))
        if s.shape[0] < 2:
            raise ValueError('a record needs at least 2 time points, got %d' % s.shape[0])
        if s.shape[1] != signals[0].shape[1]:
            raise ValueError('all records must have one number of regions, got %d and %d' % (signals[0].shape[1], s.shape[1]))
    return signals


def _device_of(arrays):
    for a in arrays:
        if isinstance(a, torch.Tensor):
            return a.device
    return current_device()


# ---- covariance
def _covariances_device(signals, estimator, correlation):
    """(cov (S, R, R), shrinkage (S,)) float64 CUDA tensors of checked signals: one library call"""
    est = _check_estimator(estimator)
    R = int(signals[0].shape[1])
    if R > lib.modl_conn_max_regions():
        raise ValueError('covariances takes at most %d regions, got %d' % (lib.modl_conn_max_regions(), R))
    if len(signals) > 65535:
        raise ValueError('covariances takes at most 65535 records in a call, got %d' % len(signals))
    device = _device_of(signals)
    parts = [as_float_tensor(s, device) for s in signals]
    dtype = torch.float32 if all(p.dtype == torch.float32 for p in parts) else torch.float64
    with torch.cuda.device(device):
        X = parts[0].to(dtype).contiguous() if len(parts) == 1 else torch.cat([p.to(dtype) for p in parts])
        S = len(parts)
        offsets = np.zeros(S + 1, dtype=np.int64)
        np.cumsum([p.shape[0] for p in parts], out=offsets[1:])
        cov = torch.empty((S, R, R), dtype=torch.float64, device=device)
        shrinkage = torch.empty(S, dtype=torch.float64, device=device)
        ws = scratch(lib.modl_conn_covariance_workspace(S, R), device)
        call('modl_conn_covariance', X, X.stride(0), offsets, S, R, est, 1 if correlation else 0, cov, shrinkage, ws, ws.numel(),
             STREAM, device=device, dtype=X)
    return cov, shrinkage


def covariances(signals, estimator='ledoit_wolf'):
    """A list of S records (T_i, R), float32 or float64, T_i >= 2 -> (cov (S, R, R) float64, shrinkage (S,) float64).

    Per record, in f64, with Xc = X - column means, E = Xc^T Xc / T: 'empirical' gives E (shrinkage 0); 'ledoit_wolf' gives
    (1 - shrinkage) E + shrinkage mu I with mu = trace(E) / R and sklearn.covariance.LedoitWolf's shrinkage (0 for R = 1).  All records go
    through one call of the library (csrc/connectivity.hip); CUDA tensors in give CUDA tensors out."""
    signals = _check_signals(signals)
    cuda = any(is_cuda(s) for s in signals)
    if not cuda and not have_gpu():
        return covariances_host(signals, estimator)
    cov, shrinkage = _covariances_device(signals, estimator, False)
    return (cov, shrinkage) if cuda else (cov.cpu().numpy(), shrinkage.cpu().numpy())


def covariances_host(signals, estimator='ledoit_wolf'):
    """`covariances` through numpy: the definitions of the module, restated"""
    signals = _check_signals(signals)
    est = _check_estimator(estimator)
    R = signals[0].shape[1]
    cov, shrinkage = np.empty((len(signals), R, R)), np.zeros(len(signals))
    for s, X in enumerate(signals):
        X = np.asarray(X, dtype=np.float64)
        T = X.shape[0]
        Xc = X - X.mean(axis=0)
        G = Xc.T @ Xc
        E = G / T
        if est == 1 and R > 1:                              # (one region: shrinkage 0, as sklearn answers)
            mu = np.trace(E) / R
            delta_ = np.sum(G ** 2) / T ** 2
            beta_ = np.sum(np.sum(Xc ** 2, axis=1) ** 2)
            beta = (beta_ / T - delta_) / (R * T)
            delta = (delta_ - 2.0 * mu * np.trace(E) + R * mu ** 2) / R
            beta = min(beta, delta)
            shrinkage[s] = 0.0 if beta == 0 else beta / delta
            E = (1.0 - shrinkage[s]) * E
            E[np.arange(R), np.arange(R)] += shrinkage[s] * mu
        cov[s] = (E + E.T) / 2
    return cov, shrinkage


# ---- small dense algebra, numpy or torch
def _T(m):
    return m.transpose(-1, -2) if isinstance(m, torch.Tensor) else np.swapaxes(m, -1, -2)


def _eigh(m):
    if isinstance(m, torch.Tensor):
        return torch.linalg.eigh(m)
    if m.ndim == 2:
        return scipy.linalg.eigh(m)
    pairs = [scipy.linalg.eigh(a) for a in m]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def _map_eigenvalues(fun, m):
    """fun on the eigenvalues of symmetric matrices (..., R, R): V fun(lambda) V^T, symmetric by construction"""
    vals, vecs = _eigh(m)
    out = (vecs * fun(vals)[..., None, :]) @ _T(vecs)
    return (out + _T(out)) / 2


def _sqrt(x):
    return x.sqrt() if isinstance(x, torch.Tensor) else np.sqrt(x)


def _log(x):
    return x.log() if isinstance(x, torch.Tensor) else np.log(x)


def _exp(x):
    return x.exp() if isinstance(x, torch.Tensor) else np.exp(x)


def _sym(m):
    return (m + _T(m)) / 2


def _correlation_of(cov):
    """cov_ij / sqrt(cov_ii cov_jj), the diagonal exactly 1"""
    d = cov.diagonal(dim1=-2, dim2=-1) if isinstance(cov, torch.Tensor) else np.diagonal(cov, axis1=-2, axis2=-1)
    out = cov / _sqrt(d[..., :, None] * d[..., None, :])
    n = cov.shape[-1]
    out[..., range(n), range(n)] = 1.0
    return out


def _precision_of(cov):
    if isinstance(cov, torch.Tensor):
        return _sym(torch.linalg.inv(cov))
    return _sym(np.stack([scipy.linalg.inv(c) for c in cov]))


def _geometric_mean(covs, max_iter, tol):
    """nilearn's iteration on (S, R, R) numpy arrays or tensors: (G, the norm / R^2 checked at every iteration)"""
    if isinstance(max_iter, bool) or not isinstance(max_iter, (int, np.integer)) or max_iter < 1:
        raise ValueError('max_iter must be a positive integer, got %r' % (max_iter,))
    if isinstance(tol, (str, bool)) or not tol > 0:
        raise ValueError('tol must be positive, got %r' % (tol,))
    if covs.ndim != 3 or covs.shape[0] < 1 or covs.shape[1] != covs.shape[2]:
        raise ValueError('geometric_mean expects (S, R, R) matrices, got shape %s' % (tuple(covs.shape),))
    size = covs.shape[1] * covs.shape[2]
    G = _sym(covs.mean(0) if isinstance(covs, torch.Tensor) else covs.mean(axis=0))
    step, norm_old, norms = 1.0, np.inf, []
    for _ in range(max_iter):
        vals, vecs = _eigh(G)
        if not float(vals.min()) > 0:
            raise ValueError('geometric_mean: the matrices must be symmetric positive definite')
        inv_sqrt = (vecs / _sqrt(vals)[None, :]) @ _T(vecs)
        root = (vecs * _sqrt(vals)[None, :]) @ _T(vecs)
        logs = _map_eigenvalues(_log, _sym(inv_sqrt @ covs @ inv_sqrt))
        L = logs.mean(0) if isinstance(logs, torch.Tensor) else logs.mean(axis=0)
        norm = float((L * L).sum()) ** 0.5                  # the one transfer of an iteration
        if not np.isfinite(norm):
            raise FloatingPointError('geometric_mean: non-finite logarithm (a matrix that is not positive definite?)')
        G = _sym(root @ _map_eigenvalues(lambda v: _exp(step * v), L) @ root)
        if norm < norm_old:
            norm_old = norm
        elif norm > norm_old:
            step /= 2.0
            norm = norm_old
        norms.append(norm / size)
        if norm / size < tol:
            break
    else:
        warnings.warn('geometric_mean: maximum number of iterations %d reached without getting to the requested tolerance '
                      '%g (last norm / R^2 = %g)' % (max_iter, tol, norms[-1]), ConvergenceWarning, stacklevel=3)
    return G, np.array(norms)


def _stack_matrices(covs, host):
    if isinstance(covs, (list, tuple)):
        if host or not any(isinstance(c, torch.Tensor) for c in covs):
            return np.stack([np.asarray(c.cpu() if isinstance(c, torch.Tensor) else c, dtype=np.float64) for c in covs])
        device = _device_of(covs)
        return torch.stack([as_float_tensor(c, device, torch.float64) for c in covs])
    if isinstance(covs, torch.Tensor):
        return covs.cpu().numpy().astype(np.float64) if host else covs.to(torch.float64)
    return np.asarray(covs, dtype=np.float64)


def geometric_mean(covs, max_iter=10, tol=1e-7, return_norms=False):
    """The geometric mean of S symmetric positive definite matrices (S, R, R), by nilearn's iteration: G starts at the
    arithmetic mean, step = 1; per iteration W_i = G^{-1/2} C_i G^{-1/2}, L = mean_i logm(W_i), G = G^{1/2} expm(step L) G^{1/2}
    (every matrix function through eigh, batched over the records on the device); the step is halved when ||L||_F grows; it
    stops when ||L||_F / R^2 < tol.  Not stopping within max_iter: one ConvergenceWarning, G is kept.  A non-finite L:
    FloatingPointError.  return_norms=True: (G, the norm / R^2 compared with tol at every iteration)."""
    cuda = any(is_cuda(c) for c in covs) if isinstance(covs, (list, tuple)) else is_cuda(covs)
    if not cuda and not have_gpu():
        return geometric_mean_host(covs, max_iter, tol, return_norms)
    C = _stack_matrices(covs, False)
    if not isinstance(C, torch.Tensor):
        C = torch.from_numpy(C).to(_device_of([]))
    with torch.cuda.device(C.device):
        G, norms = _geometric_mean(C, max_iter, tol)
    G = G if cuda else G.cpu().numpy()
    return (G, norms) if return_norms else G


def geometric_mean_host(covs, max_iter=10, tol=1e-7, return_norms=False):
    """`geometric_mean` through scipy.linalg.eigh"""
    G, norms = _geometric_mean(_stack_matrices(covs, True), max_iter, tol)
    return (G, norms) if return_norms else G


# ---- vectorization
def _tril(n, k, like):
    """row and column indices of the lower triangle, as `like` wants its indices"""
    i, j = np.tril_indices(n, k)
    if isinstance(like, torch.Tensor):
        return torch.from_numpy(i).to(like.device), torch.from_numpy(j).to(like.device), np.flatnonzero(i == j)
    return i, j, np.flatnonzero(i == j)


def sym_matrix_to_vec(m, discard_diagonal=False):
    """Symmetric matrices (..., R, R) -> (..., R (R + 1) / 2): the lower triangle in row-major order (0,0), (1,0), (1,1),
    (2,0) .., the diagonal elements divided by sqrt(2) (so that the vector's 2-norm is the matrix's Frobenius norm over
    sqrt(2)); discard_diagonal=True: the strict lower triangle (..., R (R - 1) / 2), unscaled."""
    if m.ndim < 2 or m.shape[-1] != m.shape[-2]:
        raise ValueError('sym_matrix_to_vec expects square matrices (..., R, R), got shape %s' % (tuple(m.shape),))
    n = m.shape[-1]
    i, j, d = _tril(n, -1 if discard_diagonal else 0, m)
    v = m[..., i, j]
    if not discard_diagonal:
        if isinstance(v, torch.Tensor):                    # (a device tensor as divisor: by a host scalar torch multiplies by the
            v = v.clone()                                   # reciprocal, which is not the division of the definition bit for bit)
            v[..., d] = v[..., d] / torch.tensor(np.sqrt(2.0), dtype=v.dtype, device=v.device)
        else:
            v = v.copy()
            v[..., d] = v[..., d] / np.sqrt(2.0)
    return v


def vec_to_sym_matrix(v, diagonal=None):
    """The inverse of `sym_matrix_to_vec`: (..., R (R + 1) / 2) -> (..., R, R), the diagonal multiplied by sqrt(2); with
    `diagonal` (..., R) the vector is the strict lower triangle (..., R (R - 1) / 2) and `diagonal` is placed as it is."""
    k = v.shape[-1]
    if diagonal is None:
        n = int((np.sqrt(8 * k + 1) - 1) / 2)
        if n * (n + 1) // 2 != k:
            raise ValueError('a vector of %d values is not the lower triangle of a square matrix' % k)
        i, j, d = _tril(n, 0, v)
    else:
        n = int(diagonal.shape[-1])
        if n * (n - 1) // 2 != k or tuple(diagonal.shape[:-1]) != tuple(v.shape[:-1]):
            raise ValueError('a diagonal of shape %s does not go with a vector of shape %s' % (tuple(diagonal.shape), tuple(v.shape)))
        i, j, d = _tril(n, -1, v)
    shape = tuple(v.shape[:-1]) + (n, n)
    m = v.new_zeros(shape) if isinstance(v, torch.Tensor) else np.zeros(shape, dtype=v.dtype)
    m[..., i, j] = v
    m[..., j, i] = v
    if diagonal is None:
        m[..., range(n), range(n)] = v[..., d] * np.sqrt(2.0)
    else:
        m[..., range(n), range(n)] = diagonal
    return m


# ---- the estimator
class ConnectivityMeasure(BaseEstimator):
    """nilearn's ConnectivityMeasure on lists of region signals (T_i, R): `fit`, `transform`, `fit_transform` give one matrix
    per record, (S, R, R), or with vectorize=True its lower triangle (`sym_matrix_to_vec`), without the diagonal when
    discard_diagonal=True.

    kind: 'covariance' (the `estimator` of `covariances`: 'ledoit_wolf' or 'empirical'), 'correlation' (cov_ij /
    sqrt(cov_ii cov_jj), diagonal exactly 1), 'precision' (the inverse), 'partial correlation' (-P_ij / sqrt(P_ii P_jj),
    diagonal exactly 1), 'tangent' (logm(whitening_ cov_i whitening_) with whitening_ = mean_^{-1/2} and mean_ the geometric mean
    of the FITTED covariances; `transform` of new records uses the fitted whitening_).  `mean_`: for tangent the geometric mean,
    otherwise the arithmetic mean of the fitted matrices of that kind.  numpy records give numpy results, CUDA tensors CUDA
    results.  The signals are taken as they are: standardize them upstream if the kind asks for it."""

    _host = False

    def __init__(self, kind='covariance', estimator='ledoit_wolf', vectorize=False, discard_diagonal=False):
        self.kind = kind
        self.estimator = estimator
        self.vectorize = vectorize
        self.discard_diagonal = discard_diagonal

    def _matrices(self, signals, fit):
        if self.kind not in KINDS:
            raise ValueError('kind must be one of %s, got %r' % (', '.join(repr(k) for k in KINDS), self.kind))
        _check_estimator(self.estimator)
        signals = _check_signals(signals)
        cuda = any(is_cuda(s) for s in signals)
        host = self._host or (not cuda and not have_gpu())
        if not fit:
            if not hasattr(self, 'mean_'):
                raise ValueError('ConnectivityMeasure is not fitted: call fit() first')
            if signals[0].shape[1] != self.mean_.shape[0]:
                raise ValueError('the records have %d regions, the fitted ones had %d' % (signals[0].shape[1], self.mean_.shape[0]))
        if host:
            signals = [s.cpu().numpy() if isinstance(s, torch.Tensor) else s for s in signals]
            cov = covariances_host(signals, self.estimator)[0]
            if self.kind == 'correlation':
                cov = _correlation_of(cov)
        else:
            cov = _covariances_device(signals, self.estimator, self.kind == 'correlation')[0]
        dev = cov.device if isinstance(cov, torch.Tensor) else None
        ctx = torch.cuda.device(dev) if dev is not None else _NoContext()
        with ctx:
            if self.kind in ('covariance', 'correlation'):
                out = cov
            elif self.kind == 'precision':
                out = _precision_of(cov)
            elif self.kind == 'partial correlation':
                out = -_correlation_of(_precision_of(cov))
                n = out.shape[-1]
                out[..., range(n), range(n)] = 1.0
            else:
                if fit:
                    mean = _geometric_mean(cov, 10, 1e-7)[0]
                    whitening = _map_eigenvalues(lambda v: 1.0 / _sqrt(v), mean)
                else:
                    mean, whitening = self._fitted_on(dev)
                out = _map_eigenvalues(_log, _sym(whitening @ cov @ whitening))
            if fit:
                if self.kind != 'tangent':
                    mean = out.mean(0) if dev is not None else out.mean(axis=0)
                    whitening = None
                back = (lambda t: t) if (cuda or dev is None) else (lambda t: t.cpu().numpy())
                self.mean_ = back(mean)
                if whitening is not None:
                    self.whitening_ = back(whitening)
                elif hasattr(self, 'whitening_'):
                    del self.whitening_
            if self.vectorize:
                out = sym_matrix_to_vec(out, self.discard_diagonal)
        return out if (cuda or dev is None) else out.cpu().numpy()

    def _fitted_on(self, dev):
        """mean_ and whitening_ where the records' matrices are"""
        pair = []
        for m in (self.mean_, self.whitening_):
            if dev is None:
                pair.append(m.cpu().numpy() if isinstance(m, torch.Tensor) else m)
            else:
                pair.append(as_float_tensor(m, dev, torch.float64))
        return pair

    def fit(self, signals, y=None):
        self._matrices(signals, True)
        return self

    def fit_transform(self, signals, y=None):
        return self._matrices(signals, True)

    def transform(self, signals):
        return self._matrices(signals, False)


class ConnectivityMeasureHost(ConnectivityMeasure):
    """`ConnectivityMeasure` through the host twins (numpy / scipy), whatever the machine has"""
    _host = True


class _NoContext:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


# ---- seed maps
def _check_seed_args(rows, seeds):
    if rows.ndim != 2 or rows.shape[1] < 1:
        raise ValueError('rows must be (time points, voxels), got shape %s' % (tuple(rows.shape),))
    if seeds.ndim == 1:
        seeds = seeds[:, None]
    if seeds.ndim != 2 or seeds.shape[1] < 1:
        raise ValueError('seeds must be (time points, seeds), got shape %s' % (tuple(seeds.shape),))
    if rows.shape[0] < 2:
        raise ValueError('a record needs at least 2 time points, got %d' % rows.shape[0])
    if seeds.shape[0] != rows.shape[0]:
        raise ValueError('seeds have %d time points, the record has %d' % (seeds.shape[0], rows.shape[0]))
    return seeds


def _constant_seed(r):
    raise ValueError('seed %d is constant over time: its correlation is not defined' % r)


def prepare_seeds_host(seeds):
    """(T, R) seeds -> float64 (T, R): every column centred and scaled to unit 2-norm.  ValueError: a constant column (its
    centred norm is at most T eps times its magnitude)."""
    s = np.asarray(seeds, dtype=np.float64)
    c = s - s.mean(axis=0)
    norm = np.sqrt((c * c).sum(axis=0))
    bad = np.flatnonzero(~(norm > s.shape[0] * np.finfo(np.float64).eps * np.abs(s).max(axis=0)))
    if bad.size:
        _constant_seed(int(bad[0]))
    return c / norm


def _prepare_seeds(seeds):
    s = seeds.to(torch.float64)
    c = s - s.mean(dim=0)
    norm = (c * c).sum(dim=0).sqrt()
    bad = torch.nonzero(~(norm > s.shape[0] * np.finfo(np.float64).eps * s.abs().amax(dim=0))).flatten()
    if bad.numel():
        _constant_seed(int(bad[0]))
    return c / norm


def seed_correlation(rows, seeds):
    """The seed-to-voxel correlation maps of one cleaned record: rows (T, V), float32 or float64, seeds (T, R) ->
    out (R, V) in the dtype of rows, out[r, v] the Pearson correlation over time of seed r and voxel v.

    The seeds are centred and scaled to unit norm in f64 and cast to the dtype of rows (plumbing); the kernel
    (modl_conn_seed_maps_*) then makes one pass over the record: the product on the matrix cores, sum x and sum x^2 per voxel
    in f64 on the way, the division by sqrt(sum x^2 - (sum x)^2 / T) in the epilogue - no centred or normalised copy of the
    record exists.  A voxel that is constant to rounding gives an exact 0, results are clipped to [-1, 1].
    ValueError: a constant seed, T < 2, more than modl_conn_max_regions() seeds."""
    cuda = is_cuda(rows)
    if not cuda and not have_gpu():
        return seed_correlation_host(rows, seeds)
    device = rows.device if cuda else _device_of([seeds])
    X = as_float_tensor(rows, device)
    s = _check_seed_args(X, as_float_tensor(seeds, device))
    R, (T, V) = int(s.shape[1]), X.shape
    if R > lib.modl_conn_max_regions():
        raise ValueError('seed_correlation takes at most %d seeds, got %d' % (lib.modl_conn_max_regions(), R))
    with torch.cuda.device(device):
        if X.stride(1) != 1 or X.stride(0) < V:
            X = X.contiguous()
        sh = _prepare_seeds(s).to(X.dtype).contiguous()
        out = torch.empty((R, V), dtype=X.dtype, device=device)
        call('modl_conn_seed_maps', X, X.stride(0), T, V, sh, R, out, V, STREAM, device=device, dtype=X)
    return out if cuda else out.cpu().numpy()


def seed_correlation_host(rows, seeds):
    """`seed_correlation` through numpy, in f64 from the same prepared seeds"""
    rows = rows.cpu().numpy() if isinstance(rows, torch.Tensor) else np.asarray(rows)
    seeds = seeds.cpu().numpy() if isinstance(seeds, torch.Tensor) else np.asarray(seeds)
    dtype = rows.dtype if rows.dtype in (np.float32, np.float64) else np.dtype(np.float64)
    seeds = _check_seed_args(rows, seeds)
    sh = prepare_seeds_host(seeds).astype(dtype).astype(np.float64)
    X = rows.astype(np.float64)
    T = X.shape[0]
    sx, sxx = X.sum(axis=0), (X * X).sum(axis=0)
    ss = sxx - sx * sx / T
    ok = ss > 8.0 * T * U64 * sxx
    out = (sh.T @ X) / np.sqrt(np.where(ok, ss, 1.0))
    out[:, ~ok] = 0.0
    return np.clip(out, -1.0, 1.0).astype(dtype)
