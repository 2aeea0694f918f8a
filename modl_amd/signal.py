"""Signal cleaning of fMRI records on the device: linear detrending, confound regression and standardization, the
arithmetic of `nilearn.signal.clean` that the reference's masker applies to every record before `partial_fit`
(modl/decomposition/fmri.py:281-296 the defaults, :525-526 and :577-585 the calls).  DESIGN.md section 20.

The three steps are ONE orthogonal projection.  `cleaning_basis` builds, on the host in f64, a matrix Q (T x q) with
orthonormal columns that spans the constant, the linear ramp and the confounds; per column x of a record (T time points x
V voxels) `clean` then computes

    r = x - Q (Q^T x),        out = r sqrt(T) / |r|  when standardizing (population variance 1),  r  otherwise.

When standardizing, a column is FLAT and comes out as exact zeros if |r|^2 <= (q T eps64)^2 |x|^2: that factor is the
worst-case f64 rounding of the projection, so what is left of such a column is rounding noise and not signal.  Without
standardization nothing is zeroed.  A NaN or Inf poisons its own column only, which comes out as NaN throughout.

Temporal filtering.  With `low_pass` and / or `high_pass` (Hz; `t_r` the repetition time in seconds)
a Butterworth filter of order `filter_order` is applied forwards and backwards (zero phase) before the projection.
`butterworth_coefficients` builds (b, a, zi) on the host in f64 with scipy.signal.butter / lfilter_zi; filtering a column
is exactly scipy.signal.filtfilt(b, a, x) with its defaults (padlen = 3 len(b), odd extension), so T > 3 len(b) is needed.
`clean` with a filter runs three steps:

    1. if `detrend`: the least-squares line (mean and ramp) is subtracted from every column, and from every confound;
    2. every column of the signals is filtered (device, csrc/filtfilt.hip), and every confound (host, scipy); a confound
       that the two steps leave at sqrt(eps64) of its norm or less (the ramp, a constant under a high-pass) is dropped;
    3. the projection above with Q2 = cleaning_basis(T, detrend=False, standardize, <filtered confounds>), standardizing
       as without a filter; when Q2 has no column the result of step 2 is the result.

This is the order of current nilearn (signals and confounds filtered alike, then regressed); older releases regressed
unfiltered confounds before filtering.  nilearn is not installed where this was written, so nothing is pinned to a run of
it: the steps are judged against scipy (tests/test_filter.py).  Without a filter nothing changes, bit for bit.

`smoothing_fwhm` needs the 3-D volume and so belongs to the masker: modl_amd/masker.py (`smooth_mask`, `ArrayMasker`,
DESIGN.md section 23) smooths and masks a 4-D volume on the device before this cleaning.
Not implemented (arguments of nilearn.signal.clean that need more than this): `sessions` (clean each session with a call
of its own) and `standardize='psc'`."""
import functools

import numpy as np
import scipy.linalg
import scipy.signal
import torch

from ._lib import lib
from .device import STREAM, call, current_device, dtype_id, have_gpu, scratch

_EPS = float(np.finfo(np.float64).eps)
CLEAN_MAX_REGRESSORS = lib.modl_clean_max_regressors()     # 64: the coefficients a thread of the kernel keeps
FILTER_MAX_TAPS = lib.modl_filtfilt_max_taps()             # 12: a band of order 5 has 11

__all__ = ['cleaning_basis', 'clean', 'clean_host', 'butterworth', 'butterworth_coefficients']


def _load_confounds(confounds, T):
    if confounds is None:
        return None
    if isinstance(confounds, str):
        confounds = np.load(confounds) if confounds.endswith('.npy') else np.loadtxt(
            confounds, delimiter=',' if confounds.endswith('.csv') else None, ndmin=2)
    if isinstance(confounds, torch.Tensor):
        confounds = confounds.detach().cpu().numpy()
    conf = np.asarray(confounds, dtype=np.float64)
    if conf.ndim == 1:
        conf = conf[:, None]
    if conf.ndim != 2:
        raise ValueError('confounds must be (n_time_points, n_confounds), got shape %s' % (conf.shape,))
    if conf.shape[0] != T:
        raise ValueError('confounds have %d time points, the signals have %d' % (conf.shape[0], T))
    if not np.all(np.isfinite(conf)):
        raise ValueError('confounds contain NaN or Inf')
    return conf


def _residualise(A, Q):
    for _ in range(2):                                   # twice is enough (classical Gram-Schmidt, repeated)
        A = A - Q.dot(Q.T.dot(A))
    return A


@functools.lru_cache(maxsize=32)
def _butterworth_cached(t_r, low_pass, high_pass, order):
    nyq = 0.5 / t_r
    for name, f in (('low_pass', low_pass), ('high_pass', high_pass)):
        if f is not None and not 0 < f < nyq:
            raise ValueError('%s = %g Hz is not inside (0, %g), the Nyquist frequency of t_r = %g s' % (name, f, nyq, t_r))
    if low_pass is not None and high_pass is not None:
        if high_pass >= low_pass:
            raise ValueError('high_pass = %g must be below low_pass = %g' % (high_pass, low_pass))
        b, a = scipy.signal.butter(order, [high_pass / nyq, low_pass / nyq], 'band')
    elif high_pass is not None:
        b, a = scipy.signal.butter(order, high_pass / nyq, 'high')
    else:
        b, a = scipy.signal.butter(order, low_pass / nyq, 'low')
    if len(b) > FILTER_MAX_TAPS:
        raise ValueError('order %d gives %d taps, at most %d are supported' % (order, len(b), FILTER_MAX_TAPS))
    return b, a, scipy.signal.lfilter_zi(b, a)


def butterworth_coefficients(t_r, low_pass=None, high_pass=None, order=5):
    """(b, a, zi), f64: scipy.signal.butter(order, ., 'low' / 'high' / 'band') at the frequencies low_pass, high_pass (Hz)
    over the Nyquist frequency 0.5 / t_r, and zi = scipy.signal.lfilter_zi(b, a).  len(b) = order + 1, 2 order + 1 for a
    band; a[0] == 1.
    ValueError: no frequency given, no or a non-positive `t_r`, a frequency outside (0, Nyquist), high_pass >= low_pass,
    order < 1, more than modl_filtfilt_max_taps() = 12 taps."""
    if low_pass is None and high_pass is None:
        raise ValueError('low_pass or high_pass must be given')
    if t_r is None:
        raise ValueError('a filter needs t_r, the repetition time in seconds')
    t_r = float(t_r)
    if not (t_r > 0 and np.isfinite(t_r)):
        raise ValueError('t_r must be positive, got %r' % t_r)
    if int(order) != order or order < 1:
        raise ValueError('order must be an integer >= 1, got %r' % (order,))
    b, a, zi = _butterworth_cached(t_r, None if low_pass is None else float(low_pass),
                                   None if high_pass is None else float(high_pass), int(order))
    return b.copy(), a.copy(), zi.copy()


def _filter_coefficients(low_pass, high_pass, t_r, filter_order):
    """None without a filter, otherwise (b, a, zi)"""
    if low_pass is None and high_pass is None:
        return None
    return butterworth_coefficients(t_r, low_pass, high_pass, filter_order)


def _check_filter_length(T, coef):
    if T <= 3 * len(coef[0]):
        raise ValueError('filtering needs more than 3 * %d = %d time points (the padding of filtfilt), got %d'
                         % (len(coef[0]), 3 * len(coef[0]), T))


def _detrend_host(x):
    """x (T, V) f64 minus the least-squares line of every column"""
    T = x.shape[0]
    ramp = np.arange(T, dtype=np.float64) - (T - 1) / 2.0
    x = x - x.mean(axis=0)
    if T > 1:
        x = x - np.outer(ramp, ramp.dot(x) / ramp.dot(ramp))
    return x


def _filter_host(x, coef, detrend):
    """steps 1 and 2 on the host in f64: (T, V) f64; a column with a NaN or Inf comes out as NaN throughout"""
    x = np.asarray(x, dtype=np.float64)
    bad = ~np.all(np.isfinite(x), axis=0)
    with np.errstate(invalid='ignore', over='ignore'):
        if detrend:
            x = _detrend_host(x)
        y = scipy.signal.filtfilt(coef[0], coef[1], x, axis=0)
    y[:, bad] = np.nan
    return y


def _filter_confounds(conf, coef, detrend):
    """steps 1 and 2 on the confounds (T, c) f64.  A confound whose norm afterwards is at most sqrt(eps64) times its norm
    before (the ramp under `detrend`, a constant under a high-pass: 156 dB down) holds rounding noise and no signal, and
    is dropped - as a regressor it would be normalised back to unit size."""
    if conf is None or conf.shape[1] == 0:
        return conf
    out = _filter_host(conf, coef, detrend)
    return out[:, np.linalg.norm(out, axis=0) > np.sqrt(_EPS) * np.linalg.norm(conf, axis=0)]


def cleaning_basis(T, detrend=True, standardize=True, confounds=None, low_pass=None, high_pass=None, t_r=None,
                   filter_order=5):
    """Q (T, q), f64, orthonormal columns: what `clean` projects out of every column.

    With a filter (`low_pass` / `high_pass`, module docstring) this is the basis Q2 of step 3: the confounds are
    detrended when `detrend`, filtered like the signals, and go through the rules below with detrend = False (the
    line has already left signals and confounds); a confound that the two steps reduce to rounding noise (norm down by
    sqrt(eps64) or more) is dropped first.

    The constant 1/sqrt(T) is in Q when detrending or standardizing, the centred and normalised linear ramp when
    detrending (not for T = 1, where it vanishes).  Confounds (array (T, c), or the path of a .npy / .csv file) are
    centred in every case, as nilearn does, residualised on what is already in Q and scaled to unit norm; a column whose
    residual norm is at most 100 eps sqrt(T) times its centred norm is dropped, the rest goes through a pivoted QR where
    columns with |R_ii| <= 100 eps are dropped (nilearn's rank rule).  With neither `detrend` nor `standardize` the
    constant is taken out of Q again: only the confounds are removed and the mean of the record is kept.
    ValueError: more than modl_clean_max_regressors() = 64 columns are left, or bad confounds."""
    T = int(T)
    if T < 1:
        raise ValueError('T must be at least 1, got %d' % T)
    conf = _load_confounds(confounds, T)
    coef = _filter_coefficients(low_pass, high_pass, t_r, filter_order)
    if coef is not None:
        _check_filter_length(T, coef)
        conf = _filter_confounds(conf, coef, detrend)
        detrend = False
    Q = np.full((T, 1), 1.0 / np.sqrt(T))
    if detrend:
        ramp = np.arange(T, dtype=np.float64) - (T - 1) / 2.0
        norm = np.linalg.norm(ramp)
        if norm > 0:
            Q = np.column_stack([Q, ramp / norm])
    if conf is not None and conf.shape[1] > 0:
        centred = conf - conf.mean(axis=0)
        centred_norm = np.linalg.norm(centred, axis=0)
        res = _residualise(centred, Q)
        res_norm = np.linalg.norm(res, axis=0)
        keep = res_norm > 100 * _EPS * np.sqrt(T) * centred_norm
        if np.any(keep):
            res = res[:, keep] / res_norm[keep]
            Qc, R, _ = scipy.linalg.qr(res, mode='economic', pivoting=True)
            rank = int(np.sum(np.abs(np.diag(R)) > 100 * _EPS))
            Qc = _residualise(Qc[:, :rank], Q)
            Q = np.column_stack([Q, Qc / np.linalg.norm(Qc, axis=0)])
    if not (detrend or standardize):
        Q = Q[:, 1:]
    if Q.shape[1] > min(T, CLEAN_MAX_REGRESSORS):
        raise ValueError('%d regressors are left after the rank rule, at most %d are supported'
                         % (Q.shape[1], min(T, CLEAN_MAX_REGRESSORS)))
    return np.ascontiguousarray(Q)


def _destination_rows(permutation, T):
    """result == cleaned[permutation]  <=>  cleaned row t goes to row dst[t], dst the inverse permutation"""
    if permutation is None:
        return None
    perm = np.asarray(permutation)
    if perm.ndim != 1 or perm.shape[0] != T or perm.dtype.kind not in 'iu' or \
            not np.array_equal(np.sort(perm), np.arange(T)):
        raise ValueError('permutation must be a permutation of 0 .. %d' % (T - 1))
    dst = np.empty(T, dtype=np.int64)
    dst[perm] = np.arange(T, dtype=np.int64)
    return dst


def _project_host(X, Q, standardize):
    """the projection in f64 numpy: (T, V) f64"""
    T, q = Q.shape
    x = np.asarray(X, dtype=np.float64)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        r = x - Q.dot(Q.T.dot(x))
        xx = np.sum(x * x, axis=0)
        if standardize:
            rr = np.sum(r * r, axis=0)
            flat = rr <= (q * T * _EPS) ** 2 * xx
            r = r * (np.sqrt(T) / np.sqrt(rr))
            r[:, flat] = 0.0
        r[:, ~np.isfinite(xx)] = np.nan                  # a NaN or Inf in a column: NaN throughout
    return r


def _check_signals(signals):
    if signals.ndim != 2:
        raise ValueError('signals must be (n_time_points, n_voxels), got shape %s' % (tuple(signals.shape),))
    if signals.shape[0] < 1 or signals.shape[1] < 1:
        raise ValueError('signals must not be empty, got shape %s' % (tuple(signals.shape),))


def _rows_ok(t):
    return t.shape[1] == 1 or t.stride(1) == 1


def _overlap(a, b):
    """do two 2-D tensors with unit column stride touch the same bytes (as address ranges)"""
    es = a.element_size()
    a0, b0 = a.data_ptr(), b.data_ptr()
    a1 = a0 + ((a.shape[0] - 1) * a.stride(0) + a.shape[1]) * es
    b1 = b0 + ((b.shape[0] - 1) * b.stride(0) + b.shape[1]) * es
    return a0 < b1 and b0 < a1


def _prepare(signals, detrend, standardize, confounds, permutation, out, basis, coef=None):
    """The one validator of `clean` and `clean_host`: (X, Q, dst) - the signals as they will be read (numpy array or CUDA
    tensor, float32 / float64, unit column stride), the basis and the kernel's destination rows.  `coef`: the filter's
    (b, a, zi) or None; with it Q is the basis of step 3.  Raises ValueError."""
    cuda = isinstance(signals, torch.Tensor)
    if cuda and not signals.is_cuda:
        raise ValueError('signals must be a numpy array or a CUDA tensor, got a tensor on %s' % signals.device)
    X = signals if cuda else np.asarray(signals)
    _check_signals(X)
    if cuda:
        if X.dtype not in (torch.float32, torch.float64):
            raise ValueError('a CUDA tensor of float32 or float64 is expected, got %s' % X.dtype)
        if not _rows_ok(X):
            X = X.contiguous()
    elif X.dtype not in (np.float32, np.float64):
        X = X.astype(np.float64)
    T = X.shape[0]
    if coef is not None:
        _check_filter_length(T, coef)
    if basis is None:
        if coef is None:
            Q = cleaning_basis(T, detrend, standardize, confounds)
        else:
            Q = cleaning_basis(T, False, standardize, _filter_confounds(_load_confounds(confounds, T), coef, detrend))
    else:
        Q = np.ascontiguousarray(basis, dtype=np.float64)
        if Q.ndim != 2 or Q.shape[0] != T or Q.shape[1] > min(T, CLEAN_MAX_REGRESSORS):
            raise ValueError('basis must be (%d, q) with q <= %d, got shape %s' % (T, min(T, CLEAN_MAX_REGRESSORS), Q.shape))
    dst = _destination_rows(permutation, T)
    if out is not None:
        if cuda:
            if not (isinstance(out, torch.Tensor) and out.is_cuda and out.device == X.device and out.dtype == X.dtype
                    and tuple(out.shape) == tuple(X.shape) and _rows_ok(out)):
                raise ValueError('out must be a CUDA tensor of the shape, dtype and device of signals with contiguous rows')
            same = out.data_ptr() == X.data_ptr() and out.stride(0) == X.stride(0)
            aliased = _overlap(out, X) and (dst is not None or not same)
        else:
            if not isinstance(out, np.ndarray) or out.shape != X.shape or out.dtype != X.dtype:
                raise ValueError('out must be a numpy array of the shape and dtype of signals')
            aliased = dst is not None and np.may_share_memory(out, X)
        if aliased:
            raise ValueError('out may alias signals only as the same view, and not together with a permutation')
    return X, Q, dst


def _finish_host(X, Q, standardize, permutation, out):
    res = X if Q.shape[1] == 0 else _project_host(X, Q, standardize).astype(X.dtype)
    if permutation is not None:
        res = res[np.asarray(permutation)]
    if out is None:
        return res
    if out is not res:
        out[...] = res
    return out


def _clean_host(X, Q, coef, detrend, standardize, permutation, out):
    if coef is None:
        return _finish_host(X, Q, standardize, permutation, out)
    F = _filter_host(X, coef, detrend)                   # f64; rounded once, by the projection or here
    F = F.astype(X.dtype) if Q.shape[1] == 0 else _project_host(F, Q, standardize).astype(X.dtype)
    return _finish_host(F, Q[:, :0], standardize, permutation, out)


def clean_host(signals, detrend=True, standardize=True, confounds=None, permutation=None, out=None, basis=None,
               low_pass=None, high_pass=None, t_r=None, filter_order=5):
    """`clean` in f64 numpy / scipy on the host, same semantics (the flat rule included), result rounded once to the
    dtype of `signals`: what `clean` runs without a GPU, and the CPU baseline of scripts/bench_clean.py."""
    if isinstance(signals, torch.Tensor):
        raise ValueError('clean_host takes a numpy array')
    coef = _filter_coefficients(low_pass, high_pass, t_r, filter_order)
    X, Q, _ = _prepare(signals, detrend, standardize, confounds, permutation, out, basis, coef)
    return _clean_host(X, Q, coef, detrend, standardize, permutation, out)


def _filtfilt_device(X, coef, detrend, dst, out):
    """X: CUDA tensor (T, V) with unit column stride; coef: (b, a, zi) f64 numpy; dst: int64 numpy or None"""
    T, V = X.shape
    b, a, zi = (np.ascontiguousarray(c, dtype=np.float64) for c in coef)
    if out is None:
        out = torch.empty((T, V), dtype=X.dtype, device=X.device)
    need = lib.modl_filtfilt_workspace(dtype_id(X), T, V, len(b))
    if need == 0:
        raise ValueError('modl_filtfilt: unsupported shape T = %d, V = %d, %d taps' % (T, V, len(b)))
    d_dst = None if dst is None else torch.from_numpy(dst).to(X.device)
    ws = scratch(need, X.device)
    call('modl_filtfilt', X, X.stride(0), T, V, b, a, zi, len(b), int(bool(detrend)), d_dst, out, out.stride(0), ws, need,
         STREAM, device=X.device, dtype=X)
    return out


def _clean_device(X, Q, standardize, dst, out):
    """X: CUDA tensor (T, V) with unit column stride; Q: f64 numpy (T, q), q >= 1; dst: int64 numpy or None"""
    T, V = X.shape
    q = Q.shape[1]
    if out is None:
        out = torch.empty((T, V), dtype=X.dtype, device=X.device)
    need = lib.modl_clean_workspace(dtype_id(X), T, V, q)
    if need == 0:
        raise ValueError('modl_clean: unsupported shape T = %d, V = %d, q = %d' % (T, V, q))
    d_Q = torch.from_numpy(np.ascontiguousarray(Q)).to(X.device)
    d_dst = None if dst is None else torch.from_numpy(dst).to(X.device)
    ws = scratch(need, X.device)
    call('modl_clean', X, X.stride(0), T, V, d_Q, q, int(bool(standardize)), d_dst, out, out.stride(0), ws, need, STREAM,
         device=X.device, dtype=X)
    return out


def clean(signals, detrend=True, standardize=True, confounds=None, permutation=None, out=None, basis=None,
          low_pass=None, high_pass=None, t_r=None, filter_order=5):
    """Detrend, filter, regress confounds out of and standardize one record (module docstring), on the device.

    signals      (T, V) time points x voxels, float32 or float64: a numpy array (a numpy array comes back) or a CUDA
                 tensor (a CUDA tensor comes back, nothing crosses the host link but the small basis).  A view with a row
                 stride is used as it stands.
    detrend      remove the mean and the linear trend of every column
    standardize  scale every column to zero mean and population variance 1; flat columns become exact zeros
    confounds    None, (T, c) array, or the path of a .npy / .csv file: regressed out of every column
    permutation  None or a permutation of 0 .. T-1: the result is clean(...)[permutation], written in that order by the
                 kernel itself (fMRIDictFact.fit folds the row permutation of every record into its cleaning)
    out          None, or where to write: same kind, shape and dtype as `signals`.  `out is signals` cleans in place;
                 together with a permutation `out` must not alias `signals`.
    basis        None, or what cleaning_basis(T, detrend, standardize, confounds) returned for this record: it is used
                 instead of building it again (`detrend` and `confounds` are then not looked at) - for a record that
                 is cleaned more than once, as in every epoch of a fit.  With a filter: what cleaning_basis returned
                 with the same filter arguments (Q2); `detrend` then still steers step 1 on the signals.
    low_pass, high_pass   None, or the cut-off frequencies in Hz of a zero-phase Butterworth filter (module docstring):
                 low_pass alone, high_pass alone, or both for a band (high_pass < low_pass).  Needs `t_r` and
                 T > 3 taps (taps = filter_order + 1, or 2 filter_order + 1 for a band).
    t_r          repetition time in seconds
    filter_order order of the Butterworth filter (5 as in nilearn)

    With nothing to remove (detrend = standardize = False, no confounds left) the input itself is returned, no launch.
    Every column is computed on its own with sums in f64 in an order that depends on T alone: clean(X[:, a:b]) has the
    bits of clean(X)[:, a:b].  Without a GPU a numpy input goes through `clean_host`.
    With a filter the record is filtered by one launch (csrc/filtfilt.hip) into a temporary of its dtype and projected
    from there; when nothing is left to project (no standardize, no confounds) that launch writes the result itself.
    ValueError: wrong ranks, a T mismatch between signals and confounds, non-finite confounds, more than 64 regressors,
    a `permutation` that is none, an `out` that does not fit or aliases the input together with a permutation, bad
    filter arguments (butterworth_coefficients) or T <= 3 taps."""
    coef = _filter_coefficients(low_pass, high_pass, t_r, filter_order)
    X, Q, dst = _prepare(signals, detrend, standardize, confounds, permutation, out, basis, coef)
    if isinstance(X, torch.Tensor):
        if coef is not None:
            if Q.shape[1] == 0:
                return _filtfilt_device(X, coef, detrend, dst, out)
            return _clean_device(_filtfilt_device(X, coef, detrend, None, None), Q, standardize, dst, out)
        if Q.shape[1] > 0:
            return _clean_device(X, Q, standardize, dst, out)
        res = X if permutation is None else X[torch.from_numpy(np.asarray(permutation, dtype=np.int64)).to(X.device)]
        if out is None:
            return res
        if not (out.data_ptr() == res.data_ptr() and out.stride(0) == res.stride(0)):
            out.copy_(res)
        return out
    if (coef is None and Q.shape[1] == 0) or not have_gpu():
        return _clean_host(X, Q, coef, detrend, standardize, permutation, out)
    device = current_device()
    res = torch.from_numpy(np.ascontiguousarray(X)).to(device)
    if coef is not None:
        res = _filtfilt_device(res, coef, detrend, dst if Q.shape[1] == 0 else None, None)
    if Q.shape[1] > 0:
        res = _clean_device(res, Q, standardize, dst, None)
    res = res.cpu().numpy()
    if out is None:
        return res
    out[...] = res
    return out


def butterworth(signals, t_r, low_pass=None, high_pass=None, order=5, detrend=False, permutation=None, out=None):
    """Zero-phase Butterworth filtering of every column of one record on the device: scipy.signal.filtfilt(b, a, x) with
    (b, a) = butterworth_coefficients(t_r, low_pass, high_pass, order), after subtracting the column's least-squares
    line when `detrend`.  `signals`, `permutation` and `out` as in `clean` (numpy in, numpy out; CUDA tensor in, CUDA
    tensor out; a view with a row stride is used as it stands); without a GPU a numpy input goes through scipy.
    A column with a NaN or Inf comes out as NaN throughout, an all-zero column as exact zeros; filtering X[:, a:b] gives
    the bits of the full result's columns a:b.
    ValueError: as butterworth_coefficients, and T <= 3 len(b)."""
    if low_pass is None and high_pass is None:
        raise ValueError('low_pass or high_pass must be given')
    return clean(signals, detrend, False, None, permutation, out, None, low_pass, high_pass, t_r, order)
