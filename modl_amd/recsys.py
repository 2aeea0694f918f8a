"""RecsysDictFact: masked (missing-data) online matrix factorization on a CSR
rating matrix (reference: modl/decomposition/recsys.py:17-314).  Same
constructor, attributes and methods; the per-sample Python loop of the
reference (`_single_sample_update`, recsys.py:168-185) runs as batched GPU
kernels (csrc/recsys.hip), the dictionary update reuses the dense path's
block-coordinate kernels."""
import ctypes as C
import os
from collections import namedtuple
from math import log, ceil

import numpy as np
import scipy.sparse as sp
import torch
from sklearn.base import BaseEstimator
from sklearn.utils import check_array, check_random_state, gen_batches

from ._lib import lib, check, RECSYS_MAX_TOPN, RECSYS_MAX_RANK_TARGETS
from .device import (STREAM, call, default_device, dtype_id, scratch, sfx, torch_dtype, ptr, stream_ptr, to_device,
                     transpose_to)
from .randomkit import batch_weight


# The largest n_components the ridge-code kernels take, per dtype: the row's k x k system, its right-hand side and 32 staged
# dictionary rows must fit the 160 KiB of LDS of a workgroup (csrc/recsys.hip: recsys_codes; include/modl_hip.h,
# modl_recsys_codes_*).  tests/test_recsys_kernels.py pins both numbers to what the entry point accepts.
MAX_COMPONENTS = {np.dtype(np.float32): 186, np.dtype(np.float64): 127}
# recommend(): the longest list modl_recsys_topn_* returns (MODL_RECSYS_MAX_TOPN), and the workspace a call may take
MAX_TOPN = RECSYS_MAX_TOPN
TOPN_WORKSPACE_BYTES = 256 << 20
# ranks(): the longest target row of one query of modl_recsys_ranks_* (MODL_RECSYS_MAX_RANK_TARGETS); longer rows are split
MAX_RANK_TARGETS = RECSYS_MAX_RANK_TARGETS

RankingScore = namedtuple('RankingScore', ['hit_rate', 'precision', 'recall', 'ndcg', 'mrr', 'auc', 'n_users', 'n_targets'])


def compute_biases(X, beta=0, inplace=False):
    """Row / column centring of a CSR matrix (recsys.py:268-306), host code."""
    if not inplace:
        X = X.copy()
    X = sp.csr_matrix(X)
    acc_u, acc_m = np.zeros(X.shape[0]), np.zeros(X.shape[1])
    n_u, n_m = X.getnnz(axis=1), X.getnnz(axis=0)
    n_u[n_u == 0] = 1
    n_m[n_m == 0] = 1
    average_rating = np.mean(X.data)
    for _ in range(2):
        w_u = (np.asarray(X.sum(axis=1))[:, 0] + average_rating * beta) / (n_u + beta)
        X.data -= np.repeat(w_u, np.diff(X.indptr))
        w_m = np.asarray(X.sum(axis=0))[0] / (n_m + beta)
        X.data -= w_m.take(X.indices, mode='clip')
        acc_u += w_u
        acc_m += w_m
    return acc_u, acc_m


def rmse(X_true, X_pred):
    """recsys.py:309-314"""
    X_true = check_array(X_true, accept_sparse='csr')
    X_pred = check_array(X_pred, accept_sparse='csr')
    return np.sqrt(np.mean((X_true.data - X_pred.data) ** 2))


def ranking_metrics(ranks, indptr, n_candidates, n_items):
    """Ranking figures at n_items from 0-based ranks: a RankingScore.  ranks[indptr[u]:indptr[u + 1]] are the ranks of the
    m targets of user u among the user's n_candidates[u] candidates (the targets are distinct candidates; a target's rank
    counts the user's other targets that beat it).  Per user, with hits = #(rank < n_items):
    hit_rate = [hits > 0]; precision = hits / n_items; recall = hits / m; ndcg = sum_{rank < n_items} 1 / log2(rank + 2) over
    its best possible value sum_{i < min(m, n_items)} 1 / log2(i + 2); mrr = 1 / (min rank + 1); auc = the share of the
    m (n_candidates - m) pairs (target, other candidate) that the target wins.  Means over the users with targets (auc: over
    those with n_candidates > m as well); NaN where no user is left.  Host code, float64."""
    ranks = np.asarray(ranks, dtype=np.int64)
    indptr = np.asarray(indptr, dtype=np.int64)
    n_candidates = np.asarray(n_candidates, dtype=np.int64)
    n_items = int(n_items)
    n_u = len(indptr) - 1
    if n_items < 1 or n_u < 0 or ranks.shape != (int(indptr[-1]) - int(indptr[0]),) or n_candidates.shape != (n_u,):
        raise ValueError('ranking_metrics: ranks, indptr and n_candidates do not fit together, or n_items < 1')
    if np.any(ranks < 0):
        raise ValueError('ranking_metrics: a rank is negative (a target outside the items?)')
    m = np.diff(indptr)
    start = indptr[:-1] - indptr[0]
    user = np.repeat(np.arange(n_u), m)
    hit = ranks < n_items
    hits = np.bincount(user, weights=hit, minlength=n_u)
    dcg = np.bincount(user, weights=np.where(hit, 1.0 / np.log2(ranks + 2.0), 0.0), minlength=n_u)
    ideal = np.concatenate([[0.0], np.cumsum(1.0 / np.log2(np.arange(n_items) + 2.0))])[np.minimum(m, n_items)]
    best = np.full(n_u, np.iinfo(np.int64).max)
    np.minimum.at(best, user, ranks)
    # j_t, the user's own targets that beat t: its place among the user's ranks (equal ranks share the first place)
    order = np.lexsort((ranks, user))
    su, sr = user[order], ranks[order]
    idx = np.arange(len(sr))
    new = np.ones(len(sr), dtype=bool)
    new[1:] = (su[1:] != su[:-1]) | (sr[1:] != sr[:-1])
    first = np.maximum.accumulate(np.where(new, idx, 0)) if len(sr) else idx
    lost = np.bincount(su, weights=(sr - (first - start[su])).astype(np.float64), minlength=n_u)
    has = m > 0
    mh = m[has].astype(np.float64)
    pairs = (m * (n_candidates - m)).astype(np.float64)
    ok = has & (n_candidates > m)
    mean = lambda v: float(np.mean(v)) if len(v) else float('nan')
    return RankingScore(hit_rate=mean((hits[has] > 0).astype(np.float64)), precision=mean(hits[has] / n_items),
                        recall=mean(hits[has] / mh), ndcg=mean(dcg[has] / ideal[has]),
                        mrr=mean(1.0 / (best[has] + 1.0)), auc=mean(1.0 - lost[ok] / pairs[ok]), n_users=int(has.sum()),
                        n_targets=int(m.sum()))


def _csr_piece(a, dtype, device):
    """a CSR array on the device; an empty one as a single unused element (the entry points refuse a NULL pointer)"""
    a = np.ascontiguousarray(a, dtype=dtype)
    return torch.from_numpy(a if a.size else np.zeros(1, dtype=dtype)).to(device)


class _RecsysDevice:
    """Device state and launches of one RecsysDictFact."""

    def __init__(self, X, k, dtype, device=None):
        self.device = torch.device(device) if device is not None else default_device()
        self.dtype = np.dtype(dtype)
        self.n, self.p = X.shape
        self.k = k
        dev = self.device
        self.plan, self.plan_batch = None, 0
        # the CSR matrix on both sides: the host copy feeds the per-batch grouping, the device copy the kernels
        self.h_indptr = np.ascontiguousarray(X.indptr, dtype=np.int32)
        self.h_indices = np.ascontiguousarray(X.indices, dtype=np.int32)
        self.h_data = np.ascontiguousarray(X.data, dtype=self.dtype)
        self.indptr = torch.from_numpy(self.h_indptr).to(dev)
        self.indices = torch.from_numpy(self.h_indices).to(dev)
        self.data = torch.from_numpy(self.h_data).to(dev)
        td = torch_dtype(self.dtype)
        self.Dt = torch.zeros((self.p, k), dtype=td, device=dev)
        self.Bt = torch.zeros((self.p, k), dtype=td, device=dev)
        self.C = torch.zeros((k, k), dtype=td, device=dev)
        self.code = torch.zeros((self.n, k), dtype=td, device=dev)
        self.comp_norm = torch.zeros(k, dtype=td, device=dev)
        self.feature_n_iter = torch.zeros(self.p, dtype=torch.int64, device=dev)
        nbytes = lib.modl_dict_update_workspace(dtype_id(self.dtype), self.p, k)
        self.ws = scratch(nbytes, dev)
        self.ws_bytes = nbytes

    def set_dictionary(self, D):
        self.Dt = transpose_to(to_device(D, self.device, dtype=self.dtype), self.k, self.p)

    def get_dictionary(self):
        return transpose_to(self.Dt, self.p, self.k).cpu().numpy()

    def codes(self, rows, alpha):
        """ridge codes of the CSR rows `rows` (None = all), written to code[rows]"""
        r = None if rows is None else torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int64)).to(self.device)
        call('modl_recsys_codes', self.Dt, self.p, self.k, self.indptr, self.indices, self.data, r, None,
             self.n if rows is None else len(rows), float(alpha), self.code, STREAM, device=self.device, dtype=self.dtype)

    def batch_update(self, batch, alpha, w, n_iter, order):
        """One minibatch (recsys.py:147-165) for the CSR rows `batch` (in this order): one asynchronous call
        (modl_recsys_minibatch_*: host grouping of the batch's ratings by item, staging, codes, B_, C_, dictionary)."""
        batch = np.ascontiguousarray(batch, dtype=np.int64)
        order = np.ascontiguousarray(order, dtype=np.int64)
        if self.plan is None or len(batch) > self.plan_batch:
            self._make_plan(len(batch))
        f = getattr(lib, 'modl_recsys_minibatch_' + sfx(self.dtype))
        check(f(self.plan, self.h_indptr.ctypes.data_as(C.c_void_p), self.h_indices.ctypes.data_as(C.c_void_p),
                self.h_data.ctypes.data_as(C.c_void_p), self.n, ptr(self.indptr), ptr(self.indices), ptr(self.data),
                batch.ctypes.data_as(C.c_void_p), len(batch), order.ctypes.data_as(C.c_void_p), float(alpha), float(w),
                float(n_iter), ptr(self.Dt), ptr(self.Bt), ptr(self.C), ptr(self.code), ptr(self.comp_norm),
                ptr(self.feature_n_iter), stream_ptr(self.device)), 'modl_recsys_minibatch')

    def fit_batches(self, rows, batch_size, alpha, learning_rate, n_iter, np_random_state):
        """A run of minibatches in ONE call (modl_recsys_fit_batches_*: the host loop of recsys.py:135-139 behind the ABI).
        `rows`: the permuted row ids of the run; the atom orders are drawn inside the library by a generator loaded with
        numpy's legacy MT19937 state and handed back afterwards, so `np_random_state` continues as if it had drawn them
        (recsys.py:196).  Returns the new n_iter_."""
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        if self.plan is None or batch_size > self.plan_batch:
            self._make_plan(batch_size)
        if getattr(self, '_order_rk', None) is None:
            h = C.c_void_p()
            check(lib.modl_rk_create(0, C.byref(h)), 'modl_rk_create')
            self._order_rk = h
        kind, key, pos, has_gauss, cached = np_random_state.get_state()
        key = np.ascontiguousarray(key, dtype=np.uint32)
        check(lib.modl_rk_set_mt_state(self._order_rk, key.ctypes.data_as(C.c_void_p), int(pos)), 'modl_rk_set_mt_state')
        n = C.c_int64(int(n_iter))
        done = C.c_int64(0)
        f = getattr(lib, 'modl_recsys_fit_batches_' + sfx(self.dtype))
        try:
            rc = f(self.plan, self.h_indptr.ctypes.data_as(C.c_void_p), self.h_indices.ctypes.data_as(C.c_void_p),
                   self.h_data.ctypes.data_as(C.c_void_p), self.n, ptr(self.indptr), ptr(self.indices), ptr(self.data),
                   rows.ctypes.data_as(C.c_void_p), len(rows), int(batch_size), self._order_rk, float(alpha),
                   float(learning_rate), C.byref(n), ptr(self.Dt), ptr(self.Bt), ptr(self.C), ptr(self.code),
                   ptr(self.comp_norm), ptr(self.feature_n_iter), stream_ptr(self.device), C.byref(done))
        finally:
            out = np.empty(624, dtype=np.uint32)
            p2 = C.c_int32()
            check(lib.modl_rk_get_mt_state(self._order_rk, out.ctypes.data_as(C.c_void_p), C.byref(p2)))
            np_random_state.set_state((kind, out, int(p2.value), has_gauss, cached))
        check(rc, 'modl_recsys_fit_batches')
        return int(n.value)

    def launch_counts(self):
        """(minibatches that ran as one launch, minibatches that ran as separate launches) of the current plan"""
        a, b = C.c_int64(0), C.c_int64(0)
        if self.plan is not None:
            check(lib.modl_recsys_plan_counts(self.plan, C.byref(a), C.byref(b)), 'modl_recsys_plan_counts')
        return int(a.value), int(b.value)

    def _make_plan(self, batch_size):
        self._free_plan()
        # the largest number of ratings a batch of this size can hold: its batch_size longest rows
        lens = np.sort(np.diff(self.h_indptr))[::-1]
        max_entries = int(lens[:batch_size].sum())
        h = C.c_void_p()
        self._pid = os.getpid()
        with torch.cuda.device(self.device):
            check(lib.modl_recsys_plan_create(dtype_id(self.dtype), self.p, self.k, batch_size, max_entries, C.byref(h)),
                  'modl_recsys_plan_create')
        self.plan, self.plan_batch = h, batch_size

    def _free_plan(self):
        # (a forked child - e.g. multiprocessing's helpers - must never release the parent's device objects)
        if getattr(self, 'plan', None) and getattr(self, '_pid', os.getpid()) == os.getpid():
            lib.modl_recsys_plan_destroy(self.plan)
            if getattr(self, '_order_rk', None):
                lib.modl_rk_destroy(self._order_rk)
                self._order_rk = None
        self.plan, self.plan_batch = None, 0

    def __del__(self):
        try:
            self._free_plan()
        except Exception:
            pass

    def predict(self, Xp, code=None):
        """the product at the pattern of Xp (row u of Xp against row u of `code`; None: code_), in double"""
        dev = self.device
        code = self.code if code is None else code
        out = torch.zeros(Xp.nnz, dtype=torch.float64, device=dev)
        ind = torch.from_numpy(Xp.indices.astype(np.int32)).to(dev)
        iptr = torch.from_numpy(Xp.indptr.astype(np.int32)).to(dev)
        call('modl_recsys_predict', out, ind, iptr, code, Xp.shape[0], self.k, self.Dt, STREAM, device=dev, dtype=self.dtype)
        return out.cpu().numpy()

    def codes_of(self, X, alpha):
        """ridge codes of the rows of ANY ratings matrix with p columns under the current dictionary, into a fresh (zero)
        buffer: rows without ratings keep a zero code.  Returns the device tensor (rows, k)."""
        dev = self.device
        indptr = _csr_piece(X.indptr, np.int32, dev)
        indices = _csr_piece(X.indices, np.int32, dev)
        data = _csr_piece(X.data, self.dtype, dev)
        code = torch.zeros((X.shape[0], self.k), dtype=torch_dtype(self.dtype), device=dev)
        call('modl_recsys_codes', self.Dt, self.p, self.k, indptr, indices, data, None, None, X.shape[0], float(alpha), code,
             STREAM, device=dev, dtype=self.dtype)
        return code

    def topn_rows_per_call(self, b, n_top):
        """the most queries of one modl_recsys_topn_* call whose workspace stays under TOPN_WORKSPACE_BYTES"""
        rows = max(int(b), 1)
        while rows > 1 and lib.modl_recsys_topn_workspace(dtype_id(self.dtype), self.p, self.k, rows, n_top) > TOPN_WORKSPACE_BYTES:
            rows = (rows + 1) // 2
        return rows

    def topn(self, code, ex_indptr, ex_indices, ex_rows, item_bias, n_top, rows_per_call=None):
        """the n_top best items (int32 tensor (b, n_top), -1 where nothing is left) of the rows of `code`; excluded for row ii
        are the entries of row ex_rows[ii] (None: ii) of the CSR pattern ex_indptr / ex_indices (None: nothing)"""
        dev = self.device
        b = code.shape[0]
        items = torch.empty((b, n_top), dtype=torch.int32, device=dev)
        scores = torch.empty((b, n_top), dtype=torch_dtype(self.dtype), device=dev)
        if rows_per_call is None:
            rows_per_call = self.topn_rows_per_call(b, n_top)
        rows_per_call = max(int(rows_per_call), 1)
        nbytes = lib.modl_recsys_topn_workspace(dtype_id(self.dtype), self.p, self.k, min(rows_per_call, max(b, 1)), n_top)
        ws = scratch(nbytes, dev)
        for s in range(0, b, rows_per_call):
            e = min(s + rows_per_call, b)
            need = lib.modl_recsys_topn_workspace(dtype_id(self.dtype), self.p, self.k, e - s, n_top)
            if need > ws.numel():                           # (a short last chunk is cut into more slabs)
                ws = scratch(need, dev)
            if ex_indptr is None:
                ex = (None, None, None)
            elif ex_rows is None:
                # rows s .. e-1 of the pattern: the row pointers are absolute, so a view of indptr addresses them
                ex = (ex_indptr[s:], ex_indices, None)
            else:
                ex = (ex_indptr, ex_indices, ex_rows[s:e])
            call('modl_recsys_topn', code[s:e], None, e - s, self.k, self.Dt, self.p, *ex, item_bias, n_top, items[s:e],
                 scores[s:e], ws, ws.numel(), STREAM, device=dev, dtype=self.dtype)
        return items

    def ranks_rows_per_call(self, b, t_max):
        """the most queries of one modl_recsys_ranks_* call whose workspace stays under TOPN_WORKSPACE_BYTES"""
        rows = max(int(b), 1)
        while rows > 1 and lib.modl_recsys_ranks_workspace(dtype_id(self.dtype), self.p, self.k, rows, t_max) > TOPN_WORKSPACE_BYTES:
            rows = (rows + 1) // 2
        return rows

    def ranks(self, code, ex_indptr, ex_indices, ex_rows, item_bias, t_indptr, t_indices, rows_per_call=None):
        """(ranks int32 (entries,), n_candidates int32 (users,)) on the host: for user u (row u of `code`; exclusions as in
        topn) the rank of every entry of row u of the host CSR pattern t_indptr / t_indices among the items that are not
        excluded (-1: not an item).  n_candidates is -1 for a user without targets: no query is run for it.  A row of more
        than MAX_RANK_TARGETS entries becomes several queries with the same code and exclusion row and a finer row pointer
        over the same t_indices: the ranks come back in entry order."""
        dev = self.device
        nu = code.shape[0]
        t_indptr = np.ascontiguousarray(t_indptr, dtype=np.int64)
        m = np.diff(t_indptr)
        pieces = -(-m // MAX_RANK_TARGETS)                         # queries per user (none without targets)
        q_user = np.repeat(np.arange(nu, dtype=np.int64), pieces)
        nq = len(q_user)
        ranks = np.zeros(int(t_indptr[-1]), dtype=np.int32)
        n_cand = np.full(nu, -1, dtype=np.int32)
        if nq == 0:
            return ranks, n_cand
        q_first = np.cumsum(pieces) - pieces                       # the first query of each user
        q_ptr = t_indptr[q_user] + MAX_RANK_TARGETS * (np.arange(nq) - q_first[q_user])
        q_ptr = np.concatenate([q_ptr, t_indptr[-1:]]).astype(np.int32)
        q_len = np.diff(q_ptr)
        t_max = int(q_len.max())
        d_user = torch.from_numpy(q_user).to(dev)
        d_ex_rows = None if ex_indptr is None else (d_user if ex_rows is None else ex_rows.index_select(0, d_user))
        d_ptr = torch.from_numpy(q_ptr).to(dev)
        d_tidx = _csr_piece(t_indices, np.int32, dev)
        d_ranks = torch.zeros(max(len(ranks), 1), dtype=torch.int32, device=dev)
        d_cand = torch.zeros(nq, dtype=torch.int32, device=dev)
        if rows_per_call is None:
            rows_per_call = self.ranks_rows_per_call(nq, t_max)
        rows_per_call = max(int(rows_per_call), 1)
        ws = scratch(lib.modl_recsys_ranks_workspace(dtype_id(self.dtype), self.p, self.k, min(rows_per_call, nq), t_max), dev)
        for s in range(0, nq, rows_per_call):
            e = min(s + rows_per_call, nq)
            ex = (None, None, None) if ex_indptr is None else (ex_indptr, ex_indices, d_ex_rows[s:e])
            # queries s .. e-1: the row pointers are absolute, so a view of them addresses the same t_indices and ranks
            call('modl_recsys_ranks', code, d_user[s:e], e - s, self.k, self.Dt, self.p, *ex, item_bias, d_ptr[s:], d_tidx, t_max,
                 d_ranks, d_cand[s:e], ws, ws.numel(), STREAM, device=dev, dtype=self.dtype)
        ranks[:] = d_ranks.cpu().numpy()[:len(ranks)]
        n_cand[q_user] = d_cand.cpu().numpy()
        return ranks, n_cand


class RecsysDictFact(BaseEstimator):
    """Matrix factorization with missing data by masked online dictionary learning
    (recsys.py:17-79 for the parameters)."""

    def __init__(self, alpha=1.0, beta=.0, n_components=30, learning_rate=1., batch_size=1, dict_init=None,
                 l1_ratio=0, n_epochs=1, random_state=None, verbose=0, detrend=False, crop=None, callback=None,
                 device=None):
        self.callback = callback
        self.verbose = verbose
        self.random_state = random_state
        self.n_epochs = n_epochs
        self.l1_ratio = l1_ratio
        self.dict_init = dict_init
        self.batch_size = batch_size
        self.learning_rate = learning_rate
        self.n_components = n_components
        self.alpha = alpha
        self.beta = beta
        self.detrend = detrend
        self.crop = crop
        self.device = device

    # device-resident attributes
    @property
    def components_(self):
        return self._dev.get_dictionary()

    @property
    def code_(self):
        return self._dev.code.cpu().numpy()

    @property
    def C_(self):
        return self._dev.C.cpu().numpy()

    @property
    def B_(self):
        return transpose_to(self._dev.Bt, self._dev.p, self._dev.k).cpu().numpy()

    @property
    def comp_norm_(self):
        return self._dev.comp_norm.cpu().numpy()

    @property
    def feature_n_iter_(self):
        return self._dev.feature_n_iter.cpu().numpy()

    def fit(self, X, y=None):
        """recsys.py:81-141"""
        if not sp.issparse(X):
            X = sp.csr_matrix(X)
        X = check_array(X, accept_sparse='csr', dtype=[np.float32, np.float64], copy=True)
        dtype = X.dtype
        n_samples, n_features = X.shape
        if self.n_components > MAX_COMPONENTS[np.dtype(dtype)]:
            raise ValueError('RecsysDictFact: n_components = %d, but at most %d components are supported for %s ratings '
                             '(%d for float32, %d for float64): the ridge system of a row must fit the LDS of a workgroup'
                             % (self.n_components, MAX_COMPONENTS[np.dtype(dtype)], np.dtype(dtype).name,
                                MAX_COMPONENTS[np.dtype(np.float32)], MAX_COMPONENTS[np.dtype(np.float64)]))
        self.random_state = check_random_state(self.random_state)
        if self.detrend:
            self.global_mean_ = float(np.mean(X.data))        # (the average rating compute_biases shrinks the row means to)
            self.row_mean_, self.col_mean_ = compute_biases(X, beta=self.beta, inplace=False)
            X.data -= np.repeat(self.row_mean_, np.diff(X.indptr)).astype(dtype)
            X.data -= self.col_mean_.take(X.indices, mode='clip').astype(dtype)
        D = self.random_state.randn(self.n_components, n_features).astype(dtype)
        D /= np.sqrt(np.sum(D ** 2, axis=1))[:, np.newaxis]
        self._dev = dev = _RecsysDevice(X, self.n_components, dtype, self.device)
        dev.set_dictionary(D)
        self._refit()
        self.feature_freq_ = np.bincount(X.indices, minlength=n_features) / n_samples
        sparsity = X.nnz / n_samples / n_features
        batch_size = int(ceil(1. / sparsity)) if self.batch_size is None else self.batch_size
        self.n_iter_ = 0
        if self.verbose:
            log_lim = log(n_samples * self.n_epochs / batch_size, 10)
            self.verbose_iter_ = ((np.logspace(0, log_lim, self.verbose, base=10) - 1) * batch_size).tolist()
        for _ in range(self.n_epochs):
            permutation = self.random_state.permutation(n_samples)
            if self.verbose or self.callback is not None or not hasattr(self.random_state, 'get_state'):
                for batch in gen_batches(n_samples, batch_size):
                    self._single_batch_fit(X, permutation[batch])
            else:
                # nothing to report between minibatches: the epoch's host loop runs behind the ABI, one call
                self.n_iter_ = dev.fit_batches(permutation, batch_size, self.alpha, self.learning_rate, self.n_iter_,
                                               self.random_state)
        if dev.plan is not None:         # (a dictionary-update launch whose workgroups could not meet must not pass for a fit)
            check(lib.modl_recsys_plan_status(dev.plan, stream_ptr(dev.device)), 'modl_recsys_plan_status')
        self._refit()
        return self

    def _callback(self):
        if self.callback is not None:
            self.callback(self)

    def _single_batch_fit(self, X, batch):
        """recsys.py:147-165"""
        if self.verbose and self.verbose_iter_ and self.n_iter_ >= self.verbose_iter_[0]:
            print('Iteration %i' % self.n_iter_)
            self.verbose_iter_ = self.verbose_iter_[1:]
            self._callback()
        batch_size = batch.shape[0]
        self.n_iter_ += batch_size
        w = batch_weight(self.n_iter_, batch_size, self.learning_rate, 0)
        order = self.random_state.permutation(self.n_components)     # recsys.py:196 (drawn for every batch)
        self._dev.batch_update(batch, self.alpha, w, self.n_iter_, order)

    def _refit(self):
        """recsys.py:254-265: ridge codes of every row with the current dictionary"""
        self._dev.codes(None, self.alpha)

    def _finish(self, out, row_bias, indptr, indices):
        """raw products at a pattern -> predictions: the row bias, col_mean_ and the crop (recsys.py:236-244)"""
        if self.detrend:
            out += np.repeat(row_bias, np.diff(indptr))
            out += self.col_mean_.take(indices, mode='clip')
        if self.crop is not None:
            out[out > self.crop[1]] = self.crop[1]
            out[out < self.crop[0]] = self.crop[0]
        return out

    def predict(self, X):
        """recsys.py:215-245"""
        if not sp.issparse(X):
            X = sp.csr_matrix(X)
        X = check_array(X, accept_sparse='csr')
        out = self._finish(self._dev.predict(X), self.row_mean_ if self.detrend else None, X.indptr, X.indices)
        return sp.csr_matrix((out, X.indices, X.indptr), shape=X.shape)

    def _fold_in(self, X):
        """(X as CSR of the fitted dtype, device codes (rows, k), row bias or None) of the rows of a ratings matrix X, which
        need not be training rows: centred as fit centres (col_mean_ at the rated items, and the row bias
        (sum_f (x_f - col_mean_[f]) + beta global_mean_) / (n_u + beta), the first pass of compute_biases for a row on its
        own), then coded on their ratings by the kernel _refit uses."""
        dev = self._dev
        if not sp.issparse(X):
            X = sp.csr_matrix(X)
        X = check_array(X, accept_sparse='csr', dtype=[np.float32, np.float64], copy=True)
        if X.shape[1] != dev.p:
            raise ValueError('RecsysDictFact: X has %d columns, the fitted dictionary %d' % (X.shape[1], dev.p))
        row_bias = None
        if self.detrend:
            data = X.data.astype(np.float64) - self.col_mean_.take(X.indices, mode='clip')
            n_u = np.diff(X.indptr)
            sums = np.bincount(np.repeat(np.arange(X.shape[0]), n_u), weights=data, minlength=X.shape[0])
            den = n_u + float(self.beta)
            row_bias = np.where(den > 0, (sums + self.beta * self.global_mean_) / np.where(den > 0, den, 1), 0.0)
            data -= np.repeat(row_bias, n_u)
            X = sp.csr_matrix((data, X.indices, X.indptr), shape=X.shape)
        X = sp.csr_matrix((X.data.astype(dev.dtype), X.indices, X.indptr), shape=X.shape)
        return X, dev.codes_of(X, self.alpha), row_bias

    def transform(self, X):
        """Ridge codes (rows of X, n_components) of the rows of a ratings matrix X under the fitted dictionary: what fit
        computes for its own rows (recsys.py:176-181), for any rows.  Rows without ratings get a zero code."""
        return self._fold_in(X)[1].cpu().numpy()

    def recommend(self, X=None, n_items=10, users=None, exclude_seen=True, rows_per_call=None):
        """The n_items items with the highest predicted rating per user: (items int64 (users, n_items), -1 where a user has
        fewer candidates; scores float64, NaN there).

        X=None: the training users (all, or the row ids `users`); their seen items are the training ratings.  X given: one new
        user per row of X, coded on their ratings (transform); their seen items are the entries of X.  exclude_seen=False
        ranks every item.  The ranking is by the uncropped prediction (equal ones by ascending item id); the scores are what
        predict gives at the returned loci.  Users go through the kernel rows_per_call at a time (default: as many as keep
        its workspace under 256 MB)."""
        n_items = int(n_items)
        if n_items < 1 or n_items > MAX_TOPN:
            raise ValueError('RecsysDictFact.recommend: n_items = %d, but a call returns between 1 and %d items per user '
                             '(MODL_RECSYS_MAX_TOPN)' % (n_items, MAX_TOPN))
        dev = self._dev
        d = dev.device
        if X is None:
            if users is None:
                rows, code, ex_rows = np.arange(dev.n), dev.code, None
            else:
                rows = np.ascontiguousarray(users, dtype=np.int64).ravel()
                if rows.size and (rows.min() < 0 or rows.max() >= dev.n):
                    raise ValueError('RecsysDictFact.recommend: users must be row ids of the training matrix')
                ex_rows = torch.from_numpy(rows).to(d)
                code = dev.code.index_select(0, ex_rows)
            row_bias = self.row_mean_[rows] if self.detrend else None
            ex_indptr, ex_indices = dev.indptr, dev.indices
        else:
            if users is not None:
                raise ValueError('RecsysDictFact.recommend: `users` selects training rows; with X every row is a user')
            X, code, row_bias = self._fold_in(X)
            ex_rows = None
            ex_indptr, ex_indices = _csr_piece(X.indptr, np.int32, d), _csr_piece(X.indices, np.int32, d)
        if not exclude_seen:
            ex_indptr = ex_indices = ex_rows = None
        bias = torch.from_numpy(np.ascontiguousarray(self.col_mean_, dtype=np.float64)).to(d) if self.detrend else None
        nq = code.shape[0]
        items = dev.topn(code, ex_indptr, ex_indices, ex_rows, bias, n_items, rows_per_call).cpu().numpy().astype(np.int64)
        # the scores: predict's own kernel and arithmetic at the returned loci (the lists end in -1: the pattern is their head)
        valid = items >= 0
        indptr = np.concatenate([[0], np.cumsum(valid.sum(axis=1))]).astype(np.int64)
        indices = items[valid].astype(np.int32)
        pattern = sp.csr_matrix((np.zeros(len(indices)), indices, indptr), shape=(nq, dev.p))
        out = self._finish(dev.predict(pattern, code), row_bias, indptr, indices)
        scores = np.full(items.shape, np.nan)
        scores[valid] = out
        return items, scores

    def _ranks(self, n_rows, t_indptr, t_indices, X, exclude_seen, rows_per_call, what):
        """(ranks, n_candidates) of _RecsysDevice.ranks for the target pattern t_indptr / t_indices over n_rows users: the
        training users (X None) or the rows of X, folded in; the queries, exclusions and item bias are those of recommend"""
        dev = self._dev
        if X is None:
            if n_rows != dev.n:
                raise ValueError('RecsysDictFact.%s: X_test has %d rows, the training matrix %d (row u is training user u; '
                                 'pass X= for other users)' % (what, n_rows, dev.n))
            code, ex_indptr, ex_indices = dev.code, dev.indptr, dev.indices
        else:
            X, code, _ = self._fold_in(X)
            if n_rows != X.shape[0]:
                raise ValueError('RecsysDictFact.%s: X_test has %d rows, X %d' % (what, n_rows, X.shape[0]))
            d = dev.device
            ex_indptr, ex_indices = _csr_piece(X.indptr, np.int32, d), _csr_piece(X.indices, np.int32, d)
        if not exclude_seen:
            ex_indptr = ex_indices = None
        bias = torch.from_numpy(np.ascontiguousarray(self.col_mean_, dtype=np.float64)).to(dev.device) if self.detrend else None
        return dev.ranks(code, ex_indptr, ex_indices, None, bias, t_indptr, t_indices, rows_per_call)

    def _test_pattern(self, X_test, what):
        if not sp.issparse(X_test):
            X_test = sp.csr_matrix(X_test)
        X_test = X_test.tocsr()
        if X_test.shape[1] != self._dev.p:
            raise ValueError('RecsysDictFact.%s: X_test has %d columns, the fitted dictionary %d'
                             % (what, X_test.shape[1], self._dev.p))
        return X_test

    def ranks(self, X_test, X=None, exclude_seen=True, rows_per_call=None):
        """The rank of every entry of X_test among the items its user has not seen: an int64 array aligned with the entries of
        X_test in CSR order.  Rank r means that r unseen items other than the entry's own are predicted above it (equal
        predictions by ascending item id): with r < N the item is recommend(n_items=N)'s column r for that user, otherwise
        it is not in that list.  The ranking is recommend's: by the uncropped prediction, formed with the same arithmetic.

        X=None: row u of X_test belongs to training user u, whose seen items are the training ratings.  X given: one new user
        per row of X and of X_test, coded on X's ratings (transform); the seen items are the entries of X.
        exclude_seen=False ranks among all items.  An entry that is itself a seen item is ranked as if it were not."""
        X_test = self._test_pattern(X_test, 'ranks')
        r, _ = self._ranks(X_test.shape[0], X_test.indptr, X_test.indices, X, exclude_seen, rows_per_call, 'ranks')
        return r.astype(np.int64)

    def ranking_score(self, X_test, n_items=10, X=None, min_rating=None, exclude_seen=True):
        """Ranking quality of recommend(n_items=n_items) on held-out ratings: a RankingScore (hit_rate, precision, recall,
        ndcg, mrr, auc: means over the users with targets; n_users, n_targets), see ranking_metrics.  The targets are the
        entries of X_test, with min_rating those rated min_rating or higher (the others stay ordinary unseen candidates).
        X as in ranks."""
        X_test = self._test_pattern(X_test, 'ranking_score')
        indptr, indices = X_test.indptr, X_test.indices
        if min_rating is not None:
            keep = X_test.data >= min_rating
            indptr = np.concatenate([[0], np.cumsum(keep)])[X_test.indptr]
            indices = indices[keep]
        r, n_cand = self._ranks(X_test.shape[0], indptr, indices, X, exclude_seen, None, 'ranking_score')
        return ranking_metrics(r, indptr, n_cand, n_items)

    def score(self, X):
        """Root mean squared error of the prediction at the loci of X (recsys.py:247-252)"""
        if not sp.issparse(X):
            X = sp.csr_matrix(X)
        X = check_array(X, accept_sparse='csr')
        return rmse(X, self.predict(X))
