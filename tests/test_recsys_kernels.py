"""The ratings path (csrc/recsys.hip) entry point by entry point, through the C ABI, against a per-minibatch CPU reference.

Three layers, as tests/test_dict_update_routes.py:

0. The reference is oracle/wrappers_oracle.py: `recsys_minibatch` (one minibatch on an explicit RecsysState) and
   `recsys_solve_row`, the inner loop of `recsys_fit` - which calls them, so tests/test_recsys.py::test_oracle_recsys_golden
   keeps pinning them to the golden recorded from the reference implementation.  It runs in float64; for f32 cases also in
   float32 on the same float32 inputs (conftest.assert_within_f32_noise).
1. CPU tests: `make_ratings` builds CSR ratings from NAMED ROW KINDS ('n<N>': N ratings; 'ends': rates item 0 and item
   p - 1; 'unsorted': column indices not ascending; 'shared': rows that rate the same six items), `make_state` a starting
   state with non-zero B_, C_, codes and budgets and a feature_n_iter seeded so that w_B is clamped for some touched items and
   not for others.  `test_cases_are_what_they_claim` checks that; `test_route_table` that the matrices of layer 2 hold every
   route and both neighbours of every boundary of `codes_route` / `expected_route`;
   `test_acceptance_rule_rejects_mutants` that the rules of layer 2 (`judge`) reject nine wrong versions of the reference
   (`MUTANTS` / `mutated_minibatch`, kept here: the oracle stays a plain transcription) in both dtypes.
2. GPU tests: direct calls of modl_recsys_codes_*, modl_recsys_update_B_*, modl_recsys_predict_*, modl_gram_axpby_*,
   modl_recsys_minibatch_* and modl_recsys_fit_batches_*.  Every minibatch asserts the route it took from the delta of
   modl_recsys_plan_counts.

Acceptance (`judge`): feature_n_iter exact; rows of code_ that the call does not solve (rows outside the batch, rows without
ratings), and the rows of Bt / Dt of items the batch does not touch, bit-identical to the input; what is computed - f64:
rel_fro < 1e-9 (comp_norm: rtol 1e-9 / atol 1e-12, the l2 rule of test_dict_update_routes.py), f32:
assert_within_f32_noise(got, reference in f32, reference in f64).

`codes_route` restates csrc/recsys.hip: recsys_codes lines 517-543 (RPL from k :521, the LDS formula :522-523, the f64 fall-back
:525-528, MODL_EINVAL :529); `expected_route` restates recsys_launch lines 723-742 (k <= kRfWide :241, b <= kRfMaxBatch and the
chunk count against kRfMaxChunks :198 / :733-734, MODL_DEBUG_RECSYS_FUSED :560, KP :757-758) and the separate launches behind
it (:791-793).  The same table is in DESIGN.md, section 10b "Ratings-path route matrix".
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import wrappers_oracle as wo

from .conftest import assert_within_f32_noise, rel_fro

DT = {'f32': np.float32, 'f64': np.float64}
EINVAL, ENOMEM = -1, -2
ALPHA = 0.1
LDS_BYTES = 160 * 1024
CHUNK, MAX_CHUNKS, MAX_BATCH_FUSED = 128, 64, 64
WIDE = {'f32': 64, 'f64': 56}


def _cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------- the dispatch, restated
def codes_route(dt, k):
    """recsys_codes: the variant of recsys_code_kernel a k-atom system takes, or 'EINVAL'"""
    tsz = 4 if dt == 'f32' else 8
    rpl = 1 if k <= 64 else 2 if k <= 128 else 0

    def lds(r):
        extra = ((k + 3) & ~3) + 3 * r * 4 * 64 if r else 0
        return tsz * (k * ((k | 1) if r else k) + k + 32 * k + 32 + extra) + 32 * 4 + 16
    use = rpl
    if rpl and lds(rpl) > LDS_BYTES:
        use = 0
    if lds(use) > LDS_BYTES:
        return 'EINVAL'
    return 'RPL%d' % use


def expected_route(dt, k, b, row_lengths, fused_switch=1):
    """recsys_launch: 'fused/KP<registers>' (one launch for codes and C_) or 'split/<codes_route>' / 'EINVAL'"""
    if k <= WIDE[dt] and b <= MAX_BATCH_FUSED and fused_switch:
        if sum(_cdiv(int(n), CHUNK) for n in row_lengths) <= MAX_CHUNKS:
            return 'fused/KP%d' % (32 if k <= 32 else WIDE[dt])
    r = codes_route(dt, k)
    return r if r == 'EINVAL' else 'split/' + r


# ---------------------------------------------------------------------------------------------------- layer 1: the builders
SHARED_ITEMS = 6
# one row of every length at which a kernel changes its path: the 32-rating sub-chunks and 128-rating chunks of both code kernels,
# and more than 1024 ratings (nine chunks: the eight-at-a-time record sum of recsys_fused_kernel)
FULL = ('n0', 'n1', 'n31', 'n32', 'n33', 'n127', 'n128', 'n129', 'n256', 'n257', 'n1100', 'ends', 'unsorted', 'shared', 'shared',
        'shared')
LIGHT = ('n0', 'n1', 'n31', 'n32', 'n33', 'n127', 'n128', 'n129', 'ends', 'unsorted', 'shared', 'shared', 'shared')   # 13 rows, 13 chunks


def make_ratings(kinds, p, dt, seed):
    """CSR ratings (scipy, int32 indices, NOT sorted where a kind says so), one row per entry of `kinds`"""
    rs = np.random.RandomState(seed)
    shared = rs.choice(p, SHARED_ITEMS, replace=False)
    others = np.setdiff1d(np.arange(p), shared)
    cols = []
    for kind in kinds:
        if kind[0] == 'n':
            c = np.sort(rs.choice(p, int(kind[1:]), replace=False))
        elif kind == 'ends':
            c = np.sort(np.concatenate([[0, p - 1], 1 + rs.choice(p - 2, 5, replace=False)]))
        elif kind == 'unsorted':
            c = np.sort(rs.choice(p, 40, replace=False))[::-1].copy()
            c[[3, 20]] = c[[20, 3]]
        elif kind == 'shared':
            c = np.sort(np.concatenate([shared, rs.choice(others, 14, replace=False)]))
        else:
            raise ValueError(kind)
        cols.append(c.astype(np.int32))
    indptr = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int32)
    indices = np.concatenate(cols).astype(np.int32)
    data = rs.randn(len(indices)).astype(dt)
    X = sp.csr_matrix((data, indices, indptr), shape=(len(kinds), p))
    assert np.array_equal(X.indices, indices) and X.indices.dtype == np.int32      # (scipy left the order alone)
    return X


def as_f64(X):
    return sp.csr_matrix((X.data.astype(np.float64), X.indices, X.indptr), shape=X.shape)


def lengths(X, rows=None):
    n = np.diff(X.indptr)
    return n if rows is None else n[np.asarray(rows)]


def make_state(X, k, dt, seed, n_iter_scale):
    """A starting state that is not trivial, built in f64 and then rounded to dt:

    - random unit atoms and random codes, then ONE reference minibatch over all rows, so that B_, C_ and the codes have the
      algorithm's own scales;
    - a ridge of mean(diag C_) on C_.  C_ of one minibatch has the rank of its rows, and the atom sweep amplifies the rounding
      of the codes, B_ and C_ by up to cond(C_).  With the ridge cond(C_) <= 1 + k; test_cases_are_what_they_claim holds it
      below 50, so that D can be held to the same rules as the codes;
    - a large budget left (comp_norm) for every other atom.  Those atoms stay inside their ball; an atom that ends ON its ball
      has used its budget up to the last bit, and its comp_norm would be rounding noise only;
    - feature_n_iter seeded around n_iter_scale = w n_iter, so that w_B is clamped for some items and not for others."""
    n, p = X.shape
    rs = np.random.RandomState(seed)
    D = rs.randn(k, p)
    D /= np.linalg.norm(D, axis=1, keepdims=True)
    st = wo.RecsysState(D, 0.1 * rs.randn(n, k), np.zeros((k, k)), np.zeros((k, p)), np.zeros(k), np.zeros(p, dtype=np.int64))
    wo.recsys_minibatch(st, as_f64(X), ALPHA, rs.permutation(n), 1.0, n, rs.permutation(k))
    st.C += np.mean(np.diag(st.C)) * np.eye(k)
    st.comp_norm = np.abs(st.comp_norm) + np.where(np.arange(k) % 2 == 0, 30.0 * (1 + rs.rand(k)), 0.0)
    st.feature_n_iter = rs.randint(0, int(2 * n_iter_scale) + 2, size=p).astype(np.int64)
    return st.copy(dt)


W = 0.35


def make_minibatch(dt, k, kinds, p, seed):
    """(X, start state, batch = every row once with the ids NOT ascending, w, n_iter, order) in dtype dt"""
    X = make_ratings(kinds, p, DT[dt], seed)
    n = X.shape[0]
    rs = np.random.RandomState(seed + 1)
    batch = rs.permutation(n).astype(np.int64)
    sh = [i for i in batch if kinds[i] == 'shared']
    if sh == sorted(sh):
        batch = batch[::-1].copy()                              # (the rows that share items: batch order is not row-id order)
    n_iter = 2 * n
    st = make_state(X, k, DT[dt], seed + 2, W * n_iter)
    return X, st, batch, W, n_iter, rs.permutation(k).astype(np.int64)


# Deliberately WRONG versions of the reference, one name each: what `judge` must reject
MUTANTS = ('row_id_order', 'w_B_not_clamped', 'ridge_mean_S', 'C_over_rated_rows', 'empty_row_zeroed', 'last_of_129_dropped',
           'last_chunk_dropped', 'n_iter_once_per_item', 'code_to_batch_position')


def mutated_minibatch(st, X, alpha, batch, w, n_iter, order, mutant):
    """wo.recsys_minibatch with ONE thing wrong.  The first half (wo.recsys_batch_statistics / recsys_solve_row) is restated
    with a fork per mutant; mutant=None is the oracle bit for bit (test_acceptance_rule_rejects_mutants asserts it).  The
    dictionary update behind it is the oracle's own."""
    assert mutant is None or mutant in MUTANTS, mutant
    D, code, Cm, B, fni = st.D, st.code, st.C, st.B, st.feature_n_iter
    k, p = D.shape
    batch = np.asarray(batch)
    lens = X.indptr[batch + 1] - X.indptr[batch]
    walk = list(enumerate(batch))
    if mutant == 'row_id_order':
        walk = sorted(walk, key=lambda t: t[1])
    bumped = set()
    for pos, i in walk:
        s, e = X.indptr[i], X.indptr[i + 1]
        nnz = e - s
        if nnz == 0:
            if mutant == 'empty_row_zeroed':
                code[i] = 0
            continue
        sub, xs = X.indices[s:e], X.data[s:e]
        keep = nnz
        if mutant == 'last_of_129_dropped' and nnz == 129:
            keep = 128
        if mutant == 'last_chunk_dropped' and nnz > 128:
            keep = 128 * ((nnz - 1) // 128)
        Ds = D[:, sub[:keep]]
        G = Ds.dot(Ds.T)
        G.flat[::k + 1] += alpha / (p / (float(np.mean(lens)) if mutant == 'ridge_mean_S' else len(sub)))
        c = np.linalg.solve(G, Ds.dot(xs[:keep]))
        if mutant == 'n_iter_once_per_item':
            fresh = np.array([f not in bumped for f in sub])
            fni[sub[fresh]] += 1
            bumped.update(sub.tolist())
        else:
            fni[sub] += 1
        code[pos if mutant == 'code_to_batch_position' else i] = c
        w_B = w * n_iter / fni[sub]
        if mutant != 'w_B_not_clamped':
            w_B = np.minimum(1, w_B)
        B[:, sub] *= 1 - w_B
        B[:, sub] += np.outer(c.astype(B.dtype), xs * w_B)
    Cm *= 1 - w
    Cm += w / (max(int(np.sum(lens != 0)), 1) if mutant == 'C_over_rated_rows' else len(batch)) * code[batch].T.dot(code[batch])
    return wo.recsys_batch_dictionary(st, X, batch, order)


def reference(X, st, steps, dt, mutant=None, restated=False):
    """the reference in dtype dt on the dt-valued inputs: `steps` = [(batch, w, n_iter, order)] applied to a copy of st
    (with a mutant, or restated=True: by mutated_minibatch)"""
    out = st.copy(dt)
    Xd = sp.csr_matrix((X.data.astype(dt), X.indices, X.indptr), shape=X.shape)
    for batch, w, n_iter, order in steps:
        if mutant is None and not restated:
            wo.recsys_minibatch(out, Xd, ALPHA, batch, w, n_iter, order)
        else:
            mutated_minibatch(out, Xd, ALPHA, batch, w, n_iter, order, mutant)
    return out


def references(dt, X, st, steps):
    refs = {'f64': reference(X, st, steps, np.float64)}
    if dt == 'f32':
        refs['f32'] = reference(X, st, steps, np.float32)
    return refs


def group_by_item(X, batch):
    """the batch's ratings grouped by item as recsys_prepare (csrc/recsys.hip :642-693) builds them: the touched items ascending,
    and per item its entries IN BATCH ORDER: (subset, fptr, entry_sample = position in the batch, entry_val)"""
    pos = np.concatenate([np.full(int(X.indptr[i + 1] - X.indptr[i]), q, dtype=np.int32) for q, i in enumerate(batch)])
    items = np.concatenate([X.indices[X.indptr[i]:X.indptr[i + 1]] for i in batch])
    vals = np.concatenate([X.data[X.indptr[i]:X.indptr[i + 1]] for i in batch])
    o = np.argsort(items, kind='stable')
    subset, counts = np.unique(items, return_counts=True)
    fptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return subset.astype(np.int32), fptr, pos[o], vals[o]


# ---------------------------------------------------------------------------------------------------- the acceptance rules
def assert_close(dt, got, ref64, ref32, what):
    if dt == 'f64':
        err = rel_fro(got, ref64)
        print('%s: rel_fro %.3e' % (what, err))
        assert err < 1e-9, (what, err)
    else:
        print('%s: err %.3e noise %.3e' % (what, rel_fro(got, ref64), rel_fro(ref32, ref64)))
        assert_within_f32_noise(got, ref32, ref64, what)


def judge(dt, got, start, refs, X, solved_rows, touched):
    """The rules of layer 2 for a state `got` reached from `start`: solved_rows = the rows of code_ the calls solve (rows of the
    batches that have ratings), touched = the items the batches rate."""
    r64, r32 = refs['f64'], refs.get('f32')
    n, p = X.shape
    solved_rows = np.unique(np.asarray(solved_rows, dtype=np.int64))
    touched = np.unique(np.asarray(touched, dtype=np.int64))
    kept_rows = np.setdiff1d(np.arange(n), solved_rows)
    kept_items = np.setdiff1d(np.arange(p), touched)
    np.testing.assert_array_equal(got.feature_n_iter, r64.feature_n_iter, err_msg='feature_n_iter')
    np.testing.assert_array_equal(got.code[kept_rows], start.code[kept_rows], err_msg='a row of code_ that is not solved changed')
    np.testing.assert_array_equal(got.B[:, kept_items], start.B[:, kept_items], err_msg='B_ of an untouched item changed')
    np.testing.assert_array_equal(got.D[:, kept_items], start.D[:, kept_items], err_msg='D of an untouched item changed')

    def part(s, name):
        a = getattr(s, name)
        return a[solved_rows] if name == 'code' else a[:, touched] if name in ('B', 'D') else a
    for name in ('code', 'C', 'B', 'D'):
        if part(r64, name).size == 0:
            continue
        assert_close(dt, part(got, name), part(r64, name), None if r32 is None else part(r32, name), name)
    if touched.size == 0:
        np.testing.assert_array_equal(got.comp_norm, start.comp_norm)
    elif dt == 'f64':
        # (budgets left sit at rounding level when the ball is hit: absolute, the l2 rule of test_dict_update_routes.py)
        np.testing.assert_allclose(got.comp_norm, r64.comp_norm, rtol=1e-9, atol=1e-12)
    else:
        assert_within_f32_noise(got.comp_norm, r32.comp_norm, r64.comp_norm, 'comp_norm')


def accepts(*args):
    try:
        judge(*args)
    except AssertionError:
        return False
    return True


def batch_facts(X, batch):
    ln = lengths(X, batch)
    solved = np.asarray(batch)[ln > 0]
    touched = np.unique(np.concatenate([X.indices[X.indptr[i]:X.indptr[i + 1]] for i in batch])) if ln.sum() else np.zeros(0, int)
    return solved, touched


# ---------------------------------------------------------------------------------------------------- layer 2: the matrices
CODES_K = {'f32': (1, 64, 65, 128, 129, 186), 'f64': (1, 64, 65, 121, 122, 127)}
CODES_REFUSED = {'f32': 187, 'f64': 128}
CODES_CASES = [(dt, k) for dt in ('f32', 'f64') for k in CODES_K[dt]]
P_FULL = 1200


def _fill(kinds, rows, kind):
    return tuple(kinds) + (kind,) * (rows - len(kinds))


# 64 / 65 rows with 62 / 63 chunks (the row limit alone decides), 64 / 65 chunks in 35 / 36 rows (the chunk limit alone decides)
ROWS64 = _fill(LIGHT + ('n0', 'n0'), 64, 'n3')
ROWS65 = _fill(LIGHT + ('n0', 'n0'), 65, 'n3')
CHUNKS64 = FULL + ('n129',) * 18 + ('n5',)
CHUNKS65 = FULL + ('n129',) * 18 + ('n5', 'n5')

MB_CASES = []


def _mb(dt, k, kinds=FULL, p=P_FULL, fused=1, tag='full'):
    MB_CASES.append(SimpleNamespace(dt=dt, k=k, kinds=kinds, p=p, fused=fused, tag=tag))


for _dt in ('f32', 'f64'):
    for _k in (1, 16, 17, 32, 33, 48, 49, 56, 57, 64, 65):      # the 16 x 16 tile counts, KP 32 / wide, the widest fused k
        _mb(_dt, _k)
    for _k in {'f32': (128, 129), 'f64': (121, 122)}[_dt]:      # the separate launches with recsys_code_kernel<T, 2> / <T, 0>
        _mb(_dt, _k)
    for _k in (1, 33, 64):                                      # the switch off: the separate launches for what would be fused
        _mb(_dt, _k, fused=0)
    _mb(_dt, 20, ROWS64, 600, tag='rows64')
    _mb(_dt, 20, ROWS65, 600, tag='rows65')
    _mb(_dt, 20, CHUNKS64, P_FULL, tag='chunks64')
    _mb(_dt, 20, CHUNKS65, P_FULL, tag='chunks65')


def kind_lengths(kinds):
    return [int(q[1:]) if q[0] == 'n' else {'ends': 7, 'unsorted': 40, 'shared': 20}[q] for q in kinds]


def mb_route(c):
    return expected_route(c.dt, c.k, len(c.kinds), kind_lengths(c.kinds), c.fused)


def mb_id(c):
    return '%s-k%d-%s-sw%d-%s' % (c.dt, c.k, c.tag, c.fused, mb_route(c).replace('/', '_'))


def mb_seed(c):
    return 100 * c.k + len(c.kinds) + (7 if c.dt == 'f32' else 0)


# ---------------------------------------------------------------------------------------------------- layer 1: CPU tests
def test_lds_table():
    """the boundaries the LDS formula gives, as DESIGN.md and include/modl_hip.h state them; modl_amd.recsys.MAX_COMPONENTS is the
    last k that is not refused"""
    def span(dt, route):
        ks = [k for k in range(1, 260) if codes_route(dt, k) == route]
        return (ks[0], ks[-1]) if ks else None
    assert [span('f32', r) for r in ('RPL1', 'RPL2', 'RPL0')] == [(1, 64), (65, 128), (129, 186)]
    assert [span('f64', r) for r in ('RPL1', 'RPL2', 'RPL0')] == [(1, 64), (65, 121), (122, 127)]
    assert all(codes_route('f32', k) == 'EINVAL' for k in range(187, 4097))
    assert all(codes_route('f64', k) == 'EINVAL' for k in range(128, 4097))
    assert CODES_REFUSED == {dt: CODES_K[dt][-1] + 1 for dt in DT}


def test_route_table():
    for dt in ('f32', 'f64'):
        ks = set(k for d, k in CODES_CASES if d == dt)
        assert {codes_route(dt, k) for k in ks} == {'RPL1', 'RPL2', 'RPL0'}
        # both neighbours of every boundary of recsys_codes, and the refusal behind the last
        bounds = {'f32': (64, 128, 186), 'f64': (64, 121, 127)}[dt]
        for kb in bounds:
            assert kb in ks and (kb + 1 in ks or kb + 1 == CODES_REFUSED[dt]), (dt, kb)
            assert codes_route(dt, kb) != codes_route(dt, kb + 1)
        assert 1 in ks and codes_route(dt, CODES_REFUSED[dt]) == 'EINVAL'
        cases = [c for c in MB_CASES if c.dt == dt]
        routes = {mb_route(c) for c in cases}
        want = {'fused/KP32', 'fused/KP%d' % WIDE[dt], 'split/RPL1', 'split/RPL2', 'split/RPL0'}
        assert routes == want, (dt, routes)
        on = set(c.k for c in cases if c.fused == 1 and c.tag == 'full')
        assert 1 in on
        for kb in (16, 32, 48, 64):                          # every multiple of 16 and its successor (the 16 x 16 tile counts)
            assert kb in on and kb + 1 in on, (dt, kb)
        by = {(c.k, c.fused, c.tag): mb_route(c) for c in cases}
        assert by[(32, 1, 'full')] == 'fused/KP32' and by[(33, 1, 'full')] == 'fused/KP%d' % WIDE[dt]
        wide = WIDE[dt]
        assert by[(wide, 1, 'full')].startswith('fused') and by[(wide + 1, 1, 'full')].startswith('split')
        assert by[(64, 1, 'full')] == ('fused/KP64' if dt == 'f32' else 'split/RPL1') and by[(65, 1, 'full')] == 'split/RPL2'
        kb = {'f32': 128, 'f64': 121}[dt]
        assert by[(kb, 1, 'full')] == 'split/RPL2' and by[(kb + 1, 1, 'full')] == 'split/RPL0'
        for k in (1, 33, 64):
            assert by[(k, 0, 'full')] == 'split/RPL1'        # (the switch alone decides: fused with it on, f64 64 apart)
        # the row limit and the chunk limit, each decided by itself
        facts = {c.tag: (len(c.kinds), sum(_cdiv(n, CHUNK) for n in kind_lengths(c.kinds)), mb_route(c)) for c in cases}
        assert facts['rows64'] == (64, 62, 'fused/KP32') and facts['rows65'] == (65, 63, 'split/RPL1')
        assert facts['chunks64'] == (35, 64, 'fused/KP32') and facts['chunks65'] == (36, 65, 'split/RPL1')
    assert len(set(mb_id(c) for c in MB_CASES)) == len(MB_CASES)


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_cases_are_what_they_claim(dt):
    X, st, batch, w, n_iter, order = make_minibatch(dt, 20, FULL, P_FULL, 5)
    n, p = X.shape
    assert 300 <= p <= 3000 and n <= 80 and X.nnz < 6000
    ln = lengths(X)
    assert list(ln) == kind_lengths(FULL)
    for want in (0, 1, 31, 32, 33, 127, 128, 129, 256, 257):
        assert want in ln
    assert ln.max() > 1024 and _cdiv(int(ln.max()), CHUNK) >= 9
    row = lambda i: X.indices[X.indptr[i]:X.indptr[i + 1]]
    ends = row(FULL.index('ends'))
    assert 0 in ends and p - 1 in ends
    assert np.any(np.diff(row(FULL.index('unsorted'))) < 0)
    sh = [i for i, q in enumerate(FULL) if q == 'shared']
    common = set(row(sh[0])) & set(row(sh[1])) & set(row(sh[2]))
    assert len(sh) >= 3 and len(common) >= SHARED_ITEMS
    in_batch = [i for i in batch if i in sh]
    assert sorted(batch) == list(range(n)) and in_batch != sorted(in_batch)            # batch order is not row-id order
    # w_B = min(1, w n_iter / n_f) with n_f counted up per entry: clamped for some touched items, not for others
    touched = batch_facts(X, batch)[1]
    ratio = w * n_iter / (st.feature_n_iter[touched] + 1)
    assert np.sum(ratio > 1) > 20 and np.sum(ratio < 1) > 20
    assert np.all(st.B != 0) or np.mean(st.B != 0) > 0.5
    assert np.all(st.code[FULL.index('n0')] != 0) and np.all(np.diag(st.C) > 0) and np.any(st.comp_norm > 1)
    assert st.D.dtype == DT[dt] and X.data.dtype == DT[dt]
    for k in (20, 64, CODES_K[dt][-2]):
        assert np.linalg.cond(make_state(X, k, np.float64, 3, 1.0).C) < 50, k
    # the ridge systems are well conditioned: the worst row is the one with a single rating (cond ~ 1 + |d|^2 p / alpha)
    for k in (1, 20, CODES_K[dt][-1]):
        D = np.random.RandomState(k).randn(k, p)
        D /= np.linalg.norm(D, axis=1, keepdims=True)
        worst = 0.0
        for i in range(n):
            if ln[i]:
                Ds = D[:, row(i)]
                G = Ds.dot(Ds.T) + ALPHA * ln[i] / p * np.eye(k)
                worst = max(worst, np.linalg.cond(G))
        assert worst < 1e4, (k, worst)


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_acceptance_rule_rejects_mutants(dt):
    """every wrong version of the reference is rejected by `judge` on the inputs of the matrix; the reference itself passes, and
    the restatement that carries the mutants is the oracle bit for bit when nothing is wrong in it"""
    X, st, batch, w, n_iter, order = make_minibatch(dt, 20, FULL, P_FULL, 5)
    steps = [(batch, w, n_iter, order)]
    refs = references(dt, X, st, steps)
    solved, touched = batch_facts(X, batch)
    assert accepts(dt, refs[dt], st, refs, X, solved, touched)
    same_bits(reference(X, st, steps, DT[dt], restated=True), refs[dt])
    assert len(MUTANTS) == 9
    survivors = [m for m in MUTANTS
                 if accepts(dt, reference(X, st, steps, DT[dt], mutant=m), st, refs, X, solved, touched)]
    assert not survivors, survivors


def test_estimator_names_the_limit():
    """RecsysDictFact.fit refuses an n_components beyond what modl_recsys_codes_* takes, with the limit in the message, before
    anything is allocated on a device (this test has none)"""
    from modl_amd import recsys
    assert recsys.MAX_COMPONENTS == {np.dtype(DT[dt]): CODES_K[dt][-1] for dt in DT}
    rs = np.random.RandomState(0)
    X = sp.random(12, 30, density=0.3, random_state=rs, format='csr')
    for dt in ('f32', 'f64'):
        est = recsys.RecsysDictFact(n_components=CODES_REFUSED[dt])
        with pytest.raises(ValueError, match='at most %d components' % CODES_K[dt][-1]):
            est.fit(X.astype(DT[dt]))
        assert not hasattr(est, '_dev')


# ---------------------------------------------------------------------------------------------------- layer 2: GPU tests
@pytest.fixture(scope='module')
def gpu():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    return torch


@pytest.fixture
def fused_switch():
    """sets MODL_DEBUG_RECSYS_FUSED; the default is back when the test ends, however it ends"""
    from modl_amd import _lib

    def put(v):
        _lib.check(_lib.lib.modl_debug_set(_lib.DEBUG_RECSYS_FUSED, int(v)), 'modl_debug_set')
    try:
        yield put
    finally:
        put(1)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to('cuda')


def _hp(a):
    return a.ctypes.data_as(C.c_void_p)


class Plan:
    """the CSR matrix and a state on the device, and a modl_recsys_plan on them"""

    def __init__(self, X, st, dt, max_batch, max_entries=None):
        from modl_amd._lib import lib, check
        from modl_amd.device import dtype_id
        self.lib, self.dt, self.k, (self.n, self.p) = lib, dt, st.D.shape[0], X.shape
        self.h_indptr = np.ascontiguousarray(X.indptr, dtype=np.int32)
        self.h_indices = np.ascontiguousarray(X.indices, dtype=np.int32)
        self.h_data = np.ascontiguousarray(X.data, dtype=DT[dt])
        self.indptr, self.indices, self.data = _dev(self.h_indptr), _dev(self.h_indices), _dev(self.h_data)
        self.load(st)
        if max_entries is None:
            max_entries = int(np.sort(np.diff(self.h_indptr))[::-1][:max_batch].sum())
        self.plan = C.c_void_p()
        check(lib.modl_recsys_plan_create(dtype_id(DT[dt]), self.p, self.k, max_batch, max_entries, C.byref(self.plan)),
              'modl_recsys_plan_create')

    def load(self, st):
        assert st.D.dtype == DT[self.dt]
        self.Dt, self.Bt, self.C, self.code = _dev(st.D.T), _dev(st.B.T), _dev(st.C), _dev(st.code)
        self.cn, self.fni = _dev(st.comp_norm), _dev(st.feature_n_iter.astype(np.int64))

    def state_args(self):
        from modl_amd.device import ptr
        return [ptr(t) for t in (self.Dt, self.Bt, self.C, self.code, self.cn, self.fni)]

    def csr_args(self, h_indices=None):
        from modl_amd.device import ptr
        return [_hp(self.h_indptr), _hp(self.h_indices if h_indices is None else h_indices), _hp(self.h_data), self.n,
                ptr(self.indptr), ptr(self.indices), ptr(self.data)]

    def minibatch(self, batch, w, n_iter, order, h_indices=None):
        batch = np.ascontiguousarray(batch, dtype=np.int64)
        order = np.ascontiguousarray(order, dtype=np.int64)
        f = getattr(self.lib, 'modl_recsys_minibatch_' + self.dt)
        return f(self.plan, *self.csr_args(h_indices), _hp(batch), len(batch), _hp(order), ALPHA, float(w), float(n_iter),
                 *self.state_args(), None)

    def counts(self):
        a, b = C.c_int64(0), C.c_int64(0)
        assert self.lib.modl_recsys_plan_counts(self.plan, C.byref(a), C.byref(b)) == 0
        return int(a.value), int(b.value)

    def state(self):
        import torch
        torch.cuda.synchronize()
        assert self.lib.modl_recsys_plan_status(self.plan, None) == 0
        h = lambda t: t.cpu().numpy()
        return wo.RecsysState(h(self.Dt).T.copy(), h(self.code), h(self.C), h(self.Bt).T.copy(), h(self.cn), h(self.fni))

    def close(self):
        if self.plan:
            self.lib.modl_recsys_plan_destroy(self.plan)
            self.plan = None


def same_bits(a, b, names=('D', 'code', 'C', 'B', 'comp_norm', 'feature_n_iter')):
    for name in names:
        np.testing.assert_array_equal(getattr(a, name), getattr(b, name), err_msg=name)


def count_delta(plan, before):
    after = plan.counts()
    return after[0] - before[0], after[1] - before[1]


# ---- modl_recsys_codes_*
@pytest.mark.gpu
@pytest.mark.parametrize('dt,k', CODES_CASES, ids=['%s-k%d-%s' % (dt, k, codes_route(dt, k)) for dt, k in CODES_CASES])
def test_codes(gpu, dt, k):
    from modl_amd._lib import lib
    from modl_amd.device import ptr
    X = make_ratings(FULL, P_FULL, DT[dt], 11 + k)
    n, p = X.shape
    rs = np.random.RandomState(k)
    D = rs.randn(k, p)
    D = (D / np.linalg.norm(D, axis=1, keepdims=True)).astype(DT[dt])
    code0 = rs.randn(n + 7, k).astype(DT[dt])
    X64, D64 = as_f64(X), D.astype(np.float64)
    ln = lengths(X)
    sol64 = {i: wo.recsys_solve_row(X64, D64, i, ALPHA)[0] for i in range(n) if ln[i]}
    sol32 = {i: wo.recsys_solve_row(X, D, i, ALPHA)[0] for i in range(n) if ln[i]} if dt == 'f32' else None
    Dt, indptr, indices, data = _dev(D.T), _dev(X.indptr), _dev(X.indices), _dev(X.data)
    empty = FULL.index('n0')
    subset = np.array([i for i in rs.permutation(n) if i == empty or rs.rand() < 0.8], dtype=np.int64)   # permuted, not all rows
    assert empty in subset and 3 < len(subset) < n and np.any(np.diff(subset) < 0)
    f = getattr(lib, 'modl_recsys_codes_' + dt)
    for ids in (None, subset):
        for remap in (False, True):
            src = np.arange(n, dtype=np.int64) if ids is None else ids
            dst = (src + 3) % (n + 7) if remap else src          # (injective, and no row lands on itself)
            code = _dev(code0)
            d_ids, d_dst = (None if ids is None else _dev(ids)), (_dev(dst) if remap else None)
            rc = f(ptr(Dt), p, k, ptr(indptr), ptr(indices), ptr(data), ptr(d_ids), ptr(d_dst), len(src), ALPHA, ptr(code), None)
            gpu.cuda.synchronize()
            assert rc == 0, rc
            got = code.cpu().numpy()
            rated = ln[src] > 0
            written = dst[rated]
            kept = np.setdiff1d(np.arange(n + 7), written)
            np.testing.assert_array_equal(got[kept], code0[kept], err_msg='a row that is not addressed, or has no ratings, changed')
            r64 = np.stack([sol64[i] for i in src[rated]])
            r32 = np.stack([sol32[i] for i in src[rated]]) if dt == 'f32' else None
            assert_close(dt, got[written], r64, r32, 'codes ids=%s remap=%s' % (ids is not None, remap))


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_codes_refuses_what_does_not_fit_lds(gpu, dt):
    """one atom beyond modl_amd.recsys.MAX_COMPONENTS is MODL_EINVAL and nothing is written (the last k that fits: test_codes)"""
    from modl_amd import recsys
    from modl_amd._lib import lib
    from modl_amd.device import ptr
    k = recsys.MAX_COMPONENTS[np.dtype(DT[dt])] + 1
    assert k == CODES_REFUSED[dt]
    X = make_ratings(LIGHT, 300, DT[dt], 3)
    rs = np.random.RandomState(0)
    D = rs.randn(k, 300).astype(DT[dt])
    code0 = rs.randn(X.shape[0], k).astype(DT[dt])
    code = _dev(code0)
    Dt, indptr, indices, data = _dev(D.T), _dev(X.indptr), _dev(X.indices), _dev(X.data)
    rc = getattr(lib, 'modl_recsys_codes_' + dt)(ptr(Dt), 300, k, ptr(indptr), ptr(indices), ptr(data), None, None, X.shape[0],
                                                 ALPHA, ptr(code), None)
    gpu.cuda.synchronize()
    assert rc == EINVAL
    np.testing.assert_array_equal(code.cpu().numpy(), code0)


# ---- modl_recsys_update_B_*
def update_B_reference(B0, fni0, subset, fptr, es, ev, code_b, w_n_iter, dt):
    """recsys_update_B_kernel (csrc/recsys.hip :153-168) in double with a rounding to T after each of its two steps.
    Returns (B, feature_n_iter, bound): bound[i] = n_e * 2 ulp_T(M_i), n_e the entries of item i and M_i the largest magnitude
    among the intermediates of its row.  Derivation: per entry the kernel computes b1 = T(b (1 - wB)) and b2 = T(b1 + c xw), each
    in double and rounded to T once.  Where the compiler contracts the multiply-add of the second step, its double result
    differs from the uncontracted one by at most the rounding of c xw: half an ulp of double at |c xw| <= M, which (T = double)
    is at most one ulp_T(M) after the final rounding, or (T = float) can at most move the rounding to T to the neighbouring
    float: one ulp_T(M).  A difference d that exists before an entry leaves it as at most d |1 - wB| + one rounding
    <= d + ulp_T(M), since 0 <= 1 - wB <= 1.  So every entry adds at most 2 ulp_T(M), and n_e entries n_e * 2 ulp_T(M)."""
    T = DT[dt]
    B, fni = B0.copy(), fni0.copy()
    bound = np.zeros(len(subset))
    for i, f in enumerate(subset):
        row = B[:, f].astype(np.float64)
        M = np.max(np.abs(row))
        for e in range(fptr[i], fptr[i + 1]):
            fni[f] += 1
            wB = min(w_n_iter / float(fni[f]), 1.0)
            xw = float(ev[e]) * wB
            b1 = (row * (1.0 - wB)).astype(T).astype(np.float64)
            add = code_b[es[e]].astype(np.float64) * xw
            row = (b1 + add).astype(T).astype(np.float64)
            M = max(M, np.max(np.abs(b1)), np.max(np.abs(add)), np.max(np.abs(row)))
        B[:, f] = row.astype(T)
        bound[i] = (fptr[i + 1] - fptr[i]) * 2 * float(np.spacing(T(M)))
    return B, fni, bound


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'f64'])
@pytest.mark.parametrize('k', [1, 63, 64, 65, 130])
def test_update_B(gpu, dt, k):
    from modl_amd._lib import lib
    from modl_amd.device import ptr
    p = 300
    for seed in range(20):                                       # (the first seed whose touched items are no multiple of 4)
        X = make_ratings(LIGHT, p, DT[dt], 40 + seed)
        batch = np.random.RandomState(seed).permutation(X.shape[0])
        subset, fptr, es, ev = group_by_item(X, batch)
        if len(subset) % 4:
            break
    u = len(subset)
    assert u % 4 != 0 and np.max(np.diff(fptr)) >= 3
    rs = np.random.RandomState(k)
    B0 = rs.randn(k, p).astype(DT[dt])
    code_b = rs.randn(len(batch), k).astype(DT[dt])
    w_n_iter = 7.3
    fni0 = rs.randint(0, 15, size=p).astype(np.int64)
    Bt, fni = _dev(B0.T), _dev(fni0)
    d = [_dev(a) for a in (subset, fptr, es, ev, code_b)]
    rc = getattr(lib, 'modl_recsys_update_B_' + dt)(ptr(Bt), k, ptr(fni), *[ptr(a) for a in d], w_n_iter, u, None)
    gpu.cuda.synchronize()
    assert rc == 0
    got, got_n = Bt.cpu().numpy().T, fni.cpu().numpy()
    ref, ref_n, bound = update_B_reference(B0, fni0, subset, fptr, es, ev, code_b, w_n_iter, dt)
    np.testing.assert_array_equal(got_n, ref_n)
    kept = np.setdiff1d(np.arange(p), subset)
    np.testing.assert_array_equal(got[:, kept], B0[:, kept])
    diff = np.max(np.abs(got[:, subset].astype(np.float64) - ref[:, subset].astype(np.float64)), axis=0)
    print('largest difference / bound: %.3g' % np.max(diff / bound))
    assert np.all(diff <= bound), (np.max(diff / bound), int(np.argmax(diff / bound)))


# ---- modl_recsys_predict_*
@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'f64'])
@pytest.mark.parametrize('k', [1, 50, 130])
def test_predict(gpu, dt, k):
    from modl_amd._lib import lib
    from modl_amd.device import ptr
    p = 300
    Xp = make_ratings(('n0', 'n1', 'n64', 'n65', 'n200', 'unsorted', 'n0'), p, DT[dt], 77)    # (not the pattern of any training matrix)
    n = Xp.shape[0]
    assert n % 4 != 0
    rs = np.random.RandomState(k + 1)
    code, D = rs.randn(n, k).astype(DT[dt]), rs.randn(k, p).astype(DT[dt])
    import torch
    out = torch.full((Xp.nnz,), np.nan, dtype=torch.float64, device='cuda')
    d_code, Dt, ind, iptr = _dev(code), _dev(D.T), _dev(Xp.indices), _dev(Xp.indptr)
    rc = getattr(lib, 'modl_recsys_predict_' + dt)(ptr(out), ptr(ind), ptr(iptr), ptr(d_code), n, k, ptr(Dt), None)
    gpu.cuda.synchronize()
    assert rc == 0
    got = out.cpu().numpy()
    rows = np.repeat(np.arange(n), np.diff(Xp.indptr))
    terms = code.astype(np.float64)[rows] * D.astype(np.float64).T[Xp.indices]          # [nnz][k], the T-valued operands
    ref = np.array([np.sum(t) for t in terms])
    # the kernel accumulates k products in double: |error| <= k 2^-53 sum |terms| (one rule for both dtypes)
    bound = k * 2.0 ** -53 * np.sum(np.abs(terms), axis=1)
    assert np.all(np.abs(got - ref) <= bound), np.max(np.abs(got - ref) / bound)


# ---- modl_gram_axpby_*
@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'f64'])
@pytest.mark.parametrize('b', [0, 1, 5, 64, 200])
@pytest.mark.parametrize('k', [1, 33, 64, 130])
def test_gram_axpby(gpu, dt, k, b):
    from modl_amd._lib import lib
    from modl_amd.device import ptr
    T = DT[dt]
    rs = np.random.RandomState(1000 * k + b)
    rows = rs.randn(max(b, 1), k).astype(T)[:b]
    C0 = rs.randn(k, k).astype(T)                               # not symmetric: a transposed store would show
    beta, alpha = T(0.65), T(0.35 / max(b, 1))
    Cd, R = _dev(C0), _dev(rs.randn(1, k).astype(T) if b == 0 else rows)
    rc = getattr(lib, 'modl_gram_axpby_' + dt)(ptr(R), b, k, ptr(Cd), float(beta), float(alpha), None)
    gpu.cuda.synchronize()
    assert rc == 0
    got = Cd.cpu().numpy()
    r64 = float(beta) * C0.astype(np.float64) + float(alpha) * rows.astype(np.float64).T.dot(rows.astype(np.float64))
    r32 = (beta * C0 + alpha * rows.T.dot(rows)).astype(T) if dt == 'f32' else None
    assert_close(dt, got, r64, r32, 'C')


# ---- modl_recsys_minibatch_*
@pytest.mark.gpu
@pytest.mark.parametrize('c', MB_CASES, ids=mb_id)
def test_minibatch(gpu, fused_switch, c):
    X, st, batch, w, n_iter, order = make_minibatch(c.dt, c.k, c.kinds, c.p, mb_seed(c))
    assert list(lengths(X)) == kind_lengths(c.kinds)
    refs = references(c.dt, X, st, [(batch, w, n_iter, order)])
    fused_switch(c.fused)
    plan = Plan(X, st, c.dt, len(batch))
    try:
        before = plan.counts()
        rc = plan.minibatch(batch, w, n_iter, order)
        assert rc == 0, rc
        got = plan.state()
        route = expected_route(c.dt, c.k, len(batch), lengths(X, batch), c.fused)
        assert count_delta(plan, before) == ((1, 0) if route.startswith('fused') else (0, 1)), route
    finally:
        plan.close()
    judge(c.dt, got, st, refs, X, *batch_facts(X, batch))


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'f64'])
@pytest.mark.parametrize('fused', [1, 0])
def test_minibatch_of_rows_without_ratings(gpu, fused_switch, dt, fused):
    """nothing to solve and no item touched: only C_ moves, by the codes the rows already have"""
    kinds = LIGHT + ('n0', 'n0')
    X = make_ratings(kinds, 300, DT[dt], 8)
    st = make_state(X, 20, DT[dt], 9, 10.0)
    batch = np.array([i for i, q in enumerate(kinds) if q == 'n0'][::-1], dtype=np.int64)
    order = np.random.RandomState(0).permutation(20)
    refs = references(dt, X, st, [(batch, W, 50, order)])
    for key in ('f64',) + (('f32',) if dt == 'f32' else ()):
        T = DT[key]
        cb = st.code[batch].astype(T)
        formula = (T(1 - W) * st.C.astype(T) + T(W / len(batch)) * cb.T.dot(cb))
        assert rel_fro(refs[key].C, formula) < (1e-12 if key == 'f64' else 1e-5)
    fused_switch(fused)
    plan = Plan(X, st, dt, len(batch))
    try:
        before = plan.counts()
        assert plan.minibatch(batch, W, 50, order) == 0
        got = plan.state()
        assert count_delta(plan, before) == ((1, 0) if fused else (0, 1))
    finally:
        plan.close()
    same_bits(got, st, ('D', 'B', 'feature_n_iter', 'code', 'comp_norm'))
    judge(dt, got, st, refs, X, [], [])


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_multi_chunk_minibatch_is_reproducible(gpu, dt):
    """the header's fixed-order sums: the same minibatch with rows of several chunks, twice from the same state: the same bits"""
    X, st, batch, w, n_iter, order = make_minibatch(dt, 33, FULL, P_FULL, 21)
    assert expected_route(dt, 33, len(batch), lengths(X, batch)).startswith('fused')
    runs = []
    plan = Plan(X, st, dt, len(batch))
    try:
        for _ in range(2):
            plan.load(st)
            assert plan.minibatch(batch, w, n_iter, order) == 0
            runs.append(plan.state())
        assert plan.counts() == (2, 0)
    finally:
        plan.close()
    same_bits(runs[0], runs[1], ('code', 'C'))


RING_KINDS = _fill(LIGHT + ('n257', 'n129', 'n129'), 80, 'n7')


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_twenty_minibatches_back_to_back(gpu, dt):
    """twenty minibatches enqueued on one plan with no synchronisation in between: the eight staging slots are reused twice over,
    the host waits on the acknowledgement word, the tickets are reset by every launch"""
    k, b = 20, 4
    X = make_ratings(RING_KINDS, 600, DT[dt], 31)
    st = make_state(X, k, DT[dt], 32, 12.0)
    rs = np.random.RandomState(33)
    perm = rs.permutation(X.shape[0])
    steps = []
    for t in range(20):
        n_iter = 40 + b * (t + 1)
        steps.append((perm[b * t:b * (t + 1)].astype(np.int64), (b / n_iter) ** 0.5, n_iter, rs.permutation(k).astype(np.int64)))
    assert sum(_cdiv(int(n), CHUNK) > 1 for n in lengths(X, perm[:80])) >= 3
    refs = references(dt, X, st, steps)
    plan = Plan(X, st, dt, b)
    try:
        for batch, w, n_iter, order in steps:
            assert plan.minibatch(batch, w, n_iter, order) == 0
        got = plan.state()
        assert plan.counts() == (20, 0)
    finally:
        plan.close()
    judge(dt, got, st, refs, X, *batch_facts(X, perm[:80]))


MIXED_KINDS = (_fill(LIGHT, 26, 'n7') + _fill(LIGHT, 26, 'n9') + ('n257',) * 13 + ('n129',) * 13 + ('n40', 'n129'))


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_fit_batches_mixing_routes_equals_single_calls(gpu, dt):
    """modl_recsys_fit_batches_* over fused, fused, split (65 chunks), fused: the same bits as one modl_recsys_minibatch_* call per
    minibatch - with the next minibatch's staged arrays riding on a fused launch, the staging launch of its own after the split
    minibatch, and the staging buffers flipped in between"""
    from modl_amd._lib import lib, check
    from modl_amd.device import ptr
    from modl_amd.randomkit import batch_weight
    k, bs, lr = 20, 26, 0.9
    X = make_ratings(MIXED_KINDS, P_FULL, DT[dt], 51)
    n = X.shape[0]
    rows = np.arange(n, dtype=np.int64)
    rows[:26] = rows[:26][::-1]
    cuts = [rows[i:i + bs] for i in range(0, n, bs)]
    routes = [expected_route(dt, k, len(q), lengths(X, q)).split('/')[0] for q in cuts]
    assert routes == ['fused', 'fused', 'split', 'fused'] and len(cuts[-1]) == 2
    assert sum(_cdiv(int(v), CHUNK) for v in lengths(X, cuts[2])) == 65
    st = make_state(X, k, DT[dt], 52, 20.0)
    seed_state = np.random.RandomState(5).get_state()
    # one call per minibatch, the draws of the Python loop (modl_amd/recsys.py: _single_batch_fit)
    rng = np.random.RandomState(5)
    single = Plan(X, st, dt, bs)
    try:
        n_iter = 0
        for q in cuts:
            n_iter += len(q)
            assert single.minibatch(q, batch_weight(n_iter, len(q), lr, 0), n_iter, rng.permutation(k)) == 0
        want = single.state()
        assert single.counts() == (3, 1)
    finally:
        single.close()
    run = Plan(X, st, dt, bs)
    rk = C.c_void_p()
    check(lib.modl_rk_create(0, C.byref(rk)), 'modl_rk_create')
    try:
        key = np.ascontiguousarray(seed_state[1], dtype=np.uint32)
        check(lib.modl_rk_set_mt_state(rk, _hp(key), int(seed_state[2])), 'modl_rk_set_mt_state')
        n_it, done = C.c_int64(0), C.c_int64(0)
        rc = getattr(lib, 'modl_recsys_fit_batches_' + dt)(run.plan, *run.csr_args(), _hp(rows), n, bs, rk, ALPHA, lr, C.byref(n_it),
                                                           *run.state_args(), None, C.byref(done))
        assert rc == 0 and done.value == 4 and n_it.value == n
        got = run.state()
        assert run.counts() == (3, 1)
    finally:
        run.close()
        lib.modl_rk_destroy(rk)
    same_bits(got, want)
    assert not np.array_equal(got.D, st.D)


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_minibatch_refusals_leave_the_plan_usable(gpu, dt):
    """every refusal is made on the host, before any device work: the state keeps its bits, and the NEXT minibatch on the same plan
    is right (the per-item counters of the grouping were cleared).  MODL_ENOMEM needs a plan of its own, with room for 100
    ratings: the valid minibatch after it is a smaller one, judged against a reference of its own."""
    k = 20
    X = make_ratings(LIGHT, 300, DT[dt], 61)
    n, p = X.shape
    st = make_state(X, k, DT[dt], 62, 8.0)
    rs = np.random.RandomState(63)
    order = rs.permutation(k).astype(np.int64)
    sh = [i for i, q in enumerate(LIGHT) if q == 'shared']
    good = np.array([sh[2], LIGHT.index('n129'), sh[0], LIGHT.index('n0'), sh[1], LIGHT.index('ends')], dtype=np.int64)
    small = np.array([sh[2], LIGHT.index('n0'), sh[0], LIGHT.index('ends')], dtype=np.int64)
    assert lengths(X, small).sum() <= 100 < lengths(X, good).sum()
    refs = {id(q): references(dt, X, st, [(q, W, 30, order)]) for q in (good, small)}
    bad_col = X.indices.copy()
    bad_col[X.indptr[sh[1] + 1] - 1] = p                         # the LAST rating of the batch below: its items are counted by then
    bad_order = order.copy()
    bad_order[5] = k
    refusals = [('b > max_batch', dict(batch=np.arange(9)), EINVAL),
                ('row id out of range', dict(batch=np.array([sh[0], n])), EINVAL),
                ('negative row id', dict(batch=np.array([sh[0], -1])), EINVAL),
                ('order entry out of range', dict(batch=good, order=bad_order), EINVAL),
                ('column index >= p', dict(batch=np.array([sh[0], sh[2], sh[1]]), h_indices=bad_col), EINVAL)]
    for max_entries, valid, cases in ((None, good, refusals),
                                      (100, small, [('more ratings than max_entries', dict(batch=good), ENOMEM)])):
        plan = Plan(X, st, dt, 8, max_entries)
        try:
            for what, kw, want in cases:
                before = plan.counts()
                rc = plan.minibatch(kw['batch'], W, 30, kw.get('order', order), kw.get('h_indices'))
                assert rc == want, (what, rc)
                assert plan.counts() == before, what
                same_bits(plan.state(), st)
                assert plan.minibatch(valid, W, 30, order) == 0, what
                assert count_delta(plan, before) == (1, 0), what
                judge(dt, plan.state(), st, refs[id(valid)], X, *batch_facts(X, valid))
                plan.load(st)
        finally:
            plan.close()
