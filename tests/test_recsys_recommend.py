"""Recommendation on the ratings path: modl_recsys_topn_* (csrc/recsys_topn.hip) through the C ABI, and
RecsysDictFact.transform / recommend through the estimator.  Structured as tests/test_recsys_kernels.py:

0. The reference is `topn_reference` below: float64 numpy, a stable sort by (-score, item) after masking.
1. CPU tests: `make_case` builds a call from NAMED QUERY KINDS ('none': no ratings and a zero code; 'all': rated everything;
   'short': exactly n_top - 1 items left; 'unsorted': exclusion row not ascending, with repeats; 'ends': items 0 and p - 1 are
   the best; 'run': n_top + 3 exactly tied best items from item 120 on, across the item-tile boundary at 128; 'n<N>': N random
   ratings).  `test_cases_are_what_they_claim` checks that, `test_judge_rejects_mutants` that `judge` rejects ten wrong versions
   of the reference in both dtypes, `test_route_table` the restated dispatch (`topn_route`) and workspace against the library.
2. GPU tests through the ABI and through the estimator.

Acceptance (`judge`), per query, with E = 2 k u_T max_f sum_c |code_c Dt[f][c]| (u = 2^-24 / 2^-53: the dot-product bound for any
summation order, once for each side; the rule of modl_recsys_predict_*), plus u_T |bias_f| in f32 for the rounding
of the item bias to T:
  - no returned item is excluded, out of range or repeated;
  - every returned score is within E of the reference score of that item;
  - the returned scores do not increase, equal returned scores come in ascending item order;
  - every item neither returned nor excluded has a reference score <= the last returned reference score + 2 E;
  - the number of -1 entries is exactly max(0, n_top - candidates), they are the tail, their scores are -inf.
Exact cases (kind='int': codes, dictionary and biases are integers of magnitude <= 8, every partial sum is exact in f32): E = 0
and the lists must EQUAL the reference, ties included.

`topn_route` restates csrc/recsys_topn.hip: topn_slabs (the user tile of 32 queries, the item tile IT = 128 (f32) / 64 (f64),
slabs of whole item tiles, at least 256 items, at most 64 slabs, about 512 workgroups), `topn_workspace` restates topn_ws and
`topn_lds` the LDS formula.  The same table is in DESIGN.md, section 14.
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import wrappers_oracle as wo

from .conftest import assert_within_f32_noise, rel_fro

DT = {'f32': np.float32, 'f64': np.float64}
U = {'f32': 2.0 ** -24, 'f64': 2.0 ** -53}
EINVAL, ENOMEM, ENOGPU = -1, -2, -4
MAX_TOPN = 128
KMAX = {'f32': 186, 'f64': 127}
USERS, MIN_SLAB, MAX_SLABS, TARGET_WGS, MERGE_MIN, KC = 32, 256, 64, 512, 32, 64
ITEM_TILE = {'f32': 128, 'f64': 64}
LDS_BYTES = 160 * 1024


def _cdiv(a, b):
    return -(-a // b)


def _up(x, a):
    return _cdiv(x, a) * a


# ---------------------------------------------------------------------------------------------------- the dispatch, restated
def topn_route(dt, p, b):
    """topn_slabs: (slabs, items per slab) of a call with b queries over p items"""
    it = ITEM_TILE[dt]
    want = min(max(TARGET_WGS // _cdiv(b, USERS), 1), MAX_SLABS)
    nst = _cdiv(p, it)
    sps = max(_cdiv(nst, want), MIN_SLAB // it)
    return _cdiv(nst, sps), sps * it


def topn_workspace(dt, p, k, b, n_top):
    """topn_ws: the bitmask of p bits per query, and with more than one slab a list per query and slab"""
    if not (b >= 1 and 1 <= p < 2 ** 31 and 1 <= n_top <= MAX_TOPN and 1 <= k <= KMAX[dt]):
        return 0
    S = topn_route(dt, p, b)[0]
    lists = b * S * n_top if S > 1 else 0
    return _up(4 * b * _cdiv(p, 32), 256) + _up((4 if dt == 'f32' else 8) * lists, 256) + _up(4 * lists, 256)


def topn_lds(dt, k, n_top):
    """topn_lds: the dynamic LDS of recsys_topn_kernel"""
    tsz, tk, it = (4, 2, 128) if dt == 'f32' else (8, 4, 64)
    kp = _up(k, tk)
    cb = it + MERGE_MIN
    o = tsz * (USERS * (kp | 1) + it * (min(kp, KC) | 1) + USERS * n_top + USERS * cb)
    o = _up(o, 8) + 8 * it + 4 * (USERS * n_top + USERS * cb + USERS + USERS * (it // 32))
    return _up(o, 16)


# ---------------------------------------------------------------------------------------------------- the builders
RUN_AT = 120
KINDS = ('none', 'all', 'short', 'unsorted', 'ends', 'run', 'n5', 'n40')


def make_case(dt, kind, k, p, b, n_top, seed, ex=True, ex_rows=True, code_rows=True, bias=True):
    """One call.  kind='rand': normal codes, dictionary and biases; kind='int': integers of magnitude <= 8.  Query ii is of
    kind KINDS[ex_row(ii) % 8]: its exclusion row and its code are built for that kind (where p is too small for a kind the
    row is a plain random one).  ex_rows / code_rows: a permutation of the exclusion rows / of the rows of a code array with
    three more rows than queries."""
    rs = np.random.RandomState(seed)
    T = DT[dt]
    draw = (lambda *s: rs.randn(*s)) if kind == 'rand' else (lambda *s: rs.randint(-8, 9, size=s).astype(np.float64))
    Dt = draw(p, k)
    code = draw(b, k)
    item_bias = draw(p) if bias else None
    ex_perm = rs.permutation(b).astype(np.int64) if (ex and ex_rows) else None
    row_of = ex_perm if ex_perm is not None else np.arange(b)
    kinds = [None] * b                                             # by query
    for ii in range(b):
        kinds[ii] = KINDS[row_of[ii] % len(KINDS)]
    can_run = p >= RUN_AT + n_top + 3 + 2
    best = lambda ii: 8.0 * np.where(code[ii] >= 0, 1.0, -1.0) if kind == 'int' else 4.0 * np.sign(code[ii]) * (1 + np.abs(code[ii]))
    done_ends = done_run = False
    for ii in range(b):
        if kinds[ii] == 'none':
            code[ii] = 0
        elif kinds[ii] == 'ends' and p >= 3 and not done_ends and k >= 2:
            Dt[0] = Dt[p - 1] = best(ii)
            if bias:
                item_bias[0] = item_bias[p - 1] = np.max(item_bias) + 1
            done_ends = True
        elif kinds[ii] == 'run' and can_run and not done_run and k >= 2:
            Dt[RUN_AT:RUN_AT + n_top + 3] = best(ii)
            if bias:
                item_bias[RUN_AT:RUN_AT + n_top + 3] = np.max(item_bias)
            done_run = True
    rows = []
    for r in range(b):                                             # by exclusion row
        kd = KINDS[r % len(KINDS)]
        if kd == 'none' or not ex:
            c = np.zeros(0, dtype=np.int64)
        elif kd == 'all':
            c = rs.permutation(p)
        elif kd == 'short' and p >= n_top:
            c = rs.permutation(p)[:p - (n_top - 1)]
        elif kd == 'unsorted' and p >= 8:
            c = np.sort(rs.choice(p, min(40, p // 2), replace=False))[::-1].copy()
            c = np.concatenate([c, c[:3], c[-1:]])                  # repeats
        elif kd in ('ends', 'run'):
            c = 1 + rs.choice(max(p - 2, 1), min(5, max(p - 2, 1)), replace=False) if p >= 3 else np.zeros(0, dtype=np.int64)
            c = c[(c < RUN_AT) | (c >= RUN_AT + n_top + 3)]         # (neither the ends nor the run)
        else:
            c = np.sort(rs.choice(p, min(int(kd[1:]) if kd[0] == 'n' else 7, p), replace=False))
        rows.append(np.asarray(c, dtype=np.int32))
    indptr = np.concatenate([[0], np.cumsum([len(c) for c in rows])]).astype(np.int32)
    indices = (np.concatenate(rows) if indptr[-1] else np.zeros(1)).astype(np.int32)    # (never an empty buffer: a NULL pointer is refused)
    code_perm = None
    code_arr = code
    if code_rows:
        code_perm = rs.permutation(b + 3)[:b].astype(np.int64)
        code_arr = draw(b + 3, k)
        code_arr[code_perm] = code
    return SimpleNamespace(dt=dt, kind=kind, k=k, p=p, b=b, n_top=n_top, Dt=np.ascontiguousarray(Dt.astype(T)),
                           code=np.ascontiguousarray(code_arr.astype(T)), code_rows=code_perm,
                           indptr=indptr if ex else None, indices=indices if ex else None, ex_rows=ex_perm,
                           item_bias=item_bias, kinds=kinds)


def query_codes(c):
    return c.code if c.code_rows is None else c.code[c.code_rows]


def exclusions(c, identity_rows=False, drop_last=False):
    """per query, the excluded items (None: no exclusion)"""
    if c.indptr is None:
        return None
    out = []
    for ii in range(c.b):
        r = ii if (c.ex_rows is None or identity_rows) else c.ex_rows[ii]
        e = c.indices[c.indptr[r]:c.indptr[r + 1]]
        out.append(e[:-1] if drop_last else e)
    return out


def all_scores(code, Dt, item_bias):
    s = code.astype(np.float64).dot(Dt.astype(np.float64).T)
    return s if item_bias is None else s + item_bias[None, :]


def topn_reference(code, Dt, excl, item_bias, n_top, mutant=None):
    """(items int64 (b, n_top), scores float64): per query the n_top best items that are not excluded, by descending score,
    equal scores by ascending item; the tail -1 / -inf.  `mutant`: one thing wrong (MUTANTS)."""
    b, p = code.shape[0], Dt.shape[0]
    S = all_scores(code, Dt, None if mutant == 'no_bias' else item_bias)
    items = np.full((b, n_top), -1, dtype=np.int64)
    scores = np.full((b, n_top), -np.inf)
    ids = np.arange(p)
    for ii in range(b):
        ok = np.ones(p, dtype=bool)
        if excl is not None and mutant != 'no_exclusion':
            ok[excl[ii]] = False
        if mutant == 'never_last':
            ok[p - 1] = False
        if mutant == 'never_first':
            ok[0] = False
        s = S[ii]
        if mutant == 'ascending':
            order = np.lexsort((ids, s))
        elif mutant == 'ties_larger_id':
            order = np.lexsort((-ids, -s))
        else:
            order = np.lexsort((ids, -s))                           # stable: by -score, then by item
        order = order[ok[order]]
        if mutant == 'slabs_not_merged':
            order = np.concatenate([o[:n_top] for o in (order[(order >= a) & (order < a + 256)] for a in range(0, p, 256))])
        take = order[:n_top]
        items[ii, :len(take)] = take
        scores[ii, :len(take)] = s[take]
        if mutant == 'tail_item_0':
            items[ii, len(take):] = 0
    return items, scores


MUTANTS = ('no_exclusion', 'last_excluded_dropped', 'ties_larger_id', 'never_last', 'never_first', 'ascending', 'no_bias',
           'ex_rows_ignored', 'tail_item_0', 'slabs_not_merged')


def case_reference(c, mutant=None):
    excl = exclusions(c, identity_rows=mutant == 'ex_rows_ignored', drop_last=mutant == 'last_excluded_dropped')
    m = mutant if mutant not in ('ex_rows_ignored', 'last_excluded_dropped') else None
    items, scores = topn_reference(query_codes(c), c.Dt, excl, c.item_bias, c.n_top, m)
    return items, scores.astype(DT[c.dt]).astype(np.float64) if c.kind == 'int' else scores


# ---------------------------------------------------------------------------------------------------- the acceptance rule
def judge(c, items, scores):
    """the rules of the module docstring for the lists (items, scores) a call on case c returned"""
    code, p, n_top = query_codes(c), c.p, c.n_top
    items = np.asarray(items).astype(np.int64)
    scores = np.asarray(scores).astype(np.float64)
    assert items.shape == (c.b, n_top) and scores.shape == (c.b, n_top)
    ref = all_scores(code, c.Dt, c.item_bias)
    absdot = np.abs(code.astype(np.float64)).dot(np.abs(c.Dt.astype(np.float64)).T)
    E = (0.0 if c.kind == 'int' else 2.0 * c.k * U[c.dt]) * np.max(absdot, axis=1)[:, None] * np.ones((1, p))
    if c.dt == 'f32' and c.item_bias is not None and c.kind != 'int':
        E = E + U['f32'] * np.abs(c.item_bias)[None, :]
    excl = exclusions(c)
    worst = 0.0
    for ii in range(c.b):
        ok = np.ones(p, dtype=bool)
        if excl is not None:
            ok[excl[ii]] = False
        cand = int(ok.sum())
        it, sc = items[ii], scores[ii]
        n_ret = min(cand, n_top)
        assert np.all(it[n_ret:] == -1) and np.all(it[:n_ret] != -1), ('the -1 entries are not exactly the tail', ii, cand)
        assert np.all(np.isneginf(sc[n_ret:])), ('a tail score is not -inf', ii)
        got = it[:n_ret]
        assert np.all((got >= 0) & (got < p)), ('item out of range', ii)
        assert len(np.unique(got)) == n_ret, ('item repeated', ii)
        assert np.all(ok[got]), ('excluded item returned', ii)
        err = np.abs(sc[:n_ret] - ref[ii, got])
        assert np.all(err <= E[ii, got]), ('score off', ii, float(np.max(err - E[ii, got])))
        if n_ret:
            worst = max(worst, float(np.max(err / np.maximum(E[ii, got], 1e-300))) if c.kind != 'int' else 0.0)
        d = np.diff(sc[:n_ret])
        assert np.all(d <= 0), ('scores increase', ii)
        assert np.all(np.diff(got)[d == 0] > 0), ('equal scores not in ascending item order', ii)
        if n_ret:
            rest = ok.copy()
            rest[got] = False
            lim = ref[ii, got[-1]] + E[ii, got[-1]] + E[ii]
            assert np.all(ref[ii][rest] <= lim[rest]), ('a better item was left out', ii)
    if c.kind == 'int':
        r_items, r_scores = case_reference(c)
        np.testing.assert_array_equal(items, r_items, err_msg='exact case: the lists differ from the reference')
        np.testing.assert_array_equal(scores, r_scores, err_msg='exact case: the scores differ from the reference')
    return worst


def accepts(c, items, scores):
    try:
        judge(c, items, scores)
    except AssertionError:
        return False
    return True


# the CPU case matrix: b = 16 queries = every kind twice, p = 700 items (three slabs of 256), every optional argument given
def cpu_cases(dt):
    return [make_case(dt, 'rand', 7, 700, 16, 10, 3), make_case(dt, 'int', 7, 700, 16, 10, 4),
            make_case(dt, 'int', 7, 700, 16, 10, 5, bias=False)]


# ---------------------------------------------------------------------------------------------------- layer 1: CPU tests
@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_judge_rejects_mutants(dt):
    """`judge` accepts the reference on every case of the matrix and rejects each wrong version of it on at least one (every
    one except 'no_bias' on the first already: the third case has no bias to ignore)"""
    cases = cpu_cases(dt)
    for c in cases:
        assert accepts(c, *case_reference(c))
    assert len(MUTANTS) == 10
    for c in cases[:2]:
        survivors = [m for m in MUTANTS if accepts(c, *case_reference(c, m))]
        assert not survivors, (c.kind, survivors)
    survivors = [m for m in MUTANTS if m != 'no_bias' and accepts(cases[2], *case_reference(cases[2], m))]
    assert not survivors, survivors


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_cases_are_what_they_claim(dt):
    for c in cpu_cases(dt):
        code, p, n_top = query_codes(c), c.p, c.n_top
        excl = exclusions(c)
        assert set(c.kinds) == set(KINDS) and c.ex_rows is not None and np.any(c.ex_rows != np.arange(c.b))
        assert c.code_rows is not None and c.code.shape[0] == c.b + 3
        S = all_scores(code, c.Dt, c.item_bias)
        ref_items, _ = case_reference(c)
        assert p % ITEM_TILE[dt] != 0 and topn_route(dt, p, c.b)[0] >= 3
        for ii, kd in enumerate(c.kinds):
            left = p - len(np.unique(excl[ii]))
            if kd == 'none':
                assert len(excl[ii]) == 0 and not np.any(code[ii])
                if c.item_bias is None:
                    assert np.all(S[ii] == S[ii, 0])                # all scores equal: the first n_top items in id order
                    assert list(ref_items[ii]) == list(range(n_top))
            if kd == 'all':
                assert left == 0 and np.all(ref_items[ii] == -1)
            if kd == 'short':
                assert left == n_top - 1 and ref_items[ii, -1] == -1 and ref_items[ii, -2] >= 0
            if kd == 'unsorted':
                e = excl[ii]
                assert np.any(np.diff(e) < 0) and len(np.unique(e)) < len(e)
        ends = [ii for ii, kd in enumerate(c.kinds) if kd == 'ends']
        assert any(sorted(ref_items[ii, :2]) == [0, p - 1] for ii in ends)
        # the run: n_top + 3 items with exactly the same best score, across the tile boundary at 128 (a multiple of both tiles)
        runs = [ii for ii, kd in enumerate(c.kinds) if kd == 'run']
        run_items = np.arange(RUN_AT, RUN_AT + n_top + 3)
        assert RUN_AT < 128 < RUN_AT + n_top + 3 and 128 % ITEM_TILE[dt] == 0
        hit = [ii for ii in runs if len(np.unique(S[ii, run_items])) == 1 and np.all(S[ii, run_items] >= np.max(S[ii]))]
        if c.kind == 'int':
            assert hit and list(ref_items[hit[0]]) == list(run_items[:n_top])
        assert c.Dt.dtype == DT[dt] and c.code.dtype == DT[dt]
        if c.kind == 'int':
            assert np.max(np.abs(c.Dt)) <= 8 and np.max(np.abs(c.code)) <= 8 and np.all(c.Dt == np.round(c.Dt))
            assert c.item_bias is None or (np.max(np.abs(c.item_bias)) <= 9 and np.all(c.item_bias == np.round(c.item_bias)))
            assert KMAX['f32'] * 64 + 9 < 2 ** 24                   # every partial sum is an integer f32 holds


def test_route_table():
    """the restated dispatch: its routes and boundaries, and the restated workspace against the library (host code: no GPU)"""
    from modl_amd._lib import lib
    for dt in ('f32', 'f64'):
        it = ITEM_TILE[dt]
        assert topn_route(dt, 1, 1) == (1, MIN_SLAB) and topn_route(dt, 256, 1)[0] == 1 and topn_route(dt, 257, 1)[0] == 2
        assert topn_route(dt, 512, 65)[0] == 2 and topn_route(dt, 513, 65)[0] == 3 and topn_route(dt, 5003, 33)[0] >= 3
        assert topn_route(dt, 10677, 1)[0] == _cdiv(_cdiv(10677, it), max(_cdiv(_cdiv(10677, it), MAX_SLABS), MIN_SLAB // it))
        assert topn_route(dt, 10 ** 6, 1)[0] <= MAX_SLABS
        assert topn_route(dt, 10677, 69878)[0] == 1                # many users: no slabs
        assert topn_route(dt, 10677, USERS * TARGET_WGS // 2)[0] == 2 and topn_route(dt, 10677, USERS * TARGET_WGS // 2 + 1)[0] == 1
        for p, b in ((1, 1), (700, 16), (5003, 65), (10677, 1), (10677, 69878), (2 ** 31 - 1, 1)):
            S, slab = topn_route(dt, p, b)
            assert slab % it == 0 and slab >= MIN_SLAB and (S - 1) * slab < p <= S * slab
        for args in ((700, 7, 16, 10), (1, 1, 1, 1), (5003, 65, 65, 128), (10677, 30, 69878, 10), (257, KMAX[dt], 33, 128),
                     (700, KMAX[dt] + 1, 16, 10), (700, 7, 16, 0), (700, 7, 16, 129), (0, 7, 16, 10), (2 ** 31, 7, 16, 10),
                     (700, 0, 16, 10), (700, 7, -1, 10), (700, 7, 0, 10)):
            got = lib.modl_recsys_topn_workspace(0 if dt == 'f32' else 1, *args)
            assert got == topn_workspace(dt, *args), (dt, args, got)
        assert lib.modl_recsys_topn_workspace(7, 700, 7, 16, 10) == 0
        # the mask is p bits per query; with one slab nothing else
        assert topn_workspace(dt, 10677, 30, 69878, 10) == _up(69878 * 4 * _cdiv(10677, 32), 256)
        assert max(topn_lds(dt, k, n) for k in range(1, KMAX[dt] + 1) for n in (1, 10, MAX_TOPN)) <= LDS_BYTES
    from modl_amd import recsys
    assert recsys.MAX_TOPN == MAX_TOPN


def _hp(a):
    return a.ctypes.data_as(C.c_void_p)


def test_topn_rejects_on_the_host():
    """the argument checks come before any device work: they answer without a device (host buffers stand in for device ones;
    nothing reads them)"""
    from modl_amd._lib import lib
    for dt in ('f32', 'f64'):
        f = getattr(lib, 'modl_recsys_topn_' + dt)
        a = np.zeros(64, dtype=DT[dt])
        i = np.zeros(64, dtype=np.int32)
        ws = np.zeros(1 << 16, dtype=np.uint8)

        def call(code=a, b=2, k=3, Dt=a, p=5, indptr=i, indices=i, n_top=2, items=i, scores=a, w=ws, nbytes=None):
            nb = w.nbytes if (nbytes is None and w is not None) else (nbytes or 0)
            return f(_hp(code) if code is not None else None, None, b, k, _hp(Dt) if Dt is not None else None, p,
                     _hp(indptr) if indptr is not None else None, _hp(indices) if indices is not None else None, None, None,
                     n_top, _hp(items) if items is not None else None, _hp(scores) if scores is not None else None,
                     _hp(w) if w is not None else None, nb, None)
        for kw in (dict(code=None), dict(Dt=None), dict(items=None), dict(scores=None), dict(indices=None), dict(b=-1),
                   dict(p=0), dict(p=2 ** 31), dict(n_top=0), dict(n_top=MAX_TOPN + 1), dict(k=0), dict(k=KMAX[dt] + 1)):
            assert call(**kw) == EINVAL, kw
        assert call(b=0) == 0 and call(b=0, w=None) == 0
        need = lib.modl_recsys_topn_workspace(0 if dt == 'f32' else 1, 5, 3, 2, 2)
        assert need > 0
        assert call(w=None) == ENOMEM and call(nbytes=need - 1) == ENOMEM
        if lib.modl_device_count() == 0:
            assert call(nbytes=need) == ENOGPU


# ---------------------------------------------------------------------------------------------------- layer 2: GPU tests
@pytest.fixture(scope='module')
def gpu():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    return torch


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to('cuda')


GUARD = 512


def run_topn(c, extra_rows=3, reverse=False):
    """one call of modl_recsys_topn_* on case c (reverse: the queries in reverse order, un-reversed afterwards); returns
    (rc, items, scores) and asserts that rows beyond b and the guard band behind the workspace are untouched"""
    import torch
    from modl_amd._lib import lib
    from modl_amd.device import ptr
    T = DT[c.dt]
    code_rows = c.code_rows if c.code_rows is not None else (np.arange(c.b, dtype=np.int64) if reverse else None)
    ex_rows = c.ex_rows if (c.ex_rows is not None or c.indptr is None) else (np.arange(c.b, dtype=np.int64) if reverse else None)
    if reverse:
        code_rows = code_rows[::-1].copy()
        ex_rows = None if ex_rows is None else ex_rows[::-1].copy()
    need = lib.modl_recsys_topn_workspace(0 if c.dt == 'f32' else 1, c.p, c.k, c.b, c.n_top)
    assert need == topn_workspace(c.dt, c.p, c.k, c.b, c.n_top)
    ws0 = np.random.RandomState(1).randint(0, 256, size=need + GUARD).astype(np.uint8)
    items0 = np.full((c.b + extra_rows, c.n_top), -77, dtype=np.int32)
    scores0 = np.full((c.b + extra_rows, c.n_top), 12345.0, dtype=T)
    d = [_dev(a) for a in (c.code, code_rows, c.Dt, c.indptr, c.indices, ex_rows, c.item_bias, items0, scores0, ws0)]
    rc = getattr(lib, 'modl_recsys_topn_' + c.dt)(ptr(d[0]), ptr(d[1]), c.b, c.k, ptr(d[2]), c.p, ptr(d[3]), ptr(d[4]), ptr(d[5]),
                                                  ptr(d[6]), c.n_top, ptr(d[7]), ptr(d[8]), ptr(d[9]), need, None)
    torch.cuda.synchronize()
    items, scores, ws = d[7].cpu().numpy(), d[8].cpu().numpy(), d[9].cpu().numpy()
    np.testing.assert_array_equal(items[c.b:], items0[c.b:], err_msg='rows of d_items beyond b changed')
    np.testing.assert_array_equal(scores[c.b:], scores0[c.b:], err_msg='rows of d_scores beyond b changed')
    np.testing.assert_array_equal(ws[need:], ws0[need:], err_msg='the guard band behind the workspace changed')
    items, scores = items[:c.b], scores[:c.b]
    if reverse:
        items, scores = items[::-1].copy(), scores[::-1].copy()
    return rc, items, scores


ABI_K = {'f32': (1, 7, 32, 33, 64, 65, 127, 186), 'f64': (1, 7, 32, 33, 64, 65, 127)}
ABI_P = (1, 31, 33, 257, 1000, 5003)           # 1000: four slabs for every b here; 5003: the slab cap of 256 items (20 / 20 / 20)
ABI_B = (1, 32, 33, 65)                        # the user tile is 32 queries
ABI_NTOP = (1, 10, 128)
ABI_CASES = [(dt, k) for dt in ('f32', 'f64') for k in ABI_K[dt]]


@pytest.mark.gpu
@pytest.mark.parametrize('dt,k', ABI_CASES, ids=['%s-k%d' % c for c in ABI_CASES])
def test_topn_abi(gpu, dt, k):
    """every p x b x n_top of the matrix; the four optional arguments walk through their sixteen combinations and the cases
    alternate between random ones (through `judge`) and integer ones (equal to the reference)"""
    n = 0
    seen = set()
    worst = 0.0
    for p in ABI_P:
        if p >= 1000 and k > 65:
            continue
        for b in ABI_B:
            for n_top in ABI_NTOP:
                flags = n % 16
                kind = 'int' if (n // 16 + n) % 2 else 'rand'
                c = make_case(dt, kind, k, p, b, n_top, 1000 * k + n, ex=bool(flags & 1), ex_rows=bool(flags & 2),
                              code_rows=bool(flags & 4), bias=bool(flags & 8))
                rc, items, scores = run_topn(c)
                assert rc == 0, (rc, p, b, n_top)
                worst = max(worst, judge(c, items, scores))
                seen.add((flags, kind))
                n += 1
    assert len(seen) == 32
    print('largest |score error| / E over the random cases: %.3g' % worst)
    assert topn_route(dt, 1000, 65)[0] >= 3 and topn_route(dt, 5003, 1)[0] >= 3


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_topn_rejects(gpu, dt):
    """every refusal returns its code and writes nothing: the outputs keep their sentinel"""
    import torch
    from modl_amd._lib import lib
    from modl_amd.device import ptr
    T = DT[dt]
    kbig = KMAX[dt] + 1
    c = make_case(dt, 'rand', 7, 300, 5, 10, 9)
    need = lib.modl_recsys_topn_workspace(0 if dt == 'f32' else 1, c.p, c.k, c.b, c.n_top)
    items0 = np.full((c.b, MAX_TOPN + 1), -77, dtype=np.int32)
    scores0 = np.full((c.b, MAX_TOPN + 1), 12345.0, dtype=T)
    big = np.zeros((c.p, kbig), dtype=T)
    base = dict(code=_dev(c.code), code_rows=_dev(c.code_rows), b=c.b, k=c.k, Dt=_dev(c.Dt), p=c.p, indptr=_dev(c.indptr),
                indices=_dev(c.indices), ex_rows=_dev(c.ex_rows), bias=_dev(c.item_bias), n_top=c.n_top, ws_bytes=need)
    f = getattr(lib, 'modl_recsys_topn_' + dt)

    def call(want, **kw):
        a = dict(base)
        a.update(kw)
        items, scores = _dev(items0), _dev(scores0)
        ws = a.pop('ws', torch.zeros(need + 16, dtype=torch.uint8, device='cuda'))
        a.setdefault('items', items)
        a.setdefault('scores', scores)
        rc = f(ptr(a['code']), ptr(a['code_rows']), a['b'], a['k'], ptr(a['Dt']), a['p'], ptr(a['indptr']), ptr(a['indices']),
               ptr(a['ex_rows']), ptr(a['bias']), a['n_top'], ptr(a['items']), ptr(a['scores']), ptr(ws), a['ws_bytes'], None)
        torch.cuda.synchronize()
        assert rc == want, (kw.keys(), rc)
        np.testing.assert_array_equal(items.cpu().numpy(), items0)
        np.testing.assert_array_equal(scores.cpu().numpy(), scores0)
    for kw in (dict(code=None), dict(Dt=None), dict(items=None), dict(scores=None), dict(indices=None), dict(b=-1), dict(p=0),
               dict(p=2 ** 31), dict(n_top=0), dict(n_top=MAX_TOPN + 1), dict(k=0), dict(k=kbig, Dt=_dev(big), code=_dev(big))):
        call(EINVAL, **kw)
    call(0, b=0)
    call(ENOMEM, ws=None)
    call(ENOMEM, ws_bytes=need - 1)
    # and the last values that are not refused run
    for kw in (dict(n_top=MAX_TOPN), dict(n_top=1)):
        c2 = make_case(dt, 'int', KMAX[dt], 300, 5, kw['n_top'], 10)
        rc, items, scores = run_topn(c2)
        assert rc == 0
        judge(c2, items, scores)


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_topn_is_repeatable(gpu, dt):
    """two calls give the same bits, and so does a call with the queries in reverse order (other tiles, other arrival orders
    in the candidate buffers); several slabs and one"""
    for p, b, kind in ((1000, 65, 'rand'), (1000, 65, 'int'), (200, 40, 'int')):
        c = make_case(dt, kind, 33, p, b, 10, 21)
        rc, i1, s1 = run_topn(c)
        rc2, i2, s2 = run_topn(c)
        rc3, i3, s3 = run_topn(c, reverse=True)
        assert rc == rc2 == rc3 == 0
        judge(c, i1, s1)
        for i, s in ((i2, s2), (i3, s3)):
            np.testing.assert_array_equal(i, i1)
            np.testing.assert_array_equal(s.view(np.uint32 if dt == 'f32' else np.uint64), s1.view(np.uint32 if dt == 'f32' else np.uint64))


def toy_ratings(n, p, dt, seed, density=0.25):
    rs = np.random.RandomState(seed)
    M = (rs.rand(n, p) < density)
    M[0] = False                                                    # a user without ratings
    M[1, :3] = True
    vals = np.clip(np.round(3 + rs.randn(n, 4).dot(rs.randn(4, p)) + 0.3 * rs.randn(n, p)), 1, 5)
    return sp.csr_matrix((vals * M).astype(dt))


def centre(est, X):
    """the centring of transform, restated: col_mean_ at the rated items, then the row bias
    (sum_f (x_f - col_mean_[f]) + beta global_mean_) / (n_u + beta)"""
    X = sp.csr_matrix(X, dtype=np.float64, copy=True)
    X.data -= est.col_mean_[X.indices]
    n_u = np.diff(X.indptr)
    bias = np.zeros(X.shape[0])
    for i in range(X.shape[0]):
        if n_u[i] + est.beta > 0:
            bias[i] = (X.data[X.indptr[i]:X.indptr[i + 1]].sum() + est.beta * est.global_mean_) / (n_u[i] + est.beta)
    X.data -= np.repeat(bias, n_u)
    return X, bias


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_transform_folds_in(gpu, dt):
    from modl_amd.recsys import RecsysDictFact
    X = toy_ratings(60, 40, DT[dt], 0)
    Xnew = toy_ratings(23, 40, DT[dt], 1)
    for detrend in (False, True):
        est = RecsysDictFact(n_components=5, alpha=0.5, beta=2.0, batch_size=8, n_epochs=2, random_state=0, detrend=detrend).fit(X)
        if not detrend:
            np.testing.assert_array_equal(est.transform(X), est.code_)      # the same kernel on the same input
            assert not hasattr(est, 'global_mean_')
        else:
            assert abs(est.global_mean_ - np.mean(X.data.astype(np.float64))) < 1e-5
        got = est.transform(Xnew)
        assert got.shape == (23, 5) and got.dtype == DT[dt]
        assert not np.any(got[0]) and np.diff(Xnew.indptr)[0] == 0         # a row without ratings is zero
        Xc = centre(est, Xnew)[0] if detrend else sp.csr_matrix(Xnew, dtype=np.float64)
        D64 = est.components_.astype(np.float64)
        rated = np.flatnonzero(np.diff(Xnew.indptr))
        r64 = np.stack([wo.recsys_solve_row(Xc, D64, i, est.alpha)[0] for i in rated])
        if dt == 'f64':
            err = rel_fro(got[rated], r64)
            print('transform detrend=%s: rel_fro %.3e' % (detrend, err))
            assert err < 1e-9
        else:
            X32 = sp.csr_matrix((Xc.data.astype(np.float32), Xc.indices, Xc.indptr), shape=Xc.shape)
            r32 = np.stack([wo.recsys_solve_row(X32, est.components_, i, est.alpha)[0] for i in rated])
            assert_within_f32_noise(got[rated], r32, r64, 'transform')


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_recommend_agrees_with_predict(gpu, dt):
    from modl_amd.recsys import RecsysDictFact
    n, p = 60, 40
    X = toy_ratings(n, p, DT[dt], 0)
    est = RecsysDictFact(n_components=5, alpha=0.5, beta=2.0, batch_size=8, n_epochs=2, random_state=0, detrend=True,
                         crop=(1.5, 4.5)).fit(X)
    items, scores = est.recommend(n_items=7)
    assert items.shape == (n, 7) and items.dtype == np.int64 and scores.dtype == np.float64

    def at_pattern(items, predictor):
        valid = items >= 0
        indptr = np.concatenate([[0], np.cumsum(valid.sum(axis=1))]).astype(np.int32)
        pat = sp.csr_matrix((np.ones(valid.sum()), items[valid].astype(np.int32), indptr), shape=(items.shape[0], p))
        out = np.full(items.shape, np.nan)
        out[valid] = predictor(pat).data
        return out
    np.testing.assert_array_equal(scores, at_pattern(items, est.predict))   # exactly predict at the returned loci (NaN at -1)
    seen = X.toarray() != 0
    for u in range(n):
        got = items[u][items[u] >= 0]
        assert len(got) == min(7, p - seen[u].sum()) and not np.any(seen[u, got]) and len(set(got)) == len(got)
    assert np.sum(scores == 4.5) + np.sum(scores == 1.5) > 0                # the crop binds somewhere: ranking is by the uncropped score
    raw = est.code_.astype(np.float64).dot(est.components_.astype(np.float64)) + est.col_mean_[None, :]
    for u in range(n):
        got = items[u][items[u] >= 0]
        assert np.all(np.diff(raw[u, got]) <= 1e-4 * (1 + np.abs(raw[u, got[:-1]])))
    # users=[...]: the matching rows of the full call; rows_per_call: the same result in chunks
    users = [17, 3, 59, 0, 3]
    i_u, s_u = est.recommend(n_items=7, users=users)
    np.testing.assert_array_equal(i_u, items[users])
    np.testing.assert_array_equal(s_u, scores[users])
    i_c, s_c = est.recommend(n_items=7, rows_per_call=7)
    np.testing.assert_array_equal(i_c, items)
    np.testing.assert_array_equal(s_c, scores)
    # exclude_seen=False can return seen items
    i_all, _ = est.recommend(n_items=7, exclude_seen=False)
    assert np.all(i_all >= 0) and any(np.any(seen[u, i_all[u]]) for u in range(n))
    # new users: exactly the entries of new_rows are excluded, and the scores are predictions from their folded-in codes
    Xnew = toy_ratings(23, p, DT[dt], 1)
    i_n, s_n = est.recommend(X=Xnew, n_items=p)
    seen_new = Xnew.toarray() != 0
    for u in range(23):
        got = i_n[u][i_n[u] >= 0]
        assert sorted(got) == list(np.flatnonzero(~seen_new[u])), u
        assert np.all(np.isnan(s_n[u][i_n[u] < 0])) and not np.any(np.isnan(s_n[u][i_n[u] >= 0]))
    Xc, bias = centre(est, Xnew)
    code = est.transform(Xnew).astype(np.float64)
    want = code.dot(est.components_.astype(np.float64)) + bias[:, None] + est.col_mean_[None, :]
    want = np.clip(want, 1.5, 4.5)
    for u in range(23):
        got = i_n[u][i_n[u] >= 0]
        np.testing.assert_allclose(s_n[u][:len(got)], want[u, got], rtol=0, atol=1e-4 if dt == 'f32' else 1e-9)
    i_n2, s_n2 = est.recommend(X=Xnew, n_items=p, rows_per_call=7)
    np.testing.assert_array_equal(i_n2, i_n)
    np.testing.assert_array_equal(s_n2, s_n)
    with pytest.raises(ValueError, match='%d' % MAX_TOPN):
        est.recommend(n_items=MAX_TOPN + 1)
