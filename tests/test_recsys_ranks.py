"""Ranks of held-out items on the ratings path: modl_recsys_ranks_* (csrc/recsys_rank.hip) through the C ABI, and
RecsysDictFact.ranks / ranking_score / ranking_metrics through the estimator.  Structured as tests/test_recsys_recommend.py,
whose cases (`make_case`), reference scores (`all_scores`) and top-N call (`run_topn`) it reuses.

0. The reference is `ref_ranks` below: float64 numpy; the rank of target t of a query is the number of items c != t that are not
   excluded and come before t in the (-score, item) order of `topn_reference`.
1. The targets of a case (`add_targets`): per query with candidates left, 8 items drawn from the reference's best 100
   non-excluded items (fewer where fewer exist) and 8 drawn from all p items (excluded ones included), interleaved and cut to
   t_max (rows that need more entries draw them the same way, with repeats); and, by (query + seed) % 8, a row without targets ('none'), with one target ('one'), with exactly t_max targets
   ('full': 64 where t_max is 64), with a repeated target ('repeat'), holding -1 and p ('outside'), and one that is three
   entries longer than t_max ('long': the excess must read -2).
2. Acceptance (`judge`), with E the per-score bound of tests/test_recsys_recommend.py (E = 2 k u_T max_f sum_c |code_c Dt[f][c]|,
   plus u_T |bias_f| in f32): a rank passes if lo <= rank <= hi, lo = #{c != t not excluded : ref_c > ref_t + E_t + E_c},
   hi = #{c != t not excluded : ref_c >= ref_t - E_t - E_c} (both scores are within their E of the reference: the sum is the
   "2 E" of equal bounds).  The -1 and -2 entries and n_candidates must be exact.  Integer cases (kind='int'): E = 0 and the
   ranks must EQUAL the reference, the tie rule included.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp

from .test_recsys_recommend import (DT, U, KMAX, EINVAL, ENOMEM, ENOGPU, USERS, KC, LDS_BYTES, make_case, query_codes, exclusions,
                                    all_scores, topn_route, run_topn, toy_ratings, _cdiv, _up, _hp, _dev)

MAX_T = 64
GUARD = 512
HEAD = 3                                                           # entries of t_indices / d_ranks in front of the call's
SPECIALS = ('plain', 'none', 'one', 'full', 'repeat', 'outside', 'long', 'plain')


# ---------------------------------------------------------------------------------------------------- restated formulas
def ranks_workspace(dt, p, k, b, t_max):
    """rank_ws: two bitmasks of p bits per query, t_max + 1 counters and t_max scores per query"""
    if not (b >= 1 and 1 <= p < 2 ** 31 and 1 <= t_max <= MAX_T and 1 <= k <= KMAX[dt]):
        return 0
    return (2 * _up(4 * b * _cdiv(p, 32), 256) + _up(4 * b * (t_max + 1), 256) + _up((4 if dt == 'f32' else 8) * b * t_max, 256))


def ranks_lds(dt, k, t_max):
    """rank_lds: the dynamic LDS of recsys_rank_sweep_kernel"""
    tsz, tk, it = (4, 2, 128) if dt == 'f32' else (8, 4, 64)
    kp = _up(k, tk)
    ldt, ldh = t_max | 1, (t_max + 1) | 1
    o = tsz * (USERS * (kp | 1) + it * (min(kp, KC) | 1) + 2 * USERS * ldt)
    o = _up(o, 8) + 8 * it + 4 * (2 * USERS * ldt + USERS * ldh + 2 * USERS + USERS * (it // 32))
    return _up(o, 16)


# ---------------------------------------------------------------------------------------------------- targets, reference
def add_targets(c, t_max, seed):
    """the target rows of case c (a list of int32 arrays, one per query) by the recipe of the module docstring"""
    rs = np.random.RandomState(seed)
    S = all_scores(query_codes(c), c.Dt, c.item_bias)
    excl = exclusions(c)
    ids = np.arange(c.p)
    rows, kinds = [], []
    for ii in range(c.b):
        ok = np.ones(c.p, dtype=bool)
        if excl is not None:
            ok[excl[ii]] = False
        plain = best = np.zeros(0, dtype=np.int64)
        if ok.any():
            order = np.lexsort((ids, -S[ii]))
            best = order[ok[order]][:100]
            a = rs.choice(best, min(8, len(best)), replace=False)
            bb = rs.choice(c.p, 8, replace=c.p < 8)
            plain = np.concatenate([np.stack([a[:len(a)], bb[:len(a)]], axis=1).ravel(), bb[len(a):]])
        kd = SPECIALS[(ii + seed) % len(SPECIALS)]

        def fill(n):                                               # more of the same: every other one from the best 100
            f = rs.randint(0, c.p, size=max(n, 0))
            if len(best):
                f[::2] = rs.choice(best, len(f[::2]))
            return f
        if kd == 'none':
            row = plain[:0]
        elif kd == 'one':
            row = np.concatenate([plain, fill(1)])[:1]
        elif kd == 'full':
            row = np.concatenate([plain[:t_max], fill(t_max - len(plain))])
        elif kd == 'repeat':
            row = np.concatenate([plain, fill(2)])[:t_max].copy()
            row[-1] = row[0]
        elif kd == 'outside':
            row = np.concatenate([[-1, c.p], plain])[:t_max]
        elif kd == 'long':
            row = np.concatenate([plain[:t_max], fill(t_max + 3 - min(len(plain), t_max))])
        else:
            row = plain[:t_max]
        rows.append(np.asarray(row, dtype=np.int32))
        kinds.append(kd)
    return rows, kinds


MUTANTS = ('no_exclusion', 'last_excluded_dropped', 'ties_larger_id', 'counts_itself', 'other_targets_not_counted',
           'excluded_target_minus1', 'no_bias', 'ex_rows_ignored', 'never_last', 'slabs_not_summed')


def ref_ranks(code, Dt, excl, item_bias, rows, t_max, mutant=None):
    """(ranks per query: a list of int64 arrays; n_candidates int64 (b,)).  `mutant`: one thing wrong (MUTANTS)."""
    b, p = code.shape[0], Dt.shape[0]
    S = all_scores(code, Dt, None if mutant == 'no_bias' else item_bias)
    ids = np.arange(p)
    out, ncand = [], np.zeros(b, dtype=np.int64)
    for ii in range(b):
        ok = np.ones(p, dtype=bool)
        if excl is not None:
            ok[excl[ii]] = False
        ncand[ii] = ok.sum()
        if mutant == 'no_exclusion':
            ok[:] = True
        if mutant == 'never_last':
            ok[p - 1] = False
        if mutant == 'other_targets_not_counted':
            own = rows[ii][:t_max]
            own = own[(own >= 0) & (own < p)]
        r = np.full(len(rows[ii]), -2, dtype=np.int64)
        for j, t in enumerate(rows[ii][:t_max]):
            if t < 0 or t >= p:
                r[j] = -1
                continue
            cand = ok.copy()
            if mutant != 'counts_itself':
                cand[t] = False
            if mutant == 'other_targets_not_counted':
                cand[own] = False
            if mutant == 'slabs_not_summed':
                cand[:t // 256 * 256] = False
                cand[(t // 256 + 1) * 256:] = False
            s = S[ii]
            tie = (ids > t) if mutant == 'ties_larger_id' else (ids < t)
            if mutant == 'counts_itself':
                tie = tie | (ids == t)
            r[j] = np.sum(cand & ((s > s[t]) | ((s == s[t]) & tie)))
            if mutant == 'excluded_target_minus1' and not ok[t]:
                r[j] = -1
        out.append(r)
    return out, ncand


def case_reference(c, rows, t_max, mutant=None):
    excl = exclusions(c, identity_rows=mutant == 'ex_rows_ignored', drop_last=mutant == 'last_excluded_dropped')
    m = mutant if mutant not in ('ex_rows_ignored', 'last_excluded_dropped') else None
    return ref_ranks(query_codes(c), c.Dt, excl, c.item_bias, rows, t_max, m)


def score_bound(dt, exact, k, code, Dt, item_bias):
    """E (b, p): the per-score bound of tests/test_recsys_recommend.py's judge"""
    absdot = np.abs(code.astype(np.float64)).dot(np.abs(Dt.astype(np.float64)).T)
    E = (0.0 if exact else 2.0 * k * U[dt]) * np.max(absdot, axis=1)[:, None] * np.ones((1, Dt.shape[0]))
    if dt == 'f32' and item_bias is not None and not exact:
        E = E + U['f32'] * np.abs(item_bias)[None, :]
    return E


def judge_ranks(dt, exact, k, code, Dt, excl, item_bias, rows, t_max, ranks, n_candidates=None):
    """the rule of the module docstring for the ranks (a list of arrays per query) of a call; returns the number of ranks
    that differ from the float64 reference (all inside their band)"""
    b, p = code.shape[0], Dt.shape[0]
    S = all_scores(code, Dt, item_bias)
    E = score_bound(dt, exact, k, code, Dt, item_bias)
    r_ref, nc_ref = ref_ranks(code, Dt, excl, item_bias, rows, t_max)
    if n_candidates is not None:
        np.testing.assert_array_equal(np.asarray(n_candidates).astype(np.int64), nc_ref, err_msg='n_candidates')
    moved = 0
    for ii in range(b):
        got = np.asarray(ranks[ii]).astype(np.int64)
        assert got.shape == r_ref[ii].shape, ('entries of the row', ii)
        fixed = r_ref[ii] < 0
        np.testing.assert_array_equal(got[fixed], r_ref[ii][fixed], err_msg='the -1 / -2 entries of query %d' % ii)
        assert np.all(got[~fixed] >= 0), ('a rank is negative', ii)
        if exact:
            np.testing.assert_array_equal(got, r_ref[ii], err_msg='exact case: the ranks of query %d differ from the reference' % ii)
            continue
        ok = np.ones(p, dtype=bool)
        if excl is not None:
            ok[excl[ii]] = False
        for j in np.flatnonzero(~fixed):
            t = rows[ii][j]
            cand = ok.copy()
            cand[t] = False
            margin = E[ii, t] + E[ii]
            lo = int(np.sum(cand & (S[ii] > S[ii, t] + margin)))
            hi = int(np.sum(cand & (S[ii] >= S[ii, t] - margin)))
            assert lo <= got[j] <= hi, ('rank outside its band', ii, j, int(t), lo, int(got[j]), hi)
            moved += int(got[j] != r_ref[ii][j])
    return moved


def judge(c, rows, t_max, ranks, n_candidates=None):
    return judge_ranks(c.dt, c.kind == 'int', c.k, query_codes(c), c.Dt, exclusions(c), c.item_bias, rows, t_max, ranks,
                       n_candidates)


def accepts(c, rows, t_max, ranks, n_candidates=None):
    try:
        judge(c, rows, t_max, ranks, n_candidates)
    except AssertionError:
        return False
    return True


def in_range_stats(c, rows, t_max):
    """(share of the in-range targets that share their score with another candidate, share with a reference rank < 128)"""
    S = all_scores(query_codes(c), c.Dt, c.item_bias)
    excl = exclusions(c)
    r_ref, _ = case_reference(c, rows, t_max)
    n = tied = low = 0
    for ii in range(c.b):
        ok = np.ones(c.p, dtype=bool)
        if excl is not None:
            ok[excl[ii]] = False
        for j, t in enumerate(rows[ii][:t_max]):
            if 0 <= t < c.p:
                cand = ok.copy()
                cand[t] = False
                n += 1
                tied += bool(np.any(cand & (S[ii] == S[ii, t])))
                low += bool(r_ref[ii][j] < 128)
    return tied / max(n, 1), low / max(n, 1)


# the CPU case matrix: every query kind of make_case twice, three slabs of 256 items, every optional argument given
def cpu_cases(dt):
    cs = [make_case(dt, 'rand', 7, 700, 16, 10, 3), make_case(dt, 'int', 7, 700, 16, 10, 4),
          make_case(dt, 'int', 7, 700, 16, 10, 5, bias=False)]
    return [(c, add_targets(c, 16, 7 + i)[0], 16) for i, c in enumerate(cs)]


# ---------------------------------------------------------------------------------------------------- layer 1: CPU tests
@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_judge_rejects_mutants(dt):
    """`judge` accepts the reference on every case of the matrix and rejects each of the ten wrong versions of it on the integer
    case with a bias; on the random case all but 'ties_larger_id' (equal scores lie inside every band: only E = 0 pins the tie
    rule) and on the integer case without a bias all but 'no_bias'"""
    cases = cpu_cases(dt)
    for c, rows, t_max in cases:
        assert accepts(c, rows, t_max, *case_reference(c, rows, t_max))
    assert len(MUTANTS) == 10
    for (c, rows, t_max), blind in zip(cases, ('ties_larger_id', None, 'no_bias')):
        survivors = [m for m in MUTANTS if m != blind and accepts(c, rows, t_max, case_reference(c, rows, t_max, m)[0])]
        assert not survivors, (c.kind, survivors)
    # a wrong n_candidates is rejected too
    r, nc = case_reference(cases[0][0], cases[0][1], 16)
    assert not accepts(cases[0][0], cases[0][1], 16, r, nc + 1)


CLAIM_SHAPES = (('f32', 1, 31, 33), ('f32', 7, 1000, 33), ('f32', 64, 257, 32), ('f32', 186, 5003, 65), ('f64', 127, 5003, 65),
                ('f64', 33, 1000, 33))


@pytest.mark.parametrize('dt,k,p,b', CLAIM_SHAPES, ids=['%s-k%d-p%d-b%d' % s for s in CLAIM_SHAPES])
def test_cases_are_what_they_claim(dt, k, p, b):
    """integer cases hold ties where they matter (at least a quarter of the in-range targets share their score with another
    candidate), at least a third of the in-range targets rank below 128, and every special row is there"""
    c = make_case(dt, 'int', k, p, b, 10, 1)
    for t_max in (16, 64):
        rows, kinds = add_targets(c, t_max, 1)
        tied, low = in_range_stats(c, rows, t_max)
        print('%s k=%d p=%d b=%d t_max=%d: tied %.2f, rank < 128 %.2f' % (dt, k, p, b, t_max, tied, low))
        assert tied >= 0.25 and low >= 1.0 / 3
        assert set(kinds) == set(SPECIALS)
        for row, kd in zip(rows, kinds):
            if kd == 'none':
                assert len(row) == 0
            if kd == 'one':
                assert len(row) == 1
            if kd == 'full':
                assert len(row) == t_max
            if kd == 'repeat':
                assert len(row) >= 2 and row[-1] == row[0]
            if kd == 'outside':
                assert row[0] == -1 and row[1] == p
            if kd == 'long':
                assert len(row) == t_max + 3
            if kd != 'long':
                assert len(row) <= t_max
    assert any(len(r) == MAX_T for r in rows)


def brute_metrics(S, cand, targets, n_items):
    """ranking figures from a dense score matrix: per user sort the candidates, read off the positions of the targets, and
    count the AUC pair by pair"""
    fig = {key: [] for key in ('hit_rate', 'precision', 'recall', 'ndcg', 'mrr', 'auc')}
    ranks, ncand = [], []
    for u in range(S.shape[0]):
        c = np.flatnonzero(cand[u])
        order = sorted(c, key=lambda f: (-S[u, f], f))
        pos = {f: i for i, f in enumerate(order)}
        t = list(targets[u])
        ranks.append([pos[f] for f in t])
        ncand.append(len(c))
        if not t:
            continue
        m = len(t)
        r = sorted(pos[f] for f in t)
        hits = sum(x < n_items for x in r)
        fig['hit_rate'].append(float(hits > 0))
        fig['precision'].append(hits / n_items)
        fig['recall'].append(hits / m)
        fig['ndcg'].append(sum(1 / np.log2(x + 2) for x in r if x < n_items) / sum(1 / np.log2(i + 2) for i in range(min(m, n_items))))
        fig['mrr'].append(1 / (r[0] + 1))
        others = [f for f in c if f not in t]
        if others:
            won = sum((S[u, f], -f) > (S[u, g], -g) for f in t for g in others)
            fig['auc'].append(won / (m * len(others)))
    return ranks, ncand, {key: (float(np.mean(v)) if v else float('nan')) for key, v in fig.items()}


def test_ranking_metrics():
    from modl_amd.recsys import ranking_metrics, RankingScore
    # by hand: 6 candidates; user 0 has targets at ranks 0 and 3, user 1 none, user 2 one target at rank 4, N = 2
    #   user 0: hits 1, precision 1/2, recall 1/2, hit 1, dcg 1, ideal 1 + 1/log2(3), mrr 1, auc 1 - (0 + 2) / (2 * 4) = 3/4
    #   user 2: hits 0, everything 0 except mrr 1/5 and auc 1 - 4 / (1 * 5) = 1/5
    got = ranking_metrics([0, 3, 4], [0, 2, 2, 3], [6, 6, 6], 2)
    assert isinstance(got, RankingScore) and got._fields == ('hit_rate', 'precision', 'recall', 'ndcg', 'mrr', 'auc', 'n_users',
                                                              'n_targets')
    want = (0.5, 0.25, 0.25, 0.5 / (1 + 1 / np.log2(3)), 0.6, 0.475, 2, 3)
    np.testing.assert_allclose(got[:6], want[:6], rtol=1e-15, atol=0)
    assert got[6:] == want[6:]
    # random small problems against the brute force, with ties, users without targets and users whose targets are all candidates
    rs = np.random.RandomState(0)
    for trial in range(30):
        n, p = 7, 12
        S = rs.randint(-3, 4, size=(n, p)).astype(np.float64) if trial % 2 else rs.randn(n, p)
        cand = rs.rand(n, p) < 0.8
        cand[:, 0] = True
        targets = []
        for u in range(n):
            c = np.flatnonzero(cand[u])
            m = 0 if u == 1 else (len(c) if u == 2 else rs.randint(0, min(5, len(c)) + 1))
            targets.append(rs.choice(c, m, replace=False))
        n_items = (1, 3, 20)[trial % 3]
        ranks, ncand, fig = brute_metrics(S, cand, targets, n_items)
        indptr = np.concatenate([[0], np.cumsum([len(t) for t in targets])])
        got = ranking_metrics(np.concatenate([np.asarray(r, dtype=np.int64) for r in ranks]), indptr, ncand, n_items)
        for key in fig:
            np.testing.assert_allclose(getattr(got, key), fig[key], rtol=1e-13, atol=0, err_msg=key)
        assert got.n_users == sum(len(t) > 0 for t in targets) and got.n_targets == indptr[-1]
    # nobody has targets: NaN, not an error; only users whose targets are all their candidates: no auc
    none = ranking_metrics([], [0, 0], [5], 3)
    assert none.n_users == 0 and np.isnan(none.hit_rate) and np.isnan(none.auc)
    full = ranking_metrics([0, 1], [0, 2], [2], 1)
    assert full.hit_rate == 1.0 and full.recall == 0.5 and np.isnan(full.auc)
    with pytest.raises(ValueError):
        ranking_metrics([0, -1], [0, 2], [5], 3)
    with pytest.raises(ValueError):
        ranking_metrics([0, 1], [0, 3], [5], 3)


ABI_K = {'f32': (1, 7, 32, 33, 64, 65, 127, 186), 'f64': (1, 7, 32, 33, 64, 65, 127)}
ABI_P = (1, 31, 33, 257, 1000, 5003)
ABI_B = (1, 32, 33, 65)
ABI_TMAX = (1, 2, 63, 64)
ABI_CASES = [(dt, k) for dt in ('f32', 'f64') for k in ABI_K[dt]]


def test_workspace_and_route_table():
    """the restated workspace against the library over the grid of the ABI test, 0 for every refused argument, and the LDS of
    every (k, t_max) within a workgroup's 160 KiB; the slabs are the top-N call's (`topn_route`)"""
    from modl_amd._lib import lib
    from modl_amd import recsys, _lib
    assert _lib.RECSYS_MAX_RANK_TARGETS == MAX_T == recsys.MAX_RANK_TARGETS
    for dt in ('f32', 'f64'):
        di = 0 if dt == 'f32' else 1
        for k in ABI_K[dt]:
            for p in ABI_P + (10677, 2 ** 31 - 1):
                for b in ABI_B + (69878,):
                    for t_max in ABI_TMAX + (10,):
                        got = lib.modl_recsys_ranks_workspace(di, p, k, b, t_max)
                        assert got == ranks_workspace(dt, p, k, b, t_max) > 0, (dt, p, k, b, t_max, got)
        for args in ((700, KMAX[dt] + 1, 16, 10), (700, 0, 16, 10), (700, 7, 16, 0), (700, 7, 16, MAX_T + 1), (0, 7, 16, 10),
                     (2 ** 31, 7, 16, 10), (700, 7, -1, 10), (700, 7, 0, 10)):
            assert lib.modl_recsys_ranks_workspace(di, *args) == 0 == ranks_workspace(dt, *args), (dt, args)
        assert lib.modl_recsys_ranks_workspace(7, 700, 7, 16, 10) == 0
        assert max(ranks_lds(dt, k, t) for k in range(1, KMAX[dt] + 1) for t in (1, 10, MAX_T)) <= LDS_BYTES
        assert topn_route(dt, 1000, 65)[0] >= 3 and topn_route(dt, 5003, 1)[0] >= 3 and topn_route(dt, 10677, 69878)[0] == 1


def test_ranks_rejects_on_the_host():
    """the argument checks come before any device work: they answer without a device (host buffers stand in for device ones;
    nothing reads or writes them)"""
    from modl_amd._lib import lib
    for dt in ('f32', 'f64'):
        f = getattr(lib, 'modl_recsys_ranks_' + dt)
        a = np.zeros(64, dtype=DT[dt])
        i = np.zeros(64, dtype=np.int32)
        out0 = np.full(64, -77, dtype=np.int32)
        out, nc = out0.copy(), out0.copy()
        ws = np.zeros(1 << 16, dtype=np.uint8)
        P = lambda x: _hp(x) if x is not None else None

        def call(code=a, b=2, k=3, Dt=a, p=5, indptr=i, indices=i, t_indptr=i, t_indices=i, t_max=2, ranks=out, w=ws, nbytes=None):
            nb = w.nbytes if (nbytes is None and w is not None) else (nbytes or 0)
            return f(P(code), None, b, k, P(Dt), p, P(indptr), P(indices), None, None, P(t_indptr), P(t_indices), t_max, P(ranks),
                     P(nc), P(w), nb, None)
        for kw in (dict(code=None), dict(Dt=None), dict(t_indptr=None), dict(t_indices=None), dict(ranks=None), dict(indices=None),
                   dict(b=-1), dict(p=0), dict(p=2 ** 31), dict(t_max=0), dict(t_max=MAX_T + 1), dict(k=0), dict(k=KMAX[dt] + 1)):
            assert call(**kw) == EINVAL, kw
        assert call(b=0) == 0 and call(b=0, w=None) == 0
        need = lib.modl_recsys_ranks_workspace(0 if dt == 'f32' else 1, 5, 3, 2, 2)
        assert need > 0
        assert call(w=None) == ENOMEM and call(nbytes=need - 1) == ENOMEM
        if lib.modl_device_count() == 0:
            assert call(nbytes=need) == ENOGPU
        np.testing.assert_array_equal(out, out0)
        np.testing.assert_array_equal(nc, out0)


def test_estimator_refuses_shapes_that_do_not_fit():
    """ranks / ranking_score check X_test against the fitted shape before any device work"""
    from modl_amd.recsys import RecsysDictFact
    est = RecsysDictFact()
    est._dev = SimpleNamespace(n=5, p=7)
    with pytest.raises(ValueError, match='columns'):
        est.ranks(sp.csr_matrix((5, 8)))
    with pytest.raises(ValueError, match='rows'):
        est.ranks(sp.csr_matrix((4, 7)))
    with pytest.raises(ValueError, match='columns'):
        est.ranking_score(sp.csr_matrix((5, 6)))


# ---------------------------------------------------------------------------------------------------- layer 2: GPU tests
@pytest.fixture(scope='module')
def gpu():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    return torch


def run_ranks(c, rows, t_max, order=None, with_ncand=True):
    """one call of modl_recsys_ranks_* on case c with the target rows `rows`.  order: the queries of the call (indices into the
    case's, any order; None: all, through the case's own optional arguments).  Returns (rc, ranks: a list of arrays in the
    order of `order`, n_candidates) and asserts that d_ranks in front of and behind the call's entries, d_n_candidates beyond b
    and the guard band behind the workspace are untouched."""
    import torch
    from modl_amd._lib import lib
    from modl_amd.device import ptr
    code_rows, ex_rows = c.code_rows, c.ex_rows
    q = np.arange(c.b) if order is None else np.asarray(order)
    if order is not None:
        code_rows = (c.code_rows if c.code_rows is not None else np.arange(c.b, dtype=np.int64))[q].copy()
        if c.indptr is not None:
            ex_rows = (c.ex_rows if c.ex_rows is not None else np.arange(c.b, dtype=np.int64))[q].copy()
    b = len(q)
    t_rows = [rows[ii] for ii in q]
    lens = np.array([len(r) for r in t_rows], dtype=np.int64)
    t_indptr = (HEAD + np.concatenate([[0], np.cumsum(lens)])).astype(np.int32)
    t_indices = np.concatenate([np.full(HEAD, 0, dtype=np.int32)] + t_rows + [np.zeros(1, dtype=np.int32)]).astype(np.int32)
    n_e = int(lens.sum())
    need = lib.modl_recsys_ranks_workspace(0 if c.dt == 'f32' else 1, c.p, c.k, b, t_max)
    assert need == ranks_workspace(c.dt, c.p, c.k, b, t_max)
    ws0 = np.random.RandomState(1).randint(0, 256, size=need + GUARD).astype(np.uint8)
    ranks0 = np.full(HEAD + n_e + 5, -77, dtype=np.int32)
    nc0 = np.full(b + 3, -77, dtype=np.int32)
    d = [_dev(a) for a in (c.code, code_rows, c.Dt, c.indptr, c.indices, ex_rows, c.item_bias, t_indptr, t_indices, ranks0, nc0, ws0)]
    rc = getattr(lib, 'modl_recsys_ranks_' + c.dt)(ptr(d[0]), ptr(d[1]), b, c.k, ptr(d[2]), c.p, ptr(d[3]), ptr(d[4]), ptr(d[5]),
                                                   ptr(d[6]), ptr(d[7]), ptr(d[8]), t_max, ptr(d[9]),
                                                   ptr(d[10]) if with_ncand else None, ptr(d[11]), need, None)
    torch.cuda.synchronize()
    ranks, nc, ws = d[9].cpu().numpy(), d[10].cpu().numpy(), d[11].cpu().numpy()
    np.testing.assert_array_equal(ranks[:HEAD], ranks0[:HEAD], err_msg='d_ranks in front of the call changed')
    np.testing.assert_array_equal(ranks[HEAD + n_e:], ranks0[HEAD + n_e:], err_msg='d_ranks behind the call changed')
    np.testing.assert_array_equal(nc[b:], nc0[b:], err_msg='d_n_candidates beyond b changed')
    np.testing.assert_array_equal(ws[need:], ws0[need:], err_msg='the guard band behind the workspace changed')
    if not with_ncand:
        np.testing.assert_array_equal(nc, nc0)
    return rc, [ranks[t_indptr[j]:t_indptr[j + 1]] for j in range(b)], nc[:b]


@pytest.mark.gpu
@pytest.mark.parametrize('dt,k', ABI_CASES, ids=['%s-k%d' % c for c in ABI_CASES])
def test_ranks_abi(gpu, dt, k):
    """every p x b x t_max of the matrix; the four optional arguments walk through their sixteen combinations and the cases
    alternate between random ones (through `judge`) and integer ones (equal to the reference)"""
    n = 0
    seen = set()
    moved = total = 0
    for p in ABI_P:
        if p >= 1000 and k > 65:
            continue
        for b in ABI_B:
            for t_max in ABI_TMAX:
                flags = n % 16
                kind = 'int' if (n // 16 + n) % 2 else 'rand'
                c = make_case(dt, kind, k, p, b, 10, 1000 * k + n, ex=bool(flags & 1), ex_rows=bool(flags & 2),
                              code_rows=bool(flags & 4), bias=bool(flags & 8))
                rows, _ = add_targets(c, t_max, n)
                rc, ranks, nc = run_ranks(c, rows, t_max, with_ncand=bool(n % 5))
                assert rc == 0, (rc, p, b, t_max)
                moved += judge(c, rows, t_max, ranks, nc if n % 5 else None)
                total += sum(len(r) for r in rows)
                seen.add((flags, kind))
                n += 1
    assert len(seen) == 32
    print('%d of %d ranks differ from the float64 reference, all inside their band' % (moved, total))


AGREE = (('rand', 33, 1000, 65), ('int', 33, 1000, 65), ('int', 7, 257, 33), ('rand', 64, 5003, 32), ('int', 1, 31, 33),
         ('rand', 0, 300, 5), ('int', 0, 300, 5))                   # k = 0: the largest k of the dtype


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_ranks_agree_with_topn(gpu, dt):
    """exact, random and integer cases alike: a target with rank < 128 that is not itself excluded sits at exactly that
    position of the list modl_recsys_topn_* returns for its query with n_top = 128, and every list entry that is a target has
    its position as its rank"""
    for kind, k, p, b in AGREE:
        c = make_case(dt, kind, k or KMAX[dt], p, b, 128, 31)
        t_max = 64 if k != 7 else 16
        rows, _ = add_targets(c, t_max, 5)
        assert in_range_stats(c, rows, t_max)[1] >= 1.0 / 3
        rc, ranks, _ = run_ranks(c, rows, t_max)
        rc2, items, _ = run_topn(c)
        assert rc == rc2 == 0
        excl = exclusions(c)
        checked = 0
        for ii in range(c.b):
            ex = set() if excl is None else set(int(f) for f in excl[ii])
            lst = [int(f) for f in items[ii]]
            for j, t in enumerate(rows[ii][:t_max]):
                t, r = int(t), int(ranks[ii][j])
                if 0 <= t < p and t not in ex:
                    if r < 128:
                        assert lst[r] == t, (kind, k, p, ii, j, t, r)
                        checked += 1
                    else:
                        assert t not in lst, (kind, k, p, ii, j, t, r)
                    if t in lst:
                        assert lst.index(t) == r, (kind, k, p, ii, j, t, r)
        assert checked > 0


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_ranks_rejects(gpu, dt):
    """every refusal returns its code and writes nothing: the outputs keep their sentinel"""
    import torch
    from modl_amd._lib import lib
    from modl_amd.device import ptr
    T = DT[dt]
    kbig = KMAX[dt] + 1
    c = make_case(dt, 'rand', 7, 300, 5, 10, 9)
    rows, _ = add_targets(c, 16, 2)
    t_indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    t_indices = np.concatenate(rows).astype(np.int32)
    need = lib.modl_recsys_ranks_workspace(0 if dt == 'f32' else 1, c.p, c.k, c.b, 16)
    ranks0 = np.full(len(t_indices) + 4, -77, dtype=np.int32)
    nc0 = np.full(c.b, -77, dtype=np.int32)
    big = np.zeros((c.p, kbig), dtype=T)
    base = dict(code=_dev(c.code), code_rows=_dev(c.code_rows), b=c.b, k=c.k, Dt=_dev(c.Dt), p=c.p, indptr=_dev(c.indptr),
                indices=_dev(c.indices), ex_rows=_dev(c.ex_rows), bias=_dev(c.item_bias), t_indptr=_dev(t_indptr),
                t_indices=_dev(t_indices), t_max=16, ws_bytes=need)
    f = getattr(lib, 'modl_recsys_ranks_' + dt)

    def call(want, **kw):
        a = dict(base)
        a.update(kw)
        ranks, nc = _dev(ranks0), _dev(nc0)
        ws = a.pop('ws', torch.zeros(need + 16, dtype=torch.uint8, device='cuda'))
        a.setdefault('ranks', ranks)
        rc = f(ptr(a['code']), ptr(a['code_rows']), a['b'], a['k'], ptr(a['Dt']), a['p'], ptr(a['indptr']), ptr(a['indices']),
               ptr(a['ex_rows']), ptr(a['bias']), ptr(a['t_indptr']), ptr(a['t_indices']), a['t_max'], ptr(a['ranks']), ptr(nc),
               ptr(ws), a['ws_bytes'], None)
        torch.cuda.synchronize()
        assert rc == want, (kw.keys(), rc)
        np.testing.assert_array_equal(ranks.cpu().numpy(), ranks0)
        np.testing.assert_array_equal(nc.cpu().numpy(), nc0)
    for kw in (dict(code=None), dict(Dt=None), dict(t_indptr=None), dict(t_indices=None), dict(ranks=None), dict(indices=None),
               dict(b=-1), dict(p=0), dict(p=2 ** 31), dict(t_max=0), dict(t_max=MAX_T + 1), dict(k=0),
               dict(k=kbig, Dt=_dev(big), code=_dev(big))):
        call(EINVAL, **kw)
    call(0, b=0)
    call(ENOMEM, ws=None)
    call(ENOMEM, ws_bytes=need - 1)
    # and the last values that are not refused run
    for t_max in (1, MAX_T):
        c2 = make_case(dt, 'int', KMAX[dt], 300, 5, 10, 10)
        rows2, _ = add_targets(c2, t_max, 3)
        rc, ranks, nc = run_ranks(c2, rows2, t_max)
        assert rc == 0
        judge(c2, rows2, t_max, ranks, nc)


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_ranks_are_repeatable(gpu, dt):
    """two calls give the same bits; so does a call with the queries in reverse order, entry for entry; and a call with 65
    queries in one piece equals calls with 32 + 33 of them, which cut the items into other slabs"""
    for p, b, kind in ((1000, 65, 'rand'), (1000, 65, 'int'), (200, 40, 'int')):
        c = make_case(dt, kind, 33, p, b, 10, 21)
        rows, _ = add_targets(c, 64, 4)
        rc, r1, n1 = run_ranks(c, rows, 64)
        rc2, r2, n2 = run_ranks(c, rows, 64)
        rev = np.arange(b)[::-1]
        rc3, r3, n3 = run_ranks(c, rows, 64, order=rev)
        rc4, r4, n4 = run_ranks(c, rows, 64, order=np.arange(32))
        rc5, r5, n5 = run_ranks(c, rows, 64, order=np.arange(32, b))
        assert rc == rc2 == rc3 == rc4 == rc5 == 0
        judge(c, rows, 64, r1, n1)
        for r, n_c in ((r2, n2), (r3[::-1], n3[::-1]), (r4 + r5, np.concatenate([n4, n5]))):
            assert len(r) == b
            for ii in range(b):
                np.testing.assert_array_equal(r[ii], r1[ii])
            np.testing.assert_array_equal(n_c, n1)


def held_out(n, p, dt, seed):
    """(train, test) of toy_ratings by train_test_split, as CSR; user 2 holds 150 more test entries at items it has not rated"""
    from modl_amd.utils.recsys import train_test_split
    X = toy_ratings(n, p, DT[dt], seed)
    train, test = train_test_split(X, train_size=0.75, random_state=seed)
    train, test = sp.csr_matrix(train), sp.lil_matrix(test)
    free = np.flatnonzero(X[2].toarray().ravel() == 0)[:150]
    assert len(free) == 150
    rs = np.random.RandomState(seed)
    for f in free:
        test[2, f] = rs.randint(1, 6)
    test = sp.csr_matrix(test, dtype=DT[dt])
    assert test[2].nnz > 2 * MAX_T and train[0].nnz == 0
    return train, test


@pytest.mark.gpu
@pytest.mark.parametrize('detrend', [False, True], ids=['plain', 'detrend'])
@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_estimator_ranks(gpu, dt, detrend):
    from modl_amd.recsys import RecsysDictFact, ranking_metrics, RankingScore
    n, p = 60, 260
    train, test = held_out(n, p, dt, 0)
    est = RecsysDictFact(n_components=5, alpha=0.5, beta=2.0, batch_size=8, n_epochs=2, random_state=0, detrend=detrend,
                         crop=(1.5, 4.5)).fit(train)
    new_train, new_test = held_out(23, p, dt, 1)
    user_of = lambda M: np.repeat(np.arange(M.shape[0]), np.diff(M.indptr))
    for X, T in ((None, test), (new_train, new_test)):
        ranks = est.ranks(T, X=X)
        assert ranks.dtype == np.int64 and ranks.shape == (T.nnz,) and np.all(ranks >= 0)
        u = user_of(T)
        for N in (1, 10, 128):
            items, _ = est.recommend(X=X, n_items=N)
            inside = np.array([T.indices[e] in items[u[e]] for e in range(T.nnz)])
            np.testing.assert_array_equal(inside, ranks < N)
            hit = np.flatnonzero(ranks < N)
            np.testing.assert_array_equal(items[u[hit], ranks[hit]], T.indices[hit])
        # ranking_score is ranking_metrics of ranks
        seen = (train if X is None else X).toarray() != 0
        n_cand = p - seen.sum(axis=1)
        got = est.ranking_score(T, n_items=10, X=X)
        assert isinstance(got, RankingScore) and got == ranking_metrics(ranks, T.indptr, n_cand, 10)
        assert got.n_users == np.sum(np.diff(T.indptr) > 0) and got.n_targets == T.nnz
        # chunks of 7 queries: the same bits
        np.testing.assert_array_equal(est.ranks(T, X=X, rows_per_call=7), ranks)
        # min_rating selects the targets without changing any other rank
        keep = T.data >= 4
        assert 0 < keep.sum() < T.nnz
        indptr4 = np.concatenate([[0], np.cumsum(keep)])[T.indptr]
        assert est.ranking_score(T, n_items=10, X=X, min_rating=4) == ranking_metrics(ranks[keep], indptr4, n_cand, 10)
        # exclude_seen=False ranks among all p items
        r_all = est.ranks(T, X=X, exclude_seen=False)
        items, _ = est.recommend(X=X, n_items=128, exclude_seen=False)
        hit = np.flatnonzero(r_all < 128)
        assert len(hit) and np.all(r_all >= ranks)
        np.testing.assert_array_equal(items[u[hit], r_all[hit]], T.indices[hit])
        assert est.ranking_score(T, n_items=10, X=X, exclude_seen=False) == ranking_metrics(r_all, T.indptr, np.full(T.shape[0], p), 10)
    # the 150 held-out entries of user 2 (three queries): the ranks of one unchunked reference computation, under `judge`
    ranks = est.ranks(test)
    code = est.code_
    Dt = np.ascontiguousarray(est.components_.T)
    bias = np.asarray(est.col_mean_, dtype=np.float64) if detrend else None
    excl = [train.indices[train.indptr[i]:train.indptr[i + 1]] for i in range(n)]
    rows = [test.indices[test.indptr[i]:test.indptr[i + 1]] for i in range(n)]
    got = [ranks[test.indptr[i]:test.indptr[i + 1]] for i in range(n)]
    moved = judge_ranks(dt, False, 5, code, Dt, excl, bias, rows, 10 ** 6, got)
    print('%s detrend=%s: %d of %d ranks differ from the float64 reference, all inside their band' % (dt, detrend, moved, test.nnz))
