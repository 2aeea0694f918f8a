"""Orthogonal matching pursuit: modl_omp_gram_* (csrc/omp.hip) and modl_somf_transform_omp through the C ABI, then
HipBackend.omp, DictFact / Coder.transform(algorithm='omp') and ImageDictFact.reconstruct / inpaint.  Laid out as
tests/test_recsys_recommend.py:

0. The reference is `omp_ref` below: the loop of csrc/omp.hip's header restated in numpy (any dtype; f64 is the reference,
   f32 the yardstick of the constants below).  `test_reference_matches_sklearn` pins it to orthogonal_mp_gram at 1e-8.
1. CPU tests: `make_rows` builds a batch from NAMED ROW KINDS ('sparse': a noisy combination of three well separated atoms;
   'dup': twice an atom that the dictionary holds twice - the tie rule, then nothing left; 'zero': an all-zero row; 'early':
   one atom and noise far below the threshold; 'late': a dense row that s atoms do not explain; 'tie': atom 0 + atom 1 with
   bitwise equal correlations; 'dense': a random row).  `test_cases_are_what_they_claim` checks that,
   `test_judge_rejects_mutants` that `judge` rejects twelve of thirteen wrong versions of the reference in both dtypes,
   `test_lds_and_workspace` the restated LDS budget and workspace, `test_omp_rejects_on_the_host` the refusals.
2. GPU tests through the ABI, the backend and the estimators.

Acceptance (`judge`) follows the DEVICE's own path: greedy selection forks when two correlations are within rounding, so
the supports are not compared with the reference's and no row is left out.  In f64, per row, with I_t the first t returned
atoms, gamma_t the exact least-squares coefficients on I_t, alpha_t = a0 - G[:, I_t] gamma_t, c_t = cond_2(G[I_t, I_t]),
A_t = max|a0| + max_i sum_j |G[i, I_j]| |gamma_t,j| (the size of the terms alpha_t is summed from; A_t >= 2 max|a0|), eps_T = 2^-23 /
2^-52, u = eps_T / 2:
  coefficients |code[I] - gamma_n| <= slack_coef(n) = C_COEF n eps_T c_n max|gamma_n| (the backward error of a Cholesky solve of
               order n, times the condition number)
  selection    max_{i not in I_t} |alpha_t,i| - |alpha_t,j| <= slack_sel(t) = C_SEL t eps_T c_t A_t for the t-th atom j (t = 0:
               none, alpha is a0 itself) - whenever the maximum is above the NOISE FLOOR floor(t) = (t + 1) u A_t + max_i sum_j
               |G[i, I_j]| slack_coef(t): what a computed alpha_i can be when the true one is zero (the rounding of its t + 1
               terms, and what the error the coefficients are allowed does to it).  At or below the floor every candidate is
               a rounding of zero, in the judge and, differently, on the device, and any pick is accepted (a row that its
               first atoms explain exactly).  An atom that equals the maximum exactly is the lowest index among the tied
               atoms that the kernel cannot tell from it: those with the same a0_i and the same G[I_t, i], bit for bit (a
               copy of an atom, two equal correlations at t = 0); a tie of two roundings in the judge's f64 is none on the
               device
  the rest     code is exactly 0 off the support, support is -1 beyond n_active, no atom twice
  stops        with a threshold the squared residual one step before the last atom, R_{n-1} = xnorm2 - gamma . a0[I], is
               > tol - slack_res (the row had not stopped yet); n < s needs one of: R_n <= tol + slack_res; max|alpha_n| <=
               floor(n) (nothing left); an atom j within slack_sel(n) of the best whose f64 Schur complement d is <= 2 * 16
               eps_T G_jj + (n + 2) u (1 + |w|_1)^2 max G_ii, w = G_II^-1 G_Ij.  The second term is the rounding of the
               kernel's own d = G_jj - w.w: the computed factor is the exact one of G + E with |E_ij| <= (n + 2) u sqrt(G_ii
               G_jj) (Higham, Accuracy and Stability, theorem 10.3), and the Schur complement moves by (1, -w)^T E (1, -w);
               it is a few eps unless atom j leans on the support with large coefficients.  slack_res = 2 (n + 1) eps_T
               (xnorm2 + n max|gamma| A_n) + 2 n slack_coef(n) A_n, the rounding of the n updates of the running residual
               and of the coefficients in them (tol (1 + slack) with slack = slack_res / tol)
With inputs the device formed itself (modl_somf_transform_omp, the masked route) `a_err` / `g_err` bound the elements of Dx and
G against their f64 values (2 p u_T |x| |d|: the dot-product bound), and enter first order: slack_sel += 2 (a_err + g_err
sum|gamma|), floor += a_err + g_err sum|gamma|, slack_coef += 2 |G_II^-1| (sqrt(n) a_err + n g_err |gamma|), the Schur bound
+= g_err (1 + |w|_1)^2.

The constants: DESIGN.md section 15.  C_COEF: the restatement run in the dtype needs 1.51 on the cases of this file and on
the shapes of `test_reference_matches_sklearn` (a one-atom row: a square root and two divisions; in f64 the judge's own
solve rounds as much as the code it judges), rounded up to 2; the device gets four times that, 8, for the other order of its
sums.  C_SEL = 1/2: with A_t >= 2 max|a0| the slack is at least t eps_T c_t max|a0|, the issue's form with c = 1, a little
over four times the 0.19 eps_T max|a0| (2.3e-8) recorded for the f32 restatement; above the floor the restatement of this
file needs 0.016.  `test_constants_hold_for_the_restatement` asserts both at a quarter.  How tight the selection rule is is
pinned by the case 'near' (two correlations 32 eps_T apart on a support of condition 1): noise of 32 eps_T max|a0| on |alpha|
before the arg-max ('noisy_sel') is refused; and the stop rule by 'almost' (a Schur complement of 2048 eps_T): a span test
that fires 1024 times too early ('eager_span') is refused.  The GPU tests print the largest error / bound ratio.

Of the thirteen mutants one, 'no_exclusion', survives on every case of this file and is listed as such (`INVISIBLE`): the
least-squares fit makes alpha vanish on the support, so an arg-max that does not exclude the support picks a selected atom
only when every other correlation is below the rounding of alpha, and then the span test (d = rounding) stops the row where
a correct kernel may stop as well ('nothing left').  On an ill-conditioned support that rounding is cond eps and could pass
the span test, and the repeat would then be caught by the no-repeats rule; no such case was found (30 seeds of 'beyond'
shapes, both dtypes).  `test_judge_rejects_mutants` asserts what the mutant does on the cases here: the same atoms, fewer.

There is no route by k or by s in csrc/omp.hip: one kernel, four samples per workgroup, LDS = 4 s (s - 1) / 2 elements
(`omp_lds` restates it; at most 63 KiB).  modl_omp_workspace is 0 for every call, so there is no "workspace one byte
short" to refuse; the NULL workspace is what a valid call passes.
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.linalg as sla

from modl_amd._lib import OMP_MAX_NONZERO

DT = {'f32': np.float32, 'f64': np.float64}
U = {'f32': 2.0 ** -24, 'f64': 2.0 ** -53}
EINVAL, ENOMEM, ENOGPU = -1, -2, -4
MAX_COMPONENTS, MAX_COMPONENTS_MULTI, WAVES = 4096, 1024, 4
C_SEL, C_COEF = 0.5, 8.0
LDS_BYTES = 64 * 1024


def omp_lds(dt, s):
    """omp_lds_bytes: the strictly lower triangle of L for each of the four samples of a workgroup"""
    return (4 if dt == 'f32' else 8) * WAVES * (s * (s - 1) // 2)


# ---------------------------------------------------------------------------------------------------- the reference
MUTANTS = ('signed', 'no_exclusion', 'ties_high', 'no_schur', 'forward_only', 'stale_gamma', 'no_delta_prev', 'stop_after',
           'support_unordered', 'stale_code', 'row0_gram', 'noisy_sel', 'eager_span')
NOISE_EPS, EAGER = 32, 1024      # 'noisy_sel': |alpha| + up to 32 eps_T max|a0| before the arg-max; 'eager_span': 1024 x the threshold


def omp_ref(G, a0, xn, s, tol, T=np.float64, mutant=None):
    """one row: (code (k,), support (s,) int, n_active); arithmetic in T.  `mutant`: one thing wrong."""
    G, a0 = np.asarray(G, dtype=T), np.asarray(a0, dtype=T)
    k = a0.shape[0]
    eps = T(np.finfo(T).eps)
    L = np.zeros((s, s), dtype=T)
    I = []
    alpha = a0.copy()
    gamma = np.zeros(0, dtype=T)
    eps_res = T(xn) if tol is not None else T(0)
    delta_prev = T(0)
    for t in range(s):
        pending = tol is not None and eps_res <= T(tol)
        if pending and mutant != 'stop_after':
            break
        cand = alpha.copy() if mutant == 'signed' else np.abs(alpha)
        if mutant == 'noisy_sel':
            cand = cand + T(NOISE_EPS) * eps * np.max(np.abs(a0)) * np.random.RandomState(t + 7).rand(k).astype(T)
        if mutant != 'no_exclusion':
            cand[I] = -np.inf
        j = int(k - 1 - np.argmax(cand[::-1])) if mutant == 'ties_high' else int(np.argmax(cand))
        if not abs(alpha[j]) > 0:
            break
        if t > 0:
            w = sla.solve_triangular(L[:t, :t], G[I, j], lower=True, check_finite=False).astype(T)
            d = G[j, j] - w.dot(w)
            if not (G[j, j] > 0 and d > T(16 * (EAGER if mutant == 'eager_span' else 1)) * eps * G[j, j]):
                break
            L[t, :t] = w
            L[t, t] = np.sqrt(G[j, j] if mutant == 'no_schur' else d)
        else:
            if not G[j, j] > 0:
                break
            L[0, 0] = np.sqrt(G[j, j])
        I.append(j)
        y = sla.solve_triangular(L[:t + 1, :t + 1], a0[I], lower=True, check_finite=False).astype(T)
        new = y if mutant == 'forward_only' else \
            sla.solve_triangular(L[:t + 1, :t + 1].T, y, lower=False, check_finite=False).astype(T)
        used = np.concatenate([gamma, np.zeros(1, dtype=T)]) if mutant == 'stale_gamma' else new
        beta = G[:, I].dot(used).astype(T)
        alpha = a0 - beta
        gamma = new
        delta = gamma.dot(beta[I])
        eps_res = eps_res - delta + (T(0) if mutant == 'no_delta_prev' else delta_prev)
        delta_prev = delta
        if pending:
            break
    code = np.zeros(k, dtype=T)
    code[I] = gamma
    support = np.full(s, -1, dtype=np.int64)
    support[:len(I)] = I
    return code, support, len(I)


def omp_batch(G, Dx, xn, s, tol, T=np.float64, mutant=None):
    """the rows of a call: G (k, k) shared or (b, k, k) one per row"""
    b, k = Dx.shape
    code, support, n = np.zeros((b, k), dtype=T), np.full((b, s), -1, dtype=np.int64), np.zeros(b, dtype=np.int64)
    row_mut = mutant if mutant not in ('support_unordered', 'stale_code', 'row0_gram') else None
    for i in range(b):
        Gi = G if G.ndim == 2 else G[0 if mutant == 'row0_gram' else i]
        code[i], support[i], n[i] = omp_ref(Gi, Dx[i], None if xn is None else xn[i], s, tol, T, row_mut)
        if mutant == 'support_unordered':
            support[i, :n[i]] = np.sort(support[i, :n[i]])
        if mutant == 'stale_code' and n[i] < k:
            code[i, np.setdiff1d(np.arange(k), support[i, :n[i]])[-1]] = 1e-3
    return code, support, n


INVISIBLE = ('no_exclusion',)     # (module docstring)


# ---------------------------------------------------------------------------------------------------- the acceptance rule
def judge(c, code, support, n_active, a_err=0.0, g_err=0.0, csel=C_SEL, ccoef=C_COEF):
    """the rules of the module docstring for what a call on case c returned; the largest (selection shortfall / slack_sel
    over the picks made above the noise floor, coefficient error / slack_coef) over the rows"""
    eps = float(np.finfo(DT[c.dt]).eps)
    u = eps / 2
    G_all, Dx = np.asarray(c.G, dtype=np.float64), np.asarray(c.Dx, dtype=np.float64)
    b, k = Dx.shape
    s, tol = c.s, c.tol
    code, support, n_active = np.asarray(code, dtype=np.float64), np.asarray(support).astype(np.int64), np.asarray(n_active)
    assert code.shape == (b, k) and support.shape == (b, s) and n_active.shape == (b,)
    worst_sel = worst_coef = 0.0

    def state(G, a0, I):
        """(gamma, alpha, cond, A, |G_II^-1|, slack_sel, noise floor) of the exact least-squares fit on I"""
        if not len(I):
            return np.zeros(0), a0.copy(), 1.0, float(np.max(np.abs(a0))), 0.0, 2 * a_err, a_err
        GII = G[np.ix_(I, I)]
        gamma = np.linalg.lstsq(GII, a0[I], rcond=None)[0]
        sv = np.linalg.svd(GII, compute_uv=False)
        cond = float(sv[0] / max(sv[-1], 1e-300))
        A = float(np.max(np.abs(a0)) + np.max(np.abs(G[:, I]).dot(np.abs(gamma))))
        t = len(I)
        formed = a_err + g_err * float(np.sum(np.abs(gamma)))
        sel = csel * t * eps * cond * A + 2 * formed
        row1 = float(np.max(np.sum(np.abs(G[:, I]), axis=1)))
        floor = (t + 1) * u * A + row1 * ccoef * t * eps * cond * float(np.max(np.abs(gamma))) + formed
        return gamma, a0 - G[:, I].dot(gamma), cond, A, 1.0 / max(sv[-1], 1e-300), sel, floor

    for i in range(b):
        G = G_all if G_all.ndim == 2 else G_all[i]
        a0 = Dx[i]
        n = int(n_active[i])
        assert 0 <= n <= s, ('n_active out of range', i, n)
        I = list(support[i, :n])
        assert np.all(support[i, n:] == -1), ('support beyond n_active is not -1', i)
        assert all(0 <= j < k for j in I) and len(set(I)) == n, ('support out of range or repeated', i, I)
        off = np.ones(k, dtype=bool)
        off[I] = False
        assert np.all(code[i, off] == 0), ('non-zero off the support', i)
        res_prev = None
        for t in range(n + 1):
            gamma, alpha, cond, A, inv, slack, floor = state(G, a0, I[:t])
            cand = np.abs(alpha)
            cand[I[:t]] = -np.inf
            top = float(np.max(cand)) if t < k else 0.0
            if t < n:
                j = I[t]
                short = top - cand[j]
                if top > floor:                                     # (below it the pick is among roundings of zero: any will do)
                    assert short <= slack, ('selection', i, t, j, short, slack)
                    if slack > 0:
                        worst_sel = max(worst_sel, short / slack)
                if short == 0:                                      # the tied atoms whose inputs are j's own, bit for bit
                    same = [q for q in np.flatnonzero(cand == top)
                            if a0[q] == a0[j] and np.array_equal(G[I[:t], q], G[I[:t], j])]
                    assert j == min(same), ('an exact tie did not go to the lowest index', i, t, j, same)
                if tol is not None:
                    res_prev = float(c.xn[i]) - gamma.dot(a0[I[:t]])
        if n:
            bound = ccoef * n * eps * cond * np.max(np.abs(gamma)) + \
                2 * inv * (np.sqrt(n) * a_err + n * g_err * np.linalg.norm(gamma))
            err = float(np.max(np.abs(code[i, I] - gamma)))
            assert err <= bound, ('coefficients', i, err, bound)
            worst_coef = max(worst_coef, err / bound)
        gmax = float(np.max(np.abs(gamma))) if n else 0.0
        xn = float(c.xn[i]) if tol is not None else 0.0
        dgam = ccoef * n * eps * cond * gmax
        slack_res = 2 * (n + 1) * eps * (abs(xn) + n * gmax * A) + 2 * n * dgam * A + \
            2 * (a_err * np.sum(np.abs(gamma)) if n else 0.0)
        if tol is not None and n:
            assert res_prev > tol - slack_res, ('the row went on after reaching the threshold', i, res_prev, tol)
        if n < s:
            reasons = []
            if tol is not None:
                reasons.append(xn - gamma.dot(a0[I]) <= tol + slack_res)
            reasons.append(top <= floor or n == k)
            for j in np.flatnonzero(cand >= top - slack):
                if G[j, j] <= 0:
                    reasons.append(True)
                elif n:
                    w = np.linalg.lstsq(G[np.ix_(I, I)], G[I, j], rcond=None)[0]
                    d = G[j, j] - G[I, j].dot(w)
                    gm = float(max(np.max(np.diag(G)[I]), G[j, j]))
                    q2 = (1 + float(np.sum(np.abs(w)))) ** 2
                    reasons.append(d <= 32 * eps * G[j, j] + ((n + 2) * u * gm + g_err) * q2)
            assert any(reasons), ('stop without a reason', i, n, top, slack, floor)
    return worst_sel, worst_coef


def accepts(c, code, support, n_active, **kw):
    try:
        judge(c, code, support, n_active, **kw)
    except AssertionError:
        return False
    return True


# ---------------------------------------------------------------------------------------------------- the builders
KINDS = ('sparse', 'dup', 'zero', 'early', 'late', 'tie', 'dense')
DUP = (2, 5)                     # atom DUP[1] is a copy of atom DUP[0] (dictionaries of at least 8 atoms)


def unit_dictionary(rs, k, p, smooth=False, signs=False):
    """random unit-norm atoms; signs: the p basis vectors, then random sign vectors (every p independent atoms are well
    conditioned, so a Schur complement that is zero is computed as a few eps)"""
    D = rs.randn(k, p)
    if signs:
        D = np.sign(D)
        D[:p] = np.eye(p)
    if smooth:
        D = np.cumsum(D, axis=1)
    if k >= 8:
        D[DUP[1]] = D[DUP[0]]
    return D / np.linalg.norm(D, axis=1)[:, None]


def make_rows(dt, k, p, b, s, seed, tol=None, kinds=KINDS, per_row=False, signs=False):
    """One call: a unit-norm dictionary (atom 5 = atom 2 when k >= 8), b rows of the kinds in turn (kinds a dictionary of
    fewer than 8 atoms cannot hold become 'dense'), G, Dx and the squared norms rounded to the dtype ONCE: they are the
    call's inputs, for the device and for the judge alike.  per_row: every row sees its own random half of the features,
    G_i = r D_S D_S^T, Dx_i = r x_S D_S^T, xn_i = r |x_S|^2 (the masked route's inputs)."""
    rs = np.random.RandomState(seed)
    T = DT[dt]
    D = unit_dictionary(rs, k, p, signs=signs)
    X = np.zeros((b, p))
    names = []
    for i in range(b):
        kd = kinds[i % len(kinds)]
        if k < 8 and kd not in ('zero', 'dense'):
            kd = 'dense'
        free = np.setdiff1d(np.arange(k), DUP + (0, 1))
        if kd == 'sparse':
            at = rs.choice(free, 3, replace=False)
            X[i] = np.array([3.0, -2.0, 1.2]).dot(D[at]) + 1e-3 * rs.randn(p)
        elif kd == 'dup':
            X[i] = 2.0 * D[DUP[0]]
        elif kd == 'early':
            X[i] = -1.5 * D[rs.choice(free)] + 1e-4 * rs.randn(p)
        elif kd == 'late':
            X[i] = 5.0 * rs.randn(p)
        elif kd == 'tie':
            X[i] = D[0] + D[1]
        elif kd == 'dense':
            X[i] = rs.randn(p)
        names.append(kd)
    if per_row:
        obs = rs.rand(b, p) < 0.5
        obs[:, :2] = True
        r = p / obs.sum(axis=1)
        G = np.stack([r[i] * (D * obs[i]).dot((D * obs[i]).T) for i in range(b)])
        Dx = np.stack([r[i] * (X[i] * obs[i]).dot((D * obs[i]).T) for i in range(b)])
        xn = r * np.sum((X * obs) ** 2, axis=1)
    else:
        G, Dx, xn = D.dot(D.T), X.dot(D.T), np.sum(X ** 2, axis=1)
        G = 0.5 * (G + G.T)
    for i, kd in enumerate(names):
        if kd == 'tie':
            Dx[i, 1] = Dx[i, 0]                                     # 1 + d0.d1 both: equal bit for bit
    if k >= 8:                                                      # the copy is one: its row, its column and its correlations
        G[..., DUP[1], :] = G[..., DUP[0], :]
        G[..., :, DUP[1]] = G[..., :, DUP[0]]
        Dx[:, DUP[1]] = Dx[:, DUP[0]]
    return SimpleNamespace(dt=dt, k=k, p=p, b=b, s=s, tol=tol, kinds=names, D=D, X=X,
                           G=np.ascontiguousarray(G.astype(T)), Dx=np.ascontiguousarray(Dx.astype(T)),
                           xn=np.ascontiguousarray(xn.astype(T)), per_row=per_row)


def _case(dt, D, X, s, kinds):
    T = DT[dt]
    G, Dx, xn = D.dot(D.T), X.dot(D.T), np.sum(X ** 2, axis=1)
    return SimpleNamespace(dt=dt, k=D.shape[0], p=D.shape[1], b=X.shape[0], s=s, tol=None, kinds=kinds, D=D, X=X,
                           G=np.ascontiguousarray((0.5 * (G + G.T)).astype(T)), Dx=np.ascontiguousarray(Dx.astype(T)),
                           xn=np.ascontiguousarray(xn.astype(T)), per_row=False)


NEAR_GAP = 16                    # 'near': the third atom's correlation is (1 - 16 eps_T) times the second's


def make_near(dt, b=12):
    """'near': the floor under the selection slack.  64 basis vectors and 16 sign vectors; row i = 6 e_a + 2 e_b + 2 (1 - 16
    eps_T) e_c with c < b: after e_a (conditioning 1, every product exact) the two correlations differ by 32 eps_T, five
    times the slack C_SEL eps_T A_1 = 6 eps_T: taking e_c first is refused, and so is selection noise of a few tens of eps"""
    rs = np.random.RandomState(5)
    D = np.concatenate([np.eye(64), np.sign(rs.randn(16, 64)) / 8.0])
    X = np.zeros((b, 64))
    for i in range(b):
        a, hi, lo = 3 * i + 2, 3 * i + 1, 3 * i
        X[i, a], X[i, hi], X[i, lo] = 6.0, 2.0, 2.0 * (1 - NEAR_GAP * float(np.finfo(DT[dt]).eps))
    return _case(dt, D, X, 3, ['near'] * b)


ALMOST_D = 2048                  # 'almost': the Schur complement of the second atom is 2048 eps_T


def make_almost(dt):
    """'almost': atom 1 = cos e_0 + sin e_1 with sin^2 = 2048 eps_T, no atom e_1; rows in the plane of e_0 and e_1.  After
    either of the two atoms the other is the only candidate and its Schur complement, 2048 eps_T, is 128 times the
    threshold: the row must go on; a span test that fires 1024 times too early stops it at one atom"""
    sin2 = ALMOST_D * float(np.finfo(DT[dt]).eps)
    D = np.eye(8)
    D[1] = 0
    D[1, 0], D[1, 1] = np.sqrt(1 - sin2), np.sqrt(sin2)
    X = np.zeros((3, 8))
    X[:, :2] = [[3.0, 1.0], [-2.0, 1.5], [1.0, 1.0]]
    return _case(dt, D, X, 2, ['almost'] * 3)


def case_reference(c, mutant=None, T=np.float64):
    return omp_batch(c.G, c.Dx, c.xn if c.tol is not None else None, c.s, c.tol, T, mutant)


def cpu_cases(dt):
    """'count': every kind, s = 6 atoms of 24 features; 'threshold': the same with a squared-residual threshold; 'beyond':
    s = 8 > p = 4 on an over-complete dictionary of basis and sign vectors; 'per_row': a Gram matrix per row"""
    return {'count': make_rows(dt, 40, 24, 14, 6, 1), 'threshold': make_rows(dt, 40, 24, 14, 6, 2, tol=1e-2),
            'beyond': make_rows(dt, 40, 4, 7, 8, 3, kinds=('dense', 'sparse'), signs=True),
            'per_row': make_rows(dt, 40, 24, 9, 5, 4, tol=1e-2, per_row=True), 'near': make_near(dt), 'almost': make_almost(dt)}


# ---------------------------------------------------------------------------------------------------- layer 1: CPU tests
SKLEARN_SHAPES = ((256, 64, 8, False), (256, 64, 32, False), (1024, 192, 16, False), (64, 64, 64, False),
                  (65, 16, 16, False), (100, 64, 10, True))


def sklearn_case(k, p, s, smooth, seed=1, b=4):
    rs = np.random.RandomState(seed)
    D = rs.randn(k, p)
    if smooth:
        D = np.cumsum(D, axis=1)
    D /= np.linalg.norm(D, axis=1)[:, None]
    Cs = np.zeros((b, k))                                           # s atoms with normal coefficients, and a little noise
    for i in range(b):
        Cs[i, rs.choice(k, s, replace=False)] = rs.randn(s)
    X = Cs.dot(D) + 0.01 * rs.randn(b, p)
    return D.dot(D.T), X.dot(D.T), np.sum(X ** 2, axis=1)


@pytest.mark.parametrize('k,p,s,smooth', SKLEARN_SHAPES)
def test_reference_matches_sklearn(k, p, s, smooth):
    """the f64 restatement against scikit-learn's orthogonal_mp_gram, by count and by threshold: 1e-8 absolute on the codes
    (well-conditioned draws: seed 1; the 64 x 64 dictionary of seed 0 has cond(G) = 1e8 and two f64 Cholesky solves differ by
    1.8e-8 on it)"""
    from sklearn.linear_model import orthogonal_mp_gram
    G, Dx, xn = sklearn_case(k, p, s, smooth)
    want = orthogonal_mp_gram(G, Dx.T, n_nonzero_coefs=s).T
    got = omp_batch(G, Dx, None, s, None)[0]
    assert np.max(np.abs(got - want)) <= 1e-8
    tol = 0.25 * float(np.min(xn))
    smax = min(k, OMP_MAX_NONZERO)
    want = orthogonal_mp_gram(G, Dx.T, tol=tol, norms_squared=xn).T
    got, _, n = omp_batch(G, Dx, xn, smax, tol)
    assert np.max(np.count_nonzero(want, axis=1)) <= smax and np.all(n >= 1)
    assert np.max(np.abs(got - want)) <= 1e-8


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_judge_rejects_mutants(dt):
    """`judge` accepts the reference (run in the dtype: what a correct device computes) on every case and rejects each wrong
    version of it on the named case"""
    cases = cpu_cases(dt)
    for c in cases.values():
        assert accepts(c, *case_reference(c, T=DT[dt]))
        assert accepts(c, *case_reference(c))
    where = dict(signed='count', no_exclusion='beyond', ties_high='count', no_schur='count', forward_only='count',
                 stale_gamma='count', no_delta_prev='threshold', stop_after='threshold', support_unordered='count',
                 stale_code='count', row0_gram='per_row', noisy_sel='near', eager_span='almost')
    assert set(where) == set(MUTANTS) and len(MUTANTS) == 13
    survivors = [m for m in MUTANTS if accepts(cases[where[m]], *case_reference(cases[where[m]], m, T=DT[dt]))]
    assert survivors == list(INVISIBLE), survivors
    for c in cases.values():                                        # all 'no_exclusion' ever does: the same atoms, fewer of them
        ref, mut = case_reference(c, T=DT[dt]), case_reference(c, 'no_exclusion', T=DT[dt])
        for i in range(c.b):
            assert mut[2][i] <= ref[2][i] and np.array_equal(mut[1][i, :mut[2][i]], ref[1][i, :mut[2][i]])


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_cases_are_what_they_claim(dt):
    cases = cpu_cases(dt)
    for name in ('count', 'threshold'):
        c = cases[name]
        assert set(c.kinds) == set(KINDS) and c.G.dtype == DT[dt] and c.s <= c.p
        code, support, n = case_reference(c)
        G = c.G.astype(np.float64)
        assert np.array_equal(G[DUP[0]], G[DUP[1]]) and np.array_equal(c.Dx[:, DUP[0]], c.Dx[:, DUP[1]])
        for i, kd in enumerate(c.kinds):
            I = list(support[i, :n[i]])
            if kd == 'zero':
                assert n[i] == 0 and not np.any(c.Dx[i])
            if kd == 'dup':                                         # the tie goes to the lower copy, then nothing is left
                assert I[0] == DUP[0] and DUP[1] not in I and n[i] < c.s
            if kd == 'tie':
                rest = np.delete(code[i], [0, 1])                   # both atoms, the lower first; what follows fits rounding
                assert c.Dx[i, 0] == c.Dx[i, 1] and I[:2] == [0, 1] and np.max(np.abs(rest)) < 1e-5
                assert c.tol is None or n[i] == 2
            if kd == 'sparse':
                assert n[i] >= 3 and abs(abs(code[i, I[0]]) - 3) < 0.1 and code[i, I[1]] < 0
            if c.tol is not None:
                if kd == 'early':
                    assert n[i] == 1
                if kd == 'late':
                    assert n[i] == c.s and float(c.xn[i]) - code[i, I].dot(c.Dx[i, I].astype(np.float64)) > 10 * c.tol
                if kd == 'sparse':
                    assert n[i] == 3
        if c.tol is not None:
            assert len(set(n[:WAVES])) >= 3                        # n_active differs inside the first workgroup
    c = cases['beyond']
    n = case_reference(c)[2]
    assert c.s > c.p and np.all(n <= c.p) and np.any(n == c.p)      # dependence stops the row at or before p
    n32 = case_reference(c, T=np.float32)[2]
    assert np.all(n32 <= c.p)
    c = cases['per_row']
    assert c.G.ndim == 3 and not np.allclose(c.G[0], c.G[1])
    c = cases['near']
    eps = float(np.finfo(DT[dt]).eps)
    for T in (np.float64, DT[dt]):
        sup = case_reference(c, T=T)[1]
        assert all(list(sup[i]) == [3 * i + 2, 3 * i + 1, 3 * i] for i in range(c.b))
    gap = c.Dx[:, 1::3][np.arange(c.b), np.arange(c.b)].astype(np.float64) - c.Dx[:, 0::3][np.arange(c.b), np.arange(c.b)]
    assert np.all(gap == 2 * NEAR_GAP * eps) and 2 * NEAR_GAP * eps > 5 * C_SEL * eps * 12
    assert np.any(case_reference(c, 'noisy_sel', T=DT[dt])[1] != sup)
    c = cases['almost']
    G = c.G.astype(np.float64)
    d = 1 - G[0, 1] ** 2
    assert abs(d / eps - ALMOST_D) < 2 and 16 * eps < d < 16 * EAGER * eps
    assert np.all(case_reference(c, T=DT[dt])[2] == 2) and np.all(case_reference(c)[2] == 2)
    assert np.all(case_reference(c, 'eager_span', T=DT[dt])[2] == 1)


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_constants_hold_for_the_restatement(dt):
    """the restatement in the dtype stays within the bounds of a QUARTER of the device's constants (C_SEL / 4, C_COEF / 4) on every case of
    this file and on the shapes of the scikit-learn check: where the constants come from"""
    todo = list(cpu_cases(dt).values())
    for k, p, s, smooth in SKLEARN_SHAPES:
        G, Dx, xn = sklearn_case(k, p, s, smooth, seed=2, b=3)
        T = DT[dt]
        todo.append(SimpleNamespace(dt=dt, k=k, p=p, b=3, s=s, tol=None, G=G.astype(T), Dx=Dx.astype(T), xn=xn.astype(T)))
    worst = [0.0, 0.0]
    for c in todo:
        ws, wc = judge(c, *case_reference(c, T=DT[dt]), csel=C_SEL / 4, ccoef=C_COEF / 4)
        worst = [max(worst[0], ws), max(worst[1], wc)]
    print('%s restatement: selection %.3g, coefficients %.3g of a quarter of the bound' % (dt, worst[0], worst[1]))


def test_lds_and_workspace():
    from modl_amd._lib import lib
    assert OMP_MAX_NONZERO == 64 and lib.modl_max_components() == MAX_COMPONENTS
    for dt in ('f32', 'f64'):
        assert omp_lds(dt, 1) == 0 and max(omp_lds(dt, s) for s in range(1, OMP_MAX_NONZERO + 1)) <= LDS_BYTES
        for args in ((1, 1, 1, 0), (33, 256, 8, 0), (33, 256, 8, 1), (9, 4096, 64, 0), (0, 5, 2, 0), (3, 5, 65, 0)):
            assert lib.modl_omp_workspace(0 if dt == 'f32' else 1, *args) == 0
    assert omp_lds('f64', 64) == 64512


def _hp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


REFUSALS = (dict(G=None), dict(Dx=None), dict(code=None), dict(support=None), dict(n_active=None), dict(b=-1), dict(k=0),
            dict(s=0), dict(s=OMP_MAX_NONZERO + 1, k=200), dict(s=6, k=5), dict(tol=0.5, xn=None), dict(g_stride=7),
            dict(g_stride=25, k=6), dict(k=MAX_COMPONENTS + 1), dict(k=MAX_COMPONENTS_MULTI + 1, multi=True))


def test_omp_rejects_on_the_host():
    """the argument checks come before any device work: they answer without a device (host buffers stand in for device ones;
    nothing reads them)"""
    from modl_amd._lib import lib
    for dt in ('f32', 'f64'):
        f = getattr(lib, 'modl_omp_gram_' + dt)
        a = np.zeros(64, dtype=DT[dt])
        i = np.zeros(64, dtype=np.int32)

        def call(G=a, g_stride=0, Dx=a, xn=a, b=2, k=5, s=2, tol=-1.0, code=a, support=i, n_active=i, multi=False):
            if multi:
                g_stride = k * k
            return f(_hp(G), g_stride, _hp(Dx), _hp(xn), b, k, s, tol, _hp(code), _hp(support), _hp(n_active), None, 0, None)
        for kw in REFUSALS:
            assert call(**kw) == EINVAL, kw
        assert call(b=0) == 0 and call(b=0, xn=None) == 0
        if lib.modl_device_count() == 0:
            assert call() == ENOGPU and call(g_stride=25) == ENOGPU and call(tol=float('nan'), xn=None) == ENOGPU


def test_transform_arguments():
    """the ValueError cases of transform(algorithm=...) are decided before anything touches the device"""
    from modl_amd.dict_fact import CodingMixin
    m = CodingMixin()
    m.n_components = 256
    assert m._omp_params('enet', None, None) is None
    assert m._omp_params('omp', None, None) == (25, None) and m._omp_params('omp', None, 0.5) == (64, 0.5)
    assert m._omp_params('omp', 7, 0.0) == (7, 0.0)
    m.n_components = 5
    assert m._omp_params('omp', None, None) == (1, None) and m._omp_params('omp', None, 1.0) == (5, 1.0)
    m.n_components = 2000
    assert m._omp_params('omp', None, None) == (64, None)
    for args, word in ((('lasso', None, None), 'enet'), (('enet', 3, None), 'omp'), (('enet', None, 1.0), 'omp'),
                       (('omp', 0, None), '64'), (('omp', 65, None), '64'), (('omp', 2.5, None), '64'),
                       (('omp', None, -1.0), '>= 0'), (('omp', None, float('nan')), '>= 0')):
        with pytest.raises(ValueError, match=word):
            m._omp_params(*args)
    m.n_components = 5
    with pytest.raises(ValueError, match='n_components = 5'):
        m._omp_params('omp', 6, None)


# ---------------------------------------------------------------------------------------------------- layer 2: GPU tests
@pytest.fixture(scope='module')
def gpu():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    return torch


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to('cuda')


PAD = 2                          # sentinel rows in front of and behind every output


def run_omp(c):
    """one call of modl_omp_gram_* on case c; returns (rc, code, support, n_active) and asserts that the rows around the
    outputs are untouched"""
    import torch
    from modl_amd._lib import lib
    from modl_amd.device import ptr
    T = DT[c.dt]
    code0 = np.full((c.b + 2 * PAD, c.k), 12345.0, dtype=T)
    sup0 = np.full((c.b + 2 * PAD, c.s), -77, dtype=np.int32)
    na0 = np.full(c.b + 2 * PAD, -77, dtype=np.int32)
    d_code, d_sup, d_na = _dev(code0), _dev(sup0), _dev(na0)
    G, Dx, xn = _dev(c.G), _dev(c.Dx), _dev(c.xn) if c.tol is not None else None
    need = lib.modl_omp_workspace(0 if c.dt == 'f32' else 1, c.b, c.k, c.s, int(c.G.ndim == 3))
    assert need == 0
    rc = getattr(lib, 'modl_omp_gram_' + c.dt)(ptr(G), c.k * c.k if c.G.ndim == 3 else 0, ptr(Dx), ptr(xn), c.b, c.k, c.s,
                                               -1.0 if c.tol is None else c.tol, ptr(d_code[PAD:]), ptr(d_sup[PAD:]),
                                               ptr(d_na[PAD:]), None, 0, None)
    torch.cuda.synchronize()
    code, sup, na = d_code.cpu().numpy(), d_sup.cpu().numpy(), d_na.cpu().numpy()
    for got, was in ((code, code0), (sup, sup0), (na, na0)):
        np.testing.assert_array_equal(got[:PAD], was[:PAD], err_msg='rows in front of an output changed')
        np.testing.assert_array_equal(got[c.b + PAD:], was[c.b + PAD:], err_msg='rows behind an output changed')
    return rc, code[PAD:c.b + PAD], sup[PAD:c.b + PAD], na[PAD:c.b + PAD]


# (k, s, b, p): b is never a multiple of the four samples of a workgroup; (1088, 4, 3): beyond 1024 atoms; there is no route
# boundary to add
ABI_SHAPES = ((1, 1, 1, 3), (65, 16, 7, 24), (64, 64, 5, 64), (256, 8, 33, 32), (1024, 16, 9, 48), (1088, 4, 3, 32))
ABI_PER_ROW = ((65, 16, 7, 40), (256, 8, 33, 32))


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'f64'])
@pytest.mark.parametrize('k,s,b,p', ABI_SHAPES, ids=['k%d-s%d-b%d' % c[:3] for c in ABI_SHAPES])
def test_omp_abi(gpu, dt, k, s, b, p):
    c = make_rows(dt, k, p, b, s, 100 + k)
    rc, code, sup, na = run_omp(c)
    assert rc == 0
    ws, wc = judge(c, code, sup, na)
    print('%s k=%d s=%d: selection %.3g, coefficients %.3g of the bound' % (dt, k, s, ws, wc))
    assert np.all(np.count_nonzero(code, axis=1) <= s)


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'f64'])
@pytest.mark.parametrize('k,s,b,p', ABI_PER_ROW, ids=['k%d-s%d-b%d' % c[:3] for c in ABI_PER_ROW])
def test_omp_abi_per_row_gram(gpu, dt, k, s, b, p):
    c = make_rows(dt, k, p, b, s, 200 + k, per_row=True)
    rc, code, sup, na = run_omp(c)
    assert rc == 0
    ws, wc = judge(c, code, sup, na)
    print('%s per-row k=%d s=%d: selection %.3g, coefficients %.3g of the bound' % (dt, k, s, ws, wc))
    assert not accepts(c, *case_reference(c, 'row0_gram'))


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_omp_threshold(gpu, dt):
    """the mixed batches with a threshold, shared and per-row: n_active differs from row to row inside a workgroup"""
    for name in ('threshold', 'per_row', 'count', 'beyond', 'near', 'almost'):
        c = cpu_cases(dt)[name]
        rc, code, sup, na = run_omp(c)
        assert rc == 0
        ws, wc = judge(c, code, sup, na)
        print('%s %s: selection %.3g, coefficients %.3g of the bound' % (dt, name, ws, wc))
        if name == 'threshold':
            assert len(set(na[:WAVES])) >= 3 and na[c.kinds.index('zero')] == 0 and na[c.kinds.index('early')] == 1
            assert na[c.kinds.index('late')] == c.s
        if name == 'near':                                          # the closer of two correlations 32 eps_T apart comes second
            assert all(list(sup[i]) == [3 * i + 2, 3 * i + 1, 3 * i] for i in range(c.b))
        if name == 'almost':                                        # a Schur complement of 2048 eps_T does not stop the row
            assert np.all(na == 2)


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_omp_refusals(gpu, dt):
    """every refusal returns its code and writes nothing (the outputs keep their sentinel), and the valid call behind it on
    the same stream runs"""
    import torch
    from modl_amd._lib import lib
    from modl_amd.device import ptr
    T = DT[dt]
    c = make_rows(dt, 40, 24, 5, 6, 7, tol=1e-2)
    f = getattr(lib, 'modl_omp_gram_' + dt)
    kbig = MAX_COMPONENTS + 1
    big = _dev(np.zeros((2, kbig), dtype=T))
    base = dict(G=_dev(c.G), g_stride=0, Dx=_dev(c.Dx), xn=_dev(c.xn), b=c.b, k=c.k, s=c.s, tol=c.tol)
    code0, sup0 = np.full((c.b, kbig), 12345.0, dtype=T), np.full((c.b, OMP_MAX_NONZERO + 1), -77, dtype=np.int32)
    na0 = np.full(c.b, -77, dtype=np.int32)
    good = None
    for kw in REFUSALS + (dict(s=c.k + 1),):
        a = dict(base, code=_dev(code0), support=_dev(sup0), n_active=_dev(na0))
        kw = dict(kw)
        if kw.pop('multi', False):
            kw['g_stride'] = kw['k'] * kw['k']
        a.update(kw)
        if a['k'] > c.k and a['G'] is not None:
            a['G'] = a['Dx'] = big                                  # (never read: the call is refused on the host)
        rc = f(ptr(a['G']), a['g_stride'], ptr(a['Dx']), ptr(a['xn']), a['b'], a['k'], a['s'], a['tol'], ptr(a['code']),
               ptr(a['support']), ptr(a['n_active']), None, 0, None)
        assert rc == EINVAL, (kw, rc)
        rc2, code, sup, na = run_omp(c)
        assert rc2 == 0
        torch.cuda.synchronize()
        for name, was in (('code', code0), ('support', sup0), ('n_active', na0)):
            if a[name] is not None:
                np.testing.assert_array_equal(a[name].cpu().numpy(), was)
        if good is None:
            judge(c, code, sup, na)
            good = (code, sup, na)
        for x, y in zip(good, (code, sup, na)):
            np.testing.assert_array_equal(x, y)
    # the last values that are not refused run: s = 64 = k, and k = 1
    for k, s, p in ((64, OMP_MAX_NONZERO, 64), (1, 1, 2)):
        c2 = make_rows(dt, k, p, 3, s, 8)
        rc, code, sup, na = run_omp(c2)
        assert rc == 0
        judge(c2, code, sup, na)


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_omp_is_repeatable(gpu, dt):
    """two calls give the same bits; a row alone gives the bits it gives inside a batch"""
    for c in (make_rows(dt, 256, 32, 33, 8, 11, tol=1e-3), make_rows(dt, 65, 40, 7, 16, 12, per_row=True)):
        one = run_omp(c)
        two = run_omp(c)
        assert one[0] == two[0] == 0
        for x, y in zip(one[1:], two[1:]):
            np.testing.assert_array_equal(x, y)
        for i in (0, 3, c.b - 1):
            ci = SimpleNamespace(**vars(c))
            ci.b, ci.Dx, ci.xn = 1, c.Dx[i:i + 1], c.xn[i:i + 1]
            ci.G = c.G[i:i + 1] if c.G.ndim == 3 else c.G
            alone = run_omp(ci)
            assert alone[0] == 0
            for x, y in zip(one[1:], alone[1:]):
                np.testing.assert_array_equal(x[i:i + 1], y)


def data_case(dt, k, p, n, s, seed, tol=None, obs=None):
    """rows and a dictionary in the dtype, and the judge's inputs recomputed from them in f64 (with obs: per row, on its
    observed entries, scaled by r = p / |S|); a_err / g_err: the dot-product bound 2 p u |x| |d| of what the device forms"""
    rs = np.random.RandomState(seed)
    T = DT[dt]
    D = unit_dictionary(rs, k, p).astype(T)
    X = np.zeros((n, p))
    for i in range(n):
        at = rs.choice(np.setdiff1d(np.arange(k), DUP), 3, replace=False)
        X[i] = np.array([3.0, -2.0, 1.2]).dot(D[at].astype(np.float64)) + (0.3 if i % 2 else 1e-3) * rs.randn(p)
    X = X.astype(T)
    X64, D64 = X.astype(np.float64), D.astype(np.float64)
    if obs is None:
        G, Dx, xn, r = D64.dot(D64.T), X64.dot(D64.T), np.sum(X64 ** 2, axis=1), 1.0
    else:
        r = p / np.maximum(obs.sum(axis=1), 1)
        G = np.stack([r[i] * (D64 * obs[i]).dot((D64 * obs[i]).T) for i in range(n)])
        Dx = np.stack([r[i] * (X64[i] * obs[i]).dot((D64 * obs[i]).T) for i in range(n)])
        xn = r * np.sum((X64 * obs) ** 2, axis=1)
    rmax = float(np.max(r))
    c = SimpleNamespace(dt=dt, k=k, p=p, b=n, s=s, tol=tol, G=G, Dx=Dx, xn=xn, D=D, X=X)
    xmax = float(np.max(np.linalg.norm(X64, axis=1)))
    c.a_err = 2 * p * U[dt] * xmax * rmax * 1.001
    c.g_err = 2 * p * U[dt] * rmax * 1.001
    return c


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'f64'])
@pytest.mark.parametrize('n,tol', [(300, None), (4097, 0.5)])
def test_somf_transform_omp(gpu, dt, n, tol):
    """modl_somf_transform_omp through HipBackend.omp (p = 48): n = 300 inside one chunk, n = 4097 across max_batch = 4096;
    the judge's Dx and G are recomputed in f64 from X and D"""
    import torch
    from modl_amd import Coder
    c = data_case(dt, 32, 48, n, 4, 5, tol=tol)
    coder = Coder(c.D)
    be, kw = coder._backend, coder._plan_kwargs(4096)
    code, sup, na = be.omp(_dev(c.X), c.s, tol, kw=kw)
    assert code.is_cuda and code.shape == (n, c.k) and sup.dtype == torch.int32 and na.dtype == torch.int32
    code, sup, na = code.cpu().numpy(), sup.cpu().numpy(), na.cpu().numpy()
    if n > 4096:
        assert np.all(na >= 1) and np.all(na <= c.s) and np.all(np.count_nonzero(code, axis=1) == na) and len(set(na)) > 1
    ws, wc = judge(c, code, sup, na, a_err=c.a_err, g_err=c.g_err)
    print('%s transform_omp n=%d: selection %.3g, coefficients %.3g of the bound' % (dt, n, ws, wc))
    # support and n_active may be left out
    from modl_amd._lib import lib
    from modl_amd.device import ptr, stream_ptr
    X = _dev(c.X[:9])
    out = torch.empty((9, c.k), dtype=X.dtype, device='cuda')
    rc = lib.modl_somf_transform_omp(be.tplan, ptr(be.Dt), None, ptr(X), X.stride(0), 9, c.s, -1.0 if tol is None else tol,
                                     ptr(out), None, None, stream_ptr(be.device))
    assert rc == 0
    np.testing.assert_array_equal(out.cpu().numpy(), be.omp(X, c.s, tol, kw=kw)[0].cpu().numpy())
    for bad in (0, OMP_MAX_NONZERO + 1, c.k + 1):
        assert lib.modl_somf_transform_omp(be.tplan, ptr(be.Dt), None, ptr(X), X.stride(0), 9, bad, -1.0, ptr(out), None, None,
                                           stream_ptr(be.device)) == EINVAL


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_estimators_transform_omp(gpu, dt):
    import torch
    from modl_amd import Coder, DictFact
    rs = np.random.RandomState(3)
    n, k, p, s = 41, 32, 24, 3
    obs = rs.rand(n, p) < 0.6
    obs[0] = False                                                  # a row nobody observed
    obs[1:6] = True                                                 # rows without a hole
    c = data_case(dt, k, p, n, s, 6, obs=obs)
    est = DictFact(n_components=k, batch_size=16, random_state=0, code_alpha=0.1)
    est.prepare(n_samples=n, X=c.X)
    est.components_ = c.D
    for e in (Coder(c.D), est):
        out = e.transform(c.X, algorithm='omp', n_nonzero_coefs=s)
        assert isinstance(out, np.ndarray) and out.dtype == DT[dt] and out.shape == (n, k)
        assert np.all(np.count_nonzero(out, axis=1) <= s)
        out_t = e.transform(_dev(c.X), algorithm='omp', n_nonzero_coefs=s)
        assert isinstance(out_t, torch.Tensor) and out_t.is_cuda
        np.testing.assert_array_equal(out_t.cpu().numpy(), out)
        np.testing.assert_array_equal(e.transform(c.X, mask=np.ones((n, p), dtype=bool), algorithm='omp', n_nonzero_coefs=s), out)
        default = e.transform(c.X, algorithm='omp')                 # max(1, k // 10) atoms
        assert np.all(np.count_nonzero(default, axis=1) <= max(1, k // 10))
        by_tol = e.transform(c.X, algorithm='omp', residual_tol=0.5)
        res = np.sum((c.X.astype(np.float64) - by_tol.astype(np.float64).dot(c.D.astype(np.float64))) ** 2, axis=1)
        assert np.all(res <= 0.5 * (1 + 1e-3)) and len(set(np.count_nonzero(by_tol, axis=1))) > 1
        masked = e.transform(c.X, mask=obs, algorithm='omp', n_nonzero_coefs=s, residual_tol=0.05)
        assert not np.any(masked[0]) and np.all(np.count_nonzero(masked, axis=1) <= s)
        np.testing.assert_array_equal(masked[1:6], e.transform(c.X[1:6], algorithm='omp', n_nonzero_coefs=s, residual_tol=0.05))
        # the holed rows against the judge, on their own Gram matrices
        be = e._backend
        code, sup, na = (t.cpu().numpy() for t in be.omp(_dev(c.X), s, 0.05, obs=_dev(obs.view(np.uint8)), kw=e._plan_kwargs(4096)))
        np.testing.assert_array_equal(code, masked)
        assert na[0] == 0 and np.all(sup[0] == -1)
        holed = np.flatnonzero((obs.sum(axis=1) > 0) & (obs.sum(axis=1) < p))
        ch = SimpleNamespace(dt=dt, k=k, p=p, b=len(holed), s=s, tol=0.05, G=c.G[holed], Dx=c.Dx[holed], xn=c.xn[holed])
        ws, wc = judge(ch, code[holed], sup[holed], na[holed], a_err=c.a_err, g_err=c.g_err)
        print('%s masked rows: selection %.3g, coefficients %.3g of the bound' % (dt, ws, wc))
        with pytest.raises(ValueError, match='64'):
            e.transform(c.X, algorithm='omp', n_nonzero_coefs=65)
        with pytest.raises(ValueError, match='n_components = %d' % k):
            e.transform(c.X, algorithm='omp', n_nonzero_coefs=k + 1)
        with pytest.raises(ValueError, match='omp'):
            e.transform(c.X, n_nonzero_coefs=3)
        with pytest.raises(ValueError, match='enet'):
            e.transform(c.X, algorithm='lars')
        with pytest.raises(ValueError, match='>= 0'):
            e.transform(c.X, algorithm='omp', residual_tol=-1)


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_default_algorithm_is_todays(gpu, dt):
    """transform(X) and transform(X, algorithm='enet') are the same bits, with and without a mask, also after an OMP call
    has used the estimator's transform plan"""
    from modl_amd import Coder
    rs = np.random.RandomState(4)
    c = data_case(dt, 32, 24, 37, 3, 9)
    obs = rs.rand(37, 24) < 0.7
    coder = Coder(c.D, code_alpha=0.05)
    plain, masked = coder.transform(c.X), coder.transform(c.X, mask=obs)
    coder.transform(c.X, algorithm='omp')
    np.testing.assert_array_equal(coder.transform(c.X, algorithm='enet'), plain)
    np.testing.assert_array_equal(coder.transform(c.X), plain)
    np.testing.assert_array_equal(coder.transform(c.X, mask=obs, algorithm='enet'), masked)
    assert np.count_nonzero(plain) > 0


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_image_reconstruct_and_inpaint_omp(gpu, dt):
    """a 24 x 24 x 3 image, 8 x 8 patches, k = 32, four atoms per patch: the result is decode + overlap-add of the codes
    that omp() returns (through reconstruct_from_patches); inpaint leaves the observed pixels alone"""
    import contextlib
    import io
    from modl_amd import reconstruct_from_patches
    from modl_amd.image import ImageDictFact, _grid, _grid_shape, _grid_patches_pass, _grid_patches_masked_pass, _stage_image
    from .test_wrappers import synth_image
    T = DT[dt]
    img = synth_image(24, 24, 3, seed=2).astype(T)
    est = ImageDictFact(patch_size=(8, 8), n_components=32, batch_size=20, alpha=0.1, random_state=0, max_patches=200)
    with contextlib.redirect_stdout(io.StringIO()):
        est.fit(img)
    be = est.dict_fact_._backend
    s = ImageDictFact.settings[est.setting]
    g = _grid(img.shape, (8, 8), 1)
    grows, gcols = _grid_shape(g)
    d_img = _stage_image(img, be.device, dtype=be.dtype)
    out = est.reconstruct(img, algorithm='omp', n_nonzero_coefs=4)
    assert out.shape == img.shape and out.dtype == T
    patches, mean, den = _grid_patches_pass(d_img, g, gcols, 0, grows, s['with_mean'], s['with_std'])
    kw = est.dict_fact_._plan_kwargs(4096)
    code, sup, na = be.omp(patches, 4, None, kw=kw)
    assert int(na.max()) <= 4 and int((code != 0).sum(dim=1).max()) <= 4
    want = reconstruct_from_patches(be.decode(code, mean, den).cpu().numpy(), img.shape, (8, 8), 1)
    np.testing.assert_array_equal(out, want)
    assert not np.array_equal(out, est.reconstruct(img))            # (the elastic-net coder gives another image)
    by_tol = est.reconstruct(img, algorithm='omp', residual_tol=0.05)
    assert by_tol.shape == img.shape and not np.array_equal(by_tol, out)
    # inpaint
    rs = np.random.RandomState(1)
    m = rs.rand(24, 24) < 0.8
    holed = np.where(m[:, :, None], img, T(-1))
    filled = est.inpaint(holed, mask=m, algorithm='omp', n_nonzero_coefs=4)
    assert filled.shape == img.shape and filled.dtype == T
    np.testing.assert_array_equal(filled[m], img[m])
    assert np.all(filled[~m] != -1)
    raw = est.inpaint(holed, mask=m, algorithm='omp', n_nonzero_coefs=4, keep_observed=False)
    d_obs = _dev(np.ascontiguousarray(np.broadcast_to(m[:, :, None], img.shape)).view(np.uint8))
    patches, mean, den, obs, nobs = _grid_patches_masked_pass(_stage_image(holed, be.device, dtype=be.dtype), d_obs, g, gcols, 0,
                                                              grows, s['with_mean'], s['with_std'])
    assert int(nobs.min()) > 0
    code = be.omp(patches, 4, None, obs=obs, kw=kw, nobs=nobs)[0]
    want = reconstruct_from_patches(be.decode(code, mean, den).cpu().numpy(), img.shape, (8, 8), 1)
    np.testing.assert_array_equal(raw, want)
    with pytest.raises(ValueError, match='64'):
        est.reconstruct(img, algorithm='omp', n_nonzero_coefs=65)
