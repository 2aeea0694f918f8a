"""The dictionary update (csrc/bcd.hip: du_route, dict_update) route by route, through modl_dict_update_f32 /
_f64, against the CPU oracle's update_dict on inputs built to leave the projection's main branch.

Three layers:

1. `make_case` (numpy + the oracle's initialisation, no GPU): the state of one dictionary update in a named *scene* -
   `generic` (the recipe test_wide_components.py has always used; for l2 with one gain per atom, so that two atoms of three
   leave their ball and the third is copied: with the recipe's single gain of 0.9 an l2 update clips nothing), `inside`, `mixed`, `dead`, `zero`, and the *controlled*
   scenes, where C is diagonal with power-of-two entries and the dictionary is zero on the subset, so that atom j's candidate
   is exactly B[j, subset] / C[j][j] and a chosen vector can be placed there: `ties`, `ties_at_level`, `spike`, `flat`,
   `boundary`, `heavy` and `copy` (a candidate inside its ball: the result is a copy, compared bit for bit).  In a controlled
   scene every fourth atom along `order` is of the `copy` kind, so that every group of four or eight atoms of the grouped
   routes mixes projected and copied atoms, and so that the budgets left (comp_norm) are not all at rounding level.
2. CPU tests: the scenes are what they claim (`test_cases_are_what_they_claim`), the matrix of layer 3 holds every route
   and both neighbours of every numeric boundary of the dispatch (`test_route_table`, against `expected_route`, a
   restatement of the dispatch conditions, which is in turn held against the library's own answer, modl_dict_update_route,
   on 256 and on 128 compute units: `library_route`), and the acceptance rules of layer 3 reject six kinds of wrong result
   (`test_acceptance_rule_rejects_mutants`); every l2 route and boundary neighbour has a case in which the oracle both clips
   and copies (`test_l2_cases_clip_and_copy`).
3. GPU tests (`test_route`): CASES, about 200 direct calls.  f64: rel_fro < 1e-9 and comp_norm to rtol 1e-9 / atol 1e-12
   (the rule of test_wide_components.py::test_dict_update_f64); f32: conftest.assert_within_f32_noise for the dictionary
   and for comp_norm; both: the rows of Dt outside `subset` bit-identical to the input; the rows of `zero` and `dead`
   atoms and the atoms of `copy` kind (l1 / elastic-net updates) bit-identical to the expected values.

Michelot passes and the cap of the spread projection (kMwgMaxPass = 23 exchanges in csrc/bcd.hip: mwg_l1_project).
`michelot_passes` restates the active-set iteration only to COUNT passes; it judges nothing.  `heavy`
(logspace(0, -3, s), radius 1e-3) takes 15 passes at s = 16 384; Gaussian vectors 4 to 10.  No `over_cap` scene exists,
because no input that needs more than 23 passes was found, and the reason is arithmetic: for a pass to drop anything the
elements it drops must lie between two consecutive levels, and going down the vector these gaps grow by a factor of at
least (c - 1), c the number of elements still active - so P passes need gaps spread over a ratio of about (P - 1)!,
while all of them must stay below the largest element.  f64 holds 2^53 ~ 18! of relative spread (f32 data: 2^24 ~ 10!).
`adversarial_michelot_vector` builds exactly that worst case greedily (each pass drops one element, gaps as small as
the format allows); `test_heavy_scene_and_the_pass_cap` runs this bounded search, together with piecewise-geometric
plateaus, and asserts what it reaches: 15 passes in f64, 12 for f32-representable data, 8 for the plateaus - no more than
`heavy` itself.  The cap is out of reach and the give-up branch of mwg_l1_project cannot be entered through the product
library.  The constant was not lowered to make one.

`expected_route` restates du_route of csrc/bcd.hip, the one function that decides the route (a DuRoute of csrc/kernels.hpp:
the family DU_SGD, DU_WIDE, DU_TINY, DU_FEW, DU_UNFUSED, DU_BLOCK, DU_PERSIST, DU_SWEEP, DU_GROUPED, DU_STAGED or DU_STEP
and the launch parameters RT, GPW, acc, shards, nfew, EPT, G, KPL, l1, pipelined, regs, spread, ept, lds); dict_update
switches on the family to du_sgd, dict_update_wide, du_unfused (tiny, few and unfused: they share their first launch),
du_block, du_persist, du_sweep, du_grouped, du_staged (pipelined or not) and du_step.  The residency of the persistent
launch is bcd_persist_fits of csrc/bcd_persist.hip.  The strings are the ones du_route_name writes for
modl_dict_update_route.  The same table is in DESIGN.md, section 10 "Dictionary-update route matrix".
"""
import os
import zlib
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import somf_oracle as _orc

from .conftest import assert_within_f32_noise, rel_fro

DT = {'f32': np.float32, 'f64': np.float64}
UPDATES = {'l2': dict(), 'l1': dict(comp_l1_ratio=1.0), 'enet': dict(comp_l1_ratio=0.5),
           'l1_pos': dict(comp_l1_ratio=1.0, comp_pos=True), 'enet_pos': dict(comp_l1_ratio=0.7, comp_pos=True),
           'sgd': dict(optimizer='sgd')}
CONTROLLED = ('ties', 'ties_at_level', 'spike', 'flat', 'boundary', 'heavy', 'copy')
SCENES = ('generic', 'inside', 'mixed', 'dead', 'zero') + CONTROLLED

# the debug switches of the dictionary update: the values the PRODUCT library accepts as distinct code paths (include/modl_hip.h;
# 2, 3 and 4 of BCD_PERSIST and 2 of ATOM_MWG belong to the diagnostics library: they inject a stalled workgroup)
SWITCH_VALUES = {'BCD_ACC': (0, 1), 'BCD_TINY': (0, 1), 'BCD_FEW': (0, 1), 'BCD_PERSIST': (0, 1), 'ATOM_MWG': (0, 1, 3),
                 'ATOM_PIPE': (0, 1)}


def switch_defaults():
    d = {name: 1 for name in SWITCH_VALUES}
    d['BCD_ACC'] = int(os.environ.get('MODL_TEST_BCD_ACC', 1))     # (conftest.py: A/B runs of the whole suite)
    return d


def _cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------- the dispatch, restated
def expected_route(dt, k, s, update, switches=None, ncu=256):
    """The route csrc/bcd.hip takes (du_route, see the module docstring), as 'family/variant/...'."""
    sw = switch_defaults()
    sw.update(switches or {})
    tsz = 4 if dt == 'f32' else 8
    u = UPDATES[update]
    rho, pos, sgd = u.get('comp_l1_ratio', 0.0), u.get('comp_pos', False), u.get('optimizer') == 'sgd'
    if k > 1024 and not sgd:
        return 'wide'
    if sgd:
        return 'sgd'
    if rho == 0.0 and not pos:
        kp = 4 * _cdiv(k, 4)
        if tsz == 4 and k <= 512:
            if sw['BCD_PERSIST'] and sw['BCD_ACC'] and _cdiv(k, 32) <= 16:
                # bcd_persist_fits: at most 255 row workgroups, the resolver + the rows resident on the chip's compute units
                # (the 160 KiB LDS bound is not binding up to 512 atoms)
                n1, n2 = _cdiv(s, 32), _cdiv(s, 64)
                if n1 <= 255 and 1 + n1 <= ncu:
                    return 'persist/RT1'
                if kp <= 256 and n2 <= 255 and 1 + n2 <= ncu:
                    return 'persist/RT2'
            rt = 1 if (s <= 2048 or k > 256) else 2
            if rt == 2 and _cdiv(s, 64) > ncu and _cdiv(s, 96) <= ncu:
                rt = 3
            nslab = _cdiv(s, 32 * rt)
            return 'block/RT%d/GPW%d/acc%d/shards%d' % (rt, 8 if kp <= 256 else 16, 1 if sw['BCD_ACC'] else 0,
                                                        4 if nslab > 64 else 1)
        if tsz == 8 and s > 192 and _cdiv(s, 32) <= 64 and sw['BCD_TINY'] and sw['BCD_FEW']:
            return 'few/nfew%d' % _cdiv(s, 32)
        if tsz == 8 and s <= 192 and sw['BCD_TINY']:
            return 'tiny'
        return 'unfused'
    l1 = rho == 1.0
    kpl = 1 if k <= 64 else 2 if k <= 128 else 4 if k <= 256 else 8 if k <= 512 else 16
    if 8 * (16 + k) + tsz * s + 16 <= 64 * 1024 and s * k <= 32000:
        return 'sweep'
    if s <= 24 * 256 and k <= 512:
        return 'grouped/EPT%d/G%d/KPL%d/%s' % (12 if s <= 12 * 256 else 20 if s <= 20 * 256 else 24, 8 if s <= 20 * 256 else 4,
                                               kpl, 'l1' if l1 else 'enet')
    if tsz * s <= 60 * 1024 and s > 24 * 256:
        nwg_corr = _cdiv(s, 256)
        mwg = l1 and nwg_corr <= 64 and sw['ATOM_MWG'] != 0
        regs = l1 and sw['ATOM_MWG'] == 1 and s <= 64 * 256
        if (mwg or regs) and _cdiv(k, 4) >= 2 and sw['ATOM_PIPE'] != 0:
            if regs:
                return 'staged_pipe/KPL%d/regs%d' % (kpl, 40 if s <= 40 * 256 else 64)
            return 'staged_pipe/KPL%d/spread/ept%d' % (kpl, 2 if nwg_corr > 32 else 1)
        # (not pipelined: KPL is atom_grad4_kernel's; the atoms run atom_corr_project_kernel<T, 0>)
        return 'staged/grad4KPL%d/%s' % (kpl, 'spread' if mwg else ('lds_l1' if l1 else 'lds_enet'))
    return 'step/KPL%d/%s' % (kpl, 'lds' if tsz * s <= 60 * 1024 else 'global')


def library_route(dt, k, s, update, ncu):
    """modl_dict_update_route: the route the library's own du_route gives a direct call under the switches set now.
    ncu > 0: on that many compute units, no device involved; 0: on the current device."""
    import ctypes as C
    from modl_amd import _lib
    u = UPDATES[update]
    buf = C.create_string_buffer(64)
    _lib.check(_lib.lib.modl_dict_update_route(_lib.MODL_F32 if dt == 'f32' else _lib.MODL_F64, k, s, 1 if u.get('optimizer') == 'sgd' else 0,
                                               int(u.get('comp_pos', False)), u.get('comp_l1_ratio', 0.0), ncu, buf, len(buf)),
               'modl_dict_update_route')
    return buf.value.decode()


# ---------------------------------------------------------------------------------------------------- layer 1: the case builder
def atoms(k, p, seed=0, dt=np.float64):
    rs = np.random.RandomState(seed)
    D = rs.randn(k, p) * (rs.rand(k, p) < 0.5) + 0.05 * rs.randn(k, p)
    return (D / np.linalg.norm(D, axis=1, keepdims=True)).astype(dt)


def params(update, k=10):
    return _orc.SomfParams(n_components=k, batch_size=16, reduction=2, code_alpha=1.0, learning_rate=0.92, random_state=0, **UPDATES[update])


def enet_norm64(v, rho):
    a = np.abs(np.asarray(v, dtype=np.float64))
    return float(np.sum(a * (rho + (1.0 - rho) * a)))


def project64(v, radius, rho, level_factor=1.0):
    """The elastic-net projection (the reference's enet.pyx:38-122, as oracle/somf_oracle_impl.inc states it) by sorting, in
    f64.  Returns (projected vector, support size).  level_factor != 1 scales the soft threshold: a mutant."""
    v = np.asarray(v, dtype=np.float64)
    if radius == 0.0:
        return np.zeros_like(v), 0
    if rho == 0.0:
        n2 = float(np.sum(v * v))
        return (v.copy() if n2 <= radius else v / np.sqrt(n2 / radius)), int(np.count_nonzero(v))
    gamma = 2.0 / rho - 2.0
    R = radius / rho
    a = np.sort(np.abs(v))[::-1]
    f = a * (1.0 + 0.5 * gamma * a)
    if f.sum() <= R:
        return v.copy(), int(np.count_nonzero(v))
    cs = np.cumsum(f)
    m = np.arange(1, len(a) + 1)
    ok = cs - m * (1.0 + 0.5 * gamma * a) * a < R * (1.0 + gamma * a) ** 2
    n = int(m[ok].max())
    sm = cs[n - 1]
    if gamma != 0.0:
        qa, qd, qc = gamma * gamma * R + gamma * n * 0.5, 2.0 * R * gamma + n, R - sm
        lv = (-qd + np.sqrt(qd * qd - 4.0 * qa * qc)) / (2.0 * qa)
    else:
        lv = (sm - R) / n
    lv *= level_factor
    out = np.where(v >= 0, 1.0, -1.0) * np.maximum(np.abs(v) - lv, 0.0) / (1.0 + lv * gamma)
    return out, n


def michelot_passes(a, radius):
    """Passes over the vector and final support of the active-set l1 projection (the shape of csrc/bcd.hip: mwg_l1_project,
    cold start).  Used to COUNT only."""
    a = np.abs(a)
    S, cnt = float(a.sum()), int(np.count_nonzero(a > 0))
    if S <= radius or cnt == 0:
        return 1, cnt
    passes, prev, lv = 1, cnt, (S - radius) / cnt
    while True:
        m = a > lv
        S, cnt = float(a[m].sum()), int(np.count_nonzero(m))
        passes += 1
        if cnt == prev or cnt == 0:
            return passes, cnt
        prev, lv = cnt, (S - radius) / cnt


def adversarial_michelot_vector(dt, n=40):
    """The worst case of the active-set iteration, built from the top element down: each new element is the largest
    value of type dt that the pass which sees it for the first time still drops ALONE.  Returns (vector, radius)."""
    top = dt(1.0)
    R = 0.5
    vals = [float(top)]
    for _ in range(n - 1):
        A = np.array(vals)
        lv = (A.sum() - R) / len(A)                   # the level of the set above: the new element must not exceed it
        bound = (len(A) + 1) * A.min() - A.sum() + R   # adding it must leave every element above it active: the new level below them
        a = float(dt(min(lv, bound)))
        for _ in range(4):                            # (rounding to dt may have gone up; the second bound is strict)
            if a > lv or (A.sum() + a - R) / (len(A) + 1) >= A.min():
                a = float(np.nextafter(dt(a), dt(0)))
        if not (0 < a < A.min()):
            break
        vals.append(a)
    return np.array(vals[::-1], dtype=dt), R


def _special_positions(k, rs, share=0.1):
    """positions along `order` of the special atoms of `dead` / `zero`: the first, the last, two adjacent ones and about
    a tenth of the rest"""
    pos = {0, k - 1}
    if k >= 6:
        m = int(rs.randint(1, k - 3))
        pos |= {m, m + 1}
    if k > 10:
        pos |= set(int(x) for x in rs.choice(k, max(1, int(share * k)), replace=False))
    if len(pos) == k and k > 1:                       # (tiny dictionaries: keep an ordinary atom)
        pos.discard(k - 1)
    return sorted(pos)


def radius_for_level(v, lv, rho):
    """the radius at which the projection of v ends at soft threshold lv (the elastic-net norm of the result)"""
    if rho == 0.0:
        return 0.5 * float(np.sum(np.asarray(v, np.float64) ** 2))
    gamma = 2.0 / rho - 2.0
    out = np.maximum(np.abs(np.asarray(v, np.float64)) - lv, 0.0) / (1.0 + lv * gamma)
    return enet_norm64(out, rho)


def _controlled_vector(scene, s, rho, rs, dt):
    """(|v| of length s, radius) of one atom of a controlled scene; values exactly representable in f32"""
    a = 2.0 ** -6
    if scene == 'ties':                                # {0, a, 2a}, the level ends inside (a, 2a)
        mag = rs.choice([0.0, a, 2 * a], size=s, p=[0.3, 0.4, 0.3])
        mag[0] = 2 * a
        return mag, radius_for_level(mag, 1.5 * a, rho)
    if scene == 'ties_at_level':                       # 4a on top; the a's leave in one pass; the 2a's sit AT the final level
        mag = rs.choice([a, 2 * a, 4 * a], size=s, p=[0.6, 0.2, 0.2])
        mag[0] = 4 * a
        return mag, radius_for_level(mag, 2 * a, rho)
    if scene == 'spike':                               # one entry far above the radius: a support of one element
        mag = np.asarray(rs.rand(s) * 1e-5, dtype=np.float32).astype(np.float64)
        mag[int(rs.randint(s))] = 1.0
        return mag, radius_for_level(mag, 0.75, rho) if rho != 0.0 else 0.25
    if scene == 'flat':
        mag = np.full(s, a)
        return mag, 0.5 * enet_norm64(mag, rho)
    if scene == 'heavy':                               # many Michelot passes
        mag = np.logspace(0, -3, s).astype(np.float32).astype(np.float64)
        return mag, 1e-3
    if scene == 'boundary':                            # the norm equal to the radius up to one ulp either side (set by the caller)
        mag = (np.abs(rs.randn(s)).astype(np.float32).astype(np.float64) + 2.0 ** -10) * a
        return mag, None
    mag = np.abs(rs.randn(s)).astype(np.float32).astype(np.float64) * a   # 'copy' (sums of order one, like every scene here)
    return mag, 2.0 * enet_norm64(mag, rho) + 0.25


def make_case(dt, k, s, scene, update, seed, order_kind='perm', sort_subset=None, diag_boost=1.0, noise=None, gain=None):
    """One dictionary update's state: D (k, p), B, C (positive semi-definite), comp_norm, subset, order, w; p = s + 200.
    order_kind: 'perm' | 'identity' | 'reversed'.  sort_subset: None = sorted for even seeds only.
    Conditioning: the recipe of test_wide_components.py (diag_boost = 0, noise = 0.01) was made for more than a thousand atoms;
    with a few atoms its C has diagonal entries near 0.1 and B's noise, divided by them, gives candidates whose norm is
    hundreds of times the radius - the budget left is then the difference of two large sums and misses atol 1e-12 by
    rounding alone, between two CPU implementations already.  So here diag_boost (added to C's diagonal) is 1 and the noise
    shrinks with the number of features beyond 2000: candidates stay within a few tens of their radius.
    gain: B = gain C D + noise (the recipe: 0.9).  With 0.9, this diagonal and this noise every l2 candidate is about 0.9 of
    its atom and lies INSIDE its ball - an l2 update that never clips.  So for l2 the default is one gain per atom: 1.15 (the
    candidate leaves its ball and is scaled back) for two atoms of three, 0.9 (a copy) for the third; every l2 case of the
    matrix then runs both branches of the l2 projection (`test_l2_cases_clip_and_copy`)."""
    dt = DT[dt] if isinstance(dt, str) else dt
    assert scene in SCENES and update in UPDATES
    p = s + 200
    u = UPDATES[update]
    rho, pos = u.get('comp_l1_ratio', 0.0), u.get('comp_pos', False)
    rs = np.random.RandomState(seed)
    pr = params(update, k)
    st = _orc.prepare(pr, n_samples=8, X=atoms(k, p, seed, dt))          # (abs for positive atoms, rows scaled to the unit ball)
    D = st.D
    A = rs.randn(k + 64, k) * (rs.rand(k + 64, k) < 0.1)
    C = np.ascontiguousarray((A.T.dot(A) / 64 + np.diag(rs.rand(k) * (rs.rand(k) < 0.97))).astype(dt))
    if diag_boost:
        C[np.arange(k), np.arange(k)] += dt(diag_boost)
    if noise is None:
        noise = 0.01 * min(1.0, 2000.0 / p)
    if gain is None:
        gain = 0.9
        if rho == 0.0 and not pos and u.get('optimizer') != 'sgd':
            gain = np.where(np.arange(k) % 3 == 1, 0.9, 1.15)[:, None]
    B = np.ascontiguousarray((C.dot(D) * gain + noise * rs.randn(k, p)).astype(dt))
    subset = np.sort(rs.choice(p, s, replace=False)).astype(np.int64)
    order = rs.permutation(k).astype(np.int64)
    comp_norm = np.zeros(k, dtype=dt)
    # ---- everything beyond the generic recipe draws from a second stream (the first one is the recipe's, unchanged)
    r2 = np.random.RandomState(seed + 7919)
    if order_kind == 'identity':
        order = np.arange(k, dtype=np.int64)
    elif order_kind == 'reversed':
        order = np.arange(k, dtype=np.int64)[::-1].copy()
    if sort_subset is None:
        sort_subset = seed % 2 == 0
    if not sort_subset:
        subset = subset[r2.permutation(s)]
    case = SimpleNamespace(dt=dt, k=k, s=s, p=p, scene=scene, update=update, D=D, B=B, C=C, comp_norm=comp_norm, subset=subset,
                           order=order, w=0.3, special=[], kinds=None)
    if scene in ('inside', 'mixed'):
        inside = order if scene == 'inside' else order[0::2]
        if scene == 'mixed':                            # the atoms in between: pushed well outside their ball
            B[order[1::2]] += (1.8 * C.dot(D)[order[1::2]]).astype(dt)
        # a dry run with unbounded budgets gives every candidate's norm along the sweep; 1.5 times it is a budget that keeps it inside
        dry = SimpleNamespace(**vars(case))
        dry.comp_norm = np.where(np.isin(np.arange(k), inside), 1e30, 0.0)
        Dd, _ = reference(dry, np.float64)
        for j in inside:
            comp_norm[j] = 1.5 * enet_norm64(Dd[j, subset], rho) + 0.1
        case.special = [int(j) for j in inside]
    elif scene == 'dead':                               # C[j][j] == 0: the atom keeps its values (and is still projected: inside)
        dead = order[_special_positions(k, r2)]
        C[dead, :] = 0
        C[:, dead] = 0
        comp_norm[dead] = 0.0625
        case.special = [int(j) for j in dead]
    elif scene == 'zero':                               # radius 0: nothing on the subset, no budget
        z = order[_special_positions(k, r2)]
        D[np.ix_(z, subset)] = 0
        B[np.ix_(z, subset)] = 0
        case.special = [int(j) for j in z]
    elif scene in CONTROLLED:
        c = 2.0 ** r2.randint(-1, 3, size=k)
        C[:] = np.diag(c).astype(dt)
        D[:, subset] = 0
        kinds = np.array([scene] * k, dtype=object)
        kinds[order[3::4]] = 'copy'
        case.kinds = kinds
        for t, j in enumerate(order):
            mag, radius = _controlled_vector(kinds[j], s, rho, r2, dt)
            sign = np.ones(s) if pos else np.where(r2.rand(s) < 0.5, -1.0, 1.0)
            v = (sign * mag[r2.permutation(s)]).astype(dt)
            B[j, subset] = v * dt(c[j])                 # (a power of two: exact)
            if radius is None:                          # boundary: the norm as type dt sums it, moved by -1, 0, +1 ulp
                n = dt(_orc.enet_norm(v, rho))
                radius = [np.nextafter(n, dt(0)), n, np.nextafter(n, dt(np.inf))][t % 3]
            comp_norm[j] = radius
        case.special = [int(j) for j in order[3::4]]
    return case


def reference(case, dt):
    """oracle.update_dict on the case's arrays as type dt: (D (k, p), comp_norm)"""
    st = _orc.SomfState()
    st.D = np.ascontiguousarray(case.D.astype(dt))
    st.B = np.ascontiguousarray(case.B.astype(dt))
    st.C = np.ascontiguousarray(case.C.astype(dt))
    st.comp_norm = np.asarray(case.comp_norm).astype(dt)
    _orc.update_dict(st, params(case.update), case.subset, case.w, order=case.order)
    return st.D, st.comp_norm


def restated_update(case, skip_projection=None, keep_budget=None, level_factor=1.0):
    """update_dict's variational branch in plain f64 numpy, with the hooks of the mutants.  Returns (D, comp_norm, supports)."""
    u = UPDATES[case.update]
    rho, pos = u.get('comp_l1_ratio', 0.0), u.get('comp_pos', False)
    D, B, C = (np.asarray(x, dtype=np.float64) for x in (case.D, case.B, case.C))
    cn = np.asarray(case.comp_norm, dtype=np.float64).copy()
    Ds = D[:, case.subset].copy()
    gs = B[:, case.subset] - C.dot(Ds)
    supports = {}
    for j in case.order:
        cn[j] += enet_norm64(Ds[j], rho)
        gs += np.outer(C[j], Ds[j])
        if C[j, j] > 1e-20:
            Ds[j] = gs[j] / C[j, j]
        if pos:
            Ds[Ds < 0] = 0
        if j != skip_projection:
            Ds[j], supports[int(j)] = project64(Ds[j], cn[j], rho, level_factor)
        if j != keep_budget:
            cn[j] -= enet_norm64(Ds[j], rho)
        gs -= np.outer(C[j], Ds[j])
    out = D.copy()
    out[:, case.subset] = Ds
    return out, cn, supports


# ---------------------------------------------------------------------------------------------------- the acceptance rules
def check_f64(D, cn, D64, cn64):
    assert rel_fro(D, D64) < 1e-9, ('D', rel_fro(D, D64))
    # the norm budgets left after the projections sit at rounding level (~1e-16) when the ball is hit: absolute
    np.testing.assert_allclose(cn, cn64, rtol=1e-9, atol=1e-12)


def check_f32(D, cn, D32, cn32, D64, cn64):
    assert_within_f32_noise(D, D32, D64, 'D')
    assert_within_f32_noise(cn, cn32, cn64, 'comp_norm')


def accepts(check, *args):
    try:
        check(*args)
    except AssertionError:
        return False
    return True


# ---------------------------------------------------------------------------------------------------- layer 3: the matrix
CASES = []


def _add(dt, k, s, update, scenes=('generic',), sw=None, order='perm', sort_subset=None):
    for scene in scenes:
        CASES.append(SimpleNamespace(dt=dt, k=k, s=s, update=update, scene=scene, sw=dict(sw or {}), order=order,
                                     sort_subset=sort_subset))


ALL4 = ('generic', 'mixed', 'dead', 'zero')
L2_SCENES = ALL4 + ('inside', 'boundary', 'flat')
PROJ_SCENES = ALL4 + CONTROLLED

# bcd_tiny_kernel: f64 l2, s <= 192
_add('f64', 33, 150, 'l2', L2_SCENES)
_add('f64', 33, 150, 'l2', order='identity')
_add('f64', 33, 150, 'l2', order='reversed')
_add('f64', 5, 1, 'l2')
_add('f64', 70, 192, 'l2')
# bcd_few_kernel: f64 l2, 193 ... 2048; nfew = 7, 16, 64
_add('f64', 70, 193, 'l2')
_add('f64', 33, 500, 'l2', L2_SCENES)
_add('f64', 33, 500, 'l2', order='identity')
_add('f64', 33, 500, 'l2', order='reversed')
_add('f64', 65, 2048, 'l2')
_add('f64', 1, 300, 'l2')
# unfused prepare / gemm / gram / resolve / apply
_add('f64', 65, 2049, 'l2')
_add('f64', 33, 2100, 'l2', L2_SCENES)
_add('f64', 33, 2100, 'l2', order='identity')
_add('f64', 33, 2100, 'l2', order='reversed')
_add('f32', 513, 300, 'l2')
_add('f32', 1024, 1000, 'l2')
_add('f64', 33, 150, 'l2', sw={'BCD_TINY': 0})
_add('f64', 33, 500, 'l2', sw={'BCD_FEW': 0})
# the persistent launch: f32 l2, k <= 512
_add('f32', 70, 1000, 'l2', L2_SCENES)
_add('f32', 70, 1000, 'l2', order='identity')
_add('f32', 70, 1000, 'l2', order='reversed')
for _k in (1, 31, 32, 33, 255, 256, 257, 512):
    _add('f32', _k, 1000, 'l2')
_add('f32', 64, 8160, 'l2')
_add('f32', 64, 8161, 'l2', ('generic', 'mixed'))
_add('f32', 256, 9000, 'l2')
_add('f32', 257, 9000, 'l2')
_add('f32', 64, 16320, 'l2')
_add('f32', 64, 16321, 'l2')
_add('f32', 512, 8160, 'l2')
_add('f32', 512, 16384, 'l2')
# bcd_block_kernel: BCD_PERSIST = 0 (and where the persistent launch does not fit)
_P0 = {'BCD_PERSIST': 0}
_add('f32', 70, 1000, 'l2', L2_SCENES, sw=_P0)
_add('f32', 70, 1000, 'l2', sw=_P0, order='identity')
_add('f32', 70, 1000, 'l2', sw=_P0, order='reversed')
_add('f32', 64, 2048, 'l2', sw=_P0)
_add('f32', 64, 2049, 'l2', ('generic', 'mixed'), sw=_P0)
_add('f32', 256, 3000, 'l2', sw=_P0)
_add('f32', 257, 3000, 'l2', ('generic', 'mixed'), sw=_P0)
_add('f32', 260, 2048, 'l2', sw=_P0)
_add('f32', 260, 2049, 'l2', sw=_P0)
_add('f32', 64, 4096, 'l2', sw=_P0)
_add('f32', 64, 4097, 'l2', sw=_P0)
_add('f32', 64, 4096, 'l2', sw={'BCD_ACC': 0})
_add('f32', 64, 4097, 'l2', sw={'BCD_ACC': 0})
_add('f32', 70, 1000, 'l2', ('generic', 'dead'), sw={'BCD_ACC': 0})
_add('f32', 64, 16384, 'l2')
_add('f32', 64, 16385, 'l2', ('generic', 'mixed', 'zero'))
_add('f32', 1, 1000, 'l2', sw=_P0)
# atom_sweep_kernel: s k <= 32 000
_add('f32', 32, 1000, 'l1', PROJ_SCENES)
_add('f64', 32, 1000, 'enet')
_add('f32', 32, 1000, 'enet_pos', order='identity')
_add('f64', 32, 1000, 'l1_pos', order='reversed')
# the grouped update: EPT 12 / 20 / 24, G = 8 and 4
_add('f32', 32, 1001, 'l1')
_add('f64', 32, 1001, 'enet')
_add('f32', 70, 3500, 'l1', PROJ_SCENES)
_add('f64', 70, 3500, 'enet', ('generic', 'heavy'))
_add('f32', 70, 5500, 'enet_pos', ('generic', 'mixed'))
_add('f64', 30, 5500, 'l1')
_add('f32', 70, 3500, 'l1', order='identity')
_add('f32', 70, 3500, 'l1', order='reversed')
for _s in (3072, 3073, 5120, 5121, 6144):
    _add('f32', 20, _s, 'l1', ('generic', 'mixed') if _s == 3072 else ('generic',))
    _add('f64', 20, _s, 'enet')
_add('f32', 20, 6144, 'enet')
_add('f32', 7, 5000, 'l1_pos')                       # fewer atoms than a group of 8 (and 6 % 4 != 0; see test_route_table for k < 4)
_add('f64', 6, 5400, 'enet')
for _k, _u in ((64, 'l1'), (65, 'l1'), (128, 'enet'), (129, 'l1'), (256, 'enet'), (257, 'enet'), (512, 'l1')):
    _add('f32', _k, 700, _u)
_add('f64', 512, 700, 'enet_pos')
_add('f32', 129, 5200, 'l1')
# the staged sweeps: l1 pipelined (atom_grad4_kernel + atom_corr_project_kernel), elastic-net atoms not pipelined
_add('f32', 10, 7000, 'l1', PROJ_SCENES)
_add('f32', 10, 10500, 'l1', CONTROLLED)
_add('f64', 10, 7000, 'l1_pos', ('heavy',))
_add('f32', 10, 7000, 'l1', CONTROLLED, sw={'ATOM_MWG': 3})
_add('f32', 10, 9000, 'l1', sw={'ATOM_MWG': 3})
_add('f32', 10, 7000, 'l1', CONTROLLED, sw={'ATOM_MWG': 0})
_add('f32', 10, 7000, 'l1', ('generic', 'heavy'), sw={'ATOM_PIPE': 0})
_add('f32', 10, 7000, 'l1', sw={'ATOM_PIPE': 0, 'ATOM_MWG': 3})
_add('f32', 10, 7000, 'l1', sw={'ATOM_PIPE': 0, 'ATOM_MWG': 0})
_add('f32', 10, 7000, 'l1', order='identity')
_add('f32', 10, 7000, 'l1', order='reversed')
for _s in (6145, 10240, 10241, 15360):
    _add('f32', 9, _s, 'l1')
for _s in (8192, 8193):
    _add('f32', 9, _s, 'l1', sw={'ATOM_MWG': 3})
_add('f64', 9, 6145, 'l1')
_add('f64', 9, 7680, 'l1')
_add('f32', 4, 9000, 'l1', ('generic', 'heavy'))
_add('f32', 5, 9000, 'l1')
_add('f32', 200, 6500, 'l1_pos')
_add('f32', 300, 6200, 'l1')
_add('f32', 520, 6200, 'l1')
_add('f32', 10, 7000, 'enet', PROJ_SCENES)
_add('f64', 10, 7000, 'enet_pos', ('generic', 'heavy'))
_add('f32', 10, 7000, 'enet', order='identity')
_add('f32', 10, 7000, 'enet', order='reversed')
for _s in (6145, 10241, 15360):
    _add('f32', 9, _s, 'enet')
_add('f64', 9, 7680, 'enet')
# atom_step_kernel
_add('f32', 6, 15400, 'l1', PROJ_SCENES)
_add('f64', 6, 7700, 'enet')
_add('f32', 6, 15400, 'l1', order='identity')
_add('f32', 6, 15400, 'l1', order='reversed')
_add('f32', 9, 15361, 'l1')
_add('f32', 9, 15361, 'enet')
_add('f64', 9, 7681, 'l1')
_add('f64', 9, 7681, 'enet')
_add('f32', 9, 16384, 'l1')
_add('f32', 9, 16385, 'l1')
_add('f32', 513, 700, 'l1', ('generic', 'dead'))
_add('f64', 513, 700, 'enet')
# sgd
_add('f32', 20, 500, 'sgd', ALL4)
_add('f64', 20, 500, 'sgd')
_add('f64', 1100, 600, 'sgd')


def _kfd_cu_count():
    """compute units of the first GPU as the kernel driver's topology lists them (no HIP call: collection must not open the
    device); 256 (an MI355X) where there is none.
    This only NAMES the route in the test id.  It reads a file format of the amdgpu driver, not of this project, and that
    simd_count / simd_per_cu equals HIP's multiProcessorCount is not guaranteed anywhere: test_route therefore asserts, with
    HIP's own count, that the id names the route the dispatch takes on this device, and fails (it does not guess) where the
    two disagree."""
    base = '/sys/class/kfd/kfd/topology/nodes'
    try:
        for node in sorted(os.listdir(base), key=lambda x: int(x) if x.isdigit() else 0):
            props = {}
            with open(os.path.join(base, node, 'properties')) as f:
                for line in f:
                    kv = line.split()
                    if len(kv) == 2:
                        props[kv[0]] = kv[1]
            simd, per = int(props.get('simd_count', 0)), int(props.get('simd_per_cu', 0) or 0)
            if simd > 0 and per > 0 and int(props.get('cpu_cores_count', 0)) == 0:
                return simd // per
    except (OSError, ValueError):
        pass
    return 256


NCU = _kfd_cu_count()


def case_route(c, ncu=None):
    return expected_route(c.dt, c.k, c.s, c.update, c.sw, NCU if ncu is None else ncu)


def case_id(c):
    sw = ''.join('-%s%d' % (n.lower(), v) for n, v in sorted(c.sw.items()))
    extra = ('' if c.order == 'perm' else '-' + c.order)
    return '%s-k%d-s%d-%s-%s%s%s@%s' % (c.dt, c.k, c.s, c.update, c.scene, sw, extra, case_route(c).replace('/', '.'))


def case_seed(c):
    key = '%s-%d-%d-%s-%s-%s-%s' % (c.dt, c.k, c.s, c.update, c.scene, sorted(c.sw.items()), c.order)
    return zlib.crc32(key.encode()) % 100000


def build(c):
    return make_case(c.dt, c.k, c.s, c.scene, c.update, case_seed(c), order_kind=c.order, sort_subset=c.sort_subset)


# ---------------------------------------------------------------------------------------------------- layer 2: CPU tests
@pytest.mark.parametrize('update', ['l2', 'l1', 'enet', 'enet_pos'])
def test_cases_are_what_they_claim(update):
    k, s = 21, 700
    rho = UPDATES[update].get('comp_l1_ratio', 0.0)

    def run(scene, **kw):
        case = make_case('f64', k, s, scene, update, 11, **kw)
        D, cn = reference(case, np.float64)
        Dr, cnr, sup = restated_update(case)
        check_f64(Dr, cnr, D, cn)                       # (the plain numpy restatement agrees with the oracle: the mutants start from it)
        return case, D, cn, sup

    case, D, cn, _ = run('generic')
    assert case.subset.tolist() != sorted(case.subset.tolist())            # odd seed: an unsorted subset
    assert len(set(case.subset.tolist())) == s and np.linalg.eigvalsh(case.C.astype(np.float64)).min() > -1e-9
    if UPDATES[update].get('comp_pos'):
        assert case.D.min() >= 0
    assert make_case('f64', k, s, 'generic', update, 10).subset.tolist() == sorted(make_case('f64', k, s, 'generic', update, 10).subset)
    assert make_case('f64', k, s, 'generic', update, 11, order_kind='identity').order.tolist() == list(range(k))
    assert make_case('f64', k, s, 'generic', update, 11, order_kind='reversed').order.tolist() == list(range(k))[::-1]

    # inside: budgets left, atoms equal to their candidates (a sweep with unbounded budgets gives the same atoms)
    case, D, cn, _ = run('inside')
    assert cn.min() > 0
    free = SimpleNamespace(**vars(case))
    free.comp_norm = np.full(k, 1e30)
    assert rel_fro(D, reference(free, np.float64)[0]) < 1e-12

    # mixed: along the order, inside atoms (budget left) alternate with atoms that hit their ball (none left)
    case, D, cn, _ = run('mixed')
    assert np.all(cn[case.order[0::2]] > 1e-3) and np.all(np.abs(cn[case.order[1::2]]) < 1e-9)

    # dead: C[j][j] == 0, rows unchanged; first, last and two adjacent positions of the order
    case, D, cn, _ = run('dead')
    where = sorted(int(np.nonzero(case.order == j)[0][0]) for j in case.special)
    assert where[0] == 0 and where[-1] == k - 1 and np.any(np.diff(where) == 1)
    assert np.all(np.diag(case.C)[case.special] == 0)
    np.testing.assert_array_equal(D[case.special], case.D[case.special])

    # zero: radius 0, rows exactly 0 on the subset
    case, D, cn, _ = run('zero')
    assert np.all(case.comp_norm[case.special] == 0) and len(case.special) >= 2
    assert np.all(D[np.ix_(case.special, case.subset)] == 0) and np.all(cn[case.special] == 0)

    for scene in CONTROLLED:
        case, D, cn, sup = run(scene)
        assert np.count_nonzero(case.C - np.diag(np.diag(case.C))) == 0
        plain = [j for j in range(k) if case.kinds[j] == scene]
        cand = case.B[:, case.subset] / np.diag(case.C)[:, None]
        if UPDATES[update].get('comp_pos'):
            cand = np.maximum(cand, 0)
        copies = [j for j in range(k) if case.kinds[j] == 'copy']
        np.testing.assert_array_equal(D[np.ix_(copies, case.subset)], cand[copies])       # the copy branch, bit for bit
        for g in range(0, k - 3, 4):                    # every group of four holds a copied and a projected atom
            assert len(set(case.kinds[case.order[g:g + 4]])) == 2 or scene == 'copy'
        if scene == 'spike' and rho != 0.0:
            assert all(sup[j] == 1 for j in plain)
            assert all(np.count_nonzero(D[j, case.subset]) == 1 for j in plain)
        # (at the level itself the support is a matter of rounding unless every sum is exact: l1 only)
        if (scene == 'ties' and rho != 0.0) or (scene == 'ties_at_level' and rho == 1.0):
            a = 2.0 ** -6
            top = 2 * a if scene == 'ties' else 4 * a
            for j in plain:
                assert sup[j] == np.count_nonzero(np.abs(cand[j]) == top)
        if scene == 'flat' and rho != 0.0:
            for j in plain:
                assert len(np.unique(np.abs(D[j, case.subset]))) == 1 and sup[j] == s
        if scene == 'boundary':
            for j in plain:
                n = _orc.enet_norm(np.ascontiguousarray(cand[j]), rho)
                assert abs(case.comp_norm[j] - n) <= np.spacing(n)
            assert len(set(np.sign(case.comp_norm[j] - _orc.enet_norm(np.ascontiguousarray(cand[j]), rho)) for j in plain)) == 3


def test_heavy_scene_and_the_pass_cap():
    """`heavy` needs at least twice the passes of a generic vector; the bounded search for an input beyond kMwgMaxPass = 23
    passes (module docstring) ends below the cap."""
    s = 16384
    heavy, R = _controlled_vector('heavy', s, 1.0, np.random.RandomState(0), np.float64)
    p_heavy, _ = michelot_passes(heavy, R)
    gen = make_case('f64', 4, s, 'generic', 'l1', 3)
    Ds = gen.D[:, gen.subset]
    cand = (gen.B[:, gen.subset] - gen.C.dot(Ds) + np.diag(gen.C)[:, None] * Ds) / np.diag(gen.C)[:, None]
    p_gen = max(michelot_passes(cand[j], enet_norm64(Ds[j], 1.0))[0] for j in range(4))
    print('passes: heavy %d, generic %d' % (p_heavy, p_gen))
    assert p_heavy >= 2 * p_gen and p_heavy >= 15
    assert michelot_passes(heavy.astype(np.float32).astype(np.float64), R)[0] >= 15
    found = {}
    for name, dt in (('f64', np.float64), ('f32', np.float32)):
        v, R = adversarial_michelot_vector(dt)
        found[name] = michelot_passes(v.astype(np.float64), R)[0]
        pad = np.concatenate([v.astype(np.float64), np.zeros(s - len(v))])   # (zeros never enter the active set)
        assert michelot_passes(pad, R)[0] == found[name]
    # piecewise-geometric plateaus: more elements per level only enlarge the active count c, i.e. the factor (c - 1) per pass
    for ratio in (0.5, 0.7, 0.9):
        for width in (1, 4, 64):
            v = np.repeat(ratio ** np.arange(s // width), width)[:s]
            for R in (1e-3, 1e-6, 1.0):
                found['plateau'] = max(found.get('plateau', 0), michelot_passes(v, R)[0])
    print('search:', found)
    assert max(found.values()) <= 22, found            # kMwgMaxPass = 23 is out of reach: no `over_cap` scene


# ---- the route table
ROUTES_REQUIRED = [
    'tiny', 'few/nfew7', 'few/nfew16', 'few/nfew64', 'unfused', 'persist/RT1', 'persist/RT2',
    'block/RT1/GPW8/acc1/shards1', 'block/RT1/GPW16/acc1/shards1', 'block/RT1/GPW16/acc1/shards4', 'block/RT2/GPW8/acc1/shards1',
    'block/RT2/GPW8/acc1/shards4', 'block/RT3/GPW8/acc1/shards4', 'block/RT2/GPW8/acc0/shards1', 'block/RT2/GPW8/acc0/shards4',
    'block/RT1/GPW8/acc0/shards1', 'sweep',
    'grouped/EPT12/G8/KPL1/l1', 'grouped/EPT12/G8/KPL1/enet', 'grouped/EPT20/G8/KPL1/l1', 'grouped/EPT20/G8/KPL1/enet',
    'grouped/EPT24/G4/KPL1/l1', 'grouped/EPT24/G4/KPL1/enet', 'grouped/EPT12/G8/KPL2/l1', 'grouped/EPT12/G8/KPL2/enet',
    'grouped/EPT12/G8/KPL4/l1', 'grouped/EPT12/G8/KPL8/l1', 'grouped/EPT12/G8/KPL8/enet', 'grouped/EPT24/G4/KPL2/enet',
    'grouped/EPT24/G4/KPL4/l1',
    'staged_pipe/KPL1/regs40', 'staged_pipe/KPL1/regs64', 'staged_pipe/KPL1/spread/ept1', 'staged_pipe/KPL1/spread/ept2',
    'staged_pipe/KPL4/regs40', 'staged_pipe/KPL8/regs40', 'staged_pipe/KPL16/regs40',
    'staged/grad4KPL1/spread', 'staged/grad4KPL1/lds_l1', 'staged/grad4KPL1/lds_enet',
    'step/KPL1/global', 'step/KPL16/lds', 'sgd', 'wide',
]

# (what, the fields both neighbours share, (s or k below, its route prefix), (s or k above, its route prefix))
BOUNDARIES = [
    ('tiny | few', dict(dt='f64', update='l2'), ('s', 192, 'tiny'), ('s', 193, 'few')),
    ('few | unfused', dict(dt='f64', update='l2'), ('s', 2048, 'few/nfew64'), ('s', 2049, 'unfused')),
    ('fused | unfused', dict(dt='f32', update='l2'), ('k', 512, 'persist'), ('k', 513, 'unfused')),
    ('persistent RT 1 | 2', dict(dt='f32', update='l2', k=64), ('s', 8160, 'persist/RT1'), ('s', 8161, 'persist/RT2')),
    ('persistent RT 2 | block', dict(dt='f32', update='l2', k=64), ('s', 16320, 'persist/RT2'), ('s', 16321, 'block/RT2')),
    ('persistent kp 256 | 260', dict(dt='f32', update='l2', s=9000), ('k', 256, 'persist/RT2'), ('k', 257, 'block/RT1/GPW16')),
    ('block RT 1 | 2', dict(dt='f32', update='l2', k=64), ('s', 2048, 'block/RT1'), ('s', 2049, 'block/RT2')),
    ('block RT 2 | 3', dict(dt='f32', update='l2', k=64), ('s', 16384, 'block/RT2'), ('s', 16385, 'block/RT3')),
    ('block GPW 8 | 16', dict(dt='f32', update='l2', s=3000), ('k', 256, 'block/RT2/GPW8'), ('k', 257, 'block/RT1/GPW16')),
    ('block shards, RT 1', dict(dt='f32', update='l2', k=260), ('s', 2048, 'block/RT1/GPW16/acc1/shards1'),
     ('s', 2049, 'block/RT1/GPW16/acc1/shards4')),
    ('block shards, RT 2', dict(dt='f32', update='l2', k=64), ('s', 4096, 'block/RT2/GPW8/acc1/shards1'),
     ('s', 4097, 'block/RT2/GPW8/acc1/shards4')),
    ('block shards, no accumulator', dict(dt='f32', update='l2', k=64), ('s', 4096, 'block/RT2/GPW8/acc0/shards1'),
     ('s', 4097, 'block/RT2/GPW8/acc0/shards4')),
    ('persistent k 31 | 32', dict(dt='f32', update='l2', s=1000), ('k', 31, 'persist'), ('k', 32, 'persist')),
    ('persistent k 32 | 33', dict(dt='f32', update='l2', s=1000), ('k', 32, 'persist'), ('k', 33, 'persist')),
    ('persistent k 255 | 256', dict(dt='f32', update='l2', s=1000), ('k', 255, 'persist'), ('k', 256, 'persist')),
    ('persistent k 256 | 257', dict(dt='f32', update='l2', s=1000), ('k', 256, 'persist'), ('k', 257, 'persist')),
    ('sweep | grouped', dict(dt='f32', update='l1', k=32), ('s', 1000, 'sweep'), ('s', 1001, 'grouped')),
    ('sweep | grouped', dict(dt='f64', update='enet', k=32), ('s', 1000, 'sweep'), ('s', 1001, 'grouped')),
    ('EPT 12 | 20', dict(dt='f32', update='l1', k=20), ('s', 3072, 'grouped/EPT12/G8'), ('s', 3073, 'grouped/EPT20/G8')),
    ('EPT 12 | 20', dict(dt='f64', update='enet', k=20), ('s', 3072, 'grouped/EPT12/G8'), ('s', 3073, 'grouped/EPT20/G8')),
    ('EPT 20 | 24', dict(dt='f32', update='l1', k=20), ('s', 5120, 'grouped/EPT20/G8'), ('s', 5121, 'grouped/EPT24/G4')),
    ('EPT 20 | 24', dict(dt='f64', update='enet', k=20), ('s', 5120, 'grouped/EPT20/G8'), ('s', 5121, 'grouped/EPT24/G4')),
    ('grouped | staged', dict(dt='f32', update='l1'), ('s', 6144, 'grouped/EPT24'), ('s', 6145, 'staged_pipe')),
    ('grouped | staged', dict(dt='f32', update='enet'), ('s', 6144, 'grouped/EPT24'), ('s', 6145, 'staged/')),
    ('grouped | staged', dict(dt='f64'), ('s', 6144, 'grouped/EPT24'), ('s', 6145, 'staged')),
    ('KPL 1 | 2', dict(dt='f32', s=700), ('k', 64, 'grouped/EPT12/G8/KPL1'), ('k', 65, 'grouped/EPT12/G8/KPL2')),
    ('KPL 2 | 4', dict(dt='f32', s=700), ('k', 128, 'grouped/EPT12/G8/KPL2'), ('k', 129, 'grouped/EPT12/G8/KPL4')),
    ('KPL 4 | 8', dict(dt='f32', s=700), ('k', 256, 'grouped/EPT12/G8/KPL4'), ('k', 257, 'grouped/EPT12/G8/KPL8')),
    ('grouped | step at k', dict(dt='f32', s=700), ('k', 512, 'grouped/EPT12/G8/KPL8'), ('k', 513, 'step/KPL16')),
    ('regs 40 | 64', dict(dt='f32', update='l1', k=9), ('s', 10240, 'staged_pipe/KPL1/regs40'), ('s', 10241, 'staged_pipe/KPL1/regs64')),
    ('spread ept 1 | 2', dict(dt='f32', update='l1', k=9), ('s', 8192, 'staged_pipe/KPL1/spread/ept1'),
     ('s', 8193, 'staged_pipe/KPL1/spread/ept2')),
    ('one group | two', dict(dt='f32', update='l1', s=9000), ('k', 4, 'staged/grad4KPL1/spread'), ('k', 5, 'staged_pipe/KPL1/regs40')),
    ('LDS limit f32, l1', dict(dt='f32', update='l1', k=9), ('s', 15360, 'staged_pipe'), ('s', 15361, 'step/KPL1/global')),
    ('LDS limit f32, enet', dict(dt='f32', update='enet', k=9), ('s', 15360, 'staged/grad4KPL1/lds_enet'), ('s', 15361, 'step/KPL1/global')),
    ('LDS limit f64, l1', dict(dt='f64', update='l1', k=9), ('s', 7680, 'staged_pipe'), ('s', 7681, 'step/KPL1/global')),
    ('LDS limit f64, enet', dict(dt='f64', update='enet', k=9), ('s', 7680, 'staged/grad4KPL1/lds_enet'), ('s', 7681, 'step/KPL1/global')),
    ('64 elements per thread', dict(dt='f32', update='l1', k=9), ('s', 16384, 'step/KPL1/global'), ('s', 16385, 'step/KPL1/global')),
]


FAMILIES = ('tiny', 'few', 'unfused', 'persist', 'block', 'sweep', 'grouped', 'staged_pipe', 'staged', 'step', 'sgd', 'wide')


def hold_restatement_to_library(put, ncu):
    """expected_route == modl_dict_update_route on ncu compute units (the built library, no device): every case of the matrix
    under its switches, both neighbours of every boundary, every combination of SWITCH_VALUES at one shape per family.
    put: the debug_switches fixture.  Returns the number of comparisons."""
    import itertools
    count = [0]

    def same(dt, k, s, update, sw):
        full = switch_defaults()
        full.update(sw)
        put(full)
        want, got = expected_route(dt, k, s, update, sw, ncu), library_route(dt, k, s, update, ncu)
        assert got == want, 'the library takes %s, the restatement says %s: %s' % (got, want, (dt, k, s, update, sw, ncu))
        count[0] += 1
        return got

    for c in CASES:
        same(c.dt, c.k, c.s, c.update, c.sw)
    for what, shared, lo, hi in BOUNDARIES:
        for field, value, prefix in (lo, hi):
            want = dict(shared)
            want[field] = value
            hits = [c for c in CASES if all(getattr(c, f) == v for f, v in want.items())]
            got = [same(c.dt, c.k, c.s, c.update, c.sw) for c in hits]
            assert hits and (ncu != 256 or any(r.startswith(prefix) for r in got)), (what, want, prefix, got)
    shapes = {}
    for dt, k, s, update in [(c.dt, c.k, c.s, c.update) for c in CASES] + [('f64', 1100, 1000, 'l1')]:
        shapes.setdefault(expected_route(dt, k, s, update, dict(BCD_ACC=1), ncu).split('/')[0], (dt, k, s, update))
    assert set(shapes) == set(FAMILIES), sorted(shapes)
    names = sorted(SWITCH_VALUES)
    for values in itertools.product(*(SWITCH_VALUES[n] for n in names)):
        for shape in shapes.values():
            same(*shape, dict(zip(names, values)))
    return count[0]


def test_route_table(debug_switches):
    """The matrix holds every route and both neighbours of every boundary (on the 256 compute units of an MI355X), and the
    library's du_route takes the routes this module says it takes."""
    ncmp = hold_restatement_to_library(debug_switches, 256)
    assert ncmp >= len(CASES) + 2 * len(BOUNDARIES) + 96 * len(FAMILIES), ncmp
    routes = [case_route(c, 256) for c in CASES]
    missing = [r for r in ROUTES_REQUIRED if r not in routes and r != 'wide']
    assert not missing, missing
    assert expected_route('f64', 1100, 1000, 'l1') == 'wide' and expected_route('f64', 1100, 600, 'sgd') == 'sgd'   # (wide: test_wide_components.py)
    for what, shared, lo, hi in BOUNDARIES:
        for field, value, prefix in (lo, hi):
            want = dict(shared)
            want[field] = value
            hit = [c for c, r in zip(CASES, routes) if all(getattr(c, f) == v for f, v in want.items()) and r.startswith(prefix)]
            assert hit, (what, want, prefix)
    # scenes per route family: every family with generic, mixed, dead and zero; the projecting ones with every controlled scene; l2 with
    # inside, boundary, flat
    fam = {}
    for c, r in zip(CASES, routes):
        fam.setdefault(r.split('/')[0], set()).add(c.scene)
    for f, scenes in fam.items():
        assert set(ALL4) <= scenes, (f, scenes)
        if f in ('sweep', 'grouped', 'staged_pipe', 'staged', 'step'):
            assert set(CONTROLLED) <= scenes, (f, scenes)
        if f in ('tiny', 'few', 'unfused', 'persist', 'block'):
            assert {'inside', 'boundary', 'flat'} <= scenes, (f, scenes)
    # every launch variant meets `mixed`: each RT of the persistent launch and of bcd_block_kernel, each EPT / G of the grouped update
    for variant in ('persist/RT1', 'persist/RT2', 'block/RT1', 'block/RT2', 'block/RT3', 'grouped/EPT12/G8', 'grouped/EPT20/G8',
                    'grouped/EPT24/G4'):
        got = set(c.scene for c, r in zip(CASES, routes) if r.startswith(variant))
        assert {'generic', 'mixed'} <= got, (variant, got)
    # fewer atoms than a group of the grouped update.  G = 8: 7 atoms.  G = 4 (5120 < s <= 6144) cannot be entered with fewer than
    # four: s k <= 3 * 6144 < 32 000 and the vector fits the LDS in both types, so atom_sweep_kernel takes every such update
    assert any(r.startswith('grouped') and '/G8/' in r and c.k < 8 for c, r in zip(CASES, routes))
    assert any(r.startswith('grouped') and '/G4/' in r and c.k % 4 for c, r in zip(CASES, routes))
    for dt_ in DT:
        for upd in ('l1', 'enet', 'l1_pos', 'enet_pos'):
            assert all(expected_route(dt_, k_, s_, upd) == 'sweep' for k_ in (1, 2, 3) for s_ in (5121, 6144))
    # each projection of the staged sweeps (registers, spread, LDS copy) meets every controlled scene
    for variant in ('regs40', 'regs64', 'spread/ept1', 'lds_l1', 'lds_enet'):
        got = set(c.scene for c, r in zip(CASES, routes) if r.endswith(variant))
        assert set(CONTROLLED) <= got, (variant, got)
    # identity and reversed orders, sorted and unsorted subsets
    for f in fam:
        kinds = set(c.order for c, r in zip(CASES, routes) if r.split('/')[0] == f)
        assert {'identity', 'reversed'} <= kinds or f in ('sgd',), (f, kinds)
    unsorted = sum(case_seed(c) % 2 for c in CASES)
    assert 0.35 * len(CASES) < unsorted < 0.65 * len(CASES)
    for c in CASES:
        for name, v in c.sw.items():
            assert v in SWITCH_VALUES[name]
    assert len(set(case_id(c) for c in CASES)) == len(CASES) and 150 <= len(CASES) <= 250, len(CASES)
    assert sum(1 for c in CASES if c.k * c.k * c.s >= 512 * 512 * 8000) <= 12
    print('%d cases, %d routes, %d comparisons with the library' % (len(CASES), len(set(routes)), ncmp))


def test_route_table_on_128_compute_units(debug_switches):
    """The same comparison where the boundaries that depend on the device move: RT 2 | 3 of bcd_block_kernel at s = 64 ncu
    and 96 ncu, the persistent launch at 32 (ncu - 1) sampled rows (RT 1) and 64 (ncu - 1) (RT 2).  Then what the probe
    refuses."""
    import ctypes as C
    from modl_amd import _lib
    ncu = 128
    hold_restatement_to_library(debug_switches, ncu)
    on = dict(BCD_ACC=1, BCD_PERSIST=1)
    moved = {32 * (ncu - 1): 'persist/RT1', 32 * (ncu - 1) + 1: 'persist/RT2', 64 * (ncu - 1): 'persist/RT2',
             64 * (ncu - 1) + 1: 'block/RT2/GPW8/acc1/shards4', 64 * ncu: 'block/RT2/GPW8/acc1/shards4',
             64 * ncu + 1: 'block/RT3/GPW8/acc1/shards4', 96 * ncu: 'block/RT3/GPW8/acc1/shards4',
             96 * ncu + 1: 'block/RT2/GPW8/acc1/shards4'}
    for s, route in moved.items():
        for k in (64, 260):                              # (kp > 256: RT 1 only, in one launch or per block)
            for sw in (on, dict(on, BCD_PERSIST=0), dict(on, BCD_ACC=0)):
                debug_switches(dict(switch_defaults(), **sw))
                got = library_route('f32', k, s, 'l2', ncu)
                assert got == expected_route('f32', k, s, 'l2', sw, ncu), (k, s, sw, got)
                if k == 64 and sw is on:
                    assert got == route, (s, got, route)
    assert all(expected_route('f32', 64, s, 'l2', on, 256) != moved[s] for s in (32 * (ncu - 1) + 1, 64 * (ncu - 1) + 1, 64 * ncu + 1))
    buf = C.create_string_buffer(64)
    probe = _lib.lib.modl_dict_update_route
    debug_switches(dict(switch_defaults(), **on))
    assert probe(_lib.MODL_F32, 64, 1000, 0, 0, 0.0, ncu, buf, 64) == 0 and buf.value == b'persist/RT1'
    assert probe(_lib.MODL_F32, 64, 1000, 0, 0, 0.0, ncu, buf, len('persist/RT1')) == -1          # no room for the terminator
    for bad in ((2, 64, 1000, 0, 0, 0.0, ncu, buf, 64), (_lib.MODL_F32, 0, 1000, 0, 0, 0.0, ncu, buf, 64),
                (_lib.MODL_F32, 4097, 1000, 0, 0, 0.0, ncu, buf, 64), (_lib.MODL_F32, 64, 0, 0, 0, 0.0, ncu, buf, 64),
                (_lib.MODL_F32, 64, 1000, 0, 0, 0.0, -1, buf, 64), (_lib.MODL_F32, 64, 1000, 0, 0, 0.0, ncu, None, 64)):
        assert probe(*bad) == -1, bad


def clipped_and_copied(case, cn64):
    """(atoms the oracle's l2 projection scaled back onto their ball: no budget left; atoms it copied: budget left)"""
    scale = np.asarray(case.comp_norm, dtype=np.float64) + np.sum(case.D[:, case.subset].astype(np.float64) ** 2, axis=1)
    return int(np.sum(np.abs(cn64) < 1e-9 * scale)), int(np.sum(cn64 > 1e-3 * scale))


def test_l2_cases_clip_and_copy():
    """Every l2 route of ROUTES_REQUIRED and every l2 neighbour of BOUNDARIES has a case in which the oracle scales at least
    one atom back onto its ball and copies at least one: both branches of the l2 projection run on either side of every
    boundary (with the recipe's gain of 0.9 alone none of them clipped anything).  The cheapest such case is run."""
    routes = [case_route(c, 256) for c in CASES]
    l2 = [(c, r) for c, r in zip(CASES, routes) if c.update == 'l2' and c.k > 1]
    l2.sort(key=lambda cr: cr[0].k * cr[0].k * cr[0].s)
    wanted = [[(c, r) for c, r in l2 if r == req] for req in ROUTES_REQUIRED
              if req.split('/')[0] in ('tiny', 'few', 'unfused', 'persist', 'block')]
    for what, shared, lo, hi in BOUNDARIES:
        if shared.get('update') == 'l2':
            for field, value, prefix in (lo, hi):
                want = dict(shared)
                want[field] = value
                wanted.append([(c, r) for c, r in l2 if all(getattr(c, f) == v for f, v in want.items()) and r.startswith(prefix)])
    seen = {}
    for hits in wanted:
        assert hits
        ok = False
        for c, r in hits:
            if case_id(c) not in seen:
                case = build(c)
                seen[case_id(c)] = clipped_and_copied(case, reference(case, np.float64)[1])
            nclip, ncopy = seen[case_id(c)]
            if nclip >= 1 and ncopy >= 1:
                ok = True
                break
        assert ok, [(case_id(c), seen[case_id(c)]) for c, r in hits]
    print('%d l2 cases run: %s' % (len(seen), sorted(seen.values())[:3]))


# ---- the acceptance rules have teeth
MUTANT_CASES = [('l2 blocked', 70, 1000, 'l2'), ('grouped l1', 70, 3500, 'l1'), ('per-atom enet', 10, 7000, 'enet')]
MUTANT_BOOST = 1.0           # added to C's diagonal of these cases (make_case's default: the conditioning of layer 3)


@pytest.mark.parametrize('name,k,s,update', MUTANT_CASES, ids=[m[0].replace(' ', '_') for m in MUTANT_CASES])
def test_acceptance_rule_rejects_mutants(name, k, s, update):
    case = make_case('f32', k, s, 'generic', update, 5, diag_boost=MUTANT_BOOST)
    D64, cn64 = reference(case, np.float64)
    D32, cn32 = reference(case, np.float32)
    D0, cn0, sup = restated_update(case)
    # the unmutated restatement passes both rules (so a rejection below is the mutation's doing)
    check_f64(D0, cn0, D64, cn64)
    check_f32(D0.astype(np.float32), cn0.astype(np.float32), D32, cn32, D64, cn64)
    order = case.order
    # an atom that the projection moves (outside its ball), in the middle of the sweep
    moved = [int(j) for j in order if abs(cn64[j]) < 1e-9]
    assert moved, 'no atom of this case hits its ball'
    jm = moved[len(moved) // 2]
    mutants = {}
    mutants['one atom left unprojected'] = restated_update(case, skip_projection=jm)[:2]
    sw = SimpleNamespace(**vars(case))
    sw.order = order.copy()
    # (two neighbours that C couples most strongly: for atoms with C[i][j] == 0 the order does not matter)
    t = int(np.argmax(np.abs(case.C[order[:-1], order[1:]])))
    sw.order[[t, t + 1]] = sw.order[[t + 1, t]]
    mutants['two atoms of the order swapped'] = restated_update(sw)[:2]
    sh = SimpleNamespace(**vars(case))
    sh.subset = (case.subset + 1) % case.p
    mutants['subset shifted by one feature'] = restated_update(sh)[:2]
    mutants['comp_norm not decremented for one atom'] = restated_update(case, keep_budget=jm)[:2]
    if update != 'l2':                                  # (the l2 projection has no threshold)
        mutants['soft threshold off by 1e-4'] = restated_update(case, level_factor=1.0 + 1e-4)[:2]
    tail = case.subset[s - s % 256:]
    assert len(tail) > 0
    Dt = D0.copy()
    Dt[:, tail] = case.D[:, tail]
    mutants['the last s % 256 features not written'] = (Dt, cn0)
    survivors = []
    for what, (Dm, cnm) in mutants.items():
        if accepts(check_f64, Dm, cnm, D64, cn64):
            survivors.append(('f64', what))
        if accepts(check_f32, Dm.astype(np.float32), cnm.astype(np.float32), D32, cn32, D64, cn64):
            survivors.append(('f32', what, rel_fro(Dm, D64), rel_fro(D32, D64), rel_fro(cnm, cn64), rel_fro(cn32, cn64)))
    print('%s: %d mutants, %d survive' % (name, 2 * len(mutants), len(survivors)))
    assert not survivors, survivors


# ---------------------------------------------------------------------------------------------------- layer 3: GPU tests
@pytest.fixture(scope='module')
def gpu():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    return torch


@pytest.fixture
def debug_switches():
    """sets the dictionary update's debug switches; the defaults are back when the test ends, however it ends"""
    from modl_amd import _lib

    def put(values):
        for name, v in values.items():
            assert v in SWITCH_VALUES[name], (name, v)
            _lib.check(_lib.lib.modl_debug_set(getattr(_lib, 'DEBUG_' + name), int(v)), 'modl_debug_set')
    try:
        yield put
    finally:
        put(switch_defaults())


def run_gpu(case):
    """modl_dict_update_* on the case: (Dt (p, k) as the device left it, comp_norm)"""
    import ctypes as C
    import torch
    from modl_amd._lib import lib, check
    from modl_amd.device import dtype_id, sfx, ptr
    dt, k, s = case.dt, case.k, case.s
    u = UPDATES[case.update]
    dev = torch.device('cuda')
    Dt = torch.from_numpy(np.ascontiguousarray(case.D.T)).to(dev)
    Bt = torch.from_numpy(np.ascontiguousarray(case.B.T)).to(dev)
    Cd = torch.from_numpy(np.ascontiguousarray(case.C)).to(dev)
    cn = torch.from_numpy(np.asarray(case.comp_norm).copy()).to(dev)
    dsub = torch.from_numpy(case.subset.astype(np.int32)).to(dev)
    order = np.ascontiguousarray(case.order, dtype=np.int64)
    dord = torch.from_numpy(order.astype(np.int32)).to(dev)
    nbytes = lib.modl_dict_update_workspace(dtype_id(dt), s, k)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    f = getattr(lib, 'modl_dict_update_' + sfx(dt))
    check(f(ptr(Dt), ptr(Bt), ptr(Cd), ptr(cn), ptr(dsub), s, ptr(dord), order.ctypes.data_as(C.POINTER(C.c_int64)), k,
            1 if u.get('optimizer') == 'sgd' else 0, int(u.get('comp_pos', False)), u.get('comp_l1_ratio', 0.0), case.w,
            params(case.update).step_size, ptr(ws), nbytes, None), 'modl_dict_update')
    torch.cuda.synchronize()
    return Dt.cpu().numpy(), cn.cpu().numpy()


def dict_update_case(oracle, k, s, dt, optimizer='variational', comp_l1_ratio=0.0, comp_pos=False, seed=0):
    """The generic scene with a sorted subset through the GPU and the oracle: (D, comp_norm, D_oracle, comp_norm_oracle).
    (test_wide_components.py: more than 1024 atoms.)"""
    update = [name for name, u in UPDATES.items()
              if (u.get('optimizer', 'variational'), u.get('comp_l1_ratio', 0.0), u.get('comp_pos', False)) ==
              (optimizer, comp_l1_ratio, comp_pos)]
    assert len(update) == 1, (optimizer, comp_l1_ratio, comp_pos)
    case = make_case(dt, k, s, 'generic', update[0], seed, sort_subset=True, diag_boost=0.0, noise=0.01, gain=0.9)
    Dt, cn = run_gpu(case)
    D_orc, cn_orc = reference(case, case.dt)
    return Dt.T, cn, D_orc, cn_orc


def _judge(c, case, Dt, cn, refs):
    D = Dt.T
    outside = np.setdiff1d(np.arange(case.p), case.subset)
    np.testing.assert_array_equal(D[:, outside], case.D[:, outside], err_msg='rows of Dt outside the subset were written')
    if c.dt == 'f64':
        D64, cn64 = refs['f64']
        err = rel_fro(D, D64)
        print('rel_fro D %.3e  max |comp_norm diff| %.3e' % (err, np.max(np.abs(cn - cn64))))
        check_f64(D, cn, D64, cn64)
    else:
        (D32, cn32), (D64, cn64) = refs['f32'], refs['f64']
        print('D: err %.3e noise %.3e   comp_norm: err %.3e noise %.3e' % (rel_fro(D, D64), rel_fro(D32, D64), rel_fro(cn, cn64),
                                                                         rel_fro(cn32, cn64)))
        check_f32(D, cn, D32, cn32, D64, cn64)
    ref_own = refs[c.dt][0]
    sub = case.subset
    if c.scene == 'zero':
        assert np.all(D[np.ix_(case.special, sub)] == 0), 'an atom of radius 0 is not exactly zero'
        assert np.all(cn[case.special] == 0)
    if c.scene == 'dead' and c.update != 'sgd':
        np.testing.assert_array_equal(D[case.special], case.D[case.special], err_msg='a dead atom (C[j][j] == 0) changed')
    if c.scene in CONTROLLED and c.update in ('l1', 'enet', 'l1_pos', 'enet_pos'):
        copies = [j for j in range(case.k) if case.kinds[j] == 'copy']
        np.testing.assert_array_equal(D[np.ix_(copies, sub)], ref_own[np.ix_(copies, sub)],
                                      err_msg='an atom inside its ball is not a copy of its candidate')


@pytest.mark.gpu
@pytest.mark.parametrize('c', CASES, ids=case_id)
def test_route(gpu, debug_switches, c):
    ncu = gpu.cuda.get_device_properties(0).multi_processor_count
    route = case_route(c, ncu)
    assert route == case_route(c), 'the test id names the route of %d compute units, the device has %d: %s' % (NCU, ncu, route)
    case = build(c)
    refs = {'f64': reference(case, np.float64)}
    if c.dt == 'f32':
        refs['f32'] = reference(case, np.float32)
    debug_switches(c.sw)
    took = library_route(c.dt, c.k, c.s, c.update, 0)
    assert took == case_route(c), 'the test id names %s, on this device the library takes %s' % (case_route(c), took)
    Dt, cn = run_gpu(case)
    try:
        _judge(c, case, Dt, cn, refs)
    except AssertionError as first:
        if not route.startswith('persist'):
            raise
        # a direct call carries no plan: a persistent launch that gave up cannot say so.  Once more, one launch per block
        debug_switches({'BCD_PERSIST': 0})
        Dt2, cn2 = run_gpu(case)
        try:
            _judge(c, case, Dt2, cn2, refs)
            second = 'passes with BCD_PERSIST = 0 (bcd_block_kernel): the persistent launch alone is wrong or was not resident'
        except AssertionError as again:
            second = 'fails with BCD_PERSIST = 0 as well (arithmetic, not residency): %s' % (again,)
        raise AssertionError('persistent launch: %s\n%s' % (first, second))
