"""GPU parity of the fused minibatch step / the estimator against the golden
trajectories of the reference, the CPU oracle, and the reference's own
functional tests (modl/decomposition/tests/test_dict_fact.py)."""
import numpy as np
import pytest
from numpy.testing import assert_array_equal

from .conftest import load_golden, rel_fro
from .test_oracle_golden import small_case_params, synth, _cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def DictFact():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    from modl_amd import DictFact
    return DictFact


class Recorder:
    """records per-minibatch subsets / codes of a modl_amd.DictFact run"""

    def __init__(self, est):
        self.est, self.subsets, self.codes = est, [], []
        smp = est.feature_sampler_
        rec = self

        class Proxy:
            def yield_subset(_, r):
                s = smp.yield_subset(r)
                rec.subsets.append(s.copy())
                return s
        est.feature_sampler_ = Proxy()


@pytest.mark.parametrize('name', _cases())
def test_trajectory_small_golden(DictFact, oracle, name):
    """All aggregation modes / optimizers / atom constraints: the whole fit, against what the
    reference produced (tests/golden/traj_small.npz).  f32 end states: within the reference's own f32 noise while every
    sample did the f64 oracle's number of sweeps; a sample whose duality gap sits on the threshold may legitimately do one
    sweep more or less when its inputs differ in the last bits (these small cases have samples at 80 - 90 of max_iter = 100
    sweeps) - such flips are located with the sweep history, bounded, and allow 6e-5 more, as in the long-horizon test."""
    g = load_golden('traj_small')
    kw, X, dt = small_case_params(name)
    est = DictFact(**kw)
    est.prepare(n_samples=X.shape[0], X=X)
    rec = Recorder(est)
    nmb = kw['n_epochs'] * -(-X.shape[0] // kw['batch_size'])
    hist = est._backend.sweeps_history(nmb) if dt == np.float32 and hasattr(est._backend, 'sweeps_history') else None
    Xh = X
    first_codes = None
    for ep in range(kw['n_epochs']):
        if ep == 0:
            # first minibatch alone, to compare its codes
            est.partial_fit(Xh[:kw['batch_size']], np.arange(kw['batch_size']))
            first_codes = est.code_[:kw['batch_size']].copy()
            est.partial_fit(Xh[kw['batch_size']:], np.arange(kw['batch_size'], X.shape[0]))
        else:
            est.partial_fit(Xh)
        perm = est.shuffle()
        Xh = Xh[perm]
    assert_array_equal(np.concatenate(rec.subsets), g[name + '/subset'])          # bit-exact draws
    nb0 = int(g[name + '/code_len'][0])
    tol = 2e-5 if dt == np.float32 else 1e-9
    assert rel_fro(first_codes, g[name + '/code'][:nb0]) < tol
    if dt == np.float64:
        assert rel_fro(est.components_, g[name + '/D_final']) < tol
        assert rel_fro(est.C_, g[name + '/C_final']) < tol
        assert rel_fro(est.B_, g[name + '/B_final']) < tol
        assert rel_fro(est.code_, g[name + '/code_final']) < tol
        if (name + '/G_final') in g:
            assert rel_fro(est.G_, g[name + '/G_final']) < tol
    else:
        # f32 end state (two epochs): float summation order is unpinned, so the yardstick is the
        # reference's OWN f32 noise - its f32 run against its f64 run of the same case - not a flat tolerance
        ref64 = name[:-3] + 'f64'
        flips = 0
        if hist is not None and kw.get('code_l1_ratio', 1) != 0:
            sw64 = oracle.fit(oracle.SomfParams(**kw), X.astype(np.float64), sweeps=True).sweeps
            sw = hist()
            flips = sum(int((sw[t, :len(a)] != a).sum()) for t, a in enumerate(sw64))
            assert flips <= max(1, 5e-3 * sum(len(a) for a in sw64)), flips
        for key, val in (('D_final', est.components_), ('code_final', est.code_), ('C_final', est.C_)):
            noise = rel_fro(g[name + '/' + key], g[ref64 + '/' + key])
            err = rel_fro(val, g[ref64 + '/' + key])
            assert err <= 2 * noise + 1e-5 + (6e-5 if flips else 0.0), (key, err, noise, flips)
    assert est.n_iter_ == int(g[name + '/n_iter'])


def test_config1_golden(DictFact):
    """BASELINE config 1 on the GPU path (2000 x 500, k = 16, r = 1, f64)."""
    g = load_golden('traj_c1')
    X = synth(2000, 500, 16, 0, np.float64)
    est = DictFact(n_components=16, reduction=1, random_state=0, n_epochs=1, code_alpha=1e-4)
    est.fit(X)
    assert rel_fro(est.components_, g['c1/D_final']) < 1e-9
    assert rel_fro(est.C_, g['c1/C_final']) < 1e-9
    assert rel_fro(est.code_[:64], g['c1/code_final_head']) < 1e-9
    assert rel_fro(est.B_[:, :32], g['c1/B_final_head']) < 1e-9


def _make_pair(DictFact, oracle, dt, n, p, k, b, r, seed=0, **extra):
    rs = np.random.RandomState(seed)
    k0 = min(k, 32)
    X = ((rs.randn(n, k0) * (rs.rand(n, k0) < 0.3)).dot(rs.randn(k0, p)) / np.sqrt(0.3 * k0)
         + 0.1 * rs.randn(n, p)).astype(dt)
    kw = dict(n_components=k, batch_size=b, reduction=r, code_alpha=1.0, learning_rate=0.92, random_state=0)
    kw.update(extra)
    est = DictFact(**kw)
    est.prepare(n_samples=n, X=X)
    pr = oracle.SomfParams(**kw)
    st = oracle.prepare(pr, n_samples=n, X=X)
    return est, pr, st, X


def _one_step_pair(DictFact, oracle, dt, n, p, k, b, r, steps=1, seed=0, **extra):
    est, pr, st, X = _make_pair(DictFact, oracle, dt, n, p, k, b, r, seed, **extra)
    rows = slice(0, steps * b)
    est.partial_fit(X[rows])
    oracle.partial_fit(st, pr, X[rows])
    return est, st


@pytest.mark.parametrize('r', [1, 10])
def test_headline_shape_f64_vs_oracle(DictFact, oracle, r):
    """The metric's shape (k = 256, b = 256, l1 codes, l2 atoms) at p = 2000 so the CPU oracle
    finishes in seconds; f64: two minibatches, everything within 1e-10."""
    est, st = _one_step_pair(DictFact, oracle, np.float64, n=600, p=2000, k=256, b=256, r=r, steps=2)
    errs = (rel_fro(est.components_, st.D), rel_fro(est.code_[:512], st.code[:512]), rel_fro(est.B_, st.B),
            rel_fro(est.C_, st.C))
    assert max(errs) < 1e-10, errs


@pytest.mark.parametrize('r', [1, 10])
def test_headline_shape_f32_vs_oracle(DictFact, oracle, r):
    """f32 at the metric's shape.  Step 1 from identical state: dictionary, codes and statistics
    within 1e-5 of the f32 oracle, same sweep counts.  Step 2 is an ill-conditioned solve (~37
    sweeps) where the reference's OWN f32 rounding noise (f32 oracle vs f64 oracle) exceeds 1e-5;
    there the GPU result must be as close to the f64 ground truth as the f32 oracle is, on the
    samples whose sweep count agrees (a tolerance-stopped solver can legitimately do one sweep
    more or less when its inputs differ in the last bits)."""
    b = 256
    est, pr32, s32, X = _make_pair(DictFact, oracle, np.float32, n=600, p=2000, k=256, b=b, r=r)
    _, pr64, s64, _ = _make_pair(DictFact, oracle, np.float64, n=600, p=2000, k=256, b=b, r=r)
    s32.sweeps, s64.sweeps = [], []
    X64 = X.astype(np.float64)
    for step in range(2):
        rows = slice(step * b, (step + 1) * b)
        idx = np.arange(rows.start, rows.stop)
        est.partial_fit(X[rows], idx)
        sw_gpu = est._backend.last_sweeps()
        oracle.partial_fit(s32, pr32, X[rows], idx)
        oracle.partial_fit(s64, pr64, X64[rows], idx)
        cg, c32, c64 = est.code_[rows], s32.code[rows], s64.code[rows]
        if step == 0:
            assert_array_equal(sw_gpu, s32.sweeps[-1])
            errs = (rel_fro(est.components_, s32.D), rel_fro(cg, c32), rel_fro(est.B_, s32.B), rel_fro(est.C_, s32.C))
            assert max(errs) < 1e-5, errs
        same = (sw_gpu == s32.sweeps[-1]) & (sw_gpu == s64.sweeps[-1])
        assert same.mean() >= 0.98, same.mean()
        noise_ref = rel_fro(c32[same], c64[same])
        err_gpu = rel_fro(cg[same], c64[same])
        assert err_gpu <= 1.5 * noise_ref + 1e-6, (step, err_gpu, noise_ref)
        if same.all():
            assert rel_fro(est.components_, s64.D) <= 1.5 * rel_fro(s32.D, s64.D) + 1e-6


@pytest.mark.parametrize('r', [1, 10])
@pytest.mark.parametrize('dn', ['f64', 'f32'])
def test_headline_full_shape_golden_and_oracle(DictFact, oracle, dn, r):
    """The metric's FULL shape (k = 256, p = 10 000, b = 256, l1 codes, l2 atoms), 4 minibatches, against what the
    REAL reference produced (tests/golden/traj_headline.npz) and against the oracle run next to it: subset draws
    bit-exact; f64 <= 1e-9 on every minibatch; f32 <= 1e-5 (the north star's bound) on EVERY minibatch for codes
    and dictionary, with the share of samples whose sweep count equals the oracle's reported."""
    from .conftest import m1_rows, HEADLINE_KW, headline_observables, subset_checksum
    g = load_golden('traj_headline')
    n, p, k, b = (int(v) for v in g['shape'])
    dt = np.float32 if dn == 'f32' else np.float64
    X = np.ascontiguousarray(m1_rows(n, p).astype(dt))
    name = 'm1_r%d_%s/' % (r, dn)
    est = DictFact(reduction=r, **HEADLINE_KW)
    est.prepare(n_samples=n, X=X)
    rec = Recorder(est)
    pr = oracle.SomfParams(reduction=r, **HEADLINE_KW)
    st = oracle.prepare(pr, n_samples=n, X=X)
    st.sweeps = []
    tol = 1e-9 if dn == 'f64' else 1e-5
    agree = []
    for t in range(n // b):
        rows = slice(t * b, (t + 1) * b)
        idx = np.arange(rows.start, rows.stop)
        est.partial_fit(X[rows], idx)
        oracle.partial_fit(st, pr, X[rows], idx)
        agree.append(float(np.mean(est._backend.last_sweeps() == st.sweeps[-1])))
        code, D = est.code_[rows], est.components_
        e_code, e_D = rel_fro(code[:32], g[name + 'code_head'][t]), rel_fro(D[:, :64], g[name + 'D_head'][t])
        assert e_code < tol and e_D < tol, (t, e_code, e_D, agree)
        assert rel_fro(code, st.code[rows]) < tol and rel_fro(D, st.D) < tol, (t, agree)      # all rows / entries
    print('sweep agreement with the oracle per minibatch (%s, r=%d): %s' % (dn, r, agree))
    assert min(agree) >= (1.0 if dn == 'f64' else 0.98), agree
    assert_array_equal([len(s_) for s_ in rec.subsets], g[name + 'subset_len'])
    assert_array_equal(np.stack([s_[:64] for s_ in rec.subsets]), g[name + 'subset_head'])
    assert_array_equal([subset_checksum(s_) for s_ in rec.subsets], g[name + 'subset_sum'])
    obs = headline_observables(est.components_, est.C_, est.B_, est.comp_norm_)
    for key, val in obs.items():
        if key == 'comp_norm':
            assert np.allclose(val, g[name + key], atol=10 * tol)
        else:
            assert rel_fro(val, g[name + key]) < tol, key
    assert est.n_iter_ == int(g[name + 'n_iter'])


@pytest.mark.parametrize('variant', ['fmri', 'nmf', 'enet', 'sgd', 'full', 'average'])
def test_midsize_variants_vs_oracle(DictFact, oracle, variant):
    extra = {
        'fmri': dict(code_l1_ratio=0, comp_l1_ratio=1, code_alpha=1e-2),           # fmri.py:481-495
        'nmf': dict(comp_pos=True, code_pos=True, code_alpha=0.1),
        'enet': dict(comp_l1_ratio=0.4, code_l1_ratio=0.6, code_alpha=0.2),
        'sgd': dict(optimizer='sgd', step_size=0.05, code_alpha=0.2),
        'full': dict(G_agg='full', Dx_agg='full', code_alpha=0.3),
        'average': dict(G_agg='average', Dx_agg='average', code_alpha=0.3),
    }[variant]
    est, st = _one_step_pair(DictFact, oracle, np.float64, n=200, p=700, k=70, b=20, r=4, steps=5, **extra)
    eD, eC = rel_fro(est.components_, st.D), rel_fro(est.code_[:100], st.code[:100])
    assert eD < 1e-9 and eC < 1e-9, (variant, eD, eC)
    if variant == 'full':
        assert rel_fro(est.G_, st.G) < 1e-9


@pytest.mark.parametrize('dt,tol', [(np.float64, 1e-9), (np.float32, None)])
def test_per_sample_gram_on_the_four_wavefront_solver(DictFact, oracle, dt, tol):
    """G_agg = Dx_agg = 'average' with l1 codes at k = 128: one Gram matrix per sample (rows of G_average_), solved by
    the four-wavefront coordinate-descent kernel straight from where they are stored (other k: cd_kernel)."""
    kw = dict(n=160, p=400, k=128, b=16, r=2, G_agg='average', Dx_agg='average', code_alpha=0.3)
    if tol is not None:
        est, st = _one_step_pair(DictFact, oracle, dt, steps=3, **kw)
        eD, eC = rel_fro(est.components_, st.D), rel_fro(est.code_[:48], st.code[:48])
        assert eD < tol and eC < tol, (eD, eC)
        return
    from .conftest import assert_within_f32_noise
    est, pr, st32, X = _make_pair(DictFact, oracle, dt, **kw)
    X64 = X.astype(np.float64)
    st64 = oracle.prepare(pr, n_samples=X.shape[0], X=X64)
    est.partial_fit(X[:16])
    oracle.partial_fit(st32, pr, X[:16])
    oracle.partial_fit(st64, pr, X64[:16])
    assert_within_f32_noise(est.components_, st32.D, st64.D, 'dictionary')
    assert_within_f32_noise(est.code_[:16], st32.code[:16], st64.code[:16], 'codes')


_PLAN_LEAVES = ([('shared', k, 0.9) for k in (31, 70, 256, 513, 1025)] + [('average', k, 0.9) for k in (20, 70, 128)] +
                [(agg, k, 0.0) for agg in ('shared', 'average') for k in (50, 200, 520)])


@pytest.mark.parametrize('dt', [np.float64, np.float32], ids=['f64', 'f32'])
@pytest.mark.parametrize('agg,k,l1', _PLAN_LEAVES, ids=['%s-k%d-l1_%g' % leaf for leaf in _PLAN_LEAVES])
def test_plan_code_solve_leaves(DictFact, oracle, agg, k, l1, dt):
    """Every leaf of the code solve (csrc/code_solve.hip) as the PLAN enters it, with the plan's scratch: one-wavefront and
    four-wavefront coordinate descent through the padded copy (k = 31, 70, 513) and as stored (256), the wide solver
    (1025), per-sample matrices as stored (20, 128) and through the lazily allocated slots (70); ridge in one launch (50),
    factor + solve (average 200) and blocked (shared 200, 520; average 520, walked from the host indices).  b = 9,
    p = k + 80, two minibatches with permuted sample_indices (the second destination of the solve) that share four rows
    (on their second visit w_sample < 1: G_average_[i] is no longer the minibatch's Gram matrix), then transform (the
    shared-Gram leaf of the same k, warm start of ones).  The oracle transforms with the estimator's dictionary: both
    sides solve the same systems.  (With each side's own dictionary the f32 case at k = 1025 compares solves of inputs
    that differ by the fit's f32 noise, 5.6e-4: on this Gram matrix, condition number 2.4e6, one row of 18 - the one
    with the most sweeps, 66 - then ends 3.5e-2 away, 6.5e-3 over all rows against a noise of 3.1e-4, while from the same
    dictionary every row is within 1.4e-4 of the oracle and the sweep counts are equal.)
    f64: 1e-9 as the neighbours; f32: the oracle's own noise."""
    from .conftest import assert_within_f32_noise
    b, n, p = 9, 18, k + 80
    rs = np.random.RandomState(k)
    X = ((rs.randn(max(n, k), 32) * (rs.rand(max(n, k), 32) < 0.3)).dot(rs.randn(32, p)) / np.sqrt(0.3 * 32)
         + 0.1 * rs.randn(max(n, k), p))
    perm = rs.permutation(n)
    g = 'average' if agg == 'average' else 'masked'
    kw = dict(n_components=k, batch_size=b, reduction=2, code_alpha=0.3 if l1 else 1e-2, code_l1_ratio=l1, G_agg=g, Dx_agg=g,
              learning_rate=0.92, random_state=0)

    def fit(make, partial_fit, Xd):
        st = make(Xd)
        for m in range(2):
            rows = perm[5 * m:5 * m + b]
            partial_fit(st, Xd[rows], rows)
        return st

    def reference(dtype, D):
        pr = oracle.SomfParams(**kw)
        st = fit(lambda Xd: oracle.prepare(pr, n_samples=n, X=Xd), lambda st, Xb, rows: oracle.partial_fit(st, pr, Xb, rows),
                 X.astype(dtype))
        return st.D, st.code, oracle.transform(pr, np.ascontiguousarray(D, dtype=dtype), X[:n].astype(dtype))

    Xd = X.astype(dt)
    est = fit(lambda Xd: DictFact(**kw).prepare(n_samples=n, X=Xd), lambda est, Xb, rows: est.partial_fit(Xb, rows), Xd)
    got = (est.components_, est.code_, est.transform(Xd[:n]))
    names = ('dictionary', 'codes', 'transform')
    if dt == np.float64:
        errs = [rel_fro(a, r) for a, r in zip(got, reference(np.float64, got[0]))]
        print(agg, k, l1, dict(zip(names, errs)))
        assert max(errs) < 1e-9, dict(zip(names, errs))
    else:
        r32, r64 = reference(np.float32, got[0]), reference(np.float64, got[0])
        print(agg, k, l1, {w: (rel_fro(a, c), rel_fro(r, c)) for w, a, r, c in zip(names, got, r32, r64)})
        for w, a, r, c in zip(names, got, r32, r64):
            assert_within_f32_noise(a, r, c, w)


@pytest.mark.parametrize('agg', ['masked', 'average'])
def test_wide_ridge_estimator_vs_oracle(DictFact, oracle, agg):
    """fMRIDictFact's configuration (ridge codes, l1 atoms) at n_components = 600 > 512 through the estimator:
    the blocked ridge solve inside the minibatch step (shared Gram, and one Gram per sample for 'average')."""
    extra = dict(code_l1_ratio=0, comp_l1_ratio=1, code_alpha=1e-2, G_agg=agg, Dx_agg=agg)
    b = 12 if agg == 'masked' else 4
    est, st = _one_step_pair(DictFact, oracle, np.float64, n=640, p=900, k=600, b=b, r=2, steps=2, **extra)
    eD, eC = rel_fro(est.components_, st.D), rel_fro(est.code_[:2 * b], st.code[:2 * b])
    assert eD < 1e-9 and eC < 1e-9, (agg, eD, eC)


@pytest.mark.parametrize('variant', ['fmri', 'fmri_pos', 'enet', 'nmf_l1'])
@pytest.mark.parametrize('shape', ['groups', 'groups_ragged', 'groups_20', 'groups_24', 'few_atoms', 'per_atom'])
def test_generic_dictionary_update_multi_workgroup_vs_oracle(DictFact, oracle, variant, shape):
    """The l1 / elastic-net / positive-atom dictionary update beyond the tiny single-workgroup sweep (s k > 32 k):
    `groups` = eight atoms per launch pair (csrc/bcd.hip atom_grad_group_kernel + atom_project_group_kernel: shared
    gradient pass, corrections between the atoms of a group from registers, warm-started projections over several
    minibatches; 12 elements per thread of the projecting workgroup), `groups_ragged` = k not a multiple of the group
    and a ragged feature count, `groups_20` / `groups_24` = 4500 / 5750 sampled features (20 elements per thread; 24,
    groups of four), `few_atoms` = fewer atoms than a group, `per_atom` = more than 6144 sampled features (one launch
    per atom, atom_step_kernel)."""
    extra = {
        'fmri': dict(code_l1_ratio=0, comp_l1_ratio=1, code_alpha=1e-2),           # fmri.py:481-495
        'fmri_pos': dict(code_l1_ratio=0, comp_l1_ratio=1, code_alpha=1e-2, comp_pos=True),
        'enet': dict(comp_l1_ratio=0.4, code_l1_ratio=0.6, code_alpha=0.2),
        'nmf_l1': dict(comp_pos=True, code_pos=True, comp_l1_ratio=0.7, code_alpha=0.1),
    }[variant]
    n, p, k, b, r = {'groups': (160, 3000, 72, 20, 2), 'groups_ragged': (160, 2501, 70, 20, 3),
                     'groups_20': (120, 9000, 36, 20, 2), 'groups_24': (120, 11500, 27, 20, 2),
                     'few_atoms': (120, 6000, 6, 20, 2), 'per_atom': (100, 14000, 24, 20, 2)}[shape]
    est, st = _one_step_pair(DictFact, oracle, np.float64, n=n, p=p, k=k, b=b, r=r, steps=4, **extra)
    eD, eC = rel_fro(est.components_, st.D), rel_fro(est.code_[:80], st.code[:80])
    assert eD < 1e-9 and eC < 1e-9, (variant, shape, eD, eC)
    assert rel_fro(est.comp_norm_, st.comp_norm) < 1e-9 or np.allclose(est.comp_norm_, st.comp_norm, atol=1e-12)


@pytest.mark.parametrize('p,k,l1', [(3000, 72, 1), (9000, 36, 1), (9000, 36, 0.5), (11500, 27, 1), (11500, 27, 0.5),
                                    (14000, 20, 1), (14000, 20, 0.5), (2600, 520, 1), (14000, 520, 1)])
def test_generic_dictionary_update_f32_groups_vs_oracle(DictFact, oracle, p, k, l1):
    """f32, first minibatch from identical state, through the atom groups (12 / 20 / 24 elements per thread of the
    projecting workgroup; l1 and elastic-net atoms) and, beyond 6144 sampled features or 512 atoms (the shape class of the
    reference's HCP run), through one launch per atom (atom_step_kernel; 7000 sampled features and 520 l1 atoms: the pipelined
    sweep with the 16-registers-per-lane gradient rows riding on the atom launches, round 6): within the oracle's own f32 noise
    of its f64 run."""
    kw = dict(n=max(160, k + 40), p=p, k=k, b=20, r=2, code_l1_ratio=0, comp_l1_ratio=l1, code_alpha=1e-2)
    from .conftest import assert_within_f32_noise
    est, pr, st32, X = _make_pair(DictFact, oracle, np.float32, **kw)
    X64 = X.astype(np.float64)                                   # the same float32 records, in double precision
    st64 = oracle.prepare(pr, n_samples=X.shape[0], X=X64)
    est.partial_fit(X[:20])
    oracle.partial_fit(st32, pr, X[:20])
    oracle.partial_fit(st64, pr, X64[:20])
    assert_within_f32_noise(est.components_, st32.D, st64.D, 'dictionary')
    assert_within_f32_noise(est.code_[:20], st32.code[:20], st64.code[:20], 'codes')


@pytest.mark.parametrize('reduction', [10, 1])       # 32 workgroups on one Gram accumulator; 157 on four (acc_load_sharded)
def test_full_size_step_properties(DictFact, reduction):
    """Size-independent properties at the metric's full shape (k = 256, p = 10000, b = 256, f32)."""
    import torch
    k, p, b, n = 256, 10000, 256, 1024
    gen = torch.Generator(device='cuda').manual_seed(1)
    Z = torch.randn(n, 64, device='cuda', generator=gen) * (torch.rand(n, 64, device='cuda', generator=gen) < 0.1)
    X = (Z @ torch.randn(64, p, device='cuda', generator=gen)) / (0.1 * 64) ** 0.5 \
        + 0.1 * torch.randn(n, p, device='cuda', generator=gen)
    X = X.float().contiguous()
    runs = []
    for rep in range(2):
        est = DictFact(n_components=k, batch_size=b, reduction=reduction, code_alpha=1.0, learning_rate=0.92, random_state=0)
        est.prepare(n_samples=n, X=X[:k])
        D0 = est.components_
        rec = Recorder(est)
        est.partial_fit(X[:2 * b])
        runs.append((est.components_, est.code_[:2 * b].copy(), est.C_, rec.subsets))
        D1 = runs[-1][0]
        touched = np.unique(np.concatenate(rec.subsets))
        untouched = np.setdiff1d(np.arange(p), touched)
        assert_array_equal(D1[:, untouched], D0[:, untouched])            # only sampled columns move
        assert reduction > 1 or untouched.size == 0
        assert np.any(D1[:, touched] != D0[:, touched])
        assert np.all(np.sum(D1.astype(np.float64) ** 2, axis=1) <= 1 + 1e-4)    # atoms stay in the l2 ball
        Cm = runs[-1][2]
        assert_array_equal(Cm, Cm.T)                                      # bitwise symmetric statistics
        assert np.all(np.isfinite(D1)) and np.all(np.isfinite(runs[-1][1]))
    assert_array_equal(runs[0][0], runs[1][0])                            # run-to-run deterministic
    assert_array_equal(runs[0][1], runs[1][1])


@pytest.mark.parametrize('p,red', [(1000, 2), (6000, 1)])       # 16 workgroups on one accumulator; 94 on four (acc_load_sharded)
@pytest.mark.parametrize('scale', [1e13, 1e-9, 1.0])
def test_gram_accumulator_out_of_range_falls_back_to_records(DictFact, scale, p, red):
    """(scale 1: the accumulator itself against the records, in range.)
    The blocked dictionary update sums its 32 x 32 Gram contributions in fixed point (csrc/bcd.hip: acc_add, range
    |entry| < 2^50 in dictionary units, absolute resolution 2^-71).  Candidate atoms of norm ~1e12 - statistics scaled by
    hand, nothing a fit produces - must not come back as a wrapped integer sum, and candidate atoms of norm ~1e-10 (squared
    norms under 2^-40) must not lose their relative precision to the absolute bins: in both cases the block is summed
    from the per-workgroup records, the same result as with the accumulator switched off."""
    from modl_amd._lib import lib, check, DEBUG_BCD_ACC, DEBUG_BCD_PERSIST
    rs = np.random.RandomState(0)
    X = ((rs.randn(256, 32) * (rs.rand(256, 32) < 0.3)).dot(rs.randn(32, p)) / np.sqrt(0.3 * 32)
         + 0.1 * rs.randn(256, p)).astype(np.float32)
    out = {}
    try:
        # 2: the persistent launch (csrc/bcd_persist.hip: look-ahead accumulators, the same fixed-point bins and the same
        # fallback to per-workgroup records); 1: one launch per block with the accumulator; 0: ... with the records
        for acc in (2, 1, 0):
            check(lib.modl_debug_set(DEBUG_BCD_PERSIST, 1 if acc == 2 else 0))
            check(lib.modl_debug_set(DEBUG_BCD_ACC, min(acc, 1)))
            est = DictFact(n_components=64, batch_size=64, reduction=red, code_alpha=0.1, learning_rate=0.92, random_state=0)
            est.prepare(n_samples=256, X=X[:64])
            est.partial_fit(X[:64])
            assert np.count_nonzero(np.diag(est.C_) > 1e-6) > 32
            if scale != 1.0:
                est.B_ = est.B_ * np.float32(scale)
            if scale < 1:                                  # tiny candidates: tiny norm budgets too, else they are kept whole
                est.components_ = est.components_ * np.float32(scale)
                est.comp_norm_ = est.comp_norm_ * np.float32(scale ** 2)
            est.partial_fit(X[64:128])
            out[acc] = (est.components_, est.comp_norm_)
    finally:
        check(lib.modl_debug_set(DEBUG_BCD_ACC, 1))
        check(lib.modl_debug_set(DEBUG_BCD_PERSIST, 1))
    D0 = out[0][0]
    for acc, tol in ((1, 1e-6), (2, 1e-5)):    # (the persistent launch rounds its f32 candidates in another order: a - N' cancels)
        D1 = out[acc][0]
        assert np.all(np.isfinite(D1)) and np.all(np.isfinite(out[acc][1]))
        if scale > 1:
            assert np.all(np.abs(np.sqrt(np.sum(D1.astype(np.float64) ** 2, axis=1)) - 1) < 1e-4)   # projected onto the ball
        assert rel_fro(D1, D0) < tol, (acc, rel_fro(D1, D0))
        import sys
        sys.stderr.write('\n[accumulator vs records] scale %g: %s %.2e (gate %.0e)\n'
                         % (scale, 'block launches' if acc == 1 else 'persistent launch', rel_fro(D1, D0), tol))


@pytest.mark.parametrize('k,p,b,red', [(320, 1200, 64, 2), (512, 700, 48, 1), (40, 333, 32, 3), (250, 1200, 64, 2), (70, 2001, 96, 3)])
def test_wide_dictionaries_f32_vs_oracle(DictFact, oracle, k, p, b, red):
    """k > 256 (two registers of coefficients per lane in the solver, 16 contraction groups per wave in the
    fused dictionary update), k not a multiple of 32, k not a multiple of 4 (dead atoms pad the packed arrays of the
    fused update, the dense products stage their misaligned operands element by element, the solver runs on a
    zero-padded Gram), p not a multiple of 4: first minibatch from identical state, f32, against the f32 oracle."""
    rs = np.random.RandomState(11)
    n = max(2 * b, k)                                 # prepare() takes its initial atoms from the first k rows
    X = (rs.randn(n, 96) @ rs.randn(96, p) / 10 + 0.5 * rs.randn(n, p)).astype(np.float32)
    kw = dict(n_components=k, batch_size=b, reduction=red, code_alpha=0.3, learning_rate=0.9, random_state=0)
    est = DictFact(**kw)
    est.prepare(n_samples=n, X=X)
    est.partial_fit(X[:b], np.arange(b))
    pr = oracle.SomfParams(**kw)
    st = oracle.prepare(pr, n_samples=n, X=X)
    oracle.partial_fit(st, pr, X[:b], np.arange(b))
    eD, ec = rel_fro(est.components_, st.D), rel_fro(est.code_[:b], st.code[:b])
    assert eD < 1e-5 and ec < 1e-5, (k, p, eD, ec)
    assert rel_fro(est.C_, st.C) < 1e-5 and rel_fro(est.B_, st.B) < 1e-5


@pytest.mark.parametrize('k', [200, 320, 70])
def test_any_number_of_atoms_runs_the_vectorised_solver_f64(DictFact, oracle, k):
    """A shared Gram whose size is not 64 / 128 / 256 / 512 / 1024 is solved from a zero-padded copy (cd_padded_ld):
    the padding is dead coordinates, so in f64 two minibatches agree with the oracle to 1e-10 and every sample takes
    the oracle's number of sweeps."""
    est, pr, st, X = _make_pair(DictFact, oracle, np.float64, n=max(256, k), p=1500, k=k, b=96, r=3, seed=0)
    st.sweeps = []
    for step in range(2):
        rows = slice(96 * step, 96 * (step + 1))
        est.partial_fit(X[rows], np.arange(rows.start, rows.stop))
        oracle.partial_fit(st, pr, X[rows], np.arange(rows.start, rows.stop))
        assert_array_equal(est._backend.last_sweeps(), np.asarray(st.sweeps[-1]))
    errs = (rel_fro(est.components_, st.D), rel_fro(est.code_[:192], st.code[:192]), rel_fro(est.B_, st.B),
            rel_fro(est.C_, st.C))
    assert max(errs) < 1e-10, (k, errs)


@pytest.mark.parametrize('agg', [('masked', 'masked'), ('full', 'full'), ('average', 'average')])
def test_two_phase_equals_fused_step(DictFact, agg):
    """modl_somf_code_and_partials + modl_somf_apply_and_update_dict (the multi-GPU split: the dictionary update
    reads C_ and the sampled rows of B_ from the head buffer) and modl_somf_step give the same bits."""
    rng = np.random.RandomState(3)
    X = rng.randn(300, 96).astype(np.float32)
    out = []
    for two_phase in (False, True):
        est = DictFact(n_components=32, batch_size=40, reduction=3, code_alpha=0.5, learning_rate=0.9, random_state=0,
                       G_agg=agg[0], Dx_agg=agg[1])
        est._two_phase = two_phase
        est.prepare(n_samples=300, X=X)
        est.partial_fit(X[:200], np.arange(200))
        out.append((est.components_, est.code_.copy(), est.C_, est.B_))
    for a, b in zip(out[0], out[1]):
        assert_array_equal(a, b)


@pytest.mark.parametrize('source', ['ndarray', 'memmap'])
def test_partial_fit_streams_host_input_in_chunks(DictFact, tmp_path, source):
    """A host array larger than one chunk goes to HBM in pinned, double-buffered chunks of whole minibatches
    (dict_fact.py:313-337 is the streaming contract): three chunks + a ragged last minibatch must give the bits of
    the run with X resident on the device."""
    import torch
    rs = np.random.RandomState(2)
    b, p, k = 32, 300, 12
    n = 5 * b + 7
    X = (rs.randn(n, 20) @ rs.randn(20, p) + 0.3 * rs.randn(n, p)).astype(np.float32)
    if source == 'memmap':
        path = str(tmp_path / 'X.npy')
        np.save(path, X)
        Xin = np.load(path, mmap_mode='r')
    else:
        Xin = X
    kw = dict(n_components=k, batch_size=b, reduction=3, code_alpha=0.2, learning_rate=0.9, random_state=0)
    res = []
    for streamed in (False, True):
        est = DictFact(**kw)
        est.prepare(n_samples=n, X=X)
        if streamed:
            est._host_chunk_rows = 2 * b
            est.partial_fit(Xin)
        else:
            est.partial_fit(torch.from_numpy(X).cuda())
        res.append((est.components_, est.code_.copy(), est.C_, est.B_, est.n_iter_))
    for a, c in zip(res[0], res[1]):
        assert_array_equal(a, c)


@pytest.mark.parametrize('p,k,b', [(10000, 256, 256), (4104, 100, 200), (8192, 256, 64), (4100, 36, 256)])
def test_resident_statistics_product(DictFact, p, k, b):
    """At least 4096 features, at most 256 atoms, a minibatch that is a multiple of four: the p x k statistics product runs
    on persistent workgroups with the code matrix resident in registers (csrc/gemm_resident.hpp; reduction 1 at the
    metric's shape, config 5's 200 000 features).  Ragged last tile (p not a multiple of 16), fewer atoms than a
    workgroup's wavefronts cover, K < 256 (skipped k-steps).  After the FIRST minibatch (w = 1) B_ = code^T X / b exactly -
    checked against that product of the GPU's own codes in f64, every row; the second minibatch (the read-modify-write)
    likewise; then two minibatches against the run with MODL_DEBUG_STATS_RESIDENT = 0 (the 32 x 32 tiles)."""
    from modl_amd._lib import lib, check, DEBUG_STATS_RESIDENT
    rs = np.random.RandomState(p + k)
    n = max(3 * b, k)
    X = (rs.randn(n, 16) @ rs.randn(16, p) / 4 + 0.5 * rs.randn(n, p)).astype(np.float32)
    kw = dict(n_components=k, batch_size=b, reduction=1, code_alpha=0.3, learning_rate=0.9, random_state=0)
    est = DictFact(**kw)
    est.prepare(n_samples=n, X=X)
    est.partial_fit(X[:b], np.arange(b))
    code = est.code_[:b].astype(np.float64)
    assert rel_fro(est.B_, code.T @ X[:b].astype(np.float64) / b) < 2e-6
    assert rel_fro(est.C_, code.T @ code / b) < 2e-6
    # the read-modify-write part: the SECOND minibatch against (1 - w) B_1 + (w / b) code_2^T X_2 in f64, from the GPU's own
    # B_1 and codes
    from modl_amd.randomkit import batch_weight
    B1, C1 = est.B_.astype(np.float64), est.C_.astype(np.float64)
    est.partial_fit(X[b:2 * b], np.arange(b, 2 * b))
    w = batch_weight(est.n_iter_, b, kw['learning_rate'], 0)
    code = est.code_[b:2 * b].astype(np.float64)
    assert rel_fro(est.B_, (1 - w) * B1 + w * (code.T @ X[b:2 * b].astype(np.float64) / b)) < 2e-6
    assert rel_fro(est.C_, (1 - w) * C1 + w * (code.T @ code / b)) < 2e-6
    # and against the run with the 32 x 32 tiles (a rounding difference in B_ moves the dictionary, hence the next codes)
    res = []
    try:
        for sw in (0, 1):
            check(lib.modl_debug_set(DEBUG_STATS_RESIDENT, sw))
            e = DictFact(**kw)
            e.prepare(n_samples=n, X=X)
            e.partial_fit(X[:2 * b], np.arange(2 * b))
            res.append((e.B_.copy(), e.C_.copy(), e.components_.copy()))
    finally:
        check(lib.modl_debug_set(DEBUG_STATS_RESIDENT, 1))
    for a, c, name in zip(res[0], res[1], ('B', 'C', 'D')):
        assert rel_fro(c, a) < 1e-4, (name, rel_fro(c, a))


@pytest.mark.parametrize('p,k,b,red', [(4104, 100, 200, 1), (16416, 64, 64, 3)])
def test_resident_product_two_phase_equals_fused(DictFact, p, k, b, red):
    """The register-resident statistics product with the head mirror of the two-phase (multi-GPU) step: reduction 1 (every
    row of B_ through the 16-byte epilogue, mirrored) and a sampled set of 5472 rows (the row-indirected epilogue, element by
    element, compact mirror) - the same bits as the fused step."""
    rs = np.random.RandomState(p)
    n = max(3 * b, k)
    X = (rs.randn(n, 16) @ rs.randn(16, p) / 4 + 0.5 * rs.randn(n, p)).astype(np.float32)
    out = []
    for two_phase in (False, True):
        est = DictFact(n_components=k, batch_size=b, reduction=red, code_alpha=0.3, learning_rate=0.9, random_state=0)
        est._two_phase = two_phase
        est.prepare(n_samples=n, X=X)
        est.partial_fit(X[:3 * b], np.arange(3 * b))
        out.append((est.components_, est.code_.copy(), est.C_, est.B_))
    for a, c in zip(out[0], out[1]):
        assert_array_equal(a, c)


@pytest.mark.parametrize('k,b,red', [(32, 64, 4), (72, 50, 1)])
def test_wide_statistics_tile(DictFact, oracle, k, b, red):
    """p >= 65 536 features: the p x k statistics product runs as its own k-wide launch (csrc/gemm_wide.hpp: 32 features
    x all atoms per tile, X read once) instead of riding on the dictionary update; p not a multiple of the tile, k < 256
    (masked atoms), a ragged minibatch (K = 50 samples: zero-filled rows of the staged X tile).
    The kernel itself: after the FIRST minibatch (w = 1) B_ = code^T X / b exactly - checked against that product of the
    GPU's own codes in f64, every row.  The step around it: dictionary and codes against the f32 oracle within the
    reference's own f32 noise (f32 oracle vs f64 oracle: the code products contract over up to 65 604 features)."""
    p = 65604
    rs = np.random.RandomState(k)
    n = max(2 * b, k)
    X = (rs.randn(n, 24) @ rs.randn(24, p) / 5 + 0.5 * rs.randn(n, p)).astype(np.float32)
    kw = dict(n_components=k, batch_size=b, reduction=red, code_alpha=0.3, learning_rate=0.9, random_state=0)
    est = DictFact(**kw)
    est.prepare(n_samples=n, X=X)
    est.partial_fit(X[:b], np.arange(b))
    code = est.code_[:b].astype(np.float64)
    assert rel_fro(est.B_, code.T @ X[:b].astype(np.float64) / b) < 2e-6
    assert rel_fro(est.C_, code.T @ code / b) < 2e-6
    st = {}
    for dt in (np.float32, np.float64):
        pr = oracle.SomfParams(**kw)
        st[dt] = oracle.prepare(pr, n_samples=n, X=X.astype(dt))
        oracle.partial_fit(st[dt], pr, X[:b].astype(dt), np.arange(b))
    for got, name in ((est.components_, 'D'), (est.code_[:b], 'code')):
        ref32, ref64 = getattr(st[np.float32], name)[:got.shape[0]], getattr(st[np.float64], name)[:got.shape[0]]
        noise = rel_fro(ref32, ref64)
        assert rel_fro(got, ref64) <= 2 * noise + 1e-5, (name, rel_fro(got, ref64), noise)


def test_g_average_in_pinned_host_memory(DictFact):
    """G_average_ (n k^2 elements; a disk memmap in the reference, dict_fact.py:431-439) does not have to fit in HBM:
    kept in pinned host memory, read and written by the kernels over the host link, the fit gives the bits of the run
    with the array in HBM (two epochs: its rows are shuffled in place too)."""
    from modl_amd.dict_fact import HipBackend
    kw, X, dt = small_case_params('agg_average_average_f64')

    class HostG(DictFact):
        def _make_backend(self):
            be = HipBackend(getattr(self, 'device', None))
            be.g_average_on_host = True
            return be
    a = DictFact(**kw).fit(X)
    b = HostG(**kw).fit(X)
    assert b._backend.G_average.device.type == 'cpu' and b._backend.G_average.is_pinned()
    assert_array_equal(a.components_, b.components_)
    assert_array_equal(a.code_, b.code_)
    assert_array_equal(a.G_average_, b.G_average_)


# ---- the reference's own functional tests (modl/decomposition/tests/test_dict_fact.py) ----------
solver_dict = {'masked': {'Dx_agg': 'masked', 'G_agg': 'masked'}, 'gram': {'Dx_agg': 'masked', 'G_agg': 'full'},
               'average': {'Dx_agg': 'masked', 'G_agg': 'masked'}, 'full': {'Dx_agg': 'full', 'G_agg': 'full'}}


def generate_synthetic(n_samples=200, n_components=4, n_features=16, dictionary_rank=None):
    rng = np.random.RandomState(0)                                          # test_dict_fact.py:40-52
    if dictionary_rank is None:
        Q = rng.randn(n_components, n_features)
    else:
        V = rng.randn(dictionary_rank, n_features)
        U = rng.randn(n_components, dictionary_rank)
        Q = U.dot(V)
    code = rng.randn(n_samples, n_components)
    return code.dot(Q), Q


@pytest.mark.parametrize('solver', list(solver_dict))
def test_ref_reconstruction(DictFact, solver):                              # test_dict_fact.py:55-69
    X, Q = generate_synthetic()
    est = DictFact(n_components=4, code_alpha=1e-4, n_epochs=5, comp_l1_ratio=0, random_state=0, reduction=1,
                   **solver_dict[solver])
    est.fit(X)
    Y = est.transform(X).dot(est.components_)
    assert np.sum((X - Y) ** 2) / np.sum(X ** 2) < 0.02


@pytest.mark.parametrize('solver', list(solver_dict))
def test_ref_reconstruction_reduction_and_reproducible(DictFact, solver):   # test_dict_fact.py:71-112
    X, Q = generate_synthetic(n_features=20, n_samples=400, dictionary_rank=4)
    est = DictFact(n_components=4, code_alpha=1e-4, n_epochs=2, comp_l1_ratio=0, random_state=0, reduction=2,
                   **solver_dict[solver])
    est.fit(X)
    D1, P1 = est.components_.copy(), est.transform(X)
    assert np.sum((X - P1.dot(D1)) ** 2) / np.sum(X ** 2) < 0.02
    est.random_state = 0
    est.fit(X)
    assert_array_equal(D1, est.components_)
    assert_array_equal(P1, est.transform(X))


@pytest.mark.parametrize('solver', list(solver_dict))
def test_ref_sparse_dict_recovery(DictFact, solver):                        # test_dict_fact.py:135-154
    rng = np.random.RandomState(0)
    Q = np.zeros((4, 16))
    for i in range(2):
        for j in range(2):
            atom = np.zeros((4, 4))
            atom[2 * i:2 * (i + 1), 2 * j:2 * (j + 1)] = 1
            Q[2 * i + j] = atom.ravel()
    X = rng.randn(500, 4).dot(Q)
    rng = np.random.RandomState(0)
    dict_init = Q + rng.randn(*Q.shape) * 0.2
    est = DictFact(n_components=4, code_alpha=1e-2, n_epochs=2, code_l1_ratio=0, comp_l1_ratio=1,
                   dict_init=dict_init, random_state=0, **solver_dict[solver])
    est.fit(X)
    Qr = est.components_
    Qr /= np.sqrt(np.sum(Qr ** 2, axis=1))[:, None]
    Qn = Q / np.sqrt(np.sum(Q ** 2, axis=1))[:, None]
    Gm = np.abs(Qr.dot(Qn.T))
    assert min(np.sum(np.any(Gm > 0.95, axis=1)), np.sum(np.any(Gm > 0.95, axis=0))) >= 4


def test_transform_and_score_golden():
    from modl_amd import Coder
    g = load_golden('transform')
    for dn, tol in (('f64', 1e-10), ('f32', 1e-5)):
        X, D = g['X_' + dn], g['D_' + dn]
        for l1, alpha, pos in ((1.0, 0.1, False), (0.0, 0.1, False), (0.5, 0.05, True)):
            cd = Coder(D, code_alpha=alpha, code_l1_ratio=l1, code_pos=pos)
            key = '%s_%g_%g_%d' % (dn, l1, alpha, pos)
            assert rel_fro(cd.transform(X), g['code_' + key]) < tol, key
            assert abs(cd.score(X) - g['score_' + key]) < 1e-5 * abs(g['score_' + key])


@pytest.mark.parametrize('case', ['masked_r10', 'full_r1', 'ragged', 'wide'])
def test_chunk_call_equals_python_loop(DictFact, case):
    """modl_somf_partial_fit_chunk (the per-minibatch host loop behind the ABI: subset draw, _batch_weight, numpy's
    legacy permutation(k) restated in the library) against the Python loop of _single_batch_fit: the same draws in the
    same order, hence the same bits - dictionary, codes, statistics, n_iter_, and the numpy generator left in step."""
    rs = np.random.RandomState(2)
    p, k, b = 3000, 64, 48
    if case == 'wide':             # >= 32 768 features: the chunk call draws its subsets ahead on a worker thread (DrawAhead)
        p, k, b = 40000, 32, 24
    n = 7 * b + (17 if case == 'ragged' else 0)
    X = ((rs.randn(n, 20) * (rs.rand(n, 20) < 0.3)).dot(rs.randn(20, p)) + 0.1 * rs.randn(n, p)).astype(np.float32)
    kw = dict(n_components=k, batch_size=b, reduction=10 if case != 'full_r1' else 1, code_alpha=0.5, learning_rate=0.92,
              random_state=0)
    if case == 'full_r1':
        kw.update(G_agg='full', Dx_agg='full')
    idx = rs.permutation(n + 9)[:n]
    runs = []
    for python_loop in (True, False):
        est = DictFact(**kw)
        est._python_loop = python_loop
        est.prepare(n_samples=n + 9, X=X)
        est.partial_fit(X, idx)
        est.partial_fit(X[:3 * b])                                   # sample_indices = None: rows 0 .. of code_
        runs.append((est.components_, est.code_, est.C_, est.B_, est.n_iter_, est.sample_n_iter_.copy(),
                     est.random_state.randint(1 << 30), est.feature_sampler_.yield_subset(3.0)))
    for a, c in zip(*runs):
        assert_array_equal(a, c)


@pytest.mark.parametrize('r', [10, 1])
def test_timed_path_long_horizon_vs_oracle(DictFact, oracle, r):
    """The code path bench.py times, over a long horizon: ONE partial_fit call = ONE modl_somf_partial_fit_chunk call of
    up to 48 minibatches at the metric's full shape (k = 256, p = 10 000, b = 256) - the 8-deep pinned staging ring
    wraps five times, both device parameter blocks alternate, the staging copy of minibatch t + 1 and the statistics
    product of the rows that were not sampled ride on the dictionary update's launches, warm starts are chunk-local -
    against the CPU oracle fitted on the same rows.  Calls of 8, 16, 32 and 48 minibatches (each from a fresh
    estimator) are compared with the oracle's state after as many: f64 <= 1e-8 on D, C, B[:, :64] and the last
    minibatch's codes with the oracle's sweep count on EVERY sample of EVERY minibatch (modl_somf_sweeps_history);
    f32 <= 1e-5 FLAT (the north star's bound) as long as every sample so far did the f64
    oracle's number of sweeps - a tolerance-stopped solver may legitimately do a sweep more or less on a sample whose
    duality gap sits on the threshold when its inputs differ in the last bits (the oracle's own f32 run does it too);
    such flips must stay under 0.1 % of the samples and the distance under 2 noise + 6e-5 after one.  n_iter_ and both
    generators are left in step with the oracle's (all 48 subset draws: a subset that differed would move D by O(1))."""
    from .conftest import m1_rows, HEADLINE_KW
    import torch
    p, b, marks = 10000, 256, (8, 16, 32, 48)
    n = marks[-1] * b
    X32 = m1_rows(n, p, seed=77)
    kw = dict(HEADLINE_KW, reduction=r)
    snaps, sweeps = {}, {}
    for dt in (np.float64, np.float32):
        X = X32.astype(dt)
        pr = oracle.SomfParams(**kw)
        st = oracle.prepare(pr, n_samples=n, X=X)
        st.sweeps = []
        for t in range(marks[-1]):
            oracle.partial_fit(st, pr, X[t * b:(t + 1) * b], np.arange(t * b, (t + 1) * b))
            if t + 1 in marks:
                snaps[(dt, t + 1)] = dict(D=st.D.copy(), C=st.C.copy(), B=st.B[:, :64].copy(), code=st.code[t * b:(t + 1) * b].copy(),
                                          n_iter=st.n_iter)
        sweeps[dt] = np.stack(st.sweeps)
        snaps[(dt, 'next_subset')] = st.sampler.yield_subset(r)
    flips_ref = int((sweeps[np.float32] != sweeps[np.float64]).sum())
    report, failures = ['oracle f32 vs oracle f64: %d samples with another sweep count' % flips_ref], []
    for dt in (np.float64, np.float32):
        Xd = torch.from_numpy(X32.astype(dt)).cuda()
        for m in marks:
            est = DictFact(**kw)
            est.prepare(n_samples=n, X=X32[:256].astype(dt))
            assert est._chunk_call_applies(est._backend, np.arange(m * b))          # the one-call-per-chunk route
            hist = est._backend.sweeps_history(m)
            est.partial_fit(Xd[:m * b], np.arange(m * b))
            sw = hist()
            ref64, ref32 = snaps[(np.float64, m)], snaps[(np.float32, m)]
            got = dict(D=est.components_, C=est.C_, B=est.B_[:, :64], code=est.code_[(m - 1) * b:m * b])
            flips = int((sw != sweeps[np.float64][:m]).sum())
            assert est.n_iter_ == ref64['n_iter'] == m * b
            for key in ('D', 'C', 'B', 'code'):
                e = rel_fro(got[key], ref64[key])
                if dt == np.float64:
                    if not e < 1e-8:
                        failures.append((r, m, key, e))
                    report.append(('float64', m, key, float(e)))
                else:
                    noise = rel_fro(ref32[key], ref64[key])
                    # round 5: no sample with another sweep count -> the north star's bound, FLAT (measured 1-2e-6: the
                    # noise-relative rule passed anything under ~5e-5, i.e. a 20x regression of the f32 path); the
                    # noise rule only behind a flip
                    bound = 1e-5 if not flips else 2 * noise + 1e-5 + 6e-5
                    if not e <= bound:
                        failures.append((r, m, key, e, noise, flips))
                    report.append(('float32', m, key, float(e), 'oracle f32 noise %.2e' % noise))
            report.append((np.dtype(dt).name, m, 'samples with another sweep count than the f64 oracle', flips))
            if flips > (0 if dt == np.float64 else 1e-3 * m * b):
                failures.append((r, m, 'sweep flips', flips))
            if m == marks[-1]:
                assert_array_equal(est.feature_sampler_.yield_subset(r), snaps[(dt, 'next_subset')])
    print('long horizon r=%d:\n%s' % (r, '\n'.join(str(x) for x in report)))
    assert not failures, failures


@pytest.mark.parametrize('p', [1500, 36000])
def test_chunk_call_error_is_consistent(DictFact, p):
    """modl_somf_partial_fit_chunk, a minibatch that does not validate (a sample index outside code_) in the middle of
    a call: the call reports it, and n_iter_, sample_n_iter_, the feature sampler and the numpy generator are left
    exactly where the last ENQUEUED minibatch left them (the draws of the look-ahead rewound) - after the index is
    corrected, fitting the remaining rows gives the bits of an uninterrupted run."""
    from modl_amd._lib import ModlError
    rs = np.random.RandomState(3)
    k, b, nb = 32, 24, 9               # (p = 36 000: the subsets are drawn ahead on the chunk call's worker thread)
    n = nb * b
    X = ((rs.randn(n, 12) * (rs.rand(n, 12) < 0.4)).dot(rs.randn(12, p)) + 0.1 * rs.randn(n, p)).astype(np.float32)
    kw = dict(n_components=k, batch_size=b, reduction=5, code_alpha=0.3, learning_rate=0.92, random_state=0)
    idx = rs.permutation(n)
    clean = DictFact(**kw)
    clean.prepare(n_samples=n, X=X)
    clean.partial_fit(X, idx)
    est = DictFact(**kw)
    est.prepare(n_samples=n, X=X)
    bad = idx.copy()
    bad[4 * b + 5] = n + 3                                     # minibatch 4 is rejected before anything is enqueued for it
    with pytest.raises(ModlError):
        est.partial_fit(X, bad)
    assert est.n_iter_ == 4 * b
    want = np.zeros(n, dtype=int)
    want[idx[:4 * b]] = 1
    assert_array_equal(est.sample_n_iter_, want)
    est.partial_fit(X[4 * b:], idx[4 * b:])                    # the corrected rest
    for a, c in ((est.components_, clean.components_), (est.code_, clean.code_), (est.C_, clean.C_), (est.B_, clean.B_)):
        assert_array_equal(a, c)
    assert est.n_iter_ == clean.n_iter_
    assert_array_equal(est.sample_n_iter_, clean.sample_n_iter_)
    assert est.random_state.randint(1 << 30) == clean.random_state.randint(1 << 30)
    assert_array_equal(est.feature_sampler_.yield_subset(3.0), clean.feature_sampler_.yield_subset(3.0))


@pytest.mark.parametrize('dt', [np.float64, np.float32])
def test_wide_l2_estimator_vs_oracle(DictFact, oracle, dt):
    """512 < n_components <= 1024 with l1 codes and l2 atoms (the reference's HCP runs use 1024 maps,
    exps/hcp/decompose_hcp.py:50-60): the blocked dictionary update as separate launches (gather-GEMM + Gram + resolve +
    apply: the branch the fused block kernel does not cover) and the four-wavefront solver at k = 640, through the
    estimator, two minibatches."""
    from .conftest import assert_within_f32_noise
    kw = dict(n=700, p=1500, k=640, b=32, r=3, code_alpha=0.5)
    est, pr, st, X = _make_pair(DictFact, oracle, dt, **kw)
    X64 = X.astype(np.float64)
    st64 = oracle.prepare(pr, n_samples=X.shape[0], X=X64) if dt == np.float32 else None
    for t in range(2):
        rows = slice(t * 32, (t + 1) * 32)
        est.partial_fit(X[rows], np.arange(rows.start, rows.stop))
        oracle.partial_fit(st, pr, X[rows], np.arange(rows.start, rows.stop))
        if st64 is not None:
            oracle.partial_fit(st64, pr, X64[rows], np.arange(rows.start, rows.stop))
    if dt == np.float64:
        errs = (rel_fro(est.components_, st.D), rel_fro(est.code_[:64], st.code[:64]), rel_fro(est.C_, st.C), rel_fro(est.B_, st.B))
        assert max(errs) < 1e-9, errs
    else:
        assert_within_f32_noise(est.components_, st.D, st64.D, 'dictionary')
        assert_within_f32_noise(est.code_[:64], st.code[:64], st64.code[:64], 'codes')
        assert_within_f32_noise(est.C_, st.C, st64.C, 'C')


def test_pickle_roundtrip(DictFact):
    import pickle
    X, _ = generate_synthetic(n_features=20, n_samples=100, dictionary_rank=4)
    est = DictFact(n_components=4, code_alpha=1e-3, random_state=0, reduction=2)
    est.fit(X)
    est2 = pickle.loads(pickle.dumps(est))
    assert_array_equal(est.components_, est2.components_)
    assert_array_equal(est.code_, est2.code_)
    est.partial_fit(X[:20])
    est2.partial_fit(X[:20])
    assert_array_equal(est.components_, est2.components_)


# ---- the data-parallel protocol on the real backend: 2 processes share the GPU, increments summed over gloo ------
def _gpu_rank_main(rank, world, port, kw, X_parts, out):
    import os
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from modl_amd import DictFact as DF
        est = DF(**kw)
        X = X_parts[rank]
        est.prepare(n_samples=X.shape[0], X=X_parts[0])        # every rank initialises from the same rows
        est.partial_fit(X)
        out[rank] = dict(D=est.components_, C=est.C_, B=est.B_, code=est.code_, n_iter=est.n_iter_)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize('variant', ['l1_masked_r3', 'l1_masked_r1'])
def test_two_rank_gpu_equals_double_batch(oracle, variant):
    """R ranks with local batch b == one rank with batch R b on the concatenated rows (f64, through the C-ABI
    two-phase entry points and an all-reduce of the increments)."""
    import socket
    import torch.multiprocessing as mp
    red = 3 if variant.endswith('r3') else 1
    rs = np.random.RandomState(5)
    b, steps, p, k = 16, 5, 64, 8
    X0 = rs.randn(b * steps, 12).dot(rs.randn(12, p)) + 0.3 * rs.randn(b * steps, p)
    X1 = rs.randn(b * steps, 12).dot(rs.randn(12, p)) + 0.3 * rs.randn(b * steps, p)
    kw = dict(n_components=k, batch_size=b, reduction=red, random_state=0, learning_rate=0.9, code_alpha=0.1)
    sock = socket.socket()
    sock.bind(('127.0.0.1', 0))
    port = sock.getsockname()[1]
    sock.close()
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_gpu_rank_main, args=(2, port, kw, [X0, X1], out), nprocs=2, join=True)
    Xc = np.concatenate([np.concatenate([X0[t * b:(t + 1) * b], X1[t * b:(t + 1) * b]]) for t in range(steps)])
    pr = oracle.SomfParams(**dict(kw, batch_size=2 * b))
    st = oracle.prepare(pr, n_samples=Xc.shape[0], X=X0)
    oracle.partial_fit(st, pr, Xc)
    for r in (0, 1):
        assert rel_fro(out[r]['D'], st.D) < 1e-9, (variant, r)
        assert rel_fro(out[r]['C'], st.C) < 1e-9
        assert rel_fro(out[r]['B'], st.B) < 1e-9
        assert out[r]['n_iter'] == st.n_iter
    assert_array_equal(out[0]['D'], out[1]['D'])               # replicas stay bit-identical


def _gpu_rank_main_big(rank, world, port, kw, dtype_name, seeds, b, steps, p, out):
    import os
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from modl_amd import DictFact as DF
        from tests.conftest import m1_rows
        dt = np.dtype(dtype_name)
        X0 = m1_rows(b * steps, p, seed=seeds[0]).astype(dt)
        X = X0 if rank == 0 else m1_rows(b * steps, p, seed=seeds[rank]).astype(dt)
        est = DF(**kw)
        est.prepare(n_samples=X.shape[0], X=X0)
        est.partial_fit(X)
        D = est.components_
        out[rank] = dict(D_head=D[:, :128].copy(), D_sum=float(D.astype(np.float64).sum()),
                         D_sq=float((D.astype(np.float64) ** 2).sum()), D_bytes=D.tobytes()[:1 << 16],
                         C=est.C_, B_head=est.B_[:, :64].copy(), n_iter=est.n_iter_)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize('dtype_name,r', [('float64', 10), ('float32', 10), ('float64', 1)])
def test_two_rank_gpu_headline_shape(oracle, dtype_name, r):
    """World size 2 at the metric's shape (k = 256, p = 10 000, 128 rows per rank, 3 minibatches): both phases through
    the C-ABI, the head [C_r | sampled rows of B_r] summed over gloo, the rest of B_ kept as per-rank partial sums
    (f32: riding on the dictionary update's launches).  R ranks with local batch b == one rank with batch R b on the
    concatenated rows (f64: <= 1e-10; f32: the first minibatch... 1e-5 over all three), replicas bit-identical."""
    import socket
    import torch.multiprocessing as mp
    from .conftest import m1_rows, HEADLINE_KW
    b, steps, p = 128, 3, 10000
    kw = dict(HEADLINE_KW, batch_size=b, reduction=r)
    sock = socket.socket()
    sock.bind(('127.0.0.1', 0))
    port = sock.getsockname()[1]
    sock.close()
    mgr = mp.Manager()
    out = mgr.dict()
    seeds = (1234, 4321)
    mp.spawn(_gpu_rank_main_big, args=(2, port, kw, dtype_name, seeds, b, steps, p, out), nprocs=2, join=True)
    dt = np.dtype(dtype_name)
    X0, X1 = m1_rows(b * steps, p, seed=seeds[0]).astype(dt), m1_rows(b * steps, p, seed=seeds[1]).astype(dt)
    Xc = np.concatenate([np.concatenate([X0[t * b:(t + 1) * b], X1[t * b:(t + 1) * b]]) for t in range(steps)])
    pr = oracle.SomfParams(**dict(kw, batch_size=2 * b))
    st = oracle.prepare(pr, n_samples=Xc.shape[0], X=X0)
    oracle.partial_fit(st, pr, Xc)
    tol = 1e-10 if dt == np.float64 else 1e-5
    for rk in (0, 1):
        assert rel_fro(out[rk]['D_head'], st.D[:, :128]) < tol, (rk, rel_fro(out[rk]['D_head'], st.D[:, :128]))
        assert rel_fro(out[rk]['C'], st.C) < tol
        assert rel_fro(out[rk]['B_head'], st.B[:, :64]) < tol
        assert out[rk]['n_iter'] == st.n_iter
    for key in ('D_sum', 'D_sq', 'D_bytes'):                    # replicas stay bit-identical
        assert out[0][key] == out[1][key], key
    assert_array_equal(out[0]['D_head'], out[1]['D_head'])


def _gpu_rank_main_c5(rank, world, port, kw, dtype_name, seeds, nrows, p, out):
    import os
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from modl_amd import DictFact as DF
        from tests.conftest import m1_rows
        dt = np.dtype(dtype_name)
        X0 = m1_rows(max(nrows[0], kw['n_components']), p, seed=seeds[0]).astype(dt)
        X = X0[:nrows[0]] if rank == 0 else m1_rows(nrows[rank], p, seed=seeds[rank]).astype(dt)
        est = DF(**kw)
        est.prepare(n_samples=X.shape[0], X=X0)
        est.partial_fit(X)
        D = est.components_
        out[rank] = dict(D_head=D[:, :256].copy(), D_tail=D[:, -256:].copy(), D_sum=float(D.astype(np.float64).sum()),
                         D_sq=float((D.astype(np.float64) ** 2).sum()), D_bytes=D.tobytes()[:1 << 16],
                         C=est.C_, B_head=est.local_B_[:, :64].copy(), n_iter=est.n_iter_)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize('dtype_name,k,ragged', [('float32', 256, False), ('float64', 64, False), ('float64', 64, True)])
def test_two_rank_gpu_c5_shape(oracle, dtype_name, k, ragged):
    """World size 2 at BASELINE config 5's per-GPU shape (p = 200 000 features, reduction 12: s ~ 16 700 sampled
    features, the 17 MB head [C_r | sampled rows of B_r] summed over gloo, the wide statistics launch, 96-feature
    workgroups in the dictionary update), 64 rows per rank, two minibatches - the second one ragged in the third
    case (40 + 25 rows: weighed with the true global batch size).  R ranks == one rank with the concatenated
    minibatches: f64 (k = 64) <= 1e-10; f32 (k = 256) within the reference algorithm's own f32 noise (the oracle in
    f32 against the oracle in f64 on the same rows); replicas bit-identical."""
    import socket
    import torch.multiprocessing as mp
    from .conftest import m1_rows, HEADLINE_KW, assert_within_f32_noise
    b, p = 64, 200000
    nrows = (b + 40, b + 25) if ragged else (2 * b, 2 * b)
    kw = dict(HEADLINE_KW, n_components=k, batch_size=b, reduction=12)
    sock = socket.socket()
    sock.bind(('127.0.0.1', 0))
    port = sock.getsockname()[1]
    sock.close()
    mgr = mp.Manager()
    out = mgr.dict()
    seeds = (1234, 4321)
    mp.spawn(_gpu_rank_main_c5, args=(2, port, kw, dtype_name, seeds, nrows, p, out), nprocs=2, join=True)
    dt = np.dtype(dtype_name)
    X0 = m1_rows(max(nrows[0], k), p, seed=seeds[0])
    X1 = m1_rows(nrows[1], p, seed=seeds[1])
    parts = [(X0[:b], X1[:b]), (X0[b:nrows[0]], X1[b:nrows[1]])]

    def one_rank(dtype):
        pr = oracle.SomfParams(**dict(kw, batch_size=4 * b))            # (one call = one global minibatch)
        st = oracle.prepare(pr, n_samples=nrows[0] + nrows[1], X=X0.astype(dtype))
        row = 0
        for a, c in parts:
            Xt = np.concatenate([a, c]).astype(dtype)
            oracle.partial_fit(st, pr, Xt, np.arange(row, row + Xt.shape[0]))
            row += Xt.shape[0]
        return st
    st64 = one_rank(np.float64)
    st32 = one_rank(np.float32) if dt == np.float32 else None
    for rk in (0, 1):
        got = out[rk]
        assert got['n_iter'] == st64.n_iter == nrows[0] + nrows[1]
        for name, val, ref in (('D_head', got['D_head'], lambda s_: s_.D[:, :256]), ('D_tail', got['D_tail'], lambda s_: s_.D[:, -256:]),
                               ('C', got['C'], lambda s_: s_.C)):
            if dt == np.float64:
                assert rel_fro(val, ref(st64)) < 1e-10, (rk, name, rel_fro(val, ref(st64)))
            else:
                assert_within_f32_noise(val, ref(st32), ref(st64), (rk, name))
    # the partial sums of B_ (local_B_: no collective) add up to the one-rank statistic
    B_sum = out[0]['B_head'].astype(np.float64) + out[1]['B_head'].astype(np.float64)
    if dt == np.float64:
        assert rel_fro(B_sum, st64.B[:, :64]) < 1e-10
    else:
        assert_within_f32_noise(B_sum, st32.B[:, :64], st64.B[:, :64], 'B')
    for key in ('D_sum', 'D_sq', 'D_bytes'):                    # replicas stay bit-identical
        assert out[0][key] == out[1][key], key
    assert_array_equal(out[0]['D_head'], out[1]['D_head'])
    assert_array_equal(out[0]['D_tail'], out[1]['D_tail'])


def test_bench_two_ranks_share_gpu():
    """bench.py as the driver launches it for N = 2 (torch.distributed.run, one process per rank), both ranks on the
    only GPU of the box over gloo: the JSON line must come out, with bit-identical replicas."""
    import json
    import os
    import socket
    import subprocess
    import sys
    from .conftest import ROOT
    sock = socket.socket()
    sock.bind(('127.0.0.1', 0))
    port = sock.getsockname()[1]
    sock.close()
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
           '--master-port', str(port), os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '12', '--warmup', '4',
           '--share-gpu', '--backend', 'gloo', '--steady-steps', '0']
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith('{')][-1]
    rec = json.loads(line)
    assert rec['n_gpus'] == 2 and rec['replicas_identical'] is True and rec['finite'] is True
    assert rec['config']['global_batch'] == 512 and rec['value'] > 0


def test_bench_four_ranks_share_gpu():
    """The driver's multi-GPU launch beyond two ranks, dry: `python bench.py --gpus 4` starts four ranks (here all on the
    box's one GPU, gloo) at a small shape.  Four ranks, not eight: with this test's own process that is five processes
    holding the device at once, which keeps the suite fit to run on a shared GPU.  Persistent dictionary-update launches that cannot
    become resident next to the other ranks' are completed by their resolver workgroup and their plan falls back to one
    launch per block (`persist_recoveries` in the line counts them) - the replicas must still be bit-identical and finite."""
    import json
    import os
    import subprocess
    import sys
    from .conftest import ROOT
    env = {k_: v for k_, v in os.environ.items() if k_ not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT')}
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '4', '--share-gpu', '--backend', 'gloo',
           '--features', '4096', '--reduction', '4', '--steps', '6', '--warmup', '2', '--steady-steps', '0', '--no-cpu-baseline']
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=1500, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert rec['n_gpus'] == 4 and rec['replicas_identical'] is True and rec['finite'] is True
    assert rec['config']['global_batch'] == 4 * 256 and rec['value'] > 0
    assert rec['persist_recoveries'] >= 0


def test_bench_launches_its_own_ranks():
    """`python bench.py --gpus 2 ...` with NO launcher (the way the driver starts `--gpus 1`): the parent starts the two
    ranks itself before anything touches the GPU and relays rank 0's line as its own last stdout line."""
    import json
    import os
    import subprocess
    import sys
    from .conftest import ROOT
    env = {k_: v for k_, v in os.environ.items() if k_ not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT')}
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--share-gpu', '--backend', 'gloo',
           '--steps', '12', '--warmup', '4', '--steady-steps', '0']
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    last = r.stdout.strip().splitlines()[-1]
    rec = json.loads(last)                                           # the JSON line is the LAST line of stdout
    assert rec['n_gpus'] == 2 and rec['replicas_identical'] is True and rec['finite'] is True
    assert rec['config']['global_batch'] == 512 and rec['value'] > 0


def test_bench_plain_and_full():
    """A plain `bench.py --gpus 1 --steps K --warmup W` fits the warm-up and the timed minibatches and nothing else;
    `--full` adds the untimed section breakdown, both steady_state records and the CPU baseline with its parity block
    (small sizes here, no flip census)."""
    import json
    import os
    import subprocess
    import sys
    from .conftest import ROOT
    env = {k_: v for k_, v in os.environ.items() if k_ not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT')}
    base = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '8', '--warmup', '4']
    recs = []
    for extra in ([], ['--full', '--steady-steps', '8', '--steady-burn-in', '4', '--flip-minibatches', '0,0']):
        r = subprocess.run(base + extra, cwd=ROOT, capture_output=True, text=True, timeout=900, env=env)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        recs.append(json.loads(r.stdout.strip().splitlines()[-1]))
    plain, full = recs
    for rec in recs:
        assert rec['steps'] == 8 and rec['warmup'] == 4 and rec['value'] > 0 and rec['ms_per_step'] > 0
        assert rec['finite'] is True and rec['roofline'] is not None
        assert rec['rows']['generated'] == plain['rows']['generated']
    assert plain['rows']['fitted'] == 12 * 256
    assert plain['sections'] == {} and plain['steady_state'] == []
    assert plain['cpu_baseline'] is None and plain['parity'] is None
    assert full['rows']['fitted'] == 20 * 256
    assert 'dict_update' in full['sections'] and 'code_solve' in full['sections']
    assert [s['reduction'] for s in full['steady_state']] == [10.0, 1.0]
    assert all(s['steps'] == 8 and s['value'] > 0 for s in full['steady_state'])
    assert full['cpu_baseline']['value'] > 0
    assert full['parity']['steps'] >= 1 and full['parity']['flip_rate'] == []
    assert 'parity' in full['steady_state'][1]


def test_c5_shape_step_properties(DictFact):
    """BASELINE config 5's per-GPU shape (p = 200 000 features, k = 256, b = 256, reduction = 12, f32) through both
    the single-GPU step and the two-phase (multi-GPU) step: finite, only sampled columns move, atoms stay in the l2
    ball, run-to-run identical, and the two variants agree bit for bit."""
    import torch
    k, p, b, n, red = 256, 200000, 256, 768, 12
    gen = torch.Generator(device='cuda').manual_seed(5)
    Z = torch.randn(n, 64, device='cuda', generator=gen) * (torch.rand(n, 64, device='cuda', generator=gen) < 0.1)
    X = (Z @ torch.randn(64, p, device='cuda', generator=gen)) / (0.1 * 64) ** 0.5 \
        + 0.1 * torch.randn(n, p, device='cuda', generator=gen)
    X = X.float().contiguous()
    runs = []
    for two_phase in (False, False, True):
        est = DictFact(n_components=k, batch_size=b, reduction=red, code_alpha=1.0, learning_rate=0.92, random_state=0)
        est._two_phase = two_phase
        est.prepare(n_samples=n, X=X[:k])
        D0 = est._backend.Dt.clone()
        rec = Recorder(est)
        est.partial_fit(X[:2 * b])
        D1 = est._backend.Dt
        touched = torch.from_numpy(np.unique(np.concatenate(rec.subsets))).cuda()
        moved = (D1 != D0).any(dim=1)
        assert bool(moved[touched].any()) and int(moved.sum()) <= touched.numel()      # only sampled features move
        mask = torch.ones(p, dtype=torch.bool, device='cuda')
        mask[touched] = False
        assert not bool(moved[mask].any())
        assert bool(torch.isfinite(D1).all()) and bool(torch.isfinite(est._backend.code[:2 * b]).all())
        assert float((D1.double() ** 2).sum(dim=0).max()) <= 1 + 1e-4                  # atoms stay in the l2 ball
        runs.append((D1.clone(), est._backend.code[:2 * b].clone(), est._backend.C.clone(), est._backend.Bt.clone()))
        assert all(abs(len(s_) - p / red) < 6 * (p / red) ** 0.5 for s_ in rec.subsets)
    for a, c in zip(runs[0], runs[1]):
        assert torch.equal(a, c)                                                        # run-to-run deterministic
    for a, c in zip(runs[0], runs[2]):
        assert torch.equal(a, c)                                                        # two-phase == single-GPU step


# ---- the same protocol over RCCL itself: one rank (a 1-GPU box), every all-reduce of the step really issued ------
def _rccl_rank_main(rank, port, kw, X, out):
    import os
    import torch
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    torch.cuda.set_device(0)
    dist.init_process_group('nccl', rank=0, world_size=1)
    try:
        from modl_amd import DictFact as DF
        res = {}
        for name in ('fused', 'rccl', 'native', 'native_chunk'):
            est = DF(**kw)
            if name != 'fused':
                est._two_phase = name != 'native_chunk'          # the Python loop over minibatches / ONE call per chunk
                est._force_reduce = True                         # the head really goes through an RCCL all-reduce
                est._native_rccl = name != 'rccl'                # ... issued by torch.distributed / by the library itself
            est.prepare(n_samples=X.shape[0], X=X)
            est.partial_fit(X)
            res[name] = dict(D=est.components_, C=est.C_, B=est.B_, code=est.code_)
        out.update(res)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize('red', [4, 1])
def test_rccl_single_rank_two_phase_equals_fused(red):
    """The multi-GPU step (phase 1 with the head mirrored, RCCL all-reduce of the head, dictionary update from the
    summed head) on the nccl backend with one rank: summing over one rank is the identity, so the result must equal
    the single-GPU step bit for bit - this checks stream ordering between the HIP kernels and RCCL's own stream on a
    1-GPU box."""
    import socket
    import torch.multiprocessing as mp
    rs = np.random.RandomState(11)
    b, steps, p, k = 64, 12, 2048, 32
    X = (rs.randn(b * steps, 40).dot(rs.randn(40, p)) + 0.3 * rs.randn(b * steps, p)).astype(np.float32)
    kw = dict(n_components=k, batch_size=b, reduction=red, random_state=0, learning_rate=0.9, code_alpha=0.1)
    sock = socket.socket()
    sock.bind(('127.0.0.1', 0))
    port = sock.getsockname()[1]
    sock.close()
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_rccl_rank_main, args=(port, kw, X, out), nprocs=1, join=True)
    for name in ('D', 'C', 'B', 'code'):
        assert_array_equal(out['fused'][name], out['rccl'][name], err_msg=name)
        assert_array_equal(out['fused'][name], out['native'][name], err_msg='native ' + name)   # modl_somf_step_dist
        # modl_somf_partial_fit_chunk with the library's communicator: the staging copy of minibatch t + 1 rides on
        # the last launch of step t's dictionary update, the all-reduce sits between the two phases on the same stream
        assert_array_equal(out['fused'][name], out['native_chunk'][name], err_msg='native_chunk ' + name)


def _comm_abort_main(q):
    import ctypes as C
    import torch
    from modl_amd._lib import lib
    torch.cuda.set_device(0)
    ident = (C.c_char * 128)()
    rc = lib.modl_comm_unique_id(ident)
    if rc == -5:                                                  # MODL_ENORCCL: no librccl on this box
        q.put('norccl')
        return
    h = C.c_void_p()
    with torch.cuda.device(0):
        rcs = [rc, lib.modl_comm_create(ident, 0, 1, C.byref(h))]
    buf = torch.ones(1024, dtype=torch.float32, device='cuda')
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rcs.append(lib.modl_comm_all_reduce_sum(h, C.c_void_p(buf.data_ptr()), 1024, 0, st))
    rcs.append(lib.modl_comm_wait(h, st, 30.0))                   # drains: MODL_OK
    ok_sum = bool((buf == 1).all().item())
    rcs.append(lib.modl_comm_abort(h))
    rcs.append(lib.modl_comm_all_reduce_sum(h, C.c_void_p(buf.data_ptr()), 1024, 0, st))   # MODL_ERCCL, nothing enqueued
    rcs.append(lib.modl_comm_wait(h, st, 30.0))                   # an aborted communicator: MODL_ERCCL
    lib.modl_comm_destroy(h)
    q.put((rcs, ok_sum))


def test_comm_abort_path():
    """ABI 4: modl_comm_wait is a bounded wait that watches RCCL's asynchronous errors, modl_comm_abort ends a
    communicator; afterwards every call on it is MODL_ERCCL (not a hang, not a crash) and destroy still frees it.
    (A child process: RCCL state should not leak into the test session.)"""
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    pr = ctx.Process(target=_comm_abort_main, args=(q,))
    pr.start()
    got = q.get(timeout=300)
    pr.join(60)
    if got == 'norccl':
        pytest.skip('no librccl.so')
    rcs, ok_sum = got
    assert rcs == [0, 0, 0, 0, 0, -6, -6], rcs
    assert ok_sum and pr.exitcode == 0


@pytest.mark.parametrize('dtype,tol', [(np.float64, 1e-12), (np.float32, 1e-5)])
def test_objective_on_device_chunked(dtype, tol):
    """modl_objective_* (the three sums of dict_fact.py:108-112) against numpy, with a workspace that forces
    several row chunks, a padded leading dimension of X, and bit-reproducibility."""
    import ctypes as C
    import torch
    from modl_amd._lib import lib, check
    from modl_amd.device import ptr, stream_ptr
    rs = np.random.RandomState(0)
    n, p, k = 301, 157, 11
    X, D, code = rs.randn(n, p + 3).astype(dtype), rs.randn(k, p).astype(dtype), rs.randn(n, k).astype(dtype)
    code[rs.rand(n, k) < 0.5] = 0
    want = np.array([np.sum((X[:, :p].astype(np.float64) - code.astype(np.float64).dot(D.astype(np.float64))) ** 2),
                     np.sum(np.abs(code.astype(np.float64))), np.sum(code.astype(np.float64) ** 2)])
    dev = torch.device('cuda')
    dX, dDt, dcode = torch.from_numpy(X).to(dev), torch.from_numpy(np.ascontiguousarray(D.T)).to(dev), torch.from_numpy(code).to(dev)
    f = getattr(lib, 'modl_objective_' + ('f32' if dtype == np.float32 else 'f64'))
    outs = []
    for nbytes in (lib.modl_objective_workspace(0 if dtype == np.float32 else 1, n, p), 8 * 1024 + 64 * p * X.itemsize,
                   8 * 1024 + 64 * p * X.itemsize):
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        out = torch.full((3,), -1.0, dtype=torch.float64, device=dev)
        check(f(ptr(dX), p + 3, n, p, ptr(dDt), k, ptr(dcode), ptr(ws), nbytes, ptr(out), stream_ptr(dev)))
        outs.append(out.cpu().numpy())
        assert np.all(np.abs(outs[-1] - want) < tol * want), (outs[-1], want)
    assert np.array_equal(outs[1], outs[2])
    ws = torch.empty(64, dtype=torch.uint8, device=dev)
    assert f(ptr(dX), p + 3, n, p, ptr(dDt), k, ptr(dcode), ptr(ws), 64, ptr(out), stream_ptr(dev)) == -2      # MODL_ENOMEM


@pytest.mark.parametrize('p,k,red', [(1500, 50, 2), (1500, 100, 2), (2040, 40, 1), (900, 130, 3)])
def test_f64_dictionary_update_on_a_few_workgroups(DictFact, oracle, p, k, red):
    """Round 6: the f64 blocked dictionary update of 193 to 2048 sampled features runs as ONE launch on up to sixteen workgroups of
    128 features that exchange a block's Gram record through memory (csrc/bcd.hip: bcd_few_kernel; the shape of a masked minibatch
    of RecsysDictFact).  Against the four launches per block it replaces (MODL_DEBUG_BCD_FEW = 0) and against the oracle, over
    several minibatches: two to five blocks of atoms (the three exchange slots rotate and are restored), a ragged last workgroup."""
    from modl_amd._lib import lib, check, DEBUG_BCD_FEW
    rs = np.random.RandomState(p + k)
    n, b = 4 * 48, 48
    X = rs.randn(n, 20).dot(rs.randn(20, p)) + 0.3 * rs.randn(n, p)
    kw = dict(n_components=k, batch_size=b, reduction=red, code_alpha=0.1, random_state=0, learning_rate=0.9)
    out = {}
    for few in (1, 0):
        check(lib.modl_debug_set(DEBUG_BCD_FEW, few))
        try:
            est = DictFact(**kw)
            est.prepare(n_samples=n, X=X)
            est.partial_fit(X, np.arange(n))
            out[few] = (est.components_, est.comp_norm_, est.code_)
        finally:
            check(lib.modl_debug_set(DEBUG_BCD_FEW, 1))
    pr = oracle.SomfParams(**kw)
    st = oracle.prepare(pr, n_samples=n, X=X)
    oracle.partial_fit(st, pr, X, np.arange(n))
    assert rel_fro(out[1][0], out[0][0]) < 1e-10 and rel_fro(out[1][2], out[0][2]) < 1e-10
    assert np.allclose(out[1][1], out[0][1], rtol=0, atol=1e-10)
    assert rel_fro(out[1][0], st.D) < 1e-9 and rel_fro(out[1][2], st.code) < 1e-9


_MWG_SCRIPT = r"""
import json, sys
import numpy as np
from modl_amd import DictFact
from modl_amd._lib import lib, check, DEBUG_ATOM_MWG, DEBUG_ATOM_PIPE
dtype = np.float32 if sys.argv[1] == 'f32' else np.float64
pos = bool(int(sys.argv[2]))
rs = np.random.RandomState(11)
n, p, k, b = 96, int(sys.argv[5]), int(sys.argv[4]), 32
X = (np.abs(rs.randn(n, 10)).dot(np.abs(rs.randn(10, p))) + 0.2 * rs.randn(n, p)).astype(dtype)
kw = dict(n_components=k, batch_size=b, reduction=2, code_alpha=0.05, code_l1_ratio=0, comp_l1_ratio=1, comp_pos=pos, random_state=0,
          learning_rate=0.9)
out = {}
# (projection, gradient rows): 1 the last workgroup from registers (with riding gradient rows; spread over the launch without) /
# 0 the last workgroup from LDS / 2 the spread attempt gives up / 3 spread over the launch;
# the next group's gradient rows riding on this group's launches (1) or a launch of their own (0)
for v, pipe in ((1, 1), (1, 0), (0, 0), (2, 0), (2, 1), (3, 1)):
    check(lib.modl_debug_set(DEBUG_ATOM_MWG, v))
    check(lib.modl_debug_set(DEBUG_ATOM_PIPE, pipe))
    est = DictFact(**kw)
    est.prepare(n_samples=n, X=X)
    est.partial_fit(X, np.arange(n))
    out[(v, pipe)] = dict(D=est.components_.astype(np.float64), cn=est.comp_norm_.astype(np.float64))
check(lib.modl_debug_set(DEBUG_ATOM_MWG, 1))
check(lib.modl_debug_set(DEBUG_ATOM_PIPE, 1))
np.savez(sys.argv[3], X=X, **{'%s%d%d' % (name, v, pipe): o[name] for (v, pipe), o in out.items() for name in ('D', 'cn')})
print(json.dumps(dict(ok=True)))
"""


@pytest.mark.parametrize('dt,pos,k,p', [('f32', 1, 12, 15000), ('f64', 1, 12, 15000), ('f64', 0, 12, 15000), ('f64', 1, 14, 18000),
                                        ('f32', 0, 7, 18000), ('f32', 1, 12, 24000)])
def test_l1_projection_spread_over_the_launch(tmp_path, dt, pos, k, p):
    """Round 6, the per-atom l1 sweep of more than 6144 sampled features (one launch per atom: the shape class of the reference's
    HCP run).  The gradient rows of the next group of four atoms ride on the launches of this group's atoms (MODL_DEBUG_ATOM_PIPE;
    what this group changes is subtracted afterwards, the last two groups are put home at the end; k = 14 and 7: a short last
    group).  The projection: by the launch's last workgroup with the vector in registers (40 elements per thread, the default),
    spread over the launch's workgroups (= 3: every thread keeps an element or two, a Michelot pass is one exchange of sums through
    memory, csrc/bcd.hip: mwg_l1_project), by the last workgroup from LDS (= 0, a gradient launch per group: the old path).
    Against the old path, against a run in which a workgroup withholds its sums (diagnostics build, = 2: every wait gives up, the
    abort word is raised and the last workgroup projects the candidates alone - with a gradient launch per group the results must
    be the old path's BIT FOR BIT, with the riding rows they must be the pipelined run's to rounding) and against the oracle:
    7500 sampled features of 15 000 (30 workgroups, an element per thread) and 9000 of 18 000 (two elements per thread on 18
    workgroups: what the reference's HCP shape takes) and 12 000 of 24 000 (64 elements per thread of the projecting workgroup),
    l1 atoms with and without positivity."""
    from oracle import somf_oracle as orc
    from .conftest import assert_within_f32_noise
    f = str(tmp_path / 'mwg.npz')
    _run_diag_script(_MWG_SCRIPT, dt, str(pos), f, str(k), str(p))
    z = np.load(f)
    assert np.array_equal(z['D20'], z['D00']) and np.array_equal(z['cn20'], z['cn00'])       # the fallback IS the old path
    X = z['X']
    n, b = X.shape[0], 32
    kw = dict(n_components=k, batch_size=b, reduction=2, code_alpha=0.05, code_l1_ratio=0, comp_l1_ratio=1, comp_pos=bool(pos),
              random_state=0, learning_rate=0.9)
    pr = orc.SomfParams(**kw)
    st64 = orc.prepare(pr, n_samples=n, X=X.astype(np.float64))
    orc.partial_fit(st64, pr, X.astype(np.float64), np.arange(n))
    if dt == 'f64':
        for name in ('D11', 'D10', 'D21', 'D31'):
            assert rel_fro(z[name], z['D00']) < 1e-10, name
            assert rel_fro(z[name], st64.D) < 1e-8, name
        assert rel_fro(z['D00'], st64.D) < 1e-8
        for name in ('cn11', 'cn21', 'cn31'):
            assert np.allclose(z[name], z['cn00'], rtol=0, atol=1e-9), name
    else:
        st32 = orc.prepare(pr, n_samples=n, X=X)
        orc.partial_fit(st32, pr, X, np.arange(n))
        assert_within_f32_noise(z['D11'], st32.D, st64.D, 'dictionary, the last workgroup projects from registers, riding gradient rows')
        assert_within_f32_noise(z['D10'], st32.D, st64.D, 'dictionary, projection spread over the launch')
        assert_within_f32_noise(z['D21'], st32.D, st64.D, 'dictionary, riding gradient rows, the spread attempt gives up')
        assert_within_f32_noise(z['D31'], st32.D, st64.D, 'dictionary, projection spread over the launch, riding gradient rows')
        assert_within_f32_noise(z['D00'], st32.D, st64.D, 'dictionary, last workgroup')
    if pos:
        assert (z['D11'] >= 0).all() and (z['D21'] >= 0).all() and (z['D31'] >= 0).all()


@pytest.mark.parametrize('r', [10, 1])
def test_sweep_flip_rate(r):
    """the f32 parity gates allow for samples that do one coordinate-descent sweep more or less than in
    the f64 run (a tolerance-stopped solver, a duality gap on the threshold).  That allowance rests on the premise that the GPU
    path does not flip MORE OFTEN than the reference algorithm's own f32 arithmetic does - measured here instead of assumed:
    102 400 (reduction 10) / 51 200 (reduction 1) fresh samples of stream M1 at the metric's full shape through the f64 oracle, the
    f32 oracle and the GPU estimator (bench.py: flip_rate_block; the oracle's two runs take 0.27 / 0.77 s per minibatch on the GPU
    box's host - MODL_FLIP_MINIBATCHES overrides, profiles/r06_flip_census.json is the 204 800-sample run of both); every sample's
    sweep count compared with the f64 run's.
    GPU flips <= 2 x the f32 oracle's + 2; before its first flip each f32 run is within the north star's 1e-5 of the f64 run."""
    import importlib.util
    import json
    import os
    import sys
    from .conftest import ROOT
    spec = importlib.util.spec_from_file_location('bench_for_flips', os.path.join(ROOT, 'bench.py'))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    import torch
    nmb = int(os.environ.get('MODL_FLIP_MINIBATCHES', '400' if r == 10 else '200'))
    out = bench.flip_rate_block(float(r), nmb, torch.device('cuda', 0))
    sys.stderr.write('\nflip census r=%d: %s\n' % (r, json.dumps(out)))
    os.makedirs(os.path.join(ROOT, 'gpurun_out'), exist_ok=True)
    with open(os.path.join(ROOT, 'gpurun_out', 'flip_rate_r%d.json' % r), 'w') as fh:
        json.dump(out, fh)
    assert out['samples'] == nmb * 256
    assert out['gpu_f32_flips'] <= 2 * out['oracle_f32_flips'] + 2, out
    # while it has not flipped the GPU run is within the north star's 1e-5 of the f64 run - or, over horizons where the reference
    # algorithm's own f32 run is not (measured: 1.1e-5 after 200 flip-free minibatches at reduction 1, with the GPU at 3.3e-6),
    # within that run's distance
    if 'gpu_f32_rel_fro_flip_free' in out:
        g, o = out['gpu_f32_rel_fro_flip_free'], out.get('oracle_f32_rel_fro_flip_free')
        same = o is not None and o['minibatches'] == g['minibatches']
        for key in ('D', 'C'):
            assert g[key] <= max(1e-5, o[key] if same else 0.0), (key, g, o)


_PERSIST_RECOVERY_SCRIPT = r"""
import json, sys, warnings
import numpy as np
from modl_amd import DictFact
from modl_amd._lib import lib, check, ModlError, DEBUG_BCD_PERSIST
assert lib.modl_is_diag_build() == 1
mode = sys.argv[1]
rs = np.random.RandomState(5)
n, p, k, b = 512, 600, 64, 64
X = (rs.randn(n, 24).dot(rs.randn(24, p)) + 0.3 * rs.randn(n, p)).astype(np.float32)
kw = dict(n_components=k, batch_size=b, reduction=3, code_alpha=0.2, random_state=0)
out = {}
if mode == 'recover':
    # A: the second partial_fit's FIRST persistent launch cannot run (a workgroup that never arrives); B: one launch per block
    check(lib.modl_debug_set(DEBUG_BCD_PERSIST, 1))
    A = DictFact(**kw); A.prepare(n_samples=n, X=X)
    A.partial_fit(X[:b], np.arange(b))
    check(lib.modl_debug_set(DEBUG_BCD_PERSIST, 3))
    with warnings.catch_warnings(record=True) as wlist:
        warnings.simplefilter('always')
        A.partial_fit(X[b:4 * b], np.arange(b, 4 * b))          # three minibatches: recovered while the flag is unseen, then block launches
        D_mid = A.components_.copy()
    out['warned'] = sum('could not run' in str(w.message) for w in wlist)
    out['recoveries'] = int(A._backend.persist_recoveries)
    check(lib.modl_debug_set(DEBUG_BCD_PERSIST, 1))
    A.partial_fit(X[4 * b:], np.arange(4 * b, n))               # no prepare(): the estimator carries on
    check(lib.modl_debug_set(DEBUG_BCD_PERSIST, 0))
    B = DictFact(**kw); B.prepare(n_samples=n, X=X)
    B.partial_fit(X[:b], np.arange(b))
    B.partial_fit(X[b:4 * b], np.arange(b, 4 * b))
    DB_mid = B.components_.copy()
    B.partial_fit(X[4 * b:], np.arange(4 * b, n))
    rel = lambda a, c: float(np.linalg.norm(a - c) / np.linalg.norm(c))
    out['mid'] = rel(D_mid, DB_mid)
    out['end'] = rel(A.components_, B.components_)
    out['code'] = rel(A.code_, B.code_)
    out['norms_ok'] = bool(np.all(np.sum(A.components_ ** 2, axis=1) <= 1 + 1e-5))
    np.save(sys.argv[2], A.components_)
else:
    # the resolver loses a workgroup from the SECOND block on: S_0 has been applied, the update is incomplete
    A = DictFact(**kw); A.prepare(n_samples=n, X=X)
    A.partial_fit(X[:b], np.arange(b))
    check(lib.modl_debug_set(DEBUG_BCD_PERSIST, 4))
    try:
        A.partial_fit(X[b:4 * b], np.arange(b, 4 * b))
        out['raised'] = ''
    except ModlError as e:
        out['raised'] = str(e)
    check(lib.modl_debug_set(DEBUG_BCD_PERSIST, 1))
    A.prepare(n_samples=n, X=X)                                  # (the dictionary of the failed update is not to be trusted)
    A.partial_fit(X, np.arange(n))
    out['finite'] = bool(np.all(np.isfinite(A.components_)))
print(json.dumps(out))
"""


def _run_diag_script(script, *args):
    import json
    import os
    import subprocess
    import sys
    from .conftest import ROOT
    env = dict(os.environ)
    env['MODL_AMD_DIAG'] = '1'
    env['PYTHONPATH'] = ROOT + os.pathsep + env.get('PYTHONPATH', '')
    r = subprocess.run([sys.executable, '-c', script] + list(args), cwd=ROOT, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_persistent_launch_recovers(tmp_path):
    """The persistent dictionary-update launch needs every workgroup resident; when one never arrives (another process or a mask
    holding compute units: here simulated in the diagnostics build - modl_debug_set(MODL_DEBUG_BCD_PERSIST, 3) makes the resolver
    wait for nrow + 1 arrivals before the first block) nothing has been applied yet: the row workgroups leave, the resolver
    workgroup runs the sweep by itself (bcd_persist.hip: persist_recover) and the stream carries on.  No error, no prepare(): the
    estimator warns once, counts the event, keeps one launch per block from then on, and ends where the run on block launches
    ends, to f32 rounding (the recovered update sums in another order than the block kernel; the other minibatches then run
    the very same kernels on inputs that differ in the last bits)."""
    from oracle import somf_oracle as orc
    f = str(tmp_path / 'D.npy')
    out = _run_diag_script(_PERSIST_RECOVERY_SCRIPT, 'recover', f)
    # (the host enqueues ahead: up to the whole call's three launches may have been enqueued before the first recovery is seen)
    assert out['warned'] == 1 and 1 <= out['recoveries'] <= 3, out
    assert out['norms_ok'], out
    # right behind the recovered minibatches the two runs agree to f32 rounding; four more minibatches on this small,
    # ill-conditioned problem (k = 64 atoms on 200 sampled features) amplify that to 1e-4-class differences on the dictionary
    # and more on single codes (measured 3e-4 / 4e-3) - which is what the oracle comparison below is for
    assert out['mid'] < 2e-5 and out['end'] < 2e-3, out
    # ... and against the oracle, like any other fit
    rs = np.random.RandomState(5)
    n, p, k, b = 512, 600, 64, 64
    X = (rs.randn(n, 24).dot(rs.randn(24, p)) + 0.3 * rs.randn(n, p)).astype(np.float32)
    kw = dict(n_components=k, batch_size=b, reduction=3, code_alpha=0.2, random_state=0)
    from .conftest import assert_within_f32_noise
    pr = orc.SomfParams(**kw)
    st = orc.prepare(pr, n_samples=n, X=X.astype(np.float64), dtype=np.float64)
    st32 = orc.prepare(pr, n_samples=n, X=X)
    for lo, hi in ((0, b), (b, 4 * b), (4 * b, n)):
        orc.partial_fit(st, pr, X[lo:hi].astype(np.float64), np.arange(lo, hi))
        orc.partial_fit(st32, pr, X[lo:hi], np.arange(lo, hi))
    assert_within_f32_noise(np.load(f), st32.D, st.D, 'dictionary after a recovered launch')


def test_persistent_launch_incomplete_update_is_loud():
    """A wait that gives up AFTER the first block has been resolved (diagnostics build, MODL_DEBUG_BCD_PERSIST = 4) leaves the
    update incomplete: the plan's flag stops every further enqueue (MODL_ETIMEOUT from the next step - not only from the next
    synchronisation) and the fit raises; after prepare() the estimator works again."""
    out = _run_diag_script(_PERSIST_RECOVERY_SCRIPT, 'incomplete')
    assert 'gave up' in out['raised'], out
    assert out['finite'], out


def test_bench_c5_shape_forced_reduce():
    """BASELINE config 5's per-GPU shape as a first-class bench workload: `bench.py --features 200000 --reduction 12
    --force-reduce` prints the same line (config.workload names C5), the two-phase step with the library's own RCCL
    communicator runs as ONE modl_somf_partial_fit_chunk call per chunk also at p = 200 000 (subsets drawn ahead on the
    call's worker thread), and the roofline names the section that dominates there."""
    import json
    import os
    import subprocess
    import sys
    from .conftest import ROOT
    env = {k_: v for k_, v in os.environ.items() if k_ not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT')}
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    import socket
    sock = socket.socket()
    sock.bind(('127.0.0.1', 0))
    env['MASTER_PORT'] = str(sock.getsockname()[1])
    sock.close()
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--features', '200000', '--reduction', '12',
           '--force-reduce', '--steps', '6', '--warmup', '3', '--no-cpu-baseline']
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert rec['n_gpus'] == 1 and rec['finite'] is True and rec['value'] > 0 and rec['steps'] == 6
    assert 'C5' in rec['config']['workload'] and 'p=200k' in rec['metric']
    assert rec['config']['collective'].startswith('native RCCL'), rec['config']['collective']
    assert rec['roofline'] is not None and rec['roofline']['kernel'] in ('stats_gemm', 'dict_update', 'code_gemm', 'code_solve')
    assert rec['steady_state'] == []


def test_bench_forced_reduce_native_rccl():
    """`bench.py --gpus 1 --force-reduce --native-rccl`: the multi-GPU step as the driver's N > 1 runs execute it - one
    modl_somf_partial_fit_chunk call per chunk with the library's own RCCL communicator (world = 1: the all-reduce is the
    identity, its launch and stream ordering are real), the staging copy riding on phase 2's last launch."""
    import json
    import os
    import subprocess
    import sys
    from .conftest import ROOT
    env = {k_: v for k_, v in os.environ.items() if k_ not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT')}
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    import socket
    sock = socket.socket()
    sock.bind(('127.0.0.1', 0))
    env['MASTER_PORT'] = str(sock.getsockname()[1])
    sock.close()
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--force-reduce', '--native-rccl',
           '--steps', '12', '--warmup', '4', '--steady-steps', '0', '--no-cpu-baseline']
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert rec['n_gpus'] == 1 and rec['finite'] is True and rec['value'] > 0
    assert rec['config']['collective'].startswith('native RCCL'), rec['config']['collective']
