"""Connected regions of maps on the device: modl_amd.regions, csrc/regions.hip.

Every result is an integer or a bit-for-bit copy of an input element, so every comparison here is exact.

The judge is the pair of scipy twins, `region_labels_host` / `connected_regions_host` (scipy.ndimage.label, one map at a
time).  Layer 1 (no GPU) holds the judge itself to an independent restatement in plain numpy - labelling by min-propagation to
a fixed point, the order statistic from np.sort -, shows that the phantoms discriminate (every option changes the result)
and that each mutant of the restatement is rejected by at least one case; then the refusals of the entry points and
`extract_regions` on the oracle backend.  Layer 2 (gpu): the kernels through the C-ABI inside guard elements with a poisoned
workspace, then the Python functions and the estimators on the device, all against the judge.

The module imports the new names at the top: no test here can pass without the feature."""
import ctypes as C
import warnings

import numpy as np
import pytest

from modl_amd import masker as M
from modl_amd import regions as R
from modl_amd.regions import (Regions, connected_regions, region_labels, connected_regions_host,  # noqa: F401
                              region_labels_host)

from .test_clean import DT, EINVAL, ENOMEM, ENOGPU, same_bits
from .test_compute_mask import re_label, serpentine, u_shape, boxes, _Guarded, _Workspace, gpu  # noqa: F401

MUTANTS = ('conn26', 'size_ge', 'cutoff_gt', 'no_abs', 'cutoff_box', 'percentile', 'by_size', 'memory_order', 'nan_foreground',
           'merged')


# ------------------------------------------------------------------------------------------- the restatement (numpy)
def re_cutoff(comp, mask, threshold, strategy, mutant=None):
    dt = comp.dtype.type
    if strategy is None:
        return dt(0)
    if strategy == 'value':
        return dt(threshold)
    k, V = comp.shape
    a = comp.copy() if mutant == 'no_abs' else np.abs(comp)
    a[~np.isfinite(comp)] = 0
    a = a.ravel()
    if mutant == 'percentile':                                  # nilearn: an interpolated percentile
        return dt(np.percentile(a, 100.0 * (1.0 - threshold * V / a.size)))
    if mutant == 'cutoff_box':                                  # nilearn: over the whole box, zeros outside the mask included
        a = np.concatenate([a, np.zeros(k * (mask.size - V), dtype=a.dtype)])
        V = mask.size
    n_keep = min(a.size, max(1, int(np.floor(threshold * V + 0.5))))
    return np.sort(a)[a.size - n_keep]


def re_regions(comp, mask, min_region_size=1350, threshold=None, strategy=None, voxel_size=(1, 1, 1), mask_affine=None,
               mutant=None):
    """(labels, counts, Regions) by the rules of the module docstring of modl_amd.regions, in plain numpy"""
    k, V = comp.shape
    c = re_cutoff(comp, mask, threshold, strategy, mutant)
    volume = abs(np.linalg.det(np.asarray(mask_affine, np.float64)[:3, :3])) if mask_affine is not None else \
        float(np.prod(np.asarray(voxel_size, np.float64)))
    t = np.float64(min_region_size) / np.float64(volume)
    with np.errstate(invalid='ignore'):
        if mutant == 'nan_foreground':
            fg = ~(np.abs(comp) < c) & (comp != 0)
        elif mutant == 'no_abs':
            fg = np.isfinite(comp) & (comp != 0) & (comp >= c)
        elif mutant == 'cutoff_gt':
            fg = np.isfinite(comp) & (comp != 0) & (np.abs(comp) > c)
        else:
            fg = np.isfinite(comp) & (comp != 0) & (np.abs(comp) >= c)
    X, Y, Z = mask.shape
    x, y, z = np.unravel_index(np.arange(mask.size), mask.shape)
    memory = ((z * Y + y) * X + x).reshape(mask.shape)          # the kernels' flat index of a voxel
    merged = None
    if mutant == 'merged':
        vol = np.zeros(mask.shape, bool)
        vol[mask] = fg.any(axis=0)
        merged = re_label(vol)
    labels = np.zeros((k, V), np.int32)
    counts = np.zeros(k, np.int64)
    rows, index, sizes = [], [], []
    for m in range(k):
        vol = np.zeros(mask.shape, bool)
        vol[mask] = fg[m]
        lab = np.where(vol, merged, mask.size) if merged is not None else re_label(vol, mutant == 'conn26')
        roots, n_vox = np.unique(lab[vol], return_counts=True)  # ascending first voxel in C order: scipy's numbering
        keep = n_vox >= t if mutant == 'size_ge' else n_vox > t
        roots, n_vox = roots[keep], n_vox[keep]
        if mutant == 'by_size':
            order = np.argsort(-n_vox, kind='stable')
            roots, n_vox = roots[order], n_vox[order]
        if mutant == 'memory_order':
            order = np.argsort([memory[lab == r].min() for r in roots], kind='stable')
            roots, n_vox = roots[order], n_vox[order]
        flat = lab[mask]
        for j, (r, n) in enumerate(zip(roots, n_vox)):
            at = flat == r
            labels[m, at] = j + 1
            rows.append(np.where(at, comp[m], comp.dtype.type(0)))
            index.append(m)
            sizes.append(n)
        counts[m] = len(roots)
    regions = np.array(rows, dtype=comp.dtype).reshape(len(rows), V)
    return labels, counts, Regions(regions, np.array(index, np.int64), np.array(sizes, np.int64))


def same_result(a, b):
    return (same_bits(a[0], b[0]) and same_bits(a[1], b[1]) and same_bits(a[2].regions, b[2].regions)
            and same_bits(a[2].index, b[2].index) and same_bits(a[2].sizes, b[2].sizes))


def judge(comp, mask, **kw):
    kw = dict(kw)
    kw['thresholding_strategy'] = kw.pop('strategy', None)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        labels, counts = region_labels_host(comp, mask, **kw)
        return labels, counts, connected_regions_host(comp, mask, **kw)


# ------------------------------------------------------------------------------------------------------- the phantoms
PHANTOM_KW = dict(min_region_size=4, threshold=0.5, strategy='value')          # unit voxels: kept iff more than 4 voxels


def phantom(dt):
    """(comp (3, V), mask (7, 6, 5)).  Map 0 at the cutoff 0.5 and a minimum of 4 voxels:
      C1  5 voxels from (0, 0, 4): the first region in user order, the last in memory order, smaller than C2;
      C2  6 voxels from (1, 0, 0): the first in memory order;
      D0  (0, 1, 0) alone: the row-neighbour of C1's (0, 0, 4), no box-neighbour of it;
      A   exactly 4 voxels (dropped); B  5 voxels (kept) with a tie at the cutoff (0.5) and a negative element (-0.8);
      NaN, +Inf and -Inf next to B; D1 (2, 2, 1), diagonal to B; 0.3 at (4, 4, 2) joins A and B below the cutoff.
    Map 1 is all zero.  Map 2 is one region of 6 voxels that overlaps A and B and bridges them."""
    mask = np.ones((7, 6, 5), bool)
    mask[6, 5, :] = False
    mask[0, 3, 2] = False
    v = np.zeros((3,) + mask.shape, np.float64)
    for p in [(0, 0, 4), (0, 1, 4), (0, 2, 4), (0, 1, 3), (0, 2, 3)]:
        v[0][p] = 1.25
    for p in [(1, 0, 0), (2, 0, 0), (3, 0, 0), (1, 0, 1), (2, 0, 1), (3, 0, 1)]:
        v[0][p] = -2.0
    v[0][0, 1, 0] = 0.9
    for p in [(5, 4, 0), (5, 4, 1), (5, 4, 2), (5, 4, 3)]:
        v[0][p] = 0.75
    for p in [(3, 3, 1), (3, 3, 2), (3, 3, 3)]:
        v[0][p] = 1.0
    v[0][4, 3, 2] = 0.5
    v[0][3, 2, 2] = -0.8
    v[0][3, 4, 2], v[0][2, 3, 2], v[0][3, 3, 0] = np.nan, np.inf, -np.inf
    v[0][2, 2, 1] = 0.7
    v[0][4, 4, 2] = 0.3
    for p in [(3, 3, 2), (4, 3, 2), (4, 4, 2), (5, 4, 2), (5, 4, 3), (5, 4, 1)]:
        v[2][p] = 1.5
    return np.ascontiguousarray(np.stack([x[mask] for x in v]).astype(dt)), mask


def random_case(dt, shape, k, density, seed, mask_density=0.8, quantized=False):
    """k random maps at a foreground density under a random mask; map k // 2 is all zero when k >= 3"""
    rs = np.random.RandomState(seed)
    mask = rs.rand(*shape) < mask_density
    mask.flat[0] = True
    V = int(mask.sum())
    vals = rs.randint(-3, 4, size=(k, V)).astype(np.float64) if quantized else rs.randn(k, V)
    comp = vals * (rs.rand(k, V) < density)
    if k >= 3:
        comp[k // 2] = 0
    return np.ascontiguousarray(comp.astype(dt)), mask


def cases(dt):
    """(name, comp, mask, options) - what the restatement, the judge and the mutants are run on"""
    comp, mask = phantom(dt)
    out = [('phantom', comp, mask, PHANTOM_KW),
           ('phantom none', comp, mask, dict(min_region_size=0)),
           ('phantom ratio', comp, mask, dict(min_region_size=1, threshold=0.1, strategy='ratio_n_voxels')),
           ('phantom affine', comp, mask, dict(PHANTOM_KW, mask_affine=np.diag([2.0, -1.0, 1.0, 1.0])))]
    for i, shape in enumerate([(3, 5, 7), (6, 4, 5)]):
        comp, mask = random_case(dt, shape, 5, 0.9, 40 + i)
        V = comp.shape[1]
        # r V = an integer + 0.3: the order statistic rounds down where an interpolated percentile lets one more through
        out.append(('ratio %d' % i, comp, mask, dict(min_region_size=0, threshold=(int(0.9 * V) + 0.3) / V, strategy='ratio_n_voxels')))
        comp, mask = random_case(dt, shape, 5, 0.7, 50 + i, quantized=True)
        out.append(('ties %d' % i, comp, mask, dict(min_region_size=1, threshold=2.0, strategy='ratio_n_voxels')))
        out.append(('sized %d' % i, comp, mask, dict(min_region_size=9, voxel_size=(1.5, 1, 2), threshold=1.0, strategy='value')))
    return out


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_restatement_agrees_with_the_scipy_twins(dt):
    for name, comp, mask, kw in cases(DT[dt]):
        got, ref = re_regions(comp, mask, **kw), judge(comp, mask, **kw)
        assert same_result(got, ref), name
        labels, counts, reg = ref
        assert labels.dtype == np.int32 and counts.dtype == np.int64 and reg.regions.dtype == comp.dtype
        assert reg.index.dtype == np.int64 and reg.sizes.dtype == np.int64
        assert reg.regions.shape == (counts.sum(), comp.shape[1]) and np.array_equal(np.bincount(reg.index, minlength=len(counts)), counts)
        assert np.array_equal((reg.regions != 0).sum(axis=1), reg.sizes), name


def test_phantoms_discriminate():
    comp, mask = phantom(np.float64)
    col = {p: c for c, p in enumerate(zip(*np.nonzero(mask)))}
    labels, counts, reg = judge(comp, mask, **PHANTOM_KW)
    assert counts.tolist() == [3, 0, 1] and reg.index.tolist() == [0, 0, 0, 2] and reg.sizes.tolist() == [5, 6, 5, 6]
    first = [int(np.flatnonzero(r)[0]) for r in reg.regions]
    assert first == [col[0, 0, 4], col[1, 0, 0], col[3, 2, 2], col[3, 3, 2]]      # C1, C2, B; map 2's bridge
    assert labels[0, col[0, 1, 0]] == 0 and col[0, 1, 0] == col[0, 0, 4] + 1      # the row-neighbour is not connected
    assert all(labels[0, col[5, 4, z]] == 0 for z in range(4))                    # A: exactly the minimum, dropped
    assert reg.regions[2, col[4, 3, 2]] == 0.5 and reg.regions[2, col[3, 2, 2]] == -0.8    # the tie and the sign are kept
    assert all(labels[0, col[p]] == 0 for p in [(3, 4, 2), (2, 3, 2), (3, 3, 0), (2, 2, 1), (4, 4, 2)])
    assert labels[0, col[4, 3, 2]] == 3 and labels[2, col[4, 3, 2]] == 1           # two maps overlap in space
    # memory order would number C2 (and B) before C1
    X, Y, Z = mask.shape
    mem = [min((z * Y + y) * X + x for (x, y, z), c in col.items() if labels[0, c] == j) for j in (1, 2, 3)]
    assert mem[1] < mem[2] < mem[0]
    # every option changes the result
    base = judge(comp, mask, **PHANTOM_KW)
    for change in (dict(min_region_size=3.9), dict(min_region_size=5), dict(threshold=0.51), dict(threshold=0.2),
                   dict(threshold=None, strategy=None), dict(threshold=1.0, strategy='ratio_n_voxels'), dict(voxel_size=(2, 1, 1)),
                   dict(mask_affine=np.diag([1.0, 1.0, 0.5, 1.0]))):
        assert not same_result(judge(comp, mask, **dict(PHANTOM_KW, **change)), base), change
    assert same_result(judge(comp, mask, **dict(PHANTOM_KW, voxel_size=(3, 3, 3), mask_affine=np.eye(4))), base)   # the affine wins
    # without a cutoff the 0.3 joins A and B
    none = judge(comp, mask, min_region_size=4)
    assert none[1].tolist() == [3, 0, 1] and none[2].sizes.tolist() == [5, 6, 10, 6]


@pytest.mark.parametrize('mutant', MUTANTS)
def test_the_judge_rejects_the_mutant(mutant):
    rejected = [name for name, comp, mask, kw in cases(np.float64)
                if not same_result(re_regions(comp, mask, mutant=mutant, **kw), judge(comp, mask, **kw))]
    assert rejected, mutant


def test_empty_result_warns_and_value_errors_name_the_offender():
    comp, mask = phantom(np.float32)
    for fn in (connected_regions_host, connected_regions):
        with pytest.warns(UserWarning, match='no region is left'):
            reg = fn(comp, mask, min_region_size=1000)
        assert reg.regions.shape == (0, comp.shape[1]) and reg.regions.dtype == np.float32
        assert reg.index.shape == (0,) and reg.index.dtype == np.int64 and reg.sizes.shape == (0,) and reg.sizes.dtype == np.int64
    for fn in (connected_regions, region_labels, connected_regions_host, region_labels_host):
        for kw, match in ((dict(thresholding_strategy='percentile', threshold=1), "'ratio_n_voxels'"),
                          (dict(threshold=0.5), 'needs a thresholding_strategy'),
                          (dict(thresholding_strategy='value'), 'needs a number'),
                          (dict(thresholding_strategy='value', threshold=-1), '>= 0'),
                          (dict(thresholding_strategy='ratio_n_voxels', threshold=0), r'\(0, 3\]'),
                          (dict(thresholding_strategy='ratio_n_voxels', threshold=3.01), r'\(0, 3\]'),
                          (dict(voxel_size=(1, 0, 1)), 'voxel_size'), (dict(mask_affine=np.eye(3)), 'mask_affine'),
                          (dict(min_region_size=np.nan), 'min_region_size')):
            with pytest.raises(ValueError, match=match):
                fn(comp, mask, **kw)
        with pytest.raises(ValueError, match=r'components must be \(k, %d\)' % comp.shape[1]):
            fn(comp[:, :-1], mask)
        with pytest.raises(ValueError, match='3-D boolean'):
            fn(comp, mask.astype(np.uint8))
    with pytest.raises(ValueError, match='maps_per_pass'):
        from modl_amd.regions import _maps_per_pass
        _maps_per_pass(0, 3, (5, 6, 7), None)


# -------------------------------------------------------------------------------------------- refusals of the entry points
def _labels_call(lib, dt, p, over=None):
    a = dict(rows=p['rows'], ldr=60, M=2, V=50, col=p['col'], n=(5, 4, 3), cutoff=0.5, minv=1, labels=p['labels'], ldl=55,
             counts=p['counts'], sizes=p['sizes'], cap=25, ws=p['ws'], ws_bytes=lib.modl_region_labels_workspace(2, 5, 4, 3))
    a.update(over or {})
    return getattr(lib, 'modl_region_labels_' + dt)(a['rows'], a['ldr'], a['M'], a['V'], a['col'], *a['n'], a['cutoff'], a['minv'],
                                                   a['labels'], a['ldl'], a['counts'], a['sizes'], a['cap'], a['ws'], a['ws_bytes'],
                                                   None)


def _gather_call(lib, dt, p, over=None):
    a = dict(rows=p['rows'], ldr=60, M=2, V=50, labels=p['labels'], ldl=55, offsets=p['offsets'], R=3, out=p['out'], ldo=52)
    a.update(over or {})
    return getattr(lib, 'modl_region_gather_' + dt)(a['rows'], a['ldr'], a['M'], a['V'], a['labels'], a['ldl'], a['offsets'], a['R'],
                                                   a['out'], a['ldo'], None)


BAD_BOXES = [(0, 4, 3), (5, 0, 3), (5, 4, 0), (-5, 4, 3), (5, -4, 3), (5, 4, -3), (1 << 11, 1 << 10, 1 << 10)]


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_entry_points_refuse_bad_arguments_without_a_device(dt):
    from modl_amd._lib import lib
    bufs = dict(rows=np.ones(2 * 60, DT[dt]), col=np.arange(60, dtype=np.int32), labels=np.zeros(2 * 55, np.int32),
                counts=np.zeros(2, np.int32), sizes=np.zeros(2 * 25, np.int32), ws=np.zeros(1 << 14, np.uint8),
                offsets=np.array([0, 1, 3], np.int64), out=np.zeros(3 * 52, DT[dt]))
    p = {k: v.ctypes.data for k, v in bufs.items()}
    need = lib.modl_region_labels_workspace(2, 5, 4, 3)
    assert 16 * 2 * 60 <= need <= bufs['ws'].nbytes
    assert lib.modl_region_labels_workspace(1, 5, 4, 3) < need
    for bad in BAD_BOXES:
        assert lib.modl_region_labels_workspace(2, *bad) == 0 and lib.modl_region_max_maps(*bad, 1 << 30) == 0, bad
        assert _labels_call(lib, dt, p, dict(n=bad)) == EINVAL, bad
    for M_ in (0, -1, 65536):
        assert lib.modl_region_labels_workspace(M_, 5, 4, 3) == 0 and _labels_call(lib, dt, p, dict(M=M_)) == EINVAL
    assert lib.modl_region_labels_workspace(1, (1 << 31) - 1, 1, 1) == 0         # more tiles along n0 than a grid axis holds
    assert lib.modl_region_labels_workspace(1, 1, 1, (1 << 31) - 1) > 0          # int32 indexes the largest box
    assert lib.modl_region_labels_workspace(1, 1, 2, 1 << 30) == 0               # one voxel more is refused
    # the largest chunk within a budget: monotone, exact at the edge, capped by a grid axis
    assert lib.modl_region_max_maps(5, 4, 3, need) == 2 and lib.modl_region_max_maps(5, 4, 3, need - 1) == 1
    assert lib.modl_region_max_maps(5, 4, 3, 0) == 0 and lib.modl_region_max_maps(5, 4, 3, 1 << 40) == 65535
    for k in ('rows', 'col', 'labels', 'counts', 'sizes'):
        assert _labels_call(lib, dt, p, {k: None}) == EINVAL, k
    for over in (dict(V=0), dict(V=61), dict(ldr=49), dict(ldl=49), dict(cutoff=-0.5), dict(cutoff=float('nan')), dict(cap=-1),
                 dict(labels=p['rows']), dict(labels=p['col']), dict(counts=p['labels'] + 8), dict(sizes=p['labels'] + 4),
                 dict(sizes=p['counts']), dict(ws=p['rows']), dict(ws=p['labels']), dict(ws=p['col']), dict(ws=p['counts']),
                 dict(ws=p['sizes'])):
        assert _labels_call(lib, dt, p, over) == EINVAL, over
    assert _labels_call(lib, dt, p, dict(ws=None)) == ENOMEM and _labels_call(lib, dt, p, dict(ws_bytes=need - 1)) == ENOMEM
    for k in ('rows', 'labels', 'offsets', 'out'):
        assert _gather_call(lib, dt, p, {k: None}) == EINVAL, k
    for over in (dict(M=0), dict(V=0), dict(R=-1), dict(ldr=49), dict(ldl=49), dict(ldo=49), dict(out=p['rows']),
                 dict(out=p['labels']), dict(out=p['out'] + 1), dict(rows=p['rows'] + 2), dict(offsets=p['offsets'] + 4),
                 dict(labels=p['labels'] + 2)):
        assert _gather_call(lib, dt, p, over) == EINVAL, over
    assert _gather_call(lib, dt, p, dict(R=0)) == 0 and _gather_call(lib, dt, p, dict(R=0, out=None)) == 0     # nothing to do
    assert all(np.all(bufs[k] == 0) for k in ('labels', 'counts', 'sizes', 'ws', 'out')) and np.all(bufs['rows'] == 1)
    if lib.modl_device_count() == 0:
        assert _labels_call(lib, dt, p) == ENOGPU and _gather_call(lib, dt, p) == ENOGPU
        assert _labels_call(lib, dt, p, dict(ws=None)) == ENOMEM                  # ENOMEM before ENOGPU
        assert _labels_call(lib, dt, p, dict(sizes=None, cap=0)) == ENOGPU        # the sizes are optional


# ---------------------------------------------------------------------------------------------------- the estimators
FIT_KW = dict(n_components=3, n_epochs=1, random_state=0, batch_size=8, alpha=0.1, reduction=2)
EXTRACT_KW = dict(min_region_size=6, threshold=1.0, thresholding_strategy='ratio_n_voxels')


def _check_extract_regions(fMRIDictFact, fMRICoder, dtype):
    from .test_compute_mask import _records
    vols = _records(dtype)
    mask = np.zeros(vols[0].shape[:3], bool)
    mask[1:9, 1:8, :7] = True
    mask[4, 4, 3] = False
    for grid, twin_grid in ((dict(voxel_size=(2, 1.5, 1)), dict(voxel_size=(2, 1.5, 1))),
                            (dict(mask_affine=np.diag([1.0, -2.0, 1.0, 1.0])), dict(mask_affine=np.diag([1.0, -2.0, 1.0, 1.0])))):
        est = fMRIDictFact(mask=mask, **grid, **FIT_KW).fit(vols)
        assert not hasattr(est, 'regions_')
        got = est.extract_regions(**EXTRACT_KW)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            ref = connected_regions_host(est.components_, mask, **EXTRACT_KW, **twin_grid)
        assert ref.regions.shape[0] >= 1
        assert all(same_bits(np.asarray(a), b) for a, b in zip(got, ref))
        assert same_bits(est.regions_, ref.regions) and same_bits(est.regions_index_, ref.index)
        assert est.regions_img_.shape == mask.shape + (ref.regions.shape[0],) and np.all(est.regions_img_[~mask] == 0)
        assert same_bits(est.regions_img_[mask].T, ref.regions)
        coder = fMRICoder(est.components_, mask=mask, **grid).fit()
        again = coder.extract_regions(**EXTRACT_KW)
        assert all(same_bits(np.asarray(a), b) for a, b in zip(again, ref)) and same_bits(coder.regions_img_, est.regions_img_)
        # the regions are a dictionary like any other: region signals
        signals = fMRICoder(est.regions_, mask=mask, **grid).fit().transform(vols[:1])
        assert np.asarray(signals[0]).shape == (vols[0].shape[3], ref.regions.shape[0])
    with pytest.warns(UserWarning, match='no region is left'):
        none = est.extract_regions(min_region_size=1e9)
    assert none.regions.shape == (0, int(mask.sum())) and est.regions_img_.shape == mask.shape + (0,)
    with pytest.raises(ValueError, match='not fitted'):
        fMRIDictFact(mask=mask, **FIT_KW).extract_regions()


def test_extract_regions_host_logic():
    from .test_masker import _host_estimators
    from .test_filter import _fmri_case
    est, coder = _host_estimators()
    _check_extract_regions(est, coder, np.float64)
    recs, confs, kw = _fmri_case(np.float64)
    flat = est(**kw).fit(recs)                                  # 2-D records, no mask: nothing to be connected in
    with pytest.raises(ValueError, match='without `mask`'):
        flat.extract_regions()
    assert not hasattr(flat, 'regions_')


def test_python_functions_equal_their_host_twins():
    """without a GPU the functions ARE their twins; with one this is the device against the judge"""
    for name, comp, mask, kw in cases(np.float64):
        _check_python(comp, mask, kw, name)


def _check_python(comp, mask, kw, name, cuda=False, **extra):
    ref = judge(comp, mask, **kw)
    kw = dict(kw)
    kw['thresholding_strategy'] = kw.pop('strategy', None)
    arg = comp
    if cuda:
        import torch
        arg = torch.from_numpy(comp).cuda()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        labels, counts = region_labels(arg, mask, **kw, **extra)
        reg = connected_regions(arg, mask, **kw, **extra)
    if cuda:
        assert all(t.is_cuda for t in (labels, counts) + tuple(reg))
        labels, counts, reg = labels.cpu().numpy(), counts.cpu().numpy(), Regions(*(t.cpu().numpy() for t in reg))
    assert same_result((labels, counts, reg), ref), name
    return labels, counts, reg


# ------------------------------------------------------------------------------------------------ layer 2: the GPU
def gpu_regions(comp, mask, cutoff, min_voxels, maps_per_pass=None):
    """modl_region_labels + modl_region_gather through the C-ABI on padded rows, every output between guard elements, the
    workspace poisoned and between guard bytes: (labels, counts, Regions)"""
    import torch
    from modl_amd._lib import lib, check
    from modl_amd.device import ptr
    sfx = 'f32' if comp.dtype == np.float32 else 'f64'
    tdt = torch.float32 if comp.dtype == np.float32 else torch.float64
    col = M._Maps(mask).col
    n0, n1, n2 = col.shape
    k, V = comp.shape
    ldr, ldl, ldo = V + 3, V + 5, V + 2
    rows = np.full((k, ldr), 7.0, comp.dtype)
    rows[:, :V] = comp
    d_rows, d_col = torch.from_numpy(rows).cuda(), torch.from_numpy(col).cuda()
    cap = V // (max(min_voxels, 0) + 1)
    labels, counts, sizes = _Guarded(k * ldl, torch.int32, -777), _Guarded(k, torch.int32, -777), _Guarded(k * cap, torch.int32, -777)
    Mp = maps_per_pass or k
    ws = _Workspace(lib.modl_region_labels_workspace(Mp, n0, n1, n2))
    item = comp.dtype.itemsize
    for a in range(0, k, Mp):
        b = min(a + Mp, k)
        check(getattr(lib, 'modl_region_labels_' + sfx)(
            C.c_void_p(d_rows.data_ptr() + a * ldr * item), ldr, b - a, V, ptr(d_col), n0, n1, n2, cutoff, min_voxels,
            C.c_void_p(labels.ptr.value + a * ldl * 4), ldl, C.c_void_p(counts.ptr.value + a * 4),
            C.c_void_p(sizes.ptr.value + a * cap * 4) if cap else None, cap, ws.ptr, ws.need, None), 'modl_region_labels')
    torch.cuda.synchronize()
    ws.check()
    lab = labels.get().reshape(k, ldl)
    assert np.all(lab[:, V:] == -777)                           # the padding of the rows is not written
    lab, cnt, siz = np.ascontiguousarray(lab[:, :V]), counts.get().astype(np.int64), sizes.get().reshape(k, cap)
    assert all(np.all(siz[m, cnt[m]:] == -777) for m in range(k))
    offsets = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    Rn = int(offsets[-1])
    out = _Guarded(Rn * ldo, tdt, -777.25)
    d_lab, d_off = torch.from_numpy(labels.get().reshape(k, ldl)).cuda(), torch.from_numpy(offsets).cuda()
    check(getattr(lib, 'modl_region_gather_' + sfx)(ptr(d_rows), ldr, k, V, ptr(d_lab), ldl, ptr(d_off), Rn, out.ptr, ldo, None),
          'modl_region_gather')
    torch.cuda.synchronize()
    assert same_bits(d_rows.cpu().numpy(), rows) and same_bits(d_col.cpu().numpy(), col)         # the inputs are untouched
    reg = out.get().reshape(Rn, ldo)
    assert np.all(reg[:, V:] == -777.25)
    return lab, cnt, Regions(np.ascontiguousarray(reg[:, :V]), np.repeat(np.arange(k, dtype=np.int64), cnt),
                             np.concatenate([siz[m, :cnt[m]] for m in range(k)]).astype(np.int64))


def structured_case(dt, box):
    """all ones, a serpentine through every tile and a U joined in the last plane under a full mask; kernel box (n0, n1, n2)"""
    vols = [np.ones(box, bool), serpentine(box), u_shape(box)]
    mask = np.ones(box[::-1], bool)
    comp = np.stack([np.where(v, 1.5 + 0.25 * i, 0.0).transpose(2, 1, 0)[mask] for i, v in enumerate(vols)])
    return np.ascontiguousarray(comp.astype(dt)), mask


def random_maps_case(dt, box, seed):
    """five maps under a mask of density 0.8: random at the foreground densities 0.2, 0.3116 and 0.6, one all zero, one more"""
    rs = np.random.RandomState(seed)
    mask = rs.rand(*box[::-1]) < 0.8
    mask.flat[0] = True
    V = int(mask.sum())
    comp = np.stack([rs.randn(V) * (rs.rand(V) < p) for p in (0.2, 0.3116, 0.0, 0.6, 0.45)])
    return np.ascontiguousarray(comp.astype(dt)), mask


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'f64'])
@pytest.mark.parametrize('box', boxes(), ids=lambda b: 'x'.join(map(str, b)))
def test_gpu_kernels_agree_with_scipy(gpu, box, dt):
    comp, mask = structured_case(DT[dt], box)
    for rows in (comp, comp[1:2]):                              # k = 3 and k = 1
        got = gpu_regions(rows, mask, 0.0, 0)
        ref = judge(rows, mask, min_region_size=0)
        assert same_result(got, ref), rows.shape
    assert ref[1].tolist() == [1] and ref[2].sizes[0] == serpentine(box).sum()       # the serpentine is ONE region
    comp, mask = random_maps_case(DT[dt], box, 7)               # k = 5
    for cutoff, min_voxels in ((0.0, 0), (0.4, 2)):
        got = gpu_regions(comp, mask, cutoff, min_voxels)
        ref = judge(comp, mask, min_region_size=min_voxels + 0.5, threshold=cutoff, strategy='value')
        assert same_result(got, ref), (cutoff, min_voxels)
        assert ref[1][2] == 0                                   # the all-zero map in between
    again = gpu_regions(comp, mask, 0.4, 2)
    assert same_result(again, got)                              # two runs, the same bits
    for per_pass in (1, 2):                                     # chunks of maps: the same bits as one pass
        assert same_result(gpu_regions(comp, mask, 0.4, 2, maps_per_pass=per_pass), got), per_pass


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_gpu_python_functions_agree_with_the_twins(gpu, dt):
    import torch
    for name, comp, mask, kw in cases(DT[dt]):
        _check_python(comp, mask, kw, name, cuda=True)
        _check_python(comp, mask, kw, name, cuda=False)         # numpy in, numpy out, through the device
    comp, mask = random_maps_case(DT[dt], (19, 23, 17), 11)
    kw = dict(min_region_size=2, threshold=1.0, strategy='ratio_n_voxels')
    one = _check_python(comp, mask, kw, 'one pass', cuda=True)
    for per_pass in (1, 2):
        assert same_result(_check_python(comp, mask, kw, per_pass, cuda=True, maps_per_pass=per_pass), one)
    ref = judge(comp, mask, **kw)
    k, V = comp.shape
    wide = torch.full((2 * k, V + 9), float('nan'), dtype=torch.from_numpy(comp).dtype, device='cuda')
    wide[::2, 4:V + 4] = torch.from_numpy(comp).cuda()
    tall = torch.from_numpy(np.ascontiguousarray(comp.T)).cuda().T                 # column-major
    for view in (wide[::2, 4:V + 4], tall):
        assert not view.is_contiguous()
        before = view.clone()
        reg = connected_regions(view, mask, min_region_size=2, threshold=1.0, thresholding_strategy='ratio_n_voxels')
        labels, counts = region_labels(view, mask, min_region_size=2, threshold=1.0, thresholding_strategy='ratio_n_voxels')
        got = (labels.cpu().numpy(), counts.cpu().numpy(), Regions(*(t.cpu().numpy() for t in reg)))
        assert same_result(got, ref) and torch.equal(view, before)
    with pytest.warns(UserWarning, match='no region is left'):
        empty = connected_regions(torch.from_numpy(comp).cuda(), mask, min_region_size=1e9)
    assert empty.regions.shape == (0, V) and empty.regions.is_cuda and empty.index.shape == (0,) and empty.sizes.shape == (0,)


@pytest.mark.gpu
def test_gpu_fmri_extract_regions(gpu):
    from modl_amd.fmri import fMRIDictFact, fMRICoder
    _check_extract_regions(fMRIDictFact, fMRICoder, np.float32)
