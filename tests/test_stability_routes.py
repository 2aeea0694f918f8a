"""The Amari discrepancy kernels route by route: modl_amari_{f32,f64} (modl_amd/csrc/stability.hip: amari_norm_kernel,
amari_pair_kernel - the only user of gemm_dense_tile<T, false, false, ..., BM, BM, 32> -, amari_combine_kernel,
amari_reduce_kernel and the host planner am_plan) and modl_amd.stability.amari_pairs.  The yardstick is the float64 numpy
restatement of tests/test_stability.py (`restate`); nothing of the code under test enters a reference or a bound.

ROUTES (`SHAPES`; `test_route_table` holds every case to `route`, a restatement of am_plan and of the branches the kernels
take, and every leaf of the restatement - a call of `_leaf`, read out of this file's own text - to at least one case;
`UNREACHED` lists, with the reason, the leaves that no shape can take.  The same table is in DESIGN.md, section 8.)
  plan      tiles per pair ceil(k_a / BM) x ceil(k_b / BM), BM = 128 (f32) / 64 (f64); fewer than 512 tiles: up to
            min(ceil(512 / tiles), p // 4096) splits, kps = ceil(ceil(p / ns) / 32) 32, nsplit = ceil(p / kps); the byte
            offsets of the seven workspace blocks; `test_plan_against_the_library` holds the total to modl_amari_workspace.
            The 256 MiB cap on the partial tiles cannot bind (`test_partial_cap_cannot_bind`, by enumeration).
  staging   16-byte vector loads for a tile row band that is full, a K tile that is full and an operand whose base and row
            stride are multiples of 16 bytes; element by element otherwise (unal / edge / K tail).
  epilogue  unsplit: scaled tile in LDS, row and column maxima of the mr x nc valid part; split: raw partial tiles, then the
            combine kernel in strips of 4 rows (ceil(mr / 4) strips of a tile row, the last of nr = mr - 4 (ns - 1) rows).
  reduce    maxima over the tile records; the column maxima walk ceil(mr / 4) strip records per tile row when split.
  norms     per lane an unrolled loop `e + 192 < p` (four features per turn) and a stride-64 tail; a binary search for the
            dictionary of an atom.

  f32 [129,130] p 61    unsplit, unal, 2 x 2 tiles, edges of width 1 and 2, K tail 29   (f64 [65,66] the same at BM 64)
  f32 [128,256] p 64    every tile interior, vector loads, no K tail; p 8192: the same, split in two
  both [5,7] p 1, 31, 64, 65, 192, 193, 255, 256, 257, 449: the norm kernel's loop boundaries, 1 .. 15 K tiles
  f64 [300,5] p 40      unsplit, k_a > 256 (a second turn of the reduce kernel's row loop), 5 tile rows
  f32 [5,7] p 8197      2 splits of 4128, the last 4069 (K tail 5), unal
  f32 [129,257] p 8196  split, aligned, 2 x 3 tiles, interior and all three kinds of edge, k_b > 256
  f64 [65,130] p 8195   split, unal, 2 x 3 tiles, mr = 1 (nr = 1 < 4, one strip against 16)
  f64 [300,5] p 8194    split, aligned, 5 tile rows, the last of mr = 44: 11 strips against 16
  f32 [3,130] p 12289   3 splits, the last 4033 (K tail 1), nr = 3
  f64 [66,3,65] p 8200  three ragged pairs in one split call: roff, coff, tile0
  f32 [1,1,2,1,130,1] p 61   15 pairs, the binary search over six dictionaries; 136 atoms, a multiple of 4 after all, hence
  f32 [2,1,1,130,1,2] p 61   137 atoms: three idle wavefronts in the norm kernel's last workgroup
  f64 [1,1,2,1,66,1] p 61    the six dictionaries at BM = 64
  GPU only: B (then A) one element into a larger buffer, f32 [129,257] p 8196 and [128,256] p 64: unal for one operand only.

SCENES (deterministic; `test_cases_are_what_they_claim` checks each claim on the CPU against the restatement)
  planted   an atom is noise of norm 0.1 (every entry at least 0.005 / sqrt(p) from zero); designated atoms carry spikes of 1 at
            a set of features.  Atoms of two dictionaries match (cosine >= 0.9) iff they carry the same set, at most one atom per
            dictionary and set, so the partner of a designated row sits at ONE chosen column and the reverse.  The sets partition
            `special_features`: 0, p - 1, the last multiple of 32 below p, kps - 1, kps, (nsplit - 1) kps, the first feature of the
            norm kernel's tail loop, the feature 256 t + 192 that lane 0 reads in an unrolled turn which only lanes 0 .. (p - 193
            - 256 t) take.  Dropping any one of them from the products or from the norms moves some maximum by over 100 bounds
            (asserted).  The designated atoms are `special_atoms`: k - 1 (index mr - 1 / nc - 1 of the edge tile, the last row of
            the last strip, a row of the last tile row), 0, and the first and last atom of every tile, in opposite order in odd
            dictionaries, so that k_a - 1 does not meet k_b - 1.
  negative  A = |noise|, B = -|noise|: every cosine, every maximum is below zero (asserted).  f32 [129,130] p 61 and f64
            [65,66] p 61 (unsplit), f32 [129,257] p 8196 and f64 [65,130] p 8195 (split), all with edge tiles.
  nan_tail  planted with a NaN at feature p - 1 (the last split's K tail) of row 1 of A: that row maximum, every column
            maximum and d are NaN, nothing else.
  zero_atom planted with atom k_a - 1 of A zero (index mr - 1 of the edge tile): the same pattern at that row.
  pinf      planted with +inf in row 2 of A at feature kps - 1 (or p / 2): inf / inf, the same pattern.
  ninf      planted with -inf in atom k_b - 1 of B at feature 0: that column maximum, every row maximum and d.
            The four on f32 [129,130] p 61, f64 [65,66] p 61 (unsplit) and f32 [129,257] p 8196, f64 [65,130] p 8195 (split).

JUDGE (`judge`): u = eps / 2 of the computing dtype, S_ij = sum_c |a_ic| |b_jc|, bound_ij = (p + 8) u S_ij / (|a_i| |b_j|):
any order of p products, the once-rounded norms, two divisions.  A row maximum may differ by max_j bound_ij (max is
1-Lipschitz), a column maximum by max_i bound_ij, d by half the sum of the two means of those bounds plus 8 * 2^-53.  NaN
positions must match exactly.  The device also gets its workspace filled with 0xFF bytes (every unwritten float reads as
NaN), its outputs filled with a sentinel and followed by guard elements, and its launch count held to the restatement.

MUTANTS (`test_judge_rejects_mutants`, both dtypes: `restate_call(..., mut)`; the judge rejects each on EVERY case named
here - `mutant_cases` - and accepts the restatement rounded to the computing dtype on every case).  The device test
`test_abi_against_restatement` of the same case would fail in the same way if a kernel made the mistake; four of them were
also planted in the kernels themselves (variant libraries, MODL_HIP_LIBRARY): `T m = 0` in amari_pair_kernel failed the unsplit
`negative` cases, `ns = BM / kStripRows` in amari_reduce_kernel every split case, an amax that drops NaN all sixteen
non-finite cases, `c < nc - 1` in the row maxima of an edge tile every planted case with k_b mod BM != 0 and p > 1.
  max_from_0      the maximum started at 0                              every `negative` case
  fmax            np.fmax for the NaN-propagating maximum                every nan_tail, zero_atom, pinf and ninf case
  abs             the absolute value taken                              every `negative` case
  drop_last       the last feature dropped from the products            every planted case (spike at p - 1)
  drop_ktail      the K tail p mod 32 dropped                           every planted case with p mod 32 != 0 (spike at the last
                                                                        multiple of 32 below p)
  drop_split      the last split dropped                                every split planted case (spikes at (nsplit - 1) kps, p - 1)
  first_twice     the first feature of a later split counted twice      every split planted case (spike at kps)
  norm_no_tail    the norm without its tail-loop features               every planted case whose p has a tail turn (spike at its first
                                                                        feature): all but p = 256 and p = 8192
  skip_edge_col   column k_b - 1 of an edge tile left out of the rows'  every planted case with k_b mod BM != 0, p > 1: the partner of
                  maxima                                                designated row is column k_b - 1
  skip_edge_row   row k_a - 1 of an edge tile left out of the columns'  every planted case with k_a mod BM != 0, p > 1: the partner of
                  maxima                                                designated column is row k_a - 1
  skip_strip      the last strip of a tile left out of the column       every split planted case (partner rows k_a - 1 and BM - 1)
                  maxima
  strips_full     the last tile row's strips counted as full            split planted cases with ceil(mr / 4) < BM / 4: the records
                                                                        read are never written, NaN under the 0xFF fill
  padding_zeros   the padding of an edge tile read as zeros             every `negative` case (all have edge tiles both ways)
  mean_other_k    the means divided by the other dictionary's k         every planted case with k_a != k_b
  b_outer         b as the outer loop of the pair order                 the three six-dictionary cases (the orders agree up to n = 3)
  roff_by_kb      the row offsets advanced by k_b                       f64 [66,3,65] p 8200 and the three six-dictionary cases

MEASURED (largest |got - ref| / bound over every case on the MI355X, from this file's own run - `test_report` prints it;
recorded, not asserted): f32 0.124, f64 0.125.  65 GPU cases in 5 s, none above 0.3 s.
"""
import ctypes as C
import functools
import re
import zlib
from types import SimpleNamespace

import numpy as np
import pytest

from .test_stability import restate

DT = {'f32': np.float32, 'f64': np.float64}
ES = {'f32': 4, 'f64': 8}
BMS = {'f32': 128, 'f64': 64}                  # AmCfg<T>::BM
BK = 32                                        # AmCfg<T>::BK
STRIP = 4                                      # kStripRows
TARGET = 512                                   # kTargetItems
MIN_SPLIT = 4096                               # kMinSplitK
CAP = 256 << 20                                # kMaxPartialBytes
SIZEOF_DICT, SIZEOF_PAIR, SIZEOF_TILE = 32, 40, 16   # AmDict (ptr + 3 int64), AmPair (4 int + 3 int64), AmTile (4 int)
SENT = 7.5                                     # fills the outputs before a call: no cosine, no discrepancy is 7.5
GUARD = 8                                      # elements behind each output


def cdiv(a, b):
    return -(-a // b)


def align_up(x, a):
    return cdiv(x, a) * a


HIT = set()


def _leaf(name):
    """Marks a branch of the restatement; `all_leaves` reads the names out of this file's own text."""
    HIT.add(name)
    return name


def all_leaves():
    with open(__file__.replace('.pyc', '.py')) as f:
        return set(re.findall(r"_leaf\('([^']+)'\)", f.read()))


UNREACHED = {
    'plan/cap_binds': 'fewer than 512 tiles take at most ceil(512 / tiles) splits: under 1 023 tile-splits of 64 KiB (f32) or '
                      '32 KiB (f64), 64 MiB against the 256 MiB cap (test_partial_cap_cannot_bind)',
}


# ------------------------------------------------------------------------------------------------ the host plan, restated
def split_want(ntiles, p):
    return min(cdiv(TARGET, ntiles), p // MIN_SPLIT)


def split_cap(dt, ntiles):
    return CAP // (ntiles * BMS[dt] * BMS[dt] * ES[dt])


def am_plan(dt, ks, p):
    """am_plan of stability.hip, line by line"""
    bm, es, n = BMS[dt], ES[dt], len(ks)
    pairs, ntiles, roff, coff = [], 0, 0, 0
    for a in range(n - 1):
        for b in range(a + 1, n):
            tr, tc = cdiv(ks[a], bm), cdiv(ks[b], bm)
            pairs.append(SimpleNamespace(a=a, b=b, ka=ks[a], kb=ks[b], tr=tr, tc=tc, tile0=ntiles, roff=roff, coff=coff))
            ntiles += tr * tc
            roff += ks[a]
            coff += ks[b]
    ns, cap_binds = 1, False
    if ntiles < TARGET:
        ns = split_want(ntiles, p)
        cap_binds = split_cap(dt, ntiles) < ns
        ns = max(min(ns, split_cap(dt, ntiles)), 1)
    kps = cdiv(cdiv(p, ns), BK) * BK
    nsplit = cdiv(p, kps)
    nstrip = bm // STRIP if nsplit > 1 else 1
    off = align_up(SIZEOF_DICT * n, 256)
    off_pairs, off = off, align_up(off + SIZEOF_PAIR * len(pairs), 256)
    off_tiles, off = off, align_up(off + SIZEOF_TILE * ntiles, 256)
    off_norms, off = off, align_up(off + es * sum(ks), 256)
    off_row, off = off, align_up(off + es * ntiles * bm, 256)
    off_col, off = off, align_up(off + es * ntiles * nstrip * bm, 256)
    off_part = off
    if nsplit > 1:
        off = align_up(off + es * ntiles * nsplit * bm * bm, 256)
    return SimpleNamespace(dt=dt, bm=bm, n=n, ks=list(ks), p=p, pairs=pairs, npairs=len(pairs), ntiles=ntiles, sum_k=sum(ks),
                           nsplit=nsplit, kps=kps, nstrip=nstrip, cap_binds=cap_binds, last=p - (nsplit - 1) * kps,
                           launches=4 if nsplit > 1 else 3, off_pairs=off_pairs, off_tiles=off_tiles, off_norms=off_norms,
                           off_row=off_row, off_col=off_col, off_part=off_part, bytes=off)


@functools.lru_cache(maxsize=None)
def norm_lanes(p):
    """amari_norm_kernel per lane: (features of the unrolled loop, features of the tail loop, unrolled turns)"""
    out = []
    for lane in range(64):
        e, un, tl, turns = lane, [], [], 0
        while e + 192 < p:
            un += [e, e + 64, e + 128, e + 192]
            e += 256
            turns += 1
        while e < p:
            tl.append(e)
            e += 64
        out.append((un, tl, turns))
    return out


def tail_features(p):
    return sorted(f for _, tl, _ in norm_lanes(p) for f in tl)


def partial_turn_feature(p):
    """256 t + 192, read by lane 0 in an unrolled turn t that only some lanes take; None where every turn is taken by all"""
    lanes = norm_lanes(p)
    for t in range(max(x[2] for x in lanes)):
        if sum(1 for x in lanes if x[2] > t) < 64:
            return 256 * t + 192
    return None


def route(dt, ks, p, mis=()):
    """The route of one call: the plan and every branch the four kernels take, as a string and the launch count.  `mis`: the
    dictionaries whose base pointer is not a multiple of 16 bytes."""
    pl = am_plan(dt, ks, p)
    bm, es = pl.bm, ES[dt]
    s = (_leaf('f32/BM128') if dt == 'f32' else _leaf('f64/BM64')) + '/'
    s += (_leaf('plan/cap_binds') if pl.cap_binds else _leaf('plan/cap_slack')) + '/'
    if pl.nsplit == 1:
        s += _leaf('unsplit') + '/K%d/' % p
    else:
        s += _leaf('split') + '%d/kps%d/last%d/' % (pl.nsplit, pl.kps, pl.last)
        s += (_leaf('split/last_shorter_ragged') if (pl.kps - pl.last) % BK else _leaf('split/last_shorter_by_tiles')) + '/'
    s += (_leaf('k/tail') if pl.last % BK else _leaf('k/full')) + '%d/' % (pl.last % BK)
    s += (_leaf('k/one_tile') if cdiv(min(p, pl.kps), BK) == 1 else _leaf('k/pipelined')) + '%d/' % cdiv(min(p, pl.kps), BK)
    unal = [(p * es) % 16 != 0 or d in mis for d in range(pl.n)]                       # amari_run
    s += 'unal' + ''.join('01'[u] for u in unal) + '/'
    for q in pl.pairs:
        ua, ub = unal[q.a], unal[q.b]
        if ua and ub:
            _leaf('unal/both')
        elif ua or ub:
            _leaf('unal/one_operand')
        else:
            _leaf('unal/neither')
        kinds = []
        for ti in range(q.tr):
            mr = min(bm, q.ka - ti * bm)
            for tj in range(q.tc):
                nc = min(bm, q.kb - tj * bm)
                if mr == bm and nc == bm:
                    kinds.append(_leaf('tile/interior'))
                elif nc == bm:
                    kinds.append(_leaf('tile/edge_rows'))
                elif mr == bm:
                    kinds.append(_leaf('tile/edge_cols'))
                else:
                    kinds.append(_leaf('tile/edge_both'))
                for u, full in ((ua, mr == bm), (ub, nc == bm)):                       # TileLoader::load, per operand
                    if u:
                        _leaf('stage/guarded:unal')
                    elif not full:
                        _leaf('stage/guarded:edge')
                    else:
                        if pl.last >= BK or pl.nsplit > 1:
                            _leaf('stage/vector')
                        if pl.last % BK:
                            _leaf('stage/guarded:ktail')
        mr, nc = q.ka - (q.tr - 1) * bm, q.kb - (q.tc - 1) * bm
        s += 'pair%d-%d:%dx%d[%s]mr%d,nc%d,' % (q.a, q.b, q.tr, q.tc, ''.join({'interior': 'i', 'edge_rows': 'r', 'edge_cols': 'c', 'edge_both': 'b'}[x[5:]] for x in kinds), mr, nc)
        s += (_leaf('edge/mr%4!=0') if mr % STRIP else _leaf('edge/mr%4=0')) + '%d/' % (mr % STRIP)
        if pl.nsplit > 1:
            if mr % STRIP:
                _leaf('combine/nr<4')
            s += (_leaf('combine/last_tile_row_short') if cdiv(mr, STRIP) < bm // STRIP else _leaf('combine/last_tile_row_full'))
            s += '%d/' % cdiv(mr, STRIP)
        if q.ka > 256:
            _leaf('reduce/ka>256')
        if q.kb > 256:
            _leaf('reduce/kb>256')
        if q.ka <= 256 and q.kb <= 256:
            _leaf('reduce/k<=256')
        s += 'ka%s256,kb%s256/' % ('>' if q.ka > 256 else '<=', '>' if q.kb > 256 else '<=')
    s += (_leaf('pairs/one') if pl.npairs == 1 else _leaf('pairs/many')) + '/'
    s += (_leaf('norm/search_n=2') if pl.n == 2 else _leaf('norm/search_n>2')) + '/'
    s += (_leaf('norm/atoms%4=0') if pl.sum_k % 4 == 0 else _leaf('norm/atoms%4!=0')) + '/'
    kinds = set()
    for un, tl, turns in norm_lanes(p):
        if turns > 1:
            _leaf('norm/unrolled_twice')
        if un and tl:
            kinds.add(_leaf('norm/lane:both'))
        elif un:
            kinds.add(_leaf('norm/lane:unrolled_only'))
        elif tl:
            kinds.add(_leaf('norm/lane:tail_only'))
        else:
            kinds.add(_leaf('norm/lane:idle'))
    if len(kinds) > 1:
        _leaf('norm/lanes_differ')
    s += '+'.join(sorted(kinds)) + '/'
    s += _leaf('launches/4') if pl.launches == 4 else _leaf('launches/3')
    return SimpleNamespace(s=s, plan=pl, launches=pl.launches, unal=unal)


# ----------------------------------------------------------------------------------------------------------- the cases
NORM_P = (1, 31, 64, 65, 192, 193, 255, 256, 257, 449)
SHAPES = [
    ('f32', (129, 130), 61),
    ('f64', (65, 66), 61),
    ('f32', (128, 256), 64),
    ('f32', (128, 256), 8192),
] + [(dt, (5, 7), p) for dt in ('f32', 'f64') for p in NORM_P] + [
    ('f64', (300, 5), 40),
    ('f32', (5, 7), 8197),
    ('f32', (129, 257), 8196),
    ('f64', (65, 130), 8195),
    ('f64', (300, 5), 8194),
    ('f32', (3, 130), 12289),
    ('f64', (66, 3, 65), 8200),
    ('f32', (1, 1, 2, 1, 130, 1), 61),
    ('f32', (2, 1, 1, 130, 1, 2), 61),
    ('f64', (1, 1, 2, 1, 66, 1), 61),
]
EDGE_SHAPES = [('f32', (129, 130), 61), ('f64', (65, 66), 61), ('f32', (129, 257), 8196), ('f64', (65, 130), 8195)]
NONFINITE = ('nan_tail', 'zero_atom', 'pinf', 'ninf')
CASES = [sh + ('planted',) for sh in SHAPES] + [sh + ('negative',) for sh in EDGE_SHAPES] + \
        [sh + (scene,) for sh in EDGE_SHAPES for scene in NONFINITE]


def case_id(case):
    dt, ks, p, scene = case
    return '%s-%s-p%d-%s' % (dt, 'x'.join(str(k) for k in ks), p, scene)


def special_atoms(k, bm, fill=True):
    out = [k - 1, 0]
    for t in range(cdiv(k, bm)):
        out += [min(t * bm + bm - 1, k - 1), t * bm]
    if fill:
        out += [k // 2] + list(range(k))                                              # fillers, should a short list need them
    return list(dict.fromkeys(out))


def special_features(dt, ks, p):
    pl = am_plan(dt, ks, p)
    f = [0, p - 1, (p - 1) // BK * BK, pl.kps - 1, pl.kps, (pl.nsplit - 1) * pl.kps]
    tl = tail_features(p)
    if tl:
        f.append(tl[0])
    if partial_turn_feature(p) is not None:
        f.append(partial_turn_feature(p))
    return list(dict.fromkeys(x for x in f if 0 <= x < p))


def _noise(rs, k, p):
    z = rs.randn(k, p)
    return np.where(z < 0, -1.0, 1.0) * (np.abs(z) + 0.05) * (0.1 / np.sqrt(p))


def planted(dt, ks, p, seed):
    """-> (dictionaries, {dictionary: {match: atom}}, the feature set of every match)"""
    rs = np.random.RandomState(seed)
    bm = BMS[dt]
    # matches: as many as the longest list of designated atoms, as the second largest dictionary and as the features allow
    L = min(max(len(special_atoms(k, bm, fill=False)) for k in ks), sorted(ks)[-2], p)
    feats = special_features(dt, ks, p)
    extra = [int(x) for x in rs.permutation(p) if int(x) not in set(feats)]
    feats = feats + extra[:max(0, L - len(feats))]
    sets = [feats[m::L] for m in range(L)]
    dicts, where = [], {}
    for d, k in enumerate(ks):
        D = _noise(rs, k, p)
        order = special_atoms(k, bm)[:min(k, L)]
        if d % 2:
            order = order[::-1]
        where[d] = {m: i for m, i in enumerate(order)}
        for m, i in where[d].items():
            D[i, sets[m]] = 1.0
        dicts.append(np.ascontiguousarray(D.astype(DT[dt])))
    return dicts, where, sets


@functools.lru_cache(maxsize=None)
def build(case):
    """-> namespace: D (the dictionaries, in the computing dtype), claims (what the scene plants)"""
    dt, ks, p, scene = case
    seed = zlib.crc32(case_id(case).encode())
    pl = am_plan(dt, ks, p)
    if scene == 'negative':
        rs = np.random.RandomState(seed)
        D = [np.ascontiguousarray(((-1) ** d * np.abs(_noise(rs, k, p))).astype(DT[dt])) for d, k in enumerate(ks)]
        return SimpleNamespace(D=D, matches=[], sets=[], nan_row=None, nan_col=None)
    D, where, sets = planted(dt, ks, p, seed)
    matches = [(q, where[pr.a][m], where[pr.b][m]) for q, pr in enumerate(pl.pairs) for m in range(len(sets))
               if m in where[pr.a] and m in where[pr.b]]
    c = SimpleNamespace(D=D, matches=matches, sets=sets, nan_row=None, nan_col=None)
    if scene == 'nan_tail':
        D[0][1, p - 1] = np.nan
        c.nan_row = 1
    elif scene == 'zero_atom':
        D[0][ks[0] - 1] = 0
        c.nan_row = ks[0] - 1
    elif scene == 'pinf':
        D[0][2, pl.kps - 1 if pl.kps - 1 < p else p // 2] = np.inf
        c.nan_row = 2
    elif scene == 'ninf':
        D[1][ks[1] - 1, 0] = -np.inf
        c.nan_col = ks[1] - 1
    return c


# ----------------------------------------------------------------------------------------------- reference, bound, judge
def bounds(A, B, dt):
    """(row bounds, column bounds, bound on d) of the pair, from the inputs alone"""
    A, B = np.abs(np.asarray(A, np.float64)), np.abs(np.asarray(B, np.float64))
    u = float(np.finfo(DT[dt]).eps) / 2
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        bnd = (A.shape[1] + 8) * u * A.dot(B.T) / np.sqrt(np.sum(A ** 2, axis=1))[:, None] / np.sqrt(np.sum(B ** 2, axis=1))[None, :]
        brow, bcol = bnd.max(axis=1), bnd.max(axis=0)
        return brow, bcol, .5 * (np.mean(brow) + np.mean(bcol)) + 8 * 2.0 ** -53


def reference_of(D, dt):
    """the f64 restatement and the bounds of every pair of a call, a outer"""
    out = []
    for a in range(len(D) - 1):
        for b in range(a + 1, len(D)):
            rm, cm, d = restate(D[a], D[b])
            brow, bcol, bd = bounds(D[a], D[b], dt)
            out.append(SimpleNamespace(a=a, b=b, rm=rm, cm=cm, d=d, brow=brow, bcol=bcol, bd=bd))
    return out


@functools.lru_cache(maxsize=None)
def reference(case):
    return reference_of(build(case).D, case[0])


def _judge_vec(got, ref, bnd, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if got.shape != ref.shape:
        return 0.0, '%s: shape %s for %s' % (what, got.shape, ref.shape)
    if not np.array_equal(np.isnan(got), np.isnan(ref)):
        x = np.flatnonzero(np.isnan(got) != np.isnan(ref))
        return 0.0, '%s: NaN at other places, first [%d] got %r ref %r' % (what, x[0], got[x[0]], ref[x[0]])
    ok = ~np.isnan(ref)
    if not np.all(np.isfinite(bnd[ok])):
        return 0.0, '%s: no finite bound where the reference is finite' % what
    if not ok.any():
        return 0.0, None
    with np.errstate(invalid='ignore'):
        ratio = np.abs(got[ok] - ref[ok]) / bnd[ok]
    ratio = np.where(np.isnan(ratio), np.inf, ratio)                                  # an infinity where a number belongs
    w = int(np.argmax(ratio))
    if ratio[w] > 1:
        i = np.flatnonzero(ok)[w]
        return float(ratio[w]), '%s[%d]: got %r ref %r, %.3g bounds' % (what, i, got[i], ref[i], ratio[w])
    return float(ratio[w]), None


def judge(ref, got):
    """-> (largest error / bound, None or the first complaint).  got: {'rowmax': [...], 'colmax': [...], 'd': array}"""
    worst, why = 0.0, None
    if not (len(got['rowmax']) == len(got['colmax']) == len(got['d']) == len(ref)):
        return 0.0, 'pair count'
    for q, r in enumerate(ref):
        for w, y in (_judge_vec(got['rowmax'][q], r.rm, r.brow, 'rowmax pair %d' % q),
                     _judge_vec(got['colmax'][q], r.cm, r.bcol, 'colmax pair %d' % q),
                     _judge_vec([got['d'][q]], [r.d], np.array([r.bd]), 'd pair %d' % q)):
            worst = max(worst, w)
            why = why or y
    return worst, why


# ------------------------------------------------------------------------------------ the restatement of a call, and mutants
MUTANTS = ('max_from_0', 'fmax', 'abs', 'drop_last', 'drop_ktail', 'drop_split', 'first_twice', 'norm_no_tail', 'skip_edge_col',
           'skip_edge_row', 'skip_strip', 'strips_full', 'padding_zeros', 'mean_other_k', 'b_outer', 'roff_by_kb')


def _pair_restated(A, B, pl, mut):
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    ka, kb, p, bm = A.shape[0], B.shape[0], A.shape[1], pl.bm
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        keep = p
        if mut == 'drop_last':
            keep = p - 1
        elif mut == 'drop_ktail':
            keep = p - p % BK
        elif mut == 'drop_split':
            keep = (pl.nsplit - 1) * pl.kps
        G = A.dot(B.T) if keep == p else A[:, :keep].dot(B[:, :keep].T)
        if mut == 'first_twice':
            for s in range(1, pl.nsplit):
                G = G + np.outer(A[:, s * pl.kps], B[:, s * pl.kps])
        nf = np.ones(p, bool)
        if mut == 'norm_no_tail':
            nf[tail_features(p)] = False
        An, Bn = (A, B) if nf.all() else (A[:, nf], B[:, nf])
        na, nb = np.sqrt(np.sum(An ** 2, axis=1)), np.sqrt(np.sum(Bn ** 2, axis=1))
        Cs = G / na[:, None] / nb[None, :]
        if mut == 'abs':
            Cs = np.abs(Cs)
        red = np.fmax.reduce if mut == 'fmax' else np.maximum.reduce
        ninf = -np.inf
        Cr, Cc = Cs, Cs
        if mut == 'skip_edge_col' and kb % bm:
            Cr = Cs[:, :kb - 1]
        if mut == 'skip_edge_row' and ka % bm:
            Cc = Cs[:ka - 1]
        if mut == 'skip_strip' and pl.nsplit > 1:
            r = np.arange(ka)
            mr = np.minimum(bm, ka - r // bm * bm)
            Cc = Cs[(r % bm) // STRIP != (mr - 1) // STRIP]
        rmax = red(Cr, axis=1, initial=ninf)
        cmax = red(Cc, axis=0, initial=ninf)
        if mut == 'strips_full' and pl.nsplit > 1 and cdiv(ka - (cdiv(ka, bm) - 1) * bm, STRIP) < bm // STRIP:
            cmax = np.full(kb, np.nan)                 # records that no workgroup writes: NaN under the 0xFF fill of the workspace
        if mut == 'max_from_0' or (mut == 'padding_zeros' and kb % bm):
            rmax = np.maximum(rmax, 0)
        if mut == 'max_from_0' or (mut == 'padding_zeros' and ka % bm):
            cmax = np.maximum(cmax, 0)
        if mut == 'mean_other_k':
            d = .5 * (np.sum(1 - cmax) / ka + np.sum(1 - rmax) / kb)
        else:
            d = .5 * (np.mean(1 - cmax) + np.mean(1 - rmax))
    return rmax, cmax, d


def restate_call(D, dt, mut=None):
    """One call, restated in f64 at the level of its outputs (flat row and column buffers, one d per pair), rounded to the computing
    dtype; `mut` plants one mistake."""
    ks, p = [x.shape[0] for x in D], D[0].shape[1]
    pl = am_plan(dt, ks, p)
    order = [(q.a, q.b) for q in pl.pairs]
    if mut == 'b_outer':
        order = [(a, b) for b in range(1, pl.n) for a in range(b)]
    res = [_pair_restated(D[a], D[b], pl, mut) for a, b in order]
    n_row, n_col = sum(q.ka for q in pl.pairs), sum(q.kb for q in pl.pairs)
    row, col = np.full(n_row, SENT), np.full(n_col, SENT)
    ro = co = 0
    for (a, b), (rm, cm, _) in zip(order, res):
        m = max(0, min(len(rm), n_row - ro))
        row[ro:ro + m] = rm[:m]
        col[co:co + len(cm)] = cm[:n_col - co]
        ro += ks[b] if mut == 'roff_by_kb' else ks[a]
        co += ks[b]
    with np.errstate(over='ignore', invalid='ignore'):
        row, col = row.astype(DT[dt]), col.astype(DT[dt])
    return {'rowmax': [row[q.roff:q.roff + q.ka] for q in pl.pairs], 'colmax': [col[q.coff:q.coff + q.kb] for q in pl.pairs],
            'd': np.array([r[2] for r in res])}


def mutant_cases(mut):
    """the cases on which the judge must reject `mut`"""
    out = []
    for case in CASES:
        dt, ks, p, scene = case
        pl, bm = am_plan(dt, ks, p), BMS[dt]
        split = pl.nsplit > 1
        if mut in ('max_from_0', 'abs', 'padding_zeros'):
            ok = scene == 'negative'
        elif mut == 'fmax':
            ok = scene in NONFINITE
        elif scene != 'planted':
            ok = False
        elif mut == 'drop_last':
            ok = True
        elif mut == 'drop_ktail':
            ok = p % BK != 0
        elif mut in ('drop_split', 'first_twice', 'skip_strip'):
            ok = split
        elif mut == 'norm_no_tail':
            ok = bool(tail_features(p))
        elif mut == 'skip_edge_col':                                               # (p = 1: every cosine is 1 or -1)
            ok = p > 1 and any(q.kb % bm for q in pl.pairs)
        elif mut == 'skip_edge_row':
            ok = p > 1 and any(q.ka % bm for q in pl.pairs)
        elif mut == 'strips_full':
            ok = split and any(cdiv(q.ka - (q.tr - 1) * bm, STRIP) < bm // STRIP for q in pl.pairs)
        elif mut == 'mean_other_k':
            ok = p > 1 and any(q.ka != q.kb for q in pl.pairs)
        elif mut == 'b_outer':
            ok = pl.n >= 4
        elif mut == 'roff_by_kb':
            ok = pl.n >= 3
        if ok:
            out.append(case)
    return out


# ------------------------------------------------------------------------------------------------------------- CPU tests
@pytest.fixture(scope='module')
def lib():
    from modl_amd import _lib
    return _lib.lib


def _ws_bytes(lib, dt, ks, p):
    from modl_amd._lib import MODL_F32, MODL_F64
    k = np.array(ks, dtype=np.int64)
    return lib.modl_amari_workspace(MODL_F32 if dt == 'f32' else MODL_F64, len(ks), k.ctypes.data_as(C.c_void_p), p)


EXTRA_SHAPES = [('f64', (65, 3, 66), 8195), ('f32', (1024, 1024, 1024), 50000), ('f32', (70, 70), 200000),
                ('f64', (1500, 129), 3), ('f32', (2000, 3000), 100000), ('f64', (4000, 1), 9000)]


def test_plan_against_the_library(lib):
    for dt, ks, p in [c[:3] for c in CASES] + EXTRA_SHAPES:
        assert am_plan(dt, ks, p).bytes == _ws_bytes(lib, dt, ks, p), (dt, ks, p)
    pl = am_plan('f32', (70, 70), 200000)                       # "split 48 ways"
    assert (pl.nsplit, pl.launches) == (48, 4)
    pl = am_plan('f32', (1024,) * 3, 50000)                     # test_three_large_dictionaries_f32: 192 tiles
    assert (pl.ntiles, pl.launches) == (192, 4)


def test_partial_cap_cannot_bind():
    """The 256 MiB cap of am_plan never lowers the split count: with t < 512 tiles the split count is at most ceil(512 / t), and
    floor(256 MiB / (t BM BM sizeof T)) = floor(4096 / t) (f32) or floor(8192 / t) (f64) is never below that."""
    for dt in ('f32', 'f64'):
        most = 0
        for t in range(1, TARGET):
            assert split_cap(dt, t) >= cdiv(TARGET, t), (dt, t)
            most = max(most, t * cdiv(TARGET, t) * BMS[dt] * BMS[dt] * ES[dt])
        assert most <= 1023 * (64 << 10) and most < CAP
    # with 512 tiles or more there is no split, hence no partial tile at all
    assert am_plan('f32', (3000, 3000), 100000).nsplit == 1
    assert not any(am_plan(*c[:3]).cap_binds for c in CASES)


ROUTES = {     # the route strings of the shapes of the issue's table, written out by hand from its "reaches" column
    ('f32', (129, 130), 61): ('unsplit/K61', 'k/tail29', 'unal11', '2x2[icrb]mr1,nc2', 'launches/3'),
    ('f64', (65, 66), 61): ('f64/BM64', 'unsplit/K61', 'k/tail29', 'unal11', '2x2[icrb]mr1,nc2', 'launches/3'),
    ('f32', (128, 256), 64): ('unsplit/K64', 'k/full0', 'unal00', '1x2[ii]mr128,nc128', 'launches/3'),
    ('f64', (300, 5), 40): ('unsplit/K40', 'k/tail8', 'unal00', '5x1[ccccb]mr44,nc5', 'ka>256,kb<=256'),
    ('f32', (5, 7), 8197): ('split2/kps4128/last4069', 'k/tail5', 'unal11', '1x1[b]mr5,nc7', 'launches/4'),
    ('f32', (129, 257), 8196): ('split2/kps4128/last4068', 'unal00', '2x3[iicrrb]mr1,nc1', 'ka<=256,kb>256'),
    ('f64', (65, 130), 8195): ('split2/kps4128/last4067', 'unal11', '2x3[iicrrb]mr1,nc2', 'combine/last_tile_row_short1/'),
    ('f64', (300, 5), 8194): ('split2/kps4128/last4066', 'unal00', '5x1[ccccb]mr44,nc5', 'combine/last_tile_row_short11/'),
    ('f32', (3, 130), 12289): ('split3/kps4128/last4033', 'k/tail1', 'unal11', '1x2[rb]mr3,nc2', 'edge/mr%4!=03/'),
    ('f64', (66, 3, 65), 8200): ('split2/kps4128/last4072', 'unal000', 'pair0-1:2x1', 'pair0-2:2x2', 'pair1-2:1x2', 'pairs/many'),
    ('f32', (1, 1, 2, 1, 130, 1), 61): ('unsplit/K61', 'unal111111', 'pair4-5:2x1', 'norm/search_n>2', 'norm/atoms%4=0'),
    ('f32', (2, 1, 1, 130, 1, 2), 61): ('pair3-5:2x1', 'norm/search_n>2', 'norm/atoms%4!=0'),
}


def test_route_table():
    HIT.clear()
    for case in CASES:
        r = route(*case[:3])
        assert r.launches == (4 if r.plan.nsplit > 1 else 3)
        for part in ROUTES.get(case[:3], ()):
            assert part in r.s, (case, part, r.s)
    # the GPU-only points: one operand one element into a larger buffer
    for ks, p in (((129, 257), 8196), ((128, 256), 64)):
        for mis in ((0,), (1,)):
            r = route('f32', ks, p, mis=mis)
            assert r.unal == [d in mis for d in range(2)]
    assert am_plan('f32', (5, 7), 8197).last == 4069 and am_plan('f32', (3, 130), 12289).last == 4033
    for p, kinds in ((1, {'idle', 'tail_only'}), (192, {'tail_only'}), (193, {'unrolled_only', 'tail_only'}),
                     (255, {'unrolled_only', 'tail_only'}), (256, {'unrolled_only'}), (257, {'both', 'unrolled_only'})):
        got = set()
        for lane, (un, tl, _) in enumerate(norm_lanes(p)):
            got.add('both' if un and tl else 'unrolled_only' if un else 'tail_only' if tl else 'idle')
            assert sorted(un + tl) == list(range(lane, p, 64))                         # every feature of the lane, once
        assert got == kinds, (p, got)
    assert partial_turn_feature(255) == 192 and partial_turn_feature(449) == 448 and partial_turn_feature(256) is None
    missing = all_leaves() - HIT - set(UNREACHED)
    assert not missing, sorted(missing)
    assert not HIT & set(UNREACHED), sorted(HIT & set(UNREACHED))
    assert set(UNREACHED) <= all_leaves()


def _moved(x, y):
    with np.errstate(invalid='ignore'):
        d = np.abs(np.asarray(x, np.float64) - np.asarray(y, np.float64))
    return np.where(np.isnan(d), np.inf, d)


@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_cases_are_what_they_claim(case):
    dt, ks, p, scene = case
    c, ref, pl = build(case), reference(case), am_plan(dt, ks, p)
    assert [x.shape for x in c.D] == [(k, p) for k in ks] and all(x.dtype == DT[dt] and x.flags.c_contiguous for x in c.D)
    if scene == 'negative':
        for r in ref:
            assert np.all(r.rm < 0) and np.all(r.cm < 0) and r.d > 1
        return
    # the matches: the partner of row i is column j and nobody else, by a wide margin, and the reverse
    assert c.matches
    for q, i, j in c.matches:
        pr = pl.pairs[q]
        A, B = c.D[pr.a].astype(np.float64), c.D[pr.b].astype(np.float64)
        with np.errstate(invalid='ignore', divide='ignore'):
            row = A[i].dot(B.T) / np.linalg.norm(A[i]) / np.linalg.norm(B, axis=1)
            col = A.dot(B[j]) / np.linalg.norm(A, axis=1) / np.linalg.norm(B[j])
        if scene == 'planted':
            assert row[j] >= 0.9 and col[i] >= 0.9
            assert p == 1 or (np.argmax(row) == j and np.argmax(col) == i)         # (p = 1: every cosine is 1 or -1)
            if pr.kb > 1 and p > 1:
                assert row[j] - np.sort(row)[-2] >= max(0.3, 100 * ref[q].brow[i]), (q, i, j)
            if pr.ka > 1 and p > 1:
                assert col[i] - np.sort(col)[-2] >= max(0.3, 100 * ref[q].bcol[j]), (q, i, j)
    if scene == 'planted':
        # every special feature carries a match: without it in the products, or in the norms, a maximum moves by over 100 bounds
        feats = special_features(dt, ks, p)
        assert set(feats) <= {f for s in c.sets for f in s}
        for f in feats:
            for where in ('product', 'norm'):
                most = 0.0
                for r in ref:
                    A, B = c.D[r.a].astype(np.float64), c.D[r.b].astype(np.float64)
                    A0, B0 = A.copy(), B.copy()
                    A0[:, f] = 0
                    B0[:, f] = 0
                    with np.errstate(invalid='ignore', divide='ignore'):
                        if where == 'product':
                            Cs = A0.dot(B0.T) / np.linalg.norm(A, axis=1)[:, None] / np.linalg.norm(B, axis=1)[None, :]
                        else:
                            Cs = A.dot(B.T) / np.linalg.norm(A0, axis=1)[:, None] / np.linalg.norm(B0, axis=1)[None, :]
                    most = max(most, np.max(_moved(Cs.max(axis=1), r.rm) / r.brow), np.max(_moved(Cs.max(axis=0), r.cm) / r.bcol))
                assert most >= 100, (f, where, most)
        # the designated positions of this shape
        bm = BMS[dt]
        pos = {(q, i, j) for q, i, j in c.matches}
        for q, pr in enumerate(pl.pairs):
            if min(pr.ka, pr.kb, p) >= 2:
                assert any(qq == q and j == pr.kb - 1 for qq, i, j in pos), 'column nc - 1 of the last tile column'
                assert any(qq == q and i == pr.ka - 1 for qq, i, j in pos), 'row mr - 1 of the last tile row, the last strip'
            if min(pr.ka, pr.kb, p) >= 2 + 2 * max(pr.tr, pr.tc):
                for t in range(pr.tc):
                    assert any(qq == q and j == t * bm for qq, i, j in pos) and \
                        any(qq == q and j == min(t * bm + bm, pr.kb) - 1 for qq, i, j in pos)
                for t in range(pr.tr):
                    assert any(qq == q and i == t * bm for qq, i, j in pos) and \
                        any(qq == q and i == min(t * bm + bm, pr.ka) - 1 for qq, i, j in pos)
        return
    # the non-finite scenes: one row (one column) of NaN, the other side NaN throughout, d NaN
    r = ref[0]
    assert np.isnan(r.d)
    if c.nan_row is not None:
        assert np.flatnonzero(np.isnan(r.rm)).tolist() == [c.nan_row] and np.all(np.isnan(r.cm))
    else:
        assert np.flatnonzero(np.isnan(r.cm)).tolist() == [c.nan_col] and np.all(np.isnan(r.rm))
    finite = [x[np.isfinite(x)] for x in c.D]
    assert all(np.max(np.abs(x)) <= 1 for x in finite)


def test_every_position_is_planted_somewhere():
    """over the planted cases: a row whose partner is the last column of an edge tile (nc - 1), of an interior tile (BM - 1), the
    first column of a later tile; a column whose partner is row mr - 1 of the last tile row (the last row of the last, short strip),
    row BM - 1 (the last strip of a full tile), the first row of a later tile row - unsplit and split, both dtypes"""
    seen = set()
    for case in CASES:
        dt, ks, p, scene = case
        if scene != 'planted':
            continue
        pl, bm = am_plan(dt, ks, p), BMS[dt]
        tag = (dt, 'split' if pl.nsplit > 1 else 'unsplit')
        for q, i, j in build(case).matches:
            pr = pl.pairs[q]
            for name, x, k in (('col', j, pr.kb), ('row', i, pr.ka)):
                if k % bm and x == k - 1:
                    seen.add(tag + (name, 'last of the edge tile'))
                if k > bm and x == bm - 1:
                    seen.add(tag + (name, 'last of an interior tile'))
                if x and x % bm == 0:
                    seen.add(tag + (name, 'first of a later tile'))
                if x == 0:
                    seen.add(tag + (name, 'first'))
            if pl.nsplit > 1 and pr.tr > 1 and i >= (pr.tr - 1) * bm and cdiv(pr.ka - (pr.tr - 1) * bm, STRIP) < bm // STRIP:
                seen.add(tag + ('row', 'in the short last tile row'))
    want = {(dt, sp, name, w) for dt in DT for sp in ('split', 'unsplit') for name in ('row', 'col')
            for w in ('last of the edge tile', 'last of an interior tile', 'first of a later tile', 'first')}
    want |= {(dt, 'split', 'row', 'in the short last tile row') for dt in DT}
    assert not want - seen, sorted(want - seen)


def test_restatements_agree():
    """restate_call without a mutant is the per-pair restatement of tests/test_stability.py, rounded"""
    for case in CASES:
        dt = case[0]
        got, ref = restate_call(build(case).D, dt), reference(case)
        for q, r in enumerate(ref):
            with np.errstate(over='ignore', invalid='ignore'):
                assert np.array_equal(got['rowmax'][q], r.rm.astype(DT[dt]), equal_nan=True)
                assert np.array_equal(got['colmax'][q], r.cm.astype(DT[dt]), equal_nan=True)
            assert got['d'][q] == r.d or (np.isnan(got['d'][q]) and np.isnan(r.d))


@pytest.mark.parametrize('dt', ('f32', 'f64'))
def test_judge_accepts_the_rounded_restatement(dt):
    for case in CASES:
        if case[0] == dt:
            worst, why = judge(reference(case), restate_call(build(case).D, dt))
            assert why is None and worst <= 1, (case_id(case), why)


@pytest.mark.parametrize('mut', MUTANTS)
@pytest.mark.parametrize('dt', ('f32', 'f64'))
def test_judge_rejects_mutants(dt, mut):
    cases = mutant_cases(mut)
    assert {c[0] for c in cases} == {'f32', 'f64'}, mut
    for case in cases:
        if case[0] != dt:
            continue
        _, why = judge(reference(case), restate_call(build(case).D, dt, mut))
        assert why is not None, (mut, case_id(case))


def test_mutants_are_the_issues_list():
    assert len(MUTANTS) == 16 and len(set(MUTANTS)) == 16         # fifteen of the issue; its "row or column" mutant is two here
    with open(__file__.replace('.pyc', '.py')) as f:
        doc = f.read().split('"""')[1]
    for mut in MUTANTS:
        assert re.search(r'^  %s ' % mut, doc, re.M), mut


# ------------------------------------------------------------------------------------------------------------- GPU tests
WORST = {'f32': 0.0, 'f64': 0.0}


def to_device(D, mis=()):
    """contiguous device tensors; the dictionaries of `mis` start one element into a larger buffer"""
    import torch
    out = []
    for d, x in enumerate(D):
        if d in mis:
            buf = torch.empty(x.size + 1, dtype=torch.from_numpy(x).dtype, device='cuda')
            t = buf[1:].view(x.shape)
            t.copy_(torch.from_numpy(x))
            assert t.is_contiguous() and t.data_ptr() % 16 == x.itemsize
        else:
            t = torch.from_numpy(x).cuda()
            assert t.data_ptr() % 16 == 0
        out.append(t)
    return out


def run_abi(lib, dt, tensors, maxima=True):
    """modl_amari_* on device tensors: workspace of 0xFF bytes, outputs of SENT with GUARD elements behind; checks the guards"""
    import torch
    from modl_amd import device as dev
    ks, p = [int(t.shape[0]) for t in tensors], int(tensors[0].shape[1])
    pl = am_plan(dt, ks, p)
    ws_bytes = _ws_bytes(lib, dt, ks, p)
    assert ws_bytes == pl.bytes
    tdt = dev.torch_dtype(DT[dt])
    n_row, n_col = sum(q.ka for q in pl.pairs), sum(q.kb for q in pl.pairs)
    ws = torch.full((ws_bytes,), 0xFF, dtype=torch.uint8, device='cuda')
    d = torch.full((pl.npairs + GUARD,), SENT, dtype=torch.float64, device='cuda')
    row = torch.full((n_row + GUARD,), SENT, dtype=tdt, device='cuda') if maxima else None
    col = torch.full((n_col + GUARD,), SENT, dtype=tdt, device='cuda') if maxima else None
    ptrs = (C.c_void_p * len(ks))(*[t.data_ptr() for t in tensors])
    k64 = np.array(ks, dtype=np.int64)
    launches = C.c_int(-1)
    rc = getattr(lib, 'modl_amari_' + dt)(ptrs, k64.ctypes.data_as(C.c_void_p), len(ks), p, dev.ptr(d), dev.ptr(row), dev.ptr(col),
                                          dev.ptr(ws), ws_bytes, dev.stream_ptr(dev.default_device()), C.byref(launches))
    assert rc == 0
    torch.cuda.synchronize()
    assert launches.value == pl.launches
    out = {'d': d.cpu().numpy()}
    assert np.all(out['d'][pl.npairs:] == SENT), 'guard behind d'
    out['d'] = out['d'][:pl.npairs]
    if maxima:
        r, c = row.cpu().numpy(), col.cpu().numpy()
        assert np.all(r[n_row:] == SENT) and np.all(c[n_col:] == SENT), 'guards behind rowmax / colmax'
        out['rowmax'] = [r[q.roff:q.roff + q.ka] for q in pl.pairs]
        out['colmax'] = [c[q.coff:q.coff + q.kb] for q in pl.pairs]
    return out


def held(dt, ref, got):
    worst, why = judge(ref, got)
    assert why is None, why
    WORST[dt] = max(WORST[dt], worst)
    return worst


def same_bits(x, y):
    return all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(x, y)) and len(x) == len(y)


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_abi_against_restatement(lib, case):
    dt = case[0]
    got = run_abi(lib, dt, to_device(build(case).D))
    held(dt, reference(case), got)


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ('f32', 'f64'))
def test_without_maxima_same_d(lib, dt):
    for case in CASES:
        if case[0] == dt and case[3] in ('planted', 'nan_tail') and not (case[1] == (5, 7) and case[2] in NORM_P[1:]):
            T = to_device(build(case).D)
            assert run_abi(lib, dt, T, maxima=False)['d'].tobytes() == run_abi(lib, dt, T)['d'].tobytes(), case_id(case)


@pytest.mark.gpu
@pytest.mark.parametrize('ks,p', [((129, 257), 8196), ((128, 256), 64)], ids=['split', 'unsplit'])
def test_misaligned_base(lib, ks, p):
    """f32, p a multiple of 4: one operand of the pair starts 4 bytes into a buffer (element-wise staging), the other is aligned
    (16-byte loads)"""
    from modl_amd.stability import amari_pairs
    D = build(('f32', ks, p, 'planted')).D
    for order, mis in (((0, 1), (1,)), ((1, 0), (0,)), ((0, 1), (0,))):
        E = [D[order[0]], D[order[1]]]
        assert route('f32', [x.shape[0] for x in E], p, mis=mis).unal == [d in mis for d in range(2)]
        ref = reference_of(E, 'f32')
        T = to_device(E, mis=mis)
        assert [t.data_ptr() % 16 for t in T] == [4 if d in mis else 0 for d in range(2)]
        got = run_abi(lib, 'f32', T)
        held('f32', ref, got)
        aligned = run_abi(lib, 'f32', to_device(E))
        assert same_bits(got['rowmax'] + got['colmax'] + [got['d']], aligned['rowmax'] + aligned['colmax'] + [aligned['d']])
        r = amari_pairs(T, maxima=True)                                 # _stage uses the views in place
        assert r['launches'] == am_plan('f32', [x.shape[0] for x in E], p).launches
        held('f32', ref, r)
        assert same_bits(r['rowmax'] + r['colmax'] + [r['d']], got['rowmax'] + got['colmax'] + [got['d']])


SCALE_SHAPES = {'f32': [((129, 130), 61), ((129, 257), 8196)], 'f64': [((65, 66), 61), ((65, 130), 8195)]}


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ('f32', 'f64'))
def test_power_of_two_scaling_keeps_every_bit(lib, dt):
    e = 20 if dt == 'f32' else 200
    tiny, huge = float(np.finfo(DT[dt]).tiny), float(np.finfo(DT[dt]).max)
    for ks, p in SCALE_SHAPES[dt]:
        D = build((dt, ks, p, 'planted')).D
        base = run_abi(lib, dt, to_device(D))
        lo, hi = [np.min(np.abs(x)) for x in D], [np.max(np.abs(x)) for x in D]
        for sa, sb in ((e, 0), (-e, 0), (0, e), (e, e), (-e, -e), (e, -e)):
            # every product, every square and every sum of them stays normal
            fa, fb = 2.0 ** sa, 2.0 ** sb
            assert min(lo[0] * fa * lo[1] * fb, (lo[0] * fa) ** 2, (lo[1] * fb) ** 2) > tiny * 2 ** 30
            assert max(hi[0] * fa * hi[1] * fb, (hi[0] * fa) ** 2, (hi[1] * fb) ** 2) * p < huge / 2 ** 30
            E = [(D[0] * DT[dt](fa)).astype(DT[dt]), (D[1] * DT[dt](fb)).astype(DT[dt])]
            got = run_abi(lib, dt, to_device(E))
            assert same_bits(got['rowmax'] + got['colmax'] + [got['d']], base['rowmax'] + base['colmax'] + [base['d']]), (ks, p, sa, sb)


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ('f32', 'f64'))
def test_permuted_atoms_keep_every_bit(lib, dt):
    """A dot product's order of summation does not depend on where its row sits in a tile, in which tile, or on whether that tile
    is an edge tile: with the atoms of A permuted the row maxima are permuted bit for bit and the column maxima keep their bits"""
    for ks, p in SCALE_SHAPES[dt]:
        case = (dt, ks, p, 'planted')
        D = build(case).D
        base = run_abi(lib, dt, to_device(D))
        perm = np.random.RandomState(5).permutation(ks[0])
        assert perm[ks[0] - 1] != ks[0] - 1 or ks[0] == 1
        E = [np.ascontiguousarray(D[0][perm]), D[1]]
        got = run_abi(lib, dt, to_device(E))
        held(dt, reference_of(E, dt), got)
        assert got['rowmax'][0].tobytes() == base['rowmax'][0][perm].tobytes()
        assert got['colmax'][0].tobytes() == base['colmax'][0].tobytes()


@pytest.mark.gpu
def test_rerun_same_bits(lib):
    dt, ks, p = 'f64', (65, 3, 66), 8195                                # split, unal, three pairs
    assert 'split2' in route(dt, ks, p).s and route(dt, ks, p).unal == [True] * 3
    D = planted(dt, ks, p, 77)[0]
    T = to_device(D)
    r1, r2 = run_abi(lib, dt, T), run_abi(lib, dt, T)
    held(dt, reference_of(D, dt), r1)
    assert same_bits(r1['rowmax'] + r1['colmax'] + [r1['d']], r2['rowmax'] + r2['colmax'] + [r2['d']])


@pytest.mark.gpu
def test_wrapper_list_against_its_pairs():
    """amari_pairs on a ragged split list against the same dictionaries as two-element lists (other split counts: the bits may differ)"""
    from modl_amd.stability import amari_pairs
    case = ('f64', (66, 3, 65), 8200, 'planted')
    D, ref = build(case).D, reference(case)
    r = amari_pairs(D, maxima=True)
    assert r['dtype'] == np.float64 and r['launches'] == am_plan(*case[:3]).launches
    held('f64', ref, r)
    for q, x in enumerate(ref):
        two = amari_pairs([D[x.a], D[x.b]], maxima=True)
        assert two['launches'] == am_plan('f64', (D[x.a].shape[0], D[x.b].shape[0]), 8200).launches
        held('f64', [x], two)
        assert np.all(np.abs(two['rowmax'][0] - r['rowmax'][q]) <= 2 * x.brow)
        assert np.all(np.abs(two['colmax'][0] - r['colmax'][q]) <= 2 * x.bcol)
        assert abs(two['d'][0] - r['d'][q]) <= 2 * x.bd


@pytest.mark.gpu
def test_report():
    """the largest error / bound of this run, per dtype; recorded in DESIGN.md, not asserted beyond the judge's own 1"""
    print('\nstability routes: largest |got - ref| / bound  f32 %.3f  f64 %.3f' % (WORST['f32'], WORST['f64']))
    assert WORST['f32'] <= 1 and WORST['f64'] <= 1
