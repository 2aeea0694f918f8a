"""The image kernels route by route (modl_amd/csrc/image.hip): modl_image_patches_*, modl_image_grid_patches_*, the two masked
window kernels, modl_image_decode_*, overlap-add and finish, the weighted overlap-add and the inpaint finish, modl_objective_*.
Every result is compared element by element with the same expression in np.longdouble, or bit by bit with the same kernels
called another way (another pass cut, the twin kernel, other mask bytes).  The C ABI is called directly (modl_amd._lib.lib), so
that leading dimensions, guard words and sentinels are this file's choice.

ROUTES (`POINTS`; `test_route_table` holds every point to `expected_route`, a restatement of the dispatch, and every leaf of the
restatement - a call of `_leaf`, the list read out of this file's own text - to at least one point or to `UNREACHED`).  Lines
of modl_amd/csrc/image.hip as of this commit:
  :34-55, :59-66    patch_row: per channel, lane l adds positions l, l + 64, ... (ceil(xy / 64) trips), wave_sum, / xy; the
                    centred squares the same way; sd == 0 -> 1; den = sd sqrt(z); then ceil(P / 64) trips over the row
  :76-81, :87-88    one wavefront per patch, slot q % 4 of workgroup q / 4; n == 0 launches nothing; origin (i0, j0, c0) read
                    from idx3, the window's channels c0 .. c0 + z - 1 at stride C
  :595-597          z <= C, z <= 1024 (kPatchMaxChannels: 2 x 4 x 1024 x 8 bytes = 64 KiB of LDS for f64), ldo >= P
  :161-172          GridAxis: g = ceil((L - x) / s) + 1, origin(r) = min(r s, L - x), lo(t), hi(t)
  :186-194          the grid kernel: origin computed from q, ceil(C / 64) trips to fill (no scaling) and to write mean / den
  :288-296          masked_patch_window: ceil(P / 64) trips over the mask, cnt == P -> patch_row itself (clean)
  :301-326          holed: per channel n_c, mean over the observed, sd sqrt(xy / n_c); n_c == 0 -> mean 0, sd 1
  :328-337          holed row: unobserved elements 0; ceil(C / 64) trips to write mean / den
  :200-206, :214-221  decode: chunks of 2^21 rows at code + r0 k, out + r0 ldo, mean + r0 C, den + r0 C; unscale by e % C
  :238-255          overlap-add: one thread per (pixel, channel) of the pixel rows of the pass, [lo, hi] clamped to the pass,
                    accumulate onto acc; :452-453 i_begin = origin(row0), total = (i_end - i_begin) W C
  :263-268          finish: acc / ((hi - lo + 1)_i (hi - lo + 1)_j)
  :381-403          weighted: rows with use[q] == 0 skipped (never read), cnt += added by the thread of channel 0
  :415-419          inpaint finish: cnt > 0 and not (keep and observed) -> acc / cnt, else the input
  :127-148, :670-675  objective: chunk = (ws - 8 KiB) / (p sizeof T) rows (default workspace: min(n, 8192) rows), the residual
                    sum ACCUMULATED per chunk; obj_partial: 1024 x 256 threads, grid-stride (second trip past 262 144 elements)

SCENES
  integers   pixels, patches, codes uniform in {-3 .. 3} (images in multiples of 1 / 4): unscaled rows, rows centred over a
             power-of-two count, decoded integers, overlap sums, quotients and objective sums are exact - compared bitwise
  gaussian   the control
  offset     pixels 1000 + U(0, 1): the centring cancels three digits (f32 keeps four of seven)
  flat       a constant window (every channel) at the first origin and a constant channel 0 all over a varied image, the
             constants multiples of 1 / 4: mean bitwise the constant, rows exactly 0, den exactly 1 sqrt(z)
  scales     channel c scaled by 10^U(-3, 3)
  bytes      observed bytes / use bytes from {1, 2, 0x80, 0xFF}: the bits of the call with 1
  poison     NaN / Inf at every unobserved element, NaN in unused patch rows: the same bits, every output finite
  Every call is made twice and gives identical bits.  Outputs lie between guard words; rows have 3 elements of padding in the
  loose layout; guards and padding keep their sentinel.

JUDGES (ref in np.longdouble from the inputs; eps the dtype's machine epsilon; S = ceil(xy / 64) + 6: the additions of one
lane plus the six steps of the wavefront sum plus the division)
  mean     |mean - ref| <= dm + eps |ref|,  dm = S eps M_c,  M_c the largest |pixel| of the channel's (observed) window
  den      |den - ref| <= rho |ref|,  rho = (S / 2 + 8) eps + n_c dm^2 / (2 sum u^2): half the relative error of the sum of
           squares (S additions, two roundings in u), sqrt, sqrt(xy / n_c) (three), sqrt(z), the product; an error dm of the
           mean enters the sum of centred squares in second order only (sum u = 0), that is the last term
  row      |v - ref| <= dm / den + (rho + 2 eps) |ref|: the centred value is rounded relative to the pixel, the rest
           relative to the result; no scaling: bound 0, the bits of the pixel
  decode   (k + 8) eps (|den| sum |code| |D| + |mean|)
  sums     overlap accumulators: (cover + 1) 2^-52 (|pre-load| + sum |patch|); finish: eps |ref| (one rounding to T)
  objective  sum R^2: sum_e (2 |R_e| b_e + b_e^2) + N 2^-52 sum R^2, b_e = (k + 8) eps (|X_e| + sum |code| |D|), N = 24 +
           chunks (additions of a thread, two block sums, the final sum, one accumulation per chunk); sum |code| and sum
           code^2: N 2^-52 of the sum
  `test_judges_on_the_oracle`: the same-dtype numpy restatement (`window_rows` with T the dtype: lane sums in T in the
  kernel's order; overlap sums in f64) is under every bound on every scene and shape.

MUTANTS (`test_mutants`; mutant -> scene @ shape that rejects it)
  statistic loop stops after 64 positions      gaussian @ patch (5, 13).  INVISIBLE at xy <= 64 (asserted at (8, 8))
  statistics pooled over channels              scales @ (4, 5) z 3.  INVISIBLE at z = 1 (asserted)
  divisor sqrt(C) for z < C                    gaussian @ C 5 z 2.  INVISIBLE at z == C (asserted)
  norm over xy - 1                             gaussian @ (4, 5)
  one-pass variance                            offset @ (4, 5), both dtypes
  zero-norm rule missing                       flat @ (4, 5): non-finite row
  window read as (y, x)                        gaussian @ (4, 5).  INVISIBLE at (1, 1) (asserted)
  c0 dropped                                   gaussian @ C 5 z 2 c0 3.  INVISIBLE at c0 = 0 (asserted)
  holed: statistics over all positions         gaussian @ (4, 5) holed window
  holed: sqrt(xy / n_c) missing                gaussian @ (4, 5) holed window.  INVISIBLE without with_std (asserted)
  holed: unobserved written unscaled           gaussian @ (4, 5) holed window; poison makes it non-finite
  decode: statistics of chunk 0 reused         integers, gaussian @ n 13 with chunks of 8
  decode: n / C for n % C                      gaussian @ P 6 C 3
  grid: last origin unclamped, lo / hi off by one, count x y / (s_i s_j)
                                               the brute-force rule (`test_grid_rule`), and integers through overlap-add
  overlap-add stores                           integers with a pre-loaded accumulator.  INVISIBLE on a zero one (asserted)
  cnt incremented per channel                  C 3.  INVISIBLE at C 1 (asserted)
  pass clamp dropped                           integers, passes of one grid row.  INVISIBLE in the full call (asserted)
  objective: chunk overwrites                  integers @ two chunks.  INVISIBLE with one chunk (asserted)
  objective: |code| over ldx columns           integers @ ldx != k.  INVISIBLE at ldx == k (asserted)

MEASURED (largest |got - ref| / bound per kernel on the MI355X, f32 / f64, from this file's own run - `_report` prints them;
recorded, not asserted).  128 GPU cases; the whole file runs in 7 s, no case above 0.2 s after the first.
  patches 0.110 / 0.106       grid rows 0.117 / 0.125, mean 0.102 / 0.094, den 0.103 / 0.141
  masked rows 0.130 / 0.140, mean 0.077 / 0.098, den 0.130 / 0.178                decode 0.109 / 0.086
  overlap 0.25 / 0.30, weighted 0.25 / 0.24, finish 0.49 / 0.33, inpaint finish 0.48 / 0.17        objective 0.016 / 0.037
  numpy's same-dtype restatement on the CPU (`test_judges_on_the_oracle`): patches 0.172 / 0.150, grid 0.117 / 0.132, masked
  0.137 / 0.163, decode 0.109 / 0.086, overlap 0.25 / 0.30, finish 0.49 / 0.33, objective 0.023 / 0.032 of the bound.
"""
import ctypes as C
import itertools
import re
import zlib
from types import SimpleNamespace

import numpy as np
import pytest

DT = {'f32': np.float32, 'f64': np.float64}
LD = np.longdouble
BOTH = ('f32', 'f64')
FILL = 7.5
EINVAL, ENOMEM = -1, -2
MAXC = 1024                                    # kPatchMaxChannels (:24)
DECODE_CHUNK = 1 << 21                         # kDecodeChunk (:209)
OBJ_BLOCKS, OBJ_ROWS = 1024, 8192              # kObjBlocks (:100), the default workspace's rows (:673)
OBJ_SWEEP = OBJ_BLOCKS * 256                   # elements of one trip of obj_partial_kernel's grid-stride loop (:109)
SCALINGS = ((0, 0), (0, 1), (1, 0), (1, 1))    # (with_mean, with_std)


def cdiv(a, b):
    return -(-a // b)


HIT = set()


def _leaf(name):
    """Marks a branch of the restatement; `all_leaves` reads the names out of this file's own text."""
    HIT.add(name)
    return name


def all_leaves():
    with open(__file__.replace('.pyc', '.py')) as f:
        return set(re.findall(r"_leaf\('([^']+)'\)", f.read()))


# ---------------------------------------------------------------------------------------------------- the dispatch, restated
class Axis:
    """GridAxis (:161-172), with the wrong versions `test_grid_rule` and `test_mutants` ask for"""
    def __init__(self, L, x, s, mut=()):
        assert 1 <= s <= x <= L
        self.L, self.x, self.s, self.mut = L, x, s, mut
        self.g = cdiv(L - x, s) + 1

    def origin(self, r):
        if 'unclamped' in self.mut:
            return r * self.s
        return r * self.s if r * self.s < self.L - self.x else self.L - self.x

    def lo(self, t):
        v = (t - self.x + self.s) // self.s if t - self.x + self.s > 0 else 0
        return v + (1 if 'lo+1' in self.mut and v < self.hi(t) else 0)

    def hi(self, t):
        v = self.g - 1 if t >= self.L - self.x else t // self.s
        return v - (1 if 'hi-1' in self.mut and v > 0 else 0)

    def kind(self):
        if self.g == 1:
            return _leaf('axis/g1')
        if (self.L - self.x) % self.s:
            return _leaf('axis/clamped')
        return _leaf('axis/exact')


def brute_axis(L, x, s):
    """the origins by the rule's words: 0, s, 2 s, ... <= L - x, plus L - x when it is not the last of them"""
    o = list(range(0, L - x + 1, s))
    if o[-1] != L - x:
        o.append(L - x)
    return o


def trips(n):
    return cdiv(n, 64)


def _trip_leaf(what, n):
    t = trips(n)
    if what == 'stat':
        return _leaf('stat/1trip') if t == 1 else _leaf('stat/2trips') if t == 2 else _leaf('stat/3+trips')
    if what == 'row':
        return _leaf('row/1trip') if t == 1 else _leaf('row/2trips') if t == 2 else _leaf('row/3+trips')
    return _leaf('chan/1trip') if t == 1 else _leaf('chan/2trips') if t == 2 else _leaf('chan/3+trips')


def patches_route(x, y, z, Cc, c0, n, wm, ws, pad):
    if not (n >= 0 and x > 0 and y > 0 and 0 < z <= Cc and z <= MAXC):       # :595-597
        return _leaf('patches/einval')
    if n == 0:                                                               # :87
        return _leaf('patches/n0')
    s = [_trip_leaf('stat', x * y) if (wm or ws) else _leaf('stat/none')]     # :34-55
    s.append(_trip_leaf('row', x * y * z))                                   # :59-66
    s.append(_leaf('window/all') if z == Cc else _leaf('window/c0=0') if c0 == 0 else _leaf('window/c0>0'))    # :79-80
    s.append(_leaf('wg/partial') if n % 4 else _leaf('wg/full'))             # :76-78
    s.append(_leaf('wg/one') if n <= 4 else _leaf('wg/more'))                # :88
    s.append(_leaf('layout/loose') if pad else _leaf('layout/tight'))
    return 'patches/' + '/'.join(s) + '/slots%s' % sorted({q % 4 for q in range(n)})


def grid_route(H, W, Cc, x, y, si, sj, wm, ws):
    if not (0 < Cc <= MAXC):                                                 # :425
        return _leaf('grid/einval')
    gi, gj = Axis(H, x, si), Axis(W, y, sj)
    s = ['i:' + gi.kind(), 'j:' + gj.kind()]
    s.append(_trip_leaf('chan', Cc))                                         # :191, :194
    s.append(_leaf('stats/kept') if (wm or ws) else _leaf('stats/filled'))   # :190-191
    s.append(_trip_leaf('stat', x * y) if (wm or ws) else _leaf('stat/none'))
    s.append(_leaf('wg/partial') if (gi.g * gj.g) % 4 else _leaf('wg/full'))
    return 'grid/' + '/'.join(s) + '/g%dx%d' % (gi.g, gj.g)


def window_branch(on):
    """the branch of masked_patch_window for one window of the mask, on (xy, z) bool (:296, :312, :321)"""
    if on.all():
        return _leaf('masked/clean')
    if not on.any():
        return _leaf('masked/empty_window')
    if not on.any(axis=0).all():
        return _leaf('masked/empty_channel')
    return _leaf('masked/holed')


def decode_chunks(n, chunk=DECODE_CHUNK):                                    # :214-215
    return [(r0, min(chunk, n - r0)) for r0 in range(0, n, chunk)]


def decode_route(n, k, P, Cc, stats, pad):
    ch = decode_chunks(n)
    if not ch:                                                               # :214: no launch
        return _leaf('decode/n0')
    s = [_leaf('decode/unscale') if stats else _leaf('decode/plain')]        # :201
    s.append(_leaf('decode/one_chunk') if len(ch) == 1 else _leaf('decode/chunks'))
    if stats:
        s.append(_leaf('decode/C=1') if Cc == 1 else _leaf('decode/C=P') if Cc == P else _leaf('decode/1<C<P'))
    s.append(_leaf('layout/loose') if pad else _leaf('layout/tight'))
    return 'decode/' + '/'.join(s) + '/%s' % (ch if len(ch) < 3 else len(ch),)


def overlap_route(H, W, Cc, x, y, si, sj, passes):
    gi, gj = Axis(H, x, si), Axis(W, y, sj)
    s = ['i:' + gi.kind(), 'j:' + gj.kind()]
    for row0, nrows in passes:
        i_begin, i_end = gi.origin(row0), gi.origin(row0 + nrows - 1) + x    # :452
        total = (i_end - i_begin) * W * Cc
        s.append(_leaf('pass/whole') if (row0, nrows) == (0, gi.g) else _leaf('pass/cut'))
        s.append(_leaf('pass/i_begin>0') if i_begin else _leaf('pass/i_begin=0'))
        s.append(_leaf('pass/tail_block') if total % 256 else _leaf('pass/full_blocks'))
    return 'overlap/' + '/'.join(s)


def objective_chunks(n, p, ws_bytes, tsz):
    """None: MODL_ENOMEM (:127); else the (r0, rows) of every residual launch (:130-134)"""
    if ws_bytes < 8 * OBJ_BLOCKS + tsz * p:
        return None
    chunk = (ws_bytes - 8 * OBJ_BLOCKS) // (tsz * p)
    return [(r0, min(chunk, n - r0)) for r0 in range(0, n, chunk)]


def objective_workspace(n, p, tsz):                                          # :670-675
    return 8 * OBJ_BLOCKS + tsz * p * min(max(n, 1), OBJ_ROWS)


def objective_route(n, p, k, ws_rows, tsz, pad):
    ws = objective_workspace(n, p, tsz) if ws_rows is None else 8 * OBJ_BLOCKS + tsz * p * ws_rows
    ch = objective_chunks(n, p, ws, tsz)
    if ch is None:
        return _leaf('objective/enomem')
    if n == 0:                                                               # :132
        return _leaf('objective/n0')
    s = [_leaf('objective/one_chunk') if len(ch) == 1 else _leaf('objective/chunks')]
    s.append(_leaf('objective/two_sweeps') if max(r for _, r in ch) * p > OBJ_SWEEP else _leaf('objective/one_sweep'))
    s.append(_leaf('objective/default_ws') if ws_rows is None else _leaf('objective/own_ws'))
    s.append(_leaf('layout/loose') if pad else _leaf('layout/tight'))
    return 'objective/' + '/'.join(s) + '/chunks%d' % len(ch)


POINTS = []


def _point(probe, name, want, **sh):
    POINTS.append(SimpleNamespace(probe=probe, name=name, want=want, sh=sh))


def _p(name, patch, Cc, z, c0, n, want, img=None, scenes=('gaussian', 'offset')):
    x, y = patch
    _point('patches', name, want, x=x, y=y, C=Cc, z=z, c0=c0, n=n, H=(img or (x + 3, y + 4))[0], W=(img or (x + 3, y + 4))[1],
           scenes=scenes)


ALL_SCENES = ('integers', 'gaussian', 'offset', 'flat', 'scales')
# lane loops: xy = 1, 63, 64, 65, 129; P = xy z on both sides of 64
_p('p-xy1', (1, 1), 3, 3, 0, 6, ('stat/1trip', 'row/1trip'), scenes=('integers', 'gaussian'))
_p('p-xy63', (7, 9), 1, 1, 0, 6, ('stat/1trip', 'row/1trip'))
_p('p-xy64', (8, 8), 1, 1, 0, 6, ('stat/1trip', 'row/1trip'), scenes=ALL_SCENES)
_p('p-xy65', (5, 13), 1, 1, 0, 6, ('stat/2trips', 'row/2trips'), scenes=ALL_SCENES)
_p('p-xy129', (3, 43), 2, 2, 0, 6, ('stat/3+trips', 'row/3+trips'))
_p('p-P60', (4, 5), 3, 3, 0, 6, ('stat/1trip', 'row/1trip', 'window/all'), scenes=ALL_SCENES)
_p('p-P189', (7, 9), 3, 3, 0, 6, ('stat/1trip', 'row/3+trips'))
# channel windows
_p('p-z2-c0', (4, 5), 5, 2, 0, 6, ('window/c0=0',), scenes=ALL_SCENES)
_p('p-z2-c3', (4, 5), 5, 2, 3, 6, ('window/c0>0',), scenes=ALL_SCENES)
_p('p-z1-c1', (4, 5), 3, 1, 1, 6, ('window/c0>0',))
# channel counts
_p('p-C1', (2, 1), 1, 1, 0, 6, ('window/all',), scenes=('integers', 'gaussian', 'offset'))
_p('p-C64', (2, 1), 64, 64, 0, 6, ('row/2trips',))
_p('p-C65', (2, 1), 65, 65, 0, 6, ('row/3+trips',), scenes=ALL_SCENES)
_p('p-C1024', (2, 1), 1024, 1024, 0, 5, ('row/3+trips', 'wg/more'))
_p('p-C1024-1x1', (1, 1), 1024, 1024, 0, 3, ('stat/1trip',), img=(2, 2))
_point('patches', 'p-z1025', ('patches/einval',), x=1, y=1, C=2000, z=1025, c0=0, n=1, H=2, W=2, scenes=(), host=True)
# workgroup slots
for _n, _w in ((0, ('patches/n0',)), (1, ('wg/partial', 'wg/one', 'slots[0]')), (3, ('wg/partial', 'slots[0, 1, 2]')),
               (4, ('wg/full', 'wg/one', 'slots[0, 1, 2, 3]')), (5, ('wg/partial', 'wg/more'))):
    _p('p-n%d' % _n, (4, 5), 3, 3, 0, _n, _w, scenes=('gaussian',))


def _g(name, H, W, Cc, patch, stride, want, masked=False, weighted=False):
    _point('grid', name, want, H=H, W=W, C=Cc, x=patch[0], y=patch[1], si=stride[0], sj=stride[1], masked=masked, weighted=weighted)


# (L, x, s): (x, x, 1) g 1; (x + 1, x, x) g 2, the clamped origin overlapping by x - 1; (L - x) % s == 0 and != 0; s = 1; s = x; x = 1
_g('g-g1-g2', 4, 6, 3, (4, 5), (1, 5), ('i:axis/g1', 'j:axis/clamped', 'g1x2', 'wg/partial'))
_g('g-exact-clamped', 10, 11, 3, (4, 5), (3, 4), ('i:axis/exact', 'j:axis/clamped', 'g3x3'), weighted=True)
_g('g-clamped-exact-C1', 11, 10, 1, (5, 4), (4, 3), ('i:axis/clamped', 'j:axis/exact', 'chan/1trip'), weighted=True)
_g('g-s1-sx', 7, 15, 2, (4, 5), (1, 5), ('i:axis/exact', 'j:axis/exact', 'g4x3', 'wg/full'))
_g('g-x1', 5, 12, 3, (1, 5), (1, 5), ('i:axis/exact', 'j:axis/clamped', 'g5x3', 'wg/partial'), weighted=True)
_g('g-xy65', 9, 20, 3, (5, 13), (2, 6), ('stat/2trips', 'g3x3'))
_g('g-C65', 5, 3, 65, (2, 1), (1, 1), ('chan/2trips', 'g4x3'))
_g('g-C64', 3, 4, 64, (2, 1), (1, 1), ('chan/1trip', 'g2x4', 'pass/full_blocks'))
_g('g-C1024', 3, 2, 1024, (2, 1), (1, 1), ('chan/3+trips', 'g2x2', 'wg/full'))
# the masked window kernels: non-overlapping windows (s = x) so that each branch has a window of its own, the last column clamped
_g('m-4x5', 12, 14, 3, (4, 5), (4, 5), ('stat/1trip', 'g3x3'), masked=True)
_g('m-5x13', 15, 28, 2, (5, 13), (5, 13), ('stat/2trips', 'g3x3'), masked=True)
_g('m-C65', 6, 3, 65, (2, 1), (2, 1), ('chan/2trips', 'g3x3'), masked=True)


def _d(name, n, k, P, Cc, want, big=False):
    _point('decode', name, want, n=n, k=k, P=P, C=Cc, big=big)


_d('d-P1', 37, 1, 1, 1, ('decode/C=1',))
_d('d-P63-C3', 37, 7, 63, 3, ('decode/1<C<P',))
_d('d-P63-C63', 37, 1, 63, 63, ('decode/C=P',))
_d('d-P64-C1', 37, 7, 64, 1, ('decode/C=1',))
_d('d-P64-C64', 37, 1, 64, 64, ('decode/C=P',))
_d('d-P65-C5', 37, 1, 65, 5, ('decode/1<C<P',))
_d('d-P65-C65', 37, 7, 65, 65, ('decode/C=P',))
_d('d-n0', 0, 3, 6, 3, ('decode/n0',))
for _n in (DECODE_CHUNK - 1, DECODE_CHUNK, DECODE_CHUNK + 5):
    _d('d-chunk-%d' % _n, _n, 1, 2, 2, ('decode/chunks' if _n > DECODE_CHUNK else 'decode/one_chunk', 'decode/C=P'), big=True)


def _o(name, n, p, k, ws_rows, want, pad=0):
    _point('objective', name, want, n=n, p=p, k=k, ws_rows=ws_rows, pad=pad)


_o('o-301-ws1', 301, 157, 11, 1, ('objective/chunks', 'chunks301', 'own_ws'))
_o('o-301-ws64', 301, 157, 11, 64, ('objective/chunks', 'chunks5'))
_o('o-301-all', 301, 157, 11, 301, ('objective/one_chunk', 'one_sweep'))
_o('o-301-loose', 301, 157, 11, 64, ('layout/loose',), pad=3)
_o('o-8192', 8192, 33, 5, None, ('objective/one_chunk', 'two_sweeps', 'default_ws'))
_o('o-8193', 8193, 33, 5, None, ('objective/chunks', 'chunks2', 'two_sweeps'))
_o('o-sweep-below', 7943, 33, 5, None, ('objective/one_chunk', 'one_sweep'))      # 7943 x 33 = 262 119 <= 262 144
_o('o-sweep-above', 7944, 33, 5, None, ('objective/one_chunk', 'two_sweeps'))     # 7944 x 33 = 262 152
_o('o-n0', 0, 33, 5, None, ('objective/n0',))
_o('o-enomem', 5, 33, 5, 0, ('objective/enomem',))

POINT = {r.name: r for r in POINTS}
UNREACHED = {
    'grid/einval': 'C outside 1 .. 1024 or a bad grid: MODL_EINVAL before any launch, held by the EINVAL tests of '
                   'tests/test_image_reconstruct.py and tests/test_inpaint.py',
}


def all_cuts(g):
    """every cut of g grid rows into consecutive passes"""
    out = []
    for marks in itertools.product((0, 1), repeat=g - 1):
        edges = [0] + [i + 1 for i, m in enumerate(marks) if m] + [g]
        out.append([(a, b - a) for a, b in zip(edges[:-1], edges[1:])])
    return out


def masked_obs(r, bytes_rs=None):
    """the mask of a masked point: windows of the non-overlapping grid are numbered row-major; window 1 has holes, window 4
    lacks channel 1 (channel 0 of C 2 .. stays), window 8 is empty, window 5 has a single observed element; the rest are clean"""
    sh = r.sh
    H, W, Cc, x, y = sh['H'], sh['W'], sh['C'], sh['x'], sh['y']
    gi, gj = Axis(H, x, sh['si']), Axis(W, y, sh['sj'])
    obs = np.ones((H, W, Cc), dtype=np.uint8)
    rs = np.random.RandomState(_seed(r.name, 'mask'))

    def win(q):
        i0, j0 = gi.origin(q // gj.g), gj.origin(q % gj.g)
        return obs[i0:i0 + x, j0:j0 + y]
    win(8)[:] = 0
    win(5)[:] = 0
    win(5)[x - 1, 0, Cc - 1] = 1
    win(4)[:, :, 1 % Cc] = 0 if Cc > 1 else 1
    if Cc == 1:
        win(4)[0, 0, 0] = 0
    w1 = win(1)
    w1[rs.rand(*w1.shape) < 0.4] = 0
    w1[0, 0, :] = 1
    w1[x - 1, y - 1, 0] = 0
    if bytes_rs is not None:
        obs[obs != 0] = bytes_rs.choice(np.array([1, 2, 0x80, 0xFF], dtype=np.uint8), size=int((obs != 0).sum()))
    return obs


def masked_branches(r, origins):
    obs = masked_obs(r)
    sh = r.sh
    return [window_branch(obs[i:i + sh['x'], j:j + sh['y']].reshape(-1, sh['C']) != 0) for i, j, _ in origins]


def grid_origins(sh):
    gi, gj = Axis(sh['H'], sh['x'], sh['si']), Axis(sh['W'], sh['y'], sh['sj'])
    return [(gi.origin(r), gj.origin(c), 0) for r in range(gi.g) for c in range(gj.g)]


def patch_origins(sh):
    """the four corners, a duplicate, descending order; cut or cycled to n"""
    H, W, x, y, c0 = sh['H'], sh['W'], sh['x'], sh['y'], sh['c0']
    mid = (min(1, H - x), min(2, W - y), c0)
    o = [(H - x, W - y, c0), (H - x, 0, c0), mid, (0, W - y, c0), mid, (0, 0, c0)]
    return [o[q % len(o)] for q in range(sh['n'])]


def expected_route(r, wm=1, ws=1, pad=0, stats=True):
    sh = r.sh
    if r.probe == 'patches':
        return patches_route(sh['x'], sh['y'], sh['z'], sh['C'], sh['c0'], sh['n'], wm, ws, pad)
    if r.probe == 'grid':
        s = grid_route(sh['H'], sh['W'], sh['C'], sh['x'], sh['y'], sh['si'], sh['sj'], wm, ws)
        if sh['masked']:
            s += '/' + '/'.join(sorted(set(masked_branches(r, grid_origins(sh)))))
        else:
            g = Axis(sh['H'], sh['x'], sh['si']).g
            cuts = [[(0, g)]] + [c for c in all_cuts(g) if len(c) > 1]
            s += '/' + overlap_route(sh['H'], sh['W'], sh['C'], sh['x'], sh['y'], sh['si'], sh['sj'], [p for c in cuts for p in c])
        return s
    if r.probe == 'decode':
        return decode_route(sh['n'], sh['k'], sh['P'], sh['C'], stats, pad)
    return objective_route(sh['n'], sh['p'], sh['k'], sh['ws_rows'], 4, pad or sh['pad'])


# ---------------------------------------------------------------------------------------------------- scenes
def _seed(*what):
    return zlib.crc32(('image-' + '-'.join(str(w) for w in what)).encode()) % 100000


def eps_of(dt):
    return float(np.finfo(DT[dt]).eps)


def scene_image(scene, rs, H, W, Cc, dt, first=None, patch=None):
    """(H, W, C) float64 values that the dtype holds exactly"""
    if scene == 'integers':
        return rs.randint(-12, 13, size=(H, W, Cc)) / 4.0
    a = rs.randn(H, W, Cc)
    if scene == 'offset':
        a = 1000.0 + rs.rand(H, W, Cc)
    if scene == 'scales':
        a = a * 10.0 ** rs.uniform(-3, 3, Cc)
    if scene == 'flat':
        if first is not None:
            a[first[0]:first[0] + patch[0], first[1]:first[1] + patch[1], :] = -2.5 + 0.25 * (np.arange(Cc) % 8)
        a[:, :, 0] = 1.25
    return a.astype(DT[dt]).astype(np.float64)


def draw(scene, rs, shape, dt):
    if scene == 'integers':
        return rs.randint(-3, 4, size=shape).astype(np.float64)
    return rs.randn(*shape).astype(DT[dt]).astype(np.float64)


# ---------------------------------------------------------------------------------------------------- the kernels, restated
def lane_sum(v, T, stop64=False):
    """sum over axis 0 the way a wavefront forms it (:39, :45, wave_sum): lane l adds the elements l, l + 64, ... in turn,
    then six pairwise steps; all in T"""
    m = v.shape[0]
    t = max(trips(m), 1)
    pad = np.zeros((t * 64,) + v.shape[1:], dtype=T)
    pad[:m] = v
    pad = pad.reshape((t, 64) + v.shape[1:])
    s = np.zeros((64,) + v.shape[1:], dtype=T)
    for i in range(1 if stop64 else t):
        s = s + pad[i]
    w = 64
    while w > 1:
        w //= 2
        s = s[:w] + s[w:2 * w]
    return s[0]


def window_rows(img, origins, x, y, z, wm, ws, T, obs=None, mut=()):
    """patch_row (:29-67) and masked_patch_window (:280-338) in numpy at the type T (np.longdouble: the reference; the
    dtype: the restatement whose statistics are in T).  -> out (n, P), mean (n, z), den (n, z), obs_out (n, P), nobs (n,)"""
    img = np.asarray(img).astype(T)
    Cc, xy, n = img.shape[2], x * y, len(origins)
    r = SimpleNamespace(out=np.zeros((n, xy * z), dtype=T), mean=np.zeros((n, z), dtype=T), den=np.ones((n, z), dtype=T),
                        obs_out=np.zeros((n, xy * z), dtype=np.uint8), nobs=np.zeros(n, dtype=np.int32))
    sqrt_z = np.sqrt(T(Cc if 'sqrtC' in mut else z))
    stop = 'stop64' in mut
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        for q, (i0, j0, c0) in enumerate(origins):
            if 'drop_c0' in mut:
                c0 = 0
            if 'yx' in mut:
                v = img[i0:i0 + y, j0:j0 + x, c0:c0 + z].reshape(xy, z)
            else:
                v = img[i0:i0 + x, j0:j0 + y, c0:c0 + z].reshape(xy, z)
            on = np.ones((xy, z), dtype=bool) if obs is None else (obs[i0:i0 + x, j0:j0 + y, c0:c0 + z].reshape(xy, z) != 0)
            r.obs_out[q], r.nobs[q] = on.ravel(), on.sum()
            clean = on.all()
            son = np.ones_like(on) if 'holed_all_stats' in mut else on       # the positions the statistics run over
            nc = son.sum(axis=0)
            mean, den = np.zeros(z, dtype=T), np.ones(z, dtype=T)
            if wm:
                if 'pooled' in mut:
                    mean[:] = lane_sum(v.reshape(-1, 1), T)[0] / T(xy * z)
                else:
                    mean = np.where(nc > 0, lane_sum(np.where(son, v, T(0)), T, stop) / np.maximum(nc, 1).astype(T), T(0))
            u = v - mean
            if ws:
                if 'one_pass' in mut:
                    ss = lane_sum(np.where(son, v * v, T(0)), T) - nc.astype(T) * mean * mean
                else:
                    sq = np.where(son, u * u, T(0))
                    ss = lane_sum(sq[:xy - 1] if 'norm_xy_1' in mut else sq, T, stop)
                if 'pooled' in mut:
                    ss = np.full(z, ss.sum(), dtype=T)
                sd = np.sqrt(ss)
                if not clean:
                    if 'no_fill_factor' not in mut:
                        sd = sd * np.sqrt(T(xy) / np.maximum(nc, 1).astype(T))
                    sd = np.where(nc > 0, sd, T(1))
                if 'no_zero_rule' not in mut:
                    sd = np.where(sd == 0, T(1), sd)
                den = sd * sqrt_z
            row = u / den
            row = np.where(on, row, v if 'unobserved_unscaled' in mut else T(0))
            r.out[q], r.mean[q], r.den[q] = row.ravel(), mean, den
    return r


def patch_bounds(img, origins, x, y, z, wm, ws, ref, dt, obs=None):
    """the bounds of the docstring for out, mean, den, from the inputs and the longdouble reference"""
    eps, xy, n = eps_of(dt), x * y, len(origins)
    S = trips(xy) + 6
    b = SimpleNamespace(out=np.zeros((n, xy * z)), mean=np.zeros((n, z)), den=np.zeros((n, z)))
    with np.errstate(invalid='ignore', divide='ignore'):
        for q, (i0, j0, c0) in enumerate(origins):
            v = img[i0:i0 + x, j0:j0 + y, c0:c0 + z].reshape(xy, z)
            on = np.ones((xy, z), dtype=bool) if obs is None else (obs[i0:i0 + x, j0:j0 + y, c0:c0 + z].reshape(xy, z) != 0)
            M = np.where(on, np.abs(v), 0.0).max(axis=0)
            nc = on.sum(axis=0)
            mean, den = ref.mean[q].astype(np.float64), ref.den[q].astype(np.float64)
            dm = S * eps * M if wm else np.zeros(z)
            rho = np.zeros(z)
            if ws:
                u = np.where(on, v - mean, 0.0)
                ss = (u * u).sum(axis=0)
                rho = (S / 2.0 + 8) * eps + np.where(ss > 0, nc * dm ** 2 / (2 * np.where(ss > 0, ss, 1.0)), 0.0)
            rr = np.abs(ref.out[q].astype(np.float64)).reshape(xy, z)
            b.out[q] = (dm / den + rr * (rho + 2 * eps)).ravel() if (wm or ws) else 0.0
            b.mean[q] = dm + eps * np.abs(mean)
            b.den[q] = den * rho
    return b


def decode_restated(code, Dt, mean, den, Cc, T, chunk=DECODE_CHUNK, mut=()):
    """decode_impl (:211-223) with EpiUnscale (:198-207): the product in T, chunk by chunk"""
    n, P = code.shape[0], Dt.shape[0]
    out = np.zeros((n, P), dtype=T)
    e = np.arange(P)
    for r0, rows in decode_chunks(n, chunk):
        v = code[r0:r0 + rows].astype(T).dot(Dt.astype(T).T)
        if mean is not None:
            s0 = 0 if 'chunk0_stats' in mut else r0
            at = (np.arange(s0, s0 + rows)[:, None] * Cc + (e // Cc if 'n_div_C' in mut else e % Cc)[None]) % mean.size
            v = v * den.astype(T).ravel()[at] + mean.astype(T).ravel()[at]
        out[r0:r0 + rows] = v
    return out


def decode_bound(code, Dt, mean, den, Cc, dt):
    k, P = code.shape[1], Dt.shape[0]
    A = np.abs(code).dot(np.abs(Dt).T)
    if mean is None:
        return (k + 8) * eps_of(dt) * A
    e = np.arange(P) % Cc
    return (k + 8) * eps_of(dt) * (np.abs(den)[:, e] * A + np.abs(mean)[:, e])


def decode_ref(code, Dt, mean, den, Cc):
    v = np.asarray(code, dtype=LD).dot(np.asarray(Dt, dtype=LD).T)
    if mean is not None:
        e = np.arange(Dt.shape[0]) % Cc
        v = v * np.asarray(den, dtype=LD)[:, e] + np.asarray(mean, dtype=LD)[:, e]
    return v


def overlap_restated(patches, g, row0, nrows, acc, use=None, cnt=None, mut=(), amut=()):
    """image_overlap_add_kernel (:234-256) / ..._weighted_kernel (:378-404) as the gather they are, on acc (H, W, C) f64 (and
    cnt (H, W) int32) in place.  Rows outside the pass's patches read as 5 (what `no_pass_clamp` finds there)."""
    H, W, Cc, x, y, si, sj = g
    gi, gj = Axis(H, x, si, amut), Axis(W, y, sj, amut)
    n = nrows * gj.g
    i_begin, i_end = gi.origin(row0), min(gi.origin(row0 + nrows - 1) + x, H)
    for i in range(i_begin, i_end):
        for j in range(W):
            r_lo, r_hi = gi.lo(i), gi.hi(i)
            if 'no_pass_clamp' not in mut:
                r_lo, r_hi = max(r_lo, row0), min(r_hi, row0 + nrows - 1)
            s = np.zeros(Cc) if 'store' in mut else acc[i, j].copy()
            added = 0
            for gr in range(r_lo, r_hi + 1):
                di = i - gi.origin(gr)
                for gc in range(gj.lo(j), gj.hi(j) + 1):
                    q, dj = (gr - row0) * gj.g + gc, j - gj.origin(gc)
                    inside = 0 <= q < n and 0 <= di < x and 0 <= dj < y
                    if use is not None and inside and not use[q]:
                        continue
                    s = s + (patches[q].reshape(x, y, Cc)[di, dj].astype(np.float64) if inside else 5.0)
                    added += 1
            acc[i, j] = s
            if cnt is not None:
                cnt[i, j] += added * (Cc if 'cnt_per_channel' in mut else 1)


def overlap_ref(patches, g, passes=None, use=None, pre=None):
    """sum, sum of magnitudes and cover count per pixel by a loop over windows (a scatter: nothing of lo / hi enters)"""
    H, W, Cc, x, y, si, sj = g
    oi, oj = brute_axis(H, x, si), brute_axis(W, y, sj)
    s = np.zeros((H, W, Cc), dtype=LD) if pre is None else np.asarray(pre, dtype=LD).copy()
    a = np.abs(s).astype(np.float64)
    cnt = np.zeros((H, W), dtype=np.int64)
    for q, (i0, j0) in enumerate((i, j) for i in oi for j in oj):
        if use is not None and not use[q]:
            continue
        w = patches[q].reshape(x, y, Cc)
        s[i0:i0 + x, j0:j0 + y] += w
        a[i0:i0 + x, j0:j0 + y] += np.abs(w)
        cnt[i0:i0 + x, j0:j0 + y] += 1
    return s, a, cnt


def finish_restated(acc, g, T, mut=()):
    """image_overlap_finish_kernel (:260-269)"""
    H, W, Cc, x, y, si, sj = g
    gi, gj = Axis(H, x, si), Axis(W, y, sj)
    ci = np.array([gi.hi(t) - gi.lo(t) + 1 for t in range(H)])
    cj = np.array([gj.hi(t) - gj.lo(t) + 1 for t in range(W)])
    cnt = np.outer(ci, cj)
    if 'count_xy_over_ss' in mut:
        cnt = np.full((H, W), (x * y) // (si * sj))
    return (acc / cnt[:, :, None].astype(np.float64)).astype(T), cnt


def inpaint_restated(acc, cnt, img, obs, keep, T):
    """image_inpaint_finish_kernel (:408-420)"""
    with np.errstate(invalid='ignore', divide='ignore'):
        q = (acc / cnt[:, :, None].astype(np.float64)).astype(T)
    take = (cnt[:, :, None] > 0) & ~((obs != 0) & bool(keep))
    return np.where(take, q, img.astype(T))


def objective_restated(X, Dt, code, chunk, T, mut=(), ldx=None):
    """objective_impl (:124-150): the residual in T, the sums in f64, one accumulation per chunk"""
    n, k = code.shape
    out = np.zeros(3)
    for r0, rows in decode_chunks(n, chunk):
        R = (X[r0:r0 + rows].astype(T) - code[r0:r0 + rows].astype(T).dot(Dt.astype(T).T)).astype(np.float64)
        out[0] = (R * R).sum() + (0.0 if 'overwrite' in mut else out[0])
    flat = np.concatenate([code.ravel(), np.full(n * max((ldx or k) - k, 0), 2.0)])
    c = flat[:n * (ldx if 'code_ldx' in mut else k)]
    out[1], out[2] = np.abs(c).sum(), (c * c).sum()
    return out


def objective_ref(X, Dt, code, dt, nchunks):
    """-> (ref (3,) longdouble, bound (3,))"""
    k = code.shape[1]
    R = np.asarray(X, dtype=LD) - np.asarray(code, dtype=LD).dot(np.asarray(Dt, dtype=LD).T)
    b = (k + 8) * eps_of(dt) * (np.abs(X) + np.abs(code).dot(np.abs(Dt).T))
    N = (24 + nchunks) * 2.0 ** -52
    Ra = np.abs(R).astype(np.float64)
    ref = np.array([(R * R).sum(), np.abs(code).astype(LD).sum(), (np.asarray(code, dtype=LD) ** 2).sum()], dtype=LD)
    bound = np.array([(2 * Ra * b + b * b).sum() + N * float(ref[0]), N * float(ref[1]), N * float(ref[2])])
    return ref, bound


# ---------------------------------------------------------------------------------------------------- the judges
FIGURES = {}


def _note(what, value):
    if np.isfinite(value):
        FIGURES[what] = max(FIGURES.get(what, 0.0), float(value))


def _report():
    print('largest |got - ref| / bound so far: ' + '; '.join('%s = %.3g' % kv for kv in sorted(FIGURES.items())))


def same_bits(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def judge_exact(got, ref, what=''):
    """the exact values, bitwise apart from the sign of zero"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    bad = np.argwhere(~(got == ref))
    assert bad.size == 0, ('not the exact result', what, bad[:4], len(bad), got[tuple(bad[0])], ref[tuple(bad[0])])


def judge_bound(got, ref, bound, who=None, what=''):
    got = np.asarray(got)
    assert np.all(np.isfinite(got)), ('non-finite result', what, np.argwhere(~np.isfinite(got))[:4])
    err = np.abs(np.asarray(got, dtype=LD) - ref).astype(np.float64)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), err.shape)
    with np.errstate(invalid='ignore', divide='ignore'):
        ratio = np.where(err == 0, 0.0, err / np.where(bound == 0, 1e-300, bound))
    if who:
        _note(who, ratio.max() if ratio.size else 0.0)
    bad = np.argwhere(ratio > 1)
    assert bad.size == 0, ('over the bound', who, what, float(ratio.max()), bad[:4], len(bad))
    return float(ratio.max()) if ratio.size else 0.0


def _rejects(f, *a, **kw):
    try:
        f(*a, **kw)
    except AssertionError:
        return True
    return False


def make_patch_case(r, dt, scene, wm, ws, origins=None, obs=None):
    sh = r.sh
    x, y = sh['x'], sh['y']
    z = sh.get('z', sh['C'])
    origins = patch_origins(sh) if origins is None else origins
    rs = np.random.RandomState(_seed(r.name, dt, scene))
    first = origins[0] if origins else None
    assert all(0 <= i <= sh['H'] - x and 0 <= j <= sh['W'] - y and 0 <= c0 <= sh['C'] - z for i, j, c0 in origins), 'a window leaves the image'
    img = scene_image(scene, rs, sh['H'], sh['W'], sh['C'], dt, first, (x, y))
    c = SimpleNamespace(name=r.name, dt=dt, scene=scene, img=img, origins=origins, x=x, y=y, z=z, wm=wm, ws=ws, obs=obs,
                        H=sh['H'], W=sh['W'], C=sh['C'], P=x * y * z)
    c.ref = window_rows(img, origins, x, y, z, wm, ws, LD, obs=obs)
    c.bound = patch_bounds(img, origins, x, y, z, wm, ws, c.ref, dt, obs=obs)
    return c


def judge_patches(c, out, mean=None, den=None, who=None):
    """rows (and the kept statistics) of a case against its longdouble reference; the exact claims of the scenes on top"""
    T = DT[c.dt]
    n, xy, z = len(c.origins), c.x * c.y, c.z
    assert out.shape == (n, c.P)
    if n == 0:
        return
    judge_bound(out, c.ref.out, c.bound.out, who, (c.name, c.scene, c.wm, c.ws, 'rows'))
    if mean is not None:
        judge_bound(mean, c.ref.mean, c.bound.mean, who and who + ' mean', (c.name, c.scene, 'mean'))
        judge_bound(den, c.ref.den, c.bound.den, who and who + ' den', (c.name, c.scene, 'den'))
        if not (c.wm or c.ws):
            assert np.all(mean == 0) and np.all(den == 1), 'no scaling: mean 0 and den 1 exactly'
        if not c.wm:
            assert np.all(mean == 0)
        if not c.ws:
            assert np.all(den == 1)
    if c.obs is None and (c.scene == 'integers' and c.wm and not c.ws and xy & (xy - 1) == 0):
        judge_exact(out, c.ref.out.astype(np.float64), (c.name, 'centred over a power-of-two count'))
    if c.scene == 'flat' and c.obs is None:
        rows = out.reshape(n, xy, z)
        sqrt_z = T(np.sqrt(float(z)))
        for q, (i0, j0, c0) in enumerate(c.origins):
            w = c.img[i0:i0 + c.x, j0:j0 + c.y, c0:c0 + z].reshape(xy, z)
            flat = np.flatnonzero((w == w[0]).all(axis=0))
            assert q > 0 or len(flat) == z, 'the first window of the flat scene is constant'
            assert c0 > 0 or 0 in flat
            if c.wm:
                assert np.all(rows[q][:, flat] == 0), ('a constant channel is not exactly 0', q)
                if mean is not None:
                    assert same_bits(mean[q][flat], w[0][flat].astype(T)), 'the mean of a constant channel is not the constant'
            if c.wm and c.ws and den is not None:
                assert np.all(den[q][flat] == sqrt_z), ('zero norm: the divisor is 1 sqrt(z)', q)
            if c.wm and c.ws:
                assert np.all(np.isfinite(rows[q]))


# ---------------------------------------------------------------------------------------------------- layer 1: no GPU
def test_route_table():
    """Every point names what the restated dispatch does there, every leaf is hit or listed in UNREACHED, both neighbours of
    every numeric boundary are in the table, and the restatement agrees with modl_amd/image.py where that restates it too."""
    HIT.clear()
    for r in POINTS:
        routes = [expected_route(r, wm, ws, pad, stats) for wm, ws in SCALINGS for pad in (0, 3) for stats in (False, True)]
        for want in r.want:
            assert any(want in s for s in routes), (r.name, want, routes[-1])
    leaves = all_leaves()
    assert len(leaves) > 40 and set(UNREACHED) <= leaves
    assert leaves - HIT == set(UNREACHED), ('no point reaches', sorted(leaves - HIT - set(UNREACHED)), 'reached after all',
                                            sorted(HIT & set(UNREACHED)))
    pt = [r.sh for r in POINTS if r.probe == 'patches']
    gr = [r.sh for r in POINTS if r.probe == 'grid']
    assert {1, 63, 64, 65, 129} <= {s['x'] * s['y'] for s in pt}                             # 64 lanes: the statistics
    assert {3, 60, 63, 64, 65, 189} <= {s['x'] * s['y'] * s['z'] for s in pt}                # ... the row
    assert {1, 3, 64, 65, 1024, 2000} <= {s['C'] for s in pt} and {1024, 1025} <= {s['z'] for s in pt}
    assert {64, 65} <= {s['C'] for s in gr if not s['masked']} and 65 in {s['C'] for s in gr if s['masked']}
    assert {0, 1, 3, 4, 5} <= {s['n'] for s in pt}                                           # 4 wavefronts
    assert {(5, 2, 0), (5, 2, 3), (3, 1, 1)} <= {(s['C'], s['z'], s['c0']) for s in pt}
    assert {DECODE_CHUNK - 1, DECODE_CHUNK, DECODE_CHUNK + 5} <= {r.sh['n'] for r in POINTS if r.probe == 'decode'}
    assert decode_chunks(DECODE_CHUNK) == [(0, DECODE_CHUNK)] and decode_chunks(DECODE_CHUNK + 5) == [(0, DECODE_CHUNK), (DECODE_CHUNK, 5)]
    ob = {r.name: r.sh for r in POINTS if r.probe == 'objective'}
    assert {OBJ_ROWS, OBJ_ROWS + 1} <= {s['n'] for s in ob.values()}
    assert ob['o-sweep-below']['n'] * 33 <= OBJ_SWEEP < ob['o-sweep-above']['n'] * 33 and ob['o-sweep-below']['n'] + 1 == ob['o-sweep-above']['n']
    for tsz in (4, 8):
        assert len(objective_chunks(8192, 33, objective_workspace(8192, 33, tsz), tsz)) == 1
        assert objective_chunks(8193, 33, objective_workspace(8193, 33, tsz), tsz) == [(0, 8192), (8192, 1)]
        assert len(objective_chunks(301, 157, 8 * OBJ_BLOCKS + tsz * 157 * 64, tsz)) == 5
        assert objective_chunks(5, 33, 8 * OBJ_BLOCKS + tsz * 33 - 1, tsz) is None
    # the grid cases of the issue, on both axes
    kinds = set()
    for s in gr:
        for L, x, st in ((s['H'], s['x'], s['si']), (s['W'], s['y'], s['sj'])):
            kinds |= {('g1', L == x), ('g2', L == x + 1 and st == x and x > 1), ('exact', (L - x) % st == 0 and L > x),
                      ('clamped', (L - x) % st != 0), ('s1', st == 1 and x > 1), ('sx', st == x and x > 1), ('x1', x == 1)}
        kinds.add(('differ', Axis(s['H'], s['x'], s['si']).kind() != Axis(s['W'], s['y'], s['sj']).kind()))
    assert {(k, True) for k in ('g1', 'g2', 'exact', 'clamped', 's1', 'sx', 'x1', 'differ')} <= kinds
    assert any((Axis(s['H'], s['x'], s['si']).g * Axis(s['W'], s['y'], s['sj']).g) % 4 for s in gr)
    # every branch of the masked window in every masked point that has the channels for it
    for r in POINTS:
        if r.probe == 'grid' and r.sh['masked']:
            got = set(masked_branches(r, grid_origins(r.sh)))
            assert got == {'masked/clean', 'masked/holed', 'masked/empty_channel', 'masked/empty_window'}, (r.name, got)
    # the Python restatements of the package
    from modl_amd import image as mi
    for L, x, s in ((10, 4, 3), (11, 5, 4), (4, 4, 1), (6, 5, 5), (5, 1, 1)):
        assert list(mi._axis_origins(L, x, s)) == brute_axis(L, x, s) == [Axis(L, x, s).origin(r) for r in range(Axis(L, x, s).g)]
    for r in POINTS:
        if r.probe == 'grid':
            g = _grid_of(r.sh)
            assert mi._grid_shape(g) == (Axis(g[0], g[3], g[5]).g, Axis(g[1], g[4], g[6]).g), r.name   # modl_image_grid_shape
            assert [tuple(o) for o in mi.grid_origins(g[:3], g[3:5], g[5:])] == grid_origins(r.sh), r.name
    assert mi._passes(5, 3, 8, 2) == [(0, 2), (2, 2), (4, 1)] and [(0, 2), (2, 2), (4, 1)] in all_cuts(5)
    assert len(all_cuts(5)) == 16 and all(sum(n for _, n in c) == 5 for c in all_cuts(5))
    assert len({r.name for r in POINTS}) == len(POINTS)


def test_grid_rule():
    """lo / hi / origin against a loop over windows, for every axis with 1 <= s <= x <= L <= 14; the wrong versions fail it"""
    def check(L, x, s, mut=()):
        a, o = Axis(L, x, s, mut), brute_axis(L, x, s)
        assert a.g == len(o) and [a.origin(r) for r in range(a.g)] == o and o[-1] == L - x
        for t in range(L):
            cover = [r for r, v in enumerate(o) if v <= t < v + x]
            assert cover == list(range(a.lo(t), a.hi(t) + 1)), (L, x, s, t, cover, a.lo(t), a.hi(t))
            assert len(cover) == a.hi(t) - a.lo(t) + 1 >= 1
    n = 0
    bad = {m: 0 for m in ('unclamped', 'lo+1', 'hi-1')}
    for L in range(1, 15):
        for x in range(1, L + 1):
            for s in range(1, x + 1):
                check(L, x, s)
                n += L
                for m in bad:
                    bad[m] += _rejects(check, L, x, s, (m,))
    assert n > 3000
    assert all(v > 100 for v in bad.values()), bad
    assert not _rejects(check, 8, 4, 2, ('unclamped',)) and _rejects(check, 9, 4, 2, ('unclamped',))   # INVISIBLE when s divides L - x
    for L, x, s in ((10, 4, 3), (9, 4, 2), (7, 4, 1)):                       # the count is not x / s once the last origin is clamped or t < x
        a = Axis(L, x, s)
        assert any(a.hi(t) - a.lo(t) + 1 != x // s for t in range(L))


def test_patches_refusal():
    """z = 1025 is MODL_EINVAL before any device work, z = 1024 with n = 0 is accepted (host pointers, no GPU)"""
    from modl_amd._lib import lib
    buf = np.zeros(64)
    q = buf.ctypes.data_as(C.c_void_p)
    sh = POINT['p-z1025'].sh
    assert expected_route(POINT['p-z1025']) == 'patches/einval'
    for sfx in BOTH:
        f = getattr(lib, 'modl_image_patches_' + sfx)
        assert f(q, 2, 2, sh['C'], q, 1, 1, 1, sh['z'], 1, 1, q, sh['z'], None) == EINVAL
        assert f(q, 2, 2, sh['C'], q, 0, 1, 1, sh['z'], 1, 1, q, sh['z'], None) == EINVAL
        assert f(q, 2, 2, sh['C'], q, 0, 1, 1, 1024, 1, 1, q, 1024, None) == 0
        assert f(q, 2, 2, sh['C'], q, 1, 1, 1, 1024, 1, 1, q, 1023, None) == EINVAL      # ldo < P
        g = getattr(lib, 'modl_objective_' + sfx)
        assert g(q, 33, 5, 33, q, 5, q, q, 8 * OBJ_BLOCKS + 33 * (4 if sfx == 'f32' else 8) - 1, q, None) == ENOMEM


def _grid_of(sh):
    return (sh['H'], sh['W'], sh['C'], sh['x'], sh['y'], sh['si'], sh['sj'])


def make_overlap_case(r, dt, scene, ldp_pad=0):
    sh = r.sh
    g = _grid_of(sh)
    gi, gj = Axis(sh['H'], sh['x'], sh['si']), Axis(sh['W'], sh['y'], sh['sj'])
    rs = np.random.RandomState(_seed(r.name, dt, scene, 'overlap'))
    n, P = gi.g * gj.g, sh['x'] * sh['y'] * sh['C']
    c = SimpleNamespace(name=r.name, dt=dt, scene=scene, g=g, gi=gi, gj=gj, n=n, P=P)
    c.patches = draw(scene, rs, (n, P), dt)
    c.pre = draw(scene, rs, (sh['H'], sh['W'], sh['C']), 'f64') * 3
    return c


def make_decode_case(r, dt, scene):
    sh = r.sh
    n, k, P, Cc = sh['n'], sh['k'], sh['P'], sh['C']
    rs = np.random.RandomState(_seed(r.name, dt, scene))
    c = SimpleNamespace(name=r.name, dt=dt, scene=scene, n=n, k=k, P=P, C=Cc)
    c.code, c.Dt = draw(scene, rs, (n, k), dt), draw(scene, rs, (P, k), dt)
    c.mean = draw(scene, rs, (n, Cc), dt) * (1 if scene == 'integers' else 100)
    c.den = rs.randint(1, 5, size=(n, Cc)).astype(np.float64) if scene == 'integers' else (0.5 + np.abs(draw(scene, rs, (n, Cc), dt))).astype(DT[dt]).astype(np.float64)
    return c


def make_objective_case(r, dt, scene):
    sh = r.sh
    n, p, k = sh['n'], sh['p'], sh['k']
    rs = np.random.RandomState(_seed(r.name, dt, scene))
    c = SimpleNamespace(name=r.name, dt=dt, scene=scene, n=n, p=p, k=k, pad=sh['pad'])
    c.X, c.code, c.Dt = draw(scene, rs, (n, p), dt), draw(scene, rs, (n, k), dt), draw(scene, rs, (p, k), dt)
    tsz = np.dtype(DT[dt]).itemsize
    c.ws = objective_workspace(n, p, tsz) if sh['ws_rows'] is None else 8 * OBJ_BLOCKS + tsz * p * sh['ws_rows']
    c.chunks = objective_chunks(n, p, c.ws, tsz)
    return c


def judge_objective(c, out3, who=None):
    if c.scene == 'integers':
        R = c.X - c.code.dot(c.Dt.T)
        judge_exact(out3, np.array([(R * R).sum(), np.abs(c.code).sum(), (c.code * c.code).sum()]), (c.name, 'integers'))
    else:
        ref, bound = objective_ref(c.X, c.Dt, c.code, c.dt, len(c.chunks))
        judge_bound(out3, ref, bound, who, c.name)


@pytest.mark.parametrize('dt', BOTH)
def test_judges_on_the_oracle(dt):
    """The same-dtype numpy restatement of every kernel is within the bound on every scene and shape of the table."""
    T = DT[dt]
    worst = {}

    def note(what, v):
        worst[what] = max(worst.get(what, 0.0), v)
    for r in POINTS:
        sh = r.sh
        if r.probe == 'patches' and not sh.get('host') and sh['n']:
            for scene in sh['scenes']:
                for wm, ws in SCALINGS:
                    c = make_patch_case(r, dt, scene, wm, ws)
                    got = window_rows(c.img, c.origins, c.x, c.y, c.z, wm, ws, T)
                    assert got.out.dtype == T
                    judge_patches(c, got.out, got.mean, got.den)
                    note('patches', judge_bound(got.out, c.ref.out, c.bound.out))
        elif r.probe == 'grid':
            obs = masked_obs(r) if sh['masked'] else None
            for scene in ('gaussian', 'offset', 'scales'):
                for wm, ws in SCALINGS:
                    c = make_patch_case(r, dt, scene, wm, ws, origins=grid_origins(sh), obs=obs)
                    got = window_rows(c.img, c.origins, c.x, c.y, c.z, wm, ws, T, obs=obs)
                    judge_patches(c, got.out, got.mean, got.den)
                    note('masked' if sh['masked'] else 'grid', judge_bound(got.out, c.ref.out, c.bound.out))
            if not sh['masked']:
                for scene in ('integers', 'gaussian'):
                    c = make_overlap_case(r, dt, scene)
                    acc = c.pre.copy()
                    overlap_restated(c.patches, c.g, 0, c.gi.g, acc)
                    s, a, cnt = overlap_ref(c.patches, c.g, pre=c.pre)
                    fin, fcnt = finish_restated(acc, c.g, T)
                    assert np.array_equal(fcnt, cnt)
                    if scene == 'integers':
                        judge_exact(acc, s.astype(np.float64))
                    note('overlap', judge_bound(acc, s, (cnt[:, :, None] + 1) * 2.0 ** -52 * a))
                    note('finish', judge_bound(fin, np.asarray(acc, dtype=LD) / cnt[:, :, None], eps_of(dt) * np.abs(acc / cnt[:, :, None])))
        elif r.probe == 'decode' and not sh['big'] and sh['n']:
            for scene in ('integers', 'gaussian'):
                c = make_decode_case(r, dt, scene)
                for mean, den in ((None, None), (c.mean, c.den)):
                    got = decode_restated(c.code, c.Dt, mean, den, c.C, T)
                    ref = decode_ref(c.code, c.Dt, mean, den, c.C)
                    if scene == 'integers':
                        judge_exact(got, ref.astype(np.float64))
                    note('decode', judge_bound(got, ref, decode_bound(c.code, c.Dt, mean, den, c.C, dt)))
        elif r.probe == 'objective' and sh['n'] and r.name != 'o-enomem':
            for scene in ('integers', 'gaussian'):
                c = make_objective_case(r, dt, scene)
                got = objective_restated(c.X, c.Dt, c.code, c.chunks[0][1], T)
                judge_objective(c, got)
                if scene == 'gaussian':
                    ref, bound = objective_ref(c.X, c.Dt, c.code, dt, len(c.chunks))
                    note('objective', judge_bound(got, ref, bound))
    print('%s: same-dtype restatement / bound, largest: %s' % (dt, '; '.join('%s %.3g' % kv for kv in sorted(worst.items()))))
    assert set(worst) == {'patches', 'grid', 'masked', 'overlap', 'finish', 'decode', 'objective'} and all(v > 0 for v in worst.values())


def test_mutants():
    """Every wrong restatement is rejected by the scene and shape the docstring names; where one is invisible by
    construction, that is asserted."""
    def patches_ok(c, mut=()):
        got = window_rows(c.img, c.origins, c.x, c.y, c.z, c.wm, c.ws, DT[c.dt], obs=c.obs, mut=mut)
        judge_patches(c, got.out, got.mean, got.den)
        return got

    def case(name, dt, scene, wm=1, ws=1, **kw):
        return make_patch_case(POINT[name], dt, scene, wm, ws, **kw)

    for dt in BOTH:
        assert _rejects(patches_ok, case('p-xy65', dt, 'gaussian'), ('stop64',))
        patches_ok(case('p-xy64', dt, 'gaussian'), ('stop64',))                             # INVISIBLE at xy <= 64
        assert _rejects(patches_ok, case('p-P60', dt, 'scales'), ('pooled',))
        patches_ok(case('p-xy64', dt, 'scales'), ('pooled',))                               # INVISIBLE at z = 1
        assert _rejects(patches_ok, case('p-z2-c0', dt, 'gaussian'), ('sqrtC',))
        patches_ok(case('p-P60', dt, 'gaussian'), ('sqrtC',))                               # INVISIBLE at z == C
        assert _rejects(patches_ok, case('p-P60', dt, 'gaussian'), ('norm_xy_1',))
        assert _rejects(patches_ok, case('p-xy129', dt, 'gaussian'), ('norm_xy_1',))
        assert _rejects(patches_ok, case('p-P60', dt, 'offset'), ('one_pass',))
        assert _rejects(patches_ok, case('p-xy65', dt, 'offset'), ('one_pass',))
        assert _rejects(patches_ok, case('p-P60', dt, 'flat'), ('no_zero_rule',))
        patches_ok(case('p-P60', dt, 'gaussian'), ('no_zero_rule',))                        # INVISIBLE without a constant channel
        assert _rejects(patches_ok, case('p-P60', dt, 'gaussian', origins=[(0, 0, 0), (1, 2, 0)]), ('yx',))
        patches_ok(case('p-xy1', dt, 'gaussian'), ('yx',))                                  # INVISIBLE at (1, 1)
        assert _rejects(patches_ok, case('p-z2-c3', dt, 'gaussian'), ('drop_c0',))
        patches_ok(case('p-z2-c0', dt, 'gaussian'), ('drop_c0',))                           # INVISIBLE at c0 = 0
        m = POINT['m-4x5']
        obs, org = masked_obs(m), grid_origins(m.sh)
        holed = [o for o, b in zip(org, masked_branches(m, org)) if b == 'masked/holed'][:1]
        clean = [o for o, b in zip(org, masked_branches(m, org)) if b == 'masked/clean'][:1]
        patches_ok(case('m-4x5', dt, 'gaussian', origins=org, obs=obs))
        for mut in ('holed_all_stats', 'no_fill_factor', 'unobserved_unscaled'):
            assert _rejects(patches_ok, case('m-4x5', dt, 'gaussian', origins=holed, obs=obs), (mut,)), mut
            patches_ok(case('m-4x5', dt, 'gaussian', origins=clean, obs=obs), (mut,))       # INVISIBLE in a clean window
        patches_ok(case('m-4x5', dt, 'gaussian', 1, 0, origins=holed, obs=obs), ('no_fill_factor',))   # INVISIBLE without with_std
        c = case('m-4x5', dt, 'gaussian', origins=holed, obs=obs)
        c.img = c.img.copy()
        c.img[obs == 0] = np.nan                                                            # poison: the same bits from the restatement,
        assert same_bits(patches_ok(c).out, patches_ok(case('m-4x5', dt, 'gaussian', origins=holed, obs=obs)).out)
        assert not np.all(np.isfinite(window_rows(c.img, holed, 4, 5, 3, 1, 1, DT[dt], obs=obs, mut=('unobserved_unscaled',)).out))
        # decode
        r = SimpleNamespace(name='mut-decode', sh=dict(n=13, k=3, P=6, C=3))
        for scene in ('integers', 'gaussian'):
            c = make_decode_case(r, dt, scene)
            ref, bound = decode_ref(c.code, c.Dt, c.mean, c.den, 3), decode_bound(c.code, c.Dt, c.mean, c.den, 3, dt)
            judge_bound(decode_restated(c.code, c.Dt, c.mean, c.den, 3, DT[dt], chunk=8), ref, bound)
            assert _rejects(judge_bound, decode_restated(c.code, c.Dt, c.mean, c.den, 3, DT[dt], chunk=8, mut=('chunk0_stats',)), ref, bound)
            judge_bound(decode_restated(c.code, c.Dt, c.mean, c.den, 3, DT[dt], chunk=16, mut=('chunk0_stats',)), ref, bound)   # INVISIBLE in one chunk
            assert _rejects(judge_bound, decode_restated(c.code, c.Dt, c.mean, c.den, 3, DT[dt], mut=('n_div_C',)), ref, bound)
    # grid and overlap-add (f64 accumulators whatever the dtype)
    r = POINT['g-exact-clamped']
    c = make_overlap_case(r, 'f64', 'integers')
    s, _, cnt = overlap_ref(c.patches, c.g, pre=c.pre)
    s0 = overlap_ref(c.patches, c.g)[0]

    def overlap_ok(cuts, pre=True, use=None, **kw):
        acc = c.pre.copy() if pre else np.zeros_like(c.pre)
        cn = np.zeros(c.pre.shape[:2], dtype=np.int32)
        for row0, nrows in cuts:
            lo = row0 * c.gj.g
            overlap_restated(c.patches[lo:lo + nrows * c.gj.g], c.g, row0, nrows, acc, use=None if use is None else use[lo:], cnt=cn, **kw)
        judge_exact(acc, (s if pre else s0).astype(np.float64))
        assert np.array_equal(cn, cnt), 'cnt'
    whole, single = [(0, c.gi.g)], [(i, 1) for i in range(c.gi.g)]
    for cuts in all_cuts(c.gi.g):
        overlap_ok(cuts)
    for m in ('unclamped', 'lo+1', 'hi-1'):
        assert _rejects(overlap_ok, whole, amut=(m,)), m
    assert _rejects(overlap_ok, whole, mut=('store',)) and _rejects(overlap_ok, single, mut=('store',))
    overlap_ok(whole, pre=False, mut=('store',))                                            # INVISIBLE on a zero accumulator, one pass
    assert _rejects(overlap_ok, single, pre=False, mut=('store',))
    assert _rejects(overlap_ok, single, mut=('no_pass_clamp',))
    overlap_ok(whole, mut=('no_pass_clamp',))                                               # INVISIBLE in the full call
    assert _rejects(overlap_ok, whole, use=np.ones(c.n, dtype=np.uint8), mut=('cnt_per_channel',))
    c1 = make_overlap_case(POINT['g-clamped-exact-C1'], 'f64', 'integers')
    cn, cn_m = np.zeros(c1.pre.shape[:2], dtype=np.int32), np.zeros(c1.pre.shape[:2], dtype=np.int32)
    overlap_restated(c1.patches, c1.g, 0, c1.gi.g, c1.pre.copy(), cnt=cn)
    overlap_restated(c1.patches, c1.g, 0, c1.gi.g, c1.pre.copy(), cnt=cn_m, mut=('cnt_per_channel',))
    assert np.array_equal(cn, cn_m)                                                         # INVISIBLE at C 1
    fcnt = finish_restated(s.astype(np.float64), c.g, np.float64, ('count_xy_over_ss',))[1]
    assert not np.array_equal(fcnt, cnt)
    # objective
    r = SimpleNamespace(name='mut-objective', sh=dict(n=13, p=7, k=3, ws_rows=8, pad=2))
    c = make_objective_case(r, 'f64', 'integers')
    judge_objective(c, objective_restated(c.X, c.Dt, c.code, 8, np.float64, ldx=5))
    assert _rejects(judge_objective, c, objective_restated(c.X, c.Dt, c.code, 8, np.float64, ('overwrite',)))
    judge_objective(c, objective_restated(c.X, c.Dt, c.code, 13, np.float64, ('overwrite',)))              # INVISIBLE with one chunk
    assert _rejects(judge_objective, c, objective_restated(c.X, c.Dt, c.code, 8, np.float64, ('code_ldx',), ldx=5))
    judge_objective(c, objective_restated(c.X, c.Dt, c.code, 8, np.float64, ('code_ldx',), ldx=3))         # INVISIBLE at ldx == k


# ---------------------------------------------------------------------------------------------------- layer 2: the ABI on the device
GUARD = 64


@pytest.fixture(scope='module')
def gpu():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    return torch.device('cuda', 0)


def _tdt(dt):
    import torch
    return {'f32': torch.float32, 'f64': torch.float64, 'u8': torch.uint8, 'i32': torch.int32, 'i64': torch.int64}[dt]


class Buf:
    """a device buffer of `shape` between two runs of GUARD sentinel elements; loose rows carry the sentinel too"""
    def __init__(self, shape, dt, dev, fill=FILL):
        import torch
        self.shape, self.n, self.fill = tuple(shape), int(np.prod(shape)), fill
        self.raw = torch.full((self.n + 2 * GUARD,), fill, dtype=_tdt(dt), device=dev)
        self.t = self.raw[GUARD:GUARD + self.n].view(self.shape)

    def set(self, a):
        import torch
        self.t.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(self.t.dtype))
        return self

    @property
    def p(self):
        return C.c_void_p(self.t.data_ptr())

    def get(self, cols=None):
        """the host copy; asserts that the guards (and the columns from `cols` on) keep the sentinel"""
        raw = self.raw.cpu().numpy()
        assert np.all(raw[:GUARD] == self.fill) and np.all(raw[GUARD + self.n:] == self.fill), 'a guard word was written'
        a = raw[GUARD:GUARD + self.n].reshape(self.shape)
        if cols is not None:
            assert np.all(a[..., cols:] == self.fill), 'the padding behind a row was written'
            a = a[..., :cols]
        return a.copy()


def _dev(a, dt, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype={'u8': np.uint8, 'i64': np.int64, 'i32': np.int32}.get(dt) or DT[dt])).to(dev)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _twice(call, outs):
    """the call twice on fresh outputs: identical bits; -> the first call's host copies"""
    import torch
    res = []
    for _ in range(2):
        bufs = outs()
        assert call(*bufs) == 0
        torch.cuda.synchronize()
        res.append(bufs)
    return res


def run_patches(c, dev, pad=0, origins=None):
    """modl_image_patches_* on the case -> out (n, P)"""
    from modl_amd._lib import lib
    f = getattr(lib, 'modl_image_patches_' + c.dt)
    origins = c.origins if origins is None else origins
    n, ldo = len(origins), c.P + pad
    img = _dev(c.img, c.dt, dev)
    idx = _dev(np.array(origins, dtype=np.int64).reshape(-1, 3) if n else np.zeros((1, 3)), 'i64', dev)
    before = img.cpu().numpy().tobytes()
    got = _twice(lambda o: f(_ptr(img), c.H, c.W, c.C, _ptr(idx), n, c.x, c.y, c.z, c.wm, c.ws, o.p, ldo, None),
                 lambda: (Buf((max(n, 1), ldo), c.dt, dev),))
    a, b = (g[0].get(c.P if n else 0) for g in got)
    assert same_bits(a, b), 'a second identical call gave other bits'
    assert before == img.cpu().numpy().tobytes(), 'the image was written'
    return a[:n] if n else np.zeros((0, c.P), dtype=DT[c.dt])


def run_grid(c, sh, dev, row0=0, nrows=None, pad=0, obs=None, img=None):
    """modl_image_grid_patches_* (obs None) or ..._masked_* -> (out, mean, den[, obs_out, nobs]) of the pass"""
    from modl_amd._lib import lib
    gi, gj = Axis(sh['H'], sh['x'], sh['si']), Axis(sh['W'], sh['y'], sh['sj'])
    nrows = gi.g if nrows is None else nrows
    n, ldo, Cc = nrows * gj.g, c.P + pad, sh['C']
    imgd = _dev(c.img if img is None else img, c.dt, dev)
    head = (_ptr(imgd), sh['H'], sh['W'], Cc, sh['x'], sh['y'], sh['si'], sh['sj'], row0, nrows, c.wm, c.ws)
    if obs is None:
        f = getattr(lib, 'modl_image_grid_patches_' + c.dt)
        got = _twice(lambda o, m, d: f(*head, o.p, ldo, m.p, d.p, None),
                     lambda: (Buf((n, ldo), c.dt, dev), Buf((n, Cc), c.dt, dev), Buf((n, Cc), c.dt, dev)))
    else:
        f = getattr(lib, 'modl_image_grid_patches_masked_' + c.dt)
        od = _dev(obs, 'u8', dev)
        got = _twice(lambda o, m, d, oo, no: f(*head, o.p, ldo, m.p, d.p, _ptr(od), oo.p, no.p, None),
                     lambda: (Buf((n, ldo), c.dt, dev), Buf((n, Cc), c.dt, dev), Buf((n, Cc), c.dt, dev),
                              Buf((n, c.P), 'u8', dev, 9), Buf((n,), 'i32', dev, -7)))
    a, b = ([g[0].get(c.P)] + [t.get() for t in g[1:]] for g in got)
    assert all(same_bits(u, v) for u, v in zip(a, b)), 'a second identical call gave other bits'
    return a


def run_patches_masked(c, sh, dev, origins, obs, pad=0, img=None):
    from modl_amd._lib import lib
    f = getattr(lib, 'modl_image_patches_masked_' + c.dt)
    n, ldo, Cc = len(origins), c.P + pad, sh['C']
    imgd, od, idx = _dev(c.img if img is None else img, c.dt, dev), _dev(obs, 'u8', dev), _dev(np.array(origins), 'i64', dev)
    got = _twice(lambda o, m, d, oo, no: f(_ptr(imgd), sh['H'], sh['W'], Cc, _ptr(idx), n, sh['x'], sh['y'], Cc, c.wm, c.ws, o.p, ldo,
                                           m.p, d.p, _ptr(od), oo.p, no.p, None),
                 lambda: (Buf((n, ldo), c.dt, dev), Buf((n, Cc), c.dt, dev), Buf((n, Cc), c.dt, dev),
                          Buf((n, c.P), 'u8', dev, 9), Buf((n,), 'i32', dev, -7)))
    a, b = ([g[0].get(c.P)] + [t.get() for t in g[1:]] for g in got)
    assert all(same_bits(u, v) for u, v in zip(a, b)), 'a second identical call gave other bits'
    return a


PATCH_POINTS = [(r.name, dt) for r in POINTS if r.probe == 'patches' and not r.sh.get('host') for dt in BOTH]


@pytest.mark.gpu
@pytest.mark.parametrize('name,dt', PATCH_POINTS, ids=['%s-%s' % c for c in PATCH_POINTS])
def test_patches(gpu, name, dt):
    """modl_image_patches_*: every scaling at every point, tight and loose rows, judged per element"""
    r = POINT[name]
    for scene in r.sh['scenes']:
        for wm, ws in SCALINGS:
            c = make_patch_case(r, dt, scene, wm, ws)
            out = run_patches(c, gpu)
            judge_patches(c, out, who='patches ' + dt)
            if not (wm or ws) and len(c.origins):
                assert same_bits(out, c.ref.out.astype(DT[dt])), 'no scaling: the bits of the pixels'
            assert same_bits(run_patches(c, gpu, pad=3), out), 'ldo = P + 3 gave other bits'
            if len(c.origins) > 4:                                           # a patch's bits do not depend on its slot
                assert same_bits(run_patches(c, gpu, origins=c.origins[::-1]), out[::-1])
                assert same_bits(out[2], out[4]), 'a duplicate origin gave other bits'
    _report()


GRID_POINTS = [(r.name, dt) for r in POINTS if r.probe == 'grid' and not r.sh['masked'] for dt in BOTH]
MASKED_POINTS = [(r.name, dt) for r in POINTS if r.probe == 'grid' and r.sh['masked'] for dt in BOTH]
WEIGHTED_POINTS = [(r.name, dt) for r in POINTS if r.probe == 'grid' and r.sh['weighted'] for dt in BOTH]


@pytest.mark.gpu
@pytest.mark.parametrize('name,dt', GRID_POINTS, ids=['%s-%s' % c for c in GRID_POINTS])
def test_grid_patches(gpu, name, dt):
    """modl_image_grid_patches_*: the origins of the grid rule, the statistics kept, the bits of the index-list kernel, and
    every pass the bits of the full call"""
    r = POINT[name]
    sh = r.sh
    org = grid_origins(sh)
    gi, gj = Axis(sh['H'], sh['x'], sh['si']), Axis(sh['W'], sh['y'], sh['sj'])
    for scene in ('gaussian', 'offset', 'flat', 'scales'):
        for wm, ws in SCALINGS:
            c = make_patch_case(r, dt, scene, wm, ws, origins=org)
            out, mean, den = run_grid(c, sh, gpu)
            judge_patches(c, out, mean, den, who='grid ' + dt)
            assert same_bits(run_patches(c, gpu), out), 'the index-list kernel on the same origins gave other bits'
            if scene != 'gaussian':
                continue
            loose = run_grid(c, sh, gpu, pad=3)
            assert all(same_bits(u, v) for u, v in zip(loose, (out, mean, den))), 'ldo = P + 3 gave other bits'
            cuts = [[(i, 1) for i in range(gi.g)]] + ([[(0, 2), (2, gi.g - 2)]] if gi.g > 2 else [])
            for row0, nrows in (p for cut in cuts for p in cut):
                lo, hi = row0 * gj.g, (row0 + nrows) * gj.g
                part = run_grid(c, sh, gpu, row0, nrows)
                assert all(same_bits(u, v[lo:hi]) for u, v in zip(part, (out, mean, den))), ('a pass gave other bits', row0, nrows)
    _report()


def _poisoned(img, obs):
    img = img.copy()
    hole = np.argwhere(obs == 0)
    img[tuple(hole[0::2].T)] = np.nan
    img[tuple(hole[1::2].T)] = np.inf
    return img


@pytest.mark.gpu
@pytest.mark.parametrize('name,dt', MASKED_POINTS, ids=['%s-%s' % c for c in MASKED_POINTS])
def test_masked_windows(gpu, name, dt):
    """the two masked window kernels: every branch, mask bytes, poison, and each other's bits"""
    r = POINT[name]
    sh = r.sh
    org, obs = grid_origins(sh), masked_obs(r)
    branches = masked_branches(r, org)
    clean = np.array([b == 'masked/clean' for b in branches])
    gj = Axis(sh['W'], sh['y'], sh['sj'])
    for scene in ('gaussian', 'offset', 'scales'):
        for wm, ws in SCALINGS:
            c = make_patch_case(r, dt, scene, wm, ws, origins=org, obs=obs)
            got = run_grid(c, sh, gpu, obs=obs)
            out, mean, den, oo, nobs = got
            judge_patches(c, out, mean, den, who='masked ' + dt)
            assert np.array_equal(oo, c.ref.obs_out) and set(np.unique(oo)) <= {0, 1}, 'obs_out is the window of the mask, 0 / 1'
            assert np.array_equal(nobs, c.ref.nobs), 'nobs'
            assert np.all(out[oo == 0] == 0), 'an unobserved element is not 0'
            plain = run_grid(c, sh, gpu)
            assert all(same_bits(u[clean], v[clean]) for u, v in zip(got[:3], plain)), 'a clean window is not the unmasked kernel\'s bits'
            twin = run_patches_masked(c, sh, gpu, org, obs)
            assert all(same_bits(u, v) for u, v in zip(twin, got)), 'grid kernel and index-list kernel differ on the same origins'
            if scene != 'gaussian':
                continue
            back = run_patches_masked(c, sh, gpu, org[::-1] + org[:1], obs, pad=3)
            assert all(same_bits(u[:-1], v[::-1]) and same_bits(u[-1], v[0]) for u, v in zip(back, got)), 'descending origins, loose rows'
            by = masked_obs(r, np.random.RandomState(_seed(name, 'bytes')))
            assert {1, 2, 0x80, 0xFF} <= set(np.unique(by)) and np.array_equal(by != 0, obs != 0)
            assert all(same_bits(u, v) for u, v in zip(run_grid(c, sh, gpu, obs=by), got)), 'bytes other than 1 changed the result'
            assert all(same_bits(u, v) for u, v in zip(run_patches_masked(c, sh, gpu, org, by), got)), 'bytes other than 1 (index list)'
            pz = _poisoned(c.img, obs)
            for res in (run_grid(c, sh, gpu, obs=obs, img=pz, pad=3), run_patches_masked(c, sh, gpu, org, obs, img=pz)):
                assert all(same_bits(u, v) for u, v in zip(res, got)), 'the poison changed the result'
                assert all(np.all(np.isfinite(u)) for u in res[:3])
            part = run_grid(c, sh, gpu, 1, 2, obs=obs)
            assert all(same_bits(u, v[gj.g:3 * gj.g]) for u, v in zip(part, got)), 'a pass gave other bits'
    _report()


def run_decode(c, dev, mean, den, pad=0):
    from modl_amd._lib import lib
    f = getattr(lib, 'modl_image_decode_' + c.dt)
    ldo = c.P + pad
    code, Dt = _dev(c.code if c.n else np.zeros((1, c.k)), c.dt, dev), _dev(c.Dt, c.dt, dev)
    md, dd = (None, None) if mean is None else (_dev(mean, c.dt, dev), _dev(den, c.dt, dev))
    got = _twice(lambda o: f(_ptr(code), c.n, c.k, _ptr(Dt), c.P, c.C, _ptr(md), _ptr(dd), o.p, ldo, None),
                 lambda: (Buf((max(c.n, 1), ldo), c.dt, dev),))
    a, b = (g[0].get(c.P if c.n else 0) for g in got)
    assert same_bits(a, b), 'a second identical call gave other bits'
    return a[:c.n] if c.n else np.zeros((0, c.P), dtype=DT[c.dt])


DECODE_POINTS = [(r.name, dt) for r in POINTS if r.probe == 'decode' and not r.sh['big'] for dt in BOTH]
DECODE_BIG = [(r.name, dt) for r in POINTS if r.probe == 'decode' and r.sh['big'] for dt in BOTH]


@pytest.mark.gpu
@pytest.mark.parametrize('name,dt', DECODE_POINTS, ids=['%s-%s' % c for c in DECODE_POINTS])
def test_decode(gpu, name, dt):
    """modl_image_decode_*: the plain product and the unscaled one, C = 1, 1 < C < P, C = P; tight and loose rows"""
    r = POINT[name]
    for scene in ('integers', 'gaussian'):
        c = make_decode_case(r, dt, scene)
        for mean, den in ((None, None), (c.mean, c.den)):
            out = run_decode(c, gpu, mean, den)
            if c.n == 0:
                continue
            ref = decode_ref(c.code, c.Dt, mean, den, c.C)
            if scene == 'integers':
                judge_exact(out, ref.astype(np.float64), name)
            judge_bound(out, ref, decode_bound(c.code, c.Dt, mean, den, c.C, dt), 'decode ' + dt, name)
            assert same_bits(run_decode(c, gpu, mean, den, pad=3), out), 'ldo = P + 3 gave other bits'
    _report()


@pytest.mark.gpu
@pytest.mark.parametrize('name,dt', DECODE_BIG, ids=['%s-%s' % c for c in DECODE_BIG])
def test_decode_chunks(gpu, name, dt):
    """n on both sides of 2^21 rows: the second launch reads code, mean, den and writes out at row 2^21.  Integers (exact);
    the statistics of the rows from 2^21 on differ from those of the rows from 0 on."""
    import torch
    from modl_amd._lib import lib
    sh = POINT[name].sh
    n, T = sh['n'], DT[dt]
    m = np.arange(n)
    code = ((m % 7) - 3).astype(T).reshape(n, 1)
    Dt = np.array([[2.0], [-3.0]], dtype=T)
    mean = np.stack([(m % 5) - 2 + 10 * (m >= DECODE_CHUNK), (m % 3) + 20 * (m >= DECODE_CHUNK)], axis=1).astype(T)
    den = np.stack([1 + (m % 4) + 4 * (m >= DECODE_CHUNK), 2 + (m % 2) + 8 * (m >= DECODE_CHUNK)], axis=1).astype(T)
    want = (code * Dt.T) * den + mean
    assert want.dtype == T
    if n > DECODE_CHUNK:
        assert not np.array_equal(mean[:5], mean[DECODE_CHUNK:]) and not np.array_equal(den[:5], den[DECODE_CHUNK:])
    f = getattr(lib, 'modl_image_decode_' + dt)
    cd, Dd, md, dd = (torch.from_numpy(a).to(gpu) for a in (code, Dt, mean, den))
    outs = []
    for _ in range(2):
        out = Buf((n, 2), dt, gpu)
        assert f(_ptr(cd), n, 1, _ptr(Dd), 2, 2, _ptr(md), _ptr(dd), out.p, 2, None) == 0
        torch.cuda.synchronize()
        outs.append(out.get())
    assert same_bits(outs[0], outs[1]), 'a second identical call gave other bits'
    bad = np.flatnonzero((outs[0] != want).any(axis=1))
    assert bad.size == 0, ('rows of the decode differ', bad[:4], len(bad))


def run_overlap(c, dev, cuts, pre=None, pad=0, use=None, cnt0=None, patches=None):
    """modl_image_overlap_add_* (use None) or ..._weighted_* pass by pass onto one accumulator -> acc (H, W, C)[, cnt (H, W)]"""
    import torch
    from modl_amd._lib import lib
    H, W, Cc, x, y, si, sj = c.g
    f = getattr(lib, 'modl_image_overlap_add_' + ('weighted_' if use is not None else '') + c.dt)
    res = []
    pt = np.full((c.n, c.P + pad), np.nan)
    pt[:, :c.P] = c.patches if patches is None else patches
    pd = _dev(pt, c.dt, dev)
    ud = None if use is None else _dev(use, 'u8', dev)
    for _ in range(2):
        acc = Buf((H, W, Cc), 'f64', dev).set(np.zeros((H, W, Cc)) if pre is None else pre)
        cnt = Buf((H, W), 'i32', dev, -7).set(np.zeros((H, W)) if cnt0 is None else cnt0)
        for row0, nrows in cuts:
            at = C.c_void_p(pd.data_ptr() + row0 * c.gj.g * (c.P + pad) * pd.element_size())
            if use is None:
                assert f(at, c.P + pad, H, W, Cc, x, y, si, sj, row0, nrows, acc.p, None) == 0
            else:
                ua = C.c_void_p(ud.data_ptr() + row0 * c.gj.g)
                assert f(at, c.P + pad, H, W, Cc, x, y, si, sj, row0, nrows, acc.p, ua, cnt.p, None) == 0
        torch.cuda.synchronize()
        res.append((acc.get(), cnt.get()))
    assert same_bits(res[0][0], res[1][0]) and same_bits(res[0][1], res[1][1]), 'a second identical run gave other bits'
    return res[0] if use is not None else res[0][0]


def run_finish(c, dev, acc):
    import torch
    from modl_amd._lib import lib
    H, W, Cc, x, y, si, sj = c.g
    f = getattr(lib, 'modl_image_overlap_finish_' + c.dt)
    ad = _dev(acc, 'f64', dev)
    res = []
    for _ in range(2):
        out = Buf((H, W, Cc), c.dt, dev)
        assert f(_ptr(ad), H, W, Cc, x, y, si, sj, out.p, None) == 0
        torch.cuda.synchronize()
        res.append(out.get())
    assert same_bits(*res)
    return res[0]


@pytest.mark.gpu
@pytest.mark.parametrize('name,dt', GRID_POINTS, ids=['%s-%s' % c for c in GRID_POINTS])
def test_overlap(gpu, name, dt):
    """overlap-add and finish: the sums of a loop over windows, accumulated onto a pre-loaded accumulator, the same bits
    for every cut into passes, pixel rows outside a pass untouched, the count of the brute-force cover"""
    r = POINT[name]
    for scene in ('integers', 'gaussian'):
        c = make_overlap_case(r, dt, scene)
        s, a, cnt = overlap_ref(c.patches, c.g, pre=c.pre)
        whole = [(0, c.gi.g)]
        acc = run_overlap(c, gpu, whole, pre=c.pre)
        if scene == 'integers':
            judge_exact(acc, s.astype(np.float64), name)
        judge_bound(acc, s, (cnt[:, :, None] + 1) * 2.0 ** -52 * a, 'overlap ' + dt, name)
        assert same_bits(run_overlap(c, gpu, whole, pre=c.pre, pad=3), acc), 'ldp = P + 3 gave other bits'
        for cuts in all_cuts(c.gi.g)[1:]:
            assert same_bits(run_overlap(c, gpu, cuts, pre=c.pre), acc), ('a cut into passes gave other bits', cuts)
        if c.gi.g > 1:                                                       # one pass alone: the rows it does not cover keep their bits
            row0 = c.gi.g - 1
            one = run_overlap(c, gpu, [(row0, 1)], pre=c.pre)
            i_begin = c.gi.origin(row0)
            assert i_begin > 0 and same_bits(one[:i_begin], c.pre[:i_begin]), 'a pixel row outside the pass was written'
            first = run_overlap(c, gpu, [(0, 1)], pre=c.pre)
            assert same_bits(first[c.g[3]:], c.pre[c.g[3]:]), 'a pixel row outside the pass was written'
        fin = run_finish(c, gpu, acc)
        T = DT[dt]
        if scene == 'integers':                                              # the pass list of modl_amd/image.py (`_passes`) on the device
            from modl_amd import image as mi
            H, W, Cc, x, y, si, sj = c.g
            zero = run_finish(c, gpu, run_overlap(c, gpu, whole))
            for rpp in (None, 1, 2):
                got = mi.reconstruct_from_patches(c.patches.astype(T), (H, W, Cc), (x, y), (si, sj), rows_per_pass=rpp)
                assert got.dtype == T and same_bits(got, zero), ('reconstruct_from_patches differs from the ABI', rpp)
        with np.errstate(over='ignore'):
            assert same_bits(fin, (acc / cnt[:, :, None].astype(np.float64)).astype(T)), 'finish: acc / cover count, rounded once'
        judge_bound(fin, np.asarray(acc, dtype=LD) / cnt[:, :, None], eps_of(dt) * np.abs(acc / cnt[:, :, None]), 'finish ' + dt, name)
    _report()


@pytest.mark.gpu
@pytest.mark.parametrize('name,dt', WEIGHTED_POINTS, ids=['%s-%s' % c for c in WEIGHTED_POINTS])
def test_weighted_overlap_and_inpaint_finish(gpu, name, dt):
    """the weighted overlap-add over use bytes and the inpaint finish"""
    import torch
    from modl_amd._lib import lib
    r = POINT[name]
    T = DT[dt]
    c = make_overlap_case(r, dt, 'integers')
    H, W, Cc = c.g[:3]
    rs = np.random.RandomState(_seed(name, dt, 'use'))
    whole, single = [(0, c.gi.g)], [(i, 1) for i in range(c.gi.g)]
    cnt0 = rs.randint(0, 5, size=(H, W)).astype(np.int32)
    # all 0: acc and cnt keep their bits, and no row is read (NaN everywhere)
    acc, cnt = run_overlap(c, gpu, whole, pre=c.pre, use=np.zeros(c.n, dtype=np.uint8), cnt0=cnt0, patches=np.full((c.n, c.P), np.nan))
    assert same_bits(acc, c.pre) and np.array_equal(cnt, cnt0), 'use all 0 changed acc or cnt'
    # all 1: the bits of the unweighted kernel, cnt the cover count
    s, a, cover = overlap_ref(c.patches, c.g, pre=c.pre)
    acc, cnt = run_overlap(c, gpu, whole, pre=c.pre, use=np.ones(c.n, dtype=np.uint8))
    assert same_bits(acc, run_overlap(c, gpu, whole, pre=c.pre)) and np.array_equal(cnt, cover), 'use all 1'
    judge_exact(acc, s.astype(np.float64), name)
    # mixed, bytes, NaN in the unused rows, every cut, a pre-loaded cnt
    use = (rs.rand(c.n) < 0.6).astype(np.uint8)
    use[0], use[-1] = 1, 0
    s, a, cover = overlap_ref(c.patches, c.g, use=use, pre=c.pre)
    poisoned = np.where(use[:, None] != 0, c.patches, np.nan)
    got = run_overlap(c, gpu, whole, pre=c.pre, use=use, cnt0=cnt0, patches=poisoned, pad=3)
    judge_exact(got[0], s.astype(np.float64), name)
    assert np.array_equal(got[1], cnt0 + cover), 'cnt accumulates the used covering patches once per pixel'
    by = np.where(use != 0, rs.choice(np.array([1, 2, 0x80, 0xFF], dtype=np.uint8), size=c.n), 0).astype(np.uint8)
    by[np.flatnonzero(use)[:4]] = [1, 2, 0x80, 0xFF][:int(min(4, use.sum()))]
    for cuts, u in [(whole, by)] + [(cut, use) for cut in all_cuts(c.gi.g)[1:]] + [(single, by)]:
        res = run_overlap(c, gpu, cuts, pre=c.pre, use=u, cnt0=cnt0, patches=poisoned)
        assert same_bits(res[0], got[0]) and same_bits(res[1], got[1]), ('bytes or a cut into passes changed the result', cuts)
    # gaussian: the bound
    cg = make_overlap_case(r, dt, 'gaussian')
    s, a, cover = overlap_ref(cg.patches, cg.g, use=use, pre=cg.pre)
    accg, cntg = run_overlap(cg, gpu, whole, pre=cg.pre, use=use)
    judge_bound(accg, s, (cover[:, :, None] + 1) * 2.0 ** -52 * a, 'weighted ' + dt, name)
    assert np.array_equal(cntg, cover), 'cnt'
    # the inpaint finish on these sums: cnt 0 somewhere (use thinned further), observed elements kept or not
    cover[0, :] = 0
    img = scene_image('gaussian', rs, H, W, Cc, dt)
    obs = rs.choice(np.array([0, 1, 2, 0x80, 0xFF], dtype=np.uint8), size=(H, W, Cc))
    f = getattr(lib, 'modl_image_inpaint_finish_' + dt)
    ad, cd, im, od = _dev(accg, 'f64', gpu), _dev(cover, 'i32', gpu), _dev(img, dt, gpu), _dev(obs, 'u8', gpu)
    for keep in (0, 1):
        res = []
        for _ in range(2):
            out = Buf((H, W, Cc), dt, gpu)
            assert f(_ptr(ad), _ptr(cd), _ptr(im), _ptr(od), H, W, Cc, keep, out.p, None) == 0
            torch.cuda.synchronize()
            res.append(out.get())
        assert same_bits(*res)
        want = inpaint_restated(accg, cover, img, obs, keep, T)
        assert same_bits(res[0], want), 'inpaint finish: acc / cnt rounded once, or the input\'s bits'
        assert same_bits(res[0][cover == 0], img.astype(T)[cover == 0]), 'cnt 0: the input\'s bits'
        if keep:
            assert same_bits(res[0][obs != 0], img.astype(T)[obs != 0]), 'observed + keep: the input\'s bits'
        live = (cover[:, :, None] > 0) & ~((obs != 0) & bool(keep))
        q = np.asarray(accg, dtype=LD) / np.maximum(cover, 1)[:, :, None]
        judge_bound(res[0][live], q[live], eps_of(dt) * np.abs(q[live]).astype(np.float64), 'inpaint finish ' + dt, name)
    _report()


def run_objective(c, dev, ws_bytes=None):
    import torch
    from modl_amd._lib import lib
    f = getattr(lib, 'modl_objective_' + c.dt)
    ws_bytes = c.ws if ws_bytes is None else ws_bytes
    ldx = c.p + c.pad
    Xh = np.full((max(c.n, 1), ldx), np.nan)
    Xh[:c.n, :c.p] = c.X
    X, code, Dt = _dev(Xh, c.dt, dev), _dev(c.code if c.n else np.zeros((1, c.k)), c.dt, dev), _dev(c.Dt, c.dt, dev)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)                # ONE workspace for both calls
    res = []
    for _ in range(2):
        out = Buf((3,), 'f64', dev)
        assert f(_ptr(X), ldx, c.n, c.p, _ptr(Dt), c.k, _ptr(code), _ptr(ws), ws_bytes, out.p, None) == 0
        torch.cuda.synchronize()
        res.append(out.get())
    assert same_bits(*res), 'the same workspace twice gave other bits'
    return res[0]


OBJECTIVE_POINTS = [(r.name, dt) for r in POINTS if r.probe == 'objective' and r.name != 'o-enomem' for dt in BOTH]


@pytest.mark.gpu
@pytest.mark.parametrize('name,dt', OBJECTIVE_POINTS, ids=['%s-%s' % c for c in OBJECTIVE_POINTS])
def test_objective(gpu, name, dt):
    """modl_objective_*: one chunk and many, the default workspace at its cap of 8192 rows, one and two sweeps of the
    partial sums, n = 0, loose rows of X"""
    from modl_amd._lib import lib
    r = POINT[name]
    tsz = np.dtype(DT[dt]).itemsize
    assert lib.modl_objective_workspace(0 if dt == 'f32' else 1, r.sh['n'], r.sh['p']) == objective_workspace(r.sh['n'], r.sh['p'], tsz)
    for scene in ('integers', 'gaussian'):
        c = make_objective_case(r, dt, scene)
        out = run_objective(c, gpu)
        if c.n == 0:
            assert same_bits(out, np.zeros(3)), 'n = 0: three zeros'
            continue
        judge_objective(c, out, 'objective ' + dt)
        if scene == 'integers' and len(c.chunks) > 1:                        # the exact sums whatever the chunking
            assert same_bits(run_objective(c, gpu, objective_workspace(c.n, c.p, tsz)), out)
    _report()
