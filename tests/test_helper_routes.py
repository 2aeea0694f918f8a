"""The atom-geometry and row-movement helper kernels route by route: modl_enet_{norm,projection,scale}_*, modl_transpose_*,
modl_update_G_average_*, modl_predict_csr, modl_apply_swaps_rows_device (modl_amd/csrc/enet.hip), modl_gather_rows_*
(csrc/somf_step.hip, gather_rows_T_kernel) and the host's modl_apply_swaps_rows (csrc/rk_host.cpp), every one called by name on
buffers of the test's own layout.  The yardstick is a plain restatement in this file - exact sums (mpmath, 400 bits), the level
solved in its stable form to over 100 digits, long double for the last step - and nothing of the code under test enters a reference
or a bound.  Every device output is pre-filled with 7.5 and followed by 8 guard elements; the judge holds the padding of a padded
`ld`, the gaps of a column layout and the guards to the sentinel bit for bit.

ROUTES (`ENET_CASES` and the tables below; `test_route_table` holds every case to the route its scene is for, by the exact reference
and by `restate_project`, the line-by-line restatement of enet_projection_kernel / block_enet_project, and every n, rows, layout,
l1_ratio, aliasing and route to some case in both dtypes.  The same table is in DESIGN.md, section 25b.)
  enet       one workgroup of 256 per row, a stride-256 loop over n.  n in 1, 2, 63, 64, 65, 255, 256, 257, 511, 513, 1025 (the
             wavefront and workgroup boundaries, a fifth turn), each in all four layouts: contiguous (ld = n, inc = 1), padded
             (ld = n + 3), column atoms (ld = 1, inc = rows: the layout of scale_atoms) and column atoms of a wider matrix (inc =
             rows + 2); rows 1, 3, 5 and l1_ratio 0, 2^-10, 0.15, 0.5, 0.999, 1 rotate over them, and n 257 and 1025 take every
             l1_ratio in every layout.  The projection writes to `v` itself and to a separate `out`; every row has its own radius
             (the scale takes one per call).
  projection poisoned (the row's enet norm is not finite: NaN throughout) / zeros (radius <= 0) / l2 (l1_ratio 0, the radius in
             squared-norm units) inside, outside / quad (0 < l1_ratio < 1: the quadratic level) inside, outside / lin (l1_ratio
             1: gamma = 0) inside, outside; a final support of one element (`single`); a support that shrinks over at least four
             passes (`shrink`, l1_ratio 0.15 and above: at 2^-10 the quadratic settles within three).  The pass counts are asserted on
             the restatement, its final support against the exact one; the judge looks at the output alone.
  scale      l2 != 0 / l2 == 0 and l1 != 0 (l1_ratio 1) / a zero row (stays zero, -0.0 included) / poisoned.
  transpose  32 x 32 tiles, (rows, cols) in (1,1), (1,33), (33,1), (31,32), (32,32), (33,65), (64,31), (257,3), exact; 32 * 65536
             rows of one column (the y extent the MI355X reports, 65536: taken) and one row more (MODL_EINVAL, also without a device).
  gather     n_rows 1, 5, 300 x cols 1, 255, 256, 257, 513; src_ld and dst_ld equal to cols and larger; the identity, a reversed
             order, repeated indices; all in range.  Exact.
  swaps      n 0, 1, 2, 7, 300 x row_bytes 4, 8, 12, 1028: the device, the host and the loop i = n - 1 .. 1 of random_fast.pyx:105-119
             agree byte for byte; h_swaps[i] > i, < 0 and row_bytes 6 (device) return MODL_EINVAL and move nothing.
  predict    n_rows 1, 4, 5, 9 (the last group of four partly empty), rows of 0, 1, 64, 65, 130 entries, k 1 and 6.
  G_average  b 1, 3; k 1, 16, 17, 129 (k^2 = 16641 > 64 * 256: the grid-stride loop's second turn); w 0.3, 0, 1 by sample.

SCENES (deterministic; `test_cases_are_what_they_claim` checks each claim on the CPU)
  planted      noise of 0.05 .. 0.3 and entries of 2 .. 5.25 at element 0, n - 1, the last multiple of 256 below n and 256, of another
               size and sign in every row.  Without any one of them in the sums the result moves by over 100 bounds, and every
               entry is at least 100 bounds from the exact level (both asserted; a seed that misses the margin is passed over).
  ties         1.5 three times and 0.75, 0.25 twice, 0.0 and -0.0 in every row of twelve: duplicates above the level (asserted); -0.0
               comes out +0 (sign(0) = +1), a negative entry below the level -0.0 as in enet.pyx:121.
  edge_radius  sixteenths, so that every sum is exact in any order and the row's norm is a number of the dtype: the radius equal
               to it (copied), one ulp below (projected), one ulp above (copied), l1_ratio 0, 0.5, 1; the rows hold 0.0 and -0.0,
               which a projection with a level below zero would move.
  spread       2^-60 .. 2^40 in one row.
  near_l1      l1_ratio 0.999, radius 0.5 .. 0.6 of the norm: kappa (below) is asserted above 50 in every row.
  inside, zero_radius (radii 0, -1 and a positive one), single, shrink, allzero: the routes above.
  poisoned     NaN, +inf or -inf in row 1 of three at element 0 or n - 1: the projection and the scale give that row NaN throughout,
               the norm NaN (+inf for an infinity at l1_ratio < 1, which is that row's norm); the other rows carry the bits of the
               same call without the poison.  The pass loop is bounded by 256 passes.
  rerun        the same call twice, and a row alone against the same row as row 2 of 5, contiguous and as a column: the same bits.

JUDGE (`judge`, `judge_enet`; u_T = eps / 2 of the dtype; every constant is derived, none tuned to a device figure)
  norm        (n + 4) 2^-53 ref + u_T ref: a float64 sum of n terms of three operations each, rounded once.
  scale       (2 u_T + e_S) |ref|, e_S = (n + 8) 2^-53 (l1^2 / (4 radius l2) + 1) on the exact sums: S rounded to the dtype and the
              product rounded; the float64 error of S = (-l1 + sqrt(l1^2 + 4 radius l2)) / (2 l2) carries its cancellation factor.
  projection  the reference is the exact projection.  u_T |ref_i| + (u_T l + e_l)(1 + gamma |v_i|) / (1 + l gamma)^2 with
              e_l = (m + 8) 2^-53 l (1 + kappa), kappa = qd^2 / (4 qa |qc|) on the exact support of m entries (0 at gamma = 0):
              d u_i / d l = -(1 + gamma |v_i|) / (1 + l gamma)^2, the level is rounded to the dtype before thresholding (u_T l), and
              the closed form (-qd + sqrt(qd^2 - 4 qa qc)) / (2 qa) loses 1 + kappa.  l1_ratio 0: (2 u_T + (n + 8) 2^-53) |ref_i|
              (the scale sqrt(s / radius) rounded to the dtype, one division).  Inside the ball, radius <= 0: the bits.
              Outside the ball the enet norm of the DEVICE's result must equal the radius within the image of that bound,
              sum_i (rho + 2 (1 - rho) |ref_i|) b_i + (1 - rho) b_i^2 - a check without the reference projection in it.
              (kappa = 0 at gamma = 0 leaves the cancellation of S - R out: the scenes keep the radius at most 0.65 of the norm
              there, or make the sums exact.)
  predict     k 2^-53 sum |P||Q| against the exactly summed products; G_average: w = 0 leaves the bits, w = 1 gives G, otherwise
              3 u_T (|(1 - w) Ga| + |w G|) against the exact value.  Everything else: bit for bit.
  NaN and infinity must sit where the reference has them; a zero carries the reference's sign.
  gamma       one term more than the issue's formula, which this file's own `spread` scene showed to be missing (59 bounds in float64
              at l1_ratio 0.999 without it, in the restatement and on the device alike).  gamma = 2 / rho - 2 (enet.pyx:73,
              enet_block.hpp:50) is formed with a relative error e_g = 2^-53 (1 / (1 - rho) + 1): 2 / rho rounded, the difference
              rounded.  Its image, to first order on the exact support, with D = 1 + l gamma and F = sum u + gamma / 2 sum u^2 = R:
              gamma e_g (|ref_i| l / D + (1 + gamma |v_i|) / D^2 |F_gamma / F_l|), F_gamma = -(l / D)(sum u + gamma sum u^2) +
              sum u^2 / 2, F_l = -sum (1 + gamma u)(1 + gamma |v|) / D^2.  Negligible where gamma |v| is small; it enters the bound of
              every quadratic case, the image on the norm and the margin of the level.  `spread` at l1_ratio 0.999 (`gamma_case`:
              entries up to 2^40) is held to it like every case; its ratio against the bound WITHOUT the term is reported beside it.

MUTANTS (`test_judge_rejects_mutants`, `test_judge_rejects_movement_mutants`, both dtypes: each is a flag of the restatement, and
the judge rejects it on EVERY case named for it - `enet_mutant_cases`)
  inc_ignored          adjacent elements read and written              every planted case with inc > 1 and n > 1
  ld_ignored           every row reads row 0                           every planted case with rows > 1
  radius0              row 0's radius for all rows                     every planted projection with rows > 1
  drop_last            element n - 1 left out of the sums              every planted case
  drop_256             the elements from 256 on left out of the sums   every planted case with n > 256
  full_turns           only full turns of 256 summed                   every planted case with n mod 256 != 0
  radius_not_scaled    the radius not divided by l1_ratio              every planted projection with 0 < l1_ratio < 1
  l2_sqrt_radius       v / sqrt(radius) for v / sqrt(s / radius)       every planted projection at l1_ratio 0
  zero_radius_kept     radius == 0 not zeroing                         every zero_radius case (-0.0 for a negative entry)
  never_inside         projected although inside the ball              every edge_radius case with l1_ratio > 0 (the zeros move)
  sign0                sign(0) = 0                                     every ties projection with l1_ratio > 0 (-0.0 stays -0.0)
  nan_swallowed        a NaN thresholded to 0: the kernel before this  every poisoned projection with 0 < l1_ratio < 1, and with a NaN
                       file                                            at l1_ratio 1 (an infinity there made the level NaN, 0 * inf,
                                                                       and the row with it; at 0 the NaN reaches the scale by itself)
  swap_weights         the l1 and l2 weights of the scale swapped      every planted scale with l1_ratio != 0.5
  no_l2_zero_branch    the scale's l2 == 0 branch missing              every planted scale at l1_ratio 1
  transpose_edge_le    `<=` in the tile's edge tests                   every shape that is no multiple of 32 both ways
  transpose_swapped    rows and cols swapped in the output index       every shape that is no vector
  gather_index_ignored the index ignored                               every case whose order is not the identity
  gather_dst_ld_cols   dst_ld taken for cols                           every case with dst_ld > cols and two rows
  swaps_ascending      the swaps applied from i = 1 up                 n 7 and 300
  swaps_inverse        the inverse permutation gathered                n 7 and 300
  csr_past_64          the entries past a row's first 64 dropped       every case with a row of 65 or 130
  csr_last_group       the last, partial group of four rows dropped    n_rows 1, 5, 9
  gavg_w0              sample 0's weight for every sample              b = 3
  `a >= level` for `a > level` in the support test is the one mistake of the list that no judge of the output can reject: it is the
  same projection (`test_support_ge_is_no_mistake` has the argument and holds it on the `ties` scene built for it).
  Three were also planted in the kernels themselves (variant libraries, MODL_HIP_LIBRARY): `inc` taken for 1 in the three
  enet kernels failed test_enet_against_exact on exactly the named cases (40 norm, 64 projection and 40 scale cases of either dtype),
  `radius[0]` for `radius[blockIdx.x]` on exactly the 125 named projections of either dtype, and `<=` in both edge tests of
  transpose_kernel failed test_transpose_exact at its first shape (the guard behind the output of (1, 1) held the input's guard).

MEASURED (largest |got - ref| / bound per entry point and route on the MI355X, from this file's own run - `test_report` prints it;
the judge's 1 is what is asserted):
  norm                                           f32 0.999   f64 0.176
  scale, l2 != 0                                 f32 0.900   f64 0.174
  scale, l2 == 0 and l1 != 0                     f32 0.786   f64 0.067
  projection, l1_ratio 0 outside                 f32 0.840   f64 0.082
  projection, quadratic level outside            f32 0.968   f64 0.779
  projection, linear level outside               f32 0.928   f64 0.328
  projection, near_l1 (with kappa)               f32 0.815   f64 0.015
  projection, spread at l1_ratio 0.999           f32 0.795   f64 0.779
  projection, norm of the result against radius  f32 0.625   f64 0.778
  update_G_average                               f32 0.592   f64 0.596
  predict_csr                                    f64 0.331
  every route that copies, zeroes, poisons or moves rows (inside the ball, radius <= 0, poisoned and zero rows, transpose,
  gather, swaps): 0, the bits.  Records, not checks: near_l1 against the bound WITHOUT kappa f32 0.816, f64 32.167 - the loss of the
  reference's level formula at l1_ratio 0.999 (kappa 1.8e3 .. 4.2e3 in these rows; float32 forms the level in float64 and rounds
  once); spread at l1_ratio 0.999 against the bound WITHOUT the gamma term f32 0.795, f64 58.807.  30 GPU tests (1296 calls and
  their twins) in 12 s.
  (The float32 figures near 1 are the last rounding: half an ulp is u_T |ref| for a value just above a power of two.)
"""
import ctypes as C
import functools
import math
import re
import zlib
from fractions import Fraction
from types import SimpleNamespace

import mpmath
import numpy as np
import pytest

mp = mpmath.mp.clone()
mp.prec = 400                                  # sums of squares over 2^-120 .. 2^80 are exact, a level has over 100 digits
DT = {'f32': np.float32, 'f64': np.float64}
UI = {'f32': np.uint32, 'f64': np.uint64}
UT = {'f32': 2.0 ** -24, 'f64': 2.0 ** -53}    # u_T = eps / 2
U64 = 2.0 ** -53
LD = np.longdouble                             # the judge subtracts in it; references are rounded once from mpmath or exact
SENT = 7.5                                     # fills every output before a call; no scene produces it
GUARD = 8                                      # elements behind each output
MAX_PASS = 256                                 # MODL_MAX_PASS
MAX_GRID_Y = 65536                             # maxGridSize[1] of the MI355X
EINVAL = -1


def cdiv(a, b):
    return -(-a // b)


def fl(x, dt):
    """round to the dtype, back as float64"""
    with np.errstate(over='ignore', invalid='ignore'):
        return np.asarray(x, np.float64).astype(DT[dt]).astype(np.float64)


# ------------------------------------------------------------------------------------------------------- layouts, buffers
LAYOUTS = ('contig', 'padded', 'col', 'colwide')


def layout(lay, rows, n):
    """-> (ld, inc, elements of the buffer)"""
    if lay == 'contig':
        return n, 1, rows * n
    if lay == 'padded':
        return n + 3, 1, rows * (n + 3)
    if lay == 'col':
        return 1, rows, n * rows
    return 1, rows + 2, n * (rows + 2)


def positions(rows, n, ld, inc):
    return np.arange(rows)[:, None] * ld + np.arange(n)[None, :] * inc


def pack(V, ld, inc, size, dt):
    buf = np.full(size + GUARD, SENT, DT[dt])
    buf[positions(V.shape[0], V.shape[1], ld, inc)] = V
    return buf


# --------------------------------------------------------------------------------------- exact sums, the exact projection
def msum(a, squared=False):
    return mp.fsum([mp.mpf(float(x)) for x in a], squared=squared)


def two(x):
    """an mpf as a long double (two float64 parts added in long double)"""
    hi = float(x)
    return LD(hi) + LD(float(x - mp.mpf(hi)))


def exact_norm(x, rho):
    a = np.abs(x)
    return mp.mpf(rho) * msum(a) + (1 - mp.mpf(rho)) * msum(a, squared=True)


def _level(S, m, R, gamma):
    """the root of the level equation on a support of m entries with sum a (1 + gamma a / 2) = S > R, in its stable form;
    -> (l, kappa)"""
    if gamma == 0:
        return (S - R) / m, mp.mpf(0)
    qa = gamma * gamma * R + gamma * m / 2
    qd = 2 * R * gamma + m
    qc = R - S
    l = 2 * (-qc) / (qd + mp.sqrt(qd * qd - 4 * qa * qc))
    return l, qd * qd / (4 * qa * (-qc))


def exact_project(x, radius, rho, dt):
    """The Euclidean projection of x onto { u : sum |u| (rho + (1 - rho) |u|) <= radius } (enet.pyx:38-122: for rho == 0 the
    rescaling onto { sum u^2 <= radius }), the support found by sorting and confirmed by the optimality conditions in
    mpmath, the level to over 100 digits.  -> ref (long double), bnd, bnd without kappa, route, and the level's figures."""
    n, u = len(x), UT[dt]
    out = SimpleNamespace(l=None, kappa=0.0, m=None, gamma=None, margin=np.inf)
    if not np.all(np.isfinite(x)):
        out.ref, out.bnd, out.route = np.full(n, np.nan, LD), np.zeros(n), 'poisoned'
    elif not radius > 0:
        out.ref, out.bnd, out.route = np.zeros(n, LD), np.zeros(n), 'zeros'
    elif rho == 0:
        s = msum(x, squared=True)
        if s <= mp.mpf(radius):
            out.ref, out.bnd, out.route = x.astype(LD), np.zeros(n), 'l2/inside'
        else:
            out.ref = x.astype(LD) / two(mp.sqrt(s / mp.mpf(radius)))
            out.bnd = (2 * u + (n + 8) * U64) * np.abs(out.ref).astype(np.float64)
            out.route = 'l2/outside'
    else:
        a = np.abs(x)
        gamma = 2 / mp.mpf(rho) - 2
        R = mp.mpf(radius) / mp.mpf(rho)
        kind = 'lin' if gamma == 0 else 'quad'
        tot = msum(a) + gamma / 2 * msum(a, squared=True)
        if tot <= R:
            out.ref, out.bnd, out.route = x.astype(LD), np.zeros(n), kind + '/inside'
        else:
            srt = np.sort(a)[::-1]

            def fits(m):
                S = msum(srt[:m]) + gamma / 2 * msum(srt[:m], squared=True)
                if S <= R:
                    return None
                l, kappa = _level(S, m, R, gamma)
                if mp.mpf(float(srt[m - 1])) > l and (m == n or mp.mpf(float(srt[m])) <= l):
                    return l, kappa
                return None
            guess = restate_project(x, radius, rho, 'f64').m
            got, m = fits(guess) if 1 <= guess <= n else None, guess
            if got is None:
                for m in range(1, n + 1):
                    got = fits(m)
                    if got is not None:
                        break
            assert got is not None
            l, kappa = got
            den = two(1 + l * gamma)
            lf, gf, kf = float(l), float(gamma), float(kappa)
            pos = a.astype(LD) - two(l)
            out.ref = np.where(x >= 0, LD(1), LD(-1)) * np.where(a > lf, pos, LD(0)) / den      # sign(0) = +1; -1 * 0 = -0
            ref = np.abs(out.ref).astype(np.float64)
            image = (1 + gf * a) / (1 + lf * gf) ** 2
            e_l = (m + 8) * U64 * lf
            # gamma = 2 / rho - 2 as the kernel forms it: 2 / rho rounded (2^-53 (2 / rho) = 2^-53 gamma / (1 - rho)) and the
            # difference rounded, a relative error e_g of gamma.  Its image, to first order on the exact support, with
            # D = 1 + l gamma and F(l, gamma) = sum u + gamma / 2 sum u^2 = R:  du_i = -u_i l / D dgamma - (1 + gamma |v_i|) / D^2 dl,
            # dl = -(F_gamma / F_l) dgamma, F_gamma = -(l / D)(sum u + gamma sum u^2) + sum u^2 / 2,
            # F_l = -sum (1 + gamma u_i)(1 + gamma |v_i|) / D^2.
            if gf != 0.0:
                e_g = U64 * (1.0 / (1.0 - rho) + 1.0)
                D, us, as_ = 1 + lf * gf, ref[a > lf], a[a > lf]
                F_g = -(lf / D) * (np.sum(us) + gf * np.sum(us * us)) + 0.5 * np.sum(us * us)
                F_l = -np.sum((1 + gf * us) * (1 + gf * as_)) / D ** 2
                dl_g = gf * e_g * abs(F_g / F_l)
                g_term = gf * e_g * ref * lf / D + dl_g * image
            else:
                dl_g, g_term = 0.0, np.zeros(n)
            out.bnd = u * ref + (u * lf + e_l * (1 + kf)) * image + g_term
            out.bnd_nokappa = u * ref + (u * lf + e_l) * image + g_term
            out.bnd_nogamma = u * ref + (u * lf + e_l * (1 + kf)) * image
            out.route, out.l, out.kappa, out.m, out.gamma = kind + '/outside', lf, kf, m, gf
            out.margin = float(np.min(np.abs(a - lf))) / (u * lf + e_l * (1 + kf) + dl_g)
    for name in ('bnd_nokappa', 'bnd_nogamma'):
        if not hasattr(out, name):
            setattr(out, name, out.bnd)
    return out


def norm_image(ref, bnd, rho):
    """what a per-element bound allows the enet norm of the result to move by"""
    ref = np.abs(np.asarray(ref, np.float64))
    return float(np.sum((rho + 2 * (1 - rho) * ref) * bnd + (1 - rho) * bnd * bnd))


def exact_scale(x, radius, rho, dt):
    """enet.pyx:150-167 with exact sums: -> ref (long double), bnd, route"""
    n, u = len(x), UT[dt]
    if not np.all(np.isfinite(x)):
        return SimpleNamespace(ref=np.full(n, np.nan, LD), bnd=np.zeros(n), route='poisoned')
    a = np.abs(x)
    l1, l2, r = mp.mpf(rho) * msum(a), (1 - mp.mpf(rho)) * msum(a, squared=True), mp.mpf(radius)
    if l2 != 0:
        S, cancel, route = 2 * r / (l1 + mp.sqrt(l1 * l1 + 4 * r * l2)), l1 * l1 / (4 * r * l2) + 1, 'l2!=0'
    elif l1 != 0:
        S, cancel, route = r / l1, mp.mpf(1), 'l2==0,l1!=0'
    else:
        return SimpleNamespace(ref=x.astype(LD), bnd=np.zeros(n), route='zero_row')        # x * 0: the zeros keep their signs
    ref = x.astype(LD) * two(S)
    e_S = (n + 8) * U64 * float(cancel)
    return SimpleNamespace(ref=ref, bnd=(2 * u + e_S) * np.abs(ref).astype(np.float64), route=route)


# -------------------------------------------------------------------- the restatement of the three kernels, and its mutants
def _visited(n, mut):
    """how many of the n elements the summing loops take"""
    if mut == 'drop_last':
        return n - 1
    if mut == 'drop_256':
        return min(n, 256)
    if mut == 'full_turns':
        return n // 256 * 256
    return n


def restate_norm(x, rho, mut=None):
    a = np.abs(x[:_visited(len(x), mut)])
    with np.errstate(invalid='ignore', over='ignore'):
        return float(np.sum(a * (rho + (1.0 - rho) * a)))


def restate_project(x, radius, rho, dt, mut=None):
    """enet_projection_kernel and block_enet_project for one row, line by line in float64; -> out (rounded to the dtype), the
    route, the passes of the active-set loop and the size of the final support"""
    n = len(x)
    res = SimpleNamespace(passes=0, m=0)
    xs = x[:_visited(n, mut)]
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        if mut != 'nan_swallowed' and not math.isfinite(restate_norm(x, rho, mut)):
            res.out, res.route = np.full(n, np.nan), 'poisoned'
            return res
        if not radius > 0.0 and not (mut == 'zero_radius_kept' and radius == 0.0):
            res.out, res.route = np.zeros(n), 'zeros'
            return res
        if rho == 0.0:
            s = float(np.sum(xs * xs))
            inside = s <= radius
            scale = 1.0 if inside else float(fl(math.sqrt(radius) if mut == 'l2_sqrt_radius' else np.sqrt(np.float64(s) / radius), dt))
            res.out, res.route = fl(fl(x, dt) / scale, dt), 'l2/inside' if inside else 'l2/outside'
            return res
        gamma = 2.0 / rho - 2.0
        R = radius if mut == 'radius_not_scaled' else radius / rho
        kind = 'lin' if gamma == 0.0 else 'quad'
        a = np.abs(xs)
        term = a * (1.0 + 0.5 * gamma * a)
        tot = float(np.sum(term))
        if tot <= R and mut != 'never_inside':
            res.out, res.route = x.copy(), kind + '/inside'
            return res
        level, prev = 0.0, -1.0
        while res.passes < MAX_PASS:
            sel = a >= level if mut == 'support_ge' else a > level
            S, cnt = float(np.sum(term[sel])), float(np.count_nonzero(sel))
            if cnt == prev or cnt == 0.0:
                break
            prev = cnt
            if gamma != 0.0:
                qa = gamma * gamma * R + gamma * cnt * 0.5
                qd = 2.0 * R * gamma + cnt
                qc = R - S
                level = float((-qd + np.sqrt(np.float64(qd * qd - 4.0 * qa * qc))) / (2.0 * qa))
            else:
                level = (S - R) / cnt
            res.passes += 1
        lT = float(fl(level, dt))
        den = 1.0 + lT * gamma
        pos = np.abs(x) - lT
        pos = np.where(pos > 0, pos, 0.0)
        if mut == 'sign0':
            sgn = np.where(x > 0, 1.0, np.where(x < 0, -1.0, x))                    # sign(+-0) = +-0
        else:
            sgn = np.where(x >= 0, 1.0, -1.0)
        res.out, res.route, res.m = fl(sgn * pos / den, dt), kind + '/outside', int(prev)
    return res


def scale_factor(x, radius, rho, dt, mut=None):
    """the factor S of enet_scale_kernel, rounded to the dtype"""
    xs = x[:_visited(len(x), mut)]
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        w1, w2 = (1.0 - rho, rho) if mut == 'swap_weights' else (rho, 1.0 - rho)
        l1 = np.float64(np.sum(np.abs(xs))) * w1
        l2 = np.float64(np.sum(xs * xs)) * w2
        S = np.float64(0.0)
        if l2 != 0.0 or mut == 'no_l2_zero_branch':
            S = (-l1 + np.sqrt(l1 * l1 + 4.0 * radius * l2)) / (2.0 * l2)
        elif l1 != 0.0:
            S = radius / l1
        return float(fl(S, dt))


def restate_scale(x, radius, rho, dt, mut=None):
    with np.errstate(invalid='ignore', over='ignore'):
        return fl(x * scale_factor(x, radius, rho, dt, mut), dt)


ENET_MUTANTS = ('inc_ignored', 'ld_ignored', 'radius0', 'drop_last', 'drop_256', 'full_turns', 'radius_not_scaled',
                'l2_sqrt_radius', 'zero_radius_kept', 'never_inside', 'sign0', 'nan_swallowed', 'swap_weights', 'no_l2_zero_branch')


def restate_enet_call(c, mut=None):
    """One call of modl_enet_{norm,projection,scale} on the flat buffer the device gets -> {'out': the output buffer (norm: the
    rows + GUARD norms)}"""
    op, dt, rows, n = c.op, c.dt, c.rows, c.n
    src = c.buf.astype(np.float64)
    step = 1 if mut == 'inc_ignored' else c.inc
    if op == 'norm':
        out = np.full(rows + GUARD, SENT)
    elif op == 'projection' and not c.alias:
        out = np.full(len(src), SENT)
    else:
        out = src.copy()
    for r in range(rows):
        x = src[(0 if mut == 'ld_ignored' else r * c.ld) + np.arange(n) * step]
        w = r * c.ld + np.arange(n) * step
        if op == 'norm':
            out[r] = restate_norm(x, c.rho, mut)
        elif op == 'projection':
            res = restate_project(x, float(c.radius[0 if mut == 'radius0' else r]), c.rho, dt, mut)
            out[w] = res.out
        else:
            with np.errstate(invalid='ignore', over='ignore'):
                out[w] = fl(src[w] * scale_factor(x, float(c.radius[0]), c.rho, dt, mut), dt)
    with np.errstate(over='ignore', invalid='ignore'):
        return {'out': out.astype(DT[dt])}


# ------------------------------------------------------------------------------------------------------------- the judge
def judge(got, ref, bnd, what=''):
    """-> (largest |got - ref| / bound, None or the first complaint).  Where the bound is 0 (sentinels, padding, copies, zeros,
    moved rows) the bits must be the reference's; NaN and infinity must sit where the reference has them; a zero must carry the
    reference's sign."""
    got = np.asarray(got)
    ref, bnd = np.asarray(ref, LD), np.asarray(bnd, np.float64)
    if got.shape != ref.shape:
        return 0.0, '%s: shape %s for %s' % (what, got.shape, ref.shape)
    g = got.astype(LD)
    if not np.array_equal(np.isnan(g), np.isnan(ref)):
        i = int(np.flatnonzero(np.isnan(g) != np.isnan(ref))[0])
        return 0.0, '%s: NaN at other places, first [%d] got %r ref %r' % (what, i, got[i], float(ref[i]))
    ok = ~np.isnan(ref)
    with np.errstate(over='ignore'):
        rT = ref.astype(got.dtype)
    exact = ok & ((bnd == 0) | np.isinf(ref) | ((ref == 0) & (g == 0)))
    ui = UI['f32' if got.dtype == np.float32 else 'f64']
    bad = exact & (got.view(ui) != rT.view(ui))
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        return 0.0, '%s[%d]: got %r where %r belongs bit for bit' % (what, i, got[i], rT[i])
    rest = ok & ~exact
    if not rest.any():
        return 0.0, None
    with np.errstate(invalid='ignore', over='ignore'):
        ratio = (np.abs(g[rest] - ref[rest]) / bnd[rest]).astype(np.float64)
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    w = int(np.argmax(ratio))
    if ratio[w] > 1:
        i = int(np.flatnonzero(rest)[w])
        return float(ratio[w]), '%s[%d]: got %r ref %r, %.3g bounds' % (what, i, got[i], float(ref[i]), ratio[w])
    return float(ratio[w]), None


def judge_enet(c, e, got, detail=None):
    """got: {'out': buffer}.  The per-element judge; for a projected row also the enet norm of the result against the radius (no
    reference projection in it).  Nothing but the output is judged: what the device cannot report (pass counts) is not looked at."""
    worst, why = judge(got['out'], e.ref, e.bnd, c.id)
    if why is None and c.op == 'projection' and np.asarray(got['out']).shape == e.ref.shape:
        for r in range(c.rows):
            if e.rows[r].route.endswith('/outside'):
                w = r * c.ld + np.arange(c.n) * c.inc
                y = got['out'][w].astype(np.float64)
                nrm = float(exact_norm(y, c.rho)) if c.rho else float(msum(y, squared=True))
                tol = norm_image(e.ref[w], e.bnd[w], c.rho)
                if not abs(nrm - float(c.radius[r])) <= tol:
                    why = '%s row %d: enet norm %r of the result for radius %r, %.3g bounds' % (
                        c.id, r, nrm, float(c.radius[r]), abs(nrm - float(c.radius[r])) / tol)
                    break
                worst = max(worst, abs(nrm - float(c.radius[r])) / tol)
                if detail is not None:
                    detail['norm_check'] = max(detail.get('norm_check', 0.0), abs(nrm - float(c.radius[r])) / tol)
    return worst, why


# ------------------------------------------------------------------------------------------------------- the enet scenes
ENET_N = (1, 2, 63, 64, 65, 255, 256, 257, 511, 513, 1025)
ROWS = (1, 3, 5)
L1R = (0.0, 2.0 ** -10, 0.15, 0.5, 0.999, 1.0)
OPS = ('norm', 'projection', 'scale')
POISONS = {'nan': np.nan, 'pinf': np.inf, 'ninf': -np.inf}


def special_elements(n):
    return sorted({0, n - 1, (n - 1) // 256 * 256} | ({256} if n > 256 else set()))


def _planted_rows(rs, dt, n, rows):
    V = np.where(rs.rand(rows, n) < 0.5, -1.0, 1.0) * (0.05 + 0.25 * rs.rand(rows, n))
    for k, f in enumerate(special_elements(n)):
        V[:, f] = (2.0 + 0.5 * k) * (1 + 0.125 * np.arange(rows)) * (-1.0) ** (np.arange(rows) + k)   # (n = 1: a row differs from row 0 by its sign alone)
    return fl(V, dt)


def _norms(V, rho):
    return np.array([float(exact_norm(v, rho)) if rho else float(msum(v, squared=True)) for v in V])


def _below(x, dt):
    return float(np.nextafter(DT[dt](x), DT[dt](0)))


def _above(x, dt):
    return float(np.nextafter(DT[dt](x), DT[dt](np.inf)))


def make_rows(scene, dt, n, rows, rho, seed):
    """-> (V rows x n, radius per row), every value representable in the dtype"""
    rs = np.random.RandomState(seed)
    frac = 0.25 + 0.1 * np.arange(rows)                      # a different radius for every row, at most 0.65 of the norm
    if scene in ('planted', 'near_l1', 'inside', 'zero_radius', 'allzero') or scene.startswith('poisoned'):
        V = _planted_rows(rs, dt, n, rows)
        rad = frac * _norms(V, rho)
        if scene == 'near_l1':
            rad = (0.5 + 0.05 * np.arange(rows)) * _norms(V, rho)
        elif scene == 'inside':
            rad = (1.5 + 0.5 * np.arange(rows)) * _norms(V, rho)
        elif scene == 'zero_radius':
            rad = np.where(np.arange(rows) % 3 == 0, 0.0, np.where(np.arange(rows) % 3 == 1, -1.0, rad))
        elif scene == 'allzero':
            V[1] = 0.0
            V[1, n // 2] = -0.0
        elif scene.startswith('poisoned'):
            _, what, where = scene.split('_')
            V[1, 0 if where == 'first' else n - 1] = POISONS[what]
    elif scene == 'single':                                  # one entry of 5 over noise below every level: the projection is 1 there
        V = np.where(rs.rand(rows, n) < 0.5, -1.0, 1.0) * 1e-4 * (0.1 + 0.9 * rs.rand(rows, n))
        V[np.arange(rows), (n // 2 + np.arange(rows)) % n] = -5.0
        V, rad = fl(V, dt), 1.0 + 0.25 * np.arange(rows)
    elif scene == 'shrink':                                  # magnitudes falling geometrically: each pass drops a slice of them
        V = 2.0 ** (-np.arange(n) * (40.0 / n))[None, :] * (1 + 0.1 * rs.rand(rows, n)) * np.where(rs.rand(rows, n) < 0.5, -1.0, 1.0)
        V = fl(V[:, rs.permutation(n)], dt)
        rad = 1e-3 * (1 + np.arange(rows)) * _norms(V, rho)
    elif scene == 'ties':
        pat = np.array([1.5, 1.5, -1.5, 0.0, -0.0, 0.25, 0.75, -0.75, 1.5, 0.25, -0.25, 3.0])
        V = np.stack([np.roll(np.resize(pat, n), r) for r in range(rows)])
        rad = (0.5 + 0.04 * np.arange(rows)) * _norms(V, rho)
    elif scene == 'edge_radius':                             # sixteenths: every sum is exact in float64 in any order, and in the dtype
        V = rs.randint(8, 33, size=(rows, n)) / 16.0 * np.where(rs.rand(rows, n) < 0.5, -1.0, 1.0)
        V[:, n // 3] = 0.0
        V[:, n // 2] = -0.0
        nr = _norms(V, rho)
        assert np.all(fl(nr, dt) == nr)
        rad = np.array([(nr[r], _below(nr[r], dt), _above(nr[r], dt))[r % 3] for r in range(rows)])
    elif scene == 'spread':                                  # 2^-60 .. 2^40 in one row
        e = np.round(np.linspace(-60, 40, n)) if n > 1 else np.array([40.0])
        V = np.stack([(2.0 ** e * (1 + 0.25 * rs.rand(n)) * np.where(rs.rand(n) < 0.5, -1.0, 1.0))[rs.permutation(n)] for _ in range(rows)])
        V = fl(V, dt)
        rad = frac * _norms(V, rho)
    else:
        raise ValueError(scene)
    return V, fl(rad, dt)


def _enet_case_list():
    out = []

    def add(scene, n, rows, lay, l1r, alias=0, ops=OPS):
        for op in ops:
            for dt in ('f32', 'f64'):
                out.append((op, dt, scene, n, rows, lay, l1r, alias if op == 'projection' else 0))
    for i, n in enumerate(ENET_N):                           # every n in every layout; rows, l1_ratio and aliasing rotate
        for j, lay in enumerate(LAYOUTS):
            add('planted', n, ROWS[(i + j) % 3], lay, L1R[(i + 2 * j) % 6], (i + j) % 2)
    for i, n in enumerate((257, 1025)):                      # every l1_ratio in every layout, out aliased and apart
        for j, lay in enumerate(LAYOUTS):
            for k, l1r in enumerate(L1R):
                add('planted', n, (5, 3)[i], lay, l1r, (j + k) % 2)
                add('planted', n, (5, 3)[i], lay, l1r, (j + k + 1) % 2, ops=('projection',))
    for j, lay in enumerate(LAYOUTS):
        for k, l1r in enumerate(L1R):
            n = (65, 257, 513)[(j + k) % 3]
            add('inside', n, 3, lay, l1r, k % 2, ops=('projection',))
            add('zero_radius', n, 3, lay, l1r, (k + 1) % 2, ops=('projection',))
            add('ties', (64, 257, 1025)[(j + k) % 3], 3, lay, l1r, k % 2)
            add('spread', (2, 255, 1025)[(j + k) % 3], 3, lay, l1r, (j + k) % 2)
            if l1r:
                add('single', (1, 65, 513)[(j + k) % 3], 3, lay, l1r, j % 2, ops=('projection',))
            if l1r >= 0.15:                                  # (at 2^-10 the quadratic level settles within three passes)
                add('shrink', (511, 1025)[(j + k) % 2], 3, lay, l1r, k % 2, ops=('projection',))
        for k, l1r in enumerate((0.0, 0.5, 1.0)):
            add('edge_radius', (63, 256, 1025)[(j + k) % 3], 3, lay, l1r, (j + k) % 2, ops=('projection',))
        add('near_l1', (65, 257, 513, 1025)[j], (3, 5, 1, 3)[j], lay, 0.999, j % 2, ops=('projection',))
        add('allzero', (65, 257, 513, 1025)[j], 3, lay, (0.15, 1.0, 0.0, 0.5)[j], ops=('scale', 'norm'))
        for k, what in enumerate(POISONS):
            for where in ('first', 'last'):
                add('poisoned_%s_%s' % (what, where), (257, 64, 1025)[(j + k) % 3], 3, lay, (0.15, 1.0, 0.0)[(j + k + (where == 'last')) % 3],
                    (j + k) % 2)
    return out


ENET_CASES = _enet_case_list()


def enet_id(case):
    op, dt, scene, n, rows, lay, l1r, alias = case
    return '%s-%s-%s-n%d-r%d-%s-l1r%g%s' % (op, dt, scene, n, rows, lay, l1r, '-alias' if alias else '')


@functools.lru_cache(maxsize=None)
def _rows_of(dt, scene, n, rows, l1r):
    """the rows and radii of a scene: shared by the three entry points, every layout and both aliasings"""
    rho = float(DT[dt](l1r))
    for attempt in range(50):
        seed = zlib.crc32(('%s-%s-%d-%d-%g-%d' % (dt, scene, n, rows, l1r, attempt)).encode())
        V, rad = make_rows(scene, dt, n, rows, rho, seed)
        if scene not in ('planted', 'near_l1', 'ties'):
            break
        if all(exact_project(V[r], float(rad[r]), rho, dt).margin >= 100 for r in range(rows)):
            break                                             # every entry at least 100 bounds from the exact level
    else:
        raise AssertionError('no seed keeps the margin')
    return V, rad, rho


@functools.lru_cache(maxsize=None)
def enet_build(case):
    op, dt, scene, n, rows, lay, l1r, alias = case
    V, rad, rho = _rows_of(dt, scene, n, rows, l1r)
    if op == 'scale':
        rad = fl(np.full(rows, 1.5 if n % 2 else 0.75), dt)   # one radius per call
    ld, inc, size = layout(lay, rows, n)
    return SimpleNamespace(op=op, dt=dt, scene=scene, n=n, rows=rows, lay=lay, rho=rho, alias=alias, ld=ld, inc=inc, size=size,
                           V=V, radius=rad, buf=pack(V, ld, inc, size, dt), id=enet_id(case))


@functools.lru_cache(maxsize=None)
def _row_refs(op, dt, scene, n, rows, l1r):
    V, rad, rho = _rows_of(dt, scene, n, rows, l1r)
    if op == 'projection':
        return [exact_project(V[r], float(rad[r]), rho, dt) for r in range(rows)]
    rad = fl(np.full(rows, 1.5 if n % 2 else 0.75), dt)
    return [exact_scale(V[r], float(rad[r]), rho, dt) for r in range(rows)]


@functools.lru_cache(maxsize=None)
def enet_expected(case):
    """the whole output buffer of the call: reference, bound, the bound without kappa and without gamma's term; its rows' routes"""
    c = enet_build(case)
    e = SimpleNamespace(rows=[])
    if c.op == 'norm':
        e.ref, e.bnd = np.full(c.rows + GUARD, SENT, LD), np.zeros(c.rows + GUARD)
        for r in range(c.rows):
            with np.errstate(invalid='ignore', over='ignore'):
                x = c.V[r]
                if np.all(np.isfinite(x)):
                    e.ref[r] = two(exact_norm(x, c.rho))
                else:                                       # inf * (rho + (1 - rho) inf): NaN at rho == 1 (0 * inf), else inf
                    e.ref[r] = restate_norm(x, c.rho)
                e.bnd[r] = ((c.n + 4) * U64 + UT[c.dt]) * float(e.ref[r]) if np.isfinite(e.ref[r]) else 0.0
            e.rows.append(SimpleNamespace(route='norm'))
        e.bnd_nokappa = e.bnd_nogamma = e.bnd
        return e
    src = c.buf.astype(LD)
    e.ref = src.copy() if (c.op == 'scale' or c.alias) else np.full(len(src), SENT, LD)
    e.bnd, e.bnd_nokappa, e.bnd_nogamma = np.zeros(len(src)), np.zeros(len(src)), np.zeros(len(src))
    e.rows = _row_refs(c.op, c.dt, c.scene, c.n, c.rows, case[6])
    pos = positions(c.rows, c.n, c.ld, c.inc)
    for r, x in enumerate(e.rows):
        e.ref[pos[r]], e.bnd[pos[r]] = x.ref, x.bnd
        e.bnd_nokappa[pos[r]] = getattr(x, 'bnd_nokappa', x.bnd)
        e.bnd_nogamma[pos[r]] = getattr(x, 'bnd_nogamma', x.bnd)
    return e


def gamma_case(case):
    """`spread` at l1_ratio 0.999: entries up to 2^40, gamma |v| >> 1 - the cases that need the bound's gamma term (every other
    scene has gamma |v| < 8 at that ratio, or another ratio).  Held like every case; the ratio against the bound WITHOUT the term
    is reported beside it."""
    return case[0] == 'projection' and case[2] == 'spread' and case[6] == 0.999


def enet_mutant_cases(mut):
    """the cases on which the judge must reject `mut`"""
    out = []
    for case in ENET_CASES:
        op, dt, scene, n, rows, lay, l1r, alias = case
        ld, inc, _ = layout(lay, rows, n)
        pl, proj = scene == 'planted', op == 'projection'
        if mut == 'inc_ignored':
            ok = pl and inc > 1 and n > 1
        elif mut == 'ld_ignored':
            ok = pl and rows > 1
        elif mut == 'radius0':
            ok = pl and proj and rows > 1
        elif mut == 'drop_last':
            ok = pl
        elif mut == 'drop_256':
            ok = pl and n > 256
        elif mut == 'full_turns':
            ok = pl and n % 256 != 0
        elif mut == 'radius_not_scaled':
            ok = pl and proj and 0 < l1r < 1
        elif mut == 'l2_sqrt_radius':
            ok = pl and proj and l1r == 0
        elif mut == 'zero_radius_kept':
            ok = scene == 'zero_radius'
        elif mut == 'never_inside':
            ok = scene == 'edge_radius' and l1r > 0
        elif mut in ('support_ge', 'sign0'):
            ok = scene == 'ties' and proj and l1r > 0
        elif mut == 'nan_swallowed':                         # (at l1_ratio 0 the NaN reaches the scale and the row by itself; at
            # l1_ratio 1 an infinity makes the level NaN, 0 * inf, and the row with it: the old kernel was right there already)
            ok = scene.startswith('poisoned') and proj and (0 < l1r < 1 or (l1r == 1 and '_nan_' in scene))
        elif mut == 'swap_weights':
            ok = pl and op == 'scale' and l1r != 0.5
        elif mut == 'no_l2_zero_branch':
            ok = pl and op == 'scale' and l1r == 1
        if ok:
            out.append(case)
    return out


# ------------------------------------------------------------------------------------------------- the data-movement routes
TRANSPOSE_SHAPES = ((1, 1), (1, 33), (33, 1), (31, 32), (32, 32), (33, 65), (64, 31), (257, 3))
GATHER_CASES = [(n_rows, cols, pad, order) for n_rows in (1, 5, 300) for cols in (1, 255, 256, 257, 513)
                for pad, order in ((0, 'identity'), (0, 'reversed'), (3, 'repeated'), (5, 'reversed'))]
SWAP_CASES = [(n, rb) for n in (0, 1, 2, 7, 300) for rb in (4, 8, 12, 1028)]
CSR_ROWS = (1, 4, 5, 9)
CSR_LENS = (0, 1, 64, 65, 130)
GAVG_CASES = [(b, k) for b in (1, 3) for k in (1, 16, 17, 129)]
MOVE_MUTANTS = ('transpose_edge_le', 'transpose_swapped', 'gather_index_ignored', 'gather_dst_ld_cols', 'swaps_ascending',
                'swaps_inverse', 'csr_past_64', 'csr_last_group', 'gavg_w0')


def _values(shape, dt, seed):
    """distinct odd eighths, exactly representable in both dtypes: a wrong element cannot pass for the right one, none is a sentinel"""
    n = int(np.prod(shape))
    return ((np.random.RandomState(seed).permutation(n).astype(np.float64) - n // 3) / 4 + 0.125).reshape(shape).astype(DT[dt])


def transpose_restated(a, out_len, in_buf, mut=None):
    """-> the output buffer (rows * cols elements, then the guards)"""
    rows, cols = a.shape
    out = np.full(out_len, SENT, a.dtype)
    if mut == 'transpose_swapped':
        out[:rows * cols] = a.reshape(-1)                    # out[r * cols + c]
    else:
        out[:rows * cols] = a.T.reshape(-1)
    if mut == 'transpose_edge_le':                           # `<=` in both edge tests: an edge tile moves one more row and column
        for c in range(min(cols + 1, cdiv(cols, 32) * 32)):
            for r in range(min(rows + 1, cdiv(rows, 32) * 32)):
                if c == cols or r == rows:
                    out[c * rows + r] = in_buf[r * cols + c]
    return out


def gather_restated(src, idx, cols, dst_ld, mut=None):
    n_rows = len(idx)
    out = np.full(n_rows * dst_ld + GUARD, SENT, src.dtype)
    for r in range(n_rows):
        o = r * (cols if mut == 'gather_dst_ld_cols' else dst_ld)
        out[o:o + cols] = src[r if mut == 'gather_index_ignored' else idx[r], :cols]
    return out


def gather_inputs(case, dt):
    n_rows, cols, pad, order = case
    n_src = n_rows + 2
    src = np.full((n_src, cols + pad), SENT, DT[dt])
    src[:, :cols] = _values((n_src, cols), dt, zlib.crc32(repr(case).encode()))
    if order == 'identity':
        idx = np.arange(n_rows)
    elif order == 'reversed':
        idx = np.arange(n_src - 1, n_src - 1 - n_rows, -1)
    else:
        idx = np.random.RandomState(n_rows + cols).randint(0, n_src, n_rows) // 2 * 2 % n_src   # even rows only: repeats from 3 rows on
    return src, idx.astype(np.int64), cols + (pad + 1 if pad else 0)


def swaps_restated(a, swaps, mut=None):
    """random_fast.pyx:105-119: the swaps i = n - 1 .. 1, one after the other"""
    a = a.copy()
    n = len(a)
    if mut == 'swaps_inverse':
        perm = np.arange(n)
        for i in range(n - 1, 0, -1):
            perm[[i, swaps[i]]] = perm[[swaps[i], i]]
        out = a.copy()
        out[perm] = a
        return out
    for i in (range(1, n) if mut == 'swaps_ascending' else range(n - 1, 0, -1)):
        j = int(swaps[i])
        a[[i, j]] = a[[j, i]]
    return a


def swap_inputs(n, row_bytes):
    rs = np.random.RandomState(n * 7 + row_bytes)
    a = rs.randint(0, 256, size=(n, row_bytes)).astype(np.uint8)
    swaps = np.array([rs.randint(0, i + 1) for i in range(n)], dtype=np.int64)
    if n >= 7:
        swaps[n - 1], swaps[n - 2], swaps[1] = 0, n - 2, 0      # a far swap, a swap with itself, and the last one
    return a, swaps


def csr_inputs(n_rows, k):
    rs = np.random.RandomState(n_rows * 10 + k)
    n_cols = 140
    lens = [CSR_LENS[(u + n_rows) % len(CSR_LENS)] for u in range(n_rows)]
    if n_rows >= 5:
        lens[n_rows - 1] = 130                                 # the partly filled last group has a long row
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    indices = np.concatenate([np.sort(rs.permutation(n_cols)[:m]) for m in lens] + [np.zeros(0, np.int64)]).astype(np.int32)
    return rs.randn(n_rows, k), rs.randn(k, n_cols), indices, indptr, n_cols


def csr_reference(P, Q, indices, indptr):
    nnz, k = len(indices), P.shape[1]
    ref, bnd = np.full(nnz + GUARD, SENT, LD), np.zeros(nnz + GUARD)
    for u in range(len(indptr) - 1):
        for ii in range(indptr[u], indptr[u + 1]):
            terms = [Fraction(float(P[u, c])) * Fraction(float(Q[c, indices[ii]])) for c in range(k)]
            ref[ii] = LD(float(sum(terms)))
            bnd[ii] = k * U64 * float(sum(abs(t) for t in terms))
    return ref, bnd


def csr_restated(P, Q, indices, indptr, mut=None):
    out = np.full(len(indices) + GUARD, SENT)
    n_rows = len(indptr) - 1
    for u in range(n_rows // 4 * 4 if mut == 'csr_last_group' else n_rows):
        for ii in range(indptr[u], indptr[u + 1]):
            if mut == 'csr_past_64' and ii - indptr[u] >= 64:
                continue
            out[ii] = float(np.dot(P[u], Q[:, indices[ii]]))
    return out


def gavg_inputs(b, k, dt):
    rs = np.random.RandomState(b * 1000 + k)
    Ga = fl(rs.randn(b, k * k), dt)
    G = fl(rs.randn(k * k), dt)
    w = fl(np.array([(0.3, 0.0, 1.0)[i % 3] for i in range(b)]), dt)
    return Ga, G, w


def gavg_reference(Ga, G, w, dt):
    """(1 - w) Ga + w G exactly, rounded once; w == 0 leaves the bits, w == 1 gives G, otherwise three roundings of the dtype"""
    ref, bnd = Ga.astype(LD), np.zeros(Ga.shape)
    for i in range(len(w)):
        if w[i] == 1:
            ref[i] = G
        elif w[i] != 0:
            fw = Fraction(float(w[i]))
            t1 = [Fraction(float(x)) * (1 - fw) for x in Ga[i]]
            t2 = [Fraction(float(x)) * fw for x in G]
            ref[i] = [two(mp.mpf(x.numerator) / x.denominator) for x in map(sum, zip(t1, t2))]
            bnd[i] = [3 * UT[dt] * float(abs(x) + abs(y)) for x, y in zip(t1, t2)]
    pad = np.full(GUARD, SENT)
    return np.concatenate([ref.reshape(-1), pad.astype(LD)]), np.concatenate([bnd.reshape(-1), np.zeros(GUARD)])


def gavg_restated(Ga, G, w, dt, mut=None):
    out = np.empty_like(Ga)
    for i in range(len(w)):
        wi = w[0] if mut == 'gavg_w0' else w[i]
        out[i] = fl(fl(Ga[i] * fl(1.0 - wi, dt), dt) + fl(G * wi, dt), dt)
    return np.concatenate([out.reshape(-1), np.full(GUARD, SENT)]).astype(DT[dt])


# ------------------------------------------------------------------------------------------------------------- CPU tests
@pytest.fixture(scope='module')
def lib():
    from modl_amd import _lib
    return _lib.lib


PROJ_ROUTES = ('poisoned', 'zeros', 'l2/inside', 'l2/outside', 'quad/inside', 'quad/outside', 'lin/inside', 'lin/outside')
SCALE_ROUTES = ('l2!=0', 'l2==0,l1!=0', 'zero_row', 'poisoned')
SCENE_ROUTES = {                                             # what each scene is for, by row (r mod 3 where the rows differ)
    'planted': lambda l1r, r: ('l2' if l1r == 0 else 'lin' if l1r == 1 else 'quad') + '/outside',
    'near_l1': lambda l1r, r: 'quad/outside',
    'single': lambda l1r, r: ('lin' if l1r == 1 else 'quad') + '/outside',
    'shrink': lambda l1r, r: ('lin' if l1r == 1 else 'quad') + '/outside',
    'ties': lambda l1r, r: ('l2' if l1r == 0 else 'lin' if l1r == 1 else 'quad') + '/outside',
    'spread': lambda l1r, r: ('l2' if l1r == 0 else 'lin' if l1r == 1 else 'quad') + '/outside',
    'inside': lambda l1r, r: ('l2' if l1r == 0 else 'lin' if l1r == 1 else 'quad') + '/inside',
    'zero_radius': lambda l1r, r: 'zeros' if r % 3 < 2 else ('l2' if l1r == 0 else 'lin' if l1r == 1 else 'quad') + '/outside',
    'edge_radius': lambda l1r, r: ('l2' if l1r == 0 else 'lin' if l1r == 1 else 'quad') + ('/outside' if r % 3 == 1 else '/inside'),
}


def test_route_table():
    """every case takes the route its scene is for, by the exact reference AND by the restatement of the kernel; every route, every
    n, rows, layout and l1_ratio of the table is taken by some case, in both dtypes"""
    seen = {dt: set() for dt in DT}
    for case in ENET_CASES:
        op, dt, scene, n, rows, lay, l1r, alias = case
        seen[dt] |= {('n', op, n), ('rows', op, rows), ('lay', op, lay), ('l1r', op, l1r), ('alias', op, alias), (op, n, lay)}
        if op == 'norm':
            continue
        c, e = enet_build(case), enet_expected(case)
        for r in range(rows):
            route = e.rows[r].route
            seen[dt].add((op, route))
            if scene.startswith('poisoned'):
                assert (route == 'poisoned') == (r == 1)
                continue
            if op == 'scale':
                want = 'zero_row' if (scene == 'allzero' and r == 1) else 'l2==0,l1!=0' if l1r == 1 else 'l2!=0'
                assert route == want, (enet_id(case), r, route)
                continue
            assert route == SCENE_ROUTES[scene](l1r, r), (enet_id(case), r, route)
            res = restate_project(c.V[r], float(c.radius[r]), c.rho, dt)
            assert res.route == route, (enet_id(case), r, res.route, route)
            if route.endswith('/outside') and not route.startswith('l2'):
                assert res.m == e.rows[r].m, (enet_id(case), r, res.m, e.rows[r].m)      # the same support
                assert 2 <= res.passes + 1 < MAX_PASS
                if scene == 'single':
                    assert e.rows[r].m == 1
                    seen[dt].add('support of one')
                if scene == 'shrink':
                    assert res.passes >= 4, (enet_id(case), r, res.passes)
                    seen[dt].add('four passes')
    for dt in DT:
        for op in OPS:
            for n in ENET_N:
                assert ('n', op, n) in seen[dt] and all((op, n, lay) in seen[dt] for lay in LAYOUTS)
            assert all(('rows', op, x) in seen[dt] for x in ROWS) and all(('lay', op, x) in seen[dt] for x in LAYOUTS)
            assert all(('l1r', op, x) in seen[dt] for x in L1R)
        assert ('alias', 'projection', 0) in seen[dt] and ('alias', 'projection', 1) in seen[dt]
        assert all(('projection', x) in seen[dt] for x in PROJ_ROUTES), seen[dt]
        assert all(('scale', x) in seen[dt] for x in SCALE_ROUTES)
        assert 'support of one' in seen[dt] and 'four passes' in seen[dt]
    # the data-movement tables are the issue's
    assert {s for s in TRANSPOSE_SHAPES} == {(1, 1), (1, 33), (33, 1), (31, 32), (32, 32), (33, 65), (64, 31), (257, 3)}
    assert {c[0] for c in GATHER_CASES} == {1, 5, 300} and {c[1] for c in GATHER_CASES} == {1, 255, 256, 257, 513}
    assert {c[2] > 0 for c in GATHER_CASES} == {False, True} and {c[3] for c in GATHER_CASES} == {'identity', 'reversed', 'repeated'}
    for case in GATHER_CASES:
        src, idx, dst_ld = gather_inputs(case, 'f32')
        assert idx.min() >= 0 and idx.max() < src.shape[0] and len(idx) == case[0]         # every index in range
        assert case[3] != 'repeated' or case[0] < 3 or len(set(idx.tolist())) < len(idx)
    lens = set()
    for n_rows in CSR_ROWS:
        _, _, indices, indptr, n_cols = csr_inputs(n_rows, 6)
        lens |= set(np.diff(indptr).tolist())
        assert indices.max(initial=0) < n_cols and (n_rows % 4 == 0 or np.diff(indptr)[n_rows // 4 * 4:].sum() > 0)
    assert lens == set(CSR_LENS)
    assert 129 * 129 > 64 * 256 >= 17 * 17                                                # the grid-stride loop's second turn


def _sum_without(c, r, f):
    """row r of the case with element f left out of every sum (the writes are all made)"""
    x = c.V[r].copy()
    if c.op == 'norm':
        x[f] = 0.0
        return np.array([restate_norm(x, c.rho)])
    y = x.copy()
    y[f] = 0.0
    if c.op == 'scale':
        return x * scale_factor(y, float(c.radius[0]), c.rho, 'f64')
    ref = exact_project(y, float(c.radius[r]), c.rho, c.dt)
    if ref.l is None:
        return ref.ref.astype(np.float64)
    a = np.abs(x)
    return np.where(x >= 0, 1.0, -1.0) * np.where(a > ref.l, a - ref.l, 0.0) / (1 + ref.l * ref.gamma)


@pytest.mark.parametrize('dt', ('f32', 'f64'))
def test_cases_are_what_they_claim(dt):
    done = set()
    for case in ENET_CASES:
        if case[1] != dt:
            continue
        op, _, scene, n, rows, lay, l1r, alias = case
        c, e = enet_build(case), enet_expected(case)
        assert c.V.shape == (rows, n) and np.array_equal(fl(c.V, dt), c.V, equal_nan=True) and np.all(fl(c.radius, dt) == c.radius)
        assert np.all(np.asarray(c.buf) != SENT - 1) and not np.any(c.V == SENT)
        if op == 'projection' and rows > 1 and scene in ('planted', 'near_l1', 'spread', 'ties'):
            assert len(set(c.radius.tolist())) == rows                                   # a different radius for every row
        pos = positions(rows, n, c.ld, c.inc)
        if scene == 'planted':
            if (op, n, rows, l1r) in done:
                continue                                     # the rows of a scene are the same in every layout and aliasing
            done.add((op, n, rows, l1r))
            for r in range(rows):
                if op == 'projection' and e.rows[r].l is not None:
                    assert e.rows[r].margin >= 100                                       # the support is unambiguous
                for f in special_elements(n):
                    moved = _sum_without(c, r, f)
                    if op == 'norm':
                        ratio = abs(moved[0] - float(e.ref[r])) / e.bnd[r]
                    else:
                        b = e.bnd[pos[r]]
                        with np.errstate(divide='ignore', invalid='ignore'):
                            ratio = np.nanmax(np.where(b > 0, np.abs(moved - e.ref[pos[r]].astype(np.float64)) / b, 0.0))
                    assert ratio >= 100 or (n == 1 and op == 'scale'), (enet_id(case), r, f, ratio)
                    # (n == 1: the scale of a single entry is radius-determined whatever the entry; drop_last reads nothing there)
        elif scene == 'ties' and op == 'projection' and l1r > 0:
            for r in range(rows):
                x, l = c.V[r], e.rows[r].l
                assert e.rows[r].margin >= 100
                assert np.count_nonzero(np.abs(x) == 1.5) >= 2 and 1.5 > l               # exact duplicates above the level
                assert np.any((x == 0) & ~np.signbit(x)) and np.any((x == 0) & np.signbit(x))
                z = e.ref[pos[r]][(x == 0)]
                assert np.all(z == 0) and not np.any(np.signbit(z))                      # sign(-0) = +1: +0 comes out
        elif scene == 'edge_radius':
            nr = _norms(c.V, c.rho)
            for r in range(rows):
                want = (nr[r], _below(nr[r], dt), _above(nr[r], dt))[r % 3]
                assert c.radius[r] == want and _below(nr[r], dt) < nr[r] < _above(nr[r], dt)
                assert np.any(c.V[r] == 0)
        elif scene == 'spread' and n > 1:
            a = np.abs(c.V)
            assert a.min() < 2.0 ** -59 and a.max() >= 2.0 ** 40
        elif scene == 'near_l1':
            assert l1r == 0.999 and all(x.kappa > 50 for x in e.rows), [x.kappa for x in e.rows]
        elif scene.startswith('poisoned'):
            bad = ~np.isfinite(c.V)
            assert bad.sum() == 1 and bad[1, 0 if scene.endswith('first') else n - 1]
            if op == 'norm':
                assert not np.isfinite(e.ref[1]) and np.all(np.isfinite(e.ref[[0, 2]]))
                assert np.isnan(e.ref[1]) == (np.isnan(c.V[1]).any() or c.rho == 1.0)
            else:
                assert np.all(np.isnan(e.ref[pos[1]])) and np.all(np.isfinite(e.ref[pos[[0, 2]]]))
                # the other rows are the rows of the same call without the poison
                V2 = c.V.copy()
                V2[1] = 1.0
                for r in (0, 2):
                    x = exact_project(V2[r], float(c.radius[r]), c.rho, dt) if op == 'projection' else \
                        exact_scale(V2[r], float(c.radius[r]), c.rho, dt)
                    assert np.array_equal(x.ref, e.ref[pos[r]])


@pytest.mark.parametrize('dt', ('f32', 'f64'))
def test_judge_accepts_restatement(dt):
    worst = {}
    for case in ENET_CASES:
        if case[1] == dt:
            c, e = enet_build(case), enet_expected(case)
            got = restate_enet_call(c)
            w, why = judge_enet(c, e, got)
            assert why is None and w <= 1, why
            if gamma_case(case):
                worst['spread at 0.999'] = max(worst.get('spread at 0.999', 0.0), w)
                worst['the same without the gamma term'] = max(worst.get('the same without the gamma term', 0.0),
                                                               judge(got['out'], e.ref, e.bnd_nogamma)[0])
            worst[case[0]] = max(worst.get(case[0], 0.0), w)
    for a, out_len, in_buf in _transpose_cases(dt):
        assert judge(transpose_restated(a, out_len, in_buf), transpose_restated(a, out_len, in_buf), np.zeros(out_len))[1] is None
    for b, k in GAVG_CASES:
        Ga, G, w = gavg_inputs(b, k, dt)
        ref, bnd = gavg_reference(Ga, G, w, dt)
        r, why = judge(gavg_restated(Ga, G, w, dt), ref, bnd, 'G_average b%d k%d' % (b, k))
        assert why is None, why
    if dt == 'f64':
        for n_rows in CSR_ROWS:
            for k in (1, 6):
                P, Q, indices, indptr, _ = csr_inputs(n_rows, k)
                ref, bnd = csr_reference(P, Q, indices, indptr)
                assert judge(csr_restated(P, Q, indices, indptr), ref, bnd, 'csr')[1] is None
    print('\nrestatement, largest |got - ref| / bound (%s): %s' % (dt, worst))


def _transpose_cases(dt):
    for rows, cols in TRANSPOSE_SHAPES:
        a = _values((rows, cols), dt, rows * 100 + cols)
        in_buf = np.concatenate([a.reshape(-1), np.full(cols + GUARD, SENT - 2, DT[dt])])     # the guards of the input read as 5.5
        yield a, rows * cols + rows + GUARD, in_buf


@pytest.mark.parametrize('mut', ENET_MUTANTS)
@pytest.mark.parametrize('dt', ('f32', 'f64'))
def test_judge_rejects_mutants(dt, mut):
    cases = enet_mutant_cases(mut)
    assert {c[1] for c in cases} == {'f32', 'f64'} and len(cases) >= 4, mut
    for case in cases:
        if case[1] == dt:
            c, e = enet_build(case), enet_expected(case)
            _, why = judge_enet(c, e, restate_enet_call(c, mut))
            assert why is not None, (mut, enet_id(case))


@pytest.mark.parametrize('dt', ('f32', 'f64'))
def test_support_ge_is_no_mistake(dt):
    """`a >= level` for `a > level` in the active-set loop is the one listed mutant that no judge of the output can reject, because
    it is the same projection: an entry equal to the level adds a(1 + gamma a / 2) to S and 1 to the count, and the root of the
    level equation on the larger support is the same level (its u = 0 adds nothing to either side of sum u (1 + gamma u / 2) = R);
    entries at level 0 (the zeros) only make the first level lower, from where the levels still rise to the same fixed point.  Held
    here on the scene built for it - exact duplicates, zeros and -0.0, every l1_ratio above 0: the judge accepts the mutant, and
    its support is the restatement's."""
    cases = enet_mutant_cases('support_ge')
    assert len([c for c in cases if c[1] == dt]) >= 8
    for case in cases:
        if case[1] == dt:
            c, e = enet_build(case), enet_expected(case)
            got = restate_enet_call(c, 'support_ge')
            w, why = judge_enet(c, e, got)
            assert why is None and w <= 1, why
            for r in range(c.rows):
                assert restate_project(c.V[r], float(c.radius[r]), c.rho, dt, 'support_ge').m >= e.rows[r].m


@pytest.mark.parametrize('mut', MOVE_MUTANTS)
@pytest.mark.parametrize('dt', ('f32', 'f64'))
def test_judge_rejects_movement_mutants(dt, mut):
    n = 0
    if mut.startswith('transpose'):
        for a, out_len, in_buf in _transpose_cases(dt):
            if (mut == 'transpose_swapped' and 1 in a.shape) or (mut == 'transpose_edge_le' and a.shape == (32, 32)):
                continue                                     # a vector: both index orders are the same copy; no edge tile
            why = judge(transpose_restated(a, out_len, in_buf, mut), transpose_restated(a, out_len, in_buf), np.zeros(out_len))[1]
            assert why is not None, (mut, a.shape)
            n += 1
    elif mut.startswith('gather'):
        for case in GATHER_CASES:
            src, idx, dst_ld = gather_inputs(case, dt)
            if (mut == 'gather_index_ignored' and np.array_equal(idx, np.arange(len(idx)))) or (mut == 'gather_dst_ld_cols' and (dst_ld == case[1] or case[0] == 1)):
                continue
            ref = gather_restated(src, idx, case[1], dst_ld)
            assert judge(gather_restated(src, idx, case[1], dst_ld, mut), ref, np.zeros(len(ref)))[1] is not None, (mut, case)
            n += 1
    elif mut.startswith('swaps'):
        for nn, rb in SWAP_CASES:
            a, swaps = swap_inputs(nn, rb)
            if nn < 7:
                continue                                     # (up to two rows both orders and the inverse agree)
            assert not np.array_equal(swaps_restated(a, swaps, mut), swaps_restated(a, swaps)), (mut, nn, rb)
            n += 1
    elif mut.startswith('csr'):
        if dt == 'f32':
            return                                           # modl_predict_csr is float64 only
        for n_rows in CSR_ROWS:
            for k in (1, 6):
                P, Q, indices, indptr, _ = csr_inputs(n_rows, k)
                lens = np.diff(indptr)
                if (mut == 'csr_past_64' and lens.max() <= 64) or (mut == 'csr_last_group' and (n_rows % 4 == 0 or lens[n_rows // 4 * 4:].sum() == 0)):
                    continue
                ref, bnd = csr_reference(P, Q, indices, indptr)
                assert judge(csr_restated(P, Q, indices, indptr, mut), ref, bnd)[1] is not None, (mut, n_rows, k)
                n += 1
    else:
        for b, k in GAVG_CASES:
            if b == 1:
                continue
            Ga, G, w = gavg_inputs(b, k, dt)
            ref, bnd = gavg_reference(Ga, G, w, dt)
            assert judge(gavg_restated(Ga, G, w, dt, mut), ref, bnd)[1] is not None, (mut, b, k)
            n += 1
    assert n >= 2, mut


def test_mutants_are_the_issues_list():
    assert len(ENET_MUTANTS) == 14 and len(MOVE_MUTANTS) == 9
    with open(__file__.replace('.pyc', '.py')) as f:
        doc = f.read().split('"""')[1]
    for mut in ENET_MUTANTS + MOVE_MUTANTS:
        assert re.search(r'^  %s ' % mut, doc, re.M), mut


def test_swaps_host_against_the_loop(lib):
    """modl_apply_swaps_rows against the sequential swaps, and its refusals: nothing moves"""
    for n, rb in SWAP_CASES:
        a, swaps = swap_inputs(n, rb)
        got = a.copy()
        assert lib.modl_apply_swaps_rows(got.ctypes.data_as(C.c_void_p), n, rb, swaps.ctypes.data_as(C.c_void_p)) == 0
        assert np.array_equal(got, swaps_restated(a, swaps)), (n, rb)
    for n, rb in ((7, 12), (300, 4)):
        a, swaps = swap_inputs(n, rb)
        for i, j in ((1, 2), (n - 1, n), (1, -1), (n - 1, -1), (n // 2, n // 2 + 1)):
            bad, got = swaps.copy(), a.copy()
            bad[i] = j
            assert lib.modl_apply_swaps_rows(got.ctypes.data_as(C.c_void_p), n, rb, bad.ctypes.data_as(C.c_void_p)) == EINVAL
            assert np.array_equal(got, a), (n, rb, i, j)


# ------------------------------------------------------------------------------------------------------------- GPU tests
WORST = {}


def _note(key, w):
    WORST[key] = max(WORST.get(key, 0.0), w)


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _stream():
    from modl_amd import device as dev
    return dev.stream_ptr(dev.default_device())


def run_enet(lib, c):
    """the entry point on the case's buffer -> {'out': ...}; outputs of SENT with GUARD elements behind, padding included"""
    import torch
    from modl_amd.device import ptr
    buf = _cuda(c.buf)
    f = getattr(lib, 'modl_enet_%s_%s' % (c.op, c.dt))
    if c.op == 'norm':
        out = torch.full((c.rows + GUARD,), SENT, dtype=buf.dtype, device='cuda')
        rc = f(ptr(buf), c.rows, c.n, c.ld, c.inc, c.rho, ptr(out), _stream())
    elif c.op == 'projection':
        out = buf if c.alias else torch.full((len(c.buf),), SENT, dtype=buf.dtype, device='cuda')
        rc = f(ptr(buf), ptr(out), c.rows, c.n, c.ld, c.inc, ptr(_cuda(c.radius.astype(DT[c.dt]))), c.rho, _stream())
    else:
        out = buf
        rc = f(ptr(buf), c.rows, c.n, c.ld, c.inc, c.rho, float(c.radius[0]), _stream())
    assert rc == 0
    torch.cuda.synchronize()
    if out is not buf:
        assert buf.cpu().numpy().tobytes() == c.buf.tobytes(), 'the input changed'
    return {'out': out.cpu().numpy()}


@pytest.mark.gpu
@pytest.mark.parametrize('scene', ('planted', 'other', 'poisoned'))
@pytest.mark.parametrize('dt', ('f32', 'f64'))
@pytest.mark.parametrize('op', OPS)
def test_enet_against_exact(lib, op, dt, scene):
    bad = []
    for case in ENET_CASES:
        kind = 'planted' if case[2] == 'planted' else 'poisoned' if case[2].startswith('poisoned') else 'other'
        if case[0] != op or case[1] != dt or kind != scene:
            continue
        c, e = enet_build(case), enet_expected(case)
        got = run_enet(lib, c)
        detail = {}
        w, why = judge_enet(c, e, got, detail)
        if why is not None:
            bad.append(why)
            continue
        pos = positions(c.rows, c.n, c.ld, c.inc)
        for r in range(c.rows):                              # per row: its own elements (the norm: its own figure)
            at = np.array([r]) if op == 'norm' else pos[r]
            _note((op, dt, e.rows[r].route), judge(got['out'][at], e.ref[at], e.bnd[at])[0])
        if 'norm_check' in detail:
            _note((op, dt, 'norm of the result against the radius'), detail['norm_check'])
        if gamma_case(case):
            _note(('projection', dt, 'spread at l1_ratio 0.999'), w)
            _note(('projection', dt, 'spread at 0.999 WITHOUT the gamma term (a record)'), judge(got['out'], e.ref, e.bnd_nogamma)[0])
        if case[2] == 'near_l1':
            _note(('projection', dt, 'near_l1 with kappa'), w)
            _note(('projection', dt, 'near_l1 WITHOUT kappa (a record)'), judge(got['out'], e.ref, e.bnd_nokappa)[0])
        if case[2].startswith('poisoned'):                   # the clean rows: the bits of the same call without the poison
            V2 = c.V.copy()
            V2[1] = 1.0
            c2 = SimpleNamespace(**dict(vars(c), V=V2, buf=pack(V2, c.ld, c.inc, c.size, dt)))
            clean = run_enet(lib, c2)['out']
            for r in (0, 2):
                w_ = np.array([r]) if op == 'norm' else r * c.ld + np.arange(c.n) * c.inc
                if got['out'][w_].tobytes() != clean[w_].tobytes():
                    bad.append('%s: row %d is not the row of the clean call' % (c.id, r))
    assert not bad, '%d cases, first: %s' % (len(bad), bad[:3])


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ('f32', 'f64'))
def test_enet_rerun_and_placement_same_bits(lib, dt):
    """the same call twice, contiguous and as columns; a row alone, contiguous and as a column, against the same row as row 2 of
    the call (of 5 rows, of 3 in the `spread` point) - at l1_ratio 0.15, 1, 0 and 0.5"""
    for op in OPS:
        for scene, n, rows, l1r in (('planted', 257, 5, 0.15), ('planted', 1025, 5, 1.0), ('planted', 65, 5, 0.0),
                                    ('spread', 255, 3, 0.5)):
            V, rad, rho = _rows_of(dt, scene, n, rows, l1r)
            assert V.shape == (rows, n)
            outs = []
            for lay, sel in (('contig', None), ('contig', None), ('col', None), ('contig', 2), ('colwide', 2)):
                Vs, rs_ = (V, rad) if sel is None else (V[sel:sel + 1], rad[sel:sel + 1])
                ld, inc, size = layout(lay, Vs.shape[0], n)
                c = SimpleNamespace(op=op, dt=dt, n=n, rows=Vs.shape[0], rho=rho, alias=0, ld=ld, inc=inc, size=size, V=Vs,
                                    radius=fl(np.full(len(rs_), 1.5), dt) if op == 'scale' else rs_,
                                    buf=pack(Vs, ld, inc, size, dt), id='rerun')
                o = run_enet(lib, c)['out']
                o = o[:c.rows] if op == 'norm' else o[positions(c.rows, n, ld, inc)]
                outs.append(o if sel is None else (sel, o))
            assert outs[0].tobytes() == outs[1].tobytes() == outs[2].tobytes(), (op, scene, n, l1r)
            for sel, o in outs[3:]:
                assert o[0].tobytes() == outs[0][sel].tobytes(), (op, scene, n, l1r, sel)


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ('f32', 'f64'))
def test_transpose_exact(lib, dt):
    import torch
    from modl_amd.device import ptr
    f = getattr(lib, 'modl_transpose_' + dt)
    for a, out_len, in_buf in _transpose_cases(dt):
        rows, cols = a.shape
        src, out = _cuda(in_buf), torch.full((out_len,), SENT, dtype=_cuda(in_buf).dtype, device='cuda')
        assert f(ptr(src), ptr(out), rows, cols, _stream()) == 0
        torch.cuda.synchronize()
        why = judge(out.cpu().numpy(), transpose_restated(a, out_len, in_buf), np.zeros(out_len), 'transpose %dx%d' % a.shape)[1]
        assert why is None, why
    _note(('transpose', dt, 'exact'), 0.0)


@pytest.mark.gpu
def test_transpose_at_the_y_axis_limit(lib):
    """32 * 65536 rows of one column: the largest y extent the entry point lets through is one the device takes"""
    import torch
    from modl_amd.device import ptr
    rows = 32 * MAX_GRID_Y
    src = torch.arange(rows, dtype=torch.float32, device='cuda')
    out = torch.full((rows + GUARD,), SENT, dtype=torch.float32, device='cuda')
    assert lib.modl_transpose_f32(ptr(src), ptr(out), rows, 1, _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(out[:rows], src) and bool((out[rows:] == SENT).all())
    assert lib.modl_transpose_f32(ptr(src), ptr(out), rows + 1, 1, _stream()) == EINVAL


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ('f32', 'f64'))
def test_gather_rows_exact(lib, dt):
    import torch
    from modl_amd.device import ptr
    f = getattr(lib, 'modl_gather_rows_' + dt)
    for case in GATHER_CASES:
        n_rows, cols = case[:2]
        src, idx, dst_ld = gather_inputs(case, dt)
        ref = gather_restated(src, idx, cols, dst_ld)
        dsrc, out = _cuda(src), torch.full((len(ref),), SENT, dtype=_cuda(src).dtype, device='cuda')
        assert f(ptr(dsrc), src.shape[1], ptr(_cuda(idx)), n_rows, cols, ptr(out), dst_ld, _stream()) == 0
        torch.cuda.synchronize()
        why = judge(out.cpu().numpy(), ref, np.zeros(len(ref)), 'gather %r' % (case,))[1]
        assert why is None, why
        assert dsrc.cpu().numpy().tobytes() == src.tobytes()
    _note(('gather_rows', dt, 'exact'), 0.0)


@pytest.mark.gpu
def test_swaps_device_host_and_loop_agree(lib):
    import torch
    from modl_amd.device import ptr
    for n, rb in SWAP_CASES:
        a, swaps = swap_inputs(n, rb)
        host = a.copy()
        assert lib.modl_apply_swaps_rows(host.ctypes.data_as(C.c_void_p), n, rb, swaps.ctypes.data_as(C.c_void_p)) == 0
        buf = np.concatenate([a.reshape(-1), np.full(16, 0xA5, np.uint8)])
        d = _cuda(buf) if len(buf) else torch.zeros(16, dtype=torch.uint8, device='cuda')
        assert lib.modl_apply_swaps_rows_device(ptr(d), n, rb, swaps.ctypes.data_as(C.c_void_p), _stream()) == 0
        torch.cuda.synchronize()
        got = d.cpu().numpy()
        assert np.all(got[n * rb:] == 0xA5), 'guard'
        assert np.array_equal(got[:n * rb].reshape(n, rb), host) and np.array_equal(host, swaps_restated(a, swaps)), (n, rb)
    a, swaps = swap_inputs(7, 12)
    d = _cuda(a.reshape(-1))
    for i, j in ((1, 2), (6, 7), (1, -1), (6, -1)):
        bad = swaps.copy()
        bad[i] = j
        assert lib.modl_apply_swaps_rows_device(ptr(d), 7, 12, bad.ctypes.data_as(C.c_void_p), _stream()) == EINVAL
    assert lib.modl_apply_swaps_rows_device(ptr(d), 14, 6, np.arange(14).ctypes.data_as(C.c_void_p), _stream()) == EINVAL
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), a.reshape(-1))
    _note(('apply_swaps_rows', 'bytes', 'exact'), 0.0)


@pytest.mark.gpu
def test_predict_csr_against_fsum(lib):
    import torch
    from modl_amd.device import ptr
    for n_rows in CSR_ROWS:
        for k in (1, 6):
            P, Q, indices, indptr, n_cols = csr_inputs(n_rows, k)
            ref, bnd = csr_reference(P, Q, indices, indptr)
            data = torch.full((len(indices) + GUARD,), SENT, dtype=torch.float64, device='cuda')
            ind = _cuda(indices) if len(indices) else torch.zeros(1, dtype=torch.int32, device='cuda')
            assert lib.modl_predict_csr(ptr(data), ptr(ind), ptr(_cuda(indptr)), ptr(_cuda(P)), n_rows, k, ptr(_cuda(Q)), n_cols,
                                        _stream()) == 0
            torch.cuda.synchronize()
            w, why = judge(data.cpu().numpy(), ref, bnd, 'predict_csr rows %d k %d' % (n_rows, k))
            assert why is None, why
            _note(('predict_csr', 'f64', 'all'), w)


@pytest.mark.gpu
@pytest.mark.parametrize('dt', ('f32', 'f64'))
def test_update_G_average_against_exact(lib, dt):
    import torch
    from modl_amd.device import ptr
    for b, k in GAVG_CASES:
        Ga, G, w = gavg_inputs(b, k, dt)
        ref, bnd = gavg_reference(Ga, G, w, dt)
        d = _cuda(np.concatenate([Ga.reshape(-1), np.full(GUARD, SENT)]).astype(DT[dt]))
        assert getattr(lib, 'modl_update_G_average_' + dt)(ptr(d), ptr(_cuda(G.astype(DT[dt]))), ptr(_cuda(w.astype(DT[dt]))), b, k,
                                                           _stream()) == 0
        torch.cuda.synchronize()
        r, why = judge(d.cpu().numpy(), ref, bnd, 'G_average b%d k%d' % (b, k))
        assert why is None, why
        _note(('update_G_average', dt, 'all'), r)


@pytest.mark.gpu
def test_report():
    """the largest |got - ref| / bound of this run per entry point, dtype and route: recorded in the docstring and in DESIGN.md; the
    judge's own 1 is what is asserted (the figure WITHOUT kappa is a record of the level equation's loss, not a check)"""
    print('\nhelper routes: largest |got - ref| / bound')
    for key in sorted(WORST):
        print('  %-18s %-5s %-34s %.3f' % (key + (WORST[key],)))
    assert all(v <= 1 for k, v in WORST.items() if 'record' not in k[2])
