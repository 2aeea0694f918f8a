"""Benchmark of scoring rows with missing entries: Coder.held_out_error, the modl_masked_objective_* launch behind it,
and what a user composed before it existed.

    python scripts/bench_masked_score.py                 # 20 000 rows, p = 192, k = 256, half the entries missing, f32 + f64
    python scripts/bench_masked_score.py --rows 2000 --components 32 --no-trace

Writes profiles/masked_score_bench.json (--out), per dtype:
  held_out_error   wall time end to end, rows and mask resident on the device (the hold-out is drawn on the host, the rows
                   are coded on mask & ~H, one objective launch, eight numbers come back), and the figures it returns;
  objective        the launch pair alone on resident operands and given codes: wall time per call including the read-back
                   of the eight numbers and, from a `rocprofv3 --kernel-trace --stats` run of its own, the kernel time of
                   the tile kernel and of the final one-workgroup sum; the FLOP of the n x p x k product and the bytes the
                   launch must move (X, the selection bytes, the codes, the dictionary, the partial sums), and the TFLOP/s
                   and GB/s these imply over the tile kernel's time;
  composed         the same figures from the public pieces of before: transform(X, mask & ~H) + inverse_transform + a
                   masked torch reduction (an n x p reconstruction written and read back), in all and without the coding.
There is no earlier number for any of these: none is a threshold.  Every GPU step is a child process under its own
`timeout`; the parent never touches the GPU.
"""
import argparse
import glob
import json
import os
import shutil
import sqlite3
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DTYPES = ('f32', 'f64')


def problem(a, dt):
    """(coder, X, mask, H) on the device: rows that are sparse combinations of the atoms plus noise"""
    import numpy as np
    import torch
    from modl_amd import Coder
    T = np.float32 if dt == 'f32' else np.float64
    rs = np.random.RandomState(0)
    D = rs.randn(a.components, a.features)
    D /= np.linalg.norm(D, axis=1, keepdims=True)
    code = rs.randn(a.rows, a.components) * (rs.rand(a.rows, a.components) < 8.0 / a.components)
    X = (code @ D + 0.05 * rs.randn(a.rows, a.features)).astype(T)
    mask = rs.rand(a.rows, a.features) >= a.missing
    H = np.random.RandomState(0).random_sample((a.rows, a.features)) < a.held_out     # held_out_error's draw, random_state=0
    coder = Coder(D.astype(T), code_alpha=a.alpha)
    return coder, torch.from_numpy(X).cuda(), torch.from_numpy(mask).cuda(), torch.from_numpy(H).cuda()


def timed(f, reps):
    import torch
    f()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = f()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return sorted(ts)[len(ts) // 2] * 1e3, out


def child_wall(a):
    import torch
    out = {}
    for dt in DTYPES:
        coder, X, mask, H = problem(a, dt)
        be = coder._backend
        ms, err = timed(lambda: coder.held_out_error(X, mask=mask, held_out=a.held_out, random_state=0), a.reps)
        rec = dict(held_out_error=dict(ms=round(ms, 2), rmse=err.rmse, rmse_coded=err.rmse_coded, n_held_out=err.n_held_out,
                                       n_coded=err.n_coded))
        coded = mask & ~H
        sel = mask.to(torch.uint8) * (1 + H.to(torch.uint8))
        code = coder.transform(X, mask=coded)
        ms, s = timed(lambda: be.masked_objective(X, sel, code), 10 * a.reps)
        rec['objective'] = dict(wall_ms_per_call=round(ms, 3), out8=[float(v) for v in s])

        def composed(code=None):
            c = coder.transform(X, mask=coded) if code is None else code
            r2 = (coder.inverse_transform(c) - X).double() ** 2
            zero = torch.zeros((), dtype=torch.float64, device=X.device)
            held, cod = mask & H, coded
            return (float(torch.sqrt(torch.where(held, r2, zero).sum() / held.sum())),
                    float(torch.sqrt(torch.where(cod, r2, zero).sum() / cod.sum())))
        ms_all, figures = timed(composed, a.reps)
        ms_tail, _ = timed(lambda: composed(code), 10 * a.reps)
        rec['composed'] = dict(ms=round(ms_all, 2), ms_without_coding=round(ms_tail, 3), rmse=figures[0], rmse_coded=figures[1])
        out[dt] = rec
        del coder, X, mask, H, sel, code
        torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)


def child_trace(a):
    """per dtype: the objective launch pair a.trace_calls times on given codes (zeros: the time does not depend on them)"""
    import torch
    for dt in DTYPES:
        coder, X, mask, H = problem(a, dt)
        sel = mask.to(torch.uint8) * (1 + H.to(torch.uint8))
        code = torch.zeros((a.rows, a.components), dtype=X.dtype, device=X.device)
        for _ in range(a.trace_calls):
            coder._backend.masked_objective(X, sel, code)
        torch.cuda.synchronize()


def summarise_trace(db_path, a):
    rows = sqlite3.connect(db_path).execute('select name, duration from kernels order by start').fetchall()
    out = {}
    for dt, tags, e in (('f32', ('<float', 'IfLb0'), 4), ('f64', ('<double', 'IdLb0'), 8)):      # demangled or not
        tile = [r[1] / 1e3 for r in rows if 'masked_tile_kernel' in r[0] and any(t in r[0] for t in tags)]
        assert len(tile) == a.trace_calls, (dt, len(tile), sorted(set(r[0][:100] for r in rows)))
        tile = sorted(tile[1:])
        us = tile[len(tile) // 2]
        n, p, k = a.rows, a.features, a.components
        flop = 2.0 * n * p * k
        nbytes = n * p * (e + 1) + n * k * e + p * k * e + ((n + 63) // 64) * ((p + 63) // 64) * 64
        out[dt] = dict(tile_kernel_us=round(us, 2), flop=flop, bytes=nbytes, TFLOP_per_s=round(flop / us / 1e6, 3),
                       GB_per_s=round(nbytes / us / 1e3, 1))
    fin = sorted(r[1] / 1e3 for r in rows if 'masked_objective_final_kernel' in r[0])
    for dt in DTYPES:
        out[dt]['final_kernel_us'] = round(fin[len(fin) // 2], 2)
    return out


def run_child(cmd, limit):
    r = subprocess.run(['timeout', '-k', '10', str(limit)] + cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit('bench_masked_score: `%s` ended with status %d; nothing more is started' % (' '.join(cmd), r.returncode))
    return r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=20000)
    ap.add_argument('--features', type=int, default=192)
    ap.add_argument('--components', type=int, default=256)
    ap.add_argument('--alpha', type=float, default=0.1)
    ap.add_argument('--missing', type=float, default=0.5)
    ap.add_argument('--held-out', type=float, default=0.1)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--trace-calls', type=int, default=11)
    ap.add_argument('--no-trace', action='store_true')
    ap.add_argument('--timeout', type=int, default=300, help='seconds per GPU child process')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'masked_score_bench.json'))
    ap.add_argument('--child', choices=['wall', 'trace'])
    a = ap.parse_args()
    if a.child:
        return child_wall(a) if a.child == 'wall' else child_trace(a)
    me = [sys.executable, os.path.abspath(__file__)] + [str(v) for v in (
        '--rows', a.rows, '--features', a.features, '--components', a.components, '--alpha', a.alpha, '--missing', a.missing,
        '--held-out', a.held_out, '--reps', a.reps, '--trace-calls', a.trace_calls)]
    rec = dict(date=time.strftime('%Y-%m-%d'), command='python scripts/bench_masked_score.py', rows=a.rows, p=a.features,
               k=a.components, missing=a.missing, held_out=a.held_out, code_alpha=a.alpha)
    rec.update(json.loads(run_child(me + ['--child', 'wall'], a.timeout).strip().splitlines()[-1]))
    if a.no_trace:
        for dt in DTYPES:
            rec[dt]['objective']['kernel'] = 'not measured'
    else:
        tmp = tempfile.mkdtemp(prefix='masked_score_trace_')
        try:
            run_child(['rocprofv3', '--kernel-trace', '--stats', '-d', tmp, '-o', 't', '--'] + me + ['--child', 'trace'],
                      a.timeout)
            dbs = glob.glob(os.path.join(tmp, '**', '*.db'), recursive=True)
            assert dbs, 'rocprofv3 left no database under %s' % tmp
            for dt, k in summarise_trace(dbs[0], a).items():
                rec[dt]['objective']['kernel'] = k
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(rec), flush=True)
    with open(a.out, 'w') as f:
        json.dump(rec, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
