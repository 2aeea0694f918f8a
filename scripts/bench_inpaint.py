"""Benchmark of ImageDictFact.inpaint (masked grid patches -> per-window Gram and Dx -> multi-Gram solve -> decode with
unscale -> weighted overlap-add -> finish).

    python scripts/bench_inpaint.py                      # 512 x 512 x 3 f32, 8 x 8 patches, k = 256, 50 % missing, strides 4 and 1
    python scripts/bench_inpaint.py --size 128 --components 32 --stride 4 --no-trace

Writes profiles/inpaint_bench.json (--out), one record per stride:
  call_ms        wall time of one inpaint() call, image in host memory to image in host memory, profiler off (median of
                 --reps, after a warm-up call);
  stages         from a `rocprofv3 --kernel-trace --stats` run of its own, the dispatches of ONE call: per stage the
                 launches, the total and the per-launch time; `solver` is every kernel that is none of the named stages
                 (the coordinate descent and what surrounds it, the torch plumbing of the split included);
  masked_gram    of that stage: the FLOP it must do (the upper-triangle tiles of 64 x 64 it computes, 2 p per element, plus
                 Dx), the bytes it writes (b k^2 + b k elements) and the TFLOP/s and GB/s these imply, beside the yardsticks:
                 the project's plain f32 tile product (decode, profiles/reconstruct_bench.json) and the HBM write rate;
  solver_share   the solver's share of the kernel time of the call.
Every GPU step is a child process under its own `timeout`; the parent never touches the GPU.
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
STAGES = (('grid_patches_masked', 'image_grid_patches_masked_kernel'), ('masked_gram', 'masked_gram_kernel'),
          ('decode', 'EpiUnscale'), ('overlap_add_weighted', 'image_overlap_add_weighted_kernel'),
          ('finish', 'image_inpaint_finish_kernel'))
YARDSTICKS = dict(f32_tile_product_TFLOPs=25.0, hbm_write_note='MI355X HBM3E: 8 TB/s peak')


def holed(a):
    """(estimator fitted on the clean image, the image with --missing of its elements set to -1)"""
    import numpy as np
    from bench_reconstruct import fitted
    est, img = fitted(a)
    rs = np.random.RandomState(1)
    img = img.copy()
    img[rs.rand(*img.shape) < a.missing] = -1
    return est, img


def child_wall(a):
    import numpy as np
    import torch
    est, img = holed(a)
    stride = a.stride[0]
    est.inpaint(img, stride=stride)                                         # warm-up
    ts = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out, filled = est.inpaint(img, stride=stride, return_filled=True)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    from bench_reconstruct import synth_image
    clean = synth_image(a.size, a.size, a.channels)
    miss = img == -1
    # windows with a hole but not empty, counted on the host (an integral image of the observed elements)
    from modl_amd.image import grid_origins
    ii = np.zeros((a.size + 1, a.size + 1), dtype=np.int64)
    ii[1:, 1:] = (~miss).sum(axis=2).cumsum(axis=0).cumsum(axis=1)
    o = grid_origins(img.shape, (a.patch, a.patch), stride)
    i0, j0, i1, j1 = o[:, 0], o[:, 1], o[:, 0] + a.patch, o[:, 1] + a.patch
    nobs = ii[i1, j1] - ii[i0, j1] - ii[i1, j0] + ii[i0, j0]
    n_holed = int(((nobs > 0) & (nobs < a.patch * a.patch * a.channels)).sum())
    print(json.dumps(dict(n_holed=n_holed, n_clean=int((nobs == a.patch * a.patch * a.channels).sum()),
                          n_empty=int((nobs == 0).sum()), call_ms=round(float(np.median(ts)), 3), call_ms_all=[round(t, 3) for t in ts],
                          filled_share=round(float(filled.mean()), 4),
                          psnr_db_on_missing=round(float(-10 * np.log10(np.mean((out[miss] - clean[miss]) ** 2))), 2))),
          flush=True)


def child_trace(a):
    import torch
    est, img = holed(a)
    for _ in range(2):                                                      # the trace's last call is the measured one
        est.inpaint(img, stride=a.stride[0])
    torch.cuda.synchronize()


def gram_work(n_holed, k, p, e):
    """FLOP and bytes written of modl_masked_gram_* for n_holed rows, from the shapes alone"""
    t = -(-k // 64)
    tiles = t * (t + 1) // 2
    flop = n_holed * (tiles * 64 * 64 * 2 * p + t * 64 * 2 * p)
    return flop, n_holed * (k * k + k) * e


def summarise_trace(db_path, n_holed, k, p, e):
    rows = sqlite3.connect(db_path).execute('select name, duration, start from kernels order by start').fetchall()
    fin = [i for i, r in enumerate(rows) if STAGES[4][1] in r[0]]
    assert len(fin) >= 2, 'two inpaint calls expected in the trace'
    call = rows[fin[-2] + 1:fin[-1] + 1]
    call = call[next(i for i, r in enumerate(call) if STAGES[0][1] in r[0]):]    # (the upload / mask kernels before it)
    out = {}
    for r in call:
        stage = next((s for s, pat in STAGES if pat in r[0]), 'solver')
        o = out.setdefault(stage, dict(launches=0, total_us=0.0))
        o['launches'] += 1
        o['total_us'] += r[1] / 1e3
    kernel_us = sum(o['total_us'] for o in out.values())
    for o in out.values():
        o['total_us'] = round(o['total_us'], 2)
        o['per_launch_us'] = round(o['total_us'] / o['launches'], 2)
    if 'masked_gram' in out:
        flop, nbytes = gram_work(n_holed, k, p, e)
        g = out['masked_gram']
        g.update(rows=n_holed, flop=flop, bytes_written=nbytes, TFLOP_per_s=round(flop / g['total_us'] / 1e6, 2),
                 write_GB_per_s=round(nbytes / g['total_us'] / 1e3, 1))
    out['solver_share'] = round(out.get('solver', dict(total_us=0.0))['total_us'] / kernel_us, 3)
    out['kernel_us'] = round(kernel_us, 2)
    out['span_us'] = round((call[-1][2] + call[-1][1] - call[0][2]) / 1e3, 2)
    return out


def run_child(cmd, limit):
    r = subprocess.run(['timeout', '-k', '10', str(limit)] + cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit('bench_inpaint: `%s` ended with status %d; nothing more is started' % (' '.join(cmd), r.returncode))
    return r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--channels', type=int, default=3)
    ap.add_argument('--patch', type=int, default=8)
    ap.add_argument('--components', type=int, default=256)
    ap.add_argument('--alpha', type=float, default=0.1)
    ap.add_argument('--missing', type=float, default=0.5)
    ap.add_argument('--stride', type=int, action='append')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--no-trace', action='store_true')
    ap.add_argument('--timeout', type=int, default=420, help='seconds per GPU child process')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'inpaint_bench.json'))
    ap.add_argument('--child', choices=['wall', 'trace'])
    a = ap.parse_args()
    if a.child:
        return child_wall(a) if a.child == 'wall' else child_trace(a)
    shape = ['--size', a.size, '--channels', a.channels, '--patch', a.patch, '--components', a.components,
             '--alpha', a.alpha, '--missing', a.missing, '--reps', a.reps]
    records = []
    for stride in a.stride or [4, 1]:
        me = [sys.executable, os.path.abspath(__file__)] + [str(v) for v in shape] + ['--stride', str(stride)]
        g = -(-(a.size - a.patch) // stride) + 1
        rec = dict(date=time.strftime('%Y-%m-%d'), command='python scripts/bench_inpaint.py', image=[a.size, a.size, a.channels],
                   dtype='f32', patch=[a.patch, a.patch], k=a.components, missing=a.missing, stride=stride, n_patches=g * g,
                   yardsticks=YARDSTICKS)
        rec.update(json.loads(run_child(me + ['--child', 'wall'], a.timeout).strip().splitlines()[-1]))
        if not a.no_trace:
            tmp = tempfile.mkdtemp(prefix='inpaint_trace_')
            try:
                run_child(['rocprofv3', '--kernel-trace', '--stats', '-d', tmp, '-o', 't', '--'] + me + ['--child', 'trace'],
                          a.timeout)
                dbs = glob.glob(os.path.join(tmp, '**', '*.db'), recursive=True)
                assert dbs, 'rocprofv3 left no database under %s' % tmp
                rec['stages'] = summarise_trace(dbs[0], rec['n_holed'], a.components, a.patch * a.patch * a.channels, 4)
            finally:
                shutil.rmtree(tmp, ignore_errors=True)
        print(json.dumps(rec), flush=True)
        records.append(rec)
    with open(a.out, 'w') as f:
        json.dump(records, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
