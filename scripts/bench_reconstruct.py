"""Benchmark of ImageDictFact.reconstruct (patch grid -> codes -> decode with unscale -> overlap-add -> finish).

    python scripts/bench_reconstruct.py                      # 512 x 512 x 3 f32, 8 x 8 patches, k = 256, strides 1 and 4
    python scripts/bench_reconstruct.py --size 128 --components 32 --stride 4 --no-trace

Writes profiles/reconstruct_bench.json (--out), one record per stride:
  call_ms        wall time of one reconstruct() call, image in host memory to image in host memory (median of --reps,
                 after a warm-up call);
  host_ms        the host workaround for the same call FROM DEVICE-RESIDENT CODES: codes, means and divisors to the host,
                 numpy decode (code @ D * den + mean) and a Python scatter loop with counts;
  stages         from a `rocprofv3 --kernel-trace --stats` run of its own, the dispatches of ONE call: per stage the
                 launches, the total and the per-launch time, and for the four new stages the bytes they must move
                 (computed from the shapes, below) and the GB/s that implies; `code_solve` is every other kernel of
                 the call (the products, the coordinate descent and what surrounds them in modl_somf_transform).
Every GPU step is a child process under its own `timeout`; the parent never touches the GPU.
Bytes (e = element size, n patches of P = x y C elements, k atoms, image H W C; per pass, summed over the passes):
  grid_patches   reads the image rows of the pass once (they are L2-resident for the x y re-reads), writes n P e + 2 n C e
  decode         reads n k e + P k e + 2 n C e, writes n P e
  overlap_add    reads n P e and the f64 accumulator rows of the pass, writes those rows back
  finish         reads 8 H W C, writes H W C e
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
STAGES = (('grid_patches', 'image_grid_patches_kernel'), ('decode', 'EpiUnscale'),
          ('overlap_add', 'image_overlap_add_kernel'), ('finish', 'image_overlap_finish_kernel'))


def synth_image(h, w, c, seed=0):
    import numpy as np
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.zeros((h, w, c))
    for ch in range(c):
        for _ in range(4):
            fy, fx, ph = rs.uniform(0.05, 0.6), rs.uniform(0.05, 0.6), rs.uniform(0, 6.28)
            img[:, :, ch] += np.sin(fy * yy + fx * xx + ph)
    img += 0.05 * rs.randn(h, w, c)
    return ((img - img.min()) / (img.max() - img.min())).astype(np.float32)


def stage_bytes(H, W, C, x, y, si, sj, k, e, rows_per_pass=None):
    """bytes each new stage must move in one call (docstring above), from the shapes alone"""
    from modl_amd.image import PASS_BYTES
    gi, gj = -(-(H - x) // si) + 1, -(-(W - y) // sj) + 1
    P = x * y * C
    if rows_per_pass is None:
        rows_per_pass = max(1, PASS_BYTES // (gj * P * e))
    out = dict(grid_patches=0, decode=0, overlap_add=0, finish=8 * H * W * C + H * W * C * e)
    for r0 in range(0, gi, rows_per_pass):
        nr = min(rows_per_pass, gi - r0)
        n = nr * gj
        touched = min((r0 + nr - 1) * si, H - x) + x - min(r0 * si, H - x)
        out['grid_patches'] += touched * W * C * e + n * P * e + 2 * n * C * e
        out['decode'] += n * k * e + P * k * e + 2 * n * C * e + n * P * e
        out['overlap_add'] += n * P * e + 16 * touched * W * C
    return out, gi * gj


def fitted(a):
    import contextlib
    import io
    from modl_amd.image import ImageDictFact
    img = synth_image(a.size, a.size, a.channels)
    est = ImageDictFact(patch_size=(a.patch, a.patch), n_components=a.components, batch_size=100, alpha=a.alpha,
                        random_state=0, max_patches=5000, n_epochs=1)
    with contextlib.redirect_stdout(io.StringIO()):
        est.fit(img)
    return est, img


def child_wall(a):
    import numpy as np
    import torch
    from modl_amd import image as mi
    est, img = fitted(a)
    stride = a.stride[0]
    est.reconstruct(img, stride=stride)                                     # warm-up
    ts = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = est.reconstruct(img, stride=stride)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    # the host workaround from device-resident codes
    be = est.dict_fact_._backend
    patches, mean, den = mi.grid_patches(img, (a.patch, a.patch), stride, device=be.device)
    code = be.transform(patches, est.dict_fact_._plan_kwargs(4096), None, to_host=False)
    D = est.dict_fact_.components_
    origins = mi.grid_origins(img.shape, (a.patch, a.patch), stride)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    reps = a.patch * a.patch
    R = code.cpu().numpy() @ D * np.tile(den.cpu().numpy(), reps) + np.tile(mean.cpu().numpy(), reps)
    acc, cnt = np.zeros(img.shape), np.zeros(img.shape)
    for row, (i, j, _) in zip(R, origins):
        acc[i:i + a.patch, j:j + a.patch] += row.reshape(a.patch, a.patch, -1)
        cnt[i:i + a.patch, j:j + a.patch] += 1
    host = (acc / cnt).astype(img.dtype)
    host_ms = (time.perf_counter() - t0) * 1e3
    err = float(np.linalg.norm(out.astype(np.float64) - host) / np.linalg.norm(host))
    print(json.dumps(dict(call_ms=round(float(np.median(ts)), 3), call_ms_all=[round(t, 3) for t in ts],
                          host_ms=round(host_ms, 3), rel_fro_vs_host=err,
                          psnr_db=round(float(-10 * np.log10(np.mean((out - img) ** 2))), 2))), flush=True)


def child_trace(a):
    import torch
    est, img = fitted(a)
    for _ in range(2):                                                      # the trace's last call is the measured one
        est.reconstruct(img, stride=a.stride[0])
    torch.cuda.synchronize()


def summarise_trace(db_path, nbytes):
    rows = sqlite3.connect(db_path).execute('select name, duration, start from kernels order by start').fetchall()
    fin = [i for i, r in enumerate(rows) if STAGES[3][1] in r[0]]
    assert len(fin) >= 2, 'two reconstruct calls expected in the trace'
    call = rows[fin[-2] + 1:fin[-1] + 1]
    call = call[next(i for i, r in enumerate(call) if STAGES[0][1] in r[0]):]    # (the memset / upload kernels before it)
    out = {}
    for r in call:
        stage = next((s for s, pat in STAGES if pat in r[0]), 'code_solve')
        o = out.setdefault(stage, dict(launches=0, total_us=0.0))
        o['launches'] += 1
        o['total_us'] += r[1] / 1e3
    for stage, o in out.items():
        o['total_us'] = round(o['total_us'], 2)
        o['per_launch_us'] = round(o['total_us'] / o['launches'], 2)
        if stage in nbytes:
            o['bytes'] = nbytes[stage]
            o['GB_per_s'] = round(nbytes[stage] / o['total_us'] / 1e3, 1)
    out['span_us'] = round((call[-1][2] + call[-1][1] - call[0][2]) / 1e3, 2)
    return out


def run_child(cmd, limit):
    r = subprocess.run(['timeout', '-k', '10', str(limit)] + cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit('bench_reconstruct: `%s` ended with status %d; nothing more is started' % (' '.join(cmd), r.returncode))
    return r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--channels', type=int, default=3)
    ap.add_argument('--patch', type=int, default=8)
    ap.add_argument('--components', type=int, default=256)
    ap.add_argument('--alpha', type=float, default=0.1)
    ap.add_argument('--stride', type=int, action='append')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--no-trace', action='store_true')
    ap.add_argument('--timeout', type=int, default=420, help='seconds per GPU child process')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'reconstruct_bench.json'))
    ap.add_argument('--child', choices=['wall', 'trace'])
    a = ap.parse_args()
    if a.child:
        return child_wall(a) if a.child == 'wall' else child_trace(a)
    shape = ['--size', a.size, '--channels', a.channels, '--patch', a.patch, '--components', a.components,
             '--alpha', a.alpha, '--reps', a.reps]
    records = []
    for stride in a.stride or [1, 4]:
        me = [sys.executable, os.path.abspath(__file__)] + [str(v) for v in shape] + ['--stride', str(stride)]
        nbytes, n = stage_bytes(a.size, a.size, a.channels, a.patch, a.patch, stride, stride, a.components, 4)
        rec = dict(image=[a.size, a.size, a.channels], dtype='f32', patch=[a.patch, a.patch], k=a.components, stride=stride,
                   n_patches=n)
        rec.update(json.loads(run_child(me + ['--child', 'wall'], a.timeout).strip().splitlines()[-1]))
        if not a.no_trace:
            tmp = tempfile.mkdtemp(prefix='reconstruct_trace_')
            try:
                run_child(['rocprofv3', '--kernel-trace', '--stats', '-d', tmp, '-o', 't', '--'] + me + ['--child', 'trace'],
                          a.timeout)
                dbs = glob.glob(os.path.join(tmp, '**', '*.db'), recursive=True)
                assert dbs, 'rocprofv3 left no database under %s' % tmp
                rec['stages'] = summarise_trace(dbs[0], nbytes)
            finally:
                shutil.rmtree(tmp, ignore_errors=True)
        print(json.dumps(rec), flush=True)
        records.append(rec)
    with open(a.out, 'w') as f:
        json.dump(records, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
