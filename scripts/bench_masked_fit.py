"""Benchmark of the masked fit: ImageDictFact.fit(image, mask=) on an image with missing elements (masked patches ->
per-row Gram and Dx -> multi-Gram solve -> C_ -> masked statistics B_ -> dictionary update), then inpaint.

    python scripts/bench_masked_fit.py                   # 512 x 512 x 3 f32, 8 x 8 patches, k = 256, b = 100, 50 % missing
    python scripts/bench_masked_fit.py --size 128 --components 32 --windows 2000 --no-trace

Writes profiles/masked_fit_bench.json (--out):
  end_to_end     wall times with the profiler off: fit(image, mask=) on --windows windows (windows/s), inpaint(stride=4)
                 on the dictionary it learned, the PSNR of the filled elements against the clean image;
  minibatch      from a `rocprofv3 --kernel-trace --stats` run of its own: the kernels of the masked minibatches of one
                 partial_fit, per stage (masked Gram, solve, C_, masked statistics, dictionary update, other) the launches
                 and the time per minibatch, and each stage's share;
  masked_stats   of that stage: the FLOP of the p x k x b product and the bytes it must move (X, the mask, the codes,
                 B_ read and written), the TFLOP/s and GB/s these imply - beside the project's own unmasked statistics
                 product at the same (b, k, p) in the same trace (a DictFact.partial_fit at reduction = 1).
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
STAGES = (('patches_masked', ('image_patches_masked_kernel',)), ('masked_gram', ('masked_gram_kernel',)),
          ('masked_stats', ('masked_stats_kernel', 'masked_counts_kernel')), ('C', ('EpiAxpbyC',)),
          ('dict_update', ('bcd', 'atom_', 'dict_')),
          ('solve', ('cd_', 'chol', 'ridge', 'masked_row_norm2', 'masked_codes_finish', 'fill_kernel')))
REFERENCE_ROWS = dict(psnr_db_dictionary_from_clean_image=28.6, unmasked_config2_patches_per_s=92000)


def damaged(a):
    import numpy as np
    from bench_reconstruct import synth_image
    clean = synth_image(a.size, a.size, a.channels).astype(np.float32)
    img = clean.copy()
    img[np.random.RandomState(1).rand(*img.shape) < a.missing] = -1
    return clean, img


def estimator(a):
    from modl_amd.image import ImageDictFact
    return ImageDictFact(patch_size=(a.patch, a.patch), n_components=a.components, batch_size=a.batch, alpha=a.alpha,
                         random_state=0, max_patches=a.windows, n_epochs=1)


def child_wall(a):
    import numpy as np
    import torch
    clean, img = damaged(a)
    if a.size > 64:                                                         # warm-up (library, allocator)
        estimator(a).fit(img[:64, :64], mask=img[:64, :64] != -1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    est = estimator(a).fit(img, mask=img != -1)
    torch.cuda.synchronize()
    fit_s = time.perf_counter() - t0
    est.inpaint(img, stride=4)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = est.inpaint(img, stride=4)
    torch.cuda.synchronize()
    inpaint_s = time.perf_counter() - t0
    miss = img == -1
    n = int(est.dict_fact_.n_iter_)
    print(json.dumps(dict(windows=n, fit_s=round(fit_s, 3), windows_per_s=round(n / fit_s, 1),
                          fit_device_s=round(float(est.dict_fact_.time_), 3), inpaint_stride4_ms=round(inpaint_s * 1e3, 2),
                          psnr_db_on_missing=round(float(-10 * np.log10(np.mean((out[miss] - clean[miss]) ** 2))), 2))),
          flush=True)


def child_trace(a):
    """one buffer of masked minibatches, then the same rows without a mask at reduction = 1 (the yardstick's product)"""
    import numpy as np
    import torch
    from modl_amd import DictFact
    from modl_amd.image import _patches_masked, _stage_image, masked_candidates
    _, img = damaged(a)
    obs = img != -1
    origins = masked_candidates(obs, (a.patch, a.patch), 0.25)
    origins = origins[np.random.RandomState(0).permutation(len(origins))[:a.batch * a.trace_minibatches]]
    d_img, d_obs = _stage_image(img), torch.from_numpy(obs.view(np.uint8)).cuda()
    rows, _, _, orows, _ = _patches_masked(d_img, d_obs, origins, (a.patch, a.patch, a.channels), True, True)
    kw = dict(n_components=a.components, batch_size=a.batch, code_alpha=a.alpha, learning_rate=0.92, random_state=0)
    for masked in (True, False, True):                                     # the trace's last masked call is the measured one
        est = DictFact(reduction=1, **kw)
        est.prepare(n_samples=rows.shape[0], X=rows)
        est.partial_fit(rows, mask=orows if masked else None)
        torch.cuda.synchronize()


def summarise_trace(db_path, a):
    rows = sqlite3.connect(db_path).execute('select name, duration, start from kernels order by start').fetchall()
    gram = [i for i, r in enumerate(rows) if 'masked_gram_kernel' in r[0]]
    n_mb = a.trace_minibatches
    assert len(gram) >= 2 * n_mb, 'two masked calls expected in the trace'
    first = gram[-n_mb]
    while first > 0 and 'masked_row_norm2' in rows[first - 1][0]:
        first -= 1
    last = max(i for i, r in enumerate(rows) if i > gram[-1] and any(p in r[0] for p in STAGES[4][1]))
    call = rows[first:last + 1]
    out = {}
    for r in call:
        stage = next((s for s, pats in STAGES if any(p in r[0] for p in pats)), 'other')
        o = out.setdefault(stage, dict(launches=0, total_us=0.0))
        o['launches'] += 1
        o['total_us'] += r[1] / 1e3
    kernel_us = sum(o['total_us'] for o in out.values())
    for o in out.values():
        o['share'] = round(o['total_us'] / kernel_us, 3)
        o['per_minibatch_us'] = round(o['total_us'] / n_mb, 2)
        o['total_us'] = round(o['total_us'], 2)
    p, k, b, e = a.patch * a.patch * a.channels, a.components, a.batch, 4
    flop = 2.0 * p * k * b
    nbytes = b * p * (e + 1) + b * k * e + 2 * p * k * e
    ms = [r[1] / 1e3 for r in call if 'masked_stats_kernel' in r[0]]
    stats = dict(shape=dict(p=p, k=k, b=b), flop=flop, bytes=nbytes, product_launch_us=round(sum(ms) / len(ms), 2),
                 TFLOP_per_s=round(flop / (sum(ms) / len(ms)) / 1e6, 3), GB_per_s=round(nbytes / (sum(ms) / len(ms)) / 1e3, 1))
    # the yardstick: the launch of the unmasked step (between the two masked calls) that carries the p x k x b product
    mid = rows[gram[-2 * n_mb]:gram[-n_mb]]
    unm = [r for r in mid if 'stats' in r[0].lower() and 'masked_' not in r[0]]
    if unm:
        names = sorted(set(r[0][:120] for r in unm))
        us = sum(r[1] for r in unm) / 1e3 / n_mb
        stats['unmasked_yardstick'] = dict(kernels=names, per_minibatch_us=round(us, 2),
                                           note='carries C_ (k x k x b) and B_ (p x k x b) of the unmasked step',
                                           TFLOP_per_s=round((flop + 2.0 * k * k * b) / us / 1e6, 3))
    return dict(minibatches=n_mb, stages=out, kernel_us_per_minibatch=round(kernel_us / n_mb, 2),
                span_us_per_minibatch=round((call[-1][2] + call[-1][1] - call[0][2]) / 1e3 / n_mb, 2)), stats


def run_child(cmd, limit):
    r = subprocess.run(['timeout', '-k', '10', str(limit)] + cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit('bench_masked_fit: `%s` ended with status %d; nothing more is started' % (' '.join(cmd), r.returncode))
    return r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--channels', type=int, default=3)
    ap.add_argument('--patch', type=int, default=8)
    ap.add_argument('--components', type=int, default=256)
    ap.add_argument('--batch', type=int, default=100)
    ap.add_argument('--alpha', type=float, default=0.1)
    ap.add_argument('--missing', type=float, default=0.5)
    ap.add_argument('--windows', type=int, default=20000)
    ap.add_argument('--trace-minibatches', type=int, default=10)
    ap.add_argument('--no-trace', action='store_true')
    ap.add_argument('--timeout', type=int, default=420, help='seconds per GPU child process')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'masked_fit_bench.json'))
    ap.add_argument('--child', choices=['wall', 'trace'])
    a = ap.parse_args()
    if a.child:
        return child_wall(a) if a.child == 'wall' else child_trace(a)
    me = [sys.executable, os.path.abspath(__file__)] + [str(v) for v in (
        '--size', a.size, '--channels', a.channels, '--patch', a.patch, '--components', a.components, '--batch', a.batch,
        '--alpha', a.alpha, '--missing', a.missing, '--windows', a.windows, '--trace-minibatches', a.trace_minibatches)]
    rec = dict(date=time.strftime('%Y-%m-%d'), command='python scripts/bench_masked_fit.py', image=[a.size, a.size, a.channels],
               dtype='f32', patch=[a.patch, a.patch], k=a.components, batch=a.batch, missing=a.missing,
               reference_rows=REFERENCE_ROWS)
    rec['end_to_end'] = json.loads(run_child(me + ['--child', 'wall'], a.timeout).strip().splitlines()[-1])
    if not a.no_trace:
        tmp = tempfile.mkdtemp(prefix='masked_fit_trace_')
        try:
            run_child(['rocprofv3', '--kernel-trace', '--stats', '-d', tmp, '-o', 't', '--'] + me + ['--child', 'trace'],
                      a.timeout)
            dbs = glob.glob(os.path.join(tmp, '**', '*.db'), recursive=True)
            assert dbs, 'rocprofv3 left no database under %s' % tmp
            rec['minibatch'], rec['masked_stats'] = summarise_trace(dbs[0], a)
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(rec), flush=True)
    with open(a.out, 'w') as f:
        json.dump(rec, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
