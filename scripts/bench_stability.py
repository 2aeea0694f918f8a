"""Benchmark of modl_amd.mean_amari_discrepency (the Amari discrepancy of every pair of a list of dictionaries).

    python scripts/bench_stability.py                       # every shape below, f32 and f64
    python scripts/bench_stability.py --shape hcp --dtype f32 --reps 3
    python scripts/bench_stability.py --no-numpy            # skip the numpy timings

One JSON line per (shape, dtype):
  call_ms     wall time of one call on device-resident dictionaries (median of --reps; host planning, the small table
              copy, every launch and the copy-back of the pair values included);
  stage_ms    what host (numpy) dictionaries add: the same call on numpy inputs minus call_ms (one copy per dictionary);
  tflops, peak_frac  n (n - 1) / 2 * 2 k^2 p flop per call_ms, against the matrix-core peak: f32 157.3 TF (MI355X
              spec, 155 measured); f64 78.6 TF (AMD's public MI355X spec sheet, not measured on this chip);
  launches    kernels per call;
  numpy_ms    the reference's computation (numpy, f64 or f32 as the input) on numpy_shape; at the HCP-like shape
              numpy runs on ONE pair and numpy_ms_est scales it by the pair count;
  max_err     (f32 only, shapes with p k^2 small enough) the largest deviation of a per-pair row / column maximum
              from a float64 numpy restatement.
Shapes: hcp (n = 10, k = 1 024, p = 200 000), image (n = 10, k = 80, p = 3 072: examples/stability_selection.py),
two_large (n = 2, k = 70, p = 200 000).  The dictionaries are drawn on the device (torch.randn): the benchmark needs
no host copy of 8 GB to start.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from modl_amd.stability import amari_pairs  # noqa: E402

SHAPES = {'hcp': (10, 1024, 200000), 'image': (10, 80, 3072), 'two_large': (2, 70, 200000)}
PEAK = {'f32': 157.3e12, 'f64': 78.6e12}


def ref_numpy(dicts):
    """the reference's loop (stability.py:20-31), joblib aside"""
    ds = []
    for i, D1 in enumerate(dicts[:-1]):
        for D2 in dicts[i + 1:]:
            C = D1.dot(D2.T) / np.sqrt(np.sum(D1 ** 2, axis=1))[:, None] / np.sqrt(np.sum(D2 ** 2, axis=1))[None, :]
            ds.append(.5 * (np.mean(1 - C.max(axis=0)) + np.mean(1 - C.max(axis=1))))
    return np.mean(np.array(ds)), np.std(np.array(ds))


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def run(shape, dt, reps, with_numpy):
    n, k, p = SHAPES[shape]
    npdt = np.float32 if dt == 'f32' else np.float64
    tdt = torch.float32 if dt == 'f32' else torch.float64
    g = torch.Generator(device='cuda').manual_seed(0)
    D = [torch.randn((k, p), generator=g, device='cuda', dtype=tdt) for _ in range(n)]
    r = amari_pairs(D)                                          # warm-up
    call_ms = timed(lambda: amari_pairs(D), reps)
    host = [x.cpu().numpy() for x in D]
    host_ms = timed(lambda: amari_pairs(host), max(1, min(reps, 2)))
    npairs = n * (n - 1) // 2
    flop = npairs * 2.0 * k * k * p
    out = {'shape': shape, 'dtype': dt, 'n': n, 'k': k, 'p': p, 'pairs': npairs, 'launches': r['launches'],
           'call_ms': round(call_ms, 3), 'stage_ms': round(host_ms - call_ms, 3),
           'tflops': round(flop / call_ms / 1e9, 2), 'peak_frac': round(flop / call_ms / 1e9 / (PEAK[dt] / 1e12), 3)}
    if with_numpy:
        sub = host if shape != 'hcp' else host[:2]
        t0 = time.perf_counter()
        ref_numpy(sub)
        nm = (time.perf_counter() - t0) * 1e3
        out['numpy_shape'] = [len(sub), k, p]
        out['numpy_ms'] = round(nm, 1)
        if shape == 'hcp':
            out['numpy_ms_est'] = round(nm * npairs, 1)
    if dt == 'f32' and shape != 'hcp':
        rr = amari_pairs(host, maxima=True)
        err, q = 0.0, 0
        for a in range(n - 1):
            for b in range(a + 1, n):
                A, B = host[a].astype(np.float64), host[b].astype(np.float64)
                C = A.dot(B.T) / np.linalg.norm(A, axis=1)[:, None] / np.linalg.norm(B, axis=1)[None, :]
                err = max(err, float(np.max(np.abs(rr['rowmax'][q] - C.max(axis=1)))),
                          float(np.max(np.abs(rr['colmax'][q] - C.max(axis=0)))))
                q += 1
        out['max_err'] = err
    del D, host
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', choices=sorted(SHAPES), action='append')
    ap.add_argument('--dtype', choices=['f32', 'f64'], action='append')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--no-numpy', action='store_true')
    a = ap.parse_args()
    for shape in a.shape or ['image', 'two_large', 'hcp']:
        for dt in a.dtype or ['f32', 'f64']:
            print(json.dumps(run(shape, dt, a.reps, not a.no_numpy)), flush=True)


if __name__ == '__main__':
    main()
