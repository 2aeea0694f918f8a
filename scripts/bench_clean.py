"""Benchmark of signal cleaning on the device (csrc/clean.hip, modl_amd.signal.clean).

    python scripts/bench_clean.py                    # T = 1200, V = 200 000, f32, standardize on: q = 2 (constant + ramp)
                                                     # and q = 2 + 24 (24 confounds)
    python scripts/bench_clean.py --cpu-baseline     # adds clean_host (f64 numpy) on the same input: slow at this size

Per case, on the same device-resident record and the same basis, the routes are called in turn (--reps times each after
--warmup, every call synchronised), times as median and [min, max]:
  clean_ms    modl_amd.signal.clean(X, ...) on a CUDA tensor (basis upload, padding launch, kernel; a new output tensor);
  torch_ms    the straightforward composition R = X - Q @ (Q.T @ X); R / R.std(0, unbiased=False) in f32 torch;
  floor_ms    the bytes the kernel moves - three reads of X and one write, 16 B per f32 element - at the HBM peak of
              bench.py's roofline (8.0 TB/s); ideal_ms: one read and one write (8 B per element) at that rate.
and ratio = torch_ms / clean_ms, floor_frac = floor_ms / clean_ms, max_abs_diff between the two routes' results.
Prints one JSON line per case; --out FILE also writes them as a list.  Needs a GPU: there is no fallback.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12                                # bytes / s, bench.py: PEAK_HBM_GBS


def timed(f, warmup, reps, sync):
    for _ in range(warmup):
        f()
    sync()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        sync()
        out.append((time.perf_counter() - t0) * 1e3)
    out.sort()
    return dict(median=out[len(out) // 2], min=out[0], max=out[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--time-points', type=int, default=1200)
    ap.add_argument('--voxels', type=int, default=200000)
    ap.add_argument('--confounds', type=int, nargs='*', default=[0, 24])
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--cpu-baseline', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from modl_amd._lib import require_gpu
    from modl_amd.signal import clean, clean_host, cleaning_basis
    require_gpu()
    T, V = a.time_points, a.voxels
    gen = torch.Generator(device='cuda').manual_seed(0)
    X = 1e4 + 100 * torch.randn((T, V), generator=gen, device='cuda', dtype=torch.float32)     # BOLD-like
    sync = torch.cuda.synchronize
    records = []
    for c in a.confounds:
        conf = np.random.RandomState(c).randn(T, c) if c else None
        Q = cleaning_basis(T, True, True, conf)
        q = Q.shape[1]
        Qd = torch.from_numpy(Q).to('cuda', torch.float32)

        def composed():
            R = X - Qd @ (Qd.T @ X)
            return R / R.std(dim=0, unbiased=False)
        ours, theirs = clean(X, True, True, conf), composed()
        diff = float((ours - theirs).abs().max())
        del ours, theirs
        t_clean = timed(lambda: clean(X, True, True, conf), a.warmup, a.reps, sync)
        t_torch = timed(composed, a.warmup, a.reps, sync)
        floor = 16.0 * T * V / HBM_PEAK * 1e3
        rec = dict(T=T, V=V, dtype='f32', q=q, standardize=True, clean_ms=t_clean, torch_ms=t_torch, floor_ms=floor,
                   ideal_ms=floor / 2, ratio=t_torch['median'] / t_clean['median'], floor_frac=floor / t_clean['median'],
                   max_abs_diff=diff, reps=a.reps, warmup=a.warmup)
        if a.cpu_baseline:
            Xh = X.cpu().numpy()
            t0 = time.perf_counter()
            clean_host(Xh, True, True, conf)
            rec['host_ms'] = (time.perf_counter() - t0) * 1e3
        records.append(rec)
        print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(records, f, indent=1)


if __name__ == '__main__':
    main()
