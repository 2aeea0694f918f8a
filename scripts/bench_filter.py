"""Benchmark of temporal filtering on the device (csrc/filtfilt.hip, modl_amd.signal.butterworth / clean with a filter;
DESIGN.md section 21).

    python scripts/bench_filter.py                   # T = 1200, V = 200 000, f32, high_pass 0.01 Hz, t_r 0.72 s
    python scripts/bench_filter.py --detrend         # adds the sweep of the least-squares line
    python scripts/bench_filter.py --cpu-baseline    # adds the host route: scipy.signal.filtfilt plus the two transfers

On one device-resident record the routes are called in turn (--reps times each after --warmup, every call synchronised),
times as median and [min, max]:
  kernel_ms   modl_filtfilt_* alone: output and workspace allocated once, outside the timing;
  clean_ms    modl_amd.signal.clean(X, detrend, standardize=True, high_pass=..., t_r=...) on the CUDA tensor, end to end:
              coefficients, workspace and temporary allocated, the filter launch, then the projection's launches;
  floor_ms    device-to-device copies of the bytes the kernel moves, measured in the same run: X read once (twice with
              --detrend), the workspace (T + padlen) x V written and read in f64, the result written - as copies, which
              read and write, of half those bytes;
  host_ms     (--cpu-baseline) X.cpu(), scipy.signal.filtfilt in f64 over axis 0, the result back to the device.
floor_frac = floor_ms / kernel_ms, host_ratio = host_ms / kernel_ms.  Prints one JSON line; --out FILE also writes it.
Needs a GPU: there is no fallback."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    ap.add_argument('--dtype', choices=['f32', 'f64'], default='f32')
    ap.add_argument('--high-pass', type=float, default=0.01)
    ap.add_argument('--low-pass', type=float, default=None)
    ap.add_argument('--t-r', type=float, default=0.72)
    ap.add_argument('--order', type=int, default=5)
    ap.add_argument('--detrend', action='store_true')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--cpu-baseline', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import numpy as np
    import scipy.signal
    import torch
    from modl_amd._lib import lib, check, require_gpu
    from modl_amd.device import ptr
    from modl_amd.signal import butterworth_coefficients, clean
    require_gpu()
    T, V = a.time_points, a.voxels
    tdt = torch.float32 if a.dtype == 'f32' else torch.float64
    es = 4 if a.dtype == 'f32' else 8
    gen = torch.Generator(device='cuda').manual_seed(0)
    X = 1e4 + 100 * torch.randn((T, V), generator=gen, device='cuda', dtype=tdt)                 # BOLD-like
    sync = torch.cuda.synchronize
    high = a.high_pass if a.high_pass and a.high_pass > 0 else None
    b, a_, zi = butterworth_coefficients(a.t_r, a.low_pass, high, a.order)
    n_taps = len(b)
    need = lib.modl_filtfilt_workspace(0 if a.dtype == 'f32' else 1, T, V, n_taps)
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    out = torch.empty_like(X)
    fn = getattr(lib, 'modl_filtfilt_' + a.dtype)

    def kernel():
        check(fn(ptr(X), X.stride(0), T, V, b.ctypes.data, a_.ctypes.data, zi.ctypes.data, n_taps, int(a.detrend), None,
                 ptr(out), out.stride(0), ptr(ws), need, None), 'modl_filtfilt')
    t_kernel = timed(kernel, a.warmup, a.reps, sync)
    kw = dict(low_pass=a.low_pass, high_pass=high, t_r=a.t_r, filter_order=a.order)
    t_clean = timed(lambda: clean(X, a.detrend, True, **kw), a.warmup, a.reps, sync)
    # the floor: the kernel's bytes as device copies (a copy of n bytes reads n and writes n)
    moved = T * V * es * (2 if a.detrend else 1) + 2 * need + T * V * es
    src = torch.empty(moved // 2, dtype=torch.uint8, device='cuda')
    dst = torch.empty_like(src)
    t_floor = timed(lambda: dst.copy_(src), a.warmup, a.reps, sync)
    del src, dst
    rec = dict(T=T, V=V, dtype=a.dtype, n_taps=n_taps, low_pass=a.low_pass, high_pass=high, t_r=a.t_r, detrend=a.detrend,
               kernel_ms=t_kernel, clean_ms=t_clean, floor_ms=t_floor, bytes_moved=moved,
               floor_frac=t_floor['median'] / t_kernel['median'], gbs=moved / t_kernel['median'] / 1e6,
               library=os.environ.get('MODL_HIP_LIBRARY', 'product'), reps=a.reps, warmup=a.warmup)
    if a.cpu_baseline:
        def host():
            Xh = X.cpu().numpy().astype(np.float64)
            if a.detrend:
                Xh = scipy.signal.detrend(Xh, axis=0)
            res = scipy.signal.filtfilt(b, a_, Xh, axis=0).astype(Xh.dtype if a.dtype == 'f64' else np.float32)
            return torch.from_numpy(res).to('cuda')
        t0 = time.perf_counter()
        res = host()
        sync()
        rec['host_ms'] = (time.perf_counter() - t0) * 1e3
        kernel()
        rec['max_abs_diff_host'] = float((res - out).abs().max())
        rec['host_ratio'] = rec['host_ms'] / t_kernel['median']
        rec['host_ratio_clean'] = rec['host_ms'] / t_clean['median']
    print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(rec, f, indent=1)


if __name__ == '__main__':
    main()
