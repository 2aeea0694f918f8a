"""Benchmark of the connectivity kernels and of ConnectivityMeasure on the device (csrc/connectivity.hip,
modl_amd.connectivity).

    python scripts/bench_connectivity.py                    # seed maps, covariances at R = 100 and 400, tangent end to end
    python scripts/bench_connectivity.py --cpu-baseline     # adds sklearn's LedoitWolf on the host and the host twin's tangent
    python scripts/bench_connectivity.py --seed 1200,300512,100 --cov 64,1200,100 --tangent 64,1200,100

Seed maps (T, V, R), f32, the record resident on the device, the prepared seeds given:
  fused    one call of modl_conn_seed_maps_f32 (the output allocated once, outside the timing);
  torch    the same arithmetic composed from torch operators, nothing tuned or detuned: the per-voxel mean and sum of squares in
           f64, the record centred and normalised in f32, then matmul;
  copy     a plain copy of the record's bytes (the least any route that reads the record and writes as much could take is half
           of it; the fused route writes only the maps).
Covariances (S, T, R), f64 records resident: one call of modl_conn_covariance_f64 (Ledoit-Wolf) against a loop of torch.cov per
record (empirical: torch has no shrinkage) - and with --cpu-baseline sklearn.covariance.LedoitWolf per record on the host.
Tangent (S, T, R): ConnectivityMeasure(kind='tangent').fit_transform end to end on resident records, against the host twin with
--cpu-baseline.
The routes alternate, --runs runs of each (default 2); a run is --reps samples after --warmup, a sample is --inner calls between
two synchronisations, reported per call as median and [min, max].  `verdict` compares the routes beyond the spread of the runs:
'fused faster' only if the slowest fused median is below the fastest torch median.  Also reported: the largest |difference| of
the routes' outputs, torch.cuda.max_memory_allocated of each route above what is resident, and the arithmetic from the shapes.
Prints one JSON line; --out FILE also writes it.  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench_smooth import timed  # noqa: E402


def torch_seed_maps(torch, X, sh):
    """the composition: f64 statistics, the record centred and normalised in f32, matmul"""
    X64 = X.to(torch.float64)
    mean = X64.mean(dim=0)
    ss = (X64 * X64).sum(dim=0) - X.shape[0] * mean * mean
    Xn = (X - mean.to(X.dtype)) * ss.rsqrt().to(X.dtype)
    return torch.matmul(sh.T, Xn).clamp_(-1.0, 1.0)


def peak_above_resident(torch, f):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = f()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return int(peak)


def verdict_of(fused, other, name):
    f_med, o_med = [r['median'] for r in fused], [r['median'] for r in other]
    if max(f_med) < min(o_med):
        return 'fused faster'
    return ('%s faster' % name) if max(o_med) < min(f_med) else 'within the spread'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seed', default='1200,300512,100', help='T,V,R of the seed maps')
    ap.add_argument('--cov', default='64,1200,100;64,1200,400', help='S,T,R;... of the covariances')
    ap.add_argument('--tangent', default='64,1200,100', help='S,T,R of the end-to-end tangent')
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--inner', type=int, default=5)
    ap.add_argument('--runs', type=int, default=2)
    ap.add_argument('--cpu-baseline', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from modl_amd._lib import lib, check, require_gpu
    from modl_amd.device import ptr, stream_ptr
    from modl_amd import connectivity as K
    require_gpu()
    sync = torch.cuda.synchronize
    rec = dict(reps=a.reps, warmup=a.warmup, inner=a.inner, runs=a.runs)

    def alternate(routes):
        runs = {name: [] for name, _ in routes}
        for _ in range(a.runs):
            for name, f in routes:
                t = timed(lambda: [f() for _ in range(a.inner)], a.warmup, a.reps, sync)
                runs[name].append({key: v / a.inner for key, v in t.items()})
        return runs

    # ---- seed maps
    T, V, R = (int(x) for x in a.seed.split(','))
    gen = torch.Generator(device='cuda').manual_seed(T + V)
    X = torch.randn((T, V), generator=gen, dtype=torch.float32, device='cuda') * 10 + 1000
    seeds = torch.randn((T, R), generator=gen, dtype=torch.float64, device='cuda')
    sh = K._prepare_seeds(seeds).to(torch.float32).contiguous()
    out = torch.empty((R, V), dtype=torch.float32, device='cuda')
    spare = torch.empty_like(X)

    def fused():
        check(lib.modl_conn_seed_maps_f32(ptr(X), X.stride(0), T, V, ptr(sh), R, ptr(out), V, stream_ptr(X.device)), 'modl_conn_seed_maps')
        return out
    diff = float((fused() - torch_seed_maps(torch, X, sh)).abs().max())
    peaks = dict(fused=peak_above_resident(torch, fused), torch=peak_above_resident(torch, lambda: torch_seed_maps(torch, X, sh)))
    runs = alternate([('fused', fused), ('torch', lambda: torch_seed_maps(torch, X, sh)), ('copy', lambda: spare.copy_(X))])
    flops, xbytes = 2.0 * T * V * R, T * V * 4
    slow = max(r['median'] for r in runs['fused']) * 1e-3
    rec['seed_maps'] = dict(T=T, V=V, R=R, dtype='f32', fused_ms=runs['fused'], torch_ms=runs['torch'], copy_ms=runs['copy'],
                            verdict=verdict_of(runs['fused'], runs['torch'], 'torch'),
                            speedup=min(r['median'] for r in runs['torch']) / max(r['median'] for r in runs['fused']),
                            max_abs_difference=diff, peak_bytes_above_resident=peaks, flops=flops, record_bytes=xbytes,
                            fused_tflops=flops / slow / 1e12, fused_record_tb_per_s=xbytes / slow / 1e12)
    print(json.dumps(rec['seed_maps']), file=sys.stderr, flush=True)
    del X, spare, out
    torch.cuda.empty_cache()

    # ---- covariances
    rec['covariances'] = []
    for shape in a.cov.split(';'):
        S, T, R = (int(x) for x in shape.split(','))
        gen = torch.Generator(device='cuda').manual_seed(S + T + R)
        mix = torch.eye(R, dtype=torch.float64, device='cuda') + torch.randn((R, R), generator=gen, dtype=torch.float64, device='cuda') / R ** 0.5
        sig = [torch.randn((T, R), generator=gen, dtype=torch.float64, device='cuda') @ mix for _ in range(S)]
        stacked = torch.cat(sig)
        offsets = np.arange(S + 1, dtype=np.int64) * T
        cov = torch.empty((S, R, R), dtype=torch.float64, device='cuda')
        shr = torch.empty(S, dtype=torch.float64, device='cuda')
        need = lib.modl_conn_covariance_workspace(S, R)
        ws = torch.empty(need, dtype=torch.uint8, device='cuda')

        def one_call(est=1):
            check(lib.modl_conn_covariance_f64(ptr(stacked), R, offsets.ctypes.data, S, R, est, 0, ptr(cov), ptr(shr), ptr(ws), need,
                                               stream_ptr(stacked.device)), 'modl_conn_covariance')
            return cov

        def torch_loop():
            return [torch.cov(x.T, correction=0) for x in sig]
        diff = float((one_call(0) - torch.stack(torch_loop())).abs().max())
        runs = alternate([('fused', one_call), ('torch', torch_loop)])
        entry = dict(S=S, T=T, R=R, dtype='f64', fused_ms=runs['fused'], torch_loop_ms=runs['torch'],
                     verdict=verdict_of(runs['fused'], runs['torch'], 'torch'),
                     speedup=min(r['median'] for r in runs['torch']) / max(r['median'] for r in runs['fused']),
                     max_abs_difference_empirical=diff, workspace_bytes=need, flops=2.0 * S * T * R * R)
        if a.cpu_baseline:
            from sklearn.covariance import LedoitWolf
            host = [x.cpu().numpy() for x in sig]
            t0 = time.perf_counter()
            ref = [LedoitWolf(store_precision=False).fit(x) for x in host]
            entry['ledoit_wolf_host_ms'] = (time.perf_counter() - t0) * 1e3
            got = one_call(1).cpu().numpy()
            entry['max_abs_difference_ledoit_wolf'] = float(max(np.abs(got[s] - ref[s].covariance_).max() for s in range(S)))
        rec['covariances'].append(entry)
        print(json.dumps(entry), file=sys.stderr, flush=True)

    # ---- tangent, end to end
    S, T, R = (int(x) for x in a.tangent.split(','))
    gen = torch.Generator(device='cuda').manual_seed(7)
    mix = torch.eye(R, dtype=torch.float64, device='cuda') + torch.randn((R, R), generator=gen, dtype=torch.float64, device='cuda') / R ** 0.5
    sig = [torch.randn((T, R), generator=gen, dtype=torch.float64, device='cuda') @ mix for _ in range(S)]
    measure = K.ConnectivityMeasure(kind='tangent')
    res = measure.fit_transform(sig)
    rec['tangent'] = dict(S=S, T=T, R=R, ms=timed(lambda: measure.fit_transform(sig), 1, 3, sync))
    if a.cpu_baseline:
        host = [x.cpu().numpy() for x in sig]
        t0 = time.perf_counter()
        ref = K.ConnectivityMeasureHost(kind='tangent').fit_transform(host)
        rec['tangent']['host_ms'] = (time.perf_counter() - t0) * 1e3
        rec['tangent']['max_abs_difference'] = float(np.abs(res.cpu().numpy() - ref).max())
    print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(rec, f, indent=1)


if __name__ == '__main__':
    main()
