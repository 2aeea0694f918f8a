"""Benchmark of the FastICA sweep and of fastica_maps on the device (csrc/ica.hip, modl_amd.canica).

    python scripts/bench_canica.py                      # sweeps at (k, V, R) = (20, 200000, 10) and (70, 300512, 10), each fun
    python scripts/bench_canica.py --cpu-baseline       # adds sklearn on the host to the end-to-end timing
    python scripts/bench_canica.py --shapes 70,300512,10 --funs cube

Per shape and non-linearity two routes compute M (R, k, k) and gp (R, k) from the same whitened maps X1 (k, V) and the same
unmixing matrices W (R, k, k), all f64 and resident on the device:
  fused    one call of modl_ica_sweep_f64 (outputs and workspace allocated once, outside the timing);
  torch    the same arithmetic composed from torch f64 operators: Y = W @ X1 (R, k, V), g(Y), g'(Y).mean(-1),
           g(Y) @ X1^T / V - the route a user without the kernel would write.
The routes alternate, --runs runs of each (default 2); a run is --reps samples after --warmup, a sample is --inner sweeps
between two synchronisations, reported per sweep as median and [min, max].  `verdict` compares the routes beyond the spread of
the runs: 'fused faster' only if the slowest fused median is below the fastest torch median.  Also reported: the largest
|difference| of the two routes' outputs, the bytes each route allocates while it runs (fused: its workspace; torch: the peak
of the caching allocator over a sweep), and the arithmetic of the sweep from its shapes (4 R k^2 V flops; X1 read once is
k V 8 bytes).  `fastica` times fastica_maps end to end on planted sparse maps mixed by an orthogonal matrix
(--planted k,V; n_init = 10, cube), `fastica_host_ms` (--cpu-baseline) fastica_maps_host on the same input.
Prints one JSON line; --out FILE also writes it.  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench_smooth import timed  # noqa: E402


def torch_sweep(torch, X1, W, fun, alpha):
    V = X1.shape[1]
    Y = torch.matmul(W, X1)
    if fun == 'cube':
        g, gp = Y ** 3, (3 * Y ** 2).mean(dim=-1)
    elif fun == 'logcosh':
        g = torch.tanh(alpha * Y)
        gp = (alpha * (1 - g ** 2)).mean(dim=-1)
    else:
        e = torch.exp(-(Y ** 2) / 2)
        g, gp = Y * e, ((1 - Y ** 2) * e).mean(dim=-1)
    return torch.matmul(g, X1.T) / V, gp


def planted(np, k, V, seed=0):
    rng = np.random.RandomState(seed)
    maps = rng.laplace(size=(k, V)) * (rng.rand(k, V) < 0.15)
    q, _ = np.linalg.qr(rng.randn(k, k))
    return q @ maps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='20,200000,10;70,300512,10', help='k,V,R;...')
    ap.add_argument('--funs', default='cube,logcosh,exp')
    ap.add_argument('--planted', default='20,200000', help='k,V of the end-to-end run')
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--inner', type=int, default=10)
    ap.add_argument('--runs', type=int, default=2)
    ap.add_argument('--cpu-baseline', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from modl_amd._lib import lib, require_gpu
    from modl_amd.canica import ica_sweep, fastica_maps, fastica_maps_host
    require_gpu()
    sync = torch.cuda.synchronize
    rec = dict(reps=a.reps, warmup=a.warmup, inner=a.inner, runs=a.runs, sweeps=[])
    for shape in a.shapes.split(';'):
        k, V, R = (int(x) for x in shape.split(','))
        gen = torch.Generator(device='cuda').manual_seed(k + V)
        X1 = torch.randn((k, V), generator=gen, dtype=torch.float64, device='cuda')
        W = torch.randn((R, k, k), generator=gen, dtype=torch.float64, device='cuda') / k ** 0.5
        active = torch.arange(R, dtype=torch.int32, device='cuda')
        need = lib.modl_ica_sweep_workspace(V, k, R)
        M, gp = torch.zeros_like(W), torch.zeros((R, k), dtype=torch.float64, device='cuda')
        ws = torch.empty(need, dtype=torch.uint8, device='cuda')
        for fun in a.funs.split(','):
            alpha = 1.0
            fused = lambda: [ica_sweep(X1, W, active, fun, alpha, M, gp, ws) for _ in range(a.inner)]
            composed = lambda: [torch_sweep(torch, X1, W, fun, alpha) for _ in range(a.inner)]
            Mt, gpt = torch_sweep(torch, X1, W, fun, alpha)
            ica_sweep(X1, W, active, fun, alpha, M, gp, ws)
            sync()
            diff = max(float((M - Mt).abs().max()), float((gp - gpt).abs().max()))
            del Mt, gpt
            torch.cuda.empty_cache()
            sync()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            torch_sweep(torch, X1, W, fun, alpha)
            sync()
            torch_bytes = torch.cuda.max_memory_allocated() - base
            runs = dict(fused=[], torch=[])
            for _ in range(a.runs):                                       # the routes alternate
                for name, f in (('fused', fused), ('torch', composed)):
                    t = timed(f, a.warmup, a.reps, sync)
                    runs[name].append({key: v / a.inner for key, v in t.items()})
            f_med, t_med = [r['median'] for r in runs['fused']], [r['median'] for r in runs['torch']]
            verdict = 'fused faster' if max(f_med) < min(t_med) else ('torch faster' if max(t_med) < min(f_med) else 'within the spread')
            flops = 4.0 * R * k * k * V
            rec['sweeps'].append(dict(k=k, V=V, R=R, fun=fun, fused_ms=runs['fused'], torch_ms=runs['torch'], verdict=verdict,
                                      speedup=min(t_med) / max(f_med), max_abs_difference=diff, fused_workspace_bytes=need,
                                      torch_temporary_bytes=int(torch_bytes), flops=flops, x1_bytes=k * V * 8,
                                      fused_tflops=flops / (max(f_med) * 1e-3) / 1e12))
            print(json.dumps(rec['sweeps'][-1]), file=sys.stderr, flush=True)
        del X1, W, M, gp, ws
        torch.cuda.empty_cache()
    k, V = (int(x) for x in a.planted.split(','))
    comp = planted(np, k, V)
    d_comp = torch.from_numpy(comp).cuda()
    kw = dict(n_init=10, fun='cube', random_state=0)
    res = fastica_maps(d_comp, **kw)
    rec['fastica'] = dict(k=k, V=V, n_init=10, fun='cube', n_iter=res.n_iter.cpu().numpy().tolist(), selected=res.selected,
                          ms=timed(lambda: fastica_maps(d_comp, **kw), 1, 3, sync))
    if a.cpu_baseline:
        t0 = time.perf_counter()
        ref = fastica_maps_host(comp, **kw)
        rec['fastica_host_ms'] = (time.perf_counter() - t0) * 1e3
        rec['fastica']['n_iter_host'] = ref.n_iter.tolist()
        rec['fastica']['max_abs_difference_W'] = float(np.max(np.abs(ref.W - res.W.cpu().numpy())))
    print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(rec, f, indent=1)


if __name__ == '__main__':
    main()
