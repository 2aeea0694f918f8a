"""Benchmark of the k-means assignment, the segmented label sums and kmeans_parcels on the device (csrc/kmeans.hip,
modl_amd.parcellation).

    python scripts/bench_parcellation.py                    # V = 300512, d in {20, 100}, K in {100, 1000}, three restarts
    python scripts/bench_parcellation.py --cpu-baseline     # adds sklearn KMeans and scipy.ndimage.mean on the host
    python scripts/bench_parcellation.py --V 50000 --dims 20 --parcels 100 --rows 200

assign, per (d, K): three routes over the same components X (d, V) and the same R centre sets (K voxels of X each), f64:
  fused    one call of modl_kmeans_assign_f64 for the R sets (outputs and workspace allocated once, outside the timing);
  torch    per set, |C|^2 - 2 C @ X[:, chunk] and min(dim=0), the voxels in chunks so that the K x chunk f64 scores stay below
           --chunk-bytes (1 GiB): the route a user without the kernel would write;
  copy     a plain device copy of the bytes the kernel has to read (X once per set).
label_sums, per K: a (--rows x V) f32 record, labels uniform over the K parcels (`uniform`: the members of a parcel are spread
over the whole row) and in K contiguous runs (`runs`); routes: fused (modl_label_sums_f32 on a prepared order / offsets),
index_add (torch.zeros(T, K).index_add_(1, labels, rows) in the record's dtype) and copy (the record copied once).  The
centroid update (rows = d, f64) is timed the same way under `update`.
The routes alternate, --runs runs of each; a run is --reps samples after --warmup, a sample is --inner calls between two
synchronisations, reported per call as median and [min, max].  `verdict` compares fused with the torch route beyond the spread
of the runs.  `kmeans` times kmeans_parcels end to end (n_init = 3, tol = 1e-4) on Gaussian blobs; --cpu-baseline adds
sklearn.cluster.KMeans(algorithm='lloyd') from the same init, one restart, and scipy.ndimage.mean per row.
Prints one JSON line; --out FILE also writes it.  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench_smooth import timed  # noqa: E402


def blobs(torch, d, V, K, seed):
    gen = torch.Generator(device='cuda').manual_seed(seed)
    centres = 3 * torch.randn((K, d), generator=gen, dtype=torch.float64, device='cuda')
    member = torch.randint(K, (V,), generator=gen, device='cuda')
    return (centres[member] + torch.randn((V, d), generator=gen, dtype=torch.float64, device='cuda')).T.contiguous()


def torch_assign(torch, X, C, chunk, score, labels):
    for r in range(C.shape[0]):
        cn = (C[r] * C[r]).sum(dim=1)
        for a in range(0, X.shape[1], chunk):
            S = cn[:, None] - 2.0 * (C[r] @ X[:, a:a + chunk])
            torch.min(S, dim=0, out=(score[r, a:a + chunk], labels[r, a:a + chunk]))


def compare(runs, a, b):
    fa, fb = [r['median'] for r in runs[a]], [r['median'] for r in runs[b]]
    verdict = '%s faster' % a if max(fa) < min(fb) else ('%s faster' % b if max(fb) < min(fa) else 'within the spread')
    return verdict, min(fb) / max(fa)


def alternate(routes, a, sync):
    runs = {name: [] for name, _ in routes}
    for _ in range(a.runs):
        for name, f in routes:
            t = timed(lambda: [f() for _ in range(a.inner)], a.warmup, a.reps, sync)
            runs[name].append({key: v / a.inner for key, v in t.items()})
    return runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--V', type=int, default=300512)
    ap.add_argument('--dims', default='20,100')
    ap.add_argument('--parcels', default='100,1000')
    ap.add_argument('--restarts', type=int, default=3)
    ap.add_argument('--rows', type=int, default=1200, help='time points of the label_signals record')
    ap.add_argument('--chunk-bytes', type=int, default=1 << 30)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--inner', type=int, default=3)
    ap.add_argument('--runs', type=int, default=2)
    ap.add_argument('--kmeans', default='20,100', help='d,K of the end-to-end run')
    ap.add_argument('--cpu-baseline', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from modl_amd._lib import lib, require_gpu
    from modl_amd.parcellation import kmeans_assign, label_sums, kmeans_parcels, kmeans_init, _segments
    require_gpu()
    sync = torch.cuda.synchronize
    V, R = a.V, a.restarts
    dims, parcels = [int(x) for x in a.dims.split(',')], [int(x) for x in a.parcels.split(',')]
    rec = dict(V=V, restarts=R, reps=a.reps, warmup=a.warmup, inner=a.inner, runs=a.runs, assign=[], update=[], label_sums=[])
    for d in dims:
        for K in parcels:
            X = blobs(torch, d, V, K, d + K)
            gen = torch.Generator(device='cuda').manual_seed(1)
            C = torch.stack([X[:, torch.randperm(V, generator=gen, device='cuda')[:K]].T for _ in range(R)]).contiguous()
            active = torch.arange(R, dtype=torch.int32, device='cuda')
            need = lib.modl_kmeans_assign_workspace(V, d, K, R)
            ws = torch.empty(max(need, 8), dtype=torch.uint8, device='cuda')
            score, labels = torch.zeros((R, V), dtype=torch.float64, device='cuda'), torch.zeros((R, V), dtype=torch.int32, device='cuda')
            t_score, t_labels = torch.zeros_like(score), torch.zeros((R, V), dtype=torch.int64, device='cuda')
            chunk = max(1, min(V, a.chunk_bytes // (8 * K)))
            dst = torch.empty_like(X)
            routes = [('fused', lambda: kmeans_assign(X, C, active, score, labels, ws)),
                      ('torch', lambda: torch_assign(torch, X, C, chunk, t_score, t_labels)),
                      ('copy', lambda: [dst.copy_(X) for _ in range(R)])]
            routes[0][1](), routes[1][1]()
            sync()
            agree = float((labels.long() == t_labels).double().mean())
            diff = float((score - t_score).abs().max())
            runs = alternate(routes, a, sync)
            verdict, speedup = compare(runs, 'fused', 'torch')
            flops = 2.0 * R * K * d * V
            f_med = max(r['median'] for r in runs['fused'])
            rec['assign'].append(dict(d=d, K=K, V=V, R=R, fused_ms=runs['fused'], torch_ms=runs['torch'], copy_ms=runs['copy'],
                                      verdict=verdict, speedup_over_torch=speedup,
                                      fused_over_copy=f_med / min(r['median'] for r in runs['copy']), labels_equal_fraction=agree,
                                      max_abs_score_difference=diff, fused_workspace_bytes=need, torch_chunk_voxels=chunk,
                                      torch_score_bytes=8 * K * chunk, flops=flops, fused_tflops=flops / (f_med * 1e-3) / 1e12,
                                      read_bytes=R * d * V * 8))
            print(json.dumps(rec['assign'][-1]), file=sys.stderr, flush=True)
            # the centroid update of one restart: rows = d, f64
            order, counts, offsets = _segments(labels[0].long(), K)
            sums = torch.zeros((d, K), dtype=torch.float64, device='cuda')
            t_sums = torch.zeros((d, K), dtype=torch.float64, device='cuda')
            lab64 = labels[0].long()
            routes = [('fused', lambda: label_sums(X, order, offsets, sums)),
                      ('sort', lambda: _segments(lab64, K)),
                      ('index_add', lambda: t_sums.zero_().index_add_(1, lab64, X)),
                      ('copy', lambda: dst.copy_(X))]
            runs = alternate(routes, a, sync)
            verdict, speedup = compare(runs, 'fused', 'index_add')
            rec['update'].append(dict(d=d, K=K, V=V, fused_ms=runs['fused'], sort_ms=runs['sort'], index_add_ms=runs['index_add'],
                                      copy_ms=runs['copy'], verdict=verdict, speedup_over_index_add=speedup,
                                      fused_over_copy=max(r['median'] for r in runs['fused']) / min(r['median'] for r in runs['copy']),
                                      max_abs_difference=float((sums - t_sums).abs().max())))
            print(json.dumps(rec['update'][-1]), file=sys.stderr, flush=True)
            del X, C, score, labels, t_score, t_labels, dst, ws
            torch.cuda.empty_cache()
    T = a.rows
    gen = torch.Generator(device='cuda').manual_seed(2)
    rows = torch.randn((T, V), generator=gen, dtype=torch.float32, device='cuda')
    dst = torch.empty_like(rows)
    for K in parcels:
        for layout in ('uniform', 'runs'):
            if layout == 'uniform':
                lab = torch.randint(K, (V,), generator=gen, device='cuda')
            else:
                lab = (torch.arange(V, device='cuda') * K) // V
            order, counts, offsets = _segments(lab, K)
            sums = torch.zeros((T, K), dtype=torch.float64, device='cuda')
            t_sums = torch.zeros((T, K), dtype=torch.float32, device='cuda')
            routes = [('fused', lambda: label_sums(rows, order, offsets, sums)),
                      ('index_add', lambda: t_sums.zero_().index_add_(1, lab, rows)),
                      ('copy', lambda: dst.copy_(rows))]
            runs = alternate(routes, a, sync)
            verdict, speedup = compare(runs, 'fused', 'index_add')
            f_med = max(r['median'] for r in runs['fused'])
            rec['label_sums'].append(dict(T=T, V=V, K=K, layout=layout, dtype='f32', fused_ms=runs['fused'], index_add_ms=runs['index_add'],
                                          copy_ms=runs['copy'], verdict=verdict, speedup_over_index_add=speedup,
                                          fused_over_copy=f_med / min(r['median'] for r in runs['copy']),
                                          fused_read_gbs=T * V * 4 / (f_med * 1e-3) / 1e9,
                                          max_abs_difference=float((sums - t_sums.double()).abs().max())))
            print(json.dumps(rec['label_sums'][-1]), file=sys.stderr, flush=True)
    d, K = (int(x) for x in a.kmeans.split(','))
    X = blobs(torch, d, V, K, 7)
    init = kmeans_init(X, K, R, 0)
    t_init = timed(lambda: kmeans_init(X, K, R, 0), 0, 2, sync)
    kw = dict(init=init, tol=1e-4, max_iter=100)
    res = kmeans_parcels(X, K, **kw)
    rec['kmeans'] = dict(d=d, K=K, V=V, n_init=R, n_iter=res.n_iter.cpu().numpy().tolist(), inertia=res.inertia, init_ms=t_init,
                         ms=timed(lambda: kmeans_parcels(X, K, **kw), 1, 3, sync))
    if a.cpu_baseline:
        import warnings
        import scipy.ndimage
        from sklearn.cluster import KMeans
        Xh, ih = X.cpu().numpy(), init.cpu().numpy()
        t0 = time.perf_counter()
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            sk = KMeans(n_clusters=K, init=ih[res.selected], n_init=1, algorithm='lloyd', tol=1e-4, max_iter=100).fit(Xh.T)
        rec['kmeans'].update(sklearn_one_restart_ms=(time.perf_counter() - t0) * 1e3, sklearn_n_iter=int(sk.n_iter_),
                             sklearn_inertia=float(sk.inertia_),
                             labels_equal_fraction=float(np.mean(sk.labels_ == res.labels.cpu().numpy() - 1)))
        few = rows[:16].cpu().numpy()
        lab_h = (torch.arange(V) * parcels[0] // V).numpy() + 1
        t0 = time.perf_counter()
        for row in few:
            scipy.ndimage.mean(row, lab_h, index=np.arange(1, parcels[0] + 1))
        rec['ndimage_mean_ms_per_row'] = (time.perf_counter() - t0) * 1e3 / len(few)
    print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(rec, f, indent=1)


if __name__ == '__main__':
    main()
