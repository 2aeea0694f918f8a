"""Benchmark of region extraction on the device (csrc/regions.hip, modl_amd.regions.connected_regions).

    python scripts/bench_regions.py                     # 91 x 109 x 91, k = 64 positive sparse maps f32, resident on the device
    python scripts/bench_regions.py --maps 256 --dtype f64
    python scripts/bench_regions.py --cpu-baseline      # adds the host route: components.cpu() and the scipy twin

The mask is an ellipsoid of about a third of the box; every map is a sum of --blobs Gaussian blobs (radius 6 .. 12 voxels)
cut off at a tenth of its peak, plus specks at a density of 0.002 that the size filter drops: positive, sparse, a few regions
per map.  Voxels are 2 mm, min_region_size is nilearn's default of 1350 mm^3.  The routes are called in turn (--reps times
each after --warmup, every call synchronised), times as median and [min, max]:
  regions_ms     connected_regions(components, mask) on the CUDA tensor, end to end (the cutoff-free predicate, the workspace,
                 the labelling launches, the count that comes to the host, the gather);
  labels_ms      region_labels(...) alone: the same without the gather;
  gather_ms      modl_region_gather_* alone on the labels of the run before, output allocated outside the timing; gather_gbs
                 is the bytes of `regions` over the median;
  loop_ms        the route that existed before: unmask(components) into k volumes, then per map the predicate into a byte
                 mask and modl_label_components (3 launches each), workspace and output allocated once outside the loop.
                 It stops at the representatives: sizes, filter, numbering and gather would still have to follow;
  host_ms        (--cpu-baseline) components.cpu() and connected_regions_host (one scipy.ndimage.label per map).
Prints one JSON line; --out FILE also writes it.  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench_smooth import timed  # noqa: E402


def phantom_maps(torch, shape, k, blobs, tdt):
    """(mask (X, Y, Z) bool numpy, components (k, V) on the device)"""
    X, Y, Z = shape
    gen = torch.Generator(device='cuda').manual_seed(0)
    x, y, z = torch.meshgrid(torch.arange(X, device='cuda'), torch.arange(Y, device='cuda'), torch.arange(Z, device='cuda'),
                             indexing='ij')
    mask = ((x - X / 2) / (X * 0.43)) ** 2 + ((y - Y / 2) / (Y * 0.43)) ** 2 + ((z - Z / 2) / (Z * 0.43)) ** 2 <= 1.0
    rows = []
    for _ in range(k):
        vol = torch.zeros((X, Y, Z), dtype=torch.float64, device='cuda')
        for _ in range(blobs):
            c = torch.rand(3, generator=gen, device='cuda') * 0.6 + 0.2
            radius = 6.0 + 6.0 * float(torch.rand(1, generator=gen, device='cuda'))
            d2 = (x - c[0] * X) ** 2 + (y - c[1] * Y) ** 2 + (z - c[2] * Z) ** 2
            vol += torch.exp(-d2 / (2 * (radius / 2) ** 2))
        vol = torch.where(vol >= 0.1 * vol.max(), vol, torch.zeros_like(vol))
        specks = torch.rand((X, Y, Z), generator=gen, device='cuda') < 0.002
        vol = torch.where(specks & (vol == 0), torch.full_like(vol, 0.05), vol)
        rows.append(vol[mask].to(tdt))
    return mask.cpu().numpy(), torch.stack(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', type=int, nargs=3, default=[91, 109, 91])
    ap.add_argument('--maps', type=int, default=64)
    ap.add_argument('--blobs', type=int, default=3)
    ap.add_argument('--dtype', choices=['f32', 'f64'], default='f32')
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--cpu-baseline', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from modl_amd._lib import lib, check, require_gpu
    from modl_amd.device import ptr
    from modl_amd import masker as M
    from modl_amd import regions as R
    require_gpu()
    X, Y, Z = a.shape
    k = a.maps
    tdt = torch.float32 if a.dtype == 'f32' else torch.float64
    mask, comp = phantom_maps(torch, (X, Y, Z), k, a.blobs, tdt)
    maps = M._Maps(mask)
    V = maps.n_voxels
    kw = dict(min_region_size=1350, voxel_size=(2, 2, 2))
    sync = torch.cuda.synchronize
    run = lambda f: timed(f, a.warmup, a.reps, sync)
    rec = dict(shape=[X, Y, Z], maps=k, dtype=a.dtype, reps=a.reps, warmup=a.warmup, mask_voxels=V,
               foreground_fraction=float((comp != 0).to(torch.float64).mean()),
               workspace_bytes_per_map=lib.modl_region_labels_workspace(1, Z, Y, X))
    found = R.connected_regions(comp, maps, **kw)
    labels, counts = R.region_labels(comp, maps, **kw)
    n_regions = int(found.regions.shape[0])
    rec['regions'], rec['largest_region'] = n_regions, int(found.sizes.max()) if n_regions else 0
    rec['components_before_filter'] = int(R.region_labels(comp, maps, min_region_size=0)[1].sum())
    rec['regions_ms'] = run(lambda: R.connected_regions(comp, maps, **kw))
    rec['labels_ms'] = run(lambda: R.region_labels(comp, maps, **kw))
    offsets = torch.zeros(k + 1, dtype=torch.int64, device='cuda')
    torch.cumsum(counts, 0, out=offsets[1:])
    out = torch.empty((max(n_regions, 1), V), dtype=tdt, device='cuda')
    gather = getattr(lib, 'modl_region_gather_' + a.dtype)
    rec['gather_ms'] = run(lambda: check(gather(ptr(comp), V, k, V, ptr(labels), V, ptr(offsets), n_regions, ptr(out), V, None),
                                         'modl_region_gather'))
    rec['gather_gbs'] = n_regions * V * comp.element_size() / rec['gather_ms']['median'] / 1e6
    need = lib.modl_label_workspace(Z, Y, X)
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    root = torch.empty((Z, Y, X), dtype=torch.int32, device='cuda')

    def loop():
        vol = M.unmask(comp, maps)                                          # (X, Y, Z, k), a view of k frames
        for m in range(k):
            byte_mask = (vol[..., m] != 0).permute(2, 1, 0).contiguous().to(torch.uint8)
            check(lib.modl_label_components(ptr(byte_mask), Z, Y, X, ptr(root), ptr(ws), need, None), 'modl_label_components')

    rec['loop_ms'] = run(loop)
    if a.cpu_baseline:
        t0 = time.perf_counter()
        h = comp.cpu().numpy()
        t1 = time.perf_counter()
        ref = R.connected_regions_host(h, maps, **kw)
        t2 = time.perf_counter()
        rec['host_ms'] = dict(total=(t2 - t0) * 1e3, download=(t1 - t0) * 1e3, compute=(t2 - t1) * 1e3)
        same = ref.regions.shape == tuple(found.regions.shape)
        rec['elements_that_differ'] = int((found.regions.cpu().numpy() != ref.regions).sum()) if same else -1
        rec['index_and_sizes_equal'] = bool(same and np.array_equal(found.index.cpu().numpy(), ref.index)
                                            and np.array_equal(found.sizes.cpu().numpy(), ref.sizes))
    print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(rec, f, indent=1)


if __name__ == '__main__':
    main()
