"""Benchmark of computing a mask on the device (csrc/compute_mask.hip, modl_amd.masker.compute_*_mask).

    python scripts/bench_mask.py                     # 91 x 109 x 91 x 300 f32 (1.1 GB), resident on the device
    python scripts/bench_mask.py --frames 50 --dtype f64
    python scripts/bench_mask.py --cpu-baseline      # adds the host route: volume.cpu() and the scipy twins, on 20 frames

The volume is the 'head' phantom of tests/test_compute_mask.py scaled up, in nibabel's (Fortran) order: integer noise
1 .. 39, an ellipsoid head of about a fifth of the box, a cube joined to it by a bridge one voxel thick, two specks.  The
routes are called in turn (--reps times each after --warmup, every call synchronised), times as median and [min, max]:
  epi_ms, background_ms   compute_epi_mask(volume) and compute_background_mask(volume, connected=True, opening=2) on the
                          CUDA tensor, end to end (allocations, the values that come to the host, the result);
  mean_ms                 modl_frame_mean_* alone, output allocated outside the timing; next to it torch_mean_ms
                          (frames.mean(0, dtype=float64)) and read_ms, a read-only pass over the same bytes
                          (frames.amax()): the distance to what HBM allows; *_gbs are the volume's bytes over the medians;
  sort_threshold_ms       the sort of the mean, the first argmax of the differences, the two values to the host, the compare;
  erosion2_ms, dilation4_ms, erosion2_final_ms, largest_ms    the stages of the post-processing, each on the mask that
                          reaches it in compute_epi_mask, through the Python helpers (workspace allocated per call);
  host_ms                 (--cpu-baseline) volume.cpu() and the *_host twins on the first --host-frames frames.
Prints one JSON line; --out FILE also writes it.  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench_smooth import timed  # noqa: E402


def phantom_frames(torch, shape, T, tdt):
    """(T, Z, Y, X) on the device: the 'head' phantom at this shape, integer-valued"""
    X, Y, Z = shape
    gen = torch.Generator(device='cuda').manual_seed(0)
    frames = torch.randint(1, 40, (T, Z, Y, X), generator=gen, device='cuda').to(tdt)
    z, y, x = torch.meshgrid(torch.arange(Z, device='cuda'), torch.arange(Y, device='cuda'), torch.arange(X, device='cuda'),
                             indexing='ij')
    c = (X * 0.34, Y * 0.5 - 0.5, Z * 0.5 - 0.5)
    body = ((x - c[0]) / (X * 0.29)) ** 2 + ((y - c[1]) / (Y * 0.42)) ** 2 + ((z - c[2]) / (Z * 0.42)) ** 2 <= 1.0
    cy, cz = int(c[1]), int(c[2])
    x_end = int(body[cz, cy].nonzero().max())
    w = max(7, X // 8)
    body[cz - w // 2:cz + w // 2 + 1, cy - w // 2:cy + w // 2 + 1, x_end + 3:x_end + 3 + w] = True
    body[cz, cy, x_end + 1:x_end + 3] = True
    body[Z - 3:Z - 1, 1:3, X - 3:X - 1] = True
    body[1:3, Y - 3:Y - 1, X - 3:X - 1] = True
    frames += 400 * body.to(tdt)
    return frames, float(body.to(torch.float64).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', type=int, nargs=3, default=[91, 109, 91])
    ap.add_argument('--frames', type=int, default=300)
    ap.add_argument('--dtype', choices=['f32', 'f64'], default='f32')
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--cpu-baseline', action='store_true')
    ap.add_argument('--host-frames', type=int, default=20)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from modl_amd._lib import lib, check, require_gpu
    from modl_amd.device import ptr
    from modl_amd import masker as M
    require_gpu()
    X, Y, Z = a.shape
    T = a.frames
    tdt = torch.float32 if a.dtype == 'f32' else torch.float64
    es = 4 if a.dtype == 'f32' else 8
    frames, fraction = phantom_frames(torch, (X, Y, Z), T, tdt)
    volume = frames.permute(3, 2, 1, 0)                                     # (X, Y, Z, T), Fortran order: nibabel's
    sync = torch.cuda.synchronize
    box = X * Y * Z
    rec = dict(shape=[X, Y, Z], T=T, dtype=a.dtype, reps=a.reps, warmup=a.warmup, body_fraction=fraction,
               volume_bytes=T * box * es, label_tile=list(_tile(lib)), label_workspace_bytes=lib.modl_label_workspace(Z, Y, X))
    run = lambda f: timed(f, a.warmup, a.reps, sync)
    rec['epi_ms'] = run(lambda: M.compute_epi_mask(volume))
    rec['background_ms'] = run(lambda: M.compute_background_mask(volume, connected=True, opening=2))
    mean = torch.empty((Z, Y, X), dtype=tdt, device='cuda')
    fn = getattr(lib, 'modl_frame_mean_' + a.dtype)
    rec['mean_ms'] = run(lambda: check(fn(ptr(frames), box, T, box, 1, ptr(mean), None), 'modl_frame_mean'))
    rec['torch_mean_ms'] = run(lambda: frames.mean(0, dtype=torch.float64))
    rec['read_ms'] = run(lambda: frames.amax())
    for k in ('mean', 'torch_mean', 'read'):
        rec[k + '_gbs'] = T * box * es / rec[k + '_ms']['median'] / 1e6
    rec['max_abs_diff_torch_mean'] = float((frames.mean(0, dtype=torch.float64) - mean.to(torch.float64)).abs().max())

    state = {}

    def sort_threshold():
        s = torch.sort(mean.reshape(-1)).values
        lo, hi = M._cut_indices(0.2, 0.85, int(s.shape[0]))
        delta = s[lo + 1:hi + 1] - s[lo:hi]
        ia = int((delta == delta.max()).nonzero()[0, 0])
        pair = s[ia + lo:ia + lo + 2].cpu().numpy()
        state['threshold'] = float(pair.dtype.type(0.5) * (pair[0] + pair[1]))
        state['raw'] = (mean >= state['threshold']).to(torch.uint8)

    rec['sort_threshold_ms'] = run(sort_threshold)
    rec['threshold'] = state['threshold']
    raw = state['raw']
    eroded = M._morph_device(raw, 2, False)
    largest, info = M._largest_device(eroded)
    grown = M._morph_device(largest, 4, True)
    rec['components_after_erosion'], rec['largest_size'] = info[0], info[1]
    rec['components_before_erosion'] = M._largest_device(raw)[1][0]
    rec['erosion2_ms'] = run(lambda: M._morph_device(raw, 2, False))
    rec['largest_ms'] = run(lambda: M._largest_device(eroded))
    rec['largest_raw_ms'] = run(lambda: M._largest_device(raw))             # the thresholded mask: noise-free, with the bridge
    rec['dilation4_ms'] = run(lambda: M._morph_device(largest, 4, True))
    rec['erosion2_final_ms'] = run(lambda: M._morph_device(grown, 2, False))
    rec['mask_voxels'] = int(M.compute_epi_mask(volume).sum())
    if a.cpu_baseline:
        n = min(a.host_frames, T)
        part = frames[:n].permute(3, 2, 1, 0)
        rec['host_frames'] = n
        rec['host_ms'] = {}
        for name, host, dev in (('epi', lambda v: M.compute_epi_mask_host(v), lambda v: M.compute_epi_mask(v)),
                                ('background', lambda v: M.compute_background_mask_host(v, connected=True, opening=2),
                                 lambda v: M.compute_background_mask(v, connected=True, opening=2))):
            t0 = time.perf_counter()
            h = part.cpu().numpy()
            t1 = time.perf_counter()
            res = host(h)
            t2 = time.perf_counter()
            rec['host_ms'][name] = dict(total=(t2 - t0) * 1e3, download=(t1 - t0) * 1e3, compute=(t2 - t1) * 1e3)
            rec['host_ms'][name]['device_ms'] = run(lambda: dev(part))
            rec['host_ms'][name]['voxels_that_differ'] = int((dev(part).cpu().numpy() != res).sum())
    print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(rec, f, indent=1)


def _tile(lib):
    import ctypes as C
    tile = (C.c_int * 3)()
    lib.modl_label_tile(tile)
    return tuple(tile)


if __name__ == '__main__':
    main()
