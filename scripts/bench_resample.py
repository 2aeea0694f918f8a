"""Benchmark of resampling on the device (csrc/resample.hip, modl_amd.masker.resample).

    python scripts/bench_resample.py                 # 91 x 109 x 91 x 300 f32 (1.1 GB, 2 mm) onto 61 x 73 x 61 (3 mm)
    python scripts/bench_resample.py --frames 50 --dtype f64
    python scripts/bench_resample.py --cpu-baseline  # adds the host route: scipy.ndimage.affine_transform per frame

The volume is resident on the device in nibabel's (Fortran) order; the target grid covers the same field of view with
voxels 1.5 times as large (A = 1.5 I, b = 0: every target voxel is inside the source), the mask an ellipsoid filling
about a quarter of the target box.  The routes are called in turn (--reps times each after --warmup, every call
synchronised), times as median and [min, max]:
  box_ms[interp]     modl_resample_* alone, box mode: every voxel of the target box; output and workspace allocated once,
                     outside the timing (the workspace of 'continuous' holds the coefficients of ALL frames here);
  rows_ms[interp]    the same in rows mode: only the V voxels of the mask, as (T, V), the columns walked in the order of
                     the source's memory (d_order, what the Python layer passes); rows_unsorted_ms: without d_order;
  prefilter_ms       modl_spline_prefilter_* alone: the part of 'continuous' that precedes the gather;
  python_ms[interp]  modl_amd.masker.resample(volume, ...) on the CUDA tensor, end to end (output, workspace, and at
                     'continuous' the chunks of frames that keep the workspace within RESAMPLE_WORKSPACE_BYTES);
  grid_sample_ms     torch.nn.functional.grid_sample (trilinear, align_corners) on the same frames as channels of one
                     image: the library's 'linear' composed from a torch operator;
  copy_ms            a device-to-device copy that reads and writes as many bytes as box mode must at the least (the
                     volume in, the target box out), measured in the same run;
  host_ms[interp]    (--cpu-baseline) volume.cpu(), resample_host (scipy), the result back to the device.
Prints one JSON line; --out FILE also writes it.  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench_smooth import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', type=int, nargs=3, default=[91, 109, 91])
    ap.add_argument('--target', type=int, nargs=3, default=[61, 73, 61])
    ap.add_argument('--frames', type=int, default=300)
    ap.add_argument('--dtype', choices=['f32', 'f64'], default='f32')
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--cpu-baseline', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import torch.nn.functional as F
    from modl_amd._lib import lib, check, require_gpu
    from modl_amd.device import ptr
    from modl_amd.masker import _Maps, _ORDERS, resample, resample_host
    require_gpu()
    X, Y, Z = a.shape
    Xt, Yt, Zt = a.target
    T = a.frames
    tdt = torch.float32 if a.dtype == 'f32' else torch.float64
    es = 4 if a.dtype == 'f32' else 8
    dt = 0 if a.dtype == 'f32' else 1
    affine = np.diag([2.0, 2.0, 2.0, 1.0])
    target_affine = np.diag([3.0, 3.0, 3.0, 1.0])
    gx, gy, gz = np.ogrid[:Xt, :Yt, :Zt]
    mask = (((gx - (Xt - 1) / 2) / (0.39 * Xt)) ** 2 + ((gy - (Yt - 1) / 2) / (0.39 * Yt)) ** 2
            + ((gz - (Zt - 1) / 2) / (0.39 * Zt)) ** 2) <= 1.0
    maps = _Maps(mask)
    V = maps.n_voxels
    gen = torch.Generator(device='cuda').manual_seed(0)
    frames = 1e3 + 100 * torch.randn((T, Z, Y, X), generator=gen, device='cuda', dtype=tdt)      # BOLD-like
    volume = frames.permute(3, 2, 1, 0)                                     # (X, Y, Z, T), Fortran order: nibabel's
    sync = torch.cuda.synchronize
    _, d_vox = maps.on(frames.device)
    d_order = maps.order_on(frames.device)
    Ak = np.ascontiguousarray(1.5 * np.eye(3))                              # (symmetric under the reversal of the axes)
    bk = np.zeros(3)
    box, tbox = X * Y * Z, Xt * Yt * Zt
    need = lib.modl_resample_workspace(dt, T, Z, Y, X, 3)
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    out_box = torch.empty((T, Zt, Yt, Xt), dtype=tdt, device='cuda')
    out_rows = torch.empty((T, V), dtype=tdt, device='cuda')
    coef = torch.empty((T, Z, Y, X), dtype=tdt, device='cuda')
    fn = getattr(lib, 'modl_resample_' + a.dtype)

    def call(order, rows, sort=True):
        check(fn(ptr(frames), box, T, Z, Y, X, Ak.ctypes.data, bk.ctypes.data, order, 0.0, Zt, Yt, Xt, ptr(d_vox) if rows else None,
                 V if rows else 0, ptr(d_order) if rows and sort else None, None, ptr(out_rows if rows else out_box), V if rows else tbox, ptr(ws) if order == 3 else None,
                 need if order == 3 else 0, None), 'modl_resample')

    rec = dict(shape=[X, Y, Z], target=[Xt, Yt, Zt], T=T, V=V, mask_fraction=V / tbox, dtype=a.dtype, reps=a.reps, warmup=a.warmup,
               workspace_bytes=need, lds_line=lib.modl_resample_lds_line(), box_ms={}, rows_ms={}, rows_unsorted_ms={}, python_ms={})
    for interp, order in _ORDERS.items():
        rec['box_ms'][interp] = timed(lambda: call(order, False), a.warmup, a.reps, sync)
        rec['rows_ms'][interp] = timed(lambda: call(order, True), a.warmup, a.reps, sync)
        rec['rows_unsorted_ms'][interp] = timed(lambda: call(order, True, False), a.warmup, a.reps, sync)
        rec['python_ms'][interp] = timed(lambda: resample(volume, affine, target_affine, (Xt, Yt, Zt), interp), a.warmup, a.reps,
                                         sync)
    rec['prefilter_ms'] = timed(lambda: check(getattr(lib, 'modl_spline_prefilter_' + a.dtype)(
        ptr(frames), box, T, Z, Y, X, ptr(coef), box, ptr(ws), need, None), 'modl_spline_prefilter'), a.warmup, a.reps, sync)
    del coef
    # torch's trilinear sampling: the frames as channels of one image, normalised coordinates 2 x / (n - 1) - 1, x fastest
    oz, oy, ox = torch.meshgrid(torch.arange(Zt, device='cuda', dtype=tdt), torch.arange(Yt, device='cuda', dtype=tdt),
                                torch.arange(Xt, device='cuda', dtype=tdt), indexing='ij')
    grid = torch.stack([2 * 1.5 * ox / (X - 1) - 1, 2 * 1.5 * oy / (Y - 1) - 1, 2 * 1.5 * oz / (Z - 1) - 1], dim=-1)[None]
    try:
        sample = lambda: F.grid_sample(frames[None], grid, mode='bilinear', padding_mode='zeros', align_corners=True)
        rec['grid_sample_ms'] = timed(sample, a.warmup, a.reps, sync)
        call(1, False)
        rec['max_abs_diff_grid_sample'] = float((sample()[0] - out_box).abs().max())
        rec['grid_sample_ratio'] = rec['grid_sample_ms']['median'] / rec['box_ms']['linear']['median']
    except Exception as e:                                                  # (reported, not hidden: the record says so)
        rec['grid_sample_ms'] = dict(error=repr(e)[:300])
    moved = T * box * es + T * tbox * es
    src = torch.empty(moved // 2, dtype=torch.uint8, device='cuda')
    dst = torch.empty_like(src)
    rec['copy_ms'] = timed(lambda: dst.copy_(src), a.warmup, a.reps, sync)
    rec['bytes_moved'] = moved
    del src, dst
    rec['copies'] = {k: rec['box_ms'][k]['median'] / rec['copy_ms']['median'] for k in rec['box_ms']}
    if a.cpu_baseline:
        host = volume.cpu().numpy()
        rec['host_ms'] = {}
        for interp, order in _ORDERS.items():
            t0 = time.perf_counter()
            res = torch.from_numpy(np.ascontiguousarray(resample_host(host, affine, target_affine, (Xt, Yt, Zt), interp).T)).to('cuda')
            sync()
            rec['host_ms'][interp] = (time.perf_counter() - t0) * 1e3
            call(order, False)
            rec.setdefault('max_abs_diff_host', {})[interp] = float((res - out_box).abs().max())
    print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(rec, f, indent=1)


if __name__ == '__main__':
    main()
