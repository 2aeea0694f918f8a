"""Benchmark of smoothing and masking on the device (csrc/masker.hip, modl_amd.masker.smooth_mask).

    python scripts/bench_smooth.py                   # 91 x 109 x 91 x 300 f32 (1.1 GB), fwhm 6 mm, voxels 2 mm
    python scripts/bench_smooth.py --frames 50 --fwhm 8 --voxel 2 --dtype f64
    python scripts/bench_smooth.py --cpu-baseline    # adds the host route: scipy.ndimage plus masking plus the transfers

The volume is resident on the device in nibabel's (Fortran) order, the mask an ellipsoid filling about a quarter of the box.
The routes are called in turn (--reps times each after --warmup, every call synchronised), times as median and [min, max]:
  kernel_ms   modl_smooth_mask_* alone: output and workspace allocated once, outside the timing;
  python_ms   modl_amd.masker.smooth_mask(volume, mask, ...) on the CUDA tensor, end to end (weights, output, workspace);
  torch_ms    the same arithmetic composed from torch operators on the device: nan_to_num, then per axis a reflect-pad
              (index_select with the reflected indices) and a 1-D convolution, then index_select of the masked voxels;
  floor_ms    device-to-device copies that read the volume's bytes and write T x V elements, measured in the same run - as
              one copy, which reads and writes, of half those bytes;
  host_ms     (--cpu-baseline) volume.cpu(), smooth_mask_host (scipy.ndimage.gaussian_filter1d per axis, then the mask), the
              result back to the device.
Prints one JSON line; --out FILE also writes it.  Needs a GPU: there is no fallback."""
import argparse
import ctypes
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
    ap.add_argument('--shape', type=int, nargs=3, default=[91, 109, 91])
    ap.add_argument('--frames', type=int, default=300)
    ap.add_argument('--dtype', choices=['f32', 'f64'], default='f32')
    ap.add_argument('--fwhm', type=float, default=6.0)
    ap.add_argument('--voxel', type=float, default=2.0)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--cpu-baseline', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import torch.nn.functional as F
    from modl_amd._lib import lib, check, require_gpu
    from modl_amd.device import ptr
    from modl_amd.masker import _Maps, _weights, smooth_mask, smooth_mask_host
    require_gpu()
    X, Y, Z = a.shape
    T = a.frames
    tdt = torch.float32 if a.dtype == 'f32' else torch.float64
    es = 4 if a.dtype == 'f32' else 8
    voxel = (a.voxel,) * 3
    # an ellipsoid with semi-axes 0.39 of the box: pi / 6 * 0.78^3 = 0.25 of it
    gx, gy, gz = np.ogrid[:X, :Y, :Z]
    mask = (((gx - (X - 1) / 2) / (0.39 * X)) ** 2 + ((gy - (Y - 1) / 2) / (0.39 * Y)) ** 2
            + ((gz - (Z - 1) / 2) / (0.39 * Z)) ** 2) <= 1.0
    maps = _Maps(mask)
    V = maps.n_voxels
    gen = torch.Generator(device='cuda').manual_seed(0)
    frames = 1e3 + 100 * torch.randn((T, Z, Y, X), generator=gen, device='cuda', dtype=tdt)      # BOLD-like
    volume = frames.permute(3, 2, 1, 0)                                     # (X, Y, Z, T), Fortran order: nibabel's
    sync = torch.cuda.synchronize
    (wx, rx), (wy, ry), (wz, rz) = _weights(a.fwhm, voxel)
    d_col, d_vox = maps.on(frames.device)
    need = lib.modl_smooth_mask_workspace(0 if a.dtype == 'f32' else 1, T, Z, Y, X, rz, ry, rx)
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    out = torch.empty((T, V), dtype=tdt, device='cuda')
    fn = getattr(lib, 'modl_smooth_mask_' + a.dtype)
    tile = (ctypes.c_int * 3)()
    check(lib.modl_smooth_tile(0 if a.dtype == 'f32' else 1, rz, ry, rx, tile))

    def kernel():
        check(fn(ptr(frames), Z * Y * X, T, Z, Y, X, wz.ctypes.data if rz else None, rz, wy.ctypes.data if ry else None, ry,
                 wx.ctypes.data if rx else None, rx, ptr(d_col), V, None, ptr(out), V, ptr(ws), need, None), 'modl_smooth_mask')
    t_kernel = timed(kernel, a.warmup, a.reps, sync)
    t_python = timed(lambda: smooth_mask(volume, maps, a.fwhm, voxel), a.warmup, a.reps, sync)

    # the torch composition, on frames (T, 1, Z, Y, X); the kernel's column order: vox are flat (X, Y, Z) indices
    def reflected(n, r):
        i = np.arange(-r, n + r) % (2 * n)
        return torch.from_numpy(np.where(i < n, i, 2 * n - 1 - i)).to('cuda')
    axes = [(2, Z, wz, rz), (3, Y, wy, ry), (4, X, wx, rx)]
    idx = {ax: reflected(n, r) for ax, n, w, r in axes if r}
    kern = {}
    for ax, n, w, r in axes:
        if r:
            shape = [1, 1, 1, 1, 1]
            shape[ax] = 2 * r + 1
            kern[ax] = torch.from_numpy(w).to('cuda', tdt).reshape(shape)
    vz, vy, vx = (d_vox % Z), (d_vox // Z) % Y, d_vox // (Z * Y)
    sel = (vz * Y + vy) * X + vx                                            # the column's voxel in a (Z, Y, X) frame

    def composition():
        v = torch.nan_to_num(frames, nan=0.0, posinf=0.0, neginf=0.0).unsqueeze(1)
        for ax, n, w, r in axes:
            if r:
                v = F.conv3d(v.index_select(ax, idx[ax]), kern[ax])
        return v.reshape(T, -1).index_select(1, sel)
    try:
        t_torch = timed(composition, a.warmup, a.reps, sync)
        kernel()
        diff = float((composition() - out).abs().max())
    except Exception as e:                                                  # (reported, not hidden: the record says so)
        t_torch, diff = dict(error=repr(e)[:300]), None
    moved = T * X * Y * Z * es + T * V * es
    src = torch.empty(moved // 2, dtype=torch.uint8, device='cuda')
    dst = torch.empty_like(src)
    t_floor = timed(lambda: dst.copy_(src), a.warmup, a.reps, sync)
    del src, dst
    rec = dict(shape=[X, Y, Z], T=T, V=V, mask_fraction=V / (X * Y * Z), dtype=a.dtype, fwhm=a.fwhm, voxel=a.voxel,
               radii=[rx, ry, rz], tile=list(tile), kernel_ms=t_kernel, python_ms=t_python, torch_ms=t_torch, floor_ms=t_floor,
               bytes_moved=moved, max_abs_diff_torch=diff, floor_frac=t_floor['median'] / t_kernel['median'],
               reps=a.reps, warmup=a.warmup)
    if 'median' in t_torch:
        rec['torch_ratio'] = t_torch['median'] / t_kernel['median']
    if a.cpu_baseline:
        t0 = time.perf_counter()
        res = torch.from_numpy(smooth_mask_host(volume.cpu().numpy(), maps, a.fwhm, voxel)).to('cuda')
        sync()
        rec['host_ms'] = (time.perf_counter() - t0) * 1e3
        kernel()
        rec['max_abs_diff_host'] = float((res - out).abs().max())
        rec['host_ratio'] = rec['host_ms'] / t_kernel['median']
    print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(rec, f, indent=1)


if __name__ == '__main__':
    main()
