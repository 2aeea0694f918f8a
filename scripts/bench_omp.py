"""Benchmark of the OMP coder (csrc/omp.hip) on image patches.

    python scripts/bench_omp.py                      # 8 x 8 x 3 patches of a 512 x 512 x 3 image, k = 256, s = 4 and 16, f32
    python scripts/bench_omp.py --size 128 --components 64 --nonzero 4

Writes profiles/omp_bench.json (--out), one record per s:
  omp_ms         Coder.transform(patches, algorithm='omp', n_nonzero_coefs=s), patches and codes device-resident (median
                 of --reps calls after --warmup calls, each call synchronised: the Gram matrix, Dx = X D^T and the kernel);
  enet_ms        the elastic-net coder on the same rows through the same plan (HipBackend.transform, alpha = --alpha); the
                 two coders are called in turn, so that both see the same clocks (30 x (2 .. 9 + 40) ms: over a second);
  cpu_ms         the path a user has without it: the dictionary and --cpu-rows of the rows on the host,
                 sklearn.linear_model.orthogonal_mp_gram on G = D D^T and X D^T (the products included), and
                 cpu_ms_all_rows, that time scaled to every row;
  nnz_per_row    of both coders, and rel_residual, |X - code D| / |X|.
The dictionary is a random unit-norm one: the time of OMP by count does not depend on the data.  The GPU part is a child
process under its own `timeout`; the parent never touches the GPU.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(a):
    import numpy as np
    import torch
    from sklearn.linear_model import orthogonal_mp_gram
    from modl_amd import Coder
    from modl_amd.image import grid_patches
    from bench_reconstruct import synth_image
    img = synth_image(a.size, a.size, a.channels)
    rs = np.random.RandomState(0)
    P = a.patch * a.patch * a.channels
    D = rs.randn(a.components, P).astype(np.float32)
    D /= np.linalg.norm(D, axis=1)[:, None]
    coder = Coder(D, code_alpha=a.alpha)
    be = coder._backend
    patches = grid_patches(img, (a.patch, a.patch), 1, device=be.device)[0]
    kw = coder._plan_kwargs(4096)

    def timed(f, g):
        """f and g in turn, --reps times each after --warmup, every call synchronised; (out_f, ms_f, out_g, ms_g)"""
        for _ in range(a.warmup):
            of, og = f(), g()
        tf, tg = [], []
        for _ in range(a.reps):
            for fn, ts in ((f, tf), (g, tg)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = fn()
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
                if fn is f:
                    of = out
                else:
                    og = out
        return of, tf, og, tg

    def stats(code):
        res = patches - code @ torch.from_numpy(D).to(code.device)
        return (round(float((code != 0).sum(dim=1).double().mean()), 2),
                round(float(torch.linalg.norm(res) / torch.linalg.norm(patches)), 4))

    recs = []
    for s in a.nonzero or [4, 16]:
        code, t_omp, enet, t_enet = timed(lambda: coder.transform(patches, algorithm='omp', n_nonzero_coefs=s),
                                          lambda: be.transform(patches, kw, None, to_host=False))
        rows = patches[:a.cpu_rows]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        Xh = rows.cpu().numpy().astype(np.float64)
        Dh = coder.components_.astype(np.float64)
        ref = orthogonal_mp_gram(Dh @ Dh.T, Dh @ Xh.T, n_nonzero_coefs=s).T
        cpu_ms = (time.perf_counter() - t0) * 1e3
        nnz, rel = stats(code)
        nnz_e, rel_e = stats(enet)
        recs.append(dict(image=[a.size, a.size, a.channels], dtype='f32', patch=[a.patch, a.patch], k=a.components, s=s,
                         n_rows=int(patches.shape[0]), omp_ms=round(float(np.median(t_omp)), 3),
                         omp_ms_min_max=[round(min(t_omp), 3), round(max(t_omp), 3)], enet_ms=round(float(np.median(t_enet)), 3),
                         enet_ms_min_max=[round(min(t_enet), 3), round(max(t_enet), 3)], reps=a.reps, enet_alpha=a.alpha, cpu_rows=int(rows.shape[0]),
                         cpu_ms=round(cpu_ms, 3), cpu_ms_all_rows=round(cpu_ms * patches.shape[0] / rows.shape[0], 1),
                         nnz_per_row=dict(omp=nnz, enet=nnz_e), rel_residual=dict(omp=rel, enet=rel_e),
                         max_abs_diff_vs_sklearn=float(np.max(np.abs(code[:a.cpu_rows].cpu().numpy() - ref)))))
        print(json.dumps(recs[-1]), flush=True)
    print('RESULT ' + json.dumps(recs), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--channels', type=int, default=3)
    ap.add_argument('--patch', type=int, default=8)
    ap.add_argument('--components', type=int, default=256)
    ap.add_argument('--nonzero', type=int, action='append')
    ap.add_argument('--alpha', type=float, default=0.1)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--cpu-rows', type=int, default=4096)
    ap.add_argument('--timeout', type=int, default=420, help='seconds for the GPU child process')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'omp_bench.json'))
    ap.add_argument('--child', action='store_true')
    a = ap.parse_args()
    if a.child:
        return child(a)
    cmd = ['timeout', '-k', '10', str(a.timeout), sys.executable, os.path.abspath(__file__), '--child'] + \
        [v for v in sys.argv[1:] if v != '--child']
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    sys.stdout.write(r.stdout)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        raise SystemExit('bench_omp: the GPU child ended with status %d; nothing more is started' % r.returncode)
    recs = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('RESULT ')][-1][7:])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(recs, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
