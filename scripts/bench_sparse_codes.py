"""Benchmark of the sparse (CSR) codes route (csrc/sparse_codes.hip) against the dense route, on image patches.

    python scripts/bench_sparse_codes.py             # 8 x 8 x 3 patches of a 512 x 512 x 3 image, f32: k = 256 with OMP
                                                     # s = 4 and with the elastic net (alpha 0.1); k = 4096, 65 536 rows, OMP
    rocprofv3 --kernel-trace --stats -d DIR/NAME -- python scripts/bench_sparse_codes.py --child --kernels-only --case NAME
    python scripts/bench_sparse_codes.py --merge-stats DIR      # (no GPU) adds the kernels of that trace to the record

Writes profiles/sparse_codes_bench.json (--out): {"cases": [...], "kernels": [...]}.  Per case, patches device-resident,
the two routes called in turn (--reps times each after --warmup, every call synchronised), times as median and [min, max]:
  dense_ms       Coder.transform(patches, ...) and the (n, k) codes to the host (.cpu());
  sparse_ms      Coder.transform(patches, ..., sparse=True).to_scipy(): a scipy.sparse.csr_matrix on the host;
  inv_dense_ms   inverse_transform of the dense device codes;     inv_csr_ms: of the SparseCodes (both stay on the device);
  peak_dense_mb, peak_sparse_mb   the rise of torch.cuda.max_memory_allocated over one transform call of each route;
  nnz_per_row, dense_mb (the codes as a dense array) and csr_mb (indptr + indices + data).
--kernels-only runs, for every case, --kernel-reps times the compaction of the dense codes (chunks of 4096 rows) and the
decode of their CSR, after one dense coder call; --merge-stats reads the *kernel_stats.csv of such traces (one per case,
NAME as in the record) and records per kernel: calls, total time, the bytes the calls had to move (from the shapes: count
reads the chunk and writes indptr; fill reads the chunk and indptr and writes indices and data; decode reads the CSR and
the atom-major dictionary once and writes the rows), and that rate as a share of the HBM peak (8.0 TB/s) and of the
measured copy rate (6.29 TB/s).
The GPU part is a child process under its own `timeout`; the parent never touches the GPU.
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12          # bytes / s: specification, measured float4 copy


def cases(a):
    return [dict(name='k256_omp4', k=256, rows=None, kw=dict(algorithm='omp', n_nonzero_coefs=4)),
            dict(name='k256_enet', k=256, rows=None, kw=dict()),
            dict(name='k4096_omp4', k=a.wide_components, rows=a.wide_rows, kw=dict(algorithm='omp', n_nonzero_coefs=4))]


def kernel_bytes(n, k, p, nnz, es=4):
    """bytes each kernel has to move for ONE pass over n rows of codes (all chunks together)"""
    return dict(csr_count_kernel=n * k * es + 8 * n, csr_fill_kernel=n * k * es + 8 * n + nnz * (4 + es),
                csr_decode_kernel=8 * (n + 1) + nnz * (4 + es) + k * p * es + n * p * es)


def child(a):
    import numpy as np
    import torch
    from modl_amd import Coder
    from modl_amd.image import grid_patches
    from bench_reconstruct import synth_image
    img = synth_image(a.size, a.size, a.channels)
    rs = np.random.RandomState(0)
    P = a.patch * a.patch * a.channels
    all_patches = grid_patches(img, (a.patch, a.patch), 1, device=torch.device('cuda'))[0]

    def timed(f, g):
        for _ in range(a.warmup):
            f(), g()
        tf, tg = [], []
        for _ in range(a.reps):
            for fn, ts in ((f, tf), (g, tg)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
        return tf, tg

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        return out, round((torch.cuda.max_memory_allocated() - before) / 1e6, 1)

    def ms(ts):
        return round(float(np.median(ts)), 3), [round(min(ts), 3), round(max(ts), 3)]

    recs = []
    for c in cases(a):
        if a.case and c['name'] != a.case:
            continue
        D = rs.randn(c['k'], P).astype(np.float32)
        D /= np.linalg.norm(D, axis=1)[:, None]
        coder = Coder(D, code_alpha=a.alpha)
        be = coder._backend
        patches = all_patches if c['rows'] is None else all_patches[:c['rows']].contiguous()
        n, kw = int(patches.shape[0]), c['kw']
        if a.kernels_only:
            code = torch.as_tensor(coder.transform(patches, **kw)).to(be.device)
            nnz = 0
            for _ in range(a.kernel_reps):
                parts, nnz = [], 0
                for c0 in range(0, n, 4096):
                    parts.append(be.compact(code[c0:c0 + 4096], nnz))
                    nnz += int(parts[-1][1].shape[0])
                indptr = torch.cat([parts[0][0]] + [q[0][1:] for q in parts[1:]])
                be.decode_csr(indptr, torch.cat([q[1] for q in parts]), torch.cat([q[2] for q in parts]), n)
            torch.cuda.synchronize()
            recs.append(dict(name=c['name'], n_rows=n, k=c['k'], p=P, nnz=nnz, kernel_reps=a.kernel_reps))
            continue
        dense, peak_dense = peak(lambda: coder.transform(patches, **kw))
        sparse, peak_sparse = peak(lambda: coder.transform(patches, sparse=True, **kw))
        host = sparse.to_scipy()
        assert host.nnz == int((dense != 0).sum()), 'the two routes disagree'

        def dense_to_host():                  # (the unmasked elastic-net call hands back a host array as it is)
            out = coder.transform(patches, **kw)
            return out.cpu() if isinstance(out, torch.Tensor) else out
        t_dense, t_sparse = timed(dense_to_host, lambda: coder.transform(patches, sparse=True, **kw).to_scipy())
        dense = torch.as_tensor(dense).to(be.device)
        t_inv_dense, t_inv_csr = timed(lambda: coder.inverse_transform(dense), lambda: coder.inverse_transform(sparse))
        rec = dict(name=c['name'], image=[a.size, a.size, a.channels], dtype='f32', n_rows=n, k=c['k'], p=P, coder=kw or
                   dict(algorithm='enet', code_alpha=a.alpha), reps=a.reps, nnz=int(host.nnz),
                   nnz_per_row=round(host.nnz / n, 2), dense_mb=round(n * c['k'] * 4 / 1e6, 1),
                   csr_mb=round((8 * (n + 1) + 8 * host.nnz) / 1e6, 2), peak_dense_mb=peak_dense, peak_sparse_mb=peak_sparse)
        for name, ts in (('dense_ms', t_dense), ('sparse_ms', t_sparse), ('inv_dense_ms', t_inv_dense),
                         ('inv_csr_ms', t_inv_csr)):
            rec[name], rec[name + '_min_max'] = ms(ts)
        recs.append(rec)
        print(json.dumps(rec), flush=True)
        del dense, sparse, host
    print('RESULT ' + json.dumps(recs), flush=True)


def merge_stats(a):
    """the csr_* rows of the rocprofv3 --kernel-trace --stats runs of `--child --kernels-only --case NAME`, one run per
    case under DIR/NAME, into the record"""
    with open(a.out) as f:
        record = json.load(f)
    kernels = []
    for c in record['cases']:
        found = glob.glob(os.path.join(a.merge_stats, c['name'], '**', '*kernel_stats.csv'), recursive=True)
        if len(found) != 1:
            raise SystemExit('bench_sparse_codes: expected one *kernel_stats.csv under %s/%s, found %d'
                             % (a.merge_stats, c['name'], len(found)))
        want = kernel_bytes(c['n_rows'], c['k'], c['p'], c['nnz'])
        with open(found[0]) as f:
            for row in csv.DictReader(f):
                name = [w for w in row['Name'].replace('<', ' ').replace('(', ' ').replace('::', ' ').split() if w.startswith('csr_')]
                if not name or 'predict' in row['Name']:
                    continue
                sec = float(row['TotalDurationNs']) * 1e-9
                rec = dict(case=c['name'], kernel=name[0], calls=int(row['Calls']), total_ms=round(sec * 1e3, 3))
                if name[0] in want:
                    nbytes = want[name[0]] * a.kernel_reps
                    rec.update(bytes_moved=nbytes, tb_per_s=round(nbytes / sec / 1e12, 3),
                               share_of_hbm_peak=round(nbytes / sec / HBM_PEAK, 3),
                               share_of_measured_copy=round(nbytes / sec / HBM_COPY, 3))
                kernels.append(rec)
    record['kernels'] = dict(kernel_reps=a.kernel_reps, what='f32; per case, all calls of the trace together; bytes from '
                             'the shapes', rows=kernels)
    with open(a.out, 'w') as f:
        json.dump(record, f, indent=1)
        f.write('\n')
    print(json.dumps(record['kernels'], indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--channels', type=int, default=3)
    ap.add_argument('--patch', type=int, default=8)
    ap.add_argument('--alpha', type=float, default=0.1)
    ap.add_argument('--wide-components', type=int, default=4096)
    ap.add_argument('--wide-rows', type=int, default=65536)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--kernel-reps', type=int, default=5)
    ap.add_argument('--kernels-only', action='store_true')
    ap.add_argument('--case', default=None, help='only this case (by name)')
    ap.add_argument('--merge-stats', default=None)
    ap.add_argument('--timeout', type=int, default=420, help='seconds for the GPU child process')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sparse_codes_bench.json'))
    ap.add_argument('--child', action='store_true')
    a = ap.parse_args()
    if a.merge_stats:
        return merge_stats(a)
    if a.child:
        return child(a)
    cmd = ['timeout', '-k', '10', str(a.timeout), sys.executable, os.path.abspath(__file__), '--child'] + \
        [v for v in sys.argv[1:] if v != '--child']
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    sys.stdout.write(r.stdout)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        raise SystemExit('bench_sparse_codes: the GPU child ended with status %d; nothing more is started' % r.returncode)
    recs = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('RESULT ')][-1][7:])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(dict(cases=recs), f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
