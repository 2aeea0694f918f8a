"""Benchmark of RecsysDictFact.recommend against what a user could do without it.

    python scripts/bench_recommend.py                      # BASELINE config 4's shape: 69 878 x 10 677, k = 30 and 128, f32
    python scripts/bench_recommend.py --users 4000 --items 3000 --nnz 200000 --components 30 --reps 3

The ratings are scripts/bench_configs.py's ml10m_like (generated from a seed: no input file).  The estimator is not fitted by
minibatches - speed of recommend() does not depend on what the dictionary holds: a random unit-norm dictionary is loaded, the
biases are computed from the ratings (detrend) and every user is coded on their ratings by the kernel _refit uses.

Writes profiles/recommend_bench.json (--out), one JSON line per k:
  recommend_ms         recommend(n_items=10) for ALL users, host call to host arrays (median of --reps after a warm-up call);
  topn_ms              of that, the modl_recsys_topn_* calls alone (device events around _RecsysDevice.topn);
  baseline_ms          the same lists with torch alone, as on the commit before recommend(): per chunk of users
                       torch.matmul(code, D) + col_mean, the chunk's ratings set to -inf through precomputed index tensors,
                       torch.topk; chunks sized so that the scores take the 256 MB recommend() allows its workspace.  The index
                       tensors are built outside the timed region and the lists stay on the device;
  ratio                baseline_ms / topn_ms (device work against device work) and baseline_ms / recommend_ms;
  f32_matrix_share     2 n p k / topn time over the 157.3 TFLOP/s f32 matrix peak: the product's share of the kernel (the rest
                       is selection);
  single_user_ms       recommend(users=[u]) and the baseline for one user (latency).
Every GPU step is a child process under its own `timeout`; the parent never touches the GPU.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
F32_MATRIX_PEAK = 157.3e12
CHUNK_BYTES = 256 << 20


def loaded(a):
    """(estimator ready to recommend, ratings)"""
    import numpy as np
    from bench_configs import ml10m_like
    from modl_amd import recsys
    X = ml10m_like(a.users, a.items, a.nnz, dtype=np.float32)
    est = recsys.RecsysDictFact(n_components=a.components, alpha=1.0, beta=5.0, detrend=True, crop=(0.5, 5.0))
    est.global_mean_ = float(np.mean(X.data))
    est.row_mean_, est.col_mean_ = recsys.compute_biases(X, beta=est.beta)
    Xc = X.copy()
    Xc.data -= np.repeat(est.row_mean_, np.diff(Xc.indptr)).astype(np.float32)
    Xc.data -= est.col_mean_.take(Xc.indices).astype(np.float32)
    D = np.random.RandomState(0).randn(a.components, X.shape[1]).astype(np.float32)
    D /= np.linalg.norm(D, axis=1, keepdims=True)
    est._dev = recsys._RecsysDevice(Xc, a.components, np.float32)
    est._dev.set_dictionary(D)
    est._refit()
    return est, X


def median_ms(f, reps):
    import numpy as np
    import torch
    f()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(ts)), 3), [round(t, 3) for t in ts]


def child(a):
    import numpy as np
    import torch
    est, X = loaded(a)
    dev = est._dev
    n, p, k = dev.n, dev.p, dev.k
    bias = torch.from_numpy(est.col_mean_).to(dev.device)
    rec_ms, rec_all = median_ms(lambda: est.recommend(n_items=10), a.reps)
    topn_ms, _ = median_ms(lambda: dev.topn(dev.code, dev.indptr, dev.indices, None, bias, 10), a.reps)
    # the baseline: torch alone
    D = dev.Dt.t().contiguous()                                            # (k, p)
    bias32 = bias.to(torch.float32)
    rows_all = torch.repeat_interleave(torch.arange(n, device=dev.device), torch.diff(dev.indptr.long()))
    cols_all = dev.indices.long()
    iptr = dev.h_indptr
    chunk = max(CHUNK_BYTES // (4 * p), 1)

    def baseline(users=None):
        out = []
        if users is not None:
            u = int(users[0])
            s = torch.matmul(dev.code[u:u + 1], D) + bias32
            s[0, cols_all[iptr[u]:iptr[u + 1]]] = float('-inf')
            return [torch.topk(s, 10, dim=1)]
        for s0 in range(0, n, chunk):
            e0 = min(s0 + chunk, n)
            s = torch.matmul(dev.code[s0:e0], D) + bias32
            a0, a1 = int(iptr[s0]), int(iptr[e0])
            s[rows_all[a0:a1] - s0, cols_all[a0:a1]] = float('-inf')
            out.append(torch.topk(s, 10, dim=1))
        return out
    base_ms, base_all = median_ms(baseline, a.reps)
    # the two agree (ties apart: torch.topk does not order equal scores by item; compare the score lists)
    items, _ = est.recommend(n_items=10, users=np.arange(min(n, 512)))
    ref = torch.cat([t.values for t in baseline()])[:items.shape[0]].cpu().numpy()
    raw = (dev.code[:items.shape[0]].double() @ D.double() + bias).cpu().numpy()
    got = np.take_along_axis(raw, np.maximum(items, 0), axis=1)
    agree = float(np.max(np.abs(got - ref)[items >= 0]))
    one = [n // 2]
    one_ms, _ = median_ms(lambda: est.recommend(n_items=10, users=one), max(a.reps, 10))
    one_base_ms, _ = median_ms(lambda: baseline(one), max(a.reps, 10))
    print(json.dumps(dict(k=k, users=n, items=p, ratings=int(X.nnz), recommend_ms=rec_ms, recommend_ms_all=rec_all,
                          topn_ms=topn_ms, baseline_ms=base_ms, baseline_ms_all=base_all,
                          ratio_device=round(base_ms / topn_ms, 2), ratio_call=round(base_ms / rec_ms, 2),
                          f32_matrix_share=round(2.0 * n * p * k / (topn_ms * 1e-3) / F32_MATRIX_PEAK, 4),
                          rows_per_call=dev.topn_rows_per_call(n, 10), baseline_rows_per_chunk=chunk,
                          single_user_ms=one_ms, single_user_baseline_ms=one_base_ms,
                          max_score_difference_to_baseline=agree)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--users', type=int, default=69878)
    ap.add_argument('--items', type=int, default=10677)
    ap.add_argument('--nnz', type=int, default=10_000_000)
    ap.add_argument('--components', type=int, action='append')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--timeout', type=int, default=420, help='seconds per GPU child process')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'recommend_bench.json'))
    ap.add_argument('--child', action='store_true')
    a = ap.parse_args()
    if a.child:
        a.components = a.components[0]
        return child(a)
    lines = []
    for k in a.components or [30, 128]:
        cmd = [sys.executable, os.path.abspath(__file__), '--child', '--users', str(a.users), '--items', str(a.items), '--nnz',
               str(a.nnz), '--components', str(k), '--reps', str(a.reps)]
        r = subprocess.run(['timeout', '-k', '10', str(a.timeout)] + cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            raise SystemExit('bench_recommend: k = %d ended with status %d; nothing more is started' % (k, r.returncode))
        rec = dict(date=time.strftime('%Y-%m-%d'), command='python scripts/bench_recommend.py', dtype='f32', n_items=10)
        rec.update(json.loads(r.stdout.strip().splitlines()[-1]))
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
