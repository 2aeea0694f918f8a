"""Benchmark of RecsysDictFact.ranking_score against what a user could do without it.

    python scripts/bench_ranking.py                        # BASELINE config 4's shape: 69 878 x 10 677, k = 30, f32
    python scripts/bench_ranking.py --users 4000 --items 3000 --nnz 200000 --components 30 --reps 3

The ratings are scripts/bench_configs.py's ml10m_like (generated from a seed: no input file); --held-out (10) ratings of every
user with more than that many are taken out of the training matrix and are the targets.  As in scripts/bench_recommend.py the
estimator is not fitted by minibatches - the speed of the evaluation does not depend on what the dictionary holds.

Writes profiles/ranking_bench.json (--out), one JSON line:
  ranking_score_ms     ranking_score(test, n_items=10) for ALL users, host call to the eight figures (median of --reps after a
                       warm-up call);
  ranks_ms             of that, _RecsysDevice.ranks alone: the modl_recsys_ranks_* calls, the upload of the target pattern and
                       the copy of the ranks to the host;
  recommend_topn_ms    one pass of modl_recsys_topn_* with n_top = 10 over the same users (_RecsysDevice.topn), for scale: the
                       rank call runs its product twice (capture and count);
  baseline_ms          the same ranks with torch alone: per chunk of users torch.matmul(code, D) + col_mean, the chunk's seen
                       items set to -inf through precomputed index tensors, and per target slot one comparison count
                       (score above, or equal with a smaller id) over the chunk's score matrix; chunks sized so that the
                       scores take the 256 MB the rank call allows its workspace.  The index tensors are built outside the timed
                       region and the ranks stay on the device;
  ratio_device         baseline_ms / ranks_ms;  ranks_over_topn: ranks_ms / recommend_topn_ms;
  ranks_differ         entries whose baseline rank (f32 matmul, another summation order) differs from the kernel's.
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
CHUNK_BYTES = 256 << 20


def split(X, held_out, seed):
    """(train, test): `held_out` random ratings of every row with more than that many go to test"""
    import numpy as np
    import scipy.sparse as sp
    lens = np.diff(X.indptr)
    row = np.repeat(np.arange(X.shape[0]), lens)
    order = np.lexsort((np.random.RandomState(seed).random_sample(X.nnz), row))
    place = np.empty(X.nnz, dtype=np.int64)
    place[order] = np.arange(X.nnz) - X.indptr[:-1].astype(np.int64)[row]
    out = (place < held_out) & (lens[row] > held_out)
    part = lambda sel: sp.csr_matrix((X.data[sel], X.indices[sel], np.concatenate([[0], np.cumsum(np.bincount(row[sel], minlength=X.shape[0]))])),
                                     shape=X.shape)
    return part(~out), part(out)


def loaded(a):
    """(estimator ready to rank, held-out ratings)"""
    import numpy as np
    from bench_configs import ml10m_like
    from modl_amd import recsys
    X, test = split(ml10m_like(a.users, a.items, a.nnz, dtype=np.float32), a.held_out, 0)
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
    return est, test


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
    est, test = loaded(a)
    dev = est._dev
    n, p, k = dev.n, dev.p, dev.k
    d = dev.device
    bias = torch.from_numpy(est.col_mean_).to(d)
    score_ms, score_all = median_ms(lambda: est.ranking_score(test, n_items=10), a.reps)
    ranks_ms, _ = median_ms(lambda: dev.ranks(dev.code, dev.indptr, dev.indices, None, bias, test.indptr, test.indices), a.reps)
    topn_ms, _ = median_ms(lambda: dev.topn(dev.code, dev.indptr, dev.indices, None, bias, 10), a.reps)
    # the baseline: torch alone
    D = dev.Dt.t().contiguous()                                            # (k, p)
    bias32 = bias.to(torch.float32)
    rows_all = torch.repeat_interleave(torch.arange(n, device=d), torch.diff(dev.indptr.long()))
    cols_all = dev.indices.long()
    iptr = dev.h_indptr
    m = np.diff(test.indptr)
    slots = int(m.max())
    padded = np.full((n, slots), -1, dtype=np.int64)                       # target j of user u, -1: none
    padded[np.repeat(np.arange(n), m), np.arange(test.nnz) - np.repeat(test.indptr[:-1], m)] = test.indices
    t_cols = torch.from_numpy(padded).to(d)
    ids = torch.arange(p, device=d)[None, :]
    chunk = max(CHUNK_BYTES // (4 * p), 1)

    def baseline():
        out = torch.full((n, slots), -1, dtype=torch.int64, device=d)
        for s0 in range(0, n, chunk):
            e0 = min(s0 + chunk, n)
            s = torch.matmul(dev.code[s0:e0], D) + bias32
            a0, a1 = int(iptr[s0]), int(iptr[e0])
            tc = t_cols[s0:e0]
            own = s.gather(1, tc.clamp(min=0))                             # the targets' scores, before the seen items go
            s[rows_all[a0:a1] - s0, cols_all[a0:a1]] = float('-inf')
            for j in range(slots):
                sj, cj = own[:, j:j + 1], tc[:, j:j + 1]
                cnt = (s > sj).sum(dim=1) + ((s == sj) & (ids < cj)).sum(dim=1)
                out[s0:e0, j] = torch.where(cj[:, 0] >= 0, cnt, out[s0:e0, j])
        return out
    base_ms, base_all = median_ms(baseline, a.reps)
    got, _ = dev.ranks(dev.code, dev.indptr, dev.indices, None, bias, test.indptr, test.indices)
    ref = baseline().cpu().numpy()[padded >= 0]
    res = est.ranking_score(test, n_items=10)
    print(json.dumps(dict(k=k, users=n, items=p, ratings=int(dev.h_indptr[-1]), targets=int(test.nnz), ranking_score_ms=score_ms,
                          ranking_score_ms_all=score_all, ranks_ms=ranks_ms, recommend_topn_ms=topn_ms, baseline_ms=base_ms,
                          baseline_ms_all=base_all, ratio_device=round(base_ms / ranks_ms, 2),
                          ranks_over_topn=round(ranks_ms / topn_ms, 2), rows_per_call=dev.ranks_rows_per_call(n, slots),
                          baseline_rows_per_chunk=chunk, ranks_differ=int(np.sum(got.astype(np.int64) != ref)),
                          score={key: (round(v, 6) if isinstance(v, float) else v) for key, v in res._asdict().items()})),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--users', type=int, default=69878)
    ap.add_argument('--items', type=int, default=10677)
    ap.add_argument('--nnz', type=int, default=10_000_000)
    ap.add_argument('--components', type=int, default=30)
    ap.add_argument('--held-out', type=int, default=10)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--timeout', type=int, default=420, help='seconds for the GPU child process')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ranking_bench.json'))
    ap.add_argument('--child', action='store_true')
    a = ap.parse_args()
    if a.child:
        return child(a)
    cmd = [sys.executable, os.path.abspath(__file__), '--child', '--users', str(a.users), '--items', str(a.items), '--nnz',
           str(a.nnz), '--components', str(a.components), '--held-out', str(a.held_out), '--reps', str(a.reps)]
    r = subprocess.run(['timeout', '-k', '10', str(a.timeout)] + cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit('bench_ranking: the GPU step ended with status %d' % r.returncode)
    rec = dict(date=time.strftime('%Y-%m-%d'), command='python scripts/bench_ranking.py', dtype='f32', n_items=10)
    rec.update(json.loads(r.stdout.strip().splitlines()[-1]))
    print(json.dumps(rec), flush=True)
    with open(a.out, 'w') as f:
        f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
