"""Benchmark of the wide-dictionary route (1024 < k <= 4096: csrc/cd_wide.hip, csrc/bcd.hip dict_update_wide).

    python scripts/bench_wide_components.py                     # k = 1024, 1100, 2048, 4096; f32 and f64
    python scripts/bench_wide_components.py --ks 2048 --dtypes f64 --no-oracle

Prints ONE JSON line: for every (k, dtype) the wall time of a minibatch (ms_per_minibatch: mean over --steps timed
minibatches after --warmup, per-minibatch partial_fit calls, each synchronised) and the profiler's five sections
(code_gemm, code_solve, stats_gemm, stats_apply, dict_update: ms per minibatch, HIP events), plus the CPU oracle's time
for one minibatch at k = 2048 (f64).  Shape: p = 10 000 features, b = 256 samples per minibatch, reduction 10, l1 codes
(code_alpha 1), l2 atoms; synthetic rows (a sparse rank-32 signal plus noise).  k = 1024 is the tuned route: it checks
that the existing path did not move.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from modl_amd import DictFact  # noqa: E402

P, B, R = 10000, 256, 10


def rows(n, p, dt, seed=0):
    rs = np.random.RandomState(seed)
    k0 = 32
    X = (rs.randn(n, k0) * (rs.rand(n, k0) < 0.3)).dot(rs.randn(k0, p)) / np.sqrt(0.3 * k0) + 0.1 * rs.randn(n, p)
    return np.ascontiguousarray(X.astype(dt))


def kw(k):
    return dict(n_components=k, batch_size=B, reduction=R, code_alpha=1.0, learning_rate=0.92, random_state=0)


def run_gpu(k, dt, warmup, steps):
    n = max(k, (warmup + steps) * B)
    X = rows(n, P, dt)
    est = DictFact(**kw(k))
    est.prepare(n_samples=n, X=X)
    be = est._backend
    for t in range(warmup):
        est.partial_fit(X[t * B:(t + 1) * B], np.arange(t * B, (t + 1) * B))
    torch.cuda.synchronize()
    be.prof_enable(True)
    be.prof_reset()
    ms = []
    for t in range(warmup, warmup + steps):
        t0 = time.perf_counter()
        est.partial_fit(X[t * B:(t + 1) * B], np.arange(t * B, (t + 1) * B))
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    prof = be.prof_get()
    be.prof_enable(False)
    sec = {name: round(prof[name]['ms'] / steps, 3) if name in prof else 0.0 for name in be.PROF_SECTIONS}
    launches = {name: prof[name]['launches'] // steps for name in be.PROF_SECTIONS if name in prof}
    return dict(k=k, dtype='f32' if dt == np.float32 else 'f64', ms_per_minibatch=round(float(np.mean(ms)), 3),
                ms_min=round(float(np.min(ms)), 3), sections_ms=sec, launches=launches)


def run_oracle(k):
    from oracle import somf_oracle as orc
    orc.lib()
    X = rows(max(k, B), P, np.float64)
    pr = orc.SomfParams(**kw(k))
    st = orc.prepare(pr, n_samples=X.shape[0], X=X)
    t0 = time.perf_counter()
    orc.partial_fit(st, pr, X[:B], np.arange(B))
    return dict(k=k, dtype='f64', oracle_ms_per_minibatch=round(1e3 * (time.perf_counter() - t0), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ks', type=int, nargs='+', default=[1024, 1100, 2048, 4096])
    ap.add_argument('--dtypes', nargs='+', default=['f32', 'f64'])
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--no-oracle', action='store_true')
    a = ap.parse_args()
    out = dict(shape=dict(p=P, b=B, reduction=R), gpu=[], device=torch.cuda.get_device_name(0))
    for k in a.ks:
        for d in a.dtypes:
            out['gpu'].append(run_gpu(k, np.float32 if d == 'f32' else np.float64, a.warmup, a.steps))
            print(json.dumps(out['gpu'][-1]), file=sys.stderr, flush=True)
    if not a.no_oracle:
        out['oracle'] = run_oracle(2048)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
