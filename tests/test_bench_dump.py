"""bench.py --dump-outputs (no GPU): which arrays are written, from which rows, in which type, and the seeded feature
sample that keeps a wide dictionary within the size budget."""
import os
import types

import numpy as np
from numpy.testing import assert_array_equal

import bench


def _fake_run(k, p, row, seed=0):
    rs = np.random.RandomState(seed)
    est = types.SimpleNamespace(components_=rs.randn(k, p).astype(np.float32), C_=rs.randn(k, k).astype(np.float32),
                                B_=rs.randn(k, p).astype(np.float32),
                                code_=rs.randn(bench.CHUNK, k).astype(np.float32))
    return types.SimpleNamespace(est=est, row=row)


def _load(d):
    return {n: np.load(os.path.join(d, n + '.npy')) for n in ('components', 'C', 'B', 'code')}


def test_dump_outputs_last_minibatch(tmp_path):
    k, p = 8, 300
    row = bench.CHUNK + 3 * bench.BATCH                      # the last minibatch: rows 2b .. 3b of the second chunk
    run = _fake_run(k, p, row)
    bench.dump_outputs(run, str(tmp_path), rank=0)
    got = _load(str(tmp_path))
    for name in got:
        assert got[name].dtype == np.float32, name
    assert_array_equal(got['components'], run.est.components_)
    assert_array_equal(got['C'], run.est.C_)
    assert_array_equal(got['B'], run.est.B_)
    assert_array_equal(got['code'], run.est.code_[2 * bench.BATCH:3 * bench.BATCH])


def test_dump_outputs_other_ranks_write_nothing(tmp_path):
    bench.dump_outputs(_fake_run(4, 50, bench.BATCH), str(tmp_path / 'r1'), rank=1)
    assert not os.path.exists(str(tmp_path / 'r1'))


def test_dump_outputs_wide_sample_within_budget(tmp_path, monkeypatch):
    k, p = 8, 5000
    monkeypatch.setattr(bench, 'DUMP_MAX_BYTES', 4 * (k * k + bench.BATCH * k) + 2 * 4 * k * 700)
    run = _fake_run(k, p, bench.BATCH)
    bench.dump_outputs(run, str(tmp_path / 'a'), rank=0)
    bench.dump_outputs(run, str(tmp_path / 'b'), rank=0)
    a, b = _load(str(tmp_path / 'a')), _load(str(tmp_path / 'b'))
    assert sum(v.nbytes for v in a.values()) <= bench.DUMP_MAX_BYTES
    assert a['components'].shape == a['B'].shape == (k, 700)
    # one sample of feature columns, in increasing order, for both arrays; the same on every run
    cols = [int(np.flatnonzero((run.est.components_ == a['components'][:, j:j + 1]).all(axis=0))[0]) for j in range(700)]
    assert cols == sorted(set(cols))
    assert_array_equal(a['B'], run.est.B_[:, cols])
    for name in a:
        assert_array_equal(a[name], b[name], err_msg=name)
