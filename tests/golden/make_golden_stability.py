"""Generate tests/golden/stability.npz from the REAL reference's stability module.

Run in the build container only (needs the reference checkout; numpy and joblib):

    python tests/golden/make_golden_stability.py

It loads modl/decomposition/stability.py of the reference by path ($MODL_REF, default /root/reference/modl) and
records inputs and outputs as data.  Nothing of the reference is written into the repository.  The two upstream
cases (modl/decomposition/tests/test_stability.py: seed 23, 50 x 100, 2 and 20 dictionaries) store the seed only:
the inputs are the first draws of numpy's legacy RandomState(23), which the tests regenerate.  Every scalar's type
under the numpy that ran the reference is recorded as '<key>__type'.
"""
import importlib.util
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get('MODL_REF', '/root/reference/modl')


def load_reference():
    sys.dont_write_bytecode = True
    spec = importlib.util.spec_from_file_location('ref_stability', os.path.join(REF, 'decomposition', 'stability.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def upstream(n_dictionaries):
    rng = np.random.RandomState(23)
    return [rng.randn(50, 100) for _ in range(n_dictionaries)]


def main():
    ref = load_reference()
    out = {}

    def put(key, value):
        out[key] = np.asarray(value)
        out[key + '__type'] = np.asarray(type(value).__name__)

    # upstream test_amari_discrepency: two dictionaries, and one against itself
    D = upstream(2)
    put('up_pair_d', ref.amari_discrepency(D[0], D[1]))
    put('up_self_d', ref.amari_discrepency(D[0], D[0]))
    # upstream test_mean_amari_discrepency: 20 dictionaries
    m, s = ref.mean_amari_discrepency(upstream(20))
    put('up_mean_m', m)
    put('up_mean_s', s)
    rng = np.random.RandomState(0)
    # k1 != k2
    A, B = rng.randn(30, 64), rng.randn(45, 64)
    out['ragged_A'], out['ragged_B'] = A, B
    put('ragged_d', ref.amari_discrepency(A, B))
    put('ragged_d_rev', ref.amari_discrepency(B, A))
    # float32 inputs (the reference's sgemm)
    A, B = rng.randn(40, 80).astype(np.float32), rng.randn(40, 80).astype(np.float32)
    out['f32_A'], out['f32_B'] = A, B
    put('f32_d', ref.amari_discrepency(A, B))
    # a ragged float32 list
    L = [rng.randn(k, 64).astype(np.float32) for k in (20, 33, 47)]
    for i, X in enumerate(L):
        out['f32_list_%d' % i] = X
    m, s = ref.mean_amari_discrepency(L)
    put('f32_list_m', m)
    put('f32_list_s', s)
    # a zero atom: 0 / 0 in a whole row of C -> NaN
    A, B = rng.randn(12, 20), rng.randn(10, 20)
    A[3] = 0
    out['zero_A'], out['zero_B'] = A, B
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        put('zero_d', ref.amari_discrepency(A, B))
    # D against itself (a non-upstream shape)
    A = rng.randn(25, 33)
    out['self_A'] = A
    put('self_d', ref.amari_discrepency(A, A))
    # a list of one dictionary: (nan, nan) with numpy's RuntimeWarning
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        m, s = ref.mean_amari_discrepency([rng.randn(5, 7)])
    put('one_m', m)
    put('one_s', s)
    out['numpy_version'] = np.asarray(np.__version__)
    path = os.path.join(HERE, 'stability.npz')
    np.savez(path, **out)
    print('wrote', path, sorted(k for k in out if not k.endswith('__type')))


if __name__ == '__main__':
    main()
