"""The numpy restatement of the K-means passes (oracle/kmeans.py) against sklearn's own answers at
the edges of the kernels' envelope (tests/golden/kmeans_edges.npz, make_golden.py
gen_kmeans_edges).  tests/test_kmeans_kernels_gpu.py then holds the kernels to the restatement."""
import os

import numpy as np
import pytest

import kmeans_inputs as ki
from conftest import GOLDEN


def _skylakex_blas():
    import threadpoolctl
    return any(d.get('internal_api') == 'openblas' and d.get('architecture') == 'SkylakeX'
               and 'numpy' in d.get('filepath', '') for d in threadpoolctl.threadpool_info())


@pytest.fixture(scope='module')
def g():
    return np.load(os.path.join(GOLDEN, 'kmeans_edges.npz'))


def _ids(c):
    return '-'.join(str(v) for v in c)


@pytest.mark.parametrize('case', ki.TIES_CASES, ids=_ids)
def test_estep_restatement_vs_golden(g, case):
    """estep_distances' first minimum equals sklearn's own E-step labels on rows placed at the
    midpoint of two centers (+ 1e-6 noise), where the label is decided by the summation order."""
    from oracle.kmeans import estep_distances
    X, C = ki.ties_case(*case)
    key = 'ties_%d_%d_%d' % case
    assert ki.sha(X, C) == str(g[key + '_sha'])
    np.testing.assert_array_equal(estep_distances(X, C).argmin(1), g[key + '_labels'])


@pytest.mark.parametrize('case', ki.TIES_CASES + [(66, 48, 18)], ids=_ids)
def test_estep_restatement_vs_sklearn(case):
    """The same against sklearn's label pass run here (only where sklearn runs on the OpenBLAS
    SkylakeX kernels whose orders were measured)."""
    if not _skylakex_blas():
        pytest.skip('numpy BLAS is not OpenBLAS SkylakeX: sklearn bits differ from the pinned ones')
    from sklearn.cluster import _kmeans
    from threadpoolctl import threadpool_limits
    from oracle.kmeans import estep_distances
    X, C = ki.ties_case(*case)
    with threadpool_limits(limits=1, user_api='openmp'):
        lb, _ = _kmeans._labels_inertia_threadpool_limit(X, np.ones(len(X), np.float32), C, n_threads=1)
    np.testing.assert_array_equal(estep_distances(X, C).argmin(1), lb)


@pytest.mark.parametrize('case', [c for c in ki.TIES_CASES if c[0] >= 64], ids=_ids)
def test_ties_inputs_have_teeth(g, case):
    """The near-tie inputs tell sklearn's summation order from a plain one: the golden labels
    differ from a sequential-fp32 |c|^2 - 2 x.c argmin on at least 5 % of the rows, so a kernel
    that summed in another order fails the bit-exact label checks.  Measured shares at
    eps = 1e-6: (70, 40, 17) 18.6 %, (263, 776, 33) 47.9 %, (300, 31, 64) 8.7 %,
    (259, 520, 3) 32.4 %, (515, 1000, 5) 30.9 %, (1030, 1029, 7) 42.0 %, (1061, 768, 17) 48.3 %,
    (1061, 100, 17) 21.1 %."""
    from oracle.kmeans import estep_distances
    X, C = ki.ties_case(*case)
    ref = estep_distances(X, C).argmin(1)
    share = float((ref != ki.plain_labels(X, C)).mean())
    print('%s: sklearn order and plain order differ on %.1f %% of the rows' % (case, 100 * share))
    assert share >= 0.05


@pytest.mark.parametrize('D', ki.SHIFT_D)
def test_shift_restatement_vs_golden(g, D):
    """euclidean_dense_dense equals sklearn's _euclidean_dense_dense_wrapper bit for bit (numpy's
    pairwise row sum, which the stand-in used before, does not: last bit at D = 103)."""
    from oracle.kmeans import euclidean_dense_dense
    a, b = ki.shift_case(D)
    assert ki.sha(a, b) == str(g['shift_%d_sha' % D])
    got = euclidean_dense_dense(a, b)
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got, g['shift_%d' % D])


def test_shift_restatement_differs_from_numpy_sum(g):
    """The golden can tell the two orders apart: at D = 103 numpy's pairwise sum misses it."""
    a, b = ki.shift_case(103)
    assert (np.sqrt(((a - b) ** 2).sum(1)) != g['shift_103']).any()


def test_shift_restatement_vs_sklearn():
    from sklearn.cluster._k_means_common import _euclidean_dense_dense_wrapper
    from oracle.kmeans import euclidean_dense_dense
    for D in ki.SHIFT_D + [2, 7, 100]:
        a, b = ki.shift_case(D)
        ref = np.array([_euclidean_dense_dense_wrapper(x, y, False) for x, y in zip(a, b)], np.float32)
        np.testing.assert_array_equal(euclidean_dense_dense(a, b), ref)
        ref2 = np.array([_euclidean_dense_dense_wrapper(x, y, True) for x, y in zip(a, b)], np.float32)
        np.testing.assert_array_equal(euclidean_dense_dense(a, b, squared=True), ref2)


@pytest.mark.parametrize('case', ki.EDGE_CASES, ids=_ids)
def test_cpu_grouper_edge_goldens(g, case):
    """The host control flow on the numpy restatement equals sklearn's KMeans labels for k > 16
    (more k-means++ candidates, further cluster passes), D = 768, D % 16 != 0 and D < 32."""
    from oracle.kmeans import CpuGrouper
    X = ki.edge_case(*case)
    key = 'edge_%d_%d_%d' % case
    assert ki.sha(X) == str(g[key + '_sha'])
    np.testing.assert_array_equal(CpuGrouper().kmeans(X, case[2]), g[key + '_labels'])


@pytest.mark.parametrize('seed', ki.DUP_SEEDS)
def test_cpu_grouper_empty_clusters(g, seed):
    """8 distinct rows, 12 clusters: _relocate_empty and the empty-cluster branch of the
    averaging run (as often as recorded) and the labels equal sklearn's."""
    from oracle.kmeans import CpuGrouper

    class Counting(ki.CountingMixin, CpuGrouper):
        pass
    X = ki.dup_case(seed)
    key = 'dup_%d' % seed
    assert ki.sha(X) == str(g[key + '_sha'])
    cg = Counting()
    np.testing.assert_array_equal(cg.kmeans(X, ki.DUP_K), g[key + '_labels'])
    assert cg.relocations == int(g[key + '_relocations']) > 0
    assert cg.empty_averages == int(g[key + '_empty_averages']) > 0
