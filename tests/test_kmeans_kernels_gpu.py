"""Every K-means / cluster-score entry point of csrc/kmeans.hip on its own, at the edges of what
include/vtf.h accepts: k up to 64 (every pass of k_estep's 16-cluster loop), k-means++ with 5, 6
and 16 candidate rows (k_sqdist_rows<16>), D = 768, D % 16 != 0, D < 32, the split-remainder K
blocks, empty clusters, row shards that start off a 64-row tile, the 160-cluster / 32-set limits
and the refusals.  Expected values: the numpy restatements of oracle/kmeans.py (pinned to sklearn
on the CPU by tests/test_kmeans_oracle.py), plain numpy where numpy is what sklearn calls, float64
/ long double references with a worked-out bound where the order of the sums is free, and
sklearn's own answers from tests/golden/kmeans_edges.npz."""
import ctypes
import os

import numpy as np
import pytest
import torch

import kmeans_inputs as ki
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

E_ARG, E_LIMIT = -1, -5   # include/vtf.h


@pytest.fixture(scope='module')
def g():
    return np.load(os.path.join(GOLDEN, 'kmeans_edges.npz'))


@pytest.fixture(scope='module')
def gr():
    from videotofaces.kmeans import Grouper
    gr = Grouper('cuda:0')
    gr._bind()
    return gr


def L():
    from videotofaces import _native as nat
    return nat.lib()


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def poison(shape, dtype=torch.float32):
    return torch.full(shape, -77, dtype=dtype, device='cuda')


def _ids(c):
    return '-'.join(str(v) for v in c)


# ------------------------------------------------------------------ handle
def test_group_handle_create_stream_destroy():
    """vtf_group_create / set_stream / destroy called directly: a second handle on the current
    stream computes the same column statistics, and null arguments are refused."""
    h = ctypes.c_void_p()
    assert L().vtf_group_create(0, ctypes.byref(h)) == 0 and h.value
    assert L().vtf_group_set_stream(h, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    X = np.arange(12, dtype=np.float32).reshape(4, 3) ** 2
    mean, var = poison((3,)), poison((3,))
    assert L().vtf_colstats(h, ptr(dev(X)), 4, 3, None, ptr(mean), ptr(var)) == 0
    np.testing.assert_array_equal(mean.cpu().numpy(), X.mean(0))
    np.testing.assert_array_equal(var.cpu().numpy(), np.var(X, 0))
    assert L().vtf_group_destroy(h) == 0
    assert L().vtf_group_create(0, None) == E_ARG
    assert L().vtf_group_set_stream(None, None) == E_ARG


# ------------------------------------------------------------------ vtf_kmeans_step
def step(gr, Xd, Cd, k, labels, with_sums):
    """vtf_kmeans_step on poisoned outputs -> (labels, sums, weights, changed) on the host"""
    N, D = Xd.shape
    ld = dev(labels.astype(np.int32))
    sums = poison((k, D)) if with_sums else None
    w = poison((k,)) if with_sums else None
    changed = ctypes.c_int64(-1)
    rc = L().vtf_kmeans_step(gr._h, ptr(Xd), N, D, ptr(Cd), k, ptr(ld), ptr(sums), ptr(w), ctypes.byref(changed))
    assert rc == 0
    return (ld.cpu().numpy(), sums.cpu().numpy() if with_sums else None, w.cpu().numpy() if with_sums else None,
            changed.value)


def step_reference(X, C):
    from oracle.kmeans import estep_distances
    k = C.shape[0]
    ref = estep_distances(X, C).argmin(1).astype(np.int32)
    sums = np.zeros((k, X.shape[1]), np.float32)
    np.add.at(sums, ref, X)   # unbuffered, rows in order: sequential fp32 per cluster
    return ref, sums, np.bincount(ref, minlength=k).astype(np.float32)


def check_step(gr, X, C, ref, sums, w):
    N, k = X.shape[0], C.shape[0]
    Xd, Cd = dev(X), dev(C)
    flipped = ref.copy()
    at = np.unique(np.linspace(0, N - 1, min(N, 5)).astype(int))
    flipped[at] = (ref[at] + 1) % k if k > 1 else -1
    for start, n_changed in ((np.full(N, -1), N), (flipped, len(at))):
        for with_sums in (False, True):
            lb, s, ww, changed = step(gr, Xd, Cd, k, start, with_sums)
            np.testing.assert_array_equal(lb, ref)
            assert changed == n_changed == int((ref != start).sum())
            if with_sums:
                np.testing.assert_array_equal(s, sums)
                np.testing.assert_array_equal(ww, w)


@pytest.mark.parametrize('case', ki.TIES_CASES, ids=_ids)
def test_kmeans_step_near_ties(gr, g, case):
    """Labels bit exact against estep_distances' first minimum (and sklearn's own labels in the
    golden) on rows whose label hangs on the summation order; sums against np.add.at, weights
    against np.bincount, changed against (new != old).sum(); with and without d_sums, from labels
    -1 and from the reference labels with up to five flipped.
      (1, 32, 1)        smallest call
      (7, 40, 3)        N < 16
      (70, 40, 17)      second cluster pass; small sgemm whose edge block has m % 4 and k % 4 != 0
      (263, 776, 33)    a full chunk on the blocked kernel, a 7-row chunk on the small one; third pass
      (300, 31, 64)     D < 32 (blocked kernel at any size); the k = 64 limit
      (259, 520, 3)     small kernel on a full 256-row chunk; split-remainder K blocks
      (515, 1000, 5)    K blocks 448 + two halves
      (1030, 1029, 7)   D % 16 != 0; three K blocks
      (1061, 768, 17), (1061, 100, 17)   ViT-B's width; D = 100"""
    X, C = ki.ties_case(*case)
    ref, sums, w = step_reference(X, C)
    np.testing.assert_array_equal(ref, g['ties_%d_%d_%d' % case + '_labels'])
    check_step(gr, X, C, ref, sums, w)


def test_kmeans_step_empty_cluster(gr):
    """A center far from every row: its sums row is zeros and its weight 0."""
    X, C4 = ki.ties(300, 40, 4, 1e-6, seed=3)
    C = np.insert(C4, 2, np.float32(100), axis=0)
    ref, sums, w = step_reference(X, C)
    assert w[2] == 0 and not sums[2].any() and (w[[0, 1, 3, 4]] > 0).all()
    check_step(gr, X, C, ref, sums, w)


# ------------------------------------------------------------------ vtf_kmeans_average
def _weights(k, rng):
    """Counts with a zero before the arg-max cluster, one after it, and a tie in the maximum"""
    w = rng.integers(1, 9, k).astype(np.float32)
    if k >= 12:
        w[[1, k - 2]] = 0
        w[[k // 2, k // 2 + 3]] = 11
    return w


@pytest.mark.parametrize('D', [1, 3, 5, 103, 768, 1029])
def test_kmeans_average(gr, D):
    """Centers bit exact against the sequential reference (c *= float32(1 / float64(w)) cluster by
    cluster; an empty cluster copies the arg-max cluster's row as it stands at that moment: not yet
    scaled for the empty cluster before it, scaled for the one after), shift bit exact against the
    restated _euclidean_dense_dense.  k = 1, 12, 64."""
    from oracle.kmeans import CpuGrouper, euclidean_dense_dense
    for k in (1, 12, 64):
        rng = np.random.default_rng(100 * D + k)
        w = _weights(k, rng)
        sums = (rng.normal(0, 1, (k, D)) * np.maximum(w, 1)[:, None]).astype(np.float32)
        old = rng.normal(0, 1, (k, D)).astype(np.float32)
        ref = sums.copy()
        ref_shift = CpuGrouper()._average(ref, w, old)
        if k >= 12:
            assert int(np.argmax(w)) == k // 2
            np.testing.assert_array_equal(ref[1], sums[k // 2])   # copied before the scaling
            np.testing.assert_array_equal(ref[k - 2], ref[k // 2])  # copied after it
        np.testing.assert_array_equal(ref_shift, euclidean_dense_dense(ref, old))
        sd, shift = dev(sums), poison((k,))
        assert L().vtf_kmeans_average(gr._h, ptr(sd), ptr(dev(w)), ptr(dev(old)), k, D, ptr(shift)) == 0
        np.testing.assert_array_equal(sd.cpu().numpy(), ref, err_msg='k=%d' % k)
        np.testing.assert_array_equal(shift.cpu().numpy(), ref_shift, err_msg='k=%d' % k)


@pytest.mark.parametrize('D', ki.SHIFT_D)
def test_kmeans_average_shift_vs_sklearn_golden(gr, g, D):
    """The shift alone against sklearn's _euclidean_dense_dense_wrapper values (weights 1, so the
    averaging leaves the rows as they are)."""
    a, b = ki.shift_case(D)
    ad, shift = dev(a), poison((16,))
    assert L().vtf_kmeans_average(gr._h, ptr(ad), ptr(dev(np.ones(16, np.float32))), ptr(dev(b)), 16, D,
                                  ptr(shift)) == 0
    np.testing.assert_array_equal(ad.cpu().numpy(), a)
    np.testing.assert_array_equal(shift.cpu().numpy(), g['shift_%d' % D])


# ------------------------------------------------------------------ vtf_center_dist
@pytest.mark.parametrize('D', [1, 7, 8, 9, 100, 128, 129, 136, 264, 768, 1029])
def test_center_dist(gr, D):
    """((X - C[labels])**2).sum(axis=1) in float32, bit exact: numpy's pairwise row sum
    (sequential below 8, eight accumulators up to 128, halves at a multiple of 8 above)."""
    for N in (1, 257):
        rng = np.random.default_rng(D + N)
        X = rng.normal(0, 1, (N, D)).astype(np.float32)
        C = rng.normal(0, 1, (3, D)).astype(np.float32)
        lb = rng.integers(0, 3, N).astype(np.int32)
        ref = ((X - C[lb]) ** 2).sum(axis=1)
        assert ref.dtype == np.float32
        np.testing.assert_array_equal(gr._center_dist(dev(X), dev(C), dev(lb)), ref, err_msg='N=%d' % N)


# ------------------------------------------------------------------ vtf_colstats
@pytest.mark.parametrize('N,D', [(1, 1), (3, 65), (257, 100), (130, 768)])
def test_colstats(gr, N, D):
    """X.mean(0), np.var(X, 0) and X - mean, bit exact, with and without the centred copy."""
    X = (np.random.default_rng(N + D).normal(0.3, 1, (N, D))).astype(np.float32)
    mean = X.mean(0)
    for with_xc in (False, True):
        Xc = poison((N, D)) if with_xc else None
        m, v = poison((D,)), poison((D,))
        assert L().vtf_colstats(gr._h, ptr(dev(X)), N, D, ptr(Xc), ptr(m), ptr(v)) == 0
        np.testing.assert_array_equal(m.cpu().numpy(), mean)
        np.testing.assert_array_equal(v.cpu().numpy(), np.var(X, 0))
        if with_xc:
            np.testing.assert_array_equal(Xc.cpu().numpy(), X - mean)


# ------------------------------------------------------------------ vtf_sqdist_rows / pairwise
def sqdist_reference(X, ids):
    """squared distances of X[ids] to every row in long double, rounded to fp32 and clipped at 0,
    and the double-rounding bound (D + 2) 2^-52 (|x|^2 + |y|^2) of a float64 evaluation of
    -2 x.y + |x|^2 + |y|^2 in any order; the tolerance is one fp32 ulp of the reference plus it"""
    Xl = X.astype(np.longdouble)
    n2 = (Xl * Xl).sum(1)
    d = n2[ids, None] + n2[None, :] - 2 * (Xl[ids] @ Xl.T)
    ref = np.maximum(d, 0).astype(np.float32)
    return ref, (X.shape[1] + 2) * 2.0 ** -52 * (n2[ids, None] + n2[None, :]).astype(np.float64)


@pytest.mark.parametrize('T,D', [(T, D) for D in (31, 100, 768) for T in (1, 4, 5, 6, 16)] + [(16, 1024)])
def test_sqdist_rows(gr, T, D):
    """k_sqdist_rows<4> (T <= 4) and <16> (k-means++ asks for 5 rows from k = 21, 6 from k = 55; 16
    rows of 1024 floats fill the 64 KiB of LDS exactly) against the long double reference; repeated
    row indices; the self distance is >= 0."""
    N = 70
    X = np.random.default_rng(T * D).normal(0.2, 1, (N, D)).astype(np.float32)
    ids = np.array(([0, N - 1, 33, 33, 5, 64, 0, 69] * 2)[:T], np.int64)
    ref, bound = sqdist_reference(X, ids)
    tol = np.spacing(ref) + bound
    out = poison((T, N))
    assert L().vtf_sqdist_rows(gr._h, ptr(dev(X)), N, D, ids.ctypes.data, T, ptr(out)) == 0
    got = out.cpu().numpy()
    err = np.abs(got.astype(np.float64) - ref)
    assert (err <= tol).all(), 'worst error / bound %.3g' % (err / tol).max()
    assert (got >= 0).all() and (got[np.arange(T), ids] <= tol[np.arange(T), ids]).all()
    np.testing.assert_array_equal(gr._sqdist_rows(dev(X), ids), got)   # the wrapper: the same call


def pairwise(gr, X):
    N, D = X.shape
    out = poison((N, N))
    assert L().vtf_pairwise_euclidean(gr._h, ptr(dev(X)), N, D, ptr(out)) == 0
    return out


@pytest.mark.parametrize('D', [24, 100])
@pytest.mark.parametrize('N', [1, 63, 65, 130])
def test_pairwise_euclidean(gr, N, D):
    """The N x N matrix (one tile, a tile plus one row, three tiles) against the same long double
    reference after the square root, with the same bound; the diagonal is exactly 0."""
    X = np.random.default_rng(N + D).normal(0.2, 1, (N, D)).astype(np.float32)
    ref2, bound = sqdist_reference(X, np.arange(N))
    ref = np.sqrt(ref2)
    np.fill_diagonal(ref, 0)
    got = pairwise(gr, X).cpu().numpy()
    assert not np.diagonal(got).any()
    err = np.abs(got.astype(np.float64) - ref)
    assert (err <= np.spacing(ref) + bound).all()


# ------------------------------------------------------------------ silhouette
def singleton_labels(N, k, seed):
    """k clusters, all present, the last one holding only row N // 2"""
    rng = np.random.default_rng(seed)
    lb = rng.integers(0, k - 1, N)
    others = rng.permutation(N)
    lb[others[others != N // 2][:k - 1]] = np.arange(k - 1)
    lb[N // 2] = k - 1
    return lb.astype(np.int32)


def samples(gr, Dm, lb, k):
    """vtf_silhouette_samples on a resident distance matrix"""
    N = Dm.shape[0]
    sil = poison((N,))
    freq = np.bincount(lb, minlength=k).astype(np.int64)
    assert L().vtf_silhouette_samples(gr._h, ptr(Dm), N, ptr(dev(lb.astype(np.int32))), k, ptr(dev(freq)),
                                      ptr(sil)) == 0
    return sil.cpu().numpy()


@pytest.fixture(scope='module')
def score130(gr):
    X, sets = ki.score_case(130, 100)
    return X, sets, pairwise(gr, X)


@pytest.mark.parametrize('k', [2, 8, 9, 16, 17, 33, 64])
def test_silhouette_samples_every_kmax(gr, score130, k):
    """k_silhouette<8 | 16 | 32 | 64> on the N x N matrix of N = 130 rows, one cluster a singleton
    (its silhouette is 0): within 2e-7 of the restatement, and the one-pass sweep agrees with the
    N x N path within the same bound."""
    from oracle.kmeans import silhouette_samples
    X, _, Dm = score130
    lb = singleton_labels(130, k, seed=k)
    assert np.bincount(lb).min() >= 1 and np.bincount(lb)[k - 1] == 1 and len(np.unique(lb)) == k
    got = samples(gr, Dm, lb, k)
    assert got[65] == 0
    np.testing.assert_allclose(got, silhouette_samples(X, lb), rtol=0, atol=2e-7)
    np.testing.assert_allclose(gr.silhouette_sweep(X, [lb])[0], got, rtol=0, atol=2e-7)


def test_silhouette_samples_vs_sklearn_golden(gr, g, score130):
    X, sets, Dm = score130
    assert ki.sha(X, *[sets[n] for n in sorted(sets)]) == str(g['score_130_100_sha'])
    for name, lb in sets.items():
        got = samples(gr, Dm, lb, int(lb.max()) + 1)
        np.testing.assert_allclose(got, g['score_130_100_%s_sil' % name], rtol=0, atol=2e-7, err_msg=name)
    assert samples(gr, Dm, sets['single'], 5)[65] == 0


@pytest.mark.parametrize('N,D', ki.SCORE_CASES)
def test_silhouette_sweep_vs_sklearn_golden(gr, g, N, D):
    """The one-pass sweep (N < 64, three tiles, five tiles; D % 16 != 0) against sklearn's
    silhouette_samples within 2e-7: every label set alone (M = 1), the sets of 2, 16 and 40
    clusters in one call (N = 37 has no 40-cluster set: the singleton set takes its place), and
    all of them in one call."""
    X, sets = ki.score_case(N, D)
    key = 'score_%d_%d' % (N, D)
    assert ki.sha(X, *[sets[n] for n in sorted(sets)]) == str(g[key + '_sha'])
    names = list(sets)
    three = ['k2', 'k16', 'k40' if 'k40' in sets else 'single']
    for group in [[n] for n in names] + [three, names]:
        got = gr.silhouette_sweep(X, [sets[n] for n in group])
        for n, s in zip(group, got):
            np.testing.assert_allclose(s, g['%s_%s_sil' % (key, n)], rtol=0, atol=2e-7, err_msg='%s in %s' % (n, group))
    assert gr.silhouette_sweep(X, [sets['single']])[0][N // 2] == 0


def sweep_raw(gr, Xd, lab, ks, freq, lo, hi, sil):
    N, D = Xd.shape
    return L().vtf_silhouette_sweep(gr._h, ptr(Xd), N, D, lo, hi, ptr(lab), len(ks), ks.ctypes.data, freq.ctypes.data,
                                    ptr(sil))


def test_silhouette_sweep_shards(gr):
    """Row ranges that start off a 64-row tile, one-row ranges and the n * r // 3 thirds equal the
    full result's slice bit for bit (a row's sums do not depend on its tile); an empty range
    writes nothing."""
    X, sets = ki.score_case(130, 100)
    lbs = [sets[n] for n in ('k2', 'k16', 'k40', 'single')]
    full = gr.silhouette_sweep(X, lbs)
    thirds = [(130 * r // 3, 130 * (r + 1) // 3) for r in range(3)]
    for lo, hi in [(0, 1), (1, 64), (63, 130), (87, 88)] + thirds:
        np.testing.assert_array_equal(gr.silhouette_sweep(X, lbs, lo, hi), full[:, lo:hi], err_msg='%d:%d' % (lo, hi))
    lab = dev(np.stack(lbs).astype(np.uint8))
    ks = np.array([lb.max() + 1 for lb in lbs], np.int32)
    freq = np.concatenate([np.bincount(lb) for lb in lbs]).astype(np.int64)
    sil = poison((4, 2))
    for lo in (0, 64, 87, 130):
        assert sweep_raw(gr, dev(X), lab, ks, freq, lo, lo, sil) == 0
    assert (sil.cpu().numpy() == -77).all()


def test_silhouette_sweep_160_clusters(gr, g):
    """Four sets of 40 clusters fill the 160 cluster columns of one pass.  The sets are the
    golden's 40-cluster set with its labels rotated: the same partition, so every set gives
    sklearn's values (within 2e-7) and the same bits as the others."""
    X, sets = ki.score_case(263, 768)
    lbs = [(sets['k40'] + 13 * r) % 40 for r in range(4)]
    lab = dev(np.stack(lbs).astype(np.uint8))
    ks = np.full(4, 40, np.int32)
    freq = np.concatenate([np.bincount(lb, minlength=40) for lb in lbs]).astype(np.int64)
    sil = poison((4, 263))
    assert sweep_raw(gr, dev(X), lab, ks, freq, 0, 263, sil) == 0
    got = sil.cpu().numpy()
    for r in range(4):
        np.testing.assert_allclose(got[r], g['score_263_768_k40_sil'], rtol=0, atol=2e-7)
        np.testing.assert_array_equal(got[r], got[0])


# ------------------------------------------------------------------ vtf_cluster_sums / vtf_cluster_dist
@pytest.mark.parametrize('N,D,k', [(1, 1, 1), (257, 100, 17), (130, 768, 64)])
def test_cluster_sums_and_dist(gr, N, D, k):
    """Per-cluster float64 sums, |x|^2 sums and distance-to-centroid sums against long double
    numpy.  The atomics' order is free, so each entry may be off by N 2^-52 times the sum of its
    absolute addends; the counts are exact."""
    rng = np.random.default_rng(N + D + k)
    X = rng.normal(0.2, 1, (N, D)).astype(np.float32)
    lb = rng.integers(0, k, N).astype(np.int32)
    lb[rng.permutation(N)[:k]] = np.arange(k)
    Xd, ld = dev(X), dev(lb)
    sums, sqn = poison((k, D), torch.float64), poison((k,), torch.float64)
    cnt = poison((k,), torch.int64)
    assert L().vtf_cluster_sums(gr._h, ptr(Xd), N, D, ptr(ld), k, ptr(sums), ptr(sqn), ptr(cnt)) == 0
    sums, sqn, cnt = sums.cpu().numpy(), sqn.cpu().numpy(), cnt.cpu().numpy()
    np.testing.assert_array_equal(cnt, np.bincount(lb, minlength=k))
    Xl = X.astype(np.longdouble)
    onehot = (lb[None, :] == np.arange(k)[:, None]).astype(np.longdouble)
    bound = N * 2.0 ** -52
    assert (np.abs(sums - onehot @ Xl) <= bound * (onehot @ np.abs(Xl))).all()
    rsq = onehot @ (Xl * Xl).sum(1)
    assert (np.abs(sqn - rsq) <= bound * rsq).all()
    cent = sums / cnt[:, None]
    dsum = poison((k,), torch.float64)
    assert L().vtf_cluster_dist(gr._h, ptr(Xd), N, D, ptr(ld), k, ptr(dev(cent)), ptr(dsum)) == 0
    rd = onehot @ np.sqrt(((Xl - cent.astype(np.longdouble)[lb]) ** 2).sum(1))
    assert (np.abs(dsum.cpu().numpy() - rd) <= bound * rd).all()


# ------------------------------------------------------------------ refusals
def test_refusals_leave_outputs_alone(gr):
    """Every documented refusal returns its code before anything is launched: the poisoned outputs
    are unchanged."""
    N, D = 8, 32
    X = np.random.default_rng(0).normal(0, 1, (N, D)).astype(np.float32)
    Xd = dev(X)
    outs = []

    def out(shape, dtype=torch.float32):
        outs.append(poison(shape, dtype))
        return outs[-1]
    # k = 65
    C = dev(np.zeros((65, D), np.float32))
    changed = ctypes.c_int64(-77)
    assert L().vtf_kmeans_step(gr._h, ptr(Xd), N, D, ptr(C), 65, ptr(out((N,), torch.int32)), ptr(out((65, D))),
                               ptr(out((65,))), ctypes.byref(changed)) == E_LIMIT
    assert changed.value == -77
    # candidate rows: T = 0, T = 17, T * D * 4 > 64 KiB, an index of -1 and one of N
    ids, rows = np.zeros(17, np.int64), out((17, N))
    assert L().vtf_sqdist_rows(gr._h, ptr(Xd), N, D, ids.ctypes.data, 0, ptr(rows)) == E_ARG
    assert L().vtf_sqdist_rows(gr._h, ptr(Xd), N, D, ids.ctypes.data, 17, ptr(rows)) == E_ARG
    for bad in (-1, N):
        ids2 = np.array([0, bad, 1], np.int64)
        assert L().vtf_sqdist_rows(gr._h, ptr(Xd), N, D, ids2.ctypes.data, 3, ptr(rows)) == E_ARG
    wide = dev(np.zeros((4, 4096), np.float32))
    assert L().vtf_sqdist_rows(gr._h, ptr(wide), 4, 4096, ids.ctypes.data, 5, ptr(out((5, 4)))) == E_LIMIT
    # silhouette sweep: 33 sets, 161 clusters, a set of one cluster, bad row ranges
    lab = dev(np.zeros((33, N), np.uint8))
    sil = out((33, N))

    def sweep(ks, lo, hi):
        ks = np.array(ks, np.int32)
        return sweep_raw(gr, Xd, lab, ks, np.ones(int(ks.sum()), np.int64), lo, hi, sil)
    assert sweep([2] * 33, 0, N) == E_LIMIT
    assert sweep([40, 40, 40, 41], 0, N) == E_LIMIT
    assert sweep([2, 1], 0, N) == E_ARG
    assert sweep([2], 0, N + 1) == E_ARG
    assert sweep([2], 5, 4) == E_ARG
    # silhouette from the matrix: k = 65, N = 1
    Dm, lb, fr = dev(np.zeros((N, N), np.float32)), dev(np.zeros(N, np.int32)), dev(np.ones(65, np.int64))
    sil1 = out((N,))
    assert L().vtf_silhouette_samples(gr._h, ptr(Dm), N, ptr(lb), 65, ptr(fr), ptr(sil1)) == E_LIMIT
    assert L().vtf_silhouette_samples(gr._h, ptr(Dm), 1, ptr(lb), 2, ptr(fr), ptr(sil1)) == E_ARG
    torch.cuda.synchronize()
    for o in outs:
        assert (o.cpu().numpy() == -77).all()
    with pytest.raises(ValueError):
        gr.kmeans(np.zeros((70, 8), np.float32), 65)


# ------------------------------------------------------------------ end to end
def check_scores(gr, X, lb, want):
    got = [gr.silhouette_score(X, lb), gr.calinski_harabasz_score(X, lb), gr.davies_bouldin_score(X, lb)]
    np.testing.assert_allclose(got[0], want[0], rtol=0, atol=2e-7)
    np.testing.assert_allclose(got[1:], want[1:], rtol=1e-5)


@pytest.mark.parametrize('case', ki.EDGE_CASES, ids=_ids)
def test_kmeans_edge_goldens(gr, g, case):
    """Grouper.kmeans equals sklearn's KMeans(k, random_state=0, n_init='auto') labels for k = 17,
    33, 64 and 24 (5 and 6 k-means++ candidates, every cluster pass), D = 768, 100, 40, 31, 520 and
    1000; silhouette (2e-7), CH and DB (rtol 1e-5) on those labels equal sklearn's."""
    X = ki.edge_case(*case)
    key = 'edge_%d_%d_%d' % case
    assert ki.sha(X) == str(g[key + '_sha'])
    lb = gr.kmeans(X, case[2])
    np.testing.assert_array_equal(lb, g[key + '_labels'])
    check_scores(gr, X, lb, g[key + '_scores'])


@pytest.mark.parametrize('seed', ki.DUP_SEEDS)
def test_kmeans_empty_clusters(g, seed):
    """8 distinct rows, 12 clusters: vtf_center_dist / _relocate_empty and k_average's empty branch
    run as often as in the CPU stand-in (which equals sklearn there), and the labels are
    sklearn's."""
    from videotofaces.kmeans import Grouper

    class Counting(ki.CountingMixin, Grouper):
        pass
    X = ki.dup_case(seed)
    key = 'dup_%d' % seed
    assert ki.sha(X) == str(g[key + '_sha'])
    cg = Counting('cuda:0')
    np.testing.assert_array_equal(cg.kmeans(X, ki.DUP_K), g[key + '_labels'])
    assert cg.relocations == int(g[key + '_relocations']) > 0
    assert cg.empty_averages == int(g[key + '_empty_averages']) > 0


def test_kmeans_wide_rows(gr):
    """D = 4160: four k-means++ candidate rows (k = 9) pass vtf_sqdist_rows' 64 KiB of LDS, so
    Grouper._sqdist_rows asks for them in two calls; labels equal the CPU stand-in's, and the split
    rows equal one-row calls bit for bit."""
    from oracle.kmeans import CpuGrouper
    X = ki.blobs(120, 4160, 12, 0.5, seed=41)
    np.testing.assert_array_equal(gr.kmeans(X, 9), CpuGrouper().kmeans(X, 9))
    Xd = dev(X)
    ids = np.array([3, 119, 3, 0, 57], np.int64)
    got = gr._sqdist_rows(Xd, ids)
    for t, i in enumerate(ids):
        np.testing.assert_array_equal(got[t], gr._sqdist_rows(Xd, [i])[0])
    ref, bound = sqdist_reference(X, ids)
    assert (np.abs(got.astype(np.float64) - ref) <= np.spacing(ref) + bound).all()
