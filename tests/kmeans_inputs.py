"""Shared by the K-means edge tests: the inputs and case lists of tests/golden/make_golden.py
gen_kmeans_edges (sklearn's answers), tests/test_kmeans_oracle.py (the numpy restatement against
them on the CPU) and tests/test_kmeans_kernels_gpu.py (the kernels against both).  The golden
stores a sha256 of every input built here, so a drift of these generators shows as a hash
mismatch and not as wrong labels."""
import hashlib

import numpy as np


def ties(N, D, k, eps, seed):
    """(X, C) float32: centers C ~ N(0, 1); each row is the float64 midpoint of two distinct
    centers plus eps * N(0, 1).  Which of the two centers a row is closer to is decided by the
    last bits of |c|^2 - 2 x.c, i.e. by the summation order.  (k = 1: the center plus noise.)"""
    rng = np.random.default_rng(seed)
    C = rng.normal(0, 1, (k, D))
    a = rng.integers(0, k, N)
    b = (a + rng.integers(1, k, N)) % k if k > 1 else a
    X = (C[a] + C[b]) / 2 + eps * rng.normal(0, 1, (N, D))
    return X.astype(np.float32), C.astype(np.float32)


def blobs(N, D, planted, sd, seed):
    """float32 [N, D]: rows around `planted` centers ~ N(0, 1) with spread sd."""
    rng = np.random.default_rng(seed)
    C = rng.normal(0, 1, (planted, D))
    return (C[rng.integers(0, planted, N)] + sd * rng.normal(0, 1, (N, D))).astype(np.float32)


def duplicates(distinct, N, D, seed):
    """float32 [N, D]: N rows drawn from `distinct` distinct rows (fewer distinct rows than
    clusters leaves clusters empty: relocation and the empty branch of the averaging run)."""
    rng = np.random.default_rng(seed)
    base = rng.normal(0, 1, (distinct, D)).astype(np.float32)
    return base[rng.integers(0, distinct, N)]


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


class CountingMixin:
    """Counts the relocation calls and the averaging calls that still see an empty cluster."""
    relocations = empty_averages = 0

    def _relocate_empty(self, *a):
        self.relocations += 1
        return super()._relocate_empty(*a)

    def _average(self, sums, w, old):
        self.empty_averages += int(np.any(np.asarray(w) == 0))
        return super()._average(sums, w, old)


# (N, D, k) of the near-tie E-step cases (eps, seed below); see test_kmeans_kernels_gpu.py for
# what each shape covers
TIES_CASES = [(1, 32, 1), (7, 40, 3), (70, 40, 17), (263, 776, 33), (300, 31, 64), (259, 520, 3),
              (515, 1000, 5), (1030, 1029, 7), (1061, 768, 17), (1061, 100, 17)]
TIES_EPS = 1e-6


def ties_case(N, D, k):
    return ties(N, D, k, TIES_EPS, seed=N + D + k)


def plain_labels(X, C):
    """argmin of |c|^2 - 2 x.c with every sum a plain sequential float32 loop over d (products
    rounded, then added): what a kernel that ignored sklearn's orders would give."""
    csq = np.zeros(C.shape[0], np.float32)
    dot = np.zeros((X.shape[0], C.shape[0]), np.float32)
    for d in range(X.shape[1]):
        csq = csq + C[:, d] * C[:, d]
        dot = dot + X[:, d:d + 1] * C[None, :, d]
    return (csq[None, :] - np.float32(2) * dot).argmin(1)


# end to end: KMeans(k, random_state=0, n_init='auto') on blobs with k + 3 planted clusters
EDGE_CASES = [(300, 768, 17), (301, 768, 33), (515, 100, 64), (263, 40, 24), (130, 31, 5), (259, 520, 3),
              (70, 1000, 6)]


def edge_case(N, D, k):
    return blobs(N, D, k + 3, 0.5, seed=N + D + k)


# empty clusters: 8 distinct rows, 12 clusters
DUP_SEEDS = [0, 5]
DUP_K = 12


def dup_case(seed):
    return duplicates(8, 200, 32, seed)


# center shift: 16 pairs of rows per width
SHIFT_D = [1, 3, 4, 5, 103, 512, 768, 1029]


def shift_case(D):
    rng = np.random.default_rng(1000 + D)
    return rng.normal(0, 1, (16, D)).astype(np.float32), rng.normal(0, 1, (16, D)).astype(np.float32)


# scores: (N, D) and the label sets by name.  A silhouette needs k <= N - 1, so N = 37 has no
# 40-cluster set.
SCORE_CASES = [(37, 24), (130, 100), (263, 768)]


def score_case(N, D):
    """X and {name: labels}: random labels with every cluster present ('k2', 'k16', 'k40'), and
    'single': four clusters plus one that holds only row N // 2."""
    rng = np.random.default_rng(N + D)
    X = blobs(N, D, 6, 0.7, seed=N * D)
    sets = {}
    for k in (2, 16, 40):
        if k <= N - 1:
            lb = rng.integers(0, k, N)
            lb[rng.permutation(N)[:k]] = np.arange(k)
            sets['k%d' % k] = lb.astype(np.int32)
    lb = rng.integers(0, 4, N)
    lb[rng.permutation(N)[:4]] = np.arange(4)
    lb[N // 2] = 4
    sets['single'] = lb.astype(np.int32)
    return X, sets
