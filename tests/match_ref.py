"""Plain references for L2 descriptor matching that share nothing with oracle/ (the C restatement the device is otherwise compared
with): numpy only, the textbook definition, no blocking and no |a|^2 + |b|^2 - 2 a.b.

Integer-valued rows (what cv::SIFT emits): d^2 is summed in int64 from the differences themselves, the distance is
np.sqrt(np.float32(d^2)) -- exact, d^2 < 2^24 is asserted -- and neighbours are ordered by (float32 distance, index): a float tie goes
to the lower index even where the integers differ (cv::batchDistance compares the float32 distances).  kNN-2, the reverse best and the
distance matrix all come from that one definition.

General float rows: distances in float64, the two nearest rows and the relative gaps to the rows behind them, for tests that bound
the float32 kernels' rounding error instead of restating their summation order."""
import numpy as np

FLT_MAX = np.finfo(np.float32).max


def d2_int(q, t):
    """(nq, nt) int64 squared distances of integer-valued rows, from the differences"""
    qi = np.asarray(q).astype(np.int64); ti = np.asarray(t).astype(np.int64)
    assert np.array_equal(qi, np.asarray(q)) and np.array_equal(ti, np.asarray(t)), "rows must hold integers"
    out = np.empty((qi.shape[0], ti.shape[0]), np.int64)
    step = max(1, (1 << 22) // max(1, ti.shape[0] * ti.shape[1]))          # <= 32 MB of differences at a time
    for r in range(0, qi.shape[0], step):
        diff = qi[r:r + step, None, :] - ti[None, :, :]
        out[r:r + step] = (diff * diff).sum(-1)
    return out


def distance_matrix_int(q, t):
    """(nq, nt) float32: sqrt of the exactly represented d^2"""
    d2 = d2_int(q, t)
    assert d2.size == 0 or d2.max() < (1 << 24)
    return np.sqrt(d2.astype(np.float32))


def knn2_of_matrix(dist):
    """the two nearest columns of every row of a float32 distance matrix by (distance, index); missing: -1 / FLT_MAX"""
    nq, nt = dist.shape
    idx = np.full((nq, 2), -1, np.int32); d = np.full((nq, 2), FLT_MAX, np.float32)
    order = np.argsort(dist, axis=1, kind="stable")[:, :2]                 # stable: equal floats keep index order
    k = order.shape[1]
    idx[:, :k] = order
    d[:, :k] = np.take_along_axis(dist, order, 1)
    return idx, d


def knn2_int(q, t):
    return knn2_of_matrix(distance_matrix_int(q, t))


def reverse_best_int(q, t):
    """the nearest QUERY of every train row: kNN with the operands swapped, column 0"""
    idx, d = knn2_int(t, q)
    return idx[:, 0].copy(), d[:, 0].copy()


def knn2_f64(q, t):
    """general float rows (nt >= 3): (float64 distance matrix, indices of the two nearest rows (nq, 2), gaps (nq, 2)) with
    gaps[:, k] = (d[k + 1] - d[k]) / d[k + 1] over the sorted distances: a computed distance with relative error below gap / 2 on
    either side cannot change the order of neighbours k and k + 1"""
    q64 = np.asarray(q, np.float64); t64 = np.asarray(t, np.float64)
    diff = q64[:, None, :] - t64[None, :, :]
    dist = np.sqrt((diff * diff).sum(-1))
    order = np.argsort(dist, axis=1, kind="stable")[:, :3]
    s = np.take_along_axis(dist, order, 1)
    gaps = (s[:, 1:] - s[:, :2]) / s[:, 1:]
    return dist, order[:, :2].astype(np.int32), gaps
