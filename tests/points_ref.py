"""numpy restatement of the point-cloud neighbour search of include/sfmhip.h (sfmhip_knn_points), with exactly its operation order:
d(i, j) = sqrt((dx*dx + dy*dy) + dz*dz) in float64, neighbours ordered by (d, j), i itself excluded by index, -1 / inf where a point
has fewer than K neighbours, a point with a non-finite coordinate is nobody's neighbour and has none.

Two forms: all pairs (usable up to a few thousand points), and scipy's cKDTree for the CANDIDATES only -- their distances are recomputed
in the prescribed order and a row is accepted only if the candidates provably contain its K-set, else it is redone with all pairs."""
import numpy as np


def _dist_rows(pts, rows):
    """len(rows) x n distances in the prescribed operation order; self and anything not finite -> inf"""
    q = pts[rows]
    with np.errstate(invalid="ignore", over="ignore"):
        dx = q[:, None, 0] - pts[None, :, 0]; dy = q[:, None, 1] - pts[None, :, 1]; dz = q[:, None, 2] - pts[None, :, 2]
        d = np.sqrt((dx * dx + dy * dy) + dz * dz)
    d[np.isnan(d)] = np.inf
    d[np.arange(len(rows)), rows] = np.inf
    return d


def _allpairs_rows(pts, rows, K):
    n = pts.shape[0]
    idx = np.full((len(rows), K), -1, np.int32); dist = np.full((len(rows), K), np.inf)
    step = max(1, (1 << 24) // max(n, 1))
    for a in range(0, len(rows), step):
        r = rows[a:a + step]
        d = _dist_rows(pts, r)
        order = np.argsort(d, axis=1, kind="stable")[:, :K]          # stable: ties by ascending index
        dk = np.take_along_axis(d, order, axis=1)
        k = order.shape[1]
        idx[a:a + len(r), :k] = np.where(np.isfinite(dk), order, -1)
        dist[a:a + len(r), :k] = dk
    return idx, dist


def knn_allpairs(pts, K):
    pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
    return _allpairs_rows(pts, np.arange(pts.shape[0]), K)


def knn_kdtree(pts, K, extra=16):
    """the same table; returns (idx, dist, number of rows that needed all pairs)"""
    from scipy.spatial import cKDTree
    pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
    n = pts.shape[0]
    idx = np.full((n, K), -1, np.int32); dist = np.full((n, K), np.inf)
    finite = np.flatnonzero(np.isfinite(pts).all(axis=1))
    nf = len(finite)
    redo = np.zeros(n, bool)
    kq = min(K + extra + 1, nf)                  # the query point is among its own candidates
    if nf - 1 < K + 1 or kq < K + 2:
        redo[finite] = True                       # too few points for a margin candidate
    else:
        tree = cKDTree(pts[finite])
        _, ci = tree.query(pts[finite], k=kq)
        cand = finite[ci]                                            # nf x kq, original indices
        q = pts[finite]
        with np.errstate(over="ignore"):
            dx = q[:, None, 0] - pts[cand, 0]; dy = q[:, None, 1] - pts[cand, 1]; dz = q[:, None, 2] - pts[cand, 2]
            d = np.sqrt((dx * dx + dy * dy) + dz * dz)
        self_col = cand == finite[:, None]
        has_self = self_col.any(axis=1)
        d[self_col] = np.inf                                          # excluded by index
        # rows ordered by (d, j)
        order = np.lexsort((cand, d), axis=1)
        ds = np.take_along_axis(d, order, axis=1); js = np.take_along_axis(cand, order, axis=1)
        last = ds[:, kq - 2]                                          # the farthest real candidate (the self column sorted last)
        ok = has_self & np.isfinite(last) & (last > ds[:, K - 1])
        rows = finite[ok]
        idx[rows] = js[ok, :K]; dist[rows] = ds[ok, :K]
        redo[finite[~ok]] = True
    rr = np.flatnonzero(redo)
    if len(rr):
        idx[rr], dist[rr] = _allpairs_rows(pts, rr, K)
    return idx, dist, len(rr)


def knn(pts, K):
    pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
    if pts.shape[0] <= 3000:
        return knn_allpairs(pts, K)
    i, d, _ = knn_kdtree(pts, K)
    return i, d


def statistical_outliers(idx, dist, std_ratio):
    """(keep, mean_dist, [mu, sigma, thr]) from a neighbour table: the sequential sum ((d0 + d1) + ...) / K, inf where a neighbour is
    missing; mu, sigma over the finite means (population, two passes)"""
    K = dist.shape[1]
    m = dist[:, 0].copy()
    for k in range(1, K):
        m = m + dist[:, k]
    m = m / K
    m[(idx < 0).any(axis=1)] = np.inf
    f = m[np.isfinite(m)]
    if len(f) == 0:
        return np.zeros(len(m), bool), m, np.full(3, np.nan)
    mu = f.mean(); sigma = np.sqrt(((f - mu) ** 2).mean())
    thr = mu + std_ratio * sigma
    return m <= thr, m, np.array([mu, sigma, thr])


# ---- the clouds of the tests ---------------------------------------------------------------------------------------------
def sphere_cloud(n, seed=77):
    """the generator of test_normals_at_300k_points"""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    return d * (5.0 + 0.002 * rng.standard_normal((n, 1))) + np.array([0.3, -0.2, 0.1])


def sphere_with_outliers(n, seed=11, frac=0.01):
    """n sphere points followed by frac * n points at uniform(-4e4, 4e4)"""
    rng = np.random.default_rng(seed)
    out = rng.uniform(-4e4, 4e4, (int(round(frac * n)), 3))
    return np.concatenate([sphere_cloud(n, seed), out])


def lattice(m):
    g = np.arange(m, dtype=np.float64)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
