"""numpy restatement of the fixed-radius queries of include/sfmhip.h, with exactly their operation order.

Radius count (sfmhip_radius_count): count[i] = #{ j != i : d(i, j) <= r }, d(i, j) = sqrt((dx*dx + dy*dy) + dz*dz) in float64, i excluded
by index, a point with a non-finite coordinate has count 0 and is counted by nobody.  Two forms: all pairs (a few thousand points), and
scipy's cKDTree.query_ball_point at a slightly LARGER radius for the candidates only -- their distances are recomputed in the prescribed
order and compared with <= r.

Voxel grid (sfmhip_voxel_downsample): origin = min over the finite points - voxel * 0.5, c = floor((p - origin) / voxel), voxels in
ascending (c_x, c_y, c_z) by a stable sort of the packed key, centroids as sequential sums in ascending original index over the count."""
import numpy as np

import points_ref as pr

CELL_MAX = (1 << 21) - 1


def radius_count_allpairs(pts, r):
    pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
    n = pts.shape[0]
    count = np.zeros(n, np.int32)
    step = max(1, (1 << 24) // max(n, 1))
    for a in range(0, n, step):
        rows = np.arange(a, min(n, a + step))
        count[rows] = (pr._dist_rows(pts, rows) <= r).sum(axis=1)          # self and anything not finite: inf
    return count


def radius_count_kdtree(pts, r):
    from scipy.spatial import cKDTree
    pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
    n = pts.shape[0]
    count = np.zeros(n, np.int32)
    finite = np.flatnonzero(np.isfinite(pts).all(axis=1))
    if len(finite) < 2:
        return count
    q = pts[finite]
    # the margin: the computed distance is below the true one by at most a relative 2^-50, and squares of differences below 1e-162
    # underflow to a computed distance of 0; the tree's own arithmetic is good to a relative 1e-15
    lists = cKDTree(q).query_ball_point(q, r * (1.0 + 1e-9) + 1e-150, return_sorted=False)
    lens = np.fromiter((len(c) for c in lists), np.int64, len(lists))
    if lens.sum() == 0:
        return count
    cj = np.concatenate([np.asarray(c, np.int64) for c in lists])
    ci = np.repeat(np.arange(len(q)), lens)
    with np.errstate(over="ignore"):
        dx = q[ci, 0] - q[cj, 0]; dy = q[ci, 1] - q[cj, 1]; dz = q[ci, 2] - q[cj, 2]
        d = np.sqrt((dx * dx + dy * dy) + dz * dz)
    hit = (d <= r) & (ci != cj)
    count[finite] = np.bincount(ci[hit], minlength=len(q)).astype(np.int32)
    return count


def radius_count(pts, r):
    pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
    return radius_count_allpairs(pts, r) if pts.shape[0] <= 3000 else radius_count_kdtree(pts, r)


def radii_for_counts(pts, targets=(1, 10, 100)):
    """radii at which the median count over the finite points is about each target: the median distance to the target-th nearest
    other point (the farthest one where the cloud is smaller); nothing for a cloud without two finite points"""
    from scipy.spatial import cKDTree
    pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
    q = pts[np.isfinite(pts).all(axis=1)]
    if len(q) < 2:
        return []
    k = min(max(targets) + 1, len(q))
    d, _ = cKDTree(q).query(q, k=k)
    return [float(np.median(d[:, min(t, k - 1)])) for t in targets]


def voxel_downsample(pts, voxel):
    """(centroids m x 3, counts int32 m, voxel_of int32 n, origin 3); OverflowError where an axis needs more than 2^21 voxels"""
    pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
    n = pts.shape[0]
    voxel_of = np.full(n, -1, np.int32)
    finite = np.flatnonzero(np.isfinite(pts).all(axis=1))
    if len(finite) == 0:
        return np.empty((0, 3)), np.empty(0, np.int32), voxel_of, np.full(3, np.inf)
    p = pts[finite]
    origin = p.min(axis=0) - voxel * 0.5
    c = np.floor((p - origin) / voxel)
    if not ((c >= 0) & (c <= CELL_MAX)).all():
        raise OverflowError("the voxel is too small for the cloud's extent")
    c = c.astype(np.int64)
    key = (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]
    order = np.argsort(key, kind="stable")                    # equal keys stay in ascending original index
    ks = key[order]
    head = np.concatenate([[True], ks[1:] != ks[:-1]])
    vid = np.cumsum(head) - 1                                  # voxel number of every sorted position
    voxel_of[finite[order]] = vid
    counts = np.bincount(vid).astype(np.int32)
    starts = np.flatnonzero(head)
    ps = p[order]
    rank = np.arange(len(ps)) - starts[vid]                    # position inside the voxel
    by_rank = np.argsort(rank, kind="stable")
    bounds = np.searchsorted(rank[by_rank], np.arange(counts.max() + 1))
    sums = ps[starts].copy()                                   # x_j0
    for k in range(1, counts.max()):                           # (... + x_jk): a voxel has at most one point of rank k
        sel = by_rank[bounds[k]:bounds[k + 1]]
        sums[vid[sel]] = sums[vid[sel]] + ps[sel]
    return sums / counts[:, None].astype(np.float64), counts, voxel_of, origin
