"""numpy + scipy restatement of the clustering of include/sfmhip.h (sfmhip_cluster_dbscan, sfmhip_largest_cluster).

count[i] is the radius count of tests/radius_ref.py; point i is core iff it is finite and count[i] + 1 >= min_points; two core points
with computed d(i, j) <= r are linked; a cluster is a connected component of the core points, numbered in ascending order of its
smallest core index; a finite non-core point takes the smallest number among its core neighbours within r (border), everything else is
-1.  sizes[c] counts core and border points together.

Two forms that share nothing but the distance formula: all pairs on a dense boolean matrix (a few thousand points), and scipy's
cKDTree.query_pairs at a slightly LARGER radius for the candidate pairs only, whose distances are recomputed in the prescribed order
and compared with <= r (the margin of radius_ref.radius_count_kdtree).  The components come from scipy.sparse.csgraph in both: no
union-find is written here."""
import numpy as np

import points_ref as pr

ALLPAIRS_MAX = 3000


def _sizes(labels, n_clusters):
    return np.bincount(labels[labels >= 0], minlength=n_clusters).astype(np.int32)


def cluster_allpairs(pts, r, min_points):
    """(labels int32 n, sizes int32 C, count int32 n)"""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
    n = pts.shape[0]
    labels = np.full(n, -1, np.int32)
    if n == 0:
        return labels, np.empty(0, np.int32), np.zeros(0, np.int32)
    near = pr._dist_rows(pts, np.arange(n)) <= r                    # self and anything not finite: inf, never near
    count = near.sum(axis=1).astype(np.int32)
    core = np.isfinite(pts).all(axis=1) & (count.astype(np.int64) + 1 >= min_points)
    ci = np.flatnonzero(core)
    if len(ci) == 0:
        return labels, np.empty(0, np.int32), count
    ncomp, comp = connected_components(csr_matrix(near[np.ix_(ci, ci)]), directed=False)
    # ci ascends, so a component's first occurrence in comp is its smallest core member: number the components by that position
    _, first = np.unique(comp, return_index=True)
    number = np.empty(ncomp, np.int64)
    number[np.argsort(first)] = np.arange(ncomp)
    labels[ci] = number[comp]
    rest = np.flatnonzero(~core)
    if len(rest):
        big = np.iinfo(np.int64).max
        best = np.where(near[np.ix_(rest, ci)], number[comp][None, :], big).min(axis=1)
        labels[rest] = np.where(best == big, -1, best)
    return labels, _sizes(labels, ncomp), count


def candidate_pairs(pts, r):
    """(i, j, d): the pairs i < j of finite points the kd-tree lists at the enlarged radius, original indices, and their distances in
    the prescribed operation order"""
    from scipy.spatial import cKDTree
    pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
    finite = np.flatnonzero(np.isfinite(pts).all(axis=1))
    empty = (np.empty(0, np.int64), np.empty(0, np.int64), np.empty(0))
    if len(finite) < 2:
        return empty
    q = pts[finite]
    pairs = cKDTree(q).query_pairs(r * (1.0 + 1e-9) + 1e-150, output_type="ndarray")
    if len(pairs) == 0:
        return empty
    a, b = pairs[:, 0], pairs[:, 1]
    with np.errstate(over="ignore"):
        dx = q[a, 0] - q[b, 0]; dy = q[a, 1] - q[b, 1]; dz = q[a, 2] - q[b, 2]
        d = np.sqrt((dx * dx + dy * dy) + dz * dz)
    return finite[a].astype(np.int64), finite[b].astype(np.int64), d


def cluster_kdtree(pts, r, min_points, pairs=None):
    """(labels int32 n, sizes int32 C, count int32 n); pairs: candidate_pairs(pts, r) where the caller already has them"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
    n = pts.shape[0]
    labels = np.full(n, -1, np.int32)
    if n == 0:
        return labels, np.empty(0, np.int32), np.zeros(0, np.int32)
    i, j, d = candidate_pairs(pts, r) if pairs is None else pairs
    hit = d <= r
    i, j = i[hit], j[hit]
    count = (np.bincount(i, minlength=n) + np.bincount(j, minlength=n)).astype(np.int32)
    core = np.isfinite(pts).all(axis=1) & (count.astype(np.int64) + 1 >= min_points)
    if not core.any():
        return labels, np.empty(0, np.int32), count
    cc = core[i] & core[j]
    graph = coo_matrix((np.ones(cc.sum(), np.int8), (i[cc], j[cc])), shape=(n, n))
    _, comp = connected_components(graph, directed=False)         # over all n points: the non-core ones are isolated here
    ci = np.flatnonzero(core)
    smallest = np.full(comp.max() + 1, n, np.int64)
    np.minimum.at(smallest, comp[ci], ci)                           # every component's smallest core index (n: it has no core point)
    roots = np.sort(smallest[smallest < n])
    labels[ci] = np.searchsorted(roots, smallest[comp[ci]])
    # border: over the hits with exactly one core end, the smallest label at the core end
    best = np.full(n, np.iinfo(np.int64).max, np.int64)
    for a, b in ((i, j), (j, i)):
        sel = ~core[a] & core[b]
        np.minimum.at(best, a[sel], labels[b[sel]].astype(np.int64))
    border = ~core & (best < np.iinfo(np.int64).max)
    labels[border] = best[border]
    return labels, _sizes(labels, len(roots)), count


def cluster(pts, r, min_points):
    pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
    return cluster_allpairs(pts, r, min_points) if pts.shape[0] <= ALLPAIRS_MAX else cluster_kdtree(pts, r, min_points)


def largest(labels, sizes):
    """(keep bool n, the cluster's number or -1, its size): the most points, the smallest number among equals"""
    if len(sizes) == 0:
        return np.zeros(len(labels), bool), -1, 0
    c = int(np.argmax(sizes))                                       # argmax: the first of equal maxima
    return labels == c, c, int(sizes[c])


def census(labels, count, pts, min_points):
    """(core, border, noise) numbers"""
    core = np.isfinite(np.asarray(pts, np.float64).reshape(-1, 3)).all(axis=1) & (count.astype(np.int64) + 1 >= min_points)
    return int(core.sum()), int((~core & (labels >= 0)).sum()), int((labels < 0).sum())
