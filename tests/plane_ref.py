"""numpy restatement of the RANSAC plane segmentation defined in include/sfmhip.h (sfmhip_segment_planes): splitmix64 triples, the
plane of a hypothesis, the H x m residual matrix in chunks, the winner by argmax (numpy's argmax returns the first maximum, which is
the tie rule), the peeling of planes.  It shares no code with the library.  numpy evaluates a * x + b * y one rounded operation at a
time (no contraction), and its sqrt and division are the correctly rounded ones, which is what the definition prescribes."""
import numpy as np

_M1 = np.uint64(0x9E3779B97F4A7C15)
_M2 = np.uint64(0xBF58476D1CE4E5B9)
_M3 = np.uint64(0x94D049BB133111EB)
CHUNK = 1 << 22          # residuals per block of the H x m matrix


def r(seed, c):
    """splitmix64 on the counters c (array-like of uint64), mod 2^64"""
    c = np.asarray(c, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + (c + np.uint64(1)) * _M1
        z = (z ^ (z >> np.uint64(30))) * _M2
        z = (z ^ (z >> np.uint64(27))) * _M3
        return z ^ (z >> np.uint64(31))


def triples(seed, p, H, m):
    """(u0, u1, u2) int64 arrays of H entries: three distinct positions in an active list of m >= 3 points, round p"""
    assert m >= 3
    with np.errstate(over="ignore"):
        g = np.uint64(p) * np.uint64(H) + np.arange(H, dtype=np.uint64)
        g3 = np.uint64(3) * g
        u0 = (r(seed, g3) % np.uint64(m)).astype(np.int64)
        u1 = (r(seed, g3 + np.uint64(1)) % np.uint64(m - 1)).astype(np.int64)
        u2 = (r(seed, g3 + np.uint64(2)) % np.uint64(m - 2)).astype(np.int64)
    u1 = u1 + (u1 >= u0)
    lo, hi = np.minimum(u0, u1), np.maximum(u0, u1)
    u2 = u2 + (u2 >= lo)
    u2 = u2 + (u2 >= hi)
    return u0, u1, u2


def hypotheses(A, seed, p, H):
    """(planes H x 4, valid bool H) of round p on the active points A (m x 3); an invalid hypothesis has NaN in its row"""
    u0, u1, u2 = triples(seed, p, H, len(A))
    p0, p1, p2 = A[u0], A[u1], A[u2]
    with np.errstate(all="ignore"):
        e1, e2 = p1 - p0, p2 - p0
        mx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        my = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        mz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        s = np.sqrt((mx * mx + my * my) + mz * mz)
        valid = np.isfinite(s) & (s > 0)
        a, b, c = mx / s, my / s, mz / s
        d = -((a * p0[:, 0] + b * p0[:, 1]) + c * p0[:, 2])
    pl = np.stack([a, b, c, d], axis=1)
    pl[~valid] = np.nan
    return pl, valid


def residuals(pl, A):
    """len(pl) x len(A): e = ((a x + b y) + c z) + d"""
    with np.errstate(all="ignore"):
        return ((pl[:, 0:1] * A[None, :, 0] + pl[:, 1:2] * A[None, :, 1]) + pl[:, 2:3] * A[None, :, 2]) + pl[:, 3:4]


def counts_of(pl, valid, A, t):
    """inlier counts of every hypothesis, -1 for an invalid one"""
    H, m = len(pl), len(A)
    cnt = np.zeros(H, np.int64)
    step = max(1, CHUNK // max(m, 1))
    for h0 in range(0, H, step):
        with np.errstate(invalid="ignore"):
            cnt[h0:h0 + step] = (np.abs(residuals(pl[h0:h0 + step], A)) <= t).sum(axis=1)
    cnt[~valid] = -1
    return cnt


def signed(pl):
    """all four components negated where d < 0"""
    pl = np.array(pl, np.float64)
    return -pl if pl[3] < 0 else pl


def segment(pts, t, H, seed, min_inliers, max_planes, details=None):
    """(labels int32 n, n_planes, planes max_planes x 4, counts int32 max_planes, winner int32 max_planes), rows from n_planes on NaN /
    0 / -1.  details: a list that receives the counts array (-1: invalid) of every round that got as far as scoring."""
    pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
    n = len(pts)
    labels = np.full(n, -1, np.int32)
    planes = np.full((max_planes, 4), np.nan)
    counts = np.zeros(max_planes, np.int32)
    winner = np.full(max_planes, -1, np.int32)
    finite = np.isfinite(pts).all(axis=1)
    n_planes = 0
    for p in range(max_planes):
        act = np.flatnonzero(finite & (labels == -1))
        if len(act) < 3:
            break
        A = pts[act]
        pl, valid = hypotheses(A, seed, p, H)
        cnt = counts_of(pl, valid, A, t)
        if details is not None:
            details.append(cnt)
        h = int(np.argmax(cnt))
        if cnt[h] < 0 or cnt[h] < min_inliers:
            break
        with np.errstate(invalid="ignore"):
            inl = np.abs(residuals(pl[h:h + 1], A)[0]) <= t
        assert inl.sum() == cnt[h]
        labels[act[inl]] = p
        planes[p] = signed(pl[h])
        counts[p] = cnt[h]
        winner[p] = h
        n_planes = p + 1
    return labels, n_planes, planes, counts, winner


def refined_plane(P):
    """least-squares plane of the points P by numpy.linalg.eigh of their covariance: (a, b, c, d) with the sign rule"""
    mean = P.mean(axis=0)
    Q = P - mean
    w, V = np.linalg.eigh(Q.T @ Q / len(P))
    nrm = V[:, 0] / np.linalg.norm(V[:, 0])
    return signed(np.append(nrm, -(nrm @ mean)))


# ---- the clouds of the tests -------------------------------------------------------------------------------------------------------
def _plane_points(rng, k, normal, offset, sigma):
    """k points within the unit cube's reach on the plane normal . x = offset, with Gaussian noise sigma along the normal"""
    nrm = np.asarray(normal, np.float64) / np.linalg.norm(normal)
    u = np.cross(nrm, [1.0, 0.0, 0.0] if abs(nrm[0]) < 0.9 else [0.0, 1.0, 0.0])
    u /= np.linalg.norm(u)
    v = np.cross(nrm, u)
    st = rng.uniform(-1, 1, (k, 2))
    return offset * nrm + st[:, :1] * u + st[:, 1:] * v + rng.normal(0, sigma, (k, 1)) * nrm


def planted_scene(seed=1):
    """1500, 900 and 500 points on three planes (noise sigma 0.002) plus 600 uniform clutter points in [-1,1]^3, shuffled, every 97th
    row NaN.  Returns (pts, truth): truth[i] = the plane the row was drawn from, -1 for clutter and NaN rows."""
    rng = np.random.default_rng(seed)
    parts = [_plane_points(rng, 1500, (0.1, 0.2, 1.0), 0.3, 0.002), _plane_points(rng, 900, (1.0, -0.3, 0.2), -0.4, 0.002),
             _plane_points(rng, 500, (0.2, 1.0, -0.5), 0.1, 0.002), rng.uniform(-1, 1, (600, 3))]
    pts = np.concatenate(parts)
    truth = np.concatenate([np.full(len(q), k if k < 3 else -1) for k, q in enumerate(parts)])
    order = rng.permutation(len(pts))
    pts, truth = pts[order], truth[order]
    pts[::97] = np.nan
    truth[::97] = -1
    return pts, truth


def plane_with_clutter(n_finite, seed=2):
    """n_finite finite points, 70 % on one noisy plane and the rest clutter, with a NaN row after every 50 finite ones"""
    rng = np.random.default_rng(seed + n_finite)
    k = (7 * n_finite) // 10
    fin = np.concatenate([_plane_points(rng, k, (0.3, -0.2, 1.0), 0.2, 0.002), rng.uniform(-1, 1, (n_finite - k, 3))])
    fin = fin[rng.permutation(n_finite)]
    rows = n_finite + n_finite // 50
    pts = np.full((rows, 3), np.nan)
    keep = np.ones(rows, bool)
    keep[50::51] = False
    keep[np.flatnonzero(keep)[n_finite:]] = False
    assert keep.sum() == n_finite
    pts[keep] = fin
    return pts


def lattice_scene():
    """an 8 x 8 integer lattice at z = 0, 20 lattice points at z = +1, 20 at z = -1 and 10 at z = 2: every residual against the plane
    z = 0 is an exact integer"""
    rng = np.random.default_rng(5)
    g = np.stack(np.meshgrid(np.arange(8.0), np.arange(8.0), indexing="ij"), -1).reshape(-1, 2)
    rows = [np.column_stack([g, np.zeros(64)])]
    for z, k in ((1.0, 20), (-1.0, 20), (2.0, 10)):
        sel = g[rng.choice(64, k, replace=False)]
        rows.append(np.column_stack([sel, np.full(k, z)]))
    pts = np.concatenate(rows)
    return pts[rng.permutation(len(pts))]


def tie_scene(scene_seed=2):
    """two 20 x 20 integer lattices at z = 0 and z = 10 plus 400 clutter points at non-integer heights, shuffled: at t = 0 every triple
    from one lattice counts exactly 400"""
    rng = np.random.default_rng(scene_seed)
    g = np.stack(np.meshgrid(np.arange(20.0), np.arange(20.0), indexing="ij"), -1).reshape(-1, 2)
    clutter = np.column_stack([rng.uniform(0, 19, (400, 2)), rng.integers(1, 9, 400) + rng.uniform(0.25, 0.75, 400)])
    pts = np.concatenate([np.column_stack([g, np.zeros(400)]), np.column_stack([g, np.full(400, 10.0)]), clutter])
    return pts[rng.permutation(len(pts))]
