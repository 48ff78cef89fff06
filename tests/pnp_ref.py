"""numpy restatement of the image registration defined in include/sfmhip.h (sfmhip_register_views): splitmix64 samples of six rows, the
11 x 12 DLT system, Gaussian elimination with complete pivoting, back-substitution, the sign rule, the multiplied-out reprojection test
with the point in front of the camera, the rounds with their stop rule.  It is vectorised over the hypotheses of a round and shares no
code with the library nor with twoview_ref.py (whose elimination is written for 8 x 9): the elimination here takes any R x (R + 1)
system.  numpy evaluates one rounded operation at a time (no contraction), its argmax returns the first maximum (the pivot rule and the
tie rule), and its sqrt and division are the correctly rounded ones, which is what the definition prescribes.  The planted scenes of the
tests are at the end."""
import numpy as np

_M1 = np.uint64(0x9E3779B97F4A7C15)
_M2 = np.uint64(0xBF58476D1CE4E5B9)
_M3 = np.uint64(0x94D049BB133111EB)
BLOCK = 1 << 22          # residuals per block of the H x m matrix
SAMPLE = 6


def r(seed, c):
    """splitmix64 on the counters c (array-like of uint64), mod 2^64"""
    c = np.asarray(c, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + (c + np.uint64(1)) * _M1
        z = (z ^ (z >> np.uint64(30))) * _M2
        z = (z ^ (z >> np.uint64(27))) * _M3
        return z ^ (z >> np.uint64(31))


def samples(seed, p, H, m):
    """H x 6 int64: the positions in a list of m >= 6 rows that the hypotheses of round p draw, in draw order"""
    assert m >= SAMPLE
    with np.errstate(over="ignore"):
        g6 = np.uint64(SAMPLE) * (np.uint64(p) * np.uint64(H) + np.arange(H, dtype=np.uint64))
    pos = np.empty((H, SAMPLE), np.int64)
    chosen = np.empty((H, 0), np.int64)                    # ascending along axis 1
    for k in range(SAMPLE):
        u = (r(seed, g6 + np.uint64(k)) % np.uint64(m - k)).astype(np.int64)
        for j in range(k):
            u = u + (u >= chosen[:, j])
        pos[:, k] = u
        chosen = np.sort(np.concatenate([chosen, u[:, None]], axis=1), axis=1)
    return pos


def design(s):
    """H x 11 x 12: the two DLT rows of each of the samples s (H x 6 x 5), without the second row of sample 5"""
    X, Y, Z, x, y = (s[..., k] for k in range(5))
    one, zero = np.ones_like(X), np.zeros_like(X)
    with np.errstate(all="ignore"):
        even = np.stack([X, Y, Z, one, zero, zero, zero, zero, -(x * X), -(x * Y), -(x * Z), -x], axis=-1)
        odd = np.stack([zero, zero, zero, zero, X, Y, Z, one, -(y * X), -(y * Y), -(y * Z), -y], axis=-1)
    A = np.stack([even, odd], axis=2).reshape(len(s), 12, 12)
    return A[:, :11, :].copy()


def null_vectors(A):
    """(f H x C, valid bool H): the unit null vector of every R x C system (C = R + 1) by elimination with complete pivoting, steps 2 to 6
    of the definition; invalid rows keep whatever the arithmetic gave"""
    A = np.array(A, np.float64)
    H, R, C = A.shape
    assert C == R + 1
    hh = np.arange(H)
    perm = np.tile(np.arange(C), (H, 1))
    valid = np.ones(H, bool)
    with np.errstate(all="ignore"):
        for k in range(R):
            sub = np.abs(A[:, k:, k:]).reshape(H, -1)
            at = np.argmax(np.where(np.isnan(sub), -1.0, sub), axis=1)         # all NaN: position 0, the pivot (k, k)
            pi, pj = k + at // (C - k), k + at % (C - k)
            row = A[hh, k, :].copy(); A[hh, k, :] = A[hh, pi, :]; A[hh, pi, :] = row
            col = A[hh, :, k].copy(); A[hh, :, k] = A[hh, :, pj]; A[hh, :, pj] = col
            c = perm[hh, k].copy(); perm[hh, k] = perm[hh, pj]; perm[hh, pj] = c
            piv = A[:, k, k]
            valid &= (piv != 0) & np.isfinite(piv)
            f = A[:, k + 1:, k] / piv[:, None]
            A[:, k + 1:, k + 1:] = A[:, k + 1:, k + 1:] - f[:, :, None] * A[:, k:k + 1, k + 1:]
        z = np.zeros((H, C))
        z[:, C - 1] = 1.0
        for k in range(R - 1, -1, -1):
            s = A[:, k, k + 1] * z[:, k + 1]
            for j in range(k + 2, C):
                s = s + A[:, k, j] * z[:, j]
            z[:, k] = -s / A[:, k, k]
        f = np.empty((H, C))
        f[hh[:, None], perm] = z
        ss = f[:, 0] * f[:, 0]
        for j in range(1, C):
            ss = ss + f[:, j] * f[:, j]
        nrm = np.sqrt(ss)
        valid &= np.isfinite(nrm) & (nrm > 0)
        f = f / nrm[:, None]
    return f, valid


def depth(P, rows):
    """len(P) x len(rows): w = ((P8 X + P9 Y) + P10 Z) + P11"""
    X, Y, Z = (rows[None, :, k] for k in range(3))
    with np.errstate(all="ignore"):
        return ((P[:, 8:9] * X + P[:, 9:10] * Y) + P[:, 10:11] * Z) + P[:, 11:12]


def hypotheses_of(s):
    """(P H x 12, valid) of the samples s (H x 6 x 5): the null vector, then the sign rule on sample row 0; NaN rows where invalid"""
    P, valid = null_vectors(design(s))
    X, Y, Z = s[:, 0, 0], s[:, 0, 1], s[:, 0, 2]
    with np.errstate(all="ignore"):
        w0 = ((P[:, 8] * X + P[:, 9] * Y) + P[:, 10] * Z) + P[:, 11]
        valid = valid & (w0 != 0) & np.isfinite(w0)
        P = np.where((w0 < 0)[:, None], -P, P)
    P[~valid] = np.nan
    return P, valid


def hypotheses(rows, seed, p, H):
    """(P H x 12, valid) of round p sampled from the list rows (m x 5)"""
    return hypotheses_of(rows[samples(seed, p, H, len(rows))])


def residual_terms(P, rows):
    """(du, dv, w), each len(P) x len(rows), in the prescribed order of operations"""
    P = np.asarray(P, np.float64).reshape(-1, 12)
    X, Y, Z, x, y = (rows[None, :, k] for k in range(5))
    c = [P[:, k:k + 1] for k in range(12)]
    with np.errstate(all="ignore"):
        u = ((c[0] * X + c[1] * Y) + c[2] * Z) + c[3]
        v = ((c[4] * X + c[5] * Y) + c[6] * Z) + c[7]
        w = ((c[8] * X + c[9] * Y) + c[10] * Z) + c[11]
        return u - x * w, v - y * w, w


def inliers(P, rows, t2):
    """bool len(P) x len(rows): w > 0 and du*du + dv*dv <= t2*(w*w)"""
    du, dv, w = residual_terms(P, rows)
    with np.errstate(all="ignore"):
        return (w > 0) & (du * du + dv * dv <= t2 * (w * w))


def counts_of(P, valid, rows, t2):
    """inlier counts of every hypothesis over rows, -1 for an invalid one"""
    H, m = len(P), len(rows)
    cnt = np.zeros(H, np.int64)
    step = max(1, BLOCK // max(m, 1))
    for h0 in range(0, H, step):
        cnt[h0:h0 + step] = inliers(P[h0:h0 + step], rows, t2).sum(axis=1)
    cnt[~valid] = -1
    return cnt


def register_view(block, count, t, H, rounds, seed, min_inliers, details=None):
    """(mask uint8 len(block), count, winner, P 12) of one view.  details: a list that receives (round, best h, best count, stopped) of
    every round that got as far as scoring."""
    block = np.ascontiguousarray(block, np.float64).reshape(-1, 5)
    stride = len(block)
    t2 = t * t
    idx0 = np.flatnonzero(np.isfinite(block[:count]).all(axis=1))
    L0 = block[idx0]
    cur = np.arange(len(L0))
    best, model, winner = -1, None, -1
    for p in range(rounds):
        if len(cur) < SAMPLE:
            break
        P, valid = hypotheses(L0[cur], seed, p, H)
        cnt = counts_of(P, valid, L0, t2)
        h = int(np.argmax(cnt))
        stopped = cnt[h] < 0 or (p > 0 and cnt[h] <= best)
        if details is not None:
            details.append((p, h, int(cnt[h]), bool(stopped)))
        if stopped:
            break
        best, model, winner = int(cnt[h]), P[h].copy(), p * H + h
        cur = np.flatnonzero(inliers(model, L0, t2)[0])
        assert len(cur) == best
    mask = np.zeros(stride, np.uint8)
    if model is None or best < min_inliers:
        return mask, 0, -1, np.full(12, np.nan)
    mask[idx0[inliers(model, L0, t2)[0]]] = 1
    return mask, best, winner, model


def register_views(blocks, counts, t, H, rounds, seed, min_inliers):
    """(mask n x stride uint8, count int32 n, winner int32 n, P n x 12) of a batch: blocks n x stride x 5"""
    blocks = np.ascontiguousarray(blocks, np.float64)
    n, stride = blocks.shape[0], blocks.shape[1]
    mask = np.zeros((n, stride), np.uint8); cnt = np.zeros(n, np.int32); win = np.full(n, -1, np.int32); P = np.full((n, 12), np.nan)
    for q in range(n):
        mask[q], cnt[q], win[q], P[q] = register_view(blocks[q], int(counts[q]), t, H, rounds, seed, min_inliers)
    return mask, cnt, win, P


def pose_from_projection(P):
    """(R 3 x 3, t 3, sv_ratio) of a 3 x 4 projection matrix on normalised coordinates, through numpy.linalg.svd"""
    P = np.asarray(P, np.float64).reshape(3, 4)
    U, S, Vt = np.linalg.svd(P[:, :3])
    with np.errstate(all="ignore"):
        return U @ Vt, P[:, 3] / S.mean(), S[0] / S[2]


# ---- the planted scenes of the tests ---------------------------------------------------------------------------------------------------
FOCAL, WIDTH, HEIGHT = 800.0, 1024, 768


def rodrigues(w):
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def planted_scene(m, out, seed, coplanar=False, noise=0.5):
    """(rows m x 5 in pixels, good bool m, R, T): m world points whose camera-frame positions fill the part of a box 4 .. 10 units in front
    of a 1024 x 768 camera of focal length 800 that the image sees (coplanar: a tilted plane through that box), the world frame turned by
    about 0.4 rad and shifted against the camera's (x_cam = R X + T); Gaussian pixel noise per axis; a fraction `out` of the observations
    replaced by uniform image positions (good = False there)."""
    rng = np.random.default_rng(seed)
    z = rng.uniform(4, 10, m)
    u = np.column_stack([rng.uniform(40, WIDTH - 40, m), rng.uniform(40, HEIGHT - 40, m)])
    if coplanar:
        a, b = rng.uniform(-0.4, 0.4, 2)                   # z = 7 + a x + b y through the pixel's ray: z = 7 / (1 - a xn - b yn)
        xn, yn = (u[:, 0] - WIDTH / 2) / FOCAL, (u[:, 1] - HEIGHT / 2) / FOCAL
        z = 7.0 / (1.0 - a * xn - b * yn)
    Xc = np.column_stack([(u[:, 0] - WIDTH / 2) / FOCAL * z, (u[:, 1] - HEIGHT / 2) / FOCAL * z, z])
    axis = rng.standard_normal(3)
    R = rodrigues(0.4 * axis / np.linalg.norm(axis))
    T = rng.uniform(-1, 1, 3)
    Xw = (Xc - T) @ R                                       # R^T (x_cam - T)
    obs = u + noise * rng.standard_normal((m, 2))
    good = np.ones(m, bool)
    bad = rng.permutation(m)[:int(round(out * m))]
    good[bad] = False
    obs[bad] = np.column_stack([rng.uniform(0, WIDTH, len(bad)), rng.uniform(0, HEIGHT, len(bad))])
    return np.column_stack([Xw, obs]), good, R, T


def normalised(rows):
    """pixel observations -> coordinates normalised by K = (800, 800, 512, 384)"""
    rows = np.array(rows, np.float64)
    rows[:, 3] = (rows[:, 3] - WIDTH / 2) / FOCAL
    rows[:, 4] = (rows[:, 4] - HEIGHT / 2) / FOCAL
    return rows


def scene_rows(m, out=0.3, seed=1, coplanar=False, noise=0.5):
    """normalised rows of planted_scene (m x 5)"""
    return normalised(planted_scene(m, out, seed, coplanar, noise)[0])
