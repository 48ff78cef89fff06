"""numpy restatement of the two-view geometric verification defined in include/sfmhip.h (sfmhip_verify_pairs): splitmix64 samples of
eight rows, the 8 x 9 system, Gaussian elimination with complete pivoting, back-substitution, the multiplied-out Sampson test, the
rounds with their stop rule.  It is vectorised over the hypotheses of a round and shares no code with the library.  numpy evaluates
a * x + b * y one rounded operation at a time (no contraction), its argmax returns the first maximum (the pivot rule and the tie
rule), and its sqrt and division are the correctly rounded ones, which is what the definition prescribes.  The scenes of the tests are
at the end."""
import numpy as np

_M1 = np.uint64(0x9E3779B97F4A7C15)
_M2 = np.uint64(0xBF58476D1CE4E5B9)
_M3 = np.uint64(0x94D049BB133111EB)
BLOCK = 1 << 22          # residuals per block of the H x m matrix


def r(seed, c):
    """splitmix64 on the counters c (array-like of uint64), mod 2^64"""
    c = np.asarray(c, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + (c + np.uint64(1)) * _M1
        z = (z ^ (z >> np.uint64(30))) * _M2
        z = (z ^ (z >> np.uint64(27))) * _M3
        return z ^ (z >> np.uint64(31))


def samples(seed, p, H, m):
    """H x 8 int64: the positions in a list of m >= 8 rows that the hypotheses of round p draw, in draw order"""
    assert m >= 8
    with np.errstate(over="ignore"):
        g8 = np.uint64(8) * (np.uint64(p) * np.uint64(H) + np.arange(H, dtype=np.uint64))
    pos = np.empty((H, 8), np.int64)
    chosen = np.empty((H, 0), np.int64)                    # ascending along axis 1
    for k in range(8):
        u = (r(seed, g8 + np.uint64(k)) % np.uint64(m - k)).astype(np.int64)
        for j in range(k):
            u = u + (u >= chosen[:, j])
        pos[:, k] = u
        chosen = np.sort(np.concatenate([chosen, u[:, None]], axis=1), axis=1)
    return pos


def design(s):
    """H x 8 x 9: the rows [x2 x1, x2 y1, x2, y2 x1, y2 y1, y2, x1, y1, 1] of the samples s (H x 8 x 4)"""
    x1, y1, x2, y2 = s[..., 0], s[..., 1], s[..., 2], s[..., 3]
    with np.errstate(all="ignore"):
        return np.stack([x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, np.ones_like(x1)], axis=-1)


def null_vectors(A):
    """(F H x 9, valid bool H): the unit null vector of every 8 x 9 system by elimination with complete pivoting; NaN rows where invalid"""
    A = np.array(A, np.float64)
    H = len(A)
    hh = np.arange(H)
    perm = np.tile(np.arange(9), (H, 1))
    valid = np.ones(H, bool)
    with np.errstate(all="ignore"):
        for k in range(8):
            sub = np.abs(A[:, k:, k:]).reshape(H, -1)
            at = np.argmax(np.where(np.isnan(sub), -1.0, sub), axis=1)         # all NaN: position 0, the pivot (k, k)
            pi, pj = k + at // (9 - k), k + at % (9 - k)
            row = A[hh, k, :].copy(); A[hh, k, :] = A[hh, pi, :]; A[hh, pi, :] = row
            col = A[hh, :, k].copy(); A[hh, :, k] = A[hh, :, pj]; A[hh, :, pj] = col
            c = perm[hh, k].copy(); perm[hh, k] = perm[hh, pj]; perm[hh, pj] = c
            piv = A[:, k, k]
            valid &= (piv != 0) & np.isfinite(piv)
            f = A[:, k + 1:, k] / piv[:, None]
            A[:, k + 1:, k + 1:] = A[:, k + 1:, k + 1:] - f[:, :, None] * A[:, k:k + 1, k + 1:]
        z = np.zeros((H, 9))
        z[:, 8] = 1.0
        for k in range(7, -1, -1):
            s = A[:, k, k + 1] * z[:, k + 1]
            for j in range(k + 2, 9):
                s = s + A[:, k, j] * z[:, j]
            z[:, k] = -s / A[:, k, k]
        f = np.empty((H, 9))
        f[hh[:, None], perm] = z
        ss = f[:, 0] * f[:, 0]
        for j in range(1, 9):
            ss = ss + f[:, j] * f[:, j]
        nrm = np.sqrt(ss)
        valid &= np.isfinite(nrm) & (nrm > 0)
        F = f / nrm[:, None]
    F[~valid] = np.nan
    return F, valid


def hypotheses(rows, seed, p, H):
    """(F H x 9, valid) of round p sampled from the list rows (m x 4)"""
    return null_vectors(design(rows[samples(seed, p, H, len(rows))]))


def sampson_terms(F, rows):
    """(e, d), each len(F) x len(rows): the numerator and the denominator of the Sampson distance, in the prescribed order"""
    F = np.asarray(F, np.float64).reshape(-1, 9)
    x1, y1, x2, y2 = (rows[None, :, k] for k in range(4))
    c = [F[:, k:k + 1] for k in range(9)]
    with np.errstate(all="ignore"):
        l0 = (c[0] * x1 + c[1] * y1) + c[2]
        l1 = (c[3] * x1 + c[4] * y1) + c[5]
        l2 = (c[6] * x1 + c[7] * y1) + c[8]
        m0 = (c[0] * x2 + c[3] * y2) + c[6]
        m1 = (c[1] * x2 + c[4] * y2) + c[7]
        e = (x2 * l0 + y2 * l1) + l2
        d = ((l0 * l0 + l1 * l1) + m0 * m0) + m1 * m1
    return e, d


def inliers(F, rows, t2):
    """bool len(F) x len(rows): e*e <= t2*d"""
    e, d = sampson_terms(F, rows)
    with np.errstate(all="ignore"):
        return e * e <= t2 * d


def counts_of(F, valid, rows, t2):
    """inlier counts of every hypothesis over rows, -1 for an invalid one"""
    H, m = len(F), len(rows)
    cnt = np.zeros(H, np.int64)
    step = max(1, BLOCK // max(m, 1))
    for h0 in range(0, H, step):
        cnt[h0:h0 + step] = inliers(F[h0:h0 + step], rows, t2).sum(axis=1)
    cnt[~valid] = -1
    return cnt


def verify_pair(block, count, t, H, rounds, seed, min_inliers, details=None):
    """(mask uint8 len(block), count, winner, F 9) of one pair.  details: a list that receives (round, best h, best count, stopped) of
    every round that got as far as scoring."""
    block = np.ascontiguousarray(block, np.float64).reshape(-1, 4)
    stride = len(block)
    t2 = t * t
    idx0 = np.flatnonzero(np.isfinite(block[:count]).all(axis=1))
    L0 = block[idx0]
    cur = np.arange(len(L0))
    best, model, winner = -1, None, -1
    for p in range(rounds):
        if len(cur) < 8:
            break
        F, valid = hypotheses(L0[cur], seed, p, H)
        cnt = counts_of(F, valid, L0, t2)
        h = int(np.argmax(cnt))
        stopped = cnt[h] < 0 or (p > 0 and cnt[h] <= best)
        if details is not None:
            details.append((p, h, int(cnt[h]), bool(stopped)))
        if stopped:
            break
        best, model, winner = int(cnt[h]), F[h].copy(), p * H + h
        cur = np.flatnonzero(inliers(model, L0, t2)[0])
        assert len(cur) == best
    mask = np.zeros(stride, np.uint8)
    if model is None or best < min_inliers:
        return mask, 0, -1, np.full(9, np.nan)
    mask[idx0[inliers(model, L0, t2)[0]]] = 1
    return mask, best, winner, model


def verify_pairs(blocks, counts, t, H, rounds, seed, min_inliers):
    """(mask n x stride uint8, count int32 n, winner int32 n, F n x 9) of a batch: blocks n x stride x 4"""
    blocks = np.ascontiguousarray(blocks, np.float64)
    n, stride = blocks.shape[0], blocks.shape[1]
    mask = np.zeros((n, stride), np.uint8); cnt = np.zeros(n, np.int32); win = np.full(n, -1, np.int32); F = np.full((n, 9), np.nan)
    for q in range(n):
        mask[q], cnt[q], win[q], F[q] = verify_pair(blocks[q], int(counts[q]), t, H, rounds, seed, min_inliers)
    return mask, cnt, win, F


# ---- the scenes of the tests -------------------------------------------------------------------------------------------------------
FOCAL, WIDTH, HEIGHT = 800.0, 1024, 768


def _rodrigues(w):
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def two_view_scene(m, out, seed, pure_translation=False, noise=0.5):
    """(pix m x 4 float64 holding float32 values, good bool m): m matches between two 1024 x 768 images of focal length 800 that see 3-D
    points of depth 4 .. 9; camera 2 is camera 1 moved sideways and (unless pure_translation) turned a little; Gaussian pixel noise per
    axis, rounded to float32; a fraction `out` of the second image's points replaced by uniform ones (good = False there)."""
    rng = np.random.default_rng(seed)
    z = rng.uniform(4, 9, m)
    u1 = np.column_stack([rng.uniform(40, WIDTH - 40, m), rng.uniform(40, HEIGHT - 40, m)])
    X = np.column_stack([(u1[:, 0] - WIDTH / 2) / FOCAL * z, (u1[:, 1] - HEIGHT / 2) / FOCAL * z, z])
    R = np.eye(3) if pure_translation else _rodrigues(np.array([0.02, -0.05, 0.01]))
    T = np.array([-0.5, 0.03, 0.05])
    Y = X @ R.T + T
    u2 = np.column_stack([FOCAL * Y[:, 0] / Y[:, 2] + WIDTH / 2, FOCAL * Y[:, 1] / Y[:, 2] + HEIGHT / 2])
    u1 = u1 + noise * rng.standard_normal((m, 2)); u2 = u2 + noise * rng.standard_normal((m, 2))
    good = np.ones(m, bool)
    bad = rng.permutation(m)[:int(round(out * m))]
    good[bad] = False
    u2[bad] = np.column_stack([rng.uniform(0, WIDTH, len(bad)), rng.uniform(0, HEIGHT, len(bad))])
    pix = np.column_stack([u1, u2]).astype(np.float32).astype(np.float64)
    return pix, good


def normalised(pix):
    """pixels -> coordinates normalised by K = (800, 800, 512, 384), the gather of sfmhip_verify_matches_dev"""
    return (np.asarray(pix, np.float64) - np.array([WIDTH / 2, HEIGHT / 2, WIDTH / 2, HEIGHT / 2])) / FOCAL


def scene_rows(m, out=0.3, seed=1, pure_translation=False):
    """normalised rows of two_view_scene (m x 4)"""
    return normalised(two_view_scene(m, out, seed, pure_translation)[0])
