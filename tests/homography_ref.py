"""numpy restatement of the homography RANSAC and the F/H model selection defined in include/sfmhip.h (sfmhip_verify_pairs_h,
sfmhip_two_view_geometry): splitmix64 samples of four rows, the 8 x 9 system, the elimination of the eight-point hypothesis, the
multiplied-out forward transfer test, the rounds with their stop rule, the selection rule.  It takes r and null_vectors (and verify_pair,
for the selection) from twoview_ref.py and shares no code with the library.  The planar and the rotation-only scene of the tests are at
the end."""
import numpy as np

import twoview_ref as tv
from twoview_ref import null_vectors, r

MIN_ROWS = 4


def samples_h(seed, p, H, m):
    """H x 4 int64: the positions in a list of m >= 4 rows that the hypotheses of round p draw, in draw order"""
    assert m >= MIN_ROWS
    with np.errstate(over="ignore"):
        g4 = np.uint64(4) * (np.uint64(p) * np.uint64(H) + np.arange(H, dtype=np.uint64))
    pos = np.empty((H, 4), np.int64)
    chosen = np.empty((H, 0), np.int64)                    # ascending along axis 1
    for k in range(4):
        u = (r(seed, g4 + np.uint64(k)) % np.uint64(m - k)).astype(np.int64)
        for j in range(k):
            u = u + (u >= chosen[:, j])
        pos[:, k] = u
        chosen = np.sort(np.concatenate([chosen, u[:, None]], axis=1), axis=1)
    return pos


def design_h(s):
    """H x 8 x 9: rows 2k and 2k + 1 of the system from sample row k of s (H x 4 x 4)"""
    x1, y1, x2, y2 = s[..., 0], s[..., 1], s[..., 2], s[..., 3]
    one, zero = np.ones_like(x1), np.zeros_like(x1)
    with np.errstate(all="ignore"):
        even = np.stack([x1, y1, one, zero, zero, zero, -(x2 * x1), -(x2 * y1), -x2], axis=-1)
        odd = np.stack([zero, zero, zero, x1, y1, one, -(y2 * x1), -(y2 * y1), -y2], axis=-1)
    return np.stack([even, odd], axis=-2).reshape(s.shape[0], 8, 9)


def hypotheses_h(rows, seed, p, H):
    """(Hm H x 9, valid) of round p sampled from the list rows (m x 4)"""
    return null_vectors(design_h(rows[samples_h(seed, p, H, len(rows))]))


def transfer_terms(Hm, rows):
    """(du, dv, w), each len(Hm) x len(rows), in the prescribed order"""
    Hm = np.asarray(Hm, np.float64).reshape(-1, 9)
    x1, y1, x2, y2 = (rows[None, :, k] for k in range(4))
    c = [Hm[:, k:k + 1] for k in range(9)]
    with np.errstate(all="ignore"):
        u = (c[0] * x1 + c[1] * y1) + c[2]
        v = (c[3] * x1 + c[4] * y1) + c[5]
        w = (c[6] * x1 + c[7] * y1) + c[8]
        du = u - x2 * w
        dv = v - y2 * w
    return du, dv, w


def inliers_h(Hm, rows, t2):
    """bool len(Hm) x len(rows): du*du + dv*dv <= t2*(w*w)"""
    du, dv, w = transfer_terms(Hm, rows)
    with np.errstate(all="ignore"):
        return du * du + dv * dv <= t2 * (w * w)


def counts_of_h(Hm, valid, rows, t2):
    """inlier counts of every hypothesis over rows, -1 for an invalid one"""
    H, m = len(Hm), len(rows)
    cnt = np.zeros(H, np.int64)
    step = max(1, tv.BLOCK // max(m, 1))
    for h0 in range(0, H, step):
        cnt[h0:h0 + step] = inliers_h(Hm[h0:h0 + step], rows, t2).sum(axis=1)
    cnt[~valid] = -1
    return cnt


def verify_pair_h(block, count, t, H, rounds, seed, min_inliers, details=None):
    """(mask uint8 len(block), count, winner, Hm 9) of one pair; details as in twoview_ref.verify_pair"""
    block = np.ascontiguousarray(block, np.float64).reshape(-1, 4)
    stride = len(block)
    t2 = t * t
    idx0 = np.flatnonzero(np.isfinite(block[:count]).all(axis=1))
    L0 = block[idx0]
    cur = np.arange(len(L0))
    best, model, winner = -1, None, -1
    for p in range(rounds):
        if len(cur) < MIN_ROWS:
            break
        Hm, valid = hypotheses_h(L0[cur], seed, p, H)
        cnt = counts_of_h(Hm, valid, L0, t2)
        h = int(np.argmax(cnt))
        stopped = cnt[h] < 0 or (p > 0 and cnt[h] <= best)
        if details is not None:
            details.append((p, h, int(cnt[h]), bool(stopped)))
        if stopped:
            break
        best, model, winner = int(cnt[h]), Hm[h].copy(), p * H + h
        cur = np.flatnonzero(inliers_h(model, L0, t2)[0])
        assert len(cur) == best
    mask = np.zeros(stride, np.uint8)
    if model is None or best < min_inliers:
        return mask, 0, -1, np.full(9, np.nan)
    mask[idx0[inliers_h(model, L0, t2)[0]]] = 1
    return mask, best, winner, model


def verify_pairs_h(blocks, counts, t, H, rounds, seed, min_inliers):
    """(mask n x stride uint8, count int32 n, winner int32 n, Hm n x 9) of a batch: blocks n x stride x 4"""
    blocks = np.ascontiguousarray(blocks, np.float64)
    n, stride = blocks.shape[0], blocks.shape[1]
    mask = np.zeros((n, stride), np.uint8); cnt = np.zeros(n, np.int32); win = np.full(n, -1, np.int32); Hm = np.full((n, 9), np.nan)
    for q in range(n):
        mask[q], cnt[q], win[q], Hm[q] = verify_pair_h(blocks[q], int(counts[q]), t, H, rounds, seed, min_inliers)
    return mask, cnt, win, Hm


def select(cF, cH, hf_ratio):
    """kind of one pair: 0 none, 1 general, 2 planar or panoramic"""
    if cF == 0 and cH == 0:
        return 0
    if cH > 0 and float(cH) >= float(hf_ratio) * float(cF):
        return 2
    return 1


def two_view_geometry(blocks, counts, t_f, t_h, H, rounds, seed, min_inliers, hf_ratio, single=None):
    """(kind int32 n, mask n x stride, count int32 n, counts2 n x 2, F n x 9, Hm n x 9, winners n x 2) of a batch.  single: the results
    (F's, H's) of verify_pairs / verify_pairs_h on the same arguments, if the caller has them already."""
    blocks = np.ascontiguousarray(blocks, np.float64)
    n, stride = blocks.shape[0], blocks.shape[1]
    mF, cF, wF, F = single[0] if single else tv.verify_pairs(blocks, counts, t_f, H, rounds, seed, min_inliers)
    mH, cH, wH, Hm = single[1] if single else verify_pairs_h(blocks, counts, t_h, H, rounds, seed, min_inliers)
    kind = np.array([select(int(a), int(b), hf_ratio) for a, b in zip(cF, cH)], np.int32).reshape(n)
    mask = np.zeros((n, stride), np.uint8); cnt = np.zeros(n, np.int32)
    for q in range(n):
        if kind[q] == 1:
            mask[q], cnt[q] = mF[q], cF[q]
        elif kind[q] == 2:
            mask[q], cnt[q] = mH[q], cH[q]
    return kind, mask, cnt, np.column_stack([cF, cH]).astype(np.int32).reshape(n, 2), F, Hm, np.column_stack([wF, wH]).astype(np.int32).reshape(n, 2)


# ---- the scenes of the tests: two_view_scene's recipe with another depth or another motion ----------------------------------------
ROTATION_ONLY = np.array([0.03, -0.12, 0.02])


def scene(kind, m, out, seed, noise=0.5):
    """(pix m x 4 float64 holding float32 values, good bool m) like twoview_ref.two_view_scene.  kind "general": that scene itself;
    "planar": the depth of the point at normalised image-1 coordinates (x, y) is 6 / (0.2 x - 0.1 y + 1), the same motion; "rotation":
    the depths of the general scene, T = 0 and the rotation vector (0.03, -0.12, 0.02)."""
    if kind == "general":
        return tv.two_view_scene(m, out, seed, noise=noise)
    assert kind in ("planar", "rotation")
    rng = np.random.default_rng(seed)
    z = rng.uniform(4, 9, m)
    u1 = np.column_stack([rng.uniform(40, tv.WIDTH - 40, m), rng.uniform(40, tv.HEIGHT - 40, m)])
    xn, yn = (u1[:, 0] - tv.WIDTH / 2) / tv.FOCAL, (u1[:, 1] - tv.HEIGHT / 2) / tv.FOCAL
    if kind == "planar":
        z = 6.0 / (0.2 * xn - 0.1 * yn + 1.0)
        R, T = tv._rodrigues(np.array([0.02, -0.05, 0.01])), np.array([-0.5, 0.03, 0.05])
    else:
        R, T = tv._rodrigues(ROTATION_ONLY), np.zeros(3)
    X = np.column_stack([xn * z, yn * z, z])
    Y = X @ R.T + T
    u2 = np.column_stack([tv.FOCAL * Y[:, 0] / Y[:, 2] + tv.WIDTH / 2, tv.FOCAL * Y[:, 1] / Y[:, 2] + tv.HEIGHT / 2])
    u1 = u1 + noise * rng.standard_normal((m, 2)); u2 = u2 + noise * rng.standard_normal((m, 2))
    good = np.ones(m, bool)
    bad = rng.permutation(m)[:int(round(out * m))]
    good[bad] = False
    u2[bad] = np.column_stack([rng.uniform(0, tv.WIDTH, len(bad)), rng.uniform(0, tv.HEIGHT, len(bad))])
    pix = np.column_stack([u1, u2]).astype(np.float32).astype(np.float64)
    return pix, good


def scene_rows(kind, m, out=0.3, seed=1):
    """normalised rows of scene (m x 4)"""
    return tv.normalised(scene(kind, m, out, seed)[0])
