"""numpy restatement of the two-view relative pose defined in include/sfmhip.h (sfmhip_relative_pose).  Where the definition promises
bits it is scalar fp64 Python, one rounded operation at a time in the prescribed order: the one-sided Jacobi SVD, the sign rule, the four
candidates, E = [t]x R and the per-row test (the last one vectorised over the rows, which changes no operation).  The refinement is a
plain numpy Levenberg-Marquardt with the definition's schedule and an analytic Jacobian; its sums run in numpy's order, so it agrees
with the library to rounding, not to the bit.  It shares no code with the library.  The inputs of the tests are at the end."""
import math

import numpy as np

import twoview_ref as tv

NAN = float("nan")


# ---- the decomposition, bit for bit -------------------------------------------------------------------------------------------------
def jacobi_svd3(M):
    """(u, v, s): M (nine values, row-major) = u diag(s) v^T by one-sided Jacobi rotations; s descending; u, v lists of rows.  The
    sweep limit, the skip test, the order and the rank-two completion of the third left vector are the library's."""
    U = [[float(M[3 * i + j]) for j in range(3)] for i in range(3)]
    V = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    for _ in range(60):
        rotated = False
        for p in range(2):
            for q in range(p + 1, 3):
                a = b = c = 0.0
                for i in range(3):
                    a += U[i][p] * U[i][p]; b += U[i][q] * U[i][q]; c += U[i][p] * U[i][q]
                if c == 0.0 or abs(c) <= 1e-16 * math.sqrt(a * b):
                    continue
                rotated = True
                zeta = (b - a) / (2.0 * c)
                tn = (1.0 if zeta >= 0 else -1.0) / (abs(zeta) + math.sqrt(1.0 + zeta * zeta))
                cs = 1.0 / math.sqrt(1.0 + tn * tn)
                sn = cs * tn
                for i in range(3):
                    up, uq, vp, vq = U[i][p], U[i][q], V[i][p], V[i][q]
                    U[i][p] = cs * up - sn * uq; U[i][q] = sn * up + cs * uq
                    V[i][p] = cs * vp - sn * vq; V[i][q] = sn * vp + cs * vq
        if not rotated:
            break
    S = [math.sqrt(U[0][j] * U[0][j] + U[1][j] * U[1][j] + U[2][j] * U[2][j]) for j in range(3)]
    order = [0, 1, 2]
    for a in range(2):
        for b in range(a + 1, 3):
            if S[order[b]] > S[order[a]]:
                order[a], order[b] = order[b], order[a]
    s = [S[order[j]] for j in range(3)]
    u = [[(U[i][order[j]] / s[j]) if s[j] > 0.0 else 0.0 for j in range(3)] for i in range(3)]
    v = [[V[i][order[j]] for j in range(3)] for i in range(3)]
    if not (s[2] > 1e-15 * s[0]):
        sgn = -1.0 if det3(v) < 0 else 1.0
        u[0][2] = sgn * (u[1][0] * u[2][1] - u[2][0] * u[1][1])
        u[1][2] = sgn * (u[2][0] * u[0][1] - u[0][0] * u[2][1])
        u[2][2] = sgn * (u[0][0] * u[1][1] - u[1][0] * u[0][1])
    return u, v, s


def det3(m):
    return (m[0][0] * (m[1][1] * m[2][2] - m[2][1] * m[1][2]) - m[1][0] * (m[0][1] * m[2][2] - m[2][1] * m[0][2]) +
            m[2][0] * (m[0][1] * m[1][2] - m[1][1] * m[0][2]))


def candidates(F):
    """(ok, [(R nine, t three)] * 4, [s0, s1, s2]) of F (nine values); ok False: F not finite, s0 not finite or s1 not > 0"""
    F = [float(x) for x in np.asarray(F, np.float64).reshape(9)]
    if not all(math.isfinite(x) for x in F):
        return False, None, [NAN] * 3
    u, v, s = jacobi_svd3(F)
    if not (s[1] > 0.0) or not math.isfinite(s[0]):
        return False, None, s
    if det3(u) < 0:
        u = [[-x for x in row] for row in u]
    if det3(v) < 0:
        v = [[-x for x in row] for row in v]
    Ra = [(u[i][0] * v[j][1] - u[i][1] * v[j][0]) + u[i][2] * v[j][2] for i in range(3) for j in range(3)]
    Rb = [(u[i][1] * v[j][0] - u[i][0] * v[j][1]) + u[i][2] * v[j][2] for i in range(3) for j in range(3)]
    t = [u[0][2], u[1][2], u[2][2]]
    tn = [-x for x in t]
    return True, [(Ra, t), (Rb, t), (Ra, tn), (Rb, tn)], s


def essential(R, t):
    """E = [t]x R, nine values"""
    R = [float(x) for x in R]; t = [float(x) for x in t]
    return ([t[1] * R[6 + j] - t[2] * R[3 + j] for j in range(3)] + [t[2] * R[j] - t[0] * R[6 + j] for j in range(3)] +
            [t[0] * R[3 + j] - t[1] * R[j] for j in range(3)])


def row_tests(R, t, rows, max_depth, cos2, terms=False):
    """(front, angle): bool arrays over rows (m x 4) under the pose (R, t); terms: the prescribed values too, for the margin test"""
    R = [np.float64(x) for x in R]; t = [np.float64(x) for x in t]
    x1, y1, x2, y2 = (rows[:, k] for k in range(4))
    with np.errstate(all="ignore"):
        p0 = (R[0] * x1 + R[1] * y1) + R[2]
        p1 = (R[3] * x1 + R[4] * y1) + R[5]
        p2 = (R[6] * x1 + R[7] * y1) + R[8]
        aa = (p0 * p0 + p1 * p1) + p2 * p2
        bb = (x2 * x2 + y2 * y2) + 1.0
        ab = (p0 * x2 + p1 * y2) + p2
        at = (p0 * t[0] + p1 * t[1]) + p2 * t[2]
        bt = (x2 * t[0] + y2 * t[1]) + t[2]
        D = aa * bb - ab * ab
        n1 = ab * bt - at * bb
        n2 = aa * bt - ab * at
        front = (D > 0) & (n1 > 0) & (n2 > 0)
        if max_depth > 0:
            front &= (n1 < max_depth * D) & (n2 < max_depth * D)
        angle = front & ((ab <= 0) | (ab * ab <= cos2 * (aa * bb)))
    if terms:
        return front, angle, dict(D=D, n1=n1, n2=n2, ab=ab, aabb=aa * bb)
    return front, angle


# ---- the refinement: numpy, to rounding ---------------------------------------------------------------------------------------------
def _skew(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def rot_exp(w):
    th = math.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    a = 1.0 - th * th / 6.0 if th < 1e-9 else math.sin(th) / th
    b = 0.5 - th * th / 24.0 if th < 1e-9 else (1.0 - math.cos(th)) / (th * th)
    K = _skew(w)
    return np.eye(3) + a * K + b * (K @ K)


def tangent_basis(t):
    """(b1, b2) of refine_motion: the unit vectors spanning the tangent plane of the sphere at t"""
    f = np.abs(t)
    k = (0 if f[0] < f[2] else 2) if f[0] < f[1] else (1 if f[1] < f[2] else 2)
    e = np.zeros(3); e[k] = 1.0
    b1 = np.cross(t, e)
    b1 = b1 / np.linalg.norm(b1)
    return b1, np.cross(t, b1)


def residuals(R, t, rows):
    """Sampson residuals e / sqrt(d) of the rows under E = [t]x R"""
    e, d = tv.sampson_terms(np.array(essential(R.reshape(9), t)), rows)
    return e[0] / np.sqrt(d[0] + 1e-300)


def jacobian(R, t, rows):
    """(r, J m x 5): the residuals and their derivatives by (w0, w1, w2, alpha, beta) at zero, R <- exp([w]x) R, t <- t + alpha b1 + beta b2"""
    b1, b2 = tangent_basis(t)
    E = _skew(t) @ R
    G = [_skew(t) @ _skew(np.eye(3)[k]) @ R for k in range(3)] + [_skew(b1) @ R, _skew(b2) @ R]
    a = np.column_stack([rows[:, 0], rows[:, 1], np.ones(len(rows))])
    b = np.column_stack([rows[:, 2], rows[:, 3], np.ones(len(rows))])
    l = a @ E.T; m = b @ E
    e = (b * l).sum(axis=1)
    d = l[:, 0] ** 2 + l[:, 1] ** 2 + m[:, 0] ** 2 + m[:, 1] ** 2 + 1e-300
    s = 1.0 / np.sqrt(d)
    r = e * s
    J = np.empty((len(rows), 5))
    for k in range(5):
        dl = a @ G[k].T; dm = b @ G[k]
        de = (b * dl).sum(axis=1)
        dd = 2.0 * (l[:, 0] * dl[:, 0] + l[:, 1] * dl[:, 1] + m[:, 0] * dm[:, 0] + m[:, 1] * dm[:, 1])
        J[:, k] = s * de - 0.5 * r * dd * (s * s)
    return r, J


def apply_step(R, t, d):
    b1, b2 = tangent_basis(t)
    tn = t + d[3] * b1 + d[4] * b2
    return rot_exp(d[:3]) @ R, tn / np.linalg.norm(tn)


def lm_round(R, t, rows, iters):
    """one round of refine_motion's schedule on rows: (R, t, cost at the start, cost at the end)"""
    cost = float((residuals(R, t, rows) ** 2).sum())
    cost0, lam = cost, 1e-3
    for _ in range(iters):
        r, J = jacobian(R, t, rows)
        A = J.T @ J; g = J.T @ r
        improved = False
        for _ in range(8):
            M = A.copy()
            M[np.diag_indices(5)] += lam * (np.diag(A) + 1e-12)
            try:
                step = np.linalg.solve(M, -g)
                np.linalg.cholesky(M)
            except np.linalg.LinAlgError:
                lam *= 10
                continue
            Rn, tn = apply_step(R, t, step)
            c1 = float((residuals(Rn, tn, rows) ** 2).sum())
            if c1 < cost:
                tiny = cost - c1 <= 1e-12 * cost
                R, t, cost, lam, improved = Rn, tn, c1, max(lam * 0.3, 1e-9), True
                if tiny:
                    return R, t, cost0, cost
                break
            lam *= 10
        if not improved:
            break
    return R, t, cost0, cost


def refine(R, t, L0, in_u, thr, rounds, iters, order=None):
    """(R, t, cost at the start of the last round, cost at its end): round 0 over the rows of U, round p >= 1 over the rows of L0 that pass
    THE Sampson test under the current E; order: a permutation of L0's rows the sums run in (the result does not depend on it but for
    rounding)"""
    R = np.array(R, np.float64).reshape(3, 3); t = np.array(t, np.float64)
    idx = np.arange(len(L0)) if order is None else np.asarray(order)
    cur = L0[idx][in_u[idx]]
    c0 = c1 = float((residuals(R, t, cur) ** 2).sum())
    if iters == 0:
        return R, t, c0, c1
    for p in range(rounds):
        if p >= 1:
            keep = tv.inliers(np.array(essential(R.reshape(9), t)), L0, thr * thr)[0]
            if keep.sum() < 8:
                break
            cur = L0[idx][keep[idx]]
        R, t, c0, c1 = lm_round(R, t, cur, iters)
    return R, t, c0, c1


# ---- the whole call -------------------------------------------------------------------------------------------------------------------
def evaluate_at(pose, block, count, thr, max_depth, min_angle):
    """(n_inl, n_front, n_angle, mask_out) of a block under the pose (twelve values): functions of the pose's bits"""
    block = np.ascontiguousarray(block, np.float64).reshape(-1, 4)
    idx0 = np.flatnonzero(np.isfinite(block[:count]).all(axis=1))
    L0 = block[idx0]
    R, t = pose[:9], pose[9:12]
    c = math.cos(min_angle)
    inl = tv.inliers(np.array(essential(R, t)), L0, thr * thr)[0]
    front, angle = row_tests(R, t, L0, max_depth, c * c)
    front = front & inl; angle = angle & inl
    mask = np.zeros(len(block), np.uint8)
    mask[idx0] = inl.astype(np.uint8) + 2 * front + 4 * angle
    return int(inl.sum()), int(front.sum()), int(angle.sum()), mask


def relative_pose_pair(block, count, mask_in, F, thr, rounds=3, iters=10, max_depth=50.0, min_angle=math.radians(2.0), order=None):
    """dict(pose 12, info 10 int, quality 5, mask_out) of one pair, as the definition in sfmhip.h"""
    block = np.ascontiguousarray(block, np.float64).reshape(-1, 4)
    stride = len(block)
    count = min(max(int(count), 0), stride)
    idx0 = np.flatnonzero(np.isfinite(block[:count]).all(axis=1))
    L0 = block[idx0]
    in_u = np.ones(len(L0), bool) if mask_in is None else np.asarray(mask_in).reshape(-1)[idx0] != 0
    n_used = int(in_u.sum())
    none = dict(pose=np.full(12, np.nan), info=np.array([0, -1, 0, 0, 0, 0, n_used, 0, 0, 0], np.int32), quality=np.full(5, np.nan),
                mask_out=np.zeros(stride, np.uint8))
    ok, cands, sv = candidates(F)
    if not ok or n_used < 8:
        return none
    c = math.cos(min_angle)
    cos2 = c * c
    n4 = [int(row_tests(R, t, L0[in_u], max_depth, cos2)[0].sum()) for R, t in cands]
    cand = int(np.argmax(n4))                                           # the first maximum
    if n4[cand] == 0:
        return none
    R, t = cands[cand]
    if rounds > 0:
        R, t, c0, c1 = refine(R, t, L0, in_u, thr, rounds, iters, order)
    else:
        R, t, c0, c1 = refine(R, t, L0, in_u, thr, 0, 0, order)
    pose = np.concatenate([np.asarray(R, np.float64).reshape(9), np.asarray(t, np.float64)])
    n_inl, n_front, n_angle, mask = evaluate_at(pose, block, count, thr, max_depth, min_angle)
    return dict(pose=pose, info=np.array([1, cand] + n4 + [n_used, n_inl, n_front, n_angle], np.int32),
                quality=np.array(sv + [c0, c1]), mask_out=mask)


def threshold_margin(pose, block, count, thr, max_depth, min_angle):
    """the smallest relative distance of any row of L0 from a threshold of the Sampson, front or parallax tests under the pose"""
    block = np.ascontiguousarray(block, np.float64).reshape(-1, 4)
    L0 = block[:count][np.isfinite(block[:count]).all(axis=1)]
    R, t = pose[:9], pose[9:12]
    e, d = tv.sampson_terms(np.array(essential(R, t)), L0)
    c = math.cos(min_angle)
    _, _, w = row_tests(R, t, L0, max_depth, c * c, terms=True)
    rel = lambda x, y: np.abs(x - y) / np.maximum(np.maximum(np.abs(x), np.abs(y)), 1e-300)
    gaps = [rel(e[0] * e[0], thr * thr * d[0]), rel(w["ab"] * w["ab"], c * c * w["aabb"])]
    scale = np.abs(w["aabb"]) + 1e-300                              # D, n1, n2 against zero: relative to aa*bb
    gaps += [np.abs(w["D"]) / scale, np.abs(w["n1"]) / scale, np.abs(w["n2"]) / scale]
    if max_depth > 0:
        gaps += [rel(w["n1"], max_depth * w["D"]), rel(w["n2"], max_depth * w["D"])]
    return float(min(g.min() for g in gaps))


# ---- angles and the inputs of the tests ---------------------------------------------------------------------------------------------
def rotation_angle(Ra, Rb):
    """the angle of Ra Rb^T in radians"""
    M = np.asarray(Ra, np.float64).reshape(3, 3) @ np.asarray(Rb, np.float64).reshape(3, 3).T
    return math.atan2(0.5 * math.sqrt((M[2, 1] - M[1, 2]) ** 2 + (M[0, 2] - M[2, 0]) ** 2 + (M[1, 0] - M[0, 1]) ** 2), 0.5 * (np.trace(M) - 1.0))


def direction_angle(ta, tb):
    ta = np.asarray(ta, np.float64); tb = np.asarray(tb, np.float64)
    return math.atan2(np.linalg.norm(np.cross(ta, tb)), float(ta @ tb))


TRUE_R = tv._rodrigues(np.array([0.02, -0.05, 0.01]))
TRUE_T = np.array([-0.5, 0.03, 0.05]) / np.linalg.norm([-0.5, 0.03, 0.05])
THR = 1.0 / tv.FOCAL
CASES18 = [(m, out, seed) for m in (300, 600) for out in (0.0, 0.3, 0.5) for seed in (1, 2, 3)]
_cache = {}


def ransac_input(m, out, seed):
    """dict(rows m x 4 normalised, good, mask, count, F) of two_view_scene behind verify_pair(H = 256, rounds = 3, t = 1 px); computed once"""
    key = (m, out, seed)
    if key not in _cache:
        pix, good = tv.two_view_scene(m, out, seed)
        rows = tv.normalised(pix)
        mask, cnt, _, F = tv.verify_pair(rows, m, THR, 256, 3, seed, 8)
        for a in (rows, good, mask, F):
            a.setflags(write=False)
        _cache[key] = dict(rows=rows, good=good, mask=mask, count=cnt, F=F)
    return _cache[key]


def cand_inputs(m=120, seeds=(4, 6, 7, 9)):
    """inputs (rows, mask, F, the cand the restatement gives, what it is) built to move the winner through the four candidates: per seed
    the plain pair, F negated, the images swapped with F^T, and camera 2 turned by a half turn about its axis (x2, y2 -> -x2, -y2; F's
    first two rows negated).  Which candidate wins depends on the signs the SVD of that F happens to give its vectors (-F has F's
    candidates: the sign rule undoes the negation), so the coverage is asserted by the CPU test, not derived."""
    if "cand" not in _cache:
        res = []
        for seed in seeds:
            pix, _ = tv.two_view_scene(m, 0.2, seed)
            rows = tv.normalised(pix)
            mask, _, _, F = tv.verify_pair(rows, m, THR, 256, 3, seed, 8)
            F3 = F.reshape(3, 3)
            turned = rows * np.array([1.0, 1.0, -1.0, -1.0])
            for what, r_, F_ in (("plain", rows, F.copy()), ("-F", rows, -F), ("swapped", rows[:, [2, 3, 0, 1]].copy(), F3.T.reshape(9).copy()),
                                 ("half turn", turned, (np.diag([-1.0, -1.0, 1.0]) @ F3).reshape(9))):
                got = relative_pose_pair(r_, len(r_), mask, F_, THR, rounds=0, iters=0)
                res.append((r_, mask, F_, int(got["info"][1]), f"{what}, seed {seed}"))
        _cache["cand"] = res
    return _cache["cand"]
