"""numpy restatement of the semi-global aggregation exactly as include/sfmhip.h defines it (sfmhip_sweep_costs, sfmhip_sgm_depth,
sfmhip_plane_sweep_sgm): the 16-bit cost of a plane score, the path recurrences in unsigned integers, the winner and its sub-plane
fit in double.  The plane scores come from dense_ref.plane_sweep (its fourth result)."""
import numpy as np

import dense_ref as dr

UNSEEN = 65535
DIRECTIONS = ((0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (-1, -1), (1, -1), (-1, 1))


def costs_of(c, cost_scale):
    """rows x cols x D uint16 from the D x rows x cols plane scores of dense_ref.plane_sweep (NaN = not scored)"""
    scored = ~np.isnan(c)
    t = (1.0 - np.where(scored, c, 0.0)) * float(cost_scale)
    q = np.floor(t + 0.5)
    C = np.where(q < 0, 0, np.where(q > 65534, 65534, q))
    C = np.where(scored, C, UNSEEN).astype(np.uint16)
    return np.ascontiguousarray(C.transpose(1, 2, 0))


def sweep_costs(ref, srcs, A, b, D, wmin, wmax, r, min_sources, cost_scale):
    return costs_of(dr.plane_sweep(ref, srcs, A, b, D, wmin, wmax, r, min_sources, -1.0)[3], cost_scale)


def _step(C, prev, P1, P2):
    """one step of the recurrence for a set of pixels: C, prev n x D int64"""
    D = C.shape[1]
    m = prev.min(1, keepdims=True)
    best = np.minimum(prev, m + P2)
    best[:, 1:] = np.minimum(best[:, 1:], prev[:, :-1] + P1)
    best[:, :D - 1] = np.minimum(best[:, :D - 1], prev[:, 1:] + P1)
    return C + best - m


def path(C, dy, dx, P1, P2):
    """L_r of the direction (dy, dx): rows x cols x D int64"""
    rows, cols, D = C.shape
    C = C.astype(np.int64)
    L = np.empty_like(C)
    if dy == 0:
        xs = range(cols) if dx > 0 else range(cols - 1, -1, -1)
        for i, x in enumerate(xs):
            L[:, x] = C[:, x] if i == 0 else _step(C[:, x], L[:, x - dx], P1, P2)
        return L
    ys = range(rows) if dy > 0 else range(rows - 1, -1, -1)
    for i, y in enumerate(ys):
        L[y] = C[y]
        if i == 0:
            continue
        x = np.arange(cols)
        has = (x - dx >= 0) & (x - dx < cols)
        xv = x[has]
        L[y, xv] = _step(C[y, xv], L[y - dy, xv - dx], P1, P2)
    return L


def aggregate(C, P1, P2, paths):
    """S: rows x cols x D uint32"""
    assert paths in (4, 8) and 0 <= P1 <= P2 <= 65535
    S = np.zeros(C.shape, np.int64)
    for dy, dx in DIRECTIONS[:paths]:
        S += path(C, dy, dx, int(P1), int(P2))
    assert S.max(initial=0) < 2 ** 32
    return S.astype(np.uint32)


def winner(C, S, wmin, wmax, max_cost):
    """(plane int32, cost uint16, sum uint32, depth float32), each rows x cols"""
    rows, cols, D = C.shape
    step = (float(wmax) - float(wmin)) / (D - 1)
    seen = C != UNSEEN
    key = np.where(seen, S.astype(np.int64), np.int64(2) ** 40)
    k = key.argmin(2)                                               # the first of the smallest
    yy, xx = np.mgrid[0:rows, 0:cols]
    Ck = C[yy, xx, k]
    win = seen.any(2) & ~(Ck > max_cost)
    km, kp = np.clip(k - 1, 0, D - 1), np.clip(k + 1, 0, D - 1)
    Sk, Sl, Sr = (S[yy, xx, j].astype(np.float64) for j in (k, km, kp))
    fit = (k > 0) & (k < D - 1) & (C[yy, xx, km] != UNSEEN) & (C[yy, xx, kp] != UNSEEN)
    den = (Sl - 2.0 * Sk) + Sr
    fit &= den > 0
    wk = float(wmin) + k.astype(np.float64) * step
    with np.errstate(all="ignore"):
        w = np.where(fit, wk + ((0.5 * (Sl - Sr)) / den) * step, wk)
        d = (1.0 / w).astype(np.float32)
    plane = np.where(win, k, -1).astype(np.int32)
    cost = np.where(win, Ck, UNSEEN).astype(np.uint16)
    ssum = np.where(win, S[yy, xx, k], 0).astype(np.uint32)
    depth = np.where(win, d, np.float32(np.nan)).astype(np.float32)
    return plane, cost, ssum, depth


def sgm_depth(C, wmin, wmax, P1, P2, paths, max_cost):
    """(plane, cost, sum, depth, S)"""
    S = aggregate(C, P1, P2, paths)
    return winner(C, S, wmin, wmax, max_cost) + (S,)


def plane_sweep_sgm(ref, srcs, A, b, D, wmin, wmax, r, min_sources, cost_scale, P1, P2, paths, max_cost):
    """(plane, cost, depth) of the fused call"""
    C = sweep_costs(ref, srcs, A, b, D, wmin, wmax, r, min_sources, cost_scale)
    plane, cost, _, depth, _ = sgm_depth(C, wmin, wmax, P1, P2, paths, max_cost)
    return plane, cost, depth


def chain(images, K4, ext, sources, geometry, D, wmin, wmax, r, min_sources, sgm, rel_tol, min_consistent):
    """dense_ref.chain with the sweep routed through the semi-global path; sgm = (cost_scale, P1, P2, paths, max_cost)"""
    ext = np.asarray(ext, np.float64).reshape(-1, 6)
    views = []
    for i, img in enumerate(images):
        A, b, Rrel, trel, Rinv, c = geometry(K4, ext[i], ext[sources[i]])
        plane, cost, depth = plane_sweep_sgm(img, [images[j] for j in sources[i]], A, b, D, wmin, wmax, r, min_sources, *sgm)
        views.append(dict(A=A, b=b, Rrel=Rrel, trel=trel, Rinv=Rinv, c=c, plane=plane, cost=cost, depth=depth))
    for i, img in enumerate(images):
        w = views[i]
        w["count"], w["keep"] = dr.depth_consistency(w["depth"], [views[j]["depth"] for j in sources[i]], K4, w["Rrel"], w["trel"], rel_tol, min_consistent)
        w["xyz"], w["bgr"] = dr.depth_to_points(w["depth"], w["keep"], img, K4, w["Rinv"], w["c"])
    return views
