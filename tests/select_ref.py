"""numpy restatement of sfmhip_select_views exactly as include/sfmhip.h defines it: the covisibility counts of the views, every view's
sources ranked by the sparse points shared under a sufficient triangulation angle, and every view's inverse-depth range from the order
statistics of the depths it sees.  Written from the definition: double arithmetic in the written order, integer counts.  Plus the scenes
the tests of the selection share (the planted scene of dense_ref.py with a decoy view, and its sparse points)."""
import math

import numpy as np

import dense_ref as dr


def cos2_of(min_angle_deg):
    """the squared cosine the entry takes, as the Python and C++ layers compute it"""
    c = math.cos(float(min_angle_deg) * (math.pi / 180.0))
    return c * c


def order_statistics(m):
    """the places of zlo and zhi in the ascending list of m >= 2 depths"""
    return (2 * (m - 1)) // 100, (98 * (m - 1) + 99) // 100


def widen(zlo, zhi):
    wlo, whi = 1.0 / zhi, 1.0 / zlo
    span = whi - wlo
    if not span > 0:
        span = 0.5 * wlo
    x, y = wlo - 0.25 * span, 0.5 * wlo
    return (y if y > x else x), whi + 0.25 * span


def distinct_pairs(n_views, pts, obs_cam, obs_pt):
    """(point, view) of the distinct valid pairs, ordered by point and then view; an index out of range is dropped like a non-finite point
    (what the _dev form does; the host form refuses such input)"""
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    oc = np.asarray(obs_cam, np.int64).ravel(); op = np.asarray(obs_pt, np.int64).ravel()
    ok = (oc >= 0) & (oc < n_views) & (op >= 0) & (op < len(pts))
    oc, op = oc[ok], op[ok]
    fin = np.isfinite(pts[op]).all(1) if len(op) else np.zeros(0, bool)
    key = np.unique(op[fin] * n_views + oc[fin])
    return key // n_views, key % n_views


def select_views(ext, pts, obs_cam, obs_pt, n_src, cos2_min, geometry=dr.sweep_geometry):
    """dict(shared, score, sources, n_scored, wrange, n_depth); geometry(K4, ext_ref, ext_src) supplies Rinv and c of a view
    (dense_ref.sweep_geometry, or the library's own for a comparison in every bit)"""
    ext = np.asarray(ext, np.float64).reshape(-1, 6)
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    n = len(ext)
    geo = [geometry((1.0, 1.0, 0.0, 0.0), e, np.zeros((0, 6))) for e in ext]
    Rinv = np.array([np.asarray(g[4], np.float64).ravel() for g in geo]); cen = np.array([np.asarray(g[5], np.float64).ravel() for g in geo])
    p, v = distinct_pairs(n, pts, obs_cam, obs_pt)
    with np.errstate(all="ignore"):
        a = [pts[p, k] - cen[v, k] for k in range(3)]
        z = (a[0] * Rinv[v, 2] + a[1] * Rinv[v, 5]) + a[2] * Rinv[v, 8]
        na = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]
    shared = np.zeros((n, n), np.int32); score = np.zeros((n, n), np.int32)
    t = 1
    while t < len(p):
        e = np.nonzero(p[:-t] == p[t:])[0]                               # pairs (e, e + t) of one point: view[e] < view[e + t]
        if not len(e):
            break
        f = e + t
        with np.errstate(all="ignore"):
            d = (a[0][e] * a[0][f] + a[1][e] * a[1][f]) + a[2][e] * a[2][f]
            ok = (z[e] > 0) & (z[f] > 0) & ((d <= 0) | (d * d <= cos2_min * (na[e] * na[f])))
        np.add.at(shared, (v[e], v[f]), 1); np.add.at(shared, (v[f], v[e]), 1)
        np.add.at(score, (v[e][ok], v[f][ok]), 1); np.add.at(score, (v[f][ok], v[e][ok]), 1)
        t += 1
    sources = np.zeros((n, n_src), np.int32); n_scored = np.zeros(n, np.int32)
    for i in range(n):
        others = np.array([j for j in range(n) if j != i], np.int64)
        s = score[i, others]
        first = others[s > 0][np.lexsort((others[s > 0], -s[s > 0].astype(np.int64)))]
        rest = others[s <= 0]
        with np.errstate(all="ignore"):
            dx, dy, dz = (cen[rest, k] - cen[i, k] for k in range(3))
            d2 = (dx * dx + dy * dy) + dz * dz
        rest = rest[np.lexsort((rest, d2))]
        sources[i] = np.concatenate([first, rest])[:n_src]
        n_scored[i] = min(len(first), n_src)
    wrange = np.zeros((n, 2)); n_depth = np.zeros(n, np.int32)
    for i in range(n):
        s = np.sort(z[(v == i) & (z > 0)])
        n_depth[i] = len(s)
        if len(s) >= 2:
            lo, hi = order_statistics(len(s))
            with np.errstate(all="ignore"):
                wrange[i] = widen(np.float64(s[lo]), np.float64(s[hi]))
    return dict(shared=shared, score=score, sources=sources, n_scored=n_scored, wrange=wrange, n_depth=n_depth)


# ------------------------------------------------------------------------------------------------ scenes
def decoy_scene(offset=0.05, angle=1.2, n_per_plane=300, seed=3, decoy_points=0):
    """dense_ref.Scene plus a fifth view whose centre is `offset` along x from view 0 and which is turned by `angle` about y, and sparse
    points on the two planted planes with an observation wherever a point projects inside an image in front of it.  decoy_points: that
    many further points on the decoy's axis, seen by it alone (so that it has a depth range).  Returns (scene, ext, pts, obs_cam, obs_pt)."""
    sc = dr.Scene()
    R = dr.rodrigues([0.0, angle, 0.0])
    c = np.array([offset, 0.0, 0.0])
    ext = np.vstack([sc.EXT, np.concatenate([[0.0, angle, 0.0], -R @ c])])
    sc.EXT = ext                                                         # the instance renders the fifth view too
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(-3.2, 3.2, n_per_plane), rng.uniform(-2.4, 2.4, n_per_plane)
    (nb, hb), (nf, hf) = sc.BG, sc.FG
    bg = np.stack([x, y, (hb - nb[0] * x - nb[1] * y) / nb[2]], 1)
    x0, x1, y0, y1 = sc.FG_BOX
    x, y = rng.uniform(x0, x1, n_per_plane), rng.uniform(y0, y1, n_per_plane)
    fg = np.stack([x, y, (hf - nf[0] * x - nf[1] * y) / nf[2]], 1)
    extra = c + np.outer(np.linspace(3.0, 6.0, decoy_points), R[2]) if decoy_points else np.zeros((0, 3))
    pts = np.concatenate([bg, fg, extra])
    fx, fy, cx, cy = sc.K4
    oc, op = [], []
    for i, e in enumerate(ext):
        q = pts @ dr.rodrigues(e[:3]).T + e[3:]
        with np.errstate(all="ignore"):
            u, w = fx * q[:, 0] / q[:, 2] + cx, fy * q[:, 1] / q[:, 2] + cy
        seen = np.nonzero((q[:, 2] > 0) & (u >= 0) & (u <= sc.COLS - 1) & (w >= 0) & (w <= sc.ROWS - 1))[0]
        oc.append(np.full(len(seen), i)); op.append(seen)
    return sc, ext, pts, np.concatenate(oc).astype(np.int32), np.concatenate(op).astype(np.int32)


def chain_with_ranges(images, K4, ext, sources, ranges, geometry, D, r, min_sources, min_score, rel_tol, min_consistent):
    """dense_ref.chain with an inverse-depth range per view"""
    ext = np.asarray(ext, np.float64).reshape(-1, 6)
    views = []
    for i, img in enumerate(images):
        A, b, Rrel, trel, Rinv, c = geometry(K4, ext[i], ext[list(sources[i])])
        plane, score, depth, _ = dr.plane_sweep(img, [images[j] for j in sources[i]], A, b, D, float(ranges[i][0]), float(ranges[i][1]), r, min_sources, min_score)
        views.append(dict(A=A, b=b, Rrel=Rrel, trel=trel, Rinv=Rinv, c=c, plane=plane, score=score, depth=depth))
    for i, img in enumerate(images):
        w = views[i]
        w["count"], w["keep"] = dr.depth_consistency(w["depth"], [views[j]["depth"] for j in sources[i]], K4, w["Rrel"], w["trel"], rel_tol, min_consistent)
        w["xyz"], w["bgr"] = dr.depth_to_points(w["depth"], w["keep"], img, K4, w["Rinv"], w["c"])
    return views
