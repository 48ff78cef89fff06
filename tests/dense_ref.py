"""numpy restatement of the dense-depth stages exactly as include/sfmhip.h defines them (sfmhip_plane_sweep, sfmhip_depth_consistency,
sfmhip_depth_to_points, sfmhip_sweep_geometry): int64 window sums, float32 warp coordinates in the written order, double scores.  Plus
the renderer of the planted scene the tests use: pinhole views of analytically textured planes, every pixel evaluated on its own ray
(nothing is resampled)."""
import numpy as np

F32 = np.float32


# ------------------------------------------------------------------------------------------------ geometry
def rodrigues(w):
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-15:
        return np.eye(3) + Kx
    return np.eye(3) + np.sin(th) / th * Kx + (1 - np.cos(th)) / th ** 2 * (Kx @ Kx)


def sweep_geometry(K4, ext_ref, ext_src):
    """(A float32 n x 9, b float32 n x 3, Rrel n x 9, trel n x 3, Rinv 9, c 3) of the header's geometry call"""
    fx, fy, cx, cy = K4
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
    Rr, tr = rodrigues(ext_ref[:3]), np.asarray(ext_ref[3:], np.float64)
    A, b, Rrel, trel = [], [], [], []
    for e in np.asarray(ext_src, np.float64).reshape(-1, 6):
        Rs, ts = rodrigues(e[:3]), e[3:]
        M = Rs @ Rr.T
        t = ts - M @ tr
        Rrel.append(M.ravel()); trel.append(t)
        A.append((K @ M @ np.linalg.inv(K)).ravel()); b.append(K @ t)
    n = len(A)
    return (np.array(A).reshape(n, 9).astype(F32), np.array(b).reshape(n, 3).astype(F32), np.array(Rrel).reshape(n, 9), np.array(trel).reshape(n, 3),
            Rr.T.ravel().copy(), -Rr.T @ tr)


# ------------------------------------------------------------------------------------------------ stage 1
def gray_of(img):
    img = np.asarray(img)
    if img.ndim == 2:
        return img.astype(np.int64)
    B, G, R = (img[..., i].astype(np.int64) for i in range(3))
    return (1868 * B + 9617 * G + 4899 * R + 8192) >> 14


def _box(a, r):
    """exact sums of a (int64, rows x cols) over the (2r+1)^2 window around every pixel whose window lies inside: (rows-2r) x (cols-2r)"""
    rows, cols = a.shape
    out = np.zeros((rows - 2 * r, cols - 2 * r), np.int64)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out += a[dy:dy + rows - 2 * r, dx:dx + cols - 2 * r]
    return out


def plane_sweep(ref, srcs, A, b, D, wmin, wmax, r, min_sources, min_score):
    """(plane int32, score float32, depth float32, c) -- c: D x rows x cols plane scores, NaN where a plane is not scored (for the tests
    of the definition's quality; the library does not return it)"""
    gr = gray_of(ref)
    gs = [gray_of(s) for s in srcs]
    rows, cols = gr.shape
    n_src = len(srcs)
    A = np.asarray(A, F32).reshape(n_src, 9); b = np.asarray(b, F32).reshape(n_src, 3)
    step = (float(wmax) - float(wmin)) / (D - 1)
    plane = np.full((rows, cols), -1, np.int32); score = np.full((rows, cols), np.nan, F32); depth = np.full((rows, cols), np.nan, F32)
    c_all = np.full((D, rows, cols), np.nan)
    ih, iw = rows - 2 * r, cols - 2 * r
    if ih <= 0 or iw <= 0:
        return plane, score, depth, c_all
    n = (2 * r + 1) ** 2
    R16 = gr * 16
    Sr, Srr = _box(R16, r), _box(R16 * R16, r)
    vr = n * Srr - Sr * Sr
    u = np.arange(cols, dtype=F32)[None, :].repeat(rows, 0); v = np.arange(rows, dtype=F32)[:, None].repeat(cols, 1)
    cm1, rm1 = F32(cols - 1), F32(rows - 1)
    for k in range(D):
        wf = F32(float(wmin) + float(k) * step)
        tot = np.zeros((ih, iw)); cnt = np.zeros((ih, iw), np.int64)
        for s in range(n_src):
            a = A[s]
            with np.errstate(all="ignore"):
                q = [(a[3 * i] * u + a[3 * i + 1] * v) + (a[3 * i + 2] + wf * b[s, i]) for i in range(3)]
                assert all(x.dtype == F32 for x in q)
                sx = q[0] / q[2]; sy = q[1] / q[2]
                good = (q[2] > 0) & (sx >= 0) & (sy >= 0) & (sx < cm1) & (sy < rm1)
            sxg = np.where(good, sx, F32(0)); syg = np.where(good, sy, F32(0))
            x0f = np.floor(sxg); y0f = np.floor(syg)
            fx = np.floor((sxg - x0f) * F32(32)).astype(np.int64); fy = np.floor((syg - y0f) * F32(32)).astype(np.int64)
            x0 = x0f.astype(np.int64); y0 = y0f.astype(np.int64)
            x1 = np.minimum(x0 + 1, cols - 1); y1 = np.minimum(y0 + 1, rows - 1)          # only reached where not good
            g = gs[s]
            smp = (g[y0, x0] * (32 - fx) * (32 - fy) + g[y0, x1] * fx * (32 - fy) + g[y1, x0] * (32 - fx) * fy + g[y1, x1] * fx * fy + 32) >> 6
            smp = np.where(good, smp, 0)
            allgood = _box(good.astype(np.int64), r) == n
            Sw, Sww, Srw = _box(smp, r), _box(smp * smp, r), _box(R16 * smp, r)
            vw = n * Sww - Sw * Sw
            cov = n * Srw - Sr * Sw
            counts = allgood & (vr > 0) & (vw > 0)
            with np.errstate(all="ignore"):
                sc = cov.astype(np.float64) / np.sqrt(vr.astype(np.float64) * vw.astype(np.float64))
            tot = np.where(counts, tot + np.where(counts, sc, 0.0), tot)
            cnt += counts
        ok = cnt >= min_sources
        with np.errstate(all="ignore"):
            c_all[k, r:rows - r, r:cols - r] = np.where(ok, tot / cnt.astype(np.float64), np.nan)
    scored = ~np.isnan(c_all)
    any_scored = scored.any(0)
    cm = np.where(scored, c_all, -np.inf)
    kbest = cm.argmax(0)                                            # the first of the largest
    yy, xx = np.mgrid[0:rows, 0:cols]
    best = cm[kbest, yy, xx]
    win = any_scored & ~(best < min_score)
    km, kp = np.clip(kbest - 1, 0, D - 1), np.clip(kbest + 1, 0, D - 1)
    cl, cr = c_all[km, yy, xx], c_all[kp, yy, xx]
    fit = (kbest > 0) & (kbest < D - 1) & ~np.isnan(cl) & ~np.isnan(cr)
    with np.errstate(all="ignore"):
        den = (cl - 2.0 * best) + cr
        fit &= den < 0
        wk = float(wmin) + kbest.astype(np.float64) * step
        w = np.where(fit, wk + ((0.5 * (cl - cr)) / den) * step, wk)
        d = (1.0 / w).astype(F32)
    plane[win] = kbest[win].astype(np.int32); score[win] = best[win].astype(F32); depth[win] = d[win]
    return plane, score, depth, c_all


# ------------------------------------------------------------------------------------------------ stage 2 and 3
def _backproject(depth, K4):
    rows, cols = depth.shape
    fx, fy, cx, cy = (float(x) for x in K4)
    d = depth.astype(np.float64)
    u = np.arange(cols, dtype=np.float64)[None, :]; v = np.arange(rows, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        return ((u - cx) / fx) * d, ((v - cy) / fy) * d, d


def depth_consistency(depth, depth_srcs, K4, Rrel, trel, rel_tol, min_consistent):
    """(count uint8, keep uint8)"""
    rows, cols = depth.shape
    fx, fy, cx, cy = (float(x) for x in K4)
    fin = np.isfinite(depth)
    X0, X1, X2 = _backproject(depth, K4)
    count = np.zeros((rows, cols), np.int64)
    Rrel = np.asarray(Rrel, np.float64).reshape(-1, 9); trel = np.asarray(trel, np.float64).reshape(-1, 3)
    for s, ds in enumerate(depth_srcs):
        R, t = Rrel[s], trel[s]
        with np.errstate(all="ignore"):
            Y = [((R[3 * i] * X0 + R[3 * i + 1] * X1) + R[3 * i + 2] * X2) + t[i] for i in range(3)]
            front = fin & (Y[2] > 0)
            pu = np.floor(((fx * Y[0]) / Y[2] + cx) + 0.5); pv = np.floor(((fy * Y[1]) / Y[2] + cy) + 0.5)
            inside = front & (pu >= 0) & (pu < cols) & (pv >= 0) & (pv < rows)
            iu = np.where(inside, pu, 0).astype(np.int64); iv = np.where(inside, pv, 0).astype(np.int64)
            dsv = ds[iv, iu].astype(np.float64)
            ok = inside & np.isfinite(dsv) & (np.abs(dsv - Y[2]) <= rel_tol * Y[2])
        count += ok
    return count.astype(np.uint8), (fin & (count >= min_consistent)).astype(np.uint8)


def depth_to_points(depth, keep, img, K4, Rinv, c):
    """(xyz n x 3 float64, bgr n x 3 uint8) of the kept pixels in row-major order"""
    X0, X1, X2 = _backproject(depth, K4)
    Rinv = np.asarray(Rinv, np.float64).ravel(); c = np.asarray(c, np.float64).ravel()
    m = np.asarray(keep).astype(bool)
    with np.errstate(all="ignore"):
        xyz = np.stack([(((Rinv[3 * i] * X0 + Rinv[3 * i + 1] * X1) + Rinv[3 * i + 2] * X2) + c[i])[m] for i in range(3)], 1)
    img = np.asarray(img)
    bgr = np.repeat(img[m][:, None], 3, 1) if img.ndim == 2 else img[m]
    return xyz, np.ascontiguousarray(bgr, np.uint8)


# ------------------------------------------------------------------------------------------------ the planted scene
class Scene:
    """A tilted background plane near z = 6 and a tilted foreground rectangle near z = 4 in front of it, both textured with a sum of 14
    sinusoids of spatial frequencies up to about 12 rad per unit; pinhole views with a focal length near 110 px.  View 0 is the
    reference at the origin; views 1 .. 3 are offset by 0.3 to 0.35 in x, -x and y with a few hundredths of a radian of rotation."""
    ROWS, COLS = 72, 96
    K4 = (110.0, 110.0, 47.5, 35.5)
    EXT = np.array([[0.0, 0.0, 0.0, 0.0, 0.0, 0.0],
                    [0.01, -0.03, 0.005, -0.32, 0.01, 0.0],
                    [-0.008, 0.035, -0.004, 0.35, -0.01, 0.01],
                    [0.03, 0.006, 0.01, 0.005, -0.30, 0.0]])
    # planes n . X = h in the world frame (= camera 0); the foreground is bounded in x and y
    BG = (np.array([0.08, -0.05, 1.0]), 6.0)
    FG = (np.array([-0.10, 0.06, 1.0]), 4.0)
    FG_BOX = (-0.75, 0.65, -0.5, 0.55)

    def __init__(self, seed=7, freq_scale=1.0):
        """freq_scale: the spatial frequencies are multiplied by it (a view rendered with a longer focal length keeps its texture per pixel)"""
        rng = np.random.default_rng(seed)
        self.tex = []
        for _ in range(2):
            ang = rng.uniform(0, 2 * np.pi, 14); freq = freq_scale * rng.uniform(3.0, 12.0, 14)
            self.tex.append((freq * np.cos(ang), freq * np.sin(ang), rng.uniform(0, 2 * np.pi, 14), rng.uniform(0.5, 1.0, 14)))

    def _texture(self, which, X, Y):
        kx, ky, ph, amp = self.tex[which]
        t = sum(a * np.sin(x * X + y * Y + p) for x, y, p, a in zip(kx, ky, ph, amp))
        return np.clip(np.rint(127.5 + 30.0 * t), 0, 255).astype(np.uint8)

    def render(self, view, rows=None, cols=None):
        """(gray image uint8, depth along the view's z axis float64) of view `view`; every pixel's ray is intersected with the planes"""
        rows = rows or self.ROWS; cols = cols or self.COLS
        fx, fy, cx, cy = self.K4
        R = rodrigues(self.EXT[view, :3]); t = self.EXT[view, 3:]
        u, v = np.meshgrid(np.arange(cols, dtype=np.float64), np.arange(rows, dtype=np.float64))
        dirs = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1) @ R          # world directions R^T d
        org = -R.T @ t
        out = np.zeros((rows, cols), np.uint8); z = np.full((rows, cols), np.inf)
        for which, (nrm, h) in enumerate((self.BG, self.FG)):
            lam = (h - nrm @ org) / (dirs @ nrm)
            P = org + lam[..., None] * dirs
            hit = lam > 0
            if which == 1:
                x0, x1, y0, y1 = self.FG_BOX
                hit &= (P[..., 0] > x0) & (P[..., 0] < x1) & (P[..., 1] > y0) & (P[..., 1] < y1)
            hit &= lam < z
            out = np.where(hit, self._texture(which, P[..., 0], P[..., 1]), out)
            z = np.where(hit, lam, z)
        return out, z

    def plane_distance(self, xyz):
        """distance of world points to the nearer of the two planted planes"""
        d = [np.abs(xyz @ n - h) / np.linalg.norm(n) for n, h in (self.BG, self.FG)]
        return np.minimum(*d)


def discontinuity_mask(z, margin):
    """True where a pixel is farther than `margin` pixels (Chebyshev) from a jump of the true depth map z"""
    rows, cols = z.shape
    jump = np.zeros((rows, cols), bool)
    dx = np.abs(np.diff(z, axis=1)) > 0.5; dy = np.abs(np.diff(z, axis=0)) > 0.5
    jump[:, :-1] |= dx; jump[:, 1:] |= dx; jump[:-1, :] |= dy; jump[1:, :] |= dy
    near = np.zeros_like(jump)
    ys, xs = np.nonzero(jump)
    for y, x in zip(ys, xs):
        near[max(0, y - margin):y + margin + 1, max(0, x - margin):x + margin + 1] = True
    return ~near


# ------------------------------------------------------------------------------------------------ the whole chain on a set of views
def nearest_sources(ext, n_src):
    """for every view the n_src other views with the nearest camera centres (ties: the lower index)"""
    ext = np.asarray(ext, np.float64).reshape(-1, 6)
    cen = np.array([-rodrigues(e[:3]).T @ e[3:] for e in ext])
    out = []
    for i in range(len(ext)):
        d = np.linalg.norm(cen - cen[i], axis=1); d[i] = np.inf
        out.append([int(j) for j in np.argsort(d, kind="stable")[:n_src]])
    return out


def chain(images, K4, ext, sources, geometry, D, wmin, wmax, r, min_sources, min_score, rel_tol, min_consistent):
    """every view swept against its sources, checked against their depth maps and exported: a list of dicts per view.  geometry(K4,
    ext_ref, ext_src) supplies the arrays (sweep_geometry above, or the library's own)"""
    ext = np.asarray(ext, np.float64).reshape(-1, 6)
    views = []
    for i, img in enumerate(images):
        A, b, Rrel, trel, Rinv, c = geometry(K4, ext[i], ext[sources[i]])
        plane, score, depth, _ = plane_sweep(img, [images[j] for j in sources[i]], A, b, D, wmin, wmax, r, min_sources, min_score)
        views.append(dict(A=A, b=b, Rrel=Rrel, trel=trel, Rinv=Rinv, c=c, plane=plane, score=score, depth=depth))
    for i, img in enumerate(images):
        w = views[i]
        w["count"], w["keep"] = depth_consistency(w["depth"], [views[j]["depth"] for j in sources[i]], K4, w["Rrel"], w["trel"], rel_tol, min_consistent)
        w["xyz"], w["bgr"] = depth_to_points(w["depth"], w["keep"], img, K4, w["Rinv"], w["c"])
    return views
