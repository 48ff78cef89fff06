"""Test-side dense restatement of the oracle's LM schedule (oracle/orc_ba.c: Jacobi scaling fixed at x0, D^2 = clamp(diag)/radius,
Huber corrector, acceptance / radius rules, the three tolerances) with ANY set of constant cameras and points, and the fixed-cost
contract of sfmhip_ba_create_ex: observations whose camera, point and intrinsics are all constant are left out of the LM loop and
their cost is added to the reported costs.  Residuals and Jacobians come from orc.reproject; the normal equations are dense over the
free columns (small scenes only: <= 16 cameras, <= 1,500 points)."""
import numpy as np

import oracle as orc


def _huber(a, s):
    """rho(s), rho'(s) of HuberLoss(a) [3P], elementwise"""
    s = np.asarray(s, np.float64)
    big = (a > 0) & (s > a * a)
    r = np.sqrt(np.where(big, s, 1.0))
    rho0 = np.where(big, 2.0 * a * r - a * a, s)
    rho1 = np.where(big, np.maximum(np.finfo(np.float64).tiny, a / r), 1.0)
    return rho0, rho1


def _rotate(e, X):
    """ceres::AngleAxisRotatePoint, rows of e (n,3) applied to rows of X (n,3), incl. the theta^2 <= DBL_EPSILON branch"""
    th2 = (e * e).sum(1)
    big = th2 > np.finfo(np.float64).eps
    th = np.sqrt(np.where(big, th2, 1.0))
    c, s = np.cos(th), np.sin(th)
    w = e / th[:, None]
    wx = np.cross(w, X)
    tmp = (w * X).sum(1) * (1.0 - c)
    full = X * c[:, None] + wx * s[:, None] + w * tmp[:, None]
    small = X + np.cross(e, X)
    return np.where(big[:, None], full, small)


def obs_costs(K4, ext, pts, oc, op, uv, huber_delta=4.0):
    """1/2 rho(|r|^2) per observation (value path, vectorised)"""
    p = _rotate(ext[oc, :3], pts[op]) + ext[oc, 3:]
    r0 = K4[0] * (p[:, 0] / p[:, 2]) + K4[2] - uv[:, 0]
    r1 = K4[1] * (p[:, 1] / p[:, 2]) + K4[3] - uv[:, 1]
    return 0.5 * _huber(huber_delta, r0 * r0 + r1 * r1)[0]


def fixed_cost(K4, ext, pts, oc, op, uv, cam_const, pt_const, huber_delta=4.0):
    """1/2 sum rho over the observations with a constant camera and a constant point, from orc.reprojection_errors
    (the caller applies it only with fixed intrinsics)"""
    sel = cam_const[oc] & pt_const[op]
    e = orc.reprojection_errors(K4, ext, pts, oc[sel], op[sel], uv[sel])
    return float(0.5 * _huber(huber_delta, e * e)[0].sum())


def dense_ba(K4, ext, pts, obs_cam, obs_pt, obs_uv, opts=None, cam_const=None, pt_const=None, force_iterations=0):
    """Returns (K4, ext, pts, summary dict) like orc.ba_solve (inputs untouched).  opts: orc.ba_default_options(...) or None."""
    o = opts if opts is not None else orc.ba_default_options()
    K4 = np.array(K4, np.float64).reshape(4).copy(); ext = np.array(ext, np.float64).reshape(-1, 6).copy()
    pts = np.array(pts, np.float64).reshape(-1, 3).copy()
    oc = np.asarray(obs_cam, np.int64); op = np.asarray(obs_pt, np.int64); uv = np.asarray(obs_uv, np.float64).reshape(-1, 2)
    nc, npt = ext.shape[0], pts.shape[0]
    cfix = np.zeros(nc, bool) if cam_const is None else np.asarray(cam_const).reshape(-1).astype(bool).copy()
    if o.fix_first_camera:
        cfix[0] = True
    pfix = np.zeros(npt, bool) if pt_const is None else np.asarray(pt_const).reshape(-1).astype(bool)
    fixK = bool(o.fix_intrinsics)
    fc = 0.0
    if fixK:
        dead = cfix[oc] & pfix[op]
        fc = fixed_cost(K4, ext, pts, oc, op, uv, cfix, pfix, o.huber_delta) if dead.any() else 0.0
        oc, op, uv = oc[~dead], op[~dead], uv[~dead]
    nobs = oc.shape[0]
    # free columns: [intrinsics | free cameras ascending | free points]
    kcol = -1 if fixK else 0
    ccol = np.full(nc, -1, np.int64); base = 0 if fixK else 4
    for c in np.nonzero(~cfix)[0]:
        ccol[c] = base; base += 6
    pcol = np.full(npt, -1, np.int64)
    for p in np.nonzero(~pfix)[0]:
        pcol[p] = base; base += 3
    m = base

    def linearize(K4, ext, pts):
        A = np.zeros((2 * nobs, m)); r = np.zeros(2 * nobs); cost = 0.0
        for k in range(nobs):
            c, p = oc[k], op[k]
            rr, J = orc.reproject(K4, ext[c], pts[p], uv[k])
            rho0, rho1 = _huber(o.huber_delta, rr @ rr)
            sq = np.sqrt(rho1)
            cost += 0.5 * float(rho0)
            r[2 * k:2 * k + 2] = sq * rr
            if kcol >= 0:
                A[2 * k:2 * k + 2, 0:4] = sq * J[:, 0:4]
            if ccol[c] >= 0:
                A[2 * k:2 * k + 2, ccol[c]:ccol[c] + 6] = sq * J[:, 4:10]
            if pcol[p] >= 0:
                A[2 * k:2 * k + 2, pcol[p]:pcol[p] + 3] = sq * J[:, 10:13]
        return A, r, cost

    def free_vec(K4, ext, pts):
        x = np.zeros(m)
        if kcol >= 0:
            x[0:4] = K4
        for c in np.nonzero(ccol >= 0)[0]:
            x[ccol[c]:ccol[c] + 6] = ext[c]
        for p in np.nonzero(pcol >= 0)[0]:
            x[pcol[p]:pcol[p] + 3] = pts[p]
        return x

    def apply(K4, ext, pts, delta):
        K2, e2, p2 = K4.copy(), ext.copy(), pts.copy()
        if kcol >= 0:
            K2 += delta[0:4]
        for c in np.nonzero(ccol >= 0)[0]:
            e2[c] += delta[ccol[c]:ccol[c] + 6]
        for p in np.nonzero(pcol >= 0)[0]:
            p2[p] += delta[pcol[p]:pcol[p] + 3]
        return K2, e2, p2

    def value(K4, ext, pts):
        return float(obs_costs(K4, ext, pts, oc, op, uv, o.huber_delta).sum()) if nobs else 0.0

    summ = dict(num_residuals=2 * int(np.asarray(obs_cam).shape[0]), fixed_cost=fc)
    if m == 0:
        summ.update(termination=0, iterations=0, successful_steps=0, initial_cost=fc, final_cost=fc)
        return K4, ext, pts, summ
    A0, r, x_cost = linearize(K4, ext, pts)
    scale = 1.0 / (1.0 + np.sqrt((A0 * A0).sum(0))) if o.jacobi_scaling else np.ones(m)
    A = A0 * scale
    gmax = float(np.max(np.abs(A.T @ r / scale))) if m else 0.0
    x_norm = float(np.linalg.norm(free_vec(K4, ext, pts)))
    radius, nu = o.initial_trust_region_radius, 2.0
    it = nsucc = ninvalid = 0
    term = 1
    forced = force_iterations > 0
    max_it = force_iterations if forced else o.max_num_iterations
    initial = x_cost
    while True:
        if it >= max_it:
            term = 1; break
        if not forced and gmax <= o.gradient_tolerance:
            term = 0; break
        if not forced and radius < o.min_trust_region_radius:
            term = 0; break
        it += 1
        diag = np.clip((A * A).sum(0), o.min_lm_diagonal, o.max_lm_diagonal)
        H = A.T @ A + np.diag(diag / radius)
        ok = True
        try:
            L = np.linalg.cholesky(H)
            y = np.linalg.solve(L.T, np.linalg.solve(L, A.T @ r))
            ok = bool(np.isfinite(y).all())
        except np.linalg.LinAlgError:
            ok = False
        mcc = 0.0
        if ok:
            step = -y
            mm = A @ step
            mcc = float(-(mm * (r + 0.5 * mm)).sum())
        if not ok or not (mcc > 0.0):
            ninvalid += 1
            if ninvalid >= 5 and not forced:
                term = 2; break
            radius *= 0.5
            continue
        ninvalid = 0
        delta = step * scale
        Kc, ec, pc = apply(K4, ext, pts, delta)
        cand = value(Kc, ec, pc)
        if not np.isfinite(cand):
            cand = np.finfo(np.float64).max
        if not forced and np.linalg.norm(delta) <= o.parameter_tolerance * (x_norm + o.parameter_tolerance):
            term = 0; break
        change = x_cost - cand
        if not forced and abs(change) <= o.function_tolerance * x_cost:
            term = 0; break
        rho = change / mcc
        if rho > o.min_relative_decrease:
            K4, ext, pts = Kc, ec, pc
            x_norm = float(np.linalg.norm(free_vec(K4, ext, pts)))
            A0, r, x_cost = linearize(K4, ext, pts)
            A = A0 * scale
            gmax = float(np.max(np.abs(A.T @ r / scale)))
            t = 2.0 * rho - 1.0
            radius = min(o.max_trust_region_radius, radius / max(1.0 / 3.0, 1.0 - t ** 3))
            nu = 2.0; nsucc += 1
        else:
            radius /= nu; nu *= 2.0
    summ.update(termination=term, iterations=it, successful_steps=nsucc, initial_cost=initial + fc, final_cost=x_cost + fc,
                lm_initial_cost=initial, lm_final_cost=x_cost)
    return K4, ext, pts, summ
