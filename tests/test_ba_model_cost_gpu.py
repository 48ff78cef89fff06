"""The two scalars an LM iteration decides on, against a float64 computation on the host: the model cost change -(J step).(r + J step/2)
and the candidate cost, read back as sfmhip_ba_debug_table("step_scalars")[2] and [3].

The back-substitution (ba_back_point in ba_kernels.hpp) sums the model cost change per observation in its second pass, from the
(E y) pairs of the first; the kernels that carry the next point pass take the candidate cost from that pass, the others from
obs_cost.  The reference here linearises every observation with orc.reproject, builds the normal equations over the free columns
with the damping of oracle/orc_ba.c (Jacobi scaling fixed at x0, D^2 = clamp(diag)/radius) and solves them by eliminating the 3x3
point blocks (numpy LU, no Cholesky shortcut).

Tolerance.  The bound is not an absolute one: the reference's own step differs from the device's by rounding, so both numbers
carry that difference.  The kernels as they were before the candidate cost moved into the point pass were run through this file:
their relative deviation from the reference, per scene and for both values of SFMHIP_BA_SEAM, is recorded in PARENT_DEV below.
The kernels under test may deviate by at most four times the largest of them (two roundings of a cancelling sum differ by small
factors, not by orders); no case is left out.  Measured on the kernels under test: the same bits as before in every case.

The 30-iteration traces of (24, 4000) and of the rejecting scene are compared with the ones those earlier kernels gave
(tests/golden/ba_back2_parent_trace.npz, written by thirty_iterations() below): every accepted flag, every radius, the final cost
and the parameters are equal.

A form of the back-substitution that takes the model cost change from sums of the first pass alone (A - B/2 + y_p't - y_p'V_u y_p/2,
no second linearisation) was run through this file too: it stays inside the bound (largest deviation 3.483e-16, constant_cameras),
keeps every accepted flag, but on the rejecting scene its radii leave the earlier ones by 6e-15 at iteration 9 (the first accepted
step with rho < 0.937, where the radius is a continuous function of rho) and 2e-6 at iteration 30, and 12 of 2000 points end more
than 1e-5 from where they ended before (one by 0.10).  profiles/README.md, round 21, has the figures."""
import os

import numpy as np
import pytest

import oracle as orc
from sfm_opencv_amd import synth

from ba_dense_ref import _huber, obs_costs
from test_ba_seam_gpu import _create, _rejecting_scene

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ba_back2_parent_trace.npz")

# relative deviation of the kernels BEFORE the change from the reference below: scene -> (model cost change, candidate cost); the
# same for SFMHIP_BA_SEAM unset and 0.  (The candidate cost at radius 1e16 and on the rejecting scene carries the difference between
# the reference's step and the device's: next to no damping / a start far from the solution.)
PARENT_DEV = {
    "radius_1e-2": (0.0, 1.803e-16), "radius_1e4": (1.687e-16, 4.147e-14), "radius_1e16": (1.687e-16, 7.280e-04),
    "fix_intrinsics": (1.687e-16, 9.864e-16), "no_huber": (0.0, 1.599e-14), "free_first_camera": (0.0, 3.129e-14),
    "once_and_twice": (0.0, 2.866e-14), "tracks_of_10": (1.833e-16, 1.941e-12), "wide_blocks": (1.962e-16, 6.968e-13),
    "constants": (1.957e-16, 1.055e-15), "constant_cameras": (1.742e-16, 7.816e-15), "constant_points": (0.0, 2.914e-15),
    "far_points": (1.774e-16, 4.392e-12), "rejecting": (1.801e-16, 8.590e-09),
}
MCC_TOL = 4.0 * max(v[0] for v in PARENT_DEV.values())       # 7.8e-16: the model cost change is a sum of terms of one sign
CAND_TOL = 4.0 * max(v[1] for v in PARENT_DEV.values())


# ---------------------------------------------------------------------------------------------------------------- reference
def _linearize(K4, ext, pts, oc, op, uv, huber):
    n = oc.shape[0]
    r = np.empty((n, 2)); J = np.empty((n, 2, 13))
    for k in range(n):
        rr, Jk = orc.reproject(K4, ext[oc[k]], pts[op[k]], uv[k])
        sq = np.sqrt(_huber(huber, rr @ rr)[1])
        r[k] = sq * rr; J[k] = sq * Jk
    return r, J


def _colsq(J, oc, op, nc, npt):
    """squared column norms: intrinsics (4), cameras (nc, 6), points (npt, 3)"""
    sK = (J[:, :, 0:4] ** 2).sum((0, 1))
    sC = np.zeros((nc, 6)); np.add.at(sC, oc, (J[:, :, 4:10] ** 2).sum(1))
    sP = np.zeros((npt, 3)); np.add.at(sP, op, (J[:, :, 10:13] ** 2).sum(1))
    return sK, sC, sP


def jacobi_scale(args, o):
    """the column scaling of the whole run, fixed at the initial parameters"""
    K4, ext, pts, oc, op, uv = args
    _, J = _linearize(K4, ext, pts, oc, op, uv, o.huber_delta)
    return tuple(1.0 / (1.0 + np.sqrt(s)) for s in _colsq(J, oc, op, ext.shape[0], pts.shape[0]))


def reference_step(args, o, radius, scale, cam_const=None, pt_const=None):
    """(model cost change, candidate cost) of one LM step at the parameters in args"""
    K4, ext, pts, oc, op, uv = args
    K4 = np.asarray(K4, np.float64); ext = np.asarray(ext, np.float64).reshape(-1, 6); pts = np.asarray(pts, np.float64).reshape(-1, 3)
    oc = np.asarray(oc, np.int64); op = np.asarray(op, np.int64); uv = np.asarray(uv, np.float64).reshape(-1, 2)
    nc, npt, n = ext.shape[0], pts.shape[0], oc.shape[0]
    cfix = np.zeros(nc, bool) if cam_const is None else np.asarray(cam_const).astype(bool).copy()
    if o.fix_first_camera:
        cfix[0] = True
    pfix = np.zeros(npt, bool) if pt_const is None else np.asarray(pt_const).astype(bool)
    sK, sC, sP = scale
    r, J = _linearize(K4, ext, pts, oc, op, uv, o.huber_delta)
    # camera side: [intrinsics | camera 0 | camera 1 | ...], constant columns zero (taken out of the solve below)
    mc = 4 + 6 * nc
    E = np.zeros((n, 2, mc))
    if not o.fix_intrinsics:
        E[:, :, 0:4] = J[:, :, 0:4] * sK
    JC = J[:, :, 4:10] * sC[oc][:, None, :]
    JC[cfix[oc]] = 0.0
    for j in range(6):
        E[np.arange(n), :, 4 + 6 * oc + j] = JC[:, :, j]
    F = J[:, :, 10:13] * sP[op][:, None, :]
    F[pfix[op]] = 0.0
    free_c = np.concatenate([np.full(4, not o.fix_intrinsics), np.repeat(~cfix, 6)])
    E2 = E.reshape(2 * n, mc); r2 = r.reshape(2 * n)
    U = E2.T @ E2; gc = E2.T @ r2
    V = np.zeros((npt, 3, 3)); np.add.at(V, op, np.einsum("kai,kaj->kij", F, F))
    gp = np.zeros((npt, 3)); np.add.at(gp, op, np.einsum("kai,ka->ki", F, r))
    W = np.zeros((npt, mc, 3)); np.add.at(W, op, np.einsum("kam,kaj->kmj", E, F))
    lo, hi = o.min_lm_diagonal, o.max_lm_diagonal
    U[np.diag_indices(mc)] += np.clip(np.diag(U), lo, hi) / radius
    d = np.arange(3)
    V[:, d, d] += np.clip(V[:, d, d], lo, hi) / radius
    V[pfix] = np.eye(3)
    Vi = np.linalg.inv(V)
    Vi[pfix] = 0.0
    WVi = np.einsum("pmj,pjk->pmk", W, Vi)
    S = U - WVi.transpose(1, 0, 2).reshape(mc, -1) @ W.transpose(1, 0, 2).reshape(mc, -1).T
    rhs = gc - np.einsum("pmk,pk->m", WVi, gp)
    yc = np.zeros(mc)
    f = np.nonzero(free_c)[0]
    if f.size:
        yc[f] = np.linalg.solve(S[np.ix_(f, f)], rhs[f])
    yp = np.einsum("pjk,pk->pj", Vi, gp - np.einsum("pmj,m->pj", W, yc))
    mm = -(E @ yc) - np.einsum("kaj,kj->ka", F, yp[op])
    mcc = float(-(mm * (r + 0.5 * mm)).sum())
    Kc = K4 - (yc[0:4] * sK if not o.fix_intrinsics else 0.0)
    extc = ext - yc[4:].reshape(nc, 6) * sC * (~cfix)[:, None]
    ptsc = pts - yp * sP
    cand = float(obs_costs(Kc, extc, ptsc, oc, op, uv, o.huber_delta).sum())
    return mcc, cand


# ---------------------------------------------------------------------------------------------------------------- scenes
def _args(sc):
    return sc["K0"], sc["ext0"], sc["pts0"], sc["obs_cam"], sc["obs_pt"], sc["obs_uv"]


def _sorted(oc, op, uv):
    order = np.lexsort((op, oc))
    return oc[order].astype(np.int32), op[order].astype(np.int32), np.ascontiguousarray(uv[order])


def _random_tracks(n_cam, n_pt, lengths, seed):
    """every point seen by lengths[p] random cameras of the ring scene"""
    sc = synth.ba_scene(n_cam, n_pt)
    rng = np.random.default_rng(seed)
    L = lengths(rng, n_pt) if callable(lengths) else np.full(n_pt, lengths)
    op = np.repeat(np.arange(n_pt), L)
    oc = np.concatenate([rng.choice(n_cam, size=l, replace=False) for l in L])
    uv = synth.project(synth.K_REF, sc["ext_true"][oc], sc["pts_true"][op]) + 0.5 * rng.standard_normal((len(op), 2))
    return (sc["K0"], sc["ext0"], sc["pts0"]) + _sorted(oc, op, uv)


def _once_and_twice():
    """point 0 seen once; point 1 seen twice, both times by camera 3"""
    sc = synth.ba_scene(12, 700)
    oc, op, uv = sc["obs_cam"], sc["obs_pt"], sc["obs_uv"]
    keep = np.ones(len(op), bool)
    keep[np.nonzero(op == 0)[0][1:]] = False
    keep[op == 1] = False
    two = synth.project(synth.K_REF, sc["ext_true"][[3, 3]], sc["pts_true"][[1, 1]]) + np.array([[0.3, -0.2], [-0.4, 0.1]])
    oc = np.concatenate([oc[keep], [3, 3]]); op = np.concatenate([op[keep], [1, 1]]); uv = np.concatenate([uv[keep], two])
    assert (op == 0).sum() == 1 and (op == 1).sum() == 2
    return (sc["K0"], sc["ext0"], sc["pts0"]) + _sorted(oc, op, uv)


def _far_points():
    """points 1e3 scene units from the cameras' ring (radius 10): next to no parallax, an ill-conditioned 3x3 point block"""
    sc = synth.ba_scene(16, 700)
    rng = np.random.default_rng(23)
    phi = rng.uniform(0, 2 * np.pi, 700)
    X = 1e3 * np.stack([np.sin(phi), rng.uniform(-0.1, 0.1, 700), -np.cos(phi)], axis=1)
    oc, op = [], []
    R = np.stack([synth.angle_axis_to_rotmat(e[:3]) for e in sc["ext_true"]])
    for p in range(700):
        q = R @ X[p] + sc["ext_true"][:, 3:]
        see = np.nonzero((q[:, 2] > 0) & (np.abs(q[:, 0]) < 0.6 * q[:, 2]) & (np.abs(q[:, 1]) < 0.45 * q[:, 2]))[0][:4]
        if len(see) >= 2:
            oc += list(see); op += [p] * len(see)
    oc = np.array(oc); op = np.array(op)
    ids, op = np.unique(op, return_inverse=True)
    assert len(ids) >= 500
    X = X[ids]
    uv = synth.project(synth.K_REF, sc["ext_true"][oc], X[op]) + 0.5 * rng.standard_normal((len(op), 2))
    pts0 = X * (1.0 + 1e-3 * rng.standard_normal((len(ids), 1))) + 0.05 * rng.standard_normal(X.shape)
    return (sc["K0"], sc["ext0"], pts0) + _sorted(oc, op, uv)


def _constants():
    sc = synth.ba_scene(12, 700)
    cam = np.zeros(12, np.uint8); cam[[2, 3, 9]] = 1
    pt = np.zeros(700, np.uint8); pt[::7] = 1; pt[300:320] = 1
    return _args(sc), cam, pt


# name -> (args, options, constant cameras, constant points)
def _scene(name):
    base = lambda: _args(synth.ba_scene(12, 700))
    if name.startswith("radius_"):
        return base(), dict(initial_trust_region_radius=float(name[7:])), None, None
    if name == "fix_intrinsics":
        return base(), dict(fix_intrinsics=1), None, None
    if name == "no_huber":
        return base(), dict(huber_delta=0.0), None, None
    if name == "free_first_camera":
        return base(), dict(fix_first_camera=0), None, None
    if name == "once_and_twice":
        return _once_and_twice(), {}, None, None
    if name == "tracks_of_10":
        return _random_tracks(12, 500, 10, 5), {}, None, None
    if name == "wide_blocks":
        return _random_tracks(64, 1500, lambda rng, n: rng.integers(2, 5, size=n), 11), {}, None, None
    if name == "constants":
        a, cam, pt = _constants()
        return a, {}, cam, pt
    if name == "constant_cameras":
        return _constants()[0], {}, _constants()[1], None
    if name == "constant_points":
        return _constants()[0], {}, None, _constants()[2]
    if name == "far_points":
        return _far_points(), {}, None, None
    raise KeyError(name)


SCENES = ["radius_1e-2", "radius_1e4", "radius_1e16", "fix_intrinsics", "no_huber", "free_first_camera", "once_and_twice",
          "tracks_of_10", "wide_blocks", "constants", "constant_cameras", "constant_points", "far_points"]

_ref_cache = {}


def _reference(ctx, name):
    """scene and reference values, computed once and shared by both values of the switch"""
    if name not in _ref_cache:
        args, kw, cam, pt = _scene(name)
        o = ctx.ba_options(**kw)
        _ref_cache[name] = (args, kw, cam, pt,
                            reference_step(args, o, o.initial_trust_region_radius, jacobi_scale(args, o), cam, pt))
    return _ref_cache[name]


def _create_ex(ctx, args, seam, cam, pt, **kw):
    if cam is None and pt is None:
        return _create(ctx, args, seam, **kw)

    class _Ex:      # _create calls ctx.ba_create(*args, opts=...): the constant flags ride along
        def ba_options(self, **k):
            return ctx.ba_options(**k)

        def ba_create(self, *a, opts=None):
            return ctx.ba_create(*a, opts=opts, cam_const=cam, pt_const=pt)
    return _create(_Ex(), args, seam, **kw)


def _rel(a, b):
    return abs(a - b) / abs(b)


def _check(name, seam, got, want):
    dm, dc = _rel(got[2], want[0]), _rel(got[3], want[1])
    print("model-cost-deviation %s seam=%s mcc %.3e cand %.3e (mcc %.17g cand %.17g)" % (name, seam, dm, dc, got[2], got[3]))
    assert want[0] > 0.0 and got[8] == 0.0
    assert dm <= MCC_TOL and dc <= CAND_TOL, (name, seam, dm, dc, MCC_TOL, CAND_TOL)


@pytest.mark.parametrize("seam", [None, 0])
@pytest.mark.parametrize("name", SCENES)
def test_first_step_scalars_follow_the_reference(ctx, name, seam):
    args, kw, cam, pt, want = _reference(ctx, name)
    pb = _create_ex(ctx, args, seam, cam, pt, **kw)
    if name == "wide_blocks":
        cr = pb.debug_table("blk_crange").reshape(-1, 2)
        assert (cr[:, 1] - cr[:, 0] >= 24).any(), cr[:4]       # a block leaves the staged camera window
    if name == "tracks_of_10":
        assert (np.bincount(args[4]) == 10).all()
    s = pb.iterate(1)
    got = pb.debug_table("step_scalars")
    pb.close()
    assert s["iterations"] == 1 and got.shape == (9,)
    _check(name, seam, got, want)


@pytest.mark.parametrize("seam", [None, 0])
def test_a_rejected_step_follows_the_reference(ctx, seam):
    """the rejecting scene of test_ba_seam_gpu: the first step LM rejects, from the parameters and the radius it was taken at"""
    args = _rejecting_scene()
    kw = dict(initial_trust_region_radius=1e6)
    o = ctx.ba_options(**kw)
    key = "rejecting"
    pb = _create(ctx, args, seam, **kw)
    radius, nsucc, found = o.initial_trust_region_radius, 0, None
    for _ in range(30):
        before = pb.params()
        s = pb.iterate(1)
        if s["successful_steps"] == nsucc:
            found = (before, radius, pb.debug_table("step_scalars"))
            break
        radius, nsucc = s["final_radius"], s["successful_steps"]
    pb.close()
    assert found is not None, "no step was rejected"
    before, radius, got = found
    if key not in _ref_cache:
        _ref_cache[key] = reference_step(tuple(before) + tuple(args[3:]), o, radius, jacobi_scale(args, o))
    _check(key, seam, got, _ref_cache[key])


def _trace_scene(name):
    if name == "rejecting":
        return _rejecting_scene(), dict(initial_trust_region_radius=1e6)
    return _args(synth.ba_scene(24, 4000)), {}


def thirty_iterations(ctx, name, seam):
    """accepted flags, radii, final cost and parameters of 30 forced iterations, one call each (also what wrote the golden file)"""
    args, kw = _trace_scene(name)
    pb = _create(ctx, args, seam, **kw)
    acc, rad, last = [], [], 0
    for _ in range(30):
        s = pb.iterate(1)
        acc.append(int(s["successful_steps"] > last)); rad.append(s["final_radius"]); last = s["successful_steps"]
    K, ext, pts = pb.params()
    pb.close()
    return dict(accepted=np.array(acc, np.int32), radius=np.array(rad, np.float64), cost=np.float64(s["final_cost"]), K=K, ext=ext, pts=pts)


@pytest.mark.parametrize("seam", [None, 0])
@pytest.mark.parametrize("name", ["ring_24_4000", "rejecting"])
def test_thirty_iterations_decide_as_before(ctx, name, seam):
    """every flag, radius, the final cost and the parameters equal what the kernels gave before (the golden file)"""
    got = thirty_iterations(ctx, name, seam)
    g = np.load(GOLDEN)
    want = {k: g[name + "." + k] for k in got}
    d = np.abs(got["radius"] / want["radius"] - 1.0)
    print("decisions %s seam=%s accepted %d of 30, radius equal in %d, largest relative difference %.3e, cost %.3e, K %.3e ext %.3e pts %.3e" % (
        name, seam, got["accepted"].sum(), (d == 0).sum(), d.max(), abs(got["cost"] - want["cost"]) / want["cost"],
        np.abs(got["K"] - want["K"]).max(), np.abs(got["ext"] - want["ext"]).max(), np.abs(got["pts"] - want["pts"]).max()))
    assert np.array_equal(got["accepted"], want["accepted"])
    if name == "rejecting":
        assert (got["accepted"] == 0).sum() >= 1
    assert np.array_equal(got["radius"], want["radius"]) and got["cost"] == want["cost"]
    for k in ("K", "ext", "pts"):
        assert np.array_equal(got[k], want[k])
