"""GPU: constant parameter blocks in bundle adjustment (sfmhip_ba_create_ex / _solve_ex / _solve_multi_ex), against the oracle
where it can express the problem and against the dense test-side reference (tests/ba_dense_ref.py, itself checked against the
oracle in test_ba_const_cpu.py) where it cannot.  Tolerances are those of tests/test_ba_gpu.py: reduced systems 1e-9 relative to
the largest entry and 1e-12 on the cost; after 6 forced steps 1e-8 relative on the cost and 1e-6 x scene scale on the parameters
(10: points / extrinsics, 3000: intrinsics); to convergence the same iteration count and termination and 1e-6 on the cost
(parameters are not compared there: they wander along the flat directions of the problem); several contexts 1e-9."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle as orc
from sfm_opencv_amd import _lib, api, synth
from ba_dense_ref import dense_ba, fixed_cost

pytestmark = pytest.mark.gpu

FREE = dict(max_num_iterations=6, function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0)


def _args(sc):
    return sc["K0"], sc["ext0"], sc["pts0"], sc["obs_cam"], sc["obs_pt"], sc["obs_uv"]


def _relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _cam_mask(n, idx):
    m = np.zeros(n, bool); m[list(idx)] = True
    return m


def _pt_mask(n, frac=0.3, seed=11):
    return np.random.default_rng(seed).random(n) < frac


def _orc_opts(o):
    return orc.ba_default_options(**{k: getattr(o, k) for k in ("fix_first_camera", "fix_intrinsics", "jacobi_scaling", "huber_delta")})


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _constants_kept(sc, out, cm, pm, fixK):
    """constant blocks come back bit for bit (the sign of a zero included)"""
    K, e, p = out[:3]
    assert np.array_equal(_bits(e[cm]), _bits(sc["ext0"][cm]))
    if pm is not None:
        assert np.array_equal(_bits(p[pm]), _bits(sc["pts0"][pm]))
    if fixK:
        assert np.array_equal(_bits(K), _bits(sc["K0"]))


def _check_forced(mine, ref):
    K, e, p, s = mine
    Ko, eo, po, so = ref[:4]
    assert s["iterations"] == so["iterations"] == 6
    assert s["successful_steps"] == so["successful_steps"]
    assert abs(s["final_cost"] - so["final_cost"]) <= 1e-8 * so["final_cost"]
    assert abs(s["initial_cost"] - so["initial_cost"]) <= 1e-12 * so["initial_cost"]
    assert np.abs(p - po).max() <= 1e-6 * 10.0
    assert np.abs(e - eo).max() <= 1e-6 * 10.0
    assert np.abs(K - Ko).max() <= 1e-6 * 3000.0


def _check_converged(mine, ref):
    s, so = mine[3], ref[3]
    assert s["termination"] == so["termination"]
    assert s["iterations"] == so["iterations"]
    assert abs(s["final_cost"] - so["final_cost"]) <= 1e-6 * so["final_cost"]


def _forced(ctx, sc, o, cm=None, pm=None, n=6):
    pb = ctx.ba_create(*_args(sc), opts=o, cam_const=cm, pt_const=pm)
    s = pb.iterate(n)
    K, e, p = pb.params()
    pb.close()
    return K, e, p, s


# ---------------------------------------------------------------------------------------------------------------- item 3
@pytest.mark.parametrize("jacobi", [1, 0])
@pytest.mark.parametrize("fixK", [0, 1])
def test_camera_mask_reduced_system_is_the_oracle_with_rows_deleted(ctx, jacobi, fixK):
    sc = synth.ba_scene(12, 700)
    nc = 12
    for idx in ([4], [0, 5, 9], [c for c in range(nc) if c != 7]):
        cm = _cam_mask(nc, idx)
        keep = np.concatenate([np.arange(6 * c, 6 * c + 6) for c in range(nc) if not cm[c]] + ([] if fixK else [6 * nc + np.arange(4)]))
        for radius in (1e4, 3.0):
            o = ctx.ba_options(fix_first_camera=0, jacobi_scaling=jacobi, fix_intrinsics=fixK)
            pb = ctx.ba_create(*_args(sc), opts=o, cam_const=cm)
            S, rhs, cost = pb.reduced_system(radius)
            pb.close()
            So, rhso, costo = orc.ba_reduced_system(*_args(sc), radius, opts=_orc_opts(o))
            So, rhso = So[np.ix_(keep, keep)], rhso[keep]
            assert S.shape == So.shape == (keep.size, keep.size)
            assert abs(cost - costo) <= 1e-12 * costo
            assert _relerr(S, So) <= 1e-9 and _relerr(rhs, rhso) <= 1e-9


# ---------------------------------------------------------------------------------------------------------------- item 4
def _subset(sc, sel):
    """the observations `sel`, their points renumbered to the points they observe"""
    op = sc["obs_pt"][sel]
    ids, inv = np.unique(op, return_inverse=True)
    return sc["K0"], sc["ext0"], sc["pts0"][ids], sc["obs_cam"][sel], inv.astype(np.int32), sc["obs_uv"][sel]


@pytest.mark.parametrize("r", [50.0, 3.0])
def test_point_mask_reduced_system_is_the_sum_of_two_oracle_systems(ctx, r):
    """free points' observations at -r plus the constant points' observations at -1e-20 (their Schur term vanishes, only the U part
    remains); cost and rhs add up the same way"""
    sc = synth.ba_scene(12, 700)
    pm = _pt_mask(700)
    o = ctx.ba_options(jacobi_scaling=0)
    pb = ctx.ba_create(*_args(sc), opts=o, pt_const=pm)
    S, rhs, cost = pb.reduced_system(-r)
    pb.close()
    oo = orc.ba_default_options(jacobi_scaling=0)
    free_obs = ~pm[sc["obs_pt"]]
    Sa, ra, ca = orc.ba_reduced_system(*_subset(sc, free_obs), -r, opts=oo)
    Sb, rb, cb = orc.ba_reduced_system(*_subset(sc, ~free_obs), -1e-20, opts=oo)
    So, rhso, costo = Sa + Sb, ra + rb, ca + cb
    assert abs(cost - costo) <= 1e-12 * costo
    assert _relerr(S, So) <= 1e-9 and _relerr(rhs, rhso) <= 1e-9


# ---------------------------------------------------------------------------------------------------------------- item 5
def test_constant_camera_k_follows_the_relabelled_oracle(ctx):
    k = 5
    for sc, f in ((synth.ba_scene(16, 1500), 6), (synth.ba_scene(12, 600), 0)):
        nc = sc["ext0"].shape[0]
        cm = _cam_mask(nc, [k])
        perm = np.arange(nc); perm[[0, k]] = perm[[k, 0]]
        swapped = (sc["K0"], sc["ext0"][perm], sc["pts0"], perm[sc["obs_cam"]].astype(np.int32), sc["obs_pt"], sc["obs_uv"])
        o = ctx.ba_options(fix_first_camera=0)
        if f:
            mine = _forced(ctx, sc, o, cm)
        else:
            mine = ctx.ba_solve(*_args(sc), opts=o, cam_const=cm)
        Ko, eo, po, so, _ = orc.ba_solve(*swapped, force_iterations=f)
        assert np.array_equal(mine[1][k], sc["ext0"][k])
        if f:
            _check_forced(mine, (Ko, eo[perm], po, so))
        else:
            _check_converged(mine, (Ko, eo[perm], po, so))


# ---------------------------------------------------------------------------------------------------------------- item 6
def _mixed_cases():
    return [
        ("cams+points", (8, 400), [0, 3, 6], 0.3, dict()),
        ("cams+points fixed K", (8, 400), [0, 3, 6], 0.3, dict(fix_intrinsics=1)),
        ("motion-only", (8, 400), [], 1.0, dict()),
        ("pnp", (1, 300), [], 1.0, dict(fix_first_camera=0, fix_intrinsics=1)),
        ("structure-only", (8, 400), list(range(8)), 0.0, dict(fix_intrinsics=1)),
        # constant cameras in the middle of the index range (renumbered internally), no constant point: 16 cameras for the indices,
        # 400 points like the cases above (what the dense reference costs grows with the cube of the point count)
        ("cams 4 9 10", (16, 400), [4, 9, 10], 0.0, dict()),
        ("cams 3 8 fixed K", (16, 400), [3, 8], 0.0, dict(fix_intrinsics=1)),
        ("cams 2 7 12 free first camera", (16, 400), [2, 7, 12], 0.0, dict(fix_first_camera=0)),
    ]


@pytest.mark.parametrize("name,shape,cams,frac,kw", _mixed_cases(), ids=[c[0] for c in _mixed_cases()])
def test_mixed_masks_follow_the_dense_reference(ctx, name, shape, cams, frac, kw):
    sc = synth.ba_scene(*shape)
    nc, npt = shape
    cm = _cam_mask(nc, cams)
    pm = _pt_mask(npt, frac) if frac < 1.0 else np.ones(npt, bool)
    o = ctx.ba_options(**kw)
    oo = _orc_opts(o)
    cfix = cm | (np.arange(nc) == 0) if o.fix_first_camera else cm
    mine = _forced(ctx, sc, o, cm, pm)
    ref = dense_ba(*_args(sc), opts=oo, cam_const=cm, pt_const=pm, force_iterations=6)
    _constants_kept(sc, mine, cfix, pm, o.fix_intrinsics)
    if name == "structure-only":
        pb = ctx.ba_create(*_args(sc), opts=o, cam_const=cm, pt_const=pm)
        assert pb.reduced_system(1e4)[0].shape == (0, 0)             # n = 0
        pb.close()
    _check_forced(mine, ref)
    conv = ctx.ba_solve(*_args(sc), opts=o, cam_const=cm, pt_const=pm)
    _constants_kept(sc, conv, cfix, pm, o.fix_intrinsics)
    _check_converged(conv, dense_ba(*_args(sc), opts=oo, cam_const=cm, pt_const=pm))
    if o.fix_intrinsics:
        # the fixed cost: 1/2 sum rho over the fully constant observations (orc.reprojection_errors), in both reported costs
        dead = cfix[sc["obs_cam"]] & pm[sc["obs_pt"]]
        fc = fixed_cost(*_args(sc), cfix, pm) if dead.any() else 0.0
        assert mine[3]["num_residuals"] == 2 * sc["n_obs"]
        if dead.any():
            # without the fully constant observations: the same trajectory, the cost net of the fixed part
            keep = ~dead
            sub = (sc["K0"], sc["ext0"], sc["pts0"], sc["obs_cam"][keep], sc["obs_pt"][keep], sc["obs_uv"][keep])
            pb = ctx.ba_create(*sub, opts=o, cam_const=cm, pt_const=pm)
            s2 = pb.iterate(6)
            K2, e2, p2 = pb.params()
            pb.close()
            # the library's own fixed cost, against 1/2 sum rho from orc.reprojection_errors: the two runs differ by exactly that part
            assert abs(mine[3]["initial_cost"] - s2["initial_cost"] - fc) <= 1e-12 * fc
            assert abs(mine[3]["final_cost"] - s2["final_cost"] - fc) <= 1e-12 * fc
            for a, b in (("initial_cost", "initial_cost"), ("final_cost", "final_cost")):
                assert abs((mine[3][a] - fc) - s2[b]) <= 1e-12 * s2[b]
                assert abs(mine[3][a] - ref[3][a]) <= (1e-12 if a == "initial_cost" else 1e-8) * ref[3][a]
            assert np.array_equal(e2, mine[1]) and np.array_equal(p2, mine[2])


def test_nothing_free_returns_convergence_at_the_fixed_cost(ctx):
    sc = synth.ba_scene(6, 200)
    o = ctx.ba_options(fix_intrinsics=1)
    cm = np.ones(6, bool); pm = np.ones(200, bool)
    K, e, p, s = ctx.ba_solve(*_args(sc), opts=o, cam_const=cm, pt_const=pm)
    fc = fixed_cost(*_args(sc), cm, pm)
    assert s["termination"] == 0 and s["iterations"] == 0 and s["initial_cost"] == s["final_cost"]
    assert abs(s["final_cost"] - fc) <= 1e-12 * fc
    assert np.array_equal(K, sc["K0"]) and np.array_equal(e, sc["ext0"]) and np.array_equal(p, sc["pts0"])


# ---------------------------------------------------------------------------------------------------------------- item 7
def _solve_ex_raw(ctx, sc, o, cm, pm):
    """sfmhip_ba_solve_ex straight through ctypes (NULL masks where None)"""
    K4 = sc["K0"].copy(); ext = sc["ext0"].copy(); pts = sc["pts0"].copy()
    oc, op, uv = sc["obs_cam"], sc["obs_pt"], sc["obs_uv"]
    s = _lib.BASummary()
    ptr = lambda a: None if a is None else np.ascontiguousarray(a, np.uint8).ctypes.data
    cma = None if cm is None else np.ascontiguousarray(cm, np.uint8)
    pma = None if pm is None else np.ascontiguousarray(pm, np.uint8)
    ctx._check(ctx.lib.sfmhip_ba_solve_ex(ctx.h, K4.ctypes.data, ext.ctypes.data, ext.shape[0], pts.ctypes.data, pts.shape[0],
                                          oc.ctypes.data, op.ctypes.data, uv.ctypes.data, oc.shape[0], ptr(cma), ptr(pma),
                                          C.byref(o), C.byref(s)))
    return K4, ext, pts, s.asdict()


def _same_bits(a, b):
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x, y)
    for key in ("termination", "iterations", "successful_steps", "initial_cost", "final_cost", "num_residuals", "final_gradient_max_norm"):
        assert a[3][key] == b[3][key], key


def test_null_and_zero_masks_and_camera_zero_mask_equal_the_legacy_call(ctx):
    sc = synth.ba_scene(12, 700)
    o = ctx.ba_options()
    legacy = ctx.ba_solve(*_args(sc), opts=o)
    _same_bits(_solve_ex_raw(ctx, sc, o, None, None), legacy)
    _same_bits(ctx.ba_solve(*_args(sc), opts=o, cam_const=np.zeros(12, bool), pt_const=np.zeros(700, bool)), legacy)
    o0 = ctx.ba_options(fix_first_camera=0)
    _same_bits(ctx.ba_solve(*_args(sc), opts=o0, cam_const=_cam_mask(12, [0])), legacy)
    # resident form too: forced steps
    _same_bits(_forced(ctx, sc, o0, _cam_mask(12, [0])), _forced(ctx, sc, o))


def test_masked_reruns_are_bitwise_identical_and_seam_on_off_agree(ctx):
    sc = synth.ba_scene(12, 700)
    cm = _cam_mask(12, [2, 7]); pm = _pt_mask(700)
    o = ctx.ba_options()
    a = ctx.ba_solve(*_args(sc), opts=o, cam_const=cm, pt_const=pm)
    b = ctx.ba_solve(*_args(sc), opts=o, cam_const=cm, pt_const=pm)
    _same_bits(a, b)
    _constants_kept(sc, a, cm | (np.arange(12) == 0), pm, False)
    old = os.environ.get("SFMHIP_BA_SEAM")
    try:
        outs = []
        for seam in ("4", "0"):
            os.environ["SFMHIP_BA_SEAM"] = seam
            outs.append(_forced(ctx, sc, o, cm, pm, n=8))
    finally:
        if old is None:
            os.environ.pop("SFMHIP_BA_SEAM", None)
        else:
            os.environ["SFMHIP_BA_SEAM"] = old
    _same_bits(outs[0], outs[1])


def test_solvers_agree_with_masks(ctx):
    sc = synth.ba_scene(16, 1500)
    cm = _cam_mask(16, [3, 9]); pm = _pt_mask(1500)
    outs = [_forced(ctx, sc, ctx.ba_options(solver=sol), cm, pm) for sol in (0, 1)]
    for K, e, p, s in outs[1:]:
        assert np.abs(K - outs[0][0]).max() <= 1e-10 * np.abs(outs[0][0]).max()
        assert np.abs(e - outs[0][1]).max() <= 1e-10 and np.abs(p - outs[0][2]).max() <= 1e-10
        _constants_kept(sc, (K, e, p), cm | (np.arange(16) == 0), pm, False)


def test_chain_solver_with_constant_cameras_inside_the_chain(ctx, capfd):
    sc = synth.ba_scene(20, 1200, max_len=4)
    cm = _cam_mask(20, [6, 13])           # constant cameras inside the chain: 17 free cameras, band <= 3
    pm = _pt_mask(1200)
    outs = []
    for sol in (0, 1):
        o = ctx.ba_options(solver=sol, verbose=1)
        capfd.readouterr()
        outs.append(_forced(ctx, sc, o, cm, pm))
        C.CDLL(None).fflush(None)             # the library's printf buffer, when stdout is not a terminal
        txt = capfd.readouterr().out
        assert ("chain (fronts in LDS)" in txt) == (sol == 0), txt
        assert "17 free cameras" in txt
    a, b = outs
    assert np.abs(a[1] - b[1]).max() <= 1e-10 and np.abs(a[2] - b[2]).max() <= 1e-10 and np.abs(a[0] - b[0]).max() <= 1e-10 * np.abs(b[0]).max()
    _constants_kept(sc, a, cm | (np.arange(20) == 0), pm, False)


# ---------------------------------------------------------------------------------------------------------------- item 8
@pytest.mark.parametrize("n_ctx", [2, 3])
@pytest.mark.parametrize("case", ["cams+points", "cams+points fixed K", "motion-only 14 cams", "structure-only", "pnp"])
def test_multi_context_with_masks_follows_the_single_context_steps(ctx, n_ctx, case):
    if case == "motion-only 14 cams":
        # band 0 with >= 12 free cameras and free intrinsics: without the gate this would take the chain solver under the hook
        sc = synth.ba_scene(14, 2000); cm = np.zeros(14, bool); pm = np.ones(2000, bool); kw = {}
    elif case == "structure-only":
        # every camera constant, intrinsics fixed: n = 0 under the hook (the packed message and the plan of an empty reduced system)
        sc = synth.ba_scene(24, 4000); cm = np.ones(24, bool); pm = np.zeros(4000, bool); kw = dict(fix_intrinsics=1)
    elif case == "pnp":
        # one free camera, every point constant, intrinsics fixed: every point shards to rank 0, the other ranks hold nothing
        sc = synth.ba_scene(1, 600); cm = np.zeros(1, bool); pm = np.ones(600, bool); kw = dict(fix_first_camera=0, fix_intrinsics=1)
    else:
        sc = synth.ba_scene(24, 4000); cm = _cam_mask(24, [0, 5, 11, 17]); pm = _pt_mask(4000)
        kw = dict(fix_intrinsics=1) if "fixed K" in case else {}
    o = ctx.ba_options(**FREE, **kw)
    Kr, er, pr, sr = ctx.ba_solve(*_args(sc), opts=o, cam_const=cm, pt_const=pm)
    ctxs = [api.Context(0, use_torch_stream=False) for _ in range(n_ctx)]
    try:
        K, e, p, s = api.ba_solve_multi(ctxs, *_args(sc), opts=o, cam_const=cm, pt_const=pm)
    finally:
        for c in ctxs:
            c.close()
    assert sr["iterations"] == s["iterations"] == 6 and s["successful_steps"] == sr["successful_steps"]
    assert abs(s["initial_cost"] - sr["initial_cost"]) <= 1e-9 * sr["initial_cost"]
    assert abs(s["final_cost"] - sr["final_cost"]) <= 1e-9 * sr["final_cost"]
    assert _relerr(e, er) <= 1e-9 and _relerr(K, Kr) <= 1e-9 and _relerr(p, pr) <= 1e-9
    _constants_kept(sc, (K, e, p), cm | (np.arange(cm.size) == 0) if o.fix_first_camera else cm, pm, o.fix_intrinsics)


def _resident_shards(sc, o_kw, pm, world, script):
    """The multi-process path in one process: `world` contexts, each creates its point shard with sfmhip_ba_create_ex (its own shard's
    pt_const) and installs an all-reduce hook that sums the ranks' buffers; `script(pb)` runs on every rank in its own thread.
    Returns (script results, point ids, hook call counts) per rank."""
    import threading
    import torch
    from sfm_opencv_amd import dist as sdist
    ctxs = [api.Context(0, use_torch_stream=False) for _ in range(world)]
    probs, ids = [], []
    for r in range(world):
        pts_l, oc, op, uv, pid = sdist.shard_points(sc["obs_cam"], sc["obs_pt"], sc["obs_uv"], sc["pts0"], r, world)
        probs.append(ctxs[r].ba_create(sc["K0"], sc["ext0"], pts_l, oc, op, uv, opts=ctxs[r].ba_options(**o_kw), pt_const=pm[pid]))
        ids.append(pid)
    bar = threading.Barrier(world)
    slots = [None] * world
    counts = [[] for _ in range(world)]

    def make_hook(r):
        def hook(ptr, count, stream):
            ctxs[r].synchronize()
            slots[r] = torch.as_tensor(sdist._CudaView(ptr, count), device="cuda")
            counts[r].append(count)
            bar.wait()
            if r == 0:
                assert len({s.numel() for s in slots}) == 1, [s.numel() for s in slots]     # one collective, one size on every rank
                total = slots[0].clone()
                for q in range(1, world):
                    total += slots[q]
                for q in range(world):
                    slots[q].copy_(total)
                torch.cuda.synchronize()
            bar.wait()
            return 0
        return hook

    out, errs = [None] * world, []

    def run(r):
        try:
            probs[r].set_allreduce(make_hook(r), r, world)
            out[r] = script(probs[r])
        except Exception as e:                                      # pragma: no cover
            errs.append(e); bar.abort()

    th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in th: t.start()
    for t in th: t.join(180)
    assert not errs and all(x is not None for x in out), errs
    for pb in probs: pb.close()
    for c in ctxs: c.close()
    return out, ids, counts


def test_resident_shards_agree_when_only_one_holds_constant_points(ctx, capfd):
    """create_ex + set_allreduce per rank, the constant points all in rank 0's shard (rank 1's own masks are those of a legacy
    problem): both ranks make the same collectives, neither takes the chain solver (a narrow band the chain solver would take
    unmasked), and the steps follow the single-context run"""
    from sfm_opencv_amd import dist as sdist
    sc = synth.ba_scene(24, 4000, max_len=4)
    ids0 = sdist.shard_points(sc["obs_cam"], sc["obs_pt"], sc["obs_uv"], sc["pts0"], 0, 2)[4]
    pm = np.zeros(4000, bool); pm[ids0[::3]] = True
    kw = dict(verbose=1)

    def script(pb):
        s = pb.iterate(5)
        return s, pb.params()
    capfd.readouterr()
    out, ids, counts = _resident_shards(sc, kw, pm, 2, script)
    C.CDLL(None).fflush(None)
    txt = capfd.readouterr().out
    assert "reduced system" in txt and "chain (fronts in LDS)" not in txt, txt
    assert counts[0] == counts[1]
    ref = _forced(ctx, sc, ctx.ba_options(), None, pm, n=5)
    for r in range(2):
        s, (K, e, p) = out[r]
        assert s["iterations"] == ref[3]["iterations"] == 5 and s["successful_steps"] == ref[3]["successful_steps"]
        assert abs(s["final_cost"] - ref[3]["final_cost"]) <= 1e-9 * ref[3]["final_cost"]
        assert _relerr(e, ref[1]) <= 1e-9 and _relerr(K, ref[0]) <= 1e-9 and _relerr(p, ref[2][ids[r]]) <= 1e-9
        assert np.array_equal(_bits(p[pm[ids[r]]]), _bits(sc["pts0"][ids[r]][pm[ids[r]]]))


def test_resident_shards_run_again_after_reset(ctx):
    """a hooked masked problem run to convergence, reset and run again: the same result bit for bit on every rank, and the
    convergence of the single-context run (the tolerance tests see the same |x| over the free parameters each time)"""
    sc = synth.ba_scene(24, 4000)
    pm = _pt_mask(4000)

    def script(pb):
        a = pb.run(); pa = pb.params()
        pb.reset()
        b = pb.run(); pbb = pb.params()
        return a, pa, b, pbb
    out, ids, counts = _resident_shards(sc, {}, pm, 2, script)
    ref = ctx.ba_solve(*_args(sc), pt_const=pm)
    for r in range(2):
        a, pa, b, pbb = out[r]
        for key in ("termination", "iterations", "successful_steps", "final_cost", "initial_cost"):
            assert a[key] == b[key], key
        for x, y in zip(pa, pbb):
            assert np.array_equal(_bits(x), _bits(y))
        assert a["termination"] == ref[3]["termination"] and a["iterations"] == ref[3]["iterations"]
        assert abs(a["final_cost"] - ref[3]["final_cost"]) <= 1e-6 * ref[3]["final_cost"]


# ---------------------------------------------------------------------------------------------------------------- item 9
def test_windowed_ba_on_the_c4_scene(ctx):
    cfg = synth.CONFIGS["C4"]
    sc = synth.ba_scene_mt(cfg["n_img"], cfg["n_pt"])
    nc, npt = sc["ext0"].shape[0], sc["pts0"].shape[0]
    cm = np.arange(nc) < nc - 20                      # the last 20 cameras free
    seen_free = np.zeros(npt, bool); seen_free[sc["obs_pt"][~cm[sc["obs_cam"]]]] = True
    pm = ~seen_free                                    # points seen by no free camera: constant
    o = ctx.ba_options(fix_intrinsics=1)
    a = ctx.ba_solve(*_args(sc), opts=o, cam_const=cm, pt_const=pm)
    b = ctx.ba_solve(*_args(sc), opts=o, cam_const=cm, pt_const=pm)
    assert a[3]["termination"] != 2
    assert a[3]["final_cost"] < a[3]["initial_cost"]
    _constants_kept(sc, a, cm, pm, True)
    _same_bits(a, b)
