"""GPU: sfmhip_select_views against the numpy restatement of its definition (tests/select_ref.py), fed with the library's own geometry
arrays: every output is equal in every bit, on the smallest scenes at which each part of the unit can still go wrong.  Then the entry
forms, determinism, the argument rules, an injected allocation failure, and the layers above (api.dense_cloud_for_all with and without
observations, and the C++ mirror)."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import dense_ref as dr
import select_ref as sr
from sfm_opencv_amd import _lib, api, synth

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("shared", "score", "sources", "n_scored", "wrange", "n_depth")
COS2_1DEG = sr.cos2_of(1.0)


def _same(a, b):
    a = np.asarray(a); b = np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _raw(ctx, ext_a, pts_a, oc_a, op_a, n_src_a, cos2_a, **over):
    """sfmhip_select_views straight through ctypes into outputs that hold a sentinel: (rc, dict of outputs, outputs untouched)"""
    ext = np.ascontiguousarray(ext_a, np.float64).reshape(-1, 6); pts = np.ascontiguousarray(pts_a, np.float64).reshape(-1, 3)
    oc = np.ascontiguousarray(oc_a, np.int32).ravel(); op = np.ascontiguousarray(op_a, np.int32).ravel()
    n = len(ext)
    a = dict(ext=ext.ctypes.data, n_views=n, pts=pts.ctypes.data if len(pts) else None, n_pt=len(pts), oc=oc.ctypes.data if len(oc) else None,
             op=op.ctypes.data if len(op) else None, n_obs=len(oc), cos2=cos2_a, n_src=n_src_a, want=NAMES)
    a.update(over)
    k = max(int(a["n_src"]), 1)
    out = dict(shared=np.full((n, n), -7, np.int32), score=np.full((n, n), -7, np.int32), sources=np.full((n, k), -7, np.int32), n_scored=np.full(n, -7, np.int32),
               wrange=np.full((n, 2), -7.0), n_depth=np.full(n, -7, np.int32))
    rc = ctx.lib.sfmhip_select_views(ctx.h, a["ext"], a["n_views"], a["pts"], a["n_pt"], a["oc"], a["op"], a["n_obs"], a["cos2"], a["n_src"],
                                     *[out[name].ctypes.data if name in a["want"] else None for name in NAMES])
    return rc, out, all((out[name] == -7).all() for name in NAMES)


def _check(ctx, ext, pts, oc, op, n_src, cos2=COS2_1DEG):
    rc, got, _ = _raw(ctx, ext, pts, oc, op, n_src, cos2)
    assert rc == 0, ctx.lib.sfmhip_last_error(ctx.h)
    exp = sr.select_views(ext, pts, oc, op, n_src, cos2, api.sweep_geometry)
    for name in NAMES:
        assert _same(got[name], exp[name]), (name, got[name], exp[name])
    return exp


# ------------------------------------------------------------------------------------------------ the scenes
def _ring(n_cam, n_pt, **kw):
    sc = synth.ba_scene(n_cam, n_pt, **kw)
    return sc["ext_true"], sc["pts_true"], sc["obs_cam"], sc["obs_pt"]


def _two_views_one_point():
    return np.array([[0, 0, 0, 0, 0, 0], [0, 0.02, 0, -1.0, 0, 0]], float), np.array([[0.2, 0.1, 5.0]]), [0, 1], [0, 0]


def _decoy():
    return sr.decoy_scene()[1:]


def _track_longer_than_a_wave():
    ext, pts, _, _ = _ring(70, 40)
    return ext, pts, np.repeat(np.arange(70), 40), np.tile(np.arange(40), 70)


def _one_hot_counter():
    rng = np.random.default_rng(4)
    n = 20000
    pts = np.stack([rng.uniform(-3, 3, n), rng.uniform(-2, 2, n), rng.uniform(4, 9, n)], 1)
    ext = np.array([[0, 0, 0, 0, 0, 0], [0.0, -0.05, 0.0, -0.6, 0, 0]], float)
    return ext, pts, np.repeat([0, 1], n), np.tile(np.arange(n), 2)


def _unseen_and_once_seen_views():
    ext, pts, oc, op = _ring(6, 100)
    keep = oc != 2
    four = np.nonzero(oc == 4)[0]
    keep[four[1:]] = False
    assert (oc[keep] == 2).sum() == 0 and (oc[keep] == 4).sum() == 1
    return ext, pts, oc[keep], op[keep]


def _ties():
    """four views on a square around a fifth that sees nothing, all looking along z; the points lie on the axis of symmetry, so the scores of
    the four are equal in pairs and the centre distances of the fifth are all equal"""
    cen = np.array([[1.0, 0, 0], [0, 1.0, 0], [-1.0, 0, 0], [0, -1.0, 0], [0, 0, 0]])
    ext = np.concatenate([np.zeros((5, 3)), -cen], 1)
    pts = np.array([[0, 0, 4.0], [0, 0, 5.0], [0, 0, 6.0]])
    return ext, pts, np.repeat(np.arange(4), 3), np.tile(np.arange(3), 4)


def _repeats_bad_points_and_a_point_behind():
    ext, pts, oc, op = _ring(6, 60, seed=11)
    pts = pts.copy()
    pts[3, 1] = np.nan; pts[7, 0] = np.inf
    pts[11] = 40.0 * pts[11] / np.linalg.norm(pts[11])
    return ext, pts, np.concatenate([oc, [0, 5, 2], oc[:25], [0, 5, 2]]), np.concatenate([op, [11, 11, 11], op[:25], [11, 11, 11]])


SCENES = {
    "two views, one point": (_two_views_one_point, 1),
    "decoy": (_decoy, 2),
    "ring 12 x 400": (lambda: _ring(12, 400), 2),
    "ring 30 x 3000, more than one sort tile": (lambda: _ring(30, 3000), 3),
    "track longer than a wave": (_track_longer_than_a_wave, 2),
    "65 views": (lambda: _ring(65, 500), 2),
    "130 views": (lambda: _ring(130, 800), 4),
    "every add on one counter": (_one_hot_counter, 1),
    "eight sources of nine views": (lambda: _ring(9, 200), 8),
    "a view unseen and a view seen once": (_unseen_and_once_seen_views, 3),
    "ties": (_ties, 3),
    "repeats, bad points, a point behind": (_repeats_bad_points_and_a_point_behind, 2),
}


@pytest.mark.parametrize("name", list(SCENES))
def test_scene_equals_the_restatement(ctx, name):
    build, n_src = SCENES[name]
    ext, pts, oc, op = build()
    exp = _check(ctx, ext, pts, oc, op, n_src)
    if name == "ring 30 x 3000, more than one sort tile":
        assert len(oc) > 2 * 4096
    if name == "track longer than a wave":
        off = ~np.eye(70, dtype=bool)
        assert (exp["shared"][off] == 40).all() and (exp["n_depth"] == 40).all()
    if name == "every add on one counter":
        assert exp["shared"][0, 1] == 20000 and 0 < exp["score"][0, 1] <= 20000
    if name == "a view unseen and a view seen once":
        assert exp["n_depth"][2] == 0 and exp["n_depth"][4] == 1 and (exp["wrange"][[2, 4]] == 0).all() and exp["n_scored"][2] == 0
        assert (exp["n_scored"] < 3).any() and (exp["wrange"][0] > 0).all()
    if name == "ties":
        assert exp["sources"][4].tolist() == [0, 1, 2] and exp["n_scored"].tolist() == [3, 3, 3, 3, 0]
        assert exp["sources"][0].tolist() == [1, 2, 3] and exp["score"][0, 1] == exp["score"][0, 3] == 3
    if name == "repeats, bad points, a point behind":
        assert (exp["score"] < exp["shared"]).any()
    if name == "decoy":
        assert all(4 not in exp["sources"][i] for i in range(4))


@pytest.mark.parametrize("cos2", [0.0, 1.0])
def test_the_ends_of_the_angle_rule(ctx, cos2):
    ext, pts, oc, op = _ring(12, 400)
    exp = _check(ctx, ext, pts, oc, op, 2, cos2)
    if cos2 == 1.0:
        assert _same(exp["score"], exp["shared"])                        # every pair in front of both views counts
    else:
        assert (exp["score"] <= exp["shared"]).all() and 0 < exp["score"].sum() < exp["shared"].sum()   # only rays past a right angle count


# ------------------------------------------------------------------------------------------------ entry forms, determinism
@pytest.fixture(scope="module")
def ring():
    ext, pts, oc, op = _ring(30, 3000)
    return ext, pts, oc, op, sr.select_views(ext, pts, oc, op, 3, COS2_1DEG, api.sweep_geometry)


def test_two_runs_give_the_same_bytes(ctx, ring):
    ext, pts, oc, op, exp = ring
    a = ctx.select_views(ext, pts, oc, op, 3, 1.0); b = ctx.select_views(ext, pts, oc, op, 3, 1.0)
    assert all(_same(x, y) for x, y in zip(a, b)) and all(_same(getattr(a, n), exp[n]) for n in NAMES)


def test_dev_form_on_resident_arrays_equals_the_host_form(ctx, ring):
    import torch
    ext, pts, oc, op, exp = ring
    dev = torch.device("cuda", ctx.device)
    n = len(ext)
    # two observations with an index out of range: the _dev form ignores them
    oc2 = np.concatenate([oc, [n, 0]]).astype(np.int32); op2 = np.concatenate([op, [0, len(pts)]]).astype(np.int32)
    d_pts = torch.from_numpy(np.ascontiguousarray(pts)).to(dev); d_oc = torch.from_numpy(oc2).to(dev); d_op = torch.from_numpy(op2).to(dev)
    out = dict(shared=torch.full((n, n), -7, dtype=torch.int32, device=dev), score=torch.full((n, n), -7, dtype=torch.int32, device=dev),
               sources=torch.full((n, 3), -7, dtype=torch.int32, device=dev), n_scored=torch.full((n,), -7, dtype=torch.int32, device=dev),
               wrange=torch.full((n, 2), -7.0, dtype=torch.float64, device=dev), n_depth=torch.full((n,), -7, dtype=torch.int32, device=dev))
    torch.cuda.synchronize(dev)
    ctx.select_views_dev(ext, d_pts, len(pts), d_oc, d_op, len(oc2), 3, 1.0, *[out[name] for name in NAMES])
    ctx.synchronize()
    for name in NAMES:
        assert _same(out[name].cpu().numpy(), exp[name]), name
    # any output may be left out
    only = torch.full((n, 3), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    ctx.select_views_dev(ext, d_pts, len(pts), d_oc, d_op, len(oc2), 3, 1.0, d_sources=only)
    ctx.synchronize()
    assert _same(only.cpu().numpy(), exp["sources"])
    rc, got, _ = _raw(ctx, ext, pts, oc, op, 3, COS2_1DEG, want=("wrange", "n_scored"))
    assert rc == 0 and _same(got["wrange"], exp["wrange"]) and _same(got["n_scored"], exp["n_scored"]) and (got["shared"] == -7).all()


def test_no_observation_is_no_error(ctx):
    ext = _ring(5, 10)[0]
    exp = _check(ctx, ext, np.zeros((0, 3)), [], [], 2)
    assert (exp["shared"] == 0).all() and (exp["wrange"] == 0).all() and (exp["n_scored"] == 0).all()
    _check(ctx, ext, np.ones((3, 3)), [], [], 2)


# ------------------------------------------------------------------------------------------------ errors
def test_bad_arguments_leave_the_outputs_alone(ctx):
    ext, pts, oc, op = _ring(6, 50)
    assert _raw(ctx, ext, pts, oc, op, 2, COS2_1DEG)[0::2] == (0, False)
    bad_ext = ext.copy(); bad_ext[3, 4] = np.nan
    inf_ext = ext.copy(); inf_ext[2, 0] = np.inf
    neg = oc.copy(); neg[5] = -1
    high = oc.copy(); high[7] = 6
    pneg = op.copy(); pneg[0] = -1
    phigh = op.copy(); phigh[9] = 50
    many = np.zeros((4097, 6)); many[:, 3] = np.arange(4097)
    cases = [dict(ext=None), dict(pts=None), dict(oc=None), dict(op=None), dict(n_views=1), dict(n_src=0), dict(n_src=6), dict(n_src=9), dict(cos2=-0.1),
             dict(cos2=1.5), dict(cos2=float("nan")), dict(cos2=float("inf")), dict(n_pt=-1), dict(n_obs=-1), dict(ext=bad_ext.ctypes.data),
             dict(ext=inf_ext.ctypes.data), dict(oc=neg.ctypes.data), dict(oc=high.ctypes.data), dict(op=pneg.ctypes.data), dict(op=phigh.ctypes.data),
             dict(n_pt=49), dict(ext=many.ctypes.data, n_views=4097)]
    for over in cases:
        assert _raw(ctx, ext, pts, oc, op, 2, COS2_1DEG, **over)[0::2] == (_lib.E_ARG, True), over
    assert ctx.lib.sfmhip_select_views(None, ext.ctypes.data, 6, pts.ctypes.data, 50, oc.ctypes.data, op.ctypes.data, len(oc), COS2_1DEG, 2, *([None] * 6)) == _lib.E_ARG
    assert _raw(ctx, ext[:3], pts, oc % 3, op, 8, COS2_1DEG)[0::2] == (_lib.E_ARG, True)       # n_src above n_views - 1
    with pytest.raises(ValueError):
        ctx.select_views(ext, pts, oc, op, 2, min_angle_deg=91.0)
    assert _raw(ctx, ext, pts, oc, op, 2, COS2_1DEG)[0] == 0


def test_a_failed_allocation_is_an_error_and_the_next_call_works(ctx, ring):
    import torch
    ext, pts, oc, op, exp = ring
    for failing in (1, 2):                                                # the host form's first block, its arrays
        assert ctx.lib.sfmhip_debug_fail_allocations(ctx.h, failing) == 0
        for _ in range(failing):
            rc, _, untouched = _raw(ctx, ext, pts, oc, op, 3, COS2_1DEG)
            assert rc == _lib.E_HIP and untouched
        rc, got, _ = _raw(ctx, ext, pts, oc, op, 3, COS2_1DEG)
        assert rc == 0 and all(_same(got[n], exp[n]) for n in NAMES)
    # the _dev form's only block, the unit's temporaries: nothing has been enqueued when it fails
    dev = torch.device("cuda", ctx.device)
    d_pts = torch.from_numpy(np.ascontiguousarray(pts)).to(dev); d_oc = torch.from_numpy(oc).to(dev); d_op = torch.from_numpy(op).to(dev)
    d_src = torch.full((len(ext), 3), -7, dtype=torch.int32, device=dev); d_w = torch.full((len(ext), 2), -7.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    assert ctx.lib.sfmhip_debug_fail_allocations(ctx.h, 1) == 0
    with pytest.raises(api.SfmHipError):
        ctx.select_views_dev(ext, d_pts, len(pts), d_oc, d_op, len(oc), 3, 1.0, d_sources=d_src, d_wrange=d_w)
    ctx.synchronize()
    assert (d_src == -7).all().item() and (d_w == -7.0).all().item()
    ctx.select_views_dev(ext, d_pts, len(pts), d_oc, d_op, len(oc), 3, 1.0, d_sources=d_src, d_wrange=d_w)
    ctx.synchronize()
    assert _same(d_src.cpu().numpy(), exp["sources"]) and _same(d_w.cpu().numpy(), exp["wrange"])


# ------------------------------------------------------------------------------------------------ the layers above
@pytest.fixture(scope="module")
def decoy_dense():
    sc, ext, pts, oc, op = sr.decoy_scene(decoy_points=6)
    return sc, ext, pts, oc, op, [sc.render(v)[0] for v in range(5)]


def test_dense_cloud_with_observations_equals_the_chain_on_ranked_sources(ctx, decoy_dense):
    sc, ext, pts, oc, op, images = decoy_dense
    sel = sr.select_views(ext, pts, oc, op, 2, COS2_1DEG, api.sweep_geometry)
    assert all(4 not in sel["sources"][i] for i in range(4)) and sel["n_depth"][4] == 6
    exp = sr.chain_with_ranges(images, sc.K4, ext, sel["sources"], sel["wrange"], api.sweep_geometry, 32, 2, 1, -1.0, 0.01, 2)
    xyz, bgr = api.dense_cloud_for_all(images, sc.K4, ext, sparse_pts=pts, n_src=2, planes=32, radius=2, min_score=-1.0, rel_tol=0.01, min_consistent=2, ctx=ctx,
                                       observations=(oc, op))
    assert _same(xyz, np.concatenate([e["xyz"] for e in exp])) and _same(bgr, np.concatenate([e["bgr"] for e in exp]))
    kept = [int(e["keep"].sum()) for e in exp]
    assert all(k > 0.3 * sc.ROWS * sc.COLS for k in kept[:4]), kept
    # an explicit range still wins, and a view that sees fewer than two points raises as it does today
    exp2 = dr.chain(images, sc.K4, ext, [list(r) for r in sel["sources"]], api.sweep_geometry, 16, 0.12, 0.32, 2, 1, -1.0, 0.01, 2)
    xyz2, _ = api.dense_cloud_for_all(images, sc.K4, ext, sparse_pts=pts, n_src=2, planes=16, radius=2, wmin=0.12, wmax=0.32, min_score=-1.0, rel_tol=0.01,
                                      min_consistent=2, ctx=ctx, observations=(oc, op))
    assert _same(xyz2, np.concatenate([e["xyz"] for e in exp2]))
    few = oc != 4
    with pytest.raises(ValueError, match="fewer than two sparse points"):
        api.dense_cloud_for_all(images, sc.K4, ext, sparse_pts=pts, n_src=2, planes=16, ctx=ctx, observations=(oc[few], op[few]))


def test_dense_cloud_without_observations_is_what_it_was(ctx, decoy_dense):
    sc, ext, pts, oc, op, images = decoy_dense
    exp = dr.chain(images, sc.K4, ext, dr.nearest_sources(ext, 2), api.sweep_geometry, 16, 0.12, 0.32, 2, 1, -1.0, 0.01, 1)
    xyz, bgr = api.dense_cloud_for_all(images, sc.K4, ext, n_src=2, planes=16, radius=2, wmin=0.12, wmax=0.32, min_score=-1.0, rel_tol=0.01, min_consistent=1, ctx=ctx)
    assert _same(xyz, np.concatenate([e["xyz"] for e in exp])) and _same(bgr, np.concatenate([e["bgr"] for e in exp]))
    assert api.dense_sources(ext, 2) == dr.nearest_sources(ext, 2) and len(xyz) > 0


def test_module_level_call_and_mesh_take_observations(ctx, decoy_dense):
    sc, ext, pts, oc, op, images = decoy_dense
    sel = api.select_views(ext, pts, oc, op, n_src=2, min_angle_deg=1.0, ctx=ctx)
    exp = sr.select_views(ext, pts, oc, op, 2, COS2_1DEG, api.sweep_geometry)
    assert sel._fields == NAMES and all(_same(getattr(sel, n), exp[n]) for n in NAMES)
    xyz, bgr, tri = api.dense_mesh_for_all(images, sc.K4, ext, sparse_pts=pts, n_src=2, planes=16, min_score=-1.0, ctx=ctx, voxels=32, observations=(oc, op))
    print("mesh with ranked sources:", len(xyz), "vertices,", len(tri), "triangles")
    assert len(tri) > 100 and len(xyz) == len(bgr)


def test_cpp_mirror_writes_the_same_arrays(ring, tmp_path):
    ext, pts, oc, op, exp = ring
    host = os.path.join(HERE, "host")
    subprocess.check_call(["make", "-C", host, "-f", "select.mk", "select_test"], stdout=subprocess.DEVNULL)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<4i", len(ext), len(pts), len(oc), 3)); f.write(struct.pack("<d", 1.0))
        f.write(np.ascontiguousarray(ext, np.float64).tobytes()); f.write(np.ascontiguousarray(pts, np.float64).tobytes())
        f.write(np.ascontiguousarray(oc, np.int32).tobytes()); f.write(np.ascontiguousarray(op, np.int32).tobytes())
    out = subprocess.run([os.path.join(host, "select_test"), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    raw = open(tmp_path / "out.bin", "rb").read()
    at = 0
    for name in NAMES:
        e = exp[name]
        got = np.frombuffer(raw, e.dtype, e.size, at).reshape(e.shape)
        at += e.nbytes
        assert _same(got, e), name
    assert at == len(raw)
