"""GPU: the dense-depth stages (sfmhip_plane_sweep, sfmhip_depth_consistency, sfmhip_depth_to_points) against the numpy restatement of
their definition (tests/dense_ref.py), fed with the library's own geometry arrays: every output byte is equal.  Then determinism, the
entry forms, the export's cap, the argument rules, an injected allocation failure, and the layers above (api.dense_cloud_for_all and
its C++ mirror)."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import dense_ref as dr
from sfm_opencv_amd import _lib, api

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
WMIN, WMAX = 1.0 / 8.0, 1.0 / 3.0


def _same(a, b):
    a = np.asarray(a); b = np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def scene():
    sc = dr.Scene()
    return sc, [sc.render(v)[0] for v in range(4)]


def _geo(sc, ref, srcs):
    return api.sweep_geometry(sc.K4, sc.EXT[ref], sc.EXT[list(srcs)])


def _check_sweep(ctx, ref, srcs, A, b, D, r, min_sources=1, min_score=-1.0, wmin=WMIN, wmax=WMAX):
    got = ctx.plane_sweep(ref, srcs, A, b, D, wmin, wmax, r, min_sources, min_score)
    exp = dr.plane_sweep(ref, srcs, A, b, D, wmin, wmax, r, min_sources, min_score)[:3]
    for name, g, e in zip(("plane", "score", "depth"), got, exp):
        assert _same(g, e), (name, int((g.view(np.uint32) != e.view(np.uint32)).sum()))
    return got


# ------------------------------------------------------------------------------------------------ the whole chain on the planted scene
@pytest.fixture(scope="module")
def chain(ctx, scene):
    """the four 96 x 72 views, three sources each, D = 48, r = 2: the library's outputs and the restatement's, computed once"""
    sc, images = scene
    sources = dr.nearest_sources(sc.EXT, 3)
    exp = dr.chain(images, sc.K4, sc.EXT, sources, api.sweep_geometry, 48, WMIN, WMAX, 2, 1, -1.0, 0.01, 2)
    got = []
    for i, img in enumerate(images):
        e = exp[i]
        plane, score, depth = ctx.plane_sweep(img, [images[j] for j in sources[i]], e["A"], e["b"], 48, WMIN, WMAX, 2, 1, -1.0)
        got.append(dict(plane=plane, score=score, depth=depth))
    for i, img in enumerate(images):
        e, g = exp[i], got[i]
        g["count"], g["keep"] = ctx.depth_consistency(g["depth"], [got[j]["depth"] for j in sources[i]], sc.K4, e["Rrel"], e["trel"], 0.01, 2)
        g["xyz"], g["bgr"], g["n_found"] = ctx.depth_to_points(g["depth"], g["keep"], img, sc.K4, e["Rinv"], e["c"])
    return sources, exp, got


@pytest.mark.parametrize("what", ["plane", "score", "depth", "count", "keep", "xyz", "bgr"])
def test_planted_scene_equals_the_restatement(chain, what):
    _, exp, got = chain
    for i, (e, g) in enumerate(zip(exp, got)):
        assert _same(g[what], e[what]), (i, what)
        assert g["n_found"] == len(e["xyz"]) == int(e["keep"].sum())
    assert (exp[0]["plane"] >= 0).mean() > 0.8 and exp[0]["keep"].mean() > 0.5           # the case is not an empty one


# ------------------------------------------------------------------------------------------------ the sweep at its edges
def test_odd_sizes_that_are_no_multiple_of_a_tile(ctx):
    sc = dr.Scene()
    images = [sc.render(v, rows=71, cols=97)[0] for v in range(3)]
    A, b, *_ = _geo(sc, 0, (1, 2))
    plane, _, _ = _check_sweep(ctx, images[0], images[1:], A, b, 16, 2)
    assert (plane >= 0).mean() > 0.5


def test_radius_zero_scores_nothing(ctx, scene):
    sc, images = scene
    A, b, *_ = _geo(sc, 0, (1, 2))
    plane, score, depth = _check_sweep(ctx, images[0], images[1:3], A, b, 8, 0)
    assert (plane == -1).all() and np.isnan(score).all() and np.isnan(depth).all()


def test_radius_five_on_a_small_image(ctx):
    sc = dr.Scene()
    images = [sc.render(v, rows=30, cols=40)[0] for v in range(3)]
    A, b, *_ = _geo(sc, 0, (1, 2))
    plane, _, _ = _check_sweep(ctx, images[0], images[1:], A, b, 12, 5)
    assert (plane >= 0).sum() > 50 and (plane[:5] == -1).all() and (plane[:, -5:] == -1).all()


def test_more_tiles_than_workgroups(ctx):
    """the grid is at most eight workgroups per CU and a workgroup walks the tiles with the grid's stride: 65 x 33 tiles of 32 x 16 pixels
    are more than 8 x 256, so some workgroups take a second tile (a plain shift along x, two planes, one source: a second of numpy)"""
    rng = np.random.default_rng(9)
    rows, cols = 33 * 16 - 5, 65 * 32 - 7
    base = rng.integers(0, 256, (rows, cols + 8), dtype=np.uint8)
    ref, src = np.ascontiguousarray(base[:, :cols]), np.ascontiguousarray(base[:, 3:cols + 3])
    A = np.eye(3, dtype=np.float32).reshape(1, 9); b = np.array([[-3.0, 0.0, 0.0]], np.float32)
    plane, score, _ = _check_sweep(ctx, ref, [src], A, b, 2, 1, wmin=0.5, wmax=1.0)
    # the plane w = 1 undoes the shift exactly, wherever the window's samples are good (sy < rows - 1 leaves the last two rows out)
    assert (plane[1:-2, 4:-1] == 1).all() and (score[1:-2, 4:-1] == 1.0).all()


@pytest.mark.parametrize("rows,cols", [(20, 3), (4, 40), (1, 1)])
def test_image_smaller_than_the_window_is_not_an_error(ctx, rows, cols):
    sc = dr.Scene()
    rng = np.random.default_rng(rows)
    images = [rng.integers(0, 256, (rows, cols), dtype=np.uint8) for _ in range(2)]
    A, b, *_ = _geo(sc, 0, (1,))
    plane, _, _ = _check_sweep(ctx, images[0], images[1:], A, b, 4, 2)
    assert (plane == -1).all()


def test_two_planes_never_take_the_fit(ctx, scene):
    sc, images = scene
    A, b, *_ = _geo(sc, 0, (1, 2))
    plane, _, depth = _check_sweep(ctx, images[0], images[1:3], A, b, 2, 2, wmin=1.0 / 6.0, wmax=1.0 / 4.0)
    ok = plane >= 0
    assert ok.sum() > 1000 and set(np.unique(depth[ok])) <= {np.float32(1.0 / (1.0 / 6.0)), np.float32(1.0 / (1.0 / 4.0))}


def test_constant_source_never_counts(ctx, scene):
    sc, images = scene
    A, b, *_ = _geo(sc, 0, (1, 2))
    flat = np.full_like(images[1], 93)
    both = _check_sweep(ctx, images[0], [flat, images[2]], A, b, 12, 2)
    only = ctx.plane_sweep(images[0], [images[2]], A[1:], b[1:], 12, WMIN, WMAX, 2, 1, -1.0)
    assert all(_same(x, y) for x, y in zip(both, only)) and (both[0] >= 0).sum() > 1000
    none = _check_sweep(ctx, images[0], [flat], A[:1], b[:1], 12, 2)
    assert (none[0] == -1).all()


def test_source_that_sees_nothing_is_never_good(ctx, scene):
    sc, images = scene
    away = np.array([[0.0, np.pi, 0.0, 0.3, 0.0, 0.0]])                  # looks the other way: q_2 < 0 everywhere
    A, b, *_ = api.sweep_geometry(sc.K4, sc.EXT[0], np.concatenate([away, sc.EXT[1:2]]))
    both = _check_sweep(ctx, images[0], [images[3], images[1]], A, b, 12, 2)
    only = ctx.plane_sweep(images[0], [images[1]], A[1:], b[1:], 12, WMIN, WMAX, 2, 1, -1.0)
    assert all(_same(x, y) for x, y in zip(both, only)) and (both[0] >= 0).sum() > 1000
    assert (_check_sweep(ctx, images[0], [images[3]], A[:1], b[:1], 12, 2)[0] == -1).all()


def test_min_sources_above_the_sources_and_min_score_above_one(ctx, scene):
    sc, images = scene
    A, b, *_ = _geo(sc, 0, (1, 2))
    assert (_check_sweep(ctx, images[0], images[1:3], A, b, 12, 2, min_sources=3)[0] == -1).all()
    assert (_check_sweep(ctx, images[0], images[1:3], A, b, 12, 2, min_score=1.5)[0] == -1).all()
    some = _check_sweep(ctx, images[0], images[1:3], A, b, 12, 2, min_sources=2, min_score=0.8)[0]
    assert 500 < (some >= 0).sum() < some.size - 500                     # both rules cut, neither cuts everything


def test_bgr_input(ctx, scene):
    sc, images = scene
    A, b, *_ = _geo(sc, 0, (1, 2))
    gray = ctx.plane_sweep(images[0], images[1:3], A, b, 12, WMIN, WMAX, 2, 1, -1.0)
    rep = [np.repeat(im[:, :, None], 3, 2) for im in images[:3]]         # B = G = R = g: the formula's weights add up to 2^14
    got = ctx.plane_sweep(rep[0], rep[1:], A, b, 12, WMIN, WMAX, 2, 1, -1.0)
    assert all(_same(x, y) for x, y in zip(got, gray))
    rng = np.random.default_rng(5)
    col = [np.clip(r.astype(np.int64) + rng.integers(-40, 41, r.shape), 0, 255).astype(np.uint8) for r in rep]
    _check_sweep(ctx, col[0], col[1:], A, b, 12, 2)
    # the export carries the pixel's three bytes
    depth = np.where(gray[0] >= 0, gray[2], np.float32(np.nan)); keep = (gray[0] >= 0).astype(np.uint8)
    _, _, _, _, Rinv, c = _geo(sc, 0, (1,))
    xyz, bgr, n = ctx.depth_to_points(depth, keep, col[0], sc.K4, Rinv, c)
    exyz, ebgr = dr.depth_to_points(depth, keep, col[0], sc.K4, Rinv, c)
    assert n == len(exyz) and _same(xyz, exyz) and _same(bgr, ebgr)


def test_padded_rows(ctx, scene):
    sc, images = scene
    A, b, *_ = _geo(sc, 0, (1, 2))
    dense = ctx.plane_sweep(images[0], images[1:3], A, b, 12, WMIN, WMAX, 2, 1, -1.0)
    rows, cols = images[0].shape
    bufs = [np.full((rows, cols + 13), 0xAB, np.uint8) for _ in range(3)]
    for buf, im in zip(bufs, images):
        buf[:, :cols] = im
    views = [buf[:, :cols] for buf in bufs]
    assert api._dense_images(views)[5] == cols + 13                      # passed where they lie
    got = ctx.plane_sweep(views[0], views[1:], A, b, 12, WMIN, WMAX, 2, 1, -1.0)
    assert all(_same(x, y) for x, y in zip(got, dense))
    assert all((buf[:, cols:] == 0xAB).all() and np.array_equal(buf[:, :cols], im) for buf, im in zip(bufs, images))
    keep = (dense[0] >= 0).astype(np.uint8)
    _, _, _, _, Rinv, c = _geo(sc, 0, (1,))
    a = ctx.depth_to_points(dense[2], keep, views[0], sc.K4, Rinv, c); e = ctx.depth_to_points(dense[2], keep, images[0], sc.K4, Rinv, c)
    assert a[2] == e[2] and _same(a[0], e[0]) and _same(a[1], e[1])


# ------------------------------------------------------------------------------------------------ determinism and entry forms
def test_two_runs_give_the_same_bytes(ctx, scene, chain):
    sc, images = scene
    sources, exp, got = chain
    e = exp[1]
    again = ctx.plane_sweep(images[1], [images[j] for j in sources[1]], e["A"], e["b"], 48, WMIN, WMAX, 2, 1, -1.0)
    assert all(_same(x, got[1][k]) for x, k in zip(again, ("plane", "score", "depth")))


def test_dev_forms_on_resident_arrays_equal_the_host_forms(ctx, scene, chain):
    import torch
    sc, images = scene
    sources, exp, got = chain
    rows, cols = images[0].shape
    dev = torch.device("cuda", ctx.device)
    d_img = [torch.from_numpy(im).to(dev) for im in images]
    d_depth = []
    for i in range(4):
        plane = torch.empty((rows, cols), dtype=torch.int32, device=dev); score = torch.empty((rows, cols), dtype=torch.float32, device=dev)
        depth = torch.empty((rows, cols), dtype=torch.float32, device=dev)
        ctx.plane_sweep_dev(d_img[i], [d_img[j] for j in sources[i]], rows, cols, 1, cols, exp[i]["A"], exp[i]["b"], 48, WMIN, WMAX, 2, 1, -1.0, plane, score, depth)
        d_depth.append(depth)
        if i == 0:
            ctx.synchronize()
            assert _same(plane.cpu().numpy(), got[0]["plane"]) and _same(score.cpu().numpy(), got[0]["score"])
    count = torch.empty((rows, cols), dtype=torch.uint8, device=dev); keep = torch.empty((rows, cols), dtype=torch.uint8, device=dev)
    xyz = torch.zeros((rows * cols, 3), dtype=torch.float64, device=dev); bgr = torch.zeros((rows * cols, 3), dtype=torch.uint8, device=dev)
    n = torch.zeros(1, dtype=torch.int32, device=dev)
    e = exp[2]
    ctx.depth_consistency_dev(d_depth[2], [d_depth[j] for j in sources[2]], rows, cols, sc.K4, e["Rrel"], e["trel"], 0.01, 2, count, keep)
    ctx.depth_to_points_dev(d_depth[2], keep, d_img[2], rows, cols, 1, cols, sc.K4, e["Rinv"], e["c"], xyz, bgr, rows * cols, n)
    ctx.synchronize()
    m = int(n.item())
    g = got[2]
    assert _same(d_depth[2].cpu().numpy(), g["depth"]) and _same(count.cpu().numpy(), g["count"]) and _same(keep.cpu().numpy(), g["keep"])
    assert m == g["n_found"] and _same(xyz[:m].cpu().numpy(), g["xyz"]) and _same(bgr[:m].cpu().numpy(), g["bgr"])


# ------------------------------------------------------------------------------------------------ export, errors
def test_cap_below_the_count_cuts_nothing_silently(ctx, scene, chain):
    sc, images = scene
    _, exp, got = chain
    e, g = exp[0], got[0]
    full = g["n_found"]
    cap = full // 3
    xyz = np.full((cap + 1, 3), -7.0); bgr = np.full((cap + 1, 3), 0xCD, np.uint8); n = C.c_int32(-1)
    K4 = np.array(sc.K4); depth = g["depth"]; keep = g["keep"]; img = images[0]
    rc = ctx.lib.sfmhip_depth_to_points(ctx.h, depth.ctypes.data, keep.ctypes.data, img.ctypes.data, img.shape[0], img.shape[1], 1, img.shape[1], K4.ctypes.data,
                                        e["Rinv"].ctypes.data, e["c"].ctypes.data, xyz.ctypes.data, bgr.ctypes.data, cap, C.byref(n))
    assert rc == 0 and n.value == full and cap > 100
    assert _same(xyz[:cap], g["xyz"][:cap]) and _same(bgr[:cap], g["bgr"][:cap])
    assert (xyz[cap] == -7.0).all() and (bgr[cap] == 0xCD).all()
    xyz0, bgr0, n0 = ctx.depth_to_points(depth, keep, img, sc.K4, e["Rinv"], e["c"], cap=0)
    assert n0 == full and len(xyz0) == 0 and len(bgr0) == 0


def _raw_sweep(ctx, images, geo_A, geo_b, **over):
    """sfmhip_plane_sweep straight through ctypes with outputs that hold a sentinel: (rc, outputs untouched)"""
    rows, cols = images[0].shape[:2]
    a = dict(ref=images[0].ctypes.data, src=[im.ctypes.data for im in images[1:]], n_src=len(images) - 1, rows=rows, cols=cols, channels=1, ld=cols,
             A=geo_A.ctypes.data, b=geo_b.ctypes.data, D=8, wmin=WMIN, wmax=WMAX, r=2, min_sources=1, min_score=0.0, plane=True, score=True, depth=True)
    a.update(over)
    plane = np.full((rows, cols), 77, np.int32); score = np.full((rows, cols), 5.0, np.float32); depth = np.full((rows, cols), 6.0, np.float32)
    src = (C.c_void_p * 8)(*a["src"]) if a["src"] is not None else None
    rc = ctx.lib.sfmhip_plane_sweep(ctx.h, a["ref"], src, a["n_src"], a["rows"], a["cols"], a["channels"], a["ld"], a["A"], a["b"], a["D"], a["wmin"], a["wmax"], a["r"],
                                    a["min_sources"], a["min_score"], plane.ctypes.data if a["plane"] else None, score.ctypes.data if a["score"] else None,
                                    depth.ctypes.data if a["depth"] else None)
    return rc, bool((plane == 77).all() and (score == 5.0).all() and (depth == 6.0).all())


def test_bad_arguments_leave_the_outputs_alone(ctx, scene):
    sc, images = scene
    A, b, Rrel, trel, Rinv, c = _geo(sc, 0, (1, 2))
    ims = images[:3]
    assert _raw_sweep(ctx, ims, A, b) == (0, False)
    bad = [dict(ref=None), dict(src=None), dict(src=[ims[1].ctypes.data, None]), dict(A=None), dict(b=None), dict(plane=False), dict(score=False), dict(depth=False),
           dict(n_src=0), dict(n_src=9), dict(rows=0), dict(cols=0), dict(rows=16385), dict(cols=16385), dict(channels=2), dict(channels=4), dict(ld=ims[0].shape[1] - 1),
           dict(D=1), dict(D=4097), dict(wmin=WMAX, wmax=WMAX), dict(wmin=WMAX, wmax=WMIN), dict(wmin=0.0), dict(wmin=-1.0), dict(wmax=float("inf")),
           dict(wmin=float("nan")), dict(r=-1), dict(r=6), dict(min_sources=0), dict(min_score=float("nan"))]
    for over in bad:
        assert _raw_sweep(ctx, ims, A, b, **over) == (_lib.E_ARG, True), over
    # the other two stages
    rows, cols = ims[0].shape
    depth = np.ones((rows, cols), np.float32); keep = np.ones((rows, cols), np.uint8); K4 = np.array(sc.K4)
    count = np.full((rows, cols), 9, np.uint8); kept = np.full((rows, cols), 9, np.uint8)
    srcs = (C.c_void_p * 8)(depth.ctypes.data, depth.ctypes.data)

    def cons(depth_p=depth.ctypes.data, src=srcs, n_src=2, r_=rows, c_=cols, K=K4.ctypes.data, R=Rrel.ctypes.data, t=trel.ctypes.data, tol=0.01, mc=1,
             cnt=count.ctypes.data, kp=kept.ctypes.data):
        return ctx.lib.sfmhip_depth_consistency(ctx.h, depth_p, src, n_src, r_, c_, K, R, t, tol, mc, cnt, kp)
    for kw in (dict(depth_p=None), dict(src=None), dict(n_src=0), dict(n_src=9), dict(r_=0), dict(c_=16385), dict(K=None), dict(R=None), dict(t=None), dict(tol=-0.1),
               dict(tol=float("nan")), dict(mc=-1), dict(cnt=None, kp=None)):
        assert cons(**kw) == _lib.E_ARG, kw
    assert (count == 9).all() and (kept == 9).all()
    assert cons() == 0 and not (count == 9).any()
    xyz = np.full((rows * cols, 3), -7.0); bgr = np.full((rows * cols, 3), 0xCD, np.uint8); n = C.c_int32(-5)

    def pts(d=depth.ctypes.data, k=keep.ctypes.data, im=ims[0].ctypes.data, r_=rows, c_=cols, ch=1, ld=cols, K=K4.ctypes.data, Ri=Rinv.ctypes.data, cc=c.ctypes.data,
            x=xyz.ctypes.data, bg=bgr.ctypes.data, cap=rows * cols, nf=C.byref(n)):
        return ctx.lib.sfmhip_depth_to_points(ctx.h, d, k, im, r_, c_, ch, ld, K, Ri, cc, x, bg, cap, nf)
    for kw in (dict(d=None), dict(k=None), dict(im=None), dict(r_=0), dict(c_=0), dict(ch=2), dict(ld=cols - 1), dict(K=None), dict(Ri=None), dict(cc=None),
               dict(x=None, bg=None), dict(cap=-1), dict(nf=None)):
        assert pts(**kw) == _lib.E_ARG, kw
    assert (xyz == -7.0).all() and (bgr == 0xCD).all() and n.value == -5
    assert pts() == 0 and n.value == rows * cols


def test_a_failed_allocation_is_an_error_and_the_next_call_works(ctx, scene, chain):
    sc, images = scene
    sources, exp, got = chain
    e, g = exp[0], got[0]
    srcs = [images[j] for j in sources[0]]
    for failing in (1, 2):
        assert ctx.lib.sfmhip_debug_fail_allocations(ctx.h, failing) == 0
        for _ in range(failing):
            rc, untouched = _raw_sweep(ctx, [images[0]] + srcs, e["A"], e["b"])
            assert rc == _lib.E_HIP and untouched
        again = ctx.plane_sweep(images[0], srcs, e["A"], e["b"], 48, WMIN, WMAX, 2, 1, -1.0)
        assert all(_same(x, g[k]) for x, k in zip(again, ("plane", "score", "depth")))
    assert ctx.lib.sfmhip_debug_fail_allocations(ctx.h, 1) == 0
    with pytest.raises(api.SfmHipError):
        ctx.depth_consistency(g["depth"], [got[j]["depth"] for j in sources[0]], sc.K4, e["Rrel"], e["trel"], 0.01, 2)
    assert ctx.lib.sfmhip_debug_fail_allocations(ctx.h, 1) == 0
    with pytest.raises(api.SfmHipError):
        ctx.depth_to_points(g["depth"], g["keep"], images[0], sc.K4, e["Rinv"], e["c"])
    xyz, bgr, n = ctx.depth_to_points(g["depth"], g["keep"], images[0], sc.K4, e["Rinv"], e["c"])
    assert n == g["n_found"] and _same(xyz, g["xyz"]) and _same(bgr, g["bgr"])


# ------------------------------------------------------------------------------------------------ the layers above
@pytest.fixture(scope="module")
def cloud(ctx, scene):
    sc, images = scene
    return api.dense_cloud_for_all(images, sc.K4, sc.EXT, n_src=3, planes=48, radius=2, wmin=WMIN, wmax=WMAX, min_score=-1.0, rel_tol=0.01, min_consistent=2, ctx=ctx)


def test_dense_cloud_for_all(ctx, scene, chain, cloud):
    sc, images = scene
    _, exp, _ = chain
    xyz, bgr = cloud
    assert _same(xyz, np.concatenate([e["xyz"] for e in exp])) and _same(bgr, np.concatenate([e["bgr"] for e in exp]))
    assert len(xyz) >= 4 * 0.5 * sc.ROWS * sc.COLS * 0.5                  # many times half a view's pixels
    step = (WMAX - WMIN) / 47
    assert (sc.plane_distance(xyz) <= 6.6 ** 2 * step).mean() >= 0.98     # the CPU test's bound (no true depth exceeds 6.6)
    cen, counts, voxel_of, _ = ctx.voxel_downsample(xyz, 0.1)
    assert 100 < len(cen) < len(xyz) and counts.sum() == len(xyz)
    nrm = ctx.estimate_normals(xyz, 10)
    assert nrm.shape == xyz.shape and np.isfinite(nrm).mean() > 0.99
    # the range from sparse points, and the voxel option
    rng = np.random.default_rng(2)
    sparse = np.stack([rng.uniform(-1.5, 1.5, 400), rng.uniform(-1, 1, 400), rng.uniform(3.9, 6.4, 400)], 1)
    vx, vb = api.dense_cloud_for_all(images, sc.K4, sc.EXT, sparse_pts=sparse, n_src=2, planes=32, radius=2, min_score=0.6, voxel=0.1, ctx=ctx)
    assert 100 < len(vx) < len(xyz) and vb.shape == vx.shape and (sc.plane_distance(vx) <= 0.3).mean() >= 0.95


def test_cpp_mirror_writes_the_same_cloud(scene, cloud, tmp_path):
    sc, images = scene
    host = os.path.join(HERE, "host")
    subprocess.check_call(["make", "-C", host, "-f", "dense.mk", "dense_test"], stdout=subprocess.DEVNULL)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<10i", 4, sc.ROWS, sc.COLS, 1, 3, 48, 2, 1, 2, 0)); f.write(struct.pack("<5d", WMIN, WMAX, -1.0, 0.01, 0.0))
        f.write(np.array(sc.K4).tobytes()); f.write(np.ascontiguousarray(sc.EXT).tobytes())
        for im in images:
            f.write(im.tobytes())
    out = subprocess.run([os.path.join(host, "dense_test"), "cloud", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    raw = open(tmp_path / "out.bin", "rb").read()
    (n,) = struct.unpack_from("<i", raw, 0)
    xyz = np.frombuffer(raw, "<f8", 3 * n, 4).reshape(-1, 3); bgr = np.frombuffer(raw, np.uint8, 3 * n, 4 + 24 * n).reshape(-1, 3)
    assert n == len(cloud[0]) and _same(xyz, cloud[0]) and _same(bgr, cloud[1])
