"""GPU: the dense mesh (sfmhip_tsdf_integrate, sfmhip_tsdf_mesh) against the numpy restatement of its definition (tests/tsdf_ref.py): every
byte of the volume, the counts, the vertices, their colours and the triangles is equal.  Then the edges of the definition, determinism,
the entry forms, the caps, the argument rules, an injected allocation failure, and the layers above (api.dense_mesh_for_all, the .ply
writer and the C++ mirror)."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import dense_ref as dr
import tsdf_ref as tr
from sfm_opencv_amd import _lib, api, formats

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _same(a, b):
    a = np.asarray(a); b = np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _integrate(ctx, dims, origin, voxel, trunc, depths, keeps, imgs, K4, R, t, vol=None):
    """the views into a (new) volume, 8 per call: (dsum, wsum, csum)"""
    d, w, c = vol if vol is not None else tr.new_volume(dims, imgs is not None)
    for i0 in range(0, len(depths), 8):
        sl = slice(i0, i0 + 8)
        ctx.tsdf_integrate(dims, origin, voxel, trunc, depths[sl], None if keeps is None else keeps[sl], None if imgs is None else imgs[sl], K4, R[sl], t[sl], d, w, c)
    return d, w, c


def _check_volume(ctx, dims, origin, voxel, trunc, depths, keeps, imgs, K4, R, t):
    got = _integrate(ctx, dims, origin, voxel, trunc, depths, keeps, imgs, K4, R, t)
    exp = tr.new_volume(dims, imgs is not None)
    tr.integrate(dims, origin, voxel, trunc, depths, keeps, imgs, K4, R, t, *exp)
    for name, g, e in zip(("dsum", "wsum", "csum"), got, exp):
        assert (g is None and e is None) or _same(g, e), (name, int((g != e).sum()))
    return got


def _check_mesh(ctx, dims, origin, voxel, vol, min_weight):
    d, w, c = vol
    xyz, bgr, tri, nv, nt = ctx.tsdf_mesh(dims, origin, voxel, d, w, c, min_weight)
    exyz, ebgr, etri = tr.mesh(dims, origin, voxel, d, w, c, min_weight)
    assert (nv, nt) == (len(exyz), len(etri))
    assert _same(xyz, exyz) and _same(tri, etri) and ((bgr is None and ebgr is None) or _same(bgr, ebgr))
    return xyz, bgr, tri


# ------------------------------------------------------------------------------------------------ the fused sphere, computed once
@pytest.fixture(scope="module")
def sphere(ctx):
    """14 views of the unit sphere into 24^3 voxels, trunc = 3 voxels, random BGR images, keep masks that drop a checkerboard of pixels"""
    depths, R, t = tr.sphere_views(14)
    rng = np.random.default_rng(11)
    imgs = [rng.integers(0, 256, (96, 96, 3), dtype=np.uint8) for _ in depths]
    board = (np.indices((96, 96)).sum(0) % 2).astype(np.uint8)
    keeps = [board if i % 2 == 0 else (1 - board).astype(np.uint8) for i in range(len(depths))]
    dims, origin, voxel = tr.sphere_box(24)
    vol = _check_volume(ctx, dims, origin, voxel, 3 * voxel, depths, keeps, imgs, tr.SPHERE_K4, R, t)
    return dict(dims=dims, origin=origin, voxel=voxel, trunc=3 * voxel, depths=depths, keeps=keeps, imgs=imgs, R=R, t=t, vol=vol)


@pytest.fixture(scope="module")
def sphere_mesh(ctx, sphere):
    s = sphere
    return _check_mesh(ctx, s["dims"], s["origin"], s["voxel"], s["vol"], 1)


def test_fused_sphere_equals_the_restatement(sphere, sphere_mesh):
    d, w, c = sphere["vol"]
    xyz, bgr, tri = sphere_mesh
    assert w.max() >= 3 and (d < 0).any() and (c.sum(1) > 0).any()
    st = tr.mesh_stats(xyz, tri)
    assert len(tri) > 1000 and st["duplicated"] == 0 and st["volume"] > 0 and len(np.unique(bgr)) > 50


# ------------------------------------------------------------------------------------------------ the planted scene through the device chain
PLANES, N_SRC, WMIN, WMAX = 32, 2, 1.0 / 8.0, 1.0 / 3.0
SCENE_VOLUME = ((40, 30, 20), (-3.0, -2.25, 3.4), 0.15)
SCENE_TRUNC_VOXELS, SCENE_MIN_WEIGHT = 3, 2


@pytest.fixture(scope="module")
def planted(ctx):
    """dense_ref.Scene at 96 x 72: the restatement's chain (sweep, consistency) and the library's, computed once"""
    sc = dr.Scene()
    images = [sc.render(v)[0] for v in range(4)]
    sources = dr.nearest_sources(sc.EXT, N_SRC)
    exp = dr.chain(images, sc.K4, sc.EXT, sources, api.sweep_geometry, PLANES, WMIN, WMAX, 2, 1, -1.0, 0.01, 2)
    depth = [ctx.plane_sweep(images[i], [images[j] for j in sources[i]], exp[i]["A"], exp[i]["b"], PLANES, WMIN, WMAX, 2, 1, -1.0)[2] for i in range(4)]
    keep = [ctx.depth_consistency(depth[i], [depth[j] for j in sources[i]], sc.K4, exp[i]["Rrel"], exp[i]["trel"], 0.01, 2)[1] for i in range(4)]
    R = np.array([np.asarray(e["Rinv"]).reshape(3, 3).T.ravel() for e in exp])                 # world to camera, as dense_mesh_for_all forms it
    return dict(sc=sc, images=images, exp=exp, depth=depth, keep=keep, R=R, t=np.ascontiguousarray(sc.EXT[:, 3:]))


def test_planted_scene_through_the_device_chain(ctx, planted):
    p = planted
    dims, origin, voxel = SCENE_VOLUME
    assert np.mean([k.mean() for k in p["keep"]]) > 0.4
    vol = _check_volume(ctx, dims, origin, voxel, SCENE_TRUNC_VOXELS * voxel, p["depth"], p["keep"], p["images"], p["sc"].K4, p["R"], p["t"])
    xyz, bgr, tri = _check_mesh(ctx, dims, origin, voxel, vol, SCENE_MIN_WEIGHT)
    assert len(tri) > 500 and (bgr[:, 0] == bgr[:, 2]).all()                                   # gray images: B = G = R


# ------------------------------------------------------------------------------------------------ shapes
@pytest.mark.parametrize("dims,origin,voxel,empty", [((17, 9, 5), (-1.5, -0.79, -0.44), 3.0 / 17, False), ((2, 2, 2), (0.8, -0.2, -0.2), 0.2, False),
                                                     ((1, 7, 7), (0.9, -0.7, -0.7), 0.2, True)])
def test_small_and_degenerate_volumes(ctx, sphere, dims, origin, voxel, empty):
    s = sphere
    pick = [0, 2, 6]
    vol = _check_volume(ctx, dims, origin, voxel, 3 * voxel, [s["depths"][i] for i in pick], None, [s["imgs"][i] for i in pick], tr.SPHERE_K4, s["R"][pick], s["t"][pick])
    assert vol[1].max() >= 1
    xyz, bgr, tri = _check_mesh(ctx, dims, origin, voxel, vol, 1)
    assert (len(tri) == 0 and len(xyz) == 0) if empty else len(tri) > 0


def test_more_voxels_than_one_grid_of_workgroups(ctx, sphere):
    """130 x 130 x 40 voxels are 2641 workgroups of 256, more than the 8 per CU a launch is sized to: every thread walks with the grid's stride"""
    s = sphere
    dims, voxel = (130, 130, 40), 3.0 / 130
    origin = (-1.5, -1.5, -20 * voxel)
    pick = [0, 2, 7]
    vol = _check_volume(ctx, dims, origin, voxel, 4 * voxel, [s["depths"][i] for i in pick], None, None, tr.SPHERE_K4, s["R"][pick], s["t"][pick])
    xyz, bgr, tri = _check_mesh(ctx, dims, origin, voxel, vol, 1)
    assert bgr is None and len(tri) > 5000 and np.abs(np.linalg.norm(xyz, axis=1) - 1.0).max() < 2 * voxel


# ------------------------------------------------------------------------------------------------ the edges of the definition
def test_edges_of_the_definition(ctx):
    """one camera at the origin looking along z, dyadic numbers throughout: voxels behind the camera and at Y_2 = 0, voxels that project
    outside the image, NaN and infinite depths, s == -trunc (counts) and s > trunc (clamped), a voxel with dsum == 0 (outside),
    min_weight = 3, gray images in padded rows, and no colour at all"""
    dims, origin, voxel, trunc = (5, 5, 8), (-1.25, -1.25, -1.25), 0.5, 0.5
    K4 = (4.0, 4.0, 3.5, 3.5)
    eye = np.eye(3).ravel()
    depth = np.full((8, 8), 1.5, np.float32)
    depth[0, 0] = np.nan; depth[3, 3] = np.inf; depth[7, 7] = -np.inf
    bufs = [np.full((8, 13), 0xAB, np.uint8) for _ in range(3)]
    rng = np.random.default_rng(4)
    for b in bufs:
        b[:, :8] = rng.integers(0, 256, (8, 8), dtype=np.uint8)
    gray = [b[:, :8] for b in bufs]
    assert api._dense_images(gray)[5] == 13                                                   # passed where they lie
    # one view: the column of voxels on the optical axis, z = -1, -0.5, 0, 0.5, 1, 1.5, 2, 2.5
    d, w, c = _check_volume(ctx, dims, origin, voxel, trunc, [depth], None, gray[:1], K4, eye[None], np.zeros((1, 3)))
    col = np.arange(8) * 25 + 2 * 5 + 2
    assert d[col].tolist() == [0, 0, 0, 32767, 32767, 0, -32767, 0] and w[col].tolist() == [0, 0, 0, 1, 1, 1, 1, 0]
    px = int(gray[0][4, 4])
    assert c[col[5]].tolist() == [px, px, px] and c[col[7]].tolist() == [0, 0, 0]
    corner = 3 * 25                                                                            # (0, 0, 3): X = (-1, -1, 0.5) projects to pu = -4
    assert w[corner] == 0
    assert all((b[:, 8:] == 0xAB).all() for b in bufs)
    # three views: the same camera, the camera half a unit to the side, and the first again with another map
    other = np.full((8, 8), 1.5, np.float32); other[:, 5:] = 1.75
    depths = [depth, depth, other]
    R = np.stack([eye] * 3); t = np.array([[0.0, 0, 0], [-0.5, 0, 0], [0.0, 0, 0]])
    keep = np.ones((8, 8), np.uint8); keep[2, :] = 0
    vol = _check_volume(ctx, dims, origin, voxel, trunc, depths, [None, keep, None], gray, K4, R, t)
    assert vol[1].max() == 3 and (vol[0] == 0)[vol[1] > 0].any()
    bare = _check_volume(ctx, dims, origin, voxel, trunc, depths, [None, keep, None], None, K4, R, t)
    assert bare[2] is None and _same(bare[0], vol[0]) and _same(bare[1], vol[1])
    n_tri = {}
    for mw in (1, 3):
        xyz, bgr, tri = _check_mesh(ctx, dims, origin, voxel, vol, mw)
        n_tri[mw] = len(tri)
        assert _check_mesh(ctx, dims, origin, voxel, bare, mw)[1] is None
    assert n_tri[1] > n_tri[3] > 0
    # a vertex on an edge whose outside end has dsum == 0 lies on that voxel's centre, and its triangles have no area: they are kept
    p = xyz[tri]
    assert (np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1) == 0).any()


# ------------------------------------------------------------------------------------------------ determinism and entry forms
def test_any_split_and_order_of_the_views_gives_the_same_volume(ctx, sphere):
    s = sphere
    vol = tr.new_volume(s["dims"])
    for part in ([13, 12, 11, 10, 9], [8, 7, 6, 5, 4], [3, 2, 1, 0]):
        ctx.tsdf_integrate(s["dims"], s["origin"], s["voxel"], s["trunc"], [s["depths"][i] for i in part], [s["keeps"][i] for i in part], [s["imgs"][i] for i in part],
                           tr.SPHERE_K4, s["R"][part], s["t"][part], *vol)
    assert all(_same(a, b) for a, b in zip(vol, s["vol"]))


def test_two_runs_give_the_same_bytes(ctx, sphere, sphere_mesh):
    s = sphere
    again = _integrate(ctx, s["dims"], s["origin"], s["voxel"], s["trunc"], s["depths"], s["keeps"], s["imgs"], tr.SPHERE_K4, s["R"], s["t"])
    assert all(_same(a, b) for a, b in zip(again, s["vol"]))
    xyz, bgr, tri, _, _ = ctx.tsdf_mesh(s["dims"], s["origin"], s["voxel"], *s["vol"], 1)
    assert _same(xyz, sphere_mesh[0]) and _same(bgr, sphere_mesh[1]) and _same(tri, sphere_mesh[2])


def test_dev_forms_on_resident_arrays_equal_the_host_forms(ctx, sphere, sphere_mesh):
    import torch
    s = sphere
    dev = torch.device("cuda", ctx.device)
    nvox = 24 ** 3
    d_depth = [torch.from_numpy(x).to(dev) for x in s["depths"]]; d_keep = [torch.from_numpy(x).to(dev) for x in s["keeps"]]
    d_img = [torch.from_numpy(x).to(dev) for x in s["imgs"]]
    d_d = torch.zeros(nvox, dtype=torch.int32, device=dev); d_w = torch.zeros(nvox, dtype=torch.int32, device=dev)
    d_c = torch.zeros((nvox, 3), dtype=torch.int32, device=dev)
    for sl in (slice(0, 8), slice(8, 14)):
        ctx.tsdf_integrate_dev(s["dims"], s["origin"], s["voxel"], s["trunc"], d_depth[sl], d_keep[sl], d_img[sl], 96, 96, 3, 288, tr.SPHERE_K4, s["R"][sl], s["t"][sl],
                               d_d, d_w, d_c)
    nv, nt = len(sphere_mesh[0]), len(sphere_mesh[2])
    xyz = torch.zeros((nv, 3), dtype=torch.float64, device=dev); bgr = torch.zeros((nv, 3), dtype=torch.uint8, device=dev)
    tri = torch.zeros((nt, 3), dtype=torch.int32, device=dev); n = torch.zeros(2, dtype=torch.int32, device=dev)
    ctx.tsdf_mesh_dev(s["dims"], s["origin"], s["voxel"], d_d, d_w, d_c, 1, xyz, bgr, nv, tri, nt, n[0:1], n[1:2])
    ctx.synchronize()
    assert _same(d_d.cpu().numpy(), s["vol"][0]) and _same(d_w.cpu().numpy(), s["vol"][1]) and _same(d_c.cpu().numpy().view(np.uint32), s["vol"][2])
    assert n.cpu().numpy().tolist() == [nv, nt]
    assert _same(xyz.cpu().numpy(), sphere_mesh[0]) and _same(bgr.cpu().numpy(), sphere_mesh[1]) and _same(tri.cpu().numpy(), sphere_mesh[2])


# ------------------------------------------------------------------------------------------------ caps, errors
def test_caps_below_the_counts_write_only_the_prefix(ctx, sphere, sphere_mesh):
    s = sphere
    exyz, ebgr, etri = sphere_mesh
    vcap, tcap = len(exyz) // 3, len(etri) // 2 + 1
    xyz = np.full((vcap + 1, 3), -7.0); bgr = np.full((vcap + 1, 3), 0xCD, np.uint8); tri = np.full((tcap + 1, 3), -9, np.int32)
    nv, nt = C.c_int32(-1), C.c_int32(-1)
    dims = np.array(s["dims"], np.int32); origin = np.array(s["origin"]); d, w, c = s["vol"]
    rc = ctx.lib.sfmhip_tsdf_mesh(ctx.h, dims.ctypes.data, origin.ctypes.data, s["voxel"], d.ctypes.data, w.ctypes.data, c.ctypes.data, 1, xyz.ctypes.data, bgr.ctypes.data,
                                  vcap, tri.ctypes.data, tcap, C.byref(nv), C.byref(nt))
    assert rc == 0 and (nv.value, nt.value) == (len(exyz), len(etri)) and vcap > 100 and tcap > 100
    assert _same(xyz[:vcap], exyz[:vcap]) and _same(bgr[:vcap], ebgr[:vcap]) and _same(tri[:tcap], etri[:tcap])
    assert (xyz[vcap] == -7.0).all() and (bgr[vcap] == 0xCD).all() and (tri[tcap] == -9).all()
    x0, b0, t0, n0, m0 = ctx.tsdf_mesh(s["dims"], s["origin"], s["voxel"], d, w, c, 1, vertex_cap=0, triangle_cap=0)
    assert (n0, m0) == (len(exyz), len(etri)) and len(x0) == 0 and len(b0) == 0 and len(t0) == 0


def _raw_integrate(ctx, s, **over):
    """sfmhip_tsdf_integrate straight through ctypes on a volume that holds a sentinel: (rc, volume untouched)"""
    n = 2
    a = dict(dims=np.array(s["dims"], np.int32), origin=np.array(s["origin"]), voxel=s["voxel"], trunc=s["trunc"], depth=[x.ctypes.data for x in s["depths"][:n]],
             keep=[x.ctypes.data for x in s["keeps"][:n]], img=[x.ctypes.data for x in s["imgs"][:n]], n_views=n, rows=96, cols=96, channels=3, ld=288,
             K4=np.array(tr.SPHERE_K4), R=np.ascontiguousarray(s["R"][:n]), t=np.ascontiguousarray(s["t"][:n]), dsum=True, wsum=True, csum=True)
    a.update(over)
    nvox = 24 ** 3
    d = np.full(nvox, 5, np.int32); w = np.full(nvox, 6, np.int32); c = np.full((nvox, 3), 7, np.uint32)

    def arr(x):
        return None if x is None else (C.c_void_p * 8)(*x)

    def ptr(x):
        return None if x is None else x.ctypes.data
    rc = ctx.lib.sfmhip_tsdf_integrate(ctx.h, ptr(a["dims"]), ptr(a["origin"]), a["voxel"], a["trunc"], arr(a["depth"]), arr(a["keep"]), arr(a["img"]), a["n_views"], a["rows"],
                                       a["cols"], a["channels"], a["ld"], ptr(a["K4"]), ptr(a["R"]), ptr(a["t"]), d.ctypes.data if a["dsum"] else None,
                                       w.ctypes.data if a["wsum"] else None, c.ctypes.data if a["csum"] else None)
    return rc, bool((d == 5).all() and (w == 6).all() and (c == 7).all())


def test_bad_arguments_leave_the_outputs_alone(ctx, sphere):
    s = sphere
    assert _raw_integrate(ctx, s) == (0, False)
    assert _raw_integrate(ctx, s, keep=None)[0] == 0 and _raw_integrate(ctx, s, keep=[None, s["keeps"][1].ctypes.data])[0] == 0
    assert _raw_integrate(ctx, s, img=None, csum=False, channels=7, ld=0)[0] == 0             # without images their layout is not read
    one = s["depths"][0].ctypes.data
    bad = [dict(dims=None), dict(origin=None), dict(depth=None), dict(depth=[one, None]), dict(K4=None), dict(R=None), dict(t=None), dict(dsum=False), dict(wsum=False),
           dict(img=None), dict(csum=False), dict(img=[s["imgs"][0].ctypes.data, None]), dict(dims=np.array([0, 24, 24], np.int32)), dict(dims=np.array([24, -1, 24], np.int32)),
           dict(dims=np.array([1024, 1024, 257], np.int32)), dict(dims=np.array([1 << 20, 1 << 20, 1 << 20], np.int32)), dict(n_views=0), dict(n_views=9), dict(rows=0),
           dict(cols=0), dict(rows=16385), dict(cols=16385), dict(channels=2), dict(channels=4), dict(ld=287), dict(voxel=0.0), dict(voxel=-1.0), dict(voxel=float("inf")),
           dict(voxel=float("nan")), dict(trunc=0.0), dict(trunc=-0.1), dict(trunc=float("inf")), dict(trunc=float("nan")),
           dict(origin=np.array([0.0, float("nan"), 0.0]))]
    for over in bad:
        assert _raw_integrate(ctx, s, **over) == (_lib.E_ARG, True), {k: (v if not isinstance(v, np.ndarray) else v.tolist()) for k, v in over.items()}
    # the extraction
    dims = np.array(s["dims"], np.int32); origin = np.array(s["origin"]); d, w, c = s["vol"]
    xyz = np.full((50, 3), -7.0); bgr = np.full((50, 3), 0xCD, np.uint8); tri = np.full((50, 3), -9, np.int32)
    nv, nt = C.c_int32(-5), C.c_int32(-6)

    def mesh(dims_p=dims.ctypes.data, origin_p=origin.ctypes.data, voxel=s["voxel"], d_p=d.ctypes.data, w_p=w.ctypes.data, c_p=c.ctypes.data, mw=1, x=xyz.ctypes.data,
             b=bgr.ctypes.data, vcap=50, t=tri.ctypes.data, tcap=50, pv=C.byref(nv), pt=C.byref(nt)):
        return ctx.lib.sfmhip_tsdf_mesh(ctx.h, dims_p, origin_p, voxel, d_p, w_p, c_p, mw, x, b, vcap, t, tcap, pv, pt)
    zero = np.array([24, 0, 24], np.int32); huge = np.array([1024, 1024, 257], np.int32)
    for kw in (dict(dims_p=None), dict(origin_p=None), dict(d_p=None), dict(w_p=None), dict(pv=None), dict(pt=None), dict(dims_p=zero.ctypes.data), dict(dims_p=huge.ctypes.data),
               dict(mw=0), dict(mw=-1), dict(vcap=-1), dict(tcap=-1), dict(c_p=None), dict(voxel=0.0), dict(voxel=float("nan"))):
        assert mesh(**kw) == _lib.E_ARG, kw
    assert (xyz == -7.0).all() and (bgr == 0xCD).all() and (tri == -9).all() and (nv.value, nt.value) == (-5, -6)
    assert mesh(c_p=None, b=None) == 0 and nv.value > 50 and (bgr == 0xCD).all() and not (xyz == -7.0).any()


def test_a_failed_allocation_is_an_error_and_the_next_call_works(ctx, sphere, sphere_mesh):
    s = sphere
    for failing in (1, 2):                                                                     # the next `failing` allocations fail
        assert ctx.lib.sfmhip_debug_fail_allocations(ctx.h, failing) == 0
        for _ in range(failing):
            assert _raw_integrate(ctx, s) == (_lib.E_HIP, True)
        assert _raw_integrate(ctx, s) == (0, False)
    assert ctx.lib.sfmhip_debug_fail_allocations(ctx.h, 1) == 0
    with pytest.raises(api.SfmHipError):
        ctx.tsdf_mesh(s["dims"], s["origin"], s["voxel"], *s["vol"], 1, vertex_cap=10, triangle_cap=10)
    xyz, bgr, tri, _, _ = ctx.tsdf_mesh(s["dims"], s["origin"], s["voxel"], *s["vol"], 1)
    assert _same(xyz, sphere_mesh[0]) and _same(bgr, sphere_mesh[1]) and _same(tri, sphere_mesh[2])


# ------------------------------------------------------------------------------------------------ the layers above
@pytest.fixture(scope="module")
def scene_mesh(ctx, planted):
    p = planted
    return api.dense_mesh_for_all(p["images"], p["sc"].K4, p["sc"].EXT, n_src=N_SRC, planes=PLANES, radius=2, wmin=WMIN, wmax=WMAX, min_score=-1.0, rel_tol=0.01,
                                  min_consistent=2, ctx=ctx, trunc_voxels=SCENE_TRUNC_VOXELS, min_weight=SCENE_MIN_WEIGHT, volume=SCENE_VOLUME)


def test_dense_mesh_for_all_equals_the_restatement_chain(planted, scene_mesh):
    p = planted
    dims, origin, voxel = SCENE_VOLUME
    vol = tr.new_volume(dims)
    tr.integrate(dims, origin, voxel, SCENE_TRUNC_VOXELS * voxel, [e["depth"] for e in p["exp"]], [e["keep"] for e in p["exp"]], p["images"], p["sc"].K4, p["R"], p["t"], *vol)
    exyz, ebgr, etri = tr.mesh(dims, origin, voxel, *vol, SCENE_MIN_WEIGHT)
    xyz, bgr, tri = scene_mesh
    assert _same(xyz, exyz) and _same(bgr, ebgr) and _same(tri, etri)
    near = p["sc"].plane_distance(exyz) <= 1.5 * voxel
    print(f"{len(xyz)} vertices, {len(tri)} triangles, {near.mean():.4f} within 1.5 voxels of a planted plane")
    assert len(tri) > 500 and (p["sc"].plane_distance(xyz) <= 1.5 * voxel).mean() == near.mean() > 0.5


def test_tsdf_bounds_encloses_the_trimmed_cloud():
    rng = np.random.default_rng(2)
    sparse = np.stack([rng.uniform(-1.5, 1.5, 400), rng.uniform(-1, 1, 400), rng.uniform(3.9, 6.4, 400)], 1)
    sparse[0] = (1e6, 0, 0); sparse[1] = np.nan
    dims, origin, voxel = api.tsdf_bounds(sparse, 64, 0.1)
    lo = np.array(origin); hi = lo + np.array(dims) * voxel
    inside = np.isfinite(sparse).all(1) & (sparse >= lo).all(1) & (sparse <= hi).all(1)
    assert max(dims) == 64 and min(dims) >= 2 and inside.sum() >= 0.9 * 398 and hi[0] < 10 and voxel > 0


def test_mesh_ply_round_trip(scene_mesh, tmp_path):
    xyz, bgr, tri = scene_mesh
    path = tmp_path / "mesh.ply"
    formats.write_mesh_ply(path, xyz, bgr, tri)
    raw = open(path, "rb").read()
    assert raw.startswith(b"ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % len(xyz)) and b"property list uchar int vertex_indices\nend_header\n" in raw
    x2, b2, t2 = formats.read_mesh_ply(path)
    assert _same(x2, xyz.astype(np.float32)) and _same(b2, bgr) and _same(t2, tri)


def test_cpp_mirror_writes_the_same_mesh_file(planted, scene_mesh, tmp_path):
    p = planted
    sc = p["sc"]
    host = os.path.join(HERE, "host")
    subprocess.check_call(["make", "-C", host, "-f", "tsdf.mk", "tsdf_test"], stdout=subprocess.DEVNULL)
    dims, origin, voxel = SCENE_VOLUME
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<10i", 4, sc.ROWS, sc.COLS, 1, N_SRC, PLANES, 2, 1, 2, 0)); f.write(struct.pack("<5d", WMIN, WMAX, -1.0, 0.01, 0.0))
        f.write(struct.pack("<5i", *dims, SCENE_MIN_WEIGHT, 0)); f.write(struct.pack("<5d", *origin, voxel, float(SCENE_TRUNC_VOXELS)))
        f.write(np.array(sc.K4).tobytes()); f.write(np.ascontiguousarray(sc.EXT).tobytes())
        for im in p["images"]:
            f.write(im.tobytes())
    out = subprocess.run([os.path.join(host, "tsdf_test"), str(tmp_path / "in.bin"), str(tmp_path / "out.ply")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert open(tmp_path / "out.ply", "rb").read() == formats.mesh_ply_bytes(*scene_mesh)
