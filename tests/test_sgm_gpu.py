"""GPU: the semi-global path of the dense step (sfmhip_sweep_costs, sfmhip_sgm_depth, sfmhip_plane_sweep_sgm) against the numpy
restatement of its definition (tests/sgm_ref.py): every output byte is equal, the aggregated volume S included.  Then the edges of the
path kernels (plane counts around the wave size, images of one row or column, long thin images), determinism, the entry forms, the
argument rules, an injected allocation failure, and the layers above (api.dense_cloud_for_all(sgm=...) and its C++ mirror)."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import dense_ref as dr
import sgm_ref as sr
from sfm_opencv_amd import _lib, api

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
WMIN, WMAX = 1.0 / 8.0, 1.0 / 3.0
D, R, SCALE, P1, P2 = 48, 1, 262144.0, 512, 4096
NAMES = ("plane", "cost", "sum", "depth", "S")


def _same(a, b):
    a = np.asarray(a); b = np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _check_sgm(ctx, vol, p1, p2, paths, max_cost=65535, wmin=WMIN, wmax=WMAX):
    got = ctx.sgm_depth(vol, wmin, wmax, p1, p2, paths, max_cost, return_sums=True)
    exp = sr.sgm_depth(vol, wmin, wmax, p1, p2, paths, max_cost)
    for name, g, e in zip(NAMES, got, exp):
        assert _same(g, e), (name, vol.shape, paths, int((g != e).sum()))
    return got


def _volume(rng, rows, cols, planes, shift=0):
    """random costs, about a tenth of them 65535 (not scored) and some 65534 (the clamp)"""
    vol = (rng.integers(0, 65535, (rows, cols, planes)) >> shift).astype(np.uint16)
    u = rng.random(vol.shape)
    vol[u < 0.10] = 65535
    vol[(u >= 0.10) & (u < 0.13)] = 65534
    return vol


# ------------------------------------------------------------------------------------------------ the planted scene
@pytest.fixture(scope="module")
def scene():
    sc = dr.Scene()
    return sc, [sc.render(v)[0] for v in range(4)]


@pytest.fixture(scope="module")
def planted(ctx, scene):
    """view 0 against views 1 and 2 at 96 x 72, 48 planes, r = 1: the library's cost volume and the restatement's, computed once"""
    sc, images = scene
    A, b, *_ = api.sweep_geometry(sc.K4, sc.EXT[0], sc.EXT[1:3])
    exp = sr.sweep_costs(images[0], images[1:3], A, b, D, WMIN, WMAX, R, 1, SCALE)
    got = ctx.sweep_costs(images[0], images[1:3], A, b, D, WMIN, WMAX, R, 1, SCALE)
    return A, b, exp, got


def test_cost_volume_of_the_planted_scene(planted):
    _, _, exp, got = planted
    assert _same(got, exp), int((got != exp).sum())
    assert (exp != 65535).mean() > 0.8 and (exp[1:-1, 1:-1] == 65535).any() and len(np.unique(exp)) > 1000     # not an empty case


@pytest.mark.parametrize("paths", [4, 8])
def test_planted_scene_equals_the_restatement(ctx, scene, planted, paths):
    sc, images = scene
    A, b, exp, _ = planted
    plane, cost, _, depth, _ = _check_sgm(ctx, exp, P1, P2, paths)
    fused = ctx.plane_sweep_sgm(images[0], images[1:3], A, b, D, WMIN, WMAX, R, 1, SCALE, P1, P2, paths, 65535)
    for name, g, e in zip(("plane", "cost", "depth"), fused, (plane, cost, depth)):
        assert _same(g, e), (name, paths)
    assert (plane >= 0).mean() > 0.8
    # a max_cost that cuts some winners and not all
    cut = ctx.plane_sweep_sgm(images[0], images[1:3], A, b, D, WMIN, WMAX, R, 1, SCALE, P1, P2, paths, 2000)
    ecut = sr.plane_sweep_sgm(images[0], images[1:3], A, b, D, WMIN, WMAX, R, 1, SCALE, P1, P2, paths, 2000)
    assert all(_same(g, e) for g, e in zip(cut, ecut)) and 100 < (cut[0] >= 0).sum() < (plane >= 0).sum() - 100


# ------------------------------------------------------------------------------------------------ random volumes at the kernels' edges
IMAGES = [(1, 1), (1, 37), (37, 1), (9, 7), (33, 65), (300, 5), (5, 300)]


@pytest.mark.parametrize("planes", [2, 63, 64, 65, 128, 129, 256])
def test_random_volumes(ctx, planes):
    """plane counts around the 64 lanes of a wave (one to four planes per lane, lanes past the last plane); images of one pixel, one row,
    one column, and long thin ones with many short lines one way and few long lines the other"""
    rng = np.random.default_rng(planes)
    for i, (rows, cols) in enumerate(IMAGES):
        vol = _volume(rng, rows, cols, planes, shift=(0, 5)[i % 2])
        for paths in (4, 8):
            _check_sgm(ctx, vol, 700 >> (5 * (i % 2)), 9000 >> (5 * (i % 2)), paths)


def test_the_largest_penalties(ctx):
    rng = np.random.default_rng(1)
    vol = _volume(rng, 33, 65, 65)
    got = _check_sgm(ctx, vol, 65535, 65535, 8)
    assert got[4].max() > 8 * 65535                                # sums past 19 bits


def test_a_constant_volume_takes_plane_zero_without_a_fit(ctx):
    vol = np.full((9, 7, 65), 1234, np.uint16)
    plane, cost, ssum, depth, S = _check_sgm(ctx, vol, 10, 100, 8)
    assert (plane == 0).all() and (cost == 1234).all() and (S == 8 * 1234).all() and (depth == np.float32(1.0 / WMIN)).all()
    vol[:, :, 0] = 2000                                            # an interior winner on a flat floor: den = 0, no fit either
    vol[:, :, 3] = 1000
    plane, _, _, depth, _ = _check_sgm(ctx, vol, 0, 0, 4)
    assert (plane == 3).all() and len(np.unique(depth)) == 1


def test_a_pixel_with_every_plane_unscored(ctx):
    rng = np.random.default_rng(2)
    vol = _volume(rng, 9, 7, 64, shift=5)
    vol[4, 3, :] = 65535; vol[0, 0, :] = 65535; vol[8, :, :] = 65535
    plane, cost, ssum, depth, _ = _check_sgm(ctx, vol, 20, 300, 8)
    for at in ((4, 3), (0, 0), (8, 5)):
        assert plane[at] == -1 and cost[at] == 65535 and ssum[at] == 0 and np.isnan(depth[at])
    assert (plane[:8] >= 0).sum() == 8 * 7 - 2


def test_max_cost_below_every_cost(ctx):
    rng = np.random.default_rng(3)
    vol = np.maximum(_volume(rng, 9, 7, 65, shift=5), 50).astype(np.uint16)
    plane, cost, ssum, depth, S = _check_sgm(ctx, vol, 20, 300, 8, max_cost=49)
    assert (plane == -1).all() and (cost == 65535).all() and (ssum == 0).all() and np.isnan(depth).all() and S.min() >= 8 * 50
    assert (_check_sgm(ctx, vol, 20, 300, 8, max_cost=50)[0] >= 0).any()


# ------------------------------------------------------------------------------------------------ the cost kernel at its edges
@pytest.mark.parametrize("planes", [16, 17])
def test_costs_at_odd_sizes(ctx, planes):
    """71 x 97 is no multiple of a tile; 17 planes are no multiple of the plane group and take the 16-bit stores, 16 the 8-byte store"""
    sc = dr.Scene()
    images = [sc.render(v, rows=71, cols=97)[0] for v in range(3)]
    A, b, *_ = api.sweep_geometry(sc.K4, sc.EXT[0], sc.EXT[1:3])
    got = ctx.sweep_costs(images[0], images[1:], A, b, planes, WMIN, WMAX, 2, 1, 4096.0)
    exp = sr.sweep_costs(images[0], images[1:], A, b, planes, WMIN, WMAX, 2, 1, 4096.0)
    assert _same(got, exp) and (exp != 65535).mean() > 0.5
    two = ctx.sweep_costs(images[0], images[1:], A, b, planes, WMIN, WMAX, 2, 2, 4096.0)
    assert _same(two, sr.sweep_costs(images[0], images[1:], A, b, planes, WMIN, WMAX, 2, 2, 4096.0)) and (two == 65535).sum() > (exp == 65535).sum()


def test_costs_of_padded_rows_and_of_an_image_smaller_than_the_window(ctx, scene, planted):
    sc, images = scene
    A, b, exp, _ = planted
    rows, cols = images[0].shape
    bufs = [np.full((rows, cols + 13), 0xAB, np.uint8) for _ in range(3)]
    for buf, im in zip(bufs, images):
        buf[:, :cols] = im
    views = [buf[:, :cols] for buf in bufs]
    assert api._dense_images(views)[5] == cols + 13                      # passed where they lie
    assert _same(ctx.sweep_costs(views[0], views[1:], A, b, D, WMIN, WMAX, R, 1, SCALE), exp)
    assert all((buf[:, cols:] == 0xAB).all() for buf in bufs)
    rng = np.random.default_rng(4)
    small = [rng.integers(0, 256, (4, 40), dtype=np.uint8) for _ in range(3)]
    assert (ctx.sweep_costs(small[0], small[1:], A, b, 4, WMIN, WMAX, 2, 1, SCALE) == 65535).all()
    fused = ctx.plane_sweep_sgm(small[0], small[1:], A, b, 4, WMIN, WMAX, 2)
    assert (fused[0] == -1).all() and (fused[1] == 65535).all() and np.isnan(fused[2]).all()


# ------------------------------------------------------------------------------------------------ determinism and entry forms
def test_two_runs_give_the_same_bytes(ctx, scene, planted):
    sc, images = scene
    A, b, exp, got = planted
    assert _same(ctx.sweep_costs(images[0], images[1:3], A, b, D, WMIN, WMAX, R, 1, SCALE), got)
    one = ctx.sgm_depth(exp, WMIN, WMAX, P1, P2, 8, 65535, return_sums=True)
    two = ctx.sgm_depth(exp, WMIN, WMAX, P1, P2, 8, 65535, return_sums=True)
    assert all(_same(x, y) for x, y in zip(one, two))
    f1 = ctx.plane_sweep_sgm(images[0], images[1:3], A, b, D, WMIN, WMAX, R, 1, SCALE, P1, P2, 8, 65535)
    f2 = ctx.plane_sweep_sgm(images[0], images[1:3], A, b, D, WMIN, WMAX, R, 1, SCALE, P1, P2, 8, 65535)
    assert all(_same(x, y) for x, y in zip(f1, f2))


def test_dev_forms_on_resident_arrays_equal_the_host_forms(ctx, scene, planted):
    import torch
    sc, images = scene
    A, b, exp, _ = planted
    rows, cols = images[0].shape
    dev = torch.device("cuda", ctx.device)
    d_img = [torch.from_numpy(im).to(dev) for im in images[:3]]
    host = ctx.sgm_depth(exp, WMIN, WMAX, P1, P2, 8, 65535, return_sums=True)

    def u16(t):
        return t.cpu().numpy().view(np.uint16)

    # the volume at an address that is a multiple of 8 bytes, and at one that is not (the cost kernel then stores 16 bits at a time)
    room = torch.zeros(rows * cols * D + 1, dtype=torch.int16, device=dev)
    for off in (0, 1):
        d_vol = room[off:off + rows * cols * D]
        d_vol.fill_(-1)
        ctx.sweep_costs_dev(d_img[0], d_img[1:], rows, cols, 1, cols, A, b, D, WMIN, WMAX, R, 1, SCALE, d_vol)
        ctx.synchronize()
        assert _same(u16(d_vol).reshape(rows, cols, D), exp), off
    plane = torch.empty((rows, cols), dtype=torch.int32, device=dev); cost = torch.empty((rows, cols), dtype=torch.int16, device=dev)
    ssum = torch.empty((rows, cols), dtype=torch.int32, device=dev); depth = torch.empty((rows, cols), dtype=torch.float32, device=dev)
    S = torch.empty((rows, cols, D), dtype=torch.int32, device=dev)
    ctx.sgm_depth_dev(d_vol, rows, cols, D, WMIN, WMAX, P1, P2, 8, 65535, plane, cost, ssum, depth, S)
    ctx.synchronize()
    got = (plane.cpu().numpy(), u16(cost), ssum.cpu().numpy().view(np.uint32), depth.cpu().numpy(), S.cpu().numpy().view(np.uint32))
    assert all(_same(g, h) for g, h in zip(got, host))
    # outputs that are not asked for, and the sums from the block cache
    depth.fill_(0.0)
    ctx.sgm_depth_dev(d_vol, rows, cols, D, WMIN, WMAX, P1, P2, 8, 65535, None, None, None, depth, None)
    ctx.synchronize()
    assert _same(depth.cpu().numpy(), host[3])
    plane.fill_(7); cost.fill_(7); depth.fill_(7.0)
    ctx.plane_sweep_sgm_dev(d_img[0], d_img[1:], rows, cols, 1, cols, A, b, D, WMIN, WMAX, R, 1, SCALE, P1, P2, 8, 65535, plane, cost, depth)
    ctx.synchronize()
    assert _same(plane.cpu().numpy(), host[0]) and _same(u16(cost), host[1]) and _same(depth.cpu().numpy(), host[3])


# ------------------------------------------------------------------------------------------------ errors
def _raw_fused(ctx, images, geo_A, geo_b, **over):
    """sfmhip_plane_sweep_sgm straight through ctypes with outputs that hold a sentinel: (rc, outputs untouched)"""
    rows, cols = images[0].shape[:2]
    a = dict(ref=images[0].ctypes.data, src=[im.ctypes.data for im in images[1:]], n_src=len(images) - 1, rows=rows, cols=cols, channels=1, ld=cols, A=geo_A.ctypes.data,
             b=geo_b.ctypes.data, D=8, wmin=WMIN, wmax=WMAX, r=2, min_sources=1, scale=SCALE, P1=P1, P2=P2, paths=8, max_cost=65535, plane=True, cost=True, depth=True)
    a.update(over)
    plane = np.full((rows, cols), 77, np.int32); cost = np.full((rows, cols), 5, np.uint16); depth = np.full((rows, cols), 6.0, np.float32)
    src = (C.c_void_p * 8)(*a["src"]) if a["src"] is not None else None
    rc = ctx.lib.sfmhip_plane_sweep_sgm(ctx.h, a["ref"], src, a["n_src"], a["rows"], a["cols"], a["channels"], a["ld"], a["A"], a["b"], a["D"], a["wmin"], a["wmax"],
                                        a["r"], a["min_sources"], a["scale"], a["P1"], a["P2"], a["paths"], a["max_cost"], plane.ctypes.data if a["plane"] else None,
                                        cost.ctypes.data if a["cost"] else None, depth.ctypes.data if a["depth"] else None)
    return rc, bool((plane == 77).all() and (cost == 5).all() and (depth == 6.0).all())


SWEEP_BAD = [dict(ref=None), dict(src=None), dict(A=None), dict(b=None), dict(n_src=0), dict(n_src=9), dict(rows=0), dict(cols=16385), dict(channels=2), dict(ld=1),
             dict(D=1), dict(D=257), dict(wmin=WMAX, wmax=WMIN), dict(wmin=0.0), dict(wmax=float("inf")), dict(wmin=float("nan")), dict(r=-1), dict(r=6),
             dict(min_sources=0), dict(scale=0.0), dict(scale=-1.0), dict(scale=float("inf")), dict(scale=float("nan"))]
SGM_BAD = [dict(P1=-1), dict(P1=P2 + 1), dict(P2=65536), dict(paths=0), dict(paths=5), dict(paths=16), dict(max_cost=-1), dict(max_cost=65536)]


def test_bad_arguments_leave_the_outputs_alone(ctx, scene):
    sc, images = scene
    A, b, *_ = api.sweep_geometry(sc.K4, sc.EXT[0], sc.EXT[1:3])
    ims = images[:3]
    rows, cols = ims[0].shape
    assert _raw_fused(ctx, ims, A, b) == (0, False)
    for over in SWEEP_BAD + SGM_BAD + [dict(src=[ims[1].ctypes.data, None]), dict(plane=False), dict(cost=False), dict(depth=False)]:
        assert _raw_fused(ctx, ims, A, b, **over) == (_lib.E_ARG, True), over
    # the cost volume alone
    vol = np.full((rows, cols, 8), 9, np.uint16)
    src = (C.c_void_p * 8)(ims[1].ctypes.data, ims[2].ctypes.data)

    def costs(ref=ims[0].ctypes.data, src=src, n_src=2, rows=rows, cols=cols, channels=1, ld=cols, A=A.ctypes.data, b=b.ctypes.data, D=8, wmin=WMIN, wmax=WMAX, r=2,
              min_sources=1, scale=SCALE, out=vol.ctypes.data):
        return ctx.lib.sfmhip_sweep_costs(ctx.h, ref, src, n_src, rows, cols, channels, ld, A, b, D, wmin, wmax, r, min_sources, scale, out)
    for over in SWEEP_BAD + [dict(out=None)]:
        assert costs(**over) == _lib.E_ARG, over
    assert (vol == 9).all()
    assert costs() == 0 and not (vol == 9).all()
    # the aggregation alone
    outs = [np.full((rows, cols), 77, np.int32), np.full((rows, cols), 5, np.uint16), np.full((rows, cols), 3, np.uint32), np.full((rows, cols), 6.0, np.float32),
            np.full((rows, cols, 8), 4, np.uint32)]

    def sgm(cost=vol.ctypes.data, rows=rows, cols=cols, D=8, wmin=WMIN, wmax=WMAX, P1=P1, P2=P2, paths=8, max_cost=65535, ptrs=tuple(o.ctypes.data for o in outs)):
        return ctx.lib.sfmhip_sgm_depth(ctx.h, cost, rows, cols, D, wmin, wmax, P1, P2, paths, max_cost, *ptrs)
    for over in SGM_BAD + [dict(cost=None), dict(rows=0), dict(cols=0), dict(rows=16385), dict(D=1), dict(D=257), dict(wmin=WMAX, wmax=WMIN), dict(wmin=-1.0),
                           dict(wmax=float("nan")), dict(ptrs=(None, None, None, None, outs[4].ctypes.data))]:
        assert sgm(**over) == _lib.E_ARG, over
    assert (outs[0] == 77).all() and (outs[1] == 5).all() and (outs[2] == 3).all() and (outs[3] == 6.0).all() and (outs[4] == 4).all()
    assert sgm(ptrs=(outs[0].ctypes.data, None, None, None, None)) == 0
    assert not (outs[0] == 77).any() and (outs[1] == 5).all() and (outs[4] == 4).all()
    assert _same(outs[0], sr.sgm_depth(vol, WMIN, WMAX, P1, P2, 8, 65535)[0])


def test_a_failed_allocation_is_an_error_and_the_next_call_works(ctx, scene, planted):
    import torch
    sc, images = scene
    A, b, exp, _ = planted
    ims = images[:3]
    good = ctx.plane_sweep_sgm(ims[0], ims[1:], A, b, 8, WMIN, WMAX, 2, 1, SCALE, P1, P2, 8, 65535)
    for failing in (1, 2):
        assert ctx.lib.sfmhip_debug_fail_allocations(ctx.h, failing) == 0
        for _ in range(failing):
            rc, untouched = _raw_fused(ctx, ims, A, b)
            assert rc == _lib.E_HIP and untouched
        again = ctx.plane_sweep_sgm(ims[0], ims[1:], A, b, 8, WMIN, WMAX, 2, 1, SCALE, P1, P2, 8, 65535)
        assert all(_same(x, y) for x, y in zip(again, good))
    assert ctx.lib.sfmhip_debug_fail_allocations(ctx.h, 1) == 0
    with pytest.raises(api.SfmHipError):
        ctx.sweep_costs(ims[0], ims[1:], A, b, D, WMIN, WMAX, R, 1, SCALE)
    assert ctx.lib.sfmhip_debug_fail_allocations(ctx.h, 1) == 0
    with pytest.raises(api.SfmHipError):
        ctx.sgm_depth(exp, WMIN, WMAX, P1, P2, 8)
    # the enqueue-only form takes its volumes before it enqueues anything
    rows, cols = ims[0].shape
    dev = torch.device("cuda", ctx.device)
    d_img = [torch.from_numpy(im).to(dev) for im in ims]
    plane = torch.full((rows, cols), 7, dtype=torch.int32, device=dev); cost = torch.full((rows, cols), 7, dtype=torch.int16, device=dev)
    depth = torch.full((rows, cols), 7.0, dtype=torch.float32, device=dev)
    assert ctx.lib.sfmhip_debug_fail_allocations(ctx.h, 2) == 0
    for _ in range(2):
        with pytest.raises(api.SfmHipError):
            ctx.plane_sweep_sgm_dev(d_img[0], d_img[1:], rows, cols, 1, cols, A, b, 8, WMIN, WMAX, 2, 1, SCALE, P1, P2, 8, 65535, plane, cost, depth)
    ctx.synchronize()
    assert bool((plane == 7).all()) and bool((cost == 7).all()) and bool((depth == 7.0).all())
    ctx.plane_sweep_sgm_dev(d_img[0], d_img[1:], rows, cols, 1, cols, A, b, 8, WMIN, WMAX, 2, 1, SCALE, P1, P2, 8, 65535, plane, cost, depth)
    ctx.synchronize()
    assert _same(plane.cpu().numpy(), good[0]) and _same(cost.cpu().numpy().view(np.uint16), good[1]) and _same(depth.cpu().numpy(), good[2])
    assert _same(ctx.sgm_depth(exp, WMIN, WMAX, P1, P2, 8)[0], sr.sgm_depth(exp, WMIN, WMAX, P1, P2, 8, 65535)[0])


# ------------------------------------------------------------------------------------------------ the layers above
CLOUD = dict(n_src=2, planes=32, radius=2, wmin=WMIN, wmax=WMAX, rel_tol=0.01, min_consistent=2)
SGM = (SCALE, P1, P2, 8, 60000)


@pytest.fixture(scope="module")
def cloud(ctx, scene):
    sc, images = scene
    return api.dense_cloud_for_all(images, sc.K4, sc.EXT, ctx=ctx, sgm=SGM, **CLOUD)


def test_dense_cloud_with_sgm_equals_the_chain_of_the_restatement(scene, cloud):
    sc, images = scene
    sources = dr.nearest_sources(sc.EXT, 2)
    exp = sr.chain(images, sc.K4, sc.EXT, sources, api.sweep_geometry, 32, WMIN, WMAX, 2, 1, SGM, 0.01, 2)
    xyz, bgr = cloud
    assert _same(xyz, np.concatenate([e["xyz"] for e in exp])) and _same(bgr, np.concatenate([e["bgr"] for e in exp]))
    assert len(xyz) >= 4 * 0.25 * sc.ROWS * sc.COLS
    assert (sc.plane_distance(xyz) <= 6.6 ** 2 * (WMAX - WMIN) / 31).mean() >= 0.98     # within a plane step, as tests/test_dense_cpu.py reasons


def test_dense_cloud_without_sgm_is_the_winner_per_pixel_as_before(ctx, scene, cloud):
    """the parent's output on these inputs is the chain of dense_ref in every bit (tests/test_dense_gpu.py holds it to that)"""
    sc, images = scene
    sources = dr.nearest_sources(sc.EXT, 2)
    exp = dr.chain(images, sc.K4, sc.EXT, sources, api.sweep_geometry, 32, WMIN, WMAX, 2, 1, -1.0, 0.01, 2)
    for kw in (dict(), dict(sgm=None)):
        xyz, bgr = api.dense_cloud_for_all(images, sc.K4, sc.EXT, ctx=ctx, min_score=-1.0, **CLOUD, **kw)
        assert _same(xyz, np.concatenate([e["xyz"] for e in exp])) and _same(bgr, np.concatenate([e["bgr"] for e in exp]))
    assert not _same(xyz, cloud[0])


def test_cpp_mirror_writes_the_same_cloud(scene, cloud, tmp_path):
    sc, images = scene
    host = os.path.join(HERE, "host")
    subprocess.check_call(["make", "-C", host, "-f", "sgm.mk", "sgm_test"], stdout=subprocess.DEVNULL)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<13i", 4, sc.ROWS, sc.COLS, 1, 2, 32, 2, 1, 2, SGM[1], SGM[2], SGM[3], SGM[4])); f.write(struct.pack("<4d", WMIN, WMAX, 0.01, SGM[0]))
        f.write(np.array(sc.K4).tobytes()); f.write(np.ascontiguousarray(sc.EXT).tobytes())
        for im in images:
            f.write(im.tobytes())
    out = subprocess.run([os.path.join(host, "sgm_test"), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    raw = open(tmp_path / "out.bin", "rb").read()
    (n,) = struct.unpack_from("<i", raw, 0)
    xyz = np.frombuffer(raw, "<f8", 3 * n, 4).reshape(-1, 3); bgr = np.frombuffer(raw, np.uint8, 3 * n, 4 + 24 * n).reshape(-1, 3)
    assert n == len(cloud[0]) and _same(xyz, cloud[0]) and _same(bgr, cloud[1])
