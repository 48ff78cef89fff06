"""GPU: DBSCAN / Euclidean clustering and the largest-cluster filter (sfmhip_cluster_dbscan, sfmhip_cluster_dbscan_dev,
sfmhip_largest_cluster) through the C-ABI, the Python layer and the NViewReconstruct driver.  The reference is tests/cluster_ref.py
(numpy + scipy, no union-find); labels, sizes and the number of clusters must equal it exactly, on every row, for every method."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cluster_ref as cr
import points_ref as pr
import radius_ref as rr
from sfm_opencv_amd import _lib, api, formats
from test_points_gpu import GOLD, HOST, METHODS, _cloud_and_ref
from test_radius_gpu import RADIUS_CLOUDS, _cloud

pytestmark = pytest.mark.gpu
_I32P = C.POINTER(C.c_int32)
MIN_POINTS = (1, 2, 5, 10)
_ref_cache = {}


def _ref(tag, pts, r, mp):
    """the reference's (labels, sizes, count), computed once per case; the candidate pairs of a large cloud once per radius"""
    if (tag, r, mp) not in _ref_cache:
        if len(pts) <= cr.ALLPAIRS_MAX:
            _ref_cache[(tag, r, mp)] = cr.cluster_allpairs(pts, r, mp)
        else:
            if (tag, r) not in _ref_cache:
                _ref_cache[(tag, r)] = cr.candidate_pairs(pts, r)
            _ref_cache[(tag, r, mp)] = cr.cluster_kdtree(pts, r, mp, pairs=_ref_cache[(tag, r)])
    return _ref_cache[(tag, r, mp)]


def _check(ctx, tag, pts, r, mp, methods=METHODS):
    labels, sizes, _ = _ref(tag, pts, r, mp)
    for method in methods:
        got, gsizes = ctx.cluster_dbscan(pts, r, mp, method)
        assert got.dtype == np.int32 and got.shape == (len(pts),) and gsizes.dtype == np.int32
        assert len(gsizes) == len(sizes), (tag, r, mp, method, len(gsizes), len(sizes))
        bad = np.flatnonzero(got != labels)
        assert len(bad) == 0, (tag, r, mp, method, len(bad), bad[:5], got[bad[:5]], labels[bad[:5]])
        assert np.array_equal(gsizes, sizes), (tag, r, mp, method)
    return labels, sizes


def _radii(name, pts):
    radii = (rr.radii_for_counts(pts) or [1.0]) + [0.0] + ([2e-3] if name == "far_clamped" else [])
    return list(dict.fromkeys(radii))


# ---- every cloud of the radius tests ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(RADIUS_CLOUDS))
def test_clusters_equal_the_reference_on_every_row(ctx, name):
    pts = _cloud(name)
    for r in _radii(name, pts):
        # a radius that takes in most of a large cloud: one setting is enough (and the reference's pair list stays small otherwise)
        whole = len(pts) > cr.ALLPAIRS_MAX and np.median(_ref(name, pts, r, 1)[2]) > len(pts) / 2
        for mp in (1,) if whole else MIN_POINTS:
            labels, sizes = _check(ctx, name, pts, r, mp)
            if len(pts):
                print(f"[cluster] {name}: r = {r:.6g}, min_points {mp}: {len(sizes)} clusters, largest {sizes.max() if len(sizes) else 0}, "
                      f"noise {(labels < 0).sum()}")
    if name == "far_clamped":                  # the clamped border cells link their companions: far points do sit in clusters of two or more
        labels, sizes, _ = _ref(name, pts, 2e-3, 2)
        far = labels[5000:]
        assert (far >= 0).sum() >= 100 and (sizes[far[far >= 0]] >= 2).all()


def test_lattice_and_ply_values(ctx):
    pts = pr.lattice(32)
    for r, mp, n_clusters, noise, largest in ((1.0, 1, 1, 0, 32768), (1.0, 7, 1, 368, 32400), (1.0, 6, 1, 8, 32760), (1.0, 8, 0, 32768, 0),
                                              (0.999999, 1, 32768, 0, 1), (float(np.sqrt(2.0)), 19, 1, 8, 32760)):
        labels, sizes = _check(ctx, "lattice_32", pts, r, mp)
        assert (len(sizes), int((labels < 0).sum()), int(sizes.max()) if len(sizes) else 0) == (n_clusters, noise, largest), (r, mp)
    ch = _cloud_and_ref("crazyhorse_ply")[0]
    for r, mp, n_clusters, largest in ((0.0, 1, 1456, 3), (0.0, 2, 92, 3), (0.2, 1, 246, 1011), (0.2, 5, 20, 1005), (1.0, 5, 9, 1384)):
        labels, sizes = _check(ctx, "crazyhorse_ply", ch, r, mp)
        assert (len(sizes), int(sizes.max())) == (n_clusters, largest), (r, mp)


# ---- shapes at which a union-find that loses a hook, reads a stale parent or propagates instead of hooking goes wrong ---------------
def _chain(n=50000, drop=None):
    x = np.arange(n, dtype=np.float64)
    if drop is not None:
        x = np.delete(x, drop)
    x = x[np.random.default_rng(41).permutation(len(x))]
    return np.stack([x, np.zeros_like(x), np.zeros_like(x)], axis=1)


def test_chain_of_50000_points(ctx):
    pts = _chain()
    labels, sizes = _check(ctx, "chain", pts, 1.0, 1)
    assert sizes.tolist() == [50000] and not labels.any()
    labels, sizes = _check(ctx, "chain", pts, 1.0, 3)
    _, _, count = _ref("chain", pts, 1.0, 3)
    assert sizes.tolist() == [50000] and cr.census(labels, count, pts, 3) == (49998, 2, 0)
    labels, sizes = _check(ctx, "chain", pts, 0.999999, 1)
    assert len(sizes) == 50000 and np.array_equal(labels, np.arange(50000))
    cut = _chain(drop=20000)
    labels, sizes = _check(ctx, "chain_cut", cut, 1.0, 1)
    assert sorted(sizes.tolist()) == [20000, 29999]
    assert np.array_equal(labels == labels[np.argmin(cut[:, 0])], cut[:, 0] < 20000)


def _helix(n=50000, radius=50.0, pitch=3.0, step=0.9):
    c = pitch / (2.0 * np.pi)
    theta = np.arange(n) * (step / np.hypot(radius, c))
    p = np.stack([radius * np.cos(theta), radius * np.sin(theta), c * theta], axis=1)
    return p[np.random.default_rng(43).permutation(n)]


def test_helix_of_50000_points(ctx):
    pts = _helix()
    labels, sizes = _check(ctx, "helix", pts, 1.0, 1)
    assert sizes.tolist() == [50000]
    labels, sizes = _check(ctx, "helix", pts, 0.85, 1)
    assert len(sizes) == 50000 and np.array_equal(labels, np.arange(50000))


def _dumbbell(drop=None):
    bar = np.stack([np.arange(8.0, 20.0), np.zeros(12), np.zeros(12)], axis=1)
    if drop is not None:
        bar = np.delete(bar, drop, axis=0)
    return np.concatenate([pr.lattice(8), pr.lattice(8) + np.array([20.0, 0.0, 0.0]), bar])


def test_dumbbell(ctx):
    pts = _dumbbell()
    assert len(pts) == 1036
    labels, sizes = _check(ctx, "dumbbell", pts, 1.0, 1)
    assert sizes.tolist() == [1036]
    labels, sizes = _check(ctx, "dumbbell", pts, 1.0, 4)
    _, _, count = _ref("dumbbell", pts, 1.0, 4)
    assert sizes.tolist() == [513, 513] and cr.census(labels, count, pts, 4) == (1024, 2, 10)
    for method in METHODS:                                        # equal sizes: the smaller number wins
        keep, glabels, gsizes = ctx.largest_cluster(pts, 1.0, 4, method)
        assert np.array_equal(glabels, labels) and np.array_equal(gsizes, sizes)
        assert np.array_equal(keep, labels == 0) and keep.sum() == 513 and keep[0]
    cut = _dumbbell(drop=6)
    labels, sizes = _check(ctx, "dumbbell_cut", cut, 1.0, 1)
    assert sizes.tolist() == [518, 517]                             # the left ball keeps six bar points, the right one five


def _contested(b_first):
    rng = np.random.default_rng(47)
    a = np.concatenate([rng.uniform(-0.01, 0.01, (9, 3)), [[0.9, 0.0, 0.0]]])
    b = np.concatenate([rng.uniform(-0.01, 0.01, (9, 3)) + [3.6, 0.0, 0.0], [[2.7, 0.0, 0.0]]])
    mid = np.array([[1.8, 0.0, 0.0]])
    return np.concatenate([b, mid, a] if b_first else [a, mid, b])


@pytest.mark.parametrize("b_first", [False, True])
def test_contested_border_point_takes_the_smaller_number(ctx, b_first):
    pts = _contested(b_first)
    tag = f"contested_{b_first}"
    labels, sizes, count = _ref(tag, pts, 1.0, 10)
    # on the reference: the point is not core and its two neighbours are core points of different clusters
    near = np.flatnonzero(pr._dist_rows(pts, np.array([10]))[0] <= 1.0)
    assert count[10] == 2 and len(near) == 2 and (count[near] + 1 >= 10).all() and sorted(labels[near].tolist()) == [0, 1]
    assert labels.tolist() == [0] * 11 + [1] * 10 and sizes.tolist() == [11, 10]
    _check(ctx, tag, pts, 1.0, 10)


def test_degenerate_inputs(ctx):
    for method in METHODS:
        labels, sizes = ctx.cluster_dbscan(np.zeros((0, 3)), 0.5, 1, method)
        assert labels.shape == (0,) and sizes.shape == (0,)
        keep, labels, sizes = ctx.largest_cluster(np.zeros((0, 3)), 0.5, 1, method)
        assert keep.shape == (0,) and labels.shape == (0,) and sizes.shape == (0,)
    one = np.array([[0.5, -1.0, 2.0]])
    assert _check(ctx, "one", one, 0.5, 1)[0].tolist() == [0]
    assert _check(ctx, "one", one, 0.5, 2)[0].tolist() == [-1]
    same = np.tile(np.array([[0.25, -1.5, 3.0]]), (5000, 1))
    labels, sizes = _check(ctx, "same", same, 0.0, 1)                 # every union lands on one root
    assert sizes.tolist() == [5000]
    labels, sizes = _check(ctx, "same", same, 0.0, 5000)
    assert sizes.tolist() == [5000]
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [1, 2, -np.inf], [np.nan, np.nan, np.nan]] * 70)
    labels, sizes = _check(ctx, "bad", bad, 1.0, 1)
    assert (labels == -1).all() and len(sizes) == 0
    for method in METHODS:
        keep, _, _ = ctx.largest_cluster(bad, 1.0, 1, method)
        assert not keep.any()
    few = pr.sphere_cloud(300, seed=5)
    labels, sizes = _check(ctx, "few", few, 100.0, 301)               # min_points larger than n: nobody is core
    assert (labels == -1).all() and len(sizes) == 0


def test_rerun_is_identical_and_the_fallback_count_stays_zero(ctx):
    pts, _, _ = _cloud_and_ref("sphere_outliers")
    r = rr.radii_for_counts(pts)[1]
    ctx.radius_count(pts, r, "grid")                                  # the counter is 0 going in, whatever ran before
    a = ctx.cluster_dbscan(pts, r, 5, "grid"); b = ctx.cluster_dbscan(pts, r, 5, "grid")
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert ctx.points_fallback_count() == 0
    _check(ctx, "sphere_outliers", pts, r, 5, methods=(2,))


def test_device_form_on_torch_tensors(ctx):
    import torch
    pts, _, _ = _cloud_and_ref("sphere_20000")
    n = len(pts)
    r = rr.radii_for_counts(pts)[1]
    labels, sizes, count = _ref("sphere_20000", pts, r, 10)
    with torch.cuda.stream(ctx.torch_stream):
        d_pts = torch.from_numpy(pts).to("cuda", non_blocking=False)
        for method in METHODS:
            d_lab = torch.full((n,), -7, dtype=torch.int32, device="cuda"); d_nc = torch.full((1,), -7, dtype=torch.int32, device="cuda")
            d_sz = torch.full((n,), -7, dtype=torch.int32, device="cuda"); d_cnt = torch.full((n,), -7, dtype=torch.int32, device="cuda")
            ctx.cluster_dbscan_dev(d_pts.data_ptr(), n, r, 10, d_lab.data_ptr(), d_nc.data_ptr(), d_sz.data_ptr(), d_cnt.data_ptr(), method)
            nc = int(d_nc.cpu()[0])                                   # same stream: ordered behind the clustering
            assert nc == len(sizes) and np.array_equal(d_lab.cpu().numpy(), labels), method
            assert np.array_equal(d_sz.cpu().numpy()[:nc], sizes) and not d_sz.cpu().numpy()[nc:].any()
            assert np.array_equal(d_cnt.cpu().numpy(), count)
            d_lab.fill_(-7); d_nc.fill_(-7)                           # labels and the number only
            ctx.cluster_dbscan_dev(d_pts.data_ptr(), n, r, 10, d_lab.data_ptr(), d_nc.data_ptr(), 0, 0, method)
            assert int(d_nc.cpu()[0]) == nc and np.array_equal(d_lab.cpu().numpy(), labels), method


def test_largest_cluster_on_the_ply(ctx):
    pts = _cloud_and_ref("crazyhorse_ply")[0]
    labels, sizes, _ = _ref("crazyhorse_ply", pts, 0.2, 1)
    want, c, size = cr.largest(labels, sizes)
    assert size == 1011 and want.sum() == 1011
    for method in METHODS:
        keep, glabels, gsizes = ctx.largest_cluster(pts, 0.2, 1, method)
        assert keep.dtype == bool and np.array_equal(keep, want), method
        assert np.array_equal(glabels, labels) and np.array_equal(gsizes, sizes)
    # the C-ABI's own numbers, labels not asked for
    keep = np.zeros(len(pts), np.uint8); nc = C.c_int(-7); big = C.c_int(-7)
    assert ctx.lib.sfmhip_largest_cluster(ctx.h, pts.ctypes.data, len(pts), 0.2, 1, 0, keep.ctypes.data, None, C.byref(nc), C.byref(big)) == 0
    assert (nc.value, big.value) == (246, 1011) and np.array_equal(keep.astype(bool), want)


def test_bad_arguments_leave_the_outputs_alone(ctx):
    lib, h = ctx.lib, ctx.h
    pts = np.random.default_rng(3).uniform(-1, 1, (100, 3))
    lab = np.full(100, -7, np.int32); sz = np.full(100, -7, np.int32); cnt = np.full(100, -7, np.int32); keep = np.full(100, 7, np.uint8)
    nc = C.c_int(-7); big = C.c_int(-7)
    p, l, s, c, k = pts.ctypes.data, lab.ctypes.data, sz.ctypes.data, cnt.ctypes.data, keep.ctypes.data
    for r, mp, method, n in ((-1.0, 1, 1, 100), (np.nan, 1, 2, 100), (np.inf, 1, 0, 100), (0.5, 0, 1, 100), (0.5, -2, 2, 100), (0.5, 1, 3, 100),
                             (0.5, 1, -1, 100), (0.5, 1, 1, -1)):
        assert lib.sfmhip_cluster_dbscan(h, p, n, r, mp, method, l, C.byref(nc), s, c) == _lib.E_ARG
        assert lib.sfmhip_cluster_dbscan_dev(h, p, n, r, mp, method, l, c, s, None) == _lib.E_ARG
        assert lib.sfmhip_largest_cluster(h, p, n, r, mp, method, k, l, C.byref(nc), C.byref(big)) == _lib.E_ARG
    # NULL with n > 0
    assert lib.sfmhip_cluster_dbscan(h, None, 100, 0.5, 1, 1, l, C.byref(nc), s, c) == _lib.E_ARG
    assert lib.sfmhip_cluster_dbscan(h, p, 100, 0.5, 1, 1, None, C.byref(nc), s, c) == _lib.E_ARG
    assert lib.sfmhip_cluster_dbscan(h, p, 100, 0.5, 1, 1, l, None, s, c) == _lib.E_ARG
    assert lib.sfmhip_cluster_dbscan_dev(h, p, 100, 0.5, 1, 1, None, c, None, None) == _lib.E_ARG
    assert lib.sfmhip_cluster_dbscan_dev(h, p, 100, 0.5, 1, 1, l, None, None, None) == _lib.E_ARG
    assert lib.sfmhip_largest_cluster(h, p, 100, 0.5, 1, 1, None, l, C.byref(nc), C.byref(big)) == _lib.E_ARG
    assert (lab == -7).all() and (sz == -7).all() and (cnt == -7).all() and (keep == 7).all() and (nc.value, big.value) == (-7, -7)
    # n == 0: OK, no array touched, the numbers are 0
    assert lib.sfmhip_cluster_dbscan(h, None, 0, 0.5, 1, 2, None, C.byref(nc), None, None) == 0 and nc.value == 0
    assert lib.sfmhip_cluster_dbscan_dev(h, None, 0, 0.5, 1, 2, None, None, None, None) == 0
    nc.value = -7
    assert lib.sfmhip_largest_cluster(h, None, 0, 0.5, 1, 2, None, None, C.byref(nc), C.byref(big)) == 0 and (nc.value, big.value) == (0, 0)
    with pytest.raises(ValueError):
        ctx.cluster_dbscan(pts, 0.5, 1, "fastest")
    with pytest.raises(api.SfmHipError):
        ctx.cluster_dbscan(pts, 0.5, 0)


def test_a_failed_allocation_is_an_error_and_the_next_call_works(ctx):
    pts, _, _ = _cloud_and_ref("sphere_1000")
    r = rr.radii_for_counts(pts)[1]
    lab = np.empty(1000, np.int32); nc = C.c_int(0)
    for method in (1, 2):
        assert ctx.lib.sfmhip_debug_fail_allocations(ctx.h, 1) == 0
        assert ctx.lib.sfmhip_cluster_dbscan(ctx.h, pts.ctypes.data, 1000, r, 5, method, lab.ctypes.data, C.byref(nc), None, None) == _lib.E_HIP
        _check(ctx, "sphere_1000", pts, r, 5, methods=(method,))


# ---- driver ----------------------------------------------------------------------------------------------------------------------
def test_driver_largest_cluster_option(ctx, tmp_path):
    subprocess.check_call(["make", "-C", HOST], stdout=subprocess.DEVNULL)
    exe = os.path.join(HOST, "NViewReconstruct")
    feat = os.path.join(GOLD, "crazyhorse_features.bin")
    plain, filt, both = tmp_path / "plain", tmp_path / "filtered", tmp_path / "both"
    for d in (plain, filt, both):
        d.mkdir()
    o0 = subprocess.run([exe, feat, str(plain), "--quiet"], capture_output=True, text=True)
    o1 = subprocess.run([exe, feat, str(filt), "--quiet", "--largest-cluster=0.2"], capture_output=True, text=True)
    o2 = subprocess.run([exe, feat, str(both), "--quiet", "--radius-outliers=0.2,3", "--largest-cluster=0.2,3", "--voxel-size=0.2"],
                        capture_output=True, text=True)
    assert o0.returncode == 0 and o1.returncode == 0 and o2.returncode == 0, o1.stdout[-2000:] + o1.stderr[-2000:] + o2.stderr[-2000:]
    assert "cluster filter" not in o0.stdout
    for f in ("structure.yml", "structure_ba.yml"):                                   # the option touches the .ply only
        assert (plain / f).read_bytes() == (filt / f).read_bytes(), f
    pts = formats.read_structure_yml(filt / "structure_ba.yml")["points"]
    labels, sizes, _ = cr.cluster(pts, 0.2, 1)
    want, _, size = cr.largest(labels, sizes)
    assert 0 < size < len(pts)
    assert f"cluster filter: kept {size} of {len(pts)} points ({len(sizes)} clusters)" in o1.stdout
    ply0 = formats.read_ply_binary(plain / "structure_ba.ply"); ply1 = formats.read_ply_binary(filt / "structure_ba.ply")
    assert len(ply0) == len(pts) and len(ply1) == size
    for col in ("x", "y", "z", "r", "g", "b"):                                        # coordinates and colours follow the kept points
        assert np.array_equal(ply1[col], ply0[col][want]), col
    # with the radius filter before it and the voxel grid behind it: the three lines in that order, each on what the one before left
    keep, _ = ctx.radius_outliers(pts, 0.2, 3)
    labels, sizes, _ = cr.cluster(pts[keep], 0.2, 3)
    want, _, size = cr.largest(labels, sizes)
    cen = ctx.voxel_downsample(pts[keep][want], 0.2)[0]
    lines = [f"radius filter: kept {keep.sum()} of {len(pts)} points", f"cluster filter: kept {size} of {keep.sum()} points ({len(sizes)} clusters)",
             f"voxel grid: {size} points -> {len(cen)} voxels"]
    at = [o2.stdout.find(ln) for ln in lines]
    assert min(at) >= 0 and at == sorted(at), (at, re.findall(r"^(?:radius|cluster|voxel).*$", o2.stdout, re.M))
    assert len(formats.read_ply_binary(both / "structure_ba.ply")) == len(cen)
