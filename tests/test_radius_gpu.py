"""GPU: the fixed-radius point-cloud queries -- neighbour count within a radius (brute force, cell grid, auto), the radius outlier filter,
voxel-grid down-sampling and radius-limited normals -- through the C-ABI, the Python layer and the NViewReconstruct driver.  The
reference is the numpy restatement of tests/radius_ref.py: counts, voxel numbers and origins must equal it exactly and centroids bit
for bit, for every method, on every row."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import points_ref as pr
import radius_ref as rr
from sfm_opencv_amd import _lib, api, formats
from test_points_gpu import CLOUDS, GOLD, HOST, METHODS, _cloud_and_ref, _same_bits

pytestmark = pytest.mark.gpu
_I32P = C.POINTER(C.c_int32)
LATTICE_RADII = (1.0, float(np.sqrt(2.0)), 0.999999, 0.0)
_count_cache = {}


def _ref_count(name, pts, r):
    if (name, r) not in _count_cache:
        # a radius that takes in most of the cloud: all pairs outright (the kd-tree would only list them all as candidates)
        _count_cache[(name, r)] = rr.radius_count_allpairs(pts, r) if r >= 1e5 else rr.radius_count(pts, r)
    return _count_cache[(name, r)]


def _radii(name, pts):
    radii = (rr.radii_for_counts(pts) or [1.0]) + [0.0] + (list(LATTICE_RADII) if name == "lattice_32" else [])
    if name == "far_clamped":
        radii += [2e-3, 1e5, 1e8]
    return list(dict.fromkeys(radii))                     # each once, in order


def _far_clamped():
    """a sphere, 100 points so far out (4e7 against a cloud of size 5) that the grid clamps them into its border cells at every radius
    used here, and 60 companions within 2e-3 of some of those: the border cells' queries have neighbours to count"""
    rng = np.random.default_rng(31)
    far = rng.uniform(-4e7, 4e7, (100, 3))
    near = far[rng.integers(0, 100, 60)] + rng.uniform(-1e-3, 1e-3, (60, 3))
    return np.concatenate([pr.sphere_cloud(5000, seed=31), far, near])


RADIUS_CLOUDS = {**CLOUDS, "far_clamped": _far_clamped}
_extra = {}


def _cloud(name):
    if name in CLOUDS:
        return _cloud_and_ref(name)[0]
    if name not in _extra:
        _extra[name] = np.ascontiguousarray(RADIUS_CLOUDS[name](), np.float64)
    return _extra[name]


def _division_case():
    return pr.lattice(32) * 0.1 + np.array([0.3, -0.2, 0.1])


# ---- counts ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(RADIUS_CLOUDS))
def test_radius_count_equals_the_reference_on_every_row(ctx, name):
    pts = _cloud(name)
    if name == "far_clamped":
        assert rr.radius_count(pts, 2e-3)[5000:].sum() >= 100            # the far points do have neighbours to count
    for r in _radii(name, pts):
        ref = _ref_count(name, pts, r)
        for method in METHODS:
            got = ctx.radius_count(pts, r, method)
            assert got.dtype == np.int32 and got.shape == (len(pts),)
            bad = np.flatnonzero(got != ref)
            assert len(bad) == 0, (name, r, method, len(bad), bad[:5], got[bad[:5]], ref[bad[:5]])
        if len(pts):
            print(f"[radius] {name}: r = {r:.6g}, median count {np.median(ref):g}")


def test_radius_count_values_on_the_lattice_and_the_ply(ctx):
    pts = pr.lattice(32)
    for method in METHODS:
        c = ctx.radius_count(pts, 1.0, method)
        assert {int(v): int((c == v).sum()) for v in np.unique(c)} == {3: 8, 4: 360, 5: 5400, 6: 27000}
        c = ctx.radius_count(pts, np.sqrt(2.0), method)
        assert {int(v): int((c == v).sum()) for v in np.unique(c)} == {6: 8, 9: 360, 13: 5400, 18: 27000}
        assert not ctx.radius_count(pts, 0.999999, method).any() and not ctx.radius_count(pts, 0.0, method).any()
        c = ctx.radius_count(_cloud_and_ref("crazyhorse_ply")[0], 0.0, method)
        assert np.bincount(c).tolist() == [1364, 182, 3]                 # the fixture's exact duplicates


def test_radius_count_rerun_is_identical(ctx):
    pts, _, _ = _cloud_and_ref("sphere_outliers")
    r = rr.radii_for_counts(pts)[1]
    a = ctx.radius_count(pts, r, "grid"); b = ctx.radius_count(pts, r, "grid")
    print(f"[radius] sphere_outliers, r = {r:.6g}: fallback list {ctx.points_fallback_count()}")
    assert np.array_equal(a, b) and np.array_equal(a, _ref_count("sphere_outliers", pts, r))
    assert ctx.points_fallback_count() == 0                      # the radius grid decides every query itself (border cells included)
    ctx.knn_points(pts, 10, "grid")
    assert ctx.points_fallback_count() >= 200                    # ... and the counter is the one the kNN grid reports its list in


def test_radius_count_device_form_on_torch_tensors(ctx):
    import torch
    pts, _, _ = _cloud_and_ref("sphere_20000")
    r = rr.radii_for_counts(pts)[1]
    ref = _ref_count("sphere_20000", pts, r)
    with torch.cuda.stream(ctx.torch_stream):
        d_pts = torch.from_numpy(pts).to("cuda", non_blocking=False)
        for method in METHODS:
            d_count = torch.full((len(pts),), -7, dtype=torch.int32, device="cuda")
            ctx.radius_count_dev(d_pts.data_ptr(), len(pts), r, d_count.data_ptr(), method)
            assert np.array_equal(d_count.cpu().numpy(), ref), method            # same stream: ordered behind the search


# ---- filter ----------------------------------------------------------------------------------------------------------------------
def test_radius_filter_removes_the_far_points(ctx):
    """20,000 sphere points + 200 at uniform(-4e4, 4e4), r = 0.5, at least 10 neighbours: exactly the 200 go"""
    pts = pr.sphere_with_outliers(20000, seed=11)
    ref = rr.radius_count(pts, 0.5)
    assert 26 <= ref[:20000].min() and ref[:20000].max() <= 78 and not ref[20000:].any()       # the precondition, on the reference
    for method in METHODS:
        keep, count = ctx.radius_outliers(pts, 0.5, 10, method)
        assert keep.dtype == bool and np.array_equal(count, ref), method
        assert np.array_equal(keep, count >= 10)
        assert np.array_equal(np.flatnonzero(~keep), np.arange(20000, 20200))
    bad = _cloud_and_ref("non_finite_rows")[0]
    keep, count = ctx.radius_outliers(bad, 1e3, 1, "grid")
    assert not keep[[7, 500, 1199]].any() and not count[[7, 500, 1199]].any() and keep.sum() == len(bad) - 3
    assert (count[keep] == len(bad) - 4).all()                                                 # a non-finite point is counted by nobody


# ---- voxels ----------------------------------------------------------------------------------------------------------------------
VOXEL_CASES = {
    **{f"crazyhorse_{h}": (lambda: _cloud_and_ref("crazyhorse_ply")[0], h) for h in (0.05, 0.2, 1.0)},
    **{f"sphere_{h}": (lambda: _cloud_and_ref("sphere_20000")[0], h) for h in (0.1, 0.5, 20.0)},
    "lattice_2.0": (lambda: pr.lattice(32), 2.0),
    "division_0.2": (_division_case, 0.2),
    "identical_2000": (lambda: _cloud_and_ref("identical_2000")[0], 0.3),
    "non_finite_rows": (lambda: _cloud_and_ref("non_finite_rows")[0], 0.25),
    "cube_0": (lambda: np.zeros((0, 3)), 1.0),
    "only_non_finite": (lambda: np.array([[np.nan, 0, 0], [0, np.inf, 0], [1, 2, -np.inf], [np.nan, np.nan, np.nan]]), 1.0),
}
VOXEL_EXPECT = {"crazyhorse_0.05": (1225, 5), "crazyhorse_0.2": (564, 37), "crazyhorse_1.0": (142, 430), "sphere_0.1": (15149, 6),
                "sphere_0.5": (1701, 34), "sphere_20.0": (4, 19980), "lattice_2.0": (4913, 8), "identical_2000": (1, 2000)}


@pytest.mark.parametrize("case", list(VOXEL_CASES))
def test_voxel_downsample_equals_the_reference(ctx, case):
    make, h = VOXEL_CASES[case]
    pts = np.ascontiguousarray(make(), np.float64).reshape(-1, 3)
    rcen, rcounts, rvof, rorigin = rr.voxel_downsample(pts, h)
    if case == "division_0.2":                                   # the case keeps its teeth: a reciprocal would bin differently
        assert (np.floor((pts - rorigin) / h) != np.floor((pts - rorigin) * (1.0 / h))).any(axis=1).sum() > 0
    cen, counts, vof, origin = ctx.voxel_downsample(pts, h)
    assert len(cen) == len(rcen) and cen.shape == (len(rcen), 3), (case, len(cen), len(rcen))
    assert counts.dtype == np.int32 and np.array_equal(counts, rcounts)
    assert vof.dtype == np.int32 and np.array_equal(vof, rvof)
    if len(pts):
        assert np.array_equal(origin, rorigin), (origin, rorigin)
    assert _same_bits(cen, rcen)
    assert counts.sum() == np.isfinite(pts).all(axis=1).sum()
    if case in VOXEL_EXPECT:
        assert (len(cen), counts.max()) == VOXEL_EXPECT[case]
    if case == "identical_2000":
        assert _same_bits(cen, pts[:1])
    cen2, counts2, vof2, origin2 = ctx.voxel_downsample(pts, h)              # a rerun gives the same bits
    assert _same_bits(cen, cen2) and np.array_equal(counts, counts2) and np.array_equal(vof, vof2) and np.array_equal(origin, origin2)


def test_voxel_too_small_for_the_extent_is_an_argument_error(ctx):
    pts, _, _ = _cloud_and_ref("crazyhorse_ply")               # z reaches 2.8e4: 2.8M voxels of 0.01
    n = len(pts)
    cen = np.empty((n, 3)); m = np.zeros(1, np.int32)
    rc = ctx.lib.sfmhip_voxel_downsample(ctx.h, pts.ctypes.data, n, 0.01, cen.ctypes.data, None, None, m.ctypes.data_as(_I32P), None)
    assert rc == _lib.E_ARG and "voxel is too small" in ctx.lib.sfmhip_last_error(ctx.h).decode()
    with pytest.raises(api.SfmHipError):
        ctx.voxel_downsample(pts, 0.01)
    cen, counts, _, _ = ctx.voxel_downsample(pts, 0.2)           # the next call works
    assert (len(cen), counts.max()) == (564, 37)


def test_voxel_device_form_on_torch_tensors(ctx):
    import torch
    pts, _, _ = _cloud_and_ref("sphere_20000")
    n = len(pts)
    rcen, rcounts, rvof, rorigin = rr.voxel_downsample(pts, 0.5)
    with torch.cuda.stream(ctx.torch_stream):
        d_pts = torch.from_numpy(pts).to("cuda", non_blocking=False)
        d_cen = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
        d_counts = torch.zeros(n, dtype=torch.int32, device="cuda"); d_vof = torch.zeros(n, dtype=torch.int32, device="cuda")
        d_nv = torch.full((1,), -7, dtype=torch.int32, device="cuda"); d_org = torch.zeros(3, dtype=torch.float64, device="cuda")
        ctx.voxel_downsample_dev(d_pts.data_ptr(), n, 0.5, d_cen.data_ptr(), d_counts.data_ptr(), d_vof.data_ptr(), d_nv.data_ptr(), d_org.data_ptr())
        nv = int(d_nv.cpu()[0])
        assert nv == len(rcen)
        assert _same_bits(d_cen.cpu().numpy()[:nv], rcen) and np.array_equal(d_counts.cpu().numpy()[:nv], rcounts)
        assert np.array_equal(d_vof.cpu().numpy(), rvof) and np.array_equal(d_org.cpu().numpy(), rorigin)
        # centroids and the number only
        d_cen.zero_(); d_nv.fill_(-7)
        ctx.voxel_downsample_dev(d_pts.data_ptr(), n, 0.5, d_cen.data_ptr(), 0, 0, d_nv.data_ptr())
        assert int(d_nv.cpu()[0]) == nv and _same_bits(d_cen.cpu().numpy()[:nv], rcen)
        # too small a voxel: -1, and the call itself is OK
        ch = _cloud_and_ref("crazyhorse_ply")[0]
        d_ch = torch.from_numpy(ch).to("cuda", non_blocking=False)
        ctx.voxel_downsample_dev(d_ch.data_ptr(), len(ch), 0.01, d_cen.data_ptr(), d_counts.data_ptr(), d_vof.data_ptr(), d_nv.data_ptr())
        assert int(d_nv.cpu()[0]) == -1


# ---- hybrid normals --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sphere_20000", "crazyhorse_ply"])
def test_hybrid_normals_are_the_normals_of_the_neighbours_within_the_radius(ctx, name):
    pts, _, rdist = _cloud_and_ref(name)
    K = 10
    r = float(np.median(rdist[:, 4]))                            # the reference's median 5th-neighbour distance
    m = (rdist[:, :K] <= r).sum(axis=1)                          # the order is total: the first m entries are those within r
    got = ctx.estimate_normals(pts, K, method=1, radius=r)
    assert _same_bits(got, ctx.estimate_normals(pts, K, method=2, radius=r))
    assert _same_bits(got, ctx.estimate_normals(pts, K, radius=r))
    print(f"[radius] {name}: r = {r:.6g}, neighbours within r: {np.bincount(m, minlength=K + 1).tolist()}")
    assert len(np.unique(m)) >= 5                                # the radius does cut neighbourhoods
    for k in np.unique(m):
        rows = np.flatnonzero(m == k)
        if k == 0:
            assert np.isnan(got[rows]).all()
        else:
            assert _same_bits(got[rows], ctx.estimate_normals(pts, int(k))[rows]), (name, k)
    big = float(rdist[:, K - 1][np.isfinite(rdist[:, K - 1])].max()) * 1.5
    assert _same_bits(ctx.estimate_normals(pts, K, radius=big), ctx.estimate_normals(pts, K))


# ---- arguments -------------------------------------------------------------------------------------------------------------------
def test_argument_errors(ctx):
    lib, h = ctx.lib, ctx.h
    pts = np.random.default_rng(3).uniform(-1, 1, (100, 3))
    cnt = np.empty(100, np.int32); keep = np.empty(100, np.uint8); cen = np.empty((100, 3)); nrm = np.empty((100, 3)); m = C.c_int32(0)
    p, c, k, ce, no = pts.ctypes.data, cnt.ctypes.data, keep.ctypes.data, cen.ctypes.data, nrm.ctypes.data
    for r, method, n in ((np.nan, 1, 100), (np.inf, 2, 100), (-1.0, 0, 100), (-np.inf, 1, 100), (0.5, 3, 100), (0.5, -1, 100), (0.5, 1, -1)):
        assert lib.sfmhip_radius_count(h, p, n, r, method, c) == _lib.E_ARG
        assert lib.sfmhip_radius_count_dev(h, p, n, r, method, c) == _lib.E_ARG
        assert lib.sfmhip_radius_outliers(h, p, n, r, 2, method, k, c) == _lib.E_ARG
        assert lib.sfmhip_estimate_normals_hybrid(h, p, n, 10, r, method, no) == _lib.E_ARG
    assert lib.sfmhip_radius_outliers(h, p, 100, 0.5, 0, 1, k, c) == _lib.E_ARG
    assert lib.sfmhip_radius_outliers(h, p, 100, 0.5, -3, 1, k, c) == _lib.E_ARG
    for K in (0, 17):
        assert lib.sfmhip_estimate_normals_hybrid(h, p, 100, K, 0.5, 1, no) == _lib.E_ARG
    for voxel, n in ((0.0, 100), (-1.0, 100), (np.nan, 100), (np.inf, 100), (0.5, -1)):
        assert lib.sfmhip_voxel_downsample(h, p, n, voxel, ce, None, None, C.byref(m), None) == _lib.E_ARG
        assert lib.sfmhip_voxel_downsample_dev(h, p, n, voxel, ce, None, None, c, None) == _lib.E_ARG
    # NULL with n > 0
    assert lib.sfmhip_radius_count(h, None, 100, 0.5, 1, c) == _lib.E_ARG and lib.sfmhip_radius_count(h, p, 100, 0.5, 1, None) == _lib.E_ARG
    assert lib.sfmhip_radius_count_dev(h, None, 100, 0.5, 1, c) == _lib.E_ARG and lib.sfmhip_radius_count_dev(h, p, 100, 0.5, 1, None) == _lib.E_ARG
    assert lib.sfmhip_radius_outliers(h, p, 100, 0.5, 2, 1, None, c) == _lib.E_ARG and lib.sfmhip_radius_outliers(h, None, 100, 0.5, 2, 1, k, c) == _lib.E_ARG
    assert lib.sfmhip_voxel_downsample(h, None, 100, 0.5, ce, None, None, C.byref(m), None) == _lib.E_ARG
    assert lib.sfmhip_voxel_downsample(h, p, 100, 0.5, None, None, None, C.byref(m), None) == _lib.E_ARG
    assert lib.sfmhip_voxel_downsample(h, p, 100, 0.5, ce, None, None, None, None) == _lib.E_ARG
    assert lib.sfmhip_voxel_downsample_dev(h, p, 100, 0.5, None, None, None, c, None) == _lib.E_ARG
    assert lib.sfmhip_voxel_downsample_dev(h, p, 100, 0.5, ce, None, None, None, None) == _lib.E_ARG
    assert lib.sfmhip_estimate_normals_hybrid(h, None, 100, 10, 0.5, 1, no) == _lib.E_ARG
    assert lib.sfmhip_estimate_normals_hybrid(h, p, 100, 10, 0.5, 1, None) == _lib.E_ARG
    # n == 0: OK, no pointer touched
    assert lib.sfmhip_radius_count(h, None, 0, 0.5, 2, None) == 0
    assert lib.sfmhip_radius_count_dev(h, None, 0, 0.5, 2, None) == 0
    assert lib.sfmhip_radius_outliers(h, None, 0, 0.5, 2, 2, None, None) == 0
    assert lib.sfmhip_voxel_downsample(h, None, 0, 0.5, None, None, None, None, None) == 0
    assert lib.sfmhip_voxel_downsample_dev(h, None, 0, 0.5, None, None, None, None, None) == 0
    assert lib.sfmhip_estimate_normals_hybrid(h, None, 0, 10, 0.5, 2, None) == 0
    with pytest.raises(ValueError):
        ctx.radius_count(pts, 0.5, "fastest")
    keep0, count0 = ctx.radius_outliers(np.zeros((0, 3)), 0.5, 2)
    assert keep0.shape == (0,) and count0.shape == (0,)


def test_a_failed_allocation_is_an_error_and_the_next_call_works(ctx):
    pts, _, _ = _cloud_and_ref("sphere_1000")
    r = rr.radii_for_counts(pts)[1]
    ref = _ref_count("sphere_1000", pts, r)
    cnt = np.empty(1000, np.int32); keep = np.empty(1000, np.uint8); cen = np.empty((1000, 3)); m = C.c_int32(0)
    for method in (1, 2):
        assert ctx.lib.sfmhip_debug_fail_allocations(ctx.h, 1) == 0
        assert ctx.lib.sfmhip_radius_count(ctx.h, pts.ctypes.data, 1000, r, method, cnt.ctypes.data) == _lib.E_HIP
        assert np.array_equal(ctx.radius_count(pts, r, method), ref)
        assert ctx.lib.sfmhip_debug_fail_allocations(ctx.h, 1) == 0
        assert ctx.lib.sfmhip_radius_outliers(ctx.h, pts.ctypes.data, 1000, r, 5, method, keep.ctypes.data, None) == _lib.E_HIP
        k2, c2 = ctx.radius_outliers(pts, r, 5, method)
        assert np.array_equal(c2, ref) and np.array_equal(k2, ref >= 5)
    assert ctx.lib.sfmhip_debug_fail_allocations(ctx.h, 1) == 0
    assert ctx.lib.sfmhip_voxel_downsample(ctx.h, pts.ctypes.data, 1000, 0.5, cen.ctypes.data, None, None, C.byref(m), None) == _lib.E_HIP
    rcen, rcounts, _, _ = rr.voxel_downsample(pts, 0.5)
    got = ctx.voxel_downsample(pts, 0.5)
    assert _same_bits(got[0], rcen) and np.array_equal(got[1], rcounts)
    assert ctx.lib.sfmhip_debug_fail_allocations(ctx.h, 1) == 0
    with pytest.raises(api.SfmHipError):
        ctx.estimate_normals(pts, 10, radius=r)
    assert _same_bits(ctx.estimate_normals(pts, 10, radius=1e9), ctx.estimate_normals(pts, 10))


# ---- driver ----------------------------------------------------------------------------------------------------------------------
def test_driver_radius_outliers_and_voxel_size_options(ctx, tmp_path):
    subprocess.check_call(["make", "-C", HOST], stdout=subprocess.DEVNULL)
    exe = os.path.join(HOST, "NViewReconstruct")
    feat = os.path.join(GOLD, "crazyhorse_features.bin")
    plain, filt = tmp_path / "plain", tmp_path / "filtered"
    plain.mkdir(); filt.mkdir()
    o0 = subprocess.run([exe, feat, str(plain), "--quiet"], capture_output=True, text=True)
    o1 = subprocess.run([exe, feat, str(filt), "--quiet", "--radius-outliers=0.2,3", "--voxel-size=0.2"], capture_output=True, text=True)
    assert o0.returncode == 0 and o1.returncode == 0, o1.stdout[-2000:] + o1.stderr[-2000:]
    assert "radius filter" not in o0.stdout and "voxel grid" not in o0.stdout
    for f in ("structure.yml", "structure_ba.yml"):                                   # the options touch the .ply only
        assert (plain / f).read_bytes() == (filt / f).read_bytes(), f
    pts = formats.read_structure_yml(filt / "structure_ba.yml")["points"]
    keep, _ = ctx.radius_outliers(pts, 0.2, 3)
    assert 0 < keep.sum() < len(pts)
    assert f"radius filter: kept {keep.sum()} of {len(pts)} points" in o1.stdout
    cen, counts, vof, _ = ctx.voxel_downsample(pts[keep], 0.2)
    assert 0 < len(cen) < keep.sum()
    assert f"voxel grid: {keep.sum()} points -> {len(cen)} voxels" in o1.stdout
    ply0 = formats.read_ply_binary(plain / "structure_ba.ply"); ply1 = formats.read_ply_binary(filt / "structure_ba.ply")
    assert len(ply0) == len(pts) and len(ply1) == len(cen)
    for a, col in enumerate("xyz"):
        assert np.array_equal(ply1[col], cen[:, a].astype(np.float32))
    for col in "rgb":                                                                  # integer-rounded mean colours
        s = np.bincount(vof, weights=ply0[col][keep].astype(np.float64), minlength=len(cen)).astype(np.int64)
        assert np.array_equal(ply1[col].astype(np.int64), (2 * s + counts) // (2 * counts.astype(np.int64))), col
    nrm = ctx.estimate_normals(cen, 10)
    for a, col in enumerate(("nx", "ny", "nz")):
        assert np.array_equal(ply1[col], nrm[:, a].astype(np.float32), equal_nan=True)
    # MIN defaults to 2
    o2 = subprocess.run([exe, feat, str(filt), "--quiet", "--radius-outliers=0.2"], capture_output=True, text=True)
    keep2, _ = ctx.radius_outliers(pts, 0.2, 2)
    assert o2.returncode == 0 and f"radius filter: kept {keep2.sum()} of {len(pts)} points" in o2.stdout and "voxel grid" not in o2.stdout
