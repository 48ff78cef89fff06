"""GPU: the point-cloud neighbour search (sfmhip_knn_points: brute force, cell grid, auto), the normals and the statistical outlier
filter built on it, through the C-ABI, the Python layer and the NViewReconstruct driver.  The reference is the numpy restatement of
tests/points_ref.py; indices must equal it exactly and distances bit for bit, for every method, on every row."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import points_ref as pr
from sfm_opencv_amd import _lib, api, formats

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
HOST = os.path.join(ROOT, "sfm_opencv_amd", "host")
METHODS = (1, 2, 0)          # SFMHIP_POINTS_BRUTE, _GRID, _AUTO
KS = (1, 6, 10, 16)


def _cube(n, seed=3):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (n, 3))


def _crazyhorse():
    ply = formats.read_ply_binary(os.path.join(GOLD, "structure_ba_crazyhorse.ply"))
    return np.stack([ply["x"], ply["y"], ply["z"]], axis=1).astype(np.float64)


def _line(n=1500):
    t = np.random.default_rng(8).uniform(-3, 3, n)
    return np.stack([0.5 + 2.0 * t, -1.0 + 0.25 * t, 3.0 - t], axis=1)


def _with_bad_rows():
    p = pr.sphere_cloud(1200, seed=21)
    p[7] = [np.nan, 0.1, 0.2]; p[500] = [1.0, np.inf, 0.0]; p[1199] = [-np.inf, np.nan, 2.0]
    return p


CLOUDS = {
    **{f"cube_{n}": (lambda n=n: _cube(n)) for n in (0, 1, 2, 5, 11, 17, 255, 256, 257, 513, 1000, 20000)},
    "sphere_1000": lambda: pr.sphere_cloud(1000),
    "sphere_20000": lambda: pr.sphere_cloud(20000),
    "lattice_32": lambda: pr.lattice(32),
    "crazyhorse_ply": _crazyhorse,
    "sphere_outliers": lambda: pr.sphere_with_outliers(20000, seed=11),
    "identical_2000": lambda: np.tile(np.array([[0.25, -1.5, 3.0]]), (2000, 1)),
    "line": _line,
    "non_finite_rows": _with_bad_rows,
}
_cache = {}


def _cloud_and_ref(name):
    """the cloud and its reference table at K = 16 (the table at a smaller K is its first K columns: the order is total)"""
    if name not in _cache:
        pts = np.ascontiguousarray(CLOUDS[name](), np.float64).reshape(-1, 3)
        idx, dist = pr.knn(pts, 16) if len(pts) else (np.empty((0, 16), np.int32), np.empty((0, 16)))
        _cache[name] = (pts, idx, dist)
    return _cache[name]


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@pytest.mark.parametrize("name", list(CLOUDS))
def test_knn_equals_the_reference_on_every_row(ctx, name):
    pts, ridx, rdist = _cloud_and_ref(name)
    if name == "crazyhorse_ply":
        assert len(pts) - len(np.unique(pts, axis=0)) >= 90              # the fixture's exact duplicates are what this case is for
    for K in KS:
        for method in METHODS:
            idx, dist = ctx.knn_points(pts, K, method)
            assert idx.shape == (len(pts), K) and dist.shape == (len(pts), K)
            bad = np.flatnonzero((idx != ridx[:, :K]).any(axis=1))
            assert len(bad) == 0, (name, K, method, len(bad), bad[:5], idx[bad[:2]], ridx[bad[:2], :K])
            assert _same_bits(dist, rdist[:, :K]), (name, K, method)


@pytest.mark.parametrize("name", list(CLOUDS))
def test_grid_normals_equal_brute_force_normals_bit_for_bit(ctx, name):
    pts, _, _ = _cloud_and_ref(name)
    for K in (6, 10):
        a = ctx.estimate_normals(pts, K, method=1); b = ctx.estimate_normals(pts, K, method=2); c = ctx.estimate_normals(pts, K)
        assert _same_bits(a, b) and _same_bits(a, c), (name, K)


@pytest.mark.parametrize("outliers", [False, True])
def test_grid_normals_at_300k_points(ctx, outliers):
    pts = pr.sphere_with_outliers(300_000, seed=77) if outliers else pr.sphere_cloud(300_000)
    a = ctx.estimate_normals(pts, 10, method="brute"); b = ctx.estimate_normals(pts, 10, method="grid")
    print(f"[points] 300k{' + 1 % outliers' if outliers else ''}: fallback list {ctx.points_fallback_count()}")
    assert _same_bits(a, b)
    assert np.isfinite(a).all()


def _check_filter(ctx, pts, K, ratio, expect_removed=None):
    ridx, rdist = pr.knn(pts, K)
    rkeep, rm, rstats = pr.statistical_outliers(ridx, rdist, ratio)
    # precondition, on the reference alone: no point so close to the threshold that the last bits of mu / sigma decide it
    f = np.isfinite(rm)
    assert np.abs(rm[f] - rstats[2]).min() > 1e-9 * rstats[2]
    if expect_removed is not None:
        assert np.array_equal(np.flatnonzero(~rkeep), expect_removed)
    for method in METHODS:
        keep, m, stats = ctx.statistical_outliers(pts, K, ratio, method)
        assert keep.dtype == bool and _same_bits(m, rm), method
        assert np.abs(stats - rstats).max() <= 1e-12 * np.abs(rstats).max() and (np.abs(stats - rstats) <= 1e-12 * np.abs(rstats)).all(), (stats, rstats)
        assert np.array_equal(keep, m <= stats[2])
        assert np.array_equal(keep, rkeep), (method, np.flatnonzero(keep != rkeep)[:10])
        keep2, m2, stats2 = ctx.statistical_outliers(pts, K, ratio, method)           # fixed-order sums: a rerun gives the same bits
        assert np.array_equal(keep, keep2) and _same_bits(m, m2) and _same_bits(stats, stats2)
    return rkeep


def test_outlier_filter_removes_the_far_points(ctx):
    """20,000 sphere points + 200 at uniform(-4e4, 4e4), K = 10, ratio 2: the reference removes exactly the 200"""
    pts = pr.sphere_with_outliers(20000, seed=11)
    _check_filter(ctx, pts, 10, 2.0, expect_removed=np.arange(20000, 20200))


def test_outlier_filter_without_far_points(ctx):
    """a cloud whose tail is part of it: the noisy sphere plus a sparse halo.  Seed 4 was searched on the CPU for the precondition."""
    rng = np.random.default_rng(4)
    halo = pr.sphere_cloud(300, seed=5) * rng.uniform(1.0, 1.3, (300, 1))
    pts = np.concatenate([pr.sphere_cloud(8000, seed=4), halo])
    keep = _check_filter(ctx, pts, 8, 1.5)
    assert 0 < (~keep).sum() < 600


def test_outlier_filter_degenerate_inputs(ctx):
    keep, m, stats = ctx.statistical_outliers(_cube(5), 10, 2.0, "grid")           # n - 1 < K: nobody has K neighbours
    assert not keep.any() and np.isinf(m).all() and np.isnan(stats).all()
    keep, m, stats = ctx.statistical_outliers(np.zeros((0, 3)), 10)
    assert keep.shape == (0,) and m.shape == (0,)
    keep, m, stats = ctx.statistical_outliers(np.tile([[1.0, 2.0, 3.0]], (50, 1)), 4, 2.0, 2)
    assert keep.all() and not m.any() and stats.tolist() == [0.0, 0.0, 0.0]


def test_rerun_gives_the_same_bits(ctx):
    pts = pr.sphere_with_outliers(20000, seed=11)
    a = ctx.knn_points(pts, 10, "grid"); b = ctx.knn_points(pts, 10, "grid")
    assert np.array_equal(a[0], b[0]) and _same_bits(a[1], b[1])
    assert ctx.points_fallback_count() >= 200           # the far points cannot be certified inside RMAX rings


def test_device_form_on_torch_tensors(ctx):
    import torch
    pts, ridx, rdist = _cloud_and_ref("sphere_20000")
    K = 10
    with torch.cuda.stream(ctx.torch_stream):
        d_pts = torch.from_numpy(pts).to("cuda", non_blocking=False)
        for method in METHODS:
            d_idx = torch.full((len(pts), K), -7, dtype=torch.int32, device="cuda")
            d_dist = torch.zeros((len(pts), K), dtype=torch.float64, device="cuda")
            ctx.knn_points_dev(d_pts.data_ptr(), len(pts), K, d_idx.data_ptr(), d_dist.data_ptr(), method)
            idx = d_idx.cpu().numpy(); dist = d_dist.cpu().numpy()                  # same stream: ordered behind the search
            assert np.array_equal(idx, ridx[:, :K]) and _same_bits(dist, rdist[:, :K]), method
        # indices only / distances only
        d_idx = torch.zeros((len(pts), K), dtype=torch.int32, device="cuda")
        ctx.knn_points_dev(d_pts.data_ptr(), len(pts), K, d_idx.data_ptr(), 0, "grid")
        assert np.array_equal(d_idx.cpu().numpy(), ridx[:, :K])
    h_idx, _ = ctx.knn_points(pts, K, "grid")
    assert np.array_equal(h_idx, ridx[:, :K])


def test_argument_errors(ctx):
    lib, h = ctx.lib, ctx.h
    pts = _cube(100); idx = np.empty((100, 16), np.int32); dist = np.empty((100, 16)); keep = np.empty(100, np.uint8)
    p, i, d, k = pts.ctypes.data, idx.ctypes.data, dist.ctypes.data, keep.ctypes.data
    for K, method, n in ((0, 1, 100), (17, 2, 100), (10, 3, 100), (10, -1, 100), (10, 1, -1)):
        assert lib.sfmhip_knn_points(h, p, n, K, method, i, d) == _lib.E_ARG
        assert lib.sfmhip_knn_points_dev(h, p, n, K, method, i, d) == _lib.E_ARG
        assert lib.sfmhip_estimate_normals_ex(h, p, n, K, method, d) == _lib.E_ARG
        assert lib.sfmhip_statistical_outliers(h, p, n, K, 2.0, method, k, None, None) == _lib.E_ARG
    assert lib.sfmhip_knn_points(h, None, 100, 10, 1, i, d) == _lib.E_ARG
    assert lib.sfmhip_statistical_outliers(h, p, 100, 10, 2.0, 1, None, None, None) == _lib.E_ARG
    # n == 0: OK, no pointer touched
    assert lib.sfmhip_knn_points(h, None, 0, 10, 2, None, None) == 0
    assert lib.sfmhip_estimate_normals_ex(h, None, 0, 10, 2, None) == 0
    assert lib.sfmhip_statistical_outliers(h, None, 0, 10, 2.0, 2, None, None, None) == 0
    with pytest.raises(ValueError):
        ctx.knn_points(pts, 10, "fastest")


@pytest.mark.parametrize("method", [1, 2])
def test_a_failed_allocation_is_an_error_and_the_next_call_works(ctx, method):
    pts, ridx, _ = _cloud_and_ref("sphere_1000")
    idx = np.empty((1000, 10), np.int32)
    assert ctx.lib.sfmhip_debug_fail_allocations(ctx.h, 1) == 0
    assert ctx.lib.sfmhip_knn_points(ctx.h, pts.ctypes.data, 1000, 10, method, idx.ctypes.data, None) == _lib.E_HIP
    got, _ = ctx.knn_points(pts, 10, method)
    assert np.array_equal(got, ridx[:, :10])
    assert ctx.lib.sfmhip_debug_fail_allocations(ctx.h, 1) == 0
    with pytest.raises(api.SfmHipError):
        ctx.statistical_outliers(pts, 10, 2.0, method)
    keep, _, _ = ctx.statistical_outliers(pts, 10, 2.0, method)
    assert keep.sum() > 900


def test_driver_filter_outliers_option(ctx, tmp_path):
    subprocess.check_call(["make", "-C", HOST], stdout=subprocess.DEVNULL)
    exe = os.path.join(HOST, "NViewReconstruct")
    feat = os.path.join(GOLD, "crazyhorse_features.bin")
    plain, filt = tmp_path / "plain", tmp_path / "filtered"
    plain.mkdir(); filt.mkdir()
    o0 = subprocess.run([exe, feat, str(plain), "--quiet"], capture_output=True, text=True)
    o1 = subprocess.run([exe, feat, str(filt), "--quiet", "--filter-outliers"], capture_output=True, text=True)
    assert o0.returncode == 0 and o1.returncode == 0, o1.stdout[-2000:] + o1.stderr[-2000:]
    assert "outlier filter" not in o0.stdout
    for f in ("structure.yml", "structure_ba.yml"):                                   # the option touches the .ply only
        assert (plain / f).read_bytes() == (filt / f).read_bytes(), f
    pts = formats.read_structure_yml(filt / "structure_ba.yml")["points"]
    keep, _, _ = ctx.statistical_outliers(pts, 10, 2.0)
    assert f"outlier filter: kept {keep.sum()} of {len(pts)} points" in o1.stdout
    assert 0 < keep.sum() < len(pts)
    ply0 = formats.read_ply_binary(plain / "structure_ba.ply"); ply1 = formats.read_ply_binary(filt / "structure_ba.ply")
    assert len(ply0) == len(pts) and len(ply1) == keep.sum()
    kept = pts[keep]
    for a, col in enumerate("xyz"):
        assert np.array_equal(ply1[col], kept[:, a].astype(np.float32))
    assert all(np.array_equal(ply1[c], ply0[c][keep]) for c in ("r", "g", "b"))
    nrm = ctx.estimate_normals(kept, 10)
    for a, col in enumerate(("nx", "ny", "nz")):
        assert np.array_equal(ply1[col], nrm[:, a].astype(np.float32), equal_nan=True)
    # another ratio is read from the option
    o2 = subprocess.run([exe, feat, str(filt), "--quiet", "--filter-outliers=0.5"], capture_output=True, text=True)
    keep2, _, _ = ctx.statistical_outliers(pts, 10, 0.5)
    assert o2.returncode == 0 and f"outlier filter: kept {keep2.sum()} of {len(pts)} points" in o2.stdout and keep2.sum() < keep.sum()
