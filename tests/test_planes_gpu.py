"""GPU: RANSAC plane segmentation (sfmhip_segment_planes, sfmhip_segment_planes_dev, sfmhip_segment_plane) through the C-ABI, the
Python layer and the NViewReconstruct driver.  The reference is tests/plane_ref.py, a numpy restatement of the definition in
include/sfmhip.h.  In every comparison with it labels, counts, winner and the number of planes must be EQUAL and the planes equal in
every bit (compared as uint64 views, the NaN rows behind the last plane included).  The refined plane is the one output that is not
defined bit for bit by the header; it is compared with numpy.linalg.eigh of the inliers' covariance."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import plane_ref as pf
from sfm_opencv_amd import _lib, api, formats

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
HOST = os.path.join(os.path.dirname(HERE), "sfm_opencv_amd", "host")
SCORE_CHUNK = 512            # planes.hip: active points staged in LDS per pass of plane_score_kernel
SCORE_MAX_WG = 2048          # planes.hip: workgroups of plane_score_kernel at most; beyond them a workgroup strides over several chunks
_cache = {}


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _raw(ctx, pts, t, H, seed, min_inliers, max_planes, refined=True):
    """the C-ABI's own arrays, all max_planes rows: (labels, n_planes, planes, counts, winner, refined)"""
    pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
    n = len(pts)
    labels = np.full(n, -7, np.int32); planes = np.full((max_planes, 4), 7.0); ref = np.full((max_planes, 4), 7.0)
    counts = np.full(max_planes, -7, np.int32); winner = np.full(max_planes, -7, np.int32); m = C.c_int(-7)
    rc = ctx.lib.sfmhip_segment_planes(ctx.h, pts.ctypes.data, n, t, H, seed, min_inliers, max_planes, labels.ctypes.data, C.byref(m),
                                       planes.ctypes.data, ref.ctypes.data if refined else None, counts.ctypes.data, winner.ctypes.data)
    assert rc == 0, ctx.lib.sfmhip_last_error(ctx.h)
    return labels, m.value, planes, counts, winner, ref


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _check(ctx, pts, t, H, seed, min_inliers, max_planes, ref=None, tag=None):
    """the library against the restatement, on every output the header defines bit for bit; returns (library's, reference's)"""
    if ref is None:
        ref = pf.segment(pts, t, H, seed, min_inliers, max_planes)
    got = _raw(ctx, pts, t, H, seed, min_inliers, max_planes)
    labels, n_planes, planes, counts, winner = ref
    what = (tag, t, H, seed, min_inliers, max_planes)
    assert got[1] == n_planes, (what, got[1], n_planes, got[3], counts)
    assert np.array_equal(got[3], counts) and got[3].dtype == np.int32, (what, got[3], counts)
    assert np.array_equal(got[4], winner), (what, got[4], winner)
    bad = np.flatnonzero(got[0] != labels)
    assert len(bad) == 0, (what, len(bad), bad[:5], got[0][bad[:5]], labels[bad[:5]])
    assert np.array_equal(_bits(got[2]), _bits(planes)), (what, got[2], planes)
    assert got[3].sum() == (got[0] >= 0).sum()
    assert np.isnan(got[5][n_planes:]).all() and np.isfinite(got[5][:n_planes]).all()
    return got, ref


def _check_refined(pts, got):
    """refined[p] against numpy.linalg.eigh on the inliers: sine of the angle between the normals and |d - d_ref| <= 1e-10"""
    labels, n_planes, refined = got[0], got[1], got[5]
    for p in range(n_planes):
        want = pf.refined_plane(pts[labels == p])
        sine = np.linalg.norm(np.cross(want[:3], refined[p, :3]))             # the same for opposite normals (a plane through the origin: d = +-0)
        print(f"[planes] refined {p}: sine {sine:.3g}, |d - d_ref| {abs(want[3] - refined[p, 3]):.3g}")
        assert sine <= 1e-10 and abs(want[3] - refined[p, 3]) <= 1e-10, (p, want, refined[p])
        assert abs(np.linalg.norm(refined[p, :3]) - 1) <= 4e-16 and not refined[p, 3] < 0


# ---- the planted scene: hypothesis-block edges and the stop rule -------------------------------------------------------------------
@pytest.mark.parametrize("H", (1, 63, 64, 65, 256, 257, 1000))
def test_planted_scene_equals_the_reference(ctx, H):
    pts, _ = _cached("planted", pf.planted_scene)
    for max_planes in (1, 3, 5):
        ref = _cached(("planted", H, max_planes), lambda: pf.segment(pts, 0.006, H, 12345, 50, max_planes))
        got, _ = _check(ctx, pts, 0.006, H, 12345, 50, max_planes, ref=ref, tag="planted")
        print(f"[planes] planted: H = {H}, max_planes {max_planes}: {got[1]} planes, counts {got[3][:got[1]]}, winner {got[4][:got[1]]}")
        # what the restatement gives for this scene (computed on the CPU): one hypothesis finds nothing, 63 .. 65 go on past the three
        # planted planes onto clutter, 256 and more find the three and stop
        if H == 1:
            assert got[1] == 0 and (got[0] == -1).all()
        elif H <= 65:
            assert got[1] == max_planes
        else:
            assert got[1] == min(max_planes, 3) and (got[3][:3][:got[1]] >= (1480, 880, 480)[:got[1]]).all()


# ---- active-set sizes around the tile of the scoring kernel ------------------------------------------------------------------------
@pytest.mark.parametrize("m", (255, 256, 257, SCORE_CHUNK - 1, SCORE_CHUNK, SCORE_CHUNK + 1, 1023, 1024, 1025, 4095, 4096, 4097, 65537))
def test_active_set_sizes(ctx, m):
    pts = pf.plane_with_clutter(m)
    assert np.isfinite(pts).all(axis=1).sum() == m and len(pts) > m
    got, _ = _check(ctx, pts, 0.006, 64, 3, 20, 2, tag=f"m={m}")
    assert got[1] >= 1 and got[3][0] >= 0.6 * m


def test_a_workgroup_that_strides_over_several_chunks(ctx):
    # H = 4096 is 16 blocks of 256 hypotheses, which leaves SCORE_MAX_WG / 16 = 128 workgroups along the points: 128 * SCORE_CHUNK =
    # 65536 active points are one chunk each, the 131 chunks of this cloud make the first three workgroups take two (the last one partial)
    m = (SCORE_MAX_WG // 16) * SCORE_CHUNK + 2 * SCORE_CHUNK + 7
    pts = pf.plane_with_clutter(m)
    _check(ctx, pts, 0.006, 4096, 11, 20, 1, tag="strided")


# ---- the inclusive threshold, in exact arithmetic ----------------------------------------------------------------------------------
def test_inclusive_threshold_on_a_lattice(ctx):
    pts = pf.lattice_scene()
    below = float(np.nextafter(1.0, 0.0))
    for t, want in ((0.0, 64), (1.0, 104), (below, None), (2.0, 114)):
        got, ref = _check(ctx, pts, t, 256, 7, 3, 1, tag="lattice")
        print(f"[planes] lattice: t = {t!r}: count {got[3][0]}, plane {got[2][0]}")
        if want is not None:
            assert got[3][0] == want and np.array_equal(np.abs(got[2][0]), [0, 0, 1, 0])
        else:
            assert got[3][0] not in (64, 104)              # the points at |z| = 1 are out: 89 on a skew plane in the restatement
    _check_refined(pts, _raw(ctx, pts, 1.0, 256, 7, 3, 1))


# ---- the tie rule -------------------------------------------------------------------------------------------------------------------
def _tie_seeds():
    pts = pf.tie_scene()
    found = []
    for seed in range(200):
        pl, valid = pf.hypotheses(pts, seed, 0, 256)
        cnt = pf.counts_of(pl, valid, pts, 0.0)
        ties = np.flatnonzero(cnt == cnt.max())
        heights = {int(round(abs(pl[h, 3]))) for h in ties}
        if cnt.max() == 400 and len(ties) > 1 and ties[0] >= 64 and len({h // 64 for h in ties}) >= 2 and heights == {0, 10}:
            found.append((seed, ties))
    return pts, found


def test_the_smallest_h_wins_a_tie(ctx):
    pts, found = _cached("ties", _tie_seeds)
    print("[planes] tie seeds:", [(s, t[:4].tolist()) for s, t in found])
    assert len(found) >= 1
    for seed, ties in found:
        got, _ = _check(ctx, pts, 0.0, 256, seed, 3, 1, tag="tie")
        assert got[4][0] == ties[0] and got[3][0] == 400


# ---- degenerate inputs -------------------------------------------------------------------------------------------------------------
def test_degenerate_inputs(ctx):
    tri = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0.5]])
    line = np.array([[0.0, 0, 0], [1, 1, 1], [2, 2, 2], [3, 3, 3]])
    rng = np.random.default_rng(4)
    cases = {
        "n=1": tri[:1], "n=2": tri[:2], "n=3": tri, "3 collinear": line[:3], "4 collinear": line,
        "all NaN": np.full((40, 3), np.nan), "coincident": np.tile([[0.25, -1.5, 3.0]], (50, 1)),
        "1e200": rng.uniform(-1, 1, (60, 3)) * 1e200, "two finite": np.concatenate([tri[:2], np.full((5, 3), np.inf)]),
    }
    for tag, pts in cases.items():
        for max_planes in (1, 3):
            got, _ = _check(ctx, pts, 0.01, 64, 5, 3, max_planes, tag=tag)
            if tag == "n=3":
                assert got[1] == 1 and got[3][0] == 3 and (got[0] == 0).all()
            else:
                assert got[1] == 0 and (got[0] == -1).all(), tag
    # min_inliers above n
    pts = _cached("planted", pf.planted_scene)[0]
    got, _ = _check(ctx, pts, 0.006, 256, 12345, len(pts) + 1, 3, tag="min_inliers > n")
    assert got[1] == 0
    # n == 0
    labels, planes, counts, winner, refined = ctx.segment_planes(np.empty((0, 3)), 0.1, max_planes=3)
    assert labels.shape == (0,) and planes.shape == (0, 4) and counts.shape == (0,) and winner.shape == (0,) and refined.shape == (0, 4)


# ---- a larger cloud ----------------------------------------------------------------------------------------------------------------
def test_a_cloud_of_100000_points(ctx):
    pts = pf.plane_with_clutter(100000, seed=11)
    got, _ = _check(ctx, pts, 0.006, 1024, 99, 100, 1, tag="100k")
    assert got[3][0] >= 65000
    _check_refined(pts, got)


# ---- the refined plane -------------------------------------------------------------------------------------------------------------
def test_refined_plane_against_eigh(ctx):
    pts = _cached("planted", pf.planted_scene)[0]
    got = _raw(ctx, pts, 0.006, 256, 12345, 50, 5)
    assert got[1] == 3 and got[3].sum() == (got[0] >= 0).sum()
    _check_refined(pts, got)
    # the refined plane of a planted plane lies closer to its points than the three-point plane it was refined from
    for p in range(3):
        P = pts[got[0] == p]
        rms = [np.sqrt(np.mean((P @ pl[:3] + pl[3]) ** 2)) for pl in (got[2][p], got[5][p])]
        assert rms[1] <= rms[0]


# ---- consistency and reruns --------------------------------------------------------------------------------------------------------
def test_reruns_and_the_other_forms_give_the_same_bits(ctx):
    import torch
    pts = _cached("planted", pf.planted_scene)[0]
    n = len(pts)
    a = _raw(ctx, pts, 0.006, 257, 12345, 50, 5)
    b = _raw(ctx, pts, 0.006, 257, 12345, 50, 5)
    for x, y in zip(a, b):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
    # without the refined plane nothing else changes
    c = _raw(ctx, pts, 0.006, 257, 12345, 50, 5, refined=False)
    for k in range(5):
        assert np.asarray(a[k]).tobytes() == np.asarray(c[k]).tobytes()
    assert (c[5] == 7.0).all()
    # the device form on torch tensors
    with torch.cuda.stream(ctx.torch_stream):
        d_pts = torch.from_numpy(pts).to("cuda", non_blocking=False)
        d_lab = torch.full((n,), -7, dtype=torch.int32, device="cuda"); d_np = torch.full((1,), -7, dtype=torch.int32, device="cuda")
        d_pl = torch.full((5, 4), 7.0, dtype=torch.float64, device="cuda"); d_rf = torch.full((5, 4), 7.0, dtype=torch.float64, device="cuda")
        d_ct = torch.full((5,), -7, dtype=torch.int32, device="cuda"); d_wn = torch.full((5,), -7, dtype=torch.int32, device="cuda")
        ctx.segment_planes_dev(d_pts.data_ptr(), n, 0.006, 5, d_lab.data_ptr(), d_np.data_ptr(), d_pl.data_ptr(), d_rf.data_ptr(), d_ct.data_ptr(),
                               d_wn.data_ptr(), hypotheses=257, seed=12345, min_inliers=50)
        dev = (d_lab.cpu().numpy(), int(d_np.cpu()[0]), d_pl.cpu().numpy(), d_ct.cpu().numpy(), d_wn.cpu().numpy(), d_rf.cpu().numpy())
        for x, y in zip(a, dev):
            assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
        d_lab.fill_(-7); d_np.fill_(-7); d_pl.fill_(7.0)                       # the required outputs only
        ctx.segment_planes_dev(d_pts.data_ptr(), n, 0.006, 5, d_lab.data_ptr(), d_np.data_ptr(), d_pl.data_ptr(), hypotheses=257, seed=12345, min_inliers=50)
        assert int(d_np.cpu()[0]) == a[1] and np.array_equal(d_lab.cpu().numpy(), a[0]) and d_pl.cpu().numpy().tobytes() == a[2].tobytes()
    # the Python layer trims to the number of planes
    labels, planes, counts, winner, refined = ctx.segment_planes(pts, 0.006, max_planes=5, hypotheses=257, seed=12345, min_inliers=50)
    P = a[1]
    assert planes.shape == (P, 4) and refined.shape == (P, 4) and counts.dtype == np.int32 and winner.dtype == np.int32 and labels.dtype == np.int32
    assert np.array_equal(labels, a[0]) and planes.tobytes() == a[2][:P].tobytes() and np.array_equal(counts, a[3][:P])
    assert np.array_equal(winner, a[4][:P]) and refined.tobytes() == a[5][:P].tobytes()
    # segment_plane is the max_planes = 1 case
    one = _raw(ctx, pts, 0.006, 257, 12345, 50, 1)
    plane, keep, ref1 = ctx.segment_plane(pts, 0.006, hypotheses=257, seed=12345, min_inliers=50)
    assert keep.dtype == bool and np.array_equal(keep, one[0] == 0) and plane.tobytes() == one[2][0].tobytes() and ref1.tobytes() == one[5][0].tobytes()
    cnt = C.c_int(-7); k8 = np.full(n, 7, np.uint8); pl = np.full(4, 7.0)
    assert ctx.lib.sfmhip_segment_plane(ctx.h, pts.ctypes.data, n, 0.006, 257, 12345, 50, pl.ctypes.data, k8.ctypes.data, C.byref(cnt), None) == 0
    assert cnt.value == one[3][0] == k8.sum() and pl.tobytes() == one[2][0].tobytes()
    # no plane found: NaN, keep all 0, count 0, and still OK
    assert ctx.lib.sfmhip_segment_plane(ctx.h, pts.ctypes.data, n, 0.006, 257, 12345, n + 1, pl.ctypes.data, k8.ctypes.data, C.byref(cnt), None) == 0
    assert cnt.value == 0 and not k8.any() and np.isnan(pl).all()
    plane, keep, ref1 = ctx.segment_plane(pts, 0.006, hypotheses=1, seed=12345, min_inliers=50)
    assert np.isnan(plane).all() and np.isnan(ref1).all() and not keep.any()


# ---- errors ------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_leave_the_outputs_alone(ctx):
    lib, h = ctx.lib, ctx.h
    pts = np.random.default_rng(3).uniform(-1, 1, (100, 3))
    lab = np.full(100, -7, np.int32); pl = np.full((3, 4), 7.0); rf = np.full((3, 4), 7.0); ct = np.full(3, -7, np.int32); wn = np.full(3, -7, np.int32)
    keep = np.full(100, 7, np.uint8); m = C.c_int(-7); cnt = C.c_int(-7)
    p, l, P, R, c, w, k = (a.ctypes.data for a in (pts, lab, pl, rf, ct, wn, keep))
    for t, H, mi, mp, n in ((-1.0, 64, 3, 3, 100), (np.nan, 64, 3, 3, 100), (np.inf, 64, 3, 3, 100), (0.1, 0, 3, 3, 100), (0.1, 65537, 3, 3, 100),
                            (0.1, 64, 2, 3, 100), (0.1, 64, 3, 0, 100), (0.1, 64, 3, 65, 100), (0.1, 64, 3, 3, -1)):
        assert lib.sfmhip_segment_planes(h, p, n, t, H, 1, mi, mp, l, C.byref(m), P, R, c, w) == _lib.E_ARG, (t, H, mi, mp, n)
        assert lib.sfmhip_segment_planes_dev(h, p, n, t, H, 1, mi, mp, l, c, P, R, c, w) == _lib.E_ARG, (t, H, mi, mp, n)
        if mp == 3:
            assert lib.sfmhip_segment_plane(h, p, n, t, H, 1, mi, P, k, C.byref(cnt), R) == _lib.E_ARG, (t, H, mi, n)
    # NULL with n > 0
    assert lib.sfmhip_segment_planes(h, None, 100, 0.1, 64, 1, 3, 3, l, C.byref(m), P, R, c, w) == _lib.E_ARG
    assert lib.sfmhip_segment_planes(h, p, 100, 0.1, 64, 1, 3, 3, None, C.byref(m), P, R, c, w) == _lib.E_ARG
    assert lib.sfmhip_segment_planes(h, p, 100, 0.1, 64, 1, 3, 3, l, None, P, R, c, w) == _lib.E_ARG
    assert lib.sfmhip_segment_planes(h, p, 100, 0.1, 64, 1, 3, 3, l, C.byref(m), None, R, c, w) == _lib.E_ARG
    assert lib.sfmhip_segment_planes_dev(h, p, 100, 0.1, 64, 1, 3, 3, None, c, P, None, None, None) == _lib.E_ARG
    assert lib.sfmhip_segment_planes_dev(h, p, 100, 0.1, 64, 1, 3, 3, l, None, P, None, None, None) == _lib.E_ARG
    assert lib.sfmhip_segment_planes_dev(h, p, 100, 0.1, 64, 1, 3, 3, l, c, None, None, None, None) == _lib.E_ARG
    assert lib.sfmhip_segment_plane(h, p, 100, 0.1, 64, 1, 3, None, k, C.byref(cnt), R) == _lib.E_ARG
    assert lib.sfmhip_segment_plane(h, p, 100, 0.1, 64, 1, 3, P, None, C.byref(cnt), R) == _lib.E_ARG
    assert (lab == -7).all() and (pl == 7).all() and (rf == 7).all() and (ct == -7).all() and (wn == -7).all() and (keep == 7).all()
    assert (m.value, cnt.value) == (-7, -7)
    # n == 0: OK, no array touched, the numbers are 0
    assert lib.sfmhip_segment_planes(h, None, 0, 0.1, 64, 1, 3, 3, None, C.byref(m), None, None, None, None) == 0 and m.value == 0
    assert lib.sfmhip_segment_planes_dev(h, None, 0, 0.1, 64, 1, 3, 3, None, None, None, None, None, None) == 0
    assert lib.sfmhip_segment_plane(h, None, 0, 0.1, 64, 1, 3, None, None, C.byref(cnt), None) == 0 and cnt.value == 0
    with pytest.raises(api.SfmHipError):
        ctx.segment_planes(pts, -0.5)
    with pytest.raises(api.SfmHipError):
        ctx.segment_plane(pts, 0.1, hypotheses=0)


def test_a_failed_allocation_is_an_error_and_the_next_call_works(ctx):
    pts = _cached("planted", pf.planted_scene)[0]
    n = len(pts)
    lab = np.empty(n, np.int32); pl = np.empty((3, 4)); m = C.c_int(0)
    ref = _cached(("planted", 256, 3), lambda: pf.segment(pts, 0.006, 256, 12345, 50, 3))
    for failing in (1, 2):                      # the first block a call takes (the cloud), then both that one and the next
        assert ctx.lib.sfmhip_debug_fail_allocations(ctx.h, failing) == 0
        for _ in range(failing):
            rc = ctx.lib.sfmhip_segment_planes(ctx.h, pts.ctypes.data, n, 0.006, 256, 12345, 50, 3, lab.ctypes.data, C.byref(m), pl.ctypes.data, None, None, None)
            assert rc == _lib.E_HIP
        _check(ctx, pts, 0.006, 256, 12345, 50, 3, ref=ref, tag="after a failed allocation")


# ---- driver ------------------------------------------------------------------------------------------------------------------------
def test_driver_planes_option(ctx, tmp_path):
    subprocess.check_call(["make", "-C", HOST], stdout=subprocess.DEVNULL)
    exe = os.path.join(HOST, "NViewReconstruct")
    feat = os.path.join(GOLD, "crazyhorse_features.bin")
    plain, flagged = tmp_path / "plain", tmp_path / "planes"
    plain.mkdir(); flagged.mkdir()
    o0 = subprocess.run([exe, feat, str(plain), "--quiet"], capture_output=True, text=True)
    o1 = subprocess.run([exe, feat, str(flagged), "--quiet", "--planes=0.05,2"], capture_output=True, text=True)
    assert o0.returncode == 0 and o1.returncode == 0, o1.stdout[-2000:] + o1.stderr[-2000:]
    for f in ("structure.yml", "structure_ba.yml", "structure_ba.ply"):               # the option changes no file
        assert (plain / f).read_bytes() == (flagged / f).read_bytes(), f
    lines = re.findall(r"^plane (\d+): (\S+) (\S+) (\S+) (\S+) \((\d+) points\)$", o1.stdout, re.M)
    assert not re.search(r"^plane \d+:", o0.stdout, re.M)
    # a run without the flag prints what it always printed: the flagged run's output minus its plane lines (the output directory aside,
    # and the one measured figure, the solver's wall time)
    strip = lambda s, d: re.sub(r"^ Time \(s\): .*$", " Time (s): T", re.sub(r"^plane \d+:.*\n", "", s, flags=re.M).replace(str(d), "OUT"), flags=re.M)      # noqa: E731
    assert strip(o1.stdout, flagged) == strip(o0.stdout, plain)
    # The .ply stores float32; without a filter its rows are the points of structure_ba.yml, which holds the doubles the driver ran on
    pts = formats.read_structure_yml(flagged / "structure_ba.yml")["points"]
    ply = formats.read_ply_binary(flagged / "structure_ba.ply")
    assert len(ply) == len(pts) and np.array_equal(ply["x"], pts[:, 0].astype(np.float32)) and np.array_equal(ply["z"], pts[:, 2].astype(np.float32))
    labels, planes, counts, winner, refined = ctx.segment_planes(pts, 0.05, max_planes=2)
    assert 1 <= len(counts) == len(lines), (lines, counts)
    for k, ln in enumerate(lines):
        assert int(ln[0]) == k and int(ln[5]) == counts[k] == (labels == k).sum()
        assert np.array_equal(np.array([float(v) for v in ln[1:5]]), refined[k])      # %.17g round-trips a double
