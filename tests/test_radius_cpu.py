"""CPU side of the fixed-radius point-cloud queries (sfmhip_radius_count, sfmhip_radius_outliers, sfmhip_voxel_downsample,
sfmhip_estimate_normals_hybrid): the numpy reference of tests/radius_ref.py agrees with itself and with values counted by hand on
the lattice, the binding, the library and the header carry the new entry points, and the two count kernels are compiled without
scratch."""
import collections
import os
import subprocess

import numpy as np
import pytest

import points_ref as pr
import radius_ref as rr
from sfm_opencv_amd import _lib, formats
from test_codeobj_cpu import LIB, READELF, _kernel_table
from test_points_cpu import _clouds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["sfmhip_radius_count", "sfmhip_radius_count_dev", "sfmhip_radius_outliers", "sfmhip_voxel_downsample",
               "sfmhip_voxel_downsample_dev", "sfmhip_estimate_normals_hybrid"]


def _crazyhorse():
    ply = formats.read_ply_binary(os.path.join(ROOT, "tests", "golden", "structure_ba_crazyhorse.ply"))
    return np.stack([ply["x"], ply["y"], ply["z"]], axis=1).astype(np.float64)


def _hist(a):
    return dict(collections.Counter(np.asarray(a).tolist()))


def test_radius_reference_forms_agree():
    for name, pts in _clouds():
        radii = rr.radii_for_counts(pts) + [0.0]
        if "lattice" in name:
            radii += [1.0, np.sqrt(2.0), 0.999999]
        for r in radii:
            a = rr.radius_count_allpairs(pts, r); b = rr.radius_count_kdtree(pts, r)
            assert np.array_equal(a, b), (name, r)


def test_radius_reference_on_non_finite_rows_and_duplicates():
    pts = np.array([[0, 0, 0], [1, 0, 0], [np.nan, 0, 0], [0, 2, 0], [np.inf, 1, 1], [1, 0, 0]], float)
    for f in (rr.radius_count_allpairs, rr.radius_count_kdtree):
        assert f(pts, 0.0).tolist() == [0, 1, 0, 0, 0, 1]
        assert f(pts, 1.0).tolist() == [2, 2, 0, 0, 0, 2]
        assert f(pts, 2.0).tolist() == [3, 2, 0, 1, 0, 2]
        assert f(pts, 1e6).tolist() == [3, 3, 0, 3, 0, 3]


def test_lattice_counts():
    """32^3 unit lattice: 6 face neighbours at 1, 12 edge neighbours at sqrt(2) (computed exactly: sqrt(2.0)), less at faces, edges
    and corners of the cube"""
    pts = pr.lattice(32)
    assert _hist(rr.radius_count(pts, 1.0)) == {3: 8, 4: 360, 5: 5400, 6: 27000}
    assert _hist(rr.radius_count(pts, np.sqrt(2.0))) == {6: 8, 9: 360, 13: 5400, 18: 27000}
    assert not rr.radius_count(pts, 0.999999).any() and not rr.radius_count(pts, 0.0).any()


def test_crazyhorse_duplicates_at_radius_zero():
    pts = _crazyhorse()
    assert len(pts) == 1549
    assert _hist(rr.radius_count(pts, 0.0)) == {0: 1364, 1: 182, 2: 3}


@pytest.mark.parametrize("cloud, voxel, n_voxels, largest", [
    ("crazyhorse", 0.05, 1225, 5), ("crazyhorse", 0.2, 564, 37), ("crazyhorse", 1.0, 142, 430),
    ("sphere", 0.1, 15149, 6), ("sphere", 0.5, 1701, 34), ("sphere", 20.0, 4, 19980)])
def test_voxel_reference_values(cloud, voxel, n_voxels, largest):
    pts = _crazyhorse() if cloud == "crazyhorse" else pr.sphere_cloud(20000)
    cen, counts, voxel_of, origin = rr.voxel_downsample(pts, voxel)
    assert (len(cen), counts.max()) == (n_voxels, largest)
    assert counts.sum() == len(pts) and np.array_equal(np.bincount(voxel_of), counts)
    assert np.array_equal(origin, pts.min(axis=0) - voxel * 0.5)
    # the rule, restated the slow way on a few voxels: members in ascending index, sequential sum, lexicographic numbering
    c = np.floor((pts - origin) / voxel).astype(np.int64)
    uniq = np.unique(c, axis=0)                                  # rows in ascending lexicographic order
    assert len(uniq) == n_voxels
    for v in (0, n_voxels // 2, n_voxels - 1, int(np.argmax(counts))):
        members = np.flatnonzero((c == uniq[v]).all(axis=1))
        assert np.array_equal(members, np.flatnonzero(voxel_of == v))
        s = pts[members[0]].copy()
        for j in members[1:]:
            s = s + pts[j]
        assert np.array_equal((s / len(members)).view(np.uint64), cen[v].view(np.uint64))


def test_voxel_reference_on_the_lattice_and_the_division_case():
    cen, counts, voxel_of, _ = rr.voxel_downsample(pr.lattice(32), 2.0)
    assert len(cen) == 4913 and _hist(counts) == {1: 8, 2: 180, 4: 1350, 8: 3375}
    # a true division, not a multiplication by the reciprocal: the two differ on this cloud, so a kernel that multiplies is caught
    p = pr.lattice(32) * 0.1 + np.array([0.3, -0.2, 0.1]); h = 0.2
    o = p.min(axis=0) - h * 0.5
    differ = (np.floor((p - o) / h) != np.floor((p - o) * (1.0 / h))).any(axis=1).sum()
    assert differ > 0
    print(f"[radius] division case: {differ} rows differ")
    _, _, vof, org = rr.voxel_downsample(p, h)
    assert np.array_equal(org, o)
    c = np.floor((p - o) / h).astype(np.int64)
    assert len(np.unique(c, axis=0)) == vof.max() + 1


def test_voxel_reference_degenerate_inputs():
    cen, counts, voxel_of, origin = rr.voxel_downsample(np.full((5, 3), np.nan), 1.0)
    assert cen.shape == (0, 3) and len(counts) == 0 and (voxel_of == -1).all() and np.isinf(origin).all()
    p = np.array([[0.0, 0, 0], [np.nan, 0, 0], [0.4, 0.4, 0.4], [3, 0, 0]])
    cen, counts, voxel_of, origin = rr.voxel_downsample(p, 1.0)
    assert voxel_of.tolist() == [0, -1, 0, 1] and counts.tolist() == [2, 1] and origin.tolist() == [-0.5, -0.5, -0.5]
    assert cen.tolist() == [[0.2, 0.2, 0.2], [3.0, 0.0, 0.0]]
    with pytest.raises(OverflowError):
        rr.voxel_downsample(_crazyhorse(), 0.01)                # 2.8M voxels along z


def test_binding_library_and_header_carry_the_radius_entry_points():
    assert all(s in _lib.SYMBOLS for s in NEW_SYMBOLS)
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.split()}
    assert all(s in exported for s in NEW_SYMBOLS), sorted(set(NEW_SYMBOLS) - exported)
    lib = _lib.load()
    assert all(hasattr(lib, s) for s in NEW_SYMBOLS)
    hdr = open(os.path.join(ROOT, "include", "sfmhip.h")).read()
    assert all(f"int {s}" in hdr for s in NEW_SYMBOLS)


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not found")
def test_count_kernels_have_no_scratch_and_fit_four_waves_per_simd(tmp_path):
    """the two count kernels hold a query, a counter and the gate: far less state than the kNN kernels, which meet the same bound"""
    assert os.path.exists(LIB), "build libsfmhip.so first (__graft_entry__.build)"
    t = _kernel_table(tmp_path)
    for frag, lds in (("points_radius_grid_kernel", 0), ("points_radius_brute_kernel", 3 * 256 * 8)):
        hits = [(k, v) for k, v in t.items() if frag in k]
        assert len(hits) == 1, (frag, sorted(t))
        name, k = hits[0]
        assert k["scratch"] == 0 and (k["spill"] or 0) == 0, (name, k)
        assert k["vgpr"] + k["agpr"] <= 128, (name, k)
        assert k["lds"] == lds, (name, k)
