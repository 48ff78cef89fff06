"""CPU side of the clustering (sfmhip_cluster_dbscan, sfmhip_cluster_dbscan_dev, sfmhip_largest_cluster): the two forms of the reference
of tests/cluster_ref.py agree, reproduce values derived by hand and from the committed cloud, and equal scikit-learn's DBSCAN label
for label; header, binding and library carry the entry points; the new kernels are compiled without scratch."""
import os
import subprocess

import numpy as np
import pytest

import cluster_ref as cr
import points_ref as pr
import radius_ref as rr
from sfm_opencv_amd import _lib
from test_codeobj_cpu import LIB, READELF, _kernel_table
from test_points_cpu import _clouds
from test_radius_cpu import _crazyhorse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["sfmhip_cluster_dbscan", "sfmhip_cluster_dbscan_dev", "sfmhip_largest_cluster"]
MIN_POINTS = (1, 2, 5, 10)
SEVEN = np.array([[0, 0, 0], [1, 0, 0], [np.nan, 0, 0], [0, 2, 0], [np.inf, 1, 1], [1, 0, 0], [5, 5, 5]], float)
_FORMS = (cr.cluster_allpairs, cr.cluster_kdtree)


def _same(a, b):
    return all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("mp", MIN_POINTS)
@pytest.mark.parametrize("which", range(3))
def test_cluster_reference_forms_agree(which, mp):
    for name, pts in list(_clouds())[which:which + 1]:
        for r in rr.radii_for_counts(pts) + [0.0]:
            want = rr.radius_count_kdtree(pts, r)
            if True:
                a = cr.cluster_allpairs(pts, r, mp); b = cr.cluster_kdtree(pts, r, mp)
                assert _same(a, b), (name, r, mp)
                labels, sizes, count = a
                assert np.array_equal(count, want), (name, r, mp)                # count IS the radius count
                assert sizes.sum() + (labels < 0).sum() == len(pts) and (sizes > 0).all()
                # numbered in ascending order of the smallest core member
                core = count + 1 >= mp
                firsts = [np.flatnonzero(core & (labels == c))[0] for c in range(len(sizes))]
                assert firsts == sorted(firsts), (name, r, mp)


@pytest.mark.parametrize("r, mp, labels", [
    (0.0, 1, [0, 1, -1, 2, -1, 1, 3]),
    (0.0, 2, [-1, 0, -1, -1, -1, 0, -1]),
    (1.0, 1, [0, 0, -1, 1, -1, 0, 2]),
    (1.0, 3, [0, 0, -1, -1, -1, 0, -1]),
    (2.0, 4, [0, 0, -1, 0, -1, 0, -1])])
def test_seven_points_by_hand(r, mp, labels):
    for f in _FORMS:
        got, sizes, count = f(SEVEN, r, mp)
        assert got.tolist() == labels, (f.__name__, got)
        assert sizes.tolist() == np.bincount([v for v in labels if v >= 0]).tolist()
    # (2, 4): point 3 has two neighbours (0 at distance 2 and ... nobody else): not core, adopted by cluster 0 through core point 0
    if (r, mp) == (2.0, 4):
        assert count.tolist() == [3, 2, 0, 1, 0, 2, 0]


@pytest.mark.parametrize("r, mp, n_clusters, core, border, noise, largest", [
    (1.0, 1, 1, 32768, 0, 0, 32768),
    (1.0, 7, 1, 27000, 5400, 368, 32400),
    (1.0, 6, 1, 32400, 360, 8, 32760),
    (1.0, 8, 0, 0, 0, 32768, 0),
    (0.999999, 1, 32768, 32768, 0, 0, 1),
    (float(np.sqrt(2.0)), 19, 1, 27000, 5760, 8, 32760)])
def test_lattice_values(r, mp, n_clusters, core, border, noise, largest):
    pts = pr.lattice(32)
    labels, sizes, count = cr.cluster_kdtree(pts, r, mp)
    assert len(sizes) == n_clusters and cr.census(labels, count, pts, mp) == (core, border, noise)
    assert cr.largest(labels, sizes)[2] == largest
    if n_clusters == 32768:
        assert np.array_equal(labels, np.arange(32768))


@pytest.mark.parametrize("r, mp, n_clusters, top, census", [
    (0.0, 1, 1456, [3], None),
    (0.0, 2, 92, None, (185, 0, 1364)),
    (0.2, 1, 246, [1011, 63, 27], None),
    (0.2, 5, 20, [1005], (1137, 76, 336)),
    (1.0, 5, 9, [1384], None)])
def test_crazyhorse_values(r, mp, n_clusters, top, census):
    pts = _crazyhorse()
    a = cr.cluster_allpairs(pts, r, mp); b = cr.cluster_kdtree(pts, r, mp)
    assert _same(a, b)
    labels, sizes, count = a
    assert len(sizes) == n_clusters
    if top:
        assert np.sort(sizes)[::-1][:len(top)].tolist() == top
    if census:
        assert cr.census(labels, count, pts, mp) == census


def test_largest_takes_the_smallest_number_among_equals():
    labels = np.array([1, 0, 1, -1, 0, 2], np.int32)
    keep, c, size = cr.largest(labels, np.array([2, 2, 1], np.int32))
    assert (c, size) == (0, 2) and keep.tolist() == [False, True, False, False, True, False]
    keep, c, size = cr.largest(np.full(4, -1, np.int32), np.empty(0, np.int32))
    assert (c, size) == (-1, 0) and not keep.any()


def _sklearn_cases():
    sphere = pr.sphere_cloud(20000)
    for r in rr.radii_for_counts(sphere):
        for mp in (1, 5, 10):
            yield "sphere_20000", sphere, r, mp, False
    lat = pr.lattice(32)
    for r, mp in ((1.0, 1), (1.0, 7), (1.0, 6), (1.0, 8), (0.999999, 1), (float(np.sqrt(2.0)), 19)):
        yield "lattice_32", lat, r, mp, True
    ch = _crazyhorse()
    for r, mp in ((0.2, 1), (0.2, 5), (1.0, 5)):
        yield "crazyhorse", ch, r, mp, False


@pytest.mark.parametrize("cloud", ["sphere_20000", "lattice_32", "crazyhorse"])
def test_labels_equal_scikit_learn_dbscan(cloud):
    DBSCAN = pytest.importorskip("sklearn.cluster").DBSCAN
    near_of = {}
    for name, pts, r, mp, exact in (c for c in _sklearn_cases() if c[0] == cloud):
        labels, _, _ = cr.cluster(pts, r, mp)
        if not exact:                 # the precondition: no pair sits where the two libraries' distance arithmetic could disagree
            if r not in near_of:
                d = cr.candidate_pairs(pts, r)[2]
                near_of[r] = (np.abs(d - r) <= 1e-9 * r, d)
            near, d = near_of[r]
            assert not (near & (d != r)).any(), (name, r)
            # d == r exactly does occur: radii_for_counts returns a median of neighbour distances, which is one of the cloud's own
            # distances where the two middle values are the two directions of one pair (sphere_20000, third radius).  Such a pair
            # must not matter: the labels are the same at the double just below r, where every rule excludes it.
            if near.any():
                assert np.array_equal(cr.cluster(pts, np.nextafter(r, 0.0), mp)[0], labels), (name, r, mp)
        finite = np.isfinite(pts).all(axis=1)
        theirs = DBSCAN(eps=r, min_samples=mp, algorithm="kd_tree").fit(pts[finite]).labels_
        assert np.array_equal(labels[finite], theirs), (name, r, mp)


def test_binding_library_and_header_carry_the_cluster_entry_points():
    assert all(s in _lib.SYMBOLS for s in NEW_SYMBOLS)
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.split()}
    assert all(s in exported for s in NEW_SYMBOLS), sorted(set(NEW_SYMBOLS) - exported)
    lib = _lib.load()
    assert all(hasattr(lib, s) for s in NEW_SYMBOLS)
    hdr = open(os.path.join(ROOT, "include", "sfmhip.h")).read()
    assert all(f"int {s}" in hdr for s in NEW_SYMBOLS)


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not found")
def test_cluster_kernels_have_no_scratch(tmp_path):
    assert os.path.exists(LIB), "build libsfmhip.so first (__graft_entry__.build)"
    t = _kernel_table(tmp_path)
    names = ("cluster_init_kernel", "cluster_link_brute_kernel", "cluster_link_grid_kernel", "cluster_flatten_kernel", "cluster_label_kernel",
             "cluster_border_brute_kernel", "cluster_border_grid_kernel", "cluster_sizes_kernel", "cluster_largest_kernel", "cluster_keep_kernel")
    for frag in names:
        hits = [(k, v) for k, v in t.items() if frag in k]
        assert len(hits) == 1, (frag, sorted(t))
        name, k = hits[0]
        assert k["scratch"] == 0 and (k["spill"] or 0) == 0, (name, k)
        assert k["vgpr"] + k["agpr"] <= 128, (name, k)
        assert k["lds"] <= 8 * 1024, (name, k)               # at most the all-pairs sweeps' tiles: three of coordinates, one of flags
