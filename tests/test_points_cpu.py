"""CPU side of the point-cloud neighbour search (sfmhip_knn_points and friends): the numpy reference of tests/points_ref.py agrees with
itself (all pairs against kd-tree candidates), the binding and the library carry the new entry points, and the two search kernels are
compiled the way they were designed: no scratch, registers for four waves per SIMD."""
import os
import subprocess

import numpy as np
import pytest

import points_ref as pr
from sfm_opencv_amd import _lib
from test_codeobj_cpu import LIB, READELF, _kernel_table

NEW_SYMBOLS = ["sfmhip_knn_points", "sfmhip_knn_points_dev", "sfmhip_estimate_normals_ex", "sfmhip_statistical_outliers"]


def _clouds():
    rng = np.random.default_rng(5)
    yield "random 3000", rng.uniform(-1, 1, (3000, 3))
    p = rng.uniform(-1, 1, (1000, 3)); p[800:] = p[rng.integers(0, 800, 200)]
    yield "1000 with 200 exact duplicates", p
    yield "12^3 lattice", pr.lattice(12)


@pytest.mark.parametrize("K", [1, 10, 16])
def test_reference_forms_agree(K):
    for name, pts in _clouds():
        ia, da = pr.knn_allpairs(pts, K)
        ik, dk, redone = pr.knn_kdtree(pts, K)
        assert np.array_equal(ia, ik), name
        assert np.array_equal(da.view(np.uint64), dk.view(np.uint64)), name
        assert redone < len(pts) or "duplicates" in name or "lattice" in name, name      # the kd-tree path is exercised
        # the rule itself, row by row on a few rows: ascending (d, j), self excluded
        for i in (0, len(pts) // 2, len(pts) - 1):
            assert i not in ia[i]
            key = list(zip(da[i], ia[i]))
            assert key == sorted(key)


def test_reference_handles_missing_and_non_finite():
    pts = np.array([[0, 0, 0], [1, 0, 0], [np.nan, 0, 0], [0, 2, 0], [np.inf, 1, 1]], float)
    idx, dist = pr.knn_allpairs(pts, 3)
    assert idx.tolist() == [[1, 3, -1], [0, 3, -1], [-1, -1, -1], [0, 1, -1], [-1, -1, -1]]
    assert np.isinf(dist[idx < 0]).all() and dist[0, 0] == 1.0 and dist[0, 1] == 2.0
    i2, d2, _ = pr.knn_kdtree(pts, 3)
    assert np.array_equal(idx, i2) and np.array_equal(dist.view(np.uint64), d2.view(np.uint64))
    keep, m, st = pr.statistical_outliers(idx, dist, 2.0)
    assert np.isinf(m).all() and not keep.any() and np.isnan(st).all()


def test_binding_and_library_carry_the_point_cloud_entry_points():
    assert all(s in _lib.SYMBOLS for s in NEW_SYMBOLS)
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.split()}
    assert all(s in exported for s in NEW_SYMBOLS), sorted(set(NEW_SYMBOLS) - exported)
    lib = _lib.load()
    assert all(hasattr(lib, s) for s in NEW_SYMBOLS)
    assert _lib.POINTS_METHODS == {"auto": 0, "brute": 1, "grid": 2}
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sfmhip.h")).read()
    for name, val in (("SFMHIP_POINTS_AUTO", 0), ("SFMHIP_POINTS_BRUTE", 1), ("SFMHIP_POINTS_GRID", 2)):
        assert f"#define {name}" in hdr and hdr.split(f"#define {name}")[1].split()[0] == str(val)


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not found")
def test_search_kernels_have_no_scratch_and_fit_four_waves_per_simd(tmp_path):
    """Both kernels keep the sorted top-16 of a query (16 doubles + 16 indices = 48 registers) in VGPRs and are built around workgroups of
    256 threads at FOUR waves per SIMD -- four workgroups per CU, which is what hides the latency of the binary searches and of the
    candidate loads of the grid kernel: at most 128 VGPRs (512 per SIMD lane / 4), nothing in scratch, nothing spilled."""
    assert os.path.exists(LIB), "build libsfmhip.so first (__graft_entry__.build)"
    t = _kernel_table(tmp_path)
    for frag, lds in (("points_knn_grid_kernel", 0), ("points_knn_brute_kernel", 3 * 256 * 8)):
        hits = [(k, v) for k, v in t.items() if frag in k]
        assert len(hits) == 1, (frag, sorted(t))
        name, k = hits[0]
        assert k["scratch"] == 0 and (k["spill"] or 0) == 0, (name, k)
        assert k["vgpr"] + k["agpr"] <= 128, (name, k)
        assert k["lds"] == lds, (name, k)
