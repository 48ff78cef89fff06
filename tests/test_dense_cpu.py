"""CPU: the dense-depth definition of include/sfmhip.h on its numpy restatement (tests/dense_ref.py).  Quality is a property of the
definition: it is tested here on the restatement alone, and the bit-equality of tests/test_dense_gpu.py carries it over to the device.
Also the host-only geometry helper against numpy (the library loads without a GPU) and the sweep kernel's resource metadata."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dense_ref as dr
from sfm_opencv_amd import _lib
from test_codeobj_cpu import LIB, READELF, _kernel_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, WMIN, WMAX, R = 48, 1.0 / 8.0, 1.0 / 3.0, 2
STEP = (WMAX - WMIN) / (D - 1)


@pytest.fixture(scope="module")
def scene():
    sc = dr.Scene()
    rendered = [sc.render(v) for v in range(4)]
    return sc, [im for im, _ in rendered], [z for _, z in rendered]


def _sweep0(scene, n_src):
    sc, images, _ = scene
    A, b, *_ = dr.sweep_geometry(sc.K4, sc.EXT[0], sc.EXT[1:1 + n_src])
    return dr.plane_sweep(images[0], images[1:1 + n_src], A, b, D, WMIN, WMAX, R, 1, -1.0)


@pytest.mark.parametrize("n_src,bound", [(3, 0.95), (2, 0.95), (1, 0.90)])
def test_winning_plane_is_the_true_one_away_from_discontinuities(scene, n_src, bound):
    _, _, zs = scene
    plane, score, depth, _ = _sweep0(scene, n_src)
    scored = plane >= 0
    k_true = (1.0 / zs[0] - WMIN) / STEP
    sel = scored & dr.discontinuity_mask(zs[0], R + 2)
    frac = (np.abs(plane[sel] - k_true[sel]) <= 1.0).mean()
    print(f"n_src={n_src}: {frac:.4f} of {sel.sum()} pixels within one plane; {scored.mean():.3f} of all pixels scored")
    assert sel.sum() > 0.5 * plane.size
    assert frac >= bound
    assert np.isnan(depth[~scored]).all() and np.isnan(score[~scored]).all() and np.isfinite(depth[scored]).all()


@pytest.fixture(scope="module")
def chained(scene):
    sc, images, _ = scene
    src = dr.nearest_sources(sc.EXT, 3)
    return dr.chain(images, sc.K4, sc.EXT, src, dr.sweep_geometry, D, WMIN, WMAX, R, 1, -1.0, 0.01, 2)


def test_consistency_keeps_the_true_depths(scene, chained):
    sc, _, zs = scene
    v = chained[0]
    keep = v["keep"].astype(bool)
    good = np.abs(1.0 / v["depth"][keep].astype(np.float64) - 1.0 / zs[0][keep]) <= STEP
    interior = np.zeros_like(keep); interior[R:-R, R:-R] = True
    print(f"kept {keep.sum()} of {interior.sum()} interior pixels, {good.mean():.4f} within one plane step")
    assert good.mean() >= 0.98
    assert keep[interior].sum() >= 0.5 * interior.sum()
    assert not keep[~np.isfinite(v["depth"])].any() and (v["count"][keep] >= 2).all()


def test_exported_points_lie_on_the_planted_planes(scene, chained):
    """a step of the inverse depth w moves a point at depth z by z*z*step along its ray, and the planted planes are tilted by less than
    0.13, so a point within one plane step of the truth is nearer than z_max^2 * step to its plane; the 98 % of the consistency test"""
    sc, images, zs = scene
    for i, v in enumerate(chained):
        assert v["xyz"].shape == (int(v["keep"].sum()), 3) and v["bgr"].shape == v["xyz"].shape
        zmax = zs[i][np.isfinite(zs[i])].max()
        near = sc.plane_distance(v["xyz"]) <= zmax * zmax * STEP
        print(f"view {i}: {len(near)} points, {near.mean():.4f} within {zmax * zmax * STEP:.3f} of a plane")
        assert len(near) >= 0.5 * (sc.ROWS - 2 * R) * (sc.COLS - 2 * R) and near.mean() >= 0.98
        assert (v["bgr"][:, 0] == images[i][v["keep"].astype(bool)]).all()


def test_sweep_geometry_agrees_with_numpy():
    lib = _lib.load()
    rng = np.random.default_rng(3)
    for n_src in (1, 3, 8):
        K4 = np.array([1100.0 + 50 * rng.random(), 1090.0 + 50 * rng.random(), 640.5, 360.25])
        ext_ref = np.concatenate([0.4 * rng.standard_normal(3), rng.standard_normal(3)])
        ext_src = np.concatenate([0.4 * rng.standard_normal((n_src, 3)), rng.standard_normal((n_src, 3))], 1)
        if n_src == 1:
            ext_ref[:3] = 0.0                                       # the small-angle branch
        A = np.zeros((n_src, 9), np.float32); b = np.zeros((n_src, 3), np.float32)
        Rrel = np.zeros((n_src, 9)); trel = np.zeros((n_src, 3)); Rinv = np.zeros(9); c = np.zeros(3)
        rc = lib.sfmhip_sweep_geometry(K4.ctypes.data, ext_ref.ctypes.data, ext_src.ctypes.data, n_src, A.ctypes.data, b.ctypes.data, Rrel.ctypes.data,
                                       trel.ctypes.data, Rinv.ctypes.data, c.ctypes.data)
        assert rc == 0
        eA, eb, eR, et, eRi, ec = dr.sweep_geometry(K4, ext_ref, ext_src)
        for got, exp in ((Rrel, eR), (trel, et), (Rinv, eRi), (c, ec)):
            assert np.abs(got - exp).max() <= 1e-12 * max(1.0, np.abs(exp).max())
        # A and b are the double values rounded to float: half an ulp of float, relative to the row's largest entry
        K = np.array([[K4[0], 0, K4[2]], [0, K4[1], K4[3]], [0, 0, 1.0]])
        for s in range(n_src):
            Ad = K @ eR[s].reshape(3, 3) @ np.linalg.inv(K); bd = K @ et[s]
            assert np.abs(A[s].reshape(3, 3) - Ad).max() <= 2.0 ** -24 * np.abs(Ad).max() + 1e-12 * np.abs(Ad).max()
            assert np.abs(b[s] - bd).max() <= 2.0 ** -24 * np.abs(bd).max() + 1e-12 * np.abs(bd).max()
    # argument rules: the outputs are left alone
    A = np.full(9, 7.0, np.float32)
    K4 = np.array([0.0, 1.0, 0.0, 0.0]); e = np.zeros(6)
    assert lib.sfmhip_sweep_geometry(K4.ctypes.data, e.ctypes.data, e.ctypes.data, 1, A.ctypes.data, None, None, None, None, None) == _lib.E_ARG
    K4[0] = 1.0
    assert lib.sfmhip_sweep_geometry(K4.ctypes.data, e.ctypes.data, e.ctypes.data, 9, A.ctypes.data, None, None, None, None, None) == _lib.E_ARG
    assert lib.sfmhip_sweep_geometry(None, e.ctypes.data, e.ctypes.data, 1, A.ctypes.data, None, None, None, None, None) == _lib.E_ARG
    assert (A == 7.0).all()
    assert lib.sfmhip_sweep_geometry(K4.ctypes.data, e.ctypes.data, e.ctypes.data, 1, A.ctypes.data, None, None, None, None, None) == 0
    assert np.array_equal(A, np.eye(3, dtype=np.float32).ravel())


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not found")
def test_sweep_kernel_without_scratch_and_with_the_lds_the_design_states(tmp_path):
    assert os.path.exists(LIB), "build libsfmhip.so first (__graft_entry__.build)"
    t = _kernel_table(tmp_path)
    hits = sorted(k for k in t if "sweep_kernel" in k)
    assert len(hits) == 6, hits                                            # one instantiation per window radius 0 .. 5
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    said = re.search(r"sweep_kernel keeps (\d+) bytes of LDS", design)
    assert said, "DESIGN.md 4g does not say what sweep_kernel keeps in LDS"
    for name in hits:
        k = t[name]
        assert k["scratch"] == 0 and (k["spill"] or 0) == 0, (name, k)
        assert k["lds"] == int(said.group(1)), (name, k, said.group(0))
        radius = int(re.search(r"ILi(\d)E", name).group(1))
        # 256 threads per workgroup, a wave per SIMD: four workgroups per CU up to the usual radius 2, three at the larger windows
        assert k["vgpr"] + k["agpr"] <= (128 if radius <= 2 else 168), (name, k)
    for name in ("consistency_kernel", "points_write_kernel", "points_count_kernel", "dense_gray_kernel"):
        (kk,) = [t[x] for x in t if name in x]
        assert kk["scratch"] == 0 and (kk["spill"] or 0) == 0, (name, kk)


def test_cpp_mirror_takes_the_same_depth_range_from_sparse_points(tmp_path):
    """sfm::dense_depth_range of host/sfm_ops.hpp against api.dense_depth_range: the same doubles (no GPU call is made)"""
    import struct
    import subprocess
    from sfm_opencv_amd import api
    host = os.path.join(ROOT, "tests", "host")
    subprocess.check_call(["make", "-C", host, "-f", "dense.mk", "dense_test"], stdout=subprocess.DEVNULL)
    rng = np.random.default_rng(11)
    for n in (3, 57, 1000):
        pts = rng.uniform([-2, -2, 3], [2, 2, 9], (n, 3)); pts[0, 2] = -1.0
        ext = np.array([[0.02, -0.05, 0.01, 0.3, -0.1, 0.2]])
        with open(tmp_path / "in.bin", "wb") as f:
            f.write(struct.pack("<10i", 1, 1, 1, 1, 1, 2, 0, 1, 1, n)); f.write(struct.pack("<5d", 0, 0, 0, 0, 0)); f.write(struct.pack("<4d", 1, 1, 0, 0))
            f.write(ext.tobytes()); f.write(pts.tobytes()); f.write(b"\0")
        subprocess.check_call([os.path.join(host, "dense_test"), "range", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
        got = np.fromfile(tmp_path / "out.bin", "<f8")
        exp = np.array(api.dense_depth_range(pts, ext[0]))
        assert 0 < exp[0] < exp[1] and np.array_equal(got, exp), (got, exp)
