"""CPU: the dense mesh as include/sfmhip.h defines it, on its numpy restatement (tests/tsdf_ref.py).  What the definition promises --
outward normals in every tetrahedron case, a closed oriented manifold where the volume is observed, sums that do not depend on how the
views are split -- is tested here on the restatement alone, and the bit-equality of tests/test_tsdf_gpu.py carries it over to the device.
Also the resource metadata of the new kernels against what DESIGN.md 4i states."""
import itertools
import os
import re

import numpy as np
import pytest

import tsdf_ref as tr
from test_codeobj_cpu import LIB, READELF, _kernel_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the 84 cases
def test_every_mixed_tetrahedron_case_has_outward_normals():
    cases = 0
    for tet, sg in zip(tr.TETS, tr.SIGMA):
        P = np.array([tr.corner(c) for c in tet], np.float64)
        for ins in itertools.product((False, True), repeat=4):
            if sum(ins) in (0, 4):
                continue
            cases += 1
            tris = tr.tet_triangles(list(ins), sg)
            assert len(tris) == (2 if sum(ins) == 2 else 1)
            inside = np.array(ins)
            out_dir = P[~inside].mean(0) - P[inside].mean(0)
            for t in tris:
                for x, y in t:
                    assert ins[x] != ins[y]                                       # a vertex lies on an edge that changes sign
                p = [0.5 * (P[x] + P[y]) for x, y in t]                           # every s = 0.5
                nrm = np.cross(p[1] - p[0], p[2] - p[0])
                assert nrm @ out_dir > 0, (tet, ins, t)
            if len(tris) == 2:                                                    # a quad split along Q0 - Q2, both halves turning the same way
                a, b = tris
                common = set(a) & set(b)
                assert a[0] == b[0] and len(common) == 2 and len(set(a) | set(b)) == 4
                (q2,) = common - {a[0]}
                assert not set(q2) & set(a[0])                                    # Q0 = E(k,m) and Q2 = E(l,n) share no corner: the quad's diagonal
    assert cases == 84
    assert tr.SIGMA == [1, -1, -1, 1, 1, -1]


# ------------------------------------------------------------------------------------------------ the analytic sphere
@pytest.fixture(scope="module", params=[16, 17])
def analytic(request):
    n = request.param
    dims, origin, voxel, dsum, wsum = tr.analytic_sphere(n)
    xyz, bgr, tri = tr.mesh(dims, origin, voxel, dsum, wsum, None, 1)
    return n, dims, origin, voxel, dsum, wsum, xyz, tri


def test_analytic_sphere_is_a_closed_oriented_manifold(analytic):
    n, dims, origin, voxel, dsum, wsum, xyz, tri = analytic
    st = tr.mesh_stats(xyz, tri)
    err = np.abs(np.linalg.norm(xyz, axis=1) - 1.0).max() / voxel
    print(f"n = {n}: {len(xyz)} vertices, {len(tri)} triangles, {st}, radius error {err:.4f} voxel, volume {st['volume'] / (4 * np.pi / 3):.4f} of the sphere's")
    assert len(tri) > 500 and tri.min() == 0 and tri.max() == len(xyz) - 1
    assert st["duplicated"] == 0 and st["boundary"] == 0
    assert st["euler"] == 2
    assert st["volume"] > 0 and abs(st["volume"] - 4 * np.pi / 3) <= 0.03 * 4 * np.pi / 3
    assert err <= 0.1


def test_inverted_sphere_has_the_same_vertices_and_the_opposite_volume(analytic):
    n, dims, origin, voxel, dsum, wsum, xyz, tri = analytic
    ixyz, _, itri = tr.mesh(dims, origin, voxel, -dsum - 1, wsum, None, 1)
    st, ist = tr.mesh_stats(xyz, tri), tr.mesh_stats(ixyz, itri)
    assert len(ixyz) == len(xyz) and len(itri) == len(tri)
    assert ist["duplicated"] == 0 and ist["boundary"] == 0 and ist["euler"] == 2
    assert ist["volume"] < 0 and abs(ist["volume"] + st["volume"]) <= 0.01 * st["volume"]


# ------------------------------------------------------------------------------------------------ the fused sphere
N, TRUNC_VOXELS = 24, 3.0


def _fuse(views, order=None, calls=1):
    depths, R, t = views
    dims, origin, voxel = tr.sphere_box(N)
    order = list(range(len(depths))) if order is None else order
    dsum, wsum, _ = tr.new_volume(dims, False)
    for part in np.array_split(np.array(order), calls):
        tr.integrate(dims, origin, voxel, TRUNC_VOXELS * voxel, [depths[i] for i in part], None, None, tr.SPHERE_K4, R[part], t[part], dsum, wsum, None)
    return dims, origin, voxel, dsum, wsum


@pytest.fixture(scope="module")
def views14():
    return tr.sphere_views(14)


def test_fourteen_views_close_the_sphere(views14):
    dims, origin, voxel, dsum, wsum = _fuse(views14)
    xyz, _, tri = tr.mesh(dims, origin, voxel, dsum, wsum, None, 1)
    st = tr.mesh_stats(xyz, tri)
    err = np.abs(np.linalg.norm(xyz, axis=1) - 1.0).max() / voxel
    print(f"14 views: {len(xyz)} vertices, {len(tri)} triangles, {st}, radius error {err:.4f} voxel, weights {wsum.min()} .. {wsum.max()}")
    assert len(tri) > 1000 and st["duplicated"] == 0 and st["boundary"] == 0 and st["euler"] == 2 and st["volume"] > 0
    assert err <= 1.0                                                             # the bias of the projective distance, below a voxel


def test_six_axis_views_leave_the_surface_open_not_broken(views14):
    """min_weight and coverage decide closure, not the extractor: what is extracted is still oriented consistently"""
    depths, R, t = views14
    dims, origin, voxel, dsum, wsum = _fuse((depths[:6], R[:6], t[:6]))
    xyz, _, tri = tr.mesh(dims, origin, voxel, dsum, wsum, None, 1)
    st = tr.mesh_stats(xyz, tri)
    print(f"6 views: {len(xyz)} vertices, {len(tri)} triangles, {st}")
    assert len(tri) > 1000 and st["duplicated"] == 0 and st["boundary"] > 0


def test_the_volume_does_not_depend_on_how_the_views_are_split(views14):
    one = _fuse(views14)
    three = _fuse(views14, calls=3)
    back = _fuse(views14, order=list(range(13, -1, -1)), calls=2)
    for other in (three, back):
        assert np.array_equal(one[3], other[3]) and np.array_equal(one[4], other[4])
    assert one[4].max() >= 3 and (one[3] != 0).any()


def test_colour_and_keep_maps_enter_the_sums(views14):
    depths, R, t = views14
    dims, origin, voxel = tr.sphere_box(12)
    rng = np.random.default_rng(3)
    imgs = [rng.integers(0, 256, (96, 96, 3), dtype=np.uint8) for _ in range(2)]
    keep = (np.indices((96, 96)).sum(0) % 2).astype(np.uint8)
    d0, w0, c0 = tr.new_volume(dims)
    tr.integrate(dims, origin, voxel, 3 * voxel, depths[:2], None, imgs, tr.SPHERE_K4, R[:2], t[:2], d0, w0, c0)
    d1, w1, c1 = tr.new_volume(dims)
    tr.integrate(dims, origin, voxel, 3 * voxel, depths[:2], [keep, None], imgs, tr.SPHERE_K4, R[:2], t[:2], d1, w1, c1)
    assert (w1 <= w0).all() and 0 < w1.sum() < w0.sum() and (c0.sum(1) <= 3 * 255 * w0).all() and c0.dtype == np.uint32
    assert ((c0 == 0).all(1) | (w0 > 0)).all()
    xyz, bgr, tri = tr.mesh(dims, origin, voxel, d0, w0, c0, 1)
    assert bgr.shape == xyz.shape and bgr.dtype == np.uint8 and len(tri) > 0


# ------------------------------------------------------------------------------------------------ code objects
KERNELS = ("tsdf_integrate_kernel", "tsdf_cell_kernel", "tsdf_edge_kernel", "tsdf_vertex_kernel", "tsdf_triangle_kernel")


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not found")
def test_tsdf_kernels_without_scratch_and_with_the_lds_the_design_states(tmp_path):
    assert os.path.exists(LIB), "build libsfmhip.so first (__graft_entry__.build)"
    t = _kernel_table(tmp_path)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert sorted(k for k in t if "tsdf" in k and not any(name in k for name in KERNELS)) == []
    for kernel in KERNELS:
        hits = sorted(k for k in t if kernel in k)
        assert len(hits) == 1, (kernel, hits)
        said = re.search(kernel + r" keeps (\d+) bytes of LDS and stays within (\d+) registers", design)
        assert said, f"DESIGN.md 4i does not say what {kernel} keeps in LDS and how many registers it may take"
        k = t[hits[0]]
        assert k["scratch"] == 0 and (k["spill"] or 0) == 0, (kernel, k)
        assert k["lds"] == int(said.group(1)), (kernel, k, said.group(0))
        assert int(said.group(2)) <= 64 and k["vgpr"] + k["agpr"] <= int(said.group(2)), (kernel, k)     # eight waves per SIMD
