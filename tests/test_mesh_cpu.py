"""CPU: the mesh clean-up as include/sfmhip.h defines it, on its numpy restatement (tests/mesh_ref.py).  What the definitions are good for
-- components that are the graph's, outward normals, smoothing that behaves as Laplacian and Taubin smoothing do, a simplification that
leaves a clean smaller mesh near the old one -- is tested here on the restatement alone, and the bit-equality of tests/test_mesh_gpu.py
carries it over to the device.  Also the resource metadata of the kernels of mesh.hip and the declarations in the header."""
import os
import re

import numpy as np
import pytest

import mesh_ref as mr
import tsdf_ref as tr
from sfm_opencv_amd import _lib
from test_codeobj_cpu import LIB, READELF, _kernel_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ components
def test_components_are_those_of_the_vertex_graph():
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    xyz, bgr, tri = mr.two_spheres_and_fragments()
    nv = len(xyz)
    tri_label, vertex_label, sizes = mr.components(nv, tri)
    tv = tri[mr.valid_mask(nv, tri)]
    e = np.concatenate([tv[:, [0, 1]], tv[:, [0, 2]]])
    n_all, lab = connected_components(coo_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(nv, nv)), directed=False)
    ref = vertex_label >= 0
    assert ref.sum() == len(np.unique(tv)) and (~ref).sum() >= 5
    assert len(sizes) == len(np.unique(lab[ref])) == 2 + 6                          # two spheres and six fragments
    # the same partition of the referenced vertices: a bijection between the two numberings
    pairs = np.unique(np.stack([vertex_label[ref], lab[ref]], 1), axis=0)
    assert len(pairs) == len(sizes) and len(np.unique(pairs[:, 0])) == len(np.unique(pairs[:, 1])) == len(sizes)
    # numbered by the smallest vertex, sizes in triangles, invalid triangles out
    firsts = [np.flatnonzero(vertex_label == c)[0] for c in range(len(sizes))]
    assert firsts == sorted(firsts)
    assert sizes.sum() == len(tv) == len(tri) - 2 and (tri_label == -1).sum() == 2
    assert sorted(sizes.tolist())[:6] == [1, 1, 1, 1, 2, 2] and sizes.max() == len(mr.sphere_mesh(16)[1])
    # the filter: the fragments go, the largest is the first sphere (the smaller number of the two equals)
    fx, fb, ft, vmap = mr.filter_components(xyz, bgr, tri, min_triangles=3)
    assert len(ft) == 2 * len(mr.sphere_mesh(16)[1]) and len(fx) == 2 * len(mr.sphere_mesh(16)[0])
    lx, lb, lt, lmap = mr.filter_components(xyz, bgr, tri, keep_largest=True)
    assert np.array_equal(lx, mr.sphere_mesh(16)[0]) and len(lt) == len(mr.sphere_mesh(16)[1])
    st = tr.mesh_stats(lx, lt)
    assert st["boundary"] == 0 and st["duplicated"] == 0 and st["euler"] == 2


# ------------------------------------------------------------------------------------------------ normals and smoothing on the sphere
@pytest.mark.parametrize("n", [16, 24])
def test_normals_point_outwards_on_the_sphere(n):
    xyz, tri, _ = mr.sphere_mesh(n)
    nrm = mr.vertex_normals(xyz, tri)
    dots = (nrm * xyz).sum(1) / np.linalg.norm(xyz, axis=1)
    print(f"n = {n}: minimum of normal . radial {dots.min():.4f}")
    assert np.allclose(np.linalg.norm(nrm, axis=1), 1.0, atol=1e-12)
    assert (dots > 0).all()


@pytest.mark.parametrize("n", [16, 24])
def test_laplacian_shrinks_and_taubin_keeps_the_volume(n):
    xyz, tri, _ = mr.sphere_mesh(n)
    v0 = tr.mesh_stats(xyz, tri)["volume"]
    vols = [tr.mesh_stats(mr.smooth(xyz, tri, k, 0.5, 0.0), tri)["volume"] for k in range(1, 11)]
    assert all(b < a for a, b in zip([v0] + vols, vols))                            # every Laplacian step lowers the volume
    taubin = tr.mesh_stats(mr.smooth(xyz, tri, 10, 0.5, -0.53), tri)["volume"]
    print(f"n = {n}: volume after 10 iterations, of the original: Taubin {taubin / v0:.4f}, Laplacian {vols[-1] / v0:.4f}")
    assert abs(taubin - v0) < abs(vols[-1] - v0)
    assert np.array_equal(mr.smooth(xyz, tri, 0, 0.5, -0.53), xyz)
    # the step is a step: two Laplacian iterations are one after the other
    assert np.array_equal(mr.smooth(mr.smooth(xyz, tri, 1, 0.5, 0.0), tri, 1, 0.5, 0.0), mr.smooth(xyz, tri, 2, 0.5, 0.0))


# ------------------------------------------------------------------------------------------------ simplification
@pytest.mark.parametrize("n,cells", [(16, 2.0), (16, 3.0), (24, 2.0), (24, 3.0)])
def test_simplification_leaves_a_clean_smaller_mesh_near_the_old_one(n, cells):
    xyz, tri, voxel = mr.sphere_mesh(n)
    sx, sb, st, vmap = mr.simplify(xyz, mr.colours(len(xyz)), tri, cells * voxel)
    print(f"n = {n}, {cells} voxels: {len(xyz)} -> {len(sx)} vertices, {len(tri)} -> {len(st)} triangles, {tr.mesh_stats(sx, st)}")
    assert 0 < len(sx) < len(xyz) and 0 < len(st) < len(tri) and sb.shape == sx.shape
    assert (st[:, 0] != st[:, 1]).all() and (st[:, 1] != st[:, 2]).all() and (st[:, 0] != st[:, 2]).all()
    assert (st[:, 0] < st[:, 1]).all() and (st[:, 0] < st[:, 2]).all()              # rotated: the smallest index first
    assert len(np.unique(st, axis=0)) == len(st) and np.array_equal(st, np.unique(st, axis=0))
    assert np.array_equal(np.unique(st), np.arange(len(sx)))                        # no unreferenced vertex
    moved = np.linalg.norm(xyz[vmap >= 0] - sx[vmap[vmap >= 0]], axis=1)
    assert (vmap >= 0).all() and moved.max() <= cells * voxel * np.sqrt(3.0)
    assert tr.mesh_stats(sx, st)["volume"] > 0.8 * tr.mesh_stats(xyz, tri)["volume"]


def test_the_24_sphere_at_two_voxels_is_still_a_closed_sphere():
    xyz, tri, voxel = mr.sphere_mesh(24)
    sx, _, st, _ = mr.simplify(xyz, None, tri, 2.0 * voxel)
    stats = tr.mesh_stats(sx, st)
    assert stats["boundary"] == 0 and stats["duplicated"] == 0 and stats["euler"] == 2


def test_hand_made_cases_of_the_definition():
    H = mr.hand_made()
    xyz, bgr, tri = H["tie"]
    tl, vl, sizes = mr.components(len(xyz), tri)
    assert tl.tolist() == [1, 1, 0, 0] and sizes.tolist() == [2, 2] and vl.tolist() == [0, 0, 0, 1, 1, 1, 0, 1]
    assert mr.filter_components(xyz, bgr, tri, keep_largest=True)[2].tolist() == [[0, 1, 2], [2, 1, 3]]
    xyz, bgr, tri = H["bowtie"]
    assert mr.components(len(xyz), tri)[2].tolist() == [2]                          # a shared vertex connects
    xyz, bgr, tri = H["vvv"]
    tl, vl, sizes = mr.components(len(xyz), tri)
    assert tl.tolist() == [0, 1, 0] and vl[6] == 1 and sizes.tolist() == [2, 1]
    assert (mr.vertex_normals(xyz, tri)[6] == 0).all() and np.array_equal(mr.smooth(xyz, tri, 3, 0.5, 0.0)[6], xyz[6])
    xyz, bgr, tri = H["out_of_range"]
    assert mr.components(len(xyz), tri)[0].tolist() == [0, -1, -1, 1, -1]
    xyz, bgr, tri = H["duplicates"]
    sx, sb, st, vmap = mr.simplify(xyz, bgr, tri, 0.1)                              # every vertex its own cluster
    assert len(st) == 3 and len(sx) == 6 and vmap.tolist() == [0, 2, 1, 3, 4, 5, -1, -1]   # clusters in ascending (x, y, z) cell
    xyz, bgr, tri = H["nan"]
    assert (mr.simplify(xyz, bgr, tri, 0.1)[3][3] == -1) and len(mr.simplify(xyz, bgr, tri, 0.1)[2]) == 1
    for name in ("nv0", "nt0", "both0"):
        xyz, bgr, tri = H[name]
        assert len(mr.components(len(xyz), tri)[2]) == 0 and len(mr.simplify(xyz, bgr, tri, 0.5)[0]) == 0
        assert len(mr.filter_components(xyz, bgr, tri)[2]) == 0 and mr.smooth(xyz, tri, 2, 0.5, -0.53).shape == xyz.shape


# ------------------------------------------------------------------------------------------------ code objects, declarations
@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not found")
def test_mesh_kernels_without_scratch(tmp_path):
    """every kernel of mesh.hip: no scratch, no spills, at most 64 registers (eight waves per SIMD), and the LDS DESIGN.md 4j states.
    Reads the kernel metadata only."""
    assert os.path.exists(LIB), "build libsfmhip.so first (__graft_entry__.build)"
    t = _kernel_table(tmp_path)
    src = open(os.path.join(ROOT, "sfm_opencv_amd", "csrc", "mesh.hip")).read()
    names = re.findall(r"__global__ __launch_bounds__\(256\) void (mesh_[a-z0-9_]+)\(", src)
    assert len(names) == len(set(names)) >= 20
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for kernel in names:
        hits = sorted(k for k in t if k.startswith(f"_Z{len(kernel)}{kernel}"))        # the mangled name: its length, then the name
        assert len(hits) == 1, (kernel, hits)
        k = t[hits[0]]
        assert k["scratch"] == 0 and (k["spill"] or 0) == 0, (kernel, k)
        assert k["vgpr"] + k["agpr"] <= 64, (kernel, k)
        said = re.search(kernel + r" keeps (\d+) bytes of LDS", design)
        assert k["lds"] == (int(said.group(1)) if said else 0), (kernel, k)


def test_the_header_declares_the_new_calls():
    hdr = open(os.path.join(ROOT, "include", "sfmhip.h")).read()
    for base in ("components", "filter_components", "simplify", "vertex_normals", "smooth"):
        for form in ("", "_dev"):
            name = f"sfmhip_mesh_{base}{form}"
            assert re.search(r"\bint " + name + r"\s*\(", hdr), name
            assert name in _lib.SYMBOLS and hasattr(_lib.load(), name)
    assert "cluster_connected_triangles" in hdr and "NO boundary pinning" in hdr
