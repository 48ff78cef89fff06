"""GPU: the mesh clean-up (sfmhip_mesh_components, _filter_components, _simplify, _vertex_normals, _smooth) against the numpy restatement of
its definition (tests/mesh_ref.py): every byte of every output of every call is equal.  Then determinism, the entry forms, the argument
rules, an injected allocation failure, and the layers above (api.dense_mesh_for_all, the .ply writer and the C++ mirror)."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import mesh_ref as mr
import tsdf_ref as tr
from sfm_opencv_amd import _lib, api, formats
from test_tsdf_gpu import N_SRC, PLANES, SCENE_MIN_WEIGHT, SCENE_TRUNC_VOXELS, SCENE_VOLUME, WMAX, WMIN, planted  # noqa: F401  (planted: a fixture)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _same(a, b):
    a = np.asarray(a); b = np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _same_mesh(got, exp):
    return all((g is None and e is None) or _same(g, e) for g, e in zip(got, exp)) and len(got) == len(exp)


def _check_all(ctx, xyz, bgr, tri, cells, steps=2):
    """every call on one mesh against the restatement; cells: the cluster cells to simplify with"""
    nv = len(xyz)
    got = ctx.mesh_components(nv, tri)
    exp = mr.components(nv, tri)
    assert _same_mesh(got, exp), "components"
    for mt, kl in ((1, False), (3, False), (1, True), (2, True)):
        assert _same_mesh(ctx.mesh_filter_components(xyz, bgr, tri, mt, kl), mr.filter_components(xyz, bgr, tri, mt, kl)), ("filter", mt, kl)
    for cell in cells:
        assert _same_mesh(ctx.mesh_simplify(xyz, bgr, tri, cell), mr.simplify(xyz, bgr, tri, cell)), ("simplify", cell)
    assert _same(ctx.mesh_vertex_normals(xyz, tri), mr.vertex_normals(xyz, tri)), "normals"
    assert _same(ctx.mesh_smooth(xyz, tri, steps, 0.5, 0.0), mr.smooth(xyz, tri, steps, 0.5, 0.0)), "laplacian"
    assert _same(ctx.mesh_smooth(xyz, tri, steps, 0.5, -0.53), mr.smooth(xyz, tri, steps, 0.5, -0.53)), "taubin"
    return exp


# ------------------------------------------------------------------------------------------------ shapes
@pytest.mark.parametrize("n", [16, 24])
def test_sphere_meshes_equal_the_restatement(ctx, n):
    xyz, tri, voxel = mr.sphere_mesh(n)
    _, _, sizes = _check_all(ctx, xyz, mr.colours(len(xyz)), tri, (2 * voxel, 3 * voxel, 1.5 * voxel), steps=3)
    assert sizes.tolist() == [len(tri)]
    assert _same(ctx.mesh_smooth(xyz, tri, 10, 0.5, -0.53), mr.smooth(xyz, tri, 10, 0.5, -0.53))


def test_two_spheres_and_fragments_equal_the_restatement(ctx):
    xyz, bgr, tri = mr.two_spheres_and_fragments()
    _, _, sizes = _check_all(ctx, xyz, bgr, tri, (0.4, 0.15))
    assert len(sizes) == 8
    assert _same_mesh(ctx.mesh_filter_components(xyz, None, tri, 3, False), mr.filter_components(xyz, None, tri, 3, False))       # without colours
    assert _same_mesh(ctx.mesh_simplify(xyz, None, tri, 0.4), mr.simplify(xyz, None, tri, 0.4))


@pytest.mark.parametrize("name", sorted(mr.hand_made()))
def test_hand_made_meshes_equal_the_restatement(ctx, name):
    xyz, bgr, tri = mr.hand_made()[name]
    _check_all(ctx, xyz, bgr, tri, (0.1, 0.75, 10.0))


@pytest.mark.parametrize("shuffled", [False, True])
def test_a_strip_of_5000_triangles(ctx, shuffled):
    """the chain shape that makes union-find trees deep, in index order and shuffled"""
    xyz, tri = mr.strip(5000, shuffled)
    _, vl, sizes = _check_all(ctx, xyz, mr.colours(len(xyz)), tri, (1.3,))
    assert sizes.tolist() == [5000] and (vl == 0).all()


@pytest.fixture(scope="module")
def random_mesh():
    xyz, tri = mr.random_mesh()
    return xyz, mr.colours(len(xyz)), tri


def test_300000_random_triangles(ctx, random_mesh):
    """more than one grid row of workgroups, indices above 2^16 (several radix digits), sort lengths off the tile size"""
    xyz, bgr, tri = random_mesh
    assert len(tri) % 256 != 0 and tri.max() > 1 << 16
    _, _, sizes = _check_all(ctx, xyz, bgr, tri, (0.05,), steps=1)
    assert sizes.max() > 100000


def test_more_than_2_to_21_vertices_sorts_the_triangles_in_two_passes(ctx):
    """three times the bits of a cluster number no longer fit one 64-bit key from 2^21 vertices on"""
    nv = (1 << 21) + 5
    rng = np.random.default_rng(9)
    xyz = rng.uniform(-1.0, 1.0, (nv, 3))
    tri = rng.integers(0, nv, (3000, 3)).astype(np.int32)
    tri[:50] = rng.integers(nv - 40, nv, (50, 3))                                             # the top of the index range
    tri[50:60] = tri[40:50][:, [1, 2, 0]]                                                     # duplicates under rotation
    for cell in (0.01, 0.3):
        assert _same_mesh(ctx.mesh_simplify(xyz, None, tri, cell), mr.simplify(xyz, None, tri, cell)), cell
    assert _same(ctx.mesh_vertex_normals(xyz, tri), mr.vertex_normals(xyz, tri))
    assert _same_mesh(ctx.mesh_components(nv, tri), mr.components(nv, tri))


def test_a_cluster_cell_too_small_for_the_extent_is_an_argument_error(ctx):
    xyz, bgr, tri = mr.hand_made()["bowtie"]
    with pytest.raises(OverflowError):
        mr.simplify(xyz, bgr, tri, 1e-7)
    with pytest.raises(api.SfmHipError):
        ctx.mesh_simplify(xyz, bgr, tri, 1e-7)
    assert _same_mesh(ctx.mesh_simplify(xyz, bgr, tri, 0.1), mr.simplify(xyz, bgr, tri, 0.1))


# ------------------------------------------------------------------------------------------------ determinism and entry forms
def test_two_runs_give_the_same_bytes(ctx, random_mesh):
    xyz, bgr, tri = random_mesh
    for call in (lambda: ctx.mesh_components(len(xyz), tri), lambda: ctx.mesh_filter_components(xyz, bgr, tri, 2, False), lambda: ctx.mesh_simplify(xyz, bgr, tri, 0.05),
                 lambda: (ctx.mesh_vertex_normals(xyz, tri),), lambda: (ctx.mesh_smooth(xyz, tri, 2, 0.5, -0.53),)):
        assert _same_mesh(call(), call())


def test_zero_iterations_are_a_copy(ctx):
    xyz, tri, _ = mr.sphere_mesh(16)
    assert _same(ctx.mesh_smooth(xyz, tri, 0, 0.5, -0.53), xyz) and _same(ctx.mesh_smooth(xyz, tri, 0, 0.5, 0.0), xyz)


def test_dev_forms_on_resident_arrays_equal_the_host_forms(ctx):
    import torch
    xyz, bgr, tri = mr.two_spheres_and_fragments()
    nv, nt = len(xyz), len(tri)
    dev = torch.device("cuda", ctx.device)
    d_xyz, d_bgr, d_tri = torch.from_numpy(xyz).to(dev), torch.from_numpy(bgr).to(dev), torch.from_numpy(tri).to(dev)

    def i32(n, fill=-7):
        return torch.full((max(n, 1),), fill, dtype=torch.int32, device=dev)
    tl, vl, sz, n = i32(nt), i32(nv), i32(nt), i32(2)
    ctx.mesh_components_dev(nv, d_tri, nt, tl, vl, n[0:1], sz)
    ctx.synchronize()
    etl, evl, esz = ctx.mesh_components(nv, tri)
    assert n[0].item() == len(esz) and _same(tl.cpu().numpy(), etl) and _same(vl.cpu().numpy(), evl)
    assert _same(sz.cpu().numpy(), np.concatenate([esz, np.zeros(nt - len(esz), np.int32)]))                # all nt entries, zero from C on
    for call, params, host in ((ctx.mesh_filter_components_dev, (3, True), ctx.mesh_filter_components(xyz, bgr, tri, 3, True)),
                               (ctx.mesh_filter_components_dev, (1, False), ctx.mesh_filter_components(xyz, bgr, tri, 1, False)),
                               (ctx.mesh_simplify_dev, (0.4,), ctx.mesh_simplify(xyz, bgr, tri, 0.4))):
        o_xyz = torch.zeros((nv, 3), dtype=torch.float64, device=dev); o_bgr = torch.zeros((nv, 3), dtype=torch.uint8, device=dev)
        o_tri = torch.zeros((nt, 3), dtype=torch.int32, device=dev); vmap = i32(nv)
        call(d_xyz, d_bgr, nv, d_tri, nt, *params, o_xyz, o_bgr, o_tri, vmap, n[0:1], n[1:2])
        ctx.synchronize()
        mv, mt = n.cpu().numpy().tolist()
        assert _same_mesh((o_xyz[:mv].cpu().numpy(), o_bgr[:mv].cpu().numpy(), o_tri[:mt].cpu().numpy(), vmap.cpu().numpy()), host), params
        assert (o_xyz[mv:] == 0).all().item() and (o_tri[mt:] == 0).all().item()                            # only the first rows are written
    o = torch.zeros((nv, 3), dtype=torch.float64, device=dev)
    ctx.mesh_vertex_normals_dev(d_xyz, nv, d_tri, nt, o)
    ctx.synchronize()
    assert _same(o.cpu().numpy(), ctx.mesh_vertex_normals(xyz, tri))
    for its, mu in ((1, 0.0), (2, 0.0), (3, -0.53), (0, -0.53)):
        ctx.mesh_smooth_dev(d_xyz, nv, d_tri, nt, its, 0.5, mu, o)
        ctx.synchronize()
        assert _same(o.cpu().numpy(), ctx.mesh_smooth(xyz, tri, its, 0.5, mu)), (its, mu)


# ------------------------------------------------------------------------------------------------ errors
class _Raw:
    """the host forms straight through ctypes on outputs that hold a sentinel"""

    def __init__(self, ctx, xyz, bgr, tri):
        self.ctx, self.xyz, self.bgr, self.tri = ctx, np.ascontiguousarray(xyz), np.ascontiguousarray(bgr), np.ascontiguousarray(tri)
        self.nv, self.nt = len(xyz), len(tri)
        self.reset()

    def reset(self):
        nv, nt = self.nv, self.nt
        self.o_xyz = np.full((nv, 3), -7.0); self.o_bgr = np.full((nv, 3), 0xCD, np.uint8); self.o_tri = np.full((nt, 3), -9, np.int32)
        self.o_map = np.full(nv, -11, np.int32); self.o_lab = np.full(nt, -13, np.int32); self.o_vlab = np.full(nv, -15, np.int32); self.o_sz = np.full(nt, -17, np.int32)
        self.m, self.k = C.c_int(-5), C.c_int(-6)

    def untouched(self):
        return bool((self.o_xyz == -7.0).all() and (self.o_bgr == 0xCD).all() and (self.o_tri == -9).all() and (self.o_map == -11).all() and (self.o_lab == -13).all() and
                    (self.o_vlab == -15).all() and (self.o_sz == -17).all() and (self.m.value, self.k.value) == (-5, -6))

    def call(self, which, **kw):
        a = dict(xyz=self.xyz.ctypes.data, bgr=self.bgr.ctypes.data, nv=self.nv, tri=self.tri.ctypes.data, nt=self.nt, o_xyz=self.o_xyz.ctypes.data,
                 o_bgr=self.o_bgr.ctypes.data, o_tri=self.o_tri.ctypes.data, o_map=self.o_map.ctypes.data, m=C.byref(self.m), k=C.byref(self.k), min_triangles=1,
                 keep_largest=0, voxel=0.4, iterations=2, lam=0.5, mu=-0.53, o_lab=self.o_lab.ctypes.data, o_vlab=self.o_vlab.ctypes.data, o_sz=self.o_sz.ctypes.data)
        a.update(kw)
        lib, h = self.ctx.lib, self.ctx.h
        if which == "components":
            return lib.sfmhip_mesh_components(h, a["nv"], a["tri"], a["nt"], a["o_lab"], a["o_vlab"], a["m"], a["o_sz"])
        if which == "filter":
            return lib.sfmhip_mesh_filter_components(h, a["xyz"], a["bgr"], a["nv"], a["tri"], a["nt"], a["min_triangles"], a["keep_largest"], a["o_xyz"], a["o_bgr"],
                                                     a["o_tri"], a["o_map"], a["m"], a["k"])
        if which == "simplify":
            return lib.sfmhip_mesh_simplify(h, a["xyz"], a["bgr"], a["nv"], a["tri"], a["nt"], a["voxel"], a["o_xyz"], a["o_bgr"], a["o_tri"], a["o_map"], a["m"], a["k"])
        if which == "normals":
            return lib.sfmhip_mesh_vertex_normals(h, a["xyz"], a["nv"], a["tri"], a["nt"], a["o_xyz"])
        return lib.sfmhip_mesh_smooth(h, a["xyz"], a["nv"], a["tri"], a["nt"], a["iterations"], a["lam"], a["mu"], a["o_xyz"])


CALLS = ("components", "filter", "simplify", "normals", "smooth")


def test_bad_arguments_leave_the_outputs_alone(ctx):
    xyz, bgr, tri = mr.two_spheres_and_fragments()
    r = _Raw(ctx, xyz, bgr, tri)
    inf, nan = float("inf"), float("nan")
    bad = {"components": [dict(nv=-1), dict(nt=-1), dict(nv=(1 << 30) + 1), dict(nt=(1 << 28) + 1), dict(tri=None), dict(o_lab=None), dict(m=None), dict(o_lab=r.tri.ctypes.data)],
           "filter": [dict(nv=-1), dict(nt=-1), dict(nv=(1 << 30) + 1), dict(nt=(1 << 28) + 1), dict(xyz=None), dict(tri=None), dict(o_xyz=None), dict(o_bgr=None),
                      dict(o_tri=None), dict(m=None), dict(k=None), dict(min_triangles=0), dict(min_triangles=-3), dict(keep_largest=2), dict(keep_largest=-1),
                      dict(o_xyz=r.xyz.ctypes.data), dict(o_tri=r.tri.ctypes.data), dict(o_bgr=r.bgr.ctypes.data)],
           "simplify": [dict(nv=-1), dict(nt=-1), dict(xyz=None), dict(tri=None), dict(o_xyz=None), dict(o_bgr=None), dict(o_tri=None), dict(m=None), dict(k=None),
                        dict(voxel=0.0), dict(voxel=-1.0), dict(voxel=inf), dict(voxel=nan), dict(o_xyz=r.xyz.ctypes.data), dict(voxel=1e-7)],
           "normals": [dict(nv=-1), dict(nt=-1), dict(xyz=None), dict(tri=None), dict(o_xyz=None), dict(o_xyz=r.xyz.ctypes.data)],
           "smooth": [dict(nv=-1), dict(nt=-1), dict(xyz=None), dict(tri=None), dict(o_xyz=None), dict(o_xyz=r.xyz.ctypes.data), dict(iterations=-1), dict(iterations=1001),
                      dict(lam=inf), dict(lam=nan), dict(mu=-inf), dict(mu=nan)]}
    for which in CALLS:
        for kw in bad[which]:
            assert r.call(which, **kw) == _lib.E_ARG, (which, kw)
            assert r.untouched(), (which, kw)
    # what is allowed: no colours, no map, no vertex labels, no sizes, 1000 iterations' worth of arguments on an empty mesh
    assert r.call("filter", bgr=None, o_bgr=None, o_map=None) == 0 and (r.o_bgr == 0xCD).all() and (r.o_map == -11).all() and r.m.value > 0
    assert r.call("components", o_vlab=None, o_sz=None) == 0 and (r.o_vlab == -15).all() and (r.o_sz == -17).all() and r.m.value == 8
    assert r.call("smooth", nv=0, nt=0, xyz=None, tri=None, o_xyz=None, iterations=1000) == 0


def test_a_failed_allocation_is_an_error_and_the_next_call_works(ctx):
    xyz, bgr, tri = mr.two_spheres_and_fragments()
    r = _Raw(ctx, xyz, bgr, tri)
    for which in CALLS:
        for failing in (1, 2):                                                                # the next `failing` allocations fail
            assert ctx.lib.sfmhip_debug_fail_allocations(ctx.h, failing) == 0
            for _ in range(failing):
                assert r.call(which) == _lib.E_HIP and r.untouched(), which
            assert r.call(which) == 0 and not r.untouched(), which
            r.reset()
    assert ctx.lib.sfmhip_debug_fail_allocations(ctx.h, 1) == 0
    with pytest.raises(api.SfmHipError):
        ctx.mesh_simplify(xyz, bgr, tri, 0.4)
    assert _same_mesh(ctx.mesh_simplify(xyz, bgr, tri, 0.4), mr.simplify(xyz, bgr, tri, 0.4))


# ------------------------------------------------------------------------------------------------ the layers above
OPTIONS = dict(min_component=20, keep_largest=False, simplify_voxels=2.0, smooth=(3, 0.5, -0.53), normals=True)


def _scene(ctx, p, **options):
    return api.dense_mesh_for_all(p["images"], p["sc"].K4, p["sc"].EXT, n_src=N_SRC, planes=PLANES, radius=2, wmin=WMIN, wmax=WMAX, min_score=-1.0, rel_tol=0.01,
                                  min_consistent=2, ctx=ctx, trunc_voxels=SCENE_TRUNC_VOXELS, min_weight=SCENE_MIN_WEIGHT, volume=SCENE_VOLUME, **options)


@pytest.fixture(scope="module")
def scene(ctx, planted):  # noqa: F811
    """the planted scene of test_tsdf_gpu.py: the restatement's raw mesh, the library's with the defaults and with the options"""
    p = planted
    dims, origin, voxel = SCENE_VOLUME
    vol = tr.new_volume(dims)
    tr.integrate(dims, origin, voxel, SCENE_TRUNC_VOXELS * voxel, [e["depth"] for e in p["exp"]], [e["keep"] for e in p["exp"]], p["images"], p["sc"].K4, p["R"], p["t"], *vol)
    return dict(raw=tr.mesh(dims, origin, voxel, *vol, SCENE_MIN_WEIGHT), plain=_scene(ctx, p), cleaned=_scene(ctx, p, **OPTIONS), voxel=voxel)


def _chain(xyz, bgr, tri, voxel, o):
    """the restatement of the clean-up, in the order dense_mesh_for_all runs it"""
    xyz, bgr, tri, _ = mr.filter_components(xyz, bgr, tri, o["min_component"], o["keep_largest"])
    xyz, bgr, tri, _ = mr.simplify(xyz, bgr, tri, o["simplify_voxels"] * voxel)
    xyz = mr.smooth(xyz, tri, *o["smooth"])
    return xyz, bgr, tri, mr.vertex_normals(xyz, tri)


def test_dense_mesh_for_all_with_the_defaults_is_what_it_was(scene):
    assert len(scene["plain"]) == 3 and _same_mesh(scene["plain"], scene["raw"])


def test_dense_mesh_for_all_with_the_options_equals_the_restatement_chain(ctx, planted, scene):  # noqa: F811
    exp = _chain(*scene["raw"], scene["voxel"], OPTIONS)
    got = scene["cleaned"]
    print(f"{len(scene['raw'][0])} -> {len(got[0])} vertices, {len(scene['raw'][2])} -> {len(got[2])} triangles")
    assert len(got) == 4 and _same_mesh(got, exp)
    length = np.linalg.norm(got[3], axis=1)                                                   # a unit normal, or zeros where the corners cancel
    assert 0 < len(got[2]) < len(scene["raw"][2]) and ((np.abs(length - 1.0) < 1e-12) | (length == 0)).all() and (length > 0).mean() > 0.9
    largest = _scene(ctx, planted, keep_largest=True)
    assert len(largest) == 3 and _same_mesh(largest, mr.filter_components(*scene["raw"], 1, True)[:3])


def test_mesh_ply_round_trip_with_normals(scene, tmp_path):
    xyz, bgr, tri, nrm = scene["cleaned"]
    path = tmp_path / "mesh.ply"
    formats.write_mesh_ply(path, xyz, bgr, tri, nrm)
    x2, b2, t2, n2 = formats.read_mesh_ply(path)
    assert _same(x2, xyz.astype(np.float32)) and _same(b2, bgr) and _same(t2, tri) and _same(n2, nrm.astype(np.float32))
    formats.write_mesh_ply(path, xyz, bgr, tri)
    assert len(formats.read_mesh_ply(path)) == 3 and open(path, "rb").read() == formats.mesh_ply_bytes(xyz, bgr, tri)
    raw = formats.mesh_ply_bytes(xyz, bgr, tri)
    assert raw.startswith(b"ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % len(xyz)) and b"comment" not in raw[:400]      # files without normals keep their bytes
    assert formats.mesh_ply_bytes(xyz, bgr, tri, nrm)[:120].count(b"comment normals") == 1


def test_cpp_mirror_writes_the_same_mesh_file(scene, tmp_path):
    host = os.path.join(HERE, "host")
    subprocess.check_call(["make", "-C", host, "-f", "mesh.mk", "mesh_test"], stdout=subprocess.DEVNULL)
    xyz, bgr, tri = scene["raw"]
    o = OPTIONS
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<6i", len(xyz), len(tri), o["min_component"], int(o["keep_largest"]), o["smooth"][0], 1))
        f.write(struct.pack("<3d", o["simplify_voxels"] * scene["voxel"], o["smooth"][1], o["smooth"][2]))
        f.write(np.ascontiguousarray(xyz).tobytes()); f.write(np.ascontiguousarray(bgr).tobytes()); f.write(np.ascontiguousarray(tri).tobytes())
    out = subprocess.run([os.path.join(host, "mesh_test"), str(tmp_path / "in.bin"), str(tmp_path / "out.ply")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert open(tmp_path / "out.ply", "rb").read() == formats.mesh_ply_bytes(*scene["cleaned"])
