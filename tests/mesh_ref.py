"""numpy restatement of the mesh clean-up exactly as include/sfmhip.h defines it (sfmhip_mesh_components, _filter_components, _simplify,
_vertex_normals, _smooth): integer work for the components and the clustering's bookkeeping, doubles in the written order for the sums
(np.add.at adds in index order, which is the order the header words).  Simplification reuses radius_ref.voxel_downsample.  Plus the
meshes the tests share."""
import numpy as np

import radius_ref as rr
import tsdf_ref as tr


def _mesh(xyz, tri):
    xyz = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
    tri = np.ascontiguousarray(tri, np.int32).reshape(-1, 3)
    valid = ((tri >= 0) & (tri < len(xyz))).all(1) if len(tri) else np.zeros(0, bool)
    return xyz, tri, valid


def valid_mask(nv, tri):
    tri = np.ascontiguousarray(tri, np.int32).reshape(-1, 3)
    return ((tri >= 0) & (tri < nv)).all(1) if len(tri) else np.zeros(0, bool)


# ------------------------------------------------------------------------------------------------ components
def components(nv, tri):
    """(tri_label int32 nt, vertex_label int32 nv, sizes int32 C): min-label propagation with pointer jumping until nothing changes; a
    component's root is its smallest vertex, and the components are numbered in ascending order of their roots"""
    tri = np.ascontiguousarray(tri, np.int32).reshape(-1, 3)
    valid = valid_mask(nv, tri)
    tv = tri[valid].astype(np.int64)
    root = np.arange(nv, dtype=np.int64)
    while len(tv):
        m = root[tv].min(1)
        new = root.copy()
        for k in range(3):
            np.minimum.at(new, tv[:, k], m)
        new = new[new]
        if np.array_equal(new, root):
            break
        root = new
    ref = np.zeros(nv, bool)
    ref[tv.ravel()] = True
    roots = np.flatnonzero(ref & (root == np.arange(nv)))                  # ascending: the numbering
    number = np.full(nv, -1, np.int64)
    number[roots] = np.arange(len(roots))
    vertex_label = np.where(ref, number[root], -1).astype(np.int32)
    tri_label = np.full(len(tri), -1, np.int32)
    tri_label[valid] = vertex_label[tv[:, 0]]
    sizes = np.bincount(tri_label[valid], minlength=len(roots)).astype(np.int32)
    return tri_label, vertex_label, sizes


def filter_components(xyz, bgr, tri, min_triangles=1, keep_largest=False):
    """(xyz_out, bgr_out or None, tri_out, vertex_map)"""
    xyz, tri, valid = _mesh(xyz, tri)
    nv = len(xyz)
    tri_label, _, sizes = components(nv, tri)
    keep_c = sizes >= min_triangles
    if keep_largest:
        best = np.zeros(len(sizes), bool)
        if len(sizes):
            best[int(np.argmax(sizes))] = True                             # argmax: the first among equals
        keep_c &= best
    keep_t = valid & keep_c[np.where(valid, tri_label, 0)] if len(sizes) else np.zeros(len(tri), bool)
    kept_v = np.zeros(nv, bool)
    kept_v[tri[keep_t].ravel()] = True
    vertex_map = np.where(kept_v, np.cumsum(kept_v) - 1, -1).astype(np.int32)
    tri_out = vertex_map[tri[keep_t]].astype(np.int32).reshape(-1, 3)
    return xyz[kept_v], None if bgr is None else np.asarray(bgr, np.uint8).reshape(-1, 3)[kept_v], tri_out, vertex_map


# ------------------------------------------------------------------------------------------------ vertex clustering
def simplify(xyz, bgr, tri, voxel):
    """(xyz_out, bgr_out or None, tri_out, vertex_map); OverflowError where an axis needs more than 2^21 cells"""
    xyz, tri, valid = _mesh(xyz, tri)
    nv = len(xyz)
    tv = tri[valid].astype(np.int64)
    ref = np.zeros(nv, bool)
    ref[tv.ravel()] = True
    masked = xyz.copy()
    masked[~ref] = np.nan
    cen, counts, cluster_of, _ = rr.voxel_downsample(masked, voxel)
    m = cluster_of.astype(np.int64)[tv]
    m = m[(m >= 0).all(1)]
    m = m[(m[:, 0] != m[:, 1]) & (m[:, 1] != m[:, 2]) & (m[:, 0] != m[:, 2])]
    first = m.argmin(1)
    rot = np.stack([m[np.arange(len(m)), (first + k) % 3] for k in range(3)], 1) if len(m) else np.zeros((0, 3), np.int64)
    rot = np.unique(rot, axis=0) if len(rot) else rot                      # distinct rows in ascending lexicographic order
    used = np.zeros(len(cen), bool)
    used[rot.ravel()] = True
    renum = np.where(used, np.cumsum(used) - 1, -1)
    vertex_map = np.where(cluster_of >= 0, renum[np.maximum(cluster_of, 0)], -1).astype(np.int32) if len(cen) else np.full(nv, -1, np.int32)
    bgr_out = None
    if bgr is not None:
        bgr = np.asarray(bgr, np.uint8).reshape(-1, 3)
        sums = np.zeros((len(cen), 3), np.int64)
        inc = cluster_of >= 0
        np.add.at(sums, cluster_of[inc], bgr[inc].astype(np.int64))
        c = counts.astype(np.int64)[:, None]
        bgr_out = ((2 * sums + c) // (2 * c)).astype(np.uint8)[used]
    return cen[used], bgr_out, renum[rot].astype(np.int32).reshape(-1, 3), vertex_map


# ------------------------------------------------------------------------------------------------ normals
def vertex_normals(xyz, tri):
    xyz, tri, valid = _mesh(xyz, tri)
    tv = tri[valid].astype(np.int64)
    S = np.zeros((len(xyz), 3))
    with np.errstate(all="ignore"):
        p0, p1, p2 = xyz[tv[:, 0]], xyz[tv[:, 1]], xyz[tv[:, 2]]
        e1, e2 = p1 - p0, p2 - p0
        N = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
        np.add.at(S, tv.ravel(), np.repeat(N, 3, axis=0))                  # ascending (t, corner)
        l = np.sqrt((S[:, 0] * S[:, 0] + S[:, 1] * S[:, 1]) + S[:, 2] * S[:, 2])
        ok = (l > 0) & np.isfinite(l)
        out = np.zeros_like(S)
        out[ok] = S[ok] / l[ok, None]
    return out


# ------------------------------------------------------------------------------------------------ smoothing
def adjacency(nv, tri):
    """(v, w) of the distinct directed pairs, v != w, in ascending (v, w)"""
    tri = np.ascontiguousarray(tri, np.int32).reshape(-1, 3)
    tv = tri[valid_mask(nv, tri)].astype(np.int64)
    v = np.concatenate([tv[:, 0], tv[:, 0], tv[:, 1], tv[:, 1], tv[:, 2], tv[:, 2]])
    w = np.concatenate([tv[:, 1], tv[:, 2], tv[:, 0], tv[:, 2], tv[:, 0], tv[:, 1]])
    key = np.unique((v * max(nv, 1) + w)[v != w])
    return key // max(nv, 1), key % max(nv, 1)


def smooth(xyz, tri, iterations, lam, mu):
    xyz = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
    v, w = adjacency(len(xyz), tri)
    deg = np.bincount(v, minlength=len(xyz))
    has = deg > 0
    x = xyz.copy()
    factors = [lam] * iterations if mu == 0 else [lam, mu] * iterations
    with np.errstate(all="ignore"):
        for f in factors:
            m = np.zeros_like(x)
            np.add.at(m, v, x[w])                                          # ascending w within a vertex
            m[has] = m[has] / deg[has, None].astype(np.float64)
            out = x.copy()
            out[has] = x[has] + f * (m[has] - x[has])
            x = out
    return x


# ------------------------------------------------------------------------------------------------ what the tests share
_SPHERES = {}


def sphere_mesh(n):
    """(xyz, tri, voxel) of tsdf_ref.analytic_sphere(n), computed once"""
    if n not in _SPHERES:
        dims, origin, voxel, dsum, wsum = tr.analytic_sphere(n)
        xyz, _, tri = tr.mesh(dims, origin, voxel, dsum, wsum, None, 1)
        _SPHERES[n] = (xyz, tri, voxel)
    return _SPHERES[n]


def colours(nv, seed=5):
    return np.random.default_rng(seed).integers(0, 256, (nv, 3), dtype=np.uint8)


def two_spheres_and_fragments(seed=3):
    """(xyz, bgr, tri): the 16^3 sphere twice (the copy moved by 4 and listed first in neither array: its vertices and triangles are
    interleaved with the first's), six detached fragments of one or two triangles, a few unreferenced vertices and two invalid triangles"""
    xyz, tri, _ = sphere_mesh(16)
    nv = len(xyz)
    rng = np.random.default_rng(seed)
    frag_xyz = rng.uniform(8.0, 9.0, (20, 3))
    frag_tri = np.array([[0, 1, 2], [3, 4, 5], [5, 4, 6], [7, 8, 9], [10, 11, 12], [12, 11, 13], [14, 15, 16], [17, 18, 19]], np.int32) + 2 * nv
    all_xyz = np.concatenate([xyz, xyz + np.array([4.0, 0.0, 0.0]), frag_xyz, rng.uniform(-1, 1, (5, 3))])
    all_tri = np.concatenate([tri, tri + nv, frag_tri, np.array([[0, 1, len(all_xyz)], [-1, 2, 3]], np.int32)])
    order = rng.permutation(len(all_tri))
    return all_xyz, colours(len(all_xyz)), np.ascontiguousarray(all_tri[order])


def strip(n, shuffled=False, seed=1):
    """a strip of n triangles on n + 2 vertices in index order (a chain: the union-find's deep case), optionally with its triangles shuffled"""
    i = np.arange(n, dtype=np.int32)
    tri = np.where((i % 2 == 0)[:, None], np.stack([i, i + 1, i + 2], 1), np.stack([i + 1, i, i + 2], 1)).astype(np.int32)
    xyz = np.stack([(np.arange(n + 2) // 2) * 0.5, (np.arange(n + 2) % 2) * 0.5, np.sin(np.arange(n + 2) * 0.1)], 1)
    if shuffled:
        tri = tri[np.random.default_rng(seed).permutation(n)]
    return xyz, np.ascontiguousarray(tri)


def random_mesh(nv=200_000, nt=300_007, seed=7):
    """random triangles over random vertices: indices above 2^16, a triangle count off every tile size, many components"""
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.0, 1.0, (nv, 3)), rng.integers(0, nv, (nt, 3)).astype(np.int32)


def hand_made():
    """name -> (xyz, bgr or None, tri): the small cases of the definition"""
    P = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.5], [2, 0, 1], [2, 1, 0], [3, 3, 3], [0.5, 0.5, 2]])
    Z3 = np.zeros((0, 3))
    nanP = P.copy(); nanP[3, 1] = np.nan
    c = colours(8)
    return {
        "nv0": (Z3, None, np.array([[0, 1, 2]], np.int32)),
        "nt0": (P, c, np.zeros((0, 3), np.int32)),
        "both0": (Z3, None, np.zeros((0, 3), np.int32)),
        "one": (P[:3], c[:3], np.array([[0, 1, 2]], np.int32)),
        "bowtie": (P, c, np.array([[0, 1, 2], [2, 3, 5]], np.int32)),
        "vvv": (P, c, np.array([[0, 1, 2], [6, 6, 6], [1, 1, 2]], np.int32)),
        "out_of_range": (P, c, np.array([[0, 1, 2], [-1, 1, 2], [3, 4, 8], [3, 4, 5], [2 ** 31 - 1, 0, 1]], np.int32)),
        "nan": (nanP, c, np.array([[0, 1, 2], [1, 3, 2], [3, 4, 5], [1, 4, 3]], np.int32)),
        "duplicates": (P, c, np.array([[0, 1, 2], [1, 2, 0], [0, 2, 1], [2, 1, 0], [0, 1, 2], [3, 4, 5]], np.int32)),
        "tie": (P, c, np.array([[3, 4, 5], [5, 4, 7], [0, 1, 2], [2, 1, 6]], np.int32)),
    }
