"""numpy restatement of the dense mesh exactly as include/sfmhip.h defines it (sfmhip_tsdf_integrate, sfmhip_tsdf_mesh): doubles in the
written order, integer sums, the tetrahedron rules from the permutation's parity as the header words them.  Vectorised over the volume; the
84 mixed tetrahedron cases are a loop.  Plus what the tests share: pinhole views of an analytic sphere and the bookkeeping of a
triangle mesh (directed edges, Euler characteristic, signed volume)."""
import itertools

import numpy as np

Q = 32767.0
TETS = [(0, 1, 3, 7), (0, 1, 5, 7), (0, 2, 3, 7), (0, 2, 6, 7), (0, 4, 5, 7), (0, 4, 6, 7)]


def corner(c):
    """(dx, dy, dz) of the corner code c = dx + 2 dy + 4 dz"""
    return c & 1, (c >> 1) & 1, (c >> 2) & 1


def sigma(tet):
    """the sign of det[c1 - c0, c2 - c0, c3 - c0]"""
    p = np.array([corner(c) for c in tet], np.float64)
    return int(np.sign(np.linalg.det(p[1:] - p[0])))


SIGMA = [sigma(t) for t in TETS]


def permutation_sign(p):
    s = 1
    for a in range(len(p)):
        for b in range(a + 1, len(p)):
            if p[a] > p[b]:
                s = -s
    return s


def tet_triangles(ins, sg):
    """the triangles of one tetrahedron as triples of position pairs (x, y) = E(x, y): ins = the inside flags of the positions 0 .. 3,
    sg = the tetrahedron's parity"""
    n = sum(ins)
    if n in (0, 4):
        return []
    if n in (1, 3):
        k = ins.index(n == 1)
        l, m, nn = [x for x in range(4) if x != k]
        a, b = ((k, l), (k, m), (k, nn)), ((k, l), (k, nn), (k, m))
        pos = permutation_sign((k, l, m, nn)) * sg > 0
        if n == 3:
            pos = not pos
        return [a if pos else b]
    k, l = [x for x in range(4) if ins[x]]
    m, nn = [x for x in range(4) if not ins[x]]
    q = ((k, m), (k, nn), (l, nn), (l, m))
    if permutation_sign((k, l, m, nn)) * sg > 0:
        return [(q[0], q[1], q[2]), (q[0], q[2], q[3])]
    return [(q[0], q[2], q[1]), (q[0], q[3], q[2])]


def centres(dims, origin, voxel):
    """X_a of every voxel, three arrays of shape (nz, ny, nx)"""
    nx, ny, nz = dims
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return tuple(float(origin[a]) + (idx.astype(np.float64) + 0.5) * float(voxel) for a, idx in enumerate((i, j, k)))


def new_volume(dims, colour=True):
    n = int(dims[0]) * int(dims[1]) * int(dims[2])
    return np.zeros(n, np.int32), np.zeros(n, np.int32), (np.zeros((n, 3), np.uint32) if colour else None)


def integrate(dims, origin, voxel, trunc, depths, keeps, imgs, K4, R, t, dsum, wsum, csum):
    """adds the views to (dsum, wsum, csum) in place; keeps: None or a list whose entries may be None; imgs: None exactly when csum is"""
    nx, ny, nz = dims
    fx, fy, cx, cy = (float(x) for x in K4)
    X0, X1, X2 = centres(dims, origin, voxel)
    R = np.asarray(R, np.float64).reshape(-1, 9); t = np.asarray(t, np.float64).reshape(-1, 3)
    trunc = float(trunc)
    for s, depth in enumerate(depths):
        rows, cols = depth.shape
        r, tt = R[s], t[s]
        with np.errstate(all="ignore"):
            Y = [((r[3 * i] * X0 + r[3 * i + 1] * X1) + r[3 * i + 2] * X2) + tt[i] for i in range(3)]
            ok = Y[2] > 0
            pu = np.floor(((fx * Y[0]) / Y[2] + cx) + 0.5); pv = np.floor(((fy * Y[1]) / Y[2] + cy) + 0.5)
            ok &= (pu >= 0) & (pu < cols) & (pv >= 0) & (pv < rows)
            iu = np.where(ok, pu, 0).astype(np.int64); iv = np.where(ok, pv, 0).astype(np.int64)
            d = depth[iv, iu]
            ok &= np.isfinite(d)
            if keeps is not None and keeps[s] is not None:
                ok &= keeps[s][iv, iu] != 0
            sd = d.astype(np.float64) - Y[2]
            ok &= sd >= -trunc
            q = np.floor((np.where(sd > trunc, trunc, sd) / trunc) * Q + 0.5)
        dsum += np.where(ok, q, 0.0).astype(np.int32).ravel()
        wsum += ok.astype(np.int32).ravel()
        if csum is not None:
            img = np.asarray(imgs[s])
            px = img[iv, iu]
            if img.ndim == 2:
                px = px[..., None].repeat(3, -1)
            csum += np.where(ok[..., None], px, 0).astype(np.uint32).reshape(-1, 3)


def _shift(a, dz, dy, dx, fill):
    """out[k, j, i] = a[k + dz, j + dy, i + dx] where that lies in the array, else fill (shifts of -1, 0, 1)"""
    out = np.full_like(a, fill)
    nz, ny, nx = a.shape

    def sl(n, d):
        return (slice(max(0, -d), n - max(0, d)), slice(max(0, d), n - max(0, -d)))
    (zk, zs), (yk, ys), (xk, xs) = sl(nz, dz), sl(ny, dy), sl(nx, dx)
    out[zk, yk, xk] = a[zs, ys, xs]
    return out


def mesh(dims, origin, voxel, dsum, wsum, csum, min_weight):
    """(xyz nv x 3 float64, bgr nv x 3 uint8 or None, tri nt x 3 int32)"""
    nx, ny, nz = (int(x) for x in dims)
    nvox = nx * ny * nz
    D = np.asarray(dsum, np.int64).reshape(nz, ny, nx); W = np.asarray(wsum, np.int64).reshape(nz, ny, nx)
    valid = W >= min_weight
    inside = D < 0
    # the cell above every voxel: processed when its 8 corners exist and are valid
    proc = np.ones((nz, ny, nx), bool)
    corner_in = []
    for c in range(8):
        dx, dy, dz = corner(c)
        proc &= _shift(valid, dz, dy, dx, False)
        corner_in.append(_shift(inside, dz, dy, dx, False))
    # the edges a voxel owns
    has = np.zeros((nvox, 7), bool)
    for d in range(1, 8):
        dx, dy, dz = corner(d)
        exists = _shift(np.ones((nz, ny, nx), bool), dz, dy, dx, False)
        crossing = exists & (inside != corner_in[d])
        belongs = np.zeros((nz, ny, nx), bool)
        for e in range(8):
            if e & d:
                continue
            ex, ey, ez = corner(e)
            belongs |= _shift(proc, -ez, -ey, -ex, False)
        has[:, d - 1] = (crossing & belongs).ravel()
    vid = (np.cumsum(has.ravel()) - 1).reshape(nvox, 7)
    va, dd = np.nonzero(has)
    off = np.array([corner(c)[0] + corner(c)[1] * nx + corner(c)[2] * nx * ny for c in range(8)], np.int64)
    vb = va + off[dd + 1]
    Df, Wf = D.ravel(), W.ravel()
    num = Df[va] * Wf[vb]; den = num - Df[vb] * Wf[va]
    s = num.astype(np.float64) / den.astype(np.float64)
    X = [x.ravel() for x in centres(dims, origin, voxel)]
    xyz = np.stack([X[c][va] + s * (X[c][vb] - X[c][va]) for c in range(3)], 1).reshape(-1, 3)
    bgr = None
    if csum is not None:
        Cs = np.asarray(csum, np.int64).reshape(nvox, 3)
        ma = (2 * Cs[va] + Wf[va, None]) // (2 * Wf[va, None]); mb = (2 * Cs[vb] + Wf[vb, None]) // (2 * Wf[vb, None])
        bgr = np.floor((ma.astype(np.float64) + s[:, None] * (mb.astype(np.float64) - ma.astype(np.float64))) + 0.5).astype(np.uint8).reshape(-1, 3)
    # triangles
    cells = np.nonzero(proc.ravel())[0]
    cin = np.stack([ci.ravel()[cells] for ci in corner_in], 1)                    # n_cells x 8
    keys, rows = [], []
    for t, (tet, sg) in enumerate(zip(TETS, SIGMA)):
        for ins in itertools.product((False, True), repeat=4):
            tris = tet_triangles(list(ins), sg)
            if not tris:
                continue
            sel = np.ones(len(cells), bool)
            for p in range(4):
                sel &= cin[:, tet[p]] == ins[p]
            base = cells[sel]
            if not len(base):
                continue
            for jj, tr in enumerate(tris):
                ids = []
                for x, y in tr:
                    lo, hi = tet[min(x, y)], tet[max(x, y)]
                    ids.append(vid[base + off[lo], (hi - lo) - 1])
                rows.append(np.stack(ids, 1)); keys.append((base * 6 + t) * 2 + jj)
    if rows:
        order = np.argsort(np.concatenate(keys), kind="stable")
        tri = np.concatenate(rows)[order].astype(np.int32)
    else:
        tri = np.zeros((0, 3), np.int32)
    return xyz, bgr, tri


# ------------------------------------------------------------------------------------------------ what the tests share
def look_at(c):
    """(R, t) world to camera of a camera at c that looks at the origin"""
    c = np.asarray(c, np.float64)
    z = -c / np.linalg.norm(c)
    up = np.array([0.0, 0.0, 1.0]) if abs(z[2]) < 0.9 else np.array([0.0, 1.0, 0.0])
    x = np.cross(up, z); x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    return R, -R @ c


def sphere_depth(R, t, K4, rows, cols, rad=1.0):
    """float32 depth along z of the unit sphere at the world origin, NaN off it"""
    fx, fy, cx, cy = K4
    v, u = np.mgrid[0:rows, 0:cols]
    d = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones((rows, cols))], -1)
    a = (d * d).sum(-1); b = -2 * (d @ t); c = t @ t - rad * rad
    disc = b * b - 4 * a * c
    z = np.full((rows, cols), np.nan, np.float32)
    ok = disc > 0
    z[ok] = ((-b[ok] - np.sqrt(disc[ok])) / (2 * a[ok])).astype(np.float32)
    return z


SPHERE_K4 = (120.0, 120.0, 47.5, 47.5)
SPHERE_CAMS = [(4, 0, 0), (-4, 0, 0), (0, 4, 0), (0, -4, 0), (0, 0, 4), (0, 0, -4)] + [(2.3 * a, 2.3 * b, 2.3 * c) for a in (-1, 1) for b in (-1, 1) for c in (-1, 1)]


def sphere_views(n_cams=14, rows=96, cols=96):
    """(depths, R n x 9, t n x 3): 6 views on the axes at distance 4, then 8 on the cube diagonals at distance 2.3 sqrt(3)"""
    poses = [look_at(c) for c in SPHERE_CAMS[:n_cams]]
    return [sphere_depth(R, t, SPHERE_K4, rows, cols) for R, t in poses], np.array([R.ravel() for R, _ in poses]), np.array([t for _, t in poses])


def sphere_box(n):
    """dims, origin, voxel of n^3 voxels over [-1.5, 1.5]^3"""
    return (n, n, n), (-1.5, -1.5, -1.5), 3.0 / n


def analytic_sphere(n, trunc_voxels=3.0):
    """dsum quantised from |X| - 1 (clamped at the truncation distance), wsum = 1"""
    dims, origin, voxel = sphere_box(n)
    X0, X1, X2 = centres(dims, origin, voxel)
    trunc = trunc_voxels * voxel
    sd = np.sqrt(X0 * X0 + X1 * X1 + X2 * X2) - 1.0
    dsum = np.floor(np.clip(sd, -trunc, trunc) / trunc * Q + 0.5).astype(np.int32).ravel()
    return dims, origin, voxel, dsum, np.ones_like(dsum)


def mesh_stats(xyz, tri):
    """dict: duplicated directed edges, boundary edges (directed edges without their reverse), Euler characteristic V - E + F over the
    undirected edges, signed volume"""
    e = np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]]).astype(np.int64)
    n = int(max(len(xyz), 1))
    key = e[:, 0] * n + e[:, 1]; rev = e[:, 1] * n + e[:, 0]
    uniq, cnt = np.unique(key, return_counts=True)
    und = np.unique(np.minimum(e[:, 0], e[:, 1]) * n + np.maximum(e[:, 0], e[:, 1]))
    p = xyz[tri]
    vol = float(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0) if len(tri) else 0.0
    return dict(duplicated=int((cnt > 1).sum()), boundary=int((~np.isin(rev, uniq)).sum()), euler=len(xyz) - len(und) + len(tri), volume=vol)
