"""Independent references and shared cases for the per-element geometry kernels (triangulate.hip, plane_fit / eig3_min of normals.hip).

Nothing here shares code with the kernels or with oracle/: the null vectors come from mpmath's SVD at MP_DPS digits on systems built
exactly from the inputs, the N-view system is the UNSQUARED 2m x 4 stack (the kernel and the oracle square it), reprojection errors and
plane-fit moments are numpy.longdouble (64-bit mantissa), eigenvalues numpy.linalg.eigh.  The generators of the cases live here too so
that tests/test_geometry_ref_cpu.py (oracle vs reference, runs without a GPU) and the two GPU files look at the same inputs.

mpmath work is limited to sample_rows(): at most 100 rows of a case, a fixed stride plus the first and last row of every 256-row block
(the kernels' workgroup); every other row is still covered by the bit comparison with the oracle."""
import functools

import mpmath as mp
import numpy as np

import points_ref as pr
from sfm_opencv_amd import synth

MP_DPS = 50
EPS64 = 2.0 ** -52
LD = np.longdouble

# c of the two-view bound  ulp32(v_ref_i)/2 + c * EPS64 * sigma1 / (sigma3 - sigma4): 8 x the largest value the oracle needs over all
# two-view cases below (test_geometry_ref_cpu.py asserts that it needs no more than the measured value).  Measured: 0 -- on every
# sampled row the oracle's float32 vector is the correctly rounded reference vector -- so the bound is the float32 cast alone.
C_TWO_VIEW_MEASURED = 0.0
C_TWO_VIEW = 8.0 * C_TWO_VIEW_MEASURED


def sample_rows(n, limit=100):
    """fixed stride plus the first and last row of every 256-row block, at most `limit` rows"""
    edge = {r for b in range(0, n, 256) for r in (b, min(b + 255, n - 1))}
    room = max(limit - len(edge), 1)
    stride = max(1, -(-n // room))
    return np.array(sorted(edge | set(range(0, n, stride))), np.int64)


def same_bits(a, b):
    """equal bit for bit; non-finite entries compare by kind (NaN with NaN, +-inf with the same sign), not by payload"""
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(u)[~na], b.view(u)[~nb]))


def _mpf(x):
    return mp.mpf(float(x))


# ---------------------------------------------------------------------------------------------------------------- two views
K_FULL = np.array([[synth.K_REF[0], 0, synth.K_REF[2]], [0, synth.K_REF[1], synth.K_REF[3]], [0, 0, 1.0]])
TWO_VIEW_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 513)
# name: (baseline, depth, pixel noise).  Only the first carries pixel noise: at a baseline / depth of 1e-4 a disparity is 0.3 px, and
# noise of that size would close the gap sigma3 - sigma4 that the bound divides by; the others keep the float32 rounding of the pixels.
TWO_VIEW_GEOMETRIES = {
    "b1_d10_noise": (1.0, 10.0, 0.3),
    "b0.1_d10": (0.1, 10.0, 0.0),
    "b0.01_d10": (0.01, 10.0, 0.0),
    "b0.001_d10": (0.001, 10.0, 0.0),
    "b1_d1000": (1.0, 1000.0, 0.0),
    "b1_d1e4": (1.0, 1e4, 0.0),
    "b1_d10_clean": (1.0, 10.0, 0.0),
}


def projection_f32(K, R, T):
    """float32 K times float32 [R | T], each dot product in double and rounded once"""
    fK = np.asarray(K, np.float64).astype(np.float32).astype(np.float64)
    RT = np.concatenate([np.asarray(R, np.float64), np.asarray(T, np.float64).reshape(3, 1)], axis=1).astype(np.float32).astype(np.float64)
    return (fK @ RT).astype(np.float32)


def two_view_case(geom, n, seed=1):
    """float32 P1, P2 (3 x 4) and pixels (n x 2) of `geom`: camera 1 at the origin, camera 2 one baseline to its side and turned
    towards the scene, points in a box of +-0.3 x +-0.2 x (0.6 .. 1.4) depths"""
    b, d, noise = TWO_VIEW_GEOMETRIES[geom]
    rng = np.random.default_rng([seed, n, sorted(TWO_VIEW_GEOMETRIES).index(geom)])
    R2 = synth.angle_axis_to_rotmat(np.array([0.02, -0.15, 0.01]) * min(1.0, 10.0 * b / d)); T2 = b * np.array([-1.0, 0.05, 0.1])
    X = d * np.stack([rng.uniform(-0.3, 0.3, n), rng.uniform(-0.2, 0.2, n), rng.uniform(0.6, 1.4, n)], axis=1)

    def pix(R, T):
        p = X @ R.T + T
        uv = np.stack([synth.K_REF[0] * p[:, 0] / p[:, 2] + synth.K_REF[2], synth.K_REF[1] * p[:, 1] / p[:, 2] + synth.K_REF[3]], 1)
        return (uv + noise * rng.standard_normal((n, 2))).astype(np.float32)
    return dict(P1=projection_f32(K_FULL, np.eye(3), np.zeros(3)), P2=projection_f32(K_FULL, R2, T2), xy1=pix(np.eye(3), np.zeros(3)),
                xy2=pix(R2, T2), X=X)


def two_view_degenerate(n=257):
    """systems without a defined null vector: the only claim is that the kernel and the oracle do the same arithmetic on them"""
    s = two_view_case("b1_d10_noise", n, seed=9)
    out = {}
    out["identical_cameras"] = dict(s, P2=s["P1"].copy())
    out["identical_cameras_and_pixels"] = dict(s, P2=s["P1"].copy(), xy2=s["xy1"].copy())
    out["zero_P2"] = dict(s, P2=np.zeros((3, 4), np.float32))
    big = dict(s, xy1=s["xy1"].copy(), xy2=s["xy2"].copy())
    big["xy1"][0, 0] = 1e6; big["xy2"][n - 1, 1] = -1e6; big["xy1"][n // 2] = [1e6, 1e6]
    out["pixel_1e6"] = big
    bad = dict(s, xy1=s["xy1"].copy(), xy2=s["xy2"].copy())
    bad["xy1"][0, 0] = np.nan; bad["xy2"][n - 1, 1] = np.nan; bad["xy1"][n // 2, 1] = np.inf; bad["xy2"][n - 2] = [-np.inf, np.nan]
    out["nan_pixel"] = bad
    return out


def null_vector_two_view(P1, P2, xy1, xy2, rows):
    """(v len(rows) x 4, sigma len(rows) x 4): unit right singular vector of the smallest singular value and sigma1 >= .. >= sigma4 of
    the 4 x 4 DLT system, built exactly from the float32 inputs (a product of two 24-bit numbers is exact at MP_DPS digits)"""
    P = [np.asarray(P1, np.float32).reshape(3, 4), np.asarray(P2, np.float32).reshape(3, 4)]
    xy = [np.asarray(xy1, np.float32).reshape(-1, 2), np.asarray(xy2, np.float32).reshape(-1, 2)]
    v = np.empty((len(rows), 4)); sig = np.empty((len(rows), 4))
    with mp.workdps(MP_DPS):
        Pm = [[[_mpf(p[r, k]) for k in range(4)] for r in range(3)] for p in P]
        for o, i in enumerate(rows):
            A = mp.matrix(4, 4)
            for j in range(2):
                x, y = _mpf(xy[j][i, 0]), _mpf(xy[j][i, 1])
                for k in range(4):
                    A[2 * j, k] = x * Pm[j][2][k] - Pm[j][0][k]
                    A[2 * j + 1, k] = y * Pm[j][2][k] - Pm[j][1][k]
            _, S, V = mp.svd_r(A)                           # A = U diag(S) V, S descending: the null vector is the last ROW of V
            nrm = mp.sqrt(sum(V[3, k] ** 2 for k in range(4)))
            v[o] = [float(V[3, k] / nrm) for k in range(4)]
            sig[o] = [float(S[k]) for k in range(4)]
    return v, sig


def two_view_bound(v_ref, sig, c=C_TWO_VIEW):
    """per-component bound on |float32 null vector - v_ref| after sign alignment: the float32 cast plus the singular-vector
    perturbation of a backward-stable fp64 SVD"""
    ulp32 = np.spacing(np.abs(v_ref).astype(np.float32)).astype(np.float64)
    return 0.5 * ulp32 + c * EPS64 * (sig[:, 0] / (sig[:, 2] - sig[:, 3]))[:, None]


def two_view_needed_c(h, v_ref, sig):
    """the smallest c with which two_view_bound admits the float32 null vectors h (len x 4), per row"""
    h = np.asarray(h, np.float64)
    sgn = np.sign((h * v_ref).sum(1, keepdims=True))
    excess = np.abs(h * sgn - v_ref) - 0.5 * np.spacing(np.abs(v_ref).astype(np.float32)).astype(np.float64)
    return np.maximum(excess, 0.0).max(1) / (EPS64 * sig[:, 0] / (sig[:, 2] - sig[:, 3]))


@functools.lru_cache(maxsize=None)
def two_view_reference(geom, n):
    """(case, rows, v_ref, sigma) of a two-view case, computed once per process"""
    s = two_view_case(geom, n)
    rows = sample_rows(n)
    v, sig = null_vector_two_view(s["P1"], s["P2"], s["xy1"], s["xy2"], rows)
    return s, rows, v, sig


def two_view_cases():
    """every geometry at the size with three workgroups, every size on the noisy geometry"""
    return [(g, 513) for g in TWO_VIEW_GEOMETRIES] + [("b1_d10_noise", n) for n in TWO_VIEW_SIZES if n != 513]


def dehomogenise_f32(xyzw):
    """store_point restated in numpy: float32(h_i * float32(1 / float64(h_3))) widened to float64, from a 4 x n float32 array"""
    h = np.asarray(xyzw, np.float32)
    with np.errstate(all="ignore"):
        inv = (1.0 / h[3].astype(np.float64)).astype(np.float32)
        return np.stack([h[0] * inv, h[1] * inv, h[2] * inv], axis=1).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------- tracks
def _rodrigues_mp(w):
    """rotation matrix of an angle-axis vector, the full formula at every angle (no first-order branch)"""
    w = [_mpf(x) for x in w]
    th = mp.sqrt(w[0] ** 2 + w[1] ** 2 + w[2] ** 2)
    R = mp.eye(3)
    if th == 0:
        return R
    a = [x / th for x in w]
    Kx = mp.matrix([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return R + mp.sin(th) * Kx + (1 - mp.cos(th)) * (Kx * Kx)


def dlt_tracks(K4, ext6, obs_cam, obs_pt, obs_uv, points):
    """(v len x 4, x len x 3, sigma len x 4) for the listed points: the SVD null vector of the unsquared 2m x 4 system on normalised
    image coordinates, x = v[:3] / v[3].  A point with fewer than two observations gets NaN."""
    ext6 = np.asarray(ext6, np.float64).reshape(-1, 6); obs_uv = np.asarray(obs_uv, np.float64).reshape(-1, 2)
    v = np.full((len(points), 4), np.nan); x = np.full((len(points), 3), np.nan); sig = np.full((len(points), 4), np.nan)
    with mp.workdps(MP_DPS):
        fx, fy, cx, cy = (_mpf(k) for k in K4)
        Rt = {}
        for o, p in enumerate(points):
            ks = np.flatnonzero(np.asarray(obs_pt) == p)
            if len(ks) < 2:
                continue
            A = mp.matrix(2 * len(ks), 4)
            for r, k in enumerate(ks):
                c = int(obs_cam[k])
                if c not in Rt:
                    R = _rodrigues_mp(ext6[c, :3])
                    Rt[c] = [[R[i, 0], R[i, 1], R[i, 2], _mpf(ext6[c, 3 + i])] for i in range(3)]
                xn = (_mpf(obs_uv[k, 0]) - cx) / fx; yn = (_mpf(obs_uv[k, 1]) - cy) / fy
                for j in range(4):
                    A[2 * r, j] = xn * Rt[c][2][j] - Rt[c][0][j]
                    A[2 * r + 1, j] = yn * Rt[c][2][j] - Rt[c][1][j]
            _, S, V = mp.svd_r(A)
            nrm = mp.sqrt(sum(V[3, k] ** 2 for k in range(4)))
            v[o] = [float(V[3, k] / nrm) for k in range(4)]
            sig[o] = [float(S[k]) for k in range(4)]
            if V[3, 3] != 0:
                x[o] = [float(V[3, k] / V[3, 3]) for k in range(3)]
    return v, x, sig


def _rodrigues_ld(w):
    w = np.asarray(w, LD)
    th = np.sqrt((w * w).sum())
    if th == 0:
        return np.eye(3, dtype=LD)
    a = w / th
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], LD)
    return np.eye(3, dtype=LD) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def reprojection_errors(K4, ext6, pts, obs_cam, obs_pt, obs_uv):
    """|K (R X + t) / z - uv| per observation in numpy.longdouble (returned as longdouble); inf / NaN where IEEE division gives them"""
    ext6 = np.asarray(ext6, np.float64).reshape(-1, 6)
    R = np.stack([_rodrigues_ld(e[:3]) for e in ext6]); t = ext6[:, 3:].astype(LD)
    X = np.asarray(pts, np.float64).reshape(-1, 3).astype(LD)[np.asarray(obs_pt)]
    c = np.asarray(obs_cam)
    p = np.einsum("kab,kb->ka", R[c], X) + t[c]
    uv = np.asarray(obs_uv, np.float64).reshape(-1, 2).astype(LD)
    K4 = np.asarray(K4, np.float64).astype(LD)
    with np.errstate(all="ignore"):
        du = K4[0] * p[:, 0] / p[:, 2] + K4[2] - uv[:, 0]; dv = K4[1] * p[:, 1] / p[:, 2] + K4[3] - uv[:, 1]
        return np.sqrt(du * du + dv * dv)


def _centre_to_ext(w, C):
    w = np.asarray(w, np.float64)
    return np.concatenate([w, -synth.angle_axis_to_rotmat(w) @ np.asarray(C, np.float64)])


TRACK_SIZES = (1, 2, 255, 256, 257)
TRACK_LENGTHS = (40, 0, 1, 2, 3)            # of point p: TRACK_LENGTHS[p % 5], "40" = every camera


def mixed_tracks_scene(n_pt, seed=2):
    """40 cameras, three of them at the edges of the rotation formula (camera 0: |w|^2 <= DBL_EPSILON, camera 1: w = 0 and t = 0,
    camera 2: |w| = pi - 1e-9, on the far side of the scene and looking back), the others along a baseline of 1 at depth 10; track
    lengths 40, 0, 1, 2, 3 interleaved; point 253 sees camera 5 twice (and camera 9), point 254 is the same pixel of camera 7 three times
    (rank 2: `equality_only`); observations shuffled.  0.1 px noise."""
    rng = np.random.default_rng([seed, n_pt])
    n_cam = 40
    ext = np.zeros((n_cam, 6))
    ext[0] = _centre_to_ext([1e-9, -5e-9, 2e-9], [-0.5, 0.02, 0.0])
    ax = np.array([0.02, 1.0, 0.01]); ax /= np.linalg.norm(ax)
    ext[2] = _centre_to_ext(ax * (np.pi - 1e-9), [0.3, 0.1, 20.0])
    for c in range(3, n_cam):
        ext[c] = _centre_to_ext(0.03 * rng.standard_normal(3), [-0.5 + (c - 3) / 36.0, 0.05 * np.sin(c), 0.05 * np.cos(c)])
    assert ext[0, :3] @ ext[0, :3] <= np.finfo(np.float64).eps and not ext[1].any()
    X = np.stack([rng.uniform(-3, 3, n_pt), rng.uniform(-2, 2, n_pt), rng.uniform(6, 14, n_pt)], axis=1)
    cams = []
    for p in range(n_pt):
        L = TRACK_LENGTHS[p % 5]
        cams.append(np.arange(n_cam) if L == n_cam else np.sort(rng.permutation(n_cam)[:L]))
    if n_pt > 254:
        cams[253] = np.array([5, 5, 9]); cams[254] = np.array([7, 7, 7])
    obs_pt = np.concatenate([np.full(len(c), p) for p, c in enumerate(cams)]).astype(np.int32)
    obs_cam = np.concatenate(cams).astype(np.int32)
    uv = synth.project(synth.K_REF, ext[obs_cam], X[obs_pt]) + 0.1 * rng.standard_normal((len(obs_pt), 2))
    equality_only = []
    if n_pt > 254:
        k = np.flatnonzero(obs_pt == 254); uv[k] = uv[k[0]]; equality_only = [254]
    perm = rng.permutation(len(obs_pt))
    return dict(K4=synth.K_REF.copy(), ext=ext, obs_cam=obs_cam[perm], obs_pt=obs_pt[perm], obs_uv=np.ascontiguousarray(uv[perm]),
                n_pt=n_pt, X=X, n_views=np.array([len(c) for c in cams], np.int32), equality_only=equality_only)


# name: (baseline, depth, cameras); every point is seen by every camera, 0.1 px noise, 64 points
TRACK_GEOMETRIES = {"b1_d10_c40": (1.0, 10.0, 40), "b0.01_d10_c2": (0.01, 10.0, 2), "b0.01_d10_c40": (0.01, 10.0, 40), "b1_d1000_c3": (1.0, 1000.0, 3)}


def geometry_tracks_scene(name, n_pt=64, seed=3):
    b, d, n_cam = TRACK_GEOMETRIES[name]
    rng = np.random.default_rng([seed, sorted(TRACK_GEOMETRIES).index(name)])
    ext = np.stack([_centre_to_ext(0.02 * rng.standard_normal(3), [b * (c / (n_cam - 1) - 0.5), 0.05 * b * np.sin(c), 0.05 * b * np.cos(c)])
                    for c in range(n_cam)])
    X = d * np.stack([rng.uniform(-0.3, 0.3, n_pt), rng.uniform(-0.2, 0.2, n_pt), rng.uniform(0.6, 1.4, n_pt)], axis=1)
    obs_pt = np.repeat(np.arange(n_pt), n_cam).astype(np.int32); obs_cam = np.tile(np.arange(n_cam), n_pt).astype(np.int32)
    uv = synth.project(synth.K_REF, ext[obs_cam], X[obs_pt]) + 0.1 * rng.standard_normal((len(obs_pt), 2))
    perm = rng.permutation(len(obs_pt))
    return dict(K4=synth.K_REF.copy(), ext=ext, obs_cam=obs_cam[perm], obs_pt=obs_pt[perm], obs_uv=np.ascontiguousarray(uv[perm]),
                n_pt=n_pt, X=X, n_views=np.full(n_pt, n_cam, np.int32), equality_only=[])


# The oracle's relative deviation from dlt_tracks / reprojection_errors below, as measured (test_geometry_ref_cpu.py holds the oracle to 4 x
# these, so that the GPU tests' bound -- 8 x the oracle's deviation, computed there -- cannot grow with a mistake the two share).
ORACLE_TRACK_DEVIATION = {"mixed_1": 1.9e-16, "mixed_2": 4.8e-16, "mixed_255": 1.6e-14, "mixed_256": 3.4e-14, "mixed_257": 3.2e-14,
                          "b1_d10_c40": 7.7e-16, "b0.01_d10_c2": 1.3e-12, "b0.01_d10_c40": 5.9e-12, "b1_d1000_c3": 1.2e-13}
ORACLE_REPROJ_DEVIATION = {1: 1.5e-14, 255: 2.8e-13, 256: 4.3e-13, 257: 4.1e-13}


def track_cases():
    return [f"mixed_{n}" for n in TRACK_SIZES] + list(TRACK_GEOMETRIES)


def track_args(sc):
    return sc["K4"], sc["ext"], sc["obs_cam"], sc["obs_pt"], sc["obs_uv"], sc["n_pt"]


@functools.lru_cache(maxsize=None)
def track_reference(name):
    """(scene, points, v, x_ref, sigma): the mpmath DLT of at most 40 points of the case that have two or more observations (a fixed
    stride, block edges and the special tracks first)"""
    sc = mixed_tracks_scene(int(name[6:])) if name.startswith("mixed_") else geometry_tracks_scene(name)
    ok = np.flatnonzero(sc["n_views"] >= 2)
    special = [p for p in (0, 253, 254, 255) if p in ok]
    pick = sorted(set(special) | set(ok[::max(1, -(-len(ok) // (40 - len(special))))].tolist()))
    v, x, sig = dlt_tracks(sc["K4"], sc["ext"], sc["obs_cam"], sc["obs_pt"], sc["obs_uv"], pick)
    return sc, np.array(pick, np.int64), v, x, sig


def track_deviation(pts, name):
    """max |x - x_ref| / max |x_ref| over the reference points of the case that are not `equality_only`"""
    sc, pick, _, x, _ = track_reference(name)
    keep = ~np.isin(pick, sc["equality_only"])
    if not keep.any():
        return 0.0
    return float(np.abs(np.asarray(pts)[pick[keep]] - x[keep]).max() / np.abs(x[keep]).max())


REPROJ_SIZES = (1, 255, 256, 257)


def reprojection_case(n_obs, seed=4):
    """observations of the mixed scene's cameras at perturbed points.  From 255 observations on: observation 253 is a point behind its
    camera, 254 (the last thread of the first workgroup) a point with z == 0 exactly (camera 1 is the identity at the origin), 252 and,
    past 255, the last observation a NaN point."""
    sc = mixed_tracks_scene(257)
    rng = np.random.default_rng([seed, n_obs])
    pts = np.concatenate([sc["X"] + 0.01 * rng.standard_normal(sc["X"].shape), [[0.3, -0.2, -8.0], [1.5, -0.5, 0.0], [np.nan] * 3]])
    obs_pt = rng.integers(0, 257, n_obs).astype(np.int32); obs_cam = rng.integers(3, 40, n_obs).astype(np.int32)
    if n_obs >= 255:
        obs_pt[253] = 257; obs_cam[253] = 1
        obs_pt[254] = 258; obs_cam[254] = 1
        obs_pt[252] = 259
        if n_obs > 255:
            obs_pt[n_obs - 1] = 259
    uv = synth.project(synth.K_REF, sc["ext"][obs_cam], sc["X"][np.minimum(obs_pt, 256)]) + 0.5 * rng.standard_normal((n_obs, 2))
    return dict(K4=sc["K4"], ext=sc["ext"], pts=pts, obs_cam=obs_cam, obs_pt=obs_pt, obs_uv=np.ascontiguousarray(uv))


def reprojection_deviation(err, ref):
    """max |err - ref| / max(ref, 1) over the finite reference entries, and whether the non-finite ones agree in kind"""
    err = np.asarray(err, np.float64); f = np.isfinite(ref)
    with np.errstate(invalid="ignore"):
        kinds = np.array_equal(np.isnan(err), np.isnan(ref)) and np.array_equal(np.isposinf(err), np.isposinf(ref))
    dev = float((np.abs(err[f].astype(LD) - ref[f]) / np.maximum(ref[f], 1)).max()) if f.any() else 0.0
    return dev, bool(kinds)


# ---------------------------------------------------------------------------------------------------------------- normals
NORMAL_SIZES = (1, 2, 3, 5, 17, 255, 256, 257, 600)
NORMAL_KS = (1, 2, 3, 10, 16)


def _sphere(n, seed=77):
    return pr.sphere_cloud(n, seed=seed) if n else np.zeros((0, 3))


def _lattice(n):
    return pr.lattice(8)[:n]


def _line(n):
    t = np.random.default_rng(8).permutation(4 * n)[:n] - 2 * n             # distinct integers: every point exactly on the line
    return np.array([0.5, -1.0, 3.0]) + t[:, None] * np.array([0.5, 0.25, -0.25])


def _plane_z7(n):
    rng = np.random.default_rng(12)
    return np.stack([rng.integers(-50, 51, n), rng.integers(-50, 51, n), np.full(n, 7)], axis=1).astype(np.float64)


def _tilted_plane(n):
    rng = np.random.default_rng(13)
    nrm = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    e1 = np.cross(nrm, [0, 0, 1.0]); e1 /= np.linalg.norm(e1); e2 = np.cross(nrm, e1)
    uv = rng.uniform(-2, 2, (n, 2))
    return np.array([0.4, -1.1, 2.5]) + uv[:, :1] * e1 + uv[:, 1:] * e2


def _far_sphere(n):
    rng = np.random.default_rng(14)
    d = rng.standard_normal((n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    return d * 5e-3 + np.array([1e6, -2e6, 3e6])


def _non_finite(n):
    """n = 1200: the cloud of test_points_gpu.py; smaller n: the same three kinds of bad row at rows 7, n / 2 and n - 1"""
    p = _sphere(n, seed=21)
    bad = [[np.nan, 0.1, 0.2], [1.0, np.inf, 0.0], [-np.inf, np.nan, 2.0]]
    for r, b in zip((min(7, n - 1), 500 if n == 1200 else n // 2, n - 1), bad):
        p[r] = b
    return p


NORMAL_CLOUDS = {
    "cube": lambda n: np.random.default_rng(3).uniform(-1.0, 1.0, (n, 3)),
    "sphere": _sphere,
    "lattice8": _lattice,
    "line": _line,
    "identical": lambda n: np.tile(np.array([[0.25, -1.5, 3.0]]), (n, 1)),
    "plane_z7": _plane_z7,
    "tilted_plane": _tilted_plane,
    "far_sphere": _far_sphere,
    "sphere_x5": lambda n: np.repeat(_sphere(-(-n // 5), seed=31), 5, axis=0)[:n],
    "non_finite": _non_finite,
    "sphere_2p100": lambda n: _sphere(n) * 2.0 ** 100,
    "sphere_2m100": lambda n: _sphere(n) * 2.0 ** -100,
}


def normal_sizes(name):
    if name == "lattice8":
        return NORMAL_SIZES[:-1] + (512,)          # the whole lattice(8) in place of 600
    if name == "non_finite":
        return NORMAL_SIZES + (1200,)
    return NORMAL_SIZES


def plane_fit_reference(pts, neighbour_rows):
    """per row: mean and covariance C (divided by the neighbour count) of the listed neighbours (-1: none) in longdouble, eigenvalues
    (ascending) of C by numpy.linalg.eigh, and the magnitudes the error scale needs.  Rows without a neighbour: count 0, the rest NaN."""
    pts = np.asarray(pts, np.float64).reshape(-1, 3); nb = np.asarray(neighbour_rows).reshape(pts.shape[0], -1)
    valid = nb >= 0
    cnt = valid.sum(1)
    with np.errstate(all="ignore"):
        P = np.where(valid[..., None], pts[np.where(valid, nb, 0)], 0.0).astype(LD)
        mean = P.sum(1) / cnt[:, None].astype(LD)
        d = np.where(valid[..., None], P - mean[:, None, :], LD(0))
        C = np.einsum("nka,nkb->nab", d, d) / cnt[:, None, None].astype(LD)
    lam = np.full((pts.shape[0], 3), np.nan)
    has = cnt > 0
    if has.any():
        lam[has] = np.linalg.eigh(C[has].astype(np.float64))[0]
    maxp = np.abs(P).max(axis=(1, 2)).astype(np.float64); maxd = np.abs(d).max(axis=(1, 2)).astype(np.float64)
    return dict(count=cnt, mean=mean, C=C, lam=lam, scale=lam[:, 2] + EPS64 * maxp * maxd)


def normal_metrics(nrm, ref):
    """what the tests assert about normals against plane_fit_reference, over the rows with a neighbour: (largest | |n| - 1 | / eps,
    largest Rayleigh excess (n'Cn - lambda_min) / (eps scale), rows that break the sign rule n.mean <= 0 (beyond 8 eps |mean|),
    whether exactly the rows without a neighbour are NaN in all three components)"""
    nrm = np.asarray(nrm, np.float64); has = ref["count"] > 0
    nan_ok = bool(np.isnan(nrm[~has]).all() and np.isfinite(nrm[has]).all())
    if not has.any() or not nan_ok:
        return 0.0, 0.0, 0, nan_ok
    n = nrm[has].astype(LD); C = ref["C"][has]; mean = ref["mean"][has]
    unit = float(np.abs(np.sqrt((n * n).sum(1)) - 1).max() / EPS64)
    excess = np.einsum("na,nab,nb->n", n, C, n) - ref["lam"][has, 0].astype(LD)
    with np.errstate(all="ignore"):
        rel = np.where(excess <= 0, LD(0), excess / (EPS64 * ref["scale"][has].astype(LD)))    # a scale of 0 (identical points) admits 0 only
    rel = np.where(np.isnan(rel), np.inf, rel)
    dot = (n * mean).sum(1); mlen = np.sqrt((mean * mean).sum(1))
    sign_bad = int(((dot > 0) & (np.abs(dot) > 8 * EPS64 * mlen)).sum())
    return unit, float(rel.max()), sign_bad, nan_ok


@functools.lru_cache(maxsize=None)
def normals_cloud_and_table(name, n):
    """the cloud and its reference neighbour table at K = 16 (a smaller K is its first columns: the order is total)"""
    pts = np.ascontiguousarray(NORMAL_CLOUDS[name](n), np.float64).reshape(-1, 3)
    idx, dist = pr.knn(pts, 16)
    pts.setflags(write=False); idx.setflags(write=False); dist.setflags(write=False)
    return pts, idx, dist


def hybrid_radius(dist):
    """one radius per cloud: the median nearest-neighbour distance, so that about half the rows keep no neighbour at all and the others
    keep a few; 0 where every point coincides with another"""
    d0 = dist[:, 0][np.isfinite(dist[:, 0])]
    return float(np.median(d0)) if len(d0) else 1.0


def hybrid_table(idx, dist, K, r):
    return np.where(dist[:, :K] <= r, idx[:, :K], -1)
