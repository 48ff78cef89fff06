"""CPU: the numpy restatement of the image registration (tests/pnp_ref.py, the reference of tests/test_pnp_gpu.py) against the properties
the definition in include/sfmhip.h promises, and sfmhip_pose_from_projection, which is host code and needs no GPU."""
import ctypes as C

import numpy as np
import pytest

import pnp_ref as pr
from sfm_opencv_amd import _lib, api

T2 = 2.0 / pr.FOCAL          # two pixels on normalised coordinates


@pytest.mark.parametrize("m", (6, 7, 40, 1000))
def test_samples_are_distinct_in_range_and_the_prescribed_draws(m):
    H, seed, p = 300, 5, 2
    pos = pr.samples(seed, p, H, m)
    srt = np.sort(pos, axis=1)
    assert pos.shape == (H, 6) and pos.min() >= 0 and pos.max() < m and (srt[:, 1:] > srt[:, :-1]).all()
    # the definition, one hypothesis at a time, in plain integers
    mask64 = (1 << 64) - 1

    def r(c):
        z = (seed + (c + 1) * 0x9E3779B97F4A7C15) & mask64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & mask64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & mask64
        return z ^ (z >> 31)
    for h in (0, 1, 77, H - 1):
        g, chosen, want = p * H + h, [], []
        for k in range(6):
            u = r(6 * g + k) % (m - k)
            for s in sorted(chosen):
                u += u >= s
            chosen.append(u); want.append(u)
        assert pos[h].tolist() == want, (h, pos[h], want)
    if m == 6:
        assert (srt == np.arange(6)).all()


def test_a_hypothesis_of_six_exact_rows_fits_its_eleven_equations():
    worst = 0.0
    for seed in range(8):
        rows = pr.scene_rows(6, out=0.0, seed=40 + seed, noise=0.0)
        s = rows[None, :, :]
        P, valid = pr.hypotheses_of(s)
        assert valid[0]
        A = pr.design(s)[0]
        res = np.abs(A @ P[0]).max() / np.abs(A).max()
        worst = max(worst, res)
        # and the twelfth, the row that was left out, follows from the exact geometry
        du, dv, w = pr.residual_terms(P, rows)
        assert (w > 0).all() and np.abs(du / w).max() < 1e-9 and np.abs(dv / w).max() < 1e-9, (seed, du, dv)
        assert abs(np.linalg.norm(P[0]) - 1.0) < 1e-15
    print(f"[pnp] |A p| / |A| of exact six-row hypotheses: {worst:.3g}")
    assert worst < 1e-12                                    # rounding level of an 11 x 12 elimination with complete pivoting


def test_the_null_vector_against_svd():
    rng = np.random.default_rng(3)
    A = rng.standard_normal((50, 11, 12))
    f, valid = pr.null_vectors(A)
    assert valid.all()
    for a, v in zip(A, f):
        n = np.linalg.svd(a)[2][-1]
        assert min(np.abs(v - n).max(), np.abs(v + n).max()) < 1e-10
    # the elimination is size-generic: on 8 x 9 it is the one of the two-view reference, bit for bit
    import twoview_ref as tv
    A = rng.standard_normal((50, 8, 9))
    assert np.array_equal(pr.null_vectors(A)[0].view(np.uint64), tv.null_vectors(A)[0].view(np.uint64))


def test_every_valid_hypothesis_sees_its_first_sample_in_front():
    rows = pr.scene_rows(300, out=0.5, seed=2)
    rows[7] = rows[3]                                       # some samples hold a repeated row: an exact zero pivot
    pos = pr.samples(9, 0, 2048, len(rows))
    P, valid = pr.hypotheses_of(rows[pos])
    w0 = pr.depth(P, rows)[np.arange(len(P)), pos[:, 0]]
    assert valid.sum() > 1500 and (w0[valid] > 0).all() and np.isnan(P[~valid]).all()
    both = (pos == 3).any(axis=1) & (pos == 7).any(axis=1)
    assert both.any() and not valid[both].any()
    # the rule negates, it does not recompute: without it the hypotheses are these up to sign
    f, v0 = pr.null_vectors(pr.design(rows[pos]))
    assert np.array_equal(np.abs(f[valid]), np.abs(P[valid]))
    assert ((f[valid] != P[valid]).any(axis=1)).sum() > 100   # and it does fire


SCENES = [(m, out, seed) for m in (40, 300, 2000) for out in (0.3, 0.5) for seed in range(4)]


@pytest.fixture(scope="module")
def general_results():
    """(m, out, recall, wrong, sv_ratio, rotation error, translation error) of the 24 general planted scenes at H = 1024, 3 rounds, 2 px"""
    res = []
    for m, out, seed in SCENES:
        rows_px, good, R, T = pr.planted_scene(m, out, 100 + seed)
        mask, cnt, win, P = pr.register_view(pr.normalised(rows_px), m, T2, 1024, 3, 7, 6)
        mask = mask.astype(bool)
        Rg, tg, sv = pr.pose_from_projection(P)
        res.append((m, out, (mask & good).sum() / good.sum(), int((mask & ~good).sum()), sv, np.abs(Rg - R).max(), np.abs(tg - T).max()))
    return res


def test_quality_on_the_general_planted_scenes(general_results):
    for m, out, recall, wrong, sv, er, et in general_results:
        print(f"[pnp] m {m} out {out}: recall {recall:.3f}, wrong {wrong}, sv_ratio {sv:.4f}, |R - R0| {er:.2e}, |t - t0| {et:.2e}")
    # What the restatement reaches on these scenes: recall 0.994 .. 1.000, no wrong correspondence accepted.  The bounds leave the scene
    # generator room: a true match at 0.5 px noise per axis lies beyond 2 px with probability exp(-8) = 3e-4, so what is missed beyond
    # that is the model's own error (a DLT from six noisy rows, re-sampled from its inliers twice), and a uniform wrong observation
    # falls within 2 px of its point's image with probability pi 2^2 / (1024 x 768) = 1.6e-5, 0.016 expected over all 24 scenes
    assert min(r[2] for r in general_results) >= 0.98
    assert max(r[3] for r in general_results) <= 1
    assert max(r[4] for r in general_results) <= 1.09


def test_pose_from_projection_on_noise_free_scenes():
    lib = _lib.load()
    ref_err, lib_err = [], []
    for m, seed in [(40, s) for s in range(6)] + [(300, s) for s in range(6)]:
        rows_px, good, R0, T0 = pr.planted_scene(m, 0.0, 300 + seed, noise=0.0)
        mask, cnt, win, P = pr.register_view(pr.normalised(rows_px), m, 1e-6, 64, 2, 7, 6)
        assert cnt == m
        Rn, tn, svn = pr.pose_from_projection(P)
        ref_err.append(max(np.abs(Rn - R0).max(), np.abs(tn - T0).max()))
        R = np.full(9, 7.0); t = np.full(3, 7.0); sv = C.c_double(7.0)
        assert lib.sfmhip_pose_from_projection(P.ctypes.data, R.ctypes.data, t.ctypes.data, C.byref(sv)) == 0
        lib_err.append(max(np.abs(R.reshape(3, 3) - R0).max(), np.abs(t - T0).max()))
        assert abs(sv.value - svn) <= 1e-12 * svn and 1.0 <= sv.value < 1.0 + 1e-9
        assert abs(np.linalg.det(R.reshape(3, 3)) - 1.0) < 1e-14 and np.abs(R.reshape(3, 3) @ R.reshape(3, 3).T - np.eye(3)).max() < 1e-14
    # the tolerance: ten times the error that the reference's own P shows through numpy.linalg.svd on these scenes (5.1e-14 where this
    # was written, so 5.1e-13: the error is the elimination's, in P, not the SVD's)
    tol = 10.0 * max(ref_err)
    print(f"[pnp] pose of noise-free scenes: numpy.linalg.svd {max(ref_err):.3g}, library {max(lib_err):.3g}, tolerance {tol:.3g}")
    assert max(lib_err) <= tol and tol < 1e-11


def test_sv_ratio_separates_coplanar_scenes_from_general_ones(general_results):
    lib = _lib.load()
    planar = []
    for m, out, seed in [(m, out, s) for m in (40, 300) for out in (0.3, 0.5) for s in range(3)]:
        rows_px, good, R0, T0 = pr.planted_scene(m, out, 200 + seed, coplanar=True)
        mask, cnt, win, P = pr.register_view(pr.normalised(rows_px), m, T2, 1024, 3, 7, 6)
        mask = mask.astype(bool)
        assert (mask & good).sum() >= 0.98 * good.sum() and (mask & ~good).sum() <= 1            # the inlier set is still right
        R = np.full(9, 7.0); t = np.full(3, 7.0); sv = C.c_double(7.0)
        rc = lib.sfmhip_pose_from_projection(P.ctypes.data, R.ctypes.data, t.ctypes.data, C.byref(sv))
        assert rc in (_lib.OK, _lib.E_NUMERIC) and (rc == _lib.OK or (R == 7.0).all() and (t == 7.0).all())
        planar.append(sv.value)
        ok, _, _, sv2 = api.pose_from_projection(P)
        assert ok == (rc == 0) and sv2 == sv.value
    general = [r[4] for r in general_results]
    print(f"[pnp] sv_ratio: general {min(general):.4f} .. {max(general):.4f}, coplanar {min(planar):.3g} .. {max(planar):.3g}")
    assert max(general) < api.SV_RATIO_MAX < min(planar) and min(planar) > 1e9


def test_pose_from_projection_fails_cleanly():
    lib = _lib.load()
    good = np.array([[2.0, 0, 0, 2], [0, 2.0, 0, 4], [0, 0, 2.0, 6]])

    def call(P):
        P = np.ascontiguousarray(P, np.float64)
        R = np.full(9, 7.0); t = np.full(3, 7.0); sv = C.c_double(7.0)
        return lib.sfmhip_pose_from_projection(P.ctypes.data, R.ctypes.data, t.ctypes.data, C.byref(sv)), R, t, sv.value
    rc, R, t, sv = call(good)
    assert rc == 0 and np.array_equal(R.reshape(3, 3), np.eye(3)) and np.array_equal(t, [1.0, 2.0, 3.0]) and sv == 1.0
    for bad in (np.full((3, 4), np.nan), np.where(np.arange(12).reshape(3, 4) == 5, np.inf, good), np.zeros((3, 4))):
        rc, R, t, sv = call(bad)
        assert rc == _lib.E_NUMERIC and (R == 7.0).all() and (t == 7.0).all() and sv == 7.0
    mirror = good.copy(); mirror[2, 2] = -2.0                # det < 0: a reflection
    rc, R, t, sv = call(mirror)
    assert rc == _lib.E_NUMERIC and (R == 7.0).all() and (t == 7.0).all() and sv == 1.0
    R = np.zeros(9); t = np.zeros(3); sv = C.c_double(0)
    assert lib.sfmhip_pose_from_projection(None, R.ctypes.data, t.ctypes.data, C.byref(sv)) == _lib.E_ARG
    assert lib.sfmhip_pose_from_projection(good.ctypes.data, R.ctypes.data, t.ctypes.data, None) == _lib.E_ARG
    ok, R, t, sv = api.pose_from_projection(np.full(12, np.nan))
    assert not ok and np.isnan(R).all() and np.isnan(t).all() and np.isnan(sv)
