"""CPU: the numpy restatement of the homography RANSAC and the F/H selection (tests/homography_ref.py, the reference of
tests/test_homography_gpu.py) against independent arithmetic -- distinct samples, the elimination's null vector of the 8 x 9 homography
system against numpy.linalg.svd, the exact fit of a hypothesis to its four rows -- the selection on planted general, planar and
rotation-only scenes, and the surface of the cross-compiled library."""
import numpy as np
import pytest

import homography_ref as hr
import twoview_ref as tv
from sfm_opencv_amd import _lib, api

T1 = 1.0 / tv.FOCAL


def _well_spread(p):
    """four pixels: no two within 50 px, no three within 20 px of a line"""
    for i in range(4):
        for j in range(i + 1, 4):
            if np.linalg.norm(p[i] - p[j]) < 50:
                return False
    for a, b, c in ((0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3)):
        for i, j, k in ((a, b, c), (a, c, b), (b, c, a)):
            d, e = p[j] - p[i], p[k] - p[i]
            if abs(d[0] * e[1] - d[1] * e[0]) / np.linalg.norm(d) < 20:
                return False
    return True


def _spread_samples():
    """(rows 1000 x 4 x 4 normalised): the first 1,000 samples of 4,096 draws on the noisy planar scene that are well spread in both images"""
    pix, _ = hr.scene("planar", 1000, 0.0, 5)
    pos = hr.samples_h(3, 0, 4096, len(pix))
    keep = [h for h in range(len(pos)) if _well_spread(pix[pos[h], :2]) and _well_spread(pix[pos[h], 2:])][:1000]
    assert len(keep) == 1000
    return tv.normalised(pix)[pos[keep]]


@pytest.mark.parametrize("m", (4, 5, 1000))
def test_the_four_positions_of_a_sample_are_distinct_and_in_range(m):
    for p in (0, 1, 7):
        pos = hr.samples_h(12345, p, 1024, m)
        assert pos.shape == (1024, 4) and pos.min() >= 0 and pos.max() < m
        assert (np.diff(np.sort(pos, axis=1), axis=1) > 0).all()
    if m == 4:
        assert (np.sort(pos, axis=1) == np.arange(4)).all()
    else:
        assert len(np.unique(pos[:, 0])) > 1
    assert np.array_equal(hr.samples_h(7, 1, 64, 500)[:32], hr.samples_h(7, 2, 32, 500))          # g = p H + h


def test_null_vector_against_svd_and_exact_fit():
    """measured over the 1,000 well-spread samples: 5.33e-14 against the SVD's vector (the bound is ten times that: conditioning varies
    from sample to sample), |A h| 2.5e-16, du and dv of the sample's own rows 5.8e-16 |w|"""
    S = _spread_samples()
    A = hr.design_h(S)
    Hm, valid = tv.null_vectors(A)
    assert valid.all() and np.allclose(np.linalg.norm(Hm, axis=1), 1.0, rtol=0, atol=4e-16)
    worst = res = fit = 0.0
    for h in range(len(A)):
        v = np.linalg.svd(A[h])[2][-1]
        worst = max(worst, min(np.abs(v - Hm[h]).max(), np.abs(v + Hm[h]).max()))
        res = max(res, np.abs(A[h] @ Hm[h]).max())
        du, dv, w = hr.transfer_terms(Hm[h], S[h])
        fit = max(fit, (np.abs(du) / np.abs(w)).max(), (np.abs(dv) / np.abs(w)).max())
    print(f"[homography] null vector against SVD: {worst:.3g}; |A h| {res:.3g}; exact fit {fit:.3g} |w|")
    assert worst <= 5.4e-13
    assert fit <= 1e-9


def test_design_rows():
    s = np.array([[[2.0, 3.0, 5.0, 7.0]] * 4])
    A = hr.design_h(s)
    assert A.shape == (1, 8, 9)
    assert np.array_equal(A[0, 0], [2, 3, 1, 0, 0, 0, -10, -15, -5]) and np.array_equal(A[0, 1], [0, 0, 0, 2, 3, 1, -14, -21, -7])
    assert np.array_equal(A[0, 6], A[0, 0]) and np.array_equal(A[0, 7], A[0, 1])


def test_four_rows_with_one_repeated_give_no_model():
    rows = hr.scene_rows("planar", 16, out=0.0, seed=2)[:4].copy()
    rows[3] = rows[1]
    Hm, valid = hr.hypotheses_h(rows, 2, 0, 64)
    assert not valid.any() and np.isnan(Hm).all()                 # every sample holds the repeated row: an exact zero pivot
    mask, cnt, win, model = hr.verify_pair_h(rows, 4, 2 * T1, 64, 3, 2, 4)
    assert cnt == 0 and win == -1 and np.isnan(model).all() and not mask.any()


def test_inlier_rule_against_a_transfer_distance_with_division():
    rows = hr.scene_rows("planar", 600, out=0.3, seed=4)
    Hm, valid = hr.hypotheses_h(rows, 9, 0, 64)
    assert valid.all()
    t2 = (2 * T1) ** 2
    got = hr.inliers_h(Hm, rows, t2)
    p1 = np.column_stack([rows[:, 0], rows[:, 1], np.ones(len(rows))])
    q = np.einsum("hij,nj->hni", Hm.reshape(-1, 3, 3), p1)
    dist2 = (q[..., 0] / q[..., 2] - rows[:, 2]) ** 2 + (q[..., 1] / q[..., 2] - rows[:, 3]) ** 2
    clear = np.abs(dist2 - t2) >= 1e-6 * t2
    assert clear.mean() > 0.999 and 0.01 < got.mean() < 0.95
    assert np.array_equal(got[clear], (dist2 <= t2)[clear])


SCENES = [(kind, m, seed) for kind in ("general", "planar", "rotation") for m in (60, 300, 513, 2000) for seed in (1, 2, 3)]


@pytest.mark.parametrize("kind,m,seed", SCENES)
def test_selection_on_planted_scenes(kind, m, seed):
    """t_f = 1 px, t_h = 2 px, H = 256, 3 rounds, hf_ratio 0.8, 30 / 40 / 50 % wrong matches: general scenes are kind 1 (cH / cF measured
    0.00 .. 0.29), planar and rotation-only scenes kind 2 (0.92 .. 1.04); the selected mask keeps at least 85 % of the true matches
    (measured 0.871 .. 1.0)"""
    out = (0.3, 0.4, 0.5)[((60, 300, 513, 2000).index(m) + seed) % 3]
    pix, good = hr.scene(kind, m, out, seed)
    k, mask, cnt, c2, F, Hm, win = hr.two_view_geometry(tv.normalised(pix)[None], [m], T1, 2 * T1, 256, 3, 0, 8, 0.8)
    kept = mask[0][good].sum() / good.sum()
    print(f"[homography] {kind} m {m} seed {seed} out {out}: kind {k[0]}, cF {c2[0, 0]}, cH {c2[0, 1]}, kept {kept:.3f}, wrong {int(mask[0][~good].sum())}")
    assert k[0] == (1 if kind == "general" else 2)
    assert mask[0].sum() == cnt[0] == c2[0, k[0] - 1]
    assert kept >= 0.85


def test_selection_rule():
    assert hr.select(0, 0, 0.8) == 0 and hr.select(10, 0, 0.8) == 1 and hr.select(0, 9, 0.8) == 2
    assert hr.select(10, 8, 0.8) == 2 and hr.select(10, 7, 0.8) == 1 and hr.select(15, 12, 0.8) == 2


def test_library_and_context_carry_the_new_entry_points():
    lib = _lib.load()
    for name in ("sfmhip_verify_pairs_h", "sfmhip_verify_pairs_h_dev", "sfmhip_two_view_geometry", "sfmhip_two_view_geometry_dev",
                 "sfmhip_two_view_geometry_matches_dev"):
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None
    for name in ("verify_pairs_h", "verify_pairs_h_dev", "two_view_geometry", "two_view_geometry_dev", "two_view_geometry_matches_dev"):
        assert callable(getattr(api.Context, name)), name
    assert callable(api.two_view_geometry_for_all)
