"""CPU: the numpy restatement of the two-view verification (tests/twoview_ref.py, the reference of tests/test_twoview_gpu.py) against
independent arithmetic -- distinct samples, the elimination's null vector against numpy.linalg.svd, the multiplied-out inlier rule
against a Sampson distance computed with its division -- the quality of the definition on synthetic pairs, and the surface of the
cross-compiled library."""
import numpy as np
import pytest

import twoview_ref as tv
from sfm_opencv_amd import _lib


@pytest.mark.parametrize("m", (8, 9, 1000))
def test_the_eight_positions_of_a_sample_are_distinct_and_in_range(m):
    for p in (0, 1, 7):
        pos = tv.samples(12345, p, 1024, m)
        assert pos.shape == (1024, 8) and pos.min() >= 0 and pos.max() < m
        assert (np.diff(np.sort(pos, axis=1), axis=1) > 0).all()
    if m == 8:
        assert (np.sort(pos, axis=1) == np.arange(8)).all()
    else:
        assert len(np.unique(pos[:, 0])) > 1 and len(np.unique(pos, axis=0)) > 512          # the draws differ between hypotheses


def test_rounds_draw_from_different_counters():
    a, b = tv.samples(7, 0, 64, 500), tv.samples(7, 1, 64, 500)
    assert not np.array_equal(a, b)
    assert np.array_equal(tv.samples(7, 1, 64, 500)[:32], tv.samples(7, 2, 32, 500))          # g = p H + h: round 1 of 64 from h = 0 = round 2 of 32


def test_null_vector_against_svd():
    """measured: 5.1e-13 against the SVD's vector, |A f| 2.6e-16"""
    rows = tv.scene_rows(1000, out=0.0, seed=5)
    A = tv.design(rows[tv.samples(3, 0, 256, len(rows))])
    F, valid = tv.null_vectors(A)
    assert valid.all() and np.allclose(np.linalg.norm(F, axis=1), 1.0, rtol=0, atol=4e-16)
    worst = res = 0.0
    for h in range(len(A)):
        v = np.linalg.svd(A[h])[2][-1]
        worst = max(worst, min(np.abs(v - F[h]).max(), np.abs(v + F[h]).max()))
        res = max(res, np.abs(A[h] @ F[h]).max())
    print(f"[twoview] null vector against SVD: {worst:.3g}; |A f| {res:.3g}")
    assert worst <= 1e-9
    assert res <= 1e-13


def test_invalid_hypotheses():
    rows = tv.scene_rows(16, out=0.0, seed=2)[:8]
    dup = rows.copy(); dup[5] = dup[2]
    F, valid = tv.null_vectors(tv.design(dup[None]))
    assert not valid[0] and np.isnan(F).all()                      # a - (a / a) * a: an exact zero pivot
    nan = tv.design(rows[None]); nan[0, 3, 4] = np.nan
    F, valid = tv.null_vectors(nan)
    assert not valid[0] and np.isnan(F).all()


def test_inlier_rule_against_a_sampson_distance_with_division():
    rows = tv.scene_rows(600, out=0.3, seed=4)
    F, valid = tv.hypotheses(rows, 9, 0, 64)
    assert valid.all()
    t2 = (1.0 / 800) ** 2
    got = tv.inliers(F, rows, t2)
    Fm = F.reshape(-1, 3, 3)
    p1 = np.column_stack([rows[:, 0], rows[:, 1], np.ones(len(rows))]); p2 = np.column_stack([rows[:, 2], rows[:, 3], np.ones(len(rows))])
    l = np.einsum("hij,nj->hni", Fm, p1); mt = np.einsum("hji,nj->hni", Fm, p2)
    e = np.einsum("hni,ni->hn", l, p2)
    dist2 = e ** 2 / (l[..., 0] ** 2 + l[..., 1] ** 2 + mt[..., 0] ** 2 + mt[..., 1] ** 2)
    clear = np.abs(dist2 - t2) >= 1e-6 * t2
    assert clear.mean() > 0.999 and 0.05 < got.mean() < 0.95
    assert np.array_equal(got[clear], (dist2 <= t2)[clear])


QUALITY = [(2000, 0.3), (300, 0.3), (300, 0.5), (60, 0.3)]


@pytest.mark.parametrize("pure_translation", (False, True))
@pytest.mark.parametrize("m,out", QUALITY)
def test_quality_of_the_definition(m, out, pure_translation):
    """H = 1024, rounds = 3, t = 1 px: at least 0.8 of the true inliers kept, at most 2 % of the wrong matches accepted (scene seed 1)"""
    pix, good = tv.two_view_scene(m, out, 1, pure_translation)
    det = []
    mask, cnt, win, F = tv.verify_pair(tv.normalised(pix), m, 1.0 / tv.FOCAL, 1024, 3, 0, 8, det)
    kept, wrong = mask[good].sum() / good.sum(), int(mask[~good].sum())
    print(f"[twoview] m {m} out {out} translation {pure_translation}: kept {kept:.3f}, wrong {wrong} of {(~good).sum()}, rounds {det}")
    assert mask.sum() == cnt and win // 1024 == max(d[0] for d in det if not d[3])
    assert kept >= 0.8
    assert wrong <= 0.02 * (~good).sum()


def test_a_pair_is_a_function_of_its_own_rows():
    a, b = tv.scene_rows(100, seed=3), tv.scene_rows(40, seed=4)
    blocks = np.full((2, 120, 4), np.nan); blocks[0, :100] = a; blocks[1, :40] = b; blocks[1, 40:] = 7.0
    mask, cnt, win, F = tv.verify_pairs(blocks, [100, 40], 1 / 800, 128, 3, 5, 8)
    m0, c0, w0, F0 = tv.verify_pair(b, 40, 1 / 800, 128, 3, 5, 8)
    assert np.array_equal(mask[1, :40], m0) and not mask[1, 40:].any() and cnt[1] == c0 and win[1] == w0
    assert np.array_equal(F[1].view(np.uint64), F0.view(np.uint64))


def test_library_exports_the_verification_entry_points():
    lib = _lib.load()
    for name in ("sfmhip_verify_pairs", "sfmhip_verify_pairs_dev", "sfmhip_verify_matches_dev"):
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None
