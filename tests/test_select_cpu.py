"""CPU: the numpy restatement of sfmhip_select_views (tests/select_ref.py) against plain Python loops written from the header, the places
of its order statistics, and what the selection is for: on the planted scene with a decoy view next to view 0 the nearest camera
centres hand the dense chain the wrong neighbours, and the shared sparse points hand it the right ones."""
import math

import numpy as np
import pytest

import dense_ref as dr
import select_ref as sr
from sfm_opencv_amd import synth


def _same(a, b):
    a = np.asarray(a); b = np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _loops(ext, pts, obs_cam, obs_pt, n_src, cos2_min):
    """the header's definition, one scalar at a time"""
    ext = np.asarray(ext, np.float64).reshape(-1, 6); pts = np.asarray(pts, np.float64).reshape(-1, 3)
    n = len(ext)
    Rinv, cen = [], []
    for e in ext:
        g = dr.sweep_geometry((1.0, 1.0, 0.0, 0.0), e, np.zeros((0, 6)))
        Rinv.append([float(x) for x in g[4]]); cen.append([float(x) for x in g[5]])
    seen = {}                                                             # point -> set of views
    for c, p in zip(obs_cam, obs_pt):
        c, p = int(c), int(p)
        if 0 <= c < n and 0 <= p < len(pts) and all(math.isfinite(x) for x in pts[p]):
            seen.setdefault(p, set()).add(c)
    shared = [[0] * n for _ in range(n)]; score = [[0] * n for _ in range(n)]
    depths = [[] for _ in range(n)]

    def ray(p, i):
        a = [float(pts[p][k]) - cen[i][k] for k in range(3)]
        return a, (a[0] * Rinv[i][2] + a[1] * Rinv[i][5]) + a[2] * Rinv[i][8]
    for p, views in seen.items():
        views = sorted(views)
        for i in views:
            z = ray(p, i)[1]
            if z > 0:
                depths[i].append(z)
        for x, i in enumerate(views):
            for j in views[x + 1:]:
                (a, zi), (b, zj) = ray(p, i), ray(p, j)
                d = (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]
                na = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]; nb = (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]
                shared[i][j] += 1; shared[j][i] += 1
                if zi > 0 and zj > 0 and (d <= 0 or d * d <= cos2_min * (na * nb)):
                    score[i][j] += 1; score[j][i] += 1
    sources, n_scored, wrange = [], [], []
    for i in range(n):
        first = sorted((j for j in range(n) if j != i and score[i][j] > 0), key=lambda j: (-score[i][j], j))

        def d2(j):
            dx, dy, dz = (cen[j][k] - cen[i][k] for k in range(3))
            return (dx * dx + dy * dy) + dz * dz
        rest = sorted((j for j in range(n) if j != i and score[i][j] == 0), key=lambda j: (d2(j), j))
        sources.append((first + rest)[:n_src]); n_scored.append(min(len(first), n_src))
        s = sorted(depths[i]); m = len(s)
        if m < 2:
            wrange.append((0.0, 0.0))
            continue
        zlo, zhi = s[(2 * (m - 1)) // 100], s[(98 * (m - 1) + 99) // 100]
        wlo, whi = 1.0 / zhi, 1.0 / zlo
        span = whi - wlo
        if not span > 0:
            span = 0.5 * wlo
        x, y = wlo - 0.25 * span, 0.5 * wlo
        wrange.append((y if y > x else x, whi + 0.25 * span))
    return dict(shared=np.array(shared, np.int32), score=np.array(score, np.int32), sources=np.array(sources, np.int32), n_scored=np.array(n_scored, np.int32),
                wrange=np.array(wrange, np.float64), n_depth=np.array([len(d) for d in depths], np.int32))


def _check(ext, pts, oc, op, n_src, cos2):
    got = sr.select_views(ext, pts, oc, op, n_src, cos2); exp = _loops(ext, pts, oc, op, n_src, cos2)
    for k in exp:
        assert _same(got[k], exp[k]), k
    return got


# ------------------------------------------------------------------------------------------------ 1. the restatement against loops
def test_restatement_equals_loops_on_a_ring_scene():
    sc = synth.ba_scene(7, 120)
    got = _check(sc["ext_true"], sc["pts_true"], sc["obs_cam"], sc["obs_pt"], 3, sr.cos2_of(1.0))
    assert got["shared"].sum() > 0 and (got["shared"] == got["shared"].T).all() and (np.diag(got["shared"]) == 0).all()
    assert (got["score"] <= got["shared"]).all() and got["score"].sum() > 0


def test_restatement_equals_loops_with_repeats_bad_points_and_points_behind():
    sc = synth.ba_scene(6, 60, seed=11)
    pts = sc["pts_true"].copy()
    pts[3, 1] = np.nan; pts[7, 0] = np.inf
    pts[11] = 40.0 * pts[11] / np.linalg.norm(pts[11])                   # outside the ring: behind some of its cameras
    oc = np.concatenate([sc["obs_cam"], [0, 5, 2]]).astype(np.int32); op = np.concatenate([sc["obs_pt"], [11, 11, 11]]).astype(np.int32)
    once = _check(sc["ext_true"], pts, oc, op, 2, sr.cos2_of(2.0))
    twice = _check(sc["ext_true"], pts, np.concatenate([oc, oc[:25], oc[-3:]]), np.concatenate([op, op[:25], op[-3:]]), 2, sr.cos2_of(2.0))
    assert all(_same(once[k], twice[k]) for k in once)                   # a repeated pair counts once
    assert (once["score"] < once["shared"]).any()
    clean = sr.select_views(sc["ext_true"], sc["pts_true"], sc["obs_cam"], sc["obs_pt"], 2, sr.cos2_of(2.0))
    assert once["shared"].sum() < clean["shared"].sum()                  # the two non-finite points took their pairs with them


def test_restatement_equals_loops_on_the_smallest_scenes():
    ext = np.array([[0, 0, 0, 0, 0, 0], [0, 0, 0, -1.0, 0, 0], [0, 0.1, 0, 1.0, 0, 0]], float)
    pts = np.array([[0.2, 0.1, 5.0]])
    got = _check(ext[:2], pts, [0, 1], [0, 0], 1, sr.cos2_of(1.0))
    assert got["shared"].tolist() == [[0, 1], [1, 0]] and got["score"].tolist() == [[0, 1], [1, 0]] and got["n_depth"].tolist() == [1, 1]
    assert (got["wrange"] == 0).all() and got["sources"].tolist() == [[1], [0]]
    none = _check(ext, pts, [], [], 2, sr.cos2_of(1.0))                   # no observation: the centres alone
    assert none["sources"].tolist() == [[1, 2], [0, 2], [0, 1]] and (none["n_scored"] == 0).all() and (none["shared"] == 0).all()
    for c2 in (0.0, 1.0):
        _check(ext, np.array([[0.2, 0.1, 5.0], [0.0, 0.0, 3.0], [-0.5, 0.0, -2.0]]), [0, 1, 2, 0, 1, 2, 0, 1], [0, 0, 0, 1, 1, 1, 2, 2], 2, c2)


# ------------------------------------------------------------------------------------------------ 2. the order statistics
@pytest.mark.parametrize("m,lo,hi", [(2, 0, 1), (3, 0, 2), (51, 1, 49), (101, 2, 98), (102, 2, 99)])
def test_order_statistic_places(m, lo, hi):
    """the places are the 2nd and 98th percentile's, the lower rounded down and the upper rounded up: never interpolated, always inside"""
    assert sr.order_statistics(m) == (lo, hi)
    assert lo == math.floor(0.02 * (m - 1) + 1e-12) and hi == math.ceil(0.98 * (m - 1) - 1e-12) and 0 <= lo <= hi <= m - 1


def test_range_of_a_view_comes_from_the_points_it_sees():
    ext = np.array([[0, 0, 0, 0, 0, 0], [0, 0, 0, -1.0, 0, 0]], float)
    z = np.linspace(4.0, 6.0, 101)
    pts = np.stack([np.zeros(101), np.zeros(101), z], 1)
    far = np.array([[0.0, 0.0, 50.0]])                                    # in the cloud, seen by nobody
    got = sr.select_views(ext, np.concatenate([pts, far]), np.repeat([0, 1], 101), np.tile(np.arange(101), 2), 1, sr.cos2_of(1.0))
    assert got["n_depth"].tolist() == [101, 101]
    assert tuple(got["wrange"][0]) == sr.widen(z[2], z[98])
    lo, hi = got["wrange"][0]
    assert lo < 1 / 6.0 < 1 / 4.0 < hi and lo > 1 / 8.0


# ------------------------------------------------------------------------------------------------ 3. and 4. the decoys
@pytest.fixture(scope="module")
def decoy():
    sc, ext, pts, oc, op = sr.decoy_scene()
    return sc, ext, pts, oc, op, sr.select_views(ext, pts, oc, op, 2, sr.cos2_of(1.0))


def test_decoy_is_nearest_to_every_view_and_shares_nothing(decoy):
    sc, ext, pts, oc, op, sel = decoy
    assert len(pts) == 600 and (oc == 4).sum() == 0 and all((oc == i).sum() > 200 for i in range(4))
    near = dr.nearest_sources(ext, 2)
    assert all(4 in near[i] for i in range(4))
    assert all(4 not in sel["sources"][i] for i in range(4)) and (sel["n_scored"][:4] == 2).all()
    assert sel["n_scored"][4] == 0 and sel["n_depth"][4] == 0 and sorted(sel["sources"][4]) == sorted(near[4])
    assert (sel["shared"][4] == 0).all() and (sel["wrange"][:4, 0] < 1 / 6.5).all() and (sel["wrange"][:4, 1] > 1 / 3.9).all()


def test_dense_chain_keeps_pixels_with_ranked_sources_and_none_with_nearest(decoy):
    sc, ext, pts, oc, op, sel = decoy
    images = [sc.render(v)[0] for v in range(5)]
    args = (48, 0.12, 0.32, 2, 1, -1.0, 0.01, 2)
    near = dr.chain(images, sc.K4, ext, dr.nearest_sources(ext, 2), dr.sweep_geometry, *args)
    ranked = dr.chain(images, sc.K4, ext, [list(r) for r in sel["sources"]], dr.sweep_geometry, *args)
    kept_near = [int(v["keep"].sum()) for v in near]; kept_ranked = [int(v["keep"].sum()) for v in ranked]
    print("kept with nearest centres", kept_near, "with ranked sources", kept_ranked)
    assert all(kept_ranked[i] > kept_near[i] for i in range(4))
    assert all(kept_ranked[i] > 0.3 * sc.ROWS * sc.COLS for i in range(4))


def test_a_decoy_without_parallax_is_shared_but_not_scored():
    sc, ext, pts, oc, op = sr.decoy_scene(offset=0.02, angle=0.0)
    sel = sr.select_views(ext, pts, oc, op, 2, sr.cos2_of(1.0))
    assert sel["shared"][0, 4] > 200 and sel["score"][0, 4] == 0 and sel["score"][4, 0] == 0
    assert 4 not in sel["sources"][0] and 4 in dr.nearest_sources(ext, 2)[0]
    assert sel["score"][1, 4] > 200                                      # far enough from the other views
    # without an angle to ask for, sharing is all that counts
    assert sr.select_views(ext, pts, oc, op, 2, 1.0)["score"][0, 4] == sel["shared"][0, 4]
