"""CPU: the numpy restatement of the plane segmentation (tests/plane_ref.py) checked against what is known independently of it -- the
published splitmix64 sequence, the range and distinctness of its triples, numpy's SVD plane of a planted plane -- and the presence of
the three entry points in the library and in api.Context."""
import os

import numpy as np

import plane_ref as pf
from sfm_opencv_amd import _lib, api


def test_splitmix64_reproduces_the_published_sequence():
    # the first outputs of splitmix64 seeded with 0 (Vigna's splitmix64.c; the sequence java.util.SplittableRandom is built on):
    # the state after k + 1 steps is seed + (k + 1) * golden gamma, which is r(k)
    want = [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F, 0xF88BB8A8724C81EC, 0x1B39896A51A8749B]
    got = pf.r(0, np.arange(5, dtype=np.uint64))
    assert [int(v) for v in got] == want


def test_triples_are_distinct_and_in_range():
    for m in range(3, 71):
        for p in (0, 3):
            u0, u1, u2 = pf.triples(12345, p, 512, m)
            for u in (u0, u1, u2):
                assert u.min() >= 0 and u.max() < m, (m, p)
            assert ((u0 != u1) & (u0 != u2) & (u1 != u2)).all(), (m, p)
    # every position is drawn, and rounds differ
    u = np.concatenate(pf.triples(1, 0, 512, 7))
    assert set(u.tolist()) == set(range(7))
    assert not np.array_equal(pf.triples(1, 0, 512, 70)[0], pf.triples(1, 1, 512, 70)[0])


def test_the_winner_on_a_planted_plane_agrees_with_the_svd_plane():
    pts, truth = pf.planted_scene()
    sigma, t = 0.002, 0.006
    labels, n_planes, planes, counts, winner = pf.segment(pts, t, 256, 12345, 50, 3)
    assert n_planes == 3 and counts.sum() == (labels >= 0).sum()
    for p in range(3):
        src = np.bincount(truth[labels == p] + 1).argmax() - 1            # the planted plane most of the inliers came from
        assert src >= 0
        P = pts[truth == src]
        assert counts[p] >= 0.95 * len(P)
        c = P.mean(axis=0)
        nrm = np.linalg.svd(P - c)[2][2]
        # a plane through three points of noise sigma spread over an extent of 2: the normal is off by a few sigma / extent, and the
        # winner keeps 95 % of the points within t = 3 sigma, so its tilt over the half extent 1 stays below t
        assert np.sqrt(max(0.0, 1.0 - float(planes[p, :3] @ nrm) ** 2)) <= t
        assert abs(abs(planes[p, :3] @ c + planes[p, 3])) <= t
        assert planes[p, 3] >= 0 and abs(np.linalg.norm(planes[p, :3]) - 1) <= 4e-16
    assert sigma < t


def test_the_library_exports_the_entry_points():
    names = ("sfmhip_segment_planes", "sfmhip_segment_planes_dev", "sfmhip_segment_plane")
    for name in names:
        assert name in _lib.SYMBOLS
    assert os.path.exists(_lib.LIB_PATH), "build libsfmhip.so first (__graft_entry__.build)"
    lib = _lib.load()
    for name in names:
        assert hasattr(lib, name), name
    for meth in ("segment_planes", "segment_planes_dev", "segment_plane"):
        assert callable(getattr(api.Context, meth, None)), meth
