"""CPU: the restatement of sfmhip_build_tracks (tests/tracks_ref.py) against scipy's connected components and against hand cases with
their expected arrays written out, its invariances, the scene -> match lists -> tracks round trip, and the argument checks the Python
wrappers make before they need a device."""
import numpy as np
import pytest

import tracks_ref as tr
from sfm_opencv_amd import api, synth


def _first_member_labels(labels):
    """component labels -> the smallest member of every item's component"""
    first = np.full(labels.max() + 1, -1, np.int64)
    for g in range(len(labels) - 1, -1, -1):
        first[labels[g]] = g
    return first[labels]


@pytest.mark.parametrize("n, m, seed", [(1, 0, 0), (50, 20, 1), (300, 200, 2), (300, 2000, 3), (2000, 1500, 4)])
def test_roots_equal_scipy_components(n, m, seed):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    rng = np.random.default_rng(seed)
    e = rng.integers(0, n, size=(m, 2))
    root = tr.roots_of(n, e)
    _, lab = connected_components(coo_matrix((np.ones(m), (e[:, 0], e[:, 1])), shape=(n, n)), directed=False)
    assert np.array_equal(root, _first_member_labels(lab))


def test_hand_case_invalid_elements():
    m, c = tr.pack([[(0, 0)], [(0, 0), (1, 1), (2, 0)], [(0, 0)], [(0, 0), (-1, -1), (1, 7)]], stride=3)
    c[:] = [1, 3, 1, 9]
    out = tr.build_tracks([2, 2], [(0, 0), (0, 1), (0, 5), (1, 0)], m, c)
    assert out["track_of"].tolist() == [0, 1, 0, 1]
    assert out["stats"].tolist() == [2, 4, 2, 0, 0, 5, 2, 0]
    assert out["obs_cam"].tolist() == [0, 1, 0, 1] and out["obs_pt"].tolist() == [0, 0, 1, 1] and out["obs_kp"].tolist() == [0, 0, 1, 1]
    assert out["track_len"].tolist() == [2, 2] and out["counts_out"].tolist() == [0, 2, 0, 1]
    assert out["matches_out"][1]["queryIdx"].tolist() == [0, 1] and out["matches_out"][3]["trainIdx"].tolist() == [0]


def test_hand_case_conflict():
    """a0-b0, b0-c0, c0-a1: features a0 = 0, a1 = 1, b0 = 2, c0 = 3 in one component with two key points of image a"""
    m, c = tr.pack([[(0, 0)], [(0, 0)], [(0, 1)]])
    args = ([2, 1, 1], [(0, 1), (1, 2), (2, 0)], m, c)
    out = tr.build_tracks(*args)
    assert out["track_of"].tolist() == [-1] * 4 and out["stats"].tolist() == [0, 0, 1, 1, 0, 0, 0, 0] and out["counts_out"].tolist() == [0, 0, 0]
    out = tr.build_tracks(*args, flags=tr.KEEP_FIRST)
    assert out["track_of"].tolist() == [0, -1, 0, 0] and out["stats"].tolist() == [1, 3, 1, 1, 0, 0, 3, 0]
    assert out["obs_cam"].tolist() == [0, 1, 2] and out["obs_kp"].tolist() == [0, 0, 0] and out["counts_out"].tolist() == [1, 1, 0]
    out = tr.build_tracks(*args, min_len=4, flags=tr.KEEP_FIRST)
    assert out["track_of"].tolist() == [-1] * 4 and out["stats"].tolist() == [0, 0, 1, 1, 1, 0, 0, 0]


def test_hand_case_smallest_track_and_no_edges():
    m, c = tr.pack([[(1, 0)]])
    out = tr.build_tracks([2, 1], [(0, 1)], m, c)
    assert out["track_of"].tolist() == [-1, 0, 0] and out["stats"].tolist() == [1, 2, 1, 0, 0, 0, 2, 0] and out["track_len"].tolist() == [2]
    out = tr.build_tracks([2, 1], np.zeros((0, 2)), np.zeros((0, 0), tr.DMATCH), [])
    assert out["track_of"].tolist() == [-1] * 3 and not out["stats"].any()
    out = tr.build_tracks([0, 0], [(0, 1)], m, c)
    assert len(out["track_of"]) == 0 and not out["stats"].any() and out["counts_out"].tolist() == [0]


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("track_of", "obs_cam", "obs_pt", "obs_kp", "track_len")) and np.array_equal(a["stats"], b["stats"])


def test_invariance_under_order_and_duplication():
    rng = np.random.default_rng(5)
    n_kp = rng.integers(0, 40, size=9)
    pairs = np.array([(i, j) for i in range(9) for j in range(9) if i != j and rng.random() < 0.4], np.int32)
    lists = []
    for a, b in pairs:
        k = int(min(n_kp[a], n_kp[b]) // 2)
        lists.append(np.stack([rng.permutation(n_kp[a])[:k], rng.permutation(n_kp[b])[:k]], 1))
    m, c = tr.pack(lists)
    for flags in (0, tr.KEEP_FIRST):
        base = tr.build_tracks(n_kp, pairs, m, c, min_len=3, flags=flags)
        assert base["stats"][3] > 0
        perm = rng.permutation(len(pairs))
        shuffled = [lists[q][rng.permutation(len(lists[q]))] for q in perm]
        m2, c2 = tr.pack(shuffled)
        assert _same(base, tr.build_tracks(n_kp, pairs[perm], m2, c2, min_len=3, flags=flags))
        doubled = [np.concatenate([e, e[::-1]]) for e in lists] + [e[:, ::-1] for e in lists]
        m3, c3 = tr.pack(doubled)
        assert _same(base, tr.build_tracks(n_kp, np.concatenate([pairs, pairs[:, ::-1]]), m3, c3, min_len=3, flags=flags))


@pytest.mark.parametrize("reach", [1, 3])
def test_scene_round_trip(reach):
    sc = synth.ba_scene(12, 400)
    kp, _, pairs, lists, pt_of = tr.scene_lists(sc, reach)
    m, c = tr.pack(lists)
    out = tr.build_tracks([len(k) for k in kp], pairs, m, c, kp=kp)
    assert out["stats"].tolist()[:6] == [400, sc["n_obs"], 400, 0, 0, 0]
    assert tr.same_partition(out["track_of"], np.concatenate(pt_of))                 # every scene point is one track
    assert np.array_equal(out["counts_out"], c)
    x = np.concatenate([k["x"] for k in kp]).astype(np.float64)
    off = np.concatenate([[0], np.cumsum([len(k) for k in kp])])
    assert np.array_equal(out["obs_uv"][:, 0], x[off[out["obs_cam"]] + out["obs_kp"]])


def test_wrappers_check_their_arguments_before_they_need_a_device():
    kp = [np.zeros((3, 2)), np.zeros((2, 2))]
    one = [np.zeros(1, api.DMATCH)]
    with pytest.raises(ValueError):
        api.tracks_for_all(kp, None, one, min_len=1)
    with pytest.raises(ValueError):
        api.tracks_for_all(kp, None, one, conflicts="split")
    with pytest.raises(ValueError):
        api.tracks_for_all(kp, None, one + one)                                      # the chain of two images is one pair
    with pytest.raises(ValueError):
        api.tracks_for_all(kp, [(0, 2)], one)
    with pytest.raises(ValueError):
        api.tracks_for_all(kp, [(1, 1)], one)
    with pytest.raises(ValueError):
        api.tracks_for_all([], None, [])
    with pytest.raises(ValueError):
        api.structure_from_tracks(np.eye(3), np.zeros((3, 6)), kp, None, one)        # one pose per image
    n_kp, pairs, matches, counts = api._tracks_inputs(kp, None, [np.zeros(0, api.DMATCH)])
    assert n_kp.tolist() == [3, 2] and pairs.tolist() == [[0, 1]] and matches.shape == (1, 0) and counts.tolist() == [0]
    assert api.DMATCH == tr.DMATCH and api.KEYPOINT == tr.KEYPOINT
