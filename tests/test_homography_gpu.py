"""GPU: the homography RANSAC and the F/H model selection (sfmhip_verify_pairs_h, sfmhip_two_view_geometry and their device and match-list
forms) through the C-ABI, the Python layer and the NViewReconstruct driver.  The reference is tests/homography_ref.py (with
tests/twoview_ref.py for F), a numpy restatement of the definition in include/sfmhip.h.  In every comparison with it masks, counts,
winners and kinds must be EQUAL and Hm and F equal in every bit (compared as uint64 views, the NaN rows of the pairs without a model
included)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import homography_ref as hr
import twoview_ref as tv
from sfm_opencv_amd import _lib, api, features_io
from test_twoview_gpu import _bits, _blocks, _check_winner_in_parts, _match_scene, _subset

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
HOST = os.path.join(os.path.dirname(HERE), "sfm_opencv_amd", "host")
CHUNK = 512                  # twoview.hip: rows staged in LDS per pass of homography_score_kernel
T1 = 1.0 / tv.FOCAL          # one pixel on normalised coordinates
T2 = 2.0 / tv.FOCAL          # the homography's threshold in the tests
_cache = {}


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _raw_h(ctx, blocks, counts, t, H, rounds, seed, min_inliers, want_H=True):
    """sfmhip_verify_pairs_h on the C-ABI's own arrays: (mask n x stride, count, winner, Hm n x 9), pre-filled with values the call never writes"""
    blocks = np.ascontiguousarray(blocks, np.float64); counts = np.ascontiguousarray(counts, np.int32)
    n, stride = blocks.shape[0], blocks.shape[1]
    mask = np.full((n, stride), 7, np.uint8); cnt = np.full(n, -7, np.int32); win = np.full(n, -7, np.int32); Hm = np.full((n, 9), 7.0)
    rc = ctx.lib.sfmhip_verify_pairs_h(ctx.h, blocks.ctypes.data, stride, counts.ctypes.data, n, t, H, rounds, seed, min_inliers, mask.ctypes.data,
                                       cnt.ctypes.data, Hm.ctypes.data if want_H else None, win.ctypes.data if want_H else None)
    assert rc == 0, ctx.lib.sfmhip_last_error(ctx.h)
    return mask, cnt, win, Hm


def _check_h(ctx, blocks, counts, t, H, rounds, seed, min_inliers, ref=None, tag=None):
    """the library against the restatement on every output; returns the library's"""
    if ref is None:
        ref = hr.verify_pairs_h(blocks, counts, t, H, rounds, seed, min_inliers)
    got = _raw_h(ctx, blocks, counts, t, H, rounds, seed, min_inliers)
    what = (tag, t, H, rounds, seed, min_inliers)
    assert np.array_equal(got[1], ref[1]) and got[1].dtype == np.int32, (what, got[1], ref[1], got[2], ref[2])
    assert np.array_equal(got[2], ref[2]), (what, got[2], ref[2])
    bad = np.argwhere(got[0] != ref[0])
    assert len(bad) == 0, (what, len(bad), bad[:5])
    assert np.array_equal(_bits(got[3]), _bits(ref[3])), (what, got[3], ref[3])
    assert np.array_equal(got[0].sum(axis=1), got[1])
    return got


def _raw_g(ctx, blocks, counts, t_f, t_h, H, rounds, seed, min_inliers, ratio, optional=True):
    """sfmhip_two_view_geometry on pre-filled arrays: (kind, mask, count, counts2, F, Hm, winners)"""
    blocks = np.ascontiguousarray(blocks, np.float64); counts = np.ascontiguousarray(counts, np.int32)
    n, stride = blocks.shape[0], blocks.shape[1]
    kind = np.full(n, -7, np.int32); mask = np.full((n, stride), 7, np.uint8); cnt = np.full(n, -7, np.int32); c2 = np.full((n, 2), -7, np.int32)
    F = np.full((n, 9), 7.0); Hm = np.full((n, 9), 7.0); win = np.full((n, 2), -7, np.int32)
    opt = [a.ctypes.data if optional else None for a in (c2, F, Hm, win)]
    rc = ctx.lib.sfmhip_two_view_geometry(ctx.h, blocks.ctypes.data, stride, counts.ctypes.data, n, t_f, t_h, H, rounds, seed, min_inliers, ratio,
                                          kind.ctypes.data, mask.ctypes.data, cnt.ctypes.data, *opt)
    assert rc == 0, ctx.lib.sfmhip_last_error(ctx.h)
    return kind, mask, cnt, c2, F, Hm, win


def _same_g(got, ref, what=None):
    for k, name in enumerate(("kind", "mask", "count", "counts2")):
        assert np.array_equal(got[k], ref[k]), (what, name, got[k], ref[k])
    assert np.array_equal(_bits(got[4]), _bits(ref[4])) and np.array_equal(_bits(got[5]), _bits(ref[5])), (what, "models")
    assert np.array_equal(got[6], ref[6]), (what, "winners", got[6], ref[6])
    assert np.array_equal(got[1].sum(axis=1), got[2])


# ---- one pair: list lengths around the chunk of the scoring kernel, hypothesis-block edges, the number of rounds -----------------------
@pytest.mark.parametrize("H", (1, 65, 256, 257))
def test_single_pair_equals_the_reference(ctx, H):
    for m in (0, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3):
        rows = _cached(("rows", m), lambda: hr.scene_rows("planar", m, out=0.3, seed=10 + m))
        blocks, counts = _blocks([rows])
        for rounds in (1, 3, 8):
            got = _check_h(ctx, blocks, counts, T2, H, rounds, 77, 4, tag=f"m={m}")
            print(f"[homography] m = {m}, H = {H}, rounds = {rounds}: count {got[1][0]}, winner {got[2][0]}")
            if m < 4:
                assert got[1][0] == 0 and got[2][0] == -1 and np.isnan(got[3]).all() and not got[0].any()
            elif H >= 256 and m >= CHUNK - 1:
                assert got[1][0] >= 0.5 * m                           # 70 % of the rows are true matches on one plane


def test_a_workgroup_that_strides_over_several_chunks(ctx):
    # the shape and the parts of the test of this name in test_twoview_gpu.py, through homography_score_kernel
    H, m, seed = 65536, 8 * CHUNK + 2 * CHUNK + 7, 21
    rows = hr.scene_rows("planar", m, out=0.3, seed=12)
    got = _raw_h(ctx, *_blocks([rows]), T2, H, 1, seed, 4)
    pos = hr.samples_h(seed, 0, H, m)
    srt = np.sort(pos, axis=1)
    assert pos.min() >= 0 and pos.max() < m and (srt[:, 1:] > srt[:, :-1]).all()
    assert 0 <= got[2][0] < H
    sub = np.union1d(_subset(H), [got[2][0]])
    Hm, valid = hr.null_vectors(hr.design_h(rows[pos[sub]]))
    cnt = hr.counts_of_h(Hm, valid, rows, T2 * T2)
    _check_winner_in_parts(got, sub, Hm, valid, cnt, hr.inliers_h(got[3][0], rows, T2 * T2)[0])
    assert got[1][0] >= 0.5 * m


# ---- input edges -----------------------------------------------------------------------------------------------------------------------
def test_rows_behind_the_count_are_never_read(ctx):
    rows = _cached(("rows", 300), lambda: hr.scene_rows("rotation", 300, out=0.3, seed=3))
    ref = hr.verify_pairs_h(*_blocks([rows]), T2, 256, 3, 5, 4)
    for fill in (7.0, np.nan):
        blocks, counts = _blocks([rows], stride=300 + 77, fill=fill)
        got = _check_h(ctx, blocks, counts, T2, 256, 3, 5, 4, tag=f"fill={fill}")
        assert not got[0][:, 300:].any() and np.array_equal(got[0][:, :300], ref[0]) and np.array_equal(_bits(got[3]), _bits(ref[3]))
    assert ref[1][0] > 150


def test_non_finite_rows_are_never_sampled_and_never_inliers(ctx):
    rows = hr.scene_rows("planar", 700, out=0.3, seed=4).copy()
    rows[::37] = np.nan
    rows[5, 2] = np.inf
    rows[6, 1] = -np.inf
    blocks, counts = _blocks([rows])
    got = _check_h(ctx, blocks, counts, T2, 256, 3, 1, 4, tag="non-finite")
    assert got[1][0] > 300 and not got[0][0, ::37].any() and not got[0][0, 5] and not got[0][0, 6]
    finite = rows[np.isfinite(rows).all(axis=1)]
    alone = _raw_h(ctx, *_blocks([finite]), T2, 256, 3, 1, 4)
    assert alone[1][0] == got[1][0] and alone[2][0] == got[2][0] and np.array_equal(_bits(alone[3]), _bits(got[3]))      # the same L_0


def test_duplicate_rows(ctx):
    base = hr.scene_rows("planar", 40, out=0.0, seed=6)
    four = base[:4].copy(); four[3] = four[1]
    got = _check_h(ctx, *_blocks([four]), T2, 64, 3, 2, 4, tag="dup4")
    assert got[1][0] == 0 and got[2][0] == -1 and np.isnan(got[3]).all() and not got[0].any()      # every hypothesis: an exact zero pivot
    five = base[:5].copy(); five[3] = five[1]
    got = _check_h(ctx, *_blocks([five]), T2, 64, 3, 2, 4, tag="dup5")
    assert got[1][0] >= 4 and got[0][0, 1] == got[0][0, 3]


def test_ties_go_to_the_smallest_h_and_round_1_stops(ctx):
    base = hr.scene_rows("planar", 200, out=0.3, seed=8)
    rows = np.concatenate([np.repeat(base[:2], 40, axis=0), base[2:]])           # duplicates: many hypotheses are invalid, h = 0 among them
    det = []
    hr.verify_pair_h(rows, len(rows), 1e6, 257, 3, 3, 4, det)
    Hm, valid = hr.hypotheses_h(rows, 3, 0, 257)
    first = int(np.flatnonzero(valid)[0])
    assert det == [(0, first, len(rows), False), (1, det[1][1], len(rows), True)] and first > 0
    got = _check_h(ctx, *_blocks([rows]), 1e6, 257, 3, 3, 4, tag="ties")
    assert got[1][0] == len(rows) and got[2][0] == first and got[0].all()


def test_threshold_zero(ctx):
    rows = hr.scene_rows("planar", 300, out=0.3, seed=9)
    _check_h(ctx, *_blocks([rows]), 0.0, 256, 3, 1, 4, tag="t=0")
    # integer rows under a translation by (1, 2): every hypothesis of four rows in general position satisfies all rows exactly or nearly
    g = np.stack(np.meshgrid(np.arange(6.0), np.arange(5.0), indexing="ij"), -1).reshape(-1, 2)
    lat = np.column_stack([g, g[:, 0] + 1, g[:, 1] + 2])
    got = _check_h(ctx, *_blocks([lat]), 0.0, 256, 2, 3, 4, tag="t=0 lattice")
    print(f"[homography] t = 0 on the lattice: count {got[1][0]}, winner {got[2][0]}")


def test_min_inliers_around_a_pairs_count(ctx):
    rows = _cached(("rows", 300), lambda: hr.scene_rows("rotation", 300, out=0.3, seed=3))
    blocks, counts = _blocks([rows])
    c = int(_check_h(ctx, blocks, counts, T2, 256, 3, 5, 4)[1][0])
    assert c > 150
    got = _check_h(ctx, blocks, counts, T2, 256, 3, 5, c, tag="min_inliers = count")
    assert got[1][0] == c
    got = _check_h(ctx, blocks, counts, T2, 256, 3, 5, c + 1, tag="min_inliers = count + 1")
    assert got[1][0] == 0 and got[2][0] == -1 and np.isnan(got[3]).all() and not got[0].any()


# ---- a batch, and the combined call ------------------------------------------------------------------------------------------------
KINDS = ("general", "planar", "rotation")
SIZES = (0, 5, 8, 300, 3, 2000, 64, 513, 9, 1100, 40, 150)
G = (256, 4, 11, 8, 0.8)         # H, rounds, seed, min_inliers, hf_ratio of the batch


def _batch():
    """twelve pairs of mixed kinds; the references of both single-model calls and of the combined one"""
    rows = [hr.scene_rows(KINDS[k % 3], m, out=(0.3, 0.5, 0.1, 0.4)[k % 4], seed=20 + k) for k, m in enumerate(SIZES)]
    blocks, counts = _blocks(rows, stride=2000, fill=np.nan)
    H, rounds, seed, mi, ratio = G
    refF = tv.verify_pairs(blocks, counts, T1, H, rounds, seed, mi)
    refH = hr.verify_pairs_h(blocks, counts, T2, H, rounds, seed, mi)
    return blocks, counts, refF, refH, hr.two_view_geometry(blocks, counts, T1, T2, H, rounds, seed, mi, ratio, single=(refF, refH))


def test_a_batch_equals_its_pairs_alone(ctx):
    blocks, counts, refF, ref, refG = _cached("batch", _batch)
    H, rounds, seed, mi, ratio = G
    rounds_of = ref[2] // H
    assert len(set(rounds_of[ref[2] >= 0].tolist())) >= 2, rounds_of           # the models come from different rounds
    got = _check_h(ctx, blocks, counts, T2, H, rounds, seed, mi, ref=ref, tag="batch")
    again = _raw_h(ctx, blocks, counts, T2, H, rounds, seed, mi)
    for a, b in zip(got, again):
        assert a.tobytes() == b.tobytes()
    for q in (2, 3, 5, 7, 10):                                                  # alone, in a block of its own length
        one = _raw_h(ctx, blocks[q:q + 1, :max(1, counts[q])], counts[q:q + 1], T2, H, rounds, seed, mi)
        assert np.array_equal(one[0][0], got[0][q, :max(1, counts[q])]) and one[1][0] == got[1][q] and one[2][0] == got[2][q]
        assert np.array_equal(_bits(one[3][0]), _bits(got[3][q]))
    # Hm and winner are optional
    part = _raw_h(ctx, blocks, counts, T2, H, rounds, seed, mi, want_H=False)
    assert part[0].tobytes() == got[0].tobytes() and part[1].tobytes() == got[1].tobytes() and (part[2] == -7).all() and (part[3] == 7).all()


def test_the_combined_call_is_the_two_calls_and_the_rule(ctx):
    blocks, counts, refF, refH, refG = _cached("batch", _batch)
    H, rounds, seed, mi, ratio = G
    assert set(refG[0].tolist()) == {0, 1, 2}, refG[0]
    for q, m in enumerate(SIZES):
        if m >= 64:
            assert refG[0][q] == (1 if KINDS[q % 3] == "general" else 2), (q, m, refG[0], refG[3])
    got = _raw_g(ctx, blocks, counts, T1, T2, H, rounds, seed, mi, ratio)
    _same_g(got, refG, "batch")
    print(f"[homography] batch kinds {got[0].tolist()}, counts2 {got[3].tolist()}")
    # against the library's own single-model calls
    from test_twoview_gpu import _raw
    f = _raw(ctx, blocks, counts, T1, H, rounds, seed, mi); h = _raw_h(ctx, blocks, counts, T2, H, rounds, seed, mi)
    assert np.array_equal(got[3], np.column_stack([f[1], h[1]])) and np.array_equal(got[6], np.column_stack([f[2], h[2]]))
    assert np.array_equal(_bits(got[4]), _bits(f[3])) and np.array_equal(_bits(got[5]), _bits(h[3]))
    for q in range(len(counts)):
        want = (np.zeros_like(f[0][q]), f[0][q], h[0][q])[got[0][q]]
        assert np.array_equal(got[1][q], want), q
    again = _raw_g(ctx, blocks, counts, T1, T2, H, rounds, seed, mi, ratio)
    for a, b in zip(got, again):
        assert a.tobytes() == b.tobytes()
    # null optional outputs leave the others unchanged
    part = _raw_g(ctx, blocks, counts, T1, T2, H, rounds, seed, mi, ratio, optional=False)
    for k in (0, 1, 2):
        assert part[k].tobytes() == got[k].tobytes()
    assert (part[3] == -7).all() and (part[4] == 7).all() and (part[5] == 7).all() and (part[6] == -7).all()


def test_only_h_reaches_min_inliers_and_neither_does(ctx):
    # t_f = 0: F keeps little more than its own eight rows, below min_inliers = 20.  Pair 0 is a plane (H reaches it), pair 1 is all
    # wrong matches (neither does), pair 2 a general scene
    rng = np.random.default_rng(5)
    rows = [hr.scene_rows("planar", 100, out=0.1, seed=71), tv.normalised(np.column_stack([rng.uniform(0, 1024, (50, 1)), rng.uniform(0, 768, (50, 1)),
            rng.uniform(0, 1024, (50, 1)), rng.uniform(0, 768, (50, 1))])), hr.scene_rows("general", 300, out=0.3, seed=72)]
    blocks, counts = _blocks(rows)
    ref = hr.two_view_geometry(blocks, counts, 0.0, T2, 256, 3, 9, 20, 0.8)
    assert ref[0][0] == 2 and ref[3][0, 0] == 0 and ref[3][0, 1] >= 80 and np.isnan(ref[4][0]).all(), (ref[0], ref[3])
    assert ref[0][1] == 0 and not ref[3][1].any() and not ref[1][1].any() and np.isnan(ref[4][1]).all() and np.isnan(ref[5][1]).all(), (ref[0], ref[3])
    got = _raw_g(ctx, blocks, counts, 0.0, T2, 256, 3, 9, 20, 0.8)
    _same_g(got, ref, "only H / neither")
    # the ratio decides on the computed product: at hf_ratio = cH / cF + a little the pair turns general
    blocks, counts, refF, refH, refG = _cached("batch", _batch)
    q = 7
    cF, cH = refG[3][q]
    assert cF > 0 and cH > 0
    for ratio in (cH / cF, np.nextafter(cH / cF, 9.0) * (1 + 1e-12)):
        ref = hr.two_view_geometry(blocks[q:q + 1], counts[q:q + 1], T1, T2, 256, 4, 11, 8, ratio, single=([a[q:q + 1] for a in refF], [a[q:q + 1] for a in refH]))
        _same_g(_raw_g(ctx, blocks[q:q + 1], counts[q:q + 1], T1, T2, 256, 4, 11, 8, ratio), ref, ("ratio", ratio))


def test_a_batch_longer_than_one_launch(ctx):
    # twoview.hip enqueues a batch in slices of 32768 pairs: pairs at the end of the first slice and in the second, everything else empty
    n, stride = 32768 + 5, 16
    blocks = np.full((n, stride, 4), np.nan); counts = np.zeros(n, np.int32)
    live = (0, 32767, 32768, n - 1)
    for k, q in enumerate(live):
        rows = hr.scene_rows(("planar", "general")[k & 1], 12 + k, out=0.0, seed=60 + k)
        blocks[q, :len(rows)] = rows; counts[q] = len(rows)
    got = _raw_g(ctx, blocks, counts, T1, T2, 64, 2, 3, 8, 0.8)
    for q in live:
        ref = hr.two_view_geometry(blocks[q:q + 1], counts[q:q + 1], T1, T2, 64, 2, 3, 8, 0.8)
        assert ref[2][0] >= 8 and ref[0][0] in (1, 2)
        _same_g([a[q:q + 1] for a in got], ref, q)
    rest = np.ones(n, bool); rest[list(live)] = False
    assert not got[0][rest].any() and not got[1][rest].any() and not got[2][rest].any() and not got[3][rest].any() and (got[6][rest] == -1).all()
    assert np.isnan(got[4][rest]).all() and np.isnan(got[5][rest]).all()


# ---- the Python layer and the device entry points --------------------------------------------------------------------------------------
def test_python_layer_and_device_arrays(ctx):
    import torch
    blocks, counts, refF, refH, refG = _cached("batch", _batch)
    H, rounds, seed, mi, ratio = G
    lists = [blocks[q, :counts[q]] for q in range(len(counts))]
    masks, cnt, Hm, win = ctx.verify_pairs_h(lists, T2, hypotheses=H, rounds=rounds, seed=seed, min_inliers=mi)
    assert np.array_equal(cnt, refH[1]) and np.array_equal(win, refH[2]) and np.array_equal(_bits(Hm.reshape(-1, 9)), _bits(refH[3]))
    for q, m in enumerate(masks):
        assert m.dtype == bool and np.array_equal(m, refH[0][q, :counts[q]].astype(bool))
    kind, masks, cnt, c2, F, Hm, wins = ctx.two_view_geometry(lists, T1, T2, hypotheses=H, rounds=rounds, seed=seed, min_inliers=mi, hf_ratio=ratio)
    assert np.array_equal(kind, refG[0]) and np.array_equal(cnt, refG[2]) and np.array_equal(c2, refG[3]) and np.array_equal(wins, refG[6])
    assert np.array_equal(_bits(F.reshape(-1, 9)), _bits(refG[4])) and np.array_equal(_bits(Hm.reshape(-1, 9)), _bits(refG[5]))
    for q, m in enumerate(masks):
        assert np.array_equal(m, refG[1][q, :counts[q]].astype(bool))
    n, stride = blocks.shape[:2]
    d_corr = torch.from_numpy(blocks).cuda(); d_counts = torch.from_numpy(counts).cuda()
    i32 = lambda *s: torch.full(s, -7, dtype=torch.int32, device="cuda")      # noqa: E731
    d_mask = torch.full((n, stride), 7, dtype=torch.uint8, device="cuda"); d_cnt = i32(n); d_Hm = torch.full((n, 9), 7.0, dtype=torch.float64, device="cuda")
    d_win = i32(n)
    torch.cuda.synchronize()
    ctx.verify_pairs_h_dev(d_corr, stride, d_counts, n, T2, d_mask, d_cnt, d_Hm, d_win, hypotheses=H, rounds=rounds, seed=seed, min_inliers=mi)
    ctx.synchronize()
    assert np.array_equal(d_mask.cpu().numpy(), refH[0]) and np.array_equal(d_cnt.cpu().numpy(), refH[1]) and np.array_equal(d_win.cpu().numpy(), refH[2])
    assert np.array_equal(_bits(d_Hm.cpu().numpy()), _bits(refH[3]))
    d_kind = i32(n); d_c2 = i32(n, 2); d_w2 = i32(n, 2); d_F = torch.full((n, 9), 7.0, dtype=torch.float64, device="cuda")
    d_mask.fill_(7); d_cnt.fill_(-7); d_Hm.fill_(7.0)
    keep = d_corr.clone()
    torch.cuda.synchronize()
    ctx.two_view_geometry_dev(d_corr, stride, d_counts, n, T1, T2, d_kind, d_mask, d_cnt, d_c2, d_F, d_Hm, d_w2, hypotheses=H, rounds=rounds, seed=seed,
                              min_inliers=mi, hf_ratio=ratio)
    ctx.synchronize()
    got = [a.cpu().numpy() for a in (d_kind, d_mask, d_cnt, d_c2, d_F, d_Hm, d_w2)]
    _same_g(got, refG, "device arrays")
    assert torch.equal(keep.view(torch.int64), d_corr.view(torch.int64))


def _rotation_match_scene():
    """_match_scene of test_twoview_gpu.py with image 2 replaced by a rotation-only view of image 1: the key points of image 2 that pair 1
    refers to are those of image 1 turned by homography_ref.ROTATION_ONLY, with 0.5 px noise and 30 % of them uniform"""
    kps, lists = _match_scene()
    kps = [k.copy() for k in kps]
    rng = np.random.default_rng(77)
    l = lists[1]
    a = kps[1][l["queryIdx"]]
    xn = np.column_stack([(a["x"].astype(np.float64) - tv.WIDTH / 2) / tv.FOCAL, (a["y"].astype(np.float64) - tv.HEIGHT / 2) / tv.FOCAL, np.ones(len(l))])
    Y = xn @ tv._rodrigues(hr.ROTATION_ONLY).T
    u2 = np.column_stack([tv.FOCAL * Y[:, 0] / Y[:, 2] + tv.WIDTH / 2, tv.FOCAL * Y[:, 1] / Y[:, 2] + tv.HEIGHT / 2]) + 0.5 * rng.standard_normal((len(l), 2))
    bad = rng.permutation(len(l))[:int(round(0.3 * len(l)))]
    u2[bad] = np.column_stack([rng.uniform(0, tv.WIDTH, len(bad)), rng.uniform(0, tv.HEIGHT, len(bad))])
    kps[2]["x"][l["trainIdx"]] = u2[:, 0].astype(np.float32); kps[2]["y"][l["trainIdx"]] = u2[:, 1].astype(np.float32)
    return kps, lists


def _gathered(kps, lists, K4, mpp):
    fx, fy, cx, cy = K4
    rows = []
    for q, l in enumerate(lists):
        a, b = kps[q][l["queryIdx"]], kps[q + 1][l["trainIdx"]]
        rows.append(np.column_stack([(a["x"].astype(np.float64) - cx) / fx, (a["y"].astype(np.float64) - cy) / fy,
                                     (b["x"].astype(np.float64) - cx) / fx, (b["y"].astype(np.float64) - cy) / fy]))
    return _blocks(rows, stride=mpp)


@pytest.mark.parametrize("K4", ((1.0, 1.0, 0.0, 0.0), (800.0, 790.0, 512.0, 384.0)))
def test_two_view_geometry_matches_dev(ctx, K4):
    import torch
    kps, lists = _cached("rotation match scene", _rotation_match_scene)
    mpp = 450
    matches = np.zeros((2, mpp), api.DMATCH); matches["queryIdx"] = -3; matches["trainIdx"] = 10 ** 6       # behind the counts: never read
    counts = np.array([len(l) for l in lists], np.int32)
    for q, l in enumerate(lists):
        matches[q, :len(l)] = l
    t = 1.0 if K4[0] == 1.0 else 1.0 / (0.5 * (K4[0] + K4[1]))
    blocks, _ = _gathered(kps, lists, K4, mpp)
    want = hr.two_view_geometry(blocks, counts, t, 2 * t, 256, 3, 2, 15, 0.8)
    assert want[0].tolist() == [1, 2] and want[2][0] > 200 and want[2][1] > 40, (want[0], want[3])
    _same_g(_raw_g(ctx, blocks, counts, t, 2 * t, 256, 3, 2, 15, 0.8), want, "gathered rows")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()      # noqa: E731
    d_kp = [dev(k) for k in kps]
    d_m, d_c = dev(matches), torch.from_numpy(counts).cuda()
    i32 = lambda *s: torch.full(s, -7, dtype=torch.int32, device="cuda")      # noqa: E731
    d_out = torch.full((2 * mpp * 16,), 0xEE, dtype=torch.uint8, device="cuda"); d_co = i32(2); d_kind = i32(2); d_c2 = i32(2, 2); d_w2 = i32(2, 2)
    d_F = torch.full((2, 9), 7.0, dtype=torch.float64, device="cuda"); d_Hm = torch.full((2, 9), 7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ctx.two_view_geometry_matches_dev(d_kp, [[0, 1], [1, 2]], K4, d_m, mpp, d_c, t, 2 * t, d_kind, d_out, d_co, d_c2, d_F, d_Hm, d_w2, hypotheses=256,
                                      rounds=3, seed=2, min_inliers=15, hf_ratio=0.8)
    ctx.synchronize()
    out = d_out.cpu().numpy().view(api.DMATCH).reshape(2, mpp)
    assert np.array_equal(d_kind.cpu().numpy(), want[0]) and np.array_equal(d_co.cpu().numpy(), want[2]) and np.array_equal(d_c2.cpu().numpy(), want[3])
    assert np.array_equal(d_w2.cpu().numpy(), want[6])
    assert np.array_equal(_bits(d_F.cpu().numpy()), _bits(want[4])) and np.array_equal(_bits(d_Hm.cpu().numpy()), _bits(want[5]))
    for q, l in enumerate(lists):
        keep = want[1][q, :len(l)].astype(bool)
        assert out[q, :want[2][q]].tobytes() == l[keep].tobytes()                                    # the ordered subsequence the selected mask chooses
        assert (out[q, want[2][q]:].view(np.uint8) == 0xEE).all()                                    # nothing written behind it
    assert d_m.cpu().numpy().tobytes() == matches.tobytes()
    for k, d in zip(kps, d_kp):
        assert d.cpu().numpy().tobytes() == k.tobytes()
    # the optional outputs: the others are the same without them
    d_out2 = torch.full((2 * mpp * 16,), 0xEE, dtype=torch.uint8, device="cuda"); d_co2 = i32(2); d_kind2 = i32(2)
    torch.cuda.synchronize()
    ctx.two_view_geometry_matches_dev(d_kp, [[0, 1], [1, 2]], K4, d_m, mpp, d_c, t, 2 * t, d_kind2, d_out2, d_co2, hypotheses=256, rounds=3, seed=2,
                                      min_inliers=15, hf_ratio=0.8)
    ctx.synchronize()
    assert torch.equal(d_out, d_out2) and torch.equal(d_co, d_co2) and torch.equal(d_kind, d_kind2)


def test_two_view_geometry_for_all(ctx):
    kps, lists = _cached("rotation match scene", _rotation_match_scene)
    K = np.array([[800.0, 0, 512], [0, 800.0, 384], [0, 0, 1]])
    out, info = api.two_view_geometry_for_all(K, kps, lists, px=1.0, px_h=2.0, hypotheses=256, seed=2, ctx=ctx)
    blocks, counts = _gathered(kps, lists, (800.0, 800.0, 512.0, 384.0), 400)
    want = hr.two_view_geometry(blocks, counts, T1, T2, 256, 3, 2, 15, 0.8)
    assert [i[0] for i in info] == want[0].tolist() == [1, 2]
    for q, l in enumerate(lists):
        kind, cnt, cF, cH, F, Hm = info[q]
        assert (cnt, cF, cH) == (want[2][q], want[3][q, 0], want[3][q, 1]) and out[q].tobytes() == l[want[1][q, :len(l)].astype(bool)].tobytes()
        assert np.array_equal(_bits(F.reshape(9)), _bits(want[4][q])) and np.array_equal(_bits(Hm.reshape(9)), _bits(want[5][q]))
    # a pair of kind 0 keeps its matches
    out, info = api.two_view_geometry_for_all(K, kps, lists, px=1.0, px_h=2.0, hypotheses=256, seed=2, min_inliers=100, ctx=ctx)
    assert info[1][:4] == (0, 0, 0, 0) and out[1].tobytes() == lists[1].tobytes() and info[0][0] == 1 and len(out[0]) == info[0][1] > 100


# ---- errors ------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_leave_the_outputs_alone(ctx):
    lib, h = ctx.lib, ctx.h
    rows = hr.scene_rows("planar", 100, seed=3)
    blocks, counts = _blocks([rows, rows[:50]])
    mask = np.full((2, 100), 7, np.uint8); cnt = np.full(2, -7, np.int32); F = np.full((2, 9), 7.0); Hm = np.full((2, 9), 7.0); win = np.full((2, 2), -7, np.int32)
    kind = np.full(2, -7, np.int32); c2 = np.full((2, 2), -7, np.int32)
    b, c, M, n_, F_, H_, w, k_, c2_ = (a.ctypes.data for a in (blocks, counts, mask, cnt, F, Hm, win, kind, c2))
    pairs = np.array([[0, 1], [1, 2]], np.int32); K4 = np.array([1.0, 1.0, 0.0, 0.0]); kp = (C.c_void_p * 3)(b, b, b)
    # the homography call: t, H, rounds, min_inliers (>= 4), stride, n_pairs
    for t, H, rounds, mi, stride, n in ((-1.0, 64, 3, 4, 100, 2), (np.nan, 64, 3, 4, 100, 2), (np.inf, 64, 3, 4, 100, 2), (0.1, 0, 3, 4, 100, 2),
                                        (0.1, 65537, 3, 4, 100, 2), (0.1, 64, 0, 4, 100, 2), (0.1, 64, 9, 4, 100, 2), (0.1, 64, 3, 3, 100, 2),
                                        (0.1, 64, 3, 4, -1, 2), (0.1, 64, 3, 4, 100, -1)):
        what = (t, H, rounds, mi, stride, n)
        assert lib.sfmhip_verify_pairs_h(h, b, stride, c, n, t, H, rounds, 1, mi, M, n_, H_, w) == _lib.E_ARG, what
        assert lib.sfmhip_verify_pairs_h_dev(h, b, stride, c, n, t, H, rounds, 1, mi, M, n_, H_, w) == _lib.E_ARG, what
    # the combined calls: t_f, t_h, H, rounds, min_inliers (>= 8), hf_ratio, stride, n_pairs
    ok = dict(tf=0.1, th=0.2, H=64, rounds=3, mi=8, ratio=0.8, stride=100, n=2)
    for bad in (dict(tf=-1.0), dict(tf=np.nan), dict(tf=np.inf), dict(th=-1.0), dict(th=np.nan), dict(th=np.inf), dict(H=0), dict(H=65537), dict(rounds=0),
                dict(rounds=9), dict(mi=7), dict(ratio=0.0), dict(ratio=-0.5), dict(ratio=np.nan), dict(ratio=np.inf), dict(stride=-1), dict(n=-1)):
        a = dict(ok, **bad)
        head = (a["tf"], a["th"], a["H"], a["rounds"], 1, a["mi"], a["ratio"])
        assert lib.sfmhip_two_view_geometry(h, b, a["stride"], c, a["n"], *head, k_, M, n_, c2_, F_, H_, w) == _lib.E_ARG, bad
        assert lib.sfmhip_two_view_geometry_dev(h, b, a["stride"], c, a["n"], *head, k_, M, n_, c2_, F_, H_, w) == _lib.E_ARG, bad
        assert lib.sfmhip_two_view_geometry_matches_dev(h, kp, 3, pairs.ctypes.data, a["n"], K4.ctypes.data, b, a["stride"], c, *head, k_, b, n_, c2_, F_, H_,
                                                        w) == _lib.E_ARG, bad
    # NULL with n_pairs > 0
    for args in ((None, 100, c, 2, 0.1, 64, 3, 1, 4, M, n_, H_, w), (b, 100, None, 2, 0.1, 64, 3, 1, 4, M, n_, H_, w),
                 (b, 100, c, 2, 0.1, 64, 3, 1, 4, None, n_, H_, w), (b, 100, c, 2, 0.1, 64, 3, 1, 4, M, None, H_, w)):
        assert lib.sfmhip_verify_pairs_h(h, *args) == _lib.E_ARG
        assert lib.sfmhip_verify_pairs_h_dev(h, *args) == _lib.E_ARG
    g = (0.1, 0.2, 64, 3, 1, 8, 0.8)
    for args in ((None, 100, c, 2, *g, k_, M, n_), (b, 100, None, 2, *g, k_, M, n_), (b, 100, c, 2, *g, None, M, n_), (b, 100, c, 2, *g, k_, None, n_),
                 (b, 100, c, 2, *g, k_, M, None)):
        assert lib.sfmhip_two_view_geometry(h, *args, c2_, F_, H_, w) == _lib.E_ARG
        assert lib.sfmhip_two_view_geometry_dev(h, *args, c2_, F_, H_, w) == _lib.E_ARG
    # the match-list form: a pair that names an image that is not there; a K without a focal length; no key points; no kind
    wrong = np.array([[0, 1], [1, 3]], np.int32); K0 = np.array([0.0, 1.0, 0.0, 0.0])
    tail = (b, 100, c, *g)
    assert lib.sfmhip_two_view_geometry_matches_dev(h, kp, 3, wrong.ctypes.data, 2, K4.ctypes.data, *tail, k_, b, n_, c2_, F_, H_, w) == _lib.E_ARG
    assert lib.sfmhip_two_view_geometry_matches_dev(h, kp, 3, pairs.ctypes.data, 2, K0.ctypes.data, *tail, k_, b, n_, c2_, F_, H_, w) == _lib.E_ARG
    assert lib.sfmhip_two_view_geometry_matches_dev(h, None, 3, pairs.ctypes.data, 2, K4.ctypes.data, *tail, k_, b, n_, c2_, F_, H_, w) == _lib.E_ARG
    assert lib.sfmhip_two_view_geometry_matches_dev(h, kp, 3, pairs.ctypes.data, 2, K4.ctypes.data, *tail, None, b, n_, c2_, F_, H_, w) == _lib.E_ARG
    for a in (mask, F, Hm):
        assert (a == 7).all()
    for a in (cnt, win, kind, c2):
        assert (a == -7).all()
    # n_pairs == 0: OK, no pointer touched
    assert lib.sfmhip_verify_pairs_h(h, None, 100, None, 0, 0.1, 64, 3, 1, 4, None, None, None, None) == 0
    assert lib.sfmhip_verify_pairs_h_dev(h, None, 100, None, 0, 0.1, 64, 3, 1, 4, None, None, None, None) == 0
    assert lib.sfmhip_two_view_geometry(h, None, 100, None, 0, *g, None, None, None, None, None, None, None) == 0
    assert lib.sfmhip_two_view_geometry_dev(h, None, 100, None, 0, *g, None, None, None, None, None, None, None) == 0
    assert lib.sfmhip_two_view_geometry_matches_dev(h, None, 0, None, 0, None, None, 100, None, *g, None, None, None, None, None, None, None) == 0
    with pytest.raises(api.SfmHipError):
        ctx.verify_pairs_h([rows], -0.5)
    with pytest.raises(api.SfmHipError):
        ctx.two_view_geometry([rows], 0.1, 0.2, hf_ratio=0.0)


def test_a_failed_allocation_is_an_error_and_the_next_call_works(ctx):
    rows = _cached(("rows", 300), lambda: hr.scene_rows("rotation", 300, out=0.3, seed=3))
    blocks, counts = _blocks([rows])
    mask = np.empty((1, 300), np.uint8); cnt = np.empty(1, np.int32); kind = np.empty(1, np.int32)
    for failing in (1, 2):
        assert ctx.lib.sfmhip_debug_fail_allocations(ctx.h, failing) == 0
        for _ in range(failing):
            rc = ctx.lib.sfmhip_verify_pairs_h(ctx.h, blocks.ctypes.data, 300, counts.ctypes.data, 1, T2, 256, 3, 5, 4, mask.ctypes.data, cnt.ctypes.data, None, None)
            assert rc == _lib.E_HIP
        _check_h(ctx, blocks, counts, T2, 256, 3, 5, 4, tag="after a failed allocation")
        assert ctx.lib.sfmhip_debug_fail_allocations(ctx.h, failing) == 0
        for _ in range(failing):
            rc = ctx.lib.sfmhip_two_view_geometry(ctx.h, blocks.ctypes.data, 300, counts.ctypes.data, 1, T1, T2, 256, 3, 5, 8, 0.8, kind.ctypes.data, mask.ctypes.data,
                                                  cnt.ctypes.data, None, None, None, None)
            assert rc == _lib.E_HIP
        _same_g(_raw_g(ctx, blocks, counts, T1, T2, 256, 3, 5, 8, 0.8), hr.two_view_geometry(blocks, counts, T1, T2, 256, 3, 5, 8, 0.8), "after a failed allocation")


# ---- driver ------------------------------------------------------------------------------------------------------------------------
def _geometry_lines(log):
    return [(int(a), b, int(c), int(d), int(e), int(f)) for a, b, c, d, e, f in
            re.findall(r"^pair (\d+): geometry (general|planar-or-panoramic|none), kept (\d+) of (\d+) \(F (\d+), H (\d+)\)$", log, re.M)]


def test_driver_two_view_geometry_option(tmp_path):
    subprocess.check_call(["make", "-C", HOST], stdout=subprocess.DEVNULL)
    exe = os.path.join(HOST, "NViewReconstruct")
    out = subprocess.run([exe, os.path.join(GOLD, "crazyhorse_features.bin"), str(tmp_path), "--quiet", "--two-view-geometry"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    lines = _geometry_lines(out.stdout)
    print(f"[homography] crazyhorse: {lines}")
    assert [l[0] for l in lines] == list(range(6)) and all(0 <= k <= m for _, _, k, m, _, _ in lines)
    assert out.stdout.count("its two-view pose is ill-determined") == sum(l[1] == "planar-or-panoramic" for l in lines)
    for f in ("structure.yml", "structure_ba.yml", "structure_ba.ply"):
        assert (tmp_path / f).stat().st_size > 0, f
    assert "Save structure done." in out.stdout
    # both options at once: an error
    both = subprocess.run([exe, os.path.join(GOLD, "crazyhorse_features.bin"), str(tmp_path), "--quiet", "--two-view-geometry", "--verify-matches"],
                          capture_output=True, text=True)
    assert both.returncode != 0 and "exclude each other" in both.stdout
    # the synthetic scene of test_drivers_gpu.py: every pair is general, and the flag does not cost accuracy
    from test_drivers_gpu import _scene
    K, Rs, Ts, descs, kps, cols, X = _scene()
    feat = tmp_path / "features.bin"
    features_io.write_features(feat, K, kps, descs, cols, poses=list(zip(Rs, Ts)))
    rmse = []
    for flags in ([], ["--two-view-geometry=1.0,2.0,1024,3,0.8"]):
        d = tmp_path / ("with" if flags else "without"); d.mkdir()
        o = subprocess.run([exe, str(feat), str(d), "--poses-from-file", "--quiet"] + flags, capture_output=True, text=True)
        assert o.returncode == 0, o.stdout[-2000:] + o.stderr[-2000:]
        rmse.append(float(re.search(r"Final   RMSE\(pixel\): ([0-9.eE+-]+)", o.stdout).group(1)))
        got = _geometry_lines(o.stdout)
        assert len(got) == (4 if flags else 0) and all(kind == "general" and 15 <= k <= m and k == cf for _, kind, k, m, cf, _ in got), got
    print(f"[homography] synthetic scene: final RMSE {rmse[0]} without, {rmse[1]} with --two-view-geometry")
    assert rmse[1] <= 1.05 * rmse[0]
