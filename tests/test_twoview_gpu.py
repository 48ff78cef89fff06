"""GPU: two-view geometric verification (sfmhip_verify_pairs, sfmhip_verify_pairs_dev, sfmhip_verify_matches_dev) through the C-ABI, the
Python layer and the NViewReconstruct driver.  The reference is tests/twoview_ref.py, a numpy restatement of the definition in
include/sfmhip.h.  In every comparison with it mask, count and winner must be EQUAL and F equal in every bit (compared as uint64 views,
the NaN rows of the pairs without a model included)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import twoview_ref as tv
from sfm_opencv_amd import _lib, api, features_io

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
HOST = os.path.join(os.path.dirname(HERE), "sfm_opencv_amd", "host")
CHUNK = 512                  # twoview.hip: rows staged in LDS per pass of twoview_score_kernel
T1 = 1.0 / tv.FOCAL          # one pixel on normalised coordinates
_cache = {}


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _blocks(rows_list, stride=None, fill=0.0):
    """(blocks n x stride x 4, counts): the rows of every pair at the start of its block, `fill` behind them"""
    counts = np.array([len(r) for r in rows_list], np.int32)
    stride = max(1, int(counts.max()) if len(counts) else 1) if stride is None else stride
    blocks = np.full((len(rows_list), stride, 4), fill)
    for q, r in enumerate(rows_list):
        blocks[q, :len(r)] = r
    return blocks, counts


def _raw(ctx, blocks, counts, t, H, rounds, seed, min_inliers, want_F=True):
    """the C-ABI's own arrays: (mask n x stride, count, winner, F n x 9), pre-filled with values the call never writes"""
    blocks = np.ascontiguousarray(blocks, np.float64); counts = np.ascontiguousarray(counts, np.int32)
    n, stride = blocks.shape[0], blocks.shape[1]
    mask = np.full((n, stride), 7, np.uint8); cnt = np.full(n, -7, np.int32); win = np.full(n, -7, np.int32); F = np.full((n, 9), 7.0)
    rc = ctx.lib.sfmhip_verify_pairs(ctx.h, blocks.ctypes.data, stride, counts.ctypes.data, n, t, H, rounds, seed, min_inliers, mask.ctypes.data,
                                     cnt.ctypes.data, F.ctypes.data if want_F else None, win.ctypes.data if want_F else None)
    assert rc == 0, ctx.lib.sfmhip_last_error(ctx.h)
    return mask, cnt, win, F


def _check(ctx, blocks, counts, t, H, rounds, seed, min_inliers, ref=None, tag=None):
    """the library against the restatement on every output; returns the library's"""
    if ref is None:
        ref = tv.verify_pairs(blocks, counts, t, H, rounds, seed, min_inliers)
    got = _raw(ctx, blocks, counts, t, H, rounds, seed, min_inliers)
    what = (tag, t, H, rounds, seed, min_inliers)
    assert np.array_equal(got[1], ref[1]) and got[1].dtype == np.int32, (what, got[1], ref[1], got[2], ref[2])
    assert np.array_equal(got[2], ref[2]), (what, got[2], ref[2])
    bad = np.argwhere(got[0] != ref[0])
    assert len(bad) == 0, (what, len(bad), bad[:5])
    assert np.array_equal(_bits(got[3]), _bits(ref[3])), (what, got[3], ref[3])
    assert np.array_equal(got[0].sum(axis=1), got[1])
    return got


# ---- one pair: list lengths around the chunk of the scoring kernel, hypothesis-block edges, the number of rounds -----------------------
@pytest.mark.parametrize("H", (1, 65, 256, 257, 1024))
def test_single_pair_equals_the_reference(ctx, H):
    for m in (0, 7, 8, 9, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3):
        rows = _cached(("rows", m), lambda: tv.scene_rows(m, out=0.3, seed=10 + m))
        blocks, counts = _blocks([rows])
        for rounds in (1, 3, 8):
            got = _check(ctx, blocks, counts, T1, H, rounds, 77, 8, tag=f"m={m}")
            print(f"[twoview] m = {m}, H = {H}, rounds = {rounds}: count {got[1][0]}, winner {got[2][0]}")
            if m < 8:
                assert got[1][0] == 0 and got[2][0] == -1 and np.isnan(got[3]).all() and not got[0].any()
            elif H >= 256 and m >= CHUNK - 1:
                assert got[1][0] >= 0.5 * m                           # 70 % of the rows are true matches


def _subset(H, n=512):
    """n fixed values of h in ascending order, the edges of the first two hypothesis blocks and the last h among them"""
    must = [0, 255, 256, H - 1]
    rest = [int(h) for h in np.random.default_rng(1).permutation(H)[:n] if h not in must][:n - len(must)]
    return np.array(sorted(must + rest))


def _check_winner_in_parts(got, sub, models, valid, cnt, inl):
    """one pair, one round: the library's outputs against the restatement's models / valid bits / counts of the hypotheses sub (ascending,
    the library's winner among them) and the winner's reference inliers inl"""
    win = int(got[2][0])
    k = int(np.searchsorted(sub, win))
    assert sub[k] == win and valid[k]
    assert np.array_equal(_bits(got[3][0]), _bits(models[k]))
    assert np.array_equal(got[0][0], inl.astype(np.uint8))
    assert got[1][0] == got[0][0].sum() and got[1][0] == cnt[k]
    print(f"winner {win}, count {cnt[k]}; {int(valid.sum())} of {len(sub)} reference hypotheses valid, largest other count {np.delete(cnt, k).max()}")
    assert (cnt[valid] <= cnt[k]).all()
    assert (sub[valid & (cnt == cnt[k])] >= win).all()                   # a count equal to the winner's only at a larger h


def test_a_workgroup_that_strides_over_several_chunks(ctx):
    # H = 65536 is 256 blocks of 256 hypotheses, which leaves SCORE_MAX_WG / 256 = 8 workgroups along the rows: 8 * CHUNK rows are one
    # chunk each, the 11 chunks of this list make the first three workgroups take two (the last one partial).  The restatement over all
    # H hypotheses takes half a minute here, so it is applied in parts: the samples of all H (integer work), the hypotheses and counts
    # of 512 fixed values of h and of the library's winner.
    H, m, seed = 65536, 8 * CHUNK + 2 * CHUNK + 7, 21
    rows = tv.scene_rows(m, out=0.3, seed=12)
    got = _raw(ctx, *_blocks([rows]), T1, H, 1, seed, 8)
    pos = tv.samples(seed, 0, H, m)
    srt = np.sort(pos, axis=1)
    assert pos.min() >= 0 and pos.max() < m and (srt[:, 1:] > srt[:, :-1]).all()
    assert 0 <= got[2][0] < H
    sub = np.union1d(_subset(H), [got[2][0]])
    F, valid = tv.null_vectors(tv.design(rows[pos[sub]]))
    cnt = tv.counts_of(F, valid, rows, T1 * T1)
    _check_winner_in_parts(got, sub, F, valid, cnt, tv.inliers(got[3][0], rows, T1 * T1)[0])
    assert got[1][0] >= 0.5 * m


def test_rows_behind_the_count_are_never_read(ctx):
    rows = _cached(("rows", 300), lambda: tv.scene_rows(300, out=0.3, seed=3))
    ref = tv.verify_pairs(*_blocks([rows]), T1, 256, 3, 5, 8)
    for fill in (7.0, np.nan):
        blocks, counts = _blocks([rows], stride=300 + 77, fill=fill)
        got = _check(ctx, blocks, counts, T1, 256, 3, 5, 8, tag=f"fill={fill}")
        assert not got[0][:, 300:].any() and np.array_equal(got[0][:, :300], ref[0]) and np.array_equal(_bits(got[3]), _bits(ref[3]))
    assert ref[1][0] > 150


def test_non_finite_rows_are_never_sampled_and_never_inliers(ctx):
    rows = tv.scene_rows(700, out=0.3, seed=4).copy()
    rows[::37] = np.nan
    rows[5, 2] = np.inf
    rows[6, 1] = -np.inf
    blocks, counts = _blocks([rows])
    got = _check(ctx, blocks, counts, T1, 256, 3, 1, 8, tag="non-finite")
    assert got[1][0] > 300 and not got[0][0, ::37].any() and not got[0][0, 5] and not got[0][0, 6]
    finite = rows[np.isfinite(rows).all(axis=1)]
    alone = _raw(ctx, *_blocks([finite]), T1, 256, 3, 1, 8)
    assert alone[1][0] == got[1][0] and alone[2][0] == got[2][0] and np.array_equal(_bits(alone[3]), _bits(got[3]))      # the same L_0


def test_duplicate_rows(ctx):
    base = tv.scene_rows(40, out=0.0, seed=6)
    eight = base[:8].copy(); eight[5] = eight[2]
    got = _check(ctx, *_blocks([eight]), T1, 64, 3, 2, 8, tag="dup8")
    assert got[1][0] == 0 and got[2][0] == -1 and np.isnan(got[3]).all() and not got[0].any()      # every hypothesis: an exact zero pivot
    nine = base[:9].copy(); nine[5] = nine[2]
    got = _check(ctx, *_blocks([nine]), T1, 64, 3, 2, 8, tag="dup9")
    assert got[1][0] >= 8 and got[0][0, 2] == got[0][0, 5]


def test_ties_go_to_the_smallest_h_and_round_1_stops(ctx):
    rows = tv.scene_rows(200, out=0.3, seed=8)
    rows = np.concatenate([rows[:3], rows[:3], rows[3:]])           # duplicates: some hypotheses are invalid
    det = []
    ref1 = tv.verify_pair(rows, len(rows), 1e6, 257, 3, 4, 8, det)
    F, valid = tv.hypotheses(rows, 4, 0, 257)
    first = int(np.flatnonzero(valid)[0])
    assert det == [(0, first, len(rows), False), (1, det[1][1], len(rows), True)] and not valid.all()
    got = _check(ctx, *_blocks([rows]), 1e6, 257, 3, 4, 8, tag="ties")
    assert got[1][0] == len(rows) and got[2][0] == first and got[0].all()


def test_threshold_zero(ctx):
    rows = tv.scene_rows(300, out=0.3, seed=9)
    _check(ctx, *_blocks([rows]), 0.0, 256, 3, 1, 8, tag="t=0")
    # integer rows with y2 = y1 and x2 = x1 + 1 or 2: F = [0 0 0; 0 0 -1; 0 1 0] / sqrt 2 satisfies them all with e = 0 exactly
    g = np.stack(np.meshgrid(np.arange(6.0), np.arange(5.0), indexing="ij"), -1).reshape(-1, 2)
    lat = np.column_stack([g, g[:, 0] + 1 + (g[:, 1] % 2), g[:, 1]])
    got = _check(ctx, *_blocks([lat]), 0.0, 256, 2, 3, 8, tag="t=0 lattice")
    print(f"[twoview] t = 0 on the lattice: count {got[1][0]}, winner {got[2][0]}")


def _batch():
    sizes = (0, 5, 8, 300, 7, 2000, 64, 513, 9, 1100, 40, 150)
    rows = [tv.scene_rows(m, out=(0.3, 0.5, 0.1)[k % 3], seed=20 + k, pure_translation=bool(k & 1)) for k, m in enumerate(sizes)]
    blocks, counts = _blocks(rows, stride=2000, fill=np.nan)
    return blocks, counts, tv.verify_pairs(blocks, counts, T1, 256, 4, 11, 8)


def test_a_batch_equals_its_pairs_alone(ctx):
    blocks, counts, ref = _cached("batch", _batch)
    rounds_of = ref[2] // 256
    assert len(set(rounds_of[ref[2] >= 0].tolist())) >= 2, rounds_of           # the models come from different rounds
    got = _check(ctx, blocks, counts, T1, 256, 4, 11, 8, ref=ref, tag="batch")
    again = _raw(ctx, blocks, counts, T1, 256, 4, 11, 8)
    for a, b in zip(got, again):
        assert a.tobytes() == b.tobytes()
    for q in (2, 3, 5, 7):                                                      # alone, in a block of its own length
        one = _raw(ctx, blocks[q:q + 1, :max(1, counts[q])], counts[q:q + 1], T1, 256, 4, 11, 8)
        assert np.array_equal(one[0][0], got[0][q, :max(1, counts[q])]) and one[1][0] == got[1][q] and one[2][0] == got[2][q]
        assert np.array_equal(_bits(one[3][0]), _bits(got[3][q]))
    # F and winner are optional
    part = _raw(ctx, blocks, counts, T1, 256, 4, 11, 8, want_F=False)
    assert part[0].tobytes() == got[0].tobytes() and part[1].tobytes() == got[1].tobytes() and (part[2] == -7).all() and (part[3] == 7).all()


def test_a_batch_longer_than_one_launch(ctx):
    # twoview.hip enqueues a batch in slices of 32768 pairs (the pairs are the z dimension of the scoring grid): pairs at the end of the
    # first slice and in the second, everything else empty
    n, stride = 32768 + 5, 16
    blocks = np.full((n, stride, 4), np.nan); counts = np.zeros(n, np.int32)
    live = (0, 32767, 32768, n - 1)
    for k, q in enumerate(live):
        rows = tv.scene_rows(12 + k, out=0.0, seed=60 + k)
        blocks[q, :len(rows)] = rows; counts[q] = len(rows)
    got = _raw(ctx, blocks, counts, T1, 64, 2, 3, 8)
    for q in live:
        mask, cnt, win, F = tv.verify_pair(blocks[q], int(counts[q]), T1, 64, 2, 3, 8)
        assert cnt >= 8 and got[1][q] == cnt and got[2][q] == win and np.array_equal(got[0][q], mask) and np.array_equal(_bits(got[3][q]), _bits(F)), q
    rest = np.ones(n, bool); rest[list(live)] = False
    assert not got[0][rest].any() and not got[1][rest].any() and (got[2][rest] == -1).all() and np.isnan(got[3][rest]).all()


def test_min_inliers_around_a_pairs_count(ctx):
    rows = _cached(("rows", 300), lambda: tv.scene_rows(300, out=0.3, seed=3))
    blocks, counts = _blocks([rows])
    c = int(_check(ctx, blocks, counts, T1, 256, 3, 5, 8)[1][0])
    assert c > 150
    got = _check(ctx, blocks, counts, T1, 256, 3, 5, c, tag="min_inliers = count")
    assert got[1][0] == c
    got = _check(ctx, blocks, counts, T1, 256, 3, 5, c + 1, tag="min_inliers = count + 1")
    assert got[1][0] == 0 and got[2][0] == -1 and np.isnan(got[3]).all() and not got[0].any()


# ---- the Python layer and the device entry points --------------------------------------------------------------------------------------
def test_python_layer_and_device_arrays(ctx):
    import torch
    blocks, counts, ref = _cached("batch", _batch)
    masks, cnt, F, win = ctx.verify_pairs([blocks[q, :counts[q]] for q in range(len(counts))], T1, hypotheses=256, rounds=4, seed=11)
    assert np.array_equal(cnt, ref[1]) and np.array_equal(win, ref[2]) and np.array_equal(_bits(F.reshape(-1, 9)), _bits(ref[3]))
    for q, m in enumerate(masks):
        assert m.dtype == bool and np.array_equal(m, ref[0][q, :counts[q]].astype(bool))
    n, stride = blocks.shape[:2]
    d_corr = torch.from_numpy(blocks).cuda(); d_counts = torch.from_numpy(counts).cuda()
    d_mask = torch.full((n, stride), 7, dtype=torch.uint8, device="cuda"); d_cnt = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    d_F = torch.full((n, 9), 7.0, dtype=torch.float64, device="cuda"); d_win = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.verify_pairs_dev(d_corr, stride, d_counts, n, T1, d_mask, d_cnt, d_F, d_win, hypotheses=256, rounds=4, seed=11)
    ctx.synchronize()
    assert np.array_equal(d_mask.cpu().numpy(), ref[0]) and np.array_equal(d_cnt.cpu().numpy(), ref[1]) and np.array_equal(d_win.cpu().numpy(), ref[2])
    assert np.array_equal(_bits(d_F.cpu().numpy()), _bits(ref[3]))


def _match_scene():
    """three images, two pairs: key points (with some no match refers to) and match lists as sfmhip_match_pairs_dev leaves them"""
    rng = np.random.default_rng(31)
    kps, lists = [np.zeros(0, api.KEYPOINT)] * 3, []
    n_kp = (700, 900, 650)
    kps = [np.zeros(k, api.KEYPOINT) for k in n_kp]
    for k in kps:
        k["x"] = rng.uniform(0, 1024, len(k)).astype(np.float32); k["y"] = rng.uniform(0, 768, len(k)).astype(np.float32)
    for q, m in enumerate((400, 90)):
        pix, _ = tv.two_view_scene(m, 0.3, 40 + q)
        qi = np.sort(rng.permutation(n_kp[q])[:m]); ti = rng.permutation(n_kp[q + 1])[:m]
        kps[q]["x"][qi] = pix[:, 0]; kps[q]["y"][qi] = pix[:, 1]
        if q == 1:                                                     # image 1 is the train image of pair 0: keep what pair 0 put there
            free = np.setdiff1d(np.arange(n_kp[1]), lists[0]["trainIdx"])
            qi = np.sort(rng.permutation(free)[:m])
            kps[1]["x"][qi] = pix[:, 0]; kps[1]["y"][qi] = pix[:, 1]
        kps[q + 1]["x"][ti] = pix[:, 2]; kps[q + 1]["y"][ti] = pix[:, 3]
        lst = np.zeros(m, api.DMATCH)
        lst["queryIdx"] = qi; lst["trainIdx"] = ti; lst["imgIdx"] = 0; lst["distance"] = rng.uniform(10, 200, m).astype(np.float32)
        lists.append(lst)
    return kps, lists


@pytest.mark.parametrize("K4", ((1.0, 1.0, 0.0, 0.0), (800.0, 790.0, 512.0, 384.0)))
def test_verify_matches_dev(ctx, K4):
    import torch
    kps, lists = _cached("match scene", _match_scene)
    mpp = 450
    matches = np.zeros((2, mpp), api.DMATCH); matches["queryIdx"] = -3; matches["trainIdx"] = 10 ** 6       # behind the counts: never read
    counts = np.array([len(l) for l in lists], np.int32)
    for q, l in enumerate(lists):
        matches[q, :len(l)] = l
    fx, fy, cx, cy = K4
    t = 1.0 if fx == 1.0 else 1.0 / (0.5 * (fx + fy))
    rows = []
    for q, l in enumerate(lists):
        a, b = kps[q][l["queryIdx"]], kps[q + 1][l["trainIdx"]]
        rows.append(np.column_stack([(a["x"].astype(np.float64) - cx) / fx, (a["y"].astype(np.float64) - cy) / fy,
                                     (b["x"].astype(np.float64) - cx) / fx, (b["y"].astype(np.float64) - cy) / fy]))
    blocks, _ = _blocks(rows, stride=mpp)
    want = _check(ctx, blocks, counts, t, 256, 3, 2, 15, tag=f"gathered rows {K4}")      # sfmhip_verify_pairs on the gathered rows (and the restatement)
    assert want[1][0] > 200 and want[1][1] > 40
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()      # noqa: E731
    d_kp = [dev(k) for k in kps]
    d_m, d_c = dev(matches), torch.from_numpy(counts).cuda()
    d_out = torch.full((2 * mpp * 16,), 0xEE, dtype=torch.uint8, device="cuda"); d_co = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    d_F = torch.full((2, 9), 7.0, dtype=torch.float64, device="cuda"); d_w = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.verify_matches_dev(d_kp, [[0, 1], [1, 2]], K4, d_m, mpp, d_c, t, d_out, d_co, d_F, d_w, hypotheses=256, rounds=3, seed=2, min_inliers=15)
    ctx.synchronize()
    out = d_out.cpu().numpy().view(api.DMATCH).reshape(2, mpp)
    assert np.array_equal(d_co.cpu().numpy(), want[1]) and np.array_equal(d_w.cpu().numpy(), want[2])
    assert np.array_equal(_bits(d_F.cpu().numpy()), _bits(want[3]))
    for q, l in enumerate(lists):
        keep = want[0][q, :len(l)].astype(bool)
        assert out[q, :want[1][q]].tobytes() == l[keep].tobytes()                                    # the ordered subsequence the mask selects
        assert (out[q, want[1][q]:].view(np.uint8) == 0xEE).all()                                    # nothing written behind it
    assert d_m.cpu().numpy().tobytes() == matches.tobytes()


def test_verify_matches_for_all(ctx):
    kps, lists = _cached("match scene", _match_scene)
    K = np.array([[800.0, 0, 512], [0, 800.0, 384], [0, 0, 1]])
    out, info = api.verify_matches_for_all(K, kps, lists, px=1.0, hypotheses=256, seed=2, ctx=ctx)
    assert len(out) == 2 and [len(o) for o in out] == [c for c, _ in info] and all(c >= 15 for c, _ in info)
    rows = [tv.normalised(np.column_stack([kps[q]["x"][l["queryIdx"]], kps[q]["y"][l["queryIdx"]], kps[q + 1]["x"][l["trainIdx"]],
                                           kps[q + 1]["y"][l["trainIdx"]]])) for q, l in enumerate(lists)]
    for q, l in enumerate(lists):
        mask, cnt, win, F = tv.verify_pair(rows[q], len(l), 1.0 / 800, 256, 3, 2, 15)
        assert cnt == info[q][0] and out[q].tobytes() == l[mask.astype(bool)].tobytes() and np.array_equal(_bits(info[q][1].reshape(9)), _bits(F))
    # a pair without a model keeps its matches
    out, info = api.verify_matches_for_all(K, kps, lists, px=1.0, hypotheses=256, seed=2, min_inliers=100, ctx=ctx)
    assert info[1][0] == 0 and np.isnan(info[1][1]).all() and out[1].tobytes() == lists[1].tobytes() and len(out[0]) == info[0][0] > 100


# ---- errors ------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_leave_the_outputs_alone(ctx):
    lib, h = ctx.lib, ctx.h
    rows = tv.scene_rows(100, seed=3)
    blocks, counts = _blocks([rows, rows[:50]])
    mask = np.full((2, 100), 7, np.uint8); cnt = np.full(2, -7, np.int32); F = np.full((2, 9), 7.0); win = np.full(2, -7, np.int32)
    b, c, M, n_, F_, w = (a.ctypes.data for a in (blocks, counts, mask, cnt, F, win))
    pairs = np.array([[0, 1], [1, 2]], np.int32); K4 = np.array([1.0, 1.0, 0.0, 0.0]); kp = (C.c_void_p * 3)(b, b, b)
    for t, H, rounds, mi, stride, n in ((-1.0, 64, 3, 8, 100, 2), (np.nan, 64, 3, 8, 100, 2), (np.inf, 64, 3, 8, 100, 2), (0.1, 0, 3, 8, 100, 2),
                                        (0.1, 65537, 3, 8, 100, 2), (0.1, 64, 0, 8, 100, 2), (0.1, 64, 9, 8, 100, 2), (0.1, 64, 3, 7, 100, 2),
                                        (0.1, 64, 3, 8, -1, 2), (0.1, 64, 3, 8, 100, -1)):
        what = (t, H, rounds, mi, stride, n)
        assert lib.sfmhip_verify_pairs(h, b, stride, c, n, t, H, rounds, 1, mi, M, n_, F_, w) == _lib.E_ARG, what
        assert lib.sfmhip_verify_pairs_dev(h, b, stride, c, n, t, H, rounds, 1, mi, M, n_, F_, w) == _lib.E_ARG, what
        assert lib.sfmhip_verify_matches_dev(h, kp, 3, pairs.ctypes.data, n, K4.ctypes.data, b, stride, c, t, H, rounds, 1, mi, b, n_, F_, w) == _lib.E_ARG, what
    # NULL with n_pairs > 0
    for args in ((None, 100, c, 2, 0.1, 64, 3, 1, 8, M, n_, F_, w), (b, 100, None, 2, 0.1, 64, 3, 1, 8, M, n_, F_, w),
                 (b, 100, c, 2, 0.1, 64, 3, 1, 8, None, n_, F_, w), (b, 100, c, 2, 0.1, 64, 3, 1, 8, M, None, F_, w)):
        assert lib.sfmhip_verify_pairs(h, *args) == _lib.E_ARG
        assert lib.sfmhip_verify_pairs_dev(h, *args) == _lib.E_ARG
    # a pair that names an image that is not there; a K without a focal length
    bad = np.array([[0, 1], [1, 3]], np.int32)
    assert lib.sfmhip_verify_matches_dev(h, kp, 3, bad.ctypes.data, 2, K4.ctypes.data, b, 100, c, 0.1, 64, 3, 1, 8, b, n_, F_, w) == _lib.E_ARG
    K0 = np.array([0.0, 1.0, 0.0, 0.0])
    assert lib.sfmhip_verify_matches_dev(h, kp, 3, pairs.ctypes.data, 2, K0.ctypes.data, b, 100, c, 0.1, 64, 3, 1, 8, b, n_, F_, w) == _lib.E_ARG
    assert lib.sfmhip_verify_matches_dev(h, None, 3, pairs.ctypes.data, 2, K4.ctypes.data, b, 100, c, 0.1, 64, 3, 1, 8, b, n_, F_, w) == _lib.E_ARG
    assert (mask == 7).all() and (cnt == -7).all() and (F == 7).all() and (win == -7).all()
    # n_pairs == 0: OK, no pointer touched
    assert lib.sfmhip_verify_pairs(h, None, 100, None, 0, 0.1, 64, 3, 1, 8, None, None, None, None) == 0
    assert lib.sfmhip_verify_pairs_dev(h, None, 100, None, 0, 0.1, 64, 3, 1, 8, None, None, None, None) == 0
    assert lib.sfmhip_verify_matches_dev(h, None, 0, None, 0, None, None, 100, None, 0.1, 64, 3, 1, 8, None, None, None, None) == 0
    with pytest.raises(api.SfmHipError):
        ctx.verify_pairs([rows], -0.5)
    with pytest.raises(api.SfmHipError):
        ctx.verify_pairs([rows], 0.1, rounds=9)


def test_a_failed_allocation_is_an_error_and_the_next_call_works(ctx):
    rows = _cached(("rows", 300), lambda: tv.scene_rows(300, out=0.3, seed=3))
    blocks, counts = _blocks([rows])
    mask = np.empty((1, 300), np.uint8); cnt = np.empty(1, np.int32)
    for failing in (1, 2):
        assert ctx.lib.sfmhip_debug_fail_allocations(ctx.h, failing) == 0
        for _ in range(failing):
            rc = ctx.lib.sfmhip_verify_pairs(ctx.h, blocks.ctypes.data, 300, counts.ctypes.data, 1, T1, 256, 3, 5, 8, mask.ctypes.data, cnt.ctypes.data, None, None)
            assert rc == _lib.E_HIP
        _check(ctx, blocks, counts, T1, 256, 3, 5, 8, tag="after a failed allocation")


# ---- driver ------------------------------------------------------------------------------------------------------------------------
def _verified_lines(log):
    return [(int(a), int(b), int(c)) for a, b, c in re.findall(r"^pair (\d+): verified (\d+) of (\d+)$", log, re.M)]


def test_driver_verify_matches_option(tmp_path):
    subprocess.check_call(["make", "-C", HOST], stdout=subprocess.DEVNULL)
    exe = os.path.join(HOST, "NViewReconstruct")
    out = subprocess.run([exe, os.path.join(GOLD, "crazyhorse_features.bin"), str(tmp_path), "--quiet", "--verify-matches"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    lines = _verified_lines(out.stdout)
    print(f"[twoview] crazyhorse: {lines}")
    assert [l[0] for l in lines] == list(range(6)) and all(0 <= k <= m for _, k, m in lines)
    for f in ("structure.yml", "structure_ba.yml", "structure_ba.ply"):
        assert (tmp_path / f).stat().st_size > 0, f
    assert "Save structure done." in out.stdout
    # the synthetic scene of test_drivers_gpu.py: the flag does not cost accuracy
    from test_drivers_gpu import _scene
    K, Rs, Ts, descs, kps, cols, X = _scene()
    feat = tmp_path / "features.bin"
    features_io.write_features(feat, K, kps, descs, cols, poses=list(zip(Rs, Ts)))
    rmse = []
    for flags in ([], ["--verify-matches=1.0,1024,3"]):
        d = tmp_path / ("with" if flags else "without"); d.mkdir()
        o = subprocess.run([exe, str(feat), str(d), "--poses-from-file", "--quiet"] + flags, capture_output=True, text=True)
        assert o.returncode == 0, o.stdout[-2000:] + o.stderr[-2000:]
        rmse.append(float(re.search(r"Final   RMSE\(pixel\): ([0-9.eE+-]+)", o.stdout).group(1)))
        got = _verified_lines(o.stdout)
        assert len(got) == (4 if flags else 0) and all(15 <= k <= m for _, k, m in got), got
    print(f"[twoview] synthetic scene: final RMSE {rmse[0]} without, {rmse[1]} with --verify-matches")
    assert rmse[1] <= 1.05 * rmse[0]
