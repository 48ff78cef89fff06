"""GPU: the two-view relative pose (sfmhip_relative_pose and its device form) through the C-ABI, the Python layer and the driver.  The
reference is tests/relpose_ref.py, a numpy restatement of the definition in include/sfmhip.h that test_relpose_cpu.py checks against
numpy's SVD, scipy and the truth of the scenes.  The decomposition and the vote are compared in every bit; the refined pose within the
restatement's own spread over the order of its rows; the integers and the mask are recomputed from the bits of the pose the library
returned and must be EQUAL."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import homography_ref as hr
import relpose_ref as rp
import twoview_ref as tv
from sfm_opencv_amd import _lib, api
from test_relpose_cpu import ORDER_DIR_SPREAD, ORDER_ROT_SPREAD

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANGLE = math.radians(2.0)
# the library against the restatement after the refinement: 100 times the restatement's spread over five orders of its rows (measured on
# the CPU, test_relpose_cpu.py: 4.062e-10 and 2.857e-09 rad), with a floor of 1e-12 rad
ROT_BOUND = max(100 * ORDER_ROT_SPREAD, 1e-12)
DIR_BOUND = max(100 * ORDER_DIR_SPREAD, 1e-12)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _blocks(rows_list, stride=None, fill=0.0):
    counts = np.array([len(r) for r in rows_list], np.int32)
    stride = max(1, int(counts.max()) if len(counts) else 1) if stride is None else stride
    blocks = np.full((len(rows_list), stride, 4), fill)
    for q, r in enumerate(rows_list):
        blocks[q, :len(r)] = r
    return blocks, counts


def _masks(mask_list, stride, fill=0):
    out = np.full((len(mask_list), stride), fill, np.uint8)
    for q, m in enumerate(mask_list):
        out[q, :len(m)] = m
    return out


def _raw(ctx, blocks, counts, mask_in, F, t=rp.THR, rounds=3, iters=10, max_depth=50.0, min_angle=ANGLE, optional=True):
    """sfmhip_relative_pose on the C-ABI's own arrays, pre-filled with values the call never writes: (pose, info, quality, mask_out)"""
    blocks = np.ascontiguousarray(blocks, np.float64); counts = np.ascontiguousarray(counts, np.int32); F = np.ascontiguousarray(F, np.float64)
    n, stride = blocks.shape[0], blocks.shape[1]
    pose = np.full((n, 12), 7.0); info = np.full((n, 10), -7, np.int32); quality = np.full((n, 5), 7.0); mask = np.full((n, stride), 9, np.uint8)
    if mask_in is not None:
        mask_in = np.ascontiguousarray(mask_in, np.uint8)
        assert mask_in.shape == (n, stride)
    rc = ctx.lib.sfmhip_relative_pose(ctx.h, blocks.ctypes.data, stride, counts.ctypes.data, n, mask_in.ctypes.data if mask_in is not None else None,
                                      F.ctypes.data, t, rounds, iters, max_depth, min_angle, pose.ctypes.data, info.ctypes.data,
                                      quality.ctypes.data if optional else None, mask.ctypes.data if optional else None)
    assert rc == 0, ctx.lib.sfmhip_last_error(ctx.h)
    return pose, info, quality, mask


def _consistent(got, q, block, count, t=rp.THR, max_depth=50.0, min_angle=ANGLE, tag=None):
    """info and mask_out of pair q are what the restatement's per-row tests give at the pose the library returned; or the no-pose values"""
    pose, info, quality, mask = (a[q] for a in got)
    if info[0] == 0:
        assert np.isnan(pose).all() and np.isnan(quality).all() and not mask.any() and info[1] == -1 and not info[2:6].any() and not info[7:].any(), (tag, info)
        return
    assert info[0] == 1 and np.isfinite(pose).all() and np.isfinite(quality).all(), (tag, info, pose)
    n_inl, n_front, n_angle, want = rp.evaluate_at(pose, block, count, t, max_depth, min_angle)
    assert info[7:].tolist() == [n_inl, n_front, n_angle], (tag, info, n_inl, n_front, n_angle)
    assert np.array_equal(mask, want), (tag, np.flatnonzero(mask != want)[:5])
    R = pose[:9].reshape(3, 3)
    assert abs(np.linalg.det(R) - 1) < 1e-9 and abs(np.linalg.norm(pose[9:]) - 1) < 1e-12, tag


def _same_vote(got, q, ref, tag):
    """pose, cand, n4 and the singular values of pair q equal the restatement's in every bit (iters = 0)"""
    pose, info, quality, _ = (a[q] for a in got)
    assert info[:7].tolist() == ref["info"][:7].tolist(), (tag, info, ref["info"])
    assert np.array_equal(_bits(pose), _bits(ref["pose"])), (tag, pose, ref["pose"])
    assert np.array_equal(_bits(quality[:3]), _bits(ref["quality"][:3])), (tag, quality, ref["quality"])


# ---- bits: the decomposition and the vote ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_used", [8, 9, 255, 256, 257, 600])
def test_decomposition_and_vote_in_every_bit(ctx, n_used):
    a = rp.ransac_input(600, 0.3, 1)
    rows = a["rows"].copy()
    rows[[5, 100, 300]] = np.nan; rows[7, 2] = np.inf                     # NaN rows inside: not in L0, whatever their mask byte says
    mask = np.zeros(600, np.uint8)
    if n_used == 600:
        rows = a["rows"]; mask[:] = 1                                       # every row, the outliers included
    else:
        ok = np.flatnonzero((a["mask"] != 0) & np.isfinite(rows).all(axis=1))
        mask[ok[:n_used]] = 1; mask[[5, 100, 300, 7]] = 1
    stride = 640                                                            # NaN and garbage behind the count
    blocks, counts = _blocks([rows], stride, fill=np.nan)
    blocks[0, 600:620] = 1e300; blocks[0, 620:630] = rp.ransac_input(300, 0.0, 1)["rows"][:10]
    mask_in = _masks([mask], stride, fill=1)
    ref = rp.relative_pose_pair(blocks[0], 600, mask_in[0], a["F"], rp.THR, rounds=3, iters=0)
    assert ref["info"][0] == 1 and ref["info"][6] == n_used
    for rounds, iters in ((3, 0), (0, 10), (0, 0)):
        got = _raw(ctx, blocks, counts, mask_in, a["F"][None], rounds=rounds, iters=iters)
        _same_vote(got, 0, ref, (n_used, rounds, iters))
        _consistent(got, 0, blocks[0], 600, tag=n_used)
        assert got[1][0].tolist() == ref["info"].tolist() and np.array_equal(got[3][0], ref["mask_out"])
        assert got[2][0, 3] == got[2][0, 4] and abs(got[2][0, 3] - ref["quality"][3]) <= 1e-9 * ref["quality"][3]
    if n_used == 600:                                                       # mask_in NULL against all ones
        null = _raw(ctx, blocks, counts, None, a["F"][None], iters=0)
        for x, y in zip(null, got):
            assert x.tobytes() == y.tobytes()


def test_all_four_candidates_in_every_bit(ctx):
    inputs = rp.cand_inputs()
    assert {c[3] for c in inputs} == {0, 1, 2, 3}
    blocks, counts = _blocks([c[0] for c in inputs])
    got = _raw(ctx, blocks, counts, _masks([c[1] for c in inputs], blocks.shape[1]), np.stack([c[2] for c in inputs]), iters=0)
    for q, (rows, mask, F, cand, what) in enumerate(inputs):
        ref = rp.relative_pose_pair(rows, len(rows), mask, F, rp.THR, rounds=0, iters=0)
        _same_vote(got, q, ref, what)
        assert got[1][q, 1] == cand and got[1][q].tolist() == ref["info"].tolist() and np.array_equal(got[3][q], ref["mask_out"]), what


# ---- the whole call: repeatable, and a pair does not depend on its batch -----------------------------------------------------------
def _mixed_batch():
    """70 pairs in blocks of 640 rows: the 18 RANSAC inputs, the candidate inputs, short and empty blocks, pairs without a pose"""
    rows, masks, Fs = [], [], []
    for case in rp.CASES18:
        a = rp.ransac_input(*case)
        rows.append(a["rows"]); masks.append(a["mask"]); Fs.append(a["F"])
    for r_, m_, F_, _, _ in rp.cand_inputs():
        rows.append(r_); masks.append(m_); Fs.append(F_)
    a = rp.ransac_input(300, 0.3, 2)
    ok = np.flatnonzero(a["mask"])
    for k in (0, 7, 8, 9, 64, 65):                                          # empty, |U| = 7 (no pose), short sets
        m = np.zeros(300, np.uint8); m[ok[:k]] = 1
        rows.append(a["rows"] if k else a["rows"][:0]); masks.append(m if k else m[:0]); Fs.append(a["F"])
    rows.append(a["rows"]); masks.append(a["mask"]); Fs.append(np.full(9, np.nan))                    # no pose: NaN F
    rows.append(hr.scene_rows("rotation", 200, 0.2, 3)); masks.append(np.ones(200, np.uint8)); Fs.append(a["F"])     # an F that is not the pair's
    k = 0
    while len(rows) < 70:                                                   # the RANSAC inputs again with every row in U, then with their rows reversed
        b = rp.ransac_input(*rp.CASES18[k % 18])
        rows.append(b["rows"] if k < 18 else b["rows"][::-1]); masks.append(np.ones(len(b["rows"]), np.uint8) if k < 18 else b["mask"][::-1]); Fs.append(b["F"])
        k += 1
    blocks, counts = _blocks(rows, 640, fill=np.nan)
    return blocks, counts, _masks(masks, 640, fill=1), np.stack(Fs)


def test_a_batch_equals_itself_and_its_pairs_alone(ctx):
    blocks, counts, mask_in, F = _mixed_batch()
    assert len(counts) == 70
    got = _raw(ctx, blocks, counts, mask_in, F)
    again = _raw(ctx, blocks, counts, mask_in, F)
    for x, y in zip(got, again):
        assert x.tobytes() == y.tobytes()
    status = got[1][:, 0]
    assert (status == 0).sum() >= 3 and (status == 1).sum() >= 60, status
    assert got[1][34].tolist() == [0, -1, 0, 0, 0, 0, 0, 0, 0, 0] and counts[34] == 0       # the empty pair
    for q in range(70):
        _consistent(got, q, blocks[q], int(counts[q]), tag=q)
        c = max(1, int(counts[q]))
        one = _raw(ctx, blocks[q:q + 1, :c], counts[q:q + 1], mask_in[q:q + 1, :c], F[q:q + 1])             # alone, in a block of its own length
        assert one[0].tobytes() == got[0][q].tobytes() and one[1].tobytes() == got[1][q].tobytes() and one[2].tobytes() == got[2][q].tobytes(), q
        assert np.array_equal(one[3][0], got[3][q, :c]) and not got[3][q, c:].any(), q
    part = _raw(ctx, blocks, counts, mask_in, F, optional=False)          # quality and mask_out are optional
    assert part[0].tobytes() == got[0].tobytes() and part[1].tobytes() == got[1].tobytes() and (part[2] == 7).all() and (part[3] == 9).all()


def test_a_batch_longer_than_one_launch(ctx):
    # relpose.hip enqueues a batch in slices of 32768 pairs: pairs at the end of the first slice and in the second, everything else empty
    n, stride = 32768 + 5, 16
    a = rp.ransac_input(300, 0.0, 1)
    ok = np.flatnonzero(a["mask"])
    blocks = np.full((n, stride, 4), np.nan); counts = np.zeros(n, np.int32); F = np.full((n, 9), np.nan); mask_in = np.ones((n, stride), np.uint8)
    live = (0, 32767, 32768, n - 1)
    for k, q in enumerate(live):
        rows = a["rows"][ok[20 * k:20 * k + 12 + k]]
        blocks[q, :len(rows)] = rows; counts[q] = len(rows); F[q] = a["F"]
    got = _raw(ctx, blocks, counts, mask_in, F)
    for q in live:
        one = _raw(ctx, blocks[q:q + 1], counts[q:q + 1], mask_in[q:q + 1], F[q:q + 1])
        assert one[1][0, 0] == 1 and one[1][0, 6] == counts[q]
        for x, y in zip(got, one):
            assert x[q].tobytes() == y[0].tobytes(), q
        _consistent(got, q, blocks[q], int(counts[q]), tag=q)
    rest = np.ones(n, bool); rest[list(live)] = False
    assert np.isnan(got[0][rest]).all() and (got[1][rest] == [0, -1, 0, 0, 0, 0, 0, 0, 0, 0]).all() and np.isnan(got[2][rest]).all() and not got[3][rest].any()


# ---- the refinement ---------------------------------------------------------------------------------------------------------------
def test_refined_pose_against_the_restatement(ctx):
    ins = [rp.ransac_input(*c) for c in rp.CASES18]
    blocks, counts = _blocks([a["rows"] for a in ins], fill=np.nan)
    mask_in = _masks([a["mask"] for a in ins], blocks.shape[1])
    F = np.stack([a["F"] for a in ins])
    got = _raw(ctx, blocks, counts, mask_in, F)
    one = _raw(ctx, blocks, counts, mask_in, F, rounds=1)
    for q, (case, a) in enumerate(zip(rp.CASES18, ins)):
        ref = rp.relative_pose_pair(a["rows"], len(a["rows"]), a["mask"], a["F"], rp.THR)
        rot, dirn = rp.rotation_angle(got[0][q, :9], ref["pose"][:9]), rp.direction_angle(got[0][q, 9:], ref["pose"][9:])
        print(f"{case}: library against restatement rot {rot:.3e} dir {dirn:.3e} rad; cost {got[2][q, 3]:.6e} -> {got[2][q, 4]:.6e}")
        assert rot <= ROT_BOUND and dirn <= DIR_BOUND, (case, rot, dirn)
        assert got[1][q, :7].tolist() == ref["info"][:7].tolist() and np.array_equal(_bits(got[2][q, :3]), _bits(ref["quality"][:3]))
        _consistent(got, q, blocks[q], int(counts[q]), tag=case)
        _consistent(one, q, blocks[q], int(counts[q]), tag=case)
        assert one[2][q, 4] <= one[2][q, 3] and got[2][q, 4] <= got[2][q, 3], case


def test_integers_equal_the_restatements_away_from_the_thresholds(ctx):
    """Where no row lies within a relative 1e-6 of a threshold under the restatement's pose, a pose 1e-7 rad away decides every row the
    same way: info and mask_out equal the restatement's own."""
    found = []
    for seed in range(1, 40):
        pix, _ = tv.two_view_scene(300, 0.3, seed)
        rows = tv.normalised(pix)
        mask, cnt, _, F = tv.verify_pair(rows, 300, rp.THR, 256, 3, seed, 8)
        ref = rp.relative_pose_pair(rows, 300, mask, F, rp.THR)
        if ref["info"][0] == 1 and rp.threshold_margin(ref["pose"], rows, 300, rp.THR, 50.0, ANGLE) >= 1e-6:
            found.append((rows, mask, F, ref, seed))
        if len(found) == 4:
            break
    assert len(found) == 4
    blocks, counts = _blocks([f[0] for f in found])
    got = _raw(ctx, blocks, counts, _masks([f[1] for f in found], 300), np.stack([f[2] for f in found]))
    for q, (rows, mask, F, ref, seed) in enumerate(found):
        assert rp.threshold_margin(ref["pose"], rows, 300, rp.THR, 50.0, ANGLE) >= 1e-6             # the precondition
        assert got[1][q].tolist() == ref["info"].tolist(), (seed, got[1][q], ref["info"])
        assert np.array_equal(got[3][q], ref["mask_out"]), seed


# ---- edges -------------------------------------------------------------------------------------------------------------------------
def test_seven_rows_nan_F_and_a_depth_bound_give_no_pose(ctx):
    a = rp.ransac_input(300, 0.3, 1)
    ok = np.flatnonzero(a["mask"])
    seven = np.zeros(300, np.uint8); seven[ok[:7]] = 1
    eight = np.zeros(300, np.uint8); eight[ok[:8]] = 1
    bad_F = a["F"].copy(); bad_F[4] = np.nan
    blocks, counts = _blocks([a["rows"]] * 4)
    got = _raw(ctx, blocks, counts, np.stack([seven, eight, a["mask"], a["mask"]]), np.stack([a["F"], a["F"], bad_F, np.zeros(9)]))
    assert got[1][:, 0].tolist() == [0, 1, 0, 0] and got[1][:, 6].tolist() == [7, 8, a["count"], a["count"]]
    for q in range(4):
        _consistent(got, q, blocks[q], 300, tag=q)
    # the scene is 8 to 18 baselines deep: nothing is in front and nearer than one baseline
    got = _raw(ctx, blocks[:1], counts[:1], a["mask"][None], a["F"][None], max_depth=1.0)
    assert got[1][0].tolist() == [0, -1, 0, 0, 0, 0, a["count"], 0, 0, 0] and np.isnan(got[0]).all() and np.isnan(got[2]).all() and not got[3].any()
    got = _raw(ctx, blocks[:1], counts[:1], a["mask"][None], a["F"][None], max_depth=0.0)              # no bound
    assert got[1][0, 0] == 1
    _consistent(got, 0, blocks[0], 300, max_depth=0.0)


def test_parallax_angles(ctx):
    a = rp.ransac_input(600, 0.0, 1)
    blocks, counts = _blocks([a["rows"]])
    n_angle = {}
    for deg in (0.0, 2.0, 4.0, 90.0):
        ang = math.pi / 2 if deg == 90.0 else math.radians(deg)
        got = _raw(ctx, blocks, counts, a["mask"][None], a["F"][None], min_angle=ang)
        _consistent(got, 0, blocks[0], 600, min_angle=ang, tag=deg)
        n_angle[deg] = int(got[1][0, 9]); n_front = int(got[1][0, 8])
    assert n_angle[0.0] == n_front > 500 and n_angle[90.0] == 0 and 0 < n_angle[4.0] < n_front and n_angle[4.0] <= n_angle[2.0] <= n_front, (n_angle, n_front)


def test_a_pure_rotation_ends(ctx):
    rows = hr.scene_rows("rotation", 300, 0.2, 3)
    mask, cnt, _, F = tv.verify_pair(rows, 300, rp.THR, 256, 3, 3, 8)
    assert cnt > 150                                                        # accepted with a high count although its F is not determined
    blocks, counts = _blocks([rows])
    got = _raw(ctx, blocks, counts, mask[None], F[None], rounds=8, iters=50)
    _consistent(got, 0, blocks[0], 300, tag="rotation")


# ---- errors and layers -----------------------------------------------------------------------------------------------------------
def test_bad_arguments_leave_the_outputs_alone(ctx):
    lib, h = ctx.lib, ctx.h
    a = rp.ransac_input(300, 0.3, 1)
    blocks, counts = _blocks([a["rows"], a["rows"][:50]])
    mask_in = np.ones((2, 300), np.uint8); F = np.stack([a["F"], a["F"]])
    pose = np.full((2, 12), 7.0); info = np.full((2, 10), -7, np.int32); quality = np.full((2, 5), 7.0); mask = np.full((2, 300), 9, np.uint8)
    b, c, mi, F_, p_, i_, q_, m_ = (x.ctypes.data for x in (blocks, counts, mask_in, F, pose, info, quality, mask))
    good = dict(t=0.1, rounds=3, iters=10, md=50.0, ang=0.03, stride=300, n=2)
    for k, v in (("t", -1.0), ("t", np.nan), ("t", np.inf), ("md", -1.0), ("md", np.nan), ("md", np.inf), ("ang", -0.1), ("ang", np.nan), ("ang", 1.6),
                 ("rounds", -1), ("rounds", 9), ("iters", -1), ("iters", 51), ("stride", -1), ("n", -1)):
        g = dict(good); g[k] = v
        for fn in (lib.sfmhip_relative_pose, lib.sfmhip_relative_pose_dev):
            assert fn(h, b, g["stride"], c, g["n"], mi, F_, g["t"], g["rounds"], g["iters"], g["md"], g["ang"], p_, i_, q_, m_) == _lib.E_ARG, (k, v)
    for args in ((None, 300, c, 2, mi, F_), (b, 300, None, 2, mi, F_), (b, 300, c, 2, mi, None)):
        for fn in (lib.sfmhip_relative_pose, lib.sfmhip_relative_pose_dev):
            assert fn(h, *args, 0.1, 3, 10, 50.0, 0.03, p_, i_, q_, m_) == _lib.E_ARG
    for outs in ((None, i_, q_, m_), (p_, None, q_, m_)):
        for fn in (lib.sfmhip_relative_pose, lib.sfmhip_relative_pose_dev):
            assert fn(h, b, 300, c, 2, mi, F_, 0.1, 3, 10, 50.0, 0.03, *outs) == _lib.E_ARG
    assert (pose == 7).all() and (info == -7).all() and (quality == 7).all() and (mask == 9).all()
    for fn in (lib.sfmhip_relative_pose, lib.sfmhip_relative_pose_dev):     # n_pairs == 0: OK, no pointer touched
        assert fn(h, None, 100, None, 0, None, None, 0.1, 3, 10, 50.0, 0.03, None, None, None, None) == 0
    with pytest.raises(api.SfmHipError):
        ctx.relative_pose([a["rows"]], None, a["F"][None], -0.5)
    with pytest.raises(api.SfmHipError):
        ctx.relative_pose([a["rows"]], None, a["F"][None], 0.1, min_angle_deg=91.0)


def test_a_failed_allocation_is_an_error_and_the_next_call_works(ctx):
    a = rp.ransac_input(300, 0.3, 1)
    blocks, counts = _blocks([a["rows"]])
    want = _raw(ctx, blocks, counts, a["mask"][None], a["F"][None])
    pose = np.empty((1, 12)); info = np.empty((1, 10), np.int32)
    for failing in (1, 2):
        assert ctx.lib.sfmhip_debug_fail_allocations(ctx.h, failing) == 0
        for _ in range(failing):
            rc = ctx.lib.sfmhip_relative_pose(ctx.h, blocks.ctypes.data, 300, counts.ctypes.data, 1, None, a["F"].ctypes.data, rp.THR, 3, 10, 50.0, ANGLE,
                                              pose.ctypes.data, info.ctypes.data, None, None)
            assert rc == _lib.E_HIP
        got = _raw(ctx, blocks, counts, a["mask"][None], a["F"][None])
        for x, y in zip(got, want):
            assert x.tobytes() == y.tobytes()


def test_python_layer_and_device_arrays(ctx):
    import torch
    blocks, counts, mask_in, F = _mixed_batch()
    n, stride = blocks.shape[:2]
    want = _raw(ctx, blocks, counts, mask_in, F)
    lists = [blocks[q, :counts[q]] for q in range(n)]
    pose, info, quality, masks = ctx.relative_pose(lists, [mask_in[q, :counts[q]] for q in range(n)], F.reshape(n, 3, 3), rp.THR)
    assert pose.tobytes() == want[0].tobytes() and info.tobytes() == want[1].tobytes() and quality.tobytes() == want[2].tobytes()
    for q, m in enumerate(masks):
        assert m.dtype == np.uint8 and np.array_equal(m, want[3][q, :counts[q]])
    d_corr = torch.from_numpy(blocks).cuda(); d_counts = torch.from_numpy(counts).cuda(); d_min = torch.from_numpy(mask_in).cuda(); d_F = torch.from_numpy(F).cuda()
    d_pose = torch.full((n, 12), 7.0, dtype=torch.float64, device="cuda"); d_info = torch.full((n, 10), -7, dtype=torch.int32, device="cuda")
    d_q = torch.full((n, 5), 7.0, dtype=torch.float64, device="cuda"); d_mask = torch.full((n, stride), 9, dtype=torch.uint8, device="cuda")
    keep = d_corr.clone()
    torch.cuda.synchronize()
    ctx.relative_pose_dev(d_corr, stride, d_counts, n, d_min, d_F, rp.THR, d_pose, d_info, d_q, d_mask)
    ctx.synchronize()
    assert d_pose.cpu().numpy().tobytes() == want[0].tobytes() and d_info.cpu().numpy().tobytes() == want[1].tobytes()
    assert d_q.cpu().numpy().tobytes() == want[2].tobytes() and np.array_equal(d_mask.cpu().numpy(), want[3])
    assert torch.equal(keep.view(torch.int64), d_corr.view(torch.int64))    # the inputs are left alone
    d_pose2 = torch.full((n, 12), 7.0, dtype=torch.float64, device="cuda"); d_info2 = torch.full((n, 10), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.relative_pose_dev(d_corr, stride, d_counts, n, d_min, d_F, rp.THR, d_pose2, d_info2)        # without the optional outputs
    ctx.synchronize()
    assert torch.equal(d_pose.view(torch.int64), d_pose2.view(torch.int64)) and torch.equal(d_info, d_info2)


def _chain_of_two():
    """three images: pair (0, 1) a general scene with 30 % wrong matches, pair (1, 2) a planar one"""
    g, good = tv.two_view_scene(400, 0.3, 5)
    p, _ = hr.scene("planar", 300, 0.2, 6)
    pts = [g[:, :2], np.concatenate([g[:, 2:], p[:, :2]]), p[:, 2:]]
    kps = []
    for xy in pts:
        k = np.zeros(len(xy), api.KEYPOINT); k["x"] = xy[:, 0]; k["y"] = xy[:, 1]
        kps.append(k)
    m0 = np.zeros(400, api.DMATCH); m0["queryIdx"] = np.arange(400); m0["trainIdx"] = np.arange(400)
    m1 = np.zeros(300, api.DMATCH); m1["queryIdx"] = 400 + np.arange(300); m1["trainIdx"] = np.arange(300)
    return kps, [m0, m1], good


def test_relative_pose_for_all(ctx):
    kps, lists, good = _chain_of_two()
    K = np.array([[800.0, 0, 512], [0, 800.0, 384], [0, 0, 1]])
    out = api.relative_pose_for_all(K, kps, lists, px=1.0, px_h=2.0, hypotheses=256, seed=2, ctx=ctx)
    assert [o["kind"] for o in out] == [1, 2]
    g, p = out
    assert g["ok"] and g["R"].shape == (3, 3) and g["t"].shape == (3,) and g["kept"].dtype == bool and len(g["kept"]) == 400
    rot, dirn = math.degrees(rp.rotation_angle(g["R"], rp.TRUE_R)), math.degrees(rp.direction_angle(g["t"], rp.TRUE_T))
    c = g["counts"]
    inl_kept, wrong = (g["kept"] & good).sum() / good.sum(), int((g["kept"] & ~good).sum())
    print(f"general pair: rot {rot:.3f} dir {dirn:.3f} deg, counts {c}, sv {g['sv']}, kept {inl_kept:.3f} wrong {wrong}")
    assert rot <= 0.5 and dirn <= 3.0
    assert c["n_inl"] > c["n_used"] > 15 and g["kept"].sum() == c["n_front"] and inl_kept >= 0.9 and wrong <= 0.02 * c["n_inl"]
    assert c["n4"][c["cand"]] == max(c["n4"]) and np.isfinite(g["sv"]).all() and g["sv"][0] >= g["sv"][1] >= g["sv"][2]
    # the planar pair comes back kind 2 without a pose
    assert not p["ok"] and np.isnan(p["R"]).all() and np.isnan(p["t"]).all() and not p["kept"].any() and len(p["kept"]) == 300


# ---- driver ------------------------------------------------------------------------------------------------------------------------
def test_driver_pose_device_option(tmp_path):
    """tests/golden/crazyhorse_features.bin: seven images of a statue; its first pair is general (asserted below from the driver's own
    geometry line).  Bundle adjustment reaches the same minimum from either start, only the kept matches of the first pair differ: the
    final RMSE may not be more than 1.05 times that of the same run without --pose-device."""
    host = os.path.join(ROOT, "sfm_opencv_amd", "host")
    subprocess.check_call(["make", "-C", host], stdout=subprocess.DEVNULL)
    exe = os.path.join(host, "NViewReconstruct")
    feat = os.path.join(ROOT, "tests", "golden", "crazyhorse_features.bin")
    rmse = {}
    for name, flags in (("without", ["--two-view-geometry"]), ("with", ["--two-view-geometry", "--pose-device"])):
        d = tmp_path / name; d.mkdir()
        out = subprocess.run([exe, feat, str(d), "--quiet"] + flags, capture_output=True, text=True)
        assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
        log = out.stdout
        assert re.search(r"^pair 0: geometry general, kept \d+ of \d+ ", log, re.M), log[:2000]
        line = re.search(r"^pair 0: pose on device, kept (\d+) of (\d+), (\d+) in front, (\d+) with parallax$", log, re.M)
        if name == "with":
            assert line, log[:3000]
            k, m, front, ang = (int(x) for x in line.groups())
            print(f"[relpose] crazyhorse: {line.group(0)}")
            assert 15 < k <= m and front == k and ang <= front
        else:
            assert not line and "device pose" not in log                   # without the option nothing changes
        assert "Save structure done." in log
        rmse[name] = float(re.search(r"Final   RMSE\(pixel\): ([0-9.eE+-]+)", log).group(1))
        for f in ("structure.yml", "structure_ba.yml", "structure_ba.ply"):
            assert (d / f).stat().st_size > 0, f
    print(f"[relpose] crazyhorse: final RMSE {rmse['without']} without, {rmse['with']} with --pose-device")
    assert rmse["with"] <= 1.05 * rmse["without"], rmse
    # the option needs --two-view-geometry
    alone = subprocess.run([exe, feat, str(tmp_path), "--quiet", "--pose-device"], capture_output=True, text=True)
    assert alone.returncode != 0 and "--pose-device needs --two-view-geometry" in alone.stdout
    # its arguments, and the two-view driver, which takes the same switch for its find_transform
    two = subprocess.run([os.path.join(host, "TwoViewReconstruct"), feat, str(tmp_path), "--quiet", "--two-view-geometry", "--pose-device=2,5"],
                         capture_output=True, text=True)
    assert two.returncode == 0, two.stdout[-2000:] + two.stderr[-2000:]
    assert re.search(r"^pair 0: (pose on device, kept \d+ of \d+, \d+ in front, \d+ with parallax|device pose rejected \(.*\), host fallback)$", two.stdout, re.M)
    assert "successful!!!" in two.stdout
