"""SFMHIP_BA_SEAM: the pieces of an LM iteration that ride inside its big kernels (bit 2: the point pass of the next linearisation
inside the back-substitution, ba_back_kernel_lin) must leave every bit where the separate launches put it.  The switch is read per
handle in sfmhip_ba_create, so one process builds both forms."""
import os

import numpy as np
import pytest

from sfm_opencv_amd import synth

pytestmark = pytest.mark.gpu

N_IT = 30


def _args(sc):
    return sc["K0"], sc["ext0"], sc["pts0"], sc["obs_cam"], sc["obs_pt"], sc["obs_uv"]


def _create(ctx, args, seam, **kw):
    old = os.environ.get("SFMHIP_BA_SEAM")
    try:
        if seam is None:
            os.environ.pop("SFMHIP_BA_SEAM", None)
        else:
            os.environ["SFMHIP_BA_SEAM"] = str(seam)
        return ctx.ba_create(*args, opts=ctx.ba_options(**kw))
    finally:
        if old is None:
            os.environ.pop("SFMHIP_BA_SEAM", None)
        else:
            os.environ["SFMHIP_BA_SEAM"] = old


def _trace(pb, n=N_IT):
    """n forced iterations, one call each (the adopted point pass is state of the handle and must survive the call boundary):
    the per-iteration summaries that the decision depends on."""
    out = []
    for _ in range(n):
        s = pb.iterate(1)
        out.append((s["final_cost"], s["final_radius"], s["final_gradient_max_norm"], s["successful_steps"]))
    return out


def _assert_same(ctx, args, **kw):
    off = _create(ctx, args, 0, **kw); on = _create(ctx, args, None, **kw)
    t_off, t_on = _trace(off), _trace(on)
    assert t_on == t_off, [(i, a, b) for i, (a, b) in enumerate(zip(t_on, t_off)) if a != b][:3]
    for x, y in zip(on.params(), off.params()):
        assert np.array_equal(x, y)
    # all iterations in one call: the same bits again
    one = _create(ctx, args, None, **kw); s = one.iterate(N_IT)
    assert s["final_cost"] == t_off[-1][0] and s["iterations"] == N_IT
    for x, y in zip(one.params(), off.params()):
        assert np.array_equal(x, y)
    n_acc = t_off[-1][3]
    off.close(); on.close(); one.close()
    return n_acc


@pytest.mark.parametrize("shape", [(50, 80000), (24, 4000)])
def test_switch_off_and_default_agree_bit_for_bit(ctx, shape):
    sc = synth.ba_scene(*shape)
    assert _assert_same(ctx, _args(sc)) >= 5        # accepted steps: the adopted point pass has been used


def _rejecting_scene():
    sc = synth.ba_scene(24, 2000, seed=2)
    rng = np.random.default_rng(7)
    pts0 = sc["pts0"].copy(); ext0 = sc["ext0"].copy()
    pts0 += rng.normal(0, 1.0, pts0.shape)
    ext0[1:] += rng.normal(0, 0.2, ext0[1:].shape)
    return sc["K0"], ext0, pts0, sc["obs_cam"], sc["obs_pt"], sc["obs_uv"]


def test_rejected_steps_and_missed_radius_fall_back_to_the_point_kernel(ctx):
    """A start far from the solution with a large first radius: LM rejects steps and accepted steps end at a radius other than the
    guessed min(max, 3 radius), so the adopted pass must be dropped and ba_point_kernel run instead."""
    args = _rejecting_scene()
    kw = dict(initial_trust_region_radius=1e6)
    probe = _create(ctx, args, None, **kw)
    s = probe.iterate(N_IT)
    probe.close()
    assert s["iterations"] - s["successful_steps"] >= 1, s        # the condition: this scene leaves the fast path
    _assert_same(ctx, args, **kw)


def test_reset_rearms_the_adopted_pass(ctx):
    sc = synth.ba_scene(24, 4000)
    pb = _create(ctx, _args(sc), None)
    first = _trace(pb); p1 = pb.params()
    pb.reset()
    second = _trace(pb); p2 = pb.params()
    assert first == second
    for x, y in zip(p1, p2):
        assert np.array_equal(x, y)
    # and a reduced-system query in between (it rebuilds the point side with another radius) does not leak into the loop
    pb.reset(); pb.iterate(3); pb.reduced_system(7.0); rest = _trace(pb, N_IT - 3)
    assert rest[-1][:3] == first[-1][:3]
    for x, y in zip(pb.params(), p1):
        assert np.array_equal(x, y)
    pb.close()


@pytest.mark.parametrize("kw", [dict(fix_intrinsics=1), dict(fix_intrinsics=0, huber_delta=0.0), dict(fix_first_camera=0)])
def test_fixed_intrinsics_and_free_first_camera(ctx, kw):
    sc = synth.ba_scene(16, 3000)
    _assert_same(ctx, _args(sc), **kw)


def test_constant_first_camera_and_an_unobserved_camera_in_the_middle(ctx):
    """cam_pos < 0 (the constant first camera) inside the blocks' camera ranges, and a free camera no observation touches."""
    sc = synth.ba_scene(12, 2500)
    keep = sc["obs_cam"] != 6
    args = (sc["K0"], sc["ext0"], sc["pts0"], sc["obs_cam"][keep], sc["obs_pt"][keep], sc["obs_uv"][keep])
    _assert_same(ctx, args)


def test_blocks_wider_than_the_staged_camera_window(ctx):
    """Random tracks over 64 cameras: a block of 256 points spans more cameras than ba_back_kernel stages in LDS (BACK_NCL = 24)
    and reads the camera records from global memory."""
    sc = synth.ba_scene(64, 3000)
    rng = np.random.default_rng(11)
    n_pt = sc["n_pt"]
    L = rng.integers(2, 5, size=n_pt)
    obs_pt = np.repeat(np.arange(n_pt), L).astype(np.int32)
    obs_cam = np.concatenate([rng.choice(64, size=l, replace=False) for l in L]).astype(np.int32)
    order = np.lexsort((obs_pt, obs_cam)); obs_cam, obs_pt = obs_cam[order], obs_pt[order]
    uv = synth.project(synth.K_REF, sc["ext_true"][obs_cam], sc["pts_true"][obs_pt]) + 0.5 * rng.standard_normal((len(obs_pt), 2))
    # keep what lies in front of its camera (the ring cameras look at the origin, the points sit in a ball around it: all of it)
    args = (sc["K0"], sc["ext0"], sc["pts0"], obs_cam, obs_pt, uv)
    pb = _create(ctx, args, None)
    import ctypes as C
    n = C.c_size_t()
    ctx._check(ctx.lib.sfmhip_ba_debug_table(pb.h, b"blk_crange", None, 0, C.byref(n)))
    cr = np.empty(n.value // 4, np.int32)
    ctx._check(ctx.lib.sfmhip_ba_debug_table(pb.h, b"blk_crange", cr.ctypes.data, cr.nbytes, C.byref(n)))
    pb.close()
    cr = cr.reshape(-1, 2)
    assert (cr[:, 1] - cr[:, 0] >= 24).any(), cr[:4]
    _assert_same(ctx, args)


def test_two_ranks_on_one_card_still_follow_the_single_rank(ctx):
    """The multi-rank path keeps its own launches (the switch does not reach it); same tolerances as
    test_ba_gpu.test_two_point_shards_on_one_gpu_match_unsharded."""
    from test_ba_gpu import _run_sharded_on_one_gpu
    sc = synth.ba_scene(24, 4000)
    ref = _create(ctx, _args(sc), None); sr = ref.iterate(5); Kr, extr, ptsr = ref.params(); ref.close()
    out, params, ids, counts = _run_sharded_on_one_gpu(sc, 5)
    for r in range(2):
        assert out[r]["iterations"] == sr["iterations"] and out[r]["successful_steps"] == sr["successful_steps"]
        assert abs(out[r]["final_cost"] - sr["final_cost"]) <= 1e-9 * sr["final_cost"]
        K, ext, pts = params[r]
        assert np.abs(ext - extr).max() <= 1e-9 and np.abs(K - Kr).max() <= 1e-9 * np.abs(Kr).max()
        assert np.abs(pts - ptsr[ids[r]]).max() <= 1e-9
