"""SFMHIP_BA_SEAM bits 3..6: the one-workgroup reductions of an LM iteration moved off its critical path -- 8: the intrinsic block
and the scalars reduced by a front group of ba_camschur_kernel instead of by ba_fold_kernel; 16: ba_camstep_kernel with the gradient
maximum in a workgroup of its own; 32: one backward launch for the elimination tree below the top (chol_tree_backward_kernel);
64: ba_back_reduce_kernel with its loads in flight.  Every piece must leave every bit where the launches of SFMHIP_BA_SEAM=0 put
it: same operands, same order of every sum, so the comparison is for equality and needs no reference."""
import numpy as np
import pytest

from sfm_opencv_amd import synth
from test_ba_seam_gpu import N_IT, _args, _create, _rejecting_scene, _trace

pytestmark = pytest.mark.gpu

NEW_BITS = (8, 16, 32, 64)


def _run(ctx, args, seam, n=N_IT, **kw):
    pb = _create(ctx, args, seam, **kw)
    t = _trace(pb, n)
    plan = pb.debug_table("solver_plan")
    p = pb.params()
    pb.close()
    return t, p, plan


def _assert_bits_agree(ctx, args, seams, **kw):
    """Every switch value in `seams` against 0: per-iteration cost, radius, gradient norm and step count, then the parameters."""
    t0, p0, plan0 = _run(ctx, args, 0, **kw)
    plans = {0: plan0}
    for seam in seams:
        t, p, plan = _run(ctx, args, seam, **kw)
        assert t == t0, (seam, [(i, a, b) for i, (a, b) in enumerate(zip(t, t0)) if a != b][:3])
        for x, y in zip(p, p0):
            assert np.array_equal(x, y), seam
        assert np.array_equal(plan[:3], plan0[:3]), (seam, plan, plan0)      # the switch does not change the plan itself
        plans[seam] = plan
    return t0, plans


@pytest.mark.parametrize("shape", [(50, 80000), (24, 4000)])
def test_each_new_bit_alone_and_all_together_against_none(ctx, shape):
    sc = synth.ba_scene(*shape)
    t0, _ = _assert_bits_agree(ctx, _args(sc), NEW_BITS + (4 | 8, None))
    assert t0[-1][3] >= 5        # accepted steps


def test_two_parallel_separator_levels_in_one_backward_launch(ctx):
    """400 cameras, band 5: sixteen leaves, two levels of mutually independent separators below the top.  The plan is read back, so
    the test cannot pass on a plan whose backward sweep has nothing to merge."""
    sc = synth.ba_scene(400, 40000)
    _, plans = _assert_bits_agree(ctx, _args(sc), (32, None))
    leaves, levels, top_panels, one_launch = plans[None]
    assert leaves == 16 and levels >= 2 and top_panels >= 1, plans[None]
    assert one_launch == 1 and plans[32][3] == 1 and plans[0][3] == 0, plans


@pytest.mark.parametrize("n_cam,n_pt", [(50, 20000), (12, 2500)])
def test_switch_is_inert_without_parallel_separator_levels(ctx, n_cam, n_pt):
    """50 cameras: two leaves under the top, no parallel separator level; 12 cameras: one workgroup factors the whole system
    (chol_sparse_kernel).  Neither has a per-level backward loop to merge; the other pieces still apply."""
    sc = synth.ba_scene(n_cam, n_pt)
    _, plans = _assert_bits_agree(ctx, _args(sc), NEW_BITS + (None,))
    for plan in plans.values():
        assert plan[1] == 0 and plan[3] == 0, plans
    assert plans[None][0] == (2 if n_cam == 50 else 1), plans


def test_rejected_steps_feed_the_moved_reduction_from_the_point_kernel(ctx):
    """The scene of test_ba_seam_gpu that rejects steps and misses the guessed radius: the records the front group reduces then come
    from ba_point_kernel, not from the adopted pass of the last back-substitution."""
    args = _rejecting_scene()
    kw = dict(initial_trust_region_radius=1e6)
    t0, _ = _assert_bits_agree(ctx, args, (8, 4 | 8, None), **kw)
    assert N_IT - t0[-1][3] >= 1, t0[-1]        # the condition: at least one rejected step


@pytest.mark.parametrize("kw", [dict(fix_intrinsics=1), dict(fix_first_camera=0)])
def test_fixed_intrinsics_and_free_first_camera(ctx, kw):
    sc = synth.ba_scene(16, 3000)
    _assert_bits_agree(ctx, _args(sc), NEW_BITS + (None,), **kw)


def test_two_ranks_on_one_card_still_follow_the_single_rank(ctx):
    """Multi-rank handles take the pieces that do not depend on the rank count (the front group writes this rank's slot behind the
    message memset); tolerances of test_ba_gpu.test_two_point_shards_on_one_gpu_match_unsharded."""
    from test_ba_gpu import _run_sharded_on_one_gpu
    sc = synth.ba_scene(24, 4000)
    ref = _create(ctx, _args(sc), 0); sr = ref.iterate(5); Kr, extr, ptsr = ref.params(); ref.close()
    out, params, ids, counts = _run_sharded_on_one_gpu(sc, 5)
    for r in range(2):
        assert out[r]["iterations"] == sr["iterations"] and out[r]["successful_steps"] == sr["successful_steps"]
        assert abs(out[r]["final_cost"] - sr["final_cost"]) <= 1e-9 * sr["final_cost"]
        K, ext, pts = params[r]
        assert np.abs(ext - extr).max() <= 1e-9 and np.abs(K - Kr).max() <= 1e-9 * np.abs(Kr).max()
        assert np.abs(pts - ptsr[ids[r]]).max() <= 1e-9
