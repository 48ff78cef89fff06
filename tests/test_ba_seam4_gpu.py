"""SFMHIP_BA_SEAM bit 8 (256): the LM step is judged under the next Schur build.  With bits 2 and 3 also set, ba_loop queues the next
ba_camschur_kernel at the candidate right behind ba_back_kernel_lin, its front group does ba_back_reduce_kernel's job (the sums and
the publication of the step scalars), and an accepted step with the guessed radius folds that launch's partials; any other outcome
leaves them unfolded and builds again.  Same operands and the same order of every sum as with the switch at 0, so every comparison
is for equality.  The path is taken only inside calls of more than one iteration (never in a call's last), so the handles under
test run in calls of several iterations and are compared at every call boundary with the per-iteration trace of SFMHIP_BA_SEAM=0:
cost, radius, gradient norm, accepted steps, the nine published step scalars, and K, extrinsics and points."""
import os

import numpy as np
import pytest

from sfm_opencv_amd import api, synth
from test_ba_seam_gpu import N_IT, _args, _create, _rejecting_scene

pytestmark = pytest.mark.gpu

BIT = 256
SEAMS = (BIT, None)          # the bit alone (inert: it needs bits 2 and 3), and with all the others as when the variable is unset
MIXED = (2, 3, 1, 7, 5, 2, 10)
assert sum(MIXED) == N_IT


def _state(pb, s):
    return (s["final_cost"], s["final_radius"], s["final_gradient_max_norm"], s["successful_steps"],
            pb.debug_table("step_scalars").tobytes(), [x.copy() for x in pb.params()])


def _run(ctx, args, seam, calls, prep=None, **kw):
    """one handle, iterate(n) for n in calls: the state after every call"""
    pb = _create(ctx, args, seam, **kw)
    if prep is not None:
        prep(pb)
    out = [_state(pb, pb.iterate(n)) for n in calls]
    return pb, out


def _reference(ctx, args, n=N_IT, prep=None, **kw):
    pb, ref = _run(ctx, args, 0, [1] * n, prep=prep, **kw)
    pb.close()
    return ref


def _assert_follows(ref, calls, out, what):
    at = np.cumsum(calls) - 1
    for k, (i, got) in enumerate(zip(at, out)):
        assert got[:5] == ref[i][:5], (what, "call", k, "iteration", int(i), got[:4], ref[i][:4])
        for x, y in zip(got[5], ref[i][5]):
            assert np.array_equal(x, y), (what, "call", k, "iteration", int(i))


def _assert_bits_agree(ctx, args, patterns=((N_IT,), MIXED), n=N_IT, prep=None, **kw):
    ref = _reference(ctx, args, n, prep=prep, **kw)
    for seam in SEAMS:
        for calls in patterns:
            pb, out = _run(ctx, args, seam, calls, prep=prep, **kw)
            pb.close()
            _assert_follows(ref, calls, out, (seam, calls))
    return ref


def _decisions(ctx, ref, r0, **kw):
    """per iteration of a reference trace: (accepted, accepted with the radius the back-substitution guessed, error flag)"""
    rmax = ctx.ba_options(**kw).max_trust_region_radius
    out, prev_r, prev_n = [], r0, 0
    for cost, radius, _, nsucc, scal, _ in ref:
        acc = nsucc > prev_n
        out.append((acc, acc and radius == min(rmax, prev_r / (1.0 / 3.0)), np.frombuffer(scal)[8] != 0.0))
        prev_r, prev_n = radius, nsucc
    return out


def _experiments_build(ctx):
    """the speculation counters and SFMHIP_FUSE_MAX_BLOCKS exist only in -DSFMHIP_EXPERIMENTS builds of the library"""
    sc = synth.ba_scene(8, 300)
    pb = ctx.ba_create(*_args(sc))
    try:
        pb.debug_table("speculation")
        return True
    except api.SfmHipError:
        return False
    finally:
        pb.close()


def test_all_steps_accepted(ctx):
    sc = synth.ba_scene(24, 4000)
    ref = _assert_bits_agree(ctx, _args(sc), patterns=((N_IT,), MIXED, (2,) * 15))
    d = _decisions(ctx, ref, ctx.ba_options().initial_trust_region_radius)
    assert all(a and hit for a, hit, _ in d), d          # the condition: every launch queued ahead is adopted


def test_rejected_steps_and_radius_misses(ctx):
    args = _rejecting_scene()
    kw = dict(initial_trust_region_radius=1e6)
    ref = _assert_bits_agree(ctx, args, patterns=((N_IT,), MIXED, (2,) * 15), **kw)
    d = _decisions(ctx, ref, 1e6, **kw)
    assert any(not a for a, _, _ in d), d                # at least one rejected step
    assert any(a and not hit for a, hit, _ in d), d      # at least one accepted step whose radius is not the guess
    assert any(hit for _, hit, _ in d), d                # and launches that are adopted in between
    # a miss right behind a hit: that iteration had its launch queued ahead, and it was left unfolded
    assert any(d[i][1] and not d[i + 1][1] for i in range(N_IT - 2)), d


def test_calls_of_one_two_and_seven_iterations_alternating(ctx):
    """`built` and the adopted point pass are carried from call to call; a call's last iteration queues nothing ahead"""
    sc = synth.ba_scene(24, 4000)
    calls = (1, 2, 7) * 3
    ref = _assert_bits_agree(ctx, _args(sc), patterns=(calls,))
    args = _rejecting_scene()
    _assert_bits_agree(ctx, args, patterns=(calls,), initial_trust_region_radius=1e6)
    assert sum(calls) == N_IT and len(ref) == N_IT


_SUMMARY = ("termination", "iterations", "successful_steps", "initial_cost", "final_cost", "final_radius", "final_gradient_max_norm")


def test_run_to_convergence_twice_on_one_handle(ctx):
    """sfmhip_ba_run ends through a tolerance while a launch queued ahead is in flight; the parameters are read, then the handle runs again"""
    sc = synth.ba_scene(24, 4000)
    got = {}
    for seam in (0,) + SEAMS:
        pb = _create(ctx, _args(sc), seam, max_num_iterations=200)
        s1 = pb.run(); p1 = pb.params()
        s2 = pb.run(); p2 = pb.params()
        scal = pb.debug_table("step_scalars").tobytes()
        pb.close()
        got[seam] = ([s1[k] for k in _SUMMARY], p1, [s2[k] for k in _SUMMARY], p2, scal)
    s1 = dict(zip(_SUMMARY, got[0][0]))
    assert s1["termination"] == 0 and 3 <= s1["iterations"] < 200, s1        # converged: left through a tolerance, not the iteration limit
    for seam in SEAMS:
        assert got[seam][0] == got[0][0] and got[seam][2] == got[0][2] and got[seam][4] == got[0][4], (seam, got[seam][0], got[0][0], got[seam][2], got[0][2])
        for x, y in zip(got[seam][1] + got[seam][3], got[0][1] + got[0][3]):
            assert np.array_equal(x, y), seam


class _Masked:
    """ctx whose ba_create goes through sfmhip_ba_create_ex with the given masks"""

    def __init__(self, ctx, cam_const=None, pt_const=None):
        self.ctx, self.cam_const, self.pt_const, self.ba_options = ctx, cam_const, pt_const, ctx.ba_options

    def ba_create(self, *args, opts=None):
        return self.ctx.ba_create(*args, opts=opts, cam_const=self.cam_const, pt_const=self.pt_const)


@pytest.mark.parametrize("kw", [dict(fix_intrinsics=1), dict(fix_first_camera=0)])
def test_fixed_intrinsics_and_free_first_camera(ctx, kw):
    sc = synth.ba_scene(16, 3000)
    ref = _assert_bits_agree(ctx, _args(sc), **kw)
    assert ref[-1][3] >= 5


def test_constant_points(ctx):
    """ba_back_lin_const_kernel writes the second set"""
    sc = synth.ba_scene(16, 3000)
    const = np.zeros(3000, np.uint8); const[::7] = 1
    ref = _assert_bits_agree(_Masked(ctx, pt_const=const), _args(sc))
    assert ref[-1][3] >= 5


N_FAIL = 110


def test_a_point_block_that_is_not_positive_definite_at_the_candidate(ctx):
    """Forty points keep one observation: two residuals for three coordinates.  With next to no damping (radius 1e30, min_lm_diagonal
    1e-300) their blocks fail the Cholesky, the iteration is invalid and the radius halves until the damping carries the third
    direction.  The first step that works is accepted and its radius triples: back above where the blocks failed, so the point pass
    the back-substitution ran ahead at the candidate raises the flag of the second set.  That set is adopted, and the flag must make
    the NEXT iteration invalid, with the launch queued ahead as without it."""
    sc = synth.ba_scene(12, 2500)
    keep = np.ones(len(sc["obs_cam"]), bool)
    for p in range(40):
        keep[np.nonzero(sc["obs_pt"] == p)[0][1:]] = False
    args = (sc["K0"], sc["ext0"], sc["pts0"], sc["obs_cam"][keep], sc["obs_pt"][keep], sc["obs_uv"][keep])
    kw = dict(initial_trust_region_radius=1e30, min_lm_diagonal=1e-300)
    ref = _assert_bits_agree(ctx, args, patterns=((N_FAIL,), (2, 3, 1, 7, 5) * 6 + (2,)), n=N_FAIL, **kw)
    d = _decisions(ctx, ref, 1e30, **kw)
    # the condition: an adopted set whose flag was up (a step accepted with the guessed radius, the next iteration invalid)
    assert any(d[i][1] and d[i + 1][2] for i in range(N_FAIL - 1)), d
    assert ref[-1][3] >= 3 and ref[-1][0] < ref[0][0], ref[-1][:4]


def test_above_the_one_launch_size_nothing_is_queued_ahead(ctx):
    """Camera items and pair chunks on two streams (C5's form), reached on a small scene through the experiments build's size knob"""
    if not _experiments_build(ctx):
        pytest.skip("SFMHIP_FUSE_MAX_BLOCKS is read only by -DSFMHIP_EXPERIMENTS builds; no small scene exceeds the default 4096 workgroups")
    sc = synth.ba_scene(24, 4000)
    old = os.environ.get("SFMHIP_FUSE_MAX_BLOCKS")
    os.environ["SFMHIP_FUSE_MAX_BLOCKS"] = "0"
    try:
        _assert_bits_agree(ctx, _args(sc))
        pb = _create(ctx, _args(sc), None); pb.iterate(N_IT)
        assert list(pb.debug_table("speculation")) == [0, 0]
        pb.close()
    finally:
        if old is None:
            os.environ.pop("SFMHIP_FUSE_MAX_BLOCKS", None)
        else:
            os.environ["SFMHIP_FUSE_MAX_BLOCKS"] = old


def test_under_an_allreduce_hook_the_bit_changes_nothing(ctx):
    """world 1 with a hook installed: the multi-rank path, one collective per iteration whose speculative build is adopted"""
    sc = synth.ba_scene(24, 4000)
    counts = {}

    def hooked(key):
        def prep(pb):
            counts[key] = []
            pb.set_allreduce(lambda ptr, count, stream: counts[key].append(count) or 0, 0, 1)
        return prep

    ref = _reference(ctx, _args(sc), prep=hooked(0))
    for seam in SEAMS:
        for calls in ((N_IT,), MIXED):
            pb, out = _run(ctx, _args(sc), seam, calls, prep=hooked((seam, calls)))
            pb.close()
            _assert_follows(ref, calls, out, (seam, calls))
    # the hook is called as often, with the same message sizes, as with the switch at 0
    one = counts[(None, (N_IT,))]
    assert counts[(BIT, (N_IT,))] == one and len(one) >= N_IT
    ref_one = _run(ctx, _args(sc), 0, (N_IT,), prep=hooked("seam 0, one call"))[0]
    ref_one.close()
    assert counts["seam 0, one call"] == one
    assert counts[(None, MIXED)] == counts[(BIT, MIXED)]


def test_speculation_counters(ctx):
    """Experiments build: every eligible iteration queues its launch ahead, and on the all-accepted scene all are adopted"""
    if not _experiments_build(ctx):
        pytest.skip("the speculation counters exist only in -DSFMHIP_EXPERIMENTS builds of the library")
    sc = synth.ba_scene(24, 4000)
    for calls in ((N_IT,), (1, 2, 7) * 3):
        pb = _create(ctx, _args(sc), None)
        for n in calls:
            pb.iterate(n)
        eligible = sum(n - 1 for n in calls)           # all but a call's last iteration
        assert list(pb.debug_table("speculation")) == [eligible, eligible], calls
        pb.close()
    for seam in (BIT, 0, BIT | 4, BIT | 8):            # without bits 2 and 3 nothing is queued ahead
        pb = _create(ctx, _args(sc), seam); pb.iterate(N_IT)
        assert list(pb.debug_table("speculation")) == [0, 0], seam
        pb.close()
    # rejecting scene: launches that are not adopted, and none queued behind a step that missed its guess
    pb = _create(ctx, _rejecting_scene(), None, initial_trust_region_radius=1e6); pb.iterate(N_IT)
    launched, adopted = pb.debug_table("speculation")
    pb.close()
    ref = _reference(ctx, _rejecting_scene(), initial_trust_region_radius=1e6)
    d = _decisions(ctx, ref, 1e6, initial_trust_region_radius=1e6)
    expect_l = sum(1 for i in range(N_IT - 1) if i == 0 or d[i - 1][1])
    expect_a = sum(1 for i in range(N_IT - 1) if (i == 0 or d[i - 1][1]) and d[i][1])
    assert (launched, adopted) == (expect_l, expect_a) and adopted < launched, (launched, adopted, expect_l, expect_a)
