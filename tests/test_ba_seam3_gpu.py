"""SFMHIP_BA_SEAM bit 7 (128): a node's first pivot block factored under its assembly -- nodes with an assembly step (the
separators of chol_node_forward_kernel, chol_top_kernel) fold that block first, by all threads, and everything else beside wave 0's
factorisation.  The sums, their order and the factorisation are those of SFMHIP_BA_SEAM=0, so every comparison is for equality.
(The same overlap for leaves and chol_sparse_kernel, once bit 8, gained nothing measurable and was taken out with its bit:
profiles/README.md, round 20; the cases written for it stay, they cost milliseconds.)"""
import numpy as np
import pytest

from sfm_opencv_amd import synth
from test_ba_seam_gpu import N_IT, _args, _rejecting_scene
from test_ba_seam2_gpu import _assert_bits_agree

pytestmark = pytest.mark.gpu

SEAMS = (128, 4 | 128, None)


@pytest.mark.parametrize("shape,leaves", [((50, 20000), 2), ((24, 4000), None)])
def test_the_bit_alone_and_unset_against_none(ctx, shape, leaves):
    """50 cameras: two leaves and a top, the smallest plan with an assembling node."""
    sc = synth.ba_scene(*shape)
    t0, plans = _assert_bits_agree(ctx, _args(sc), SEAMS)
    assert t0[-1][3] >= 5        # accepted steps
    if leaves is not None:
        assert plans[None][0] == leaves and plans[None][2] >= 1, plans[None]


def test_separators_that_assemble_from_children(ctx):
    """400 cameras: sixteen leaves, two levels of separators below the top, each assembling from its children's update buffers.  The
    plan is read back, so the test cannot pass without such separators."""
    sc = synth.ba_scene(400, 40000)
    _, plans = _assert_bits_agree(ctx, _args(sc), SEAMS)
    leaves, levels, top_panels, _ = plans[None]
    assert leaves == 16 and levels >= 2 and top_panels >= 1, plans[None]


def test_one_workgroup_factors_the_whole_system(ctx):
    """12 cameras: chol_sparse_kernel has no assembly step, the switch must be inert there."""
    sc = synth.ba_scene(12, 2500)
    _, plans = _assert_bits_agree(ctx, _args(sc), SEAMS)
    assert plans[None][0] == 1 and plans[None][1] == 0, plans[None]


@pytest.mark.parametrize("kw", [dict(fix_intrinsics=1), dict(fix_first_camera=0)])
def test_fixed_intrinsics_and_free_first_camera(ctx, kw):
    sc = synth.ba_scene(16, 3000)
    _assert_bits_agree(ctx, _args(sc), SEAMS, **kw)


class _ConstantCameras:
    """ctx whose ba_create goes through sfmhip_ba_create_ex with the given camera mask"""

    def __init__(self, ctx, cam_const):
        self.ctx, self.cam_const, self.ba_options = ctx, cam_const, ctx.ba_options

    def ba_create(self, *args, opts=None):
        return self.ctx.ba_create(*args, opts=opts, cam_const=self.cam_const)


def test_constant_cameras_give_masked_rows_in_the_first_pivot_block(ctx):
    """sfmhip_ba_create_ex with cameras 2, 3 and 9 held constant: their rows are masked, so the damping sets their diagonal to 1.0
    in the first pivot block (cameras 2 and 3) and behind it (camera 9)."""
    sc = synth.ba_scene(16, 3000)
    const = np.zeros(16, np.uint8); const[[2, 3, 9]] = 1
    t0, _ = _assert_bits_agree(_ConstantCameras(ctx, const), _args(sc), SEAMS)
    assert t0[-1][3] >= 5


def test_rejected_steps_change_the_radius_between_solves(ctx):
    """The scene of test_ba_seam_gpu that rejects steps: the damping terms folded into the first pivot block change from solve to
    solve, also downwards."""
    args = _rejecting_scene()
    kw = dict(initial_trust_region_radius=1e6)
    t0, _ = _assert_bits_agree(ctx, args, SEAMS, **kw)
    assert N_IT - t0[-1][3] >= 1, t0[-1]        # the condition: at least one rejected step


N_FAIL = 100


@pytest.mark.parametrize("shape", [(12, 2500), (50, 20000)])
def test_a_first_pivot_block_that_is_not_positive_definite(ctx, shape):
    """Camera 1, the first free camera and so inside the first pivot block of the first leaf (50 cameras) or of the only node (12
    cameras), keeps two observations: four residuals for six parameters, a reduced block of rank four.  With next to no damping
    (radius 1e30, min_lm_diagonal 1e-300) that block's factorisation breaks down: the iteration is invalid, which halves the radius
    every time (ordinary rejections divide by 2, 4, 8, ...) and leaves the cost where it is, until the damping carries the two
    missing directions; then LM steps again.  The same iterations fail and the same recover under every switch value."""
    sc = synth.ba_scene(*shape)
    keep = np.ones(len(sc["obs_cam"]), bool)
    keep[np.nonzero(sc["obs_cam"] == 1)[0][2:]] = False
    args = (sc["K0"], sc["ext0"], sc["pts0"], sc["obs_cam"][keep], sc["obs_pt"][keep], sc["obs_uv"][keep])
    kw = dict(solver=1, initial_trust_region_radius=1e30, min_lm_diagonal=1e-300)
    t0, _ = _assert_bits_agree(ctx, args, SEAMS, n=N_FAIL, **kw)
    cost, radius, _, steps = map(np.array, zip(*t0))
    assert np.isfinite(cost).all() and np.isfinite(radius).all()
    # iterations 0 and 1 are invalid: no step, the cost unchanged, the radius halved twice
    assert steps[1] == 0 and cost[1] == cost[0] and radius[0] == 1e30 * 0.5 and radius[1] == 1e30 * 0.25, t0[:3]
    # and the iterations after the breakdown work
    assert steps[-1] >= 3 and cost[-1] < cost[0], t0[-1]
