"""GPU: every reduced-camera solver selection under the all-reduce hook, and the rest of the chain solver's gate.

Under a hook the ranks exchange the packed message of ba_pack_kernel: the 32x32 blocks of S with block row >= block column.  After the
unpack every entry in a block above the block diagonal still holds the rank's LOCAL partial sum, so a solver that used one would
solve another system on every rank.  The hooked tests of tests/test_ba_gpu.py run band-5 scenes (nested dissection) or masked ones;
here the same comparison -- point shards on one card against the unsharded run, the bars of
test_two_point_shards_on_one_gpu_match_unsharded and test_multi_context_solve_follows_the_single_gpu_steps -- runs on what they do
not reach: band-3 scenes (the chain solver of csrc/ba_chain.hpp, held to the carried part of S by the poisoned solve of
tests/host/chain_emu_test.cpp), the one-workgroup sparse solver and the dense blocked fallback.  Every test asserts the solver named
by the library's verbose line, so none can pass through a silent change of the selection.

Unhooked: the chain solver between 200 and 640 free cameras (32 leaves) against solver = 1 and the oracle with the bars of
test_chain_solver_on_narrow_bands, and the edges of its gate (12..640 free cameras)."""
import ctypes as C
import re

import numpy as np
import pytest

import oracle as orc
from sfm_opencv_amd import api, synth
from test_ba_gpu import _args, _relerr, _run_sharded_on_one_gpu

pytestmark = pytest.mark.gpu

CHAIN = "chain (fronts in LDS)"
SPARSE = "one workgroup, sparse panels"
DENSE = "dense blocked"


def _captured(capfd):
    C.CDLL(None).fflush(None)                 # the library's printf buffer, when stdout is not a terminal
    return capfd.readouterr().out


def _plans(txt):
    """(free cameras, solver) of every '[sfmhip_ba] reduced system: ...' line"""
    return [(int(m.group(1)), m.group(2).strip())
            for m in re.finditer(r"\[sfmhip_ba\] reduced system: \d+ unknowns \((\d+) free cameras, band \d+ cameras\); solver: ([^\n]*)", txt)]


def _two_shards_against_unsharded(ctx, capfd, sc, kw, solver):
    ref = ctx.ba_create(*_args(sc), opts=ctx.ba_options(**kw))
    sr = ref.iterate(5); Kr, extr, ptsr = ref.params()
    ref.close()
    capfd.readouterr()
    out, params, ids, counts = _run_sharded_on_one_gpu(sc, 5, opts_of_rank=lambda r: dict(verbose=1, **kw))
    plans = _plans(_captured(capfd))
    # every rank planned (once or more) and every plan names the expected solver
    assert len(plans) >= 2 and all(p[1] == solver for p in plans), plans
    assert counts[0] == counts[1] and len(counts[0]) >= 3 + 1 + 5, counts     # both ranks make the same sequence of collectives
    for r in range(2):
        K, ext, pts = params[r]
        print("rank %d: cost %.3e (rel), ext %.3e, K %.3e (of scale), points %.3e" % (
            r, abs(out[r]["final_cost"] - sr["final_cost"]) / sr["final_cost"], np.abs(ext - extr).max(),
            np.abs(K - Kr).max() / np.abs(Kr).max(), np.abs(pts - ptsr[ids[r]]).max()))
    for r in range(2):
        assert out[r]["iterations"] == sr["iterations"] and out[r]["successful_steps"] == sr["successful_steps"]
        assert abs(out[r]["final_cost"] - sr["final_cost"]) <= 1e-9 * sr["final_cost"]
        K, ext, pts = params[r]
        assert np.abs(ext - extr).max() <= 1e-9 and np.abs(K - Kr).max() <= 1e-9 * np.abs(Kr).max()
        assert np.abs(pts - ptsr[ids[r]]).max() <= 1e-9
    return plans


# 16 cameras: one launch.  61, no constant camera: 61 free cameras, the camera x intrinsics coupling of every one of them above the
# block diagonal.  200: 16 leaves, tree levels in the second kernel (whose staging reads the separators' coupling).  30 with the
# intrinsics held: the control, a solve without the border.
@pytest.mark.parametrize("shape,kw", [((16, 1500), dict()), ((61, 9000), dict(fix_first_camera=0)), ((200, 30000), dict()),
                                       ((30, 4000), dict(fix_intrinsics=1))])
def test_two_point_shards_take_the_chain_solver_and_match_unsharded(ctx, capfd, shape, kw):
    """Five forced iterations on band-3 scenes, two point shards whose hook sums the packed messages, against the unsharded run."""
    sc = synth.ba_scene(*shape, max_len=4)
    plans = _two_shards_against_unsharded(ctx, capfd, sc, kw, CHAIN)
    assert all(p[0] == shape[0] - kw.get("fix_first_camera", 1) for p in plans), plans


def test_three_contexts_take_the_chain_solver_and_follow_the_single_gpu_steps(ctx, capfd):
    """sfmhip_ba_solve_multi over three contexts on a band-3 scene with free intrinsics: five LM steps with every tolerance switched
    off against sfmhip_ba_solve, 1e-9 on the cost and on every parameter; a second call on the same contexts bit for bit."""
    sc = synth.ba_scene(61, 9000, max_len=4)
    tol = dict(max_num_iterations=5, function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0)
    Kr, extr, ptsr, sr = ctx.ba_solve(*_args(sc), opts=ctx.ba_options(**tol))
    ctxs = [api.Context(0, use_torch_stream=False) for _ in range(3)]
    capfd.readouterr()
    o = ctx.ba_options(verbose=1, **tol)
    K, ext, pts, s = api.ba_solve_multi(ctxs, *_args(sc), opts=o)
    K2, ext2, pts2, s2 = api.ba_solve_multi(ctxs, *_args(sc), opts=o)
    plans = _plans(_captured(capfd))
    for c in ctxs:
        c.close()
    assert len(plans) >= 2 * 3 and all(p == (60, CHAIN) for p in plans), plans
    print("cost %.3e (rel), ext %.3e, K %.3e, points %.3e" % (abs(s["final_cost"] - sr["final_cost"]) / sr["final_cost"],
                                                               _relerr(ext, extr), _relerr(K, Kr), _relerr(pts, ptsr)))
    assert sr["iterations"] == s["iterations"] == 5 and s["successful_steps"] == sr["successful_steps"]
    assert abs(s["final_cost"] - sr["final_cost"]) <= 1e-9 * sr["final_cost"]
    assert _relerr(ext, extr) <= 1e-9 and _relerr(K, Kr) <= 1e-9 and _relerr(pts, ptsr) <= 1e-9
    assert np.array_equal(ext, ext2) and np.array_equal(pts, pts2) and np.array_equal(K, K2)


def test_two_point_shards_take_the_one_workgroup_solver_and_match_unsharded(ctx, capfd):
    """11 free cameras, band 5: below the chain solver's and the nested dissection's sizes."""
    _two_shards_against_unsharded(ctx, capfd, synth.ba_scene(12, 2500), dict(), SPARSE)


# 40 cameras and 3000 points are the scene of test_non_chain_tracks_take_the_dense_solver_and_match_oracle.  Its 238 unknowns are 8
# block rows, which the one-workgroup solver still takes (at most SRMAX = 8 blocks below a panel), whatever that test's name says; the
# dense blocked fallback starts where a full pattern has more: 56 cameras, 334 unknowns, 11 block rows.
@pytest.mark.parametrize("n_cam,n_pt,solver", [(40, 3000, SPARSE), (56, 4000, DENSE)])
def test_two_point_shards_of_non_chain_tracks_match_unsharded(ctx, capfd, n_cam, n_pt, solver):
    """Tracks through arbitrary (non-consecutive) cameras, re-drawn as in test_non_chain_tracks_take_the_dense_solver_and_match_oracle:
    the reduced system has no band at all."""
    rng = np.random.default_rng(17)
    sc = synth.ba_scene(n_cam, n_pt)
    L = np.bincount(sc["obs_pt"], minlength=sc["n_pt"])
    obs_pt = np.repeat(np.arange(sc["n_pt"]), L)
    obs_cam = np.concatenate([rng.choice(sc["n_cam"], l, replace=False) for l in L])
    uv = synth.project(sc["K_true"], sc["ext_true"][obs_cam], sc["pts_true"][obs_pt]) + 0.5 * rng.standard_normal((obs_pt.size, 2))
    order = np.lexsort((obs_pt, obs_cam))
    sc = dict(sc, obs_cam=obs_cam[order].astype(np.int32), obs_pt=obs_pt[order].astype(np.int32), obs_uv=np.ascontiguousarray(uv[order]))
    _two_shards_against_unsharded(ctx, capfd, sc, dict(), solver)


# ------------------------------------------------------------------------------------------------
# the chain solver above 200 free cameras (32 leaves, three tree levels in the second kernel), no hook
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,kw,oracle", [((300, 36000), dict(), True), ((640, 64000), dict(), False)])
def test_chain_solver_up_to_the_end_of_its_range(ctx, capfd, shape, kw, oracle):
    """Five forced steps, solver = 0 twice and solver = 1 once: 1e-11 on the cost and 1e-10 on the parameters between the two
    solvers, the two solver = 0 runs bit for bit; at 300 cameras also the oracle (1e-8 on the cost).

    Camera 0 is constant as by default (299 and 639 free cameras); a step at exactly 640 free cameras is part of
    test_chain_solver_gate_edges.  Without a constant camera the bar between the two solvers is not one the pair can be held to at this
    length -- the gauge is held by the damping alone and the three implementations part at the rounding level.  Measured on an MI355X,
    640 cameras and 64000 points, fix_first_camera = 0, relative difference of the final cost: chain solver against oracle 4.4e-12,
    solver 1 against oracle 3.9e-11, chain solver against solver 1 3.4e-11 (points 9.3e-11); with camera 0 constant 2.1e-12, 2.6e-14
    and 2.1e-12 (points 3.7e-11)."""
    sc = synth.ba_scene(*shape, max_len=4)
    runs = {}
    for solver in (0, 0, 1):
        capfd.readouterr()
        pb = ctx.ba_create(*_args(sc), opts=ctx.ba_options(solver=solver, verbose=1, **kw))
        s = pb.iterate(5)
        runs.setdefault(solver, []).append((s, pb.params()))
        pb.close()
        plans = _plans(_captured(capfd))
        assert len(plans) == 1 and plans[0][0] == shape[0] - kw.get("fix_first_camera", 1), plans
        assert (plans[0][1] == CHAIN) == (solver == 0), plans
    (s0, p0), (s0b, p0b) = runs[0]
    (s1, p1), = runs[1]
    print("cost %.3e (rel), parameters %s" % (abs(s0["final_cost"] - s1["final_cost"]) / s1["final_cost"], ["%.3e" % _relerr(x, y) for x, y in zip(p0, p1)]))
    assert s0["iterations"] == s1["iterations"] == 5 and s0["successful_steps"] == s1["successful_steps"]
    if oracle:
        so = orc.ba_solve(*_args(sc), force_iterations=5, opts=orc.ba_default_options(**kw))[3]
        print("cost against the oracle %.3e (rel)" % (abs(s0["final_cost"] - so["final_cost"]) / so["final_cost"]))
        assert s0["iterations"] == so["iterations"] and s0["successful_steps"] == so["successful_steps"]
        assert abs(s0["final_cost"] - so["final_cost"]) <= 1e-8 * so["final_cost"]
    assert abs(s0["final_cost"] - s1["final_cost"]) <= 1e-11 * s1["final_cost"]
    for x, y in zip(p0, p1):
        assert _relerr(x, y) <= 1e-10
    for x, y in zip(p0, p0b):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("n_cam,n_pt,fix_first,chain", [(12, 1200, 0, True), (12, 1200, 1, False), (641, 64000, 1, True), (641, 64000, 0, False)])
def test_chain_solver_gate_edges(ctx, capfd, n_cam, n_pt, fix_first, chain):
    """solver = 0 on a band-3 scene takes the chain solver from 12 to 640 free cameras and not at 11 or 641."""
    sc = synth.ba_scene(n_cam, n_pt, max_len=4)
    capfd.readouterr()
    pb = ctx.ba_create(*_args(sc), opts=ctx.ba_options(solver=0, verbose=1, fix_first_camera=fix_first))
    s = pb.iterate(1)
    pb.close()
    plans = _plans(_captured(capfd))
    assert len(plans) == 1 and plans[0][0] == n_cam - fix_first, plans
    assert (plans[0][1] == CHAIN) == chain, plans
    assert np.isfinite(s["final_cost"]) and s["final_cost"] < s["initial_cost"]
