"""CPU: constant parameter blocks in bundle adjustment (sfmhip_ba_create_ex / _solve_ex / _solve_multi_ex).

The C-ABI and the Python keywords exist, and the dense test-side reference (tests/ba_dense_ref.py) that the GPU tests compare
against reproduces the oracle wherever the oracle can express the problem: default options, fixed intrinsics, no constant camera,
and a constant camera k != 0 (given to the oracle as camera 0 after swapping k and 0).  Tolerances are those of the GPU-vs-oracle
tests (tests/test_ba_gpu.py): after 6 forced steps 1e-8 relative on the cost and 1e-6 x scene scale on the parameters (10 for
points / extrinsics, 3000 for the intrinsics); to convergence the same iteration count and termination, cost within 1e-6."""
import inspect
import os
import re

import numpy as np
import pytest

import oracle as orc
from sfm_opencv_amd import _lib, api, synth
from ba_dense_ref import dense_ba, fixed_cost, obs_costs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sfmhip_ba_create_ex", "sfmhip_ba_solve_ex", "sfmhip_ba_solve_multi_ex")


def _args(sc):
    return sc["K0"], sc["ext0"], sc["pts0"], sc["obs_cam"], sc["obs_pt"], sc["obs_uv"]


def test_new_entry_points_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "sfmhip.h")).read()
    declared = set(re.findall(r"\b(sfmhip_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    for s in NEW:
        assert s in declared, s
        assert hasattr(lib, s), s
        assert s in _lib.SYMBOLS, s
    # the masks travel as (const uint8_t* cam_const, const uint8_t* pt_const) right before the options
    for s in NEW:
        m = re.search(s + r"\s*\(([^;]*)\);", hdr, re.S)
        assert m and re.search(r"const uint8_t\* cam_const,\s*const uint8_t\* pt_const,\s*const sfm_ba_options\*", m.group(1)), s


def test_python_keywords():
    for fn in (api.Context.ba_create, api.Context.ba_solve, api.ba_solve_multi, api.BAProblem.__init__):
        p = inspect.signature(fn).parameters
        assert p["cam_const"].default is None and p["pt_const"].default is None, fn
    p = inspect.signature(api.bundle_adjustment).parameters
    assert p["const_cameras"].default is None and p["const_points"].default is None


def test_mask_helpers():
    assert api._const_mask(None, 3) is None
    m = api._const_mask([True, False, 1], 3)
    assert m.dtype == np.uint8 and list(m) == [1, 0, 1]
    with pytest.raises(ValueError):
        api._const_mask([1, 0], 3)
    assert list(api._index_mask([2, 0], 4)) == [1, 0, 1, 0]
    with pytest.raises(ValueError):
        api._index_mask([4], 4)


def _check_forced(mine, ref):
    K, e, p, s = mine
    Ko, eo, po, so = ref[:4]
    assert s["iterations"] == so["iterations"] == 6
    assert s["successful_steps"] == so["successful_steps"]
    assert abs(s["final_cost"] - so["final_cost"]) <= 1e-8 * so["final_cost"]
    assert np.abs(p - po).max() <= 1e-6 * 10.0
    assert np.abs(e - eo).max() <= 1e-6 * 10.0
    assert np.abs(K - Ko).max() <= 1e-6 * 3000.0


def _check_converged(mine, ref):
    s, so = mine[3], ref[3]
    assert s["termination"] == so["termination"]
    assert s["iterations"] == so["iterations"]
    assert abs(s["final_cost"] - so["final_cost"]) <= 1e-6 * so["final_cost"]


@pytest.mark.parametrize("kw", [dict(), dict(fix_intrinsics=1), dict(fix_first_camera=0)])
def test_dense_reference_matches_oracle(kw):
    sc = synth.ba_scene(8, 400)
    o = orc.ba_default_options(**kw)
    _check_forced(dense_ba(*_args(sc), opts=o, force_iterations=6), orc.ba_solve(*_args(sc), opts=o, force_iterations=6))
    _check_converged(dense_ba(*_args(sc), opts=o), orc.ba_solve(*_args(sc), opts=o))


def test_dense_reference_constant_camera_k_matches_relabelled_oracle():
    sc = synth.ba_scene(8, 400)
    k = 5
    cm = np.zeros(8, bool); cm[k] = True
    perm = np.arange(8); perm[[0, k]] = perm[[k, 0]]
    swapped = (sc["K0"], sc["ext0"][perm], sc["pts0"], perm[sc["obs_cam"]].astype(np.int32), sc["obs_pt"], sc["obs_uv"])
    for f in (6, 0):
        K, e, p, s = dense_ba(*_args(sc), opts=orc.ba_default_options(fix_first_camera=0), cam_const=cm, force_iterations=f)
        Ko, eo, po, so, _ = orc.ba_solve(*swapped, opts=orc.ba_default_options(), force_iterations=f)
        assert np.array_equal(e[k], sc["ext0"][k])
        if f:
            _check_forced((K, e, p, s), (Ko, eo[perm], po, so))
        else:
            _check_converged((K, e, p, s), (Ko, eo[perm], po, so))


def test_dense_reference_fixed_cost_contract():
    """fixed intrinsics + constant cameras + constant points: the fully constant observations leave the loop, their cost is
    added to both reported costs, and dropping them from the input gives the same trajectory net of that cost"""
    sc = synth.ba_scene(6, 200)
    rng = np.random.default_rng(3)
    cm = np.zeros(6, bool); cm[[0, 1, 2]] = True
    pm = rng.random(200) < 0.3
    o = orc.ba_default_options(fix_intrinsics=1)
    K, e, p, s = dense_ba(*_args(sc), opts=o, cam_const=cm, pt_const=pm, force_iterations=4)
    dead = cm[sc["obs_cam"]] & pm[sc["obs_pt"]]
    assert dead.any()
    fc = fixed_cost(sc["K0"], sc["ext0"], sc["pts0"], sc["obs_cam"], sc["obs_pt"], sc["obs_uv"], cm, pm)
    vc = obs_costs(sc["K0"], sc["ext0"], sc["pts0"], sc["obs_cam"][dead], sc["obs_pt"][dead], sc["obs_uv"][dead]).sum()
    assert abs(fc - vc) <= 1e-12 * fc and s["fixed_cost"] == fc
    assert np.array_equal(e[cm], sc["ext0"][cm]) and np.array_equal(p[pm], sc["pts0"][pm]) and np.array_equal(K, sc["K0"])
    keep = ~dead
    K2, e2, p2, s2 = dense_ba(sc["K0"], sc["ext0"], sc["pts0"], sc["obs_cam"][keep], sc["obs_pt"][keep], sc["obs_uv"][keep],
                              opts=o, cam_const=cm, pt_const=pm, force_iterations=4)
    assert s2["fixed_cost"] == 0.0
    assert abs((s["final_cost"] - fc) - s2["final_cost"]) <= 1e-12 * s2["final_cost"]
    assert np.array_equal(p, p2) and np.array_equal(e, e2)
