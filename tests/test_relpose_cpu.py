"""CPU: the numpy restatement of the two-view relative pose (tests/relpose_ref.py) against independent code and against the truth of the
scenes, so that the GPU tests compare the library with something that is itself checked; and the C-ABI surface of the new calls."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import relpose_ref as rp
import twoview_ref as tv
from sfm_opencv_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["sfmhip_relative_pose", "sfmhip_relative_pose_dev"]

# Two optimisers on the same residual and set stop at different points of a flat minimum.  Measured over the 18 inputs: the largest angle
# between the restatement's refined pose and scipy's least_squares(method="lm") from the same start is 2.307e-07 rad in the rotation
# and 1.552e-06 rad in the baseline direction; the tolerance is ten times that.
SCIPY_ROT_TOL = 10 * 2.307e-07
SCIPY_DIR_TOL = 10 * 1.552e-06
# The restatement against itself with its rows in another order (reversed, three shuffles): measured 4.062e-10 rad in the rotation and
# 2.857e-09 rad in the baseline direction over the 18 inputs.  test_relpose_gpu.py allows the library 100 times these.
ORDER_ROT_SPREAD = 4.062e-10
ORDER_DIR_SPREAD = 2.857e-09


def _refined(case):
    a = rp.ransac_input(*case)
    key = ("refined",) + tuple(case)
    if key not in rp._cache:
        rp._cache[key] = rp.relative_pose_pair(a["rows"], len(a["rows"]), a["mask"], a["F"], rp.THR)
    return a, rp._cache[key]


@pytest.mark.parametrize("case", rp.CASES18[::3] + rp.CASES18[1::3] + rp.CASES18[2::3])
def test_candidates_match_numpy_svd(case):
    a = rp.ransac_input(*case)
    ok, cands, sv = rp.candidates(a["F"])
    assert ok
    U, S, Vt = np.linalg.svd(a["F"].reshape(3, 3))
    assert np.allclose(sv, S, rtol=1e-12, atol=1e-15)
    if np.linalg.det(U) < 0: U = -U
    if np.linalg.det(Vt) < 0: Vt = -Vt
    W = np.array([[0.0, 1, 0], [-1, 0, 0], [0, 0, 1]])
    want_R = [U @ W @ Vt, U @ W.T @ Vt]
    # the singular vectors of a matrix with distinct singular values are determined up to the sign of (u_j, v_j) together, and flipping
    # pair 0 or 1 turns Ra into Rb: as SETS the two rotations and the baseline up to sign must agree
    got_R = [np.array(cands[0][0]).reshape(3, 3), np.array(cands[1][0]).reshape(3, 3)]
    for R in got_R:
        assert abs(np.linalg.det(R) - 1) < 1e-12 and np.allclose(R @ R.T, np.eye(3), atol=1e-12)
        assert min(rp.rotation_angle(R, w) for w in want_R) < 1e-9
    assert rp.rotation_angle(got_R[0], got_R[1]) > 1.0
    t = np.array(cands[0][1])
    assert min(np.abs(t - U[:, 2]).max(), np.abs(t + U[:, 2]).max()) < 1e-9
    assert cands[2][0] == cands[0][0] and cands[3][0] == cands[1][0] and cands[2][1] == [-x for x in t] and cands[1][1] == cands[0][1]


def test_jacobi_svd_on_rank_two_and_scaled_matrices():
    rng = np.random.default_rng(5)
    for k in range(20):
        M = rng.standard_normal((3, 3)) * 10.0 ** rng.integers(-6, 6)
        if k % 2:
            M[:, 2] = 0.3 * M[:, 0] - 2.0 * M[:, 1]                   # rank two: the completed third left vector
        u, v, s = (np.array(x) for x in rp.jacobi_svd3(M.reshape(9)))
        assert s[0] >= s[1] >= s[2] >= 0
        assert np.allclose(s, np.linalg.svd(M, compute_uv=False), rtol=1e-10, atol=1e-12 * s[0])
        assert np.allclose(u @ np.diag(s) @ v.T, M, rtol=0, atol=1e-12 * s[0])
        assert np.allclose(u.T @ u, np.eye(3), atol=1e-9) and np.allclose(v.T @ v, np.eye(3), atol=1e-12)


def test_analytic_jacobian_against_differences():
    a = rp.ransac_input(300, 0.3, 1)
    rows = a["rows"][a["mask"] != 0]
    R, t = rp.TRUE_R, rp.TRUE_T
    r, J = rp.jacobian(R, t, rows)
    for k in range(5):
        d = np.zeros(5); d[k] = 1e-6
        Rp, tp = rp.apply_step(R, t, d); Rm, tm = rp.apply_step(R, t, -d)
        num = (rp.residuals(Rp, tp, rows) - rp.residuals(Rm, tm, rows)) / 2e-6
        assert np.abs(num - J[:, k]).max() <= 1e-6 * np.abs(J[:, k]).max(), k


@pytest.mark.parametrize("case", rp.CASES18)
def test_refined_pose_against_scipy_and_the_truth(case):
    from scipy.optimize import least_squares
    a, got = _refined(case)
    m = len(a["rows"])
    assert got["info"][0] == 1
    R, t = got["pose"][:9].reshape(3, 3), got["pose"][9:]
    # (a) scipy on the same residual and the same set, the one the last round ran over
    two = rp.relative_pose_pair(a["rows"], m, a["mask"], a["F"], rp.THR, rounds=2)
    R2, t2 = two["pose"][:9].reshape(3, 3), two["pose"][9:]
    rows = a["rows"][tv.inliers(np.array(rp.essential(R2.reshape(9), t2)), a["rows"], rp.THR ** 2)[0]]
    b1, b2 = rp.tangent_basis(t2)

    def moved(d):
        tn = t2 + d[3] * b1 + d[4] * b2
        return rp.rot_exp(d[:3]) @ R2, tn / np.linalg.norm(tn)

    sol = least_squares(lambda d: rp.residuals(*moved(d), rows), np.zeros(5), method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15)
    Rs, ts = moved(sol.x)
    rot, dirn = rp.rotation_angle(Rs, R), rp.direction_angle(ts, t)
    print(f"{case}: scipy rot {rot:.3e} dir {dirn:.3e} rad")
    assert rot <= SCIPY_ROT_TOL and dirn <= SCIPY_DIR_TOL, (case, rot, dirn)
    # (b) the truth of the scene
    rot, dirn = math.degrees(rp.rotation_angle(R, rp.TRUE_R)), math.degrees(rp.direction_angle(t, rp.TRUE_T))
    inl = (got["mask_out"] & 1).astype(bool)
    kept, wrong = (inl & a["good"]).sum() / a["good"].sum(), int((inl & ~a["good"]).sum())
    print(f"{case}: truth rot {rot:.3f} dir {dirn:.3f} deg, n_inl {got['info'][7]} (RANSAC {a['count']}), kept {kept:.3f}, wrong {wrong}")
    assert rot <= 0.5 and dirn <= 3.0, (case, rot, dirn)
    assert got["info"][7] == inl.sum() and got["info"][7] > a["count"], (case, got["info"], a["count"])
    assert kept >= 0.9 and wrong <= 0.02 * got["info"][7], (case, kept, wrong)
    assert got["quality"][4] <= got["quality"][3] and got["info"][6] == a["count"]
    assert got["info"][9] <= got["info"][8] <= got["info"][7] and set(np.unique(got["mask_out"])) <= {0, 1, 3, 7}


def test_row_order_spread_is_the_recorded_one():
    rot = dirn = 0.0
    for case in rp.CASES18:
        a, base = _refined(case)
        m = len(a["rows"])
        rng = np.random.default_rng(100 + case[2])
        for order in [np.arange(m)[::-1]] + [rng.permutation(m) for _ in range(3)]:
            g = rp.relative_pose_pair(a["rows"], m, a["mask"], a["F"], rp.THR, order=order)
            rot = max(rot, rp.rotation_angle(g["pose"][:9], base["pose"][:9])); dirn = max(dirn, rp.direction_angle(g["pose"][9:], base["pose"][9:]))
    print(f"spread over five row orders: rot {rot:.3e} dir {dirn:.3e} rad")
    assert rot <= 1.0001 * ORDER_ROT_SPREAD and dirn <= 1.0001 * ORDER_DIR_SPREAD, (rot, dirn)


def test_every_candidate_wins_somewhere():
    inputs = rp.cand_inputs()
    assert {c[3] for c in inputs} == {0, 1, 2, 3}, [(c[3], c[4]) for c in inputs]
    for rows, mask, F, cand, what in inputs:
        got = rp.relative_pose_pair(rows, len(rows), mask, F, rp.THR, rounds=0, iters=0)
        n4 = got["info"][2:6]
        assert got["info"][0] == 1 and n4[cand] == n4.max() and n4[cand] >= 0.9 * got["info"][6], (what, got["info"])


def test_no_pose_values():
    a = rp.ransac_input(300, 0.3, 1)
    rows, mask = a["rows"], a["mask"]
    seven = np.zeros(300, np.uint8); seven[np.flatnonzero(mask)[:7]] = 1
    bad_F = a["F"].copy(); bad_F[4] = np.nan
    for got, n_used in ((rp.relative_pose_pair(rows, 300, seven, a["F"], rp.THR), 7), (rp.relative_pose_pair(rows, 300, mask, bad_F, rp.THR), a["count"]),
                        (rp.relative_pose_pair(rows, 300, mask, np.zeros(9), rp.THR), a["count"]),
                        (rp.relative_pose_pair(rows, 300, mask, a["F"], rp.THR, max_depth=1.0), a["count"])):
        assert np.isnan(got["pose"]).all() and np.isnan(got["quality"]).all() and not got["mask_out"].any()
        assert got["info"].tolist() == [0, -1, 0, 0, 0, 0, n_used, 0, 0, 0]


def test_c_abi_surface():
    assert all(s in _lib.SYMBOLS for s in NEW_SYMBOLS)
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.strip()}
    assert all(s in exported for s in NEW_SYMBOLS), sorted(set(NEW_SYMBOLS) - exported)
    lib = _lib.load()
    for s in NEW_SYMBOLS:
        assert getattr(lib, s).argtypes is not None
    hdr = open(os.path.join(ROOT, "include", "sfmhip.h")).read()
    assert all(f"int {s}" in hdr for s in NEW_SYMBOLS)
    # without a context the calls are argument errors, not crashes
    assert lib.sfmhip_relative_pose(None, None, 0, None, 0, None, None, 0.1, 3, 10, 50.0, 0.03, None, None, None, None) == _lib.E_ARG
