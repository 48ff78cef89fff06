"""CPU: the references of tests/geometry_ref.py and the inputs of the GPU geometry tests, validated against the oracle, so that
tests/test_triangulate_edges_gpu.py and tests/test_normals_fit_gpu.py cannot fail because of their own yardstick.

For every case the oracle's deviation from the independent reference is printed (pytest -s) and the preconditions the GPU tests rely on
are asserted: the conditioning of the two-view cases, the constant c of their bound, the rank deficiency of the tracks that are compared
with the oracle only, and the oracle's own Rayleigh excess on every finite cloud.  Measured here (oracle vs reference only):

  two-view   sigma1 / (sigma3 - sigma4) from 2.7 (b1_d10, b1_d1000, b1_d1e4: a far point is a well-defined HOMOGENEOUS vector) to 2.3e3
             (b0.001_d10); on every sampled row the oracle's float32 null vector is the correctly rounded reference vector, i.e. it
             needs c = 0 (geometry_ref.C_TWO_VIEW_MEASURED): its fp64 error, at most eps64 sigma1 / gap ~ 5e-13, only shows where the
             reference lies that close to a float32 rounding boundary, and no sampled component does
  tracks     relative deviation of the oracle from the mpmath DLT of the unsquared system: 1.9e-16 (mixed_1) .. 3.4e-14 (mixed_256),
             7.7e-16 (b1_d10_c40), 1.3e-12 (b0.01_d10_c2), 5.9e-12 (b0.01_d10_c40), 1.2e-13 (b1_d1000_c3)
  reproj     1.5e-14 (n_obs = 1) .. 4.3e-13 (256) against max(err, 1): a few roundings of a pixel coordinate of some thousands
  normals    Rayleigh excess of the oracle at most 3.1 eps scale (lattice8), | |n| - 1 | at most 1.1 eps, no sign violation"""
import numpy as np
import pytest

import geometry_ref as gr
import oracle as orc

EPS = gr.EPS64


# ---------------------------------------------------------------------------------------------------------------- two views
@pytest.mark.parametrize("geom,n", gr.two_view_cases())
def test_two_view_case_is_well_conditioned_and_the_oracle_meets_the_bound(geom, n):
    s, rows, v, sig = gr.two_view_reference(geom, n)
    assert len(rows) <= 100 and rows[0] == 0 and rows[-1] == n - 1
    kappa = sig[:, 0] / (sig[:, 2] - sig[:, 3])
    assert kappa.max() <= 1e5, (geom, n, kappa.max())
    assert np.abs(np.linalg.norm(v, axis=1) - 1).max() <= 4 * EPS
    ow, ox = orc.triangulate2(s["P1"], s["P2"], s["xy1"], s["xy2"])
    need = gr.two_view_needed_c(ow[:, rows].T, v, sig)
    sgn = np.sign((ow[:, rows].T * v).sum(1, keepdims=True))
    print(f"[two-view] {geom} n={n}: kappa max {kappa.max():.3g}, oracle needs c = {need.max():.3g}, "
          f"|h - v_ref| max {np.abs(ow[:, rows].T * sgn - v).max():.3g}")
    assert need.max() <= gr.C_TWO_VIEW_MEASURED
    assert (np.abs(ow[:, rows].T * sgn - v) <= gr.two_view_bound(v, sig)).all()
    # store_point's restatement in numpy reproduces the oracle's xyz from the oracle's xyzw
    assert gr.same_bits(gr.dehomogenise_f32(ow), ox)
    # the triangulated points are the scene's (noise-free cases; a point at depth 1e4 seen over a baseline of 1 moves by float32 pixels)
    if gr.TWO_VIEW_GEOMETRIES[geom][2] == 0.0 and geom.endswith("d10_clean"):
        assert np.abs(ox - s["X"]).max() < 1e-2


@pytest.mark.parametrize("geom", list(gr.TWO_VIEW_GEOMETRIES))
def test_two_view_reference_agrees_with_lapack(geom):
    """the mpmath null vector against numpy.linalg.svd of the same system in fp64, to the perturbation bound of a stable SVD"""
    s, rows, v, sig = gr.two_view_reference(geom, 513)
    for o, i in enumerate(rows[::10]):
        o *= 10
        A = np.empty((4, 4))
        for j, (P, xy) in enumerate(((s["P1"], s["xy1"]), (s["P2"], s["xy2"]))):
            P = P.astype(np.float64); x, y = xy[i].astype(np.float64)
            A[2 * j] = x * P[2] - P[0]; A[2 * j + 1] = y * P[2] - P[1]
        _, S, Vt = np.linalg.svd(A)
        w = Vt[3] * np.sign(Vt[3] @ v[o])
        assert np.abs(S[:3] - sig[o, :3]).max() <= 16 * EPS * S[0]
        assert np.abs(w - v[o]).max() <= 16 * EPS * sig[o, 0] / (sig[o, 2] - sig[o, 3])


def test_two_view_degenerate_inputs_are_what_they_claim():
    cases = gr.two_view_degenerate()
    assert set(cases) == {"identical_cameras", "identical_cameras_and_pixels", "zero_P2", "pixel_1e6", "nan_pixel"}
    s = cases["nan_pixel"]
    ow, ox = orc.triangulate2(s["P1"], s["P2"], s["xy1"], s["xy2"])
    bad = ~(np.isfinite(s["xy1"]).all(1) & np.isfinite(s["xy2"]).all(1))
    assert bad.sum() == 4 and np.isnan(ox[[0, 256]]).all() and np.isfinite(ox[~bad]).all()
    # what include/sfmhip.h says about systems without a one-dimensional null space: a finite unit xyzw, xyz inf where w is 0
    for name in ("zero_P2", "identical_cameras", "identical_cameras_and_pixels"):
        s = cases[name]
        ow, ox = orc.triangulate2(s["P1"], s["P2"], s["xy1"], s["xy2"])
        assert np.isfinite(ow).all() and np.abs(np.linalg.norm(ow.astype(np.float64), axis=0) - 1).max() < 1e-6 and not np.isnan(ox).any()
        assert np.array_equal(np.isinf(ox).any(1), ow[3] == 0)
    assert not cases["zero_P2"]["P2"].any() and np.array_equal(cases["identical_cameras"]["P1"], cases["identical_cameras"]["P2"])


# ---------------------------------------------------------------------------------------------------------------- tracks
@pytest.mark.parametrize("name", gr.track_cases())
def test_tracks_oracle_deviation_and_rank(name):
    sc, pick, v, x, sig = gr.track_reference(name)
    assert len(pick) <= 40
    opts, onv = orc.triangulate_tracks(*gr.track_args(sc))
    assert np.array_equal(onv, sc["n_views"])
    assert np.array_equal(np.isnan(opts).all(1), sc["n_views"] < 2) and np.array_equal(np.isnan(opts).any(1), sc["n_views"] < 2)
    eq = np.isin(pick, sc["equality_only"])
    # a track compared with the oracle only really is rank deficient, and no other track is
    assert (sig[eq, 2] / sig[eq, 0] < 1e-12).all()
    assert (sig[~eq, 2] / sig[~eq, 0] > 1e-8).all()
    dev = gr.track_deviation(opts, name)
    k2 = ((sig[~eq, 0] / sig[~eq, 2]) ** 2).max() if (~eq).any() else 0.0
    print(f"[tracks] {name}: {len(pick)} reference points, oracle deviation {dev:.3g} ({dev / EPS:.3g} eps, {dev / (EPS * k2) if k2 else 0:.3g} eps kappa^2)")
    assert dev <= 4 * max(gr.ORACLE_TRACK_DEVIATION[name], 2 * EPS), (name, dev)         # the recorded value; 4: another libm's sin / cos
    if name.startswith("mixed_") and sc["n_pt"] > 254:
        assert 253 in pick and 254 in pick and sc["equality_only"] == [254]
    # the reference lands on the scene (0.1 px noise): it triangulates what the cases say it does
    if name in ("mixed_257", "b1_d10_c40"):
        assert np.abs(x[~eq] - sc["X"][pick[~eq]]).max() < 0.05


def test_rodrigues_edges_of_the_mixed_scene():
    sc = gr.mixed_tracks_scene(257)
    w = sc["ext"][:, :3]
    assert 0 < w[0] @ w[0] <= np.finfo(np.float64).eps and not sc["ext"][1].any()
    assert abs(np.linalg.norm(w[2]) - (np.pi - 1e-9)) < 1e-15
    lens = np.bincount(sc["obs_pt"], minlength=257)
    assert np.array_equal(lens, sc["n_views"]) and set(lens.tolist()) == {0, 1, 2, 3, 40}
    assert sorted(sc["obs_cam"][sc["obs_pt"] == 253].tolist()) == [5, 5, 9] and (sc["obs_cam"][sc["obs_pt"] == 254] == 7).all()
    assert not np.array_equal(sc["obs_pt"], np.sort(sc["obs_pt"]))                  # shuffled


@pytest.mark.parametrize("n_obs", gr.REPROJ_SIZES)
def test_reprojection_oracle_deviation(n_obs):
    c = gr.reprojection_case(n_obs)
    ref = gr.reprojection_errors(c["K4"], c["ext"], c["pts"], c["obs_cam"], c["obs_pt"], c["obs_uv"])
    oerr = orc.reprojection_errors(c["K4"], c["ext"], c["pts"], c["obs_cam"], c["obs_pt"], c["obs_uv"])
    dev, kinds = gr.reprojection_deviation(oerr, ref)
    print(f"[reproj] n_obs={n_obs}: oracle deviation {dev:.3g} ({dev / EPS:.3g} eps)")
    # fx x / z + cx - u cancels pixel coordinates of a few thousand: a handful of roundings of that size, against max(err, 1)
    assert kinds and dev <= 16 * EPS * max(1.0, np.abs(c["obs_uv"]).max())
    assert dev <= 4 * gr.ORACLE_REPROJ_DEVIATION[n_obs]                                   # the recorded value
    if n_obs >= 255:
        assert np.isfinite(ref[253]) and ref[253] > 1.0          # behind the camera: an ordinary number
        assert np.isposinf(ref[254])                             # z == 0 exactly, x != 0
        assert np.isnan(ref[252]) and (n_obs == 255 or np.isnan(ref[n_obs - 1]))
        assert np.isfinite(np.delete(ref, [252, 254, n_obs - 1])).all()
    else:
        assert np.isfinite(ref).all() and ref.max() < 50.0


# ---------------------------------------------------------------------------------------------------------------- normals
@pytest.mark.parametrize("name", list(gr.NORMAL_CLOUDS))
def test_normals_oracle_meets_the_reference(name):
    worst = [0.0, 0.0]
    for n in gr.normal_sizes(name):
        pts, idx, dist = gr.normals_cloud_and_table(name, n)
        assert pts.shape == (n, 3)
        finite = bool(np.isfinite(pts).all())
        assert finite == (name != "non_finite")
        for K in gr.NORMAL_KS:
            ref = gr.plane_fit_reference(pts, idx[:, :K])
            assert np.array_equal(ref["count"] == 0, ~np.isfinite(pts).all(1) | (np.isfinite(pts).all(1).sum() < 2))
            if not finite or n < 2:
                continue                                        # the oracle's search is not defined there
            unit, excess, sign_bad, nan_ok = gr.normal_metrics(orc.estimate_normals(pts, K), ref)
            worst = [max(worst[0], unit), max(worst[1], excess)]
            assert nan_ok and sign_bad == 0 and unit <= 4 and excess <= 4, (name, n, K, unit, excess, sign_bad, nan_ok)
        r = gr.hybrid_radius(dist)
        tab = gr.hybrid_table(idx, dist, 10, r)
        if finite and n >= 17 and name not in ("identical", "sphere_x5", "lattice8"):
            empty = ((tab >= 0).sum(1) == 0).mean()
            assert 0.2 < empty < 0.8, (name, n, empty)            # the hybrid radius leaves rows without and rows with neighbours
    print(f"[normals] {name}: oracle | |n| - 1 | <= {worst[0]:.3g} eps, Rayleigh excess <= {worst[1]:.3g} eps scale")


@pytest.mark.parametrize("n", [17, 257, 600])
def test_scaling_by_a_power_of_two_is_exact_in_the_oracle(n):
    base = orc.estimate_normals(gr.normals_cloud_and_table("sphere", n)[0], 10)
    for name in ("sphere_2p100", "sphere_2m100"):
        pts, idx, _ = gr.normals_cloud_and_table(name, n)
        assert np.array_equal(idx, gr.normals_cloud_and_table("sphere", n)[1])
        assert gr.same_bits(orc.estimate_normals(pts, 10), base)


def test_reference_plane_fit_on_an_exact_plane():
    pts, idx, _ = gr.normals_cloud_and_table("plane_z7", 257)
    ref = gr.plane_fit_reference(pts, idx[:, :10])
    assert (ref["lam"][:, 0] == 0).all() and (ref["C"][:, 2, :] == 0).all() and (ref["mean"][:, 2] == 7).all()
    nrm = np.tile([[0.0, 0.0, -1.0]], (257, 1))
    assert gr.normal_metrics(nrm, ref) == (0.0, 0.0, 0, True)
    assert gr.normal_metrics(-nrm, ref)[2] == 257                                # the sign rule sees a flipped normal
    tilt = nrm.copy(); tilt[:, 0] = 1e-7; tilt /= np.linalg.norm(tilt, axis=1, keepdims=True)
    assert gr.normal_metrics(tilt, ref)[1] > 16                                  # and the excess a normal 1e-7 rad off
