"""GPU: plane_fit / eig3_min of normals.hip (shared by normals_kernel, normals_from_knn_kernel and the hybrid path) on the clouds where
a 3 x 3 eigen-solver goes wrong, against a reference that shares no code with it (tests/geometry_ref.py: longdouble moments over the
neighbour sets of tests/points_ref.py, numpy.linalg.eigh eigenvalues).

On every row with a neighbour: unit length to 4 eps; Rayleigh excess n'Cn - lambda_min <= 16 eps scale, scale = lambda_max + eps max|p|
max|p - mean| (the oracle stays within 4 eps scale -- measured 3.1 -- in tests/test_geometry_ref_cpu.py; the excess stays meaningful with
repeated eigenvalues and implies sin^2 <= excess / (lambda_2 - lambda_1) wherever there is a gap); the sign rule n.mean <= 0 unless
|n.mean| <= 8 eps |mean|.  A row without a neighbour (n = 1, a non-finite row, a hybrid radius that excludes everybody) is NaN in all
three components, and no other row is.  Every method (brute force, grid, auto) gives the same bits, equal to the oracle's wherever the
oracle's search is defined (all rows finite, n >= 2): both sides compile without FMA contraction and use correctly rounded fp64 sqrt
and division.  Scaling a cloud by 2^+-100 scales every operation exactly: the normals do not change in any bit."""
import numpy as np
import pytest

import geometry_ref as gr
import oracle as orc

pytestmark = pytest.mark.gpu
METHODS = (1, 2, 0)          # SFMHIP_POINTS_BRUTE, _GRID, _AUTO


def _check(nrm, ref, what):
    unit, excess, sign_bad, nan_ok = gr.normal_metrics(nrm, ref)
    assert nan_ok, what
    assert unit <= 4 and excess <= 16 and sign_bad == 0, (what, unit, excess, sign_bad)
    return unit, excess


@pytest.mark.parametrize("name", list(gr.NORMAL_CLOUDS))
def test_normals_follow_the_reference_and_equal_the_oracle(ctx, name):
    worst = [0.0, 0.0]
    for n in gr.normal_sizes(name):
        pts, idx, dist = gr.normals_cloud_and_table(name, n)
        oracle_defined = bool(np.isfinite(pts).all()) and n >= 2
        for K in gr.NORMAL_KS:
            ref = gr.plane_fit_reference(pts, idx[:, :K])
            got = [ctx.estimate_normals(pts, K, method=m) for m in METHODS]
            u, e = _check(got[0], ref, (name, n, K))
            worst = [max(worst[0], u), max(worst[1], e)]
            assert gr.same_bits(got[0], got[1]) and gr.same_bits(got[0], got[2]), (name, n, K)
            if oracle_defined:
                o = orc.estimate_normals(pts, K)
                assert gr.same_bits(got[0], o), (name, n, K, np.flatnonzero((got[0] != o).any(1))[:5])
    print(f"[normals] {name}: | |n| - 1 | <= {worst[0]:.3g} eps, Rayleigh excess <= {worst[1]:.3g} eps scale")


@pytest.mark.parametrize("name", list(gr.NORMAL_CLOUDS))
def test_hybrid_normals_follow_the_reference(ctx, name):
    """one radius per cloud (the median nearest-neighbour distance of the reference table): rows whose neighbours all lie beyond it are
    NaN, the others are fitted to the neighbours with dist <= r"""
    for n in gr.normal_sizes(name):
        pts, idx, dist = gr.normals_cloud_and_table(name, n)
        r = gr.hybrid_radius(dist)
        for K in gr.NORMAL_KS:
            ref = gr.plane_fit_reference(pts, gr.hybrid_table(idx, dist, K, r))
            got = [ctx.estimate_normals(pts, K, method=m, radius=r) for m in METHODS]
            _check(got[0], ref, (name, n, K, r))
            assert gr.same_bits(got[0], got[1]) and gr.same_bits(got[0], got[2]), (name, n, K)


@pytest.mark.parametrize("n", [17, 257, 600])
def test_normals_of_a_cloud_scaled_by_a_power_of_two_do_not_change(ctx, n):
    base, _, dist = gr.normals_cloud_and_table("sphere", n)
    r = gr.hybrid_radius(dist)
    for K in gr.NORMAL_KS:
        for m in METHODS:
            a = ctx.estimate_normals(base, K, method=m); h = ctx.estimate_normals(base, K, method=m, radius=r)
            for name, f in (("sphere_2p100", 2.0 ** 100), ("sphere_2m100", 2.0 ** -100)):
                pts = gr.normals_cloud_and_table(name, n)[0]
                assert gr.same_bits(ctx.estimate_normals(pts, K, method=m), a), (name, n, K, m)
                assert gr.same_bits(ctx.estimate_normals(pts, K, method=m, radius=r * f), h), (name, n, K, m)
