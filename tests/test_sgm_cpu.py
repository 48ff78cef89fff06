"""CPU: the semi-global aggregation as include/sfmhip.h defines it, on its numpy restatement (tests/sgm_ref.py).  What it buys is a
property of the definition: it is tested here on the restatement alone, and the bit-equality of tests/test_sgm_gpu.py carries it over to
the device.  Also the resource metadata of the new kernels against what DESIGN.md 4h states."""
import os
import re

import numpy as np
import pytest

import dense_ref as dr
import sgm_ref as sr
from test_codeobj_cpu import LIB, READELF, _kernel_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, WMIN, WMAX, R = 48, 1.0 / 8.0, 1.0 / 3.0, 1
STEP = (WMAX - WMIN) / (D - 1)


@pytest.fixture(scope="module")
def swept():
    """the planted scene at 96 x 72, view 0 against views 1 and 2 with the small, noisy window"""
    sc = dr.Scene()
    rendered = [sc.render(v) for v in range(3)]
    A, b, *_ = dr.sweep_geometry(sc.K4, sc.EXT[0], sc.EXT[1:3])
    plane, _, _, c = dr.plane_sweep(rendered[0][0], [rendered[1][0], rendered[2][0]], A, b, D, WMIN, WMAX, R, 1, -1.0)
    return plane, c, rendered[0][1]


def test_aggregation_brings_more_pixels_to_the_true_plane(swept):
    plane, c, z = swept
    C = sr.costs_of(c, 262144)
    sgm_plane = sr.sgm_depth(C, WMIN, WMAX, 512, 4096, 8, 65535)[0]
    k_true = (1.0 / z - WMIN) / STEP
    away = dr.discontinuity_mask(z, R + 2)
    share = {}
    for name, p in (("winner-take-all", plane), ("sgm", sgm_plane)):
        sel = (p >= 0) & away
        share[name] = (np.abs(p[sel] - k_true[sel]) <= 1.0).mean()
        print(f"{name}: {share[name]:.4f} of {sel.sum()} pixels within one plane")
        assert sel.sum() > 0.5 * p.size
    assert share["sgm"] >= share["winner-take-all"] + 0.03


@pytest.mark.parametrize("paths", [4, 8])
def test_without_penalties_the_sum_is_the_cost_times_the_paths(swept, paths):
    _, c, _ = swept
    C = sr.costs_of(c, 262144)
    plane, cost, ssum, depth, S = sr.sgm_depth(C, WMIN, WMAX, 0, 0, paths, 65535)
    assert S.dtype == np.uint32 and np.array_equal(S, paths * C.astype(np.uint32))
    seen = C != sr.UNSEEN
    first = np.where(seen, C.astype(np.int64), 1 << 20).argmin(2)  # the first of the smallest seen costs
    any_seen = seen.any(2)
    assert np.array_equal(plane[any_seen], first[any_seen]) and (plane[~any_seen] == -1).all() and any_seen.mean() > 0.8
    yy, xx = np.nonzero(any_seen)
    assert np.array_equal(cost[any_seen], C[yy, xx, first[any_seen]]) and np.array_equal(ssum[any_seen], paths * cost[any_seen].astype(np.uint32))
    assert np.isnan(depth[~any_seen]).all() and np.isfinite(depth[any_seen]).all()


def test_costs_are_the_rounded_scaled_scores():
    c = np.array([1.0, 0.999998, 0.75, -1.0, np.nan, 1.0 - 65534.4 / 262144, 1.0 - 65534.6 / 262144]).reshape(-1, 1, 1)
    assert sr.costs_of(c, 262144).ravel().tolist() == [0, 1, 65534, 65534, 65535, 65534, 65534]
    assert sr.costs_of(c, 4.0).ravel().tolist()[:5] == [0, 0, 1, 8, 65535]


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not found")
def test_sgm_kernels_without_scratch_and_with_the_lds_the_design_states(tmp_path):
    assert os.path.exists(LIB), "build libsfmhip.so first (__graft_entry__.build)"
    t = _kernel_table(tmp_path)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for kernel, count in (("sgm_cost_kernel", 6), ("sgm_path_kernel", 4), ("sgm_winner_kernel", 1)):
        hits = sorted(k for k in t if kernel in k)
        assert len(hits) == count, (kernel, hits)
        said = re.search(kernel + r" keeps (\d+) bytes of LDS", design)
        assert said, f"DESIGN.md 4h does not say what {kernel} keeps in LDS"
        for name in hits:
            k = t[name]
            assert k["scratch"] == 0 and (k["spill"] or 0) == 0, (name, k)
            assert k["lds"] == int(said.group(1)), (name, k, said.group(0))
            assert k["vgpr"] + k["agpr"] <= 128, (name, k)         # four waves per SIMD
    assert not [k for k in t if "sweep_kernel" in k and "sgm" in k]
