"""Normals by brute force (SFMHIP_POINTS_BRUTE) against the cell grid (SFMHIP_POINTS_GRID): host clock around the synchronous
sfmhip_estimate_normals_ex call (both copies included), the two methods alternating in one process, warm-up first, best of --reps.
Clouds: the noisy sphere of test_normals_at_300k_points, that sphere with 1 % far outliers (uniform(-4e4, 4e4)), and the points of
synth.ba_scene_mt(200, n) (a volume).  Brute force at 2M points runs once.  Prints one line per (cloud, n) with the grid's fallback
list length, then the smallest size from which the grid wins by >= 10 % on every cloud -- the threshold of SFMHIP_POINTS_AUTO.

    python experiments/time_points.py [--sizes 10000,30000,...] [--clouds sphere,outliers,ba] [--reps 5] [--K 10]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sfm_opencv_amd import api, synth  # noqa: E402


def sphere(n, seed=77):
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    return d * (5.0 + 0.002 * rng.standard_normal((n, 1))) + np.array([0.3, -0.2, 0.1])


def cloud(kind, n):
    if kind == "sphere":
        return sphere(n)
    if kind == "outliers":
        m = n // 100
        return np.concatenate([sphere(n - m), np.random.default_rng(11).uniform(-4e4, 4e4, (m, 3))])
    if kind == "ba":
        return np.ascontiguousarray(synth.ba_scene_mt(200, n)["pts0"])
    raise ValueError(kind)


def timed(ctx, pts, K, method, reps):
    best, out = float("inf"), None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = ctx.estimate_normals(pts, K, method)
        best = min(best, time.perf_counter() - t0)
    return best * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10000,30000,100000,300000,1000000,2000000")
    ap.add_argument("--clouds", default="sphere,outliers,ba")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--K", type=int, default=10)
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]
    clouds = a.clouds.split(",")
    ctx = api.Context(0)
    ratio = {}
    print(f"# K = {a.K}, best of {a.reps} after a warm-up, ms per sfmhip_estimate_normals_ex incl. H2D / D2H")
    print(f"# {'cloud':9s} {'n':>8s} {'brute ms':>10s} {'grid ms':>9s} {'grid/brute':>10s} {'fallback':>9s}  same bits")
    for n in sizes:
        for kind in clouds:
            pts = cloud(kind, n)
            once = n >= 2_000_000                      # brute force at 2M: seconds per call
            if not once:
                ctx.estimate_normals(pts, a.K, "brute")
            ctx.estimate_normals(pts, a.K, "grid")
            tb = tg = float("inf")
            for _ in range(1 if once else a.reps):     # alternating
                t, nb = timed(ctx, pts, a.K, "brute", 1); tb = min(tb, t)
                t, ng = timed(ctx, pts, a.K, "grid", 1); tg = min(tg, t)
            if once:
                t, ng = timed(ctx, pts, a.K, "grid", max(1, a.reps - 1)); tg = min(tg, t)
            fb = ctx.points_fallback_count()
            same = np.array_equal(nb.view(np.uint64), ng.view(np.uint64))
            ratio[(kind, n)] = tg / tb
            print(f"  {kind:9s} {n:8d} {tb:10.2f} {tg:9.2f} {tg / tb:10.3f} {fb:9d}  {same}", flush=True)
    wins = [n for n in sizes if all(ratio[(k, m)] <= 0.9 for k in clouds for m in sizes if m >= n)]
    print(f"# grid faster by >= 10 % on every cloud from n = {min(wins) if wins else 'never'}")
    ctx.close()


if __name__ == "__main__":
    main()
