"""Neighbour count within a radius by brute force (SFMHIP_POINTS_BRUTE) against the cell grid (SFMHIP_POINTS_GRID), and voxel-grid
down-sampling: host clock around the synchronous sfmhip_radius_count / sfmhip_voxel_downsample call (both copies included), the two
methods alternating in one process, warm-up first, best of --reps.  Clouds: those of time_points.py (noisy sphere, that sphere with 1 %
far outliers, a volume).  Radii: the median distance to the 10th and to the 100th nearest other point of 2000 random points of the cloud
(a kd-tree on the host), so the median count is about 10 and about 100.  The voxel size is the first of the two radii (the outlier
cloud is voxelised without its far points: they would need more than 2^21 voxels along an axis).  Brute force at 2M points runs once.
Prints one line per (cloud, n, r) with the grid's fallback list length, then the smallest size from which the grid wins by >= 10 % on
every cloud at both radii -- the threshold of SFMHIP_POINTS_AUTO for this query.

    python experiments/time_radius.py [--sizes 20000,100000,...] [--clouds sphere,outliers,ba] [--reps 5]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "experiments"))
from sfm_opencv_amd import api  # noqa: E402
from time_points import cloud  # noqa: E402


def radii(pts, targets=(10, 100), n_query=2000):
    from scipy.spatial import cKDTree
    q = pts[np.random.default_rng(1).choice(len(pts), min(n_query, len(pts)), replace=False)]
    d, _ = cKDTree(pts).query(q, k=max(targets) + 1)
    return [float(np.median(d[:, t])) for t in targets]


def best_of(f, reps):
    best, out = float("inf"), None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = f()
        best = min(best, time.perf_counter() - t0)
    return best * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="20000,100000,300000,2000000")
    ap.add_argument("--clouds", default="sphere,outliers,ba")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]
    clouds = a.clouds.split(",")
    ctx = api.Context(0)
    ratio = {}
    print(f"# best of {a.reps} after a warm-up, ms per sfmhip_radius_count / sfmhip_voxel_downsample incl. H2D / D2H")
    print(f"# {'cloud':9s} {'n':>8s} {'r':>10s} {'median':>7s} {'brute ms':>10s} {'grid ms':>9s} {'grid/brute':>10s} {'fallback':>9s}  same")
    for n in sizes:
        for kind in clouds:
            pts = cloud(kind, n)
            once = n >= 2_000_000                      # brute force at 2M: seconds per call
            rs = radii(pts)
            for r in rs:
                if not once:
                    ctx.radius_count(pts, r, "brute")
                ctx.radius_count(pts, r, "grid")
                tb = tg = float("inf")
                for _ in range(1 if once else a.reps):     # alternating
                    t, cb = best_of(lambda: ctx.radius_count(pts, r, "brute"), 1); tb = min(tb, t)
                    t, cg = best_of(lambda: ctx.radius_count(pts, r, "grid"), 1); tg = min(tg, t)
                if once:
                    t, cg = best_of(lambda: ctx.radius_count(pts, r, "grid"), max(1, a.reps - 1)); tg = min(tg, t)
                fb = ctx.points_fallback_count()
                ratio[(kind, n, r)] = tg / tb
                print(f"  {kind:9s} {n:8d} {r:10.4g} {np.median(cg):7g} {tb:10.2f} {tg:9.2f} {tg / tb:10.3f} {fb:9d}  {np.array_equal(cb, cg)}", flush=True)
            vp = pts[np.abs(pts).max(axis=1) < 1e3] if kind == "outliers" else pts
            ctx.voxel_downsample(vp, rs[0])
            tv, out = best_of(lambda: ctx.voxel_downsample(vp, rs[0]), a.reps)
            print(f"  {kind:9s} {len(vp):8d} voxel {rs[0]:.4g}: {tv:9.2f} ms, {len(out[0])} voxels, largest {out[1].max()}", flush=True)
    wins = [n for n in sizes if all(v <= 0.9 for (k, m, r), v in ratio.items() if m >= n)]
    print(f"# grid faster by >= 10 % on every cloud and radius from n = {min(wins) if wins else 'never'}")
    ctx.close()


if __name__ == "__main__":
    main()
