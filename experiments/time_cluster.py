"""DBSCAN / Euclidean clustering by brute force (SFMHIP_POINTS_BRUTE) against the cell grid (SFMHIP_POINTS_GRID): host clock around the
synchronous sfmhip_cluster_dbscan call (both copies included), the two methods alternating in one process, warm-up first, best of
--reps.  Clouds: those of time_points.py (noisy sphere, that sphere with 1 % far outliers, a volume).  Radius: the median distance to
the 10th nearest other point of 2000 random points of the cloud (time_radius.radii), min_points 1 (Euclidean cluster extraction: no
border sweep) and 10.  In the same run sfmhip_radius_count on the grid, same cloud and radius: the yardstick -- the clustering makes
three neighbourhood sweeps (count, link, border) over one binning where the count makes one.  Brute force at 2M points runs once.
Prints one line per (cloud, n, min_points), then the smallest size from which the grid wins by >= 10 % on every cloud and setting --
the threshold of SFMHIP_POINTS_AUTO for this call -- and the clustering / radius-count ratios.

    python experiments/time_cluster.py [--sizes 20000,100000,...] [--clouds sphere,outliers,ba] [--reps 5]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "experiments"))
from sfm_opencv_amd import api  # noqa: E402
from time_points import cloud  # noqa: E402
from time_radius import best_of, radii  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="20000,100000,300000,2000000")
    ap.add_argument("--clouds", default="sphere,outliers,ba")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--min-points", default="1,10")
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]
    clouds = a.clouds.split(",")
    mps = [int(s) for s in a.min_points.split(",")]
    ctx = api.Context(0)
    ratio, against_count = {}, {}
    print(f"# best of {a.reps} after a warm-up, ms per sfmhip_cluster_dbscan / sfmhip_radius_count incl. H2D / D2H")
    print(f"# {'cloud':9s} {'n':>8s} {'r':>10s} {'min_pts':>7s} {'brute ms':>10s} {'grid ms':>9s} {'grid/brute':>10s} {'count ms':>9s} {'grid/count':>10s} "
          f"{'clusters':>9s} {'largest':>8s} {'noise':>7s} {'fallback':>9s}  same")
    for n in sizes:
        for kind in clouds:
            pts = cloud(kind, n)
            once = n >= 2_000_000                      # brute force at 2M: seconds per call
            r = radii(pts, targets=(10,))[0]
            ctx.radius_count(pts, r, "grid")
            tc, _ = best_of(lambda: ctx.radius_count(pts, r, "grid"), a.reps)
            for mp in mps:
                if not once:
                    ctx.cluster_dbscan(pts, r, mp, "brute")
                ctx.cluster_dbscan(pts, r, mp, "grid")
                tb = tg = float("inf")
                for _ in range(1 if once else a.reps):     # alternating
                    t, cb = best_of(lambda: ctx.cluster_dbscan(pts, r, mp, "brute"), 1); tb = min(tb, t)
                    t, cg = best_of(lambda: ctx.cluster_dbscan(pts, r, mp, "grid"), 1); tg = min(tg, t)
                if once:
                    t, cg = best_of(lambda: ctx.cluster_dbscan(pts, r, mp, "grid"), max(1, a.reps - 1)); tg = min(tg, t)
                fb = ctx.points_fallback_count()
                ratio[(kind, n, mp)] = tg / tb
                against_count[(kind, n, mp)] = tg / tc
                labels, sizes_c = cg
                same = np.array_equal(cb[0], cg[0]) and np.array_equal(cb[1], cg[1])
                print(f"  {kind:9s} {n:8d} {r:10.4g} {mp:7d} {tb:10.2f} {tg:9.2f} {tg / tb:10.3f} {tc:9.2f} {tg / tc:10.2f} {len(sizes_c):9d} "
                      f"{int(sizes_c.max()) if len(sizes_c) else 0:8d} {int((labels < 0).sum()):7d} {fb:9d}  {same}", flush=True)
    wins = [n for n in sizes if all(v <= 0.9 for (k, m, mp), v in ratio.items() if m >= n)]
    print(f"# grid faster by >= 10 % on every cloud and setting from n = {min(wins) if wins else 'never'}")
    for n in sizes:
        vs = [v for (k, m, mp), v in against_count.items() if m == n]
        print(f"# n = {n}: clustering on the grid takes {min(vs):.2f} .. {max(vs):.2f} times the radius count on the grid")
    ctx.close()


if __name__ == "__main__":
    main()
