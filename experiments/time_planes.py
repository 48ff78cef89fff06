"""RANSAC plane segmentation (sfmhip_segment_planes): host clock around the synchronous call (both copies included), warm-up first, best
of --reps, for one plane and for four, with 256 and 1024 hypotheses per round.  Clouds: those of time_cluster.py (noisy sphere, that
sphere with 1 % far outliers, a volume) plus a planted scene of three planes (50 / 25 / 15 % of the points, noise sigma 0.002, the rest
clutter in [-1, 1]^3).  The threshold is 0.006 on every cloud and min_inliers is n / 100: on the curved clouds a round finds a thin cap or
nothing, which is the cheap end (a round after the stop only launches), on the planted scene four rounds find three planes.

Beside each time: the device time of the same work on a resident cloud (sfmhip_segment_planes_dev between two events on the context's
stream).  The share of plane_score_kernel in it comes from a kernel trace of one case, taken in a run of its own (--trace).

    python experiments/time_planes.py [--sizes 300000,2000000] [--clouds sphere,outliers,ba,planes] [--reps 5]
    rocprofv3 --kernel-trace --stats -d DIR -- python experiments/time_planes.py --trace      # one case: planted scene, 2M, H 1024, 1 plane
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
from time_radius import best_of  # noqa: E402

T = 0.006


def planted(n):
    """three planes with 50 / 25 / 15 % of the points and 10 % clutter, shuffled"""
    rng = np.random.default_rng(21)
    parts = []
    for share, normal, offset in ((0.50, (0.1, 0.2, 1.0), 0.3), (0.25, (1.0, -0.3, 0.2), -0.4), (0.15, (0.2, 1.0, -0.5), 0.1)):
        k = int(share * n)
        nrm = np.asarray(normal) / np.linalg.norm(normal)
        u = np.cross(nrm, [1.0, 0.0, 0.0]); u /= np.linalg.norm(u)
        v = np.cross(nrm, u)
        st = rng.uniform(-1, 1, (k, 2))
        parts.append(offset * nrm + st[:, :1] * u + st[:, 1:] * v + rng.normal(0, 0.002, (k, 1)) * nrm)
    parts.append(rng.uniform(-1, 1, (n - sum(len(p) for p in parts), 3)))
    pts = np.concatenate(parts)
    return np.ascontiguousarray(pts[rng.permutation(n)])


def make(kind, n):
    return planted(n) if kind == "planes" else cloud(kind, n)


def device_ms(ctx, pts, H, max_planes, min_inliers, reps):
    """best device time of sfmhip_segment_planes_dev on a resident cloud, between two events on the context's stream"""
    import torch
    n = len(pts)
    with torch.cuda.stream(ctx.torch_stream):
        d_pts = torch.from_numpy(pts).to("cuda")
        d_lab = torch.empty(n, dtype=torch.int32, device="cuda"); d_np = torch.empty(1, dtype=torch.int32, device="cuda")
        d_pl = torch.empty((max_planes, 4), dtype=torch.float64, device="cuda"); d_rf = torch.empty_like(d_pl)
        d_ct = torch.empty(max_planes, dtype=torch.int32, device="cuda"); d_wn = torch.empty_like(d_ct)
        best = float("inf")
        for it in range(reps + 1):
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            ctx.segment_planes_dev(d_pts.data_ptr(), n, T, max_planes, d_lab.data_ptr(), d_np.data_ptr(), d_pl.data_ptr(), d_rf.data_ptr(),
                                   d_ct.data_ptr(), d_wn.data_ptr(), hypotheses=H, seed=0, min_inliers=min_inliers)
            e1.record()
            e1.synchronize()
            if it:
                best = min(best, e0.elapsed_time(e1))
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="300000,2000000")
    ap.add_argument("--clouds", default="sphere,outliers,ba,planes")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trace", action="store_true", help="one case, five calls: for a kernel trace")
    a = ap.parse_args()
    ctx = api.Context(0, use_torch_stream=True)
    if a.trace:
        pts = planted(2_000_000)
        for _ in range(5):
            out = ctx.segment_planes(pts, T, max_planes=1, hypotheses=1024, seed=0, min_inliers=len(pts) // 100)
        print(f"# traced: planted scene, 2000000 points, H 1024, 1 plane, 5 calls; counts {out[2].tolist()}")
        ctx.close()
        return
    sizes = [int(s) for s in a.sizes.split(",")]
    print(f"# best of {a.reps} after a warm-up; call ms: host clock around sfmhip_segment_planes incl. H2D / D2H; device ms: sfmhip_segment_planes_dev "
          f"on a resident cloud between two stream events; t = {T}, min_inliers = n / 100, seed 0, refined planes included")
    print(f"# {'cloud':9s} {'n':>8s} {'H':>5s} {'max_planes':>10s} {'call ms':>9s} {'device ms':>10s} {'found':>6s}  counts")
    for n in sizes:
        for kind in a.clouds.split(","):
            pts = make(kind, n)
            for H in (256, 1024):
                for mp in (1, 4):
                    f = lambda: ctx.segment_planes(pts, T, max_planes=mp, hypotheses=H, seed=0, min_inliers=n // 100)      # noqa: E731
                    f()
                    tc, out = best_of(f, a.reps)
                    td = device_ms(ctx, pts, H, mp, n // 100, a.reps)
                    print(f"  {kind:9s} {n:8d} {H:5d} {mp:10d} {tc:9.2f} {td:10.3f} {len(out[2]):6d}  {out[2].tolist()}", flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
