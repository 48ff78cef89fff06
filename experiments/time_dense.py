"""Dense depth (sfmhip_plane_sweep and the chain behind it): warm-up first, best of --reps.

The views are the planted scene of tests/dense_ref.py (two textured planes, four views) rendered at the case's size with the focal length
and the texture frequencies scaled to it, so a pixel sees what a pixel of the tests' 96 x 72 views sees.  Cases: 1024 x 768 and
3648 x 2736, 64 and 128 planes, r = 2, two sources, [wmin, wmax] = [1/8, 1/3], images resident on the device.
  sweep ms   sfmhip_plane_sweep_dev of view 0 (the gray planes and the sweep kernel) between two events on the context's stream
  chain ms   all four views swept, checked (rel_tol 0.01, two agreeing sources) and exported, the same way (no copy to the host)
  Gtriple/s  (pixel x plane x source) triples of the sweep per second, in 1e9
For scale only, the numpy restatement of tests/dense_ref.py runs the smallest case once (host clock) and its bytes are compared.

    python experiments/time_dense.py [--reps 3] [--no-numpy]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dense_ref as dr  # noqa: E402

WMIN, WMAX, R, N_SRC = 1.0 / 8.0, 1.0 / 3.0, 2, 2


def views(rows, cols):
    scale = cols / dr.Scene.COLS
    sc = dr.Scene(freq_scale=scale)
    fx, fy, cx, cy = dr.Scene.K4
    sc.K4 = (fx * scale, fy * scale, (cx + 0.5) * scale - 0.5, (cy + 0.5) * scale - 0.5)
    return sc, [sc.render(v, rows=rows, cols=cols)[0] for v in range(4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-numpy", action="store_true")
    ap.add_argument("--sizes", default="1024x768,3648x2736")
    a = ap.parse_args()
    import torch
    from sfm_opencv_amd import api
    ctx = api.Context(0, use_torch_stream=True)
    print(f"# best of {a.reps} after a warm-up; r = {R}, {N_SRC} sources, w in [1/8, 1/3], resident images; events on the context's stream")
    print(f"# {'size':>11s} {'planes':>6s} {'sweep ms':>9s} {'Gtriple/s':>9s} {'chain ms':>9s} {'scored':>7s} {'kept':>7s} {'points':>9s}")
    first = True
    for size in a.sizes.split(","):
        cols, rows = (int(x) for x in size.split("x"))
        sc, images = views(rows, cols)
        sources = api.dense_sources(sc.EXT, N_SRC)
        geo = [api.sweep_geometry(sc.K4, sc.EXT[i], sc.EXT[sources[i]]) for i in range(4)]
        npx = rows * cols
        with torch.cuda.stream(ctx.torch_stream):
            d_img = [torch.from_numpy(im).to("cuda") for im in images]
            d_depth = [torch.empty(npx, dtype=torch.float32, device="cuda") for _ in range(4)]
            d_plane = torch.empty(npx, dtype=torch.int32, device="cuda"); d_score = torch.empty(npx, dtype=torch.float32, device="cuda")
            d_keep = torch.empty(npx, dtype=torch.uint8, device="cuda"); d_n = torch.zeros(4, dtype=torch.int32, device="cuda")
            d_xyz = torch.empty((npx, 3), dtype=torch.float64, device="cuda"); d_bgr = torch.empty((npx, 3), dtype=torch.uint8, device="cuda")
            for D in (64, 128):
                def sweep(i):
                    ctx.plane_sweep_dev(d_img[i], [d_img[j] for j in sources[i]], rows, cols, 1, cols, geo[i][0], geo[i][1], D, WMIN, WMAX, R, 1, -1.0, d_plane, d_score,
                                        d_depth[i])

                def chain():
                    for i in range(4):
                        sweep(i)
                    for i in range(4):
                        _, _, Rrel, trel, Rinv, c = geo[i]
                        ctx.depth_consistency_dev(d_depth[i], [d_depth[j] for j in sources[i]], rows, cols, sc.K4, Rrel, trel, 0.01, 2, None, d_keep)
                        ctx.depth_to_points_dev(d_depth[i], d_keep, d_img[i], rows, cols, 1, cols, sc.K4, Rinv, c, d_xyz, d_bgr, npx, d_n[i:])

                def timed(f):
                    best = float("inf")
                    for it in range(a.reps + 1):
                        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
                        e0.record(); f(); e1.record(); e1.synchronize()
                        if it:
                            best = min(best, e0.elapsed_time(e1))
                    return best
                tc = timed(chain)
                ts = timed(lambda: sweep(0))
                plane0 = d_plane.cpu().numpy(); depth0 = d_depth[0].cpu().numpy(); n = d_n.cpu().numpy()
                print(f"  {cols:5d}x{rows:<5d} {D:6d} {ts:9.3f} {npx * D * N_SRC / ts / 1e6:9.2f} {tc:9.3f} {(plane0 >= 0).mean():7.3f} {n.sum() / (4 * npx):7.3f} {int(n.sum()):9d}",
                      flush=True)
                if first and not a.no_numpy:
                    first = False
                    t0 = time.perf_counter()
                    ep, _, ed, _ = dr.plane_sweep(images[0], [images[j] for j in sources[0]], geo[0][0], geo[0][1], D, WMIN, WMAX, R, 1, -1.0)
                    tn = time.perf_counter() - t0
                    same = ep.tobytes() == plane0.tobytes() and ed.tobytes() == depth0.tobytes()
                    print(f"#   numpy restatement of that sweep, one host thread: {tn * 1e3:.0f} ms ({tn * 1e3 / ts:.0f} x); the same bytes: {same}", flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
