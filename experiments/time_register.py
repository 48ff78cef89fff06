"""Image registration (sfmhip_register_views): warm-up first, best of --reps.

The cases are 1, 32 and 199 views x 2000 correspondences (planted scenes of tests/pnp_ref.py: 30 % wrong observations, 0.5 px noise),
H = 1024, rounds 1 and 3, t = 2 px on coordinates normalised by f = 800.  Every case is timed with the blocks resident (the _dev call
between two events on the context's stream) and from host arrays (host clock around the synchronous call, both copies included).  The
last line is the host solvePnPRansac of sfm_geometry.hpp on one such view (tests/host/geom_test), for scale only.

    python experiments/time_register.py [--reps 5]
    rocprofv3 --kernel-trace --stats -d DIR -- python experiments/time_register.py --trace      # 199 views, rounds 3, five calls
"""
import argparse
import os
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pnp_ref as pr  # noqa: E402  (the scene generator only)

T = 2.0 / pr.FOCAL
H = 1024


def batch(n_views, m):
    blocks = np.empty((n_views, m, 5))
    good = np.empty((n_views, m), bool)
    px = []
    for q in range(n_views):
        rows, good[q], _, _ = pr.planted_scene(m, 0.3, 1000 + q)
        blocks[q] = pr.normalised(rows)
        px.append(rows)
    return blocks, np.full(n_views, m, np.int32), good, px


def best_of(f, reps):
    best, out = float("inf"), None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = f()
        best = min(best, time.perf_counter() - t0)
    return best * 1e3, out


def device_ms(ctx, blocks, counts, rounds, reps):
    """(best ms, mask bool) of the _dev call on resident blocks"""
    import torch
    n, stride = blocks.shape[:2]
    with torch.cuda.stream(ctx.torch_stream):
        d_corr = torch.from_numpy(blocks).to("cuda"); d_counts = torch.from_numpy(counts).to("cuda")
        d_mask = torch.empty((n, stride), dtype=torch.uint8, device="cuda"); d_cnt = torch.empty(n, dtype=torch.int32, device="cuda")
        d_P = torch.empty((n, 12), dtype=torch.float64, device="cuda"); d_win = torch.empty(n, dtype=torch.int32, device="cuda")
        best = float("inf")
        for it in range(reps + 1):
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            ctx.register_views_dev(d_corr, stride, d_counts, n, T, d_mask, d_cnt, d_P, d_win, hypotheses=H, rounds=rounds, seed=0)
            e1.record()
            e1.synchronize()
            if it:
                best = min(best, e0.elapsed_time(e1))
        return best, d_mask.cpu().numpy().astype(bool)


def host_pnp_ms(rows_px, reps):
    """best ms of tests/host/geom_test pnp on one view, its process start and file reading included (a few ms), and its inlier count"""
    host = os.path.join(ROOT, "tests", "host")
    subprocess.check_call(["make", "-C", host, "geom_test"], stdout=subprocess.DEVNULL)
    K = np.array([[pr.FOCAL, 0, pr.WIDTH / 2], [0, pr.FOCAL, pr.HEIGHT / 2], [0, 0, 1.0]])
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "in.bin"), "wb") as f:
            f.write(K.astype("<f8").tobytes()); f.write(struct.pack("<i", len(rows_px)))
            f.write(rows_px[:, :3].astype(np.float32).tobytes()); f.write(rows_px[:, 3:].astype(np.float32).tobytes())
        run = lambda args: subprocess.check_call([os.path.join(host, "geom_test")] + args)      # noqa: E731
        t_pnp, _ = best_of(lambda: run(["pnp", os.path.join(d, "in.bin"), os.path.join(d, "out.bin")]), reps)
        n_in = struct.unpack_from("<i", open(os.path.join(d, "out.bin"), "rb").read(), 124)[0]
        return t_pnp, n_in


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--views", type=int, default=199)
    ap.add_argument("--rows", type=int, default=2000)
    ap.add_argument("--trace", action="store_true", help="the batch with rounds 3, five calls: for a kernel trace")
    a = ap.parse_args()
    from sfm_opencv_amd import api
    ctx = api.Context(0, use_torch_stream=True)
    blocks, counts, good, px = batch(a.views, a.rows)
    if a.trace:
        for _ in range(5):
            device_ms(ctx, blocks, counts, 3, 1)
        print(f"# traced: {a.views} views x {a.rows} rows, H {H}, rounds 3, 5 x 2 calls of sfmhip_register_views_dev")
        ctx.close()
        return
    print(f"# best of {a.reps} after a warm-up; device ms: the _dev call on resident blocks between two stream events; call ms: host clock around the "
          f"synchronous call incl. H2D / D2H; H = {H}, t = 2 px, 30 % wrong observations, seed 0")
    print(f"# {'views':>5s} {'rows':>5s} {'rounds':>6s} {'device ms':>10s} {'call ms':>9s} {'kept':>6s} {'wrong':>7s}")
    for n_views in sorted({1, min(32, a.views), a.views}):
        b, c, g = blocks[:n_views], counts[:n_views], good[:n_views]
        for rounds in (1, 3):
            td, mask = device_ms(ctx, b, c, rounds, a.reps)
            f = lambda: ctx.register_views(list(b), T, hypotheses=H, rounds=rounds, seed=0)[0]      # noqa: E731
            f()
            tc, out = best_of(f, a.reps)
            assert np.array_equal(np.stack(out), mask)
            kept = (mask & g).sum() / g.sum(); wrong = (mask & ~g).sum() / (~g).sum()
            print(f"  {n_views:5d} {a.rows:5d} {rounds:6d} {td:10.3f} {tc:9.2f} {kept:6.3f} {wrong:7.4f}", flush=True)
    ctx.close()
    t_host, n_in = host_pnp_ms(px[0], a.reps)
    print(f"# host solvePnPRansac (geom_test pnp, process start included), one view of {a.rows} rows: {t_host:.2f} ms, {n_in} inliers at its 8 px")


if __name__ == "__main__":
    main()
