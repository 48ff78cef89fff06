"""Two-view relative pose (sfmhip_relative_pose): warm-up first, best of --reps.

The batch is the chain case of time_verify.py with general scenes only (the pose is for pairs of kind 1): 199 pairs x 2000
correspondences, 30 % wrong matches, 0.5 px noise, coordinates normalised by f = 800.  sfmhip_two_view_geometry_dev (H = 1024, rounds 3,
t_f = 1 px, t_h = 2 px) runs first on the resident blocks and leaves the mask and F the pose call consumes; it is timed too, for scale.
The pose call (rounds 3, iters 10, 50 baselines, 2 degrees) is timed with the blocks resident (the _dev call between two events on the
context's stream, and a train of 20 calls between two events divided by 20) and from host arrays (host clock around the synchronous
call, both copies included), for the batch and for one pair alone.

    python experiments/time_relpose.py [--reps 5]
    rocprofv3 --kernel-trace --stats -d DIR -- python experiments/time_relpose.py --trace      # five calls of the pose call on the batch
"""
import argparse
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import relpose_ref as rp  # noqa: E402  (the truth of the scene and the angle functions only)
import twoview_ref as tv  # noqa: E402

TF = 1.0 / tv.FOCAL
TH = 2.0 / tv.FOCAL
H = 1024


def batch(n_pairs, m):
    blocks = np.empty((n_pairs, m, 4))
    good = np.empty((n_pairs, m), bool)
    for q in range(n_pairs):
        pix, good[q] = tv.two_view_scene(m, 0.3, 1000 + q)
        blocks[q] = tv.normalised(pix)
    return blocks, np.full(n_pairs, m, np.int32), good


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=199)
    ap.add_argument("--rows", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--trace", action="store_true", help="five calls of the pose call on the batch: for a kernel trace")
    a = ap.parse_args()
    import torch
    from sfm_opencv_amd import api
    ctx = api.Context(0, use_torch_stream=True)
    blocks, counts, good = batch(a.pairs, a.rows)
    print(f"# best of {a.reps} after a warm-up; device ms: the _dev call on resident blocks between two stream events; train ms: 20 such calls between two "
          f"events, per call; call ms: host clock around the synchronous call incl. H2D / D2H; rounds {a.rounds}, iters {a.iters}, t = 1 px, 50 baselines, 2 deg")
    print(f"# {'call':>12s} {'pairs':>5s} {'rows':>5s} {'device ms':>10s} {'train ms':>9s} {'call ms':>9s}")
    for n in (a.pairs, 1):
        b, c, g = blocks[:n], counts[:n], good[:n]
        with torch.cuda.stream(ctx.torch_stream):
            d_corr = torch.from_numpy(b).to("cuda"); d_counts = torch.from_numpy(c).to("cuda")
            d_mask = torch.empty((n, a.rows), dtype=torch.uint8, device="cuda"); d_cnt = torch.empty(n, dtype=torch.int32, device="cuda")
            d_F = torch.empty((n, 9), dtype=torch.float64, device="cuda"); d_kind = torch.zeros(n, dtype=torch.int32, device="cuda")
            d_pose = torch.empty((n, 12), dtype=torch.float64, device="cuda"); d_info = torch.empty((n, 10), dtype=torch.int32, device="cuda")
            d_q = torch.empty((n, 5), dtype=torch.float64, device="cuda"); d_mo = torch.empty((n, a.rows), dtype=torch.uint8, device="cuda")
            geometry = lambda: ctx.two_view_geometry_dev(d_corr, a.rows, d_counts, n, TF, TH, d_kind, d_mask, d_cnt, 0, d_F, 0, 0, hypotheses=H, rounds=3, seed=0)   # noqa: E731
            pose = lambda: ctx.relative_pose_dev(d_corr, a.rows, d_counts, n, d_mask, d_F, TF, d_pose, d_info, d_q, d_mo, rounds=a.rounds, iters=a.iters)   # noqa: E731

            def timed(f, calls=1):
                best = float("inf")
                for it in range(a.reps + 1):
                    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(calls):
                        f()
                    e1.record(); e1.synchronize()
                    if it:
                        best = min(best, e0.elapsed_time(e1) / calls)
                return best
            if a.trace:
                geometry()
                for _ in range(5):
                    pose()
                torch.cuda.synchronize()
                print(f"# traced: {n} pairs x {a.rows} rows, 5 calls of sfmhip_relative_pose_dev")
                break
            tg = timed(geometry)
            tp, tt = timed(pose), timed(pose, 20)
            kind = d_kind.cpu().numpy(); mask = d_mask.cpu().numpy(); F = d_F.cpu().numpy()
            got = d_pose.cpu().numpy(), d_info.cpu().numpy(), d_q.cpu().numpy(), d_mo.cpu().numpy()
        lists = list(b)
        f_host = lambda: ctx.relative_pose(lists, list(mask), F, TF, rounds=a.rounds, iters=a.iters)   # noqa: E731
        out = f_host()
        th = float("inf")
        for _ in range(a.reps):
            t0 = time.perf_counter(); out = f_host(); th = min(th, (time.perf_counter() - t0) * 1e3)
        assert out[0].tobytes() == got[0].tobytes() and out[1].tobytes() == got[1].tobytes()
        g_host = lambda: ctx.two_view_geometry(lists, TF, TH, hypotheses=H, rounds=3, seed=0)   # noqa: E731
        g_host(); t0 = time.perf_counter(); g_host(); tgh = (time.perf_counter() - t0) * 1e3
        print(f"  {'geometry F+H':>12s} {n:5d} {a.rows:5d} {tg:10.3f} {'-':>9s} {tgh:9.2f}")
        print(f"  {'pose':>12s} {n:5d} {a.rows:5d} {tp:10.3f} {tt:9.3f} {th:9.2f}", flush=True)
        pose_, info = got[0], got[1]
        okq = np.flatnonzero(info[:, 0] == 1)
        rot = [math.degrees(rp.rotation_angle(pose_[q, :9], rp.TRUE_R)) for q in okq]
        dirn = [math.degrees(rp.direction_angle(pose_[q, 9:], rp.TRUE_T)) for q in okq]
        inl = (got[3] & 1).astype(bool)
        print(f"#   kind 1: {int((kind == 1).sum())} of {n}; status 1: {len(okq)}; rotation error max {max(rot):.3f} deg, baseline direction error max {max(dirn):.3f} deg "
              f"(median {np.median(dirn):.3f}); n_inl / RANSAC count mean {np.mean(info[okq, 7] / info[okq, 6]):.3f}; true matches kept {(inl & g).sum() / g.sum():.3f}, "
              f"wrong among inliers {(inl & ~g).sum() / inl.sum():.4f}; n_front / n_inl min {np.min(info[okq, 8] / info[okq, 7]):.3f}")
    ctx.close()


if __name__ == "__main__":
    main()
