"""Two-view geometric verification (sfmhip_verify_pairs): warm-up first, best of --reps.

The batch case is the chain case: 199 pairs x 2000 correspondences (30 % wrong matches, 0.5 px noise, t = 1 px on coordinates normalised
by f = 800), H = 1024, rounds 1 and 3, with the blocks resident (sfmhip_verify_pairs_dev between two events on the context's stream)
and from host arrays (host clock around the synchronous sfmhip_verify_pairs, both copies included).  The single-pair case is one such
pair; its launch fills few CUs, so it is latency-bound and is reported, not tuned for.

For scale, --host-baseline times the host's find_transform (findEssentialMat + recoverPose of sfm_geometry.hpp, a sequential RANSAC, a
different algorithm) on one such pair in pixels through tests/host/geom_test: wall clock of the process, start-up and file I/O included,
with the same run on 16 correspondences beside it as the fixed cost.  It needs no GPU.

    python experiments/time_verify.py [--reps 5] [--host-baseline]
    rocprofv3 --kernel-trace --stats -d DIR -- python experiments/time_verify.py --trace      # the batch case, rounds 3, five calls
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
import twoview_ref as tv  # noqa: E402  (the scene generator only)

T = 1.0 / tv.FOCAL
H = 1024


def batch(n_pairs, m):
    blocks = np.empty((n_pairs, m, 4))
    good = np.empty((n_pairs, m), bool)
    for q in range(n_pairs):
        pix, good[q] = tv.two_view_scene(m, 0.3, 1000 + q, pure_translation=bool(q & 1))
        blocks[q] = tv.normalised(pix)
    return blocks, np.full(n_pairs, m, np.int32), good


def best_of(f, reps):
    best, out = float("inf"), None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = f()
        best = min(best, time.perf_counter() - t0)
    return best * 1e3, out


def device_ms(ctx, blocks, counts, rounds, reps):
    import torch
    n, stride = blocks.shape[:2]
    with torch.cuda.stream(ctx.torch_stream):
        d_corr = torch.from_numpy(blocks).to("cuda"); d_counts = torch.from_numpy(counts).to("cuda")
        d_mask = torch.empty((n, stride), dtype=torch.uint8, device="cuda"); d_cnt = torch.empty(n, dtype=torch.int32, device="cuda")
        d_F = torch.empty((n, 9), dtype=torch.float64, device="cuda"); d_win = torch.empty(n, dtype=torch.int32, device="cuda")
        best = float("inf")
        for it in range(reps + 1):
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            ctx.verify_pairs_dev(d_corr, stride, d_counts, n, T, d_mask, d_cnt, d_F, d_win, hypotheses=H, rounds=rounds, seed=0)
            e1.record()
            e1.synchronize()
            if it:
                best = min(best, e0.elapsed_time(e1))
        return best, d_mask.cpu().numpy().astype(bool), d_win.cpu().numpy()


def host_baseline():
    exe = os.path.join(ROOT, "tests", "host", "geom_test")
    subprocess.check_call(["make", "-C", os.path.dirname(exe), "geom_test"], stdout=subprocess.DEVNULL)
    K = np.array([[tv.FOCAL, 0, tv.WIDTH / 2], [0, tv.FOCAL, tv.HEIGHT / 2], [0, 0, 1.0]])
    print("# host find_transform (findEssentialMat + recoverPose, sequential RANSAC) through tests/host/geom_test: wall clock of the process, best of 5")
    with tempfile.TemporaryDirectory() as d:
        for m in (16, 2000):
            pix, good = tv.two_view_scene(m, 0.3 if m > 16 else 0.0, 1000)
            with open(os.path.join(d, "in.bin"), "wb") as f:
                f.write(K.astype("<f8").tobytes()); f.write(struct.pack("<i", m))
                f.write(pix[:, :2].astype(np.float32).tobytes()); f.write(pix[:, 2:].astype(np.float32).tobytes())
            run = lambda: subprocess.run([exe, "essential", os.path.join(d, "in.bin"), os.path.join(d, "out.bin")], capture_output=True, check=True)      # noqa: E731
            ms, _ = best_of(run, 5)
            raw = open(os.path.join(d, "out.bin"), "rb").read()
            ok = struct.unpack_from("<i", raw, 0)[0]; nm = struct.unpack_from("<i", raw, 100)[0]
            mask = np.frombuffer(raw, np.uint8, nm, 104).astype(bool)
            kept = mask[good].mean() if nm == m else float("nan")
            print(f"  m {m:5d}: {ms:8.2f} ms  ok {ok}  kept {kept:.3f} of the true matches, {int(mask[~good].sum()) if nm == m else -1} wrong ones accepted")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=199)
    ap.add_argument("--rows", type=int, default=2000)
    ap.add_argument("--trace", action="store_true", help="the batch case with rounds 3, five calls: for a kernel trace")
    ap.add_argument("--host-baseline", action="store_true", help="only the host's find_transform on one pair (no GPU)")
    a = ap.parse_args()
    if a.host_baseline:
        host_baseline()
        return
    from sfm_opencv_amd import api
    ctx = api.Context(0, use_torch_stream=True)
    blocks, counts, good = batch(a.pairs, a.rows)
    if a.trace:
        for _ in range(5):
            td, mask, win = device_ms(ctx, blocks, counts, 3, 1)
        print(f"# traced: {a.pairs} pairs x {a.rows} rows, H {H}, rounds 3, 5 x 2 calls of sfmhip_verify_pairs_dev")
        ctx.close()
        return
    print(f"# best of {a.reps} after a warm-up; device ms: sfmhip_verify_pairs_dev on resident blocks between two stream events; call ms: host clock "
          f"around sfmhip_verify_pairs incl. H2D / D2H; H = {H}, t = 1 px, 30 % wrong matches, seed 0")
    print(f"# {'pairs':>5s} {'rows':>5s} {'rounds':>6s} {'device ms':>10s} {'call ms':>9s} {'kept':>6s} {'wrong':>7s}  models by round")
    for n_pairs in (a.pairs, 1):
        b, c, g = blocks[:n_pairs], counts[:n_pairs], good[:n_pairs]
        for rounds in (1, 3):
            td, mask, win = device_ms(ctx, b, c, rounds, a.reps)
            f = lambda: ctx.verify_pairs(list(b), T, hypotheses=H, rounds=rounds, seed=0)      # noqa: E731
            f()
            tc, out = best_of(f, a.reps)
            assert np.array_equal(np.stack(out[0]), mask)
            kept = (mask & g).sum() / g.sum(); wrong = (mask & ~g).sum() / (~g).sum()
            by_round = np.bincount(win[win >= 0] // H, minlength=rounds).tolist()
            print(f"  {n_pairs:5d} {a.rows:5d} {rounds:6d} {td:10.3f} {tc:9.2f} {kept:6.3f} {wrong:7.4f}  {by_round}", flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
