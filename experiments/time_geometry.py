"""Homography RANSAC and F/H model selection (sfmhip_verify_pairs_h, sfmhip_two_view_geometry): warm-up first, best of --reps.

The batch case is the chain case of time_verify.py: 199 pairs x 2000 correspondences (30 % wrong matches, 0.5 px noise), H = 1024,
rounds 1 and 3, t_f = 1 px and t_h = 2 px on coordinates normalised by f = 800.  The pairs cycle through the three scene kinds of
tests/homography_ref.py (general, planar, rotation-only), so that both models have work in every round.  Each of the three calls (F
alone, H alone, both with the selection) is timed with the blocks resident (the _dev call between two events on the context's stream)
and from host arrays (host clock around the synchronous call, both copies included).

    python experiments/time_geometry.py [--reps 5]
    rocprofv3 --kernel-trace --stats -d DIR -- python experiments/time_geometry.py --trace      # the combined call, rounds 3, five calls
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import homography_ref as hr  # noqa: E402  (the scene generators only)
import twoview_ref as tv  # noqa: E402

TF = 1.0 / tv.FOCAL
TH = 2.0 / tv.FOCAL
H = 1024
KINDS = ("general", "planar", "rotation")


def batch(n_pairs, m):
    blocks = np.empty((n_pairs, m, 4))
    good = np.empty((n_pairs, m), bool)
    for q in range(n_pairs):
        pix, good[q] = hr.scene(KINDS[q % 3], m, 0.3, 1000 + q)
        blocks[q] = tv.normalised(pix)
    return blocks, np.full(n_pairs, m, np.int32), good


def best_of(f, reps):
    best, out = float("inf"), None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = f()
        best = min(best, time.perf_counter() - t0)
    return best * 1e3, out


def device_ms(ctx, which, blocks, counts, rounds, reps):
    """(best ms, kind or None, mask bool, counts2 or None) of one of the three _dev calls on resident blocks"""
    import torch
    n, stride = blocks.shape[:2]
    with torch.cuda.stream(ctx.torch_stream):
        d_corr = torch.from_numpy(blocks).to("cuda"); d_counts = torch.from_numpy(counts).to("cuda")
        d_mask = torch.empty((n, stride), dtype=torch.uint8, device="cuda"); d_cnt = torch.empty(n, dtype=torch.int32, device="cuda")
        d_F = torch.empty((n, 9), dtype=torch.float64, device="cuda"); d_Hm = torch.empty((n, 9), dtype=torch.float64, device="cuda")
        d_win = torch.empty((n, 2), dtype=torch.int32, device="cuda"); d_kind = torch.zeros(n, dtype=torch.int32, device="cuda")
        d_c2 = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
        best = float("inf")
        for it in range(reps + 1):
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            if which == "F":
                ctx.verify_pairs_dev(d_corr, stride, d_counts, n, TF, d_mask, d_cnt, d_F, d_win, hypotheses=H, rounds=rounds, seed=0)
            elif which == "H":
                ctx.verify_pairs_h_dev(d_corr, stride, d_counts, n, TH, d_mask, d_cnt, d_Hm, d_win, hypotheses=H, rounds=rounds, seed=0)
            else:
                ctx.two_view_geometry_dev(d_corr, stride, d_counts, n, TF, TH, d_kind, d_mask, d_cnt, d_c2, d_F, d_Hm, d_win, hypotheses=H, rounds=rounds,
                                          seed=0)
            e1.record()
            e1.synchronize()
            if it:
                best = min(best, e0.elapsed_time(e1))
        both = which == "F+H"
        return best, d_kind.cpu().numpy() if both else None, d_mask.cpu().numpy().astype(bool), d_c2.cpu().numpy() if both else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=199)
    ap.add_argument("--rows", type=int, default=2000)
    ap.add_argument("--trace", action="store_true", help="the combined call on the batch with rounds 3, five calls: for a kernel trace")
    a = ap.parse_args()
    from sfm_opencv_amd import api
    ctx = api.Context(0, use_torch_stream=True)
    blocks, counts, good = batch(a.pairs, a.rows)
    if a.trace:
        for _ in range(5):
            device_ms(ctx, "F+H", blocks, counts, 3, 1)
        print(f"# traced: {a.pairs} pairs x {a.rows} rows, H {H}, rounds 3, 5 x 2 calls of sfmhip_two_view_geometry_dev")
        ctx.close()
        return
    want = np.array([1 if KINDS[q % 3] == "general" else 2 for q in range(a.pairs)])
    print(f"# best of {a.reps} after a warm-up; device ms: the _dev call on resident blocks between two stream events; call ms: host clock around the "
          f"synchronous call incl. H2D / D2H; H = {H}, t_f = 1 px, t_h = 2 px, 30 % wrong matches, seed 0; pairs cycle general / planar / rotation-only")
    print(f"# {'call':>5s} {'pairs':>5s} {'rows':>5s} {'rounds':>6s} {'device ms':>10s} {'call ms':>9s} {'kept':>6s} {'wrong':>7s}  kinds right")
    for n_pairs in (a.pairs, 1):
        b, c, g = blocks[:n_pairs], counts[:n_pairs], good[:n_pairs]
        for which in ("F", "H", "F+H"):
            for rounds in (1, 3):
                td, kind, mask, c2 = device_ms(ctx, which, b, c, rounds, a.reps)
                if which == "F":
                    f = lambda: ctx.verify_pairs(list(b), TF, hypotheses=H, rounds=rounds, seed=0)[0]      # noqa: E731
                elif which == "H":
                    f = lambda: ctx.verify_pairs_h(list(b), TH, hypotheses=H, rounds=rounds, seed=0)[0]      # noqa: E731
                else:
                    f = lambda: ctx.two_view_geometry(list(b), TF, TH, hypotheses=H, rounds=rounds, seed=0)[1]      # noqa: E731
                f()
                tc, out = best_of(f, a.reps)
                assert np.array_equal(np.stack(out), mask)
                kept = (mask & g).sum() / g.sum(); wrong = (mask & ~g).sum() / (~g).sum()
                right = f"{int((kind == want[:n_pairs]).sum())} of {n_pairs}" if kind is not None else "-"
                print(f"  {which:>5s} {n_pairs:5d} {a.rows:5d} {rounds:6d} {td:10.3f} {tc:9.2f} {kept:6.3f} {wrong:7.4f}  {right}", flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
