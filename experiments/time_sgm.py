"""Semi-global aggregation of the sweep's cost volume (sfmhip_sweep_costs, sfmhip_sgm_depth, sfmhip_plane_sweep_sgm): warm-up first, best
of --reps.  The views and the cases are those of experiments/time_dense.py: 1024 x 768 and 3648 x 2736, 64 and 128 planes, r = 2, two
sources, images resident.  Eight paths, cost_scale 262144, P1 = 512, P2 = 4096.

  default     between two events on the context's stream: the cost sweep (sfmhip_sweep_costs_dev), the aggregation with its winner
              (sfmhip_sgm_depth_dev, 4 and 8 paths), the fused call (sfmhip_plane_sweep_sgm_dev) and, for scale, the winner-take-all sweep
              (sfmhip_plane_sweep_dev); the share of pixels that get a depth either way
  --trace DIR / --stats DIR   the kernels of the fused call one by one, from a kernel trace:
                  rocprofv3 --kernel-trace --output-format csv -d DIR -- python experiments/time_sgm.py --trace DIR
                  python experiments/time_sgm.py --stats DIR
              per case the cost kernel, each of the eight path passes in the header's order, and the winner, best of the traced calls but
              the first; beside the passes their algorithmic bytes (a pass reads the costs, 2 bytes, and reads and writes S, 4 + 4 bytes,
              per pixel and plane; the first pass only writes S) and the fraction of --copy-rate they reach
  --against LIB   sfmhip_plane_sweep_dev of this tree's library and of another build of it (the parent commit's), loaded side by side in
              this process and run in turns, --runs times a side, each the best of --reps on the host's clock around the call and a
              synchronise: the two ranges per case

    python experiments/time_sgm.py [--reps 3] [--sizes 1024x768,3648x2736]
"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from time_dense import N_SRC, R, WMAX, WMIN, views          # noqa: E402

SCALE, P1, P2, MAX_COST = 262144.0, 512, 4096, 65535
DIRECTIONS = ["(0,1)", "(0,-1)", "(1,0)", "(-1,0)", "(1,1)", "(-1,-1)", "(1,-1)", "(-1,1)"]


def cases(sizes):
    for size in sizes.split(","):
        cols, rows = (int(x) for x in size.split("x"))
        yield rows, cols, views(rows, cols)


def run_events(a):
    import torch
    from sfm_opencv_amd import api
    ctx = api.Context(0, use_torch_stream=True)
    print(f"# best of {a.reps} after a warm-up; r = {R}, {N_SRC} sources, w in [1/8, 1/3], resident images; events on the context's stream; ms")
    print(f"# {'size':>11s} {'planes':>6s} {'costs':>8s} {'sgm 4':>8s} {'sgm 8':>8s} {'fused 8':>8s} {'wta sweep':>9s} {'depth sgm':>9s} {'depth wta':>9s}")
    for rows, cols, (sc, images) in cases(a.sizes):
        sources = api.dense_sources(sc.EXT, N_SRC)
        A, b, *_ = api.sweep_geometry(sc.K4, sc.EXT[0], sc.EXT[sources[0]])
        npx = rows * cols
        with torch.cuda.stream(ctx.torch_stream):
            d_img = [torch.from_numpy(im).to("cuda") for im in images]
            d_src = [d_img[j] for j in sources[0]]
            d_plane = torch.empty(npx, dtype=torch.int32, device="cuda"); d_cost = torch.empty(npx, dtype=torch.int16, device="cuda")
            d_score = torch.empty(npx, dtype=torch.float32, device="cuda"); d_depth = torch.empty(npx, dtype=torch.float32, device="cuda")
            for D in (64, 128):
                d_vol = torch.empty(npx * D, dtype=torch.int16, device="cuda")

                def timed(f):
                    best = float("inf")
                    for it in range(a.reps + 1):
                        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
                        e0.record(); f(); e1.record(); e1.synchronize()
                        if it:
                            best = min(best, e0.elapsed_time(e1))
                    return best
                t_cost = timed(lambda: ctx.sweep_costs_dev(d_img[0], d_src, rows, cols, 1, cols, A, b, D, WMIN, WMAX, R, 1, SCALE, d_vol))
                t_sgm = [timed(lambda: ctx.sgm_depth_dev(d_vol, rows, cols, D, WMIN, WMAX, P1, P2, p, MAX_COST, d_plane, d_cost, None, d_depth)) for p in (4, 8)]
                t_fused = timed(lambda: ctx.plane_sweep_sgm_dev(d_img[0], d_src, rows, cols, 1, cols, A, b, D, WMIN, WMAX, R, 1, SCALE, P1, P2, 8, MAX_COST, d_plane,
                                                                d_cost, d_depth))
                got_sgm = float((d_plane >= 0).float().mean())
                t_wta = timed(lambda: ctx.plane_sweep_dev(d_img[0], d_src, rows, cols, 1, cols, A, b, D, WMIN, WMAX, R, 1, -1.0, d_plane, d_score, d_depth))
                got_wta = float((d_plane >= 0).float().mean())
                print(f"  {cols:5d}x{rows:<5d} {D:6d} {t_cost:8.3f} {t_sgm[0]:8.3f} {t_sgm[1]:8.3f} {t_fused:8.3f} {t_wta:9.3f} {got_sgm:9.3f} {got_wta:9.3f}", flush=True)
                del d_vol
    ctx.close()


def run_trace(a):
    import torch
    from sfm_opencv_amd import api
    ctx = api.Context(0, use_torch_stream=True)
    plan = []
    for rows, cols, (sc, images) in cases(a.sizes):
        sources = api.dense_sources(sc.EXT, N_SRC)
        A, b, *_ = api.sweep_geometry(sc.K4, sc.EXT[0], sc.EXT[sources[0]])
        npx = rows * cols
        with torch.cuda.stream(ctx.torch_stream):
            d_img = [torch.from_numpy(im).to("cuda") for im in images]
            d_plane = torch.empty(npx, dtype=torch.int32, device="cuda"); d_cost = torch.empty(npx, dtype=torch.int16, device="cuda")
            d_depth = torch.empty(npx, dtype=torch.float32, device="cuda")
            for D in (64, 128):
                for _ in range(a.reps + 1):
                    ctx.plane_sweep_sgm_dev(d_img[0], [d_img[j] for j in sources[0]], rows, cols, 1, cols, A, b, D, WMIN, WMAX, R, 1, SCALE, P1, P2, 8, MAX_COST, d_plane,
                                            d_cost, d_depth)
                ctx.synchronize()
                plan.append(dict(rows=rows, cols=cols, D=D, calls=a.reps + 1))
    with open(os.path.join(a.trace, "manifest.json"), "w") as f:
        json.dump(plan, f)
    ctx.close()


def run_stats(a):
    plan = json.load(open(os.path.join(a.stats, "manifest.json")))
    tr = sorted(glob.glob(os.path.join(a.stats, "**", "*kernel_trace.csv"), recursive=True))
    assert tr, f"no *kernel_trace.csv under {a.stats}"
    rows = [r for r in csv.DictReader(open(tr[-1])) if "sgm_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    print(f"# the kernels of sfmhip_plane_sweep_sgm_dev (rocprofv3 --kernel-trace), ms, best of the calls but the first; GB: what a path pass must move")
    print(f"# (2 bytes of cost read and 4 + 4 of S read and written per pixel and plane, the first pass 2 + 4); share: of {a.copy_rate} TB/s")
    at = 0
    for p in plan:
        best = {}
        for call in range(p["calls"]):
            seq = rows[at:at + 10]; at += 10
            names = [("sgm_cost_kernel" in seq[0]["Kernel_Name"])] + [("sgm_path_kernel" in r["Kernel_Name"]) for r in seq[1:9]] + [("sgm_winner_kernel" in seq[9]["Kernel_Name"])]
            assert all(names), [r["Kernel_Name"][:30] for r in seq]
            if call:
                for i, r in enumerate(seq):
                    ms = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
                    best[i] = min(best.get(i, float("inf")), ms)
        vol = p["rows"] * p["cols"] * p["D"]
        print(f"  {p['cols']}x{p['rows']} {p['D']} planes: cost kernel {best[0]:.3f}, winner {best[9]:.3f}, the ten {sum(best.values()):.3f}")
        for i in range(8):
            gb = vol * (6 if i == 0 else 10) / 1e9
            steps = p["cols"] if i < 2 else p["rows"] if i < 4 else min(p["rows"], p["cols"])
            print(f"    path {DIRECTIONS[i]:>7s} {best[1 + i]:8.3f} ms {gb:7.3f} GB {gb / best[1 + i] / a.copy_rate:6.3f} of the copy rate; {best[1 + i] * 1e6 / steps:7.1f} ns per step of the longest line")
    assert at == len(rows), (at, len(rows))


class Bare:
    """sfmhip_plane_sweep_dev of one build of the library, bound by hand (another build need not have this tree's symbols)"""

    def __init__(self, path):
        self.lib = C.CDLL(path)
        self.h = C.c_void_p()
        self.lib.sfmhip_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        assert self.lib.sfmhip_create(0, C.byref(self.h)) == 0
        vp, i32, f64 = C.c_void_p, C.c_int, C.c_double
        self.lib.sfmhip_plane_sweep_dev.argtypes = [vp, vp, C.POINTER(vp), i32, i32, i32, i32, C.c_size_t, vp, vp, i32, f64, f64, i32, i32, f64, vp, vp, vp]
        self.lib.sfmhip_synchronize.argtypes = [vp]
        self.lib.sfmhip_destroy.argtypes = [vp]

    def sweep_ms(self, d_ref, d_src, rows, cols, A, b, D, outs, reps):
        src = (C.c_void_p * 8)(*[t.data_ptr() for t in d_src])
        best = float("inf")
        for it in range(reps + 1):
            t0 = time.perf_counter()
            rc = self.lib.sfmhip_plane_sweep_dev(self.h, d_ref.data_ptr(), src, len(d_src), rows, cols, 1, cols, A.ctypes.data, b.ctypes.data, D, WMIN, WMAX, R, 1, -1.0,
                                                 *[t.data_ptr() for t in outs])
            assert rc == 0 and self.lib.sfmhip_synchronize(self.h) == 0
            if it:
                best = min(best, (time.perf_counter() - t0) * 1e3)
        return best


def run_against(a):
    import torch
    from sfm_opencv_amd import _lib, api
    builds = {"this tree": Bare(_lib.LIB_PATH), "other build": Bare(a.against)}
    print(f"# sfmhip_plane_sweep_dev, ms: {a.runs} runs a side in turns, each the best of {a.reps} after a warm-up (host clock around the call and a synchronise)")
    print(f"# this tree: {os.path.relpath(_lib.LIB_PATH, ROOT)}; other build: {a.against}")
    for rows, cols, (sc, images) in cases(a.sizes):
        sources = api.dense_sources(sc.EXT, N_SRC)
        A, b, *_ = api.sweep_geometry(sc.K4, sc.EXT[0], sc.EXT[sources[0]])
        npx = rows * cols
        d_img = [torch.from_numpy(im).to("cuda") for im in images]
        outs = [torch.empty(npx, dtype=torch.int32, device="cuda"), torch.empty(npx, dtype=torch.float32, device="cuda"), torch.empty(npx, dtype=torch.float32, device="cuda")]
        torch.cuda.synchronize()
        for D in (64, 128):
            ms = {k: [] for k in builds}
            for run in range(a.runs):
                for k, bld in list(builds.items())[::-1 if run % 2 else 1]:          # who goes first changes with every turn
                    ms[k].append(bld.sweep_ms(d_img[0], [d_img[j] for j in sources[0]], rows, cols, A, b, D, outs, a.reps))
            lo = max(min(v) for v in ms.values()); hi = min(max(v) for v in ms.values())
            print(f"  {cols:5d}x{rows:<5d} {D:4d} planes: " + "; ".join(f"{k} {min(v):.3f} .. {max(v):.3f}" for k, v in ms.items()) + f"; the ranges overlap: {lo <= hi}", flush=True)
    for bld in builds.values():
        bld.lib.sfmhip_destroy(bld.h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--sizes", default="1024x768,3648x2736")
    ap.add_argument("--trace", default="", help="directory for manifest.json: a few fused calls per case, for a kernel trace")
    ap.add_argument("--stats", default="", help="directory of a rocprofv3 --kernel-trace run of --trace: print its per-kernel table")
    ap.add_argument("--against", default="", help="another build of libsfmhip.so whose sfmhip_plane_sweep_dev is timed in turns with this tree's")
    ap.add_argument("--copy-rate", type=float, default=6.29, help="achievable copy rate of the device in TB/s")
    a = ap.parse_args()
    if a.stats:
        run_stats(a)
    elif a.trace:
        run_trace(a)
    elif a.against:
        run_against(a)
    else:
        run_events(a)


if __name__ == "__main__":
    main()
