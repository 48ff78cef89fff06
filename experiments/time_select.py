"""The view selection (sfmhip_select_views): --runs timed runs after a warm-up, median and min .. max, on sparse models of the sizes the
bundle adjustment is timed at.

  scenes      c4       synth.ba_scene(200, 300000): about 1.2 M observations, tracks of 2 to 6 consecutive views (a chain scene)
              c5       synth.ba_scene(1000, 2000000): about 8 M observations
              twoview  two views that both see every point, with c4's observation count: every add of the pair kernel lands on one
                       counter, the worst case for its atomics
  default     per scene: the call on resident arrays (between two events on the context's stream, every output asked for) and from host
              arrays (the host form on the host's clock, both copies included), and for scale, not as a speed-up, the numpy restatement
              of tests/select_ref.py on the same input, compared with the library's outputs (c5 is left out of it; --no-ref: no scene).
              Beside the resident time: the pair visits (sum over the tracks of L (L - 1) / 2) and the bytes the pair kernel must read
              at least (keys, heads and rays of the sorted list once: 44 bytes per observation).
  --trace SCENE   the resident call alone, a warm-up and --runs runs, for a kernel trace of its own:
                  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python experiments/time_select.py --trace c4
  --stats DIR     the per-kernel split of such a trace, per call: the radix sort's and the scan's kernels (sortscan.hip) against each
                  kernel of select.hip

    python experiments/time_select.py [--runs 5] [--scenes c4,c5,twoview] [--no-ref]
"""
import argparse
import csv
import glob
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_SRC, MIN_ANGLE = 4, 1.0
NAMES = ("shared", "score", "sources", "n_scored", "wrange", "n_depth")


def spread(v):
    return f"{statistics.median(v):9.3f} ({min(v):.3f} .. {max(v):.3f})"


def scene(name):
    """(ext, pts, obs_cam, obs_pt)"""
    from sfm_opencv_amd import synth
    if name in ("c4", "c5"):
        n_cam, n_pt = (200, 300000) if name == "c4" else (1000, 2000000)
        sc = synth.ba_scene(n_cam, n_pt)
        return sc["ext_true"], sc["pts_true"], sc["obs_cam"], sc["obs_pt"]
    if name == "twoview":
        n = len(scene("c4")[2]) // 2
        rng = np.random.default_rng(4)
        pts = np.stack([rng.uniform(-3, 3, n), rng.uniform(-2, 2, n), rng.uniform(4, 9, n)], 1)
        ext = np.array([[0, 0, 0, 0, 0, 0], [0.0, -0.05, 0.0, -0.6, 0, 0]], float)
        order = rng.permutation(2 * n)                                       # no order the sort could profit from
        return ext, pts, np.repeat([0, 1], n).astype(np.int32)[order], np.tile(np.arange(n), 2).astype(np.int32)[order]
    raise ValueError(name)


def resident(ctx, torch, ext, pts, oc, op, n_src):
    n = len(ext)
    dev = torch.device("cuda", ctx.device)
    d_in = (torch.from_numpy(np.ascontiguousarray(pts)).to(dev), torch.from_numpy(np.ascontiguousarray(oc, np.int32)).to(dev),
            torch.from_numpy(np.ascontiguousarray(op, np.int32)).to(dev))
    d_out = dict(shared=torch.empty((n, n), dtype=torch.int32, device=dev), score=torch.empty((n, n), dtype=torch.int32, device=dev),
                 sources=torch.empty((n, n_src), dtype=torch.int32, device=dev), n_scored=torch.empty(n, dtype=torch.int32, device=dev),
                 wrange=torch.empty((n, 2), dtype=torch.float64, device=dev), n_depth=torch.empty(n, dtype=torch.int32, device=dev))
    torch.cuda.synchronize(dev)

    def call():
        ctx.select_views_dev(ext, d_in[0], len(pts), d_in[1], d_in[2], len(oc), n_src, MIN_ANGLE, *[d_out[k] for k in NAMES])
    return call, d_out


def pair_visits(oc, op):
    L = np.bincount(np.unique(np.asarray(op, np.int64) * 4096 + np.asarray(oc, np.int64)) // 4096)
    return int((L * (L - 1) // 2).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--scenes", default="c4,c5,twoview")
    ap.add_argument("--no-ref", action="store_true")
    ap.add_argument("--trace", default=None)
    ap.add_argument("--stats", default=None)
    a = ap.parse_args()
    if a.stats:
        return stats(a.stats)
    import torch
    from sfm_opencv_amd import api
    ctx = api.Context(0, use_torch_stream=True)
    if a.trace:
        ext, pts, oc, op = scene(a.trace)
        n_src = min(N_SRC, len(ext) - 1)
        call, _ = resident(ctx, torch, ext, pts, oc, op, n_src)
        for _ in range(a.runs + 1):
            call()
            ctx.synchronize()
        print(f"traced {a.trace}: {a.runs + 1} calls")
        return 0
    import select_ref as sr
    print(f"sfmhip_select_views, n_src {N_SRC}, min angle {MIN_ANGLE} deg; times in ms, median (min .. max) of {a.runs} runs after a warm-up")
    for name in a.scenes.split(","):
        ext, pts, oc, op = scene(name)
        n_src = min(N_SRC, len(ext) - 1)
        visits = pair_visits(oc, op)
        print(f"\n{name}: {len(ext)} views, {len(pts)} points, {len(oc)} observations, {visits} pair visits")
        call, d_out = resident(ctx, torch, ext, pts, oc, op, n_src)
        call(); ctx.synchronize()
        ms = []
        for _ in range(a.runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); call(); e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        print(f"  resident arrays (events)         {spread(ms)}   pair kernel reads at least {44 * len(oc) / 1e6:.1f} MB")
        ctx.select_views(ext, pts, oc, op, n_src, MIN_ANGLE)
        hs = []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            got = ctx.select_views(ext, pts, oc, op, n_src, MIN_ANGLE)
            hs.append(1e3 * (time.perf_counter() - t0))
        print(f"  host arrays, both copies (clock) {spread(hs)}")
        same = all(np.array_equal(d_out[k].cpu().numpy(), getattr(got, k)) for k in NAMES)
        print(f"  the two forms agree: {same}")
        if not a.no_ref and name != "c5":
            t0 = time.perf_counter()
            exp = sr.select_views(ext, pts, oc, op, n_src, sr.cos2_of(MIN_ANGLE), api.sweep_geometry)
            t1 = time.perf_counter()
            ok = all(np.asarray(getattr(got, k)).tobytes() == exp[k].tobytes() for k in NAMES)
            print(f"  numpy restatement (clock, once)  {1e3 * (t1 - t0):9.1f}   equal to the library in every bit: {ok}")
        print(f"  hottest counter: shared max {int(got.shared.max())}, score max {int(got.score.max())}; sources by score: {int(got.n_scored.sum())} of {got.sources.size}")
    ctx.close()
    return 0


def stats(d):
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        print("no kernel_stats.csv under", d)
        return 1
    rows = []
    for f in files:
        rows += list(csv.DictReader(open(f)))
    calls = max((int(r["Calls"]) for r in rows if "select_pair_kernel" in r["Name"] or "select_rank_kernel" in r["Name"]), default=1)
    group = {}
    for r in rows:
        nm = r["Name"]
        key = ("sort: " if "sfm_sort" in nm else "scan: " if "sfm_scan" in nm else "") + nm.split("(")[0]
        g = group.setdefault(key, [0, 0.0])
        g[0] += int(r["Calls"]); g[1] += float(r["TotalDurationNs"])
    total = sum(v[1] for v in group.values())
    print(f"{calls} calls traced; per call, microseconds (launches)")
    for key, (n, ns) in sorted(group.items(), key=lambda kv: -kv[1][1]):
        print(f"  {key:48s} {ns / calls / 1e3:10.1f}  ({n / calls:5.1f})  {100 * ns / total:5.1f} %")
    sortscan = sum(v[1] for k, v in group.items() if k.startswith(("sort: ", "scan: ")) or "sfm_run_head" in k)
    print(f"  sorts, scans and run heads together {sortscan / calls / 1e3:10.1f}  {100 * sortscan / total:5.1f} %;  all kernels {total / calls / 1e3:10.1f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
