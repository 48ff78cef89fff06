"""The track builder (sfmhip_build_tracks): --runs timed runs after a warm-up, median and min .. max.

  cases       chain    200 images x about 5000 key points, the 199 consecutive pairs (synth.ba_scene(200, 250000) as key points and lists)
              reach5   1000 images x about 2000 key points, every pair within reach 5 (synth.ba_scene(1000, 500000))
              giant    2 images x 1 M key points, one list k - k and one that links every key point of the second image to key point 0
                       of the first: one component of 2 M features, every union meets one root
  default     per case: the call on resident arrays (between two events on the context's stream, every output asked for) and from host
              arrays (the host form on the host's clock, all copies included), and for scale, not as a speed-up, the Python restatement
              of tests/tracks_ref.py on the chain case, compared with the library's outputs (--no-ref: not run).
  --trace CASE    the resident call alone, a warm-up and --runs runs, for a kernel trace of its own:
                  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python experiments/time_tracks.py --trace chain
  --stats DIR     the per-kernel split of such a trace, per call: the radix sort's and the scan's kernels (sortscan.hip) against each
                  kernel of tracks.hip

    python experiments/time_tracks.py [--runs 5] [--cases chain,reach5,giant] [--no-ref]
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

NAMES = ("track_of", "obs_cam", "obs_pt", "obs_kp", "obs_uv", "track_len", "matches_out", "counts_out", "stats")


def spread(v):
    return f"{statistics.median(v):9.3f} ({min(v):.3f} .. {max(v):.3f})"


def case(name):
    """(n_kp, pairs, matches, counts, kp)"""
    import tracks_ref as tr
    from sfm_opencv_amd import synth
    if name in ("chain", "reach5"):
        sc = synth.ba_scene(200, 250000) if name == "chain" else synth.ba_scene(1000, 500000)
        kp, _, pairs, lists, _ = tr.scene_lists(sc, 1 if name == "chain" else 5)
        return (np.array([len(k) for k in kp], np.int32), pairs) + tr.pack(lists) + (kp,)
    if name == "giant":
        n = 1000000
        m = np.zeros((2, n), tr.DMATCH)
        m["queryIdx"][0] = np.arange(n); m["trainIdx"] = np.arange(n)[None, :]
        kp = [np.zeros(n, tr.KEYPOINT), np.zeros(n, tr.KEYPOINT)]
        return np.array([n, n], np.int32), np.array([(0, 1), (0, 1)], np.int32), m, np.array([n, n], np.int32), kp
    raise ValueError(name)


def resident(ctx, torch, n_kp, pairs, m, c, kp, conflicts):
    dev = torch.device("cuda", ctx.device)
    n = int(n_kp.sum()); P, S = m.shape
    d_m = torch.from_numpy(m.view(np.uint8).reshape(P, S * 16)).to(dev); d_c = torch.from_numpy(c).to(dev)
    d_kp = [torch.from_numpy(k.view(np.uint8)).to(dev) for k in kp]
    i32 = dict(dtype=torch.int32, device=dev)
    d_out = dict(track_of=torch.empty(n, **i32), obs_cam=torch.empty(n, **i32), obs_pt=torch.empty(n, **i32), obs_kp=torch.empty(n, **i32),
                 obs_uv=torch.empty((n, 2), dtype=torch.float64, device=dev), track_len=torch.empty(n // 2, **i32),
                 matches_out=torch.empty((P, S * 16), dtype=torch.uint8, device=dev), counts_out=torch.empty(P, **i32), stats=torch.empty(8, **i32))
    torch.cuda.synchronize(dev)

    def call():
        ctx.build_tracks_dev(n_kp, pairs, d_m, S, d_c, d_kp, 2, conflicts, *[d_out[k] for k in NAMES])
    return call, d_out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--cases", default="chain,reach5,giant")
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
        n_kp, pairs, m, c, kp = case(a.trace)
        call, _ = resident(ctx, torch, n_kp, pairs, m, c, kp, "keep-first")
        for _ in range(a.runs + 1):
            call()
            ctx.synchronize()
        print(f"traced {a.trace}: {a.runs + 1} calls")
        return 0
    import tracks_ref as tr
    print(f"sfmhip_build_tracks, min_len 2, keep-first; times in ms, median (min .. max) of {a.runs} runs after a warm-up")
    for name in a.cases.split(","):
        n_kp, pairs, m, c, kp = case(name)
        n = int(n_kp.sum())
        print(f"\n{name}: {len(n_kp)} images, {n} features, {len(pairs)} pairs x {m.shape[1]} slots, {int(c.sum())} elements")
        call, d_out = resident(ctx, torch, n_kp, pairs, m, c, kp, "keep-first")
        call(); ctx.synchronize()
        ms = []
        for _ in range(a.runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); call(); e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        print(f"  resident arrays (events)         {spread(ms)}")
        ctx.build_tracks(n_kp, pairs, m, c, kp=kp, conflicts="keep-first")
        hs = []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            got = ctx.build_tracks(n_kp, pairs, m, c, kp=kp, conflicts="keep-first")
            hs.append(1e3 * (time.perf_counter() - t0))
        print(f"  host arrays, all copies (clock)  {spread(hs)}")
        st = d_out["stats"].cpu().numpy()
        same = np.array_equal(st, got[6]) and np.array_equal(d_out["track_of"].cpu().numpy(), got[0]) and np.array_equal(d_out["obs_uv"].cpu().numpy()[:st[1]], got[4])
        print(f"  the two forms agree: {same};  stats {st.tolist()}")
        if not a.no_ref and name == "chain":
            t0 = time.perf_counter()
            exp = tr.build_tracks(n_kp, pairs, m, c, 2, tr.KEEP_FIRST, kp)
            t1 = time.perf_counter()
            ok = all(np.array_equal(g, exp[k]) for g, k in zip(got[:4] + (got[5], got[6], got[8]), ("track_of", "obs_cam", "obs_pt", "obs_kp", "track_len", "stats", "counts_out")))
            print(f"  Python restatement (clock, once) {1e3 * (t1 - t0):9.1f}   equal to the library: {ok}")
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
    calls = max((int(r["Calls"]) for r in rows if "tracks_link_kernel" in r["Name"]), default=1)
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
