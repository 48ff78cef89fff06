"""AKAZE on the device (sfmhip_akaze_extract, csrc/akaze.hip): times on a 1024x768 (crazyhorse size) and a 3648x2736 (the reference's
desktop images) texture, by the method of experiments/time_sift.py (its texture, its clocks).

  call ms    host clock around the synchronous sfmhip_akaze_extract: upload of the image, every kernel, download of key points and rows
  device ms  sfmhip_akaze_extract_dev on a resident image between two events on the context's stream
both after a warm-up, best and median of --reps.

    python experiments/time_akaze.py [--sizes 768x1024,2736x3648] [--reps 7]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python experiments/time_akaze.py --trace 2736x3648
    python experiments/time_akaze.py --stats DIR|CSV --trace 2736x3648      # per-stage table of that trace
    python experiments/time_akaze.py --host BIN_DIR --threads 1             # the host extractor (NViewReconstruct --akaze --features-only), for scale"""
import argparse
import csv
import glob
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from time_sift import parse_size, texture, timed          # noqa: E402

STAGES = [("FED", ("akaze_fed_kernel",)), ("blurs", ("akaze_blur_rows_kernel", "akaze_blur_cols_kernel")),
          ("derivatives", ("akaze_deriv1_kernel", "akaze_det_kernel")), ("flow, k_percentile, gray, halfsample",
                                                                         ("akaze_flow_kernel", "akaze_hmax_kernel", "akaze_hist_kernel", "akaze_kcontrast_kernel",
                                                                          "akaze_gray_kernel", "akaze_half_kernel")),
          ("maxima (scan, keys, gather)", ("akaze_maxima_kernel", "akaze_key_kernel", "akaze_gather_kernel")), ("suppression", ("akaze_suppress",)),
          ("sub-pixel fit, keys, count", ("akaze_subpixel_kernel", "akaze_compact_kernel", "akaze_resp_key_kernel", "akaze_count_kernel")),
          ("the three radix sorts and the scan", ("setup_",)),
          ("orientation + descriptor", ("akaze_describe_kernel",))]


def device_ms(ctx, img, cap, reps):
    import torch
    with torch.cuda.stream(ctx.torch_stream):
        d_img = torch.from_numpy(img).to("cuda")
        d_kp = torch.empty((cap, 28), dtype=torch.uint8, device="cuda"); d_desc = torch.empty((cap, 61), dtype=torch.uint8, device="cuda")
        d_n = torch.zeros(1, dtype=torch.int32, device="cuda")
        ts = []
        for it in range(reps + 1):
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            ctx.akaze_extract_dev(d_img, d_kp, d_desc, d_n)
            e1.record()
            e1.synchronize()
            if it:
                ts.append(e0.elapsed_time(e1))
        return min(ts), float(np.median(ts)), int(d_n.item())


def suppression_rounds(xysr, ol):
    """rounds the suppression needs on a list of raw maxima in scan order (akaze_extrema stage 0): a candidate is resolved in the round after
    the last of its predecessors -- the earlier candidates of its level or the one below within 2 size + 1 of it (float, the kernel's
    test) -- so its round is 1 + the largest round among them, and the list needs the largest round of all"""
    x, y, size, level = xysr[:, 0], xysr[:, 1], xysr[:, 2], ol[:, 1]
    start = np.searchsorted(level, np.arange(18))          # sorted by level, and by y within a level
    rnd = np.zeros(len(level), np.int32)
    one, two = np.float32(1), np.float32(2)
    for c in range(len(level)):
        reach = two * size[c] + one
        r = 0
        for lv in (level[c] - 1, level[c]):
            if lv < 0:
                continue
            s0, s1 = start[lv], min(start[lv + 1], c)
            lo = s0 + np.searchsorted(y[s0:s1], y[c] - reach); hi = s0 + np.searchsorted(y[s0:s1], y[c] + reach, side="right")
            if hi > lo:
                dx = x[c] - x[lo:hi]; dy = y[c] - y[lo:hi]
                near = dx * dx + dy * dy <= reach * reach
                if near.any():
                    r = max(r, int(rnd[lo:hi][near].max()))
        rnd[c] = r + 1
    return int(rnd.max()) if len(rnd) else 0, np.bincount(rnd)[1:]


def run_times(sizes, reps):
    from sfm_opencv_amd import api
    ctx = api.Context(0, use_torch_stream=True)
    print(f"# warm-up, then best / median of {reps}; call ms: host clock around sfmhip_akaze_extract (image up, key points and rows down); "
          "device ms: sfmhip_akaze_extract_dev on a resident image between two stream events")
    print("# rounds: what the suppression needs on the image's raw maxima, counted on the host from the list (suppression_rounds); the first "
          "32 run over all workgroups")
    print(f"# {'image':>10s} {'key points':>10s} {'raw maxima':>10s} {'rounds':>6s} {'call best':>10s} {'call med':>9s} {'device best':>11s} {'device med':>10s}")
    for rows, cols in sizes:
        img = texture(rows, cols)
        n = len(ctx.akaze_extract(img)[0])
        raw_xysr, raw_ol = ctx.akaze_extrema(img, 0, cap=1 << 21)
        raw = len(raw_ol)
        rounds, per_round = suppression_rounds(raw_xysr, raw_ol)
        cap = n + 1024
        cb, cm, out = timed(lambda: ctx.akaze_extract(img, cap=cap), reps)
        db, dm, nd = device_ms(ctx, img, cap, reps)
        assert len(out[0]) == n == nd
        print(f"  {rows:5d}x{cols:<5d} {n:10d} {raw:10d} {rounds:6d} {cb:10.2f} {cm:9.2f} {db:11.3f} {dm:10.3f}", flush=True)
        print(f"#   candidates resolved per round: {' '.join(str(v) for v in per_round)}", flush=True)
    ctx.close()


def run_trace(size):
    from sfm_opencv_amd import api
    ctx = api.Context(0, use_torch_stream=True)
    img = texture(*size)
    cap = max(8192, size[0] * size[1] // 64)          # room for every row from the first call on: all traced extractions do the same work
    n = len(ctx.akaze_extract(img, cap=cap)[0])
    assert n < cap
    for _ in range(5):
        ctx.akaze_extract(img, cap=cap)
    print(f"# traced: {size[0]}x{size[1]}, {n} key points")
    ctx.close()


def run_stats(d, size):
    files = [d] if os.path.isfile(d) else sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True))
    assert files, f"no *kernel_stats.csv under {d}"
    rows = list(csv.DictReader(open(files[-1])))
    calls = [int(r["Calls"]) for r in rows if "akaze_gray_kernel" in r["Name"]][0]          # one launch per extraction
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    print(f"# per-stage device time of {calls} extractions on {size[0]}x{size[1]} (rocprofv3 --kernel-trace --stats), per call")
    print(f"# {'stage':40s} {'launches':>8s} {'us / call':>10s} {'share':>7s}")
    seen = 0.0
    for stage, subs in STAGES:
        rs = [r for r in rows if any(s in r["Name"] for s in subs)]
        ns = sum(float(r["TotalDurationNs"]) for r in rs); seen += ns
        print(f"  {stage:40s} {sum(int(r['Calls']) for r in rs) // calls:8d} {ns / calls / 1e3:10.1f} {100 * ns / total:6.1f}%")
    print(f"  {'(anything else)':40s} {'':8s} {(total - seen) / calls / 1e3:10.1f} {100 * (total - seen) / total:6.1f}%")
    print(f"  {'total':40s} {'':8s} {total / calls / 1e3:10.1f}")
    print("# the suppression's kernels (a round = one akaze_suppress_round_kernel + one _publish_; launches behind the last round return at once):")
    for r in rows:
        if "akaze_suppress" in r["Name"]:
            print(f"#   {r['Name'].split('(')[0]:34s} {int(r['Calls']) // calls:3d} launches {float(r['TotalDurationNs']) / calls / 1e3:8.1f} us per call, "
                  f"{float(r['MinNs']) / 1e3:.1f} .. {float(r['MaxNs']) / 1e3:.1f} us each")


def run_host(bin_dir, sizes, threads):
    """for scale only (the CPU of whatever machine this runs on)"""
    exe = os.path.join(bin_dir, "NViewReconstruct")
    print("# host extractor, for scale: wall time of NViewReconstruct --akaze --features-only on t copies of the image with t OpenMP threads")
    print(f"# {'image':>10s} {'threads':>7s} {'wall s':>8s} {'s / image':>9s}")
    for rows, cols in sizes:
        img = texture(rows, cols)
        for t in threads:
            with tempfile.TemporaryDirectory() as d:
                for i in range(t):
                    with open(os.path.join(d, "%02d.ppm" % i), "wb") as f:
                        f.write(b"P6\n%d %d\n255\n" % (cols, rows)); f.write(np.ascontiguousarray(img[:, :, ::-1]).tobytes())
                env = dict(os.environ, OMP_NUM_THREADS=str(t))
                t0 = time.perf_counter()
                subprocess.run([exe, d, d, "--akaze", "--features-only"], check=True, stdout=subprocess.DEVNULL, env=env)
                wall = time.perf_counter() - t0
            print(f"  {rows:5d}x{cols:<5d} {t:7d} {wall:8.2f} {wall / t:9.2f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="768x1024,2736x3648")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--trace", default="", help="ROWSxCOLS: a few calls of that size, for a kernel trace (with --stats: the size that was traced)")
    ap.add_argument("--stats", default="", help="directory of a rocprofv3 --kernel-trace --stats run of --trace: print its per-stage table")
    ap.add_argument("--host", default="", help="directory of the built drivers: time the host extractor instead")
    ap.add_argument("--threads", default="1")
    a = ap.parse_args()
    sizes = [parse_size(s) for s in a.sizes.split(",")]
    if a.stats:
        run_stats(a.stats, parse_size(a.trace))
    elif a.trace:
        run_trace(parse_size(a.trace))
    elif a.host:
        run_host(a.host, sizes, [int(t) for t in a.threads.split(",")])
    else:
        run_times(sizes, a.reps)


if __name__ == "__main__":
    main()
