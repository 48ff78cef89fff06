"""SIFT on the device (sfmhip_sift_extract, csrc/sift.hip): times on a 1024x768 (crazyhorse size) and a 3648x2736 (the reference's desktop
images) texture.

  call ms    host clock around the synchronous sfmhip_sift_extract: upload of the image, every kernel, download of key points and descriptors
  device ms  sfmhip_sift_extract_dev on a resident image between two events on the context's stream
both after a warm-up, best and median of --reps.

    python experiments/time_sift.py [--sizes 768x1024,2736x3648] [--reps 7]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python experiments/time_sift.py --trace 2736x3648      # a few calls of one size
    python experiments/time_sift.py --stats DIR|CSV --trace 2736x3648      # per-kernel table of that trace; the blur passes against their bytes
    python experiments/time_sift.py --host BIN_DIR --threads 1,16      # the host extractor (NViewReconstruct --sift --features-only), for scale

The bytes a blur pass must move are counted from the level sizes: a float read and a float written per pixel, and for the column pass of a
level that yields a DoG the previous level read and the DoG written as well."""
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

HBM_GBS = 8000.0          # MI355X peak HBM bandwidth, GB/s


def texture(h, w, seed=5):
    """the blobs-on-a-gradient recipe of tests/test_features_cpu.py at any size: 700 blobs per 480x360 pixels, each drawn inside 4 sigma"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    img = 90 + 30 * np.sin(xx / 97.0) + 20 * np.cos(yy / 71.0)
    for _ in range(int(700 * h * w / (480 * 360))):
        cx, cy = rng.uniform(0, w), rng.uniform(0, h)
        s = rng.uniform(2.0, 9.0); a = rng.uniform(-70, 70)
        x0, x1 = max(int(cx - 4 * s), 0), min(int(cx + 4 * s) + 1, w); y0, y1 = max(int(cy - 4 * s), 0), min(int(cy + 4 * s) + 1, h)
        img[y0:y1, x0:x1] += a * np.exp(-((xx[y0:y1, x0:x1] - cx) ** 2 + (yy[y0:y1, x0:x1] - cy) ** 2) / (2 * s * s))
    g = np.clip(img, 0, 255)
    return np.stack([g * 0.8, g * 0.9, g], 2).astype(np.uint8)          # BGR


def level_sizes(rows, cols):
    """[(rows, cols)] per octave, the rule of build_pyramid"""
    H, W = 2 * rows, 2 * cols
    n_oct = max(1, int(np.floor(np.log2(min(H, W)) - 2.0 + 0.5)))
    out = []
    for o in range(n_oct):
        if o > 0:
            if H < 24 or W < 24:
                break
            H, W = H // 2, W // 2
        out.append((H, W))
    return out


def blur_bytes(rows, cols):
    """(row-pass bytes, column-pass bytes) of one extraction"""
    rb = cb = 0
    for o, (H, W) in enumerate(level_sizes(rows, cols)):
        px = H * W
        n_plain = 1 if o == 0 else 0          # the base blur: no DoG
        rb += (5 + n_plain) * 8 * px
        cb += n_plain * 8 * px + 5 * 16 * px
    return rb, cb


def parse_size(s):
    r, c = s.split("x")
    return int(r), int(c)


def timed(f, reps):
    f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); out = f(); ts.append((time.perf_counter() - t0) * 1e3)
    return min(ts), float(np.median(ts)), out


def device_ms(ctx, img, cap, reps):
    import torch
    with torch.cuda.stream(ctx.torch_stream):
        d_img = torch.from_numpy(img).to("cuda")
        d_kp = torch.empty((cap, 28), dtype=torch.uint8, device="cuda"); d_desc = torch.empty((cap, 128), dtype=torch.float32, device="cuda")
        d_n = torch.zeros(1, dtype=torch.int32, device="cuda")
        ts = []
        for it in range(reps + 1):
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            ctx.sift_extract_dev(d_img, d_kp, d_desc, d_n)
            e1.record()
            e1.synchronize()
            if it:
                ts.append(e0.elapsed_time(e1))
        return min(ts), float(np.median(ts)), int(d_n.item())


def run_times(sizes, reps):
    from sfm_opencv_amd import api
    ctx = api.Context(0, use_torch_stream=True)
    print(f"# warm-up, then best / median of {reps}; call ms: host clock around sfmhip_sift_extract (image up, key points and descriptors down); "
          "device ms: sfmhip_sift_extract_dev on a resident image between two stream events")
    print(f"# {'image':>10s} {'key points':>10s} {'call best':>10s} {'call med':>9s} {'device best':>11s} {'device med':>10s}")
    for rows, cols in sizes:
        img = texture(rows, cols)
        n = len(ctx.sift_extract(img)[0])
        cap = n + 1024
        cb, cm, out = timed(lambda: ctx.sift_extract(img, cap=cap), reps)
        db, dm, nd = device_ms(ctx, img, cap, reps)
        assert len(out[0]) == n == nd
        print(f"  {rows:5d}x{cols:<5d} {n:10d} {cb:10.2f} {cm:9.2f} {db:11.3f} {dm:10.3f}", flush=True)
    ctx.close()


def run_trace(size):
    from sfm_opencv_amd import api
    ctx = api.Context(0, use_torch_stream=True)
    img = texture(*size)
    n = len(ctx.sift_extract(img)[0])          # (two extractions where the first offer of 8192 rows was too small)
    for _ in range(4):
        ctx.sift_extract(img, cap=n + 1024)
    print(f"# traced: {size[0]}x{size[1]}, {n} key points")
    ctx.close()


def run_stats(d, size):
    files = [d] if os.path.isfile(d) else sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True))
    assert files, f"no *kernel_stats.csv under {d}"
    rows = list(csv.DictReader(open(files[-1])))
    calls = [int(r["Calls"]) for r in rows if r["Name"].startswith("sift_base_kernel")][0]          # one launch per extraction
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    print(f"# per-kernel device time of {calls} extractions on {size[0]}x{size[1]} (rocprofv3 --kernel-trace --stats), per call; kernels below 0.5 % summed")
    print(f"# {'kernel':44s} {'launches':>8s} {'us / call':>10s} {'share':>7s}")
    small = 0.0
    per = {}
    for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"])):
        ns = float(r["TotalDurationNs"]); name = r["Name"].split("(")[0].replace("void ", "")
        per[name] = ns / calls
        if ns < 0.005 * total:
            small += ns
            continue
        print(f"  {name:44s} {int(r['Calls']) // calls:8d} {ns / calls / 1e3:10.1f} {100 * ns / total:6.1f}%")
    print(f"  {'(the rest)':44s} {'':8s} {small / calls / 1e3:10.1f} {100 * small / total:6.1f}%")
    print(f"  {'total':44s} {'':8s} {total / calls / 1e3:10.1f}")
    rb, cb = blur_bytes(*size)
    for name, b in (("sift_blur_rows_kernel", rb), ("sift_blur_cols_kernel", cb)):
        ns = sum(v for k, v in per.items() if name in k)          # the five instances together
        if ns:
            gbs = b / ns          # bytes per ns = GB/s
            print(f"# {name}<5 .. 13>: {b / 1e6:.1f} MB to move per call, {ns / 1e3:.1f} us -> {gbs:.0f} GB/s = {100 * gbs / HBM_GBS:.0f} % of {HBM_GBS:.0f} GB/s")


def run_host(bin_dir, sizes, threads):
    """for scale only (the CPU of whatever machine this runs on): NViewReconstruct --sift --features-only over t copies of the image on t threads"""
    exe = os.path.join(bin_dir, "NViewReconstruct")
    print("# host extractor, for scale (another machine class): wall time of NViewReconstruct --sift --features-only on t copies of the image with "
          "t OpenMP threads (one image per thread), image reading included")
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
                subprocess.run([exe, d, d, "--sift", "--features-only"], check=True, stdout=subprocess.DEVNULL, env=env)
                wall = time.perf_counter() - t0
            print(f"  {rows:5d}x{cols:<5d} {t:7d} {wall:8.2f} {wall / t:9.2f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="768x1024,2736x3648")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--trace", default="", help="ROWSxCOLS: a few calls of that size, for a kernel trace (with --stats: the size that was traced)")
    ap.add_argument("--stats", default="", help="directory of a rocprofv3 --kernel-trace --stats run of --trace: print its per-kernel table")
    ap.add_argument("--host", default="", help="directory of the built drivers: time the host extractor instead")
    ap.add_argument("--threads", default="1,16")
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
