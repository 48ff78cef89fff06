"""Baseline JPEG decoding on the device (sfmhip_jpeg_decode[_dev], csrc/jpeg.hip): times on 1024x768 (crazyhorse size) and 3648x2736
(the reference's desktop images) files, 4:2:2 and 4:2:0, without restart markers, with one MCU row per interval and with 4 MCUs per
interval; the texture and the clocks of experiments/time_sift.py.  Files are written with Pillow where it is importable (quality 90);
otherwise give a directory of .jpg files with --dir.

  call ms     host clock around the synchronous sfmhip_jpeg_decode: parse, upload, kernels, pixels back to host memory
  dev ms      host clock around sfmhip_jpeg_decode_dev + a synchronise: the same without the download, the image stays resident
  stream ms   the device side of that call between two events on the context's stream (uploads and kernels, not the host's parsing)
  +sift / +akaze ms   host clock around sfmhip_jpeg_decode_dev followed by the extractor on the resident image, to the synchronise
each for entropy = 1 (Huffman stage on the host) and 2 (on the device), after a warm-up, best and median of --reps.

    python experiments/time_jpeg.py [--sizes 768x1024,2736x3648] [--reps 7]
    python experiments/time_jpeg.py --sweep 2736x3648           # host against device entropy stage by interval count: the automatic threshold
    python experiments/time_jpeg.py --host TESTS_HOST_DIR       # tests/host/jpeg_test on the same files (decode + PPM written), for scale
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python experiments/time_jpeg.py --trace DIR/manifest.json
    python experiments/time_jpeg.py --stats DIR                 # per-kernel table of that trace"""
import argparse
import csv
import glob
import io
import json
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

SAMPLING = {"4:2:2": 1, "4:2:0": 2}
RESTART = {"none": {}, "row": dict(restart_marker_rows=1), "4mcu": dict(restart_marker_blocks=4)}
_textures = {}


def encode(size, sampling, restart_opts):
    from PIL import Image
    if size not in _textures:
        _textures[size] = np.ascontiguousarray(texture(*size)[:, :, ::-1])          # RGB for Pillow
    buf = io.BytesIO()
    Image.fromarray(_textures[size]).save(buf, "JPEG", quality=90, subsampling=SAMPLING[sampling], **restart_opts)
    return buf.getvalue()


def files(sizes, folder):
    """[(label, bytes)]"""
    if folder:
        return [(os.path.basename(p), open(p, "rb").read()) for p in sorted(glob.glob(os.path.join(folder, "*.jpg")))]
    return [(f"{r}x{c} {s} {k}", encode((r, c), s, RESTART[k])) for r, c in sizes for s in SAMPLING for k in RESTART]


def dev_times(ctx, data, entropy, reps, then=None):
    """(wall best, wall median, stream best) of jpeg_decode_dev (+ then(image)) to the synchronise"""
    import torch
    with torch.cuda.stream(ctx.torch_stream):
        wall, stream = [], []
        for it in range(reps + 1):
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            ctx.synchronize()
            t0 = time.perf_counter()
            e0.record()
            img, status = ctx.jpeg_decode_dev(data, entropy)
            if then:
                then(img)
            e1.record()
            e1.synchronize()
            t1 = time.perf_counter()
            if it:
                wall.append((t1 - t0) * 1e3); stream.append(e0.elapsed_time(e1))
        assert int(status.item()) == 0
        return min(wall), float(np.median(wall)), min(stream)


def run_times(sizes, reps, folder):
    import torch
    from sfm_opencv_amd import api
    ctx = api.Context(0, use_torch_stream=True)
    cap = 1 << 17
    d_kp = torch.empty((cap, 28), dtype=torch.uint8, device="cuda"); d_n = torch.zeros(1, dtype=torch.int32, device="cuda")
    d_f = torch.empty((cap, 128), dtype=torch.float32, device="cuda"); d_b = torch.empty((cap, 61), dtype=torch.uint8, device="cuda")
    print(f"# warm-up, then best / median of {reps}, ms; e = entropy stage (1 host, 2 device); call: sfmhip_jpeg_decode, pixels back on the host; "
          "dev: sfmhip_jpeg_decode_dev + synchronise (host clock); stream: its device side between two stream events; +sift / +akaze: "
          "decode_dev then the extractor on the resident image (host clock)")
    print(f"# {'file':28s} {'bytes':>8s} {'intervals':>9s} {'e':>1s} {'call best':>9s} {'call med':>8s} {'dev best':>8s} {'dev med':>8s} {'stream':>7s} {'+sift':>7s} {'+akaze':>7s}")
    for label, data in files(sizes, folder):
        info = api.jpeg_info(data)
        ref = ctx.jpeg_decode(data, 1)
        for entropy in (1, 2):
            if entropy == 2 and info[4] == 1 and info[0] * info[1] > (1 << 20):
                print(f"  {label:28s} {len(data):8d} {info[4]:9d} 2  (one interval = one lane: not timed at this size)")
                continue
            assert np.array_equal(ctx.jpeg_decode(data, entropy), ref)          # the same bytes, whoever decodes the entropy stage
            cb, cm, _ = timed(lambda: ctx.jpeg_decode(data, entropy), reps)
            db, dm, sb = dev_times(ctx, data, entropy, reps)
            sift = dev_times(ctx, data, entropy, reps, lambda img: ctx.sift_extract_dev(img, d_kp, d_f, d_n))[0]
            akaze = dev_times(ctx, data, entropy, reps, lambda img: ctx.akaze_extract_dev(img, d_kp, d_b, d_n))[0]
            print(f"  {label:28s} {len(data):8d} {info[4]:9d} {entropy:1d} {cb:9.2f} {cm:8.2f} {db:8.2f} {dm:8.2f} {sb:7.2f} {sift:7.2f} {akaze:7.2f}", flush=True)
    ctx.close()


def run_sweep(size, reps):
    """the entropy stage on the host against the device by interval count, on one image (4:2:0): dev ms of both, alternating"""
    from sfm_opencv_amd import api
    ctx = api.Context(0, use_torch_stream=True)
    mcu_rows = -(-size[0] // 16); mcu_cols = -(-size[1] // 16)
    print(f"# {size[0]}x{size[1]} 4:2:0, {mcu_rows} x {mcu_cols} MCUs; dev ms (host clock, decode_dev + synchronise), best of {reps}, the two stages alternating")
    print(f"# {'MCUs / interval':>15s} {'intervals':>9s} {'host stage':>10s} {'device stage':>12s}")
    for blocks in (mcu_cols * 32, mcu_cols * 16, mcu_cols * 8, mcu_cols * 4, mcu_cols * 2, mcu_cols, mcu_cols // 2, mcu_cols // 4, 16, 4, 1):
        if blocks < 1 or blocks > 65535:
            continue
        data = encode(size, "4:2:0", dict(restart_marker_blocks=blocks))
        n_int = api.jpeg_info(data)[4]
        best = {1: 1e9, 2: 1e9}
        for _ in range(2):
            for e in (1, 2):
                best[e] = min(best[e], dev_times(ctx, data, e, reps)[0])
        print(f"  {blocks:15d} {n_int:9d} {best[1]:10.2f} {best[2]:12.2f}", flush=True)
    ctx.close()


def run_trace(manifest, sizes, reps):
    from sfm_opencv_amd import api
    ctx = api.Context(0, use_torch_stream=True)
    plan = []
    for label, data in files(sizes, ""):
        if not label.endswith("4:2:0 row") and not label.endswith("4:2:0 4mcu") and not label.endswith("4:2:0 none"):
            continue
        n_int = api.jpeg_info(data)[4]
        for entropy in (1, 2):
            if entropy == 2 and n_int == 1:
                continue
            for _ in range(reps):
                ctx.jpeg_decode_dev(data, entropy)
            ctx.synchronize()
            plan.append(dict(file=label, entropy=entropy, intervals=n_int, calls=reps))
    with open(manifest, "w") as f:
        json.dump(plan, f)
    ctx.close()


def run_stats(d):
    plan = json.load(open(os.path.join(d, "manifest.json")))
    tr = sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True))
    assert tr, f"no *kernel_trace.csv under {d}"
    rows = [r for r in csv.DictReader(open(tr[-1])) if "jpeg_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    print("# per-kernel device time of sfmhip_jpeg_decode_dev (rocprofv3 --kernel-trace), us per call: mean over the calls but the first")
    print(f"# {'file':28s} {'intervals':>9s} {'e':>1s} {'huffman':>9s} {'idct':>8s} {'colour':>8s}")
    at = 0
    for p in plan:
        per = {"jpeg_huffman_kernel": [], "jpeg_idct_kernel": [], "jpeg_colour_kernel": []}
        for _ in range(p["calls"]):
            while True:
                r = rows[at]; at += 1
                k = [n for n in per if n in r["Kernel_Name"]][0]
                per[k].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
                if k == "jpeg_colour_kernel":
                    break
        m = {k: (float(np.mean(v[1:])) if len(v) > 1 else float("nan")) for k, v in per.items()}
        assert (len(per["jpeg_huffman_kernel"]) > 0) == (p["entropy"] == 2)
        print(f"  {p['file']:28s} {p['intervals']:9d} {p['entropy']:1d} {m['jpeg_huffman_kernel']:9.1f} {m['jpeg_idct_kernel']:8.1f} {m['jpeg_colour_kernel']:8.1f}")
    assert at == len(rows)


def run_host(bin_dir, sizes, folder):
    """for scale only (the CPU of whatever machine this runs on)"""
    exe = os.path.join(bin_dir, "jpeg_test")
    print("# host decoder, for scale: wall time of tests/host/jpeg_test (sfm_jpeg.hpp through imread, one thread; the PPM is written too), best of 3")
    print(f"# {'file':28s} {'bytes':>8s} {'wall s':>8s}")
    with tempfile.TemporaryDirectory() as d:
        for label, data in files(sizes, folder):
            src = os.path.join(d, "in.jpg")
            open(src, "wb").write(data)
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                subprocess.run([exe, src, os.path.join(d, "out.pnm")], check=True)
                ts.append(time.perf_counter() - t0)
            print(f"  {label:28s} {len(data):8d} {min(ts):8.3f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="768x1024,2736x3648")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--dir", default="", help="a directory of .jpg files to time instead of generated ones")
    ap.add_argument("--sweep", default="", help="ROWSxCOLS: host against device entropy stage by interval count")
    ap.add_argument("--trace", default="", help="manifest file to write: a few calls per file and entropy stage, for a kernel trace")
    ap.add_argument("--stats", default="", help="directory of a rocprofv3 --kernel-trace run of --trace (holds manifest.json): print its per-kernel table")
    ap.add_argument("--host", default="", help="directory of the built tests/host/jpeg_test: time the host decoder instead")
    a = ap.parse_args()
    sizes = [parse_size(s) for s in a.sizes.split(",")]
    if a.stats:
        run_stats(a.stats)
    elif a.trace:
        run_trace(a.trace, sizes, min(a.reps, 5))
    elif a.sweep:
        run_sweep(parse_size(a.sweep), a.reps)
    elif a.host:
        run_host(a.host, sizes, a.dir)
    else:
        run_times(sizes, a.reps, a.dir)


if __name__ == "__main__":
    main()
