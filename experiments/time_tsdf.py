"""The dense mesh (sfmhip_tsdf_integrate, sfmhip_tsdf_mesh): --runs timed runs after a warm-up, median and min .. max.  8 pinhole views of
1024 x 768 (f = 900) of the unit sphere from the camera positions of tests/tsdf_ref.py, analytic float32 depth maps, random BGR images,
keep maps that drop every eighth pixel, into a resident volume of 128^3 and of 256^3 voxels over [-1.5, 1.5]^3, truncation at 4 voxels, min_weight 2.

  default     integrate (all 8 views, one call) and mesh (counts known, caps exact), each between two events on the context's stream on
              resident arrays, and with the copies (the host forms, host clock around the call).  Beside integrate: the bytes of the volume
              it must move (20 bytes read and 20 written per voxel that a view counts in; the whole volume for comparison) per second
              against --copy-rate, and the fp64 issue bound (--f64-per-view fp64 VALU instructions per voxel and view in the ISA, 4 cycles
              each on 1,024 SIMDs at 2.4 GHz).  Beside mesh: ms per million cells and per million triangles.  For scale, at 128^3 only:
              the numpy restatement's time on the same input.
  --trace DIR / --stats DIR   the kernels one by one, from a kernel trace of its own:
                  rocprofv3 --kernel-trace --output-format csv -d DIR -- python experiments/time_tsdf.py --trace DIR
                  python experiments/time_tsdf.py --stats DIR
              integrate in three forms -- 8 views with colour and keep maps, 8 views with neither (8 bytes per voxel, one gather per view),
              1 view with both -- so that the gathers and the per-view arithmetic can be told apart; then the mesh's kernels and scans.

    python experiments/time_tsdf.py [--runs 5] [--sizes 128,256]
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import tsdf_ref as tr                                       # noqa: E402

ROWS, COLS, N_VIEWS = 768, 1024, 8
K4 = (900.0, 900.0, 511.5, 383.5)
TRUNC_VOXELS, MIN_WEIGHT = 4, 2
PICK = [0, 1, 2, 3, 6, 9, 10, 13]                           # four views on the axes, four on the diagonals


def scene():
    poses = [tr.look_at(tr.SPHERE_CAMS[i]) for i in PICK]
    depths = [tr.sphere_depth(R, t, K4, ROWS, COLS) for R, t in poses]
    rng = np.random.default_rng(1)
    imgs = [rng.integers(0, 256, (ROWS, COLS, 3), dtype=np.uint8) for _ in poses]
    diag = np.indices((ROWS, COLS)).sum(0)
    keeps = [((diag + i) % 8 != 0).astype(np.uint8) for i in range(len(poses))]         # every eighth pixel dropped, another eighth per view
    return depths, keeps, imgs, np.array([R.ravel() for R, _ in poses]), np.array([t for _, t in poses])


def spread(v):
    return f"{statistics.median(v):8.3f} ({min(v):.3f} .. {max(v):.3f})"


def run_events(a):
    import torch
    from sfm_opencv_amd import api
    ctx = api.Context(0, use_torch_stream=True)
    depths, keeps, imgs, R, t = scene()
    print(f"# median (min .. max) of {a.runs} runs after a warm-up, ms; {N_VIEWS} views of {COLS} x {ROWS}, BGR, keep maps; trunc {TRUNC_VOXELS} voxels, min_weight {MIN_WEIGHT}")
    with torch.cuda.stream(ctx.torch_stream):
        d_depth = [torch.from_numpy(x).to("cuda") for x in depths]; d_keep = [torch.from_numpy(x).to("cuda") for x in keeps]
        d_img = [torch.from_numpy(x).to("cuda") for x in imgs]

        def events(f, before=None):
            out = []
            for it in range(a.runs + 1):
                if before:
                    before()
                e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
                e0.record(); f(); e1.record(); e1.synchronize()
                if it:
                    out.append(e0.elapsed_time(e1))
            return out

        def clock(f):
            out = []
            for it in range(a.runs + 1):
                ctx.synchronize()
                t0 = time.perf_counter(); f(); dt = (time.perf_counter() - t0) * 1e3
                if it:
                    out.append(dt)
            return out
        for n in (int(x) for x in a.sizes.split(",")):
            dims, origin, voxel = tr.sphere_box(n)
            nvox, cells = n ** 3, (n - 1) ** 3
            d_d = torch.zeros(nvox, dtype=torch.int32, device="cuda"); d_w = torch.zeros(nvox, dtype=torch.int32, device="cuda")
            d_c = torch.zeros((nvox, 3), dtype=torch.int32, device="cuda"); d_n = torch.zeros(2, dtype=torch.int32, device="cuda")

            def zero():
                d_d.zero_(); d_w.zero_(); d_c.zero_()

            def integrate():
                ctx.tsdf_integrate_dev(dims, origin, voxel, TRUNC_VOXELS * voxel, d_depth, d_keep, d_img, ROWS, COLS, 3, 3 * COLS, K4, R, t, d_d, d_w, d_c)
            t_int = events(integrate, zero)
            touched = int((d_w > 0).sum())
            ctx.tsdf_mesh_dev(dims, origin, voxel, d_d, d_w, d_c, MIN_WEIGHT, None, None, 0, None, 0, d_n[0:1], d_n[1:2])
            ctx.synchronize()
            nv, nt = (int(x) for x in d_n.cpu().numpy())
            d_xyz = torch.empty((nv, 3), dtype=torch.float64, device="cuda"); d_bgr = torch.empty((nv, 3), dtype=torch.uint8, device="cuda")
            d_tri = torch.empty((nt, 3), dtype=torch.int32, device="cuda")
            t_mesh = events(lambda: ctx.tsdf_mesh_dev(dims, origin, voxel, d_d, d_w, d_c, MIN_WEIGHT, d_xyz, d_bgr, nv, d_tri, nt, d_n[0:1], d_n[1:2]))
            # the host forms: the maps, images and the volume go up, the volume or the mesh comes back
            vol = tr.new_volume(dims)
            t_int_h = clock(lambda: ctx.tsdf_integrate(dims, origin, voxel, TRUNC_VOXELS * voxel, depths, keeps, imgs, K4, R, t, *vol))
            h_d, h_w, h_c = d_d.cpu().numpy(), d_w.cpu().numpy(), d_c.cpu().numpy().view(np.uint32)
            t_mesh_h = clock(lambda: ctx.tsdf_mesh(dims, origin, voxel, h_d, h_w, h_c, MIN_WEIGHT, vertex_cap=nv, triangle_cap=nt))
            med = statistics.median(t_int)
            moved, whole = touched * 40, nvox * 40
            f64_ms = nvox / 64 * N_VIEWS * a.f64_per_view * 4 / 1024 / 2.4e6
            mm = statistics.median(t_mesh)
            print(f"  {n}^3: {touched} of {nvox} voxels counted in, {nv} vertices, {nt} triangles")
            print(f"    integrate, resident   {spread(t_int)}   {moved / 1e6:.1f} MB moved = {moved / med / 1e9:.3f} TB/s = {moved / med / 1e9 / a.copy_rate:.3f} of {a.copy_rate} TB/s"
                  f" (whole volume: {whole / 1e6:.1f} MB, {whole / med / 1e9:.3f} TB/s); fp64 issue bound {f64_ms:.3f} ms = {f64_ms / med:.2f} of the time")
            print(f"    integrate, host form  {spread(t_int_h)}")
            print(f"    mesh, resident        {spread(t_mesh)}   {mm / (cells / 1e6):.4f} ms per million cells, {mm / (nt / 1e6):.3f} ms per million triangles")
            print(f"    mesh, host form       {spread(t_mesh_h)}", flush=True)
            if n <= a.numpy_up_to:
                ref = tr.new_volume(dims)
                t0 = time.perf_counter(); tr.integrate(dims, origin, voxel, TRUNC_VOXELS * voxel, depths, keeps, imgs, K4, R, t, *ref); t1 = time.perf_counter()
                x, b, tri = tr.mesh(dims, origin, voxel, *ref, MIN_WEIGHT); t2 = time.perf_counter()
                same = np.array_equal(ref[0], h_d) and np.array_equal(ref[1], h_w) and np.array_equal(ref[2], h_c) and len(x) == nv and len(tri) == nt
                print(f"    numpy restatement, for scale: integrate {(t1 - t0) * 1e3:.0f} ms, mesh {(t2 - t1) * 1e3:.0f} ms; the same volume and counts: {same}", flush=True)
            del d_d, d_w, d_c, d_xyz, d_bgr, d_tri
    ctx.close()


def run_trace(a):
    import torch
    from sfm_opencv_amd import api
    ctx = api.Context(0, use_torch_stream=True)
    depths, keeps, imgs, R, t = scene()
    plan = []
    with torch.cuda.stream(ctx.torch_stream):
        d_depth = [torch.from_numpy(x).to("cuda") for x in depths]; d_keep = [torch.from_numpy(x).to("cuda") for x in keeps]
        d_img = [torch.from_numpy(x).to("cuda") for x in imgs]
        for n in (int(x) for x in a.sizes.split(",")):
            dims, origin, voxel = tr.sphere_box(n)
            nvox = n ** 3
            d_d = torch.zeros(nvox, dtype=torch.int32, device="cuda"); d_w = torch.zeros(nvox, dtype=torch.int32, device="cuda")
            d_c = torch.zeros((nvox, 3), dtype=torch.int32, device="cuda"); d_n = torch.zeros(2, dtype=torch.int32, device="cuda")
            calls = a.runs + 1
            for form in ("8 views, colour and keep", "8 views, depth only", "1 view, colour and keep"):
                for _ in range(calls):
                    if form.startswith("8 views, depth"):
                        ctx.tsdf_integrate_dev(dims, origin, voxel, TRUNC_VOXELS * voxel, d_depth, None, None, ROWS, COLS, 3, 3 * COLS, K4, R, t, d_d, d_w, None)
                    else:
                        k = 8 if form.startswith("8") else 1
                        ctx.tsdf_integrate_dev(dims, origin, voxel, TRUNC_VOXELS * voxel, d_depth[:k], d_keep[:k], d_img[:k], ROWS, COLS, 3, 3 * COLS, K4, R[:k], t[:k],
                                               d_d, d_w, d_c)
                ctx.synchronize()
            d_d.zero_(); d_w.zero_(); d_c.zero_()
            ctx.tsdf_integrate_dev(dims, origin, voxel, TRUNC_VOXELS * voxel, d_depth, d_keep, d_img, ROWS, COLS, 3, 3 * COLS, K4, R, t, d_d, d_w, d_c)
            ctx.tsdf_mesh_dev(dims, origin, voxel, d_d, d_w, d_c, MIN_WEIGHT, None, None, 0, None, 0, d_n[0:1], d_n[1:2])
            ctx.synchronize()
            nv, nt = (int(x) for x in d_n.cpu().numpy())
            d_xyz = torch.empty((nv, 3), dtype=torch.float64, device="cuda"); d_bgr = torch.empty((nv, 3), dtype=torch.uint8, device="cuda")
            d_tri = torch.empty((nt, 3), dtype=torch.int32, device="cuda")
            for _ in range(calls):
                ctx.tsdf_mesh_dev(dims, origin, voxel, d_d, d_w, d_c, MIN_WEIGHT, d_xyz, d_bgr, nv, d_tri, nt, d_n[0:1], d_n[1:2])
            ctx.synchronize()
            plan.append(dict(n=n, calls=calls, nt=nt, nv=nv, touched=int((d_w > 0).sum())))
            del d_d, d_w, d_c, d_xyz, d_bgr, d_tri
    with open(os.path.join(a.trace, "manifest.json"), "w") as f:
        json.dump(plan, f)
    ctx.close()


def run_stats(a):
    plan = json.load(open(os.path.join(a.stats, "manifest.json")))
    tr_files = sorted(glob.glob(os.path.join(a.stats, "**", "*kernel_trace.csv"), recursive=True))
    assert tr_files, f"no *kernel_trace.csv under {a.stats}"
    rows = [r for r in csv.DictReader(open(tr_files[-1])) if "tsdf_" in r["Kernel_Name"] or "setup_scan" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))

    def ms(r):
        return (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
    print("# kernel times from a rocprofv3 --kernel-trace run, ms, median (min .. max) of the calls but the first")
    at = 0
    for p in plan:
        n, calls = p["n"], p["calls"]
        print(f"  {n}^3")
        med = {}
        for form in ("8 views, colour and keep", "8 views, depth only", "1 view, colour and keep"):
            seq = rows[at:at + calls]; at += calls
            assert all("tsdf_integrate_kernel" in r["Kernel_Name"] for r in seq), [r["Kernel_Name"][:30] for r in seq]
            v = [ms(r) for r in seq[1:]]
            med[form] = statistics.median(v)
            print(f"    tsdf_integrate_kernel, {form:<26s} {spread(v)}")
        per_view = (med["8 views, colour and keep"] - med["1 view, colour and keep"]) / 7
        f64 = n ** 3 / 64 * a.f64_per_view * 4 / 1024 / 2.4e6
        print(f"      a further view costs {per_view:.4f} ms; its fp64 issue bound ({a.f64_per_view} instructions) is {f64:.4f} ms; the colour and keep gathers and csum cost "
              f"{med['8 views, colour and keep'] - med['8 views, depth only']:.4f} ms of the 8-view call")
        assert "tsdf_integrate_kernel" in rows[at]["Kernel_Name"]           # the one that fills the volume the mesh calls take
        at += 1
        # a mesh call runs from its tsdf_cell_kernel to its tsdf_triangle_kernel: the counting call, the warm-up, then the timed ones
        agg = {}
        for call in range(calls + 1):
            end = next(i for i in range(at, len(rows)) if "tsdf_triangle_kernel" in rows[i]["Kernel_Name"]) + 1
            seq = rows[at:end]; at = end
            assert "tsdf_cell_kernel" in seq[0]["Kernel_Name"] and sum("tsdf_" in r["Kernel_Name"] for r in seq) == 4, [r["Kernel_Name"][:24] for r in seq]
            if call >= 2:
                tot = {}
                for r in seq:
                    key = "the scans' kernels" if "setup_scan" in r["Kernel_Name"] else r["Kernel_Name"].split("(")[0].split(" ")[-1]
                    tot[key] = tot.get(key, 0.0) + ms(r)
                tot["the call's kernels"] = sum(tot.values())
                for k, v in tot.items():
                    agg.setdefault(k, []).append(v)
        for k, v in agg.items():
            print(f"    mesh: {k:<24s} {spread(v)}")
    assert at == len(rows), (at, len(rows))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--sizes", default="128,256")
    ap.add_argument("--numpy-up-to", type=int, default=128, help="largest volume side at which the numpy restatement is timed too")
    ap.add_argument("--trace", default="", help="directory for manifest.json: the calls of a kernel trace")
    ap.add_argument("--stats", default="", help="directory of a rocprofv3 --kernel-trace run of --trace: print its per-kernel table")
    ap.add_argument("--copy-rate", type=float, default=6.29, help="achievable copy rate of the device in TB/s")
    ap.add_argument("--f64-per-view", type=int, default=84, help="fp64 VALU instructions per voxel and counted view in tsdf_integrate_kernel's ISA")
    a = ap.parse_args()
    if a.stats:
        run_stats(a)
    elif a.trace:
        run_trace(a)
    else:
        run_events(a)


if __name__ == "__main__":
    main()
