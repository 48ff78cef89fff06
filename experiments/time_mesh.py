"""The mesh clean-up (sfmhip_mesh_components, _filter_components, _simplify, _vertex_normals, _smooth): --runs timed runs after a warm-up,
median and min .. max.  The input is the mesh of experiments/time_tsdf.py: 8 views of the unit sphere fused into 128^3 and 256^3 voxels
(89,826 / 370,518 triangles), with its colours.

  default     every call, and the chain filter(min 10) -> simplify(2 voxels) -> smooth(10, 0.5, -0.53) -> normals, resident (between two
              events on the context's stream; the chain reads its counts back between the steps, as api.dense_mesh_for_all does, so it is
              timed on the host's clock) and from host arrays (the host forms, host clock, copies included).  Beside each resident
              call: the bytes it must move -- its inputs once, its outputs once; a smoothing step 48 bytes per vertex -- per second,
              against --copy-rate.  For scale: the numpy restatement's time on the same input.
  --trace DIR / --stats DIR   the kernels of each call, from a kernel trace of its own:
                  rocprofv3 --kernel-trace --output-format csv -d DIR -- python experiments/time_mesh.py --trace DIR
                  python experiments/time_mesh.py --stats DIR
              per call: the time in the radix sort's and the scan's kernels (sortscan.hip) and in each kernel of mesh.hip / points.hip.

    python experiments/time_mesh.py [--runs 5] [--sizes 128,256]
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
sys.path.insert(0, os.path.join(ROOT, "experiments"))

import mesh_ref as mr                                       # noqa: E402
import time_tsdf as tt                                      # noqa: E402
import tsdf_ref as tr                                       # noqa: E402

MIN_COMPONENT, CELLS, SMOOTH = 10, 2.0, (10, 0.5, -0.53)
CALLS = ("components", "filter", "simplify", "normals", "smooth")


def spread(v):
    return f"{statistics.median(v):8.3f} ({min(v):.3f} .. {max(v):.3f})"


def raw_mesh(ctx, torch, n, inputs):
    """the resident mesh of time_tsdf.py's scene at n^3 voxels: (d_xyz, d_bgr, d_tri, nv, nt, voxel)"""
    d_depth, d_keep, d_img, R, t = inputs
    dims, origin, voxel = tr.sphere_box(n)
    nvox = n ** 3
    d_d = torch.zeros(nvox, dtype=torch.int32, device="cuda"); d_w = torch.zeros(nvox, dtype=torch.int32, device="cuda")
    d_c = torch.zeros((nvox, 3), dtype=torch.int32, device="cuda"); d_n = torch.zeros(2, dtype=torch.int32, device="cuda")
    ctx.tsdf_integrate_dev(dims, origin, voxel, tt.TRUNC_VOXELS * voxel, d_depth, d_keep, d_img, tt.ROWS, tt.COLS, 3, 3 * tt.COLS, tt.K4, R, t, d_d, d_w, d_c)
    ctx.tsdf_mesh_dev(dims, origin, voxel, d_d, d_w, d_c, tt.MIN_WEIGHT, None, None, 0, None, 0, d_n[0:1], d_n[1:2])
    ctx.synchronize()
    nv, nt = (int(x) for x in d_n.cpu().numpy())
    d_xyz = torch.empty((nv, 3), dtype=torch.float64, device="cuda"); d_bgr = torch.empty((nv, 3), dtype=torch.uint8, device="cuda")
    d_tri = torch.empty((nt, 3), dtype=torch.int32, device="cuda")
    ctx.tsdf_mesh_dev(dims, origin, voxel, d_d, d_w, d_c, tt.MIN_WEIGHT, d_xyz, d_bgr, nv, d_tri, nt, d_n[0:1], d_n[1:2])
    ctx.synchronize()
    return d_xyz, d_bgr, d_tri, nv, nt, voxel


def resident_calls(ctx, torch, d_xyz, d_bgr, d_tri, nv, nt, voxel):
    """name -> a function that enqueues the call on the resident mesh; the outputs are allocated once"""
    o_xyz = torch.empty((nv, 3), dtype=torch.float64, device="cuda"); o_bgr = torch.empty((nv, 3), dtype=torch.uint8, device="cuda")
    o_tri = torch.empty((nt, 3), dtype=torch.int32, device="cuda"); o_map = torch.empty(nv, dtype=torch.int32, device="cuda")
    tl = torch.empty(nt, dtype=torch.int32, device="cuda"); vl = torch.empty(nv, dtype=torch.int32, device="cuda"); sz = torch.empty(nt, dtype=torch.int32, device="cuda")
    n = torch.zeros(2, dtype=torch.int32, device="cuda")
    return {
        "components": lambda: ctx.mesh_components_dev(nv, d_tri, nt, tl, vl, n[0:1], sz),
        "filter": lambda: ctx.mesh_filter_components_dev(d_xyz, d_bgr, nv, d_tri, nt, MIN_COMPONENT, False, o_xyz, o_bgr, o_tri, o_map, n[0:1], n[1:2]),
        "simplify": lambda: ctx.mesh_simplify_dev(d_xyz, d_bgr, nv, d_tri, nt, CELLS * voxel, o_xyz, o_bgr, o_tri, o_map, n[0:1], n[1:2]),
        "normals": lambda: ctx.mesh_vertex_normals_dev(d_xyz, nv, d_tri, nt, o_xyz),
        "smooth": lambda: ctx.mesh_smooth_dev(d_xyz, nv, d_tri, nt, *SMOOTH, o_xyz),
    }, (o_xyz, o_bgr, o_tri, n)


def chain_resident(ctx, torch, d_xyz, d_bgr, d_tri, nv, nt, voxel, bufs):
    """filter -> simplify -> smooth -> normals on the resident mesh, the counts read back between the steps: (nv, nt) at the end"""
    (a_xyz, a_bgr, a_tri, n), (b_xyz, b_bgr, b_tri, _) = bufs
    ctx.mesh_filter_components_dev(d_xyz, d_bgr, nv, d_tri, nt, MIN_COMPONENT, False, a_xyz, a_bgr, a_tri, None, n[0:1], n[1:2])
    ctx.synchronize()
    nv, nt = (int(x) for x in n.cpu().numpy())
    ctx.mesh_simplify_dev(a_xyz, a_bgr, nv, a_tri, nt, CELLS * voxel, b_xyz, b_bgr, b_tri, None, n[0:1], n[1:2])
    ctx.synchronize()
    nv, nt = (int(x) for x in n.cpu().numpy())
    ctx.mesh_smooth_dev(b_xyz, nv, b_tri, nt, *SMOOTH, a_xyz)
    ctx.mesh_vertex_normals_dev(a_xyz, nv, b_tri, nt, b_xyz)
    ctx.synchronize()
    return nv, nt


def setup(a):
    import torch
    from sfm_opencv_amd import api
    ctx = api.Context(0, use_torch_stream=True)
    depths, keeps, imgs, R, t = tt.scene()
    return torch, ctx, (depths, keeps, imgs, R, t)


def run_events(a):
    torch, ctx, (depths, keeps, imgs, R, t) = setup(a)
    print(f"# median (min .. max) of {a.runs} runs after a warm-up, ms; the mesh of time_tsdf.py's scene; filter: min {MIN_COMPONENT} triangles; simplify: {CELLS} voxels; "
          f"smooth: {SMOOTH}")
    with torch.cuda.stream(ctx.torch_stream):
        inputs = ([torch.from_numpy(x).to("cuda") for x in depths], [torch.from_numpy(x).to("cuda") for x in keeps], [torch.from_numpy(x).to("cuda") for x in imgs], R, t)

        def events(f):
            out = []
            for it in range(a.runs + 1):
                e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
                e0.record(); f(); e1.record(); e1.synchronize()
                if it:
                    out.append(e0.elapsed_time(e1))
            return out

        def clock(f):
            out = []
            for it in range(a.runs + 1):
                ctx.synchronize()
                t0 = time.perf_counter(); f(); ctx.synchronize(); dt = (time.perf_counter() - t0) * 1e3
                if it:
                    out.append(dt)
            return out
        for size in (int(x) for x in a.sizes.split(",")):
            d_xyz, d_bgr, d_tri, nv, nt, voxel = raw_mesh(ctx, torch, size, inputs)
            xyz, bgr, tri = d_xyz.cpu().numpy(), d_bgr.cpu().numpy(), d_tri.cpu().numpy()
            calls, bufs_a = resident_calls(ctx, torch, d_xyz, d_bgr, d_tri, nv, nt, voxel)
            _, bufs_b = resident_calls(ctx, torch, d_xyz, d_bgr, d_tri, nv, nt, voxel)
            host = {
                "components": lambda: ctx.mesh_components(nv, tri),
                "filter": lambda: ctx.mesh_filter_components(xyz, bgr, tri, MIN_COMPONENT, False),
                "simplify": lambda: ctx.mesh_simplify(xyz, bgr, tri, CELLS * voxel),
                "normals": lambda: ctx.mesh_vertex_normals(xyz, tri),
                "smooth": lambda: ctx.mesh_smooth(xyz, tri, *SMOOTH),
            }
            fx, fb, ft, _ = host["filter"]()
            sx, sb, st, _ = host["simplify"]()
            steps = SMOOTH[0] * (1 if SMOOTH[2] == 0 else 2)
            moved = {"components": 12 * nt + 4 * nt + 4 * nv + 4 * nt, "filter": 27 * nv + 12 * nt + 27 * len(fx) + 12 * len(ft) + 4 * nv,
                     "simplify": 27 * nv + 12 * nt + 27 * len(sx) + 12 * len(st) + 4 * nv, "normals": 24 * nv + 12 * nt + 24 * nv, "smooth": 12 * nt + steps * 48 * nv}
            print(f"  {size}^3: {nv} vertices, {nt} triangles; after the filter {len(fx)} / {len(ft)}, after the simplification {len(sx)} / {len(st)}")
            for name in CALLS:
                v = events(calls[name]); med = statistics.median(v)
                print(f"    {name:<11s} resident  {spread(v)}   {moved[name] / 1e6:7.1f} MB to move = {moved[name] / med / 1e9:.4f} TB/s = {moved[name] / med / 1e9 / a.copy_rate:.4f} of "
                      f"{a.copy_rate} TB/s")
                print(f"    {name:<11s} host form {spread(clock(host[name]))}", flush=True)
            end = chain_resident(ctx, torch, d_xyz, d_bgr, d_tri, nv, nt, voxel, (bufs_a, bufs_b))
            print(f"    chain       resident  {spread(clock(lambda: chain_resident(ctx, torch, d_xyz, d_bgr, d_tri, nv, nt, voxel, (bufs_a, bufs_b))))}   (host clock: two read-backs of "
                  f"the counts inside) -> {end[0]} vertices, {end[1]} triangles")

            def chain_host():
                x, b, t3, _ = ctx.mesh_filter_components(xyz, bgr, tri, MIN_COMPONENT, False)
                x, b, t3, _ = ctx.mesh_simplify(x, b, t3, CELLS * voxel)
                x = ctx.mesh_smooth(x, t3, *SMOOTH)
                return x, b, t3, ctx.mesh_vertex_normals(x, t3)
            print(f"    chain       host form {spread(clock(chain_host))}", flush=True)
            if size <= a.numpy_up_to:
                ref = {"components": lambda: mr.components(nv, tri), "filter": lambda: mr.filter_components(xyz, bgr, tri, MIN_COMPONENT, False),
                       "simplify": lambda: mr.simplify(xyz, bgr, tri, CELLS * voxel), "normals": lambda: (mr.vertex_normals(xyz, tri),),
                       "smooth": lambda: (mr.smooth(xyz, tri, *SMOOTH),)}
                line = []
                for name in CALLS:
                    t0 = time.perf_counter(); exp = ref[name](); dt = (time.perf_counter() - t0) * 1e3
                    got = host[name]()
                    got = got if isinstance(got, tuple) else (got,)
                    same = all((g is None and e is None) or (g.shape == e.shape and g.tobytes() == e.tobytes()) for g, e in zip(got, exp))
                    line.append(f"{name} {dt:.0f} ms (the same bytes: {same})")
                print("    numpy restatement, for scale: " + ", ".join(line), flush=True)
    ctx.close()


def run_trace(a):
    torch, ctx, (depths, keeps, imgs, R, t) = setup(a)
    plan = []
    os.makedirs(a.trace, exist_ok=True)
    with torch.cuda.stream(ctx.torch_stream):
        inputs = ([torch.from_numpy(x).to("cuda") for x in depths], [torch.from_numpy(x).to("cuda") for x in keeps], [torch.from_numpy(x).to("cuda") for x in imgs], R, t)
        one = torch.zeros((1, 3), dtype=torch.float64, device="cuda"); one_out = torch.zeros((1, 3), dtype=torch.float64, device="cuda")
        for size in (int(x) for x in a.sizes.split(",")):
            d_xyz, d_bgr, d_tri, nv, nt, voxel = raw_mesh(ctx, torch, size, inputs)
            calls, _ = resident_calls(ctx, torch, d_xyz, d_bgr, d_tri, nv, nt, voxel)
            for name in CALLS:
                ctx.mesh_vertex_normals_dev(one, 1, None, 0, one_out)       # the mark between two phases: a normals call without a sort
                for _ in range(a.runs + 1):
                    calls[name]()
                ctx.synchronize()
            plan.append(dict(size=size, nv=nv, nt=nt, calls=a.runs + 1))
    with open(os.path.join(a.trace, "manifest.json"), "w") as f:
        json.dump(plan, f)
    ctx.close()


def run_stats(a):
    plan = json.load(open(os.path.join(a.stats, "manifest.json")))
    files = sorted(glob.glob(os.path.join(a.stats, "**", "*kernel_trace.csv"), recursive=True))
    assert files, f"no *kernel_trace.csv under {a.stats}"
    rows = [r for r in csv.DictReader(open(files[-1])) if any(s in r["Kernel_Name"] for s in ("mesh_", "setup_rs", "setup_scan", "voxel_"))]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    names = [r["Kernel_Name"].split("(")[0].split(" ")[-1] for r in rows]
    marks = [i for i in range(len(rows) - 1) if names[i] == "mesh_tri_normal_kernel" and names[i + 1] == "mesh_run_start_kernel"]
    assert len(marks) == len(plan) * len(CALLS), (len(marks), len(plan))
    print("# kernel times from a rocprofv3 --kernel-trace run: ms per call (the first call of each phase left out), summed per kernel")
    for pi, p in enumerate(plan):
        print(f"  {p['size']}^3: {p['nv']} vertices, {p['nt']} triangles")
        for ci, name in enumerate(CALLS):
            m = marks[pi * len(CALLS) + ci]
            nxt = marks[pi * len(CALLS) + ci + 1] if pi * len(CALLS) + ci + 1 < len(marks) else len(rows)
            seg = list(range(m + 3, nxt))                                   # past the mark's three kernels
            if nxt < len(rows) and ci == len(CALLS) - 1:                    # the next size's tsdf mesh runs scans before its first mark
                last = max(i for i in seg if names[i] == "mesh_smooth_step_kernel")
                seg = [i for i in seg if i <= last]
            per = len(seg) // p["calls"]
            assert per * p["calls"] == len(seg), (name, len(seg), p["calls"])
            tot = {}
            for i in seg[per:]:
                key = "radix sort (sfm_sort_*)" if "sfm_sort_" in names[i] else "scans (sfm_scan_*)" if "sfm_scan_" in names[i] else names[i]
                tot[key] = tot.get(key, 0.0) + (int(rows[i]["End_Timestamp"]) - int(rows[i]["Start_Timestamp"])) / 1e6 / (p["calls"] - 1)
            total = sum(tot.values())
            print(f"    {name}: {per} launches, {total:.3f} ms in kernels")
            for k, v in sorted(tot.items(), key=lambda kv: -kv[1]):
                print(f"        {k:<28s} {v:7.3f}  {v / total:5.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--sizes", default="128,256")
    ap.add_argument("--numpy-up-to", type=int, default=256, help="largest volume side at which the numpy restatement is timed too")
    ap.add_argument("--trace", default="", help="directory for manifest.json: the calls of a kernel trace")
    ap.add_argument("--stats", default="", help="directory of a rocprofv3 --kernel-trace run of --trace: print its per-kernel table")
    ap.add_argument("--copy-rate", type=float, default=6.29, help="achievable copy rate of the device in TB/s")
    a = ap.parse_args()
    if a.stats:
        run_stats(a)
    elif a.trace:
        run_trace(a)
    else:
        run_events(a)


if __name__ == "__main__":
    main()
