"""What constant parameter blocks cost at C4 (sfmhip_ba_create_ex): per LM iteration (host clock over forced iterations, best of
3 x 20, then the library's phase events) and end to end (sfmhip_ba_solve_ex from host arrays, best of 3), for
  unmasked          every block free but camera 0 (the legacy problem, through the legacy entry point)
  window            the last 20 cameras free, points seen by no free camera constant, intrinsics fixed (local BA)
  motion-only       every point constant
  structure-only    every camera constant, intrinsics fixed (n = 0)
usage: python experiments/time_ba_const.py [C4 ...]"""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sfm_opencv_amd import api, synth

names = [a for a in sys.argv[1:] if not a.startswith("--")] or ["C4"]
ctx = api.Context(0, use_torch_stream=True)
for name in names:
    cfg = synth.CONFIGS[name]
    sc = synth.ba_scene_mt(cfg["n_img"], cfg["n_pt"])
    args = (sc["K0"], sc["ext0"], sc["pts0"], sc["obs_cam"], sc["obs_pt"], sc["obs_uv"])
    nc, npt = sc["ext0"].shape[0], sc["pts0"].shape[0]
    win = np.arange(nc) < nc - 20
    seen = np.zeros(npt, bool); seen[sc["obs_pt"][~win[sc["obs_cam"]]]] = True
    cases = [("unmasked", {}, None, None), ("window", dict(fix_intrinsics=1), win, ~seen),
             ("motion-only", {}, None, np.ones(npt, bool)), ("structure-only", dict(fix_intrinsics=1), np.ones(nc, bool), None)]
    for label, kw, cm, pm in cases:
        o = ctx.ba_options(**kw)
        pb = ctx.ba_create(*args, opts=o, cam_const=cm, pt_const=pm)
        pb.iterate(3)
        best = 1e9
        for rep in range(3):
            pb.reset(); pb.iterate(3); ctx.synchronize()
            t = time.perf_counter(); s = pb.iterate(20); ctx.synchronize(); best = min(best, (time.perf_counter() - t) / 20)
        ctx.set_kernel_timing(True)
        pb.reset(); pb.iterate(3); pb.iterate(20); ph = pb.phase_ms()
        ctx.set_kernel_timing(False)
        n = pb.reduced_system(1e4)[0].shape[0]
        pb.close()
        e2e = 1e9
        for rep in range(3):
            t = time.perf_counter(); K, e, p, se = ctx.ba_solve(*args, opts=o, cam_const=cm, pt_const=pm); e2e = min(e2e, time.perf_counter() - t)
        n_free_pts = npt - (0 if pm is None else int(pm.sum()))
        print(f"{name} {label}: n = {n}, free points {n_free_pts}; {best*1e3:.4f} ms/iteration (best of 3 x 20); phases: linearise {ph[0]:.4f} "
              f"solve {ph[1]:.4f} back {ph[2]:.4f} total {ph[3]:.4f}; kernels [4]={ph[4]:.4f} [5]={ph[5]:.4f}; end to end {e2e*1e3:.2f} ms "
              f"({se['iterations']} it, termination {se['termination']}, cost {se['initial_cost']:.6e} -> {se['final_cost']:.6e})", flush=True)
