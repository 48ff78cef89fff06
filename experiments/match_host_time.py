"""Host side of match.hip, for comparing two builds (profiles/README.md, rounds 13 and 15).

  python experiments/match_host_time.py calls   the timed path of bench.py region B on six 700-row sets: three passes of
                                                refresh_descsets + match_pairs_dev, plain and with cross check, on SIFT-like
                                                and on 61-byte Hamming2 sets; then three passes each of triangulate2 (257 points),
                                                triangulate_tracks and reprojection_errors (3 cameras / 40 points) and params() of
                                                a 4-camera / 30-point BA problem with constant points.  Run under
                                                `rocprofv3 --hip-trace --stats --` to count the HIP API calls of a build.
  python experiments/match_host_time.py time    host clock around sfmhip_match_features_l2 / _hamming2 at 5,000 rows
                                                (x 128 floats / x 61 bytes), dense rows and rows embedded in ld = 160 / 80,
                                                best of 5 after warm-up.
"""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sfm_opencv_amd import api, synth  # noqa: E402


def calls():
    import torch
    ctx = api.Context(0, use_torch_stream=True)
    pairs = np.stack([np.arange(5), np.arange(1, 6)], 1).astype(np.int32)
    m = torch.zeros((5, 700, 4), dtype=torch.int32, device="cuda"); c = torch.zeros((5,), dtype=torch.int32, device="cuda")
    for chain, make in ((synth.sift_descriptor_chain(6, 700, seed=3), ctx.descset_l2),
                        (synth.akaze_descriptor_chain(6, 700, seed=3), ctx.descset_hamming2)):
        sets = [make(torch.from_numpy(d).cuda()) for d in chain]
        for cross in (False, True):
            for _ in range(3):
                ctx.refresh_descsets(sets)
                ctx.match_pairs_dev(sets, pairs, m, 700, c, cross_check=cross)
            ctx.synchronize()
        print("calls:", chain[0].dtype, c.cpu().numpy().tolist())
    # the host entry points of triangulate.hip and sfmhip_ba_get_params
    import oracle as orc
    s = synth.two_view_scene(257)
    P1 = orc.projection_matrix(s["K"], s["R1"], s["T1"]); P2 = orc.projection_matrix(s["K"], s["R2"], s["T2"])
    sc = synth.ba_scene(3, 40, seed=7, min_len=2, max_len=3, perturb=False)
    tr = (sc["K_true"], sc["ext_true"], sc["obs_cam"], sc["obs_pt"], sc["obs_uv"])
    sb = synth.ba_scene(4, 30, seed=9)
    pb = ctx.ba_create(sb["K0"], sb["ext0"], sb["pts0"], sb["obs_cam"], sb["obs_pt"], sb["obs_uv"], pt_const=np.arange(30) % 3 == 0)
    pb.iterate(2)
    for _ in range(3):
        xyz = ctx.triangulate2(P1, P2, s["xy1"], s["xy2"])[1]
    for _ in range(3):
        pts, nv = ctx.triangulate_tracks(*tr, sc["n_pt"])
    for _ in range(3):
        err = ctx.reprojection_errors(tr[0], tr[1], sc["pts_true"], *tr[2:])
    for _ in range(3):
        par = pb.params()
    print("calls: geometry", float(xyz.sum()), float(pts.sum()), int(nv.sum()), float(err.sum()), float(par[2].sum()))
    pb.close(); ctx.close()


def timed():
    ctx = api.Context(0)
    for name, fn, chain, ld in (("sfmhip_match_features_l2", ctx.lib.sfmhip_match_features_l2, synth.sift_descriptor_chain(2, 5000, seed=5), 160),
                                ("sfmhip_match_features_hamming2", ctx.lib.sfmhip_match_features_hamming2, synth.akaze_descriptor_chain(2, 5000, seed=5), 80)):
        dim = chain[0].shape[1]
        wide = [np.zeros((5000, ld), chain[0].dtype) for _ in chain]
        for w, d in zip(wide, chain):
            w[:, :dim] = d
        out = np.zeros(5000, api.DMATCH); n = C.c_int()
        for layout, mats, l in (("dense", chain, dim), (f"ld={ld}", wide, ld)):
            ms = []
            for rep in range(8):          # 3 warm-up calls, best of the 5 that follow
                t0 = time.perf_counter()
                rc = fn(ctx.h, mats[0].ctypes.data, 5000, mats[1].ctypes.data, 5000, dim, l, l, out.ctypes.data, C.byref(n))
                ms.append((time.perf_counter() - t0) * 1e3)
                assert rc == 0
            print(f"time: {name} 5000x{dim} {layout}: best of 5 {min(ms[3:]):.3f} ms  (all: {' '.join('%.3f' % x for x in ms)})  matches {n.value}")
    ctx.close()


if __name__ == "__main__":
    {"calls": calls, "time": timed}[sys.argv[1]]()
