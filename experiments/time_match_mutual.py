"""Cross check (SFMHIP_MATCH_MUTUAL) on the C4 chain (200 images x 5000 rows, 199 consecutive pairs), descriptors resident, for
SIFT / L2 and AKAZE / Hamming2: device time per call of, in the same process,
  plain     match_pairs_dev (kNN-2 + ratio tail)
  mutual    match_pairs_dev(cross_check=True) (the int8 path finds the reverse best inside its kNN kernel; the Hamming2 paths run a
            second kNN-2 with the operands swapped)
  two-pass  match_pairs_dev + one knn2_dev per pair in the reverse direction (the existing entry points; the caller's filter on
            the host is not counted)
plus the kNN kernel time per call of the plain and the mutual form (sfmhip_match_kernel_ms averages over launch sequences; a call that
runs two -- the swapped second pass of the exact fp32 / VALU Hamming2 paths -- counts both).
python3 experiments/time_match_mutual.py [n_img] [n_desc] [reps]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from sfm_opencv_amd import api, synth

n_img = int(sys.argv[1]) if len(sys.argv) > 1 else 200
n_desc = int(sys.argv[2]) if len(sys.argv) > 2 else 5000
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
ctx = api.Context(0, use_torch_stream=True)
pairs = np.stack([np.arange(n_img - 1), np.arange(1, n_img)], 1).astype(np.int32)


def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts))


def kernel_ms(fn):
    fn(); torch.cuda.synchronize()
    ctx.match_kernel_ms()
    ctx.set_kernel_timing(True)
    for _ in range(4):
        fn()
    torch.cuda.synchronize()
    k, m, seqs, _ = ctx.match_kernel_ms()
    ctx.set_kernel_timing(False)
    per_call = seqs / 4.0                       # launch sequences per call
    return k * per_call, m * per_call


for norm in ("L2", "Hamming2"):
    if norm == "L2":
        sets = [ctx.descset_l2(t) for t in synth.sift_descriptor_chain_device(n_img, n_desc)]
    else:
        sets = [ctx.descset_hamming2(t) for t in synth.akaze_descriptor_chain_device(n_img, n_desc)]
    torch.cuda.synchronize()
    d_matches = torch.zeros((n_img - 1, n_desc, 4), dtype=torch.int32, device="cuda")
    d_counts = torch.zeros((n_img - 1,), dtype=torch.int32, device="cuda")
    ridx = torch.empty((n_desc, 2), dtype=torch.int32, device="cuda"); rdist = torch.empty((n_desc, 2), dtype=torch.float32, device="cuda")

    def plain():
        ctx.match_pairs_dev(sets, pairs, d_matches, n_desc, d_counts)

    def mutual():
        ctx.match_pairs_dev(sets, pairs, d_matches, n_desc, d_counts, cross_check=True)

    def two_pass():
        ctx.match_pairs_dev(sets, pairs, d_matches, n_desc, d_counts)
        for a, b in pairs:
            ctx.knn2_dev(sets[b], sets[a], ridx, rdist)

    res = {name: timed(f) for name, f in (("plain", plain), ("mutual", mutual), ("two-pass", two_pass))}
    plain(); torch.cuda.synchronize(); n_plain = int(d_counts.sum().item())
    mutual(); torch.cuda.synchronize(); n_mut = int(d_counts.sum().item())
    kp, kpm = kernel_ms(plain)
    km, kmm = kernel_ms(mutual)
    print("%-8s C%d chain %d x %d: plain %.3f ms (min %.3f)  mutual %.3f ms (min %.3f) = %.2fx plain  two-pass %.3f ms (min %.3f) = %.2fx plain"
          % (norm, 4, n_img, n_desc, *res["plain"], *res["mutual"], res["mutual"][0] / res["plain"][0], *res["two-pass"],
             res["two-pass"][0] / res["plain"][0]))
    print("         kNN kernel per call: plain %.3f ms (merge + re-score %.3f)  mutual %.3f ms (merge + re-score %.3f)  matches: plain %d  mutual %d"
          % (kp, kpm, km, kmm, n_plain, n_mut))
    for s in sets:
        s.close()
