"""world_size 2 over gloo: the sharding of the hot path and the all-reduce hook (the N>1 host logic of bench.py).
CPU test: the per-rank arithmetic is done by the oracle (no GPU in this container).  GPU test (-m gpu): the two ranks are
two processes that drive libsfmhip on the one card of the box (rehearsal knobs SFM_DIST_BACKEND=gloo, SFM_LOCAL_DEVICE=0)
through the same hook that sums the library's device buffers over RCCL on an 8-GPU node."""
import os
import socket

import numpy as np
import pytest

from sfm_opencv_amd import dist as sdist
from sfm_opencv_amd import synth


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _worker(rank, world, port, out_dir):
    import torch.distributed as dist
    import oracle as orc
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    orc.set_num_threads(2)
    r, w, _ = sdist.init_process_group("gloo")
    assert (r, w) == (rank, world)
    sc = synth.ba_scene(9, 400)
    o = orc.ba_default_options(jacobi_scaling=0)
    pts_l, oc_l, op_l, uv_l, ids = sdist.shard_points(sc["obs_cam"], sc["obs_pt"], sc["obs_uv"], sc["pts0"], rank, world)
    S, rhs, cost = orc.ba_reduced_system(sc["K0"], sc["ext0"], pts_l, oc_l, op_l, uv_l, -25.0, opts=o)
    n = S.shape[0]
    msg = np.concatenate([S.reshape(-1), rhs, [cost, float(len(ids)), float(len(oc_l))]])
    hook = sdist.make_allreduce_hook(device="cpu")
    assert hook(msg.ctypes.data, msg.size, 0) == 0
    # a second, different buffer through the same hook (its cache is keyed by (address, count)): a fresh copy of this
    # rank's three tail scalars must come back as the sum over ranks, i.e. equal to the tail of the first message
    tail = np.array([cost, float(len(ids)), float(len(oc_l))])
    assert hook(tail.ctypes.data, 3, 0) == 0
    tail_ok = np.array_equal(tail, msg[-3:])
    Sf, rf, cf = orc.ba_reduced_system(sc["K0"], sc["ext0"], sc["pts0"], sc["obs_cam"], sc["obs_pt"], sc["obs_uv"], -25.0, opts=o)
    ok = (np.abs(msg[:n * n].reshape(n, n) - Sf).max() <= 1e-12 * np.abs(Sf).max()
          and np.abs(msg[n * n:n * n + n] - rf).max() <= 1e-12 * np.abs(rf).max() and tail_ok
          and abs(msg[-3] - cf) <= 1e-12 * cf)
    pairs_g, images, pairs_l = sdist.shard_pairs(23, rank, world)
    np.save(os.path.join(out_dir, f"r{rank}.npy"),
            np.array([ok, len(ids), len(oc_l), pairs_g[0, 0], pairs_g[-1, 1], images[0], images[-1], len(pairs_l)], float))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_sharding_and_allreduce(tmp_path):
    import torch.multiprocessing as mp
    port = _free_port()
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    a = np.load(tmp_path / "r0.npy"); b = np.load(tmp_path / "r1.npy")
    assert a[0] == 1 and b[0] == 1                       # summed partial systems == full system on both ranks
    assert a[1] + b[1] == 400                            # points partitioned
    sc = synth.ba_scene(9, 400)
    assert a[2] + b[2] == sc["n_obs"]                    # every observation on exactly one rank
    assert abs(a[2] - b[2]) <= 0.1 * sc["n_obs"]         # balanced by observation count
    # chain pairs 0..21 split in two contiguous blocks with one halo image
    assert (a[3], a[4], b[3], b[4]) == (0, 11, 11, 22) and a[7] + b[7] == 22
    assert (a[5], a[6], b[5], b[6]) == (0, 11, 11, 22)


@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_shard_helpers_cover_everything(world):
    sc = synth.ba_scene(7, 333)
    seen_obs = 0; seen_pts = []
    for r in range(world):
        pts_l, oc, op, uv, ids = sdist.shard_points(sc["obs_cam"], sc["obs_pt"], sc["obs_uv"], sc["pts0"], r, world)
        assert np.array_equal(pts_l, sc["pts0"][ids]) and (op >= 0).all() and (op < len(ids)).all()
        seen_obs += len(oc); seen_pts += list(ids)
    assert seen_obs == sc["n_obs"] and sorted(seen_pts) == list(range(333))
    # camera windows: a rank's points start at cameras no lower than the previous rank's
    firsts = []
    for r in range(world):
        _, oc, op, _, ids = sdist.shard_points(sc["obs_cam"], sc["obs_pt"], sc["obs_uv"], sc["pts0"], r, world)
        if len(oc):
            f = np.full(len(ids), 10**9); np.minimum.at(f, op, oc); firsts.append((f.min(), f.max()))
    assert all(firsts[i][1] <= firsts[i + 1][0] for i in range(len(firsts) - 1))
    # the round 1-2 partition by id stays available: contiguous id ranges in rank order
    by_id = [sdist.shard_points(sc["obs_cam"], sc["obs_pt"], sc["obs_uv"], sc["pts0"], r, world, by="id")[4] for r in range(world)]
    assert np.array_equal(np.concatenate(by_id), np.arange(333))
    pairs = [sdist.shard_pairs(10, r, world)[0] for r in range(world)]
    allp = np.concatenate([p for p in pairs if len(p)])
    assert np.array_equal(allp, np.stack([np.arange(9), np.arange(1, 10)], 1))
    assert sdist.shard_range(0, 0, world) == (0, 0)


def _gpu_worker(rank, world, port, out_dir, shape, n_iter):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      SFM_DIST_BACKEND="gloo", SFM_LOCAL_DEVICE="0")
    import time
    import torch
    import torch.distributed as dist
    from sfm_opencv_amd import api
    r, w, local = sdist.init_process_group()
    assert (r, w, local) == (rank, world, 0)
    torch.cuda.set_device(local)
    ctx = api.Context(local, use_torch_stream=True)
    sc = synth.ba_scene(*shape)
    pts_l, oc_l, op_l, uv_l, ids = sdist.shard_points(sc["obs_cam"], sc["obs_pt"], sc["obs_uv"], sc["pts0"], rank, world)
    pb = ctx.ba_create(sc["K0"], sc["ext0"], pts_l, oc_l, op_l, uv_l)
    inner = sdist.make_allreduce_hook()
    calls = [0]

    def hook(ptr, count, stream):
        calls[0] += 1
        return inner(ptr, count, stream)

    pb.set_allreduce(hook, rank, world)
    s = pb.iterate(n_iter)
    torch.cuda.synchronize(); dist.barrier()
    c0 = calls[0]
    t0 = time.perf_counter()
    s2 = pb.iterate(n_iter)
    torch.cuda.synchronize(); dist.barrier()
    ms = 1e3 * (time.perf_counter() - t0) / n_iter
    calls_timed = calls[0] - c0
    pb.reset()
    s = pb.iterate(n_iter)
    K, ext, pts = pb.params()
    np.savez(os.path.join(out_dir, f"g{rank}.npz"), K=K, ext=ext, pts=pts, ids=ids, cost=s["final_cost"], succ=s["successful_steps"], ms=ms,
             calls_timed=calls_timed, succ_timed=s2["successful_steps"])
    pb.close(); ctx.close()
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(24, 4000), (200, 60000)])
def test_two_processes_drive_libsfmhip_over_gloo(ctx, tmp_path, shape):
    """The real N>1 path: one PROCESS per rank (here both on the box's one card), torch.distributed for the exchange, the
    library's packed reduced-system message and its five step scalars summed by sfm_opencv_amd.dist's hook; against the
    unsharded solve of the same scene in this process.  (200 cameras: four dissection segments.)"""
    import torch.multiprocessing as mp
    n_iter = 5
    sc = synth.ba_scene(*shape)
    ref = ctx.ba_create(sc["K0"], sc["ext0"], sc["pts0"], sc["obs_cam"], sc["obs_pt"], sc["obs_uv"])
    sr = ref.iterate(n_iter); Kr, extr, ptsr = ref.params(); ref.close()
    mp.spawn(_gpu_worker, args=(2, _free_port(), str(tmp_path), shape, n_iter), nprocs=2, join=True)
    for r in range(2):
        g = np.load(tmp_path / f"g{r}.npz")
        assert int(g["succ"]) == sr["successful_steps"] and abs(float(g["cost"]) - sr["final_cost"]) <= 1e-9 * sr["final_cost"]
        assert np.abs(g["ext"] - extr).max() <= 1e-9 and np.abs(g["K"] - Kr).max() <= 1e-9 * np.abs(Kr).max()
        assert np.abs(g["pts"] - ptsr[g["ids"]]).max() <= 1e-9
        # ONE collective per LM iteration where the step is accepted with rho >= 0.937 (radius x 3, the guess the speculative
        # linearisation was damped with): the step scalars ride in that linearisation's message.  A rejected step, or one accepted
        # with a smaller radius growth, costs a second one (the old count).  Iterations 6-10 of the 24-camera scene all hit; the
        # 200-camera scene is closer to convergence there and misses four times.
        # (successful_steps counts from the start of the problem: both iterate() calls)
        assert int(g["succ_timed"]) == 2 * n_iter, int(g["succ_timed"])
        assert n_iter <= int(g["calls_timed"]) <= (n_iter + 1 if shape[0] == 24 else 2 * n_iter - 1), int(g["calls_timed"])
        print(f"[gloo rehearsal {shape}] rank {r}: {float(g['ms']):.3f} ms per LM iteration with two processes on one card, "
              f"{int(g['calls_timed'])} hook calls in {n_iter} iterations")


@pytest.mark.gpu
def test_native_rccl_hook_world_one(ctx):
    """The in-library RCCL hook (csrc/rccl.hip: dlopen'ed librccl, ncclAllReduce on the context's stream) on a communicator of
    one rank -- all the box has.  The multi-rank code path runs (packed message, folded step scalars, speculative linearisation)
    and must reproduce the plain single-rank iterations."""
    if not ctx.rccl_available():
        pytest.skip("librccl.so not found")
    import torch
    sc = synth.ba_scene(24, 4000)
    args = (sc["K0"], sc["ext0"], sc["pts0"], sc["obs_cam"], sc["obs_pt"], sc["obs_uv"])
    ref = ctx.ba_create(*args); sr = ref.iterate(6); pr = ref.params(); ref.close()
    comm = ctx.rccl_comm_create(ctx.rccl_unique_id(), 0, 1)
    x = torch.arange(5, dtype=torch.float64, device="cuda")
    ctx.rccl_allreduce_f64(comm, x.data_ptr(), 5); ctx.synchronize()
    assert x.tolist() == [0.0, 1.0, 2.0, 3.0, 4.0]
    pb = ctx.ba_create(*args)
    pb.set_rccl(comm, 0, 1)
    s = pb.iterate(6); p = pb.params()
    assert s["successful_steps"] == sr["successful_steps"] and abs(s["final_cost"] - sr["final_cost"]) <= 1e-11 * sr["final_cost"]
    for a, b in zip(p, pr):
        assert np.abs(a - b).max() <= 1e-9 * max(1.0, np.abs(b).max())
    # and the whole LM loop to its termination
    pb.reset(); s2 = pb.run()
    ref = ctx.ba_create(*args); s3 = ref.run(); ref.close()
    assert s2["iterations"] == s3["iterations"] and abs(s2["final_cost"] - s3["final_cost"]) <= 1e-9 * s3["final_cost"]
    pb.close()
    ctx.rccl_comm_destroy(comm)


@pytest.mark.gpu
def test_bench_starts_its_own_ranks_and_reports_one_line(tmp_path):
    """`python bench.py --gpus 2` without a launcher: the parent spawns the two ranks (here sharing one card over gloo, the rehearsal
    knobs of dist.py), rank 0 prints ONE JSON line with n_gpus = 2, strong scaling, and the whole-job figures."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SFM_DIST_BACKEND="gloo", SFM_LOCAL_DEVICE="0")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--config", "small", "--steps", "6", "--warmup", "2",
                          "--full", "--no-cpu-baseline", "--no-gemm"], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    lines = [l for l in out.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 6 and d["scaling"] == "strong" and d["metric"] == "ba_iterations_per_sec"
    assert d["value"] > 0 and d["ba_cost"]["after_timed_steps"] < d["ba_cost"]["initial"]
    assert d["matched_pairs_per_sec"]["value"] > 0 and d["cpu_baseline"] is None


@pytest.mark.gpu
def test_bench_under_the_drivers_launcher(tmp_path):
    """The way the driver starts N > 1: `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1
    --master-port P bench.py --gpus N ...` (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* from the environment) -- here two ranks on one
    card over gloo."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ, SFM_DIST_BACKEND="gloo", SFM_LOCAL_DEVICE="0")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                          "--master-port", str(port), os.path.join(root, "bench.py"), "--gpus", "2", "--config", "small", "--steps", "6",
                          "--warmup", "2", "--full", "--no-cpu-baseline", "--no-gemm"], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    lines = [l for l in out.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["value"] > 0 and d["matched_pairs_per_sec"]["value"] > 0
