"""GPU: the cross check (SFMHIP_MATCH_MUTUAL) -- the reverse best of every train row (sfmhip_knn2_mutual_dev) on every kNN path,
bit for bit against the oracle's kNN-2 with the operands swapped, and mutual matching (sfmhip_match_pairs_ex and the Python / C++
layers above it) against the oracle's ratio tail filtered by that reverse best."""
import os
import subprocess

import numpy as np
import pytest

import oracle as orc
from sfm_opencv_amd import _lib, api, features_io, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def _mutual_dev(ctx, q, t, path):
    import torch
    ham = q.dtype == np.uint8
    mk = ctx.descset_hamming2 if ham else ctx.descset_l2
    qs = mk(np.ascontiguousarray(q)); ts = mk(np.ascontiguousarray(t))
    nq, nt = q.shape[0], t.shape[0]
    idx = torch.empty((max(nq, 1), 2), dtype=torch.int32, device="cuda"); dist = torch.empty((max(nq, 1), 2), dtype=torch.float32, device="cuda")
    ri = torch.full((max(nt, 1),), -7, dtype=torch.int32, device="cuda"); rd = torch.empty((max(nt, 1),), dtype=torch.float32, device="cuda")
    ctx.knn2_mutual_dev(qs, ts, idx, dist, ri, rd, force_path=path)
    pi = torch.empty_like(idx); pdist = torch.empty_like(dist)
    if nq:
        ctx.knn2_dev(qs, ts, pi, pdist, force_path=path)
    ctx.synchronize()
    return (idx[:nq].cpu().numpy(), dist[:nq].cpu().numpy(), ri[:nt].cpu().numpy(), rd[:nt].cpu().numpy(),
            pi[:nq].cpu().numpy(), pdist[:nq].cpu().numpy())


def _check_mutual(ctx, q, t, path):
    i2, d2, ri, rd, pi, pd = _mutual_dev(ctx, q, t, path)
    knn = orc.knn2_hamming2 if q.dtype == np.uint8 else orc.knn2_l2
    if t.shape[0]:
        oi, od = knn(t, q)
        assert np.array_equal(ri, oi[:, 0]), f"rev_idx mismatch at train rows {np.nonzero(ri != oi[:, 0])[0][:10]}"
        assert np.array_equal(rd.view(np.uint32), od[:, 0].view(np.uint32))
    # the forward half is what sfmhip_knn2_dev gives
    assert np.array_equal(i2, pi) and np.array_equal(d2.view(np.uint32), pd.view(np.uint32))
    return ri, rd


L2_SHAPES = [(1, 2), (5, 3), (128, 128), (129, 255), (300, 1000), (2000, 2000), (513, 4500), (4500, 513)]


@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("nq,nt", L2_SHAPES)
def test_reverse_best_l2(ctx, nq, nt, path):
    d = synth.sift_descriptor_chain(2, max(nq, nt), seed=11 + nq)
    _check_mutual(ctx, d[0][:nq], d[1][:nt], path)


@pytest.mark.parametrize("path", [3, 4])
@pytest.mark.parametrize("nq,nt", [(1, 1), (2, 1), (3, 2), (70, 33), (256, 257), (513, 300), (1000, 3000), (300, 4097), (9000, 257)])
def test_reverse_best_hamming2(ctx, nq, nt, path):
    d = synth.akaze_descriptor_chain(2, max(nq, nt), nbytes=61, seed=nq + nt)
    _check_mutual(ctx, d[0][:nq], d[1][:nt], path)


@pytest.mark.parametrize("path", [2, 4])
def test_reverse_best_10k(ctx, path):
    if path == 2:
        d = synth.sift_descriptor_chain(2, 10000, seed=4)
    else:
        d = synth.akaze_descriptor_chain(2, 10000, nbytes=61, seed=4)
    _check_mutual(ctx, d[0], d[1], path)


@pytest.mark.parametrize("path", [1, 2, 3, 4])
def test_reverse_ties_go_to_the_lowest_query(ctx, path):
    """every query row repeated 8 times, spread over waves, workgroups and (for 10k rows) query blocks: the lowest copy wins"""
    rng = np.random.default_rng(3)
    if path <= 2:
        q = np.tile(rng.integers(0, 3, (90, 128)), (8, 1)).astype(np.float32)
        t = rng.integers(0, 3, (300, 128)).astype(np.float32)
    else:
        q = np.tile(rng.integers(0, 256, (90, 61), dtype=np.uint8), (8, 1))
        t = rng.integers(0, 256, (300, 61), dtype=np.uint8)
    ri, _ = _check_mutual(ctx, q, t, path)
    assert (ri < 90).all()


def _three_squares(n):
    for a in range(int(n ** 0.5), -1, -1):
        for b in range(int((n - a * a) ** 0.5), -1, -1):
            c2 = n - a * a - b * b
            c = int(round(c2 ** 0.5))
            if c * c == c2 and max(a, b, c) <= 255:
                return a, b, c
    return None


def test_reverse_sqrt_collision_rescore(ctx):
    """the transpose of test_knn2_l2_sqrt_collision_rescore: two QUERY rows at d^2 >= 2^22 share a float sqrtf; the lower query index
    (larger integer distance) must win -- the int8 path's column re-score"""
    base = 125 * 200 * 200
    k = next(k for k in range(1, 5000)
             if np.sqrt(np.float32(base + k)) == np.sqrt(np.float32(base + k + 1)) and _three_squares(k) and _three_squares(k + 1))
    rng = np.random.default_rng(5)
    q = rng.integers(230, 256, (300, 128)).astype(np.float32)
    q[0, :125] = 200; q[0, 125:] = _three_squares(k + 1)
    q[1, :125] = 200; q[1, 125:] = _three_squares(k)
    t = np.zeros((130, 128), np.float32)
    t[1:] = rng.integers(0, 3, (129, 128))
    oi, od = orc.knn2_l2(t, q)
    assert oi[0, 0] == 0 and oi[0, 1] == 1 and od[0, 0] == od[0, 1]
    ri, _ = _check_mutual(ctx, q, t, 2)
    assert ri[0] == 0


@pytest.mark.parametrize("path", [1, 2, 3, 4])
@pytest.mark.parametrize("nq", [1, 100, 129, 300, 513])
def test_pad_query_rows_never_win(ctx, path, nq):
    rng = np.random.default_rng(nq)
    if path <= 2:
        q = rng.integers(200, 256, (nq, 128)).astype(np.float32)       # every real query far from the trains
        t = np.zeros((70, 128), np.float32)
    else:
        q = np.full((nq, 61), 0xFF, np.uint8)                          # all-0xFF queries against all-zero trains
        t = np.zeros((70, 61), np.uint8)
    ri, _ = _check_mutual(ctx, q, t, path)
    assert ((ri >= 0) & (ri < nq)).all()


@pytest.mark.parametrize("path", [1, 2, 3, 4])
def test_reverse_with_no_queries(ctx, path):
    ham = path > 2
    q = np.zeros((0, 61), np.uint8) if ham else np.zeros((0, 128), np.float32)
    t = (np.random.default_rng(1).integers(0, 256, (40, 61), dtype=np.uint8) if ham
         else np.random.default_rng(1).integers(0, 256, (40, 128)).astype(np.float32))
    _, _, ri, rd, _, _ = _mutual_dev(ctx, q, t, path)
    assert (ri == -1).all()
    assert (rd == (np.float32(2.0 ** 31) if ham else np.finfo(np.float32).max)).all()


def _want_mutual(q, t, ratio=0.6):
    knn = orc.knn2_hamming2 if q.dtype == np.uint8 else orc.knn2_l2
    plain = orc.ratio_filter(*knn(q, t), ratio=ratio)
    if len(plain) == 0 or t.shape[0] == 0:
        return plain, plain
    rev = knn(t, q)[0][:, 0]
    return plain, plain[rev[plain["trainIdx"]] == plain["queryIdx"]]


def _chains(random=False):
    if random:          # no structure: the ratio test lets many one-sided matches through, the cross check must remove them
        rng = np.random.default_rng(17)
        return ([rng.integers(0, 256, (r, 128)).astype(np.float32) for r in (600, 900, 300, 700)],
                [rng.integers(0, 256, (r, 61), dtype=np.uint8) for r in (500, 900, 130, 600)])
    sift = [c.copy() for c in synth.sift_descriptor_chain(5, 1500, seed=21)]
    sift[2] = sift[2][:700]
    ak = synth.akaze_descriptor_chain(4, 900, seed=2)
    ak = [ak[0][:500], ak[1], ak[2][:130], ak[3]]
    return sift, ak


@pytest.mark.parametrize("ratio", [0.6, 0.99])
def test_mutual_matching_chains(ctx, ratio):
    n_fewer = 0
    for chain in _chains(random=ratio > 0.6):
        sets = ctx.descsets_host(chain)
        pairs = np.stack([np.arange(len(chain) - 1), np.arange(1, len(chain))], 1)
        plain = ctx.match_pairs(sets, pairs, ratio=ratio)
        mut = ctx.match_pairs(sets, pairs, ratio=ratio, cross_check=True)
        again = ctx.match_pairs(sets, pairs, ratio=ratio, cross_check=True)
        for p, (a, b) in enumerate(pairs):
            wp, wm = _want_mutual(chain[a], chain[b], ratio)
            assert np.array_equal(plain[p], wp)
            assert np.array_equal(mut[p], wm), p
            assert np.array_equal(again[p], mut[p])
            assert np.isin(mut[p]["queryIdx"], plain[p]["queryIdx"]).all()
            n_fewer += len(mut[p]) < len(plain[p])
            assert len(mut[p]) > 0
        if ratio != 0.6:
            continue
        # the Python entry points above the C-ABI
        got = api.match_features_for_all(chain, ctx=ctx, cross_check=True)
        for g, w in zip(got, mut):
            assert np.array_equal(g, w)
        assert np.array_equal(api.match_features(chain[0], chain[1], ctx=ctx, cross_check=True), mut[0])
        assert all(np.array_equal(g, w) for g, w in zip(api.match_features_for_all(chain, ctx=ctx), plain))
    if ratio > 0.6:
        assert n_fewer > 0          # (the synthetic chains' ratio-0.6 matches are often all mutual already)


def test_flags_zero_is_the_plain_entry_point_and_bad_flags_are_refused(ctx):
    import ctypes as C
    chain = _chains()[0]
    sets = ctx.descsets_host(chain)
    pairs = np.array([[0, 1], [1, 2], [3, 4]], np.int32)
    arr = (C.c_void_p * len(sets))(*[s.handle for s in sets])
    mpp = 1500
    outs = []
    for fn, extra in ((ctx.lib.sfmhip_match_pairs, ()), (ctx.lib.sfmhip_match_pairs_ex, (0,))):
        out = np.zeros((3, mpp), api.DMATCH); cnt = np.zeros(3, np.int32)
        assert fn(ctx.h, arr, len(sets), pairs.ctypes.data, 3, 0.6, 10.0, 5.0, *extra, out.ctypes.data, mpp, cnt.ctypes.data) == 0
        outs.append((out.tobytes(), cnt.tobytes()))
    assert outs[0] == outs[1]
    out = np.zeros((3, mpp), api.DMATCH); cnt = np.zeros(3, np.int32)
    for bad in (2, 3, -1, 1 << 8):
        assert ctx.lib.sfmhip_match_pairs_ex(ctx.h, arr, len(sets), pairs.ctypes.data, 3, 0.6, 10.0, 5.0, bad, out.ctypes.data, mpp, cnt.ctypes.data) == _lib.E_ARG
        assert ctx.lib.sfmhip_match_pairs_ex_dev(ctx.h, arr, len(sets), pairs.ctypes.data, 3, 0.6, 10.0, 5.0, bad, out.ctypes.data, mpp, cnt.ctypes.data) == _lib.E_ARG
    carr = (C.c_void_p * 1)(ctx.h.value)
    ptrs = (C.c_void_p * 2)(chain[0].ctypes.data, chain[1].ctypes.data)
    rows = np.array([c.shape[0] for c in chain[:2]], np.int32)
    assert ctx.lib.sfmhip_match_pairs_multi_ex(carr, 1, 1, ptrs, rows.ctypes.data, 128, None, 2, pairs.ctypes.data, 1, 0.6, 10.0, 5.0, 2,
                                               out.ctypes.data, mpp, cnt.ctypes.data) == _lib.E_ARG


@pytest.mark.parametrize("nq,nt", [(0, 50), (50, 0), (50, 1), (1, 1)])
def test_mutual_matching_edge_sizes(ctx, nq, nt):
    rng = np.random.default_rng(nq + 3 * nt)
    for mats in ([rng.integers(0, 256, (nq, 128)).astype(np.float32), rng.integers(0, 256, (nt, 128)).astype(np.float32)],
                 [rng.integers(0, 256, (nq, 61), dtype=np.uint8), rng.integers(0, 256, (nt, 61), dtype=np.uint8)]):
        sets = [ctx.descset_hamming2(m) if m.dtype == np.uint8 else ctx.descset_l2(m) for m in mats]
        got = ctx.match_pairs(sets, [[0, 1]], ratio=0.99, cross_check=True)[0]
        _, want = _want_mutual(mats[0], mats[1])
        assert np.array_equal(got, want)


@pytest.mark.parametrize("n_ctx", [1, 2, 3])
def test_mutual_matching_over_several_contexts(ctx, n_ctx):
    ctxs = [api.Context(0) for _ in range(n_ctx)]
    for chain in _chains():
        pairs = np.stack([np.arange(len(chain) - 1), np.arange(1, len(chain))], 1)
        want = ctx.match_pairs(ctx.descsets_host(chain), pairs, cross_check=True)
        got = api.match_pairs_multi(ctxs, chain, pairs, cross_check=True)
        assert len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want))
    for c in ctxs:
        c.close()


def test_host_convenience_forms(ctx):
    d = synth.sift_descriptor_chain(2, 700, seed=8)
    i2, d2, ri, rd = ctx.knn2_mutual_l2(d[0], d[1][:500])
    oi, od = orc.knn2_l2(d[1][:500], d[0])
    assert np.array_equal(ri, oi[:, 0]) and np.array_equal(rd.view(np.uint32), od[:, 0].view(np.uint32))
    assert np.array_equal(i2, orc.knn2_l2(d[0], d[1][:500])[0])
    h = synth.akaze_descriptor_chain(2, 400, nbytes=61, seed=8)
    i2, d2, ri, rd = ctx.knn2_mutual_hamming2(h[0][:300], h[1])
    oi, od = orc.knn2_hamming2(h[1], h[0][:300])
    assert np.array_equal(ri, oi[:, 0]) and np.array_equal(rd.view(np.uint32), od[:, 0].view(np.uint32))


@pytest.mark.parametrize("fixture", ["crazyhorse_features.bin", "crazyhorse_features_akaze.bin"])
def test_nview_driver_with_cross_check(ctx, tmp_path, fixture):
    host = os.path.join(ROOT, "sfm_opencv_amd", "host")
    subprocess.check_call(["make", "-C", host], stdout=subprocess.DEVNULL)
    path = os.path.join(GOLD, fixture)
    out = subprocess.run([os.path.join(host, "NViewReconstruct"), path, str(tmp_path), "--quiet", "--cross-check"], capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert "Save structure done." in out.stdout
    for f in ("structure.yml", "structure_ba.yml", "structure_ba.ply"):
        assert (tmp_path / f).stat().st_size > 0
    descs = features_io.read_features(path)["descriptors"]
    plain = api.match_features_for_all(descs, ctx=ctx)
    mut = api.match_features_for_all(descs, ctx=ctx, cross_check=True)
    assert all(len(m) <= len(p) for m, p in zip(mut, plain)) and sum(map(len, mut)) > 0
