"""How descriptor sets are built and refreshed (the host half of match.hip), against the CPU oracle: the two refresh entry points
on every layout the preparation kernel tells apart, Hamming2 rows from strided host matrices through the per-image C entry
points, and a failed device allocation in every constructor and in the cross-check launch sequence."""
import ctypes as C

import numpy as np
import pytest

import oracle as orc
from sfm_opencv_amd import _lib, api, synth

pytestmark = pytest.mark.gpu

# (columns of the tensor, first column of the rows, dim)
LAYOUTS = {
    "dim128": (128, 0, 128), "dim64": (64, 0, 64), "dim32": (32, 0, 32),              # 16 values per lane
    "dim100": (100, 0, 100), "dim40": (40, 0, 40),                                  # 4 values per lane, dim_pad 128 / 64
    "ld132": (132, 0, 128),                                                         # strided, still the fast path
    "ld129": (129, 0, 128),                                                         # ld % 4 != 0: slow path
    "ld160_col1": (160, 1, 128),                                                    # base not 16-byte aligned: slow path
}
ROWS = (1, 129, 300)


def _int_rows(rng, rows, cols):
    return rng.integers(0, 256, (rows, cols)).astype(np.float32)


def _knn_dev(ctx, qs, ts, nq):
    import torch
    idx = torch.empty((nq, 2), dtype=torch.int32, device="cuda"); dist = torch.empty((nq, 2), dtype=torch.float32, device="cuda")
    ctx.knn2_dev(qs, ts, idx, dist, force_path=2)
    ctx.synchronize()
    return idx.cpu().numpy(), dist.cpu().numpy()


def _check_sets_hold(ctx, sets, rows):
    """kNN-2 of every set against the next one on the int8 path equals the oracle's on `rows`"""
    for i in range(len(sets)):
        j = (i + 1) % len(sets)
        gi, gd = _knn_dev(ctx, sets[i], sets[j], rows[i].shape[0])
        oi, od = orc.knn2_l2(rows[i], rows[j])
        assert np.array_equal(gi, oi), (i, j)
        assert np.array_equal(gd.view(np.uint32), od.view(np.uint32)), (i, j)
        assert sets[i].info()["exact_u8"]


@pytest.mark.parametrize("batched", [False, True], ids=["DescSet.refresh", "Context.refresh_descsets"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_refresh_takes_up_rows_rewritten_in_place(ctx, layout, batched):
    import torch
    cols, c0, dim = LAYOUTS[layout]
    rng = np.random.default_rng(sum(map(ord, layout)))
    base = [torch.from_numpy(_int_rows(rng, r, cols)).cuda() for r in ROWS]
    sets = [ctx.descset_l2(b[:, c0:c0 + dim]) for b in base]
    new = [_int_rows(rng, r, cols) for r in ROWS]
    for b, n in zip(base, new):
        b.copy_(torch.from_numpy(n))
    torch.cuda.synchronize()
    if batched:
        ctx.refresh_descsets(sets)
    else:
        for s in sets:
            s.refresh()
    _check_sets_hold(ctx, sets, [np.ascontiguousarray(n[:, c0:c0 + dim]) for n in new])


def test_refresh_descsets_mixed_dims_and_a_hamming2_set(ctx):
    """dim 32 and dim 128 in one launch (the block covers the fewest rows any of them needs); the Hamming2 set is passed over"""
    import torch
    rng = np.random.default_rng(17)
    shapes = [(300, 32), (129, 128), (129, 32), (300, 128)]
    base = [torch.from_numpy(_int_rows(rng, r, d)).cuda() for r, d in shapes]
    sets = [ctx.descset_l2(b) for b in base]
    hrows = rng.integers(0, 256, (70, 61), dtype=np.uint8)
    ham = ctx.descset_hamming2(torch.from_numpy(hrows).cuda())
    new = [_int_rows(rng, r, d) for r, d in shapes]
    for b, n in zip(base, new):
        b.copy_(torch.from_numpy(n))
    torch.cuda.synchronize()
    ctx.refresh_descsets([sets[0], sets[1], ham, sets[2], sets[3]])
    _check_sets_hold(ctx, [sets[0], sets[2]], [new[0], new[2]])
    _check_sets_hold(ctx, [sets[1], sets[3]], [new[1], new[3]])
    gi, gd = ctx.knn2_hamming2(hrows, hrows)
    hq = torch.empty((70, 2), dtype=torch.int32, device="cuda"); hd = torch.empty((70, 2), dtype=torch.float32, device="cuda")
    ctx.knn2_dev(ham, ham, hq, hd)
    ctx.synchronize()
    oi, od = orc.knn2_hamming2(hrows, hrows)
    assert np.array_equal(hq.cpu().numpy(), oi) and np.array_equal(hd.cpu().numpy().view(np.uint32), od.view(np.uint32))
    assert np.array_equal(gi, oi) and np.array_equal(gd.view(np.uint32), od.view(np.uint32))


# ------------------------------------------------------------------------------------------------
# Hamming2 rows of matrices embedded in wider buffers, through the per-image C entry points
# ------------------------------------------------------------------------------------------------
def _embedded(rows, ld=80, col=3):
    wide = np.full((max(rows.shape[0], 1), ld), 0xA5, np.uint8)
    view = wide[:rows.shape[0], col:col + rows.shape[1]]
    view[...] = rows
    return wide, view


@pytest.mark.parametrize("nbytes", [61, 64, 32])
@pytest.mark.parametrize("nq,nt", [(1, 1), (70, 33), (257, 300)])
def test_hamming2_strided_host_rows_through_the_per_image_entry_points(ctx, nq, nt, nbytes):
    d = synth.akaze_descriptor_chain(2, max(nq, nt), nbytes=nbytes, seed=nq + nbytes)
    q, t = np.ascontiguousarray(d[0][:nq]), np.ascontiguousarray(d[1][:nt])
    qw, qv = _embedded(q); tw, tv = _embedded(t)
    assert qv.ctypes.data % 4 == 3 and qv.strides[0] == 80
    idx = np.empty((nq, 2), np.int32); dist = np.empty((nq, 2), np.float32)
    assert ctx.lib.sfmhip_knn2_hamming2_u8(ctx.h, qv.ctypes.data, nq, tv.ctypes.data, nt, nbytes, 80, 80, idx.ctypes.data, dist.ctypes.data) == 0
    oi, od = orc.knn2_hamming2(q, t)
    assert np.array_equal(idx, oi) and np.array_equal(dist.view(np.uint32), od.view(np.uint32))
    out = np.zeros(nq, api.DMATCH); n = C.c_int(-1)
    assert ctx.lib.sfmhip_match_features_hamming2(ctx.h, qv.ctypes.data, nq, tv.ctypes.data, nt, nbytes, 80, 80, out.ctypes.data, C.byref(n)) == 0
    assert np.array_equal(out[:n.value], orc.match_features_hamming2(q, t))


def test_hamming2_per_image_entry_points_without_query_rows(ctx):
    t = synth.akaze_descriptor_chain(1, 33, nbytes=61, seed=4)[0]
    tw, tv = _embedded(t); qw, qv = _embedded(t[:0])
    idx = np.empty((1, 2), np.int32); dist = np.empty((1, 2), np.float32)
    assert ctx.lib.sfmhip_knn2_hamming2_u8(ctx.h, qv.ctypes.data, 0, tv.ctypes.data, 33, 61, 80, 80, idx.ctypes.data, dist.ctypes.data) == 0
    out = np.zeros(1, api.DMATCH); n = C.c_int(-1)
    assert ctx.lib.sfmhip_match_features_hamming2(ctx.h, qv.ctypes.data, 0, tv.ctypes.data, 33, 61, 80, 80, out.ctypes.data, C.byref(n)) == 0
    assert n.value == 0


# ------------------------------------------------------------------------------------------------
# a failed allocation is an error, and the next call works
# ------------------------------------------------------------------------------------------------
def _batch_create(ctx, mats):
    """the batch constructor through the library itself: (rc, handles)"""
    ham = mats[0].dtype == np.uint8
    n = len(mats)
    ptrs = (C.c_void_p * n)(*[m.ctypes.data for m in mats])
    rows = np.array([m.shape[0] for m in mats], np.int32)
    ld = (C.c_size_t * n)(*[m.shape[1] for m in mats])
    out = (C.c_void_p * n)(*[0xdead0] * n)
    fn = ctx.lib.sfmhip_descsets_create_hamming2_host if ham else ctx.lib.sfmhip_descsets_create_l2_host
    rc = fn(ctx.h, ptrs, rows.ctypes.data, mats[0].shape[1], ld, n, out)
    return rc, [out[i] for i in range(n)]


def _chain_of(case):
    if case == "hamming2_batch":
        return [np.ascontiguousarray(c) for c in synth.akaze_descriptor_chain(3, 40, nbytes=61, seed=8)]
    chain = [np.ascontiguousarray(c).copy() for c in synth.sift_descriptor_chain(3, 40, seed=8)]
    if case == "l2_batch_one_float_image":
        chain[1][20, 5] += 0.25
    return chain


@pytest.mark.parametrize("case", ["l2_batch", "l2_batch_one_float_image", "hamming2_batch"])
def test_a_failed_allocation_in_a_batch_constructor_leaves_no_set_and_the_next_call_works(ctx, case):
    chain = _chain_of(case)
    assert ctx.lib.sfmhip_debug_fail_allocations(ctx.h, 1) == 0
    rc, handles = _batch_create(ctx, chain)
    assert rc == _lib.E_HIP and handles == [None] * 3
    assert ctx.lib.sfmhip_debug_fail_allocations(ctx.h, 0) == 0
    rc, handles = _batch_create(ctx, chain)
    assert rc == 0 and all(handles)
    sets = [api.DescSet(ctx, C.c_void_p(h), 40) for h in handles]
    ham = case == "hamming2_batch"
    if case == "l2_batch_one_float_image":
        assert [s.info()["exact_u8"] for s in sets] == [True, False, True]
    ratio = 0.97 if ham else 0.6
    knn = orc.knn2_hamming2 if ham else orc.knn2_l2
    got = ctx.match_pairs(sets, [[0, 1], [1, 2]], ratio=ratio)
    for p, g in enumerate(got):
        assert np.array_equal(g, orc.ratio_filter(*knn(chain[p], chain[p + 1]), ratio=ratio)), p
    assert sum(len(g) for g in got) > 0


@pytest.mark.parametrize("kind", ["l2_40x40", "hamming2_40x61"])
def test_a_failed_allocation_in_a_per_image_constructor_and_the_next_call_works(ctx, kind):
    rng = np.random.default_rng(23)
    if kind == "l2_40x40":
        q = _int_rows(rng, 40, 40)
        t = np.clip(q[rng.permutation(40)] + rng.integers(-1, 2, (40, 40)), 0, 255).astype(np.float32)
        make, knn, ratio = ctx.descset_l2, orc.knn2_l2, 0.6
    else:
        q, t = [np.ascontiguousarray(c) for c in synth.akaze_descriptor_chain(2, 40, nbytes=61, seed=9)]
        make, knn, ratio = ctx.descset_hamming2, orc.knn2_hamming2, 0.97
    ts = make(t)
    assert ctx.lib.sfmhip_debug_fail_allocations(ctx.h, 1) == 0
    with pytest.raises(api.SfmHipError, match=r"libsfmhip error -2"):
        make(q)
    assert ctx.lib.sfmhip_debug_fail_allocations(ctx.h, 0) == 0
    qs = make(q)
    got = ctx.match_pairs([qs, ts], [[0, 1]], ratio=ratio)[0]
    assert len(got) > 0 and np.array_equal(got, orc.ratio_filter(*knn(q, t), ratio=ratio))


def test_a_failed_allocation_in_a_cross_check_and_the_next_call_works(ctx):
    q, t = [np.ascontiguousarray(c) for c in synth.sift_descriptor_chain(2, 40, seed=12)]
    sets = [ctx.descset_l2(q), ctx.descset_l2(t)]
    assert ctx.lib.sfmhip_debug_fail_allocations(ctx.h, 1) == 0
    with pytest.raises(api.SfmHipError, match=r"libsfmhip error -2"):
        ctx.match_pairs(sets, [[0, 1]], cross_check=True)
    assert ctx.lib.sfmhip_debug_fail_allocations(ctx.h, 0) == 0
    got = ctx.match_pairs(sets, [[0, 1]], cross_check=True)[0]
    plain = orc.ratio_filter(*orc.knn2_l2(q, t))
    rev = orc.knn2_l2(t, q)[0][:, 0]
    want = plain[rev[plain["trainIdx"]] == plain["queryIdx"]]
    assert len(want) > 0 and np.array_equal(got, want)
