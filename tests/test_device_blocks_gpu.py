"""GPU: every call takes its device temporaries from the context's block cache (csrc/common.hpp, sfmhip_ctx::pool).  The calls
that used to own a grow-only block of the context -- kNN workspace and result rows, descriptor tables, the track / reprojection
blocks, the permutation block of sfmhip_ba_get_params -- and sfmhip_triangulate2_f32 (four hipMalloc per call) now share blocks
with everything else, in stream order.  Checked here: a failed allocation is reported and leaves the context usable; the calls
alternate on one context, large -> small -> large, over blocks that come back with somebody else's contents; the reverse pass
of the paths without a fused reverse returns its workspace before the forward pass asks for one.  Every comparison is exact."""
import numpy as np
import pytest

import oracle as orc
from sfm_opencv_amd import _lib, api, synth

pytestmark = pytest.mark.gpu


def _same(a, b):
    """two results (an array, or a list / tuple of them): the same shapes and the same bytes"""
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _tracks_args():
    sc = synth.ba_scene(3, 40, seed=7, min_len=2, max_len=3, perturb=False)          # 3 cameras, 40 points seen by 2-3 of them
    return sc["K_true"], sc["ext_true"], sc["obs_cam"], sc["obs_pt"], sc["obs_uv"], sc["n_pt"]


def _reproj_args():
    K4, ext, oc, op, uv, n_pt = _tracks_args()
    return K4, ext, synth.ba_scene(3, 40, seed=7, min_len=2, max_len=3, perturb=False)["pts_true"], oc, op, uv


def _l2_chain(n_img, rows):
    return synth.sift_descriptor_chain(n_img, rows, seed=40 + rows)


def _chain_pairs(n_img):
    return np.stack([np.arange(n_img - 1), np.arange(1, n_img)], 1).astype(np.int32)


def _knn2_dev(ctx, sets, rows):
    import torch
    idx = torch.empty((rows, 2), dtype=torch.int32, device="cuda"); dist = torch.empty((rows, 2), dtype=torch.float32, device="cuda")
    ctx.knn2_dev(sets[0], sets[1], idx, dist)
    ctx.synchronize()
    return idx.cpu().numpy(), dist.cpu().numpy()


def _small_ba(ctx):
    """4 cameras / 30 points, every third point constant: params() runs the device permutation and the restore kernel"""
    sc = synth.ba_scene(4, 30, seed=9)
    pb = ctx.ba_create(sc["K0"], sc["ext0"], sc["pts0"], sc["obs_cam"], sc["obs_pt"], sc["obs_uv"], pt_const=np.arange(30) % 3 == 0)
    pb.iterate(2)
    return pb, sc


def _call(ctx, name):
    """(setup on ctx, the call under test as a function without arguments, the oracle's result or None)"""
    if name.startswith("triangulate2"):
        s = synth.two_view_scene(int(name.split("_")[1]))
        P1 = orc.projection_matrix(s["K"], s["R1"], s["T1"]); P2 = orc.projection_matrix(s["K"], s["R2"], s["T2"])
        return (lambda: ctx.triangulate2(P1, P2, s["xy1"], s["xy2"])), None
    if name == "triangulate_tracks":
        return (lambda: ctx.triangulate_tracks(*_tracks_args())), None
    if name == "reprojection_errors":
        return (lambda: ctx.reprojection_errors(*_reproj_args())), None
    if name.startswith("match_pairs"):          # match_pairs_<images>_<rows>: the chain pairs of <images> sets of <rows> rows
        n_img, rows = (int(v) for v in name.split("_")[2:])
        chain = _l2_chain(n_img, rows); sets = ctx.descsets_host(chain)
        want = [orc.match_features_l2(chain[a], chain[b]) for a, b in _chain_pairs(n_img)]
        return (lambda: ctx.match_pairs(sets, _chain_pairs(n_img))), want
    if name == "knn2_dev":
        chain = _l2_chain(2, 40); sets = ctx.descsets_host(chain)
        return (lambda: _knn2_dev(ctx, sets, 40)), orc.knn2_l2(chain[0], chain[1])
    if name == "ba_params":
        pb, _ = _small_ba(ctx)
        return (lambda: pb.params()), None
    raise KeyError(name)


_fresh_results = {}


def _fresh(name):
    """the call's result on a context of its own (computed once)"""
    if name not in _fresh_results:
        c = api.Context(0)
        _fresh_results[name] = _call(c, name)[0]()
        c.close()
    return _fresh_results[name]


CALLS = ["triangulate2_1", "triangulate2_257", "triangulate_tracks", "reprojection_errors", "match_pairs_2_40", "knn2_dev", "ba_params"]


@pytest.mark.parametrize("name", CALLS)
def test_a_failed_allocation_is_reported_and_the_next_call_works(ctx, name):
    call, want = _call(ctx, name)
    first = call()
    assert want is None or _same(first, want)
    assert _same(first, _fresh(name))
    assert ctx.lib.sfmhip_debug_fail_allocations(ctx.h, 1) == 0
    try:
        with pytest.raises(api.SfmHipError, match=r"libsfmhip error %d: injected allocation failure" % _lib.E_HIP):
            call()
    finally:
        assert ctx.lib.sfmhip_debug_fail_allocations(ctx.h, 0) == 0
    assert _same(call(), first)


def test_former_scratch_users_alternate_on_one_context(ctx):
    """large -> small -> large over one cache: the three 300-row pairs leave blocks that the small calls cannot take (more than 4x
    their size and above 1 MB, or simply busy) or take with stale contents, and get theirs back with the small calls' contents"""
    big = "match_pairs_4_300"
    for step in (big, "triangulate_tracks", "match_pairs_2_40", "reprojection_errors", "ba_params", big, "trim", big):
        if step == "trim":
            ctx.trim()
            continue
        call, want = _call(ctx, step)
        got = call()
        assert want is None or _same(got, want), step
        assert _same(got, _fresh(step)), step


def _want_mutual(q, t, ratio):
    knn = orc.knn2_hamming2 if q.dtype == np.uint8 else orc.knn2_l2
    plain = orc.ratio_filter(*knn(q, t), ratio=ratio)
    rev = knn(t, q)[0][:, 0]
    return plain[rev[plain["trainIdx"]] == plain["queryIdx"]]


@pytest.mark.parametrize("rows", [40, 129])
@pytest.mark.parametrize("kind", ["exact_f32", "hamming2_valu"])
def test_cross_check_on_the_paths_without_a_fused_reverse(ctx, kind, rows):
    """the swapped kNN-2 takes a workspace and returns it, then the forward pass takes one (the same block, behind it on the stream)"""
    if kind == "exact_f32":
        q, t = (c.copy() for c in synth.sift_descriptor_chain(2, rows, seed=rows))
        q[0, 0] += 0.5          # not an integer: the pair leaves the int8 path for the exact fp32 kernels
        sets = ctx.descsets_host([q, t])
        assert sets[0].info()["exact_u8"] == 0 and sets[1].info()["exact_u8"] == 1
    else:
        q, t = synth.akaze_descriptor_chain(2, rows, nbytes=64, seed=rows)          # 64-byte rows: above the FP4 path's 61
        sets = ctx.descsets_host([q, t])
    want = _want_mutual(q, t, 0.99)
    assert 0 < len(want) < rows
    for _ in range(2):
        assert _same(ctx.match_pairs(sets, [[0, 1]], ratio=0.99, cross_check=True)[0], want)
