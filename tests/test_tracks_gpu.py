"""GPU: sfmhip_build_tracks against its restatement (tests/tracks_ref.py).  Every output is compared in every byte, through the raw ctypes
call into sentinel-filled arrays, so that "nothing behind the written prefix is touched" is part of the comparison.  Each case is the
smallest shape at which its part can go wrong; the references are computed once and shared."""
import ctypes as C
import functools
import os
import struct
import subprocess

import numpy as np
import pytest

import tracks_ref as tr
from sfm_opencv_amd import _lib, api, synth

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))

I32_FILL, F64_FILL, BYTE_FILL = -7777, -12345.5, 0xA5
OUTPUTS = ("track_of", "obs_cam", "obs_pt", "obs_kp", "obs_uv", "track_len", "matches_out", "counts_out", "stats")


def _sentinels(n, P, S):
    a = dict(track_of=np.full(n, I32_FILL, np.int32), obs_cam=np.full(n, I32_FILL, np.int32), obs_pt=np.full(n, I32_FILL, np.int32),
             obs_kp=np.full(n, I32_FILL, np.int32), obs_uv=np.full((n, 2), F64_FILL), track_len=np.full(n // 2, I32_FILL, np.int32),
             counts_out=np.full(P, I32_FILL, np.int32), stats=np.full(8, I32_FILL, np.int32))
    a["matches_out"] = np.frombuffer(bytes([BYTE_FILL]) * (P * S * 16), tr.DMATCH).reshape(P, S).copy()
    return a


def _expected(ref, n, P, S, with_uv):
    """the sentinel arrays with what the definition writes: track_of, counts_out and stats whole, of the others the prefixes"""
    e = _sentinels(n, P, S)
    e["track_of"][:] = ref["track_of"]; e["counts_out"][:] = ref["counts_out"]; e["stats"][:] = ref["stats"]
    no, nt = len(ref["obs_cam"]), len(ref["track_len"])
    for k in ("obs_cam", "obs_pt", "obs_kp"):
        e[k][:no] = ref[k]
    if with_uv:
        e["obs_uv"][:no] = ref["obs_uv"]
    e["track_len"][:nt] = ref["track_len"]
    for q, m in enumerate(ref["matches_out"]):
        e["matches_out"][q, :len(m)] = m
    return e


def _kp_table(kp):
    return (C.c_void_p * len(kp))(*[(k.ctypes.data if k is not None and len(k) else None) for k in kp])


def _call(ctx, n_kp, pairs, matches, counts, kp=None, min_len=2, flags=0, null=(), out=None):
    """the raw host call into sentinel-filled arrays (or into `out`); the outputs named in `null` are passed as NULL"""
    n_kp = np.ascontiguousarray(n_kp, np.int32); pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    P = len(pairs); S = matches.shape[1] if P else 0
    out = out or _sentinels(int(n_kp.sum()), P, S)
    if kp is None:
        null = tuple(null) + ("obs_uv",)
    p = {k: (None if k in null or out[k].size == 0 else out[k].ctypes.data) for k in OUTPUTS}
    rc = ctx.lib.sfmhip_build_tracks(ctx.h, len(n_kp), n_kp.ctypes.data, pairs.ctypes.data if P else None, P, matches.ctypes.data if P * S else None, S,
                                     counts.ctypes.data if P else None, _kp_table(kp) if kp is not None else None, min_len, flags,
                                     p["track_of"], p["obs_cam"], p["obs_pt"], p["obs_kp"], p["obs_uv"], p["track_len"], p["matches_out"], p["counts_out"], p["stats"])
    return rc, out


def _assert_bytes(got, want, skip=()):
    for k in OUTPUTS:
        if k not in skip:
            assert got[k].tobytes() == want[k].tobytes(), (k, got["stats"], want["stats"])


# ---------------------------------------------------------------------------------------------------------------------------------------
# the cases: name -> (n_kp, pairs, matches, counts, kp or None)
# ---------------------------------------------------------------------------------------------------------------------------------------
def _random_kp(n_kp, seed):
    rng = np.random.default_rng(seed)
    kp = []
    for c in n_kp:
        k = np.zeros(c, tr.KEYPOINT); k["x"] = rng.random(c) * 1000; k["y"] = rng.random(c) * 700
        kp.append(k)
    return kp


def _sized(n_feat, seed):
    """three images of n_feat key points in all, a third of the smallest image matched at random in every pair: roots all over the range"""
    rng = np.random.default_rng(seed)
    a = n_feat // 3; n_kp = [a, n_feat - 2 * a - 1, a + 1]
    lists = []
    pairs = [(0, 1), (1, 2), (2, 0)]
    for i, j in pairs:
        k = min(n_kp[i], n_kp[j]) // 3
        lists.append(np.stack([rng.permutation(n_kp[i])[:k], rng.permutation(n_kp[j])[:k]], 1))
    return (n_kp, pairs) + tr.pack(lists) + (None,)


def _corrupt(lists, n_kp, pairs, frac, seed):
    rng = np.random.default_rng(seed)
    out = []
    for (a, b), m in zip(pairs, lists):
        m = m.copy()
        hit = rng.random(len(m)) < frac
        m["trainIdx"][hit] = rng.integers(0, n_kp[b], size=int(hit.sum()))
        out.append(m)
    return out


@functools.lru_cache(maxsize=None)
def _case(name):
    if name == "smallest":
        return ([1, 1], [(0, 1)]) + tr.pack([[(0, 0)]]) + (None,)
    if name == "conflict":
        return ([2, 1, 1], [(0, 1), (1, 2), (2, 0)]) + tr.pack([[(0, 0)], [(0, 0)], [(0, 1)]]) + (None,)
    if name in ("chain70", "chain70_reversed"):
        pairs = [(i, i + 1) for i in range(69)]
        if name.endswith("reversed"):
            pairs = pairs[::-1]
        return ([1] * 70, pairs) + tr.pack([[(0, 0)]] * 69) + (None,)
    if name == "giant":
        k = np.arange(10000)
        return ([10000, 10000], [(0, 1), (0, 1)]) + tr.pack([np.stack([k, k], 1), np.stack([np.zeros_like(k), k], 1)]) + (None,)
    if name == "invalid":
        m, c = tr.pack([[(0, 0)], [(0, 0), (1, 1), (2, 0)], [(0, 0)], [(0, 0), (-1, -1), (1, 7)]], stride=3)
        c[:] = [1, 3, 1, 9]
        return ([2, 2], [(0, 0), (0, 1), (0, 5), (1, 0)], m, c, None)
    if name == "empty_images":
        n_kp = [0, 3, 0, 0, 2, 0]
        kp = _random_kp(n_kp, 3)
        kp[0] = kp[2] = kp[5] = None
        return (n_kp, [(1, 4), (4, 1), (0, 1), (4, 5)]) + tr.pack([[(0, 1), (2, 0)], [(1, 0)], [(0, 0)], [(1, 0)]]) + (kp,)
    if name.startswith("n"):
        return _sized(int(name[1:]), len(name))
    if name == "both_directions":
        n_kp, pairs, m, c, _ = _sized(900, 11)
        lists = [m[q, :c[q]] for q in range(3)]
        rev = []
        for e in lists:
            r = e.copy(); r["queryIdx"] = e["trainIdx"]; r["trainIdx"] = e["queryIdx"]
            rev.append(np.concatenate([r, r]))
        return (n_kp, list(pairs) + [(j, i) for i, j in pairs]) + tr.pack([np.concatenate([e, e]) for e in lists] + rev) + (None,)
    if name.startswith("scene"):
        sc = synth.ba_scene(30, 3000)
        kp, _, pairs, lists, _ = tr.scene_lists(sc, 3 if "reach3" in name else 1)
        n_kp = [len(k) for k in kp]
        if "corrupt" in name:
            lists = _corrupt(lists, n_kp, pairs, 0.02, 17)
        return (n_kp, pairs) + tr.pack(lists) + (kp,)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _ref(name, min_len=2, flags=0):
    n_kp, pairs, m, c, kp = _case(name)
    kpz = None if kp is None else [k if k is not None else np.zeros(0, tr.KEYPOINT) for k in kp]
    return tr.build_tracks(n_kp, pairs, m, c, min_len, flags, kpz)


def _check(ctx, name, min_len=2, flags=0):
    n_kp, pairs, m, c, kp = _case(name)
    ref = _ref(name, min_len, flags)
    rc, got = _call(ctx, n_kp, pairs, m, c, kp, min_len, flags)
    assert rc == 0, ctx.lib.sfmhip_last_error(ctx.h)
    _assert_bytes(got, _expected(ref, int(np.sum(n_kp)), len(pairs), m.shape[1], kp is not None))
    return ref


CASES = [("smallest", 2, 0), ("conflict", 2, 0), ("conflict", 2, 1), ("conflict", 4, 1), ("chain70", 2, 0), ("chain70_reversed", 2, 0), ("giant", 2, 0), ("giant", 2, 1),
         ("invalid", 2, 0), ("empty_images", 2, 0), ("n255", 2, 1), ("n256", 2, 1), ("n257", 2, 0), ("n65535", 2, 1), ("n65537", 3, 1), ("n9000", 2, 0),
         ("both_directions", 2, 1), ("scene_chain", 2, 0), ("scene_chain", 3, 0), ("scene_reach3", 2, 0), ("scene_reach3", 3, 1), ("scene_chain_corrupt", 2, 0),
         ("scene_chain_corrupt", 2, 1), ("scene_reach3_corrupt", 3, 0), ("scene_reach3_corrupt", 2, 1)]


@pytest.mark.parametrize("name, min_len, flags", CASES)
def test_every_output_equals_the_restatement(ctx, name, min_len, flags):
    ref = _check(ctx, name, min_len, flags)
    s = ref["stats"].tolist()
    assert s[7] == 0
    if name == "smallest":
        assert s == [1, 2, 1, 0, 0, 0, 2, 0]
    if name == "conflict":
        assert s == {(2, 0): [0, 0, 1, 1, 0, 0, 0, 0], (2, 1): [1, 3, 1, 1, 0, 0, 3, 0], (4, 1): [0, 0, 1, 1, 1, 0, 0, 0]}[(min_len, flags)]
        if (min_len, flags) == (2, 1):
            assert ref["track_of"].tolist() == [0, -1, 0, 0]
    if name.startswith("chain70"):
        assert s == [1, 70, 1, 0, 0, 0, 70, 0]
    if name == "giant":
        assert s[2:4] == [1, 1] and s[0] == flags
    if name == "invalid":
        assert ref["track_of"].tolist() == [0, 1, 0, 1] and s[5] == 5
    if name.startswith("n") or "corrupt" in name:
        assert s[0] > 0 and s[3] > 0                                       # tracks and conflicts both occur
    if name in ("scene_chain", "scene_reach3"):
        sc = synth.ba_scene(30, 3000)
        _, _, _, _, pt_of = tr.scene_lists(sc, 1)
        want = np.concatenate(pt_of)
        if min_len == 3:
            want = np.where(np.bincount(sc["obs_pt"])[want] >= 3, want, -1)
        assert tr.same_partition(ref["track_of"], want) and s[3] == 0      # the tracks are the scene's points
    if "corrupt" in name:
        _, pairs, m, c, _ = _case(name)
        for q, kept in enumerate(ref["matches_out"]):                       # the survivors: a subset of the input in the input's order
            src = m[q, :c[q]]                                                # a key point of the query image occurs once in a pair's list
            order = np.argsort(src["queryIdx"], kind="stable")
            pos = order[np.searchsorted(src["queryIdx"][order], kept["queryIdx"])]
            assert src[pos].tobytes() == kept.tobytes() and (np.diff(pos) > 0).all()
        assert 0 < ref["counts_out"].sum() < c.sum()


def test_both_directions_and_duplicates_change_nothing(ctx):
    n_kp, pairs, m, c, _ = _case("both_directions")
    _, got = _call(ctx, n_kp, pairs, m, c, None, 2, 1)
    _, half = _call(ctx, n_kp, pairs[:3], m[:3], c[:3], None, 2, 1)
    _assert_bytes(got, half, skip=("matches_out", "counts_out", "stats"))
    assert np.array_equal(got["stats"][:5], half["stats"][:5])


def test_two_runs_and_any_order_give_the_same_bytes(ctx):
    n_kp, pairs, m, c, kp = _case("scene_reach3_corrupt")
    pairs = np.asarray(pairs)
    rc, a = _call(ctx, n_kp, pairs, m, c, kp, 2, 1)
    rc2, b = _call(ctx, n_kp, pairs, m, c, kp, 2, 1)
    assert rc == 0 and rc2 == 0
    _assert_bytes(a, b)
    rng = np.random.default_rng(23)
    perm = rng.permutation(len(pairs))
    lists = []
    for q in perm:
        e = m[q, :c[q]][rng.permutation(c[q])]
        lists.append(np.concatenate([e, e[:len(e) // 2]]))                  # shuffled inside the pair, half of the edges twice
    m2, c2 = tr.pack(lists)
    rc3, d = _call(ctx, n_kp, pairs[perm], m2, c2, kp, 2, 1)
    assert rc3 == 0
    _assert_bytes(a, d, skip=("matches_out", "counts_out"))


def test_dev_form_on_resident_tensors_equals_the_host_form(ctx):
    import torch
    n_kp, pairs, m, c, kp = _case("scene_chain_corrupt")
    ref = _ref("scene_chain_corrupt", 2, 1)
    n = int(np.sum(n_kp)); P, S = m.shape
    dev = torch.device("cuda", ctx.device)
    d_m = torch.from_numpy(m.view(np.uint8).reshape(P, S * 16)).to(dev); d_c = torch.from_numpy(c).to(dev)
    d_kp = [torch.from_numpy(k.view(np.uint8)).to(dev) for k in kp]
    sent = _sentinels(n, P, S)
    d = {k: torch.from_numpy(v.view(np.uint8).reshape(-1) if k == "matches_out" else v).to(dev) for k, v in sent.items()}
    torch.cuda.synchronize(dev)
    ctx.build_tracks_dev(n_kp, pairs, d_m, S, d_c, d_kp, 2, "keep-first", d["track_of"], d["obs_cam"], d["obs_pt"], d["obs_kp"], d["obs_uv"], d["track_len"],
                         d["matches_out"], d["counts_out"], d["stats"])
    ctx.synchronize()
    got = {k: (v.cpu().numpy().view(tr.DMATCH).reshape(P, S) if k == "matches_out" else v.cpu().numpy()) for k, v in d.items()}
    _assert_bytes(got, _expected(ref, n, P, S, True))
    # the Python wrapper of the host form trims to the same prefixes
    t = ctx.build_tracks(n_kp, pairs, m, c, kp=kp, min_len=2, conflicts="keep-first")
    assert np.array_equal(t[0], ref["track_of"]) and np.array_equal(t[1], ref["obs_cam"]) and np.array_equal(t[4], ref["obs_uv"]) and np.array_equal(t[5], ref["track_len"])
    assert np.array_equal(t[6], ref["stats"]) and np.array_equal(t[8], ref["counts_out"])


@pytest.mark.parametrize("null", [(k,) for k in OUTPUTS] + [("track_of", "counts_out"), OUTPUTS])
def test_any_output_may_be_null(ctx, null):
    n_kp, pairs, m, c, kp = _case("scene_chain_corrupt")
    want = _expected(_ref("scene_chain_corrupt", 2, 0), int(np.sum(n_kp)), len(pairs), m.shape[1], True)
    sent = _sentinels(int(np.sum(n_kp)), len(pairs), m.shape[1])
    for k in null:
        want[k] = sent[k]
    rc, got = _call(ctx, n_kp, pairs, m, c, kp, 2, 0, null=null)
    assert rc == 0
    _assert_bytes(got, want)


def test_no_pairs_and_no_features(ctx):
    rc, got = _call(ctx, [2, 1], np.zeros((0, 2), np.int32), np.zeros((0, 0), tr.DMATCH), np.zeros(0, np.int32))
    assert rc == 0 and got["track_of"].tolist() == [-1] * 3 and not got["stats"].any() and got["obs_cam"].tolist() == [I32_FILL] * 3
    m, c = tr.pack([[(0, 0)]])
    rc, got = _call(ctx, [0, 0], [(0, 1)], m, c)
    assert rc == 0 and not got["stats"].any() and got["counts_out"].tolist() == [0]
    rc, got = _call(ctx, [2, 2], [(0, 1)], np.zeros((1, 0), tr.DMATCH), np.array([4], np.int32))
    assert rc == 0 and got["track_of"].tolist() == [-1] * 4 and not got["stats"].any() and got["counts_out"].tolist() == [0]


def test_bad_arguments_leave_the_outputs_alone(ctx):
    n_kp, pairs, m, c, _ = _case("conflict")
    kp = _random_kp(n_kp, 1)
    n_kp = np.array(n_kp, np.int32); pairs = np.array(pairs, np.int32)
    fresh = _sentinels(4, 3, 1)
    bad = [dict(min_len=1), dict(min_len=0), dict(flags=2), dict(flags=-1), dict(n_kp=np.array([2, -1, 1], np.int32)),
           dict(kp=[kp[0], None, kp[2]])]
    for kw in bad:
        args = dict(n_kp=n_kp, pairs=pairs, matches=m, counts=c, kp=kp, min_len=2, flags=0); args.update(kw)
        rc, got = _call(ctx, out=_sentinels(4, 3, 1), **args)
        assert rc == _lib.E_ARG, kw
        _assert_bytes(got, fresh)
    lib, h = ctx.lib, ctx.h
    o = _sentinels(4, 3, 1)
    p = {k: o[k].ctypes.data for k in OUTPUTS}

    def raw(n_img=3, nk=n_kp.ctypes.data, pr=pairs.ctypes.data, P=3, mm=m.ctypes.data, S=1, cc=c.ctypes.data, kpt=None, hh=h, **ov):
        q = dict(p, obs_uv=None); q.update(ov)
        return lib.sfmhip_build_tracks(hh, n_img, nk, pr, P, mm, S, cc, kpt, 2, 0, q["track_of"], q["obs_cam"], q["obs_pt"], q["obs_kp"], q["obs_uv"], q["track_len"],
                                       q["matches_out"], q["counts_out"], q["stats"])
    big = np.full(3, 2 ** 30, np.int32)
    for rc in (raw(hh=None), raw(nk=None), raw(pr=None), raw(mm=None), raw(cc=None), raw(P=-1), raw(S=-1), raw(n_img=0), raw(n_img=65537), raw(nk=big.ctypes.data),
               raw(obs_uv=o["obs_uv"].ctypes.data), raw(obs_cam=p["track_of"]), raw(obs_pt=p["obs_kp"] + 4), raw(matches_out=m.ctypes.data), raw(counts_out=c.ctypes.data),
               raw(stats=p["track_of"])):
        assert rc == _lib.E_ARG
    _assert_bytes(o, fresh)
    assert raw() == 0 and o["stats"].tolist() == [0, 0, 1, 1, 0, 0, 0, 0]


def test_a_failed_allocation_is_an_error_and_the_next_call_works(ctx):
    import torch
    n_kp, pairs, m, c, kp = _case("scene_chain")
    n = int(np.sum(n_kp)); P, S = m.shape
    assert ctx.lib.sfmhip_debug_fail_allocations(ctx.h, 1) == 0
    rc, got = _call(ctx, n_kp, pairs, m, c, kp)
    assert rc == _lib.E_HIP
    _assert_bytes(got, _sentinels(n, P, S))
    # the enqueue-only form: its first block is the pair table
    dev = torch.device("cuda", ctx.device)
    d_m = torch.from_numpy(m.view(np.uint8).reshape(P, S * 16)).to(dev); d_c = torch.from_numpy(c).to(dev)
    d_t = torch.full((n,), I32_FILL, dtype=torch.int32, device=dev); d_s = torch.full((8,), I32_FILL, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    assert ctx.lib.sfmhip_debug_fail_allocations(ctx.h, 1) == 0
    with pytest.raises(api.SfmHipError):
        ctx.build_tracks_dev(n_kp, pairs, d_m, S, d_c, d_track_of=d_t, d_stats=d_s)
    ctx.synchronize()
    assert (d_t.cpu().numpy() == I32_FILL).all() and (d_s.cpu().numpy() == I32_FILL).all()
    ctx.build_tracks_dev(n_kp, pairs, d_m, S, d_c, d_track_of=d_t, d_stats=d_s)
    ctx.synchronize()
    ref = _ref("scene_chain")
    assert np.array_equal(d_t.cpu().numpy(), ref["track_of"]) and np.array_equal(d_s.cpu().numpy(), ref["stats"])
    _check(ctx, "scene_chain")


def test_cpp_mirror_writes_the_same_arrays(ctx, tmp_path):
    n_kp, pairs, m, c, kp = _case("scene_chain_corrupt")
    ref = _ref("scene_chain_corrupt", 3, 1)
    host = os.path.join(HERE, "host")
    subprocess.check_call(["make", "-C", host, "-f", "tracks.mk", "tracks_test"], stdout=subprocess.DEVNULL)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<4i", len(n_kp), len(pairs), 3, 1)); f.write(np.asarray(n_kp, np.int32).tobytes())
        for k in kp:
            f.write(k.tobytes())
        f.write(np.ascontiguousarray(pairs, np.int32).tobytes()); f.write(c.tobytes())
        for q in range(len(pairs)):
            f.write(m[q, :c[q]].tobytes())
    out = subprocess.run([os.path.join(host, "tracks_test"), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    want = b"".join([ref["stats"].tobytes(), ref["track_of"].tobytes(), ref["obs_cam"].tobytes(), ref["obs_pt"].tobytes(), ref["obs_kp"].tobytes(),
                     ref["obs_uv"].tobytes(), ref["track_len"].tobytes(), ref["counts_out"].tobytes()] + [e.tobytes() for e in ref["matches_out"]])
    assert open(tmp_path / "out.bin", "rb").read() == want


# ---------------------------------------------------------------------------------------------------------------------------------------
# end to end: tracks -> N-view triangulation -> bundle adjustment
# ---------------------------------------------------------------------------------------------------------------------------------------
def _point_of_track(tracks, pt_of):
    """the scene point of every track, by its observations; every observation of a track must name the same point"""
    pt = np.array([pt_of[i][k] for i, k in zip(tracks.obs_cam, tracks.obs_kp)])
    first = np.full(len(tracks.track_len), -1, np.int64)
    first[tracks.obs_pt[::-1]] = pt[::-1]
    assert np.array_equal(first[tracks.obs_pt], pt)
    return first


def test_structure_from_tracks_noise_free(ctx):
    sc = synth.ba_scene(9, 400, noise_px=0.0, outlier_frac=0.0)
    _, xy, pairs, lists, pt_of = tr.scene_lists(sc, 1)
    structure, idx, tracks = api.structure_from_tracks(sc["K_true"], sc["ext_true"], xy, pairs, lists, ctx=ctx)
    assert tracks.stats.tolist()[:6] == [400, sc["n_obs"], 400, 0, 0, 0] and structure.shape == (400, 3)
    pt = _point_of_track(tracks, pt_of)
    assert sorted(pt.tolist()) == list(range(400))
    err = np.abs(structure - sc["pts_true"][pt]).max()
    print("structure_from_tracks, noise-free: max |X - X_true| = %.3g" % err)
    assert err < 1e-7                                                      # the bound of tests/test_fullsize_gpu.py on triangulate_tracks
    assert all(np.array_equal(np.sort(pt[i[i >= 0]]), np.sort(p)) for i, p in zip(idx, pt_of))
    assert [len(a) for a in tracks.matches_for_all] == [len(a) for a in lists]


def test_tracks_feed_bundle_adjustment_like_the_scenes_own_lists(ctx):
    sc = synth.ba_scene(9, 400, noise_px=0.5, outlier_frac=0.0)
    kp, _, pairs, lists, pt_of = tr.scene_lists(sc, 1)
    structure, idx, tracks = api.structure_from_tracks(sc["K_true"], sc["ext_true"], kp, pairs, lists, ctx=ctx)
    assert tracks.stats[0] == 400 and tracks.stats[1] == sc["n_obs"]
    opts = ctx.ba_options(max_num_iterations=4)
    K1, e1 = sc["K_true"].copy(), sc["ext_true"].copy()
    s1 = api.bundle_adjustment(K1, e1, idx, kp, structure, ctx=ctx, opts=opts)
    # the same call on the scene's own lists: the same observations (the key points' floats) under the scene's point numbers
    uv = np.stack([np.concatenate([k["x"] for k in kp]), np.concatenate([k["y"] for k in kp])], 1).astype(np.float64)
    oc = np.concatenate([np.full(len(p), i, np.int32) for i, p in enumerate(pt_of)]); op = np.concatenate(pt_of).astype(np.int32)
    structure2, _ = ctx.triangulate_tracks(sc["K_true"], sc["ext_true"], oc, op, uv, 400)
    K2, e2 = sc["K_true"].copy(), sc["ext_true"].copy()
    s2 = api.bundle_adjustment(K2, e2, [p.astype(np.int32) for p in pt_of], kp, structure2, ctx=ctx, opts=opts)
    print("final cost through tracks %.12g, through the scene's lists %.12g" % (s1["final_cost"], s2["final_cost"]))
    assert s1["num_residuals"] == s2["num_residuals"] and s1["final_cost"] < s1["initial_cost"]
    # one problem under two numberings of its points: the bound of tests/test_ba_gpu.py::test_observation_order_invariance
    assert s1["final_cost"] <= s2["final_cost"] * (1.0 + 1e-9)
