"""The definition of sfmhip_build_tracks (include/sfmhip.h) restated in numpy / plain Python, written from the definition and not from the
kernels: a sequential union-find over the valid elements, a stable argsort by root, a walk over the runs.  Helpers that turn a synthetic
scene into key points and match lists live here too, so that the CPU and the GPU tests build the same inputs."""
import numpy as np

DMATCH = np.dtype([("queryIdx", "<i4"), ("trainIdx", "<i4"), ("imgIdx", "<i4"), ("distance", "<f4")])
KEYPOINT = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
KEEP_FIRST = 1


def roots_of(n, edges):
    """root[g] = the smallest member of g's component, by a sequential union-find (min-root hooking, path halving)"""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in edges:
        ra, rb = find(int(a)), find(int(b))
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(g) for g in range(n)], np.int64).reshape(n)


def valid_elements(n_kp, pairs, matches, counts):
    """(mask of the valid elements (n_pairs, max_per_pair), number of ignored ones, ga, gb: the global ids of both ends)"""
    n_kp = np.asarray(n_kp, np.int64); n_img = len(n_kp)
    off = np.concatenate([[0], np.cumsum(n_kp)])
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    P = len(pairs); S = matches.shape[1] if matches.ndim == 2 else 0
    c = np.clip(np.asarray(counts, np.int64).reshape(P), 0, S)
    taken = np.arange(S)[None, :] < c[:, None]
    a, b = pairs[:, 0], pairs[:, 1]
    pair_ok = (a >= 0) & (a < n_img) & (b >= 0) & (b < n_img) & (a != b)
    sa = np.where(pair_ok, a, 0); sb = np.where(pair_ok, b, 0)
    qi = matches["queryIdx"].astype(np.int64).reshape(P, S); ti = matches["trainIdx"].astype(np.int64).reshape(P, S)
    ok = taken & pair_ok[:, None] & (qi >= 0) & (qi < n_kp[sa][:, None]) & (ti >= 0) & (ti < n_kp[sb][:, None])
    return ok, int(taken.sum() - ok.sum()), off[sa][:, None] + qi, off[sb][:, None] + ti


def build_tracks(n_kp, pairs, matches, counts, min_len=2, flags=0, kp=None):
    """every output of sfmhip_build_tracks as a dict: track_of (n_feat), obs_cam / obs_pt / obs_kp (n_obs), obs_uv (n_obs, 2; with kp),
    track_len (n_tracks), matches_out (list of arrays, one per pair), counts_out, stats (8)"""
    n_kp = np.asarray(n_kp, np.int64); n_img = len(n_kp)
    off = np.concatenate([[0], np.cumsum(n_kp)]); n = int(off[-1])
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2); P = len(pairs)
    matches = np.asarray(matches, DMATCH).reshape(P, -1) if P else np.zeros((0, 0), DMATCH)
    track_of = np.full(n, -1, np.int32)
    out = dict(track_of=track_of, obs_cam=np.zeros(0, np.int32), obs_pt=np.zeros(0, np.int32), obs_kp=np.zeros(0, np.int32), obs_uv=np.zeros((0, 2)),
               track_len=np.zeros(0, np.int32), matches_out=[np.zeros(0, DMATCH) for _ in range(P)], counts_out=np.zeros(P, np.int32), stats=np.zeros(8, np.int32))
    if n == 0 or P == 0:
        return out
    ok, ignored, ga, gb = valid_elements(n_kp, pairs, matches, counts)
    root = roots_of(n, zip(ga[ok], gb[ok]))
    order = np.argsort(root, kind="stable")
    img_of = np.repeat(np.arange(n_img), n_kp)
    n_tracks = multi = conflicting = short = longest = 0
    oc, op, okp, tl = [], [], [], []
    r = 0
    while r < n:
        e = r
        while e < n and root[order[e]] == root[order[r]]:
            e += 1
        members = order[r:e]
        first = [j == 0 or img_of[members[j]] != img_of[members[j - 1]] for j in range(len(members))]
        length = sum(first)
        if len(members) >= 2:
            multi += 1
            conflict = length < len(members)
            conflicting += conflict
            if not conflict or (flags & KEEP_FIRST):
                if length >= min_len:
                    for g, f in zip(members, first):
                        if f:
                            track_of[g] = n_tracks
                            oc.append(img_of[g]); op.append(n_tracks); okp.append(g - off[img_of[g]])
                    tl.append(length); longest = max(longest, length)
                    n_tracks += 1
                else:
                    short += 1
        r = e
    out["obs_cam"] = np.array(oc, np.int32).reshape(-1); out["obs_pt"] = np.array(op, np.int32).reshape(-1); out["obs_kp"] = np.array(okp, np.int32).reshape(-1)
    out["track_len"] = np.array(tl, np.int32).reshape(-1)
    if kp is not None:
        out["obs_uv"] = np.array([[float(kp[i]["x"][k]), float(kp[i]["y"][k])] for i, k in zip(oc, okp)], np.float64).reshape(-1, 2)
    safe_a = np.where(ok, ga, 0); safe_b = np.where(ok, gb, 0)
    keep = ok & (track_of[safe_a] >= 0) & (track_of[safe_b] >= 0)
    out["matches_out"] = [matches[q][keep[q]] for q in range(P)]
    out["counts_out"] = keep.sum(1).astype(np.int32)
    out["stats"] = np.array([n_tracks, len(oc), multi, conflicting, short, ignored, longest, 0], np.int32)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# inputs: packing, and a synthetic scene as key points and match lists
# ---------------------------------------------------------------------------------------------------------------------------------------
def pack(lists, stride=None):
    """(matches (n_pairs, stride) padded with -1, counts) of a list of DMATCH arrays or of (queryIdx, trainIdx) pair lists"""
    arrs = []
    for m in lists:
        if not (isinstance(m, np.ndarray) and m.dtype == DMATCH):
            e = np.asarray(m, np.int64).reshape(-1, 2)
            m = np.zeros(len(e), DMATCH); m["queryIdx"] = e[:, 0]; m["trainIdx"] = e[:, 1]; m["distance"] = 1.0
        arrs.append(m)
    S = max([len(m) for m in arrs], default=0) if stride is None else stride
    out = np.zeros((len(arrs), S), DMATCH)
    out["queryIdx"] = -1; out["trainIdx"] = -1; out["imgIdx"] = -1
    for q, m in enumerate(arrs):
        out[q, :len(m)] = m
    return out, np.array([len(m) for m in arrs], np.int32)


def scene_lists(sc, reach=1):
    """A synth.ba_scene as key points and match lists: key point k of image i is the k-th observation of camera i (the scene lists them by
    (camera, point)); pair (i, j), i < j <= i + reach, matches the key points of the points both see.  Returns (kp: KEYPOINT arrays,
    xy: (n, 2) float64 arrays, pairs, lists of DMATCH arrays, point of every key point per image)"""
    n_cam = sc["n_cam"]
    oc, op, uv = sc["obs_cam"], sc["obs_pt"], sc["obs_uv"]
    kp, xy, pt_of = [], [], []
    for i in range(n_cam):
        sel = np.nonzero(oc == i)[0]
        k = np.zeros(len(sel), KEYPOINT); k["x"] = uv[sel, 0]; k["y"] = uv[sel, 1]; k["size"] = 1.0
        kp.append(k); xy.append(uv[sel].copy()); pt_of.append(op[sel].astype(np.int64))
    pairs, lists = [], []
    for i in range(n_cam):
        for j in range(i + 1, min(n_cam, i + reach + 1)):
            _, qa, tb = np.intersect1d(pt_of[i], pt_of[j], assume_unique=True, return_indices=True)
            m = np.zeros(len(qa), DMATCH); m["queryIdx"] = qa; m["trainIdx"] = tb; m["imgIdx"] = 0; m["distance"] = 0.25
            pairs.append((i, j)); lists.append(m)
    return kp, xy, np.array(pairs, np.int32).reshape(-1, 2), lists, pt_of


def same_partition(label_a, label_b):
    """two labelings of the same items (-1: none, compared as such) describe one partition"""
    a = np.asarray(label_a, np.int64); b = np.asarray(label_b, np.int64)
    if a.shape != b.shape or not np.array_equal(a < 0, b < 0):
        return False
    m = a >= 0
    ab = np.unique(np.stack([a[m], b[m]], 1), axis=0)
    return len(ab) == len(np.unique(a[m])) == len(np.unique(b[m]))
