"""GPU: the L2 matching kernels of csrc/match.hip at the row lengths, layouts and key values the other test_match_* files leave out --
every instantiation of the int8 kernels (32-, 64- and 128-byte rows; plain, mutual, distance matrix) on rows of all 0 / all 255 /
alternating values and on sets smaller than a tile, pad rows against the worst real row, the distance matrix's three store layouts
at small and odd sizes, the exact fp32 kernel on unaligned rows and at row lengths with and without 16-wide blocks, both re-score
kernels on rows with a tail and with lists fed by more than one pair, and the byte upload at 32 and 64 values.

Integer-valued rows are compared bit for bit with TWO references: the oracle (oracle/orc_match.c) and tests/match_ref.py (int64
squared distances, float32 sqrt, ordered by (float32 distance, index)), which shares no code with it.  General float rows are
compared bit for bit with the oracle and, independently, with float64 distances to a bound worked out from the kernel's summation
order (see test_exact_kernel_layouts_and_row_lengths)."""
import functools

import numpy as np
import pytest

import match_ref as mr
import oracle as orc

pytestmark = pytest.mark.gpu
FLT_MAX = mr.FLT_MAX


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def corner_rows(dim):
    """all 0, all 255, 0/255 alternating, 255/0 alternating, all 128, all 127: biased int8 -128, 127, 0 and -1"""
    alt = np.tile([0, 255], dim)[:dim]
    return np.stack([np.zeros(dim), np.full(dim, 255), alt, 255 - alt, np.full(dim, 128), np.full(dim, 127)]).astype(np.float32)


# ------------------------------------------------------------------------------------------------
# how rows reach a set
# ------------------------------------------------------------------------------------------------
def _host(rows):
    """host rows: integer-valued ones of 32, 64 or 128 values cross as bytes (prep_l2_u8_batched_kernel), the others as floats"""
    return np.ascontiguousarray(rows, np.float32)


def _dense(rows):
    import torch
    return torch.from_numpy(np.array(rows, np.float32)).cuda()          # (a copy: the shared cases are read-only)


def _view(rows, extra, col):
    """the rows as a view of a wider CUDA tensor whose other cells are NaN: a read outside the rows poisons a distance"""
    import torch
    wide = torch.full((max(rows.shape[0], 1), rows.shape[1] + extra), float("nan"), dtype=torch.float32, device="cuda")
    v = wide[:rows.shape[0], col:col + rows.shape[1]]
    v.copy_(torch.from_numpy(np.array(rows, np.float32)))
    return v


def _stride_plus_1(rows):
    v = _view(rows, 1, 0)
    assert v.stride(0) == rows.shape[1] + 1
    return v


def _from_column_1(rows):
    v = _view(rows, 4, 1)
    assert v.data_ptr() % 16 == 4
    return v


LAYOUTS = {"dense": _dense, "stride_dim_plus_1": _stride_plus_1, "from_column_1": _from_column_1}


# ------------------------------------------------------------------------------------------------
# device calls
# ------------------------------------------------------------------------------------------------
def _knn(ctx, qs, ts, nq, path):
    import torch
    idx = torch.full((nq, 2), -7, dtype=torch.int32, device="cuda"); dist = torch.full((nq, 2), -7.0, dtype=torch.float32, device="cuda")
    ctx.knn2_dev(qs, ts, idx, dist, force_path=path)
    ctx.synchronize()
    return idx.cpu().numpy(), dist.cpu().numpy()


def _mutual(ctx, qs, ts, nq, nt, path):
    import torch
    idx = torch.full((nq, 2), -7, dtype=torch.int32, device="cuda"); dist = torch.full((nq, 2), -7.0, dtype=torch.float32, device="cuda")
    ri = torch.full((nt,), -7, dtype=torch.int32, device="cuda"); rd = torch.full((nt,), -7.0, dtype=torch.float32, device="cuda")
    ctx.knn2_mutual_dev(qs, ts, idx, dist, ri, rd, force_path=path)
    ctx.synchronize()
    return idx.cpu().numpy(), dist.cpu().numpy(), ri.cpu().numpy(), rd.cpu().numpy()


def _distmat(ctx, qs, ts, nq, nt, layout="vector"):
    """the matrix in a buffer filled with -1, a guard band on either side: (matrix (nq, ld), guard before, guard after)"""
    import torch
    if layout == "vector":          # 16-byte stores; the base is off a 128-byte line, so never the parity tiling
        ld, guard = (nt + 1 + 3) // 4 * 4, 36
    elif layout == "scalar":        # an odd row stride
        assert nt % 2 == 1
        ld, guard = nt, 33
    else:                           # parity: rows alternate between line-aligned and half a line off
        ld, guard = nt + (16 - nt) % 32, 32
        assert ld % 32 == 16 and ld >= nt
    buf = torch.full((2 * guard + nq * ld,), -1.0, dtype=torch.float32, device="cuda")
    out = buf[guard:guard + nq * ld].view(nq, ld)
    assert buf.data_ptr() % 128 == 0
    assert out.data_ptr() % 128 == {"vector": 16, "scalar": 4, "parity": 0}[layout]
    ctx.l2_distance_matrix_dev(qs, ts, out)
    ctx.synchronize()
    got = buf.cpu().numpy()
    return got[guard:guard + nq * ld].reshape(nq, ld), got[:guard], got[guard + nq * ld:]


def _assert_knn(got, want, what):
    (gi, gd), (wi, wd) = got, want
    assert np.array_equal(gi, wi), f"{what}: index mismatch at rows {np.nonzero((gi != wi).reshape(len(gi), -1).any(1))[0][:10]}"
    assert np.array_equal(_bits(gd), _bits(wd)), f"{what}: distance bits differ at rows {np.nonzero((_bits(gd) != _bits(wd)).reshape(len(gi), -1).any(1))[0][:10]}"


def _int_refs(q, t):
    """[(name, forward kNN-2, reverse best, distance matrix)] of integer rows from the two references"""
    oi, od = orc.knn2_l2(t, q)
    dm = mr.distance_matrix_int(q, t)
    ri, rd = mr.knn2_of_matrix(np.ascontiguousarray(dm.T))
    return [("oracle", orc.knn2_l2(q, t), (oi[:, 0], od[:, 0]), orc.l2_distance_matrix(q, t)),
            ("int64 reference", mr.knn2_of_matrix(dm), (ri[:, 0], rd[:, 0]), dm)]


def _check_int8(ctx, q, t, mkq=_dense, mkt=_host, matrix=True):
    """forced int8 path: plain kNN-2, mutual kNN-2 (forward half and reverse best) and the distance matrix against both references"""
    nq, nt = q.shape[0], t.shape[0]
    qs, ts = ctx.descset_l2(mkq(q)), ctx.descset_l2(mkt(t))
    assert qs.info()["exact_u8"] and ts.info()["exact_u8"]
    plain = _knn(ctx, qs, ts, nq, 2)
    mi, md, ri, rd = _mutual(ctx, qs, ts, nq, nt, 2)
    dm = _distmat(ctx, qs, ts, nq, nt)[0][:, :nt] if matrix else None
    for name, fwd, rev, mat in _int_refs(q, t):
        _assert_knn(plain, fwd, f"knn2 vs {name}")
        _assert_knn((mi, md), fwd, f"mutual forward half vs {name}")
        _assert_knn((ri, rd), rev, f"reverse best vs {name}")
        if matrix:
            assert np.array_equal(_bits(dm), _bits(mat)), f"distance matrix vs {name}"
    return plain, (ri, rd)


# ------------------------------------------------------------------------------------------------
# a. the int8 path at every row length, all three kernels, on the corner values of the keys
# ------------------------------------------------------------------------------------------------
def _corner_case(dim, nq, nt, seed):
    rng = np.random.default_rng(seed)
    q = np.concatenate([corner_rows(dim), rng.integers(0, 256, (nq - 6, dim)).astype(np.float32)])
    pool = np.concatenate([corner_rows(dim), (255 * rng.integers(0, 2, (max(nt - 6, 0), dim))).astype(np.float32)])
    # fewer trains than corner rows: one run per group of nt corner rows, so that every corner row is a train once
    return q, [pool[s:s + nt] for s in (range(0, 6, nt) if nt < 6 else (0,))]


@pytest.mark.parametrize("nt", [1, 2, 3, 33, 129, 257])
@pytest.mark.parametrize("dim", [32, 64, 40, 100, 128])
def test_int8_kernels_on_corner_rows(ctx, dim, nt):
    """knn2_i8_kernel / knn2_i8_mutual_kernel / distmat_i8_kernel <1>, <2> (dim 32, 64; 40 zero-padded to 64) and <4> (100 zero-padded,
    128); 70 queries against 1 .. 257 trains, then the same rows with query and train swapped: the key treats the sides differently
    (|b|^2 + 2 sum b on the train side, the complement on the query side), so (q = 0, t = 255) and (q = 255, t = 0) are two corners"""
    q, trains = _corner_case(dim, 70, nt, 1000 * dim + nt)
    for t in trains:
        _check_int8(ctx, q, t)
        _check_int8(ctx, t, q)


@pytest.mark.parametrize("dim", [32, 64])
def test_int8_kernels_on_corner_rows_over_several_chunks(ctx, dim):
    q, (t,) = _corner_case(dim, 129, 4500, dim)
    _check_int8(ctx, q, t)
    _check_int8(ctx, t, q)


# ------------------------------------------------------------------------------------------------
# b. pad rows against the worst real row
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nt", [1, 2, 31, 33, 45, 100, 257])
@pytest.mark.parametrize("dim", [32, 64, 128])
def test_l2_pad_rows_never_beat_the_worst_real_row(ctx, dim, nt):
    """The L2 twin of test_knn2_hamming2_matrix_core_kernel_pad_rows_never_beat_the_worst_real_row: EVERY real distance at the
    maximum dim * 255^2 for the row length, train counts that are no multiples of a tile -- the neighbours must be real rows 0 and
    1 (lowest indices on the tie), and every train's nearest query row 0, never one of the rows that pad a set to whole tiles."""
    worst = np.sqrt(np.float32(dim * 65025))
    second_i, second_d = (1, worst) if nt > 1 else (-1, FLT_MAX)
    for nq in (1, 70, 129):
        for qv, tv in ((0, 255), (255, 0)):
            q = np.full((nq, dim), qv, np.float32); t = np.full((nt, dim), tv, np.float32)
            qs, ts = ctx.descset_l2(_dense(q)), ctx.descset_l2(_host(t))
            assert qs.info()["exact_u8"] and ts.info()["exact_u8"]
            mi, md, ri, rd = _mutual(ctx, qs, ts, nq, nt, 2)
            for what, (i, d) in (("path 2", _knn(ctx, qs, ts, nq, 2)), ("path 1", _knn(ctx, qs, ts, nq, 1)), ("mutual", (mi, md))):
                assert (i[:, 0] == 0).all() and (i[:, 1] == second_i).all(), (what, nq, qv)
                assert (d[:, 0] == worst).all() and (d[:, 1] == second_d).all(), (what, nq, qv)
            assert (ri == 0).all() and (rd == worst).all(), (nq, qv)


# ------------------------------------------------------------------------------------------------
# c. the distance matrix, small and odd
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _matrix_case(dim):
    rng = np.random.default_rng(300 + dim)
    q = np.concatenate([corner_rows(dim), rng.integers(0, 256, (294, dim)).astype(np.float32)])
    t = np.concatenate([corner_rows(dim), rng.integers(0, 256, (507, dim)).astype(np.float32)])
    return _frozen(q, t, orc.l2_distance_matrix(q, t), mr.distance_matrix_int(q, t))


MATRIX_SHAPES = [(1, 1), (5, 3), (33, 129), (130, 257), (300, 513)]
# the parity tiling: a workgroup takes the 128 rows of ONE parity out of 256 -- an incomplete group (no odd row at all), exactly one
# workgroup per parity, more than one group; train counts inside the first shifted window, and past one / several 128-train blocks
PARITY_SHAPES = [(nq, nt) for nq in (1, 129, 300) for nt in (3, 257, 513)]


@pytest.mark.parametrize("layout,nq,nt", [(l, a, b) for l in ("vector", "scalar") for a, b in MATRIX_SHAPES]
                         + [("parity", a, b) for a, b in PARITY_SHAPES])
@pytest.mark.parametrize("dim", [32, 64, 100, 128])
def test_distance_matrix_small_and_odd(ctx, dim, layout, nq, nt):
    """distmat_i8_kernel<1>, <2>, <4> with fewer rows than one tile on either side, through the 16-byte stores, the scalar stores
    (odd row stride) and the row-parity tiling; nothing outside the matrix is written"""
    q, t, om, im = _matrix_case(dim)
    qs, ts = ctx.descset_l2(_dense(q[:nq])), ctx.descset_l2(_host(t[:nt]))
    assert qs.info()["exact_u8"] and ts.info()["exact_u8"]
    got, before, after = _distmat(ctx, qs, ts, nq, nt, layout)
    assert np.array_equal(_bits(got[:, :nt]), _bits(om[:nq, :nt])), "vs oracle"
    assert np.array_equal(_bits(got[:, :nt]), _bits(im[:nq, :nt])), "vs int64 reference"
    assert (got[:, nt:] == -1.0).all(), "columns past nt"
    assert (before == -1.0).all() and (after == -1.0).all(), "guard bands"


# ------------------------------------------------------------------------------------------------
# d. the exact fp32 kernel, unaligned and at odd row lengths
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _float_case(dim):
    rng = np.random.default_rng(7000 + dim)
    q = (rng.standard_normal((70, dim)) * 50).astype(np.float32)
    t = (rng.standard_normal((333, dim)) * 50).astype(np.float32)
    oi, od = orc.knn2_l2(q, t)
    ri, rd = orc.knn2_l2(t, q)
    d64, i64, gaps = mr.knn2_f64(q, t)
    return _frozen(q, t, oi, od, np.ascontiguousarray(ri[:, 0]), np.ascontiguousarray(rd[:, 0]), orc.l2_distance_matrix(q, t), d64, i64, gaps)


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("dim", [1, 3, 15, 16, 17, 40, 130, 256])
def test_exact_kernel_layouts_and_row_lengths(ctx, dim, layout):
    """knn2_exact_f32_kernel<4, ALIGNED, STORE_ALL> for both values of either flag: general float rows, dense / with row stride
    dim + 1 / starting at column 1 of a wider tensor (the last two take the unaligned loads except where dim + 1 is a multiple of 4
    on an aligned base), row lengths without a 16-wide block (1, 3, 15), without a tail (16, 256), with both, and above 128 (no int8
    copy at all).  Bit for bit against the oracle; and against float64 distances to the relative bound (dim/16 + 8) 2^-24, which
    follows from the kernel's summation order: one rounded subtraction and one rounded product per term, at most dim/16 + 4
    additions of positive terms on a term's way into the sum, one square root.  (The oracle itself stays within 3.1 * 2^-24 on
    these inputs.)  The indices must be the float64 nearest two wherever the float64 relative gap to the next row exceeds twice
    the bound, which may leave out at most 2 % of the rows."""
    import torch
    q, t, oi, od, ri, rd, om, d64, i64, gaps = _float_case(dim)
    nq, nt = q.shape[0], t.shape[0]
    mk = LAYOUTS[layout]
    qs, ts = ctx.descset_l2(mk(q)), ctx.descset_l2(mk(t))
    assert not qs.info()["exact_u8"] and not ts.info()["exact_u8"]
    gi, gd = _knn(ctx, qs, ts, nq, 0)
    _assert_knn((gi, gd), (oi, od), "knn2 vs oracle")
    out = torch.full((nq, nt), -1.0, dtype=torch.float32, device="cuda")
    ctx.l2_distance_matrix_dev(qs, ts, out)
    ctx.synchronize()
    gm = out.cpu().numpy()
    assert np.array_equal(_bits(gm), _bits(om)), "distance matrix vs oracle"
    mi, md, gri, grd = _mutual(ctx, qs, ts, nq, nt, 1)
    _assert_knn((mi, md), (oi, od), "mutual forward half vs oracle")
    _assert_knn((gri, grd), (ri, rd), "reverse best vs oracle, operands swapped")
    # independently of the oracle
    bound = (dim / 16 + 8) * 2.0 ** -24
    err = np.abs(gm.astype(np.float64) - d64)
    worst = float((err / d64).max())
    print(f"dim {dim} {layout}: largest relative error {worst / 2.0 ** -24:.2f} * 2^-24 (bound {bound / 2.0 ** -24:.2f})")
    assert (err <= bound * d64).all()
    assert (np.abs(gd.astype(np.float64) - np.take_along_axis(d64, i64, 1)) <= bound * np.take_along_axis(d64, i64, 1))[gi == i64].all()
    clear = (gaps > 2 * bound).all(1)
    left_out = 1.0 - clear.mean()
    print(f"dim {dim} {layout}: {left_out:.2%} of the rows left out of the index comparison (smallest gap {gaps.min():.2e})")
    assert left_out <= 0.02
    assert np.array_equal(gi[clear], i64[clear])


# ------------------------------------------------------------------------------------------------
# e. the re-score kernels on rows with a tail, unaligned, and with lists fed by several pairs
# ------------------------------------------------------------------------------------------------
RESCORE_DIM = 100                            # six 16-wide blocks and a tail of four
RESCORE_BASE = 97 * 210 * 210                # 4,277,700 >= 2^22


def _forward_collision():
    """test_knn2_l2_sqrt_collision_rescore at 100 values: the zero query row sees d^2 = base + 3 at train 0 and base + 2 at train 1,
    which share one float32 square root; the lower index must win although its integer distance is larger"""
    rng = np.random.default_rng(5)
    t = rng.integers(235, 256, (300, RESCORE_DIM)).astype(np.float32)
    t[0, :97] = 210; t[0, 97:] = (1, 1, 1)
    t[1, :97] = 210; t[1, 97:] = (1, 1, 0)
    q = np.zeros((130, RESCORE_DIM), np.float32)
    q[1:] = rng.integers(0, 3, (129, RESCORE_DIM))
    # the preconditions, on the references alone
    d2 = mr.d2_int(q[:1], t)[0]
    assert d2[0] == RESCORE_BASE + 3 and d2[1] == RESCORE_BASE + 2 and d2[1] >= 2 ** 22 and d2[2:].min() > d2[0]
    assert np.sqrt(np.float32(d2[0])) == np.sqrt(np.float32(d2[1]))
    for idx, dist in (orc.knn2_l2(q, t), mr.knn2_int(q, t)):
        assert idx[0].tolist() == [0, 1] and dist[0, 0] == dist[0, 1]
    return q, t


@pytest.mark.parametrize("layout", ["dense", "stride_dim_plus_1"])
def test_forward_rescore_on_rows_with_a_tail(ctx, layout):
    """knn2_exact_f32_kernel over the re-score list, rows of 96 + 4 values: aligned (dense, row stride 100) and unaligned (101)"""
    q, t = _forward_collision()
    (gi, _), _ = _check_int8(ctx, q, t, mkq=LAYOUTS[layout], mkt=LAYOUTS[layout], matrix=False)
    assert gi[0].tolist() == [0, 1]


@pytest.mark.parametrize("layout", ["dense", "stride_dim_plus_1"])
def test_reverse_rescore_on_rows_with_a_tail(ctx, layout):
    """the transpose: rev_rescore_l2_kernel, two QUERY rows sharing a float32 root for train row 0"""
    t, q = _forward_collision()
    _, (ri, _) = _check_int8(ctx, q, t, mkq=LAYOUTS[layout], mkt=LAYOUTS[layout], matrix=False)
    assert ri[0] == 0


def _reverse_collision_pair(nq, nt, i0, j, seed):
    """A pair whose MATCH LISTS show the reverse re-score.  Train j is the zero row; queries i0 and i0 + 1 are its nearest, at
    d^2 = base + 3 and base + 2 with one float32 root, so the cross check must keep i0 -> j and drop i0 + 1 -> j (integer order
    says the opposite).  Every other train is 0 on the first 97 values and 200..255 on the last three: at least 3 * 199^2 farther
    from both, 1.4 % in distance, so both rows pass a ratio test of 0.99 in the forward direction; every other query (235..255
    everywhere) is about equally far from all trains and passes none.  All d^2 are >= 2^22: every row of the pair is on the
    forward re-score list and every train on the reverse one."""
    rng = np.random.default_rng(seed)
    t = np.zeros((nt, RESCORE_DIM), np.float32)
    t[:, 97:] = rng.integers(200, 256, (nt, 3))
    t[j] = 0
    q = rng.integers(235, 256, (nq, RESCORE_DIM)).astype(np.float32)
    q[i0, :97] = 210; q[i0, 97:] = (1, 1, 1)
    q[i0 + 1, :97] = 210; q[i0 + 1, 97:] = (1, 1, 0)
    d2 = mr.d2_int(q, t)
    assert d2[i0, j] == RESCORE_BASE + 3 and d2[i0 + 1, j] == RESCORE_BASE + 2 and d2.min() >= 2 ** 22
    assert np.sqrt(np.float32(d2[i0, j])) == np.sqrt(np.float32(d2[i0 + 1, j]))
    assert mr.reverse_best_int(q, t)[0][j] == i0 and int(np.argmin(d2[:, j])) == i0 + 1
    return q, t


def _want_lists(q, t, ratio, knn):
    """plain and mutual match lists from a reference's kNN-2 (the ratio tail is the oracle's either way)"""
    plain = orc.ratio_filter(*knn(q, t), ratio=ratio)
    rev = knn(t, q)[0][:, 0]
    return plain, plain[rev[plain["trainIdx"]] == plain["queryIdx"]]


def test_rescore_lists_fed_by_several_pairs(ctx):
    """Three pairs in one call: two with a planted collision each, at different rows, and an ordinary one.  The forward list is per
    pair (list_off, row_count[pair]); the reverse list is shared by all pairs through one counter."""
    rng = np.random.default_rng(9)
    qa, ta = _reverse_collision_pair(130, 300, 0, 0, 1)
    qb, tb = _reverse_collision_pair(200, 150, 57, 101, 2)
    qc = rng.integers(0, 256, (180, RESCORE_DIM)).astype(np.float32)
    tc = np.clip(qc[rng.permutation(180)[:160]] + rng.integers(-1, 2, (160, RESCORE_DIM)), 0, 255).astype(np.float32)
    mats = [qa, ta, qb, tb, qc, tc]
    pairs = np.array([[0, 1], [2, 3], [4, 5]])
    want = [[_want_lists(mats[a], mats[b], 0.99, knn) for a, b in pairs] for knn in (orc.knn2_l2, mr.knn2_int)]
    for p, (i0, j) in enumerate(((0, 0), (57, 101))):
        plain, mutual = want[1][p]
        assert plain["queryIdx"].tolist() == [i0, i0 + 1] and plain["trainIdx"].tolist() == [j, j] and mutual["queryIdx"].tolist() == [i0]
    assert len(want[1][2][1]) > 100
    sets = ctx.descsets_host(mats)
    assert all(s.info()["exact_u8"] for s in sets)
    got_plain = ctx.match_pairs(sets, pairs, ratio=0.99)
    got_mutual = ctx.match_pairs(sets, pairs, ratio=0.99, cross_check=True)
    for name, w in zip(("oracle", "int64 reference"), want):
        for p in range(3):
            assert np.array_equal(got_plain[p], w[p][0]), (name, p)
            assert np.array_equal(got_mutual[p], w[p][1]), (name, p)


# ------------------------------------------------------------------------------------------------
# f. the byte upload at 32 and 64 values
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [32, 64])
def test_byte_upload_of_short_rows(ctx, dim):
    """prep_l2_u8_batched_kernel with 2 and 4 lanes per row: a ragged chain through descsets_host, one image with a single
    non-integer value (it goes the float way); the sets match like per-image sets and like the oracle, and the float rows
    re-created on the device are the caller's (the exact kernel on them gives the oracle's neighbours)"""
    rng = np.random.default_rng(dim)
    sizes = (333, 1, 70, 333, 129)
    scene = rng.integers(0, 256, (400, dim))          # every image: a sample of these rows, each value moved by at most one
    chain = [np.clip(scene[rng.permutation(400)[:r]] + rng.integers(-1, 2, (r, dim)), 0, 255).astype(np.float32) for r in sizes]
    chain[3][200, 5] += 0.25
    batch = ctx.descsets_host(chain)
    infos = [s.info() for s in batch]
    assert [i["exact_u8"] for i in infos] == [True, True, True, False, True] and [i["rows"] for i in infos] == list(sizes)
    single = [ctx.descset_l2(_host(c)) for c in chain]
    all_pairs = np.array([[0, 1], [1, 2], [2, 3], [3, 4], [4, 0], [0, 2]])
    int_pairs = np.array([[0, 1], [1, 2], [4, 0], [0, 2], [2, 0]])          # no float image among them: the int8 kernels
    for pairs in (all_pairs, int_pairs):
        got = ctx.match_pairs(batch, pairs); want = ctx.match_pairs(single, pairs)
        for (a, b), g, w in zip(pairs, got, want):
            assert np.array_equal(g, w) and np.array_equal(g, orc.match_features_l2(chain[a], chain[b])), (a, b)
        assert sum(len(g) for g in got) > 50
    for a, b in all_pairs:
        _assert_knn(_knn(ctx, batch[a], batch[b], sizes[a], 1), orc.knn2_l2(chain[a], chain[b]), f"exact kernel on batch-built sets {a} -> {b}")
    for a, b in int_pairs:
        got = _knn(ctx, batch[a], batch[b], sizes[a], 2)
        _assert_knn(got, orc.knn2_l2(chain[a], chain[b]), f"int8 kernel on batch-built sets {a} -> {b} vs oracle")
        _assert_knn(got, mr.knn2_int(chain[a], chain[b]), f"int8 kernel on batch-built sets {a} -> {b} vs int64 reference")
