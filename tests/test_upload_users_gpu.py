"""The users of the pinned staging ring (csrc/context.hip) across the ring's own edges, every row checked: descriptor batches whose
byte rows (sfm_upload_produced under stage_host_images of match.hip: float -> byte conversion, Hamming rows) or float rows (sfm_upload)
cross the 16 MiB and 32 MiB piece boundaries, with images of no rows, of one row, one large image that holds a piece boundary, and
row strides above the row length.  The sizes are the smallest that cross the boundaries: the constants are the ring's.

The check needs neither upload path nor a tolerance.  Images come in pairs; the second of a pair holds the rows of the first in a
known random order, and the rows of an image are distinct (asserted on the CPU).  So kNN-2 of the first against the second must
name, for EVERY row, the row the permutation put it at, at distance exactly 0, with the second neighbour farther away.  One wrong,
missing or misplaced row anywhere in either image breaks that.  tests/test_upload_gpu.py tests the ring by itself."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

Mi = 1 << 20
STAGE = 16 * Mi
N_PAIRS = 36
BIG = 40_000
# pairs (both images) without rows: at the start, two pairs = four images in a row in the middle, at the end; pairs of one-row images
NO_ROWS = (0, 5, 6, N_PAIRS - 1)
ONE_ROW = (1, 9, N_PAIRS - 2)
BIG_AT = 14


def pair_rows(w, total_bytes, rng):
    """rows per image of the N_PAIRS pairs (uneven): in all at least total_bytes / w rows, and the first image of pair BIG_AT, of about
    BIG rows, holds the first piece boundary of the transfer in its middle"""
    per_piece = STAGE // w                                   # rows of a piece: the piece is the largest multiple of w in 16 MiB
    need = -(-total_bytes // w) + 1
    rows = np.zeros(N_PAIRS, np.int64)
    rows[list(ONE_ROW)] = 1
    plain = [k for k in range(N_PAIRS) if k not in NO_ROWS + ONE_ROW and k != BIG_AT]
    before = [k for k in plain if k < BIG_AT]; behind = [k for k in plain if k > BIG_AT]
    ones_before = sum(1 for k in ONE_ROW if k < BIG_AT)

    def spread(total, n):                                    # n uneven counts >= 2 that sum to total
        wgt = rng.random(n) ** 3 + 0.02
        c = 2 + np.floor(wgt / wgt.sum() * (total - 2 * n)).astype(np.int64)
        c[np.argmax(c)] += total - c.sum()
        assert c.min() >= 2 and c.sum() == total
        return c

    front = (per_piece - BIG // 2) & ~1                      # rows in front of the big image: the boundary falls into its middle
    rows[before] = spread(front // 2 - ones_before, len(before))
    rows[BIG_AT] = BIG
    rest = need - 2 * int(rows.sum())
    rows[behind] = spread(max(-(-rest // 2), 40 * len(behind)), len(behind))
    return rows


def build_pairs(w, total_bytes, dtype, seed, pad=19):
    """(images, permutations): 2 * N_PAIRS images of w columns; every third image is a view into rows of w + pad elements whose
    gap holds 165 (0xA5), which must never arrive"""
    rng = np.random.default_rng(seed)
    rows = pair_rows(w, total_bytes, rng)
    imgs, perms = [], []
    for k, n in enumerate(rows):
        n = int(n)
        a = rng.integers(0, 256, (n, w), dtype=np.uint8)
        if w >= 3:                                           # distinct rows by construction: the row number in the first three columns
            a[:, 0] = np.arange(n) & 255; a[:, 1] = (np.arange(n) >> 8) & 255; a[:, 2] = np.arange(n) >> 16
        perm = rng.permutation(n)
        for img in (a, a[perm]):
            img = img.astype(dtype)
            if len(imgs) % 3 == 2:
                wide = np.full((max(n, 1), w + pad), 165, dtype)
                wide[:n, :w] = img
                img = wide[:n, :w]
                assert img.strides[0] == (w + pad) * img.itemsize
            imgs.append(img)
        perms.append(perm)
    return imgs, perms


def assert_layout(imgs, w, crossings):
    """what the case is there for, on the CPU: the byte rows cross `crossings` piece boundaries, one of them inside the big image"""
    piece = STAGE // w * w
    first = np.concatenate([[0], np.cumsum([m.shape[0] for m in imgs])]) * w
    assert crossings * STAGE < first[-1] and crossings * piece < first[-1] <= (crossings + 1) * piece
    lo, hi = first[2 * BIG_AT], first[2 * BIG_AT + 1]
    assert hi - lo >= BIG * w and lo < piece < hi and (piece - lo) // w >= BIG // 4 and (hi - piece) // w >= BIG // 4
    n = [m.shape[0] for m in imgs]
    assert n[0] == n[1] == 0 and n[-1] == n[-2] == 0 and n[10:14] == [0, 0, 0, 0] and n.count(1) == 2 * len(ONE_ROW)
    assert len(set(n)) > N_PAIRS // 2                                           # uneven
    for m in imgs:                                                              # distinct rows within an image
        r = m[:, :3].astype(np.int64)
        assert len(np.unique(r[:, 0] | (r[:, 1] << 8) | (r[:, 2] << 16))) == len(r)


def knn(ctx, q, t, n):
    import torch
    idx = torch.empty((n, 2), dtype=torch.int32, device="cuda"); dist = torch.empty((n, 2), dtype=torch.float32, device="cuda")
    ctx.knn2_dev(q, t, idx, dist)
    ctx.synchronize()
    return idx.cpu().numpy(), dist.cpu().numpy()


def check_every_row(ctx, sets, imgs, perms):
    assert len(sets) == len(imgs) == 2 * len(perms)
    for k, perm in enumerate(perms):
        n = len(perm)
        q, t = sets[2 * k], sets[2 * k + 1]
        assert q.rows == t.rows == n == imgs[2 * k].shape[0]
        if n == 0:
            assert q.info()["rows"] == 0 and t.info()["rows"] == 0
            continue
        assert np.array_equal(np.asarray(imgs[2 * k])[perm], np.asarray(imgs[2 * k + 1]))     # the pair is what this check assumes
        idx, dist = knn(ctx, q, t, n)
        at = np.empty(n, np.int32); at[perm] = np.arange(n, dtype=np.int32)      # row perm[r] of the first image is row r of the second
        bad = np.flatnonzero((idx[:, 0] != at) | (dist[:, 0] != 0) | ~(dist[:, 1] > 0))
        assert bad.size == 0, (k, n, bad[:8], idx[bad[:8]], dist[bad[:8]])


def close_all(sets):
    for s in sets:
        s.close()


@pytest.mark.parametrize("dim,total,crossings", [(128, 36 * Mi + Mi // 2, 2), (64, 16 * Mi + Mi // 4, 1), (32, 16 * Mi + Mi // 4, 1)])
def test_l2_byte_rows_arrive_in_every_row(ctx, dim, total, crossings):
    imgs, perms = build_pairs(dim, total, np.float32, 1000 + dim)
    assert_layout(imgs, dim, crossings)
    sets = ctx.descsets_host(imgs)
    try:
        assert all(s.info()["exact_u8"] for s in (sets[2], sets[2 * BIG_AT], sets[2 * BIG_AT + 1], sets[-3]))      # the byte path was taken
        check_every_row(ctx, sets, imgs, perms)
    finally:
        close_all(sets)


@pytest.mark.parametrize("nbytes,total,crossings", [(61, 32 * Mi + Mi // 4, 2), (64, 16 * Mi + Mi // 4, 1)])
def test_hamming_rows_arrive_in_every_row(ctx, nbytes, total, crossings):
    """61-byte rows: the piece is 275,036 rows = 16,777,196 bytes, not 16 MiB"""
    imgs, perms = build_pairs(nbytes, total, np.uint8, 2000 + nbytes)
    assert_layout(imgs, nbytes, crossings)
    sets = ctx.descsets_host(imgs)
    try:
        check_every_row(ctx, sets, imgs, perms)
    finally:
        close_all(sets)


@pytest.mark.parametrize("rows,dim", [(41_000, 128), (2_049, 33)])
def test_float_rows_arrive_in_every_row(ctx, rows, dim):
    """Rows that cross as floats through sfm_upload: one value that is no integer takes a 128-column image off the byte path (two
    images of 20 MiB: two pieces each, the second image starts on the buffer the first one ended on); 33 columns never take it, and
    2,049 rows of 132 bytes are just above the 256 KiB of the parallel fill, an odd row width through its 64-byte granule."""
    rng = np.random.default_rng(rows + dim)
    a = rng.integers(0, 256, (rows, dim), dtype=np.uint8).astype(np.float32)
    a[:, 0] = np.arange(rows) & 255; a[:, 1] = np.arange(rows) >> 8               # distinct rows
    a[rows // 2, dim - 1] = 0.5
    perm = rng.permutation(rows)
    imgs = [a, np.ascontiguousarray(a[perm])]
    assert len(np.unique(a[:, 0].astype(np.int64) + 256 * a[:, 1].astype(np.int64))) == rows
    assert (a.nbytes > STAGE) == (dim == 128) and a.nbytes >= 256 << 10
    sets = ctx.descsets_host(imgs)
    try:
        assert not sets[0].info()["exact_u8"] and not sets[1].info()["exact_u8"]          # the float way
        check_every_row(ctx, sets, imgs, [perm])
    finally:
        close_all(sets)
