"""The packed 32-bit keys of the int8 L2 kernels (csrc/match.hip: knn2_i8_body, its column pass, merge_kernel's re-score threshold),
restated with exact Python integers.  The constants are read out of match.hip, so a changed margin is seen here.  No GPU.

Forward key of (query a, train b), biased int8 rows of DP bytes, tile = index of the 32-row tile inside the chunk:
    ((|b|^2 + 2 sum b) << 7) + tile + ((sum ~a b) << 8)  =  (|b|^2 - 2 a.b) * 128 + tile
pad train rows are zero rows whose train-side term is PAD_NORM.  Column key of the same pair, r = query row inside the workgroup:
    ((sum ~a b) << 8) + (|a|^2 << 7) + r  =  (|a|^2 - 2 a.b - 2 sum b) * 128 + r
pad query rows are zero rows whose query-side term is QV_PAD; a column minimum counts only below QV_REAL_MAX."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, "sfm_opencv_amd", "csrc", "match.hip")).read()
ROW_BYTES = (32, 64, 128)
CORNERS = (-128, -1, 0, 127)          # values 0, 127, 128, 255 after the bias


def _define(name):
    m = re.search(r"^#define %s[ \t]+(.+?)[ \t]*(?://.*)?$" % name, SRC, re.M)
    assert m, name
    expr = m.group(1)
    assert re.fullmatch(r"[0-9 ()<+\-]+", expr), (name, expr)          # integer literals, shifts, sums
    return int(eval(expr, {"__builtins__": {}}))


PAD_NORM = _define("PAD_NORM")
QV_PAD = _define("QV_PAD")
QV_REAL_MAX = _define("QV_REAL_MAX")
RESCORE_D2 = _define("RESCORE_D2")


def _tile_field():
    """(bits of the tile field, the mask the merge decodes it with), from the statements that pack and unpack the keys"""
    pack = re.search(r"<< (\d+)\) \+ \(blk \* TILES \+ tile\)", SRC)
    unpack = re.findall(r"\(m([12]) >> (\d+)\) \+ qn\) << 32\) \| \(unsigned int\)\(t_begin \+ \(m\1 & (\d+)\) \* 32", SRC)
    col = re.search(r"\(m >> (\d+)\) \+ TN\[j\]", SRC)
    colrow = re.search(r"qb \* 128 \+ \(m & (\d+)\)", SRC)
    assert pack and len(unpack) == 2 and col and colrow
    bits = int(pack.group(1))
    for _, shift, mask in unpack:
        assert int(shift) == bits and int(mask) == (1 << bits) - 1
    assert int(col.group(1)) == bits and int(colrow.group(1)) == (1 << bits) - 1
    assert re.search(r"\(unsigned\)QN\[qrow\] << %d\)" % bits, SRC)
    return bits, (1 << bits) - 1


TILE_BITS, TILE_MASK = _tile_field()


def fwd_key(a, b, dp, tile, tn=None):
    """uniform rows: every byte of the query a, of the train b; tn: the train-side term (PAD_NORM for a pad row)"""
    if tn is None:
        tn = dp * (b * b + 2 * b)
    s = dp * (~a) * b
    return (tn << TILE_BITS) + tile + (s << (TILE_BITS + 1))


def col_key(a, b, dp, r, qv=None):
    if qv is None:
        qv = ((dp * a * a) << TILE_BITS) + r
    s = dp * (~a) * b
    return (s << (TILE_BITS + 1)) + qv


def test_constants_are_the_ones_the_margins_were_worked_out_for():
    assert (PAD_NORM, RESCORE_D2, TILE_BITS) == ((1 << 23) - 1, 1 << 22, 7)
    assert QV_PAD == 3 << 29 and QV_REAL_MAX == (1 << 30) + (1 << 28)


def test_keys_decode_to_the_squared_distance():
    for dp in ROW_BYTES:
        for a in CORNERS:
            for b in CORNERS:
                d2 = dp * (a - b) ** 2
                for tile in (0, TILE_MASK):
                    k = fwd_key(a, b, dp, tile)
                    assert -(1 << 31) <= k < (1 << 31)
                    assert (k >> TILE_BITS) + dp * a * a == d2 and k & TILE_MASK == tile          # merge: (m >> 7) + qn, m & 127
                    c = col_key(a, b, dp, tile)
                    assert -(1 << 31) <= c < (1 << 31)
                    assert (c >> TILE_BITS) + dp * (b * b + 2 * b) == d2 and c & TILE_MASK == tile      # col_flush: (m >> 7) + TN[j]


def test_every_real_forward_key_is_below_every_pad_train_key():
    """per coordinate the key is linear in b^2 - 2ab, so rows of one repeated value reach the extremes: checked over ALL value pairs"""
    v = np.arange(-128, 128, dtype=np.int64)
    per = v[None, :] ** 2 - 2 * v[:, None] * v[None, :]            # [a, b]
    for dp in ROW_BYTES:
        hi = max(fwd_key(a, b, dp, TILE_MASK) for a in CORNERS for b in CORNERS)
        lo = min(fwd_key(a, b, dp, 0) for a in CORNERS for b in CORNERS)
        assert hi == int(per.max()) * dp * 128 + TILE_MASK and lo == int(per.min()) * dp * 128          # the corners ARE the extremes
        pad_lo = min(fwd_key(a, 0, dp, 0, tn=PAD_NORM) for a in CORNERS)
        pad_hi = max(fwd_key(a, 0, dp, TILE_MASK, tn=PAD_NORM) for a in CORNERS)
        assert pad_lo == PAD_NORM << TILE_BITS                         # a pad row's bytes are zero: the query does not move its key
        assert -(1 << 31) <= lo and hi < pad_lo and pad_hi < (1 << 31) - 1          # ... and stays below the INT_MAX of an empty slot
    assert fwd_key(127, -128, 128, TILE_MASK) == 801112191


def test_column_keys_real_below_qv_real_max_pad_queries_above():
    v = np.arange(-128, 128, dtype=np.int64)
    per = v[:, None] ** 2 - 2 * v[:, None] * v[None, :] - 2 * v[None, :]          # |a|^2 - 2ab - 2b at [a, b]
    for dp in ROW_BYTES:
        hi = max(col_key(a, b, dp, TILE_MASK) for a in CORNERS for b in CORNERS)
        lo = min(col_key(a, b, dp, 0) for a in CORNERS for b in CORNERS)
        assert hi == int(per.max()) * dp * 128 + TILE_MASK and lo == int(per.min()) * dp * 128
        assert -(1 << 31) <= lo and hi < QV_REAL_MAX
        # pad query rows are zero rows (a = 0 after the bias, ~a = -1 in every byte) with QV_PAD as their term; any train row
        pad = [col_key(0, b, dp, 0, qv=QV_PAD) for b in (-128, 0, 127)]
        assert min(pad) >= QV_REAL_MAX and max(pad) < (1 << 31)
    assert col_key(127, -128, 128, TILE_MASK) == 801128575
    assert min(col_key(0, b, 128, 0, qv=QV_PAD) for b in (-128, 127)) == 1606451200
    assert max(col_key(0, b, 128, 0, qv=QV_PAD) for b in (-128, 127)) <= 1614807167


def test_float_sqrt_is_strictly_increasing_below_the_rescore_threshold_and_not_above():
    assert 128 * 255 * 255 < (1 << 24)                                 # every d^2 is a float32 integer
    s = np.sqrt(np.arange(RESCORE_D2 + 1, dtype=np.float32))
    assert s.dtype == np.float32 and (np.diff(s) > 0).all()
    # ... and the re-score is needed, not merely harmless: two neighbours above the threshold share a root
    hi = np.sqrt(np.arange(RESCORE_D2, RESCORE_D2 + 4096, dtype=np.float32))
    ties = np.nonzero(np.diff(hi) == 0)[0]
    assert len(ties) > 0 and RESCORE_D2 + int(ties[0]) == (1 << 22) + 2896


def test_a_chunk_needs_no_more_tile_indices_than_the_field_holds():
    m = re.search(r"\{ 128, KNN_STAGE_ROWS, (\d+), false, true, 0 \},\s*// KNN_I8", SRC)
    assert m, "the KNN_I8 row of KNN_PATHS"
    max_chunk_rows = int(m.group(1))
    assert max_chunk_rows % 32 == 0 and max_chunk_rows // 32 <= TILE_MASK + 1
