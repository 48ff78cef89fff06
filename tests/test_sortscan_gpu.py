"""The stable radix sort and the exclusive scan of csrc/sortscan.hip by themselves, through sfmhip_debug_sort_pairs and
sfmhip_debug_scan_u32, against numpy in every bit.  The contract (csrc/sortscan.hpp): the sort orders by the low
8 * max(1, ceil(bits / 8)) bits of the keys, equal ones in their input order, and returns the keys whole; the prefix sums are modulo
2^32 and the 64-bit total is exact while every tile of 4096 counters and every group of 256 tile totals sums below 2^32.
The sizes sit around the 64-lane rounds, the 1024-element wave pieces and the 4096-element tiles of the kernels."""
import ctypes as C

import numpy as np
import pytest

from sfm_opencv_amd import _lib

pytestmark = pytest.mark.gpu

TILE = 4096
SORT_SIZES = [0, 1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 3 * TILE + 1]
SORT_BITS = [0, 1, 8, 9, 32, 33, 64]
SCAN_SIZES = [0, 1, 255, 256, 257, 4095, 4096, 4097, 256 * TILE, 256 * TILE + 1]


def sorted_width(bits):
    return 8 * max(1, -(-bits // 8))


def width_mask(bits):
    return np.uint64((1 << sorted_width(bits)) - 1)


def key_patterns(n, bits, rng):
    w = sorted_width(bits)
    i = np.arange(n, dtype=np.uint64)
    rnd = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    # a few distinct values inside the sorted width, random bits above it (none above 64)
    above = (rnd >> np.uint64(w)) << np.uint64(w) if w < 64 else np.zeros(n, np.uint64)
    return {
        "all equal": np.full(n, 0x0123456789abcdef, np.uint64),
        "two alternating": np.where(i % np.uint64(2) == 0, np.uint64(0xa5), np.uint64(0x5a)),
        "random 64-bit": rnd,
        "strictly descending": np.uint64(n) - i,
        "top byte only": (rng.integers(0, 256, n, dtype=np.uint64) << np.uint64(56)) | np.uint64(0x00c0ffee),
        "bits above the width": above | rng.integers(0, 5, n, dtype=np.uint64),
    }


def check_sort(ctx, keys, vals, bits, what):
    got_k, got_v = ctx.debug_sort_pairs(keys, vals, bits)
    perm = np.argsort(keys & width_mask(bits), kind="stable")
    assert np.array_equal(got_k, keys[perm]), what
    assert np.array_equal(got_v, (perm if vals is None else vals[perm]).astype(np.uint32)), what


@pytest.mark.parametrize("bits", SORT_BITS)
@pytest.mark.parametrize("n", SORT_SIZES)
def test_sort_is_stable_on_the_stated_width_and_returns_the_keys_whole(ctx, n, bits):
    rng = np.random.default_rng(1000 * n + bits)
    for name, keys in key_patterns(n, bits, rng).items():
        check_sort(ctx, keys, None, bits, (name, "identity values"))
        check_sort(ctx, keys, rng.integers(0, n // 2 + 1, n, dtype=np.uint32), bits, (name, "given values"))


def test_sort_histogram_scan_over_several_tiles(ctx):
    n = 17 * TILE + 5                                # 256 * 18 digit counters: the scan of the histogram takes two tiles
    rng = np.random.default_rng(17)
    keys = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    check_sort(ctx, keys, None, 64, "identity values")
    check_sort(ctx, keys & np.uint64(0xffff), rng.integers(0, 1 << 32, n, dtype=np.uint32), 16, "given values")


def test_sort_histogram_scan_over_more_than_256_tiles(ctx):
    n = 4097 * TILE + 3                              # 256 * 4098 digit counters are 257 scan tiles: the top kernel's second trip
    keys = np.random.default_rng(4097).integers(0, 1 << 16, n, dtype=np.uint64)
    check_sort(ctx, keys, None, 16, "16-bit keys")


def check_scan(ctx, counters):
    got, total = ctx.debug_scan_u32(counters)
    c = np.cumsum(counters, dtype=np.uint64)
    excl = np.concatenate([np.zeros(1, np.uint64), c[:-1]])[:counters.size]
    assert np.array_equal(got, (excl & np.uint64(0xffffffff)).astype(np.uint32))
    assert total == (int(c[-1]) if counters.size else 0)


@pytest.mark.parametrize("n", SCAN_SIZES)
def test_scan_matches_the_exclusive_cumsum(ctx, n):
    check_scan(ctx, np.random.default_rng(n).integers(0, 16, n, dtype=np.uint32))
    check_scan(ctx, np.zeros(n, np.uint32))


def test_scan_wraps_modulo_2_32_under_an_exact_total(ctx):
    n = 600 * TILE                                   # a tile sums to 12,288,000 and 256 tiles to 3,145,728,000, both below 2^32
    counters = np.full(n, 3000, np.uint32)
    assert int(counters.sum(dtype=np.uint64)) == 7_372_800_000 > 1 << 32
    check_scan(ctx, counters)


def test_argument_errors(ctx):
    lib = ctx.lib
    k = np.arange(8, dtype=np.uint64); v = np.arange(8, dtype=np.uint32); ko = np.empty(8, np.uint64); vo = np.empty(8, np.uint32)
    K, V, KO, VO = (a.ctypes.data for a in (k, v, ko, vo))
    assert lib.sfmhip_debug_sort_pairs(ctx.h, K, V, 8, 64, KO, VO) == 0
    assert lib.sfmhip_debug_sort_pairs(ctx.h, K, V, 8, 64, None, VO) == _lib.E_ARG
    assert lib.sfmhip_debug_sort_pairs(ctx.h, K, V, 8, 64, KO, None) == _lib.E_ARG
    assert lib.sfmhip_debug_sort_pairs(ctx.h, None, V, 8, 64, KO, VO) == _lib.E_ARG
    assert lib.sfmhip_debug_sort_pairs(ctx.h, K, V, 8, -1, KO, VO) == _lib.E_ARG
    assert lib.sfmhip_debug_sort_pairs(ctx.h, K, V, 8, 65, KO, VO) == _lib.E_ARG
    assert lib.sfmhip_debug_sort_pairs(ctx.h, K, V, 8, 64, K, VO) == _lib.E_ARG          # an output that is an input
    assert lib.sfmhip_debug_sort_pairs(ctx.h, K, V, 8, 64, KO, V) == _lib.E_ARG
    assert lib.sfmhip_debug_sort_pairs(ctx.h, K, V, 8, 64, KO, KO + 8) == _lib.E_ARG     # the two outputs overlap
    assert lib.sfmhip_debug_sort_pairs(None, K, V, 8, 64, KO, VO) == _lib.E_ARG
    total = C.c_uint64(0)
    assert lib.sfmhip_debug_scan_u32(ctx.h, V, 8, VO, C.byref(total)) == 0 and total.value == 28
    assert lib.sfmhip_debug_scan_u32(ctx.h, V, 8, VO, None) == 0                          # the total is optional
    assert lib.sfmhip_debug_scan_u32(ctx.h, V, 8, None, C.byref(total)) == _lib.E_ARG
    assert lib.sfmhip_debug_scan_u32(ctx.h, None, 8, VO, C.byref(total)) == _lib.E_ARG
    assert lib.sfmhip_debug_scan_u32(ctx.h, V, 8, V, C.byref(total)) == _lib.E_ARG
    assert lib.sfmhip_debug_scan_u32(ctx.h, V, 8, V + 16, C.byref(total)) == _lib.E_ARG
    assert lib.sfmhip_debug_scan_u32(None, V, 8, VO, C.byref(total)) == _lib.E_ARG
    assert np.array_equal(ko, k) and np.array_equal(vo, np.concatenate([[0], np.cumsum(v)[:-1]]))   # the refused calls wrote nothing
