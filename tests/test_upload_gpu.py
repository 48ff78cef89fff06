"""The pinned staging ring under every large host array (sfm_upload / sfm_upload_produced of csrc/context.hip) by itself, through
sfmhip_debug_upload_many: what arrives on the device against the source arrays, byte for byte.  The sizes sit on the ring's own edges
(the 256 KiB threshold of the parallel fill, the 16 MiB piece, the third piece that reuses buffer 0), the granules include one that
does not divide 16 MiB (61, the AKAZE row) and the largest legal one.  The statistics come from the fill the hook runs on the copy
threads, the expected piece count from the plan restated below.  tests/test_copy_pool_cpu.py holds the same arithmetic on the CPU."""
import ctypes as C

import numpy as np
import pytest

from sfm_opencv_amd import _lib

pytestmark = pytest.mark.gpu

Ki, Mi = 1 << 10, 1 << 20
STAGE = 16 * Mi
SIZES = [0, 1, 63, 64, 65, 256 * Ki - 1, 256 * Ki, 256 * Ki + 1, 16 * Mi - 1, 16 * Mi, 16 * Mi + 1, 32 * Mi, 32 * Mi + 1, 48 * Mi + 5]
GRANULES = [1, 61, 64, 128, 512, 16 * Mi]


def plan(nbytes, granule):
    """the (off, n) pieces of a transfer: pieces of the largest multiple of the granule that fits a 16 MiB buffer, the last one shorter"""
    piece = STAGE // granule * granule if 0 < granule <= STAGE else STAGE
    return [(off, min(piece, nbytes - off)) for off in range(0, nbytes, piece)]


@pytest.fixture(scope="module")
def noise():
    """random bytes, shared and never written: the sources are slices of it"""
    a = np.random.default_rng(20240611).integers(0, 256, 48 * Mi + 5 + 4096, dtype=np.uint8)
    a.setflags(write=False)
    return a


def check_stats(stats, sizes, granules):
    produced = [(b, g) for b, g in zip(sizes, granules) if g]
    plans = [plan(b, g) for b, g in produced]
    assert stats["violations"] == 0
    assert stats["bytes"] == sum(b for b, _ in produced)
    assert stats["pieces"] == sum(len(p) for p in plans)
    if any(n >= 256 * Ki for p in plans for _, n in p):
        assert 4 <= stats["nt"] <= 16
    else:
        assert stats["nt"] == (1 if any(len(p) for p in plans) else 0)


@pytest.mark.parametrize("granule", GRANULES)
def test_one_transfer_arrives_whole_at_every_size(ctx, noise, granule):
    for k, nbytes in enumerate(SIZES):
        src = noise[k:k + nbytes]
        (got,), stats = ctx.debug_upload_many([src], [granule])
        assert np.array_equal(got, src), (nbytes, granule)
        check_stats(stats, [nbytes], [granule])
        assert stats["pieces"] == len(plan(nbytes, granule)) and stats["bytes"] == nbytes


def test_one_transfer_through_the_plain_copy_at_every_size(ctx, noise):
    """granule 0: sfm_upload, whose fill is the library's own (no statistics)"""
    for k, nbytes in enumerate(SIZES):
        src = noise[100 + k:100 + k + nbytes]
        (got,), stats = ctx.debug_upload_many([src], [0])
        assert np.array_equal(got, src), nbytes
        assert stats == dict(pieces=0, bytes=0, violations=0, nt=0)


BACK_TO_BACK = [20 * Mi, 3, 16 * Mi, 300 * Ki, 33 * Mi]


def _back_to_back(ctx, noise, granules, shift):
    srcs, at = [], shift
    for b in BACK_TO_BACK:          # other bytes in every call: what an earlier call left in a buffer or an area cannot pass for them
        srcs.append(noise[at:at + b]); at += 4099
    got, stats = ctx.debug_upload_many(srcs, granules)
    for i, (g, s) in enumerate(zip(got, srcs)):
        assert np.array_equal(g, s), (i, granules)
    check_stats(stats, BACK_TO_BACK, granules)


def test_back_to_back_transfers_reuse_the_buffers_in_order(ctx, noise):
    """Five transfers with no host wait between them: 2 + 1 + 1 + 1 + 3 pieces on two buffers, so a buffer is refilled inside a
    transfer and across transfers (and across calls: the ring's state carries over), the caller-only fill of 3 bytes next to the
    parallel one of 300 KiB, produced transfers next to plain ones."""
    import torch
    a, b = [61, 0, 128, 0, 61], [0, 61, 0, 128, 0]
    _back_to_back(ctx, noise, a, 0)
    _back_to_back(ctx, noise, b, 1000)
    home = ctx.torch_stream.cuda_stream if ctx.torch_stream is not None else None
    other = torch.cuda.Stream(device=ctx.device)
    try:
        ctx.set_stream(other.cuda_stream)
        _back_to_back(ctx, noise, a, 2000)
    finally:
        ctx.set_stream(home)
    _back_to_back(ctx, noise, b, 3000)


def _raw(ctx, srcs, granules, outs, stats, n=None, null=()):
    k = len(srcs)
    ptrs = (C.c_void_p * k)(*[s.ctypes.data for s in srcs]); optrs = (C.c_void_p * k)(*[o if isinstance(o, int) else o.ctypes.data for o in outs])
    nb = (C.c_size_t * k)(*[s.size for s in srcs]); gr = (C.c_size_t * k)(*granules)
    args = dict(src=ptrs, bytes=nb, granule=gr, out=optrs, stats=None if stats is None else stats.ctypes.data)
    for name in null:
        args[name] = None
    return ctx.lib.sfmhip_debug_upload_many(ctx.h, args["src"], args["bytes"], args["granule"], k if n is None else n, args["out"], args["stats"])


def test_a_failed_allocation_is_an_error_with_nothing_written_and_the_next_call_works(ctx, noise):
    sizes = [300 * Ki, 17 * Mi]
    srcs = [noise[7:7 + b] for b in sizes]
    outs = [np.full(b, 0xEE, np.uint8) for b in sizes]
    stats = np.full(4, 77, np.uint64)
    assert ctx.lib.sfmhip_debug_fail_allocations(ctx.h, 1) == 0
    try:
        assert _raw(ctx, srcs, [61, 128], outs, stats) == _lib.E_HIP
    finally:
        assert ctx.lib.sfmhip_debug_fail_allocations(ctx.h, 0) == 0
    assert all((o == 0xEE).all() for o in outs) and (stats == 77).all()
    assert _raw(ctx, srcs, [61, 128], outs, stats) == 0
    assert all(np.array_equal(o, s) for o, s in zip(outs, srcs))
    check_stats(dict(zip(("pieces", "bytes", "violations", "nt"), (int(v) for v in stats))), sizes, [61, 128])


def test_argument_errors(ctx, noise):
    srcs = [noise[:1000].copy(), noise[1000:3000].copy()]
    outs = [np.full(1000, 0xEE, np.uint8), np.full(2000, 0xEE, np.uint8)]
    stats = np.full(4, 77, np.uint64)
    E = _lib.E_ARG
    empty = np.full(4, 5, np.uint64)
    assert _raw(ctx, srcs, [61, 0], outs, empty, n=0) == 0 and (empty == 0).all()              # nothing to do: no fill ran
    assert ctx.lib.sfmhip_debug_upload_many(ctx.h, None, None, None, 0, None, None) == 0
    assert ctx.lib.sfmhip_debug_upload_many(None, None, None, None, 0, None, None) == E
    assert _raw(ctx, srcs, [61, 0], outs, stats, n=-1) == E
    for name in ("src", "bytes", "granule", "out"):
        assert _raw(ctx, srcs, [61, 0], outs, stats, null=(name,)) == E, name
    assert _raw(ctx, srcs, [61, 0], [outs[0], 0], stats) == E                                  # a null output of a non-empty source
    assert _raw(ctx, srcs, [61, 0], [outs[0], srcs[1]], stats) == E                            # an output that is a source
    assert _raw(ctx, srcs, [61, 0], [outs[0], srcs[0][500:]], stats) == E                      # ... or lies inside another one
    assert _raw(ctx, srcs, [61, 0], [outs[1][:1000], outs[1][999:]], stats) == E               # two outputs share a byte
    assert _raw(ctx, srcs, [61, 0], outs, outs[1][8:40].view(np.uint64)) == E                  # the statistics inside an output
    # a granule above the buffer size cannot be kept: refused by sfm_upload_produced, after the first transfer was queued
    assert _raw(ctx, srcs, [61, STAGE + 1], outs, stats) == E
    assert _raw(ctx, [srcs[0], srcs[1][:0]], [61, STAGE + 1], [outs[0], outs[1][:0]], stats) == E   # ... whatever the byte count
    assert all((o == 0xEE).all() for o in outs) and (stats == 77).all()                        # the refused calls wrote nothing
    assert _raw(ctx, srcs, [61, STAGE], outs, None) == 0                                       # the statistics are optional
    assert all(np.array_equal(o, s) for o, s in zip(outs, srcs))
