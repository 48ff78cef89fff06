"""GPU: baseline JPEG decoding on the device (sfmhip_jpeg_decode / sfmhip_jpeg_decode_dev, sfm_opencv_amd/csrc/jpeg.hip).

The bar is the project's usual one for integer arithmetic: the bytes of the host decoder (sfm_jpeg.hpp) -- through the committed
fixtures also the bytes of an independent libjpeg build -- for every fixture and every choice of the entropy stage; the host's verdict
and, where it accepts, its bytes on damaged streams; then the resident image straight into the extractors, and the drivers' flag."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import jpeg_cases as jc
from sfm_opencv_amd import _lib, api

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST = os.path.join(ROOT, "sfm_opencv_amd", "host")
ENTROPY = (0, 1, 2)                 # automatic, host, device


def _dev(ctx, data, entropy):
    img, status = ctx.jpeg_decode_dev(data, entropy)
    ctx.synchronize()
    return img.cpu().numpy(), int(status.item())


# ------------------------------------------------------------------------------------------------ 1. the fixtures
@pytest.mark.parametrize("name", jc.ALL)
def test_every_fixture_decodes_to_the_committed_bytes(ctx, name):
    data, ref = jc.jpg_bytes(name), jc.golden(name)
    for entropy in ENTROPY:
        got = ctx.jpeg_decode(data, entropy)
        assert got.shape == ref.shape and got.dtype == np.uint8, (name, entropy, got.shape)
        assert np.array_equal(got, ref), (name, entropy, int((got != ref).sum()))
        got, status = _dev(ctx, np.frombuffer(data, np.uint8), entropy)
        assert status == 0 and got.shape == ref.shape and np.array_equal(got, ref), (name, entropy, status)


def test_row_stride_padding_is_left_alone_and_runs_repeat(ctx):
    import torch
    for name in ("d420_dri5_odd", "dgray_dri4", "c422_odd_q60"):
        data, ref = np.frombuffer(jc.jpg_bytes(name), np.uint8), jc.golden(name)
        rows, cols = ref.shape[:2]; row = ref[0].size
        for entropy in ENTROPY:
            for pad in (1, 13):
                buf = np.full((rows, row + pad), 0xA5, np.uint8)
                ctx._check(ctx.lib.sfmhip_jpeg_decode(ctx.h, data.ctypes.data, data.size, entropy, buf.ctypes.data, row + pad))
                assert np.array_equal(buf[:, :row].reshape(ref.shape), ref) and (buf[:, row:] == 0xA5).all(), (name, entropy, pad)
                d = torch.full((rows, row + pad), 0xA5, dtype=torch.uint8, device="cuda"); st = torch.full((1,), 7, dtype=torch.int32, device="cuda")
                ctx._check(ctx.lib.sfmhip_jpeg_decode_dev(ctx.h, data.ctypes.data, data.size, entropy, C.c_void_p(d.data_ptr()), row + pad, C.c_void_p(st.data_ptr())))
                ctx.synchronize()
                assert int(st.item()) == 0 and np.array_equal(d.cpu().numpy(), buf), (name, entropy, pad)
            a, b = ctx.jpeg_decode(data, entropy), ctx.jpeg_decode(data, entropy)
            assert a.tobytes() == b.tobytes() == ref.tobytes()


def test_argument_rules(ctx):
    data, ref = np.frombuffer(jc.jpg_bytes("c420_q75"), np.uint8), jc.golden("c420_q75")
    out = np.full(ref.shape, 0xA5, np.uint8)
    lib = ctx.lib
    for args in ((None, data.size, 0, out.ctypes.data, 240), (data.ctypes.data, data.size, 0, None, 240), (data.ctypes.data, data.size, 0, out.ctypes.data, 239),
                 (data.ctypes.data, data.size, 3, out.ctypes.data, 240), (data.ctypes.data, data.size, -1, out.ctypes.data, 240)):
        assert lib.sfmhip_jpeg_decode(ctx.h, *args) == _lib.E_ARG, args[1:]
        assert lib.sfmhip_last_error(ctx.h)
    assert lib.sfmhip_jpeg_decode_dev(ctx.h, data.ctypes.data, data.size, 0, out.ctypes.data, 240, None) == _lib.E_ARG
    assert (out == 0xA5).all()


def test_unsupported_and_damaged_headers_are_refused_with_the_output_left_alone(ctx):
    data = jc.jpg_bytes("c420_q75")
    for bad in (open(os.path.join(jc.JDIR, "progressive_unsupported.jpg"), "rb").read(), data[:200], b"\xff\xd8" + bytes(range(256)) * 4):
        for entropy in ENTROPY:
            with pytest.raises(api.SfmHipError):
                ctx.jpeg_decode(bad, entropy)
            with pytest.raises(api.SfmHipError):
                ctx.jpeg_decode_dev(bad, entropy)
            buf = np.frombuffer(bad, np.uint8); out = np.full(1 << 16, 0xA5, np.uint8)
            assert ctx.lib.sfmhip_jpeg_decode(ctx.h, buf.ctypes.data, buf.size, entropy, out.ctypes.data, 1 << 12) == _lib.E_ARG
            assert (out == 0xA5).all()


# ------------------------------------------------------------------------------------------------ 2. damaged streams: the host's verdict, the host's bytes
def _same_as_host(ctx, data, tmp_path, tag):
    """the host program's verdict on these bytes; where it accepts, its bytes for both entropy stages"""
    ref = jc.host_decode(data, tmp_path, tag)
    buf = np.frombuffer(data, np.uint8)
    for entropy in ENTROPY:
        if ref is None:
            with pytest.raises(api.SfmHipError):
                ctx.jpeg_decode(data, entropy)
            info = None
            try:
                info = api.jpeg_info(data)
            except api.SfmHipError:
                pass
            if info is not None:                # the headers are whole: the output of the host entry is left alone
                out = np.full((info[0], info[1] * info[2]), 0xA5, np.uint8)
                assert ctx.lib.sfmhip_jpeg_decode(ctx.h, buf.ctypes.data, buf.size, entropy, out.ctypes.data, info[1] * info[2]) == _lib.E_ARG
                assert (out == 0xA5).all(), (tag, entropy)
        else:
            got = ctx.jpeg_decode(data, entropy)
            assert got.shape == ref.shape and np.array_equal(got, ref), (tag, entropy, int((got != ref).sum()))
            got, status = _dev(ctx, data, entropy)
            assert status == 0 and np.array_equal(got, ref), (tag, entropy, status)
    return ref is not None


@pytest.mark.parametrize("name", ["c420_restart_q80", "d420_dri1"])
def test_damaged_streams_get_the_host_verdict_and_bytes(ctx, tmp_path, name):
    accepted = {}
    for label, data in jc.damaged_streams(name).items():
        accepted[label] = _same_as_host(ctx, data, tmp_path, label)
    # a marker short, the host cannot finish the scan; bytes after a planted EOI read as zeros, which the standard tables decode
    assert not accepted["rst_removed"] and not accepted["cut"] and accepted["eoi_planted"], accepted
    # the library is whole afterwards
    assert np.array_equal(ctx.jpeg_decode(jc.jpg_bytes(name), 2), jc.golden(name))


def test_a_corrupt_segment_sets_the_status_of_the_enqueue_only_entry(ctx, tmp_path):
    """where the host refuses the random segment, the device entropy stage says so in *d_status and nowhere else"""
    for name in ("c420_restart_q80", "d420_dri1"):
        data = jc.damaged_streams(name)["segment_random"]
        ref = jc.host_decode(data, tmp_path, name)
        _, status = _dev(ctx, data, 2)
        assert (status == 0) == (ref is not None), (name, status)
        assert 0 <= status < 16


def test_extreme_quantiser_matches_the_host(ctx, tmp_path):
    assert _same_as_host(ctx, jc.quantiser_ffff(jc.jpg_bytes("c444_q90")), tmp_path, "q16")


# ------------------------------------------------------------------------------------------------ 3. the resident image into the extractors
def test_resident_image_goes_straight_into_the_extractors(ctx):
    import torch
    data = jc.jpg_bytes("d420_dri5_odd")
    host_img = ctx.jpeg_decode(data)
    cap = 4096
    for entropy in (1, 2):
        d_img, status = ctx.jpeg_decode_dev(data, entropy)
        kp = torch.zeros((cap, 28), dtype=torch.uint8, device="cuda"); n = torch.zeros(1, dtype=torch.int32, device="cuda")
        desc = torch.zeros((cap, 128), dtype=torch.float32, device="cuda")
        ctx.sift_extract_dev(d_img, kp, desc, n)
        akp = torch.zeros((cap, 28), dtype=torch.uint8, device="cuda"); an = torch.zeros(1, dtype=torch.int32, device="cuda")
        adesc = torch.zeros((cap, 61), dtype=torch.uint8, device="cuda")
        ctx.akaze_extract_dev(d_img, akp, adesc, an)
        ctx.synchronize()
        assert int(status.item()) == 0
        k0, d0 = ctx.sift_extract(host_img)
        m = int(n.item())
        assert m == len(k0) and m > 10
        assert kp[:m].cpu().numpy().tobytes() == k0.tobytes() and desc[:m].cpu().numpy().tobytes() == d0.tobytes()
        k1, d1 = ctx.akaze_extract(host_img)
        m = int(an.item())
        assert m == len(k1) and m > 10
        assert akp[:m].cpu().numpy().tobytes() == k1.tobytes() and adesc[:m].cpu().numpy().tobytes() == d1.tobytes()


# ------------------------------------------------------------------------------------------------ 4. driver
def _texture(h, w, seed):
    """smooth random blobs on a gradient: plenty of DoG extrema at several scales (the recipe of tests/test_sift_gpu.py)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = 90 + 30 * np.sin(xx / 97.0) + 20 * np.cos(yy / 71.0)
    for _ in range(700):
        cx, cy = rng.uniform(0, w), rng.uniform(0, h)
        s = rng.uniform(2.0, 9.0); a = rng.uniform(-70, 70)
        img += a * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * s * s))
    return np.clip(img, 0, 255)


def test_nview_driver_decodes_on_the_device(ctx, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    subprocess.check_call(["make", "-C", HOST], stdout=subprocess.DEVNULL)
    exe = os.path.join(HOST, "NViewReconstruct")
    img = _texture(136, 176, 31)
    d = tmp_path / "imgs"; d.mkdir()
    (d / "K.txt").write_text("300 300 88 68\n")
    for i in range(3):
        g = np.roll(img, (3 * i, 5 * i), (0, 1))
        rgb = np.stack([g, g * 0.9, g * 0.8], 2).astype(np.uint8)
        # 11 x 9 MCUs: no markers, one MCU per interval (99: the automatic choice is the device stage), one MCU row per interval (9: the host stage)
        Image.fromarray(rgb).save(str(d / ("%02d.jpg" % i)), "JPEG", quality=90, subsampling=2, restart_marker_blocks=(0, 1, 11)[i])
    outs = {}
    for tag, extra in (("dev", ["--jpeg-device"]), ("host", [])):
        feat = tmp_path / (tag + ".feat")
        r = subprocess.run([exe, str(d), str(tmp_path), "--sift", "--sift-device"] + extra + ["--features-only", "--save-features=" + str(feat)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-400:]
        outs[tag] = (r.stdout, open(feat, "rb").read())
    assert outs["dev"][0].count("2D feature point detected.") == 3
    assert outs["dev"][1] == outs["host"][1] and outs["dev"][0] == outs["host"][0]
