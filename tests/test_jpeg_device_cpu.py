"""CPU: what the device JPEG decoder (sfm_opencv_amd/csrc/jpeg.hip) has on the host side -- sfmhip_jpeg_info, the argument rules
without a device, the three kernels' resources in the code object, the drivers' --jpeg-device flag, and the refactored
sfm_jpeg.hpp (parse_headers + decode_scan with a coefficient sink) under AddressSanitizer + UBSan in a stand-alone program."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import jpeg_cases as jc
from sfm_opencv_amd import _lib, api
from test_codeobj_cpu import LIB, READELF, _kernel_table

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST = os.path.join(ROOT, "sfm_opencv_amd", "host")

# (rows, cols, channels, restart interval, intervals) of the nine fixtures of tests/golden/jpeg, restated from their save options:
# c420_restart_q80 is 70 x 90 in 16 x 16 MCUs (6 x 5 = 30) with 3 MCUs per interval; c422_restart_rows_opt is 40 x 100 in 16 x 8 MCUs
# (7 per row, 5 rows) with one row per interval
OLD_INFO = {
    "c444_q90": (53, 75, 3, 0, 1), "c422_q85": (64, 96, 3, 0, 1), "c422_odd_q60": (45, 67, 3, 0, 1), "c420_q75": (48, 80, 3, 0, 1),
    "c420_odd_q95": (51, 77, 3, 0, 1), "c420_restart_q80": (70, 90, 3, 3, 10), "c422_restart_rows_opt": (40, 100, 3, 7, 5),
    "gray_q80": (37, 59, 1, 0, 1), "c420_q20": (56, 72, 3, 0, 1),
}


def _index():
    rows = {}
    for ln in open(os.path.join(jc.DDIR, "index.txt")):
        if ln.strip() and not ln.startswith("#"):
            f = ln.split()
            rows[f[0]] = tuple(int(v) for v in f[1:])
    return rows


def test_jpeg_info_reads_the_headers_of_every_fixture():
    index = _index()
    assert sorted(index) == sorted(jc.ALL)
    for name in jc.ALL:
        got = api.jpeg_info(jc.jpg_bytes(name))
        assert got == index[name], (name, got)
        assert got[:2] == jc.golden(name).shape[:2] and got[2] == (1 if jc.golden(name).ndim == 2 else 3), name
        if name in OLD_INFO:
            assert got == OLD_INFO[name], (name, got)
    # the restart cases are what their names say
    assert index["d420_dri1"][3:] == (1, 88) and index["d420_dri5_odd"][3:] == (5, 24) and index["d420_one_interval"][3:] == (100, 1)
    assert index["d420_tiny"][3:] == (0, 1) and index["d420_q100"][3:] == (4, 3)
    # a uint8 array is as good as bytes
    assert api.jpeg_info(np.frombuffer(jc.jpg_bytes("gray_q80"), np.uint8)) == OLD_INFO["gray_q80"]


def test_jpeg_info_refuses_what_the_decoder_refuses():
    data = jc.jpg_bytes("c420_q75")
    for bad in (open(os.path.join(jc.JDIR, "progressive_unsupported.jpg"), "rb").read(), data[:200], b"\xff\xd8" + bytes(range(256)) * 4,
                data[:3], b""):
        with pytest.raises(api.SfmHipError):
            api.jpeg_info(bad)
    lib = _lib.load()
    buf = np.frombuffer(data, np.uint8)
    v = [C.c_int(0) for _ in range(5)]
    assert lib.sfmhip_jpeg_info(buf.ctypes.data, buf.size, C.byref(v[0]), C.byref(v[1]), C.byref(v[2]), C.byref(v[3]), None) == _lib.E_ARG
    assert lib.sfmhip_jpeg_info(None, buf.size, *[C.byref(x) for x in v]) == _lib.E_ARG
    # a file cut inside its scan still has its headers
    s = jc.scan_start(data)
    assert api.jpeg_info(data[:s + 10]) == OLD_INFO["c420_q75"]


def test_decoding_needs_a_context():
    lib = _lib.load()
    buf = np.frombuffer(jc.jpg_bytes("c420_q75"), np.uint8)
    out = np.full((48, 80, 3), 0xA5, np.uint8)
    assert lib.sfmhip_jpeg_decode(None, buf.ctypes.data, buf.size, 0, out.ctypes.data, 240) == _lib.E_ARG
    assert lib.sfmhip_jpeg_decode_dev(None, buf.ctypes.data, buf.size, 0, out.ctypes.data, 240, out.ctypes.data) == _lib.E_ARG
    assert (out == 0xA5).all()
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(api.SfmHipError):
            api.Context(0)


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not found")
def test_jpeg_kernels_have_no_scratch_and_the_lds_the_source_derives(tmp_path):
    assert os.path.exists(LIB), "build libsfmhip.so first (__graft_entry__.build)"
    t = _kernel_table(tmp_path)
    src = open(os.path.join(ROOT, "sfm_opencv_amd", "csrc", "jpeg.hip")).read()

    def const(name):
        m = re.search(r"constexpr int [^;]*\b%s = ([^,;]+)[,;]" % name, src)
        assert m, name
        return m.group(1).strip()

    # the Huffman kernel's LDS is what the source says: the tables decode_symbol reads (look, mincode, maxcode, valptr, vals), eight of
    # them, and the 64 bytes of the zigzag order
    assert const("JPEG_HUFF_TABLE_BYTES") == "512 * 2 + (17 + 18 + 17) * 4 + 256" and const("JPEG_HUFF_TABLES") == "8"
    assert const("JPEG_HUFF_LDS_BYTES") == "JPEG_HUFF_TABLES * JPEG_HUFF_TABLE_BYTES + 64"
    huff_lds = 8 * (512 * 2 + (17 + 18 + 17) * 4 + 256) + 64
    want_lds = {"jpeg_huffman_kernel": huff_lds,
                "jpeg_idct_kernel": int(const("JPEG_IDCT_BLOCKS")) * int(const("JPEG_WS_BLOCK")) * 4,
                "jpeg_colour_kernel": 4 * 256 * 4}
    for kernel, lds in want_lds.items():
        ks = [(k, v) for k, v in t.items() if kernel in k]
        assert len(ks) == 1, (kernel, [k for k, _ in ks])
        name, k = ks[0]
        assert k["scratch"] == 0 and (k["spill"] or 0) == 0, (name, k)
        assert k["lds"] == lds, (name, k, lds)


def test_drivers_list_the_flag_and_refuse_it_without_a_device_extractor(tmp_path):
    subprocess.check_call(["make", "-C", HOST], stdout=subprocess.DEVNULL)
    for exe in ("NViewReconstruct", "TwoViewReconstruct"):
        path = os.path.join(HOST, exe)
        usage = subprocess.run([path], capture_output=True, text=True).stdout
        assert "[--jpeg-device]" in usage and "[--sift-device]" in usage and "[--akaze-device]" in usage, exe
        for extra in ([], ["--sift"], ["--akaze"], ["--sift", "--akaze-device"], ["--akaze", "--sift-device"]):
            r = subprocess.run([path, str(tmp_path), str(tmp_path), "--jpeg-device", "--features-only"] + extra, capture_output=True, text=True)
            assert r.returncode != 0 and "--jpeg-device" in r.stdout, (exe, extra, r.stdout[-300:])


def test_parser_and_coefficient_sink_under_sanitizers(tmp_path):
    """the refactored header in a stand-alone program (tests/host/jpeg_scan_test.cpp, -fsanitize=address,undefined): all 18 fixtures
    and the damaged buffers of the GPU test; clean, and every component of an accepted file receives blocks x 64 coefficients"""
    subprocess.check_call(["make", "-C", jc.HOSTDIR, "-f", "jpeg_scan.mk", "jpeg_scan_test"], stdout=subprocess.DEVNULL)
    exe = os.path.join(jc.HOSTDIR, "jpeg_scan_test")
    files, expect = [], {}
    for name in jc.ALL:
        files.append(jc.jpg_path(name))
        expect[files[-1]] = "ok"
    extra = {"progressive": open(os.path.join(jc.JDIR, "progressive_unsupported.jpg"), "rb").read(),
             "cut200": jc.jpg_bytes("c420_q75")[:200], "junk": b"\xff\xd8" + bytes(range(256)) * 4,
             "q16": jc.quantiser_ffff(jc.jpg_bytes("c444_q90"))}
    for name in ("c420_restart_q80", "d420_dri1"):
        for label, data in jc.damaged_streams(name).items():
            extra[name + "." + label] = data
    for label, data in extra.items():
        p = tmp_path / (label + ".jpg")
        p.write_bytes(data)
        files.append(str(p))
    for label in ("progressive", "cut200", "junk"):
        expect[str(tmp_path / (label + ".jpg"))] = "refused-headers"
    for name in ("c420_restart_q80", "d420_dri1"):
        for label in ("rst_removed", "cut"):                    # a marker short: the scan cannot be completed
            expect[str(tmp_path / (name + "." + label + ".jpg"))] = "refused-scan"
    r = subprocess.run([exe] + files, capture_output=True, text=True)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stdout[-600:], r.stderr[-600:])
    lines = {ln.split()[0]: ln.split()[1:] for ln in r.stdout.splitlines() if ln and not ln.startswith(" ")}
    assert sorted(lines) == sorted(files)
    index = _index()
    for path, verdict in expect.items():
        assert lines[path][0] == verdict, (path, lines[path])
    for name in jc.ALL:
        f = lines[jc.jpg_path(name)]
        rows, cols, ch, dri, n_int = (int(v) for v in f[1:6])
        assert (rows, cols, ch, dri, n_int) == index[name], name
        assert len(f) == 6 + ch                                 # one block count per component; the program checked count == blocks x 64
        if ch == 1:
            assert int(f[6]) == -(-rows // 8) * -(-cols // 8), name
