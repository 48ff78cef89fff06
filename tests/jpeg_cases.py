"""Shared by tests/test_jpeg_device_cpu.py and tests/test_jpeg_device_gpu.py: the 18 JPEG fixtures, the committed pixels, and the
damaged streams both files build (the same bytes on either side, so the host program and the device see one input)."""
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
JDIR = os.path.join(HERE, "golden", "jpeg")                 # the nine of tests/test_jpeg_cpu.py
DDIR = os.path.join(HERE, "golden", "jpeg_device")          # nine more, about restart intervals
HOSTDIR = os.path.join(HERE, "host")

OLD = ["c444_q90", "c422_q85", "c422_odd_q60", "c420_q75", "c420_odd_q95", "c420_restart_q80", "c422_restart_rows_opt", "gray_q80", "c420_q20"]
NEW = ["d420_dri1", "d420_dri5_odd", "d444_dri2", "d422_dri1_opt", "dgray_dri4", "d420_tiny", "d422_tiny_dri1", "d420_q100", "d420_one_interval"]
ALL = OLD + NEW


def jpg_path(name):
    return os.path.join(JDIR if name in OLD else DDIR, name + ".jpg")


def jpg_bytes(name):
    with open(jpg_path(name), "rb") as f:
        return f.read()


def read_pnm(path):
    """rows x cols x channels uint8 of a binary PPM / PGM as Pillow and tests/host/jpeg_test write them"""
    with open(path, "rb") as f:
        magic = f.readline().strip()
        dims = f.readline().split()
        while dims and dims[0].startswith(b"#"):
            dims = f.readline().split()
        w, h = int(dims[0]), int(dims[1])
        assert f.readline().strip() == b"255"
        ch = 3 if magic == b"P6" else 1
        a = np.frombuffer(f.read(w * h * ch), np.uint8)
    return a.reshape(h, w, ch)


_golden = {}


def golden(name):
    """the committed pixels of a fixture in the layout jpeg_decode returns: rows x cols (gray) or rows x cols x 3 BGR"""
    if name not in _golden:
        base = jpg_path(name)[:-4]
        a = read_pnm(base + (".ppm" if os.path.exists(base + ".ppm") else ".pgm"))
        a = a[:, :, 0].copy() if a.shape[2] == 1 else a[:, :, ::-1].copy()
        a.setflags(write=False)
        _golden[name] = a
    return _golden[name]


def scan_start(data):
    """offset of the first entropy-coded byte"""
    i = 2
    while i + 4 <= len(data):
        assert data[i] == 0xFF
        m = data[i + 1]; L = (data[i + 2] << 8) | data[i + 3]
        i += 2 + L
        if m == 0xDA:
            return i
    raise AssertionError("no scan")


def rst_positions(data):
    s = scan_start(data)
    return [i for i in range(s, len(data) - 1) if data[i] == 0xFF and 0xD0 <= data[i + 1] <= 0xD7]


def damaged_streams(name):
    """{label: bytes}: the file `name` (one with restart markers) damaged in four ways"""
    data = jpg_bytes(name)
    rst = rst_positions(data)
    assert len(rst) >= 4
    k = len(rst) // 2
    out = {}
    out["rst_removed"] = data[:rst[k]] + data[rst[k] + 2:]
    a, b = rst[k] + 2, rst[k + 1]                           # the bytes of one segment
    rnd = np.random.default_rng(1234).integers(0, 256, b - a, dtype=np.uint8)
    rnd[rnd == 0xFF] = 0xFE
    out["segment_random"] = data[:a] + rnd.tobytes() + data[b:]
    mid = (a + b) // 2
    if data[mid - 1] == 0xFF:                                 # do not turn a stuffed FF 00 into FF FF
        mid += 1
    planted = bytearray(data); planted[mid:mid + 2] = b"\xff\xd9"
    out["eoi_planted"] = bytes(planted)
    s = scan_start(data)
    out["cut"] = data[:s + (len(data) - s) // 2]
    return out


def quantiser_ffff(data):
    """the file with its first 8-bit quantisation table rewritten as a 16-bit one full of 0xFFFF (the construction of
    tests/test_jpeg_cpu.py::test_extreme_quantiser_and_category_values_do_not_overflow)"""
    data = bytearray(data)
    i = 2
    while i + 4 <= len(data):
        m = data[i + 1]; L = (data[i + 2] << 8) | data[i + 3]
        if m == 0xDB:
            assert data[i + 4] >> 4 == 0
            tq = data[i + 4] & 15
            rest = bytes(data[i + 4 + 65:i + 2 + L])
            seg = bytes([0x10 | tq]) + b"\xff\xff" * 64 + rest
            data[i + 2:i + 2 + L] = bytes([(len(seg) + 2) >> 8, (len(seg) + 2) & 255]) + seg
            return bytes(data)
        i += 2 + L
    raise AssertionError("no DQT")


def host_decode(data, tmp_path, tag="x"):
    """tests/host/jpeg_test on these bytes: None when the host decoder refuses them, else its pixels in jpeg_decode's layout"""
    subprocess.check_call(["make", "-C", HOSTDIR, "jpeg_test"], stdout=subprocess.DEVNULL)
    src, dst = tmp_path / (tag + ".jpg"), tmp_path / (tag + ".pnm")
    src.write_bytes(data)
    r = subprocess.run([os.path.join(HOSTDIR, "jpeg_test"), str(src), str(dst)], capture_output=True)
    assert r.returncode in (0, 1), r.stderr[-400:]
    if r.returncode == 1:
        return None
    a = read_pnm(str(dst))
    return a[:, :, 0].copy() if a.shape[2] == 1 else a[:, :, ::-1].copy()
