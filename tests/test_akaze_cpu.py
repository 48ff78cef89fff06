"""CPU: the device AKAZE (csrc/akaze.hip) as far as it can be checked without a GPU -- the five entry points are declared, exported and
bound; arguments are refused before the device is touched; without a device the call is an error, never a host fallback; the kernels use
no scratch and fit LDS; both drivers know --akaze-device; the Python restatement of the suppression (tests/akaze_suppress_ref.py) gives
what find_extrema of sfm_akaze.hpp gives."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import akaze_suppress_ref as sref
from sfm_opencv_amd import _lib, api
from test_codeobj_cpu import LIB, READELF, _kernel_table

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST = os.path.join(ROOT, "sfm_opencv_amd", "host")
NAMES = ["sfmhip_akaze_extract", "sfmhip_akaze_extract_dev", "sfmhip_akaze_scale_space", "sfmhip_akaze_extrema", "sfmhip_akaze_suppress"]


def test_the_five_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "sfmhip.h")).read()
    lib = _lib.load()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in _lib.SYMBOLS and hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None and getattr(lib, name).restype is C.c_int
    assert [len(getattr(lib, n).argtypes) for n in NAMES] == [11, 11, 13, 11, 6]
    for name in ("akaze_extract", "akaze_extract_dev", "akaze_extract_for_all", "akaze_scale_space", "akaze_extrema", "akaze_suppress"):
        assert callable(getattr(api.Context, name))


def test_akaze_extract_without_a_device_raises():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(api.SfmHipError):
        api.Context(0).akaze_extract(np.zeros((96, 96), np.uint8))
    with pytest.raises(api.SfmHipError):
        api.default_context().akaze_extract_for_all([np.zeros((96, 96), np.uint8)])


def test_bad_arguments_are_refused_before_the_device_is_touched():
    """no context exists on this path at all: whatever is answered is answered by the argument checks"""
    lib = _lib.load()
    img = np.zeros((96, 100, 3), np.uint8)
    p, n = img.ctypes.data, C.c_int32(-5)
    kp = np.zeros(4, api.KEYPOINT); desc = np.zeros((4, 61), np.uint8)
    r, c, nl, kc = C.c_int(-1), C.c_int(-1), C.c_int(-1), C.c_float(-1)
    bad = [dict(rows=0), dict(cols=0), dict(rows=-3), dict(ch=2), dict(ch=0), dict(ld=299), dict(cap=-1), dict(img=None), dict(rows=16385)]
    for b in bad:
        a = dict(img=p, rows=96, cols=100, ch=3, ld=300, cap=4)
        a.update(b)
        assert lib.sfmhip_akaze_extract(None, a["img"], a["rows"], a["cols"], a["ch"], a["ld"], 0, kp.ctypes.data, desc.ctypes.data, a["cap"], C.byref(n)) == _lib.E_ARG, b
        assert lib.sfmhip_akaze_extract_dev(None, a["img"], a["rows"], a["cols"], a["ch"], a["ld"], 0, kp.ctypes.data, desc.ctypes.data, a["cap"], None) == _lib.E_ARG, b
        assert lib.sfmhip_akaze_extrema(None, a["img"], a["rows"], a["cols"], a["ch"], a["ld"], 0, None, None, a["cap"], C.byref(n)) == _lib.E_ARG, b
        if "cap" not in b:
            assert lib.sfmhip_akaze_scale_space(None, a["img"], a["rows"], a["cols"], a["ch"], a["ld"], 0, 0, None, r, c, nl, kc) == _lib.E_ARG, b
    assert lib.sfmhip_akaze_extract(None, p, 96, 100, 3, 300, -1, kp.ctypes.data, desc.ctypes.data, 4, C.byref(n)) == _lib.E_ARG          # max_features < 0
    for level, kind in ((-1, 0), (16, 0), (0, 5), (0, -1)):
        assert lib.sfmhip_akaze_scale_space(None, p, 96, 100, 3, 300, level, kind, None, r, c, nl, kc) == _lib.E_ARG
    for stage in (-1, 3):
        assert lib.sfmhip_akaze_extrema(None, p, 96, 100, 3, 300, stage, None, None, 0, C.byref(n)) == _lib.E_ARG
    # the suppression alone: a negative count, null lists, a level out of range, levels that decrease
    xyr = np.zeros((3, 3), np.float32); kept = np.full(3, -9, np.int32)
    for lv, cnt, x in (([0, 1, 2], -1, xyr), ([0, 1, 2], 3, None), ([0, 1, 16], 3, xyr), ([-1, 0, 0], 3, xyr), ([0, 2, 1], 3, xyr)):
        lv = np.array(lv, np.int32)
        assert lib.sfmhip_akaze_suppress(None, x.ctypes.data if x is not None else None, lv.ctypes.data, cnt, kept.ctypes.data, C.byref(n)) == _lib.E_ARG, (lv, cnt)
    # a null context with good arguments is an argument error too, and nothing was written
    assert lib.sfmhip_akaze_extract(None, p, 96, 100, 3, 300, 0, kp.ctypes.data, desc.ctypes.data, 4, C.byref(n)) == _lib.E_ARG
    assert lib.sfmhip_akaze_suppress(None, xyr.ctypes.data, np.zeros(3, np.int32).ctypes.data, 3, kept.ctypes.data, C.byref(n)) == _lib.E_ARG
    assert n.value == -5 and (r.value, c.value, nl.value, kc.value) == (-1, -1, -1, -1.0) and not desc.any() and (kept == -9).all()


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not found")
def test_akaze_kernels_use_no_scratch_and_fit_lds(tmp_path):
    assert os.path.exists(LIB), "build libsfmhip.so first (__graft_entry__.build)"
    t = _kernel_table(tmp_path)
    ak = {k: v for k, v in t.items() if "akaze_" in k}
    # the two blur radii (7 for sigma 1.6, 4 for sigma 1) have an instance each, every other kernel one
    for sub, count in (("akaze_blur_rows_kernel", 2), ("akaze_blur_cols_kernel", 2), ("akaze_fed_kernel", 1), ("akaze_flow_kernel", 1), ("akaze_deriv1_kernel", 1),
                       ("akaze_det_kernel", 1), ("akaze_maxima_kernel", 1), ("akaze_suppress_kernel", 1), ("akaze_suppress_round_kernel", 1), ("akaze_suppress_publish_kernel", 1), ("akaze_suppress2_kernel", 1), ("akaze_subpixel_kernel", 1),
                       ("akaze_describe_kernel", 1), ("akaze_hmax_kernel", 1), ("akaze_hist_kernel", 1)):
        assert len([k for k in ak if sub in k]) == count, (sub, sorted(ak))
    assert len(ak) >= 20
    for name, k in ak.items():          # "no kernel in this file may use scratch": all of them, not only the hot ones
        assert k["scratch"] == 0 and (k["spill"] or 0) == 0, (name, k)
        assert k["lds"] <= 64 * 1024, (name, k)
    for sub in ("akaze_blur_rows_kernel", "akaze_blur_cols_kernel", "akaze_describe_kernel", "akaze_suppress_kernel"):
        assert all(k["lds"] > 0 for name, k in ak.items() if sub in name), sub


def test_both_drivers_list_akaze_device_in_their_usage():
    subprocess.check_call(["make", "-C", HOST], stdout=subprocess.DEVNULL)
    for exe in ("NViewReconstruct", "TwoViewReconstruct"):
        out = subprocess.run([os.path.join(HOST, exe)], capture_output=True, text=True).stdout
        assert "usage:" in out and "[--akaze-device]" in out and "[--sift-device]" in out, exe


# ------------------------------------------------------------------------------------------------ the Python restatement against the header
def build_akaze_ref(directory):
    """tests/host/akaze_ref.cpp, built with the line tests/host/Makefile uses for geom_test"""
    exe = os.path.join(str(directory), "akaze_ref")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-fopenmp", "-o", exe, os.path.join(HERE, "host", "akaze_ref.cpp"),
                           "-L" + os.path.join(ROOT, "sfm_opencv_amd"), "-lsfmhip", "-Wl,-rpath," + os.path.join(ROOT, "sfm_opencv_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def run_akaze_ref(exe, img, tmp, max_features=0):
    import struct
    img = np.ascontiguousarray(img)
    ch = 1 if img.ndim == 2 else 3
    raw_in, raw_out = os.path.join(tmp, "img.raw"), os.path.join(tmp, "ref.bin")
    img.tofile(raw_in)
    subprocess.check_call([exe, raw_in, str(img.shape[0]), str(img.shape[1]), str(ch), raw_out] + ([str(max_features)] if max_features else []))
    raw = open(raw_out, "rb").read()
    off = 0
    n_levels, = struct.unpack_from("<i", raw, off); off += 4
    levels, kc = [], []
    for _ in range(n_levels):
        r, c, k = struct.unpack_from("<iif", raw, off); off += 12
        levels.append(np.frombuffer(raw, "<f4", 5 * r * c, off).reshape(5, r, c)); off += 20 * r * c
        kc.append(np.float32(k))
    stages = []
    for _ in range(3):
        n, = struct.unpack_from("<i", raw, off); off += 4
        xysr = np.frombuffer(raw, "<f4", 4 * n, off).reshape(n, 4); off += 16 * n
        ol = np.frombuffer(raw, "<i4", 2 * n, off).reshape(n, 2); off += 8 * n
        stages.append((xysr, ol))
    m, = struct.unpack_from("<i", raw, off); off += 4
    kp = np.frombuffer(raw, api.KEYPOINT, m, off); off += 28 * m
    desc = np.frombuffer(raw, np.uint8, 61 * m, off).reshape(m, 61); off += 61 * m
    assert off == len(raw)
    return dict(n_levels=n_levels, levels=levels, kc=kc, stages=stages, kp=kp, desc=desc)


def texture(h, w, seed, blobs=700, smin=2.0, smax=9.0):
    """smooth random blobs on a gradient (the recipe of tests/test_sift_gpu.py)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = 90 + 30 * np.sin(xx / 97.0) + 20 * np.cos(yy / 71.0)
    for _ in range(blobs):
        cx, cy = rng.uniform(0, w), rng.uniform(0, h)
        s = rng.uniform(smin, smax); a = rng.uniform(-70, 70)
        img += a * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * s * s))
    return np.clip(img, 0, 255)


@pytest.mark.parametrize("shape,seed,n_levels", [((200, 260), 3, 8), ((161, 243), 21, 8), ((330, 350), 3, 12)])
def test_the_python_suppression_is_find_extrema(tmp_path, shape, seed, n_levels):
    """on the raw maxima of an image, akaze_suppress_ref.suppress keeps what find_extrema of the header returns, in its order (find_extrema
    does not show its intermediate list, so the first pass is tied to the header through the second, on three images)"""
    ref = run_akaze_ref(build_akaze_ref(tmp_path), texture(shape[0], shape[1], seed).astype(np.uint8), str(tmp_path))
    (raw, raw_ol), (out, out_ol) = ref["stages"][0], ref["stages"][1]
    assert ref["n_levels"] == n_levels and len(raw) > 60 and 30 < len(out) < len(raw) - 30          # not vacuous: both kept and suppressed candidates
    # the level sizes of the restatement are the header's
    sizes = sref.level_sizes()
    assert np.array_equal(sizes[raw_ol[:, 1]].view(np.uint32), raw[:, 2].copy().view(np.uint32))
    assert (np.diff(raw_ol[:, 1]) >= 0).all()
    aux, kept = sref.suppress(raw[:, [0, 1, 3]], raw_ol[:, 1])
    assert len(aux) >= len(kept) == len(out)
    assert np.array_equal(raw[kept].view(np.uint32), out.copy().view(np.uint32)) and np.array_equal(raw_ol[kept], out_ol)


def test_the_driver_has_no_host_path_behind_akaze_device(tmp_path):
    """NViewReconstruct --akaze --akaze-device in a process that sees no GPU: the library's refusal is printed and no image gets key
    points, while the same command without the flag extracts them on the host.  (A driver that did not know the flag, or fell back to
    the host extractor, would print the counts.)"""
    subprocess.check_call(["make", "-C", HOST], stdout=subprocess.DEVNULL)
    exe = os.path.join(HOST, "NViewReconstruct")
    d = tmp_path / "imgs"; d.mkdir()
    g = texture(120, 160, 5).astype(np.uint8)
    with open(d / "00.ppm", "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (g.shape[1], g.shape[0])); f.write(np.stack([g, g, g], 2).tobytes())
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")          # the child sees no device, whatever the machine has
    host = subprocess.run([exe, str(d), str(tmp_path), "--akaze", "--features-only"], capture_output=True, text=True, env=env)
    dev = subprocess.run([exe, str(d), str(tmp_path), "--akaze", "--akaze-device", "--features-only", "--save-features=" + str(tmp_path / "f.bin")],
                         capture_output=True, text=True, env=env)
    assert host.stdout.count("2D feature point detected.") == 1
    assert "no CPU fallback" in dev.stdout and "2D feature point detected." not in dev.stdout and "Extracting features" not in dev.stdout
