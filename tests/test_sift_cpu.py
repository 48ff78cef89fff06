"""CPU: the device SIFT (csrc/sift.hip) as far as it can be checked without a GPU -- the four entry points are declared, exported and
bound; arguments are refused before the device is touched; without a device the call is an error, never a host fallback; the blur,
extrema and descriptor kernels use no scratch and fit LDS; both drivers know --sift-device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from sfm_opencv_amd import _lib, api
from test_codeobj_cpu import LIB, READELF, _kernel_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "sfm_opencv_amd", "host")
NAMES = ["sfmhip_sift_extract", "sfmhip_sift_extract_dev", "sfmhip_sift_scale_space", "sfmhip_sift_extrema"]


def test_the_four_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "sfmhip.h")).read()
    lib = _lib.load()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in _lib.SYMBOLS and hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None and getattr(lib, name).restype is C.c_int
    assert len(lib.sfmhip_sift_extract.argtypes) == 11 and len(lib.sfmhip_sift_extract_dev.argtypes) == 11
    assert len(lib.sfmhip_sift_scale_space.argtypes) == 13 and len(lib.sfmhip_sift_extrema.argtypes) == 10
    for name in ("sift_extract", "sift_extract_dev", "sift_scale_space", "sift_extrema", "sift_extract_for_all"):
        assert callable(getattr(api.Context, name))


def test_sift_extract_without_a_device_raises():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(api.SfmHipError):
        api.Context(0).sift_extract(np.zeros((32, 32), np.uint8))
    with pytest.raises(api.SfmHipError):
        api.default_context().sift_extract_for_all([np.zeros((32, 32), np.uint8)])


def test_bad_arguments_are_refused_before_the_device_is_touched():
    """no context exists on this path at all: whatever is answered is answered by the argument checks"""
    lib = _lib.load()
    img = np.zeros((16, 24, 3), np.uint8)
    p, n = img.ctypes.data, C.c_int32(-5)
    kp = np.zeros(4, api.KEYPOINT); desc = np.zeros((4, 128), np.float32)
    r, c, no = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    bad = [dict(rows=0), dict(cols=0), dict(rows=-3), dict(ch=2), dict(ch=0), dict(ld=71), dict(cap=-1), dict(img=None), dict(rows=16385)]
    for b in bad:
        a = dict(img=p, rows=16, cols=24, ch=3, ld=72, cap=4)
        a.update(b)
        assert lib.sfmhip_sift_extract(None, a["img"], a["rows"], a["cols"], a["ch"], a["ld"], 0, kp.ctypes.data, desc.ctypes.data, a["cap"], C.byref(n)) == _lib.E_ARG, b
        assert lib.sfmhip_sift_extract_dev(None, a["img"], a["rows"], a["cols"], a["ch"], a["ld"], 0, kp.ctypes.data, desc.ctypes.data, a["cap"], None) == _lib.E_ARG, b
        assert lib.sfmhip_sift_extrema(None, a["img"], a["rows"], a["cols"], a["ch"], a["ld"], None, None, a["cap"], C.byref(n)) == _lib.E_ARG, b
        if "cap" not in b:
            assert lib.sfmhip_sift_scale_space(None, a["img"], a["rows"], a["cols"], a["ch"], a["ld"], 0, 0, 0, None, r, c, no) == _lib.E_ARG, b
    assert lib.sfmhip_sift_extract(None, p, 16, 24, 3, 72, -1, kp.ctypes.data, desc.ctypes.data, 4, C.byref(n)) == _lib.E_ARG          # max_features < 0
    for octave, index, kind in ((-1, 0, 0), (0, 6, 0), (0, 5, 1), (0, 0, 2)):
        assert lib.sfmhip_sift_scale_space(None, p, 16, 24, 3, 72, octave, index, kind, None, r, c, no) == _lib.E_ARG
    # a null context with good arguments is an argument error too, and nothing was written
    assert lib.sfmhip_sift_extract(None, p, 16, 24, 3, 72, 0, kp.ctypes.data, desc.ctypes.data, 4, C.byref(n)) == _lib.E_ARG
    assert n.value == -5 and (r.value, c.value, no.value) == (-1, -1, -1) and not desc.any()


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not found")
def test_sift_kernels_use_no_scratch_and_fit_lds(tmp_path):
    assert os.path.exists(LIB), "build libsfmhip.so first (__graft_entry__.build)"
    t = _kernel_table(tmp_path)
    # the blur kernels are instantiated for the five tap radii of the six fixed sigmas
    for sub, count in (("sift_blur_rows_kernel", 5), ("sift_blur_cols_kernel", 5), ("sift_extrema_kernel", 1), ("sift_descriptor_kernel", 1),
                       ("sift_orient_kernel", 1)):
        ks = [(k, v) for k, v in t.items() if sub in k]
        assert len(ks) == count, (sub, sorted(t))
        for name, k in ks:
            assert k["scratch"] == 0 and (k["spill"] or 0) == 0, (name, k)
            assert 0 < k["lds"] <= 64 * 1024, (name, k)


def test_both_drivers_list_sift_device_in_their_usage():
    subprocess.check_call(["make", "-C", HOST], stdout=subprocess.DEVNULL)
    for exe in ("NViewReconstruct", "TwoViewReconstruct"):
        out = subprocess.run([os.path.join(HOST, exe)], capture_output=True, text=True).stdout
        assert "usage:" in out and "[--sift-device]" in out, exe
