"""CPU side of the cross check (SFMHIP_MATCH_MUTUAL): the new kernels as compiled into libsfmhip.so use no scratch and fit the
occupancy they are built for, the C-ABI declares the flag, and the drivers advertise --cross-check.  No GPU needed."""
import os
import re
import subprocess

import pytest

from test_codeobj_cpu import LIB, READELF, _kernel_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not found")
def test_mutual_kernels_fit_their_register_budget(tmp_path):
    t = _kernel_table(tmp_path)
    # (name fragment, registers allowed, instantiations expected)
    # (name fragment, registers allowed, instantiations expected, spilled registers tolerated).  The FP4 variant sits at the plain
    # kernel's 256-register limit and spills 4 registers for the column pass (measured with them: 1.44x the plain pass at C4,
    # profiles/r05_time_match_mutual.log): bounded here so that more does not creep in unseen.
    for sub, regs, n, spills in (("knn2_i8_mutual_kernel", 168, 3, 0), ("knn2_hamming2_fp4_mutual_kernel", 256, 1, 4),
                                 ("rev_finalize_kernel", 128, 2, 0), ("rev_rescore_l2_kernel", 128, 1, 0),
                                 ("rev_from_knn_kernel", 128, 1, 0), ("mutual_filter_kernel", 128, 1, 0)):
        hits = [(k, v) for k, v in t.items() if sub in k]
        assert len(hits) == n, (sub, sorted(t)[:5])
        for name, k in hits:
            assert (k["spill"] or 0) <= spills and (spills or k["scratch"] == 0) and k["scratch"] <= 8 * spills, (name, k)
            assert k["vgpr"] + k["agpr"] <= regs, (name, k)
    for name, k in t.items():
        if "knn2_i8_mutual_kernel" in name:
            assert k["lds"] * 3 <= 160 * 1024, (name, k)          # three workgroups per CU


def test_header_declares_the_mutual_flag():
    h = open(os.path.join(ROOT, "include", "sfmhip.h")).read()
    assert re.search(r"#define\s+SFMHIP_MATCH_MUTUAL\s+1\b", h)
    for fn in ("sfmhip_knn2_mutual_dev", "sfmhip_match_pairs_ex_dev", "sfmhip_match_pairs_ex", "sfmhip_match_pairs_multi_ex"):
        assert re.search(r"\b%s\s*\(" % fn, h), fn


@pytest.mark.parametrize("prog", ["NViewReconstruct", "TwoViewReconstruct"])
def test_drivers_list_cross_check_in_their_usage(prog):
    host = os.path.join(ROOT, "sfm_opencv_amd", "host")
    subprocess.check_call(["make", "-C", host], stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(host, prog)], capture_output=True, text=True, timeout=60)     # no arguments: usage, no device
    assert out.returncode == 0 and "[--cross-check]" in out.stdout, out.stdout


# Each plain / mutual kernel pair is one body: the four __global__ kernels only call it, so neither can be tuned without the other.
_KNN_MFMA = {"knn2_i8": "__builtin_amdgcn_mfma_i32_32x32x32_i8", "knn2_hamming2_fp4": "__builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4"}


def _void_functions(src):
    """{name: text} of the void functions of match.hip, comments stripped: definitions start and close at column 0"""
    src = re.sub(r"//.*", "", src)
    return {m.group(1): m.group(0) for m in re.finditer(r"^(?:\w[^\n;{]*\s)?void\s+(\w+)\s*\([^{;]*\)\s*\{.*?^\}", src, re.M | re.S)}


@pytest.mark.parametrize("stem", sorted(_KNN_MFMA))
def test_each_kernel_pair_is_one_body(stem):
    f = _void_functions(open(os.path.join(ROOT, "sfm_opencv_amd", "csrc", "match.hip")).read())
    for kernel in (stem + "_kernel", stem + "_mutual_kernel"):
        head, body = f[kernel].split("{", 1)
        assert "__global__" in head, kernel
        assert re.search(r"\b%s_body\s*<" % stem, body) and body.count(";") == 1, (kernel, body)
        assert "__builtin_amdgcn_mfma" not in body and "__builtin_amdgcn_global_load_lds" not in body, kernel
    assert [n for n, text in f.items() if n.startswith("knn2_") and _KNN_MFMA[stem] in text] == [stem + "_body"]


# vgpr + agpr, LDS bytes, scratch bytes, spilled registers of every instantiation, as the commit before the shared bodies compiled them
# (its kept copies, read off its libsfmhip.so with _kernel_table): sharing the source must not move the register allocation.
_PARENT_RESOURCES = {"knn2_i8_kernelILi1E": (110, 33792, 0, 0), "knn2_i8_kernelILi2E": (118, 33792, 0, 0), "knn2_i8_kernelILi4E": (128, 33792, 0, 0),
                     "knn2_i8_mutual_kernelILi1E": (134, 37888, 0, 0), "knn2_i8_mutual_kernelILi2E": (139, 37888, 0, 0),
                     "knn2_i8_mutual_kernelILi4E": (150, 37888, 0, 0),
                     "knn2_hamming2_fp4_kernelILi8E": (248, 67584, 0, 0), "knn2_hamming2_fp4_mutual_kernelILi8E": (255, 73728, 20, 4)}


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not found")
def test_shared_bodies_keep_the_kept_copies_resources(tmp_path):
    t = _kernel_table(tmp_path)
    got = {sub: [(k["vgpr"] + k["agpr"], k["lds"], k["scratch"], k["spill"] or 0) for name, k in sorted(t.items()) if sub in name]
           for sub in _PARENT_RESOURCES}
    assert got == {sub: [r] for sub, r in _PARENT_RESOURCES.items()}
    assert sum("knn2_i8_" in n or "knn2_hamming2_fp4_" in n for n in t) == len(_PARENT_RESOURCES), sorted(t)
