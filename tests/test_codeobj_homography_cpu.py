"""Resource usage of the homography kernels (no GPU needed): homography_score_kernel keeps a homography and a counter per lane in registers
and its chunk of rows in LDS, like twoview_score_kernel; homography_hyp_kernel keeps its 8 x 9 matrix in registers through the same
elimination body as twoview_hyp_kernel.  Neither may touch scratch memory."""
import os

import pytest

from test_codeobj_cpu import LIB, READELF, _kernel_table


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not found")
def test_homography_kernels_have_no_scratch_and_no_spills(tmp_path):
    assert os.path.exists(LIB), "build libsfmhip.so first (__graft_entry__.build)"
    t = _kernel_table(tmp_path)
    ks = [(k, v) for k, v in t.items() if "homography_score_kernel" in k]
    assert len(ks) == 1, sorted(t)
    for name, k in ks:
        assert k["scratch"] == 0 and (k["spill"] or 0) == 0, (name, k)
        assert k["lds"] == 512 * 32, (name, k)                              # SCORE_CHUNK rows of four doubles: 16 KB
        assert k["vgpr"] <= 128, (name, k)                                  # four waves per SIMD
    hs = [(k, v) for k, v in t.items() if "homography_hyp_kernel" in k]
    assert len(hs) == 1, sorted(t)
    for name, k in hs:
        assert k["scratch"] == 0 and (k["spill"] or 0) == 0, (name, k)
        assert k["lds"] == 0 and k["vgpr"] <= 256, (name, k)                # two waves per SIMD
