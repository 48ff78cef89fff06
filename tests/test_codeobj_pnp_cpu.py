"""Resource usage of the absolute-pose kernels (no GPU needed): pnp_score_kernel keeps a projection matrix and a counter per lane in
registers and its chunk of padded five-double rows in LDS, like twoview_score_kernel; pnp_hyp_kernel keeps its 11 x 12 matrix in
registers (VGPRs and AGPRs of a single wave per SIMD) through the same elimination body as twoview_hyp_kernel.  Neither may touch
scratch memory."""
import os

import pytest

from test_codeobj_cpu import LIB, READELF, _kernel_table


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not found")
def test_pnp_kernels_have_no_scratch_and_no_spills(tmp_path):
    assert os.path.exists(LIB), "build libsfmhip.so first (__graft_entry__.build)"
    t = _kernel_table(tmp_path)
    ks = [(k, v) for k, v in t.items() if "pnp_score_kernel" in k]
    assert len(ks) == 1, sorted(t)
    for name, k in ks:
        assert k["scratch"] == 0 and (k["spill"] or 0) == 0, (name, k)
        assert k["lds"] == 512 * 48, (name, k)                              # SCORE_CHUNK rows of six doubles (five and padding): 24 KB
        assert k["vgpr"] <= 128, (name, k)                                  # four waves per SIMD
    hs = [(k, v) for k, v in t.items() if "pnp_hyp_kernel" in k]
    assert len(hs) == 1, sorted(t)
    for name, k in hs:
        assert k["scratch"] == 0 and (k["spill"] or 0) == 0, (name, k)
        assert k["lds"] == 0 and k["vgpr"] + k["agpr"] <= 512, (name, k)    # one wave per SIMD: the matrix alone is 264 registers
