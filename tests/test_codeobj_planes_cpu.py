"""Resource usage of the plane-scoring kernel (no GPU needed): plane_score_kernel keeps a plane and a counter per lane in registers
and its chunk of points in LDS; it must not touch scratch memory."""
import os

import pytest

from test_codeobj_cpu import LIB, READELF, _kernel_table


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not found")
def test_plane_score_kernel_has_no_scratch_and_no_spills(tmp_path):
    assert os.path.exists(LIB), "build libsfmhip.so first (__graft_entry__.build)"
    t = _kernel_table(tmp_path)
    ks = [(k, v) for k, v in t.items() if "plane_score_kernel" in k]
    assert len(ks) == 1, sorted(t)
    for name, k in ks:
        assert k["scratch"] == 0 and (k["spill"] or 0) == 0, (name, k)
        assert k["lds"] == 512 * 32, (name, k)                              # SCORE_CHUNK rows of four doubles
