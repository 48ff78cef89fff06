"""Resource usage of the view-selection kernels as compiled into libsfmhip.so (no GPU needed), read from the code object's notes as
tests/test_codeobj_cpu.py reads them: no scratch, nothing spilled, and no LDS (the unit settles its adds in registers by ballot)."""
import os

import pytest

from test_codeobj_cpu import LIB, READELF, _kernel_table

KERNELS = ("select_geo_kernel", "select_key_kernel", "select_ray_kernel", "select_pair_kernel", "select_mirror_kernel", "select_rank_kernel", "select_range_kernel",
           "select_widen_kernel")


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not found")
def test_select_kernels_have_no_scratch(tmp_path):
    assert os.path.exists(LIB), "build libsfmhip.so first (__graft_entry__.build)"
    t = _kernel_table(tmp_path)
    for sub in KERNELS:
        hits = [(k, v) for k, v in t.items() if sub in k]
        assert len(hits) == 1, (sub, hits)
        name, k = hits[0]
        print(name, k)
        assert k["scratch"] == 0 and (k["spill"] or 0) == 0 and k["lds"] == 0, (name, k)
        assert k["vgpr"] + k["agpr"] <= 64, (name, k)                     # eight waves per SIMD
