"""Resource usage of the constant-point forms of the per-point kernels (no GPU needed).  ba_point_kernel is a template on PTFIX and
ba_back_lin_const_kernel is ba_back_kernel_lin for problems with constant points: the forms every problem without constant points
runs stay under the budgets of test_codeobj_cpu.py / test_codeobj_seam_cpu.py, and the new ones (ba_back_const_kernel too) go under the
same budgets."""
import os

import pytest

from test_codeobj_cpu import LIB, READELF, _kernel_table


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not found")
def test_constant_point_instances_keep_the_budgets(tmp_path):
    assert os.path.exists(LIB), "build libsfmhip.so first (__graft_entry__.build)"
    t = _kernel_table(tmp_path)
    for flag, back in (("ILb0E", "ba_back_kernel_lin"), ("ILb1E", "ba_back_lin_const_kernel")):
        pk = [(k, v) for k, v in t.items() if "ba_point_kernel" + flag in k]
        bk = [(k, v) for k, v in t.items() if back in k]
        assert len(pk) == 1 and len(bk) == 1, sorted(t)
        for name, k in pk:
            assert k["scratch"] == 0 and (k["spill"] or 0) == 0 and k["vgpr"] + k["agpr"] <= 168, (name, k)
        for name, k in bk:
            assert k["vgpr"] + k["agpr"] <= 168 and (k["spill"] or 0) <= 12 and 3 * k["lds"] <= 160 * 1024, (name, k)
    # the back-substitution without the point pass, for problems with constant points: the budget of ba_back_kernel
    bc = [(k, v) for k, v in t.items() if "ba_back_const_kernel" in k]
    assert len(bc) == 1, sorted(t)
    for name, k in bc:
        assert k["vgpr"] + k["agpr"] <= 168 and (k["spill"] or 0) <= 12, (name, k)
