"""Resource usage of the back-substitution kernel that also carries the next point pass (no GPU needed): it must keep the three
waves per SIMD ba_back_kernel is built around, with its few spills outside the loops, and three workgroups' LDS must fit a CU."""
import os
import pytest

from test_codeobj_cpu import LIB, READELF, _kernel_table


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not found")
def test_back_kernel_with_the_point_pass_fits_three_waves_per_simd(tmp_path):
    assert os.path.exists(LIB), "build libsfmhip.so first (__graft_entry__.build)"
    t = _kernel_table(tmp_path)
    hits = [(k, v) for k, v in t.items() if "ba_back_kernel_lin" in k]
    assert len(hits) == 1, sorted(t)
    for name, k in hits:
        assert k["vgpr"] + k["agpr"] <= 168, (name, k)
        assert (k["spill"] or 0) <= 12, (name, k)
        assert 3 * k["lds"] <= 160 * 1024, (name, k)
    # the plain form and the point kernel are still there under their names (the switch and the fallback launch them)
    assert any("ba_back_kernel" in k and "ba_back_kernel_lin" not in k for k in t)
    for name, k in t.items():
        if "ba_point_kernel" in name:
            assert k["scratch"] == 0 and (k["spill"] or 0) == 0 and k["vgpr"] + k["agpr"] <= 168, (name, k)
