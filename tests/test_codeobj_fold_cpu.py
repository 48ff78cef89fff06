"""Code objects around SFMHIP_BA_SEAM bit 9 (no GPU needed), in the style of the chain table of test_codeobj_cpu.py.

ba_camschur_kernel_fold is ba_camschur_kernel with the camera and pair-block folds behind both roles (ba_fold_tail).  Where that tail
stands decides the roles' register allocation: with the hand-off inside the roles the camera role's constants came through vector
loads and the kernel spilled 28 registers, some of them inside its loops; behind both roles it spills 2.  The bound is
ba_camschur_kernel's own (168 registers, 12 spilled: three waves per SIMD), and that kernel must stay what the commit before the fold
compiled to.  The kernels of the solve and of the back-substitution are not touched: scratch bytes and spilled registers equal to that
commit's, registers inside the same occupancy bucket."""
import os

import pytest

from test_codeobj_cpu import LIB, READELF, _kernel_table


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not found")
def test_fold_kernel_fits_three_waves_and_its_neighbours_keep_their_figures(tmp_path):
    assert os.path.exists(LIB), "build libsfmhip.so first (__graft_entry__.build)"
    t = _kernel_table(tmp_path)

    def one(sub):
        hits = [(k, v) for k, v in t.items() if sub in k]
        assert len(hits) == 1, (sub, [k for k, _ in hits])
        return hits[0]

    name, k = one("ba_camschur_kernel_fold")
    assert k["vgpr"] + k["agpr"] <= 168 and (k["spill"] or 0) <= 12, (name, k)
    #        (name fragment,            scratch bytes, spilled registers, registers of the bucket)     measured at the parent: VGPR + AGPR / scratch / spills
    parent = [("ba_camschur_kernel5BADev", 28, 10, 168),                                                # 167 + 0 / 28 / 10
              ("chol_tree_backward_kernel", 0, 0, 256),                                                 #  97 + 0 /  0 /  0
              ("ba_back_kernel5BADev", 0, 0, 168),                                                      # 168 + 0 /  0 /  0
              ("ba_back_kernel_lin", 0, 0, 168),                                                        # 165 + 0 /  0 /  0
              ("ba_back_const_kernel", 12, 2, 168),                                                     # 168 + 0 / 12 /  2
              ("ba_back_lin_const_kernel", 12, 2, 168),                                                 # 166 + 0 / 12 /  2
              ("ba_back_reduce_kernel", 0, 0, 128)]                                                     #  80 + 0 /  0 /  0
    for sub, scratch, spills, regs in parent:
        name, k = one(sub)
        assert k["scratch"] == scratch and (k["spill"] or 0) == spills, (name, k)
        assert k["vgpr"] + k["agpr"] <= regs, (name, k)
