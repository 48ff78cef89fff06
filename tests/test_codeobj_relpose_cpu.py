"""Resource usage of the relative-pose kernel as compiled into libsfmhip.so (no GPU needed): one kernel for the whole call, no scratch, no
spilled registers, and exactly the LDS that DESIGN.md 4c says it keeps (the poses, the five derivatives of E and the reduction areas; the
rows stay in global memory).  It looks at the resource metadata of the code object only."""
import os
import re

import pytest

from test_codeobj_cpu import LIB, READELF, _kernel_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not found")
def test_one_relpose_kernel_without_scratch(tmp_path):
    assert os.path.exists(LIB), "build libsfmhip.so first (__graft_entry__.build)"
    t = _kernel_table(tmp_path)
    hits = [k for k in t if "relpose" in k]
    assert len(hits) == 1, hits
    k = t[hits[0]]
    assert k["scratch"] == 0 and (k["spill"] or 0) == 0, k
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    said = re.search(r"relpose_kernel keeps (\d+) bytes of LDS", design)
    assert said, "DESIGN.md 4c no longer says what relpose_kernel keeps in LDS"
    assert k["lds"] == int(said.group(1)), (k, said.group(0))
    assert k["vgpr"] + k["agpr"] <= 512, k                                 # one workgroup of four waves per CU: one wave per SIMD
