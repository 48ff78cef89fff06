"""Resource usage of the track kernels as compiled into libsfmhip.so (no GPU needed), read from the code object's notes as
tests/test_codeobj_cpu.py reads them: no scratch, nothing spilled, eight waves per SIMD, and LDS in the per-pair compaction only."""
import os

import pytest

from test_codeobj_cpu import LIB, READELF, _kernel_table

KERNELS = ("tracks_init_kernel", "tracks_link_kernel", "tracks_flatten_kernel", "tracks_first_kernel", "tracks_cstart_kernel", "tracks_comp_kernel",
           "tracks_keep_kernel", "tracks_scatter_kernel", "tracks_stats_kernel", "tracks_filter_kernel")


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not found")
def test_tracks_kernels_have_no_scratch(tmp_path):
    assert os.path.exists(LIB), "build libsfmhip.so first (__graft_entry__.build)"
    t = _kernel_table(tmp_path)
    assert sorted(k for k in t if "tracks_" in k and "triangulate_tracks" not in k) == sorted(k for k in t if any(sub in k for sub in KERNELS))      # no track kernel goes unlisted
    for sub in KERNELS:
        hits = [(k, v) for k, v in t.items() if sub in k]
        assert len(hits) == 1, (sub, hits)
        name, k = hits[0]
        print(name, k)
        assert k["scratch"] == 0 and (k["spill"] or 0) == 0, (name, k)
        assert k["vgpr"] + k["agpr"] <= 64, (name, k)                     # eight waves per SIMD
        assert (k["lds"] == 0) == (sub != "tracks_filter_kernel"), (name, k)
