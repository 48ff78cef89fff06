"""Resource usage of the hot kernels as compiled into libsfmhip.so (no GPU needed): no scratch, and VGPR counts inside the occupancy the
kernels are designed for.  A single spilled fragment in knn2_hamming2_fp4_kernel once cost 22 % (its reload put s_waitcnt vmcnt(0)
behind every stage's LDS-DMA prefetch, profiles/r03_hamming_fp4.md): this is the guard."""
import os, re, struct, subprocess, shutil
import pytest

LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sfm_opencv_amd", "libsfmhip.so")
READELF = shutil.which("llvm-readelf") or "/opt/rocm/lib/llvm/bin/llvm-readelf"


def _gfx950_code_objects(path):
    """the gfx950 ELFs out of the library's clang offload bundles (.hip_fatbin)"""
    blob = open(path, "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    out, at = [], 0
    while True:
        at = blob.find(magic, at)
        if at < 0:
            return out
        n, = struct.unpack_from("<Q", blob, at + len(magic))
        p = at + len(magic) + 8
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", blob, p)
            triple = blob[p + 24:p + 24 + tl].decode()
            p += 24 + tl
            if "gfx950" in triple and size:
                out.append(blob[at + off:at + off + size])
        at += len(magic)


def _kernel_table(tmp_path):
    table = {}
    for i, co in enumerate(_gfx950_code_objects(LIB)):
        f = tmp_path / f"co{i}.elf"
        f.write_bytes(co)
        txt = subprocess.run([READELF, "--notes", str(f)], capture_output=True, text=True, check=True).stdout
        for blk in txt.split("- .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk)
            if not name:
                continue
            def field(k):
                m = re.search(r"\.%s:\s+(\d+)" % k, blk)
                return int(m.group(1)) if m else None
            table[name.group(1)] = dict(vgpr=field("vgpr_count"), agpr=int(blk.split()[0]), scratch=field("private_segment_fixed_size"),
                                        lds=field("group_segment_fixed_size"), spill=field("vgpr_spill_count"))
    return table


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not found")
def test_hot_kernels_have_no_scratch_and_fit_their_occupancy(tmp_path):
    assert os.path.exists(LIB), "build libsfmhip.so first (__graft_entry__.build)"
    t = _kernel_table(tmp_path)
    assert len(t) > 40, sorted(t)[:5]

    def find(sub):
        hits = [k for k in t if sub in k]
        assert hits, f"no kernel named *{sub}* in the library"
        return [(k, t[k]) for k in hits]

    # (name fragment, registers allowed for the waves per SIMD the kernel is built around, spilled registers tolerated)
    # The fp64 BA kernels are compiled for three waves per SIMD (168 registers) and spill a few values OUTSIDE their inner loops
    # (ba_camschur_kernel: 10 registers; measured against the two-wave, spill-free build: 82 against 84 us) -- bounded here so a
    # change that pushes spills into the loops shows up.
    budget = [("knn2_hamming2_fp4_kernelILi8", 256, 0),     # 2 waves per SIMD
              ("knn2_i8_kernelILi4", 128, 0),                # 4 waves per SIMD
              ("distmat_i8_kernelILi4", 128, 0),
              ("ba_camschur_kernel", 168, 12), ("ba_point_kernel", 168, 0), ("ba_back_kernel", 168, 12),
              ("chol_node_forward_kernel", 256, 4), ("chol_top_kernel", 256, 2)]
    for sub, regs, spills in budget:
        for name, k in find(sub):
            assert (k["spill"] or 0) <= spills and (spills or k["scratch"] == 0), (name, k)
            assert k["vgpr"] + k["agpr"] <= regs, (name, k)
    for name, k in find("knn2_hamming2_fp4_kernelILi8"):
        assert 48 * 1024 < k["lds"] <= 80 * 1024, (name, k)     # two staged buffers; one 8-wave workgroup per CU

    # The chain solver's two kernels (csrc/ba_chain.hpp): latency-bound, every spilled value would sit on the chain each camera
    # waits for.  The bound is what the commit before the mirrored reads of S compiled to for gfx950: scratch and spilled registers
    # equal to it, and the register count inside the same occupancy bucket (chain_sub_kernel: eight waves per workgroup, two per
    # SIMD, 256 registers; chain_top_kernel: sixteen waves, four per SIMD, 128 registers).
    #        (name fragment,      scratch bytes, spilled registers, registers of the bucket)     measured there: VGPR + AGPR / scratch / spills
    chain = [("chain_sub_kernel", 0, 0, 256),                                                  # 215 + 0 / 0 / 0
             ("chain_top_kernel", 0, 0, 128)]                                                  # 118 + 0 / 0 / 0
    for sub, scratch, spills, regs in chain:
        hits = find(sub)
        assert len(hits) == 1, hits
        for name, k in hits:
            assert k["scratch"] == scratch and (k["spill"] or 0) == spills, (name, k)
            assert k["vgpr"] + k["agpr"] <= regs, (name, k)
