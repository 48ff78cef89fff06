"""CPU side of the cross check (SFMHIP_MATCH_MUTUAL): the new kernels as compiled into libsfmhip.so use no scratch and fit the
occupancy they are built for, the C-ABI declares the flag, and the drivers advertise --cross-check.  No GPU needed."""
import os
import re
import subprocess

import pytest

from test_codeobj_cpu import LIB, READELF, _kernel_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not found")
def test_mutual_kernels_fit_their_register_budget(tmp_path):
    t = _kernel_table(tmp_path)
    # (name fragment, registers allowed, instantiations expected)
    # (name fragment, registers allowed, instantiations expected, spilled registers tolerated).  The FP4 variant sits at the plain
    # kernel's 256-register limit and spills 4 registers for the column pass (measured with them: 1.44x the plain pass at C4,
    # profiles/r05_time_match_mutual.log): bounded here so that more does not creep in unseen.
    for sub, regs, n, spills in (("knn2_i8_mutual_kernel", 168, 3, 0), ("knn2_hamming2_fp4_mutual_kernel", 256, 1, 4),
                                 ("rev_finalize_kernel", 128, 2, 0), ("rev_rescore_l2_kernel", 128, 1, 0),
                                 ("rev_from_knn_kernel", 128, 1, 0), ("mutual_filter_kernel", 128, 1, 0)):
        hits = [(k, v) for k, v in t.items() if sub in k]
        assert len(hits) == n, (sub, sorted(t)[:5])
        for name, k in hits:
            assert (k["spill"] or 0) <= spills and (spills or k["scratch"] == 0) and k["scratch"] <= 8 * spills, (name, k)
            assert k["vgpr"] + k["agpr"] <= regs, (name, k)
    for name, k in t.items():
        if "knn2_i8_mutual_kernel" in name:
            assert k["lds"] * 3 <= 160 * 1024, (name, k)          # three workgroups per CU


def test_header_declares_the_mutual_flag():
    h = open(os.path.join(ROOT, "include", "sfmhip.h")).read()
    assert re.search(r"#define\s+SFMHIP_MATCH_MUTUAL\s+1\b", h)
    for fn in ("sfmhip_knn2_mutual_dev", "sfmhip_match_pairs_ex_dev", "sfmhip_match_pairs_ex", "sfmhip_match_pairs_multi_ex"):
        assert re.search(r"\b%s\s*\(" % fn, h), fn


@pytest.mark.parametrize("prog", ["NViewReconstruct", "TwoViewReconstruct"])
def test_drivers_list_cross_check_in_their_usage(prog):
    host = os.path.join(ROOT, "sfm_opencv_amd", "host")
    subprocess.check_call(["make", "-C", host], stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(host, prog)], capture_output=True, text=True, timeout=60)     # no arguments: usage, no device
    assert out.returncode == 0 and "[--cross-check]" in out.stdout, out.stdout


# The mutual kernels are kept copies of the plain ones (a template flag changed the plain kernels' register allocation): every code line
# of the plain kernel must still be in its mutual copy, in order, apart from the lines listed here (the LDS size, the timing-experiment
# knobs the copies leave out, the places where the column pass is threaded in).  Tuning one kernel without the other fails here.
_COPY_EXCEPTIONS = {'knn2_i8_kernel': ['__shared__ __attribute__((aligned(16))) unsigned char lds[STAGE_BYTES > MERGE_BYTES ? STAGE_BYTES : MERGE_BYTES];'], 'knn2_hamming2_fp4_kernel': ['#if !defined(H4_EXP) || !defined(SFMHIP_EXPERIMENTS)', '#undef H4_EXP', '#define H4_EXP 0', '__shared__ __attribute__((aligned(16))) unsigned char lds[STAGE_BYTES > MERGE_BYTES ? STAGE_BYTES : MERGE_BYTES];', 'const int nblocks = (H4_EXP & 32) ? 1 : (t_end - t_begin) / TROWS;', 'v4i a = (H4_EXP & 128) ? (v4i){ lane, s, at, 7 } : *(gv4)(Q + (size_t)(q0r + 32 * at + l31) * RB + 16 * (2 * s + half));', 'if (v < 16) H4_TOP2(best1[0][v], best2[0][v], p0[v]);', 'else if (v < 32) H4_TOP2(best1[1][v - 16], best2[1][v - 16], p1[v - 16]);', 'auto compute = [&]() {', 'if (g + H4_AHEAD < NG && !((H4_EXP & 8) && g >= 1)) bq[(g + H4_AHEAD) % (H4_AHEAD + 1)] = rd(g + H4_AHEAD);', 'if (!(H4_EXP & 4)) { top2_of(p0, p1, 3 * (s - 1)); top2_of(p0, p1, 3 * (s - 1) + 1); top2_of(p0, p1, 3 * (s - 1) + 2); }', 'if (blk + 1 < nblocks && !(H4_EXP & 1)) g_stage((blk + 1) & 1, blk + 1);', 'compute();', 'if (!(H4_EXP & 2)) __syncthreads();', 'if (H4_EXP & 2) __syncthreads();', 'const int off_k = 768 * pd.dim, k_pad = 1 << 20;', 'if (H4_EXP & 64) {', 'float sum = 0.0f;', 'for (int i = 0; i < 16; ++i) sum += best1[at][i] + best2[at][i];', 'if (sum == 12345.0f) part[2 * pd.part_off + tid] = 1;', 'return;']}


def _code_lines(src, name):
    i = src.index(name + "(")
    j = src.index("{", i)
    depth = 0
    for k in range(j, len(src)):
        depth += {"{": 1, "}": -1}.get(src[k], 0)
        if depth == 0:
            break
    lines = (re.sub(r"//.*", "", l).strip() for l in src[j:k + 1].split("\n"))
    return [l for l in lines if l]


@pytest.mark.parametrize("plain,mutual", [("knn2_i8_kernel", "knn2_i8_mutual_kernel"),
                                          ("knn2_hamming2_fp4_kernel", "knn2_hamming2_fp4_mutual_kernel")])
def test_mutual_kernels_still_contain_their_plain_kernel(plain, mutual):
    src = open(os.path.join(ROOT, "sfm_opencv_amd", "csrc", "match.hip")).read()
    p, m = _code_lines(src, "void " + plain), _code_lines(src, "void " + mutual)
    missing, k = [], 0
    for line in p:
        while k < len(m) and m[k] != line:
            k += 1
        if k == len(m):
            missing.append(line)
            k = 0
        else:
            k += 1
    assert missing == _COPY_EXCEPTIONS[plain], [l for l in missing if l not in _COPY_EXCEPTIONS[plain]]
