"""Compare the kNN kernels of two gfx950 device assemblies of csrc/match.hip (hipcc <the match.o flags> --cuda-device-only -S):
resource numbers, instruction count and opcode histogram per kernel; for kernels whose opcode sequence differs, the differing runs
and where each lies relative to the kernel's stage loop (head label .. last back-branch) and the MFMA stream inside it.
python3 experiments/knn_asm_diff.py parent.s branch.s"""
import collections, difflib, re, sys

KERNELS = ["_Z14knn2_i8_kernelILi%dEEvPK8PairDescPxi" % k for k in (1, 2, 4)] + \
          ["_Z21knn2_i8_mutual_kernelILi%dEEvPK8PairDescPxiPyPKx" % k for k in (1, 2, 4)] + \
          ["_Z24knn2_hamming2_fp4_kernelILi8EEvPK8PairDescPxi", "_Z31knn2_hamming2_fp4_mutual_kernelILi8EEvPK8PairDescPxiPyPKx"]
RES = ("NumVgprs", "NumAgprs", "TotalNumSgprs", "ScratchSize", "LDSByteSize", "Occupancy")


def kernel(path, name):
    """(lines of the body: ('label', text) or ('op', opcode, text), resource numbers)"""
    txt = open(path).read()
    body = txt[txt.index("\n%s:" % name):]
    end = re.search(r"\n\.Lfunc_end\d+:", body).start()
    res = {k: int(re.search(r"; %s: (\d+)" % k, body[end:]).group(1)) for k in RES}
    res["spill"] = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", txt[txt.index(".name:           %s\n" % name):]).group(1)) \
        if (".name:           %s\n" % name) in txt else None
    lines = []
    for l in body[:end].split("\n")[2:]:
        l = l.split(";")[0].rstrip()
        if re.match(r"\.LBB\d+_\d+:", l):
            lines.append(("label", l[:-1]))
        elif l.startswith("\t") and not l.lstrip().startswith("."):
            lines.append(("op", l.split()[0], " ".join(l.split())))
    return lines, res


def stage_loop(lines):
    """instruction indices (head, first MFMA, last MFMA, back-branch) and the head label of the outermost loop that holds MFMAs"""
    ops, labels = [], {}
    for l in lines:
        if l[0] == "label":
            labels[l[1]] = len(ops)
        else:
            ops.append(l)
    best = None
    for i, o in enumerate(ops):
        m = re.match(r"s_c?branch\w* (\.LBB\d+_\d+)", o[2])
        if m and labels[m.group(1)] <= i:
            h = labels[m.group(1)]
            mf = [k for k in range(h, i) if ops[k][1].startswith("v_mfma")]
            if mf and (best is None or h <= best[0]):
                best = (h, mf[0], mf[-1], i, m.group(1))
    if best is None:
        raise SystemExit("no loop around the MFMAs")
    return best


def where(i1, i2, loop):
    lo, hi = i1, max(i2, i1 + 1) - 1
    if hi < loop[0]:
        return "before the loop"
    if lo > loop[3]:
        return "after the loop"
    if hi < loop[1]:
        return "loop: before its first MFMA"
    if lo > loop[2]:
        return "loop: after its last MFMA"
    return "loop: MFMA STREAM"


a_path, b_path = sys.argv[1:3]
for name in KERNELS:
    (la, ra), (lb, rb) = kernel(a_path, name), kernel(b_path, name)
    oa, ob = [l for l in la if l[0] == "op"], [l for l in lb if l[0] == "op"]
    ha, hb = collections.Counter(o[1] for o in oa), collections.Counter(o[1] for o in ob)
    print(name)
    print("  resources  parent %s\n             branch %s  %s" % (ra, rb, "identical" if ra == rb else "DIFFERENT"))
    print("  instructions  parent %d  branch %d   opcode histogram %s" % (len(oa), len(ob), "identical" if ha == hb else "DIFFERENT"))
    if ha != hb:
        print("  histogram difference (branch - parent):", {k: hb[k] - ha[k] for k in sorted(set(ha) | set(hb)) if ha[k] != hb[k]})
    sa, sb = [o[1] for o in oa], [o[1] for o in ob]
    if sa == sb:
        print("  opcode sequence identical")
        continue
    pa, pb = stage_loop(la), stage_loop(lb)
    for tag, q in (("parent", pa), ("branch", pb)):
        print("  %s loop: head %s = instruction %d, MFMAs %d .. %d, last back-branch %d" % (tag, q[4], q[0], q[1], q[2], q[3]))
    print("  MFMA stream (opcode sequence first .. last MFMA):", "identical" if sa[pa[1]:pa[2] + 1] == sb[pb[1]:pb[2] + 1] else "DIFFERENT")
    count = collections.Counter()
    for tag, i1, i2, j1, j2 in difflib.SequenceMatcher(None, sa, sb, autojunk=False).get_opcodes():
        if tag == "equal":
            continue
        w = where(j1, j2, pb)
        count[w] += 1
        print("  %s parent[%d:%d] branch[%d:%d]  %s" % (tag, i1, i2, j1, j2, w))
        for o in oa[i1:i2]:
            print("    - " + o[2])
        for o in ob[j1:j2]:
            print("    + " + o[2])
    print("  differing runs by place:", dict(count))
