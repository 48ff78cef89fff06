"""Compare kernels of two gfx950 device assemblies of one source file (hipcc <the object's flags> --cuda-device-only -S): resource
numbers, instruction count and opcode histogram per kernel; for kernels whose opcode sequence differs, the differing runs and where
each lies: in which loop of the branch's kernel (loops are found by their back-branches and described by what they hold: barriers,
LDS reads, global loads, MFMAs), or outside every loop; where both sides have the same number of loops, the fp64 VALU count and the
opcode histogram of each pair of loop bodies.  For a kernel with MFMAs the place is given relative to its stage loop (head
label .. last back-branch) and the MFMA stream inside it.

    python3 experiments/knn_asm_diff.py parent.s branch.s [kernel ...]

A kernel is named by its mangled symbol or by a fragment of it that fits exactly one kernel; `all` stands for every kernel of the
parent's file.  Without names: the kNN kernels of csrc/match.hip."""
import collections, difflib, re, sys

KNN_KERNELS = ["_Z14knn2_i8_kernelILi%dEEvPK8PairDescPxi" % k for k in (1, 2, 4)] + \
              ["_Z21knn2_i8_mutual_kernelILi%dEEvPK8PairDescPxiPyPKx" % k for k in (1, 2, 4)] + \
              ["_Z24knn2_hamming2_fp4_kernelILi8EEvPK8PairDescPxi", "_Z31knn2_hamming2_fp4_mutual_kernelILi8EEvPK8PairDescPxiPyPKx"]
RES = ("NumVgprs", "NumAgprs", "TotalNumSgprs", "ScratchSize", "LDSByteSize", "Occupancy")


def kernel_names(path):
    return re.findall(r"^\s*\.amdhsa_kernel (\S+)", open(path).read(), re.M)


def resolve(arg, names):
    if arg in names:
        return arg
    hits = [k for k in names if arg in k]
    if len(hits) != 1:
        raise SystemExit("%r names %d kernels: %s" % (arg, len(hits), hits))
    return hits[0]


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


def loops(lines):
    """the loops of a kernel, outermost first: (head, back-branch, head label), instruction indices; one entry per head label"""
    ops, labels = [], {}
    for l in lines:
        if l[0] == "label":
            labels[l[1]] = len(ops)
        else:
            ops.append(l)
    found = {}
    for i, o in enumerate(ops):
        m = re.match(r"s_c?branch\w* (\.LBB\d+_\d+)", o[2])
        if m and labels[m.group(1)] <= i:
            found[m.group(1)] = (labels[m.group(1)], i, m.group(1))          # the last back-branch to a head wins
    return ops, sorted(found.values(), key=lambda q: (q[0], -q[1]))


def holds(ops, q):
    body = [o[1] for o in ops[q[0]:q[1] + 1]]
    what = [w for w, pre in (("barrier", "s_barrier"), ("LDS reads", "ds_read"), ("global loads", "global_load"), ("sqrt", "v_sqrt"),
                             ("atomics", "global_atomic"), ("MFMAs", "v_mfma")) if any(b.startswith(pre) for b in body)]
    return ", ".join(what) or "no memory access"


def stage_loop(ops, ls):
    """instruction indices (head, first MFMA, last MFMA, back-branch) and the head label of the outermost loop that holds MFMAs"""
    for h, i, label in ls:
        mf = [k for k in range(h, i) if ops[k][1].startswith("v_mfma")]
        if mf:
            return (h, mf[0], mf[-1], i, label)
    raise SystemExit("no loop around the MFMAs")


def where_mfma(i1, i2, loop):
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


def where_loop(i1, i2, ls):
    """the innermost loop that holds the whole run, else the innermost one it touches"""
    lo, hi = i1, max(i2, i1 + 1) - 1
    inside = [q for q in ls if q[0] <= lo and hi <= q[1]]
    if inside:
        return "in loop %s" % min(inside, key=lambda q: q[1] - q[0])[2]
    touched = [q for q in ls if lo <= q[1] and q[0] <= hi]
    if touched:
        return "across the edge of loop %s" % min(touched, key=lambda q: q[1] - q[0])[2]
    return "outside every loop"


def compare(a_path, b_path, name):
    (la, ra), (lb, rb) = kernel(a_path, name), kernel(b_path, name)
    (oa, lsa), (ob, lsb) = loops(la), loops(lb)
    ha, hb = collections.Counter(o[1] for o in oa), collections.Counter(o[1] for o in ob)
    print(name)
    print("  resources  parent %s\n             branch %s  %s" % (ra, rb, "identical" if ra == rb else "DIFFERENT"))
    print("  instructions  parent %d  branch %d   opcode histogram %s" % (len(oa), len(ob), "identical" if ha == hb else "DIFFERENT"))
    if ha != hb:
        print("  histogram difference (branch - parent):", {k: hb[k] - ha[k] for k in sorted(set(ha) | set(hb)) if ha[k] != hb[k]})
    sa, sb = [o[1] for o in oa], [o[1] for o in ob]
    if sa == sb:
        print("  opcode sequence identical")
        return
    mfma = any(s.startswith("v_mfma") for s in sb)
    if mfma:
        pa, pb = stage_loop(oa, lsa), stage_loop(ob, lsb)
        for tag, q in (("parent", pa), ("branch", pb)):
            print("  %s loop: head %s = instruction %d, MFMAs %d .. %d, last back-branch %d" % (tag, q[4], q[0], q[1], q[2], q[3]))
        print("  MFMA stream (opcode sequence first .. last MFMA):", "identical" if sa[pa[1]:pa[2] + 1] == sb[pb[1]:pb[2] + 1] else "DIFFERENT")
    else:
        for tag, ops, ls in (("parent", oa, lsa), ("branch", ob, lsb)):
            for q in ls:
                depth = sum(1 for o in ls if o[0] <= q[0] and q[1] <= o[1]) - 1
                print("  %s loop %s%s: instructions %d .. %d (%d), holds %s" % (tag, "  " * depth, q[2], q[0], q[1], q[1] - q[0] + 1, holds(ops, q)))
        if len(lsa) == len(lsb):                                     # the loops pair up in order: what each pair's bodies hold
            for qa, qb in zip(lsa, lsb):
                ca, cb = (collections.Counter(o[1] for o in ops[q[0]:q[1] + 1]) for ops, q in ((oa, qa), (ob, qb)))
                f64 = [sum(v for k, v in c.items() if "f64" in k) for c in (ca, cb)]
                print("  loop %s / %s: fp64 VALU %d / %d, opcode histogram %s" % (qa[2], qb[2], f64[0], f64[1], "identical" if ca == cb else
                      "difference (branch - parent) %s" % {k: cb[k] - ca[k] for k in sorted(set(ca) | set(cb)) if ca[k] != cb[k]}))
    count = collections.Counter()
    for tag, i1, i2, j1, j2 in difflib.SequenceMatcher(None, sa, sb, autojunk=False).get_opcodes():
        if tag == "equal":
            continue
        w = where_mfma(j1, j2, pb) if mfma else where_loop(j1, j2, lsb)
        count[w] += 1
        print("  %s parent[%d:%d] branch[%d:%d]  %s" % (tag, i1, i2, j1, j2, w))
        for o in oa[i1:i2]:
            print("    - " + o[2])
        for o in ob[j1:j2]:
            print("    + " + o[2])
    print("  differing runs by place:", dict(count))


def main():
    a_path, b_path = sys.argv[1:3]
    names = kernel_names(a_path)
    want = sys.argv[3:] or KNN_KERNELS
    for name in (names if want == ["all"] else [resolve(w, names) for w in want]):
        compare(a_path, b_path, name)


if __name__ == "__main__":
    main()
