"""The two passes of find_extrema (sfm_opencv_amd/host/sfm_akaze.hpp) on a list of candidates, restated in plain Python with float32
arithmetic: what sfmhip_akaze_suppress is held to.  tests/test_akaze_cpu.py ties it to the header through tests/host/akaze_ref.cpp."""
import numpy as np

F = np.float32


def level_sizes():
    """esigma * derivative_factor of the 16 levels.  The header takes pow in float; here the power is taken in double and rounded, and
    test_akaze_cpu compares the result with the sizes the header's code gave."""
    return np.array([F(F(1.6) * F(2.0 ** (F(F(s) / F(4)) + F(o)))) * F(1.5) for o in range(4) for s in range(4)], np.float32)


def suppress(xyr, level, sizes=None):
    """xyr: n x {x, y, response}; level: n ints, not decreasing.  Returns (aux, out): the candidate indices that occupy aux after the
    first pass, and those that survive the second, both in aux order."""
    xyr = np.asarray(xyr, np.float32).reshape(-1, 3)
    level = [int(v) for v in level]
    sizes = level_sizes() if sizes is None else np.asarray(sizes, np.float32)
    x, y, r = xyr[:, 0], xyr[:, 1], xyr[:, 2]
    aux = []
    for c in range(len(level)):
        s2 = sizes[level[c]] * sizes[level[c]]
        is_extremum, repeated, id_rep = True, False, 0
        for k, e in enumerate(aux):
            if level[e] != level[c] and level[e] != level[c] - 1:
                continue
            dx = x[c] - x[e]; dy = y[c] - y[e]
            if dx * dx + dy * dy <= s2:
                if r[c] > r[e]:
                    repeated, id_rep = True, k
                else:
                    is_extremum = False
                break
        if not is_extremum:
            continue
        if repeated:
            aux[id_rep] = c
        else:
            aux.append(c)
    out = []
    for i, a in enumerate(aux):
        keep = True
        for b in aux[i + 1:]:
            if level[b] != level[a] + 1 and level[b] != level[a]:
                continue
            dx = x[a] - x[b]; dy = y[a] - y[b]
            if dx * dx + dy * dy <= sizes[level[b]] * sizes[level[b]] and r[a] < r[b]:
                keep = False
                break
        if keep:
            out.append(a)
    return np.array(aux, np.int32), np.array(out, np.int32)
