"""Cases and plain-Python restatements for tests/test_resegment.py (minimum-error re-segmentation; the definition is in
include/s2st_hip.h next to s2st_reseg_i32)."""
import itertools

import numpy as np

STRIP = 8          # reference columns per thread (csrc/reseg.hip RS_C)
BLOCK = 256 * 8    # ... and per pass of the 256-thread wavefront (the 1024-thread one covers 8192: tests/test_resegment.py)


def clamped(ends, m):
    out, prev = [], 0
    for k, e in enumerate(ends):
        prev = min(max(int(e), prev), m)
        out.append(prev)
    out[-1] = m
    return out


def scalar_resegment(h, r, ends):
    """The definition as loops: the full table, the walk back (diagonal, then up, then left), the largest row per boundary
    column.  Returns (cuts, seg_dist, dist, D)."""
    n, m = len(h), len(r)
    e = clamped(ends, m)
    D = [[0] * (m + 1) for _ in range(n + 1)]
    for i in range(n + 1):
        D[i][0] = i
    for j in range(m + 1):
        D[0][j] = j
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            D[i][j] = min(D[i - 1][j - 1] + (h[i - 1] != r[j - 1]), D[i - 1][j] + 1, D[i][j - 1] + 1)
    path = [(n, m)]
    i, j = n, m
    while (i, j) != (0, 0):
        if i > 0 and j > 0 and D[i][j] == D[i - 1][j - 1] + (h[i - 1] != r[j - 1]):
            i, j = i - 1, j - 1
        elif i > 0 and D[i][j] == D[i - 1][j] + 1:
            i -= 1
        else:
            assert j > 0 and D[i][j] == D[i][j - 1] + 1
            j -= 1
        path.append((i, j))
    cuts = [max(i for i, j in path if j == ek) for ek in e]
    y = [D[c][ek] for c, ek in zip(cuts, e)]
    seg = [b - a for a, b in zip([0] + y, y)]
    return cuts, seg, D[n][m], D


def best_cut_sum(h, sentences, edit_distance):
    """min over all non-decreasing cuts of the summed per-sentence distances, by enumeration."""
    n, K = len(h), len(sentences)
    best = None
    for cut in itertools.combinations_with_replacement(range(n + 1), K - 1):
        at = (0,) + cut + (n,)
        s = sum(edit_distance(list(h[a:b]), list(sen)) for a, b, sen in zip(at, at[1:], sentences))
        best = s if best is None else min(best, s)
    return best


def small_cases(count, seed=7):
    """(h, sentences, ends): alphabets of 1 to 3 ids, n, m <= 7, K <= 4 -- ties everywhere; n = 0, m = 0, empty sentences and
    boundaries at column 0 occur."""
    rng = np.random.RandomState(seed)
    out = []
    for t in range(count):
        A = 1 + t % 3
        n, K = int(rng.randint(0, 8)), int(rng.randint(1, 5))
        m = int(rng.randint(0, 8)) if t % 11 else 0
        cut = sorted(int(v) for v in rng.randint(0, m + 1, K - 1))
        if t % 5 == 0 and K > 1:
            cut[0] = 0  # an empty first sentence: a boundary at column 0
        ends = cut + [m]
        r = [int(v) for v in rng.randint(0, A, m)]
        h = [int(v) for v in rng.randint(0, A, n)]
        sentences = [r[a:b] for a, b in zip([0] + ends, ends)]
        out.append((h, sentences, ends))
    return out


def noisy(ref, rng, sub=7, drop=11, vocab=5):
    """The reference with about every `sub`-th token replaced and every `drop`-th dropped."""
    out = []
    for i, t in enumerate(ref):
        if i % drop == drop - 1:
            continue
        out.append(int(rng.randint(0, vocab)) if i % sub == sub - 1 else int(t))
    return out


def even_ends(m, K):
    return [m * (k + 1) // K for k in range(K)]


def ragged_batch(seed=3):
    """[(name, h, r, ends)] around every size at which csrc/reseg.hip takes another path: m around the strip width, 63 / 64 /
    65 strips (the wave boundary), one strip more than a workgroup's pass, n in {0, 1, 2} and n >> m, K = 1, every column a
    boundary with duplicates, `ends` out of order and out of range (the clamping)."""
    rng = np.random.RandomState(seed)
    tok = lambda n, A=3: [int(v) for v in rng.randint(0, A, n)]  # noqa: E731
    out = []
    for m in (0, 1, STRIP - 1, STRIP, STRIP + 1):
        for n in (0, 1, 2, 9):
            out.append((f"m{m} n{n}", tok(n), tok(m), even_ends(m, 2)))
    for strips in (63, 64, 65):
        m = strips * STRIP - (strips % 2) * 3
        r = tok(m, 5)
        out.append((f"{strips} strips", noisy(r, rng)[:40], r, even_ends(m, 7)))
    r = tok(BLOCK + STRIP, 4)
    out.append(("a pass and a strip", noisy(r, rng)[:3], r, even_ends(len(r), 5)))
    r = tok(BLOCK + 5, 4)
    out.append(("a pass and five columns", r[BLOCK - 20:] + tok(4, 4), r, [BLOCK - 1, BLOCK, BLOCK + 1, BLOCK + 5]))
    out.append(("n >> m", tok(300), tok(5), [2, 5]))
    out.append(("K = 1", tok(30), tok(37), [37]))
    r = tok(21)
    out.append(("every column a boundary", noisy(r, rng, 3, 5, 3), r, sorted(list(range(22)) + [0, 0, 7, 7, 21])))
    out.append(("ends out of order", tok(25), tok(30), [12, 5, -3, 40, 20, 7]))
    out.append(("both empty", [], [], [0, 0]))
    r = tok(70, 2)
    out.append(("one symbol apart", [0] * 50, r, even_ends(70, 9)))
    return out


def medium_case(n_ref=200, K=9, seed=5):
    """About 150 x 200 over five symbols."""
    rng = np.random.RandomState(seed)
    r = [int(v) for v in rng.randint(0, 5, n_ref)]
    h = noisy(r, rng, 4, 5)[:150]
    return h, r, even_ends(n_ref, K)


def large_case(n_ref=2500, K=120, seed=9):
    """About 3000 x 2500, K = 120 (the device only): insertions make the hypothesis the longer side."""
    rng = np.random.RandomState(seed)
    r = [int(v) for v in rng.randint(0, 50, n_ref)]
    h = []
    for i, t in enumerate(noisy(r, rng, 7, 11, 50)):
        h.append(t)
        if i % 3 == 0:
            h.append(int(rng.randint(0, 50)))
    return h, r, even_ends(n_ref, K)
