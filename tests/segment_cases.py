"""Inputs shared by tests/test_segment.py: the enumeration the search is checked against, seeded small search problems full
of ties, the ragged batch of recordings at every boundary of the kernel, and a burst / pause recording at a given length."""
import itertools

import numpy as np

WIN, HOP, RATE = 400, 160, 16000  # the Kaldi filter bank's framing at 16 kHz
CHUNK = 32                        # csrc/segment.hip: SG_C


def enumerate_best(S, lam, min_len, max_len):
    """(cost, cuts) by enumeration of EVERY admissible cut set of T = len(S) frames, ordered by (cost, reversed cut list):
    the smallest s at the last step, then at the one before it, .. -- the tie rule of the definition."""
    T = len(S)
    if T < min_len:
        return 0, [0, T]
    keys = []

    def extend(cuts):  # every way to go on from the last cut with an admissible segment
        a = cuts[-1]
        for b in range(a + min_len, min(a + max_len, T) + 1):
            if b == T:
                keys.append((sum(int(S[c]) + lam for c in cuts[1:]), [T, *cuts[::-1]]))
            else:
                extend(cuts + [b])

    extend([0])
    assert keys, (T, min_len, max_len)  # (2 min_len <= max_len: every T >= min_len is feasible)
    if T <= 10:  # the same set by brute force over all subsets of the interior frames
        n = sum(1 for k in range(T) for inner in itertools.combinations(range(1, T), k)
                if all(min_len <= b - a <= max_len for a, b in zip([0, *inner], [*inner, T])))
        assert n == len(keys)
    best = min(keys)
    return best[0], best[1][::-1]


def small_search_cases(n=400, seed=11):
    """(S, lam, min_len, max_len): T <= 14, min_len 1..3, max_len in [2 min_len, 2 min_len + 3], S and lam in 0..2."""
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        min_len = int(rs.randint(1, 4))
        max_len = 2 * min_len + int(rs.randint(0, 4))
        T = int(rs.randint(0, 15))
        out.append((rs.randint(0, 3, T).astype(np.int64), int(rs.randint(0, 3)), min_len, max_len))
    return out


def samples_for(T, extra=0):
    """A sample count that gives T frames (0: too short for one)."""
    return WIN - 1 if T == 0 else WIN + (T - 1) * HOP + extra


def burst_pause(T, seed, burst=23, pause=6, loud=6000, quiet=4):
    """Noise bursts of ``burst`` frames and near-silence of ``pause`` frames in turn (the lengths jitter)."""
    rs = np.random.RandomState(seed)
    n = samples_for(T, int(rs.randint(0, HOP)))
    x = np.zeros(n, np.int16)
    at, on = 0, True
    while at < n:
        m = HOP * int((burst if on else pause) * rs.uniform(0.6, 1.4) + 1)
        a = loud if on else quiet
        x[at:at + m] = rs.randint(-a, a + 1, min(m, n - at))
        at, on = at + m, not on
    return x


def white_noise(T, seed, amp=3000):
    rs = np.random.RandomState(seed)
    return rs.randint(-amp, amp + 1, samples_for(T, int(rs.randint(0, HOP)))).astype(np.int16)


MIN_LEN, MAX_LEN, SMOOTH, PAD = 12, 40, 3, 2


def ragged_batch():
    """[(name, int16 samples)] for min_len 12, max_len 40: every length at which the kernels take another path."""
    rec = [("n<win", np.full(WIN - 1, 1000, np.int16)), ("T=1", white_noise(1, 1)), ("T=min_len-1", white_noise(MIN_LEN - 1, 2)),
           ("T=max_len", burst_pause(MAX_LEN, 3)), ("T=max_len+1", burst_pause(MAX_LEN + 1, 4))]
    for T in (47, 48, 49, 63, 64, 65, 95, 96, 97):  # around multiples of min_len (48), of the chunk (64) and of both (96)
        rec.append((f"T={T}", burst_pause(T, 10 + T, burst=9, pause=4)))
        assert T % MIN_LEN in (0, 1, MIN_LEN - 1) or T % CHUNK in (0, 1, CHUNK - 1)
    rec += [("zeros", np.zeros(samples_for(100, 7), np.int16)), ("all -32768", np.full(samples_for(100), -32768, np.int16)),
            ("bursts", burst_pause(300, 5)), ("white noise", white_noise(300, 6)), ("empty", np.zeros(0, np.int16))]
    return rec
