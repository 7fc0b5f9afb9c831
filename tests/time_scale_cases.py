"""Cases for tests/test_time_scale.py: the definition of include/s2st_hip.h (s2st_time_scale_pcm16) once more as plain loops over
Python ints -- it shares nothing with the package -- small seeded cases in which equal costs abound, and the ragged batches the
device form is compared on."""
import numpy as np

EXTREMES = np.array([-32768, -1, 0, 1, 32767], dtype=np.int16)


def scalar_time_scale(x, m, N, D):
    """(out, positions, hops in which two candidates shared the least cost): hop by hop, candidate by candidate, term by term."""
    x = [int(v) for v in x]
    n, Hs = len(x), N // 2
    J = -(-m // Hs)

    def at(t):
        return x[t] if 0 <= t < n else 0

    out, pos, tied = [0] * (J * Hs), [0] * J, 0
    for i in range(Hs if J else 0):
        out[i] = at(i)
    for j in range(1, J):
        a = (j * Hs * n) // m
        tpl = [at(pos[j - 1] + Hs + i) for i in range(Hs)]
        best = None
        for c in range(a - D, a + D + 1):
            cost = 0
            for i in range(Hs):
                cost += abs(at(c + i) - tpl[i])
            key = (cost, abs(c - a), c)
            if best is not None and key[0] == best[0]:
                ties_here = True
            elif best is None or key[0] < best[0]:
                ties_here = False
            if best is None or key < best:
                best = key
        tied += ties_here
        pos[j] = best[2]
        for i in range(Hs):
            wr = ((2 * i + 1) * 32768) // N
            out[j * Hs + i] = (at(best[2] + i) * wr + tpl[i] * (32768 - wr) + 16384) >> 15  # (Python's >> floors: arithmetic)
    return np.array(out[:m], dtype=np.int16), np.array(pos, dtype=np.int32), tied


def small_cases(count, seed=5):
    """[(x, m, N, D)]: N in {2, 4, 8, 16}, D in 0 .. 9, n and m in 0 .. 80 (n < N, m < Hs and m no multiple of Hs among them);
    samples from the extremes of int16 or short square waves."""
    rs = np.random.RandomState(seed)
    cases = []
    for t in range(count):
        N = (2, 4, 8, 16)[t % 4]
        D = (t // 4) % 10
        small = t % 7 == 0
        n = int(rs.randint(0, N + 1 if small else 81))
        m = int(rs.randint(0, N // 2 + 2 if t % 11 == 0 else 81))
        if t % 3 == 0:
            x = EXTREMES[rs.randint(0, len(EXTREMES), n)]
        else:  # a square wave: half-period 1 .. 6, amplitude from the extremes, a few samples flipped
            half, amp = int(rs.randint(1, 7)), int(EXTREMES[rs.randint(0, len(EXTREMES))])
            x = np.where((np.arange(n) // half) % 2 == 0, amp, -1 - amp).astype(np.int16)
            for _ in range(int(rs.randint(0, 3))):
                if n:
                    x[rs.randint(0, n)] = EXTREMES[rs.randint(0, len(EXTREMES))]
        cases.append((np.ascontiguousarray(x, dtype=np.int16), m, N, D))
    return cases


def noise_tone(n, seed, period=80, amp=9000):
    """Seeded noise on a tone: what speech looks like to a sum of absolute differences."""
    rs = np.random.RandomState(seed)
    t = np.arange(n)
    return np.clip(amp * np.sin(2 * np.pi * t / period) + rs.randint(-1500, 1501, n), -32768, 32767).astype(np.int16)


def periodic(n, period, seed):
    """An exactly periodic recording: one seeded period of noise, repeated."""
    s = np.random.RandomState(seed).randint(-20000, 20001, period).astype(np.int16)
    return s[np.arange(n) % period]


def ragged_batch(N, D, max_hops, period):
    """[(name, x, m)] for the geometry (N, D): every n / m within [1/2, 2]; the longest output has ``max_hops`` hops.
    ``period``: odd, <= D -- the recording whose best candidates sit at odd offsets."""
    Hs = N // 2
    n0 = max_hops * Hs // 2 - 3
    rec = [("empty", np.zeros(0, np.int16), 0),
           ("n=1", np.array([-7], np.int16), 1),
           ("n=1 to 2", np.array([32767], np.int16), 2),
           ("n=2 to m=1", np.array([5, -32768], np.int16), 1),
           ("n=N-1", noise_tone(N - 1, 1), N - 1),
           ("n=N to Hs+1", noise_tone(N, 2), Hs + 1),
           ("n=N stretched twice", noise_tone(N, 3), 2 * N),
           ("n=Hs to Hs-1", noise_tone(Hs, 4), Hs - 1),
           ("n=Hs to Hs+1", noise_tone(Hs, 5), Hs + 1),
           ("ratio 1/2", noise_tone(n0, 6), 2 * n0),
           ("ratio 1", noise_tone(n0, 7), n0),
           ("ratio 1.25", noise_tone(n0, 8), -(-n0 * 1000 // 1250)),
           ("ratio 2", noise_tone(n0, 9), (n0 + 1) // 2),
           ("zeros", np.zeros(n0, np.int16), -(-n0 * 1000 // 1250)),
           ("all -32768", np.full(n0, -32768, np.int16), -(-n0 * 1000 // 1250)),
           ("all 32767", np.full(n0 // 2, 32767, np.int16), n0 - 1),
           ("odd period", periodic(n0, period, 10), -(-n0 * 1000 // 1250)),
           ("odd period stretched", periodic(n0 // 2, period, 11), n0 // 2 * 3 // 2 + 1)]
    return rec
