"""Seeded inputs of the feature-extraction tests (tests/test_feature_extraction.py) and of the generator of their golden
(tools/gen_golden_audio_features.py): the golden stores a fingerprint of every input, so a test that regenerates different
samples fails on the fingerprint, not on a mysterious feature difference.

The signal is two amplitude-modulated tones on a noise floor:

    x(t) = env(t) * (0.3 sin(2 pi 440 t) + 0.15 sin(2 pi 0.145 sr t + 1)) + 0.05 randn,  env(t) = 0.5 + 0.5 sin(2 pi 3 t + seed)

with ``numpy.random.RandomState(seed)``.  The noise floor is there on purpose: it keeps every mel bin far above the clamps
(log(1e-5) / log(float32 eps)), where a log amplifies fp32 cancellation without bound -- tones alone leave mel values near
3e-9 and a fp32-against-float64 difference of about 3e-3 in the log domain, this signal keeps both below 1e-3.
"""
import hashlib

import numpy as np

N_MELS = 80

# (n_fft, win_length, hop_length, sample_rate, f_min, f_max)
LOGMEL_FFT_GEOMETRIES = [(1024, 1024, 256, 22050, 0, 8000), (2048, 1200, 300, 24000, 20, 8000), (512, 400, 160, 16000, 0, 8000)]
LOGMEL_DENSE_GEOMETRY = (1200, 1024, 300, 24000, 20, 8000)  # the stage's default: not a power of two
LOGMEL_GEOMETRIES = LOGMEL_FFT_GEOMETRIES + [LOGMEL_DENSE_GEOMETRY]


def geometry_key(g) -> str:
    return "g" + "_".join(str(int(v)) for v in g)


def logmel_lengths(g, with_long: bool = True):
    """Shortest legal input, a ragged tail, a whole number of hops, one sample fewer, and about 0.9 s."""
    n_fft, _, hop, sr = g[:4]
    lens = [n_fft // 2 + 1, 7 * hop + 3, 8 * hop, 8 * hop - 1]
    return lens + [int(0.9 * sr) + 5] if with_long else lens


def signal(n: int, sample_rate: int, seed: int) -> np.ndarray:
    t = np.arange(n, dtype=np.float64) / sample_rate
    env = 0.5 + 0.5 * np.sin(2 * np.pi * 3 * t + seed)
    x = env * (0.3 * np.sin(2 * np.pi * 440 * t) + 0.15 * np.sin(2 * np.pi * 0.145 * sample_rate * t + 1))
    return (x + 0.05 * np.random.RandomState(seed).randn(n)).astype(np.float32)


def logmel_inputs(g, with_long: bool = True):
    return [signal(n, g[3], 100 + j) for j, n in enumerate(logmel_lengths(g, with_long))]


def fbank_input(n: int, sample_rate: int, seed: int) -> np.ndarray:
    """The 16-bit range with a DC offset, as integers (what a PCM file holds)."""
    return np.round(20000.0 * signal(n, sample_rate, seed).astype(np.float64) + 37.0).astype(np.float32)


def fingerprint(arrays) -> str:
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str(a.dtype).encode() + str(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()[:16]
