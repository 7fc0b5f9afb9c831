#!/usr/bin/env python3
"""Golden vectors of Griffin-Lim at the geometry stage 3 of the recipe writes (n_fft 1200 / window 1024 / hop 300) from the
REFERENCE's own ``GriffinLim`` (fairseq/models/text_to_speech/vocoder.py:49-110), on the CPU (build container only):

    python tools/gen_golden_gl_1200.py

writes tests/golden/infer_gl_1200.npz.  TEST INFRASTRUCTURE: needs the reference checkout; nothing on the GPU machine does.
The arrangement of tools/gen_golden_audio_features.py: ``gen_golden`` (oracle/) sets up the reference import path; nothing
under oracle/ changes.

Inputs as in tests/golden/infer_gl_2048.npz (oracle/gen_golden_vocoder.py), 23 frames:
``spec = |RandomState(spec_seed).randn(601, 23)|``, the phases from numpy's global stream seeded with ``phase_seed`` -- the
tests regenerate both.  Stored for n_iter 1 and 8:
  * ``wave.n``:   the reference's fp32 waveform;
  * ``sc.n``:     its spectral convergence || |STFT(wave)| - spec || / || spec ||;
  * ``margin.n``: max |wave - float64 numpy-FFT evaluation of the same iterations| / max |wave| -- the reference's OWN
    rounding, which the tests' bound is a multiple of (``_gl_numpy_fft`` of tests/test_inference.py is that evaluation).
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.argv = [sys.argv[0]]
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import gen_golden as GG  # noqa: E402,F401  (sets up the reference import path + its stand-ins)
import infer_oracle as IO  # noqa: E402
from fairseq.models.text_to_speech.vocoder import GriffinLim  # noqa: E402
from test_inference import _gl_numpy_fft  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "infer_gl_1200.npz")
N_FFT, WIN, HOP, T = 1200, 1024, 300, 23
SPEC_SEED, PHASE_SEED = 1200, 17


def main():
    Fq = N_FFT // 2 + 1
    spec = np.abs(np.random.RandomState(SPEC_SEED).randn(Fq, T)).astype(np.float32)
    rec = {"spec_seed": SPEC_SEED, "phase_seed": PHASE_SEED, "n_fft": N_FFT, "win": WIN, "hop": HOP, "T": T}
    for n_iter in (1, 8):
        gl = GriffinLim(N_FFT, WIN, HOP, n_iter)
        np.random.seed(PHASE_SEED)
        wave = gl(torch.from_numpy(spec))
        assert wave.dtype == torch.float32 and wave.shape == (HOP * (T - 1),)
        ang = IO.initial_angles((Fq, T), np.random.RandomState(PHASE_SEED))  # the same draws, as the reference casts them
        w64 = _gl_numpy_fft(spec, ang, N_FFT, WIN, HOP, n_iter)
        scale = float(wave.abs().max())
        margin = float(np.abs(wave.numpy().astype(np.float64) - w64).max()) / scale
        mag, _ = IO.gl_transform(wave.unsqueeze(0), N_FFT, WIN, HOP)
        sc = float((mag[0] - torch.from_numpy(spec)).norm() / torch.from_numpy(spec).norm())
        rec[f"wave.{n_iter}"] = wave.numpy()
        rec[f"sc.{n_iter}"] = np.float64(sc)
        rec[f"margin.{n_iter}"] = np.float64(margin)
        print(f"GL 1200 n_iter {n_iter}: wave scale {scale:.3f}, reference fp32 vs float64 {margin:.2e}, spectral convergence {sc:.5f}")
    np.savez_compressed(OUT, **rec)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
