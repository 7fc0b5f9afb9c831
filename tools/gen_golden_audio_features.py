#!/usr/bin/env python3
"""Golden vectors of the stage 3 log-mel extraction from the REFERENCE's own classes, on the CPU (build container only):

    python tools/gen_golden_audio_features.py

writes tests/golden/audio_features.npz.  TEST INFRASTRUCTURE: needs the reference checkout; nothing on the GPU machine does.

Per geometry of tests/audio_feat_synth.py (three power-of-two n_fft for the FFT kernels, and the stage's default n_fft 1200
for the dense route) and per seeded input length:
  * ``extract_logmel_spectrogram`` (examples/speech_synthesis/data_utils.py:46-76: ``TTSSpectrogram`` + ``get_window``,
    ``TTSMelScale``, fairseq/data/audio/audio_utils.py:218-290) in fp32.  ``TTSMelScale`` asks librosa for its table; librosa is
    absent, so the table stand-in ``oracle/ref_shims_tables`` goes on THIS generator's ``sys.path`` (the arrangement of
    oracle/gen_golden_vocoder.py): the Slaney table itself stays "parity unpinned", the reference code around it is pinned.
  * ``ref_f64_err``: the largest log-domain difference between that fp32 result and a float64 numpy evaluation of the same
    definition -- the reference's own rounding error, which the tests' bound is a multiple of -- and the smallest mel value
    (the tests compare where the golden mel value is >= 1e-4 and assert that this is everywhere).
  * the fingerprint of every input (the tests regenerate the inputs from the recipe).
  * ``get_global_cmvn`` (speech_synthesis/data_utils.py:190-215), ``create_zip`` and ``get_zip_manifest``
    (speech_to_text/data_utils.py:101-132) on the geometry's arrays saved as .npy files.  Their module imports ``soundfile``,
    which is absent: an EMPTY module object of that name is put into ``sys.modules`` here for the import alone (none of the
    three functions touches it); ``helpers`` records how they were imported.
The Kaldi filter bank has no reference in this image (torchaudio is absent): its yardsticks stay oracle/data_oracle.py:
kaldi_fbank_f64 and the host ``kaldi_fbank``; nothing about it is stored here.
"""
import os
import sys
import tempfile
import types
from pathlib import Path

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.argv = [sys.argv[0]]
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "oracle", "ref_shims_tables")):
    sys.path.insert(0, p)
import gen_golden as GG  # noqa: E402,F401  (sets up the reference import path + its stand-ins)
import audio_feat_synth as AS  # noqa: E402
from fairseq.data.audio.audio_utils import TTSMelScale, TTSSpectrogram, get_window  # noqa: E402

helpers = "direct"
try:
    from examples.speech_synthesis.data_utils import extract_logmel_spectrogram, get_global_cmvn  # noqa: E402
    from examples.speech_to_text.data_utils import create_zip, get_zip_manifest  # noqa: E402
except ImportError as e:
    if "soundfile" not in str(e):
        raise
    helpers = "with an empty stand-in module for soundfile"
    sys.modules.setdefault("soundfile", types.ModuleType("soundfile"))
    from examples.speech_synthesis.data_utils import extract_logmel_spectrogram, get_global_cmvn  # noqa: E402
    from examples.speech_to_text.data_utils import create_zip, get_zip_manifest  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "audio_features.npz")


def logmel_f64(wave, g, n_mels, eps=1e-5):
    """The same definition in float64: reflect padding, frames, the reference's window and mel table (their fp32 values),
    an exact DFT, magnitude, mel projection, log(clamp)."""
    n_fft, win, hop, sr, f_min, f_max = g
    window = get_window(torch.hann_window, n_fft, win).double().numpy()
    mel = TTSMelScale(n_mels=n_mels, sample_rate=sr, f_min=f_min, f_max=f_max, n_stft=n_fft // 2 + 1).basis.double().numpy()
    x = np.pad(wave.astype(np.float64), (n_fft // 2, n_fft // 2), mode="reflect")
    T = 1 + wave.shape[0] // hop
    frames = np.stack([x[t * hop: t * hop + n_fft] for t in range(T)])
    mag = np.abs(np.fft.rfft(frames * window[None, :], axis=1))
    m = mag @ mel.T
    return np.log(np.maximum(m, eps)), m


def main():
    rec = {"helpers": helpers, "n_mels": AS.N_MELS}
    for g in AS.LOGMEL_GEOMETRIES:
        n_fft, win, hop, sr, f_min, f_max = g
        key = AS.geometry_key(g)
        waves = AS.logmel_inputs(g)
        # the classes the issue names, once directly (shape / window check), then through the reference's own wrapper
        spec = TTSSpectrogram(n_fft=n_fft, win_length=win, hop_length=hop, window_fn=torch.hann_window)
        assert spec.basis.shape == (2 * (n_fft // 2 + 1), 1, n_fft)
        err, min_mel, feats = 0.0, np.inf, []
        for j, w in enumerate(waves):
            y = extract_logmel_spectrogram(torch.from_numpy(w)[None, :], sr, None, win_length=win, hop_length=hop, n_fft=n_fft,
                                           n_mels=AS.N_MELS, f_min=f_min, f_max=f_max)
            y = y.numpy().astype(np.float32).reshape(-1, AS.N_MELS)  # (a one-frame result is squeezed to 1-D there)
            assert y.shape[0] == 1 + w.shape[0] // hop, (y.shape, w.shape)
            y64, m64 = logmel_f64(w, g, AS.N_MELS)
            err = max(err, float(np.abs(y - y64).max()))
            min_mel = min(min_mel, float(m64.min()))
            rec[f"{key}.logmel.{j}"] = y
            rec[f"{key}.fp.{j}"] = AS.fingerprint([w])
            feats.append(y)
        rec[f"{key}.ref_f64_err"] = np.float64(err)
        rec[f"{key}.min_mel"] = np.float64(min_mel)
        assert min_mel >= 1e-4, (g, min_mel)  # no value near the clamp: the comparison leaves out nothing
        with tempfile.TemporaryDirectory() as d:
            root = Path(d) / "feat"
            root.mkdir()
            for j, y in enumerate(feats):
                np.save((root / f"utt{j}.npy").as_posix(), y)
            stats = get_global_cmvn(root, Path(d) / "gcmvn.npz")
            stats = stats if isinstance(stats, dict) else dict(np.load(Path(d) / "gcmvn.npz"))
            rec[f"{key}.cmvn_mean"] = np.asarray(stats["mean"], dtype=np.float32)
            rec[f"{key}.cmvn_std"] = np.asarray(stats["std"], dtype=np.float32)
            zpath = Path(d) / "feat.zip"
            create_zip(root, zpath)
            paths, lengths = get_zip_manifest(zpath)
            import zipfile
            with zipfile.ZipFile(zpath) as z:
                order = [Path(i.filename).stem for i in z.infolist()]
                assert all(i.compress_type == zipfile.ZIP_STORED for i in z.infolist())
            rec[f"{key}.zip_order"] = np.asarray(order)
            rec[f"{key}.zip_offset"] = np.asarray([int(paths[k].split(":")[-2]) for k in order], dtype=np.int64)
            rec[f"{key}.zip_size"] = np.asarray([int(paths[k].split(":")[-1]) for k in order], dtype=np.int64)
            rec[f"{key}.zip_frames"] = np.asarray([int(lengths[k]) for k in order], dtype=np.int64)
        print(f"{key}: {sum(f.shape[0] for f in feats)} frames, ref_f64_err {err:.3e}, smallest mel value {min_mel:.3e}")
    np.savez_compressed(OUT, **rec)
    print("wrote", OUT, os.path.getsize(OUT), "bytes; reference helpers imported:", helpers)


if __name__ == "__main__":
    main()
