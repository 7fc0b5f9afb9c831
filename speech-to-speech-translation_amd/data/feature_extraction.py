"""Stage 3 feature extraction on the device (csrc/features.hip): the Kaldi filter bank of the source audio and the log-mel
spectrogram of the target audio, for whole batches of utterances, with the per-utterance moments the global CMVN statistics
are made of.

Counterpart of ``examples/speech_to_text/data_utils.py:73-98`` (``extract_fbank_features``),
``examples/speech_synthesis/data_utils.py:46-76`` (``extract_logmel_spectrogram``) and ``:190-215`` (``get_global_cmvn``).

The tables come from the code that owns them: ``audio_utils._kaldi_tables`` (povey window, Kaldi mel banks),
``vocoder.get_window`` / ``get_fourier_basis`` / ``slaney_mel_filters``.  The filter bank is the operator ``audio_utils.kaldi_fbank``
documents -- parity with torchaudio itself unpinned, as there.  The host functions below (``host_fbank``, ``host_logmel``) are
the per-utterance numpy forms the stage runs with ``--extractor host``.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np
import torch

from ..runtime import binding as bd
from . import audio_utils

FBANK_EPS = float(np.finfo(np.float32).eps)


def logmel_frames(n: int, hop_length: int) -> int:
    return 1 + n // hop_length


def _ranges(rows: np.ndarray) -> np.ndarray:
    """[n][2] int32: first non-zero column and one past the last one of each filter row (an all-zero row: 0, 0)."""
    out = np.zeros((rows.shape[0], 2), np.int32)
    for b, r in enumerate(rows):
        nz = np.flatnonzero(r)
        if nz.size:
            out[b] = (nz[0], nz[-1] + 1)
    return out


def _twiddles(n: int) -> np.ndarray:
    j = np.arange(n, dtype=np.float64)
    return np.stack([np.cos(2 * np.pi * j / n), -np.sin(2 * np.pi * j / n)], axis=1).astype(np.float32)


def _check_logmel_lengths(waves, n_fft: int):
    for w in waves:
        if w.shape[0] <= n_fft // 2:
            # torch's reflect padding (TTSSpectrogram.forward) refuses it: the padding must be smaller than the input
            raise ValueError(f"log-mel: a waveform of {w.shape[0]} samples is too short for reflect padding by n_fft // 2 = "
                             f"{n_fft // 2} (it must have more than {n_fft // 2})")


def _as_waves(waves) -> List[np.ndarray]:
    out = []
    for w in waves:
        w = np.ascontiguousarray(np.asarray(w, dtype=np.float32))
        if w.ndim != 1:
            raise ValueError("feature extraction takes 1-D waveforms (channel 0 / mono)")
        out.append(w)
    return out


def logmel_tables(sample_rate: int, n_fft: int, win_length: int, n_mels: int, f_min: float, f_max: float):
    """(window [n_fft] fp32, mel [n_mels][n_fft // 2 + 1] fp32) of TTSSpectrogram / TTSMelScale."""
    from ..vocoder import get_window, slaney_mel_filters
    return (get_window(n_fft, win_length).numpy().astype(np.float32),
            np.ascontiguousarray(slaney_mel_filters(sample_rate, n_fft, n_mels, f_min, f_max).numpy(), dtype=np.float32))


def host_fbank(wave: np.ndarray, sample_rate: float, n_bins: int = 80) -> np.ndarray:
    return audio_utils.kaldi_fbank(np.asarray(wave, dtype=np.float32), sample_rate, n_bins)


def host_logmel(wave: np.ndarray, sample_rate: int, n_fft: int, win_length: int, hop_length: int, n_mels: int, f_min: float,
                f_max: float, eps: float = 1e-5) -> np.ndarray:
    """``extract_logmel_spectrogram`` for one utterance in numpy (fp32 data, numpy's FFT): [1 + N // hop, n_mels]."""
    wave = np.asarray(wave, dtype=np.float32)
    _check_logmel_lengths([wave], n_fft)
    win, mel = logmel_tables(sample_rate, n_fft, win_length, n_mels, f_min, f_max)
    x = np.pad(wave, (n_fft // 2, n_fft // 2), mode="reflect")
    T = logmel_frames(wave.shape[0], hop_length)
    frames = np.lib.stride_tricks.as_strided(x, shape=(T, n_fft), strides=(hop_length * x.strides[0], x.strides[0]))
    spec = np.fft.rfft(frames * win[None, :], axis=1)
    mag = np.sqrt(spec.real.astype(np.float32) ** 2 + spec.imag.astype(np.float32) ** 2).astype(np.float32)
    return np.log(np.maximum(mag @ mel.T, np.float32(eps))).astype(np.float32)


def host_moments(feats: Sequence[np.ndarray]) -> np.ndarray:
    """[U][2][n_bins] float32: column sums and column sums of squares per utterance (float64 accumulation)."""
    return np.stack([np.stack([f.sum(axis=0, dtype=np.float64), (f.astype(np.float64) ** 2).sum(axis=0)]).astype(np.float32)
                     for f in feats]) if len(feats) else np.zeros((0, 2, 0), np.float32)


def global_cmvn(moments: np.ndarray, n_frames: int) -> Tuple[np.ndarray, np.ndarray]:
    """``get_global_cmvn``'s formula (speech_synthesis/data_utils.py:211-214) from per-utterance moments, folded in float64:
    mean = sum x / n, std = sqrt(max(sum x^2 / n - mean^2, 1e-10))."""
    m = np.asarray(moments, dtype=np.float64).sum(axis=0)
    mean = m[0] / n_frames
    var = m[1] / n_frames - mean ** 2
    return mean.astype(np.float32), np.sqrt(np.maximum(var, 1e-10)).astype(np.float32)


class DeviceFeatureExtractor:
    """``fbank`` / ``logmel`` of lists of 1-D waveforms on ``device``.  Utterances are taken in order into batches of at most
    ``max_samples`` padded samples (U x longest); a batch is one upload, the kernels, and ONE copy back (features and moments
    in one buffer).  A frame's bits do not depend on the batch it was extracted in.  ``fbank_batch`` is the inference form:
    the normalised, padded encoder input of a batch, left on the device.

    ``fft``: the log-mel spectrogram goes through the LDS FFT kernel where the library has a plan for n_fft (256 ... 2048 and
    240 / 400 / 1200, the stage's default); ``False`` forces the dense bf16x3 product that every other n_fft takes (A/B runs)."""

    def __init__(self, device=None, max_samples: int = 1 << 24, fft: bool = True):
        if device is None:
            device = torch.device("cpu") if bd.is_emulator() else torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        self.max_samples = int(max_samples)
        self.fft = bool(fft)
        self._tabs = {}

    # ---- tables -------------------------------------------------------------------------------------------------------
    def _dev(self, a: np.ndarray) -> torch.Tensor:
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.device)

    def _fbank_tables(self, sample_rate: float, n_bins: int):
        key = ("fbank", float(sample_rate), n_bins)
        t = self._tabs.get(key)
        if t is None:
            shift, size, padded, window, banks_t = audio_utils._kaldi_tables(float(sample_rate), n_bins, 25.0, 10.0, 20.0, 0.0)
            if padded not in (256, 512, 1024, 2048):
                raise bd.S2STHipError(f"fbank: no FFT kernel for frames padded to {padded} samples (sample rate {sample_rate})")
            banks = np.ascontiguousarray(banks_t.T)
            t = self._tabs[key] = (shift, size, padded, self._dev(window), self._dev(_twiddles(padded)), self._dev(banks),
                                   self._dev(_ranges(banks)))
        return t

    def _logmel_tables(self, sample_rate, n_fft, win_length, n_mels, f_min, f_max):
        key = ("logmel", sample_rate, n_fft, win_length, n_mels, f_min, f_max)
        t = self._tabs.get(key)
        if t is None:
            win, mel = logmel_tables(sample_rate, n_fft, win_length, n_mels, f_min, f_max)
            use_fft = self.fft and bool(bd.lib().s2st_fft_len_supported_i32(int(n_fft)))
            t = {"mel": self._dev(mel), "range": self._dev(_ranges(mel)), "fft": use_fft}
            if use_fft:
                t["win"], t["tw"] = self._dev(win), self._dev(_twiddles(n_fft))
            else:
                # the dense route of GriffinLim._transform: windowed Fourier basis, bf16x3 [hi | hi | lo] along the contraction
                from ..vocoder import get_fourier_basis
                if n_fft % 4:
                    raise bd.S2STHipError("log-mel: n_fft must be a multiple of 4")
                F = n_fft // 2 + 1
                Fp = (F + 15) // 16 * 16
                basis = get_fourier_basis(n_fft) * torch.from_numpy(win)
                fwd = torch.zeros(2 * Fp, n_fft)
                fwd[:F] = basis[:F]
                fwd[Fp:Fp + F] = basis[F:]
                hi = fwd.to(torch.bfloat16)
                lo = (fwd - hi.float()).to(torch.bfloat16)
                t["fwd3"], t["Fp"] = torch.cat([hi, hi, lo], dim=1).contiguous().to(self.device), Fp
            self._tabs[key] = t
        return t

    # ---- batching -----------------------------------------------------------------------------------------------------
    def _batches(self, lens: List[int]):
        start, longest = 0, 0
        for i, n in enumerate(lens):
            new_longest = max(longest, n, 1)
            if i > start and new_longest * (i - start + 1) > self.max_samples:
                yield start, i
                start, new_longest = i, max(n, 1)
            longest = new_longest
        if start < len(lens):
            yield start, len(lens)

    def _run(self, waves, frames_of, n_bins: int, launch):
        waves = _as_waves(waves)
        lens = [int(w.shape[0]) for w in waves]
        feats: List[np.ndarray] = []
        moments = np.zeros((len(waves), 2, n_bins), np.float32)
        for b0, b1 in self._batches(lens):
            U, Lmax = b1 - b0, max(max(lens[b0:b1]), 1)
            Ts = [frames_of(n) for n in lens[b0:b1]]
            rows, pairs = sum(Ts), sum((t + 1) // 2 for t in Ts)
            host = torch.zeros(U, Lmax, dtype=torch.float32)
            for u in range(U):
                host[u, :lens[b0 + u]] = torch.from_numpy(waves[b0 + u])
            wave = host.to(self.device)
            bd.require_device(wave)
            ln = torch.tensor(lens[b0:b1], dtype=torch.int32).to(self.device)
            offs = torch.empty(2, U + 1, dtype=torch.int32, device=self.device)
            # features [rows][n_bins], then moments [U][2][n_bins]: one buffer, one copy back
            out = torch.empty(rows * n_bins + U * 2 * n_bins, dtype=torch.float32, device=self.device)
            launch(wave, ln, out, offs, U, Lmax, rows, pairs)
            bd.call("s2st_feature_moments_f32", out, offs, out[rows * n_bins:], U, n_bins)
            res = out.cpu().numpy()
            r = 0
            for u, t in enumerate(Ts):
                feats.append(res[r * n_bins:(r + t) * n_bins].reshape(t, n_bins).copy())
                r += t
            moments[b0:b1] = res[rows * n_bins:].reshape(U, 2, n_bins)
        return feats, moments

    def moments(self, feats: Sequence[np.ndarray]) -> np.ndarray:
        """[U][2][n_bins] float32 column sums and column sums of squares of ready-made [T_u, n_bins] float32 arrays."""
        U = len(feats)
        if U == 0:
            return np.zeros((0, 2, 0), np.float32)
        n_bins = int(feats[0].shape[1])
        offs = np.zeros(U + 1, np.int32)
        offs[1:] = np.cumsum([f.shape[0] for f in feats])
        x = self._dev(np.concatenate([np.asarray(f, dtype=np.float32).reshape(-1, n_bins) for f in feats] +
                                     [np.zeros((1, n_bins), np.float32)]))
        bd.require_device(x)
        mom = torch.empty(U, 2, n_bins, dtype=torch.float32, device=self.device)
        bd.call("s2st_feature_moments_f32", x, self._dev(offs), mom, U, n_bins)
        return mom.cpu().numpy()

    # ---- the two extractors ---------------------------------------------------------------------------------------------
    def fbank(self, waves, sample_rate, n_bins: int = 80):
        """Waveforms in the 16-bit range -> ([T_u, n_bins] float32 per utterance, moments [U][2][n_bins])."""
        shift, size, padded, win, tw, banks, rng = self._fbank_tables(sample_rate, n_bins)

        def launch(wave, ln, out, offs, U, Lmax, rows, pairs):
            bd.call("s2st_fbank_kaldi_f32", wave, ln, win, tw, banks, rng, out, offs, U, Lmax, size, shift, padded, n_bins,
                    FBANK_EPS, pairs, rows)

        return self._run(waves, lambda n: 0 if n < size else 1 + (n - size) // shift, n_bins, launch)

    def fbank_batch(self, waves, sample_rate, mean, std, n_bins: int = 80, Tmax=None, out=None):
        """The filter bank of a ragged batch as the speech encoder's input (``s2st_fbank_kaldi_batch_f32``): returns
        ``(src [U, Tmax, n_bins] fp32, frames [U] int64)``, both on the device.  Row ``t < frames[u]`` of utterance ``u`` is
        ``(fbank - mean) / std`` with the bits ``_GlobalCMVN.__call__`` gives on ``fbank()``'s rows, the rows behind are +0.0
        as ``_collate_frames`` pads them; the kernel writes every element of ``src``.  ``mean`` / ``std``: [n_bins] fp32
        (device tensors are used as they are).  ``Tmax`` (default: the longest utterance's frames) may ask for more
        padding; ``out`` may supply the output tensor.

        ``waves``: 1-D arrays in the 16-bit range, all ``int16`` (uploaded as int16 and widened on the device:
        ``float(int16)`` is exactly the stage-3 value ``(x / 32768) * 2**15``), or float32 -- or 1-D fp32 tensors already
        on the device (resampled audio), which are not uploaded at all.  One upload carries the samples and the lengths;
        nothing comes back to the host."""
        shift, size, padded, win, tw, banks, rng = self._fbank_tables(sample_rate, n_bins)
        dev = self.device
        U = len(waves)
        lens = [int(w.shape[0]) for w in waves]
        for w in waves:
            if len(w.shape) != 1:
                raise ValueError("feature extraction takes 1-D waveforms (channel 0 / mono)")
        Ts = [0 if n < size else 1 + (n - size) // shift for n in lens]
        T = max(Ts, default=0)
        if Tmax is None:
            Tmax = T
        if Tmax < T:
            raise ValueError(f"fbank_batch: Tmax {Tmax} is smaller than the longest utterance's {T} frames")
        Lmax = max(max(lens, default=0), 1)
        hdr = np.asarray(lens, dtype=np.int32)
        if U and all(torch.is_tensor(w) for w in waves):
            ln = torch.from_numpy(hdr).to(dev)
            wave = torch.zeros(U, Lmax, dtype=torch.float32, device=dev)
            for u, w in enumerate(waves):
                wave[u, :lens[u]] = w.to(dev, torch.float32)
        else:
            # ONE host buffer: the lengths (int32, bit-cast to the samples' type), then the padded samples
            dt = np.int16 if U and all(isinstance(w, np.ndarray) and w.dtype == np.int16 for w in waves) else np.float32
            h = hdr.view(dt)
            host = np.zeros(h.size + U * Lmax, dt)
            host[:h.size] = h
            rows = host[h.size:].reshape(U, Lmax)
            for u, w in enumerate(waves):
                rows[u, :lens[u]] = np.asarray(w, dtype=dt)
            d = torch.from_numpy(host).to(dev)
            ln = d[:h.size].view(torch.int32)
            wave = d[h.size:].view(U, Lmax).to(torch.float32)  # (int16: widened on the device)
        mean, std = (x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)) for x in (mean, std))
        mean, std = mean.to(dev, torch.float32).contiguous(), std.to(dev, torch.float32).contiguous()
        if mean.numel() != n_bins or std.numel() != n_bins:
            raise ValueError(f"fbank_batch: mean / std must hold {n_bins} values")
        if out is None:
            out = torch.empty(U, Tmax, n_bins, dtype=torch.float32, device=dev)
        elif tuple(out.shape) != (U, Tmax, n_bins) or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError(f"fbank_batch: out must be a contiguous fp32 tensor of shape {(U, Tmax, n_bins)}")
        if U:
            bd.require_device(wave)
            offs = torch.empty(2, U + 1, dtype=torch.int32, device=dev)
            bd.call("s2st_fbank_kaldi_batch_f32", wave, ln, win, tw, banks, rng, mean, std, out, offs, U, Lmax, Tmax, size, shift,
                    padded, n_bins, FBANK_EPS, sum((t + 1) // 2 for t in Ts))
            n = ln.to(torch.int64)
            frames = torch.where(n < size, torch.zeros_like(n), 1 + torch.div(n - size, shift, rounding_mode="floor"))
        else:
            frames = torch.zeros(0, dtype=torch.int64, device=dev)
        return out, frames

    def logmel(self, waves, sample_rate, n_fft, win_length, hop_length, n_mels, f_min, f_max, eps: float = 1e-5):
        """Waveforms in [-1, 1] -> ([1 + N_u // hop, n_mels] float32 per utterance, moments [U][2][n_mels])."""
        waves = _as_waves(waves)
        _check_logmel_lengths(waves, n_fft)
        t = self._logmel_tables(int(sample_rate), int(n_fft), int(win_length), int(n_mels), float(f_min), float(f_max))

        def launch(wave, ln, out, offs, U, Lmax, rows, pairs):
            if t["fft"]:
                bd.call("s2st_logmel_f32", wave, ln, t["win"], t["tw"], t["mel"], t["range"], out, offs, U, Lmax, n_fft,
                        hop_length, n_mels, float(eps), pairs, rows)
                return
            F, Fp = n_fft // 2 + 1, t["Fp"]
            As = torch.empty(max(rows, 1), 3 * n_fft, dtype=torch.bfloat16, device=self.device)
            bd.call("s2st_logmel_frame_split_f32", wave, ln, As, offs, U, Lmax, n_fft, hop_length, rows)
            if rows == 0:
                return
            Y = torch.empty(rows, 2 * Fp, dtype=torch.float32, device=self.device)
            bd.gemm(As, t["fwd3"], Y, rows, 2 * Fp, 3 * n_fft)
            bd.call("s2st_logmel_from_stft_f32", Y, t["mel"], t["range"], out, rows, F, Fp, n_mels, float(eps))

        return self._run(waves, lambda n: logmel_frames(n, hop_length), n_mels, launch)
