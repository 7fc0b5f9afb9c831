"""Griffin-Lim vocoder on the HIP path: the counterpart of
``fairseq/models/text_to_speech/vocoder.py:24-158`` (PseudoInverseMelScale, GriffinLim,
GriffinLimVocoder) with the same constructor arguments.

The reference's STFT / inverse STFT are dense-DFT contractions (conv1d / conv_transpose1d with Fourier bases,
audio_utils.py:259-271, vocoder.py:56-98).  Round 4: for power-of-two n_fft (256 ... 2048), and since the
mixed-radix plans of csrc/fft_lds.h for 240, 400 and 1200 (stage 3's default) too, they run as real FFTs in LDS
(csrc/griffin_lim.hip: the analysis basis is rfft(window * frame), the pseudo-inverse synthesis basis is window * hop / n_fft *
irfft -- exactly); other n_fft (and S2ST_GL_FFT=0) keep the dense form: one bf16 GEMM per transform over all utterances'
frames, the bf16x3 split folded into the contraction (phase retrieval is precision-sensitive), around small HIP kernels for
polar <-> rectangular conversion, framing of the reflect-padded waveforms and overlap-add.  Either way a single utterance is
a batch of one.  The constant tables
(window, Fourier bases and their pseudo-inverses, mel filterbank pseudo-inverse) are built once on
the host at construction, as the reference does in its ``register_buffer`` calls.  The uniform draws behind the initial
phases, and running them ahead of the decode, are phase_streams.py.

The mel filterbank comes from librosa in the reference (absent in this image, version un-pinned):
``slaney_mel_filters`` restates librosa.filters.mel's defaults (htk=False, norm='slaney').
"""
from __future__ import annotations

import os

import numpy as np
import torch
import torch.nn.functional as F

from .models.hifigan import HiFiGANVocoder  # noqa: F401  (--vocoder hifigan)
from .phase_streams import PhaseSource, _HostMTStream, _UniformStream  # noqa: F401  (re-exported)
from .runtime import binding as bd


def get_window(n_fft: int, win_length: int, window_fn=torch.hann_window) -> torch.Tensor:
    padding = n_fft - win_length
    assert padding >= 0
    return F.pad(window_fn(win_length), (padding // 2, padding - padding // 2))


def get_fourier_basis(n_fft: int) -> torch.Tensor:
    basis = np.fft.fft(np.eye(n_fft))
    basis = np.vstack([np.real(basis[:n_fft // 2 + 1, :]), np.imag(basis[:n_fft // 2 + 1, :])])
    return torch.from_numpy(basis).float()


def slaney_mel_filters(sample_rate: int, n_fft: int, n_mels: int, f_min: float, f_max: float) -> torch.Tensor:
    f_sp, min_log_hz, logstep = 200.0 / 3, 1000.0, np.log(6.4) / 27.0
    min_log_mel = min_log_hz / f_sp

    def hz_to_mel(f):
        f = np.asarray(f, dtype=np.float64)
        return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, 1e-10) / min_log_hz) / logstep, f / f_sp)

    def mel_to_hz(m):
        m = np.asarray(m, dtype=np.float64)
        return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)

    f_max = sample_rate / 2.0 if f_max is None else f_max
    fft_f = np.linspace(0, sample_rate / 2.0, 1 + n_fft // 2)
    mel_f = mel_to_hz(np.linspace(hz_to_mel(f_min), hz_to_mel(f_max), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fft_f[None, :]
    w = np.zeros((n_mels, 1 + n_fft // 2))
    for i in range(n_mels):
        w[i] = np.maximum(0, np.minimum(-ramps[i] / fdiff[i], ramps[i + 2] / fdiff[i + 1]))
    w *= (2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels]))[:, None]
    return torch.from_numpy(w.astype(np.float32))


def random_phases(n_freq: int, n_frames: int) -> np.ndarray:
    """The reference's initial phases np.angle(np.exp(2j*pi*np.random.rand(F, T))) (vocoder.py:101-102), same
    draws from numpy's global RNG: angle(exp(i th)) is th wrapped into (-pi, pi], computed without the
    complex exponential (the host-side cost of a long utterance is otherwise ~10 ms)."""
    th = 2.0 * np.pi * np.random.rand(n_freq, n_frames)
    return np.where(th > np.pi, th - 2.0 * np.pi, th)


class GriffinLim:
    PHASE_CAP = 1 << 26  # doubles drawn ahead of the decode at most (512 MB of pinned memory per ring slot)

    def __init__(self, n_fft: int, win_length: int, hop_length: int, n_iter: int, device, window_fn=torch.hann_window,
                 phase_rng: str = "numpy", seed: int = 1):
        """``phase_rng``: where the initial phases' uniform draws come from when the caller passes no ``angles`` --
        "numpy" (default): numpy's global generator, one ``np.random.rand(F, T_u)`` per utterance in order, exactly the
        reference's draws (vocoder.py:101-102: a seeded run reproduces the reference's waveform); "device": the counter-based
        generator of the HIP library (``seed``, utterance, bin, frame) -- the same distribution without the ~1 ms per
        utterance-second the host generator costs, for callers that do not need numpy's stream."""
        self.n_fft, self.win_length, self.hop_length, self.n_iter, self.device = n_fft, win_length, hop_length, n_iter, device
        if phase_rng not in ("numpy", "device"):
            raise ValueError("phase_rng must be 'numpy' or 'device'")
        self.phase_rng, self.seed, self._calls = phase_rng, int(seed), 0

        win = get_window(n_fft, win_length, window_fn)
        self.F = n_fft // 2 + 1
        self._phases = PhaseSource(device, self.F)  # numpy's draws for the initial phases (prefetch_phases / batch)
        self._dense = None  # the dense bases of the GEMM path: built on first use (a 2050 x 2048 pseudo-inverse at n_fft 2048)
        self.win_sq = win ** 2
        self._wss = {}
        self.Fp = (self.F + 15) // 16 * 16
        self._bb = None
        self._win = win
        self._ft = None
        # FFT path for the n_fft the LDS FFT kernels have a plan for: 256 ... 2048 (powers of two) and the mixed-radix sizes
        # 240 / 400 / 1200 -- 1200 is what stage 3 writes into config.yaml (S2ST_GL_FFT=0: the dense-basis GEMMs of rounds
        # 1 - 3, an A/B switch; they also serve every other n_fft)
        fn = bd.lib().s2st_fft_len_supported_i32
        self.use_fft = bool(fn(int(n_fft))) and os.environ.get("S2ST_GL_FFT", "1") != "0"

    def set_inflight(self, n: int):
        """How many batches may have a run-ahead phase stream pending at once (the generator's decode chains)."""
        self._phases.set_inflight(n)

    def prefetch_phases(self, n_frames_upper: int):
        """Called by the speech generator BEFORE it decodes (``n_frames_upper``: an upper bound of the frames the batch
        will vocode): with phase_rng="numpy" and the FFT path, numpy's generator is continued while the decoder runs
        (``PhaseSource.prefetch``); otherwise the batch draws after the decode, the ordinary way.
        (The run-ahead is capped: the speech generator's upper bound is bsz x max_iter
        frames, and max_iter defaults to 6000 -- 12 GB of doubles for a batch of 64 at n_fft 2048; a batch that
        really vocodes more than the cap draws the ordinary way, after the decode: ADVICE r4)"""
        ahead = self.phase_rng == "numpy" and self.use_fft and n_frames_upper > 0
        self._phases.prefetch(min(self.F * int(n_frames_upper), self.PHASE_CAP) if ahead else 0)

    @property
    def fwd(self):
        return self._dense_bases()[0]

    @property
    def inv_t(self):
        return self._dense_bases()[1]

    def _dense_bases(self):
        """forward basis [2F][n_fft] (TTSSpectrogram) and inverse basis [n_fft][2F] (GriffinLim.__init__: pinverse)."""
        if self._dense is None:
            fwd = (get_fourier_basis(self.n_fft) * self._win).contiguous().to(self.device)
            inv = torch.pinverse(self.n_fft / self.hop_length * get_fourier_basis(self.n_fft)).T * self._win
            self._dense = (fwd, inv.t().contiguous().to(self.device))
        return self._dense

    def _fft_tables(self):
        # (made lazily on whichever stream asks first and read on others later: `.to(device)` of a pageable host tensor is a
        #  blocking copy -- the bytes are in place when it returns -- so no event is needed; the same holds for _window_sum_square)
        if self._ft is None:
            j = np.arange(self.n_fft, dtype=np.float64)
            tw = np.stack([np.cos(2 * np.pi * j / self.n_fft), -np.sin(2 * np.pi * j / self.n_fft)], axis=1).astype(np.float32)
            self._ft = (self._win.to(self.device, torch.float32).contiguous(), torch.from_numpy(tw).contiguous().to(self.device))
        return self._ft

    def _window_sum_square(self, n_frames: int) -> torch.Tensor:
        w = self._wss.get(n_frames)
        if w is None:  # vocoder.py:69-80 (a constant of the frame count)
            n = self.n_fft + self.hop_length * (n_frames - 1)
            x = torch.zeros(n, dtype=torch.float32)
            for i in range(n_frames):
                o = i * self.hop_length
                x[o: min(n, o + self.n_fft)] += self.win_sq[:max(0, min(self.n_fft, n - o))]
            w = self._wss[n_frames] = x.to(self.device)
        return w

    def __call__(self, specgram: torch.Tensor, angles: np.ndarray = None) -> torch.Tensor:
        """specgram [F, T] magnitudes -> waveform.  ``angles`` defaults to the reference's draw
        np.angle(np.exp(2j*pi*np.random.rand(F, T))) from numpy's global RNG (vocoder.py:101-102)."""
        assert specgram.shape[0] == self.F
        return self.batch([specgram], None if angles is None else [angles])[0]

    @staticmethod
    def _split(x: torch.Tensor):
        hi = x.to(torch.bfloat16)
        return hi, (x - hi.float()).to(torch.bfloat16)

    def _bases_bf16(self):
        """Constant operands of the two GEMMs, [hi | hi | lo] along the contraction (see griffin_lim.hip)."""
        if self._bb is None:
            Fq, Fp, n = self.F, self.Fp, self.n_fft
            fwd = torch.zeros(2 * Fp, n, device=self.device)  # rows: re(F) pad | im(F) pad
            fwd[:Fq] = self.fwd[:Fq]
            fwd[Fp:Fp + Fq] = self.fwd[Fq:]
            hi, lo = self._split(fwd)
            fwd3 = torch.cat([hi, hi, lo], dim=1).contiguous()  # [2Fp][3 n_fft]
            inv = torch.zeros(n, 2 * Fp, device=self.device)  # columns in the spectrum layout
            inv[:, :Fq] = self.inv_t[:, :Fq]
            inv[:, Fp:Fp + Fq] = self.inv_t[:, Fq:]
            hi, lo = self._split(inv)
            inv3 = torch.cat([hi, hi, lo], dim=1).contiguous()  # [n_fft][3 * 2Fp]
            self._bb = (fwd3, inv3)
        return self._bb

    def batch(self, specgrams, angles=None, mag_tm=None):
        """Several utterances at once: ``specgrams`` is a list of [F, T_u] magnitudes, the result the list
        of waveforms.  Griffin-Lim is sequential in its iterations but independent across utterances, so
        every STFT / inverse STFT is ONE launch over all utterances' frames (rows beyond an utterance's T_u
        are zero padding); the reference loops utterances (speech_generator.py:81-94 ->
        vocoder.py:100-123)."""
        Fq, dev = self.F, self.device
        if mag_tm is not None:
            # (the vocoder hands over the whole batch frame-major already: ``specgrams`` is then the list of frame counts)
            Ts = [int(t) for t in specgrams]
            U, Tmax = len(Ts), int(mag_tm.shape[1])
            mag = mag_tm
        else:
            U = len(specgrams)
            if U == 0:
                return []
            Ts = [int(s.shape[1]) for s in specgrams]
            Tmax = max(Ts)
            mag = torch.zeros(U, Tmax, Fq, device=dev)  # time-major: the kernels walk rows = frames
            for u, s_ in enumerate(specgrams):
                mag[u, :Ts[u]] = s_.to(dev, torch.float32).t()
        if U == 0:
            return []
        tl = torch.tensor(Ts, dtype=torch.int32).to(dev)
        uni = uoff = ang = None
        if angles is None and self.use_fft:
            # FFT path: the HOST only runs the generator (the reference's per-utterance draws from numpy's global RNG, in
            # order, into one pinned buffer); wrapping to (-pi, pi], the cast, the transposition and mag * (cos, sin) are
            # one kernel.  phase_rng="device": no host work at all.
            if self.phase_rng == "numpy":
                uni, uoff = self._phases.draw(Ts)
        else:
            if angles is None:  # the reference's per-utterance draws from numpy's global RNG, in order
                angles = [random_phases(Fq, T) for T in Ts]
            ang_h = torch.zeros(U, Tmax, Fq, dtype=torch.float32)
            for u, a_ in enumerate(angles):
                ang_h[u, :Ts[u]] = torch.from_numpy(np.ascontiguousarray(a_, dtype=np.float32)).t()
            ang = ang_h.to(dev)
        offs, tabs, o = [], [], 0
        for T in Ts:
            w = self._window_sum_square(T)
            offs.append(o)
            tabs.append(w)
            o += w.numel()
        wsq_all = torch.cat(tabs)
        wsq_off = torch.tensor(offs, dtype=torch.int64).to(dev)
        if self.use_fft:
            wave = self._run_fft(mag, tl, ang, uni, uoff, wsq_all, wsq_off, U, Tmax)
        else:
            wave = self._run_dense(mag, tl, ang, wsq_all, wsq_off, U, Tmax)
        return [wave[u, :self.hop_length * (Ts[u] - 1)].clone() for u in range(U)]

    def _run_fft(self, mag, tl, ang, uni, uoff, wsq_all, wsq_off, U, Tmax):
        """Both transforms as N-point real FFTs in LDS (csrc/griffin_lim.hip: the reference's analysis basis IS
        rfft(window * frame), its pseudo-inverse synthesis basis IS window * hop / n_fft * irfft): two launches per
        iteration, O(N log N) per frame instead of the dense contraction's 2 N (N + 2) multiply-adds x 3 (bf16x3).
        Initial phases: ``ang``, or the uniform draws ``uni`` / ``uoff``, or (both None) the device generator."""
        Fq, hop, n_fft, dev = self.F, self.hop_length, self.n_fft, self.device
        M, Lw = U * Tmax, hop * (Tmax - 1)
        win, tw = self._fft_tables()
        Xc = torch.empty(M, Fq, 2, device=dev)
        wave = torch.empty(U, max(Lw, 1), device=dev)
        two_kernels = os.environ.get("S2ST_GL_OLA_FUSE", "1") == "0"  # (A/B switch: frames through HBM, as first built)
        frames = torch.empty(M, n_fft, device=dev) if two_kernels else None

        def inverse_fft():
            if two_kernels:
                bd.call("s2st_gl_istft_frames_f32", Xc, tl, win, tw, frames, U, Tmax, n_fft, hop)
                bd.call("s2st_gl_overlap_add_b_f32", frames, wsq_all, wsq_off, tl, wave, U, Tmax, n_fft, hop, Lw)
            else:
                bd.call("s2st_gl_istft_ola_f32", Xc, tl, win, tw, wsq_all, wsq_off, wave, U, Tmax, n_fft, hop, Lw)

        if ang is not None:
            bd.call("s2st_gl_polar_c_f32", mag, ang, tl, Xc, U, Fq, Tmax)
        else:
            self._calls += 1
            bd.call("s2st_gl_polar_u_f32", mag, uni, uoff, tl, (self.seed * 1000003 + self._calls) & ((1 << 63) - 1), Xc, U, Fq, Tmax)
        inverse_fft()
        for _ in range(self.n_iter):
            bd.call("s2st_gl_stft_project_f32", wave, tl, win, tw, mag, Xc, U, Tmax, n_fft, hop, Lw)
            inverse_fft()
        return wave

    def _run_dense(self, mag, tl, ang, wsq_all, wsq_off, U, Tmax):
        """Both transforms as ONE GEMM each over all utterances' frames, on the bf16 kernel with the hi/lo split folded
        into K (``_bases_bf16``): every n_fft without an FFT plan, and S2ST_GL_FFT=0.  Initial phases: ``ang``."""
        Fq, Fp, hop, n_fft, dev = self.F, self.Fp, self.hop_length, self.n_fft, self.device
        M, Lw = U * Tmax, hop * (Tmax - 1)
        fwd3, inv3 = self._bases_bf16()
        Xs = torch.empty(M, 6 * Fp, dtype=torch.bfloat16, device=dev)
        As = torch.empty(M, 3 * n_fft, dtype=torch.bfloat16, device=dev)
        Y = torch.empty(M, 2 * Fp, device=dev)
        frames = torch.empty(M, n_fft, device=dev)
        wave = torch.empty(U, max(Lw, 1), device=dev)

        def inverse():
            bd.gemm(Xs, inv3, frames, M, n_fft, 6 * Fp)
            bd.call("s2st_gl_overlap_add_b_f32", frames, wsq_all, wsq_off, tl, wave, U, Tmax, n_fft, hop, Lw)

        bd.call("s2st_gl_polar_split_f32", mag, ang, 0, tl, Xs, U, Fq, Fp, Tmax)
        inverse()
        for _ in range(self.n_iter):
            bd.call("s2st_gl_frame_split_f32", wave, tl, As, U, Tmax, hop, n_fft, Lw)
            bd.gemm(As, fwd3, Y, M, 2 * Fp, 3 * n_fft)
            bd.call("s2st_gl_polar_split_f32", mag, Y, 1, tl, Xs, U, Fq, Fp, Tmax)
            inverse()
        return wave


class GriffinLimVocoder:
    def __init__(self, sample_rate, win_size, hop_size, n_fft, n_mels, f_min, f_max, window_fn=torch.hann_window,
                 spec_bwd_max_iter=32, device=None, phase_rng: str = "numpy", seed: int = 1):
        self.device = device or torch.device("cuda", torch.cuda.current_device())
        self.n_mels, self.F = n_mels, n_fft // 2 + 1
        basis = torch.pinverse(slaney_mel_filters(sample_rate, n_fft, n_mels, f_min, f_max))  # F x n_mels
        self.inv_mel = basis.contiguous().to(self.device)
        self.gl = GriffinLim(n_fft, win_size, hop_size, spec_bwd_max_iter, self.device, window_fn, phase_rng=phase_rng, seed=seed)

    def _magnitudes(self, xs):
        """List of [T_u, n_mels] log-mels -> (frame counts, magnitudes [U][Tmax][F], frame-major = the layout the Griffin-Lim
        kernels walk; rows beyond T_u: the mel inversion of zero padding, never read).  The whole padded batch at once:
        exp -> pseudo-inverse mel (one bf16x3 GEMM) -> clamp (vocoder.py:136-143)."""
        Ts = [int(x.shape[0]) for x in xs]
        U, Tmax, C_ = len(xs), max(Ts), int(xs[0].shape[1])
        pad = torch.zeros(U, Tmax, C_, device=self.device)
        for u, x in enumerate(xs):
            pad[u, :Ts[u]] = x.to(self.device, torch.float32)
        bd.call("s2st_exp_inplace_f32", pad, U * Tmax * C_)
        mag = torch.empty(U, Tmax, self.F, device=self.device)
        bd.gemm(pad.view(U * Tmax, C_), self.inv_mel, mag.view(U * Tmax, self.F), U * Tmax, self.F, C_, precise=True)
        bd.call("s2st_clamp_min_f32", mag, U * Tmax * self.F, 0.0)
        return Ts, mag

    def __call__(self, x: torch.Tensor, angles: np.ndarray = None) -> torch.Tensor:
        """x [T, n_mels] log-mel -> waveform [1, N] (vocoder.py:136-144)."""
        return self.batch([x], None if angles is None else [angles])[0]

    def prefetch_phases(self, n_frames_upper: int):
        self.gl.prefetch_phases(n_frames_upper)

    def set_inflight(self, n: int):
        self.gl.set_inflight(n)

    def batch(self, xs, angles=None):
        """List of [T_u, n_mels] log-mels -> list of [1, N_u] waveforms, all utterances per launch."""
        if len(xs) == 0:
            return []
        Ts, mag = self._magnitudes(xs)
        return [w.unsqueeze(0) for w in self.gl.batch(Ts, angles, mag_tm=mag)]

    @classmethod
    def from_data_cfg(cls, args, data_cfg, device=None):
        feat_cfg = data_cfg.config["features"] if hasattr(data_cfg, "config") else data_cfg["features"]
        return cls(sample_rate=feat_cfg["sample_rate"], win_size=int(feat_cfg["win_len_t"] * feat_cfg["sample_rate"]),
                   hop_size=int(feat_cfg["hop_len_t"] * feat_cfg["sample_rate"]), n_fft=feat_cfg["n_fft"],
                   n_mels=feat_cfg["n_mels"], f_min=feat_cfg["f_min"], f_max=feat_cfg["f_max"],
                   window_fn=getattr(torch, feat_cfg["window_fn"] + "_window"),
                   spec_bwd_max_iter=getattr(args, "spec_bwd_max_iter", 32), device=device,
                   phase_rng=getattr(args, "gl_phase_rng", "numpy") or "numpy", seed=int(getattr(args, "seed", 1) or 1))
