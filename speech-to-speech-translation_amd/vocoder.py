"""Griffin-Lim vocoder on the HIP path: the counterpart of
``fairseq/models/text_to_speech/vocoder.py:24-158`` (PseudoInverseMelScale, GriffinLim,
GriffinLimVocoder) with the same constructor arguments.

The reference's STFT / inverse STFT are dense-DFT contractions (conv1d / conv_transpose1d with Fourier bases,
audio_utils.py:259-271, vocoder.py:56-98).  Round 4: for power-of-two n_fft (256 ... 2048), and since the
mixed-radix plans of csrc/fft_lds.h for 240, 400 and 1200 (stage 3's default) too, they run as real FFTs in LDS
(csrc/infer.hip: the analysis basis is rfft(window * frame), the pseudo-inverse synthesis basis is window * hop / n_fft *
irfft -- exactly); other n_fft (and S2ST_GL_FFT=0) keep the dense form of rounds 1 - 3: GEMMs on the matrix cores (bf16x3
"precise" mode: phase retrieval is precision-sensitive) around small HIP kernels for polar <-> rectangular conversion,
reflect padding and overlap-add.  The constant tables
(window, Fourier bases and their pseudo-inverses, mel filterbank pseudo-inverse) are built once on
the host at construction, as the reference does in its ``register_buffer`` calls.

The mel filterbank comes from librosa in the reference (absent in this image, version un-pinned):
``slaney_mel_filters`` restates librosa.filters.mel's defaults (htk=False, norm='slaney').
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch
import torch.nn.functional as F

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


class _UniformStream:
    """numpy's global generator, run AHEAD on a background thread.  ``np.random.rand(F, T_u)`` per utterance -- what the
    reference's GriffinLim draws (vocoder.py:101-102) -- is just the next F * T_u doubles of one stream, whatever the shapes;
    only their number is unknown until the decoder has stopped.  So while the GPU decodes, a private generator started from
    the global one's state fills a pinned buffer with an upper bound of draws (numpy releases the GIL inside the fill),
    keeping a state snapshot every chunk.  ``take(n)`` hands out the first n and leaves the GLOBAL generator exactly where
    n sequential draws would have left it (nearest snapshot + the remainder drawn for real) -- provided nobody else used
    the global generator in between, else it returns None and the caller draws the ordinary way."""
    CHUNK = 1 << 20

    def __init__(self, n_upper: int, pin: bool):
        import threading
        self.state0 = np.random.get_state()
        self.n = int(n_upper)
        self.buf = torch.empty(max(self.n, 1), dtype=torch.float64, pin_memory=pin)
        self.host = self.buf.numpy()
        self.snaps = []
        self.produced = 0
        self.cv = threading.Condition()
        self.thread = threading.Thread(target=self._run, daemon=True)
        self.thread.start()

    def _run(self):
        rs = np.random.RandomState()
        rs.set_state(self.state0)
        pos = 0
        while pos < self.n:
            m = min(self.CHUNK, self.n - pos)
            snap = rs.get_state()
            self.host[pos:pos + m] = rs.random_sample(m)
            with self.cv:
                self.snaps.append((pos, snap))
                self.produced = pos + m
                self.cv.notify_all()
            pos += m

    def take(self, n: int):
        cur = np.random.get_state()
        same = cur[0] == self.state0[0] and cur[2] == self.state0[2] and np.array_equal(cur[1], self.state0[1]) \
            and cur[3] == self.state0[3] and cur[4] == self.state0[4]
        if n > self.n or not same:
            return None
        with self.cv:
            while self.produced < n:
                self.cv.wait(0.05)
            pos, snap = max((ps for ps in self.snaps if ps[0] <= n), key=lambda ps: ps[0]) if n > 0 else (0, self.state0)
        np.random.set_state(snap)
        if n > pos:
            np.random.random_sample(n - pos)  # (advance the global generator by the remainder: < one chunk)
        return self.buf[:n]


class _HostMTStream:
    """numpy's global generator continued by the library's own HOST generator (``s2st_mt19937_host_doubles``, csrc/
    mt19937_host.cpp: MT19937 + numpy's two-words-per-double conversion, several threads -- each skips to its share by running
    the recurrence alone, an order of magnitude faster than drawing), on a background thread (ctypes drops the GIL) into a
    pinned buffer while the GPU decodes.  ``take(n)``: the first n draws, and the GLOBAL numpy generator left where n
    sequential draws would have left it (the share boundary in front of n + a short output-less run) -- or None when somebody
    used the global generator in between."""

    def __init__(self, n_upper: int, pin: bool, threads: int = 0, buf: Optional[torch.Tensor] = None, upload=None,
                 start_after: Optional["_HostMTStream"] = None):
        """``upload``: (device, copy stream, ring slot) -- the generator thread then also uploads the WHOLE upper bound of
        draws on that stream as soon as they exist (the decoder is still running: the PCIe link is idle), and ``take``
        hands out a slice of the device copy; without it the caller uploads the n it takes, after the decode.
        ``start_after``: an earlier, still pending stream (two batches decoded at once): this one starts from the state
        the earlier one's ``take(n)`` leaves numpy in -- its REAL end, wherever the earlier batch stopped (round 4 guessed
        "all of its upper bound", which only holds when no utterance stops early: ADVICE r4) -- so its generator thread
        waits for that ``take``; the second batch's post-processing is held behind the first one's anyway
        (``generate_two``), and the run is hidden under the first batch's vocoder."""
        import os
        import threading
        self.upload, self.dev_buf, self.up_ev = upload, None, None
        self.start_after = start_after
        self.taken = threading.Event()  # set by take() / abandon(); end_words: numpy's state behind the draws handed out
        self.end_words = None
        self.state0 = np.random.get_state()  # (with start_after: only its constant fields are used)
        self.n = int(n_upper)
        self.threads = int(threads) or max(1, min(8, (os.cpu_count() or 2) - 1))
        # (``buf``: a caller-owned pinned buffer -- a fresh pinned allocation of this size is a hipHostMalloc, which waits
        # for the whole device: it serialised a deferred vocoder with the next batch's decode)
        self.buf = buf if buf is not None and buf.numel() >= max(self.n, 1) else \
            torch.empty(max(self.n, 1), dtype=torch.float64, pin_memory=pin)
        w = np.zeros(625, dtype=np.uint32)
        w[:624] = self.state0[1]
        w[624] = self.state0[2]
        self.state_w = w
        self.bounds = np.zeros((self.threads + 1, 625), dtype=np.uint32)
        self.rc = None
        self.thread = threading.Thread(target=self._run, daemon=True)
        self.thread.start()

    def abandon(self):
        """Nobody will ``take`` from this stream (its batch failed, or it was dropped): release a stream chained behind it
        (which then reports failure: its caller draws the ordinary way) and wait for the generator thread, which may still
        be writing the staging buffer."""
        self.taken.set()
        self.thread.join()

    def _run(self):
        if self.start_after is not None:
            prev = self.start_after
            prev.taken.wait()
            if prev.end_words is None:  # (not taken from, or its take failed: numpy's state is not ours to predict)
                self.rc = -1
                return
            self.state_w = prev.end_words.copy()  # the state behind the draws the earlier batch REALLY used
        self.rc = _mt_host(self.state_w, self.n, self.buf.data_ptr(), self.bounds, self.threads)
        if self.upload is not None and self.rc == 0 and self.n > 0:
            dev, stream, slot = self.upload
            torch.cuda.set_device(dev)
            with torch.cuda.stream(stream):
                self.dev_buf = self.buf[:self.n].to(dev, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(stream)
            self.up_ev = ev  # (published through this object only; whoever reuses the ring slot reads it after thread.join())

    def take(self, n: int):
        try:
            return self._take(n)
        finally:
            self.taken.set()  # (a stream chained behind this one starts now -- or learns that it cannot)

    def _take(self, n: int):
        if self.start_after is not None and not self.start_after.taken.is_set():
            self.start_after.abandon()  # (out of order: the earlier batch never took its draws)
        self.thread.join()
        cur = np.random.get_state()
        if self.rc != 0:
            return None
        same = cur[0] == self.state0[0] and cur[2] == int(self.state_w[624]) and np.array_equal(cur[1], self.state_w[:624]) \
            and cur[3] == self.state0[3] and cur[4] == self.state0[4]
        if n > self.n or not same:
            return None
        t = min(self.threads, (n * self.threads) // self.n) if self.n else 0
        while t > 0 and self.n * t // self.threads > n:
            t -= 1
        d0 = self.n * t // self.threads
        end = np.zeros((2, 625), dtype=np.uint32)
        if _mt_host(self.bounds[t], n - d0, None, end, 1) != 0:
            return None
        np.random.set_state((self.state0[0], end[1, :624].copy(), int(end[1, 624]), self.state0[3], self.state0[4]))
        self.end_words = end[1].copy()
        if self.dev_buf is not None:
            cur = torch.cuda.current_stream()
            cur.wait_event(self.up_ev)
            self.dev_buf.record_stream(cur)
            return self.dev_buf[:n]
        return self.buf[:n]


def _mt_host(state: np.ndarray, n: int, out_ptr, bounds: np.ndarray, threads: int) -> int:
    import ctypes
    fn = bd.lib().s2st_mt19937_host_doubles
    state = np.ascontiguousarray(state, dtype=np.uint32)
    assert bounds.flags["C_CONTIGUOUS"] and bounds.dtype == np.uint32 and bounds.shape == (threads + 1, 625)
    return int(fn(ctypes.c_void_p(state.ctypes.data), int(n), ctypes.c_void_p(out_ptr) if out_ptr else None,
                  ctypes.c_void_p(bounds.ctypes.data), int(threads)))


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
        self._pin = None
        self._streams = []  # run-ahead phase streams of the batches being decoded, oldest first (prefetch_phases / batch)

        win = get_window(n_fft, win_length, window_fn)
        self.F = n_fft // 2 + 1
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
        import os
        fn = bd.lib().s2st_fft_len_supported_i32
        self.use_fft = bool(fn(int(n_fft))) and os.environ.get("S2ST_GL_FFT", "1") != "0"

    def set_inflight(self, n: int):
        """How many batches may have a run-ahead phase stream pending at once (the generator's decode chains)."""
        self._inflight = max(2, int(n))

    def prefetch_phases(self, n_frames_upper: int):
        """Called by the speech generator BEFORE it decodes (``n_frames_upper``: an upper bound of the frames the batch
        will vocode): with phase_rng="numpy" and the FFT path, numpy's generator is continued while the decoder runs -- by the
        library's multi-threaded host generator into pinned memory (``_HostMTStream``, default), ``S2ST_GL_PHASE_STREAM=
        numpy``: by numpy itself on one background thread (``_UniformStream``), ``=off``: drawn after the decode, the ordinary
        way.  All three hand out the same doubles.  (Rounds 3 - 4 also carried a one-workgroup device kernel that continued
        numpy's stream -- 160 ms for 64 utterances, slower than one host core -- removed in round 5.)"""
        obj = None
        pending = [x for x in self._streams if x is not None]
        if self.phase_rng == "numpy" and self.use_fft and n_frames_upper > 0:
            import os
            how = os.environ.get("S2ST_GL_PHASE_STREAM", "host")
            # (the run-ahead is capped: the speech generator's upper bound is bsz x max_iter
            # frames, and max_iter defaults to 6000 -- 12 GB of doubles for a batch of 64 at n_fft 2048; a batch that
            # really vocodes more than the cap draws the ordinary way, after the decode: ADVICE r4)
            n = min(self.F * int(n_frames_upper), self.PHASE_CAP)
            if pending and not (how == "host" and isinstance(pending[-1], _HostMTStream)):
                how = "off"  # (a second batch in flight: only the host generator can be chained behind a pending one)
            if how == "numpy":
                obj = _UniformStream(n, self.device.type == "cuda")
            elif how == "host":
                up = None
                try:
                    buf = self._ring_buffer(n)
                except RuntimeError:  # (no pinned memory of that size: draw after the decode, the ordinary way)
                    buf, how = None, "off"
                if how == "host":
                    if self.device.type == "cuda" and os.environ.get("S2ST_GL_EARLY_UPLOAD", "1") != "0":
                        # the draws go to the device as soon as the host has them, under the decode (a copy stream of their own)
                        if self.__dict__.get("_copy_stream") is None:
                            from .runtime import streams
                            self._copy_stream = streams.get("phase-upload", self.device, may_share=("vocoder",))
                        up = (self.device, self._copy_stream, None)
                    obj = _HostMTStream(n, self.device.type == "cuda", buf=buf, upload=up,
                                        start_after=pending[-1] if pending else None)
                    if self.device.type == "cuda":
                        self._pin_ring[self._ring_i][2] = obj  # the stream OWNS its slot until it has been joined
            elif how != "off":
                raise ValueError("S2ST_GL_PHASE_STREAM must be host, numpy or off")
        self._streams.append(obj)
        # at most two batches are in flight; an entry nobody took (its batch failed, or the vocoder was called with explicit
        # angles) is dropped -- after its generator thread has been joined: it may still be filling / uploading its slot
        keep = max(2, int(self.__dict__.get("_inflight", 2)))
        for old in self._streams[:-keep]:
            if isinstance(old, _HostMTStream):
                old.abandon()
        del self._streams[:-keep]

    def _ring_buffer(self, n: int):
        """One of two persistent pinned staging buffers for the run-ahead draws, alternating, each guarded by the event of
        the upload that last read it (two: batch k's upload may still be in flight on the vocoder's stream when batch
        k + 1's generator starts filling)."""
        if self.device.type != "cuda":
            return None
        nslots = max(2, int(self.__dict__.get("_inflight", 2)))
        ring = self.__dict__.setdefault("_pin_ring", [])  # slots of [buffer, upload event, owner]
        while len(ring) < nslots:
            ring.append([None, None, None])
        self._ring_i = (self.__dict__.get("_ring_i", -1) + 1) % nslots
        slot = ring[self._ring_i]
        if slot[2] is not None:  # the stream that last filled the slot: its thread is joined before anything is reused
            slot[2].abandon() if not slot[2].taken.is_set() else slot[2].thread.join()
            if slot[2].up_ev is not None:
                slot[2].up_ev.synchronize()  # (its early upload has read the buffer)
            slot[2] = None
        if slot[1] is not None:
            slot[1].synchronize()  # (two batches old: long complete)
            slot[1] = None
        if slot[0] is None or slot[0].numel() < n:
            slot[0] = torch.empty(int(n * 1.05) + 1, dtype=torch.float64, pin_memory=True)
        return slot[0]

    def _ring_uploaded(self, host: torch.Tensor):
        """Record, on the current stream, that the asynchronous upload of a ring buffer was just enqueued."""
        for slot in self.__dict__.get("_pin_ring", ()):
            if slot[0] is not None and slot[0].data_ptr() == host.data_ptr():
                ev = torch.cuda.Event()
                ev.record()
                slot[1] = ev

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

    def _inverse(self, X: torch.Tensor, T: int) -> torch.Tensor:
        """X [T][2F] (real | imag) -> waveform [hop * (T - 1)] (vocoder.py:82-98)."""
        frames = torch.empty(T, self.n_fft, device=self.device)
        bd.gemm(X, self.inv_t, frames, T, self.n_fft, 2 * self.F, precise=True)
        n_out = self.hop_length * (T - 1)
        wave = torch.empty(n_out, device=self.device)
        bd.call("s2st_gl_overlap_add_f32", frames, self._window_sum_square(T), wave, T, self.n_fft, self.hop_length, n_out)
        return wave

    def _transform(self, wave: torch.Tensor, T: int) -> torch.Tensor:
        """waveform -> STFT [T][2F] (audio_utils.py:259-271: reflect pad + strided Fourier-basis conv)."""
        n = wave.numel()
        padded = torch.empty(n + self.n_fft, device=self.device)
        bd.call("s2st_reflect_pad_f32", wave, padded, n, self.n_fft // 2)
        Y = torch.empty(T, 2 * self.F, device=self.device)
        bd.gemm(padded, self.fwd, Y, T, 2 * self.F, self.n_fft, a_ld=self.hop_length, precise=True)
        return Y

    def __call__(self, specgram: torch.Tensor, angles: np.ndarray = None) -> torch.Tensor:
        """specgram [F, T] magnitudes -> waveform.  ``angles`` defaults to the reference's draw
        np.angle(np.exp(2j*pi*np.random.rand(F, T))) from numpy's global RNG (vocoder.py:101-102)."""
        Fq, T = specgram.shape
        assert Fq == self.F
        if self.use_fft:
            return self.batch([specgram], None if angles is None else [angles])[0]
        if angles is None:
            angles = random_phases(Fq, T)
        mag = specgram.to(self.device, torch.float32).contiguous()
        ang = torch.from_numpy(np.ascontiguousarray(angles, dtype=np.float32)).to(self.device)
        X = torch.empty(T, 2 * Fq, device=self.device)
        bd.call("s2st_gl_polar_f32", mag, ang, X, Fq, T)
        wave = self._inverse(X, T)
        for _ in range(self.n_iter):
            Y = self._transform(wave, T)
            bd.call("s2st_gl_project_f32", mag, Y, X, Fq, T)
            wave = self._inverse(X, T)
        return wave


    @staticmethod
    def _split(x: torch.Tensor):
        hi = x.to(torch.bfloat16)
        return hi, (x - hi.float()).to(torch.bfloat16)

    def _bases_bf16(self):
        """Constant operands of the two GEMMs, [hi | hi | lo] along the contraction (see infer.hip)."""
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
        every STFT / inverse STFT is ONE GEMM over all utterances' frames (rows beyond an utterance's T_u
        are zero padding); the reference loops utterances (speech_generator.py:81-94 ->
        vocoder.py:100-123).  The GEMMs run on the bf16 kernel with the hi/lo split folded into K."""
        Fq, Fp, hop, n_fft, dev = self.F, self.Fp, self.hop_length, self.n_fft, self.device
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
                n_all = sum(Fq * T for T in Ts)
                offs, o = [], 0
                for T in Ts:
                    offs.append(o)
                    o += Fq * T
                obj = self._streams.pop(0) if self._streams else None
                ahead = obj.take(n_all) if obj is not None else None
                if ahead is not None:  # drawn while the decoder ran (prefetch_phases)
                    uni = ahead if ahead.device == dev else ahead.to(dev, non_blocking=True)
                    if ahead.device != dev and dev.type == "cuda":
                        self._ring_uploaded(ahead)
                else:
                    ev = self.__dict__.get("_pin_ev")
                    if ev is not None:  # (the previous call's upload of this staging buffer: it may still be queued on
                        ev.synchronize()  # another stream when two batches are in flight)
                        self._pin_ev = None
                    if self._pin is None or self._pin.numel() < n_all:
                        self._pin = torch.empty(n_all, dtype=torch.float64, pin_memory=dev.type == "cuda")
                    host = self._pin.numpy()
                    for T, o in zip(Ts, offs):
                        host[o:o + Fq * T] = np.random.rand(Fq, T).reshape(-1)
                    uni = self._pin[:n_all].to(dev, non_blocking=True)
                    if dev.type == "cuda":
                        self._pin_ev = torch.cuda.Event()
                        self._pin_ev.record()
                uoff = torch.tensor(offs, dtype=torch.int64).to(dev)
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
        M, Lw = U * Tmax, hop * (Tmax - 1)
        if self.use_fft:
            # round 4: both transforms as N-point real FFTs in LDS (csrc/infer.hip: the reference's analysis basis IS
            # rfft(window * frame), its pseudo-inverse synthesis basis IS window * hop / n_fft * irfft): two launches per
            # iteration, O(N log N) per frame instead of the dense contraction's 2 N (N + 2) multiply-adds x 3 (bf16x3)
            win, tw = self._fft_tables()
            Xc = torch.empty(M, Fq, 2, device=dev)
            wave = torch.empty(U, max(Lw, 1), device=dev)
            import os
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
            return [wave[u, :hop * (Ts[u] - 1)].clone() for u in range(U)]
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
        return [wave[u, :hop * (Ts[u] - 1)].clone() for u in range(U)]


class GriffinLimVocoder:
    def __init__(self, sample_rate, win_size, hop_size, n_fft, n_mels, f_min, f_max, window_fn=torch.hann_window,
                 spec_bwd_max_iter=32, device=None, phase_rng: str = "numpy", seed: int = 1):
        self.device = device or torch.device("cuda", torch.cuda.current_device())
        self.n_mels, self.F = n_mels, n_fft // 2 + 1
        basis = torch.pinverse(slaney_mel_filters(sample_rate, n_fft, n_mels, f_min, f_max))  # F x n_mels
        self.inv_mel = basis.contiguous().to(self.device)
        self.gl = GriffinLim(n_fft, win_size, hop_size, spec_bwd_max_iter, self.device, window_fn, phase_rng=phase_rng, seed=seed)

    def __call__(self, x: torch.Tensor, angles: np.ndarray = None) -> torch.Tensor:
        """x [T, n_mels] log-mel -> waveform [1, N] (vocoder.py:136-144)."""
        T, C_ = x.shape
        xt = torch.empty(C_, T, device=self.device)  # exp(x)^T
        bd.call("s2st_exp_transpose_f32", x.to(self.device, torch.float32).contiguous(), xt, T, C_)
        spec = torch.empty(self.F, T, device=self.device)
        bd.gemm(self.inv_mel, xt, spec, self.F, T, C_, b_kmajor=False, b_ld=T, precise=True)
        bd.call("s2st_clamp_min_f32", spec, self.F * T, 0.0)
        return self.gl(spec, angles).unsqueeze(0)

    def prefetch_phases(self, n_frames_upper: int):
        self.gl.prefetch_phases(n_frames_upper)

    def set_inflight(self, n: int):
        self.gl.set_inflight(n)

    def batch(self, xs, angles=None):
        """List of [T_u, n_mels] log-mels -> list of [1, N_u] waveforms, all utterances per launch."""
        if self.gl.use_fft and len(xs) > 0:
            # the whole padded batch at once: exp -> pseudo-inverse mel (one bf16x3 GEMM, frame-major result = the layout
            # the Griffin-Lim kernels walk) -> clamp; rounds 1 - 3 ran three launches and two copies per utterance
            Ts = [int(x.shape[0]) for x in xs]
            U, Tmax, C_ = len(xs), max(Ts), int(xs[0].shape[1])
            pad = torch.zeros(U, Tmax, C_, device=self.device)
            for u, x in enumerate(xs):
                pad[u, :Ts[u]] = x.to(self.device, torch.float32)
            bd.call("s2st_exp_inplace_f32", pad, U * Tmax * C_)
            mag = torch.empty(U, Tmax, self.F, device=self.device)
            bd.gemm(pad.view(U * Tmax, C_), self.inv_mel, mag.view(U * Tmax, self.F), U * Tmax, self.F, C_, precise=True)
            bd.call("s2st_clamp_min_f32", mag, U * Tmax * self.F, 0.0)
            return [w.unsqueeze(0) for w in self.gl.batch(Ts, angles, mag_tm=mag)]
        specs = []
        for x in xs:
            T, C_ = x.shape
            xt = torch.empty(C_, T, device=self.device)
            bd.call("s2st_exp_transpose_f32", x.to(self.device, torch.float32).contiguous(), xt, T, C_)
            spec = torch.empty(self.F, T, device=self.device)
            bd.gemm(self.inv_mel, xt, spec, self.F, T, C_, b_kmajor=False, b_ld=T, precise=True)
            bd.call("s2st_clamp_min_f32", spec, self.F * T, 0.0)
            specs.append(spec)
        return [w.unsqueeze(0) for w in self.gl.batch(specs, angles)]

    @classmethod
    def from_data_cfg(cls, args, data_cfg, device=None):
        feat_cfg = data_cfg.config["features"] if hasattr(data_cfg, "config") else data_cfg["features"]
        return cls(sample_rate=feat_cfg["sample_rate"], win_size=int(feat_cfg["win_len_t"] * feat_cfg["sample_rate"]),
                   hop_size=int(feat_cfg["hop_len_t"] * feat_cfg["sample_rate"]), n_fft=feat_cfg["n_fft"],
                   n_mels=feat_cfg["n_mels"], f_min=feat_cfg["f_min"], f_max=feat_cfg["f_max"],
                   window_fn=getattr(torch, feat_cfg["window_fn"] + "_window"),
                   spec_bwd_max_iter=getattr(args, "spec_bwd_max_iter", 32), device=device,
                   phase_rng=getattr(args, "gl_phase_rng", "numpy") or "numpy", seed=int(getattr(args, "seed", 1) or 1))
from .models.hifigan import HiFiGANVocoder  # noqa: E402,F401  (--vocoder hifigan)
