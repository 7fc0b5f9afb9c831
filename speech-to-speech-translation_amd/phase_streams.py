"""Uniform draws for Griffin-Lim's initial phases, taken from numpy's global generator the way the reference does
(``np.random.rand(F, T_u)`` per utterance in order, vocoder.py:101-102) -- and, where the caller announces a batch before
it decodes, run AHEAD of the decode on a host thread: ``_UniformStream`` (numpy itself), ``_HostMTStream`` (the library's
threaded MT19937, csrc/mt19937_host.cpp, with an early upload to the device).  ``PhaseSource`` owns the pending streams,
the pinned staging buffers and the copy stream for one ``GriffinLim``."""
from __future__ import annotations

import os
from typing import Optional

import numpy as np
import torch

from .runtime import binding as bd


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


class _RingSlot:
    """One pinned staging buffer of the run-ahead draws: ``uploaded`` is the event of the upload that last read it,
    ``owner`` the stream that last filled it."""
    __slots__ = ("buf", "uploaded", "owner")

    def __init__(self):
        self.buf = self.uploaded = self.owner = None


class PhaseSource:
    """The uniform draws behind the initial phases of one ``GriffinLim``: ``prefetch`` before a batch is decoded,
    ``draw`` when it is vocoded; batches are served oldest first."""

    def __init__(self, device, F: int):
        self.device, self.F = device, int(F)
        self._pending = []  # run-ahead streams of the batches being decoded, oldest first (None: that batch draws the ordinary way)
        self._inflight = 2
        self._ring = []  # persistent pinned staging buffers of the host generator, alternating
        self._ring_i = -1
        self._copy_stream = None
        self._pin = self._pin_ev = None  # staging buffer of the ordinary draws and the event of its last upload

    def set_inflight(self, n: int):
        """How many batches may have a run-ahead phase stream pending at once (the generator's decode chains)."""
        self._inflight = max(2, int(n))

    def prefetch(self, n_doubles_upper: int):
        """Called BEFORE a batch is decoded, with an upper bound of the doubles it will draw (0: no run-ahead, the batch
        draws the ordinary way): numpy's generator is continued while the decoder runs -- by the
        library's multi-threaded host generator into pinned memory (``_HostMTStream``, default), ``S2ST_GL_PHASE_STREAM=
        numpy``: by numpy itself on one background thread (``_UniformStream``), ``=off``: drawn after the decode, the ordinary
        way.  All three hand out the same doubles.  (Rounds 3 - 4 also carried a one-workgroup device kernel that continued
        numpy's stream -- 160 ms for 64 utterances, slower than one host core -- removed in round 5.)"""
        obj = None
        pending = [x for x in self._pending if x is not None]
        n = int(n_doubles_upper)
        if n > 0:
            how = os.environ.get("S2ST_GL_PHASE_STREAM", "host")
            if pending and not (how == "host" and isinstance(pending[-1], _HostMTStream)):
                how = "off"  # (a second batch in flight: only the host generator can be chained behind a pending one)
            if how == "numpy":
                obj = _UniformStream(n, self.device.type == "cuda")
            elif how == "host":
                up = None
                try:
                    slot = self._ring_slot(n)
                except RuntimeError:  # (no pinned memory of that size: draw after the decode, the ordinary way)
                    slot, how = None, "off"
                if how == "host":
                    if self.device.type == "cuda" and os.environ.get("S2ST_GL_EARLY_UPLOAD", "1") != "0":
                        # the draws go to the device as soon as the host has them, under the decode (a copy stream of their own)
                        if self._copy_stream is None:
                            from .runtime import streams
                            self._copy_stream = streams.get("phase-upload", self.device, may_share=("vocoder",))
                        up = (self.device, self._copy_stream, None)
                    obj = _HostMTStream(n, self.device.type == "cuda", buf=slot.buf if slot is not None else None, upload=up,
                                        start_after=pending[-1] if pending else None)
                    if slot is not None:
                        slot.owner = obj  # the stream OWNS its slot until it has been joined
            elif how != "off":
                raise ValueError("S2ST_GL_PHASE_STREAM must be host, numpy or off")
        self._pending.append(obj)
        # at most two batches are in flight; an entry nobody took (its batch failed, or the vocoder was called with explicit
        # angles) is dropped -- after its generator thread has been joined: it may still be filling / uploading its slot
        for old in self._pending[:-self._inflight]:
            if isinstance(old, _HostMTStream):
                old.abandon()
        del self._pending[:-self._inflight]

    def _ring_slot(self, n: int):
        """One of two persistent pinned staging buffers for the run-ahead draws, alternating, each guarded by the event of
        the upload that last read it (two: batch k's upload may still be in flight on the vocoder's stream when batch
        k + 1's generator starts filling).  None on a host device."""
        if self.device.type != "cuda":
            return None
        while len(self._ring) < self._inflight:
            self._ring.append(_RingSlot())
        self._ring_i = (self._ring_i + 1) % self._inflight
        slot = self._ring[self._ring_i]
        if slot.owner is not None:  # the stream that last filled the slot: its thread is joined before anything is reused
            slot.owner.abandon() if not slot.owner.taken.is_set() else slot.owner.thread.join()
            if slot.owner.up_ev is not None:
                slot.owner.up_ev.synchronize()  # (its early upload has read the buffer)
            slot.owner = None
        if slot.uploaded is not None:
            slot.uploaded.synchronize()  # (two batches old: long complete)
            slot.uploaded = None
        if slot.buf is None or slot.buf.numel() < n:
            slot.buf = torch.empty(int(n * 1.05) + 1, dtype=torch.float64, pin_memory=True)
        return slot

    def _ring_uploaded(self, host: torch.Tensor):
        """Record, on the current stream, that the asynchronous upload of a ring buffer was just enqueued."""
        for slot in self._ring:
            if slot.buf is not None and slot.buf.data_ptr() == host.data_ptr():
                ev = torch.cuda.Event()
                ev.record()
                slot.uploaded = ev

    def draw(self, Ts):
        """The draws of one batch, ``np.random.rand(F, T)`` per utterance in order: (uni, device float64 -- utterance u's
        [F][T_u] block starts at uoff[u]; uoff, device int64).  Taken from the oldest pending run-ahead stream when it is
        valid, else drawn now; numpy's global generator ends where the sequential draws leave it either way."""
        Fq, dev = self.F, self.device
        n_all = sum(Fq * T for T in Ts)
        offs, o = [], 0
        for T in Ts:
            offs.append(o)
            o += Fq * T
        obj = self._pending.pop(0) if self._pending else None
        ahead = obj.take(n_all) if obj is not None else None
        if ahead is not None:  # drawn while the decoder ran (prefetch)
            uni = ahead if ahead.device == dev else ahead.to(dev, non_blocking=True)
            if ahead.device != dev and dev.type == "cuda":
                self._ring_uploaded(ahead)
        else:
            if self._pin_ev is not None:  # (the previous call's upload of this staging buffer: it may still be queued on
                self._pin_ev.synchronize()  # another stream when two batches are in flight)
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
        return uni, torch.tensor(offs, dtype=torch.int64).to(dev)
