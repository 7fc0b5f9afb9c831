"""Pause-seeking segmentation: where to cut a recording that is longer than the model takes, so that the cuts fall into pauses.

The reference has no counterpart -- it only ever sees utterances -- so the definition is this package's own, stated in
include/s2st_hip.h next to ``s2st_segment_pcm16`` and restated here, operation for operation, by ``host_segment``.
**Parity unpinned: the reference has no segmentation.**

Everything is integer and exact.  With the framing of the Kaldi filter bank at the recording's rate (``win`` = 25 ms, ``hop`` =
10 ms of samples; ``T`` = 0 if ``n < win`` else ``1 + (n - win) // hop`` frames, the count ``translate`` uses):

* frame energy ``E[t] = sum_{i < win} x[t hop + i]**2`` of the 16-bit samples, smoothed energy ``S[t]`` = the sum of ``E`` over
  ``t - w .. t + w`` clipped to the recording;
* one cut costs ``S[cut] + lam``, ``lam = floor(float(max S) * 10**(-cut_penalty_db / 10))``; a frame is speech if ``E[t] >
  thr``, ``thr = floor(float(max E) * 10**(-silence_db / 10))`` -- one IEEE double multiply and a floor each;
* the cuts ``0 = b_0 < .. < b_K = T`` with ``min_len <= b_{k+1} - b_k <= max_len`` minimise the summed cost of the interior
  cuts: ``D[0] = 0``, ``D[t] = S[t] + lam + min_{t - max_len <= s <= t - min_len} D[s]``, the step to ``T`` adds no cut cost,
  an unreachable ``t`` enters no sum, and **ties go to the smallest s at every step** (the fewest and latest cuts);
  ``T < min_len``: one segment without a search; ``1 <= min_len`` and ``2 min_len <= max_len`` make every longer ``T`` feasible;
* each segment is narrowed to ``[max(b_k, first - pad), min(b_{k+1}, last + 1 + pad))`` around its first and last speech frame;
  one without a speech frame is dropped.

Segment k covers the samples ``[b_k hop, b_{k+1} hop)``, the last one to ``n``; a trimmed span likewise (``trim_end == T`` runs
to ``n``), so a segment of ``L`` frames has at most ``L`` filter-bank frames of its own and fits a model that takes ``max_len``.

``segment(..., segmenter="device")`` runs csrc/segment.hip (an energy kernel over the ragged batch, then one workgroup per
recording for the search, back-trace and trimming; nothing is read back in between); ``segmenter="host"`` is ``host_segment``.
The two agree bit for bit.  A float waveform in [-1, 1) is first rounded by the ``s2st_wave_to_pcm16`` rule (clip, x 32768,
round half to even), so the energy is always taken from int16.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .data import audio_utils
from .runtime import binding as bd

ERR_SHAPE = -2
MAX_RING = 7168      # the device form's limit on max_len + min_len (csrc/segment.hip: the ring of D in LDS)
MAX_SMOOTH = 64      # ... and on w
_INF = np.iinfo(np.int64).max

# the defaults (design choices, not measurements; README.md states them)
MIN_SEGMENT_S = 1.0
SMOOTH_FRAMES = 10
SILENCE_DB = 40.0
CUT_PENALTY_DB = 40.0
PAD_MS = 100.0
MAX_PAUSE_MS = 1000.0


@dataclasses.dataclass
class Segmentation:
    """One recording's segments.  ``start`` / ``end`` / ``trim_start`` / ``trim_end``: int32 [K] in frames; ``dropped``: int32
    [K] (1: no speech frame; its trimmed span is empty at ``start``); ``cost``: the summed cost of the cuts; ``samples`` /
    ``trim_samples``: int64 [K][2] sample spans.  ``E`` / ``S``: int64 [T] energies, when asked for."""
    n_samples: int
    rate: int
    win: int
    hop: int
    n_frames: int
    start: np.ndarray
    end: np.ndarray
    trim_start: np.ndarray
    trim_end: np.ndarray
    dropped: np.ndarray
    cost: int
    samples: np.ndarray
    trim_samples: np.ndarray
    E: Optional[np.ndarray] = None
    S: Optional[np.ndarray] = None

    def __len__(self) -> int:
        return len(self.start)


def framing(rate: int) -> Tuple[int, int]:
    """(win, hop) in samples: the Kaldi filter bank's frame length and shift at ``rate`` -- the numbers
    ``DeviceFeatureExtractor._fbank_tables`` starts from."""
    shift, size = audio_utils._kaldi_tables(float(rate), 80, 25.0, 10.0, 20.0, 0.0)[:2]
    return int(size), int(shift)


def n_frames(n: int, win: int, hop: int) -> int:
    return 0 if n < win else 1 + (n - win) // hop


def db_factor(db: float) -> float:
    """``10**(-dB / 10)`` as the double both forms are given."""
    return 10.0 ** (-float(db) / 10.0)


def host_pcm16(x: np.ndarray) -> np.ndarray:
    """int16 as it is; a float waveform in [-1, 1) by the ``s2st_wave_to_pcm16`` rule."""
    x = np.asarray(x)
    if x.dtype == np.int16:
        return x
    return np.round(np.clip(x.astype(np.float64), -1.0, 1.0 - 1.0 / 32768) * 32768.0).astype(np.int16)


def _scale(m: int, f: float) -> int:
    p = float(m) * f  # one IEEE double multiply (m < 2**53: exact as a double)
    return 1 << 62 if p >= 2.0 ** 62 else math.floor(p)


def _check(min_len: int, max_len: int, w: int = 0, pad: int = 0, factors: Sequence[float] = ()) -> None:
    if min_len < 1 or max_len < 2 * min_len:
        raise ValueError(f"segmentation needs 1 <= min_len and 2 min_len <= max_len (min_len {min_len}, max_len {max_len})")
    if w < 0 or pad < 0:
        raise ValueError("segmentation: w and pad must not be negative")
    for f in factors:
        if not (f >= 0.0 and math.isfinite(f)):
            raise ValueError(f"segmentation: factor {f!r} must be finite and not negative")


def host_search(S: Sequence[int], lam: int, min_len: int, max_len: int, T: Optional[int] = None) -> Tuple[int, List[int]]:
    """The search alone: (cost, cuts ``[b_0 = 0, .., b_K = T]``) over smoothed energies ``S[0 .. T)`` with Python ints."""
    _check(min_len, max_len)
    T = len(S) if T is None else int(T)
    lam = int(lam)
    if T < min_len:
        return 0, [0, T]
    D = np.full(T + 1, _INF, dtype=np.int64)  # _INF: unreachable; never enters an add
    bp = np.full(T + 1, -1, dtype=np.int64)
    D[0] = 0
    for t in range(min_len, T + 1):
        lo, hi = max(0, t - max_len), t - min_len
        s = lo + int(np.argmin(D[lo:hi + 1]))  # (the first occurrence of the minimum: the smallest s)
        best = int(D[s])
        if best == _INF:
            continue
        D[t] = best + (int(S[t]) + lam if t < T else 0)
        bp[t] = s
    if D[T] == _INF:
        raise ValueError(f"no admissible segmentation of {T} frames")  # (cannot happen under the preconditions)
    cuts, t = [T], T
    while t > 0:
        t = int(bp[t])
        cuts.append(t)
    return int(D[T]), cuts[::-1]


def _assemble(n: int, rate: int, win: int, hop: int, T: int, start, end, ts, te, dropped, cost, E=None, S=None) -> Segmentation:
    start, end, ts, te, dropped = (np.ascontiguousarray(a, dtype=np.int32) for a in (start, end, ts, te, dropped))

    def at(frames):  # frame -> sample: T itself is the end of the recording
        frames = frames.astype(np.int64)
        return np.where(frames >= T, n, frames * hop)

    samples = np.stack([start.astype(np.int64) * hop, at(end)], axis=1)
    trim = np.stack([ts.astype(np.int64) * hop, at(te)], axis=1)
    trim[dropped != 0, 1] = trim[dropped != 0, 0]
    return Segmentation(int(n), int(rate), int(win), int(hop), int(T), start, end, ts, te, dropped, int(cost), samples, trim, E, S)


def host_segment(pcm: np.ndarray, rate: int, min_len: int, max_len: int, w: int = SMOOTH_FRAMES, silence_db: float = SILENCE_DB,
                 cut_penalty_db: float = CUT_PENALTY_DB, pad: int = 10, win: Optional[int] = None,
                 hop: Optional[int] = None) -> Segmentation:
    """One recording (int16, or float in [-1, 1)); ``min_len`` / ``max_len`` / ``w`` / ``pad`` in frames.  The module
    docstring's rules in numpy int64 and Python ints."""
    pf, sf = db_factor(cut_penalty_db), db_factor(silence_db)
    _check(min_len, max_len, w, pad, (pf, sf))
    if win is None or hop is None:
        win, hop = framing(rate)
    x = host_pcm16(pcm).astype(np.int64)
    n = int(x.shape[0])
    T = n_frames(n, win, hop)
    c = np.concatenate([np.zeros(1, np.int64), np.cumsum(x * x)])
    t = np.arange(T, dtype=np.int64)
    E = c[t * hop + win] - c[t * hop]
    ce = np.concatenate([np.zeros(1, np.int64), np.cumsum(E)])
    S = ce[np.minimum(T, t + w + 1)] - ce[np.maximum(0, t - w)]
    lam = _scale(int(S.max()) if T else 0, pf)
    thr = _scale(int(E.max()) if T else 0, sf)
    cost, cuts = host_search(S, lam, min_len, max_len)
    K = len(cuts) - 1
    ts, te, dropped = np.zeros(K, np.int32), np.zeros(K, np.int32), np.zeros(K, np.int32)
    speech = E > thr
    for k in range(K):
        b0, b1 = cuts[k], cuts[k + 1]
        at = np.nonzero(speech[b0:b1])[0]
        if len(at) == 0:
            ts[k], te[k], dropped[k] = b0, b0, 1
        else:
            ts[k], te[k] = max(b0, b0 + int(at[0]) - pad), min(b1, b0 + int(at[-1]) + 1 + pad)
    return _assemble(n, rate, win, hop, T, cuts[:-1], cuts[1:], ts, te, dropped, cost, E, S)


def _device_pcm16(w, device) -> torch.Tensor:
    """One recording as a 1-D int16 tensor on ``device``: int16 uploaded as it is, floats through ``s2st_wave_to_pcm16``."""
    if isinstance(w, torch.Tensor):
        if w.dtype == torch.int16:
            return w.reshape(-1).to(device)
        x = w.reshape(1, -1).to(device=device, dtype=torch.float32).contiguous()
    else:
        w = np.asarray(w)
        if w.dtype == np.int16:
            return torch.from_numpy(np.ascontiguousarray(w)).to(device)
        x = torch.from_numpy(np.ascontiguousarray(w, dtype=np.float32)).reshape(1, -1).to(device)
    N = int(x.shape[1])
    out = torch.empty(1, N, dtype=torch.int16, device=device)
    if N:
        bd.call("s2st_wave_to_pcm16", x, torch.tensor([N], dtype=torch.int32).to(device), out, 1, N)
    return out.reshape(-1)


def segment(pcm_list: Sequence, rate: int, min_len: int, max_len: int, w: int = SMOOTH_FRAMES, silence_db: float = SILENCE_DB,
            cut_penalty_db: float = CUT_PENALTY_DB, pad: int = 10, device=None, segmenter: str = "device",
            win: Optional[int] = None, hop: Optional[int] = None, return_energy: bool = False, raw: bool = False) -> List[Segmentation]:
    """A ragged batch of recordings (int16 or float numpy arrays, or device tensors) in one call: ``s2st_segment_pcm16``
    (``segmenter="device"``) or ``host_segment`` per recording (``"host"``).  Returns one ``Segmentation`` per recording."""
    if segmenter not in ("device", "host"):
        raise ValueError(f"segmenter {segmenter!r}: expected 'device' or 'host'")
    if win is None or hop is None:
        win, hop = framing(rate)
    if segmenter == "host":
        return [host_segment(p.detach().cpu().numpy() if isinstance(p, torch.Tensor) else p, rate, min_len, max_len, w,
                             silence_db, cut_penalty_db, pad, win, hop) for p in pcm_list]
    pf, sf = db_factor(cut_penalty_db), db_factor(silence_db)
    _check(min_len, max_len, w, pad, (pf, sf))
    B = len(pcm_list)
    if B == 0:
        return []
    if device is None:
        device = torch.device("cpu") if bd.is_emulator() else torch.device("cuda", torch.cuda.current_device())
    dev = torch.device(device)
    if all(not isinstance(p, torch.Tensor) and np.asarray(p).dtype == np.int16 for p in pcm_list):
        parts = [np.ascontiguousarray(p, dtype=np.int16).reshape(-1) for p in pcm_list]
        lens = [int(p.shape[0]) for p in parts]
        flat = torch.from_numpy(np.concatenate(parts) if sum(lens) else np.zeros(1, np.int16)).to(dev)  # ONE upload
    else:
        parts = [_device_pcm16(p, dev) for p in pcm_list]
        lens = [int(p.numel()) for p in parts]
        flat = torch.cat(parts) if sum(lens) else torch.zeros(1, dtype=torch.int16, device=dev)
    bd.require_device(flat)
    soff = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)).to(dev)
    Ts = [n_frames(n, win, hop) for n in lens]
    Tmax = max(Ts)
    Kcap = max(1, Tmax // min_len)
    lib = bd.lib()
    ws_bytes = int(lib.s2st_segment_workspace(B, Tmax, min_len))
    ws = torch.empty(max(ws_bytes // 8, 1), dtype=torch.int64, device=dev)
    nseg = torch.empty(B, dtype=torch.int32, device=dev)
    out = torch.empty(5, B, Kcap, dtype=torch.int32, device=dev)  # start, end, trim_start, trim_end, dropped
    cost = torch.empty(B, dtype=torch.int64, device=dev)
    rc = lib.s2st_segment_pcm16(flat.data_ptr(), soff.data_ptr(), B, Tmax, win, hop, w, min_len, max_len, pad, pf, sf, Kcap,
                                nseg.data_ptr(), *(out[j].data_ptr() for j in range(5)), cost.data_ptr(), ws.data_ptr(),
                                ws_bytes, C.c_void_p(bd.stream_ptr()))
    if rc == ERR_SHAPE:
        raise bd.S2STHipError(f"s2st_segment_pcm16: max_len + min_len = {max_len + min_len} is beyond the device form "
                              f"({MAX_RING}): use segmenter=\"host\"")
    bd.check(rc, "s2st_segment_pcm16")
    nseg, out, cost = nseg.cpu().numpy(), out.cpu().numpy(), cost.cpu().numpy()
    ES = ws[:2 * B * Tmax].cpu().numpy().reshape(2, B, Tmax) if return_energy else None
    res = []
    for b in range(B):
        K = int(nseg[b])
        E, S = (ES[0, b, :Ts[b]].copy(), ES[1, b, :Ts[b]].copy()) if return_energy else (None, None)
        res.append(_assemble(lens[b], rate, win, hop, Ts[b], *(out[j, b, :K] for j in range(5)), cost[b], E, S))
    if raw:  # (tests: the output arrays as the kernel left them, the rows behind nseg included)
        return res, {"nseg": nseg, "out": out, "cost": cost}
    return res


# ---- the command-line side (translate --segment long, python -m s2st_amd.segment) ------------------------------------------
def add_segment_flags(p) -> None:
    """The segmentation's own flags on an argparse parser."""
    a = p.add_argument
    a("--max-segment-s", type=float, default=None, help="segments last this long at most (default: what the model takes)")
    a("--min-segment-s", type=float, default=MIN_SEGMENT_S, help="... and this long at least")
    a("--silence-db", type=float, default=SILENCE_DB,
      help="a frame this far below the loudest frame's energy is silence (segments are trimmed to their speech)")
    a("--cut-penalty-db", type=float, default=CUT_PENALTY_DB,
      help="what one cut costs besides the energy it cuts through: the largest smoothed energy lowered by this")
    a("--segment-pad-ms", type=float, default=PAD_MS, help="kept around a segment's first and last speech frame")
    a("--segmenter", default="device", choices=["device", "host"],
      help="s2st_segment_pcm16 on the device, or the same rules in numpy on the host (same files)")


def segment_frames(args_or_opts, limit: Optional[int]) -> Dict:
    """The flags in frames of 10 ms: {min_len, max_len, pad, silence_db, cut_penalty_db, segmenter}.  ``limit``: the
    model's ``max_source_positions`` (None: no model)."""
    g = (lambda k, d: args_or_opts.get(k, d)) if isinstance(args_or_opts, dict) else (lambda k, d: getattr(args_or_opts, k, d))
    max_s = g("max_segment_s", None)
    max_len = limit if max_s is None else int(round(float(max_s) * 100))
    if max_len is None:
        raise SystemExit("segment: --max-segment-s is needed without a model")
    if limit is not None:
        max_len = min(max_len, int(limit))
    min_len = max(1, int(round(float(g("min_segment_s", MIN_SEGMENT_S)) * 100)))
    if max_len < 2 * min_len:
        raise SystemExit(f"segment: segments of at most {max_len} frames cannot all last {min_len} frames or more: "
                         f"--max-segment-s must be at least twice --min-segment-s")
    return {"min_len": min_len, "max_len": max_len, "pad": max(0, int(round(float(g("segment_pad_ms", PAD_MS)) / 10))),
            "silence_db": float(g("silence_db", SILENCE_DB)), "cut_penalty_db": float(g("cut_penalty_db", CUT_PENALTY_DB)),
            "segmenter": g("segmenter", "device")}


SEGMENT_COLUMNS = ["id", "k", "src_start_s", "src_end_s", "trim_start_s", "trim_end_s", "dropped"]


def segment_rows(name: str, seg, out_spans=None, out_rate: int = 0, text=None, n_text: int = 0) -> List[List[str]]:
    """One row per segment of ``seg`` (SEGMENT_COLUMNS; times as ``%.6f`` seconds, which identify a sample at any audio
    rate), then, with ``out_spans`` {k: (start, end)}, where its translation lies in the written wav (empty for a segment
    that was not translated) and, with ``text`` {k: [strings]}, the text columns."""
    rows = []
    for k in range(len(seg)):
        t = [f"{int(v) / seg.rate:.6f}" for v in (*seg.samples[k], *seg.trim_samples[k])]
        row = [name, str(k)] + t + [str(int(seg.dropped[k]))]
        if out_spans is not None:
            row += [f"{v / out_rate:.6f}" for v in out_spans[k]] if k in out_spans else ["", ""]
        if text is not None:
            row += list(text.get(k, [""] * n_text))
        rows.append(row)
    return rows


def write_segments_tsv(path: str, rows, out_columns: bool = False, text: Sequence[str] = ()) -> None:
    head = SEGMENT_COLUMNS + (["out_start_s", "out_end_s"] if out_columns else []) + list(text)
    with open(path, "w", encoding="utf-8") as f:
        f.write("\t".join(head) + "\n")
        for r in rows:
            f.write("\t".join(r) + "\n")
