"""Time-scale modification of 16-bit PCM: change the tempo of speech, keep its pitch -- and the rule that places translated
segments on the source's time line.

    python -m s2st_amd.time_scale AUDIO... --results-path OUT --tempo F [--frame-ms 40] [--search-ms 10] [--time-scaler device|host]

writes ``OUT/<id>.wav`` (16-bit PCM at the input's rate; float input rounded by the ``s2st_wave_to_pcm16`` rule), every file
``ceil(n * 1000 / round(1000 F))`` samples long.

The reference has no counterpart -- no time-scale modification of any kind -- so the definition is this package's own, stated
in include/s2st_hip.h next to ``s2st_time_scale_pcm16`` and restated here, operation for operation, by ``host_time_scale``.
**Parity unpinned: the reference has no time-scale modification.**

Waveform-similarity overlap-add on integers (no table, no floating point).  ``x``: ``n`` int16 samples, zero outside ``[0, n)``;
``m``: the output length; ``N``: an even frame length, ``Hs = N / 2``; ``D``: the search radius.  Cross-fade weights ``wr[i] =
((2 i + 1) 32768) // N``, ``wf[i] = 32768 - wr[i]``.  The output is built in ``ceil(m / Hs)`` hops:

* hop 0: ``p_0 = 0``, ``out[i] = x[i]``;
* hop ``j >= 1``: nominal position ``a_j = (j Hs n) // m``; template ``tpl[i] = x[p_{j-1} + Hs + i]`` (the natural continuation of
  what was written last); candidates ``c`` in ``[a_j - D, a_j + D]``; ``cost(c) = sum_i |x[c + i] - tpl[i]|``; ``p_j`` = the
  candidate of least cost, **ties to the smallest |c - a_j|, then to the smaller c**; ``out[j Hs + i] = (x[p_j + i] wr[i] +
  tpl[i] wf[i] + 16384) >> 15``.

``m == n`` returns ``x``; a signal of exact period ``P <= D`` (``Hs >= P``) comes out as the same periodic signal; ``|p_j - a_j| <=
D``.  ``time_scale(..., scaler="device")`` runs csrc/time_scale.hip over a ragged batch in one launch (a workgroup per
recording walks the hops); ``scaler="host"`` is ``host_time_scale``.  The two agree bit for bit, outputs and positions.

``place`` is the placement rule of ``translate --timeline source`` (pure integers; see its docstring).
"""
from __future__ import annotations

import argparse
import ctypes as C
import sys
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .runtime import binding as bd

MAX_N = 4096   # the device form's limits (csrc/time_scale.hip: the region and the template live in LDS)
MAX_D = 2048

# the defaults (design choices, not measurements; README.md states them)
FRAME_MS = 40.0      # N = 2 round(0.020 rate): two hops of 20 ms, a few pitch periods of speech
SEARCH_MS = 10.0     # D = round(0.010 rate): one period of a 100 Hz voice on either side
MAX_TEMPO = 1.25     # translate --max-tempo: how far a segment is compressed to stay in its slot
MIN_RATIO, MAX_RATIO = 0.5, 2.0  # time_scale refuses n / m outside (a quality guard: the kernel itself is total)


def geometry(rate: int, frame_ms: float = FRAME_MS, search_ms: float = SEARCH_MS) -> Tuple[int, int]:
    """(N, D) in samples at ``rate``: 960 and 240 at 24 kHz with the defaults."""
    return 2 * int(round(frame_ms / 2000.0 * rate)), int(round(search_ms / 1000.0 * rate))


def _check(N: int, D: int) -> None:
    if N < 2 or N > MAX_N or N % 2 or D < 0 or D > MAX_D:
        raise ValueError(f"time scale: needs an even frame length 2 <= N <= {MAX_N} and a search radius 0 <= D <= {MAX_D} "
                         f"(N {N}, D {D})")


def n_hops(m: int, N: int) -> int:
    return -(-int(m) // (N // 2))


def scaled_len(n: int, tempo_milli: int) -> int:
    """``ceil(n * 1000 / tempo_milli)``: the length of ``n`` samples at a tempo of ``tempo_milli`` / 1000."""
    return -(-int(n) * 1000 // int(tempo_milli))


def tempo_milli(tempo: float) -> int:
    t = int(round(1000.0 * float(tempo)))
    if t < 1:
        raise ValueError(f"tempo {tempo!r} must be positive")
    return t


def host_time_scale(x: np.ndarray, m: int, N: int, D: int) -> Tuple[np.ndarray, np.ndarray]:
    """The module docstring's rules in numpy, vectorised over the candidates of a hop.  Returns (int16 [m], int32 positions
    [ceil(m / Hs)])."""
    _check(N, D)
    x = np.asarray(x)
    if x.dtype != np.int16 or x.ndim != 1:
        raise ValueError("time scale takes 1-D int16 PCM")
    n, m, Hs = int(x.shape[0]), int(m), N // 2
    if m < 0:
        raise ValueError("time scale: the output length must not be negative")
    J = n_hops(m, N)
    # zeros around the recording: reads go down to a_j - D >= -D and up to a_j + D + 2 Hs with a_j <= max(n - 1, 0)
    xp = np.zeros(D + n + D + 2 * Hs + 1, np.int32)
    xp[D:D + n] = x
    i = np.arange(Hs, dtype=np.int64)
    wr = ((2 * i + 1) * 32768 // N).astype(np.int32)
    wf = (32768 - wr).astype(np.int32)
    out = np.zeros(J * Hs, np.int32)
    pos = np.zeros(J, np.int32)
    out[:min(Hs, J * Hs)] = xp[D:D + Hs][:min(Hs, J * Hs)]
    k = np.arange(2 * D + 1, dtype=np.int64)
    tie = np.abs(k - D) * (2 * D + 2) + k  # among equal costs: the smallest |c - a_j|, then the smaller c
    p = 0
    for j in range(1, J):
        a = (j * Hs * n) // m
        tpl = xp[D + p + Hs:D + p + 2 * Hs]
        region = xp[a:a + 2 * D + Hs]  # x[a - D .. a + D + Hs)
        cost = np.abs(np.lib.stride_tricks.sliding_window_view(region, Hs) - tpl).sum(axis=1, dtype=np.int64)
        best = np.flatnonzero(cost == cost.min())
        kb = int(best[np.argmin(tie[best])])
        p = a - D + kb
        pos[j] = p
        out[j * Hs:(j + 1) * Hs] = (xp[D + p:D + p + Hs] * wr + tpl * wf + 16384) >> 15
    return out[:m].astype(np.int16), pos


def _as_pcm16(w) -> np.ndarray:
    if isinstance(w, torch.Tensor):
        w = w.detach().cpu().numpy()
    w = np.asarray(w)
    if w.dtype != np.int16 or w.ndim != 1:
        raise ValueError("time scale takes 1-D int16 PCM (segmentation.host_pcm16 rounds a float waveform)")
    return np.ascontiguousarray(w)


def time_scale(waves: Sequence, out_lens: Sequence[int], rate: Optional[int] = None, N: Optional[int] = None,
               D: Optional[int] = None, device=None, scaler: str = "device", guard: bool = True) -> List[Tuple[np.ndarray, np.ndarray]]:
    """A ragged batch of int16 recordings in one call: recording b becomes ``out_lens[b]`` samples long.  ``N`` / ``D``: the
    frame length and search radius in samples (default: ``geometry(rate)``).  ``scaler="device"``: ``s2st_time_scale_pcm16``,
    one upload, one launch, one read-back; ``"host"``: ``host_time_scale`` per recording -- the same arrays.  Returns [(int16
    [m_b], int32 positions [hops_b])].  ``n / m`` outside [1/2, 2] is refused (``guard``): beyond it whole syllables are dropped
    or repeated, which is no longer a change of tempo; the definition and the kernel themselves are total."""
    if scaler not in ("device", "host"):
        raise ValueError(f"scaler {scaler!r}: expected 'device' or 'host'")
    if N is None or D is None:
        if rate is None:
            raise ValueError("time scale: give the sample rate, or N and D")
        gN, gD = geometry(int(rate))
        N, D = (gN if N is None else N), (gD if D is None else D)
    N, D = int(N), int(D)
    _check(N, D)
    parts = [_as_pcm16(w) for w in waves]
    ms = [int(v) for v in out_lens]
    if len(ms) != len(parts):
        raise ValueError("time scale: one output length per recording")
    for b, (p, m) in enumerate(zip(parts, ms)):
        n = int(p.shape[0])
        if m < 0:
            raise ValueError(f"time scale: recording {b}: the output length must not be negative")
        if guard and (n > MAX_RATIO * m or n < MIN_RATIO * m):
            raise ValueError(f"time scale: recording {b}: {n} samples to {m} is a tempo of {n / m if m else float('inf'):.3f}, "
                             f"outside [{MIN_RATIO}, {MAX_RATIO}]")
    if scaler == "host":
        return [host_time_scale(p, m, N, D) for p, m in zip(parts, ms)]
    B = len(parts)
    if B == 0:
        return []
    if device is None:
        device = torch.device("cpu") if bd.is_emulator() else torch.device("cuda", torch.cuda.current_device())
    dev = torch.device(device)
    lens = [int(p.shape[0]) for p in parts]
    hops = [n_hops(m, N) for m in ms]
    flat = torch.from_numpy(np.concatenate(parts) if sum(lens) else np.zeros(1, np.int16)).to(dev)  # ONE upload of the samples
    bd.require_device(flat)
    offs = np.zeros((3, B + 1), np.int64)
    for r, v in enumerate((lens, ms, hops)):
        offs[r, 1:] = np.cumsum(v)
    off = torch.from_numpy(offs).to(dev)
    out = torch.empty(max(int(offs[1, B]), 1), dtype=torch.int16, device=dev)
    pos = torch.empty(max(int(offs[2, B]), 1), dtype=torch.int32, device=dev)
    rc = bd.lib().s2st_time_scale_pcm16(flat.data_ptr(), off[0].data_ptr(), off[1].data_ptr(), B, N, D, out.data_ptr(),
                                        pos.data_ptr(), off[2].data_ptr(), C.c_void_p(bd.stream_ptr()))
    bd.check(rc, "s2st_time_scale_pcm16")
    out, pos = out.cpu().numpy(), pos.cpu().numpy()
    return [(out[offs[1, b]:offs[1, b + 1]].copy(), pos[offs[2, b]:offs[2, b + 1]].copy()) for b in range(B)]


def place(starts: Sequence[int], natural: Sequence[int], total: int, tempo_milli: int = 1000,
          max_tempo_milli: int = int(MAX_TEMPO * 1000)) -> Tuple[List[int], List[int]]:
    """Where translated segments go on the source's time line.  All quantities are integers in output samples: ``starts[k]``
    = where kept segment k began in the source (non-decreasing), ``natural[k]`` = the length of its translation, ``total`` =
    the source's length.  Segment k's slot ends where the next one's begins (the last: at ``total``).  With ``q_0 = 0``:

        start_k = max(starts[k], q_{k-1});  avail = slot_end - start_k
        want = ceil(natural[k] 1000 / tempo_milli);  least = ceil(natural[k] 1000 / max_tempo_milli)
        m_k = want if want <= avail else min(want, max(avail, least));  q_k = start_k + m_k

    Speech is never slower than ``tempo_milli``; a segment that does not fit even at ``max_tempo_milli`` runs over and
    pushes the next one.  Returns (out_start [K], out_len [K]); the output is ``max(total, q_last)`` samples long."""
    starts, natural, total = [int(v) for v in starts], [int(v) for v in natural], int(total)
    tempo_milli, max_tempo_milli = int(tempo_milli), int(max_tempo_milli)
    if len(starts) != len(natural):
        raise ValueError("place: one start per segment")
    if tempo_milli < 1 or max_tempo_milli < tempo_milli:
        raise ValueError(f"place: needs 1 <= tempo_milli <= max_tempo_milli (tempo_milli {tempo_milli}, max_tempo_milli "
                         f"{max_tempo_milli})")
    if total < 0 or any(v < 0 for v in starts) or any(v < 0 for v in natural):
        raise ValueError("place: starts, lengths and the total must not be negative")
    if any(b < a for a, b in zip(starts, starts[1:])):
        raise ValueError("place: the starts must not decrease")
    out_start, out_len, q = [], [], 0
    for k, (a, n) in enumerate(zip(starts, natural)):
        slot_end = starts[k + 1] if k + 1 < len(starts) else total
        start = max(a, q)
        avail = slot_end - start
        want, least = scaled_len(n, tempo_milli), scaled_len(n, max_tempo_milli)
        m = want if want <= avail else min(want, max(avail, least))
        out_start.append(start)
        out_len.append(m)
        q = start + m
    return out_start, out_len


# ---- the command-line side ---------------------------------------------------------------------------------------------------
def add_time_scale_flags(p, tempo_required: bool = False) -> None:
    """The flags ``translate`` and this CLI share."""
    a = p.add_argument
    a("--tempo", type=float, default=None if tempo_required else 1.0, required=tempo_required,
      help="speak this much faster (> 1) or slower (< 1) at the same pitch: an output of n samples becomes "
           "ceil(n * 1000 / round(1000 * F)) long; 1.0: nothing is done")
    a("--time-scaler", default="device", choices=["device", "host"],
      help="s2st_time_scale_pcm16 on the device, or the same rules in numpy on the host (same files)")


def make_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="s2st_amd.time_scale", allow_abbrev=False)
    p.add_argument("audio", nargs="+", help="audio files; ids are the file stems")
    p.add_argument("--results-path", required=True)
    add_time_scale_flags(p, tempo_required=True)
    p.add_argument("--frame-ms", type=float, default=FRAME_MS, help="the frame: two hops (a design choice, not a measurement)")
    p.add_argument("--search-ms", type=float, default=SEARCH_MS, help="the search radius around a hop's nominal position")
    return p


def main(argv: Optional[List[str]] = None, device: Optional[torch.device] = None) -> Dict:
    from .data.audio_utils import read_audio
    from .inference_common import default_device, write_pcm16
    from .segmentation import host_pcm16
    args = make_parser().parse_args(argv)
    try:
        tm = tempo_milli(args.tempo)
    except ValueError as e:
        raise SystemExit(f"time_scale: {e}")
    ids = [Path(f).stem for f in args.audio]
    if len(set(ids)) != len(ids):
        raise SystemExit(f"time_scale: duplicate ids {sorted({i for i in ids if ids.count(i) > 1})}")
    if args.time_scaler == "device" and device is None:
        device = default_device("time_scale", needed_for="--time-scaler device", without="--time-scaler host")
    audio = [read_audio(f) for f in args.audio]
    out_root = Path(args.results_path)
    out_root.mkdir(exist_ok=True, parents=True)
    written: List[Optional[str]] = [None] * len(audio)
    for rate in sorted({r for _, r in audio}):  # recordings are scaled at their own rate, all files of one rate in one call
        idx = [i for i, (_, r) in enumerate(audio) if r == rate]
        pcm = [host_pcm16(audio[i][0]) for i in idx]
        N, D = geometry(rate, args.frame_ms, args.search_ms)
        try:
            res = time_scale(pcm, [scaled_len(len(p), tm) for p in pcm], N=N, D=D, device=device, scaler=args.time_scaler)
        except ValueError as e:
            raise SystemExit(f"time_scale: {e}")
        for i, (y, _) in zip(idx, res):
            written[i] = str(out_root / f"{ids[i]}.wav")
            write_pcm16(written[i], y, rate)
    return {"recordings": len(audio), "tempo_milli": tm, "files": written}


def cli_main():
    r = main(sys.argv[1:])
    print(f"scaled {r['recordings']} recordings to a tempo of {r['tempo_milli'] / 1000:g}; {len(r['files'])} files under the "
          f"results path")


if __name__ == "__main__":
    cli_main()
