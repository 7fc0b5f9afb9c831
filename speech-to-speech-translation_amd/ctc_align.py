"""CTC forced alignment: where in the audio is each token of a GIVEN transcript, and how well does the audio fit it?

The reference never materialises an alignment (SURVEY.md section 0 item 2 leaves "the Viterbi forced alignment" to the
build), so the definition is this package's own -- stated in include/s2st_hip.h next to ``s2st_ctc_align_f32`` and
restated here, operation for operation, by ``host_forced_align``:

* extended sequence ``blank, y0, blank, y1, .., blank`` (S = 2 L + 1 states);
* ``d[0][0] = lp[0][blank]``, ``d[0][1] = lp[0][y0]``, every other ``d[0][s]`` is -inf; for t >= 1
  ``d[t][s] = max(d[t-1][s], d[t-1][s-1], d[t-1][s-2] if ext[s] != blank and ext[s] != ext[s-2]) + lp[t][ext[s]]``,
  one fp32 add;
* **ties go to the smaller jump**: stay wins over +1, +1 over +2 (a larger jump replaces a smaller one only when strictly
  greater); the path ends in the last state only if it is strictly better than the one before it;
* a NaN log-probability counts as -inf; -inf is IEEE -inf;
* a token's score is the fp32 sum, in frame order, of its emitted log-probabilities divided once by its frame count.

``forced_align(..., aligner="device")`` runs csrc/ctc_align.hip; ``aligner="host"`` applies the same rules in numpy fp32
to log-probabilities read back from the device.  The two agree bit for bit (integers equal, floats ``==``).

**Parity unpinned**: the reference computes no alignment; torchaudio (whose ``forced_align`` breaks ties differently) is
absent.
"""
from __future__ import annotations

import collections
import ctypes as C
from typing import List, Optional, Sequence

import numpy as np
import torch

from .runtime import binding as bd

MAX_STATES = 2049  # the device form's limit on 2 L + 1 (csrc/ctc_align.hip)
ERR_SHAPE = -2

# frame_tok [E] int32 (target index, -1 blank, -2 behind the utterance / infeasible), spans [L][2] int32 (start, end
# exclusive; -1 when infeasible), tok_scores [L] fp32, score fp32 (-inf when no path exists)
Alignment = collections.namedtuple("Alignment", "frame_tok spans tok_scores score")
Segment = collections.namedtuple("Segment", "text start end score")

_NEG = np.float32(-np.inf)


def _infeasible(E: int, L: int) -> Alignment:
    return Alignment(np.full(E, -2, np.int32), np.full((L, 2), -1, np.int32), np.zeros(L, np.float32), _NEG)


def host_forced_align(lp: np.ndarray, target: Sequence[int], blank: int = 0, n_frames: Optional[int] = None) -> Alignment:
    """One utterance: ``lp`` [E][V] fp32 log-probabilities of which the first ``n_frames`` (default: all) are valid.
    The rules of the module docstring in fp32, in the kernel's order."""
    lp = np.asarray(lp, dtype=np.float32)
    E, V = lp.shape
    T = E if n_frames is None else min(max(int(n_frames), 0), E)
    L = len(target)
    S = 2 * L + 1
    if T == 0:
        return _infeasible(E, L)
    ext = np.full(S, blank, np.int64)
    ext[1::2] = np.clip(np.asarray(target, np.int64), 0, V - 1)
    em = lp[:T][:, ext]  # [T][S]: only the S columns of a frame are gathered
    em = np.where(np.isnan(em), _NEG, em)
    has2 = np.zeros(S, bool)
    has2[3::2] = ext[3::2] != ext[1:-2:2]
    d = np.full(S + 2, _NEG, np.float32)  # two -inf guard slots in front
    d[2] = em[0, 0]
    if S > 1:
        d[3] = em[0, 1]
    bp = np.zeros((T, S), np.uint8)
    with np.errstate(invalid="ignore"):
        for t in range(1, T):
            best = d[2:].copy()
            k = bp[t]
            m = d[1:-1] > best  # strict: a tie stays
            best[m] = d[1:-1][m]
            k[m] = 1
            m = has2 & (d[:-2] > best)
            best[m] = d[:-2][m]
            k[m] = 2
            d[2:] = best + em[t]
    sc, end = d[2 + S - 1], S - 1
    if S > 1 and not sc > d[2 + S - 2]:
        sc, end = d[2 + S - 2], S - 2
    if not sc > _NEG:
        return _infeasible(E, L)
    frame_tok = np.full(E, -2, np.int32)
    s = end
    for t in range(T - 1, -1, -1):
        frame_tok[t] = (s >> 1) if (s & 1) else -1
        if t > 0:
            s -= int(bp[t, s])
    spans = np.full((L, 2), -1, np.int32)
    scores = np.zeros(L, np.float32)
    for i in range(L):
        fr = np.nonzero(frame_tok[:T] == i)[0]
        spans[i] = (fr[0], fr[-1] + 1)
        acc = np.float32(0.0)
        for v in lp[fr[0]:fr[-1] + 1, ext[2 * i + 1]]:  # in frame order
            acc = np.float32(acc + v)
        scores[i] = acc / np.float32(len(fr))
    return Alignment(frame_tok, spans, scores, np.float32(sc))


def _as_list(x) -> List[int]:
    if isinstance(x, torch.Tensor):
        return [int(v) for v in x.cpu().tolist()]
    return [int(v) for v in x]


def forced_align(lprobs: torch.Tensor, targets: Sequence[Sequence[int]], in_lens, blank: int = 0, layout: str = "BTV",
                 aligner: str = "device", route: int = 0) -> List[Alignment]:
    """``lprobs``: device fp32 log-probabilities, [B][E][V] (``layout="BTV"``) or [E][B][V] (``"TBV"``), read in place
    through its strides (only the last dimension must be contiguous); ``targets``: one list of ids per utterance;
    ``in_lens``: the valid frames of each.  ``route``: 0 picks, 1 keeps the back-pointers in LDS, 2 in a workspace (device
    form only).  Returns one ``Alignment`` per utterance."""
    if layout not in ("BTV", "TBV"):
        raise ValueError(f"layout {layout!r}: expected 'BTV' or 'TBV'")
    if aligner not in ("device", "host"):
        raise ValueError(f"aligner {aligner!r}: expected 'device' or 'host'")
    if lprobs.dim() != 3 or lprobs.dtype != torch.float32:
        raise ValueError("forced_align expects a 3-d fp32 tensor of log-probabilities")
    bd.require_device(lprobs)
    bdim, tdim = (0, 1) if layout == "BTV" else (1, 0)
    B, E, V = lprobs.shape[bdim], lprobs.shape[tdim], lprobs.shape[2]
    targets = [_as_list(t) for t in targets]
    lens = _as_list(in_lens)
    if len(targets) != B or len(lens) != B:
        raise ValueError(f"{B} utterances, {len(targets)} targets, {len(lens)} lengths")
    if not 0 <= blank < V:
        raise ValueError(f"blank {blank} outside the vocabulary of {V}")
    for b, t in enumerate(targets):
        if any(not 0 <= y < V for y in t):
            raise ValueError(f"target {b} holds an id outside the vocabulary of {V}")
    if aligner == "host":
        host = lprobs.detach().cpu().numpy()  # (the device-to-host copy is part of this form)
        return [host_forced_align(host[b] if layout == "BTV" else host[:, b], targets[b], blank, lens[b]) for b in range(B)]
    if V > 1 and lprobs.stride(2) != 1:
        raise ValueError("forced_align reads lprobs in place: its last dimension must be contiguous")
    dev = lprobs.device
    Lmax = max([len(t) for t in targets] + [0])
    tgt = torch.zeros(B, max(Lmax, 1), dtype=torch.int64)
    for b, t in enumerate(targets):
        tgt[b, :len(t)] = torch.tensor(t, dtype=torch.int64)
    tgt = tgt[:, :Lmax].contiguous().to(dev) if Lmax else tgt.to(dev)
    tl = torch.tensor([len(t) for t in targets], dtype=torch.int32).to(dev)
    il = torch.tensor(lens, dtype=torch.int32).to(dev)
    frame_tok = torch.empty(B, E, dtype=torch.int32, device=dev)
    ts = torch.empty(B, Lmax, dtype=torch.int32, device=dev)
    te = torch.empty(B, Lmax, dtype=torch.int32, device=dev)
    tsc = torch.empty(B, Lmax, dtype=torch.float32, device=dev)
    score = torch.empty(B, dtype=torch.float32, device=dev)
    lib = bd.lib()
    ws, ws_bytes = None, 0
    if route != 1 and 2 * Lmax + 1 <= MAX_STATES:
        ws_bytes = int(lib.s2st_ctc_align_workspace(B, E, Lmax))
        ws = torch.empty(max(ws_bytes, 4), dtype=torch.uint8, device=dev)
    rc = lib.s2st_ctc_align_f32(lprobs.data_ptr(), lprobs.stride(bdim), lprobs.stride(tdim), tgt.data_ptr(), Lmax,
                                il.data_ptr(), tl.data_ptr(), B, E, V, blank, route, frame_tok.data_ptr(),
                                ts.data_ptr() if Lmax else None, te.data_ptr() if Lmax else None,
                                tsc.data_ptr() if Lmax else None, score.data_ptr(), bd.ptr(ws), ws_bytes,
                                C.c_void_p(bd.stream_ptr()))
    if rc == ERR_SHAPE:
        raise bd.S2STHipError(
            f"s2st_ctc_align_f32: E = {E}, longest target = {Lmax} is beyond the device form (2 L + 1 <= {MAX_STATES}; route 1 "
            f"also needs the back-pointers to fit LDS): use aligner=\"host\"" + (" or route=0" if route == 1 else ""))
    bd.check(rc, "s2st_ctc_align_f32")
    frame_tok, ts, te, tsc, score = (x.cpu().numpy() for x in (frame_tok, ts, te, tsc, score))
    out = []
    for b, t in enumerate(targets):
        n = len(t)
        out.append(Alignment(frame_tok[b], np.stack([ts[b, :n], te[b, :n]], axis=1), tsc[b, :n], score[b]))
    return out


def segments(alignment: Alignment, symbols: Sequence[str], sep: Optional[str] = None) -> List[Segment]:
    """Merge the token spans into words: ``symbols[i]`` is the text of target token i; tokens equal to ``sep`` separate
    words and belong to none (``sep=None``: every token is a segment of its own).  A segment spans from its first token's
    start to its last token's end; its score is the mean of its tokens' scores weighted by their frame counts.  An
    infeasible alignment has no segments."""
    if len(symbols) != len(alignment.spans):
        raise ValueError(f"{len(symbols)} symbols for {len(alignment.spans)} aligned tokens")
    if not alignment.score > _NEG:
        return []
    out, cur = [], []

    def close():
        if cur:
            n = [int(alignment.spans[i][1] - alignment.spans[i][0]) for i in cur]
            sc = sum(float(alignment.tok_scores[i]) * k for i, k in zip(cur, n)) / sum(n)
            out.append(Segment("".join(symbols[i] for i in cur), int(alignment.spans[cur[0]][0]),
                               int(alignment.spans[cur[-1]][1]), sc))
            cur.clear()

    for i, sym in enumerate(symbols):
        if sep is not None and sym == sep:
            close()
            continue
        cur.append(i)
        if sep is None:
            close()
    close()
    return out
