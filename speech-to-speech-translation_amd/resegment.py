"""Minimum-error re-segmentation: score the one-line hypothesis of a long recording against its reference sentences.

    python -m s2st_amd.resegment --hyp OUT/st.txt --ref REF.tsv --doc-column 0 --text-column 1 --out OUT/st.reseg.txt \
        [--scoring sacrebleu|wer] [--punctuation-removal true] [--lowercase true] [--char-level] [--resegmenter device|host]

``translate --segment long`` cuts a recording at its pauses, not at sentence ends, and writes one line per recording; a test
set's references are one row per sentence.  Corpus BLEU clips its n-gram counts per line, so the lines have to match: the
hypothesis words are aligned to the concatenated reference sentences at least edit distance and cut where the alignment crosses
each sentence boundary (what mwerSegmenter does in IWSLT-style evaluation), and the pieces are scored as usual.  The reference
has no such step and mwerSegmenter was not at hand, so the definition is this package's own, stated in include/s2st_hip.h next
to ``s2st_reseg_i32``.  **Parity unpinned: the reference has no re-segmentation, and no mwerSegmenter was at hand.**

Tokens are equal iff they are the same string (ids by first appearance).  ``h[0..n)``: the hypothesis; ``r[0..m)``: the
reference sentences joined; ``e_1 <= .. <= e_K = m``: where they end (``e_0 = 0``; ``ends[k]`` is read as ``min(max(ends[k],
e_{k-1}), m)``, the last as ``m``).  ``D`` is the Levenshtein table (``D[i][j] = min(D[i-1][j-1] + (h[i-1] != r[j-1]), D[i-1][j]
+ 1, D[i][j-1] + 1)``), ``dist = D[n][m]``; the path walks back from ``(n, m)`` and at every cell takes the first predecessor
that attains ``D[i][j]``: **ties go diagonal, then up, then left**.  ``c_k`` = the largest ``i`` with ``(i, e_k)`` on the path
(words inserted at a sentence boundary go to the earlier sentence), piece k = ``h[c_{k-1} .. c_k)``, ``seg_dist[k] = D[c_k][e_k]
- D[c_{k-1}][e_{k-1}]`` -- the Levenshtein distance of piece k to sentence k; the ``seg_dist`` add up to ``dist``, the least
summed distance over all cuts.

``host_resegment`` is that in numpy: a row of ``D`` per step (the left neighbour's chain as ``np.minimum.accumulate(a - idx)
+ idx``), 2-bit back-pointers, the walk back.  ``resegment(..., backend="device")`` runs csrc/reseg.hip over a ragged batch in
one launch: a workgroup per document, a skewed wavefront over strips of reference columns, and -- the other formulation -- no
back-pointers but the row of the previous crossing carried forward.  The two agree bit for bit.  A document beyond the device
form's limit (``MAX_TOKENS`` per side, ``MAX_WS_BYTES`` of workspace) is done by the host form, with a line on stderr.
"""
from __future__ import annotations

import argparse
import collections
import csv
import ctypes as C
import sys
from typing import Dict, Hashable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .runtime import binding as bd
from .scoring import build_scorer, remove_punctuation

ERR_SHAPE = -2
MAX_TOKENS = 32767            # per side (csrc/reseg.hip: a distance and a row share one dword)
MAX_WS_BYTES = 4 << 30        # one launch's workspace at most: larger batches are split, a larger document goes to the host

Resegmented = collections.namedtuple("Resegmented", "pieces cuts seg_dist dist")


def clamp_ends(ends: Sequence[int], m: int) -> np.ndarray:
    """``e_k = min(max(ends[k], e_{k-1}), m)``, the last one ``m``."""
    e = np.asarray(ends, dtype=np.int64).reshape(-1)
    if e.size == 0:
        raise ValueError("resegment: a document needs at least one reference sentence")
    e = np.minimum(np.maximum(np.maximum.accumulate(e), 0), int(m))
    e[-1] = int(m)
    return e.astype(np.int32)


def host_resegment(h: Sequence[int], r: Sequence[int], ends: Sequence[int]) -> Tuple[np.ndarray, np.ndarray, int]:
    """The module docstring's rules in numpy.  Returns (cuts int32 [K], seg_dist int32 [K], dist)."""
    h, r = np.asarray(h, dtype=np.int32).reshape(-1), np.asarray(r, dtype=np.int32).reshape(-1)
    n, m = int(h.shape[0]), int(r.shape[0])
    e = clamp_ends(ends, m)
    cols = np.unique(e)                                # the distinct boundary columns, ascending
    is_b = np.zeros(m + 1, bool)
    is_b[cols] = True
    idx = np.arange(m + 1, dtype=np.int32)
    W = (m + 4) // 4                                   # bytes per row of back-pointers: four cells each
    bp = np.zeros((n + 1, W), np.uint8)                # 0 diagonal, 1 up, 2 left
    Db = np.zeros((n + 1, len(cols)), np.int32)        # D at the boundary columns
    prev = idx.copy()
    Db[0] = prev[cols]
    cell = np.zeros(4 * W, np.uint8)

    def pack(row_bp, i):
        cell[:m + 1] = row_bp
        q = cell.reshape(W, 4)
        bp[i] = q[:, 0] | (q[:, 1] << 2) | (q[:, 2] << 4) | (q[:, 3] << 6)

    first = np.full(m + 1, 2, np.uint8)
    first[0] = 1
    pack(first, 0)
    a = np.empty(m + 1, np.int32)
    for i in range(1, n + 1):
        diag = prev[:-1] + (r != h[i - 1])
        up = prev[1:] + 1
        a[0] = i
        np.minimum(diag, up, out=a[1:])
        cur = np.minimum.accumulate(a - idx) + idx     # ... and the chain of left steps
        code = np.ones(m + 1, np.uint8)
        code[1:] = np.where(cur[1:] == diag, 0, np.where(cur[1:] == up, 1, 2))
        pack(code, i)
        Db[i] = cur[cols]
        prev = cur
    # the walk back: where the path first reaches a boundary column is the largest row it has there
    reach = {}
    i, j = n, m
    reach[j] = i
    while i > 0 or j > 0:
        code = (int(bp[i, j >> 2]) >> (2 * (j & 3))) & 3
        if code == 0:
            i, j = i - 1, j - 1
        elif code == 1:
            i -= 1
        else:
            j -= 1
        if is_b[j] and j not in reach:
            reach[j] = i
    at = {int(c): q for q, c in enumerate(cols)}
    cuts = np.array([reach[int(c)] for c in e], np.int32)
    y = np.array([Db[reach[int(c)], at[int(c)]] for c in e], np.int64)
    seg = np.diff(np.concatenate([[0], y])).astype(np.int32)
    return cuts, seg, int(prev[m])


def _ids(docs_tokens: Sequence[Sequence[Sequence[Hashable]]]) -> List[List[np.ndarray]]:
    """Token -> int32 id by first appearance, over everything given."""
    table: Dict[Hashable, int] = {}
    return [[np.fromiter((table.setdefault(t, len(table)) for t in seq), np.int32, len(seq)) for seq in doc]
            for doc in docs_tokens]


def _device_batches(shapes: List[Tuple[int, int, int]], idx: List[int]) -> List[List[int]]:
    """Consecutive documents while the padded batch's workspace stays within MAX_WS_BYTES."""
    out: List[List[int]] = []
    cur: List[int] = []
    ws = lambda ii: 4 * len(ii) * ((max(shapes[i][2] for i in ii) + 1) * (max(shapes[i][0] for i in ii) + 1) +  # noqa: E731
                                   max(shapes[i][1] for i in ii) + 1 + max(shapes[i][2] for i in ii))
    for i in idx:
        if cur and ws(cur + [i]) > MAX_WS_BYTES:
            out.append(cur)
            cur = []
        cur.append(i)
    if cur:
        out.append(cur)
    return out


def device_resegment(hs: Sequence[np.ndarray], rs: Sequence[np.ndarray], es: Sequence[np.ndarray], device=None,
                     ) -> List[Tuple[np.ndarray, np.ndarray, int]]:
    """One launch of ``s2st_reseg_i32`` over a ragged batch of id arrays: one upload, one read-back."""
    B = len(hs)
    if B == 0:
        return []
    if device is None:
        device = torch.device("cpu") if bd.is_emulator() else torch.device("cuda", torch.cuda.current_device())
    dev = torch.device(device)
    lens = np.zeros((3, B + 1), np.int64)
    for row, parts in enumerate((hs, rs, es)):
        lens[row, 1:] = np.cumsum([len(p) for p in parts])
    Nmax, Mmax, Kmax = (int(np.diff(lens[row]).max()) for row in range(3))
    flat = np.concatenate([np.asarray(p, np.int32).reshape(-1) for parts in (hs, rs, es) for p in parts] + [np.zeros(1, np.int32)])
    tok = torch.from_numpy(flat).to(dev)  # ONE upload of the tokens and the ends
    bd.require_device(tok)
    off = torch.from_numpy(lens).to(dev)
    nh, nr = int(lens[0, B]), int(lens[1, B])
    lib = bd.lib()
    ws_bytes = int(lib.s2st_reseg_workspace(B, Nmax, Mmax, Kmax))
    ws = torch.empty(max(ws_bytes // 4, 1), dtype=torch.int32, device=dev)
    nk = int(lens[2, B])
    out = torch.empty(2 * nk + B, dtype=torch.int32, device=dev)  # cuts, seg_dist, dist
    rc = lib.s2st_reseg_i32(tok.data_ptr(), off[0].data_ptr(), tok[nh:].data_ptr(), off[1].data_ptr(), tok[nh + nr:].data_ptr(),
                            off[2].data_ptr(), B, Nmax, Mmax, Kmax, out.data_ptr(), out[nk:].data_ptr(), out[2 * nk:].data_ptr(),
                            ws.data_ptr(), ws_bytes, C.c_void_p(bd.stream_ptr()))
    bd.check(rc, "s2st_reseg_i32")
    out = out.cpu().numpy()
    return [(out[lens[2, b]:lens[2, b + 1]].copy(), out[nk + lens[2, b]:nk + lens[2, b + 1]].copy(), int(out[2 * nk + b]))
            for b in range(B)]


def resegment(hyps: Sequence[Sequence[Hashable]], refs: Sequence[Sequence[Sequence[Hashable]]], backend: str = "device",
              device=None) -> List[Resegmented]:
    """``hyps[d]``: document d's hypothesis tokens; ``refs[d]``: its reference sentences, a token list each.  Returns per
    document ``Resegmented(pieces, cuts, seg_dist, dist)``: the hypothesis tokens of every sentence, ``c_1 .. c_K``, the
    Levenshtein distance of every piece to its sentence, and their sum.  ``backend="device"``: ``s2st_reseg_i32``;
    ``"host"``: ``host_resegment`` per document -- the same numbers."""
    if backend not in ("device", "host"):
        raise ValueError(f"backend {backend!r}: expected 'device' or 'host'")
    if len(hyps) != len(refs):
        raise ValueError("resegment: one list of reference sentences per hypothesis")
    for d, ref in enumerate(refs):
        if len(ref) == 0:
            raise ValueError(f"resegment: document {d} needs at least one reference sentence")
    ids = _ids([[h] + list(ref) for h, ref in zip(hyps, refs)])
    hs = [doc[0] for doc in ids]
    rs = [np.concatenate(doc[1:]) if len(doc) > 1 else np.zeros(0, np.int32) for doc in ids]
    es = [np.cumsum([len(s) for s in doc[1:]]).astype(np.int32) for doc in ids]
    res: List[Optional[Tuple[np.ndarray, np.ndarray, int]]] = [None] * len(hs)
    on_device: List[int] = []
    shapes = [(len(h), len(r), len(e)) for h, r, e in zip(hs, rs, es)]
    for d, (n, m, K) in enumerate(shapes):
        if backend == "device" and n <= MAX_TOKENS and m <= MAX_TOKENS and 4 * ((K + 1) * (n + 1) + m + 1 + K) <= MAX_WS_BYTES:
            on_device.append(d)
            continue
        if backend == "device":
            print(f"resegment: document {d} ({n} x {m} tokens, {K} sentences) is beyond the device form: done on the host",
                  file=sys.stderr)
        res[d] = host_resegment(hs[d], rs[d], es[d])
    for batch in _device_batches(shapes, on_device):
        for d, one in zip(batch, device_resegment([hs[d] for d in batch], [rs[d] for d in batch], [es[d] for d in batch], device)):
            res[d] = one
    out = []
    for h, (cuts, seg, dist) in zip(hyps, res):
        at = [0] + [int(c) for c in cuts]
        out.append(Resegmented([list(h[a:b]) for a, b in zip(at, at[1:])], cuts, seg, dist))
    return out


def levenshtein(pairs: Sequence[Tuple[Sequence[Hashable], Sequence[Hashable]]], backend: str = "device", device=None) -> List[int]:
    """The Levenshtein distance of every (a, b) of a batch of sentence pairs: ``resegment`` with one sentence each."""
    return [r.dist for r in resegment([a for a, _ in pairs], [[b] for _, b in pairs], backend, device)]


# ---- documents of text (both CLIs) -----------------------------------------------------------------------------------------------
def prepare(text: str, punctuation_removal: bool = True, lowercase: bool = True) -> str:
    """``evaluate_s2s_bleu``'s preparation, in its order: punctuation-only tokens dropped, then lower-cased."""
    if punctuation_removal:
        text = remove_punctuation(text)
    return text.lower() if lowercase else text


def tokens(text: str, char_level: bool = False) -> List[str]:
    return [c for c in text if not c.isspace()] if char_level else text.split()


def resegment_documents(hyp: Dict[str, str], docs: Dict[str, List[str]], char_level: bool = False, backend: str = "device",
                        device=None) -> Dict[str, List[str]]:
    """``hyp``: {document id: prepared hypothesis text}; ``docs``: {document id: its prepared reference sentences in order}.
    Returns {document id: one hypothesis piece per sentence} (words joined by a space; characters joined by nothing).  Refused,
    naming the id: a document on one side only, a document without reference rows."""
    for d in docs:
        if d not in hyp:
            raise ValueError(f"document {d!r} has reference rows but no hypothesis")
        if len(docs[d]) == 0:
            raise ValueError(f"document {d!r} has no reference rows")
    for d in hyp:
        if d not in docs:
            raise ValueError(f"document {d!r} has a hypothesis but no reference rows")
    order = list(docs)
    res = resegment([tokens(hyp[d], char_level) for d in order], [[tokens(s, char_level) for s in docs[d]] for d in order],
                    backend, device)
    join = "" if char_level else " "
    return {d: [join.join(p) for p in r.pieces] for d, r in zip(order, res)}


def read_hyp(path: str) -> Dict[str, str]:
    """``id<TAB>text`` lines, as ``translate`` writes them.  A duplicate id is refused."""
    out: Dict[str, str] = {}
    with open(path, encoding="utf-8") as f:
        for line in f:
            line = line.rstrip("\n")
            if not line:
                continue
            d, _, text = line.partition("\t")
            if d in out:
                raise ValueError(f"document {d!r} appears twice in {path}")
            out[d] = text
    return out


def read_ref(path: str, doc_column: int, text_column: int) -> Tuple[List[Tuple[str, str]], Dict[str, List[int]]]:
    """A TSV with a header row: ([(document id, text) per row], {document id: its row numbers in file order})."""
    with open(path, encoding="utf-8") as f:
        rows = list(csv.reader(f, delimiter="\t", quoting=csv.QUOTE_NONE))[1:]
    out, docs = [], {}
    for i, row in enumerate(rows):
        if max(doc_column, text_column) >= len(row):
            raise ValueError(f"{path}: row {i + 1} has {len(row)} columns")
        out.append((row[doc_column], row[text_column]))
        docs.setdefault(row[doc_column], []).append(i)
    return out, docs


def _bool(v: str) -> bool:
    return str(v).lower() not in ("0", "false", "no", "")


def scorer_for(scoring: str, char_level: bool):
    return build_scorer(scoring, None, {f"{scoring}_char_level": True} if char_level else None)


def make_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="s2st_amd.resegment", allow_abbrev=False)
    a = p.add_argument
    a("--hyp", required=True, help="id<TAB>text, one line per document (translate's st.txt / asr.txt)")
    a("--ref", required=True, help="TSV with a header row; the rows of one document id, in file order, are its sentences")
    a("--doc-column", type=int, default=0)
    a("--text-column", type=int, default=1)
    a("--out", required=True, help="gets one `hypothesis piece<TAB>reference` line per reference row, in reference order")
    a("--scoring", default=None, choices=["sacrebleu", "wer"], help="also score the written lines")
    a("--punctuation-removal", type=_bool, default=True)
    a("--lowercase", type=_bool, default=True)
    a("--char-level", action="store_true",
      help="tokens are the characters, spaces dropped (Chinese / Japanese targets); both columns are written without spaces")
    a("--resegmenter", default="device", choices=["device", "host"],
      help="s2st_reseg_i32 on the device, or the same rules in numpy on the host (same bytes)")
    return p


def main(argv: Optional[List[str]] = None, device: Optional[torch.device] = None) -> Dict:
    from .inference_common import default_device
    args = make_parser().parse_args(argv)
    try:
        hyp = read_hyp(args.hyp)
        rows, docs = read_ref(args.ref, args.doc_column, args.text_column)
        if not rows:
            raise ValueError(f"{args.ref} has no reference rows")
        if args.resegmenter == "device" and device is None:
            device = default_device("resegment", needed_for="--resegmenter device", without="--resegmenter host")
        prep = lambda t: prepare(t, args.punctuation_removal, args.lowercase)  # noqa: E731
        refs = [prep(t) for _, t in rows]
        pieces = resegment_documents({d: prep(t) for d, t in hyp.items()}, {d: [refs[i] for i in ii] for d, ii in docs.items()},
                                     args.char_level, args.resegmenter, device)
    except ValueError as e:
        raise SystemExit(f"resegment: {e}")
    lines: List[Optional[Tuple[str, str]]] = [None] * len(rows)
    for d, ii in docs.items():
        for i, piece in zip(ii, pieces[d]):
            lines[i] = (piece, "".join(tokens(refs[i], True)) if args.char_level else refs[i])
    with open(args.out, "w", encoding="utf-8") as f:
        for piece, ref in lines:
            f.write(f"{piece}\t{ref}\n")
    result = None
    if args.scoring:
        scorer = scorer_for(args.scoring, args.char_level)
        for piece, ref in lines:
            scorer.add_string(ref, piece)
        result = scorer.result_string(4) if args.scoring == "sacrebleu" else scorer.result_string()
        print(f"Total Sentences: {len(lines)}, Sacrebleu: {result}")
    return {"documents": len(docs), "sentences": len(lines), "result": result, "out": args.out}


if __name__ == "__main__":
    main(sys.argv[1:])
