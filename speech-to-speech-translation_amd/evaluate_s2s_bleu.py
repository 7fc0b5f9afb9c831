"""``evaluate_s2s_bleu``: the counterpart of ``examples/s2s_trans/evalute_s2s_bleu.py`` (stage 8 of the recipes: ASR-BLEU,
the score the recipes report) for the MI355X path.

    python -m s2st_amd.evaluate_s2s_bleu --audio_manifest_file test.tsv --decode_save_path OUT \
        --decode_save_path_subdir wav_24000hz_griffin_lim --out_result_file asr_bleu.txt --scoring sacrebleu \
        --model_path /models/wav2vec2-large-960h-lv60-self

Row i >= 1 of the tab-separated manifest (row 0 is its header) gives an utterance id (column 0) and its reference text
(column 6).  ``<id>.wav`` is read from ``decode_save_path/decode_save_path_subdir`` (what ``generate_waveform`` wrote),
resampled to 16 kHz on the device, transcribed by the wav2vec 2.0 CTC recogniser (models/wav2vec2_ctc.py), and scored against
the reference with ``--scoring`` (``sacrebleu``: scoring.py).  Transcript and reference are punctuation-stripped
(``--punctuation_removal``, on by default as in the reference) and lower-cased; ``out_result_file`` gets one
``hypothesis<TAB>reference`` line per manifest row in manifest order, and the last line printed is
``Total Sentences: N, Sacrebleu: BLEU = ...``.

Differences from the reference script, stated:
  * the recogniser is loaded from a local directory (``--model_path``: ``config.json``, ``vocab.json``,
    ``pytorch_model.bin`` or ``model.safetensors``); nothing is downloaded;
  * utterances are batched by length: sorted by sample count, then consecutive ones join a padded batch while
    ``sentences x longest <= --batch_size`` samples (the reference batches in manifest order by the same rule); the
    output stays in manifest order;
  * only an utterance's valid frames are decoded, so ``--batch_size`` does not change a transcript;
  * ``--batch_size`` defaults to 1600000 samples (the reference: 160000; profiles/asr_bleu_rate.txt) and is clamped to
    16000000; wavs are read and resampled one length batch at a time;
  * ``--punctuation_removal`` takes ``true / false / 1 / 0`` (the reference's ``type=bool`` turns any non-empty string,
    ``False`` included, into True);
  * a wave too short for a single frame (under 400 samples at 16 kHz) gets an empty hypothesis (the reference decodes
    whatever its padded frames give);
  * ``--precise`` selects the bf16x3 products instead of bf16 operands;
  * ``--doc_column N`` (off by default; the reference has nothing like it) scores long recordings: the manifest rows that share
    the value of column N are one document's sentences, ``<doc>.wav`` is read instead of one wav per row, cut at its pauses
    (``segmentation.segment``: pieces of at most ``--max_piece_s`` seconds, the ``segment`` CLI's defaults otherwise), the
    trimmed pieces are transcribed in the same length batches, joined by a space per document and re-segmented against the
    document's rows (``resegment``: minimum edit distance, ``--resegmenter device|host``).  The output keeps its form: one
    ``hypothesis<TAB>reference`` line per manifest row.  **Parity unpinned: the reference has no re-segmentation.**
"""
from __future__ import annotations

import argparse
import csv
import os
import sys
import wave
from typing import List, Optional

import torch

from .data.audio_utils import get_waveform
from .models.wav2vec2_ctc import Wav2Vec2CTC, resample
from .scoring import build_scorer, remove_punctuation

# profiles/asr_bleu_rate.txt: utterances/s of the recogniser by --batch_size; the reference's default is 160000
DEFAULT_BATCH_SIZE = 1600000
# a padded batch's largest tensor (~102 elements per sample) is indexed in 32 bits by the engine: larger requests are clamped
MAX_BATCH_SAMPLES = 16000000
TARGET_RATE = 16000


def _bool(v: str) -> bool:
    return str(v).lower() not in ("0", "false", "no", "")


def make_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="s2st_amd.evaluate_s2s_bleu", allow_abbrev=False)
    a = p.add_argument
    a("--audio_manifest_file", required=True)
    a("--decode_save_path", required=True)
    a("--decode_save_path_subdir", default="wav_24000hz_griffin_lim")
    a("--out_result_file", required=True)
    a("--scoring", default="sacrebleu")
    a("--batch_size", type=int, default=DEFAULT_BATCH_SIZE, help="samples (at 16 kHz) per padded batch: sentences x longest")
    a("--punctuation_removal", type=_bool, default=True)
    a("--model_path", required=True, help="local directory of the recogniser in the Hugging Face layout")
    a("--precise", action="store_true", help="bf16x3 products (parity runs) instead of bf16 operands")
    a("--doc_column", type=int, default=None,
      help="score long recordings: rows that share this column's value are one document, read from <doc>.wav")
    a("--max_piece_s", type=float, default=30.0, help="--doc_column: the recogniser gets pieces of at most this many seconds")
    a("--resegmenter", default="device", choices=["device", "host"],
      help="--doc_column: s2st_reseg_i32 on the device, or the same rules in numpy on the host (same lines)")
    return p


def length_batches(lens: List[int], batch_size: int) -> List[List[int]]:
    """Indices sorted by length (ties by index), cut where ``sentences x longest`` would exceed ``batch_size`` (at most
    ``MAX_BATCH_SAMPLES``); an utterance longer than that is a batch of its own."""
    batch_size = min(int(batch_size), MAX_BATCH_SAMPLES)
    order = sorted(range(len(lens)), key=lambda i: (lens[i], i))
    out: List[List[int]] = []
    cur: List[int] = []
    for i in order:
        if cur and (len(cur) + 1) * lens[i] > batch_size:  # (sorted: lens[i] is the longest so far)
            out.append(cur)
            cur = []
        cur.append(i)
    if cur:
        out.append(cur)
    return out


def document_pieces(args, docs: List[str], wav_dir: str, device):
    """``--doc_column``: every document's wav cut at its pauses.  Returns ([(document index, float waveform of a trimmed
    piece)], [rate per document]); recordings are segmented at their own rate, all documents of one rate in one call."""
    from . import segmentation as sgm
    opt = sgm.segment_frames({"max_segment_s": args.max_piece_s}, None)
    audio = [get_waveform(os.path.join(wav_dir, d + ".wav"), mono=True, always_2d=False) for d in docs]
    pieces = []
    for rate in sorted({r for _, r in audio}):
        idx = [i for i, (_, r) in enumerate(audio) if r == rate]
        segs = sgm.segment([sgm.host_pcm16(audio[i][0]) for i in idx], rate, opt["min_len"], opt["max_len"], sgm.SMOOTH_FRAMES,
                           opt["silence_db"], opt["cut_penalty_db"], opt["pad"], device=device)
        for i, s in zip(idx, segs):
            for k in range(len(s)):
                if not s.dropped[k]:
                    a, b = (int(v) for v in s.trim_samples[k])
                    pieces.append((i, audio[i][0][a:b]))
    pieces.sort(key=lambda p: p[0])  # (stable: a document's pieces stay in order)
    return pieces, [r for _, r in audio]


def score_documents(args, rows, net, scorer, wav_dir: str) -> None:
    """``--doc_column``: transcribe the pieces of every document, re-segment the joined transcript against the document's
    rows, write and score one line per manifest row."""
    from .resegment import prepare, resegment_documents
    by_doc = {}
    for i, row in enumerate(rows):
        by_doc.setdefault(row[args.doc_column], []).append(i)
    docs = list(by_doc)
    pieces, rates = document_pieces(args, docs, wav_dir, net.device)
    n16 = [-(-len(w) * TARGET_RATE // rates[d]) for d, w in pieces]
    texts: List[str] = [""] * len(pieces)
    done = 0
    for batch in length_batches(n16, args.batch_size):
        at16k = {}
        for sr in sorted(set(rates[pieces[i][0]] for i in batch)):
            idx = [i for i in batch if rates[pieces[i][0]] == sr]
            at16k.update(zip(idx, resample([torch.from_numpy(pieces[i][1]) for i in idx], sr, TARGET_RATE, net.device)))
        for i, text in zip(batch, net.transcribe([at16k[i] for i in batch])):
            texts[i] = text
        done += len(batch)
        print(f"Processed: {done} pieces.", file=sys.stderr)
    prep = lambda t: prepare(t, args.punctuation_removal, True)  # noqa: E731
    refs = [prep(row[6]) for row in rows]
    hyp = {d: prep(" ".join(t for (j, _), t in zip(pieces, texts) if j == k)) for k, d in enumerate(docs)}
    try:
        cut = resegment_documents(hyp, {d: [refs[i] for i in ii] for d, ii in by_doc.items()}, False, args.resegmenter, net.device)
    except ValueError as e:
        raise SystemExit(f"evaluate_s2s_bleu: {e}")
    hyps: List[str] = [""] * len(rows)
    for d, ii in by_doc.items():
        for i, piece in zip(ii, cut[d]):
            hyps[i] = piece
    with open(args.out_result_file, "w") as fout:
        for hyp_i, ref in zip(hyps, refs):
            print("\t".join([hyp_i, ref]), file=fout)
            scorer.add_string(ref, hyp_i)


def main(argv: Optional[List[str]] = None, device=None, recogniser: Optional[Wav2Vec2CTC] = None):
    args = make_parser().parse_args(argv)
    scorer = build_scorer(args.scoring, None)
    net = recogniser if recogniser is not None else Wav2Vec2CTC.from_pretrained(args.model_path, device, args.precise)
    with open(args.audio_manifest_file, "r") as fin:
        rows = list(csv.reader(fin, delimiter="\t", quoting=csv.QUOTE_NONE))[1:]
    wav_dir = os.path.join(args.decode_save_path, args.decode_save_path_subdir)
    if args.doc_column is not None:
        score_documents(args, rows, net, scorer, wav_dir)
        result = scorer.result_string(4) if args.scoring == "sacrebleu" else scorer.result_string()
        print(f"Total Sentences: {len(rows)}, Sacrebleu: {result}")
        return scorer
    # lengths first (headers only), then one length batch at a time: read, resample per source rate, transcribe -- host and
    # device memory stay at one padded batch whatever the test set holds
    rates, n16 = [], []
    for row in rows:
        with wave.open(os.path.join(wav_dir, row[0] + ".wav"), "rb") as f:
            rates.append(f.getframerate())
            n16.append(-(-f.getnframes() * TARGET_RATE // f.getframerate()))
    hyps: List[str] = [""] * len(rows)
    done = 0
    for batch in length_batches(n16, args.batch_size):
        at16k = {}
        for sr in sorted(set(rates[i] for i in batch)):
            idx = [i for i in batch if rates[i] == sr]
            ws = [torch.from_numpy(get_waveform(os.path.join(wav_dir, rows[i][0] + ".wav"), mono=True, always_2d=False)[0])
                  for i in idx]
            at16k.update(zip(idx, resample(ws, sr, TARGET_RATE, net.device)))
        for i, text in zip(batch, net.transcribe([at16k[i] for i in batch])):
            hyps[i] = text
        done += len(batch)
        print(f"Processed: {done} examples.", file=sys.stderr)
    with open(args.out_result_file, "w") as fout:
        for row, hyp in zip(rows, hyps):
            ref = row[6]
            if args.punctuation_removal:
                hyp, ref = remove_punctuation(hyp), remove_punctuation(ref)
            print("\t".join([hyp.lower(), ref.lower()]), file=fout)
            scorer.add_string(ref.lower(), hyp.lower())
    result = scorer.result_string(4) if args.scoring == "sacrebleu" else scorer.result_string()
    print(f"Total Sentences: {len(rows)}, Sacrebleu: {result}")
    return scorer


if __name__ == "__main__":
    main()
