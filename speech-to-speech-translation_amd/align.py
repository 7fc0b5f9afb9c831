"""``align``: where in the source audio is each token of the source transcript, by the model's own CTC head.

    python -m s2st_amd.align DATA --config-yaml config.yaml --gen-subset SPLIT --path CKPT --results-path OUT \
        [--max-tokens N | --batch-size N] [--aligner device|host] [--frame-shift-ms 40]

The reference has no counterpart (it never materialises an alignment): the definition is
``ctc_align``'s, ties to the smaller jump.  **Parity unpinned**: the reference computes no alignment; torchaudio, whose
``forced_align`` breaks ties differently, is absent and is not reproduced.

For each batch: ``forward_encoder``, the log-probabilities of ``get_normalized_probs(log_probs=True)`` (``ctc_proj`` over
encoder tap 0, one frame per 4 input frames), the encoder lengths as frame counts, and as target what the criterion trains
this head on: ``src_text[:src_text_len]``, eos included (s2st_loss.py:236-243).  ``OUT/align-SPLIT.txt`` holds one line per
utterance in manifest order,

    id \\t n_frames \\t n_tokens \\t score \\t score/n_frames \\t sym:start:end:tok_score ...

with spans in frames (``--frame-shift-ms`` is the length of one, quoted in the closing line) and floats as ``%.9g`` of the
fp32 value, so ``--aligner device`` (csrc/ctc_align.hip) and ``--aligner host`` (numpy, same rules) write the same bytes.
An utterance without a path (fewer frames than tokens + repeats) keeps its line with ``-inf`` and no token fields and is
counted in the closing line.
"""
from __future__ import annotations

import argparse
import os
import sys
from pathlib import Path
from typing import List, Optional

import numpy as np
import torch

from . import ctc_align
from .inference_common import batch_iterator, default_device, load_task_model_dataset


def make_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="s2st_amd.align", allow_abbrev=False)
    a = p.add_argument
    a("data")
    a("--user-dir", default=None, help="accepted for command-line compatibility (this package IS the plugin)")
    a("--config-yaml", default="config.yaml")
    a("--task", default="s2s_translation")
    a("--path", required=True, help="checkpoint (reference .pt layout)")
    a("--gen-subset", default="test")
    a("--results-path", required=True, help="align-<subset>.txt is written there")
    a("--max-tokens", type=int, default=None)
    a("--batch-size", "--max-sentences", type=int, default=None, dest="batch_size")
    a("--required-batch-size-multiple", type=int, default=1)
    a("--num-shards", type=int, default=1)
    a("--shard-id", type=int, default=0)
    a("--seed", type=int, default=1)
    a("--aligner", default="device", choices=["device", "host"],
      help="s2st_ctc_align_f32 on the device, or the same rules in numpy on the host (same file)")
    a("--frame-shift-ms", type=float, default=40.0, help="length of one encoder frame (10 ms features, subsampled by 4)")
    a("--precise-gemm", action="store_true", help="bf16x3 GEMMs (fp32-accurate; parity runs)")
    return p


def f32(x) -> str:
    """``%.9g`` of the fp32 value: nine digits identify an fp32 number, so equal floats give equal text."""
    return "%.9g" % float(np.float32(x))


def format_line(utt_id: str, n_frames: int, symbols: List[str], al) -> str:
    head = [utt_id, str(n_frames), str(len(symbols))]
    if not al.score > -np.inf:
        return "\t".join(head + ["-inf", "-inf"])
    per_frame = np.float32(al.score) / np.float32(n_frames)
    fields = [f"{sym}:{int(s)}:{int(e)}:{f32(q)}" for sym, (s, e), q in zip(symbols, al.spans, al.tok_scores)]
    return "\t".join(head + [f32(al.score), f32(per_frame)] + fields)


def main(argv: Optional[List[str]] = None, device: Optional[torch.device] = None, on_model_built=None) -> dict:
    args = make_parser().parse_args(argv)
    if args.max_tokens is None and args.batch_size is None:
        args.max_tokens = 8000  # generate_waveform's default
    if device is None:
        device = default_device("align")
    task, model, margs, dataset = load_task_model_dataset(args, device, None, on_model_built)
    if not model.engine.cfg.has_ctc:
        raise SystemExit("align: the checkpoint has no CTC head (--ctc-weight 0): there is nothing to align with")
    src_texts = getattr(dataset, "src_texts", None)  # (a manifest without the column loads as empty strings)
    if src_texts is None or all(not t for t in src_texts):
        raise SystemExit(f"align: the split {args.gen_subset} has no src_text column: the CTC head emits source tokens, "
                         f"so there is no transcript to align")
    src_dict = task.source_dictionary
    model.eval()
    lines = {}
    with torch.no_grad():
        for sample in batch_iterator(task, dataset, args):
            if sample is None or len(sample) == 0 or "net_input" not in sample:
                continue
            ni = sample["net_input"]
            enc = model.forward_encoder(ni["src_speech"], ni["src_speech_lens"], collated_audios=ni.get("collated_audios_orig"),
                                        padding_mask=ni.get("padding_mask"), speaker=sample.get("speaker"))
            lprobs = model.get_normalized_probs((None, None, enc), log_probs=True)  # [B, E, V]
            B, E, _ = lprobs.shape
            pad = enc["encoder_padding_mask"]
            n_frames = (E - pad[0].sum(1)).tolist() if pad else [E] * B
            tl = sample["src_text_len"].tolist()
            targets = [sample["src_text"][b, :tl[b]].tolist() for b in range(B)]
            als = ctc_align.forced_align(lprobs, targets, n_frames, blank=0, layout="BTV", aligner=args.aligner)
            for b, idx in enumerate(sample["id"].tolist()):
                utt = dataset.ids[idx] if getattr(dataset, "ids", None) else str(idx)
                lines[idx] = (format_line(str(utt), int(n_frames[b]), [src_dict[t] for t in targets[b]], als[b]),
                              bool(als[b].score > -np.inf), int(n_frames[b]))
    Path(args.results_path).mkdir(exist_ok=True, parents=True)
    out_path = os.path.join(args.results_path, f"align-{args.gen_subset}.txt")
    n_inf = sum(1 for _, ok, _ in lines.values() if not ok)
    frames = sum(n for _, ok, n in lines.values() if ok)
    with open(out_path, "w", encoding="utf-8") as f:
        for idx in sorted(lines):  # manifest order
            f.write(lines[idx][0] + "\n")
        f.write(f"Aligned {len(lines) - n_inf} of {len(lines)} utterances of {args.gen_subset} ({n_inf} without a path), "
                f"{frames} frames of {args.frame_shift_ms:g} ms = {frames * args.frame_shift_ms / 1000.0:.2f} s\n")
    return {"path": out_path, "utterances": len(lines), "infeasible": n_inf}


def cli_main():
    main(sys.argv[1:])


if __name__ == "__main__":
    cli_main()
