"""``generate_text``: the counterpart of ``fairseq_cli/generate_for_s2st.py`` (stages 10 / 11 of the recipes,
run_baseline.sh) for the MI355X path: decode a split with the aux ASR or ST text decoder and score it.

    python -m s2st_amd.generate_text DATA --config-yaml config.yaml --gen-subset test_fisher --path checkpoint_last_avg15.pt \
        --max-tokens 50000 --beam 5 --scoring wer --results-path OUT

The reference swaps ``model.decoder`` for ``model.aux_asr_decoder`` (``--scoring wer``: source dictionary, targets
``src_text``) or ``model.aux_st_decoder`` (``--scoring sacrebleu``: target dictionary, targets ``tgt_text``) and runs
fairseq's SequenceGenerator (:107-110, 178-219); here ``--aux-decoder asr|st`` picks the head (default: by that rule) and
``AuxSequenceGenerator`` decodes, with the search on the device (``--search device``) or on the host (``--search host``,
the same hypotheses bit for bit).  Output in the reference's format (:288-333, 404-430): ``T-id``, then for the first
``--nbest`` hypotheses ``H-id score str``, ``D-id score str`` and ``P-id positional scores`` (base 2), the throughput line,
``Generate <subset> with beam=<b>: <result>``.  No ``S-`` lines: ``src_dict`` is ``None`` at that point of the reference.

``--scoring wer`` takes the scorer's options ``--wer-tokenizer none|13a --wer-lowercase --wer-remove-punct
--wer-char-level`` (scoring.py; ``13a`` is a restatement of sacrebleu's published rules, **parity unpinned**).
``--scoring sacrebleu`` decodes and writes the hypotheses -- the ``T-`` / ``D-`` lines are what an external sacrebleu scores
-- and computes no BLEU here (sacrebleu is not in the image): the closing line says so.  ``main()`` returns the scorer
(``None`` for sacrebleu), as the reference's does.
"""
from __future__ import annotations

import argparse
import math
import os
import sys
import time
from pathlib import Path
from typing import List, Optional

import torch

from .inference_common import batch_iterator, default_device, load_task_model_dataset
from .scoring import REFUSED_TOKENIZERS, TOKENIZERS, build_scorer

# profiles/aux_decode_rate.txt: the device form is faster than the host form beyond the spread of the repeats on both heads
# (2.2x / 3.9x in sentences/s at 20000 max-tokens, beam 5)
DEFAULT_SEARCH = "device"


def make_parser() -> argparse.ArgumentParser:
    """fairseq's ``options.get_generation_parser`` for what generate_for_s2st.py uses, by the fairseq names."""
    p = argparse.ArgumentParser(prog="s2st_amd.generate_text", allow_abbrev=False)
    a = p.add_argument
    a("data")
    a("--user-dir", default=None, help="accepted for command-line compatibility (this package IS the plugin)")
    a("--config-yaml", default="config.yaml")
    a("--task", default="s2s_translation")
    a("--path", required=True, help="checkpoint (reference .pt layout), e.g. the output of s2st_amd.average_checkpoints")
    a("--gen-subset", default="test")
    a("--results-path", default=None, help="write generate-<subset>.txt there (default: stdout)")
    a("--max-tokens", type=int, default=None)
    a("--batch-size", "--max-sentences", type=int, default=None, dest="batch_size")
    a("--required-batch-size-multiple", type=int, default=1)
    a("--num-shards", type=int, default=1)
    a("--shard-id", type=int, default=0)
    a("--seed", type=int, default=1)
    a("--beam", type=int, default=5)
    a("--nbest", type=int, default=1)
    a("--max-len-a", type=float, default=0.0)
    a("--max-len-b", type=int, default=200)
    a("--min-len", type=int, default=1)
    a("--lenpen", type=float, default=1.0)
    a("--unkpen", type=float, default=0.0)
    a("--scoring", default="wer", choices=["wer", "sacrebleu"])
    a("--wer-tokenizer", default="none", choices=list(TOKENIZERS) + list(REFUSED_TOKENIZERS),
      help="sacrebleu tokenizer applied before scoring: none, or 13a (restated from its published rules, parity "
           "unpinned); intl, zh and ja-mecab are refused")
    a("--wer-lowercase", action="store_true")
    a("--wer-remove-punct", action="store_true")
    a("--wer-char-level", action="store_true")
    a("--speaker-to-id", type=str, default=None)
    a("--use-hubert", type=str, default=None)
    a("--quiet", action="store_true")
    a("--precise-gemm", action="store_true", help="bf16x3 GEMMs (fp32-accurate; parity runs)")
    a("--search", default=DEFAULT_SEARCH, choices=["device", "host"],
      help="where the beam search runs: s2st_beam_step on the device, or numpy on the host (same hypotheses)")
    a("--aux-decoder", default=None, choices=["asr", "st"],
      help="the head to decode with (default: asr for --scoring wer, st for --scoring sacrebleu)")
    a("--max-batches", type=int, default=0, help="stop after this many batches (0: the whole split)")
    return p


def strip_pad(t: torch.Tensor, pad: int) -> torch.Tensor:
    return t[t.ne(pad)]


def target_string(d, tokens) -> str:
    """``Dictionary.string(.., escape_unk=True)`` with EOS stripped (fairseq/data/dictionary.py:72-108)."""
    unk, skip = d.unk(), {d.bos(), d.eos()}
    return " ".join(("<" + d[unk] + ">" if i == unk else d[i]) for i in (int(x) for x in tokens) if i not in skip)


def main(argv: Optional[List[str]] = None, device: Optional[torch.device] = None, on_model_built=None):
    args = make_parser().parse_args(argv)
    if args.max_tokens is None and args.batch_size is None:
        args.max_tokens = 12000  # generate_for_s2st.py:71-72
    if device is None:
        device = default_device("generate_text")
    which = args.aux_decoder or ("st" if args.scoring == "sacrebleu" else "asr")  # :107-110

    def configure(margs):
        if args.speaker_to_id is not None:
            margs.speaker_to_id = args.speaker_to_id
        if args.use_hubert is not None:
            margs.use_hubert = args.use_hubert

    task, model, margs, dataset = load_task_model_dataset(args, device, configure, on_model_built)
    args.aux_decoder = which
    generator = task.build_generator([model], args)
    tgt_dict = generator.tgt_dict  # (:194-199: the source dictionary for the ASR head, the target dictionary for ST)
    target_key = "src_text" if which == "asr" else "tgt_text"  # :215-219
    scorer = build_scorer("wer", tgt_dict, cfg=args) if args.scoring == "wer" else None
    out = sys.stdout
    if args.results_path is not None:
        Path(args.results_path).mkdir(exist_ok=True, parents=True)
        out = open(os.path.join(args.results_path, f"generate-{args.gen_subset}.txt"), "w", buffering=1, encoding="utf-8")
    num_sentences = num_tokens = n_batches = 0
    t_gen = 0.0
    try:
        for sample in batch_iterator(task, dataset, args):
            if sample is None or len(sample) == 0 or "net_input" not in sample:
                continue
            target = sample.get(target_key)
            t0 = time.perf_counter()
            hypos = generator.generate([model], sample)
            t_gen += time.perf_counter() - t0
            num_tokens += sum(len(h[0]["tokens"]) for h in hypos if h)
            for i, sample_id in enumerate(sample["id"].tolist()):
                target_str = None
                if target is not None:
                    target_str = target_string(tgt_dict, strip_pad(target[i, :].cpu(), tgt_dict.pad()))
                    if not args.quiet:
                        print(f"T-{sample_id}\t{target_str}", file=out)
                for j, hypo in enumerate(hypos[i][:args.nbest]):
                    hypo_str = tgt_dict.string(hypo["tokens"].int().cpu())
                    if not args.quiet:
                        score = (hypo["score"] / math.log(2)).item()  # base 2
                        print(f"H-{sample_id}\t{score}\t{hypo_str}", file=out)
                        print(f"D-{sample_id}\t{score}\t{hypo_str}", file=out)
                        pos = (hypo["positional_scores"] / math.log(2)).tolist()
                        print("P-{}\t{}".format(sample_id, " ".join("{:.4f}".format(x) for x in pos)), file=out)
                    if target_str is not None and j == 0 and scorer is not None:  # only the top hypothesis is scored
                        scorer.add_string(target_str, hypo_str)
            num_sentences += sample["id"].numel()
            n_batches += 1
            if args.max_batches and n_batches >= args.max_batches:
                break
        print("Translated {:,} sentences ({:,} tokens) in {:.1f}s ({:.2f} sentences/s, {:.2f} tokens/s)".format(
            num_sentences, num_tokens, t_gen, num_sentences / max(t_gen, 1e-9), num_tokens / max(t_gen, 1e-9)), file=out)
        result = scorer.result_string() if scorer is not None else \
            "BLEU is not computed here: score the T- / D- lines with an external sacrebleu"
        print(f"Generate {args.gen_subset} with beam={args.beam}: {result}", file=out)
    finally:
        if out is not sys.stdout:
            out.close()
    return scorer


def cli_main():
    main(sys.argv[1:])


if __name__ == "__main__":
    cli_main()
