"""``generate_waveform``: the counterpart of ``examples/s2s_trans/generate_waveform.py:127-183`` (BASELINE configs[4]) for
the MI355X path.

    python -m s2st_amd.generate_waveform DATA --config-yaml config.yaml --gen-subset test_fisher --path CKPT.pt \
        --results-path OUT --max-tokens 50000 --spec-bwd-max-iter 64 --dump-waveforms --dump-features --dump-target

loads a checkpoint in the reference's ``.pt`` layout (model flags from ``cfg["model"]``, tensors by the names of SURVEY
Appendix A), builds the task's autoregressive generator (``task.build_generator_tts``: key/value-cached decoding on the
engine, Griffin-Lim vocoder with all utterances of a batch per GEMM), walks the split in length-ordered max-tokens
batches (no shuffle) and writes, per utterance id, what the reference's ``dump_result`` writes (:67-124):
``feat/<id>.npy`` (+ ``feat_tgt/``), ``attn/<id>.npy``, ``eos/<id>.npy``, ``wav_<rate>hz_<vocoder>/<id>.wav`` (+ ``_tgt``),
``plot/<id>.png``.  Differences, stated: waveforms are written as 16-bit PCM with the standard library (``soundfile`` is
not in the image; the reference's default subtype for wav is PCM_16 too) and only at the feature sample rate (the
reference resamples through torchaudio's sox effects when ``--output-sample-rate`` differs; asking for another rate is an
error here, not a silent no-op).  Returns a summary dict (utterances, seconds, files) so tests and ``bench.py --config
infer_base`` can drive it in-process.
"""
from __future__ import annotations

import argparse
import functools
import os
import sys
from pathlib import Path
from typing import Dict, List, Optional

import torch

# (load_task_model, load_task_model_dataset, batch_iterator, dump_result and write_wav live in inference_common; tests and
# tools take them from here too)
from .inference_common import (batch_iterator, default_device, defer_vocoder, drive, dump_result, load_task_model,  # noqa: F401
                               load_task_model_dataset, write_wav)
from .runtime import streams as _streams


def make_parser() -> argparse.ArgumentParser:
    """fairseq's ``options.get_speech_generation_parser`` + generate_waveform.py:28-44, by their fairseq names."""
    p = argparse.ArgumentParser(prog="s2st_amd.generate_waveform", allow_abbrev=False)
    a = p.add_argument
    a("data")
    a("--user-dir", default=None, help="accepted for command-line compatibility (this package IS the plugin)")
    a("--config-yaml", default="config.yaml")
    a("--task", default="s2s_translation")
    a("--path", required=True, help="checkpoint (reference .pt layout)")
    a("--gen-subset", default="test")
    a("--results-path", required=True)
    a("--max-tokens", type=int, default=None)
    a("--batch-size", "--max-sentences", type=int, default=None, dest="batch_size")
    a("--required-batch-size-multiple", type=int, default=1)
    a("--skip-invalid-size-inputs-valid-test", action="store_true")
    a("--num-shards", type=int, default=1)
    a("--shard-id", type=int, default=0)
    a("--num-workers", type=int, default=0)
    a("--seed", type=int, default=1)
    a("--max-target-positions", type=int, default=None, help="AR steps at most (default: the checkpoint's value)")
    a("--eos-prob-threshold", type=float, default=0.5)
    a("--vocoder", default="griffin_lim", choices=["griffin_lim", "hifigan"])
    a("--spec-bwd-max-iter", type=int, default=8)
    a("--gl-phase-rng", default="numpy", choices=["numpy", "device"],
      help="initial Griffin-Lim phases: numpy's global generator (the reference's draws, vocoder.py:101-102) or the device's "
           "counter-based generator (same distribution, no host work)")
    a("--dump-features", action="store_true")
    a("--dump-waveforms", action="store_true")
    a("--dump-attentions", action="store_true")
    a("--dump-eos-probs", action="store_true")
    a("--dump-plots", action="store_true")
    a("--dump-target", action="store_true")
    a("--output-sample-rate", default=None, type=int)
    a("--audio-format", default="wav", choices=["wav"])
    a("--precise-gemm", action="store_true", help="bf16x3 GEMMs (fp32-accurate; parity runs)")
    a("--max-batches", type=int, default=0, help="stop after this many batches (0: the whole split)")
    return p


def main(argv: Optional[List[str]] = None, device: Optional[torch.device] = None, on_model_built=None,
         parser: Optional[argparse.ArgumentParser] = None, mtl: bool = False) -> Dict:
    """``mtl``: the flow of generate_waveform_mtl.py (see generate_waveform_mtl.py in this package): the task's own
    generator, source-transcript decoding + WER files, mel dumping only with --decode-target-mel."""
    args = (parser or make_parser()).parse_args(argv)
    decode_src = mtl and args.decode_source_text
    decode_mel = (not mtl) or args.decode_target_mel
    if not (args.dump_features or args.dump_waveforms or args.dump_attentions or args.dump_eos_probs or args.dump_plots
            or decode_src):
        raise SystemExit("nothing to do: pass at least one --dump-* flag (generate_waveform.py:128-129)")
    if args.max_tokens is None and args.batch_size is None:
        args.max_tokens = 8000  # :130-131
    if device is None:
        device = default_device("generate_waveform")

    def configure(margs):
        margs.eos_prob_threshold = args.eos_prob_threshold
        margs.spec_bwd_max_iter = args.spec_bwd_max_iter
        margs.gl_phase_rng = args.gl_phase_rng
        margs.vocoder = args.vocoder
        if args.max_target_positions is not None:
            margs.max_target_positions = args.max_target_positions

    task, model, margs, dataset = load_task_model_dataset(args, device, configure, on_model_built)
    sample_rate = task.sr
    if args.output_sample_rate not in (None, sample_rate):
        raise SystemExit(f"--output-sample-rate {args.output_sample_rate}: resampling (torchaudio sox effects in the "
                         f"reference, generate_waveform.py:148-156) is not available here; the features are {sample_rate} Hz")
    # (generate_waveform.py:158 / generate_waveform_mtl.py:164: the mtl task's build_generator IS its speech generator)
    generator = task.build_generator([model], margs) if mtl else task.build_generator_tts([model], margs)
    wer = src_f = hyp_f = None
    if decode_src:  # generate_waveform_mtl.py:183-185
        from .scoring import build_scorer
        wer = build_scorer(args.scoring, getattr(model, "src_dict", None))
        Path(args.results_path).mkdir(exist_ok=True, parents=True)
        src_f = open(os.path.join(args.results_path, "src_texts.txt"), "w")
        hyp_f = open(os.path.join(args.results_path, "hyps_src_texts.txt"), "w")
    itr = batch_iterator(task, dataset, args)
    Path(args.results_path).mkdir(exist_ok=True, parents=True)
    ids = getattr(dataset, "ids", None)
    written: List[str] = []
    n_utt = n_frames = n_batches = 0

    def finish(sample, hypos):
        """What the reference's loop does with a batch's hypotheses (generate_waveform.py:172-183 / _mtl.py:196-205)."""
        nonlocal n_utt, n_frames, n_batches
        if hasattr(hypos, "wait"):
            hypos.wait()  # (the vocoder ran on the generator's second stream, beside the next batch's decoding)
        if decode_src:  # :196-200
            for hypo in hypos:
                wer.add_string(hypo["src_texts"], hypo["hyps_src_texts"])
                src_f.write(hypo["src_texts"] + "\n")
                hyp_f.write(hypo["hyps_src_texts"] + "\n")
        for i, hypo in zip(sample["id"].tolist(), hypos):
            if decode_mel:
                dump_result(args, args.vocoder, sample_rate, ids[i] if ids is not None else i, hypo, written)
                n_frames += int(hypo["feature"].shape[0])
            n_utt += 1
        n_batches += 1

    # batch k's files are written after batch k + 1 has been enqueued, and several batches are DECODED at once where the
    # generator has that form (S2ST_DECODE_CHAINS=1: one by one): inference_common.drive
    defer = defer_vocoder(device)
    chains = _streams.default_decode_chains() if (defer and not mtl and hasattr(generator, "generate_many")) else 1
    one = None
    if mtl:  # generate_waveform_mtl.py:195
        one = functools.partial(generator.generate, decode_source_text=decode_src, decode_target_mel=decode_mel)
    t_gen = drive(generator, model, itr, finish, chains=chains, defer=defer, generate_one=one,
                  has_targ=args.dump_target and decode_mel, max_batches=args.max_batches,
                  sync_device=device if device.type == "cuda" else None)
    out = {"utterances": n_utt, "mel_frames": n_frames, "generate_seconds": t_gen, "batches": n_batches,
           "files": written, "sample_rate": sample_rate}
    if decode_src:  # :207-210
        src_f.close()
        hyp_f.close()
        out["wer"] = wer.score()
        written += [src_f.name, hyp_f.name]
        print(f"WER: {wer.score()}")
    return out


def cli_main():
    r = main(sys.argv[1:])
    print(f"generated {r['utterances']} utterances ({r['mel_frames']} mel frames) in {r['generate_seconds']:.2f} s "
          f"of generator time; {len(r['files'])} files under the results path")


if __name__ == "__main__":
    cli_main()
