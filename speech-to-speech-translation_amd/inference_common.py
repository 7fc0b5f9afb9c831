"""What the inference command-line tools share, so that none of them imports another: the device block, checkpoint / split
loading, the reference's ``dump_result``, the PCM16 wav writer and ``drive``, the pipelined loop over an AR speech generator
(``generate_waveform`` and ``translate`` run on it; ``bench.py`` keeps a copy of its own that must stay in step)."""
from __future__ import annotations

import argparse
import csv
import os
import sys
import time
import wave
from pathlib import Path
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import checkpoint_utils
from .registry import TASKS


def default_device(prog: str, needed_for: Optional[str] = None, without: Optional[str] = None) -> torch.device:
    """The process's HIP device (``LOCAL_RANK``), or the tool's refusal.  ``needed_for`` / ``without``: the flag value that
    needs a device and the one that runs without."""
    if not torch.cuda.is_available():
        if needed_for is not None:
            raise SystemExit(f"s2st_amd.{prog} {needed_for} needs a HIP device ({without} runs without one)")
        raise SystemExit(f"s2st_amd.{prog} needs a HIP device (the product path has no CPU fallback)")
    return torch.device("cuda", int(os.environ.get("LOCAL_RANK", 0)))


def write_pcm16(path: str, pcm: np.ndarray, sample_rate: int) -> None:
    """int16 samples as a 16-bit PCM mono wav."""
    with wave.open(path, "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(int(sample_rate))
        f.writeframes(np.ascontiguousarray(pcm, dtype="<i2").tobytes())


def write_wav(path: str, wave_f32: np.ndarray, sample_rate: int) -> None:
    """16-bit PCM mono (what ``soundfile.write`` makes of a float array for .wav by default)."""
    x = np.clip(np.asarray(wave_f32, dtype=np.float64).reshape(-1), -1.0, 1.0 - 1.0 / 32768)
    write_pcm16(path, np.round(x * 32768.0).astype("<i2"), sample_rate)


def read_manifest(path: str) -> Tuple[List[str], List[str], Optional[List[str]]]:
    """``translate --manifest``: (ids, audio files, speakers or None) of a TSV with the columns id, audio and optionally
    speaker; relative audio paths are taken from where they exist, else from the manifest's directory."""
    with open(path) as f:
        rows = list(csv.DictReader(f, delimiter="\t", quotechar=None, doublequote=False, lineterminator="\n",
                                   quoting=csv.QUOTE_NONE))
    if not rows or "id" not in rows[0] or "audio" not in rows[0]:
        raise SystemExit(f"translate: {path} must be a TSV with the columns id, audio and optionally speaker")
    root = Path(path).parent
    files = [r["audio"] if os.path.isabs(r["audio"]) or os.path.exists(r["audio"]) else (root / r["audio"]).as_posix()
             for r in rows]
    return [r["id"] for r in rows], files, ([r["speaker"] for r in rows] if "speaker" in rows[0] else None)


def _to_np(x):
    return None if x is None else x.detach().cpu().numpy()


def dump_result(args, vocoder_name: str, sample_rate: int, sample_id, hypo, written: List[str]) -> None:
    """generate_waveform.py:67-124."""
    out_root = Path(args.results_path)

    def save(sub, name, fn):
        d = out_root / sub
        d.mkdir(exist_ok=True, parents=True)
        fn(str(d / name))
        written.append(str(d / name))

    if args.dump_features:
        save("feat", f"{sample_id}.npy", lambda p: np.save(p, _to_np(hypo["feature"])))
        if args.dump_target:
            save("feat_tgt", f"{sample_id}.npy", lambda p: np.save(p, _to_np(hypo["targ_feature"])))
    if args.dump_attentions:
        save("attn", f"{sample_id}.npy", lambda p: np.save(p, _to_np(hypo["attn"])))
    if args.dump_eos_probs:
        save("eos", f"{sample_id}.npy", lambda p: np.save(p, _to_np(hypo["eos_prob"])))
    if args.dump_plots:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
        images = [_to_np(hypo["feature"]).T, _to_np(hypo["attn"])]
        names = ["output", "alignment"]
        if args.dump_target:
            images, names = [_to_np(hypo["targ_feature"]).T] + images, [f"target (idx={sample_id})"] + names
        fig, axes = plt.subplots(len(images) + 1, 1, figsize=(8, 2.2 * (len(images) + 1)))
        for ax, im, nm in zip(axes, images, names):
            ax.imshow(im, aspect="auto", origin="lower", interpolation="none")
            ax.set_title(nm, fontsize=8)
        axes[-1].plot(_to_np(hypo["eos_prob"]))
        axes[-1].set_title("eos prob", fontsize=8)
        fig.tight_layout()
        save("plot", f"{sample_id}.png", lambda p: fig.savefig(p))
        plt.close(fig)
    if args.dump_waveforms:
        ext = args.audio_format
        if hypo.get("waveform") is not None:
            save(f"{ext}_{sample_rate}hz_{vocoder_name}", f"{sample_id}.{ext}",
                 lambda p: write_wav(p, _to_np(hypo["waveform"]), sample_rate))
        if args.dump_target and hypo.get("targ_waveform") is not None:
            save(f"{ext}_{sample_rate}hz_{vocoder_name}_tgt", f"{sample_id}.{ext}",
                 lambda p: write_wav(p, _to_np(hypo["targ_waveform"]), sample_rate))


def load_task_model(args, device, configure=None, on_model_built=None):
    """What the generation scripts share (generate_waveform.py:134-147, fairseq_cli/generate_for_s2st.py:83-114): the
    checkpoint in the reference's ``.pt`` layout, the task set up from the command line with the checkpoint's model flags
    (``configure(margs)`` applies the script's own generation-time flags), the model with the checkpoint's tensors.
    Returns (task, model, margs)."""
    from . import criterions, models, tasks  # noqa: F401  (fill the registries)
    state = checkpoint_utils.load_checkpoint_to_cpu(args.path)
    margs = state["cfg"]["model"]
    margs = argparse.Namespace(**(vars(margs) if not isinstance(margs, dict) else margs))
    # generation-time flags override what the checkpoint carried (checkpoint_utils.load_model_ensemble_and_task +
    # generate_waveform.py:142-144: the task is set up from the command line, n_frames_per_step from the checkpoint)
    margs.data, margs.config_yaml = args.data, args.config_yaml
    margs.precise_gemm = bool(args.precise_gemm)
    margs.eval_inference = False
    margs.train_subset = None
    if configure is not None:
        configure(margs)
    for k in ("load_pretrained_encoder_from", "load_pretrained_decoder_from"):
        setattr(margs, k, None)  # the tensors come from the checkpoint itself
    task = TASKS[getattr(margs, "task", None) or args.task].setup_task(margs, device=device)
    if task.data_cfg is not None:
        margs.src_vocab_size, margs.tgt_vocab_size = len(task.source_dictionary), len(task.target_dictionary)
    model = task.build_model(margs)
    model.load_state_dict(state["model"], strict=True)
    if on_model_built is not None:
        on_model_built(model)
    return task, model, margs


def load_task_model_dataset(args, device, configure=None, on_model_built=None):
    """``load_task_model`` and the split ``--gen-subset``.  Returns (task, model, margs, dataset)."""
    task, model, margs = load_task_model(args, device, configure, on_model_built)
    dataset = task.load_dataset(args.gen_subset)
    return task, model, margs, dataset


def batch_iterator(task, dataset, args):
    """Length-ordered max-tokens batches of the split, no shuffle (generate_waveform.py:160-170)."""
    return task.get_batch_iterator(dataset, max_tokens=args.max_tokens, max_sentences=args.batch_size,
                                   max_positions=(sys.maxsize, sys.maxsize),
                                   required_batch_size_multiple=args.required_batch_size_multiple, seed=args.seed,
                                   num_shards=args.num_shards, shard_id=args.shard_id).next_epoch_itr(shuffle=False)


def defer_vocoder(device) -> bool:
    """One batch of overlap on the GPU: batch k's vocoder runs beside batch k + 1's decoding steps
    (S2ST_DEFER_VOCODER=0: strictly one after the other)."""
    return device.type == "cuda" and os.environ.get("S2ST_DEFER_VOCODER", "1") != "0"


def _groups(samples, chains: int, max_batches: int):
    """``chains`` samples at a time; None and empty ones are skipped; ``max_batches`` (0: all) cuts the stream, the short
    last group included."""
    buf, n = [], 0
    for sample in samples:
        if sample is None or len(sample) == 0:
            continue
        buf.append(sample)
        n += 1
        last = bool(max_batches and n >= max_batches)
        if len(buf) == chains or last:
            yield buf
            buf = []
        if last:
            return
    if buf:
        yield buf


def drive(generator, model, samples, finish, *, chains: int, defer: bool, generate_one=None, has_targ: bool = False,
          max_batches: int = 0, sync_device=None) -> float:
    """The pipelined loop over an AR speech generator.  ``samples``: collated batches; ``chains`` of them are decoded at once
    (``generate_many``: each on its own engine and stream -- the decoding steps of one batch leave most of the chip idle)
    where the generator has that form, a single one through ``generate_one`` (default ``generator.generate``; the mtl
    flow passes its own).  With ``defer``, ``finish(sample, hypos)`` of a group is called after the NEXT group has been
    enqueued, so that its deferred vocoder runs beside that group's decoding steps, and the last group is finished at the
    end; otherwise at once.  Returns the generator time in seconds: summed per group (synchronised on ``sync_device``) --
    or, with ``defer``, the loop's wall time: generator time cannot be told from what ``finish`` does when the two overlap."""
    many = getattr(generator, "generate_many", None)
    one = generate_one or generator.generate
    held, seconds, t_all = [], 0.0, time.perf_counter()
    for group in _groups(samples, chains if many is not None else 1, max_batches):
        t0 = time.perf_counter()
        if len(group) >= 2:
            hyps = list(many(model, group, has_targ=has_targ, defer_vocoder=defer))
        else:
            hyps = [one(model, group[0], has_targ=has_targ, defer_vocoder=defer)]
        if sync_device is not None and not defer:
            torch.cuda.synchronize(sync_device)
        seconds += time.perf_counter() - t0
        for h in held:
            finish(*h)
        held = list(zip(group, hyps))
        if not defer:
            for h in held:
                finish(*h)
            held = []
    for h in held:
        finish(*h)
    if defer:
        if sync_device is not None:
            torch.cuda.synchronize(sync_device)
        seconds = time.perf_counter() - t_all
    return seconds
