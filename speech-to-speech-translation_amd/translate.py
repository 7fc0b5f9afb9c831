"""``translate``: audio files in, translated audio files (and text) out.

    python -m s2st_amd.translate DATA --config-yaml config.yaml --path CKPT.pt --results-path OUT \
        (--inputs A.wav B.wav ... | --manifest FILE.tsv) [--src-sample-rate R] [--output-sample-rate R] [--speaker NAME] \
        [--text none|asr|st|both] [--beam 5] [--max-tokens N | --batch-size N] [--vocoder griffin_lim|hifigan] \
        [--segment long [--timeline joined|source] [--max-tempo 1.25]] [--tempo 1.0] [--time-scaler device|host] ...

The reference has no such script: its ``generate_waveform.py`` walks a split of a stage-3 data directory (features read
from a zip through a TSV manifest).  This one joins the pieces that exist into a device-resident path for NEW recordings:

    read_waveform -> (resample on the device) -> s2st_fbank_kaldi_batch_f32: filter bank, global CMVN and padding, written as
    the encoder's input -> AR decode + vocoder (``task.build_generator_tts``, driven as ``generate_waveform`` drives it) ->
    (resample on the device) -> s2st_wave_to_pcm16 -> one int16 copy to the host -> ``OUT/wav_<rate>hz_<vocoder>/<id>.wav``

and, with ``--text``, the aux ASR / ST head's beam search (``task.build_generator``, search on the device) into ``OUT/asr.txt``
/ ``OUT/st.txt`` (``id<TAB>text``, input order).  ``DATA`` + ``config.yaml`` supply what a trained model needs from its data
directory: the source CMVN statistics, the target statistics for de-normalisation, the vocoder section, the dictionaries,
the speakers.  Utterances are ordered and batched as the dataset does it (longest first, ties in input order, the native
``batch_by_size`` over frame counts), so the outputs are those of stage 3 + ``generate_waveform`` on the same audio, bit for
bit (tests/test_translate.py).  ``--manifest``: a TSV with the columns ``id``, ``audio`` and optionally ``speaker``.

Refused, each with a message: a model without the requested text head, ``--use-hubert`` models (they take raw audio; the
recipes infer with ``--use-hubert False``), text-input models, and a config whose source transforms for inference
(``src_transforms``: ``_eval``, else ``*``) are anything but nothing, ``global_cmvn`` or ``src_global_cmvn``.  An utterance
too short for one frame, or longer than the model's ``max_source_positions``, is skipped with a warning and listed in the
summary.

``--segment long`` (default ``off``: the above) translates the long ones too: an input of more frames than
``min(max_source_positions, --max-segment-s)`` is cut at its pauses (segmentation.py: an exact integer optimisation over the
filter bank's frames, on the device or with ``--segmenter host`` in numpy, bit-equal; at the source rate, after any
resampling), and its trimmed segments that hold speech enter the ordering and batching above as inputs ``id#k`` among the
others.  ``OUT/wav_.../<id>.wav`` then holds the segments' PCM in order -- in front of each from the second on a pause of zeros,
``min(gap_src_samples * out_rate // src_rate, --max-pause-ms)`` long, the gap being the source distance between the neighbours'
trimmed spans -- ``asr.txt`` / ``st.txt`` one line per recording (the segments' strings joined by a space), and
``OUT/segments.tsv`` one row per segment: ``id, k, src_start_s, src_end_s, trim_start_s, trim_end_s, dropped, out_start_s,
out_end_s`` and the text columns.  The dumps are per segment (``id#k``).  A recording without any speech is skipped and listed.
**Parity unpinned: the reference has no segmentation.**

``--tempo F`` (default 1.0: nothing is called) changes the tempo of what was generated without changing its pitch (time_scale.py:
waveform-similarity overlap-add on integers, csrc/time_scale.hip or with ``--time-scaler host`` in numpy, bit-equal): an output
of ``n`` samples -- an uncut input's, or each segment's of a cut one -- becomes ``ceil(n * 1000 / round(1000 F))`` long.
``--timeline source`` (needs ``--segment long``; default ``joined``: the above) lays a cut recording's segments out on the
SOURCE's time line instead: segment k starts where its trimmed span started in the source (in output samples), is compressed --
by ``--max-tempo`` at most -- when its translation is longer than the room up to the next segment, and pushes the next one
when even that is not enough (``time_scale.place``); zeros lie wherever no segment does, the wav is at least as long as the
recording, and ``segments.tsv`` gains a last column ``tempo`` (natural length / placed length).  An input that was not cut is
written as before.  **Parity unpinned: the reference has no time-scale modification.**
"""
from __future__ import annotations

import argparse
import functools
import os
import sys
import time
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import segmentation as sgm
from . import time_scale as tsm
from .data.audio_utils import read_audio, to_16bit_range
from .data.feature_extraction import DeviceFeatureExtractor
from .data.synthetic import batch_by_size
from .inference_common import (default_device, defer_vocoder, drive, dump_result, load_task_model, read_manifest,
                               write_pcm16)
from .models.wav2vec2_ctc import resample
from .runtime import binding as bd
from .runtime import streams as _streams
from .tasks.s2s_translation import _flag_is_true

SRC_CMVN = ("global_cmvn", "src_global_cmvn")
N_BINS = 80  # the filter bank stage 3 extracts (get_feature_manifest.py: extract_fbank_features' default)


def make_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="s2st_amd.translate", allow_abbrev=False)
    a = p.add_argument
    a("data", help="the data directory the model was trained on (config.yaml, dictionaries, CMVN statistics, speakers)")
    a("--config-yaml", default="config.yaml")
    a("--task", default="s2s_translation")
    a("--path", required=True, help="checkpoint (reference .pt layout)")
    a("--results-path", required=True)
    g = p.add_mutually_exclusive_group(required=True)
    g.add_argument("--inputs", nargs="+", default=None, help="audio files; ids are the file stems")
    g.add_argument("--manifest", default=None, help="TSV with the columns id, audio and optionally speaker")
    a("--src-sample-rate", type=int, default=None,
      help="the rate the model's source features were extracted at; inputs at other rates are resampled on the device "
           "(default: all inputs must share one rate and are taken at it)")
    a("--output-sample-rate", type=int, default=None, help="resample the generated audio (default: the feature rate)")
    a("--speaker", default=None, help="speaker name for inputs without one (speaker-conditioned models)")
    a("--text", default="none", choices=["none", "asr", "st", "both"], help="also decode the aux ASR and / or ST head")
    a("--beam", type=int, default=5)
    a("--max-len-b", type=int, default=200, help="text heads: tokens at most (generate_text's flag)")
    a("--max-tokens", type=int, default=None)
    a("--batch-size", "--max-sentences", type=int, default=None, dest="batch_size")
    a("--vocoder", default="griffin_lim", choices=["griffin_lim", "hifigan"])
    a("--spec-bwd-max-iter", type=int, default=8)
    a("--eos-prob-threshold", type=float, default=0.5)
    a("--max-target-positions", type=int, default=None, help="AR steps at most (default: the checkpoint's value)")
    a("--seed", type=int, default=None, help="seed numpy's generator (Griffin-Lim's initial phases) before translating")
    a("--dump-features", action="store_true")
    a("--dump-attentions", action="store_true")
    a("--dump-eos-probs", action="store_true")
    a("--precise-gemm", action="store_true", help="bf16x3 GEMMs (fp32-accurate; parity runs)")
    sgm.add_segment_flags(p)
    a("--segment", default="off", choices=["off", "long"],
      help="long: an input longer than the model takes is cut at its pauses (segmentation.py) and translated segment by "
           "segment; off: it is skipped")
    a("--max-pause-ms", type=float, default=sgm.MAX_PAUSE_MS,
      help="--segment long: the silence written between two segments' translations is the source pause, this long at most")
    tsm.add_time_scale_flags(p)
    a("--timeline", default="joined", choices=["joined", "source"],
      help="joined: a cut recording's translated segments follow each other with the pauses of --max-pause-ms; source (needs "
           "--segment long): each starts where it started in the source and is compressed to the room it has there.  It "
           "applies to recordings that were cut: an input that was not cut is written as before")
    a("--max-tempo", type=float, default=tsm.MAX_TEMPO,
      help="--timeline source: a segment is compressed by this factor at most (then it runs over and pushes the next one); a "
           "design choice, not a measurement; must be >= --tempo")
    return p


def check_tempo(tempo: float, max_tempo: float, timeline: str, segment: str) -> Tuple[int, int]:
    """(tempo, max tempo) in thousandths, or ValueError: the tempo within what ``time_scale`` takes, the limit not below it,
    ``timeline="source"`` only with ``segment="long"``."""
    if timeline not in ("joined", "source"):
        raise ValueError(f"timeline {timeline!r}: expected 'joined' or 'source'")
    if timeline == "source" and segment != "long":
        raise ValueError("--timeline source needs --segment long: it places the segments of a recording that was cut")
    t, mt = tsm.tempo_milli(tempo), tsm.tempo_milli(max_tempo)
    lo, hi = int(1000 * tsm.MIN_RATIO), int(1000 * tsm.MAX_RATIO)
    if not lo <= t <= hi:
        raise ValueError(f"--tempo {tempo} is outside [{tsm.MIN_RATIO}, {tsm.MAX_RATIO}]")
    if mt < t or mt > hi:
        raise ValueError(f"--max-tempo {max_tempo} must be at least --tempo {tempo} and at most {tsm.MAX_RATIO}")
    return t, mt


def pcm16(waves: Sequence[torch.Tensor], device) -> List[np.ndarray]:
    """``s2st_wave_to_pcm16`` over a ragged batch of device waveforms and ONE int16 copy to the host."""
    lens = [int(w.numel()) for w in waves]
    B, N = len(waves), max(lens, default=0)
    if B == 0 or N == 0:
        return [np.zeros(0, np.int16) for _ in waves]
    x = torch.zeros(B, N, dtype=torch.float32, device=device)
    for b, w in enumerate(waves):
        x[b, :lens[b]] = w.reshape(-1)
    ln = torch.tensor(lens, dtype=torch.int32).to(device)
    out = torch.empty(B, N, dtype=torch.int16, device=device)
    bd.call("s2st_wave_to_pcm16", x, ln, out, B, N)
    host = out.cpu().numpy()
    return [host[b, :lens[b]] for b in range(B)]


class SpeechTranslator:
    """The translator behind the CLI.  ``from_checkpoint`` builds it; ``translate`` takes waveforms and returns, per input,
    the generator's hypothesis dict (``feature``, ``attn``, ``eos_prob``, ``alignment``, ``waveform``: device tensors at the
    feature rate) with ``id``, ``src_feature`` (the encoder's input rows), ``pcm`` (int16 numpy at ``sample_rate``),
    ``sample_rate`` and the ``asr`` / ``st`` strings of the requested text heads -- or ``None`` for a skipped input (``skipped``: [(id, reason)] of the last call)."""

    def __init__(self, task, model, margs, device, src_sample_rate: Optional[int] = None,
                 output_sample_rate: Optional[int] = None, text: str = "none", beam: int = 5,
                 max_tokens: Optional[int] = None, batch_size: Optional[int] = None,
                 max_len_b: int = 200, text_max_positions: Optional[int] = None, cmvn=None, segment: str = "off",
                 max_pause_ms: float = sgm.MAX_PAUSE_MS, tempo: float = 1.0, timeline: str = "joined",
                 max_tempo: float = tsm.MAX_TEMPO, time_scaler: str = "device", **segment_options):
        """``cmvn``: (mean, std) fp32 [80] instead of the data config's source statistics (a model built without a data
        directory: tools/translate_rate.py)."""
        eng = model.engine
        if getattr(model, "hubert", None) is not None:
            raise SystemExit("translate: a --use-hubert model takes raw audio, not filter-bank features; the recipes infer "
                             "with --use-hubert False")
        if eng.cfg.text_input or _flag_is_true(getattr(margs, "input_text", "false")):
            raise SystemExit("translate: the checkpoint is a text-input model (--input-text true): it has no speech to translate")
        self.task, self.model, self.margs, self.device = task, model, margs, torch.device(device)
        self.src_sample_rate, self.output_sample_rate = src_sample_rate, output_sample_rate
        self.heads = {"none": (), "asr": ("asr",), "st": ("st",), "both": ("asr", "st")}[text]
        for which in self.heads:
            if not (eng.cfg.has_asr if which == "asr" else eng.cfg.has_st):
                raise SystemExit(f"translate: --text {text} needs the aux {which.upper()} decoder, which this model does not have")
        if max_tokens is None and batch_size is None:
            max_tokens = 8000  # generate_waveform's default
        self.max_tokens, self.batch_size = max_tokens, batch_size
        self.max_source_positions = int(getattr(margs, "max_source_positions", 3000))
        self.extractor = DeviceFeatureExtractor(self.device)
        self.mean, self.std = (torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(self.device)
                               for x in (cmvn if cmvn is not None else self._source_cmvn(task.data_cfg)))
        self.generator = task.build_generator_tts([model], margs)
        self.sample_rate = int(task.sr)
        self.vocoder_name = getattr(margs, "vocoder", None) or "griffin_lim"
        self.text_generators = {}
        for which in self.heads:
            # (the text decoders' position limit is the checkpoint's max_target_positions, as in generate_text: the
            # generation-time --max-target-positions bounds the AR mel steps only)
            ga = argparse.Namespace(aux_decoder=which, beam=beam, search="device", max_len_b=max_len_b)
            self.text_generators[which] = task.build_generator(
                [model], ga, extra_gen_cls_kwargs={"max_len": int(text_max_positions or 0)})
        self.skipped: List[Tuple[str, str]] = []
        self.seconds = {"front_end": 0.0, "generate": 0.0}
        # --segment long (segmentation.py): max_segment_s, min_segment_s, silence_db, cut_penalty_db, segment_pad_ms, segmenter
        if segment not in ("off", "long"):
            raise ValueError(f"segment {segment!r}: expected 'off' or 'long'")
        unknown = set(segment_options) - {"max_segment_s", "min_segment_s", "silence_db", "cut_penalty_db", "segment_pad_ms",
                                          "segmenter"}
        if unknown:
            raise TypeError(f"SpeechTranslator: unknown options {sorted(unknown)}")
        self.segment, self.max_pause_ms, self.segment_options = segment, float(max_pause_ms), dict(segment_options)
        self.segmentations: Dict[int, sgm.Segmentation] = {}  # of the last call: {input position: its segmentation}
        # --tempo / --timeline source (time_scale.py)
        if time_scaler not in ("device", "host"):
            raise ValueError(f"time_scaler {time_scaler!r}: expected 'device' or 'host'")
        self.tempo_milli, self.max_tempo_milli = check_tempo(tempo, max_tempo, timeline, segment)
        self.timeline, self.time_scaler = timeline, time_scaler
        self._natural: set = set()  # of the running call: the expanded positions whose PCM keeps its length until it is placed

    # ---- construction ---------------------------------------------------------------------------------------------------
    @staticmethod
    def _source_cmvn(data_cfg) -> Tuple[np.ndarray, np.ndarray]:
        """(mean, std) fp32 [80] of the config's source transform at inference; no transform: (0, 1), which leaves the
        filter bank's bits as they are."""
        if data_cfg is None:
            raise SystemExit("translate: DATA must be the model's data directory (config.yaml, dictionaries, CMVN statistics)")
        names = data_cfg.get_feature_transforms_for_src("", False).get("src_transforms") or []
        if len(names) == 0:
            return np.zeros(N_BINS, np.float32), np.ones(N_BINS, np.float32)
        if len(names) != 1 or names[0] not in SRC_CMVN:
            raise SystemExit(f"translate: the config's source transforms at inference are {list(names)}; only none, "
                             f"global_cmvn or src_global_cmvn run on this path (they are fused into the feature kernel)")
        section = data_cfg._auto_convert_to_abs_path(data_cfg.config.get(names[0]) or {})
        path = section.get("stats_npz_path")
        if path is None or not os.path.isfile(path):
            raise SystemExit(f"translate: {names[0]}: stats_npz_path {path!r} not found")
        stats = np.load(path)
        out = []
        for k in ("mean", "std"):
            v = np.asarray(stats[k]).reshape(-1)
            v32 = v.astype(np.float32)
            if v.shape[0] != N_BINS or not np.array_equal(v32.astype(v.dtype), v):
                # (float64 statistics would make the host transform a float64 operation: not what the kernel computes)
                raise SystemExit(f"translate: {path}: '{k}' must hold {N_BINS} float32 values")
            out.append(np.ascontiguousarray(v32))
        return out[0], out[1]

    @classmethod
    def from_checkpoint(cls, data: str, path: str, config_yaml: str = "config.yaml", device=None, task: str = "s2s_translation",
                        precise_gemm: bool = False, vocoder: str = "griffin_lim", spec_bwd_max_iter: int = 8,
                        eos_prob_threshold: float = 0.5,
                        max_target_positions: Optional[int] = None, on_model_built=None, **options) -> "SpeechTranslator":
        """The checkpoint's model on ``device`` with the generation-time flags of ``generate_waveform``; ``options``: the
        constructor's (src_sample_rate, output_sample_rate, text, beam, max_len_b, max_tokens, batch_size)."""
        if device is None:
            device = default_device("translate")
        largs = argparse.Namespace(data=data, config_yaml=config_yaml, path=path, task=task, precise_gemm=precise_gemm)
        trained = {}
        configure = functools.partial(cls._configure, trained, vocoder, spec_bwd_max_iter, eos_prob_threshold,
                                      max_target_positions)
        tk, model, margs = load_task_model(largs, device, configure, on_model_built)
        return cls(tk, model, margs, device, **dict(trained, **options))

    @staticmethod
    def _configure(trained, vocoder, spec_bwd_max_iter, eos_prob_threshold, max_target_positions, margs) -> None:
        """The generation-time flags on the checkpoint's model flags; ``trained`` takes what the checkpoint carried."""
        # (refused before the model is built: a HuBERT front end would want its own weights)
        if _flag_is_true(getattr(margs, "use_hubert", "false")):
            raise SystemExit("translate: a --use-hubert model takes raw audio, not filter-bank features; the recipes "
                             "infer with --use-hubert False")
        if _flag_is_true(getattr(margs, "input_text", "false")):
            raise SystemExit("translate: the checkpoint is a text-input model (--input-text true): it has no speech to "
                             "translate")
        trained["text_max_positions"] = getattr(margs, "max_target_positions", None)
        margs.eos_prob_threshold = eos_prob_threshold
        margs.spec_bwd_max_iter = spec_bwd_max_iter
        margs.gl_phase_rng = "numpy"  # (the reference's draws, as generate_waveform's default)
        margs.vocoder = vocoder
        if max_target_positions is not None:
            margs.max_target_positions = max_target_positions

    # ---- the pipeline ---------------------------------------------------------------------------------------------------
    def _frames(self, n: int, rate: int) -> int:
        shift, size = self.extractor._fbank_tables(rate, N_BINS)[:2]
        return 0 if n < size else 1 + (n - size) // shift

    def _source_rate(self, rates: Sequence[int]) -> int:
        if self.src_sample_rate is not None:
            return int(self.src_sample_rate)
        if len(set(rates)) > 1:
            raise SystemExit(f"translate: the inputs come at several sample rates {sorted(set(rates))}: pass --src-sample-rate "
                             f"(the rate the model's features were extracted at) to have them resampled")
        return int(rates[0])

    def _front_end(self, waves, rates, rate: int):
        """One batch: (resample ->) 2**15 scale -> fbank_batch, in the stage's order.  Returns (src, frames) on the device."""
        scaled = [None] * len(waves)
        for r in sorted({r for r in rates if r != rate}):
            idx = [i for i, x in enumerate(rates) if x == r]
            for i, y in zip(idx, resample([np.asarray(waves[i], dtype=np.float32) if waves[i].dtype != np.int16
                                           else waves[i].astype(np.float32) / np.float32(32768) for i in idx], r, rate,
                                          device=self.device)):
                scaled[i] = y * float(2 ** 15)
        if any(s is not None for s in scaled):
            # (a batch with resampled members lives on the device as fp32; the others join it there)
            for i, w in enumerate(waves):
                if scaled[i] is None:
                    scaled[i] = torch.from_numpy(np.asarray(to_16bit_range(w), dtype=np.float32)).to(self.device)
        else:
            scaled = [to_16bit_range(w) for w in waves]
        return self.extractor.fbank_batch(scaled, rate, self.mean, self.std, N_BINS)

    def _segment_long(self, waves, rates, rate, n_frames, ids, speakers):
        """--segment long: every input of more frames than a segment may have is cut at its pauses (segmentation.py, at the
        source rate, all such inputs in one call) and replaced, in place, by its trimmed segments that hold speech, as inputs
        ``id#k``.  Returns None when no input is that long, else the expanded (waves, rates, ids, speakers), ``origin``
        [(input, k or None)] per expanded position and ``groups`` {input: {"seg": Segmentation, "at": {k: position}}}."""
        opt = sgm.segment_frames(self.segment_options, self.max_source_positions)
        long_ = [i for i in range(len(waves)) if n_frames[i] > opt["max_len"]]
        if not long_:
            return None
        src = {}
        for i in long_:
            if rates[i] == rate:
                src[i] = waves[i]
            else:  # resampled once, on the device; its segments then are inputs at the source rate
                w = waves[i].astype(np.float32) / np.float32(32768) if waves[i].dtype == np.int16 else waves[i]
                src[i] = resample([w], rates[i], rate, device=self.device)[0].cpu().numpy()
        shift, size = self.extractor._fbank_tables(rate, N_BINS)[:2]
        t0 = time.perf_counter()
        segs = sgm.segment([src[i] for i in long_], rate, opt["min_len"], opt["max_len"], sgm.SMOOTH_FRAMES, opt["silence_db"],
                           opt["cut_penalty_db"], opt["pad"], device=self.device, segmenter=opt["segmenter"], win=size, hop=shift)
        self.seconds["segment"] = time.perf_counter() - t0
        xw, xr, xi, xs, origin, groups = [], [], [], [], [], {}
        for i in range(len(waves)):
            if i not in src:
                xw.append(waves[i]); xr.append(rates[i]); xi.append(ids[i]); origin.append((i, None))
                xs.append(None if speakers is None else speakers[i])
                continue
            seg = segs[long_.index(i)]
            groups[i] = {"seg": seg, "at": {}}
            self.segmentations[i] = seg
            for k in range(len(seg)):
                if seg.dropped[k]:
                    continue
                a, b = (int(v) for v in seg.trim_samples[k])
                groups[i]["at"][k] = len(xw)
                xw.append(src[i][a:b]); xr.append(rate); xi.append(f"{ids[i]}#{k}"); origin.append((i, k))
                xs.append(None if speakers is None else speakers[i])
        return xw, xr, xi, (None if speakers is None else xs), origin, groups

    def _join(self, name, group, got, rate):
        """The result of a segmented input: its segments' hypotheses in order, their PCM joined -- a pause of zeros in front
        of each segment from the second on, as long as the source distance between the neighbours' trimmed spans (in output
        samples), ``max_pause_ms`` at most -- and their strings joined by a space."""
        seg, ks = group["seg"], sorted(got)
        hyps = [got[k] for k in ks]
        out_rate = int(hyps[0]["sample_rate"])
        max_pause = int(self.max_pause_ms * out_rate / 1000)
        pieces, spans, pos, prev_end = [], {}, 0, None
        for k, h in zip(ks, hyps):
            a, b = (int(v) for v in seg.trim_samples[k])
            if prev_end is not None:
                pause = min((a - prev_end) * out_rate // rate, max_pause)
                pieces.append(np.zeros(pause, np.int16))
                pos += pause
            n = 0 if h["pcm"] is None else int(len(h["pcm"]))
            pieces.append(h["pcm"])
            spans[k] = (pos, pos + n)
            pos, prev_end = pos + n, b
        pcm = None if any(p is None for p in pieces) else np.concatenate(pieces)
        out = {"id": name, "segments": hyps, "segment_ids": ks, "segmentation": seg, "pcm": pcm, "sample_rate": out_rate,
               "src_rate": int(rate), "out_spans": spans}
        for which in self.heads:
            out[which] = " ".join(h[which] for h in hyps)
        return out

    def _scale(self, pcm: Sequence[np.ndarray], out_lens: Sequence[int], rate: int) -> List[np.ndarray]:
        """``pcm[b]`` at ``out_lens[b]`` samples: those whose length changes in ONE ``time_scale`` call, the others as they are."""
        idx = [b for b, (p, m) in enumerate(zip(pcm, out_lens)) if int(m) != len(p)]
        out = list(pcm)
        if idx:
            t0 = time.perf_counter()
            res = tsm.time_scale([pcm[b] for b in idx], [int(out_lens[b]) for b in idx], rate=rate, device=self.device,
                                 scaler=self.time_scaler)
            self.seconds["time_scale"] = self.seconds.get("time_scale", 0.0) + time.perf_counter() - t0
            for b, (y, _) in zip(idx, res):
                out[b] = y
        return out

    def _join_source(self, name, group, got, rate):
        """The result of a segmented input under ``timeline="source"``: every segment starts where its trimmed span started in
        the source, as long as ``time_scale.place`` allows it to be (all segments whose length changes go to the device in
        one call); zeros wherever no segment lies; at least as long as the source.  ``tempo``: {k: natural / placed length}."""
        seg, ks = group["seg"], sorted(got)
        hyps = [got[k] for k in ks]
        out_rate = int(hyps[0]["sample_rate"])
        out = {"id": name, "segments": hyps, "segment_ids": ks, "segmentation": seg, "pcm": None, "sample_rate": out_rate,
               "src_rate": int(rate), "out_spans": {}, "tempo": {}}
        if all(h["pcm"] is not None for h in hyps):
            total = -(-int(seg.n_samples) * out_rate // int(rate))
            starts = [int(seg.trim_samples[k][0]) * out_rate // int(rate) for k in ks]
            natural = [int(len(h["pcm"])) for h in hyps]
            at, lens = tsm.place(starts, natural, total, self.tempo_milli, self.max_tempo_milli)
            pcm = np.zeros(max([total] + [a + m for a, m in zip(at, lens)]), np.int16)
            for k, a, m, n, y in zip(ks, at, lens, natural, self._scale([h["pcm"] for h in hyps], lens, out_rate)):
                pcm[a:a + m] = y
                out["out_spans"][k] = (a, a + m)
                out["tempo"][k] = n / m if m else 1.0
            out["pcm"] = pcm
        for which in self.heads:
            out[which] = " ".join(h[which] for h in hyps)
        return out

    @staticmethod
    def _normalise(audio) -> Tuple[List[np.ndarray], List[int]]:
        """[(samples, rate)] -> mono int16 / float32 waveforms and their rates."""
        waves = []
        for w, _ in audio:
            w = np.asarray(w)
            if w.ndim != 1:
                raise ValueError("translate takes mono waveforms (1-D arrays)")
            waves.append(w if w.dtype == np.int16 else np.ascontiguousarray(w, dtype=np.float32))
        return waves, [int(r) for _, r in audio]

    def _frame_counts(self, waves, rates, rate: int) -> np.ndarray:
        """Filter-bank frames per input at the source rate (an input at another rate: of resample()'s output length)."""
        lens = [int(w.shape[0]) if r == rate else -(-int(w.shape[0]) * rate // r) for w, r in zip(waves, rates)]
        return np.array([self._frames(n, rate) for n in lens], dtype=np.int64)

    def _speaker_ids(self, speakers) -> Optional[List[int]]:
        if speakers is None or all(s is None for s in speakers):
            return None
        table = self.task.speaker_to_id
        if table is None:  # (as the dataset: without --speaker-to-id the speaker column is not read)
            print("translate: the model was trained without --speaker-to-id: speakers are ignored", file=sys.stderr)
            return None
        for s in speakers:
            if s not in table:
                raise SystemExit(f"translate: unknown speaker {s!r} (the model knows {sorted(table)})")
        return [int(table[s]) for s in speakers]

    def _batches(self, ids, n_frames, groups, audio_ids) -> List:
        """The dataset's order and batches: longest first, ties in input order (S2STDataset.ordered_indices), size filter,
        the native max-tokens batcher over frame counts (S2ST_TranslationTask.get_batch_iterator).  What is left out goes
        to ``skipped``; a segmented input (``groups``) learns how many of its segments to expect."""
        keep = []
        for i in np.lexsort([np.arange(len(ids)), -n_frames]):
            if n_frames[i] == 0:
                self.skipped.append((ids[i], "too short for one frame"))
            elif n_frames[i] > self.max_source_positions:
                self.skipped.append((ids[i], f"{int(n_frames[i])} frames exceed max_source_positions {self.max_source_positions}"))
            else:
                keep.append(int(i))
        for i, g in groups.items():  # a segmented input is translated if one of its segments is
            g["expected"] = len(set(g["at"].values()) & set(keep))
            if g["expected"] == 0:
                self.skipped.append((audio_ids[i], "no speech found: every segment is silence or too short for one frame"))
        for i, why in self.skipped:
            print(f"translate: skipping {i}: {why}", file=sys.stderr)
        if not keep:
            return []
        keep = np.asarray(keep, dtype=np.int64)
        return batch_by_size(keep, n_frames[keep], self.max_tokens or 0, self.batch_size or -1, 1)

    def _samples(self, batches, waves, rates, rate: int, n_frames, spk_ids):
        """The batches as collated samples: the front end, then the text heads' strings in ``sample["text"]``."""
        for b in batches:
            # (the collater's own sort of a batch, s2st_dataset.py:328-331: rows by descending length)
            _, o = torch.tensor([int(n_frames[i]) for i in b], dtype=torch.long).sort(descending=True)
            rows = [int(b[j]) for j in o.tolist()]
            t0 = time.perf_counter()
            src, frames = self._front_end([waves[i] for i in rows], [rates[i] for i in rows], rate)
            self.seconds["front_end"] += time.perf_counter() - t0
            speaker = None if spk_ids is None else torch.tensor([spk_ids[i] for i in rows], dtype=torch.long).view(-1, 1)
            # (the lengths also as the host tensor the collater makes: the engine sizes its launches from them)
            host_lens = torch.tensor([int(n_frames[i]) for i in rows], dtype=torch.long)
            sample = {"id": torch.tensor(rows, dtype=torch.long), "nsentences": len(rows), "speaker": speaker, "frames": frames,
                      "net_input": {"src_speech": src, "src_speech_lens": host_lens, "speaker": speaker}, "text": {}}
            for which, gen in self.text_generators.items():
                hyps = gen.generate([self.model], sample)
                sample["text"][which] = [gen.tgt_dict.string(h[0]["tokens"].int().cpu()) for h in hyps]
            yield sample

    def _finish(self, sink, ids, sample, hypos) -> None:
        """A decoded batch: (resample ->) s2st_wave_to_pcm16, then ``sink(position, hypo)`` per utterance."""
        if hasattr(hypos, "wait"):
            hypos.wait()  # (the vocoder ran on the generator's second stream, beside the next batch's decoding)
        outs = [h["waveform"] for h in hypos]
        out_rate = self.sample_rate
        if all(w is not None for w in outs):
            if self.output_sample_rate not in (None, self.sample_rate):
                out_rate = int(self.output_sample_rate)
                outs = resample(outs, self.sample_rate, out_rate, device=self.device)
            pcm = pcm16(outs, self.device)
            if self.tempo_milli != 1000:  # (a segment that --timeline source places keeps its length until then)
                rows = sample["id"].tolist()
                pcm = self._scale(pcm, [len(p) if i in self._natural else tsm.scaled_len(len(p), self.tempo_milli)
                                        for i, p in zip(rows, pcm)], out_rate)
        else:
            pcm = [None] * len(outs)
        src, n_frames = sample["net_input"]["src_speech"], sample["net_input"]["src_speech_lens"].tolist()
        for row, (i, hypo) in enumerate(zip(sample["id"].tolist(), hypos)):
            hypo = dict(hypo, id=ids[i], pcm=pcm[row], sample_rate=out_rate, src_feature=src[row, :n_frames[row]])
            for which in self.heads:
                hypo[which] = sample["text"][which][row]
            sink(i, hypo)

    def _run(self, audio, ids, speakers, sink, segment: Optional[str] = None, timeline: Optional[str] = None) -> None:
        """Translate ``audio`` [(samples, rate)]; ``sink(position, hypo)`` is called once per translated input."""
        dev = self.device
        self.skipped = []
        self.segmentations = {}
        self._natural = set()
        self.seconds = {"front_end": 0.0, "generate": 0.0}
        if len(audio) == 0:
            return
        rate = self._source_rate([int(r) for _, r in audio])
        waves, rates = self._normalise(audio)
        n_frames = self._frame_counts(waves, rates, rate)
        mode = self.segment if segment is None else segment
        if mode not in ("off", "long"):
            raise ValueError(f"segment {mode!r}: expected 'off' or 'long'")
        line = self.timeline if timeline is None else timeline
        check_tempo(self.tempo_milli / 1000, self.max_tempo_milli / 1000, line, mode)
        groups, audio_ids = {}, ids
        expanded = self._segment_long(waves, rates, rate, n_frames, ids, speakers) if mode == "long" else None
        if expanded is not None:
            waves, rates, ids, speakers, origin, groups = expanded
            n_frames = self._frame_counts(waves, rates, rate)  # (a segment is at the source rate; the others are as they were)
            sink = _Regroup(self, sink, origin, groups, audio_ids, rate, line)
            if line == "source":
                self._natural = {pos for pos, (_, k) in enumerate(origin) if k is not None}
        spk_ids = self._speaker_ids(speakers)
        batches = self._batches(ids, n_frames, groups, audio_ids)
        # driven as generate_waveform drives its generator (inference_common.drive): batch k's files are written after batch
        # k + 1 has been enqueued (deferred vocoder), and several batches are decoded at once where the generator has that form
        defer = defer_vocoder(dev)
        chains = _streams.default_decode_chains() if (defer and hasattr(self.generator, "generate_many")) else 1
        self.seconds["generate"] = drive(self.generator, self.model, self._samples(batches, waves, rates, rate, n_frames, spk_ids),
                                         functools.partial(self._finish, sink, ids), chains=chains, defer=defer,
                                         sync_device=dev if dev.type == "cuda" else None)

    def translate(self, audio: Sequence[Tuple[np.ndarray, int]], ids: Optional[Sequence[str]] = None,
                  speakers: Optional[Sequence[Optional[str]]] = None, segment: Optional[str] = None,
                  timeline: Optional[str] = None) -> List[Optional[Dict]]:
        """``audio``: [(samples, rate)] -- mono float waveforms in [-1, 1), or int16 PCM.  Returns one entry per input, in
        input order (``None`` for a skipped one).  ``segment`` ("off" / "long"; default: the constructor's): with "long" an
        input longer than the model takes is cut at its pauses and its entry is ``{"id", "segments": the hypotheses of its
        segments ``id#k`` in order, "segment_ids": their k, "segmentation", "pcm": their PCM joined with the pauses between
        them, "sample_rate", "src_rate", "out_spans": {k: (start, end) in pcm}}`` plus the joined ``asr`` / ``st`` strings.
        ``timeline`` ("joined" / "source"; default: the constructor's): with "source" (needs "long") that entry's ``pcm`` has
        the segments where they were in the source (``_join_source``), ``out_spans`` says where, and ``tempo`` {k: natural /
        placed length} how much each was compressed; the segments' own ``pcm`` stay as generated."""
        ids = [str(i) for i in ids] if ids is not None else [str(i) for i in range(len(audio))]
        if len(ids) != len(audio) or (speakers is not None and len(speakers) != len(audio)):
            raise ValueError("translate: ids / speakers must have one entry per input")
        if len(set(ids)) != len(ids):
            raise SystemExit(f"translate: duplicate ids {sorted({i for i in ids if ids.count(i) > 1})}")
        out: List[Optional[Dict]] = [None] * len(audio)
        self._run(audio, ids, speakers, out.__setitem__, segment, timeline)
        return out


class _Regroup:
    """The sink of a call with segmented inputs: a segment waits for its siblings; the input's joined result goes out with the
    last one.  ``origin``: [(input, k or None)] per expanded position; ``groups``: ``SpeechTranslator._segment_long``'s."""

    def __init__(self, translator, sink, origin, groups, ids, rate, timeline="joined"):
        self.translator, self.sink, self.origin, self.groups, self.ids, self.rate = translator, sink, origin, groups, ids, rate
        self.join = translator._join_source if timeline == "source" else translator._join
        self.got: Dict[int, Dict[int, Dict]] = {}

    def __call__(self, pos, hypo):
        i, k = self.origin[pos]
        if k is None:
            return self.sink(i, hypo)
        self.got.setdefault(i, {})[k] = hypo
        if len(self.got[i]) == self.groups[i]["expected"]:
            self.sink(i, self.join(self.ids[i], self.groups[i], self.got.pop(i), self.rate))


def main(argv: Optional[List[str]] = None, device: Optional[torch.device] = None, on_model_built=None) -> Dict:
    args = make_parser().parse_args(argv)
    if args.manifest is not None:
        ids, files, speakers = read_manifest(args.manifest)
    else:
        files, speakers = list(args.inputs), None
        ids = [Path(f).stem for f in files]
    if len(set(ids)) != len(ids):
        raise SystemExit(f"translate: duplicate ids {sorted({i for i in ids if ids.count(i) > 1})}: two inputs would be written "
                         f"to the same file")
    try:
        check_tempo(args.tempo, args.max_tempo, args.timeline, args.segment)  # (refused before the model is loaded)
    except ValueError as e:
        raise SystemExit(f"translate: {e}")
    if speakers is None and args.speaker is not None:
        speakers = [args.speaker] * len(files)
    elif speakers is not None:
        speakers = [s or args.speaker for s in speakers]
    tr = SpeechTranslator.from_checkpoint(
        args.data, args.path, config_yaml=args.config_yaml, device=device, task=args.task, precise_gemm=args.precise_gemm,
        vocoder=args.vocoder, spec_bwd_max_iter=args.spec_bwd_max_iter,
        eos_prob_threshold=args.eos_prob_threshold, max_target_positions=args.max_target_positions,
        on_model_built=on_model_built, src_sample_rate=args.src_sample_rate, output_sample_rate=args.output_sample_rate,
        text=args.text, beam=args.beam, max_len_b=args.max_len_b, max_tokens=args.max_tokens, batch_size=args.batch_size,
        segment=args.segment, max_pause_ms=args.max_pause_ms, max_segment_s=args.max_segment_s, min_segment_s=args.min_segment_s,
        silence_db=args.silence_db, cut_penalty_db=args.cut_penalty_db, segment_pad_ms=args.segment_pad_ms,
        segmenter=args.segmenter, tempo=args.tempo, timeline=args.timeline, max_tempo=args.max_tempo,
        time_scaler=args.time_scaler)
    if args.segment == "long":
        sgm.segment_frames(tr.segment_options, tr.max_source_positions)  # (a contradiction among the flags is refused up front)
    audio = [read_audio(f) for f in files]
    if args.seed is not None:
        np.random.seed(args.seed)
    out_root = Path(args.results_path)
    out_root.mkdir(exist_ok=True, parents=True)
    out_rate = tr.sample_rate if args.output_sample_rate is None else int(args.output_sample_rate)
    wav_dir = out_root / f"wav_{out_rate}hz_{args.vocoder}"
    wav_dir.mkdir(exist_ok=True, parents=True)
    dargs = argparse.Namespace(results_path=args.results_path, dump_features=args.dump_features, dump_target=False,
                               dump_attentions=args.dump_attentions, dump_eos_probs=args.dump_eos_probs, dump_plots=False,
                               dump_waveforms=False, audio_format="wav")
    written: List[str] = []
    texts: Dict[str, Dict[int, str]] = {which: {} for which in tr.heads}
    n_utt = n_frames = 0

    seg_rows: Dict[int, List[List[str]]] = {}
    tsv_text = list(tr.heads) + (["tempo"] if args.timeline == "source" else [])  # (the columns behind out_end_s)

    def sink(i, hypo):
        nonlocal n_utt, n_frames
        if "segments" in hypo:  # --segment long: the dumps per segment (id#k), wav and text per recording
            for k, h in zip(hypo["segment_ids"], hypo["segments"]):
                dump_result(dargs, args.vocoder, out_rate, h["id"], h, written)
                n_frames += int(h["feature"].shape[0])
            text = {k: [h[which] for which in tr.heads] for k, h in zip(hypo["segment_ids"], hypo["segments"])}
            if args.timeline == "source":
                for k in text:
                    text[k].append(f"{hypo['tempo'][k]:.6f}" if k in hypo["tempo"] else "")
            seg_rows[i] = sgm.segment_rows(ids[i], hypo["segmentation"], hypo["out_spans"], out_rate, text, len(tsv_text))
        else:
            dump_result(dargs, args.vocoder, out_rate, ids[i], hypo, written)
            n_frames += int(hypo["feature"].shape[0])
        if hypo["pcm"] is not None:
            path = str(wav_dir / f"{ids[i]}.wav")
            write_pcm16(path, hypo["pcm"], out_rate)
            written.append(path)
        for which in tr.heads:
            texts[which][i] = hypo[which]
        n_utt += 1

    t0 = time.perf_counter()
    tr._run(audio, ids, speakers, sink)
    seconds = time.perf_counter() - t0
    for which in tr.heads:
        path = str(out_root / f"{which}.txt")
        with open(path, "w", encoding="utf-8") as f:
            for i in sorted(texts[which]):
                f.write(f"{ids[i]}\t{texts[which][i]}\n")
        written.append(path)
    if args.segment == "long":
        for i, seg in tr.segmentations.items():  # (a recording none of whose segments was translated keeps its rows)
            if i not in seg_rows:
                seg_rows[i] = sgm.segment_rows(ids[i], seg, {}, out_rate, {}, len(tsv_text))
        path = str(out_root / "segments.tsv")
        sgm.write_segments_tsv(path, [r for i in sorted(seg_rows) for r in seg_rows[i]], out_columns=True, text=tsv_text)
        written.append(path)
    return {"utterances": n_utt, "mel_frames": n_frames, "seconds": seconds, "front_end_seconds": tr.seconds["front_end"],
            "files": written, "sample_rate": out_rate, "skipped": [i for i, _ in tr.skipped],
            "skipped_reasons": dict(tr.skipped)}


def cli_main():
    r = main(sys.argv[1:])
    print(f"translated {r['utterances']} utterances ({r['mel_frames']} mel frames) in {r['seconds']:.2f} s; "
          f"{len(r['files'])} files under the results path; skipped: {r['skipped'] or 'none'}")


if __name__ == "__main__":
    cli_main()
