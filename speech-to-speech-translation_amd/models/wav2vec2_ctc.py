"""wav2vec 2.0 CTC recogniser for the ASR-BLEU score, and the resampler in front of it, on the HIP path.

What ``examples/s2s_trans/evalute_s2s_bleu.py`` does through third-party libraries, per batch of generated waveforms::

    librosa.load(path, sr=16000)                          -> resample()            (s2st_resample_sinc_f32)
    Wav2Vec2Processor(batch, padding="longest")           -> s2st_w2v_ctc_forward  (normalisation kernel)
    Wav2Vec2ForCTC(input_values, attention_mask).logits   ->   "                   (conv stack, 24 pre-LN layers, lm_head)
    torch.argmax(logits, -1); processor.batch_decode(ids) ->   "  + decode()       (greedy CTC kernel; ids -> characters)

``Wav2Vec2CTC`` is the third frozen engine-backed network beside the HuBERT front end and the HiFi-GAN vocoder: the
"layer-norm" variant (``feat_extract_norm="layer"``, ``do_stable_layer_norm=True``, convolutions with bias) with a CTC
head, geometry ``facebook/wav2vec2-large-960h-lv60-self`` by default.  ``state_dict`` keys are those of
``transformers.Wav2Vec2ForCTC``; loading converts layouts and folds the positional convolution's weight norm once (both
spellings: ``weight_g`` / ``weight_v`` and ``parametrizations.weight.original0`` / ``original1``).  ``from_pretrained(dir)``
reads a local directory in the Hugging Face layout -- ``config.json``, ``vocab.json``, ``pytorch_model.bin`` or
``model.safetensors`` (parsed here: 8-byte little-endian header length, JSON index, raw tensors) -- with neither
``transformers`` nor ``safetensors``; nothing is ever downloaded.  All arithmetic runs in libs2st_hip.so; torch holds the
arenas.

**One decided deviation from the reference script.**  ``processor.batch_decode`` also decodes the frames past a short
utterance's end in a padded batch; here only an utterance's valid frames (``floor((n - k) / s) + 1`` layer by layer over its
own samples) are decoded, so a transcript does not depend on what else is in the batch.

The resampler restates resampy's published ``kaiser_best`` filter (a Kaiser-windowed sinc, 64 zero crossings, 512 table
entries per crossing, linear interpolation between entries, gain scaled by the ratio when down-sampling) as a polyphase
table per rational ratio, computed once on the host in float64 -- **parity unpinned**: neither librosa nor resampy was at
hand to compare against.  Output length ``ceil(n * to / from)``.
"""
from __future__ import annotations

import json
import math
import os
import struct
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ..runtime import binding as bd
from .speech_encoder import DEFAULT_CONV as LARGE_CONV, SpeechEncoder

REFERENCE_MODEL = "facebook/wav2vec2-large-960h-lv60-self"
POS_W = "wav2vec2.encoder.pos_conv_embed.conv.weight"
_POS_SPELLINGS = ((POS_W + "_g", POS_W + "_v"),
                  ("wav2vec2.encoder.pos_conv_embed.conv.parametrizations.weight.original0",
                   "wav2vec2.encoder.pos_conv_embed.conv.parametrizations.weight.original1"))


# ---- checkpoint files ---------------------------------------------------------------------------------------------
_ST_DTYPES = {"F64": np.float64, "F32": np.float32, "F16": np.float16, "I64": np.int64, "I32": np.int32, "I16": np.int16,
              "I8": np.int8, "U8": np.uint8, "BOOL": np.bool_}


def read_safetensors(path: str) -> Dict[str, torch.Tensor]:
    """The safetensors container: u64 little-endian header length, a JSON index {name: {dtype, shape, data_offsets}},
    then the tensors' raw little-endian bytes."""
    with open(path, "rb") as f:
        (n,) = struct.unpack("<Q", f.read(8))
        index = json.loads(f.read(n).decode("utf-8"))
        data = f.read()
    out: Dict[str, torch.Tensor] = {}
    for name, rec in index.items():
        if name == "__metadata__":
            continue
        lo, hi = rec["data_offsets"]
        shape = [int(s) for s in rec["shape"]]
        if rec["dtype"] == "BF16":
            raw = np.frombuffer(data[lo:hi], dtype="<u2").astype(np.uint32) << 16
            t = torch.from_numpy(raw.view(np.float32).copy())
        elif rec["dtype"] in _ST_DTYPES:
            dt = np.dtype(_ST_DTYPES[rec["dtype"]]).newbyteorder("<")
            t = torch.from_numpy(np.frombuffer(data[lo:hi], dtype=dt).astype(_ST_DTYPES[rec["dtype"]]).copy())
        else:
            raise ValueError(f"{path}: tensor {name!r} has unsupported dtype {rec['dtype']!r}")
        out[name] = t.reshape(shape)
    return out


def load_pretrained_files(path: str) -> Tuple[dict, Dict[str, int], Dict[str, torch.Tensor]]:
    """(config.json, vocab.json, state_dict) of a local model directory in the Hugging Face layout."""
    if not os.path.isdir(path):
        raise FileNotFoundError(
            f"--model_path {path!r} is not a directory.  Nothing is downloaded here: fetch {REFERENCE_MODEL} (the recogniser "
            "the reference's evalute_s2s_bleu.py uses) yourself and point --model_path at the directory holding its "
            "config.json, vocab.json and pytorch_model.bin or model.safetensors")
    with open(os.path.join(path, "config.json")) as f:
        config = json.load(f)
    with open(os.path.join(path, "vocab.json")) as f:
        vocab = json.load(f)
    st, pt = os.path.join(path, "model.safetensors"), os.path.join(path, "pytorch_model.bin")
    if os.path.exists(st):
        sd = read_safetensors(st)
    elif os.path.exists(pt):
        sd = torch.load(pt, map_location="cpu")
    else:
        raise FileNotFoundError(f"{path}: neither model.safetensors nor pytorch_model.bin")
    return config, vocab, sd


# ---- resampling ---------------------------------------------------------------------------------------------------
KAISER_BEST = {"num_zeros": 64, "precision": 9, "rolloff": 0.9475937167399596, "beta": 14.769656459379492}


def kaiser_best_window() -> Tuple[np.ndarray, int]:
    """resampy's ``kaiser_best`` half window (float64) and its table entries per zero crossing.  Parity unpinned."""
    nb = 2 ** KAISER_BEST["precision"]
    n = nb * KAISER_BEST["num_zeros"]
    r = KAISER_BEST["rolloff"]
    sinc = r * np.sinc(r * np.linspace(0, KAISER_BEST["num_zeros"], num=n + 1, endpoint=True))
    taper = np.kaiser(2 * n + 1, KAISER_BEST["beta"])[n:]
    return taper * sinc, nb


_tables: Dict[Tuple[int, int], Tuple[np.ndarray, int, int, int]] = {}


def polyphase_table(sr_from: int, sr_to: int) -> Tuple[np.ndarray, int, int, int]:
    """(table [L][KW] fp32, L, M, KL) of the ratio ``sr_to / sr_from = L / M``: output t reads inputs
    ``(t M) // L - KL + 1 + d`` with weights ``table[(t M) % L][d]``.  Phase p's left wing (inputs n, n - 1, ..) and right
    wing (n + 1, n + 2, ..) are the window values resampy's interpolation loop visits for the fractional time p / L,
    linearly interpolated between table entries, in float64."""
    key = (int(sr_from), int(sr_to))
    if key in _tables:
        return _tables[key]
    g = math.gcd(*key)
    L, M = key[1] // g, key[0] // g
    win, nb = kaiser_best_window()
    ratio = key[1] / key[0]
    if ratio < 1:
        win = win * ratio
    delta = np.append(np.diff(win), 0.0)
    scale = min(1.0, ratio)
    step = int(scale * nb)
    nwin = win.shape[0]
    wings = []
    for p in range(L):
        both = []
        for frac in (scale * (p / L), scale - scale * (p / L)):
            idx = frac * nb
            off = int(idx)
            eta = idx - off
            cnt = (nwin - off) // step
            pos = off + step * np.arange(cnt)
            both.append(win[pos] + eta * delta[pos])
        wings.append(both)
    KL = max(len(w[0]) for w in wings)
    KR = max(len(w[1]) for w in wings)
    table = np.zeros((L, KL + KR), np.float64)
    for p, (wl, wr) in enumerate(wings):
        table[p, KL - len(wl):KL] = wl[::-1]
        table[p, KL:KL + len(wr)] = wr
    _tables[key] = (table.astype(np.float32), L, M, KL)
    return _tables[key]


def resample(waves: Sequence[torch.Tensor], sr_from: int, sr_to: int, device=None) -> List[torch.Tensor]:
    """Band-limited resampling of a ragged list of 1-D waveforms in ONE launch; returns device tensors of
    ``ceil(n * sr_to / sr_from)`` samples.  Equal rates: the inputs, moved to the device."""
    device = torch.device(device) if device is not None else _default_device()
    waves = [torch.as_tensor(w, dtype=torch.float32).reshape(-1) for w in waves]
    if int(sr_from) == int(sr_to) or not waves:
        return [w.to(device) for w in waves]
    table, L, M, KL = polyphase_table(sr_from, sr_to)
    n_in = [int(w.numel()) for w in waves]
    n_out = [-(-n * L // M) for n in n_in]
    B, Ni, No = len(waves), max(max(n_in), 1), max(max(n_out), 1)
    # (waveforms that are already on the device -- translate.py's generated audio -- are gathered there, not on the host)
    x = torch.zeros(B, Ni, dtype=torch.float32, device=device if all(w.device == device for w in waves) else None)
    for b, w in enumerate(waves):
        x[b, :n_in[b]] = w
    x = x.to(device)
    bd.require_device(x)
    lens = torch.tensor(n_in, dtype=torch.int32).to(device)
    tab = torch.from_numpy(table).to(device)
    y = torch.empty(B, No, dtype=torch.float32, device=device)
    bd.call("s2st_resample_sinc_f32", x, lens, tab, y, B, Ni, No, L, M, KL, table.shape[1])
    return [y[b, :n_out[b]] for b in range(B)]


def _default_device() -> torch.device:
    if bd.is_emulator() or not torch.cuda.is_available():
        return torch.device("cpu")
    return torch.device("cuda", torch.cuda.current_device())


# ---- the recogniser -----------------------------------------------------------------------------------------------
class Wav2Vec2CTC(SpeechEncoder):
    """wav2vec2-large-960h-lv60-self geometry by default (conv stack 7 x 512 with bias, 24 x 1024, 16 heads, ffn 4096,
    pos conv 128 taps / 16 groups, vocabulary 32)."""
    kind = "w2v_ctc"
    CONV_W = ("wav2vec2.feature_extractor.conv_layers.", ".conv.weight")
    POS_W = POS_W
    LABEL = "wav2vec 2.0"

    def __init__(self, device=None, conv=None, embed=1024, layers=24, heads=16, ffn=4096, conv_pos=128,
                 conv_pos_groups=16, vocab=32, precise: bool = False, pad_token_id: int = 0,
                 vocab_map: Optional[Dict[str, int]] = None, word_delimiter: str = "|"):
        device = torch.device(device) if device is not None else _default_device()
        self.pad_token_id, self.word_delimiter = int(pad_token_id), word_delimiter
        self.id_to_token = {int(i): t for t, i in (vocab_map or {}).items()}
        self._create_encoder(device, conv or LARGE_CONV, embed, layers, heads, ffn, conv_pos, conv_pos_groups, precise, vocab)

    @classmethod
    def from_config(cls, config: dict, vocab_map: Optional[Dict[str, int]] = None, device=None, precise: bool = False):
        """Geometry from a transformers ``config.json``; anything but the layer-norm / stable-layer-norm variant with
        biased convolutions is refused (the group-norm variant is the HuBERT front end's, models/hubert.py)."""
        if config.get("feat_extract_norm", "group") != "layer" or not config.get("do_stable_layer_norm", False) or \
                not config.get("conv_bias", False):
            raise ValueError("only the wav2vec 2.0 'layer-norm' variant is supported (feat_extract_norm='layer', "
                             f"do_stable_layer_norm=true, conv_bias=true, as {REFERENCE_MODEL})")
        if config.get("feat_extract_activation", "gelu") != "gelu" or config.get("hidden_act", "gelu") != "gelu":
            raise ValueError("only GELU activations are supported")
        conv = list(zip(config["conv_dim"], config["conv_kernel"], config["conv_stride"]))
        return cls(device, conv=conv, embed=config["hidden_size"], layers=config["num_hidden_layers"],
                   heads=config["num_attention_heads"], ffn=config["intermediate_size"],
                   conv_pos=config["num_conv_pos_embeddings"], conv_pos_groups=config["num_conv_pos_embedding_groups"],
                   vocab=config["vocab_size"], precise=precise, pad_token_id=config.get("pad_token_id", 0) or 0,
                   vocab_map=vocab_map)

    @classmethod
    def from_pretrained(cls, path: str, device=None, precise: bool = False) -> "Wav2Vec2CTC":
        config, vocab, sd = load_pretrained_files(path)
        net = cls.from_config(config, vocab, device, precise)
        net.load_state_dict(sd)
        return net

    # -- parameters: transformers names / layouts <-> engine arena ---------------------------------------------------
    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = True):
        sd = dict(sd)
        for g_name, v_name in _POS_SPELLINGS:
            if g_name in sd and v_name in sd:
                g, v = sd.pop(g_name), sd.pop(v_name)
                sd[POS_W + "_g"], sd[POS_W + "_v"] = g, v
                break
        for k, shape in self._needed(sd, strict).items():
            if k in sd and tuple(sd[k].shape) != tuple(shape):
                raise ValueError(f"{k}: shape {tuple(sd[k].shape)}, expected {tuple(shape)}")
        self._copy_in(sd)

    # -- forward -----------------------------------------------------------------------------------------------------
    def forward_padded(self, wave: torch.Tensor, sample_lens: Sequence[int]):
        """wave [B, N] fp32 raw samples (whatever lies behind an utterance's length is ignored), 16 kHz.  Returns
        ``(logits [B, T, vocab], frame_lens list, ids [B, T] int32, counts [B] int32)``, all device tensors but the list:
        rows of ``logits`` at or past an utterance's frame count are not meaningful; ``ids[b, :counts[b]]`` are the
        collapsed token ids of its valid frames."""
        wave = wave.to(self.device, torch.float32).contiguous()
        bd.require_device(wave)
        B, N = wave.shape
        T = self.out_frames(N)
        sample_lens = [int(n) for n in sample_lens]
        if len(sample_lens) != B or max(sample_lens) > N:
            raise ValueError("one length per row, none beyond the padded width")
        frame_lens = [self.out_frames(n) for n in sample_lens]
        if T <= 0 or min(frame_lens) <= 0:
            raise ValueError(f"an utterance of {min(sample_lens)} samples is shorter than the conv stack's receptive field")
        lens = torch.tensor([sample_lens, frame_lens], dtype=torch.int32).to(self.device)
        logits = torch.empty(B, T, self.vocab, dtype=torch.float32, device=self.device)
        res = torch.empty(B * T + B, dtype=torch.int32, device=self.device)  # ids, then counts: ONE block for the host
        self._reserve(B, N)
        self._forward(wave.data_ptr(), lens[0].data_ptr(), lens[1].data_ptr(), B, N, self.pad_token_id, logits.data_ptr(),
                      res.data_ptr(), res.data_ptr() + 4 * B * T)
        self._keep = (wave, lens)
        self._last_block = res
        return logits, frame_lens, res[:B * T].view(B, T), res[B * T:]

    def forward(self, waves: Sequence[torch.Tensor]):
        """A ragged list of 1-D 16 kHz waveforms, zero-padded to the longest."""
        waves = [torch.as_tensor(w, dtype=torch.float32).reshape(-1) for w in waves]
        lens = [int(w.numel()) for w in waves]
        x = torch.zeros(len(waves), max(lens), dtype=torch.float32, device=self.device)
        for b, w in enumerate(waves):
            x[b, :lens[b]] = w.to(self.device)
        return self.forward_padded(x, lens)

    __call__ = forward

    def decode(self, ids: Sequence[int]) -> str:
        """Collapsed ids -> text as ``Wav2Vec2CTCTokenizer`` writes it: tokens joined, the word delimiter as a space,
        stripped."""
        return "".join(" " if self.id_to_token[int(i)] == self.word_delimiter else self.id_to_token[int(i)]
                       for i in ids).strip()

    def transcribe(self, waves: Sequence[torch.Tensor]) -> List[str]:
        """Text of a ragged list of 16 kHz waveforms.  An utterance shorter than the conv stack's receptive field (no frame
        at all: a degenerate generated wave) gets the empty string and stays out of the batch."""
        if not self.id_to_token:
            raise ValueError("no vocabulary: build the recogniser with vocab_map (vocab.json)")
        waves = [torch.as_tensor(w).reshape(-1) for w in waves]
        keep = [i for i, w in enumerate(waves) if self.out_frames(w.numel()) > 0]
        out = [""] * len(waves)
        if not keep:
            return out
        B = len(keep)
        self.forward([waves[i] for i in keep])
        block = self._last_block.cpu().numpy()  # the one device-to-host read of the batch
        T = (block.size - B) // B
        ids, counts = block[:B * T].reshape(B, T), block[B * T:]
        for b, i in enumerate(keep):
            out[i] = self.decode(ids[b, :counts[b]])
        return out

    FRAME_SECONDS = 0.02  # one frame per 320 samples at 16 kHz

    def encode_text(self, text: str) -> List[int]:
        """The recogniser's spelling of a text: upper case, every space a word delimiter (``decode`` strips the delimiters
        at a transcript's ends; a text that keeps them as spaces aligns them too).  A character the vocabulary does not
        hold is refused by name."""
        token_to_id = {t: i for i, t in self.id_to_token.items()}
        ids = []
        for ch in text.upper().replace(" ", self.word_delimiter):
            if ch not in token_to_id:
                raise ValueError(f"align: the character {ch!r} of {text!r} is not in the recogniser's vocabulary")
            ids.append(token_to_id[ch])
        return ids

    def align(self, waves: Sequence[torch.Tensor], texts: Sequence[str], aligner: str = "device"):
        """Word timings of known texts in 16 kHz waveforms: per utterance a list of ``ctc_align.Segment(text, start, end,
        score)`` with start / end in seconds (frame x 0.02) and the frame-weighted mean log-probability of the word's
        characters; the empty list when the text has no path through the utterance's frames.  CTC forced alignment
        (ctc_align.py: ties to the smaller jump; parity unpinned) of the characters against log-softmax of the valid
        frames' logits.  No reference counterpart: evalute_s2s_bleu.py only transcribes."""
        from .. import ctc_align
        if not self.id_to_token:
            raise ValueError("no vocabulary: build the recogniser with vocab_map (vocab.json)")
        if len(waves) != len(texts):
            raise ValueError(f"{len(waves)} waveforms, {len(texts)} texts")
        targets = [self.encode_text(t) for t in texts]
        logits, frame_lens, _, _ = self.forward(waves)
        B, T, V = logits.shape
        lprobs = torch.empty_like(logits)  # (rows behind an utterance's frames stay unwritten: the aligner never reads them)
        for b in range(B):
            bd.call("s2st_log_softmax_rows_f32", logits[b], V, lprobs[b], V, frame_lens[b], V, 1)
        als = ctc_align.forced_align(lprobs, targets, frame_lens, blank=self.pad_token_id, layout="BTV", aligner=aligner)
        out = []
        for al, ids in zip(als, targets):
            words = ctc_align.segments(al, [self.id_to_token[i] for i in ids], sep=self.word_delimiter)
            out.append([ctc_align.Segment(w.text, w.start * self.FRAME_SECONDS, w.end * self.FRAME_SECONDS, w.score)
                        for w in words])
        self.last_alignments = als
        return out
