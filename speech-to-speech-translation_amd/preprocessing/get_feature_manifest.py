"""Stage 3 of ``examples/s2s_trans/run_baseline.sh`` / ``run_prompt_tuning.sh``: audio manifests -> the data directory
``train.py`` takes as its first argument.

    python -m s2st_amd.preprocessing.get_feature_manifest --audio-manifest-root M --output-root O --ipa-vocab

Counterpart of ``examples/s2s_trans/preprocessing/get_feature_manifest.py:41-199`` (and ``get_feature_manifest_8k.py``, whose
one difference in arithmetic -- the source audio converted to 8 kHz -- is ``--src-sample-rate 8000`` here) with the same flags.
Reads ``<split>.audio_phone.tsv`` (columns id, src_audio, tgt_audio, src_text, tgt_text, speaker) and writes

  * ``src_logmelspec80.zip`` (Kaldi filter bank of the source audio, 16-bit range) and ``tgt_logmelspec80.zip`` (log-mel
    spectrogram of the target audio): ZIP_STORED archives of ``<id>.npy``;
  * ``src_gcmvn_stats.npz`` / ``tgt_gcmvn_stats.npz`` (``mean``, ``std``: ``get_global_cmvn``'s formula, 1e-10 variance floor);
  * ``<split>.tsv`` with the reference's columns and ``<zip>:<offset>:<length>`` paths as ``get_zip_manifest`` forms them;
  * ``src_vocab.txt`` / ``tgt_vocab.txt`` (``Counter.most_common`` order over the train split), ``speakers.txt``;
  * ``config.yaml``: the keys of ``examples/s2s_trans/preprocessing/data_utils.py: gen_config_yaml`` plus the ``features``
    block.  The reference writes the target statistics under the key ``tgr_global_cmvn`` (sic, data_utils.py:387) while the
    transform it lists is ``tgt_global_cmvn``: both keys are written here, so the directory loads as it stands.

Only ``csv``, ``zipfile`` and ``yaml`` are needed.  Without ``--ipa-vocab`` the reference trains a sentencepiece model: that
case is refused.  Text is taken from the manifest as it stands (g2p / phonemisation is stage 2).

PARITY UNPINNED (restatements, nothing here to check them against):
  * sample-rate changes -- sox's ``rate`` effect in the reference -- go through this package's band-limited resampler
    (``models/wav2vec2_ctc.resample`` -> ``s2st_resample_sinc_f32``, the path ``evaluate_s2s_bleu`` uses; needs the device);
  * ``--normalize-volume`` -- sox ``gain -n`` -- scales the waveform to a peak of 1.0;
  * the Kaldi filter bank is the operator ``data/audio_utils.kaldi_fbank`` documents (torchaudio itself is not in the image).

``--extractor device`` (default, see README "State" for the measurement that chose it) runs csrc/features.hip over batches of
utterances; ``--extractor host`` runs ``kaldi_fbank`` and the numpy log-mel per utterance (a machine without a GPU; the rate
yardstick).
"""
from __future__ import annotations

import argparse
import csv
import io
import zipfile
from collections import Counter
from pathlib import Path
from typing import Dict, List, Tuple

import numpy as np

from ..data import audio_utils
from ..data import feature_extraction as fx

COLUMNS = ["id", "src_audio", "tgt_audio", "src_n_frames", "tgt_n_frames", "src_text", "speaker", "tgt_text"]
SRC_NAME, TGT_NAME = "src_logmelspec80", "tgt_logmelspec80"


def load_tsv_to_dicts(path) -> List[dict]:
    with open(path, "r") as f:
        reader = csv.DictReader(f, delimiter="\t", quotechar=None, doublequote=False, lineterminator="\n",
                                quoting=csv.QUOTE_NONE)
        return [dict(e) for e in reader]


def save_tsv(rows: List[dict], path):
    with open(path, "w", newline="") as f:
        w = csv.writer(f, delimiter="\t", quotechar=None, doublequote=False, lineterminator="\n", quoting=csv.QUOTE_NONE,
                       escapechar="\\")
        w.writerow(COLUMNS)
        for r in rows:
            w.writerow([r[c] for c in COLUMNS])


def npy_bytes(a: np.ndarray) -> bytes:
    buf = io.BytesIO()
    np.save(buf, a)
    return buf.getvalue()


def get_zip_manifest(zip_path: Path) -> Tuple[Dict[str, str], Dict[str, int]]:
    """``examples/speech_to_text/data_utils.py:108-132``: ``<zip>:<offset>:<size>`` and the frame count per stem (the frame
    count from the .npy header alone)."""
    paths, lengths = {}, {}
    with zipfile.ZipFile(zip_path, mode="r") as z:
        info = z.infolist()
    with open(zip_path, "rb") as f:
        for i in info:
            assert i.compress_type == zipfile.ZIP_STORED, i.filename
            stem = Path(i.filename).stem
            offset = i.header_offset + 30 + len(i.filename)
            paths[stem] = f"{zip_path.as_posix()}:{offset}:{i.file_size}"
            f.seek(offset)
            assert audio_utils.is_npy_data(f.read(2)), i.filename
            f.seek(offset)
            version = np.lib.format.read_magic(f)
            shape = (np.lib.format.read_array_header_1_0 if version == (1, 0) else np.lib.format.read_array_header_2_0)(f)[0]
            lengths[stem] = int(shape[0])
    return paths, lengths


def load_audio(path: str) -> Tuple[np.ndarray, int]:
    """Mono float32 waveform in [-1, 1) and its sample rate."""
    wav, sr = audio_utils.get_waveform(path, normalization=True, mono=True, always_2d=False)
    return np.ascontiguousarray(wav, dtype=np.float32), int(sr)


def normalize_volume(wav: np.ndarray) -> np.ndarray:
    """sox ``gain -n``: scale to a peak of 1.0 (0 dBFS).  Parity unpinned."""
    peak = float(np.abs(wav).max()) if wav.size else 0.0
    return wav if peak == 0.0 else (wav / np.float32(peak)).astype(np.float32)


def to_rate(waves: List[np.ndarray], rates: List[int], to_sr, device) -> List[np.ndarray]:
    """Utterances whose rate differs from ``to_sr`` through the device resampler, one launch per source rate."""
    if to_sr is None:
        return waves
    out = list(waves)
    for sr in sorted({r for r in rates if r != int(to_sr)}):
        if device is None:
            raise RuntimeError(f"audio at {sr} Hz has to be resampled to {to_sr} Hz: that runs on the device (--extractor device)")
        from ..models.wav2vec2_ctc import resample
        idx = [i for i, r in enumerate(rates) if r == sr]
        for i, y in zip(idx, resample([waves[i] for i in idx], sr, int(to_sr), device=device)):
            out[i] = y.cpu().numpy()
    return out


class _Side:
    """One archive being written: the zip, the running moments (float64) and the frame counts."""

    def __init__(self, zip_path: Path):
        self.zip = zipfile.ZipFile(zip_path, "w", zipfile.ZIP_STORED)
        self.moments, self.n_frames = None, 0

    def add(self, ids, feats, moments):
        for i, f in zip(ids, feats):
            self.zip.writestr(zipfile.ZipInfo(f"{i}.npy"), npy_bytes(f))
            self.n_frames += int(f.shape[0])
        m = np.asarray(moments, dtype=np.float64).sum(axis=0)
        self.moments = m if self.moments is None else self.moments + m

    def close(self, npz_path: Path):
        self.zip.close()
        mean, std = fx.global_cmvn(self.moments[None], self.n_frames)
        np.savez(npz_path, mean=mean, std=std)


def extract(args, samples, out_root: Path, src_zip: Path, tgt_zip: Path, src_npz: Path, tgt_npz: Path):
    device = None
    if args.extractor == "device":
        ex = fx.DeviceFeatureExtractor(args.device)
        device = ex.device
    src, tgt = _Side(src_zip), _Side(tgt_zip)
    lm = dict(n_fft=args.n_fft, win_length=args.win_length, hop_length=args.hop_length, n_mels=args.n_mels, f_min=args.f_min,
              f_max=args.f_max)
    for b0 in range(0, len(samples), args.batch_utterances):
        chunk = samples[b0:b0 + args.batch_utterances]
        ids = [s["id"] for s in chunk]
        for side, column in ((src, "src_audio"), (tgt, "tgt_audio")):
            loaded = [load_audio(s[column]) for s in chunk]
            waves, rates = [w for w, _ in loaded], [r for _, r in loaded]
            if side is tgt and args.normalize_volume:
                waves = [normalize_volume(w) for w in waves]  # (the reference's effect order: gain -n, then rate)
            to_sr = args.src_sample_rate if side is src else args.sample_rate
            waves = to_rate(waves, rates, to_sr, device)
            rates = [r if to_sr is None else int(to_sr) for r in rates]
            if side is src:
                waves = [w * np.float32(2 ** 15) for w in waves]  # Kaldi compliance: the 16-bit range
            # (source audio may come at several rates when none is asked for: one extraction per rate, order restored)
            feats, moments = [None] * len(chunk), [None] * len(chunk)
            for sr in sorted(set(rates)):
                idx = [i for i, r in enumerate(rates) if r == sr]
                sub = [waves[i] for i in idx]
                if side is src:
                    f, m = ex.fbank(sub, sr, 80) if device is not None else _host(sub, lambda w: fx.host_fbank(w, sr, 80))
                else:
                    f, m = ex.logmel(sub, sr, **lm) if device is not None else _host(sub, lambda w: fx.host_logmel(w, sr, **lm))
                for k, i in enumerate(idx):
                    feats[i], moments[i] = f[k], m[k]
            side.add(ids, feats, np.stack(moments))
    src.close(src_npz)
    tgt.close(tgt_npz)


def _host(waves, fn):
    feats = [fn(w) for w in waves]
    return feats, fx.host_moments(feats)


def gen_config_yaml(out_root: Path, src_vocab_name: str, tgt_vocab_name: str, src_npz: Path, tgt_npz: Path, extra: dict):
    """``examples/s2s_trans/preprocessing/data_utils.py:135-215`` as stage 3 calls it (specaugment policy "ld", global CMVN,
    no input_channels / input_feat_per_channel)."""
    import yaml
    config = {
        "src_vocab_filename": src_vocab_name,
        "tgt_vocab_filename": tgt_vocab_name,
        "specaugment": {"time_wrap_W": 0, "freq_mask_N": 2, "freq_mask_F": 27, "time_mask_N": 2, "time_mask_T": 100,
                        "time_mask_p": 1.0},
        "src_transforms": {"_train": ["src_global_cmvn", "specaugment"], "*": ["src_global_cmvn"]},
        "tgt_transforms": {"*": ["tgt_global_cmvn"]},
        "src_global_cmvn": {"stats_npz_path": src_npz.as_posix()},
        "tgr_global_cmvn": {"stats_npz_path": tgt_npz.as_posix()},  # (sic: the key the reference writes)
        "tgt_global_cmvn": {"stats_npz_path": tgt_npz.as_posix()},  # the key the transform reads
        "audio_root": out_root.as_posix(),
    }
    config.update(extra)
    with open(out_root / "config.yaml", "w") as f:
        yaml.dump(config, f)


def process(args):
    assert "train" in args.splits
    if not args.ipa_vocab:
        raise SystemExit("without --ipa-vocab the reference trains a sentencepiece character model (spm_char): sentencepiece is "
                         "not part of this image, so that case is refused -- pass --ipa-vocab (vocabularies from the "
                         "manifest's own tokens)")
    out_root = Path(args.output_root).absolute()
    out_root.mkdir(exist_ok=True)
    manifest_root = Path(args.audio_manifest_root).absolute()
    samples = []
    for s in args.splits:
        for e in load_tsv_to_dicts(manifest_root / f"{s}.audio_phone.tsv"):
            e["split"] = s
            samples.append(e)
    src_zip, tgt_zip = out_root / f"{SRC_NAME}.zip", out_root / f"{TGT_NAME}.zip"
    src_npz, tgt_npz = out_root / "src_gcmvn_stats.npz", out_root / "tgt_gcmvn_stats.npz"
    if all(p.exists() for p in (src_zip, tgt_zip, src_npz, tgt_npz)):
        print(f"{src_zip} and {src_npz} exist.\n{tgt_zip} and {tgt_npz} exist.")
    else:
        print(f"Extracting features ({args.extractor})...")
        extract(args, samples, out_root, src_zip, tgt_zip, src_npz, tgt_npz)
    print("Fetching ZIP manifest...")
    src_paths, src_lengths = get_zip_manifest(src_zip)
    tgt_paths, tgt_lengths = get_zip_manifest(tgt_zip)
    print("Generating manifest...")
    by_split = {split: [] for split in args.splits}
    for s in samples:
        i = s["id"]
        by_split[s["split"]].append({"id": i, "src_audio": src_paths[i], "tgt_audio": tgt_paths[i],
                                     "src_n_frames": src_lengths[i], "tgt_n_frames": tgt_lengths[i],
                                     "src_text": s["src_text"], "speaker": s["speaker"], "tgt_text": s["tgt_text"]})
    for split in args.splits:
        save_tsv(by_split[split], out_root / f"{split}.tsv")
    for name, column in (("src_vocab.txt", "src_text"), ("tgt_vocab.txt", "tgt_text")):
        vocab = Counter()
        for r in by_split["train"]:
            vocab.update(r[column].split(" "))
        with open(out_root / name, "w") as f:
            for tok, c in vocab.most_common():
                f.write(f"{tok} {c}\n")
    speakers = sorted({s["speaker"] for s in samples})
    with open(out_root / "speakers.txt", "w") as f:
        for speaker in speakers:
            f.write(f"{speaker}\n")
    extra = {
        "sample_rate": args.sample_rate,
        "features": {
            "type": "spectrogram+melscale+log", "eps": 1e-5, "n_mels": args.n_mels, "n_fft": args.n_fft, "window_fn": "hann",
            "win_length": args.win_length, "hop_length": args.hop_length, "sample_rate": args.sample_rate,
            "win_len_t": args.win_length / args.sample_rate, "hop_len_t": args.hop_length / args.sample_rate,
            "f_min": args.f_min, "f_max": args.f_max, "n_stft": args.n_fft // 2 + 1,
        },
    }
    if len(speakers) > 1:
        extra["speaker_set_filename"] = "speakers.txt"
    gen_config_yaml(out_root, "src_vocab.txt", "tgt_vocab.txt", src_npz, tgt_npz, extra)


def get_parser():
    parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    parser.add_argument("--audio-manifest-root", "-m", required=True, type=str)
    parser.add_argument("--output-root", "-o", required=True, type=str)
    parser.add_argument("--splits", "-s", type=str, nargs="+", default=["train", "dev", "tst"])
    parser.add_argument("--ipa-vocab", action="store_true")
    parser.add_argument("--win-length", type=int, default=1024)
    parser.add_argument("--hop-length", type=int, default=300)
    parser.add_argument("--n-fft", type=int, default=1200)
    parser.add_argument("--n-mels", type=int, default=80)
    parser.add_argument("--f-min", type=int, default=20)
    parser.add_argument("--f-max", type=int, default=8000)
    parser.add_argument("--sample-rate", type=int, default=24000)
    parser.add_argument("--normalize-volume", "-n", action="store_true")
    parser.add_argument("--src-sample-rate", type=int, default=None,
                        help="convert the source audio to this rate first (8000: what get_feature_manifest_8k.py hard-codes)")
    parser.add_argument("--extractor", choices=["host", "device"], default="device")
    parser.add_argument("--device", type=str, default=None, help="torch device of --extractor device (default: the current one)")
    parser.add_argument("--batch-utterances", type=int, default=64, help="utterances read, extracted and written at a time")
    return parser


def main(argv=None):
    process(get_parser().parse_args(argv))


if __name__ == "__main__":
    main()
