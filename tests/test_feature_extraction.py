"""Stage 3 data preparation (csrc/features.hip, data/feature_extraction.py, preprocessing/get_feature_manifest.py).

Yardsticks: the Kaldi filter bank has no reference in the image (torchaudio is absent, parity unpinned): the device kernel is
checked against oracle/data_oracle.py: kaldi_fbank_f64 and the host ``kaldi_fbank`` within the bound this feature family
already has (tests/test_data_audio.py: 2e-3 in the log domain).  The log-mel spectrogram is checked against the REFERENCE's
``extract_logmel_spectrogram`` (tests/golden/audio_features.npz, tools/gen_golden_audio_features.py) within 8 x the reference's
own fp32-against-float64 error of the geometry: both sides are fp32 sums in different orders, each within about 1e-5 of
float64; the margin covers the differing mel summation order and the hardware log / sqrt.  The dense route (bf16x3 product)
has the family bound 2e-3.  Inputs: tests/audio_feat_synth.py (tones on a noise floor, far above the clamps)."""
import csv
import functools
import importlib
import os
import struct
import sys
import zipfile
from collections import Counter

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import audio_feat_synth as AS  # noqa: E402
from oracle import data_oracle  # noqa: E402

PKG = "speech-to-speech-translation_amd"
FAMILY_BOUND = 2e-3  # tests/test_data_audio.py:43
LOG_EPS32 = float(np.log(np.finfo(np.float32).eps))


def _fx():
    return importlib.import_module(PKG + ".data.feature_extraction")


def _extractor(backend):
    return _fx().DeviceFeatureExtractor(backend.device)


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "audio_features.npz"))


# ---- 1. filter bank ---------------------------------------------------------------------------------------------------------
# (sample rate, bins, lengths in batch order).  16 kHz: no frame (399, in the MIDDLE of the batch), one frame (400, 559), two
# (560), an odd count (5: a half-empty last pair), 98 frames; 8 kHz: 256-point transform; 24 kHz: 1024-point transform
FBANK_CASES = {
    "16k": (16000, 80, [400, 559, 560, 399, 400 + 160 * 4 + 17, 16047]),
    "8k": (8000, 80, [200, 8023]),
    "24k": (24000, 80, [600, 7440]),
    "16k-40bins": (16000, 40, [560, 1057]),
}


@functools.lru_cache(maxsize=None)
def _fbank_case(name):
    """Inputs and the two host yardsticks of a case, computed once."""
    fx = _fx()
    sr, n_bins, lens = FBANK_CASES[name]
    waves = [AS.fbank_input(n, sr, 7 + j) for j, n in enumerate(lens)]
    f64 = [data_oracle.kaldi_fbank_f64(w, sr, n_bins) for w in waves]
    host = [fx.host_fbank(w, sr, n_bins) for w in waves]
    return sr, n_bins, waves, f64, host


@pytest.mark.parametrize("name", list(FBANK_CASES))
def test_fbank_against_float64_and_host(backend, name):
    sr, n_bins, waves, f64, host = _fbank_case(name)
    ex = _extractor(backend)
    shift, size = int(sr * 0.01), int(sr * 0.025)
    batch, moments = ex.fbank(waves, sr, n_bins)  # one ragged batch
    alone = [ex.fbank([w], sr, n_bins)[0][0] for w in waves]
    assert moments.shape == (len(waves), 2, n_bins)
    worst64 = worsth = 0.0
    for w, a, b, r64, rh in zip(waves, batch, alone, f64, host):
        T = 0 if len(w) < size else 1 + (len(w) - size) // shift
        assert a.dtype == np.float32 and a.shape == b.shape == rh.shape == (T, n_bins) and r64.shape == (T, n_bins)
        assert np.array_equal(a, b)
        if T:
            worst64 = max(worst64, float(np.abs(a - r64).max()))
            worsth = max(worsth, float(np.abs(a - rh).max()))
    print(f"fbank {name} [{backend.kind}]: max |device - float64| {worst64:.3e}, max |device - host| {worsth:.3e}")
    assert worst64 < FAMILY_BOUND and worsth < FAMILY_BOUND


# ---- 2. / 3. log-mel against the reference ----------------------------------------------------------------------------------
def _logmel_against_golden(backend, golden, g, bound):
    n_fft, win, hop, sr, f_min, f_max = g
    key = AS.geometry_key(g)
    waves = AS.logmel_inputs(g, with_long=backend.kind == "hip")  # (about 0.9 s: on the GPU only)
    for j, w in enumerate(waves):
        assert AS.fingerprint([w]) == str(golden[f"{key}.fp.{j}"]), "the test's inputs are not the generator's"
    feats, _ = _extractor(backend).logmel(waves, sr, n_fft, win, hop, AS.N_MELS, f_min, f_max)
    worst = 0.0
    for j, (w, a) in enumerate(zip(waves, feats)):
        ref = golden[f"{key}.logmel.{j}"]
        assert a.dtype == np.float32 and a.shape == ref.shape == (1 + len(w) // hop, AS.N_MELS)
        # compared where the golden mel value is >= 1e-4 -- which, for these inputs, leaves out NOTHING
        mask = np.exp(ref.astype(np.float64)) >= 1e-4
        assert mask.all()
        worst = max(worst, float(np.abs(a - ref)[mask].max()))
    print(f"log-mel {key} [{backend.kind}]: max |device - reference| {worst:.3e}, bound {bound:.3e}")
    assert worst <= bound
    return worst


@pytest.mark.parametrize("g", AS.LOGMEL_FFT_GEOMETRIES, ids=AS.geometry_key)
def test_logmel_fft_route_against_the_reference(backend, golden, g):
    bd = backend.bd
    assert bd.lib().s2st_gl_fft_supported_i32(int(g[0]))
    _logmel_against_golden(backend, golden, g, 8.0 * float(golden[f"{AS.geometry_key(g)}.ref_f64_err"]))


def test_logmel_dense_route_against_the_reference(backend, golden):
    """n_fft 1200, the stage's default: no FFT kernel, the bf16x3 product with the dense basis.
    Observed: 6.7e-5 on the emulator's four short inputs, 9.1e-5 on the MI355X's five (profiles/feature_extract_rate.txt)."""
    g = AS.LOGMEL_DENSE_GEOMETRY
    assert not backend.bd.lib().s2st_gl_fft_supported_i32(int(g[0]))
    _logmel_against_golden(backend, golden, g, FAMILY_BOUND)


# ---- 4. clamps ---------------------------------------------------------------------------------------------------------------
def test_clamps_and_scaling(backend):
    ex = _extractor(backend)
    silence = np.zeros(1000, np.float32)
    fb = ex.fbank([silence], 16000)[0][0]
    assert fb.shape == (4, 80) and np.abs(fb - LOG_EPS32).max() <= 1e-6
    for g in (AS.LOGMEL_FFT_GEOMETRIES[2], AS.LOGMEL_DENSE_GEOMETRY):
        n_fft, win, hop, sr, f_min, f_max = g
        lm = ex.logmel([np.zeros(4 * hop + 1, np.float32)], sr, n_fft, win, hop, AS.N_MELS, f_min, f_max)[0][0]
        assert lm.shape == (5, AS.N_MELS) and np.abs(lm - np.log(1e-5)).max() <= 1e-6
    x = AS.fbank_input(3000, 16000, 3)
    d = ex.fbank([2 * x], 16000)[0][0] - ex.fbank([x], 16000)[0][0]
    assert np.abs(d - np.log(4.0)).max() <= 1e-4  # the front end is linear up to the log


# ---- 5. batch independence -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", [AS.LOGMEL_FFT_GEOMETRIES[0], AS.LOGMEL_DENSE_GEOMETRY], ids=AS.geometry_key)
def test_a_ragged_batch_equals_each_utterance_alone(backend, g):
    n_fft, win, hop, sr, f_min, f_max = g
    ex = _extractor(backend)
    waves = AS.logmel_inputs(g, with_long=False)
    waves = [waves[1], waves[0], waves[3], waves[2]]
    batch, mom = ex.logmel(waves, sr, n_fft, win, hop, AS.N_MELS, f_min, f_max)
    small = _fx().DeviceFeatureExtractor(backend.device, max_samples=1)  # a budget that puts every utterance in its own batch
    split, mom2 = small.logmel(waves, sr, n_fft, win, hop, AS.N_MELS, f_min, f_max)
    for w, a, b in zip(waves, batch, split):
        alone = ex.logmel([w], sr, n_fft, win, hop, AS.N_MELS, f_min, f_max)[0][0]
        assert np.array_equal(a, alone) and np.array_equal(b, alone)
    assert np.array_equal(mom, mom2)


# ---- 6. moments and global CMVN --------------------------------------------------------------------------------------------------
def test_moments_and_global_cmvn(backend, golden):
    fx = _fx()
    ex = _extractor(backend)
    sr, n_bins, waves, _, _ = _fbank_case("16k")
    feats, mom = ex.fbank(waves, sr, n_bins)
    assert np.array_equal(mom[3], np.zeros((2, n_bins), np.float32))  # the utterance without frames
    for f, m in zip(feats, mom):
        want = np.stack([f.astype(np.float64).sum(axis=0), (f.astype(np.float64) ** 2).sum(axis=0)])
        # (double accumulators in the kernel, one rounding to float32 at the end)
        assert np.allclose(m, want, rtol=1.2e-7, atol=0.0)
    assert np.array_equal(ex.moments(feats), mom)
    # the reference's get_global_cmvn over the golden arrays of a geometry (it sums in fp32: for at most 500 frames that
    # is n * eps ~ 3e-5 relative, times 3) against the moments kernel + the float64 fold of the utterances
    for g in AS.LOGMEL_GEOMETRIES:
        key = AS.geometry_key(g)
        arrays = [golden[f"{key}.logmel.{j}"] for j in range(len(AS.logmel_lengths(g)))]
        n = sum(a.shape[0] for a in arrays)
        assert n <= 500
        mean, std = fx.global_cmvn(ex.moments(arrays), n)
        for got, name in ((mean, "cmvn_mean"), (std, "cmvn_std")):
            ref = golden[f"{key}.{name}"]
            assert got.dtype == np.float32 and got.shape == ref.shape
            assert np.abs(got - ref).max() <= 1e-4 * np.abs(ref).max(), (key, name)


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals(backend, tmp_path):
    ex = _extractor(backend)
    ok = AS.signal(700, 16000, 1)
    for n in (256, 100, 0):
        with pytest.raises(ValueError, match="reflect"):
            ex.logmel([ok, ok[:n]], 16000, 512, 400, 160, AS.N_MELS, 0, 8000)
    with pytest.raises(ValueError, match="reflect"):
        _fx().host_logmel(ok[:256], 16000, 512, 400, 160, AS.N_MELS, 0, 8000)
    stage = importlib.import_module(PKG + ".preprocessing.get_feature_manifest")
    with pytest.raises(SystemExit, match="sentencepiece"):
        stage.main(["--audio-manifest-root", str(tmp_path), "--output-root", str(tmp_path / "out"), "--splits", "train"])


# ---- the archive layout against the reference's create_zip / get_zip_manifest ------------------------------------------------------
def test_zip_manifest_equals_the_reference(golden, tmp_path):
    stage = importlib.import_module(PKG + ".preprocessing.get_feature_manifest")
    assert "soundfile" in str(golden["helpers"]) or str(golden["helpers"]) == "direct"
    g = AS.LOGMEL_DENSE_GEOMETRY
    key = AS.geometry_key(g)
    order = [str(s) for s in golden[f"{key}.zip_order"]]
    zpath = tmp_path / "feat.zip"
    with zipfile.ZipFile(zpath, "w", zipfile.ZIP_STORED) as z:
        for stem in order:
            z.writestr(zipfile.ZipInfo(f"{stem}.npy"), stage.npy_bytes(golden[f"{key}.logmel.{stem[3:]}"]))
    paths, lengths = stage.get_zip_manifest(zpath)
    for k, stem in enumerate(order):
        assert paths[stem] == f"{zpath.as_posix()}:{int(golden[f'{key}.zip_offset'][k])}:{int(golden[f'{key}.zip_size'][k])}"
        assert lengths[stem] == int(golden[f"{key}.zip_frames"][k])


# ---- 8. the stage end to end -------------------------------------------------------------------------------------------------------
def _wav_bytes(x_i16, sr):
    x = np.asarray(x_i16, dtype="<i2")
    body = x.tobytes()
    hdr = b"RIFF" + struct.pack("<I", 36 + len(body)) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1, 1, sr, sr * 2, 2, 16)
    return hdr + b"data" + struct.pack("<I", len(body)) + body


SRC_WORDS = ["o l a", "k e", "t a l", "b j e n"]
TGT_WORDS = ["h @ l oU", "h aU", "A r", "j u", "f aI n"]
STAGE_ARGS = ["--ipa-vocab", "--splits", "train", "dev"]  # every other flag at the reference's default (n_fft 1200: dense route)


def _make_audio_corpus(root):
    """Six utterances, two splits, two speakers: 16 kHz source and 24 kHz target PCM files + <split>.audio_phone.tsv."""
    rs = np.random.RandomState(5)
    rows = {"train": [], "dev": []}
    waves = {}
    for i in range(6):
        split = "train" if i < 4 else "dev"
        ns, nt = int(rs.randint(4000, 6500)), int(rs.randint(3000, 5200))
        src = np.round(20000 * AS.signal(ns, 16000, 40 + i)).astype(np.int16)
        tgt = np.round(20000 * AS.signal(nt, 24000, 60 + i)).astype(np.int16)
        ps, pt = os.path.join(root, f"src{i}.wav"), os.path.join(root, f"tgt{i}.wav")
        open(ps, "wb").write(_wav_bytes(src, 16000))
        open(pt, "wb").write(_wav_bytes(tgt, 24000))
        st = " ".join(SRC_WORDS[k] for k in rs.randint(0, len(SRC_WORDS), size=3))
        tt = " ".join(TGT_WORDS[k] for k in rs.randint(0, len(TGT_WORDS), size=4))
        rows[split].append([f"utt{i}", ps, pt, st, tt, f"spk{i % 2}"])
        waves[f"utt{i}"] = (src.astype(np.float32), tgt.astype(np.float32) / np.float32(32768))
    for split, rr in rows.items():
        with open(os.path.join(root, f"{split}.audio_phone.tsv"), "w") as f:
            f.write("\t".join(["id", "src_audio", "tgt_audio", "src_text", "tgt_text", "speaker"]) + "\n")
            for r in rr:
                f.write("\t".join(r) + "\n")
    return rows, waves


def _read_tsv(path):
    with open(path) as f:
        return list(csv.DictReader(f, delimiter="\t", quotechar=None, doublequote=False, lineterminator="\n",
                                   quoting=csv.QUOTE_NONE))


def test_the_stage_end_to_end(backend, tmp_path):
    stage = importlib.import_module(PKG + ".preprocessing.get_feature_manifest")
    au = importlib.import_module(PKG + ".data.audio_utils")
    D = importlib.import_module(PKG + ".data")
    audio = tmp_path / "audio"
    audio.mkdir()
    rows, waves = _make_audio_corpus(str(audio))
    out = {}
    for extractor in ("device", "host"):
        out[extractor] = tmp_path / extractor
        stage.main(["--audio-manifest-root", str(audio), "--output-root", str(out[extractor]), "--extractor", extractor,
                    "--device", str(backend.device)] + STAGE_ARGS)
    root = out["device"]
    for name in ("src_logmelspec80.zip", "tgt_logmelspec80.zip", "src_gcmvn_stats.npz", "tgt_gcmvn_stats.npz", "train.tsv",
                 "dev.tsv", "src_vocab.txt", "tgt_vocab.txt", "speakers.txt", "config.yaml"):
        assert (root / name).is_file(), name
    for name in ("src_logmelspec80.zip", "tgt_logmelspec80.zip"):
        with zipfile.ZipFile(root / name) as z:
            assert len(z.infolist()) == 6 and all(i.compress_type == zipfile.ZIP_STORED for i in z.infolist())
    # every TSV path reads back as the extractor's own output for that utterance, bit for bit
    ex = _extractor(backend)
    ids = sorted(waves)
    src_feats, src_mom = ex.fbank([waves[i][0] for i in ids], 16000)
    tgt_feats, tgt_mom = ex.logmel([waves[i][1] for i in ids], 24000, 1200, 1024, 300, 80, 20, 8000)
    want = {i: (s, t) for i, s, t in zip(ids, src_feats, tgt_feats)}
    for split in ("train", "dev"):
        got, host = _read_tsv(root / f"{split}.tsv"), _read_tsv(out["host"] / f"{split}.tsv")
        assert list(got[0]) == ["id", "src_audio", "tgt_audio", "src_n_frames", "tgt_n_frames", "src_text", "speaker", "tgt_text"]
        assert [r["id"] for r in got] == [r[0] for r in rows[split]] == [r["id"] for r in host]
        for r, h, src_row in zip(got, host, rows[split]):
            s, t = au.get_features_or_waveform(r["src_audio"]), au.get_features_or_waveform(r["tgt_audio"])
            assert np.array_equal(s, want[r["id"]][0]) and np.array_equal(t, want[r["id"]][1])
            assert int(r["src_n_frames"]) == s.shape[0] == 1 + (len(waves[r["id"]][0]) - 400) // 160
            assert int(r["tgt_n_frames"]) == t.shape[0] == 1 + len(waves[r["id"]][1]) // 300
            assert (r["src_text"], r["tgt_text"], r["speaker"]) == (src_row[3], src_row[4], src_row[5])
            # --extractor host: the same frame counts, features within the bounds of the kernel tests
            assert (h["src_n_frames"], h["tgt_n_frames"]) == (r["src_n_frames"], r["tgt_n_frames"])
            assert np.abs(au.get_features_or_waveform(h["src_audio"]) - s).max() < FAMILY_BOUND
            assert np.abs(au.get_features_or_waveform(h["tgt_audio"]) - t).max() < FAMILY_BOUND
    # global CMVN statistics: get_global_cmvn's formula over all six utterances
    fx = _fx()
    for name, feats in (("src", src_feats), ("tgt", tgt_feats)):
        st = np.load(root / f"{name}_gcmvn_stats.npz")
        mean, std = fx.global_cmvn(fx.host_moments(feats), sum(f.shape[0] for f in feats))
        assert np.allclose(st["mean"], mean, rtol=1e-6, atol=1e-6) and np.allclose(st["std"], std, rtol=1e-6, atol=1e-6)
    # vocabularies: Counter.most_common order and counts over the train split
    for name, col in (("src_vocab.txt", 3), ("tgt_vocab.txt", 4)):
        c = Counter()
        for r in rows["train"]:
            c.update(r[col].split(" "))
        assert (root / name).read_text() == "".join(f"{t} {n}\n" for t, n in c.most_common())
    assert (root / "speakers.txt").read_text() == "spk0\nspk1\n"
    cfg = D.S2STDataConfig(root / "config.yaml")
    assert cfg.src_vocab_filename == "src_vocab.txt" and cfg.tgt_vocab_filename == "tgt_vocab.txt"
    assert cfg.speaker_set_filename == "speakers.txt" and cfg.audio_root == root.as_posix() and cfg.sample_rate == 24000
    assert cfg.src_global_cmvn_stats_npz == (root / "src_gcmvn_stats.npz").as_posix()
    assert cfg.tgt_global_cmvn_stats_npz == (root / "tgt_gcmvn_stats.npz").as_posix()
    assert cfg.config["tgr_global_cmvn"] == cfg.config["tgt_global_cmvn"]  # (the reference's spelling is kept beside it)
    assert cfg.config["features"] == {"type": "spectrogram+melscale+log", "eps": 1e-5, "n_mels": 80, "n_fft": 1200,
                                      "window_fn": "hann", "win_length": 1024, "hop_length": 300, "sample_rate": 24000,
                                      "win_len_t": 1024 / 24000, "hop_len_t": 300 / 24000, "f_min": 20, "f_max": 8000,
                                      "n_stft": 601}
    # the directory is what train.py takes: task set-up, the train split, one collated batch
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import s2st_oracle as O
    from test_engine import NANO
    tasks = importlib.import_module(PKG + ".tasks")
    a = O.make_args(**NANO)
    a.data, a.config_yaml = str(root), "config.yaml"
    task = tasks.S2ST_TranslationTask.setup_task(a)
    ds = task.load_dataset("train")
    assert len(ds) == 4
    batch = ds.collater([ds[i] for i in range(len(ds))])
    assert batch["net_input"]["src_speech"].shape[0] == 4 and batch["net_input"]["src_speech"].shape[2] == 80
