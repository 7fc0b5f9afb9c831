#!/usr/bin/env python3
"""Throughput of stage 3 (fbank / log-mel extraction) on the GPU and on the host (informational: the README's default
``--extractor`` comes from here).

    python tools/feature_extract_rate.py [--utts 256] [--repeats 5] [--inner 50] [--out profiles/feature_extract_rate.txt]

Seeded audio (tests/audio_feat_synth.signal) whose lengths are the bench corpus's (synthetic Fisher corpus, seed 1234):
source utterances of ``src_n_frames`` filter-bank frames at 16 kHz, target utterances of ``tgt_n_frames`` x 300 samples at
24 kHz.  Three parts:
  1. kernel only: the batch already on the device, device events around --inner back-to-back calls (each call: the
     offsets scan + the kernels of the route), the routes in turn per repeat (alternating runs), median and range of
     the per-call time; audio-seconds per second, and the bytes the kernel has to move (valid samples in,
     feature rows out) per second against the HBM peak;
  2. the stage end to end (``preprocessing.get_feature_manifest``: PCM files -> data directory) with --extractor device and
  3. the same corpus with --extractor host, alternating, wall clock; and the time of reading the files alone.
The stage's default n_fft 1200 is timed through the mixed-radix FFT kernel (the default) and through the dense bf16x3 product
(``DeviceFeatureExtractor(fft=False)``: what this size took before the FFT kernels had a plan for it).
Also both routes' error at n_fft 1200 against the reference golden (tests/golden/audio_features.npz), as the tests print it.
"""
import argparse
import importlib
import os
import struct
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import audio_feat_synth as AS  # noqa: E402

PKG = "speech-to-speech-translation_amd"
HBM_PEAK = 8.0e12  # bytes / s (MI355X data sheet)


def wav_bytes(x_i16, sr):
    body = np.asarray(x_i16, dtype="<i2").tobytes()
    hdr = b"RIFF" + struct.pack("<I", 36 + len(body)) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1, 1, sr, sr * 2, 2, 16)
    return hdr + b"data" + struct.pack("<I", len(body)) + body


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=50, help="calls per timed window of the kernel-only part")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feature_extract_rate.txt"))
    args = ap.parse_args()
    D = importlib.import_module(PKG + ".data.synthetic")
    fx = importlib.import_module(PKG + ".data.feature_extraction")
    stage = importlib.import_module(PKG + ".preprocessing.get_feature_manifest")
    bd = importlib.import_module(PKG + ".runtime.binding")
    import __graft_entry__ as ge
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    corpus = D.SyntheticFisherCorpus(n_utts=args.utts, seed=1234)
    n_src = [400 + 160 * (int(t) - 1) for t in corpus.src_n_frames]
    n_tgt = [300 * int(t) for t in corpus.tgt_n_frames]
    src = [AS.signal(n, 16000, 1000 + i) for i, n in enumerate(n_src)]
    tgt = [AS.signal(n, 24000, 2000 + i) for i, n in enumerate(n_tgt)]
    src16 = [np.round(20000 * w).astype(np.float32) for w in src]
    import ctypes as C
    buf = C.create_string_buffer(32)
    bd.lib().s2st_source_hash(buf, 32)
    say(f"# tools/feature_extract_rate.py --utts {args.utts} --repeats {args.repeats} --inner {args.inner}")
    say(f"# source hash {buf.value.decode()} (tree: {ge.source_hash()}); device {torch.cuda.get_device_name(0)}")
    s_src, s_tgt = sum(n_src) / 16000.0, sum(n_tgt) / 24000.0
    say(f"# {args.utts} utterances: source {s_src:.1f} s at 16 kHz ({min(n_src)} .. {max(n_src)} samples), target {s_tgt:.1f} s "
        f"at 24 kHz ({min(n_tgt)} .. {max(n_tgt)} samples)")

    # ---- 1. kernel only ----------------------------------------------------------------------------------------------
    ex = fx.DeviceFeatureExtractor(dev, max_samples=1 << 40)  # one batch: the whole corpus
    ex_dense = fx.DeviceFeatureExtractor(dev, max_samples=1 << 40, fft=False)
    forms = [("fbank 16 kHz (512-point FFT)", src16, 16000, None, ex),
             ("log-mel n_fft 2048 win 1200 hop 300 (FFT)", tgt, 24000, (2048, 1200, 300, 80, 20, 8000), ex),
             ("log-mel n_fft 1200 win 1024 hop 300 (FFT)", tgt, 24000, (1200, 1024, 300, 80, 20, 8000), ex),
             ("log-mel n_fft 1200 win 1024 hop 300 (dense)", tgt, 24000, (1200, 1024, 300, 80, 20, 8000), ex_dense)]
    runs = []
    for name, waves, sr, lm, ex in forms:
        captured = {}
        orig = ex._run

        def spy(ws, frames_of, n_bins, launch, _c=captured, _o=orig):
            def launch2(wave, ln, out, offs, U, Lmax, rows, pairs):
                _c["args"] = (wave, ln, out, offs, U, Lmax, rows, pairs)
                _c["launch"] = launch
                launch(wave, ln, out, offs, U, Lmax, rows, pairs)
            return _o(ws, frames_of, n_bins, launch2)
        ex._run = spy
        (ex.fbank(waves, sr) if lm is None else ex.logmel(waves, sr, lm[0], lm[1], lm[2], lm[3], lm[4], lm[5]))
        ex._run = orig
        rows = captured["args"][6]
        nbytes = 4.0 * sum(len(w) for w in waves) + 4.0 * rows * 80
        runs.append((name, captured, sum(len(w) for w in waves) / sr, nbytes, []))
    for name, c, _, _, _ in runs:  # warm-up
        for _ in range(3):
            c["launch"](*c["args"])
    torch.cuda.synchronize()
    for _ in range(args.repeats):
        for name, c, _, _, ts in runs:  # alternating
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.inner):
                c["launch"](*c["args"])
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) * 1e-3 / args.inner)
    say()
    say(f"{'kernel only (batch on the device)':<46} {'ms median [min .. max]':>28} {'audio-s/s':>11} {'GB/s':>8} {'of HBM peak':>12}")
    for name, c, secs, nbytes, ts in runs:
        ts = np.array(ts)
        m = float(np.median(ts))
        say(f"{name:<46} {m * 1e3:10.3f} [{ts.min() * 1e3:.3f} .. {ts.max() * 1e3:.3f}] {secs / m:11.0f} {nbytes / m / 1e9:8.1f} "
            f"{100.0 * nbytes / m / HBM_PEAK:11.2f}%")
    say("# (bytes: valid samples read + feature rows written; the dense route also moves its bf16x3 frames and the spectrum)")

    # ---- both routes' error at n_fft 1200 against the reference golden ------------------------------------------------------
    golden = np.load(os.path.join(ROOT, "tests", "golden", "audio_features.npz"))
    g = AS.LOGMEL_DENSE_GEOMETRY
    key = AS.geometry_key(g)
    say()
    for route, e_, bound in (("FFT", forms[2][4], "8 x the reference's own fp32 error"), ("dense", ex_dense, "2e-3")):
        feats, _ = e_.logmel(AS.logmel_inputs(g), g[3], g[0], g[1], g[2], AS.N_MELS, g[4], g[5])
        err = max(float(np.abs(a - golden[f"{key}.logmel.{j}"]).max()) for j, a in enumerate(feats))
        say(f"# {route} route (n_fft 1200) against the reference's extract_logmel_spectrogram, five seeded inputs: max log-domain "
            f"difference {err:.3e} (bound of the test: {bound}; the reference's own fp32 error: {float(golden[key + '.ref_f64_err']):.1e})")

    # ---- 2. / 3. the stage end to end ---------------------------------------------------------------------------------
    with tempfile.TemporaryDirectory() as d:
        audio = os.path.join(d, "audio")
        os.makedirs(audio)
        rows = []
        for i in range(args.utts):
            ps, pt = os.path.join(audio, f"s{i}.wav"), os.path.join(audio, f"t{i}.wav")
            open(ps, "wb").write(wav_bytes(np.round(20000 * src[i]).astype(np.int16), 16000))
            open(pt, "wb").write(wav_bytes(np.round(20000 * tgt[i]).astype(np.int16), 24000))
            rows.append([f"utt{i}", ps, pt, "a b", "c d", f"spk{i % 4}"])
        with open(os.path.join(audio, "train.audio_phone.tsv"), "w") as f:
            f.write("\t".join(["id", "src_audio", "tgt_audio", "src_text", "tgt_text", "speaker"]) + "\n")
            for r in rows:
                f.write("\t".join(r) + "\n")
        t0 = time.perf_counter()
        for r in rows:
            stage.load_audio(r[1])
            stage.load_audio(r[2])
        t_read = time.perf_counter() - t0
        times = {"device": [], "host": []}
        k = 0
        for rep in range(max(2, args.repeats // 2) + 1):
            for extractor in ("device", "host"):  # alternating; the first pair is the warm-up
                out = os.path.join(d, f"out{k}")
                k += 1
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                stage.main(["-m", audio, "-o", out, "--splits", "train", "--ipa-vocab", "--extractor", extractor])
                torch.cuda.synchronize()
                if rep:
                    times[extractor].append(time.perf_counter() - t0)
    say()
    say(f"{'stage end to end (files -> data directory)':<46} {'s median [min .. max]':>28} {'audio-s/s':>11} {'utt/s':>8}")
    for extractor in ("device", "host"):
        ts = np.array(times[extractor])
        m = float(np.median(ts))
        say(f"{'--extractor ' + extractor + ' (n_fft 1200)':<46} {m:10.3f} [{ts.min():.3f} .. {ts.max():.3f}] "
            f"{(s_src + s_tgt) / m:11.0f} {args.utts / m:8.1f}")
    say(f"# reading the {2 * args.utts} PCM files alone (page cache warm): {t_read:.3f} s; host threads: "
        f"{os.environ.get('OMP_NUM_THREADS', 'unset')} (OMP_NUM_THREADS), torch {torch.get_num_threads()}")
    d_, h_ = float(np.median(times["device"])), float(np.median(times["host"]))
    say(f"# faster end to end: --extractor {'device' if d_ < h_ else 'host'} ({h_ / d_:.2f} x host time / device time)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
