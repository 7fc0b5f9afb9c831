#!/usr/bin/env python3
"""Throughput of the ASR-BLEU recogniser on the GPU (informational: the README's recommended --batch_size comes from here).

    python tools/asr_bleu_rate.py [--utts 256] [--repeats 3] [--out profiles/asr_bleu_rate.txt]

Seeded 24 kHz audio (tests/w2v_ctc_synth.synth_audio) whose lengths are the bench corpus's target lengths (synthetic
Fisher corpus, seed 1234: target mel frames x 300 samples, the 12.5 ms hop of the 24 kHz vocoder dump), resampled to 16 kHz
on the device, then transcribed by the wav2vec2-large-960h-lv60-self geometry with the seeded weights of
tests/w2v_ctc_synth.py, batched by length as ``s2st_amd.evaluate_s2s_bleu`` batches, in both GEMM modes at --batch_size
160000 (the reference script's default), 1.6 M and 8 M samples.  Per row: utterances/s and audio-seconds/s of a whole pass
(host batching, upload of the padded batch, forward, the one device-to-host read per batch, id -> text), median and range
of the repeats.  If ``transformers`` is importable, its own Wav2Vec2ForCTC forward (fp32 and bf16 autocast, same padded
batches, argmax on the device) is a yardstick row; if not, the file says so.
"""
import argparse
import importlib
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import w2v_ctc_synth as WS  # noqa: E402

PKG = "speech-to-speech-translation_amd"
SIZES = (160000, 1600000, 8000000)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "asr_bleu_rate.txt"))
    args = ap.parse_args()
    D = importlib.import_module(PKG + ".data.synthetic")
    M = importlib.import_module(PKG + ".models.wav2vec2_ctc")
    EV = importlib.import_module(PKG + ".evaluate_s2s_bleu")
    bd = importlib.import_module(PKG + ".runtime.binding")
    import __graft_entry__ as ge
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    corpus = D.SyntheticFisherCorpus(n_utts=args.utts, seed=1234)
    n24 = [int(t) * 300 for t in corpus.tgt_n_frames]
    waves24 = [WS.synth_audio(n, 5000 + i, rate=24000) for i, n in enumerate(n24)]
    import ctypes as C
    buf = C.create_string_buffer(32)
    bd.lib().s2st_source_hash(buf, 32)
    say(f"# tools/asr_bleu_rate.py --utts {args.utts} --repeats {args.repeats}")
    say(f"# source hash {buf.value.decode()} (tree: {ge.source_hash()}); device {torch.cuda.get_device_name(0)}")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    waves = M.resample(waves24, 24000, 16000, dev)
    torch.cuda.synchronize()
    t_first = time.perf_counter() - t0
    t0 = time.perf_counter()
    waves = M.resample(waves24, 24000, 16000, dev)
    torch.cuda.synchronize()
    t_res = time.perf_counter() - t0
    lens = [int(w.numel()) for w in waves]
    secs = sum(lens) / 16000.0
    say(f"# {args.utts} utterances, {secs:.1f} s of audio at 16 kHz, lengths {min(lens)} .. {max(lens)} samples (median "
        f"{int(np.median(lens))}); seeded weights, large geometry (24 x 1024)")
    say(f"# resampling 24000 -> 16000 Hz, all utterances in one launch incl. host padding and upload: {t_res * 1e3:.1f} ms "
        f"(first call, with the filter table: {t_first * 1e3:.1f} ms) = {secs / t_res:.0f} audio-s/s")
    sd = WS.synth_state(WS.LARGE)
    head = f"{'form':<44} {'batches':>7} {'utt/s':>9} {'audio-s/s':>10} {'s/pass median [min .. max]':>30}"
    say()
    say(head)
    best = {}
    for precise in (False, True):
        net = M.Wav2Vec2CTC(dev, precise=precise, vocab_map=WS.VOCAB, **WS.LARGE)
        net.load_state_dict(sd)
        for bs in SIZES:
            batches = EV.length_batches(lens, bs)

            def one_pass():
                torch.cuda.synchronize()
                t = time.perf_counter()
                n = 0
                for b in batches:
                    n += len(net.transcribe([waves[i] for i in b]))
                torch.cuda.synchronize()
                return time.perf_counter() - t
            one_pass()  # warm-up: workspace growth, code objects
            ts = np.array([one_pass() for _ in range(args.repeats)])
            tag = f"{'bf16x3 (--precise)' if precise else 'bf16 operands'} --batch_size {bs}"
            say(f"{tag:<44} {len(batches):7d} {args.utts / np.median(ts):9.1f} {secs / np.median(ts):10.1f} "
                f"{np.median(ts):10.3f} [{ts.min():.3f} .. {ts.max():.3f}]")
            best[(precise, bs)] = ts
        del net
        torch.cuda.empty_cache()
    say()
    try:
        from transformers import Wav2Vec2Config, Wav2Vec2ForCTC
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import gen_golden_w2v_ctc as G
        hc = {k: v for k, v in WS.hf_config(WS.LARGE).items() if k not in ("model_type", "architectures")}
        model = Wav2Vec2ForCTC(Wav2Vec2Config(**hc)).eval()
        model.load_state_dict(G.library_state(sd, model), strict=False)
        model = model.to(dev)
        bs = SIZES[1]
        batches = EV.length_batches(lens, bs)

        def lib_pass(autocast):
            torch.cuda.synchronize()
            t = time.perf_counter()
            for b in batches:
                ws = [waves[i] for i in b]
                n = max(int(w.numel()) for w in ws)
                x = torch.zeros(len(ws), n, device=dev)
                mask = torch.zeros(len(ws), n, dtype=torch.long, device=dev)
                for j, w in enumerate(ws):
                    x[j, :w.numel()] = (w - w.mean()) / torch.sqrt(w.var(unbiased=False) + 1e-7)
                    mask[j, :w.numel()] = 1
                with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                    model(x, attention_mask=mask).logits.argmax(-1).cpu()
            torch.cuda.synchronize()
            return time.perf_counter() - t
        for autocast in (True, False):
            lib_pass(autocast)
            ts = np.array([lib_pass(autocast) for _ in range(args.repeats)])
            tag = f"transformers {'bf16 autocast' if autocast else 'fp32'} --batch_size {bs}"
            say(f"{tag:<44} {len(batches):7d} {args.utts / np.median(ts):9.1f} {secs / np.median(ts):10.1f} "
                f"{np.median(ts):10.3f} [{ts.min():.3f} .. {ts.max():.3f}]")
        say("# (yardstick: the library's forward + argmax on the same device; no resampling, no text)")
    except Exception as e:  # noqa: BLE001
        say(f"# no yardstick row: transformers' own forward could not be run on this machine ({type(e).__name__}: {e})")
    fast = {bs: np.median(best[(False, bs)]) for bs in SIZES}
    pick = min(fast, key=fast.get)
    say()
    say(f"# bf16 operands: fastest --batch_size of the three: {pick} ({args.utts / fast[pick]:.0f} utt/s; "
        + ", ".join(f"{bs}: {args.utts / fast[bs]:.0f}" for bs in SIZES) + ")")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
