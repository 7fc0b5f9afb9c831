#!/usr/bin/env python3
"""What the fused front end of ``translate`` costs against the route a user had before it (informational; gates nothing).

    python tools/translate_rate.py [--utts 256] [--repeats 5] [--steps 100] [--out profiles/translate_rate.txt]

Seeded 16-bit PCM (tests/audio_feat_synth.signal) with the bench corpus's source lengths (synthetic Fisher corpus, seed 1234),
base-size random weights as ``bench.py --config infer_base`` makes them, batches as ``translate`` forms them (--max-tokens
100000).  Timed in one process, alternating, wall clock with a device synchronisation at both ends, over all batches:
  (a) the fused front end: ``DeviceFeatureExtractor.fbank_batch`` from host PCM -- pack, ONE int16 upload, the kernel that
      writes the normalised, padded encoder input;
  (b) the existing route: ``DeviceFeatureExtractor.fbank`` (upload, kernel, copy back), the host's global CMVN per utterance,
      ``_collate_frames``, upload of the padded batch;
and a whole ``SpeechTranslator.translate`` call (--steps AR steps per batch, Griffin-Lim 64 iterations, no text heads), to show
the front end's share.  Median and range of each.
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
import audio_feat_synth as AS  # noqa: E402

PKG = "speech-to-speech-translation_amd"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=100, help="AR steps per batch of the whole-call timing")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "translate_rate.txt"))
    args = ap.parse_args()
    import s2st_amd  # noqa: F401
    import __graft_entry__ as ge
    C_ = importlib.import_module(PKG + ".configs")
    D = importlib.import_module(PKG + ".data")
    DS = importlib.import_module(PKG + ".data.s2st_dataset")
    T = importlib.import_module(PKG + ".translate")
    tasks = importlib.import_module(PKG + ".tasks")
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    corpus = D.SyntheticFisherCorpus(n_utts=args.utts, seed=1234)
    n_src = [400 + 160 * (int(t) - 1) for t in corpus.src_n_frames]
    pcm = [np.round(20000 * AS.signal(n, 16000, 1000 + i)).astype(np.int16) for i, n in enumerate(n_src)]
    rs = np.random.RandomState(4)
    mean, std = (rs.standard_normal(80) * 3 - 5.123).astype(np.float32), rs.uniform(0.7, 4.3, 80).astype(np.float32)

    a = C_.recipe_args("base_recipe")
    a.max_target_positions, a.eos_prob_threshold, a.spec_bwd_max_iter, a.vocoder = args.steps, 2.0, 64, "griffin_lim"
    task = tasks.S2ST_TranslationTask.setup_task(a, device=dev)
    torch.manual_seed(1)
    np.random.seed(1)
    model = task.build_model(a)  # random-init weights of the architecture, as bench.py --config infer_base
    tr = T.SpeechTranslator(task, model, a, dev, max_tokens=100000, cmvn=(mean, std))
    ex = tr.extractor
    order = np.argsort(-np.asarray(corpus.src_n_frames), kind="stable")
    groups = [g.tolist() for g in D.batch_by_size(order, np.asarray(corpus.src_n_frames, dtype=np.int64)[order], 100000, -1, 1)]
    buf = __import__("ctypes").create_string_buffer(32)
    tr.model.engine.lib.s2st_source_hash(buf, 32)
    say(f"# tools/translate_rate.py --utts {args.utts} --repeats {args.repeats} --steps {args.steps}")
    say(f"# source hash {buf.value.decode()} (tree: {ge.source_hash()}); device {torch.cuda.get_device_name(0)}")
    say(f"# {args.utts} utterances, {sum(n_src) / 16000.0:.1f} s of 16 kHz PCM ({min(n_src)} .. {max(n_src)} samples), "
        f"{int(np.sum(corpus.src_n_frames))} frames in {len(groups)} batches of {[len(g) for g in groups]}")

    def fused():
        out = []
        for g in groups:
            out.append(ex.fbank_batch([pcm[i] for i in g], 16000, tr.mean, tr.std))
        return out

    def existing():
        out = []
        for g in groups:
            feats, _ = ex.fbank([pcm[i].astype(np.float32) for i in g], 16000)
            frames = [torch.from_numpy(np.divide(np.subtract(f, mean), std)).float() for f in feats]
            out.append((DS._collate_frames(frames).to(dev), torch.tensor([f.shape[0] for f in feats])))
        return out

    x, y = fused(), existing()
    torch.cuda.synchronize()
    same = all(torch.equal(p[0], q[0]) for p, q in zip(x, y))
    say(f"# the two routes' encoder inputs are bit-identical on this corpus: {same}")
    del x, y
    times = {"fused": [], "existing": []}
    for _ in range(args.repeats):
        for name, fn in (("fused", fused), ("existing", existing)):  # alternating
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
    audio = [(p, 16000) for p in pcm]
    tr.translate(audio[:len(groups[0])])  # warm-up: workspaces, twin engines, vocoder tables
    whole = []
    for _ in range(max(3, args.repeats // 2)):
        np.random.seed(1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hyps = tr.translate(audio)
        torch.cuda.synchronize()
        whole.append(time.perf_counter() - t0)
    assert all(h is not None for h in hyps)
    say()
    say(f"{'front end, all batches (host PCM -> encoder input)':<58} {'ms median [min .. max]':>30} {'audio-s/s':>11}")
    med = {}
    for name, label in (("fused", "(a) fbank_batch: one int16 upload, one fused launch"),
                        ("existing", "(b) fbank + copy back + host CMVN + collate + upload")):
        ts = np.array(times[name])
        med[name] = float(np.median(ts))
        say(f"{label:<58} {med[name] * 1e3:12.2f} [{ts.min() * 1e3:.2f} .. {ts.max() * 1e3:.2f}] {sum(n_src) / 16000.0 / med[name]:11.0f}")
    fa, ea = np.array(times["fused"]), np.array(times["existing"])
    if fa.max() < ea.min():
        say(f"# (a) is faster than (b) outside the run-to-run range: {med['existing'] / med['fused']:.2f} x at the medians")
    elif ea.max() < fa.min():
        say(f"# (a) is SLOWER than (b) outside the run-to-run range: {med['fused'] / med['existing']:.2f} x at the medians; the "
            f"reason for the fused path is device residency, not time")
    else:
        say("# (a) is not faster than (b) outside the run-to-run range (the ranges overlap): the reason for the fused path is "
            "device residency, not time")
    ws = np.array(whole)
    wm = float(np.median(ws))
    say()
    say(f"whole translate call ({args.utts} utterances, {args.steps} AR steps per batch, Griffin-Lim 64 iterations, PCM out): "
        f"{wm:.3f} s median [{ws.min():.3f} .. {ws.max():.3f}], {args.utts / wm:.1f} utterances/s")
    say(f"# the fused front end's share of it: {100.0 * med['fused'] / wm:.2f} % (with route (b) it would be "
        f"{100.0 * med['existing'] / (wm - med['fused'] + med['existing']):.2f} %)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
