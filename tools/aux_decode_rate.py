#!/usr/bin/env python3
"""Rate of aux ASR / ST text decoding (stages 10 / 11: s2st_amd.generate_text) with the beam search on the host
(``--search host``: numpy, one blocking copy of the log-probabilities per generated token) and on the device (``--search
device``: s2st_beam_step, csrc/beam_search.hip).

Model: recipe_args("base_recipe"), seeded random weights.  Data: the bench's synthetic corpus, length-ordered max-tokens
batches.  Beam 5, both heads.  The two forms run ALTERNATELY in one process, ``--repeats`` times each after one warm-up batch
per form; every timed call is host clock around work that ends in a synchronise.  With random weights nearly every
hypothesis runs to max_len: the work is fixed and early termination is not exercised -- the step counts are printed.

    python tools/aux_decode_rate.py [--max-tokens 20000] [--max-len-b 50] [--batches 3] [--repeats 3] [--out FILE]
"""
import argparse
import importlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import s2st_amd  # noqa: E402,F401

PKG = "speech-to-speech-translation_amd"


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--max-tokens", type=int, default=20000)
    p.add_argument("--max-len-b", type=int, default=50)
    p.add_argument("--beam", type=int, default=5)
    p.add_argument("--batches", type=int, default=3)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--n-utts", type=int, default=512)
    p.add_argument("--polls", default="1,4,8,16,64", help="poll_every values of the device form's sweep")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "aux_decode_rate.txt"))
    args = p.parse_args()
    C = importlib.import_module(PKG + ".configs")
    tasks = importlib.import_module(PKG + ".tasks")
    D = importlib.import_module(PKG + ".data")
    seqgen = importlib.import_module(PKG + ".sequence_generator")
    dev = torch.device("cuda:0")
    a = C.recipe_args("base_recipe")
    task = tasks.S2ST_TranslationTask.setup_task(a, device=dev)
    torch.manual_seed(1)
    model = task.build_model(a)
    corpus = D.SyntheticFisherCorpus(n_utts=args.n_utts, seed=1234)
    groups = corpus.batches(max_tokens=args.max_tokens, bsz_mult=1)
    # the largest batches are the ones the recipe's --max-tokens fills: take them from the middle of the length order
    mid = len(groups) // 2
    groups = groups[mid:mid + args.batches]
    samples = [corpus.collate_batch(g.tolist()) for g in groups]
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/aux_decode_rate.py --max-tokens {args.max_tokens} --max-len-b {args.max_len_b} --beam {args.beam} "
        f"--batches {args.batches} --repeats {args.repeats}")
    say(f"# model base_recipe, seeded random weights; synthetic corpus, {len(samples)} batches of "
        f"{[int(s['id'].numel()) for s in samples]} sentences, source frames {[int(s['net_input']['src_speech'].shape[1]) for s in samples]}")
    say(f"# max_len_a 0, max_len_b {args.max_len_b}; device {torch.cuda.get_device_name(0)}")
    say("# random weights: hypotheses run to max_len -- fixed work, early termination is not exercised (steps column)")
    say("# ms/step = wall time of generate() / search steps; it includes the encoder forward and the cache set-up of the batch")

    def run(gen):
        """One pass over the batches: (seconds, sentences, generated tokens, steps, d2h copies)."""
        sec = sent = tok = steps = copies = 0
        for s in samples:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hyp = gen.generate([model], s)
            torch.cuda.synchronize()
            sec += time.perf_counter() - t0
            sent += len(hyp)
            tok += sum(len(h[0]["tokens"]) for h in hyp if h)
            steps += gen.last_steps
            copies += gen.last_d2h_copies
        return sec, sent, tok, steps, copies

    def make(which, search, poll=None):
        g = type("G", (), dict(aux_decoder=which, beam=args.beam, max_len_a=0, max_len_b=args.max_len_b, min_len=1, lenpen=1.0,
                               unkpen=0.0, search=search))()
        gen = task.build_generator([model], g)
        if poll is not None:
            gen.poll_every = poll
        return gen

    def row(tag, rs):
        sec = np.array([r[0] for r in rs])
        _, sent, tok, steps, copies = rs[0]
        ms = sec / steps * 1e3
        say(f"{tag:<28} {sent / np.median(sec):9.1f} {tok / np.median(sec):10.1f} {np.median(ms):9.3f} "
            f"[{ms.min():7.3f} .. {ms.max():7.3f}] {copies / steps:8.3f} {steps:6d}")
        return ms

    head = f"{'form':<28} {'sent/s':>9} {'tokens/s':>10} {'ms/step':>9} {'min .. max over repeats':>22} {'d2h/step':>8} {'steps':>6}"
    verdict = {}
    for which in ("asr", "st"):
        say()
        say(f"## head {which}, vocabulary {len(task.src_dict if which == 'asr' else task.tgt_dict)}, poll_every "
            f"{seqgen.DEFAULT_POLL_EVERY} (the default)")
        say(head)
        gens = {"host": make(which, "host"), "device": make(which, "device")}
        for g in gens.values():  # one warm-up batch per form
            g.generate([model], samples[0])
        torch.cuda.synchronize()
        res = {"host": [], "device": []}
        for _ in range(args.repeats):
            for k in ("host", "device"):
                res[k].append(run(gens[k]))
        ms = {k: row(f"{which} --search {k}", res[k]) for k in ("host", "device")}
        verdict[which] = (ms["device"].max() < ms["host"].min(), ms)
    say()
    say(f"## poll_every sweep, device form, head st ({args.repeats} repeats each, interleaved)")
    say(head)
    polls = [int(x) for x in args.polls.split(",")]
    gens = {pe: make("st", "device", pe) for pe in polls}
    res = {pe: [] for pe in polls}
    gens[polls[0]].generate([model], samples[0])
    torch.cuda.synchronize()
    for _ in range(args.repeats):
        for pe in polls:
            res[pe].append(run(gens[pe]))
    for pe in polls:
        row(f"st device poll_every {pe}", res[pe])
    say()
    for which, (faster, ms) in verdict.items():
        say(f"# {which}: device {np.median(ms['device']):.3f} ms/step [max {ms['device'].max():.3f}] vs host "
            f"{np.median(ms['host']):.3f} ms/step [min {ms['host'].min():.3f}]: device is "
            f"{'FASTER beyond the spread' if faster else 'NOT faster beyond the spread'}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
