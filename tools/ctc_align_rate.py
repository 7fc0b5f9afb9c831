#!/usr/bin/env python3
"""Cost of CTC forced alignment on the GPU (informational: the README quotes the medians this writes).

    python tools/ctc_align_rate.py [--utts 256] [--calls 50] [--rounds 5] [--host-utts 64] [--out profiles/ctc_align_rate.txt]

Two geometries over the bench corpus (synthetic Fisher corpus, seed 1234), seeded log-probabilities (log-softmax of
standard-normal draws), every utterance in ONE call:
  (a) the model's CTC head: frames = source frames // 4 (<= 750), target = the source text length, V = the source vocabulary;
  (b) the recogniser: frames = the 16 kHz length of the target audio / 320, one character per three frames, V = 32.
Three forms, alternated in one process for --rounds rounds: s2st_ctc_align_f32 with the back-pointers in LDS (route 1, where
the geometry fits), in the workspace (route 2) -- device events around --calls calls after a warm-up, outputs preallocated,
nothing read back -- and ctc_align.host_forced_align on the same log-probabilities including their device-to-host copy, on the
first --host-utts utterances (the numpy form takes seconds per batch; its figure is scaled to the whole batch).  The parent
of this feature has no aligner, so the host form is the basis of comparison.  Per form: median [min .. max] of the rounds;
"frame latency" = kernel time / the longest utterance's frames, the serial chain every workgroup walks.
"""
import argparse
import ctypes as C
import importlib
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "speech-to-speech-translation_amd"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=256)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-utts", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctc_align_rate.txt"))
    args = ap.parse_args()
    D = importlib.import_module(PKG + ".data.synthetic")
    CA = importlib.import_module(PKG + ".ctc_align")
    bd = importlib.import_module(PKG + ".runtime.binding")
    import __graft_entry__ as ge
    dev = torch.device("cuda:0")
    lib = bd.lib()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    buf = C.create_string_buffer(32)
    lib.s2st_source_hash(buf, 32)
    mhz = getattr(torch.cuda.get_device_properties(0), "clock_rate", 2400000) / 1000.0  # (MI355X: 2.4 GHz peak engine clock)
    say(f"# tools/ctc_align_rate.py --utts {args.utts} --calls {args.calls} --rounds {args.rounds} --host-utts {args.host_utts}")
    say(f"# source hash {buf.value.decode()} (tree: {ge.source_hash()}); device {torch.cuda.get_device_name(0)}, {mhz:.0f} MHz")
    corpus = D.SyntheticFisherCorpus(n_utts=args.utts, seed=1234)
    rs = np.random.RandomState(99)
    fr_a = np.minimum(np.maximum(corpus.src_n_frames // 4, 1), 750)
    n16 = corpus.tgt_n_frames * 200  # 24 kHz, 300 samples per frame -> 16 kHz
    fr_b = np.maximum((n16 - 400) // 320 + 1, 1)
    geos = (("a", "model head", fr_a, np.minimum(corpus.src_text_len, fr_a), int(corpus.src_vocab)),
            ("b", "recogniser", fr_b, np.maximum(fr_b // 3, 1), 32))
    summary = {}
    for tag, name, frames, tlens, V in geos:
        B, E, Lmax = len(frames), int(frames.max()), int(tlens.max())
        lp = torch.log_softmax(torch.from_numpy(rs.standard_normal((B, E, V)).astype(np.float32)), -1).to(dev)
        targets = [rs.randint(4, V, size=int(n)).tolist() for n in tlens]
        tg = torch.zeros(B, Lmax, dtype=torch.int64)
        for b, t in enumerate(targets):
            tg[b, :len(t)] = torch.tensor(t)
        tg = tg.to(dev)
        il = torch.tensor(frames.astype(np.int32)).to(dev)
        tl = torch.tensor(tlens.astype(np.int32)).to(dev)
        ft = torch.empty(B, E, dtype=torch.int32, device=dev)
        ts, te = (torch.empty(B, Lmax, dtype=torch.int32, device=dev) for _ in range(2))
        tsc = torch.empty(B, Lmax, device=dev)
        sc = torch.empty(B, device=dev)
        nws = int(lib.s2st_ctc_align_workspace(B, E, Lmax))
        ws = torch.empty(nws, dtype=torch.uint8, device=dev)

        def call(route):
            return lib.s2st_ctc_align_f32(lp.data_ptr(), E * V, V, tg.data_ptr(), Lmax, il.data_ptr(), tl.data_ptr(), B, E, V, 0,
                                          route, ft.data_ptr(), ts.data_ptr(), te.data_ptr(), tsc.data_ptr(), sc.data_ptr(),
                                          ws.data_ptr(), nws, C.c_void_p(bd.stream_ptr()))

        say()
        say(f"# ({tag}) {name}: {B} utterances in one call, frames {int(frames.min())} .. {E} (median {int(np.median(frames))}), "
            f"targets {int(tlens.min())} .. {Lmax} (median {int(np.median(tlens))}), V = {V}, workspace {nws / 2**20:.1f} MiB")
        routes = [r for r in (1, 2) if call(r) == 0]
        torch.cuda.synchronize()
        if 1 not in routes:
            say("# route 1 (back-pointers in LDS) does not fit this geometry: S2ST_ERR_SHAPE")
        ref = None
        for r in routes:  # the forms agree before they are timed
            call(r)
            got = [x.cpu().clone() for x in (ft, ts, te, tsc, sc)]
            assert ref is None or all(torch.equal(x, y) for x, y in zip(ref, got))
            ref = got
        n_host = min(args.host_utts, B)
        times = {r: [] for r in routes}
        times["host"] = []
        for _ in range(args.rounds):
            for r in routes:
                for _ in range(3):
                    call(r)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.calls):
                    call(r)
                e1.record()
                e1.synchronize()
                times[r].append(e0.elapsed_time(e1) * 1e3 / args.calls)  # us per call
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host = lp[:n_host].cpu().numpy()
            for b in range(n_host):
                CA.host_forced_align(host[b], targets[b], 0, int(frames[b]))
            times["host"].append((time.perf_counter() - t0) * 1e6 * B / n_host)
        say(f"{'form':<34} {'us per batch: median [min .. max]':>40} {'frame latency':>26}")
        for k in routes + ["host"]:
            t = np.array(times[k])
            label = {1: "device, route 1 (LDS)", 2: "device, route 2 (workspace)",
                     "host": f"host (numpy; {n_host} utts, scaled)"}[k]
            lat = "" if k == "host" else f"{np.median(t) * 1e3 / E:8.0f} ns = {np.median(t) * mhz / E:6.0f} cycles"
            say(f"{label:<34} {np.median(t):16.1f} [{t.min():.1f} .. {t.max():.1f}] {lat:>26}")
            summary[(tag, k)] = t
        best = min(routes, key=lambda r: np.median(times[r]))
        say(f"# host / device (route {best}): {np.median(times['host']) / np.median(times[best]):.0f}x")
        if len(routes) == 2:
            t1, t2 = np.array(times[1]), np.array(times[2])
            apart = t1.max() < t2.min() or t2.max() < t1.min()
            say(f"# route 2 / route 1: {np.median(t2) / np.median(t1):.2f}x (ranges {'apart' if apart else 'OVERLAP'})")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
