#!/usr/bin/env python3
"""Griffin-Lim timing on the GPU at the geometry stage 3 of the recipe writes (n_fft 1200 / window 1024 / hop 300) and, for
scale, at bench.py's config 5 geometry (2048 / 1200 / 300).

    python tools/gl_rate.py [--utts 64] [--iters 64] [--repeats 10] [--out profiles/gl_rate.txt]

One ragged batch: the target lengths (mel frames) of the bench corpus's first --utts utterances (synthetic Fisher corpus, seed
1234), magnitudes |randn|, explicit seeded initial phases (the batched launch form the bench runs).  Per route, device events
around ``GriffinLim.batch`` with --iters iterations and with 0 iterations (the initial inverse transform plus the host's
preparation of the batch, which is the same for every route); (t_iters - t_0) / iters is the time of one iteration = one
STFT + projection + inverse STFT of the whole batch.  Two warm-up calls per route, then --repeats rounds that take the
routes in turn (alternating runs); median and range.

Routes: whatever ``GriffinLim`` picks for the geometry, and the dense bf16x3 GEMM form (S2ST_GL_FFT=0).  At a commit whose
library has no FFT plan for 1200 both lines of that geometry are the dense form.  The FFT and the dense result of the same
inputs are compared (2 iterations) before anything is timed.
"""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PKG = "speech-to-speech-translation_amd"
GEOMETRIES = [(1200, 1024, 300), (2048, 1200, 300)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=64)
    ap.add_argument("--iters", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gl_rate.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/gl_rate.py needs a HIP device")
    dev = torch.device("cuda", 0)
    D = importlib.import_module(PKG + ".data.synthetic")
    V = importlib.import_module(PKG + ".vocoder")
    bd = importlib.import_module(PKG + ".runtime.binding")
    import __graft_entry__ as ge
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    corpus = D.SyntheticFisherCorpus(n_utts=args.utts, seed=1234)
    Ts = [int(t) for t in corpus.tgt_n_frames[:args.utts]]
    import ctypes as C
    buf = C.create_string_buffer(32)
    bd.lib().s2st_source_hash(buf, 32)
    say(f"# tools/gl_rate.py --utts {args.utts} --iters {args.iters} --repeats {args.repeats}")
    say(f"# source hash {buf.value.decode()} (tree: {ge.source_hash()}); device {torch.cuda.get_device_name(0)}")
    say(f"# {len(Ts)} utterances, {sum(Ts)} frames ({min(Ts)} .. {max(Ts)}), padded batch {len(Ts)} x {max(Ts)}")

    runs = []
    for n_fft, win, hop in GEOMETRIES:
        Fq = n_fft // 2 + 1
        rs = np.random.RandomState(n_fft)
        specs = [torch.from_numpy(np.abs(rs.randn(Fq, t)).astype(np.float32)).to(dev) for t in Ts]
        angs = [np.angle(np.exp(2j * np.pi * rs.rand(Fq, t))).astype(np.float32) for t in Ts]
        check = {}
        for route, env in (("default", None), ("dense", "0")):
            if env is None:
                os.environ.pop("S2ST_GL_FFT", None)
            else:
                os.environ["S2ST_GL_FFT"] = env
            gls = {n: V.GriffinLim(n_fft, win, hop, n, dev) for n in (args.iters, 0, 2)}
            os.environ.pop("S2ST_GL_FFT", None)
            name = f"n_fft {n_fft} win {win} hop {hop}: {'FFT' if gls[0].use_fft else 'dense'}" + (" (default)" if env is None else " (S2ST_GL_FFT=0)")
            check[route] = torch.cat(gls[2].batch(specs, angs))
            runs.append((name, gls, specs, angs, {args.iters: [], 0: []}))
        torch.cuda.synchronize()
        d = float((check["default"] - check["dense"]).abs().max() / check["dense"].abs().max())
        say(f"# n_fft {n_fft}: default route against the dense route after 2 iterations, same inputs: {d:.2e} of the waveform scale")
        del check
    for name, gls, specs, angs, _ in runs:  # warm-up
        for n in (args.iters, 0):
            for _ in range(2):
                gls[n].batch(specs, angs)
    torch.cuda.synchronize()
    for _ in range(args.repeats):
        for name, gls, specs, angs, ts in runs:  # alternating
            for n in (args.iters, 0):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                gls[n].batch(specs, angs)
                b.record()
                b.synchronize()
                ts[n].append(a.elapsed_time(b))
    say()
    say(f"{'route':<52} {str(args.iters) + ' iterations, ms median [min .. max]':>40} {'0 iterations':>14} {'ms / iteration':>15}")
    for name, _, _, _, ts in runs:
        t, t0 = np.array(ts[args.iters]), np.array(ts[0])
        m, m0 = float(np.median(t)), float(np.median(t0))
        say(f"{name:<52} {m:16.2f} [{t.min():.2f} .. {t.max():.2f}] {m0:14.2f} {(m - m0) / max(args.iters, 1):15.3f}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
