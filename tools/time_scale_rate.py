#!/usr/bin/env python3
"""Cost of the time-scale modification on the GPU against the host form (informational: the README quotes what this writes).

    python tools/time_scale_rate.py [--utts 256] [--tempo 1.25] [--rounds 5] [--host-utts 16] [--out profiles/time_scale_rate.txt]

The bench corpus's target lengths (synthetic Fisher corpus, seed 1234; frames of 300 samples at 24 kHz) as seeded noise on a
tone, every recording compressed by --tempo in ONE call at the default geometry of that rate.  Forms, alternated in one
process for --rounds rounds, each timed with the host clock between two synchronisations:
  * the kernel alone (s2st_time_scale_pcm16: samples already on the device, outputs preallocated, nothing read back), once with
    the candidates at odd offsets from a funnel shift (S2ST_TS_ODD=funnel) and once from a second LDS image (=image);
  * ``time_scale.time_scale`` end to end: the upload of the int16 samples, the kernel, the read-back of samples and positions;
  * ``time_scale.host_time_scale``: the same rules in numpy, over the first --host-utts recordings and scaled to the batch
    by samples.
The forms agree before they are timed.  The parent of this feature has no time-scale modification, so the host form is the
basis of comparison.  Per form: median [min .. max] of the rounds.  One workgroup walks a recording's hops, so the kernel's
time is the longest recording's: kernel time / its hop count is what a hop costs.
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
RATE = 24000


def recording(n: int, seed: int) -> np.ndarray:
    rs = np.random.RandomState(seed)
    t = np.arange(n)
    period = rs.uniform(90, 260)  # a voice's pitch at 24 kHz
    return np.clip(9000 * np.sin(2 * np.pi * t / period) + rs.randint(-1500, 1501, n), -32768, 32767).astype(np.int16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=256)
    ap.add_argument("--tempo", type=float, default=1.25)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-utts", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_scale_rate.txt"))
    args = ap.parse_args()
    TS = importlib.import_module(PKG + ".time_scale")
    D_ = importlib.import_module(PKG + ".data.synthetic")
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
    say(f"# tools/time_scale_rate.py --utts {args.utts} --tempo {args.tempo:g} --rounds {args.rounds} --host-utts {args.host_utts}")
    say(f"# source hash {buf.value.decode()} (tree: {ge.source_hash()}); device {torch.cuda.get_device_name(0)}")
    corpus = D_.SyntheticFisherCorpus(n_utts=args.utts, seed=1234)
    lens = [int(f) * 300 for f in corpus.tgt_n_frames]
    waves = [recording(n, 100 + b) for b, n in enumerate(lens)]
    tm = TS.tempo_milli(args.tempo)
    ms = [TS.scaled_len(n, tm) for n in lens]
    N, D = TS.geometry(RATE)
    Hs = N // 2
    hops = [TS.n_hops(m, N) for m in ms]
    B = len(waves)

    # the kernel alone
    offs = np.zeros((3, B + 1), np.int64)
    for r, v in enumerate((lens, ms, hops)):
        offs[r, 1:] = np.cumsum(v)
    flat = torch.from_numpy(np.concatenate(waves)).to(dev)
    off = torch.from_numpy(offs).to(dev)
    out = torch.empty(int(offs[1, B]), dtype=torch.int16, device=dev)
    pos = torch.empty(int(offs[2, B]), dtype=torch.int32, device=dev)

    def kernel(odd=None):
        if odd is None:
            os.environ.pop("S2ST_TS_ODD", None)
        else:
            os.environ["S2ST_TS_ODD"] = odd
        rc = lib.s2st_time_scale_pcm16(flat.data_ptr(), off[0].data_ptr(), off[1].data_ptr(), B, N, D, out.data_ptr(),
                                       pos.data_ptr(), off[2].data_ptr(), C.c_void_p(bd.stream_ptr()))
        os.environ.pop("S2ST_TS_ODD", None)
        assert rc == 0, rc

    def device():
        return TS.time_scale(waves, ms, N=N, D=D, device=dev)

    H = min(args.host_utts, B)

    def host():
        return [TS.host_time_scale(waves[b], ms[b], N, D) for b in range(H)]

    h = host()
    d = device()
    for b in range(H):  # the forms agree before they are timed
        assert np.array_equal(d[b][0], h[b][0]) and np.array_equal(d[b][1], h[b][1]), b
    for odd in ("funnel", "image"):
        out.zero_()
        kernel(odd)
        torch.cuda.synchronize()
        o, p = out.cpu().numpy(), pos.cpu().numpy()
        for b in range(B):
            assert np.array_equal(o[offs[1, b]:offs[1, b + 1]], d[b][0]) and np.array_equal(p[offs[2, b]:offs[2, b + 1]], d[b][1]), (odd, b)
    total_s = sum(lens) / RATE
    say(f"# {B} recordings at {RATE} Hz, {min(lens) / RATE:.2f} .. {max(lens) / RATE:.2f} s, {total_s:.1f} s in all, each compressed "
        f"by {tm / 1000:g}; N = {N}, D = {D}: {2 * D + 1} candidates of {Hs} terms per hop, {sum(hops)} hops in all, {max(hops)} in "
        f"the longest recording")
    forms = (("device, the kernel alone (as launched)", kernel), ("device, the kernel alone, odd offsets: funnel", lambda: kernel("funnel")),
             ("device, the kernel alone, odd offsets: image", lambda: kernel("image")),
             ("device, time_scale() with upload and read-back", device), (f"host (numpy), {H} recordings, scaled to the batch", host))
    times = {name: [] for name, _ in forms}
    for _ in range(3):  # (warm: code objects, allocator)
        kernel("funnel"), kernel("image"), kernel()
    device()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for name, fn in forms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
    scale = {forms[-1][0]: sum(lens) / max(sum(lens[:H]), 1)}
    say(f"{'form':<52} {'ms per batch: median [min .. max]':>36} {'x real time':>14}")
    med = {}
    for name, _ in forms:
        t = np.array(times[name]) * scale.get(name, 1.0)
        med[name] = float(np.median(t))
        say(f"{name:<52} {np.median(t):16.3f} [{t.min():.3f} .. {t.max():.3f}] {total_s / (np.median(t) / 1e3):14.0f}")
    tk, tf, ti, td, th = (med[name] for name, _ in forms)
    say(f"# host / device end to end: {th / td:.1f}x; host / kernel alone: {th / tk:.1f}x; the kernel is {tk / td * 100:.0f}% of the "
        f"end-to-end device time")
    say(f"# odd offsets, funnel against image: {tf:.3f} ms against {ti:.3f} ms per batch (ranges above)")
    # the kernel's own time: the library's per-dispatch events (s2st_profile_report: tag, launches, total us)
    for odd in ("funnel", "image"):
        lib.s2st_profile_enable(1)
        for _ in range(args.rounds):
            kernel(odd)
        torch.cuda.synchronize()
        rep = C.create_string_buffer(1 << 16)
        n = int(lib.s2st_profile_report(rep, len(rep)))
        lib.s2st_profile_enable(0)
        for row in rep.raw[:max(n, 0)].decode().splitlines():
            f = row.split("\t")
            if len(f) >= 3 and f[0].startswith("ts_"):
                us = float(f[2]) / max(int(f[1]), 1)
                terms = (2 * D + 1) * Hs
                say(f"# {f[0]} ({odd}): {us:.1f} us per launch (mean of {f[1]}) = {us * 1e3 / max(hops):.0f} ns per hop of the longest "
                    f"recording = {us * 1e3 / max(hops) / terms * 1e3:.2f} ps per term of a cost ({terms} terms per hop)")
    # what a hop costs besides its candidates: the same batch and frame at other search radii (the kernel as launched)
    say(f"# the kernel alone at other radii (N = {N}): us per hop of the longest recording, median [min .. max]")
    per_hop = {}
    for Dx in (0, D // 2, D, 2 * D):
        def at_radius():
            rc = lib.s2st_time_scale_pcm16(flat.data_ptr(), off[0].data_ptr(), off[1].data_ptr(), B, N, Dx, out.data_ptr(),
                                           pos.data_ptr(), off[2].data_ptr(), C.c_void_p(bd.stream_ptr()))
            assert rc == 0, rc
        at_radius()
        t = []
        for _ in range(args.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            at_radius()
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t0) * 1e6 / max(hops))
        per_hop[Dx] = float(np.median(t))
        say(f"#   D = {Dx:4d} ({2 * Dx + 1:4d} candidates): {np.median(t):7.2f} [{min(t):.2f} .. {max(t):.2f}]")
    slope = (per_hop[2 * D] - per_hop[D]) / (2 * D)  # us per candidate
    say(f"# from D to 2 D a candidate of {Hs} terms adds {slope * 1e3:.1f} ns to a hop; at D = {D} the candidates then account for "
        f"{slope * (2 * D + 1):.2f} us of the hop's {per_hop[D]:.2f} us, the rest is the hop's serial chain (barriers, the arg-min, "
        f"the blend, the region's commit)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
