#!/usr/bin/env python3
"""Cost of the pause-seeking segmentation on the GPU against the host form (informational: the README quotes what this writes).

    python tools/segment_rate.py [--minutes 60] [--rounds 5] [--max-segment-s 30] [--min-segment-s 1] [--out profiles/segment_rate.txt]

One synthetic recording at 16 kHz (seeded): noise bursts of 2 .. 12 s and near-silence of 0.2 .. 1.5 s in turn.  Three forms,
alternated in one process for --rounds rounds, each timed with the host clock between two synchronisations:
  * the two kernels alone (s2st_segment_pcm16: samples already on the device, outputs preallocated, nothing read back);
  * ``segmentation.segment`` end to end: the upload of the int16 samples, the kernels, the read-back of the segments;
  * ``segmentation.host_segment``: the same rules in numpy.
The forms agree before they are timed.  The parent of this feature has no segmentation, so the host form is the basis of
comparison.  Per form: median [min .. max] of the rounds.
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
RATE = 16000


def recording(minutes: float, seed: int = 7) -> np.ndarray:
    rs = np.random.RandomState(seed)
    n = int(minutes * 60 * RATE)
    x = np.empty(n, np.int16)
    at, on = 0, True
    while at < n:
        m = min(int(RATE * (rs.uniform(2.0, 12.0) if on else rs.uniform(0.2, 1.5))), n - at)
        a = 8000 if on else 6
        x[at:at + m] = rs.randint(-a, a + 1, m)
        at, on = at + m, not on
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=60.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--max-segment-s", type=float, default=30.0)
    ap.add_argument("--min-segment-s", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segment_rate.txt"))
    args = ap.parse_args()
    SG = importlib.import_module(PKG + ".segmentation")
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
    say(f"# tools/segment_rate.py --minutes {args.minutes:g} --rounds {args.rounds} --max-segment-s {args.max_segment_s:g} "
        f"--min-segment-s {args.min_segment_s:g}")
    say(f"# source hash {buf.value.decode()} (tree: {ge.source_hash()}); device {torch.cuda.get_device_name(0)}")
    x = recording(args.minutes)
    min_len, max_len = int(round(args.min_segment_s * 100)), int(round(args.max_segment_s * 100))
    win, hop = SG.framing(RATE)
    T = SG.n_frames(len(x), win, hop)
    w, pad = SG.SMOOTH_FRAMES, int(round(SG.PAD_MS / 10))
    pf, sf = SG.db_factor(SG.CUT_PENALTY_DB), SG.db_factor(SG.SILENCE_DB)

    # the kernels alone
    flat = torch.from_numpy(x).to(dev)
    soff = torch.tensor([0, len(x)], dtype=torch.int64).to(dev)
    Kcap = max(1, T // min_len)
    nws = int(lib.s2st_segment_workspace(1, T, min_len))
    ws = torch.empty(nws // 8 + 1, dtype=torch.int64, device=dev)
    nseg = torch.empty(1, dtype=torch.int32, device=dev)
    out = torch.empty(5, 1, Kcap, dtype=torch.int32, device=dev)
    cost = torch.empty(1, dtype=torch.int64, device=dev)

    def kernels():
        rc = lib.s2st_segment_pcm16(flat.data_ptr(), soff.data_ptr(), 1, T, win, hop, w, min_len, max_len, pad, pf, sf, Kcap,
                                    nseg.data_ptr(), *(out[j].data_ptr() for j in range(5)), cost.data_ptr(), ws.data_ptr(), nws,
                                    C.c_void_p(bd.stream_ptr()))
        assert rc == 0, rc

    def device():
        return SG.segment([x], RATE, min_len, max_len, device=dev)[0]

    def host():
        return SG.host_segment(x, RATE, min_len, max_len)

    kernels()
    torch.cuda.synchronize()
    d, h = device(), host()
    K = int(nseg.cpu()[0])
    for f in ("start", "end", "trim_start", "trim_end", "dropped"):  # the forms agree before they are timed
        assert np.array_equal(getattr(d, f), getattr(h, f)), f
    assert d.cost == h.cost == int(cost.cpu()[0]) and K == len(h) and np.array_equal(out[0, 0, :K].cpu().numpy(), h.start)
    say(f"# one recording of {len(x) / RATE / 60:.1f} min at {RATE} Hz: {len(x)} samples, {T} frames; segments of {min_len} .. "
        f"{max_len} frames, w = {w}, pad = {pad}: {K} segments ({int(h.dropped.sum())} dropped), longest "
        f"{int((h.end - h.start).max())} frames, trimmed speech {int((h.trim_end - h.trim_start).sum())} frames; workspace "
        f"{nws / 2**20:.1f} MiB")
    forms = (("device, the two kernels alone", kernels), ("device, segment() with upload and read-back", device),
             ("host (numpy)", host))
    times = {name: [] for name, _ in forms}
    for _ in range(args.rounds):
        for name, fn in forms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
    say(f"{'form':<46} {'ms per recording: median [min .. max]':>40} {'x real time':>14}")
    for name, _ in forms:
        t = np.array(times[name])
        say(f"{name:<46} {np.median(t):18.2f} [{t.min():.2f} .. {t.max():.2f}] {len(x) / RATE / (np.median(t) / 1e3):14.0f}")
    tk, td, th = (np.median(times[name]) for name, _ in forms)
    say(f"# host / device end to end: {th / td:.1f}x; host / kernels alone: {th / tk:.1f}x; the kernels are {tk / td * 100:.0f}% of "
        f"the end-to-end device time")
    # the two kernels apart: the library's own per-dispatch events (s2st_profile_report: tag, launches, total us)
    lib.s2st_profile_enable(1)
    for _ in range(args.rounds):
        kernels()
    torch.cuda.synchronize()
    rep = C.create_string_buffer(1 << 16)
    n = int(lib.s2st_profile_report(rep, len(rep)))
    lib.s2st_profile_enable(0)
    for row in (rep.raw[:max(n, 0)].decode().splitlines()):
        f = row.split("\t")
        if len(f) >= 3 and f[0].startswith("seg_"):
            us = float(f[2]) / max(int(f[1]), 1)
            extra = f" = {us * 1e3 / (T / min_len):.0f} ns per step of {min_len} frames" if "search" in f[0] else ""
            say(f"# {f[0]}: {us:.1f} us per launch (mean of {f[1]}){extra}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
