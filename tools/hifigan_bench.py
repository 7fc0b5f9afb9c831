#!/usr/bin/env python3
"""HiFi-GAN vocoder timing on the GPU: the HIP generator (s2st_hifigan_*) against the same generator written with torch
F.conv1d / F.conv_transpose1d in fp32 and in bf16, on HiFi-GAN V1 and on the hop-300 geometry, at infer_base's batch
(64 utterances; every utterance decodes the batch's teacher length, eos threshold 2.0, 4 mel frames per step).

    python tools/hifigan_bench.py [--iters 10] [--out profiles/hifigan_bench.txt]

Per stage (conv_pre, stage i = ups[i] + its ResBlocks, conv_post) and implementation: time, TFLOP/s, an estimate of the
HBM bytes (every conv reads its input image once and writes its outputs once: the HIP path's bf16 images + fp32 residual
stream), and the fraction of the binding roof (2.5 PFLOP/s bf16 dense, 6.3 TB/s measured HBM).  Then end-to-end ms per
batch and utterances / s.  Weights: the seeded synthetic recipe of tests/hifigan_synth.py."""
import argparse
import importlib
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hifigan_synth as HS  # noqa: E402

PKG = "speech-to-speech-translation_amd"
PEAK_FLOPS, PEAK_BW = 2.5e15, 6.3e12


def infer_base_frames(n_utts=64):
    D = importlib.import_module(PKG + ".data.synthetic")
    corpus = D.SyntheticFisherCorpus(n_utts=n_utts, seed=1234)
    order = np.argsort(-corpus.src_n_frames, kind="stable")
    b = corpus.collate_batch(order[:n_utts].tolist())
    return 4 * int(b["target_lengths"].max())


def torch_stages(w, cfg, dtype):
    """The generator as a list of stage closures x -> x (channels-first [B, C, L])."""
    nk = len(cfg["resblock_kernel_sizes"])
    W = {k: v.to(dtype) for k, v in w.items()}
    st = [lambda x: F.conv1d(x, W["conv_pre.weight"], W["conv_pre.bias"], padding=3)]
    for i, (u, k) in enumerate(zip(cfg["upsample_rates"], cfg["upsample_kernel_sizes"])):
        def stage(x, i=i, u=u, k=k):
            x = F.conv_transpose1d(F.leaky_relu(x, 0.1), W[f"ups.{i}.weight"], W[f"ups.{i}.bias"], stride=u,
                                   padding=(k - u) // 2)
            xs = None
            for j, (kr, dil) in enumerate(zip(cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"])):
                y = x
                for l in range(3):
                    p = f"resblocks.{i * nk + j}"
                    t = F.conv1d(F.leaky_relu(y, 0.1), W[f"{p}.convs1.{l}.weight"], W[f"{p}.convs1.{l}.bias"],
                                 dilation=dil[l], padding=(kr * dil[l] - dil[l]) // 2)
                    t = F.conv1d(F.leaky_relu(t, 0.1), W[f"{p}.convs2.{l}.weight"], W[f"{p}.convs2.{l}.bias"],
                                 padding=(kr - 1) // 2)
                    y = t + y
                xs = y if xs is None else xs + y
            return xs / nk
        st.append(stage)
    st.append(lambda x: torch.tanh(F.conv1d(F.leaky_relu(x, 0.01), W["conv_post.weight"], W["conv_post.bias"], padding=3)))
    return st


def stage_cost(cfg, B, T):
    """[(name, flops, hbm bytes of the HIP path)] per stage."""
    C0, nk = cfg["upsample_initial_channel"], len(cfg["resblock_kernel_sizes"])
    out = [("conv_pre", 2.0 * B * T * C0 * 7 * 80, B * T * (80 * 4 + C0 * 2))]
    L = T
    for i, (u, k) in enumerate(zip(cfg["upsample_rates"], cfg["upsample_kernel_sizes"])):
        cin, ch = C0 >> i, C0 >> (i + 1)
        Lo = (L - 1) * u - 2 * ((k - u) // 2) + k
        fl = 2.0 * B * Lo * ch * ((k + u - 1) // u) * cin
        by = B * (L * cin * 2 + Lo * ch * 6)
        for kr in cfg["resblock_kernel_sizes"]:
            fl += 6 * 2.0 * B * Lo * ch * ch * kr
            # per layer: c1 reads an image (2 B) and writes one (2 B); c2 reads an image + the fp32 residual and writes
            # fp32 + an image; the MRF epilogue also reads / writes the fp32 sum
            by += 3 * B * Lo * ch * (2 + 2 + 2 + 4 + 4 + 2) + 2 * B * Lo * ch * 4
        out.append((f"stage{i}", fl, by))
        L = Lo
    C = C0 >> len(cfg["upsample_rates"])
    out.append(("conv_post", 2.0 * B * L * C * 7, B * L * (C * 4 + 4)))
    return out


def timed(fn, iters):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    fn()
    torch.cuda.synchronize()
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--utts", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hifigan_bench.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    bd = importlib.import_module(PKG + ".runtime.binding")
    M = importlib.import_module(PKG + ".models.hifigan")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    B = args.utts
    T = infer_base_frames(B)
    say(f"HiFi-GAN vocoder, {B} utterances x {T} mel frames (infer_base batch 0), median of {args.iters}")
    for name in ("v1", "hop300"):
        cfg = HS.CONFIGS[name]
        sd = HS.synth_state(cfg)
        mel = torch.stack([HS.synth_mel(T, 1000 + u) for u in range(B)]).to(dev)
        cost = stage_cost(cfg, B, T)
        tot_fl = sum(c[1] for c in cost)
        say(f"\n== {name}: C0 {cfg['upsample_initial_channel']}, ups {cfg['upsample_rates']} / "
            f"{cfg['upsample_kernel_sizes']}, {tot_fl / 1e12:.2f} TFLOP per batch "
            f"({tot_fl / (B * T) / 1e9:.3f} GFLOP per mel frame)")
        voc = M.HiFiGANVocoder(None, cfg, device=dev, precise=False, state_dict=sd)
        frames = [T] * B
        ms_hip = timed(lambda: voc.forward_padded(mel, frames), args.iters)
        # per-dispatch timeline of the HIP path (one forward), grouped into stages by launch order: conv_pre, then per
        # stage ups[i] + 6 convs per ResBlock, then conv_post
        import ctypes as C
        lib = bd.lib()
        lib.s2st_profile_enable(1)
        voc.forward_padded(mel, frames)
        torch.cuda.synchronize()
        buf = C.create_string_buffer(1 << 20)
        lib.s2st_profile_timeline.restype = C.c_int64
        lib.s2st_profile_timeline(buf, C.c_int64(1 << 20))
        lib.s2st_profile_enable(0)
        durs = [float(ln.split("\t")[3]) * 1e-3 for ln in buf.value.decode().splitlines() if ln.count("\t") >= 3]
        per_launch = [1] + [1 + 6 * len(cfg["resblock_kernel_sizes"])] * len(cfg["upsample_rates"]) + [1]
        hip_per, i0 = [], len(durs) - sum(per_launch)  # (the bf16 weight cast, when it ran, comes first)
        for n in per_launch:
            hip_per.append(sum(durs[i0:i0 + n]))
            i0 += n
        w = {k: v.to(dev) for k, v in HS.effective(sd).items()}
        res = {"HIP bf16": (hip_per, ms_hip)}
        for label, dt in (("torch fp32", torch.float32), ("torch bf16", torch.bfloat16)):
            st = torch_stages(w, cfg, dt)
            x0 = mel.transpose(1, 2).contiguous().to(dt)
            xs = [x0]
            with torch.no_grad():
                for f in st:
                    xs.append(f(xs[-1]))
                per = [timed(lambda f=f, x=x: f(x), args.iters) for f, x in zip(st, xs[:-1])]

                def full():
                    x = x0
                    for f in st:
                        x = f(x)
                    return x
                res[label] = (per, timed(full, args.iters))
            del xs
        say(f"{'stage':<10} {'GFLOP':>8} {'MB est':>8} | " + " | ".join(f"{k:>28}" for k in res))
        for si, (sn, fl, by) in enumerate(cost):
            row = f"{sn:<10} {fl / 1e9:8.1f} {by / 1e6:8.1f} | "
            cells = []
            for k, (per, _) in res.items():
                t = per[si] * 1e-3
                frac = max(fl / PEAK_FLOPS, by / PEAK_BW) / t
                cells.append(f"{per[si]:8.3f} ms {fl / t / 1e12:6.1f} TF/s {100 * frac:5.1f}%")
            say(row + " | ".join(f"{c:>28}" for c in cells))
        say(f"HIP: {len(durs)} kernel dispatches, {sum(durs):.2f} ms of kernel time (stage columns: dispatch sums)")
        roof = max(tot_fl / PEAK_FLOPS, sum(c[2] for c in cost) / PEAK_BW) * 1e3
        say(f"end to end: HIP bf16 {ms_hip:.2f} ms ({B / ms_hip * 1e3:.0f} utt/s, {tot_fl / ms_hip / 1e9:.1f} TF/s, "
            f"{100 * roof / ms_hip:.1f}% of the binding roof)")
        for k, (_, ms) in res.items():
            if k != "HIP bf16":
                say(f"end to end: {k} {ms:.2f} ms ({B / ms * 1e3:.0f} utt/s)")
        say(f"HIP vs torch bf16: {res['torch bf16'][1] / ms_hip:.2f}x")
        del voc
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
