#!/usr/bin/env python3
"""Golden vectors of the HiFi-GAN vocoder from the REFERENCE's own Generator, on the CPU:

    python tools/gen_golden_hifigan.py --reference <checkout of the reference fairseq fork>

writes tests/golden/hifigan.npz.  TEST INFRASTRUCTURE: the reference's fairseq/models/text_to_speech/hifigan.py is loaded
from the given checkout (it imports torch only), built for three geometries (tests/hifigan_synth.py: tiny, V1, hop 300),
loaded with the seeded synthetic weight-norm state of hifigan_synth.synth_state, and run one utterance at a time, in fp32
and under torch.autocast("cpu", dtype=torch.bfloat16) (the fast-mode bound is derived from the difference).
Stored per geometry: the mel inputs' seeds and lengths, the fp32 and autocast waves; for tiny the whole state_dict, for V1
and hop 300 each tensor's float64 sum and first values (the test regenerates the tensors and fails if they differ).
Asserted here: the float64 restatement of hifigan_synth equals the reference, and the wave is not trivial
(std 0.1 - 0.9, under 5 % of the samples with |y| > 0.99)."""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hifigan_synth as HS  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "hifigan.npz")


def load_reference(ref_root):
    path = os.path.join(ref_root, "fairseq", "models", "text_to_speech", "hifigan.py")
    spec = importlib.util.spec_from_file_location("ref_hifigan", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference fairseq checkout")
    args = ap.parse_args()
    ref = load_reference(args.reference)
    torch.manual_seed(0)
    rec = {}
    for name, cfg in HS.CONFIGS.items():
        gen = ref.Generator(cfg).eval()
        sd = HS.synth_state(cfg)
        gen.load_state_dict(sd, strict=True)
        assert [k for k in gen.state_dict()] == [k for k, _ in HS.state_dict_shapes(cfg)], name
        lens = HS.LENGTHS[name]
        rec[f"{name}.lengths"] = np.array(lens, np.int32)
        for u, T in enumerate(lens):
            seed = 100 * (u + 1) + T
            mel = HS.synth_mel(T, seed)
            with torch.no_grad():
                y = gen(mel.t().unsqueeze(0))[0, 0]
                with torch.autocast("cpu", dtype=torch.bfloat16):
                    ya = gen(mel.t().unsqueeze(0))[0, 0].float()
            y64 = HS.restated_forward(sd, cfg, mel)
            err = float((y64 - y.double()).abs().max())
            std, sat = float(y.std()), float((y.abs() > 0.99).float().mean())
            print(f"{name} T={T}: N={y.numel()} std {std:.3f} |y|>0.99 {100 * sat:.2f}% restatement err {err:.2e} "
                  f"autocast err {float((ya - y).abs().max()):.3e}")
            assert err < 1e-4, (name, T, err)
            if T > 1:
                assert 0.1 <= std <= 0.9 and sat < 0.05, (name, T, std, sat)
            rec[f"{name}.{u}.seed"] = np.int64(seed)
            rec[f"{name}.{u}.wave"] = y.numpy().astype(np.float32)
            rec[f"{name}.{u}.wave_autocast"] = ya.numpy().astype(np.float32)
        if name == "tiny":
            for k, v in sd.items():
                rec[f"tiny.sd.{k}"] = v.numpy()
        else:
            rec[f"{name}.sd_sums"] = np.array([float(v.double().sum()) for v in sd.values()])
            rec[f"{name}.sd_first"] = np.stack([np.pad(v.flatten()[:4].double().numpy(), (0, 4 - min(4, v.numel())),
                                                       constant_values=np.nan) for v in sd.values()])
    np.savez_compressed(OUT, **rec)
    print(f"wrote {OUT} ({os.path.getsize(OUT) / 1e6:.2f} MB)")


if __name__ == "__main__":
    main()
