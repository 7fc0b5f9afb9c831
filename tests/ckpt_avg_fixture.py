"""The three checkpoints tests/test_average_checkpoints.py averages (and tools/gen_golden_ckpt_avg.py fed to the
reference's script): tests/golden/ckpt_nano.pt with its model tensors perturbed by a seeded generator.  The second file is
saved in half precision; all carry integer buffers (BatchNorm's ``num_batches_tracked``, set to 5, 9 and 12 here so that the
floor division shows: 26 // 3 = 8); non-model entries differ per file so that "taken from the first" can be told."""
import copy
import os

import torch

NAMES = ("checkpoint3.pt", "checkpoint4.pt", "checkpoint5.pt")
TRACKED = (5, 9, 12)


def make_inputs(golden_dir: str, out_dir: str):
    base = torch.load(os.path.join(golden_dir, "ckpt_nano.pt"), map_location="cpu", weights_only=False)
    g = torch.Generator().manual_seed(20260)
    paths = []
    os.makedirs(out_dir, exist_ok=True)
    for i, name in enumerate(NAMES):
        st = copy.deepcopy(base)
        for k, v in st["model"].items():
            if v.is_floating_point():
                w = v.float() * (1.0 + 0.1 * torch.randn(v.shape, generator=g)) + 0.01 * torch.randn(v.shape, generator=g)
                st["model"][k] = w.half() if i == 1 else w
            else:
                st["model"][k] = torch.full_like(v, TRACKED[i])
        st["extra_state"] = dict(st.get("extra_state") or {}, which_file=i)
        p = os.path.join(out_dir, name)
        torch.save(st, p)
        paths.append(p)
    return paths
