"""HiFi-GAN test geometry, seeded synthetic weights and inputs, and a float64 restatement of the generator.

Shared by tests/test_hifigan.py and tools/gen_golden_hifigan.py (which runs the reference's own Generator on what this
module makes and writes tests/golden/hifigan.npz).

Weight recipe (documented, CPU, deterministic): the tensors of the reference's state_dict are enumerated in its order
(``state_dict_shapes``); tensor number i is drawn from ``torch.Generator().manual_seed(SEED0 + i)``:
``weight_v ~ N(0, 1)``, ``weight_g ~ U(0.5, 1.5)`` (so g != ||v||: the fold is exercised), ``bias ~ N(0, 0.1^2)``.
The reference's own init (std 0.01) would give a near-silent wave; this one gives a wave of std ~0.1 - 0.9.

The restatement is written from the architecture (conv_pre 7 taps; per stage leaky_relu(0.1) -> ConvTranspose1d(k, u,
padding (k - u) // 2) -> mean over the ResBlocks of x + c2(lrelu(c1(lrelu(x)))) three times with c1 dilated;
leaky_relu(0.01) -> conv_post 7 taps -> tanh), in float64 with F.conv1d / F.conv_transpose1d.
"""
from typing import Dict, List, Tuple

import torch
import torch.nn.functional as F

SEED0 = 7000

TINY = {"upsample_initial_channel": 32, "upsample_rates": [2, 3], "upsample_kernel_sizes": [5, 7],
        "resblock_kernel_sizes": [3, 5], "resblock_dilation_sizes": [[1, 3, 5], [1, 2, 4]], "resblock": "1"}
V1 = {"upsample_initial_channel": 512, "upsample_rates": [8, 8, 2, 2], "upsample_kernel_sizes": [16, 16, 4, 4],
      "resblock_kernel_sizes": [3, 7, 11], "resblock_dilation_sizes": [[1, 3, 5]] * 3, "resblock": "1"}
HOP300 = {"upsample_initial_channel": 256, "upsample_rates": [5, 5, 4, 3], "upsample_kernel_sizes": [11, 11, 8, 7],
          "resblock_kernel_sizes": [3, 7, 11], "resblock_dilation_sizes": [[1, 3, 5]] * 3, "resblock": "1"}
CONFIGS = {"tiny": TINY, "v1": V1, "hop300": HOP300}
# mel lengths per geometry (one at a time through the reference): a 1-frame utterance, and sample counts on 128-row edges
LENGTHS = {"tiny": [1, 7, 21], "v1": [1, 4, 9], "hop300": [1, 32]}


def state_dict_shapes(cfg) -> List[Tuple[str, Tuple[int, ...]]]:
    """(name, shape) of the reference Generator's state_dict with weight norm, in its order."""
    out: List[Tuple[str, Tuple[int, ...]]] = []
    C0 = cfg["upsample_initial_channel"]

    def conv(name, cout, cin, k):
        out.extend([(name + ".bias", (cout,)), (name + ".weight_g", (cout, 1, 1)), (name + ".weight_v", (cout, cin, k))])

    conv("conv_pre", C0, 80, 7)
    for i, (u, k) in enumerate(zip(cfg["upsample_rates"], cfg["upsample_kernel_sizes"])):
        cin, cout = C0 >> i, C0 >> (i + 1)
        out.extend([(f"ups.{i}.bias", (cout,)), (f"ups.{i}.weight_g", (cin, 1, 1)), (f"ups.{i}.weight_v", (cin, cout, k))])
    nk = len(cfg["resblock_kernel_sizes"])
    for i in range(len(cfg["upsample_rates"])):
        ch = C0 >> (i + 1)
        for j, k in enumerate(cfg["resblock_kernel_sizes"]):
            for which in ("convs1", "convs2"):
                for l in range(3):
                    conv(f"resblocks.{i * nk + j}.{which}.{l}", ch, ch, k)
    conv("conv_post", 1, C0 >> len(cfg["upsample_rates"]), 7)
    return out


def synth_state(cfg) -> Dict[str, torch.Tensor]:
    sd: Dict[str, torch.Tensor] = {}
    for i, (name, shape) in enumerate(state_dict_shapes(cfg)):
        g = torch.Generator().manual_seed(SEED0 + i)
        if name.endswith("weight_v"):
            sd[name] = torch.randn(shape, generator=g)
        elif name.endswith("weight_g"):
            sd[name] = 0.5 + torch.rand(shape, generator=g)
        else:
            sd[name] = 0.1 * torch.randn(shape, generator=g)
    return sd


def synth_mel(T: int, seed: int) -> torch.Tensor:
    """[T, 80] log-mel-like input: a smooth random field around -4 (std ~1.5)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(1, 80, T + 4, generator=g)
    x = F.avg_pool1d(x, 5, 1)[0]  # smooth along time
    return (-4.0 + 3.0 * x).t().contiguous()


def fold(g: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    return g * v / v.pow(2).sum(dim=tuple(range(1, v.dim())), keepdim=True).sqrt()


def effective(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    out = {}
    for k, v in sd.items():
        if k.endswith("weight_v"):
            out[k[:-2]] = fold(sd[k[:-1] + "g"].double(), v.double())
        elif not k.endswith("weight_g"):
            out[k] = v.double()
    return out


def restated_forward(sd: Dict[str, torch.Tensor], cfg, mel: torch.Tensor) -> torch.Tensor:
    """float64 generator on one utterance: mel [T, 80] -> wave [N]."""
    w = effective(sd)
    x = F.conv1d(mel.double().t().unsqueeze(0), w["conv_pre.weight"], w["conv_pre.bias"], padding=3)
    nk = len(cfg["resblock_kernel_sizes"])
    for i, (u, k) in enumerate(zip(cfg["upsample_rates"], cfg["upsample_kernel_sizes"])):
        x = F.conv_transpose1d(F.leaky_relu(x, 0.1), w[f"ups.{i}.weight"], w[f"ups.{i}.bias"], stride=u,
                               padding=(k - u) // 2)
        xs = None
        for j, (kr, dil) in enumerate(zip(cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"])):
            y = x
            for l in range(3):
                p = f"resblocks.{i * nk + j}"
                t = F.conv1d(F.leaky_relu(y, 0.1), w[f"{p}.convs1.{l}.weight"], w[f"{p}.convs1.{l}.bias"],
                             dilation=dil[l], padding=(kr * dil[l] - dil[l]) // 2)
                t = F.conv1d(F.leaky_relu(t, 0.1), w[f"{p}.convs2.{l}.weight"], w[f"{p}.convs2.{l}.bias"],
                             padding=(kr - 1) // 2)
                y = t + y
            xs = y if xs is None else xs + y
        x = xs / nk
    x = F.conv1d(F.leaky_relu(x, 0.01), w["conv_post.weight"], w["conv_post.bias"], padding=3)
    return torch.tanh(x)[0, 0]
