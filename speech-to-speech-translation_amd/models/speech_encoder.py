"""What the two frozen wav2vec 2.0-family encoders share on the host: the HuBERT front end (models/hubert.py) and the
wav2vec 2.0 CTC recogniser (models/wav2vec2_ctc.py) are one architecture in the engine (csrc/engine_speech_encoder.cpp), so
they are one geometry, one table of reference shapes, one loader core and one frame count here.  A subclass names its
convolution weights (``CONV_W``) and its positional convolution's weight (``POS_W``) and keeps what is its own.

The engine stores conv weights in GEMM layout ``[O][k][I]`` and the weight-normed positional convolution as its effective
weight ``[G][E/G][k][E/G]``; loading converts from the reference layouts (data movement and a one-off fold: the modules
are frozen).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Tuple

import torch

from ..runtime.frozen import FrozenNet

# the feature extractor of hubert_base and of wav2vec2-large alike: (channels, kernel, stride) per layer
DEFAULT_CONV = [(512, 10, 5)] + [(512, 3, 2)] * 4 + [(512, 2, 2)] * 2


class SpeechEncoderConfigC(C.Structure):
    """s2st_w2v_ctc_config; s2st_hubert_config is its prefix (everything but ``vocab``)."""
    _fields_ = [("n_conv", C.c_int32), ("conv_dim", C.c_int32 * 8), ("conv_k", C.c_int32 * 8),
                ("conv_stride", C.c_int32 * 8)] + [(n, C.c_int32) for n in (
                    "embed", "layers", "heads", "ffn", "conv_pos", "conv_pos_groups", "precise", "vocab")]


class SpeechEncoder(FrozenNet):
    CONV_W: Tuple[str, str] = ("", "")  # (prefix, suffix) of the engine's names of the conv stack's weights
    POS_W = ""                          # the engine's name of the positional convolution's effective weight
    LABEL = ""                          # the model's name in error messages

    def _create_encoder(self, device: torch.device, conv, embed, layers, heads, ffn, conv_pos, conv_pos_groups, precise,
                        vocab=0):
        self.conv = [tuple(int(v) for v in c) for c in (conv or DEFAULT_CONV)]
        self.embed, self.layers, self.heads, self.ffn = embed, layers, heads, ffn
        self.conv_pos, self.groups, self.vocab, self.precise = conv_pos, conv_pos_groups, vocab, bool(precise)
        cfg = SpeechEncoderConfigC()
        cfg.n_conv = len(self.conv)
        for i, (c, k, s) in enumerate(self.conv):
            cfg.conv_dim[i], cfg.conv_k[i], cfg.conv_stride[i] = c, k, s
        cfg.embed, cfg.layers, cfg.heads, cfg.ffn = embed, layers, heads, ffn
        cfg.conv_pos, cfg.conv_pos_groups, cfg.precise, cfg.vocab = conv_pos, conv_pos_groups, int(self.precise), vocab
        self._create(device, cfg, self.precise)

    # -- parameters: reference names / layouts <-> engine arena ------------------------------------------------------
    def _is_conv_w(self, name: str) -> bool:
        return name.startswith(self.CONV_W[0]) and name.endswith(self.CONV_W[1])

    def reference_shapes(self) -> Dict[str, Tuple[int, ...]]:
        s: Dict[str, Tuple[int, ...]] = {}
        for n, _, _, shape in self.infos:
            if self._is_conv_w(n):
                s[n] = (shape[0], shape[2], shape[1])  # engine [O][k][I] <- reference [O][I][k]
            elif n == self.POS_W:
                s[n + "_g"] = (1, 1, self.conv_pos)
                s[n + "_v"] = (self.embed, self.embed // self.groups, self.conv_pos)
            else:
                s[n] = shape
        return s

    def _needed(self, sd: Dict[str, torch.Tensor], strict: bool) -> Dict[str, Tuple[int, ...]]:
        need = self.reference_shapes()
        missing = [k for k in need if k not in sd]
        if missing and strict:
            raise KeyError(f"missing {self.LABEL} tensors: {missing[:5]}")
        return need

    def _copy_in(self, sd: Dict[str, torch.Tensor]):
        dev = self.device
        for n, _, _, shape in self.infos:
            if n == self.POS_W:
                g = sd[n + "_g"].to(dev, torch.float32)
                v = sd[n + "_v"].to(dev, torch.float32)
                # nn.utils.weight_norm(dim=2): w[:, :, k] = g[k] * v[:, :, k] / ||v[:, :, k]||_F (wav2vec2.py:836).
                # A one-off host-side parameter fold of a frozen module.
                w = g * v / v.pow(2).sum(dim=(0, 1), keepdim=True).sqrt()
                G, Eg = self.groups, self.embed // self.groups
                self._view(n).copy_(w.view(G, Eg, Eg, self.conv_pos).permute(0, 1, 3, 2))
            elif self._is_conv_w(n):
                self._view(n).copy_(sd[n].to(dev, torch.float32).permute(0, 2, 1))
            else:
                self._view(n).copy_(sd[n].to(dev, torch.float32).view(shape))
        self.invalidate_bf16()  # (explicit: the copies above also bump torch's version counter)

    # -- geometry ------------------------------------------------------------------------------------------------------
    def out_frames(self, n_samples: int) -> int:
        """Frames of n samples: floor((n - k) / s) + 1 layer by layer (0 when too short), as ``s2st_<kind>_out_frames``."""
        n = int(n_samples)
        for _, k, s in self.conv:
            n = 0 if n < k else (n - k) // s + 1
        return n
