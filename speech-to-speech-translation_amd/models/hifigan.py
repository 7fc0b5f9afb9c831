"""HiFi-GAN vocoder (``--vocoder hifigan``) on the HIP path.

Mirrors the reference's ``HiFiGANVocoder`` (fairseq/models/text_to_speech/vocoder.py:161-186) around its ``Generator``
(fairseq/models/text_to_speech/hifigan.py:109-162): ``__call__(x)`` maps a log-mel ``[T, 80]`` / ``[B, T, 80]`` to a wave
``[1, N]`` / ``[B, 1, N]``.  ``batch(xs)`` runs a ragged list in ONE forward, each utterance computed as the reference
computes it alone (zero padding at its own end), which is what ``speech_generator.py`` calls for a batch.

The checkpoint is the reference's ``{"generator": state_dict}`` with ``weight_g`` / ``weight_v`` pairs (weight norm), or
with plain ``weight`` keys as saved after ``remove_weight_norm``; missing or unexpected keys are an error, as with a
strict ``load_state_dict``.  Loading folds the weight norm on the host in fp32 (``w = g v / ||v||``, the norm over every
dim but 0: per OUTPUT channel for ``Conv1d``'s ``[C_out, C_in, k]``, per INPUT channel for ``ConvTranspose1d``'s
``[C_in, C_out, k]``) and writes the engine's layouts: ``[C_out][k][C_in]`` for the convolutions, the polyphase form of
the transposed convolutions (include/s2st_hip.h).  The engine casts its bf16 copy once per parameter version.
All arithmetic runs in libs2st_hip.so (``s2st_hifigan_*``); torch holds the arenas.
"""
from __future__ import annotations

import ctypes as C
import json
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from ..runtime import binding as bd
from ..runtime.frozen import FrozenNet


class HiFiGANConfigC(C.Structure):
    _fields_ = [("in_dim", C.c_int32), ("initial_channel", C.c_int32), ("n_ups", C.c_int32),
                ("up_rates", C.c_int32 * 8), ("up_kernels", C.c_int32 * 8), ("n_kernels", C.c_int32),
                ("rb_kernels", C.c_int32 * 4), ("rb_dilations", (C.c_int32 * 3) * 4), ("precise", C.c_int32)]


def _polyphase(w: torch.Tensor, u: int) -> torch.Tensor:
    """ConvTranspose1d weight [C_in, C_out, k] (stride u, padding (k - u) // 2) -> [u, C_out, ceil(k/u), C_in]: output
    phase r is a stride-1 correlation whose tap n reads input row q + (r + p) // u - ceil(k/u) + 1 + n with the weight
    column j = (r + p) % u + (ceil(k/u) - 1 - n) u (zero where j >= k)."""
    cin, cout, k = w.shape
    p, M = (k - u) // 2, (k + u - 1) // u
    out = torch.zeros(u, cout, M, cin, dtype=w.dtype, device=w.device)
    for r in range(u):
        j0 = (r + p) % u
        for n in range(M):
            j = j0 + (M - 1 - n) * u
            if j < k:
                out[r, :, n, :] = w[:, :, j].t()
    return out


class HiFiGANVocoder(FrozenNet):
    """``HiFiGANVocoder(checkpoint_path, model_cfg)`` as the reference's; ``precise=True`` selects the bf16x3 products
    (``--precise-gemm``), otherwise bf16 operands with fp32 accumulation."""
    kind = "hifigan"

    def __init__(self, checkpoint_path: Optional[str], model_cfg: Dict, fp16: bool = False, device=None,
                 precise: bool = False, state_dict: Optional[Dict[str, torch.Tensor]] = None):
        device = torch.device(device) if device is not None else (
            torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu"))
        self.cfg = dict(model_cfg)
        self.precise = bool(precise)
        self.ups = list(zip(self.cfg["upsample_rates"], self.cfg["upsample_kernel_sizes"]))
        self.rb_kernels = list(self.cfg["resblock_kernel_sizes"])
        self.rb_dil = [list(d) for d in self.cfg["resblock_dilation_sizes"]]
        self.c0 = int(self.cfg["upsample_initial_channel"])
        self.in_dim = int(self.cfg.get("model_in_dim", 80))
        if len(self.rb_kernels) != len(self.rb_dil) or any(len(d) != 3 for d in self.rb_dil):
            raise ValueError("resblock_kernel_sizes / resblock_dilation_sizes: one triple of dilations per kernel")
        cfg = HiFiGANConfigC()
        cfg.in_dim, cfg.initial_channel, cfg.n_ups = self.in_dim, self.c0, len(self.ups)
        for i, (u, k) in enumerate(self.ups):
            cfg.up_rates[i], cfg.up_kernels[i] = int(u), int(k)
        cfg.n_kernels = len(self.rb_kernels)
        for j, k in enumerate(self.rb_kernels):
            cfg.rb_kernels[j] = int(k)
            for l in range(3):
                cfg.rb_dilations[j][l] = int(self.rb_dil[j][l])
        cfg.precise = int(self.precise)
        self._create(device, cfg, self.precise)
        if state_dict is None and checkpoint_path is not None:
            state_dict = torch.load(checkpoint_path, map_location="cpu")["generator"]
        if state_dict is not None:
            self.load_state_dict(state_dict)

    def cuda(self):
        return self

    def cpu(self):
        return self

    @classmethod
    def from_data_cfg(cls, args, data_cfg, device=None):
        """vocoder.py:188-194: ``data_cfg.vocoder = {type: hifigan, config: <json>, checkpoint: <path>}``."""
        vocoder_cfg = _vocoder_entry(data_cfg)
        if vocoder_cfg.get("type", "griffin_lim") != "hifigan":
            raise ValueError("--vocoder hifigan needs a `vocoder: {type: hifigan, config: ..., checkpoint: ...}` entry in "
                             "the data config")
        with open(vocoder_cfg["config"]) as f:
            model_cfg = json.load(f)
        return cls(vocoder_cfg["checkpoint"], model_cfg, fp16=bool(getattr(args, "fp16", False)), device=device,
                   precise=bool(getattr(args, "precise_gemm", False)))

    # -- parameters: reference names / layouts -> engine arena ----------------------------------------
    def reference_shapes(self) -> Dict[str, Tuple[int, ...]]:
        """The effective (weight-norm folded) shape of every tensor, in the reference's layout."""
        s: Dict[str, Tuple[int, ...]] = {}
        for n, _, _, shape in self.infos:
            if n.startswith("ups.") and n.endswith(".weight"):
                i = int(n.split(".")[1])
                cin = self.c0 >> i
                s[n] = (cin, shape[1], self.ups[i][1])
            elif n.endswith(".weight"):
                s[n] = (shape[0], shape[2], shape[1])  # engine [O][k][I] <- reference [O][I][k]
            else:
                s[n] = shape
        return s

    @staticmethod
    def fold_weight_norm(g: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
        """torch.nn.utils.weight_norm(dim=0): w = g v / ||v||, the norm over every dim but 0."""
        g, v = g.float(), v.float()
        return g * v / v.pow(2).sum(dim=tuple(range(1, v.dim())), keepdim=True).sqrt()

    def effective_weights(self, sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        need = self.reference_shapes()
        out: Dict[str, torch.Tensor] = {}
        used = set()
        for n, shape in need.items():
            if n.endswith(".weight") and n not in sd and (n + "_g") in sd and (n + "_v") in sd:
                w = self.fold_weight_norm(sd[n + "_g"].detach().cpu(), sd[n + "_v"].detach().cpu())
                used.update((n + "_g", n + "_v"))
            elif n in sd:
                w = sd[n].detach().cpu().float()
                used.add(n)
            else:
                raise KeyError(f"missing HiFi-GAN tensor: {n}")
            if tuple(w.shape) != tuple(shape):
                raise ValueError(f"{n}: shape {tuple(w.shape)}, expected {tuple(shape)}")
            out[n] = w
        extra = sorted(set(sd) - used)
        if extra:
            raise KeyError(f"unexpected HiFi-GAN tensors: {extra[:5]}")
        return out

    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = True):
        eff = self.effective_weights(sd)
        for n, _, _, shape in self.infos:
            w = eff[n]
            if n.startswith("ups.") and n.endswith(".weight"):
                w = _polyphase(w, self.ups[int(n.split(".")[1])][0])
            elif n.endswith(".weight"):
                w = w.permute(0, 2, 1)
            self._view(n).copy_(w.reshape(shape).to(self.device))
        self.invalidate_bf16()

    # -- forward ------------------------------------------------------------------------------------------
    def out_samples(self, n_frames: int) -> int:
        return int(self.lib.s2st_hifigan_out_samples(self.h, int(n_frames)))

    def forward_padded(self, mel: torch.Tensor, frames: Sequence[int]) -> torch.Tensor:
        """mel [B, T, 80] (rows >= frames[b] ignored) -> wave [B, out_samples(T)], zero past each utterance's samples."""
        mel = mel.to(self.device, torch.float32).contiguous()
        bd.require_device(mel)
        B, T, D = mel.shape
        if D != self.in_dim:
            raise ValueError(f"expected {self.in_dim} mel bins, got {D}")
        if B == 0 or T == 0:
            return torch.zeros(B, self.out_samples(T), device=self.device)
        if len(frames) != B or any(not 0 <= int(f) <= T for f in frames):
            raise ValueError(f"frames must be {B} lengths in [0, {T}]")
        fr = torch.tensor([int(f) for f in frames], dtype=torch.int32)
        if self.device.type == "cuda":
            fr = fr.pin_memory().to(self.device, non_blocking=True)
        wave = torch.empty(B, self.out_samples(T), dtype=torch.float32, device=self.device)
        self._reserve(B, T)
        self._forward(mel.data_ptr(), fr.data_ptr(), B, T, wave.data_ptr())
        self._keep = (mel, fr)
        return wave

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        """vocoder.py:175-181: (B x) T x D -> (B x) 1 x N."""
        if x.dim() == 2:
            return self.forward_padded(x.unsqueeze(0), [x.shape[0]])
        return self.forward_padded(x, [x.shape[1]] * x.shape[0]).unsqueeze(1)

    forward = __call__

    def batch(self, xs: Sequence[torch.Tensor]) -> List[torch.Tensor]:
        """Ragged list of [T_u, 80] log-mels -> list of [1, N_u] waves, one launch sequence for the whole list."""
        if len(xs) == 0:
            return []
        Ts = [int(x.shape[0]) for x in xs]
        mel = torch.zeros(len(xs), max(Ts), self.in_dim, dtype=torch.float32, device=self.device)
        for u, x in enumerate(xs):
            mel[u, :Ts[u]] = x.to(self.device, torch.float32)
        wave = self.forward_padded(mel, Ts)
        return [wave[u:u + 1, :self.out_samples(T)] for u, T in enumerate(Ts)]


def _vocoder_entry(data_cfg) -> Dict:
    if data_cfg is None:
        return {}
    v = getattr(data_cfg, "vocoder", None)
    if v is None:
        cfg = getattr(data_cfg, "config", data_cfg if isinstance(data_cfg, dict) else {})
        v = cfg.get("vocoder") if isinstance(cfg, dict) else None
    return dict(v or {})
