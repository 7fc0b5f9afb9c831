"""Frozen HuBERT front end of config 4 (``--use-hubert true``) on the HIP path.

Mirrors what the reference calls on it: ``HubertModel.extract_features(source, padding_mask)``
-> ``(features [B, T', E], frame padding mask [B, T'])`` in eval mode with ``mask=False``
(fairseq/models/hubert/hubert.py:518-534, called from
examples/s2s_trans/models/s2st_transformer.py:245-252).  ``state_dict`` keys / shapes are the
reference ``HubertModel``'s for every tensor the forward reads; the pre-training-only tensors
(``mask_emb``, ``final_proj.*``, ``label_embs_concat``) are accepted and ignored by
``load_state_dict``.  All arithmetic runs in libs2st_hip.so (``s2st_hubert_*``); torch holds the
arenas.  The engine keeps conv weights in GEMM layout and the weight-normed positional conv as
its effective weight, so loading converts layouts (data movement only, done once: the module is
frozen).
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

from ..runtime import binding as bd
from .speech_encoder import DEFAULT_CONV as BASE_CONV, SpeechEncoder

POS_W = "encoder.pos_conv.0.weight"


class HubertFrontend(SpeechEncoder):
    """hubert_base geometry by default (conv stack 7 layers, 12 x 768, 12 heads, ffn 3072, conv_pos 128/16)."""
    kind = "hubert"
    CONV_W = ("feature_extractor.conv_layers.", ".0.weight")
    POS_W = POS_W
    LABEL = "HuBERT"

    def __init__(self, device: torch.device, conv=None, embed=768, layers=12, heads=12, ffn=3072, conv_pos=128,
                 conv_pos_groups=16, precise: bool = False):
        self._create_encoder(device, conv or BASE_CONV, embed, layers, heads, ffn, conv_pos, conv_pos_groups, precise)
        self._extra: Dict[str, torch.Tensor] = {}  # reference tensors the forward does not read

    # -- parameters: reference names / layouts <-> engine arena ------------------------------------
    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = True):
        need = self._needed(sd, strict)
        self._copy_in(sd)
        for k in (POS_W + "_g", POS_W + "_v"):  # (the engine keeps only the folded weight: state_dict() hands these back)
            self._extra[k] = sd[k].to(self.device, torch.float32).clone()
        for k, v in sd.items():
            if k not in need:
                self._extra[k] = v.detach().clone()

    def state_dict(self) -> Dict[str, torch.Tensor]:
        out: Dict[str, torch.Tensor] = {}
        for n, _, _, shape in self.infos:
            if n == POS_W:
                continue
            v = self._view(n)
            if self._is_conv_w(n):
                v = v.permute(0, 2, 1).contiguous()
            out[n] = v.clone()
        out.update({k: v.clone() for k, v in self._extra.items()})
        return out

    # -- forward --------------------------------------------------------------------------------------
    def _to_device_async(self, t: torch.Tensor) -> torch.Tensor:
        """Small host tensor -> device without stalling the queue: a pageable H2D copy synchronises with
        everything already enqueued, and a fresh pin_memory() per call makes the caching host allocator
        grow (its blocks are still in flight).  A ring of reusable pinned staging buffers, each guarded by
        the event of its last copy, does neither."""
        if self.device.type != "cuda":
            return t
        ring = self.__dict__.setdefault("_pin_ring", {})
        key = (t.dtype, tuple(t.shape))
        slots = ring.setdefault(key, {"i": 0, "bufs": []})
        if len(slots["bufs"]) < 8:
            slots["bufs"].append([torch.empty(t.shape, dtype=t.dtype).pin_memory(), None])
            buf = slots["bufs"][-1]
        else:
            buf = slots["bufs"][slots["i"] % 8]
            slots["i"] += 1
            if buf[1] is not None:
                buf[1].synchronize()  # only waits if 8 later copies are still behind this one
        buf[0].copy_(t)
        out = buf[0].to(self.device, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        buf[1] = ev
        return out

    @staticmethod
    def frame_padding_mask(padding_mask: torch.Tensor, n_frames: int) -> torch.Tensor:
        """hubert.py:400-410: a frame is padding iff all samples of its chunk are."""
        extra = padding_mask.size(1) % n_frames
        if extra > 0:
            padding_mask = padding_mask[:, :-extra]
        return padding_mask.view(padding_mask.size(0), n_frames, -1).all(-1)

    @staticmethod
    def _suffix_frame_mask(padding_mask: torch.Tensor, n_frames: int):
        """``frame_padding_mask`` for the masks a collater produces (padding = a suffix of every row) without the
        [B][T][chunk] boolean reduction over millions of samples (20 - 50 ms per 24 x 8 s batch on the host: it made the
        host-fed --use-hubert step twice as long as the device-resident one): with n_b valid samples, frame f's chunk
        [f c, (f + 1) c) is all padding iff f c >= n_b.  None when some row's padding is not a suffix."""
        import numpy as np
        pm = padding_mask.detach().cpu().numpy()
        B, N = pm.shape
        chunk = (N - N % n_frames) // n_frames
        if chunk <= 0 or pm.dtype != np.bool_:
            return None
        n_pad = np.count_nonzero(pm, axis=1)
        first = np.where(n_pad > 0, pm.argmax(axis=1), N)
        if not np.array_equal(first + n_pad, np.full(B, N)):
            return None
        pad_from = -(-first // chunk)  # ceil(n_b / chunk)
        return torch.from_numpy(np.arange(n_frames)[None, :] >= pad_from[:, None])

    def stage(self, source: torch.Tensor, padding_mask: Optional[torch.Tensor] = None):
        """Host side of a call, done once per batch: upload the waveform, turn the sample-level padding mask into
        frame counts (hubert.py:400-410).  Returns ``(wave_dev, frame_lens_dev int32, frame_pad_mask_host, T)``;
        ``self.last_frame_lens`` holds the host copy of the frame counts."""
        wave = source.to(self.device, torch.float32).contiguous()
        bd.require_device(wave)
        B, N = wave.shape
        T = self.out_frames(N)
        if T <= 0:
            raise ValueError(f"{N} samples are shorter than the conv stack's receptive field")
        if padding_mask is None:
            padding_mask = torch.zeros(B, N, dtype=torch.bool)
        fpm = self._suffix_frame_mask(padding_mask, T)
        if fpm is None:  # (not a suffix mask at the sample level: the general reduction decides)
            fpm = self.frame_padding_mask(padding_mask.cpu(), T)
        if not bool(((~fpm).long().cumsum(1)[:, -1:] == (~fpm).long().sum(1, keepdim=True)).all()) or \
                bool((fpm[:, :-1] & ~fpm[:, 1:]).any()):
            raise ValueError("padding must be a suffix of every utterance")
        self.last_frame_lens = (~fpm).sum(1).long()  # host copy: the encoder's length / position bookkeeping
        lens = self._to_device_async(self.last_frame_lens.to(torch.int32))
        return wave, lens, fpm, T

    def forward_into(self, wave: torch.Tensor, lens: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
        """Device side: the frozen forward of staged inputs into ``out`` [B, T, embed] (no host work besides the
        enqueue: what a training step repeats on a prepared batch)."""
        B, N = wave.shape
        self._reserve(B, N)
        self._forward(wave.data_ptr(), lens.data_ptr(), B, N, out.data_ptr())
        self._keep = (wave, lens)
        return out

    def reserve(self, B: int, N: int):
        """Size the workspace for a [B, N] waveform batch up front (no allocation inside a training loop)."""
        self._reserve(B, N)

    def extract_features(self, source: torch.Tensor, padding_mask: Optional[torch.Tensor] = None,
                         mask: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
        if mask:
            raise NotImplementedError("the frozen front end runs with mask=False (s2st_transformer.py:248)")
        wave, lens, fpm, T = self.stage(source, padding_mask)
        out = torch.empty(wave.shape[0], T, self.embed, dtype=torch.float32, device=self.device)
        self.forward_into(wave, lens, out)
        return out, self._to_device_async(fpm)
