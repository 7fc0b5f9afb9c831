"""Base of the frozen engine-backed networks (the HuBERT front end, the HiFi-GAN vocoder, the wav2vec 2.0 CTC recogniser).

One engine handle made by ``s2st_<kind>_create``, the fp32 parameter arena (and its bf16 copy in fast mode) held by torch,
a per-geometry workspace plan, and the forward call with the bf16 freshness protocol.  Subclasses add their reference
names and layouts, host-side staging and ``reserve``.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Tuple

import torch

from . import binding as bd
from .engine import ParamInfo


class FrozenNet:
    kind = ""  # the C ABI's prefix: s2st_<kind>_create / _workspace_floats / _forward

    def _create(self, device: torch.device, cfg: C.Structure, precise: bool):
        self.device = device
        lib = self.lib = bd.lib()
        h = C.c_void_p()
        bd.check(getattr(lib, f"s2st_{self.kind}_create")(C.byref(cfg), C.byref(h)), f"s2st_{self.kind}_create")
        self.h = h
        self.n_params = int(lib.s2st_engine_param_floats(h))
        self.infos: List[Tuple[str, int, int, Tuple[int, ...]]] = []
        for i in range(lib.s2st_engine_num_params(h)):
            pi = ParamInfo()
            bd.check(lib.s2st_engine_param_info(h, i, C.byref(pi)), "param_info")
            self.infos.append((pi.name.decode(), int(pi.offset), int(pi.numel), tuple(pi.shape[:pi.ndim])))
        self.params = torch.zeros(self.n_params, dtype=torch.float32, device=device)
        lib.s2st_engine_bind(h, self.params.data_ptr(), None, None)
        self.params_bf16 = None
        if not precise:
            self.params_bf16 = torch.zeros(self.n_params, dtype=torch.bfloat16, device=device)
            lib.s2st_engine_bind_bf16(h, self.params_bf16.data_ptr())
        self.workspace: Optional[torch.Tensor] = None
        self._plan: Dict[Tuple[int, int], int] = {}
        self._ph_version = None
        self._ph_event = self._ph_stream = None

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.lib.s2st_engine_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def eval(self):  # (the reference calls hubert.eval() every forward: s2st_transformer.py:246)
        return self

    def _view(self, name):
        for n, off, numel, shape in self.infos:
            if n == name:
                return self.params[off:off + numel].view(shape)
        raise KeyError(name)

    def invalidate_bf16(self):
        """The parameters were written behind torch's version counter: the next forward refreshes the bf16 copy."""
        self._ph_version = None

    def _reserve(self, B: int, L: int):
        """Plan the workspace of a [B, L] batch (once per geometry) and grow it to fit."""
        if (B, L) not in self._plan:
            fn = f"s2st_{self.kind}_workspace_floats"
            n = int(getattr(self.lib, fn)(self.h, B, L))
            if n < 0:
                raise bd.S2STHipError(f"{fn} failed with code {n}")
            self._plan[(B, L)] = n
        need = self._plan[(B, L)]
        if self.workspace is None or self.workspace.numel() < need:
            self.workspace = torch.empty(need, dtype=torch.float32, device=self.device)

    def _forward(self, *args):
        """``s2st_<kind>_forward(h, *args, workspace, stream)`` on the current stream.
        Frozen weights: the engine's bf16 copy stays valid while nobody wrote the parameter tensor (or a view of it).
        torch's version counter sees in-place ops on the tensor and its views; writers that bypass it (``.data``, raw
        pointers: a C-side load, broadcast_ on a .data view) call invalidate_bf16().  The cast of the last refresh ran on
        ONE stream: a forward on another stream waits for that cast's event before it reads the copy."""
        cur = torch.cuda.current_stream() if self.device.type == "cuda" else None
        refreshed = self._ph_version != self.params._version
        if self.params_bf16 is not None and not refreshed:
            if self._ph_event is not None and cur is not None and self._ph_stream != cur.cuda_stream:
                cur.wait_event(self._ph_event)
            self.lib.s2st_engine_bf16_is_fresh(self.h)
        self._ph_version = self.params._version
        fn = f"s2st_{self.kind}_forward"
        bd.check(getattr(self.lib, fn)(self.h, *args, self.workspace.data_ptr(), self.workspace.numel(),
                                       bd.stream_ptr()), fn)
        if refreshed and self.params_bf16 is not None and cur is not None:  # the cast was enqueued on this stream
            self._ph_event = torch.cuda.Event()
            self._ph_event.record(cur)
            self._ph_stream = cur.cuda_stream
