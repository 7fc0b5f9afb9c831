"""ctypes binding of libs2st_hip.so (C ABI declared in include/s2st_hip.h).

The library is built in-tree by ``__graft_entry__.build()`` (hipcc, gfx950).  There is no
CPU fallback: if the shared object is missing or no HIP device is visible, the first
compute call raises.  ``load_library(path)`` with an explicit path exists so the test-suite
can load the host build made against the wave64 emulator (tests/hipemu) -- the product
never does that.
"""
from __future__ import annotations

import collections
import ctypes as C
import os
from typing import Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(os.path.dirname(_HERE), "csrc", "libs2st_hip.so")

_lib: Optional[C.CDLL] = None
_lib_is_emulator = False


class Split(C.Structure):
    _fields_ = [("ld", C.c_int64), ("bs", C.c_int64), ("per", C.c_int32), ("_pad", C.c_int32)]


class GemmOperand(C.Structure):
    _fields_ = [("p", C.c_void_p), ("kmajor", C.c_int32), ("dtype", C.c_int32), ("sp", Split),
                ("zo", C.c_int64), ("zi", C.c_int64)]


class GemmOut(C.Structure):
    _fields_ = [("p", C.c_void_p), ("sp", Split), ("zo", C.c_int64), ("zi", C.c_int64), ("h", C.c_void_p)]


class GemmEpilogue(C.Structure):
    _fields_ = [("alpha", C.c_float), ("act", C.c_int32), ("bias", C.c_void_p),
                ("drop_p", C.c_float), ("accumulate", C.c_int32), ("seed", C.c_uint64),
                ("resid", C.c_void_p), ("mask_y", C.c_void_p), ("mask_scale", C.c_float), ("colsum", C.c_void_p),
                ("colsum_part", C.c_void_p), ("bias_zo", C.c_int64)]


class GemmArgs(C.Structure):
    _fields_ = [("A", GemmOperand), ("B", GemmOperand), ("C", GemmOut), ("ep", GemmEpilogue),
                ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("batch", C.c_int32),
                ("zdiv", C.c_int32), ("precise", C.c_int32), ("splitk", C.c_int32),
                ("kchunk", C.c_int32), ("avec", C.c_int32), ("bvec", C.c_int32), ("cvec", C.c_int32),
                ("tiles_n", C.c_int32), ("ws", C.c_void_p), ("ws_floats", C.c_int64), ("slab", C.c_void_p)]


class S2STHipError(RuntimeError):
    pass


def load_library(path: Optional[str] = None, emulator: bool = False) -> C.CDLL:
    """Load the kernel library.  ``emulator=True`` is for tests only."""
    global _lib, _lib_is_emulator
    path = path or os.environ.get("S2ST_HIP_LIB") or DEFAULT_LIB
    if not os.path.exists(path):
        raise S2STHipError(
            f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'`"
            " (hipcc --offload-arch=gfx950). There is no CPU fallback.")
    _lib = C.CDLL(path)
    _lib_is_emulator = emulator
    # every entry point the library exports gets its signature from the header: struct arguments go as C.byref(...)
    for name, (ret, alist) in header_prototypes().items():
        fn = getattr(_lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = ret, [t for t, _ in alist]
    return _lib


def lib() -> C.CDLL:
    if _lib is None:
        load_library()
    return _lib


def is_emulator() -> bool:
    return _lib_is_emulator


def check(rc: int, what: str):
    if rc != 0:
        raise S2STHipError(f"{what} failed with code {rc}")


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    if t is None:
        return None
    return t.data_ptr()


def stream_ptr() -> Optional[int]:
    """Current torch HIP stream as a raw hipStream_t (None = default stream / emulator)."""
    if _lib_is_emulator or not torch.cuda.is_available():
        return None
    return torch.cuda.current_stream().cuda_stream


def require_device(t: torch.Tensor):
    if not _lib_is_emulator and not t.is_cuda:
        raise S2STHipError("s2st HIP ops need device (cuda/HIP) tensors; there is no CPU path")


def make_split(ld: int, per: int = 0, bs: int = 0) -> Split:
    return Split(ld, bs, per, 0)


def gemm(A: torch.Tensor, B: torch.Tensor, Cout: torch.Tensor, M: int, N: int, K: int, *,
         a_kmajor=True, a_ld=None, a_per=0, a_bs=0, a_zo=0, a_zi=0,
         b_kmajor=True, b_ld=None, b_per=0, b_bs=0, b_zo=0, b_zi=0,
         c_ld=None, c_per=0, c_bs=0, c_zo=0, c_zi=0,
         batch=1, zdiv=1, alpha=1.0, bias=None, act=0, drop_p=0.0, seed=0, resid=None,
         accumulate=False, precise=False, a_off=0, b_off=0, c_off=0, c_bf16=None, ws=None,
         mask_y=None, mask_scale=1.0, colsum=None, return_tile=False):
    """Raw GEMM entry (s2st_gemm_f32). Offsets are in elements.  A and B are both fp32 or both
    torch.bfloat16 tensors; ``Cout`` (fp32) may be None when only ``c_bf16`` is wanted."""
    require_device(A)
    if A.dtype != B.dtype:
        raise S2STHipError("gemm operands must have the same dtype")
    if A.dtype == torch.bfloat16:
        return _gemm_bf16(A, B, Cout, M, N, K, locals())
    g = GemmArgs()
    g.A = GemmOperand(A.data_ptr() + 4 * a_off, 1 if a_kmajor else 0, 0,
                      make_split(a_ld if a_ld is not None else (K if a_kmajor else M), a_per, a_bs),
                      a_zo, a_zi)
    g.B = GemmOperand(B.data_ptr() + 4 * b_off, 1 if b_kmajor else 0, 0,
                      make_split(b_ld if b_ld is not None else (K if b_kmajor else N), b_per, b_bs),
                      b_zo, b_zi)
    g.C = GemmOut(Cout.data_ptr() + 4 * c_off, make_split(c_ld if c_ld is not None else N, c_per, c_bs),
                  c_zo, c_zi, None)
    g.ep = GemmEpilogue(alpha, act, ptr(bias), drop_p, 1 if accumulate else 0, seed, ptr(resid), None, 1.0, None)
    g.M, g.N, g.K, g.batch, g.zdiv, g.precise = M, N, K, batch, zdiv, 1 if precise else 0
    check(lib().s2st_gemm_f32(C.byref(g), C.c_void_p(stream_ptr())), "s2st_gemm_f32")


def _gemm_bf16(A, B, Cout, M, N, K, kw):
    g = GemmArgs()
    a_ld = kw["a_ld"] if kw["a_ld"] is not None else (K if kw["a_kmajor"] else M)
    b_ld = kw["b_ld"] if kw["b_ld"] is not None else (K if kw["b_kmajor"] else N)
    g.A = GemmOperand(A.data_ptr() + 2 * kw["a_off"], 1 if kw["a_kmajor"] else 0, 1,
                      make_split(a_ld, kw["a_per"], kw["a_bs"]), kw["a_zo"], kw["a_zi"])
    g.B = GemmOperand(B.data_ptr() + 2 * kw["b_off"], 1 if kw["b_kmajor"] else 0, 1,
                      make_split(b_ld, kw["b_per"], kw["b_bs"]), kw["b_zo"], kw["b_zi"])
    h = kw["c_bf16"]
    g.C = GemmOut(Cout.data_ptr() + 4 * kw["c_off"] if Cout is not None else None,
                  make_split(kw["c_ld"] if kw["c_ld"] is not None else N, kw["c_per"], kw["c_bs"]),
                  kw["c_zo"], kw["c_zi"], h.data_ptr() + 2 * kw["c_off"] if h is not None else None)
    g.ep = GemmEpilogue(kw["alpha"], kw["act"], ptr(kw["bias"]), kw["drop_p"], 1 if kw["accumulate"] else 0,
                        kw["seed"], ptr(kw["resid"]), ptr(kw.get("mask_y")), kw.get("mask_scale", 1.0),
                        ptr(kw.get("colsum")))
    g.M, g.N, g.K, g.batch, g.zdiv, g.precise = M, N, K, kw["batch"], kw["zdiv"], 0
    if kw["ws"] is not None:
        g.ws, g.ws_floats = kw["ws"].data_ptr(), kw["ws"].numel()
    if kw.get("return_tile"):
        t = C.c_int32(0)
        check(lib().s2st_gemm_tile_f32(C.byref(g), C.byref(t), C.c_void_p(stream_ptr())), "s2st_gemm_tile_f32")
        return (t.value // 1000, t.value % 1000)
    check(lib().s2st_gemm_f32(C.byref(g), C.c_void_p(stream_ptr())), "s2st_gemm_f32")


def gemm_args_bf16(A, B, Cout, M, N, K, *, a_kmajor=True, b_kmajor=True, a_ld=None, b_ld=None, c_ld=None, bias=None,
                   act=0, resid=None, accumulate=False, c_bf16=None, alpha=1.0) -> GemmArgs:
    """One batch-1 bf16 problem for ``gemm_group`` (plain strides)."""
    g = GemmArgs()
    g.A = GemmOperand(A.data_ptr(), 1 if a_kmajor else 0, 1, make_split(a_ld or (K if a_kmajor else M)), 0, 0)
    g.B = GemmOperand(B.data_ptr(), 1 if b_kmajor else 0, 1, make_split(b_ld or (K if b_kmajor else N)), 0, 0)
    g.C = GemmOut(ptr(Cout), make_split(c_ld or N), 0, 0, ptr(c_bf16))
    g.ep = GemmEpilogue(alpha, act, ptr(bias), 0.0, 1 if accumulate else 0, 0, ptr(resid), None, 1.0, None)
    g.M, g.N, g.K, g.batch, g.zdiv, g.precise = M, N, K, 1, 1, 0
    return g


def gemm_group(problems):
    """s2st_gemm_group_f32: up to 8 bf16 problems of the same operand layouts in one persistent launch."""
    arr = (GemmArgs * len(problems))(*problems)
    check(lib().s2st_gemm_group_f32(arr, len(problems), C.c_void_p(stream_ptr())), "s2st_gemm_group_f32")


class GemmPlanInfo(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("error", "form", "bm", "bn", "splitk", "kchunk", "tiles_n", "use_slab", "vec", "cvec",
                                         "grid_x", "grid_y", "sk", "n", "total")] + \
               [("cvec_of", C.c_int32 * 8), ("tag", C.c_char * 104)]


GEMM_FORMS = ("STAGED", "RING", "W4", "P4", "PERSISTENT", "RING_256x128", "GROUP_RING", "GROUP_W4", "GROUP_PERSISTENT",
              "GROUP_PERSISTENT_256")
GemmPlan = collections.namedtuple("GemmPlan", "error form tag bm bn splitk kchunk tiles_n use_slab vec cvec grid sk n total cvec_of")


def gemm_plan(args, ncu=0, slots160=0, sk_bound=False, _info=GemmPlanInfo()) -> GemmPlan:
    """What ``gemm`` (one GemmArgs, e.g. from ``gemm_args_bf16``) or ``gemm_group`` (a list of them) would launch under the
    switches now in the environment, without launching: s2st_gemm_plan_f32.  ``ncu`` / ``slots160`` > 0 stand in for the
    device's CU count and its workgroups of the 160 x 128 4-wave form per CU (no HIP call then: a 256-CU decision can be
    asked on any host); ``error`` is the code the launch would fail with (the other fields are then None / zero)."""
    p = _info
    if isinstance(args, GemmArgs):
        rc = lib().s2st_gemm_plan_f32(C.byref(args), ncu, slots160, 1 if sk_bound else 0, C.byref(p))
    else:
        arr = (GemmArgs * len(args))(*args)
        rc = lib().s2st_gemm_group_plan_f32(arr, len(args), ncu, slots160, 1 if sk_bound else 0, C.byref(p))
    check(rc, "s2st_gemm_plan_f32")
    if p.error:
        return GemmPlan(p.error, None, None, 0, 0, 0, 0, 0, False, False, 0, (0, 0), False, 0, 0, ())
    return GemmPlan(0, GEMM_FORMS[p.form], p.tag.decode(), p.bm, p.bn, p.splitk, p.kchunk, p.tiles_n, bool(p.use_slab), bool(p.vec),
                    p.cvec, (p.grid_x, p.grid_y), bool(p.sk), p.n, p.total, tuple(p.cvec_of[:p.n]))


class AttnArgs(C.Structure):
    _fields_ = [("q", C.c_void_p), ("k", C.c_void_p), ("v", C.c_void_p), ("ldq", C.c_int64), ("ldk", C.c_int64),
                ("ldv", C.c_int64), ("o", C.c_void_p), ("oh", C.c_void_p), ("lse", C.c_void_p), ("klen", C.c_void_p),
                ("B", C.c_int32), ("H", C.c_int32), ("T", C.c_int32), ("S", C.c_int32), ("dh", C.c_int32),
                ("causal", C.c_int32), ("scale", C.c_float), ("drop_p", C.c_float), ("seed", C.c_uint64),
                ("ld_drop", C.c_int32), ("doh", C.c_void_p), ("dq", C.c_void_p), ("dk", C.c_void_p), ("dv", C.c_void_p),
                ("dqh", C.c_void_p), ("dkh", C.c_void_p), ("dvh", C.c_void_p), ("dbq", C.c_void_p), ("dbk", C.c_void_p),
                ("dbv", C.c_void_p)]


DB_SENTINEL = 7.0       # dbq / dbk / dbv under db="parts": the kernels must leave them alone
BF16_SENTINEL = -1000.0  # exactly representable in bf16; no attention output of unit-scale inputs comes near it


def flash_attention(q, k, v, H, *, klen=None, causal=False, scale=None, drop_p=0.0, seed=0, dO=None, bf16_grads=False,
                    bf16_o=False, scratch=None, layout="dense", pad=0, f32_o=True, f32_grads=True, db=None, ld_drop=None,
                    override=None, override_bwd=None, full=False):
    """Fused attention on bf16 [B, T, H*dh] / [B, S, H*dh] projections (s2st_flash_attn_*_bf16).
    Returns (o fp32, lse) and, when dO (fp32 [B, T, H*dh]) is given, also (dq, dk, dv) fp32.  ``bf16_o``: the forward also
    leaves the bf16 copy of o (what the engine does); the backward then forms D = rowsum(dO * o) inside its kernels from
    the bf16 copies instead of running the fp32 row kernel first.

    The keyword options after ``scratch`` reproduce the calling conventions of the training step (engine_ops.cpp):

    * ``layout``: "dense" (three tensors), "self" (q / k / v are column blocks of ONE packed projection [K|V|Q], T == S) or
      "cross" (dense q, k / v column blocks of a packed [K|V]); the gradients are written in the same layout.  ``pad``:
      extra columns at the end of every row of those buffers (row stride = columns + pad, a multiple of 8 elements);
    * ``f32_o`` / ``f32_grads`` = False: no fp32 O / no fp32 gradients are passed (null pointers; needs ``bf16_o`` /
      ``bf16_grads``);
    * ``db``: the projections' bias gradients -- "none", "atomic" (+= into three [H*dh] tensors) or "parts"
      (s2st_flash_attn_bwd_parts_bf16: per-(block, wave) partial rows, the three tensors stay untouched); None = "atomic"
      with ``bf16_grads`` and "none" without, as before;
    * ``ld_drop``: row stride of the dropout index space (default: S rounded up to 8);
    * ``override`` / ``override_bwd``: {field of s2st_attn_args: value or f(args) -> value} applied just before the forward /
      the backward call ("dO" in ``override_bwd`` replaces that argument), for tests of the launchers' refusals;
    * ``full`` = True: return a namespace of everything that was passed -- o, oh, lse, dq, dk, dv, dqh, dkh, dvh (views of
      the packed buffers), dbq, dbk, dbv, db_part with its views dbq_part / dbk_part / dbv_part [slots][H*dh], slots_q,
      slots_k, the packed buffers themselves (bufs: name -> tensor, data columns first, pad columns last) -- instead of
      the tuples.  A refused call raises S2STHipError carrying that namespace as ``.outputs``.

    Every output starts from a sentinel, so that a test sees what a call left alone: NaN in the fp32 buffers, ``lse``
    and the partial-sum scratch, BF16_SENTINEL in the bf16 buffers, DB_SENTINEL in dbq / dbk / dbv under "parts" (zeros
    under "atomic": the kernels add)."""
    import types
    require_device(q)
    B, T, Cm = q.shape
    S = k.shape[1]
    dh = Cm // H
    dev = q.device
    if db is None:
        db = "atomic" if bf16_grads else "none"
    if layout not in ("dense", "self", "cross") or db not in ("none", "atomic", "parts") or pad % 8:
        raise S2STHipError("flash_attention: unknown layout / db option, or pad not a multiple of 8")
    if layout == "self" and T != S:
        raise S2STHipError("flash_attention: the self-packed layout needs T == S")
    # groups of column blocks that share one buffer (the engine's packed projections), in the engine's order
    groups = {"dense": (("q",), ("k",), ("v",)), "self": (("k", "v", "q"),), "cross": (("q",), ("k", "v"))}[layout]
    src = {"q": q, "k": k, "v": v}
    bufs = {}

    def packed(dtype, fill, tag, data=None):
        """one buffer per group, [B, rows, n * Cm + pad]; returns the q / k / v column-block views"""
        views = {}
        for names in groups:
            rows = T if names[-1] == "q" else S
            buf = torch.full((B, rows, len(names) * Cm + pad), fill, dtype=dtype, device=dev)
            bufs[tag + "".join(names)] = buf
            for j, nm in enumerate(names):
                views[nm] = buf[:, :, j * Cm:(j + 1) * Cm]
                if data is not None:
                    views[nm].copy_(data[nm])
        return views

    nan = float("nan")
    inp = packed(torch.bfloat16, BF16_SENTINEL, "in_", src)
    ld = {nm: inp[nm].stride(1) for nm in "qkv"}

    def at(view):  # device address of a column-block view
        return view.data_ptr() if view is not None else None

    r = types.SimpleNamespace(bufs=bufs, slots_q=0, slots_k=0)
    a = AttnArgs()
    a.q, a.k, a.v = at(inp["q"]), at(inp["k"]), at(inp["v"])
    a.ldq, a.ldk, a.ldv = ld["q"], ld["k"], ld["v"]
    r.o = torch.full((B, T, Cm), nan, dtype=torch.float32, device=dev) if f32_o else None
    r.oh = torch.full((B, T, Cm), BF16_SENTINEL, dtype=torch.bfloat16, device=dev) if bf16_o else None
    lse = torch.full((B * H * T,), nan, dtype=torch.float32, device=dev)
    r.lse = lse.view(B, H, T)
    a.o, a.oh, a.lse, a.klen = ptr(r.o), ptr(r.oh), lse.data_ptr(), ptr(klen)
    a.B, a.H, a.T, a.S, a.dh, a.causal = B, H, T, S, dh, 1 if causal else 0
    a.scale = scale if scale is not None else dh ** -0.5
    a.drop_p, a.seed, a.ld_drop = drop_p, seed, ld_drop if ld_drop is not None else (S + 7) // 8 * 8

    def apply(ov):
        extra = {}
        for key, val in (ov or {}).items():
            val = val(a) if callable(val) else val
            if key == "dO":
                extra[key] = val
            else:
                setattr(a, key, val)
        return extra

    def run(fn, what, *args):
        try:
            check(fn(C.byref(a), *args, C.c_void_p(stream_ptr())), what)
        except S2STHipError as e:
            e.outputs = r
            raise

    apply(override)
    run(lib().s2st_flash_attn_fwd_bf16, "s2st_flash_attn_fwd_bf16")
    if dO is None:
        return r if full else (r.o, r.lse)
    doh = dO.to(torch.bfloat16).contiguous()
    if scratch is None:  # (tools/attn_stamp.py passes a larger one: the private stamp build writes clock stamps there)
        scratch = torch.zeros(B * H * T, dtype=torch.float32, device=dev)
    a.doh = doh.data_ptr()
    g32 = packed(torch.float32, nan, "g32_") if f32_grads else {"q": None, "k": None, "v": None}
    g16 = packed(torch.bfloat16, BF16_SENTINEL, "g16_") if bf16_grads else {"q": None, "k": None, "v": None}
    r.dq, r.dk, r.dv = g32["q"], g32["k"], g32["v"]
    r.dqh, r.dkh, r.dvh = g16["q"], g16["k"], g16["v"]
    a.dq, a.dk, a.dv = at(r.dq), at(r.dk), at(r.dv)
    a.dqh, a.dkh, a.dvh = at(r.dqh), at(r.dkh), at(r.dvh)
    r.dbq = r.dbk = r.dbv = r.db_part = r.dbq_part = r.dbk_part = r.dbv_part = None
    if db != "none":
        r.dbq, r.dbk, r.dbv = (torch.full((Cm,), DB_SENTINEL if db == "parts" else 0.0, dtype=torch.float32, device=dev)
                               for _ in range(3))
        a.dbq, a.dbk, a.dbv = r.dbq.data_ptr(), r.dbk.data_ptr(), r.dbv.data_ptr()
    dO_arg = apply(override_bwd).get("dO", dO)
    if db == "parts":
        sq, sk = C.c_int32(0), C.c_int32(0)
        check(lib().s2st_flash_attn_db_slots(C.byref(a), C.byref(sq), C.byref(sk)), "s2st_flash_attn_db_slots")
        r.slots_q, r.slots_k = sq.value, sk.value
        n = lib().s2st_flash_attn_db_scratch(C.byref(a))
        if n != (r.slots_q + 2 * r.slots_k) * Cm:
            raise S2STHipError("s2st_flash_attn_db_scratch disagrees with s2st_flash_attn_db_slots")
        r.db_part = torch.full((n,), nan, dtype=torch.float32, device=dev)
        rows = r.db_part.view(-1, Cm)
        r.dbq_part, r.dbk_part, r.dbv_part = (rows[:r.slots_q], rows[r.slots_q:r.slots_q + r.slots_k],
                                              rows[r.slots_q + r.slots_k:])
        run(lib().s2st_flash_attn_bwd_parts_bf16, "s2st_flash_attn_bwd_parts_bf16", ptr(dO_arg), scratch.data_ptr(),
            r.db_part.data_ptr())
    else:
        run(lib().s2st_flash_attn_bwd_bf16, "s2st_flash_attn_bwd_bf16", ptr(dO_arg), scratch.data_ptr())
    if full:
        return r
    if bf16_grads:  # also the bf16 copies + bias-gradient column sums
        return r.o, r.lse, r.dq, r.dk, r.dv, [r.dqh, r.dkh, r.dvh, r.dbq, r.dbk, r.dbv]
    return r.o, r.lse, r.dq, r.dk, r.dv


# ---------------------------------------------------------------------------------------------
# the signatures of every entry point are derived from include/s2st_hip.h (load_library) so the
# binding cannot drift from the declared C ABI
# ---------------------------------------------------------------------------------------------
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include", "s2st_hip.h")
_CT = {"int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "float": C.c_float, "double": C.c_double,
       "int": C.c_int, "s2st_split": Split}
_protos = None


def header_prototypes():
    """{name: (restype, [(ctype, argname), ...])} parsed from the C header."""
    global _protos
    if _protos is not None:
        return _protos
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(int|int32_t|int64_t|void)(\s*\*\s*|\s+)(s2st_\w+)\s*\(([^;{}]*?)\)\s*;", src, flags=re.S):
        ret, name, args = m.group(1) + m.group(2).strip(), m.group(3), m.group(4).strip()
        alist = []
        if args and args != "void":
            for a in args.split(","):
                a = " ".join(a.split())
                if "*" in a:
                    alist.append((C.c_void_p, a.split("*")[-1].strip()))
                elif a == "void":
                    continue
                else:
                    ty, nm = a.rsplit(" ", 1)
                    alist.append((_CT[ty.replace("const ", "").strip()], nm))
        out[name] = ({"int64_t": C.c_int64, "void": None}.get(ret, C.c_void_p if ret.endswith("*") else C.c_int), alist)
    _protos = out
    return out


def _bind(name):
    return getattr(lib(), name)


def call(name: str, *args):
    """Call a C-ABI entry point; torch tensors become device pointers, the trailing `stream`
    argument is filled with the current torch stream."""
    fn = _bind(name)
    conv = []
    for a in args:
        if isinstance(a, torch.Tensor):
            require_device(a)
            conv.append(a.data_ptr())
        else:
            conv.append(a)
    conv.append(stream_ptr())
    rc = fn(*conv)
    check(rc, name)
