"""tests/golden/gemm_dispatch.npz: what the bf16 GEMM launcher decides, recorded from the launcher itself.

The table is the yardstick of tests/test_gemm_dispatch.py: for every row, the plan query (s2st_gemm_plan_f32 /
binding.gemm_plan) must name the launch the recorded launcher made -- tag, grid, tile, split-K geometry, epilogue marks.

Recording procedure (the expected values come from the commit BEFORE the plan function existed, 27cd0c5, never from the
code under test):
  1. in a scratch copy of that commit, replace the body of s2st_launch (csrc/s2st_prof.h) with a recorder that launches
     nothing and stores, per call, the tag, grid, block and LDS bytes and -- for a GemmArgs / GemmGroup argument -- splitk,
     kchunk, tiles_n, cvec (groups: 4 bits per problem) and slab != nullptr; c_api.cpp exports the records as
     s2st_rec_count() / s2st_rec_get(i, char tag[128], int32 v[16]) / s2st_rec_clear() with
     v = grid.x, grid.y, grid.z, block.x, lds, kind (1 GemmArgs, 2 GemmGroup), splitk, kchunk, tiles_n, cvec, slab,
         group n, group total, group sk, group xcd_global;
  2. build it with tests/hipemu/build_emu.sh (the -DS2ST_EXPERIMENTAL host build);
  3. python tools/gen_golden_gemm_dispatch.py --record <that libs2st_emu.so>
No kernel runs, so the operand addresses are fake: 16-byte aligned ones, and ones off by 4 bytes.

The switches that the library reads once per process (S2ST_GEMM_DMA, S2ST_SPLITK_TARGET, and S2ST_GEMM_PERSIST_WGS, which
is how the recorded launcher is given a 256-CU chip on a host) get a recorder process each: PROCS below.  A row's `proc`
column names its process, `env` the per-call switches set around that one call.

Columns: the inputs of a row (shape, layouts, alignment, epilogue, switches) and what was recorded (x_*).  `form` is
derived from the recorded kernel name (FORM_OF_KERNEL)."""
import argparse
import ctypes as C
import importlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_dispatch.npz")

# ---- the sweep -------------------------------------------------------------------------------------------------------
MS = (1, 64, 127, 128, 300, 512, 2560, 2800, 3072, 4096, 4097, 4584, 5120, 5121, 9600, 19200, 307200)
NS = (1, 64, 72, 128, 512, 768, 1536, 2048, 3072, 4096)
KS = (64, 200, 512, 2048, 4096, 4608)
# the reduced list of the switch sweeps: both sides of every threshold of the pickers (M < 128; the 128 / 256 / 512-row
# limits; one round / two rounds of 128-row tiles at N = 512 and 2048 on 256 CUs; the 160-row window 4096 < M <= 5120;
# many rounds), N <= 64 / ragged / 512 / 2048, K below and above 8 K-steps and 1024
MS_R = (1, 128, 300, 512, 2800, 4096, 4584, 5121, 19200)
NS_R = (64, 72, 128, 512, 2048)
KS_R = (64, 512, 4096)
LAYOUTS = ((1, 1), (1, 0), (0, 1), (0, 0))  # (A K-contiguous, B K-contiguous)
EPILOGUES = ("plain", "h_only", "both", "bias_relu_drop", "bias_resid", "acc_ws", "acc", "acc_bias", "masked_colsum",
             "both_bias_gelu")
WS_FLOATS = 1 << 22  # small enough that the slab count is cut by the workspace on the larger outputs
TILES = ("64x64", "128x64", "128x128", "160x64", "160x128", "256x128", "256x256", "junk")
# (process switches, CU count the recorded launcher sees)
PROCS = (({}, 8), ({"S2ST_GEMM_PERSIST_WGS": "256"}, 256),
         ({"S2ST_GEMM_DMA": "0"}, 8), ({"S2ST_GEMM_DMA": "0", "S2ST_GEMM_PERSIST_WGS": "256"}, 256),
         ({"S2ST_SPLITK_TARGET": "64"}, 8), ({"S2ST_SPLITK_TARGET": "64", "S2ST_GEMM_PERSIST_WGS": "256"}, 256))
FORMS = ("STAGED", "RING", "W4", "P4", "PERSISTENT", "RING_256x128", "GROUP_RING", "GROUP_W4", "GROUP_PERSISTENT",
         "GROUP_PERSISTENT_256")
# the groups of test_gemm.py::test_bf16_group_of_weight_gradients, (N_out, K_in, T) each, at both of its sizes and for
# both tile lists; the last one mixes operand layouts (an error)
GROUPS = tuple([(256, 128, t1), (128, 256, t1), (128, 128, t2), (384, 128, t2)] for t1, t2 in ((200, 136), (4584, 3120))) + \
         tuple([(256, 128, t1), (512, 256, t1), (320, 128, t2), (384, 384, t2)] for t1, t2 in ((200, 136), (4584, 3120))) + \
         ("mixed",)
GROUP_ENVS = ({}, {"S2ST_GROUP_ONESHOT": "1", "S2ST_GEMM_W4": "0"}, {"S2ST_GROUP_ONESHOT": "1", "S2ST_GEMM_W4": "2"},
              {"S2ST_GROUP_ONESHOT": "0"}, {"S2ST_GROUP_ONESHOT": "0", "S2ST_GROUP_TILE": "128"},
              {"S2ST_GROUP_ONESHOT": "0", "S2ST_GROUP_TILE": "256"}, {"S2ST_GROUP_TILE": "256"},
              {"S2ST_GEMM_PERSIST": "0"}, {"S2ST_GEMM_FAST_EPI": "0"},
              {"S2ST_GEMM_STREAMK": "1", "+sk": "1"}, {"S2ST_GEMM_STREAMK": "0", "+sk": "1"},
              {"S2ST_GEMM_STREAMK": "1", "S2ST_STREAMK_MIN_STEPS": "2", "+sk": "1"})

IN_COLS = ("proc", "ncu", "env", "sk", "group", "M", "N", "K", "batch", "akm", "bkm", "per", "mis", "epi")
OUT_COLS = ("x_rc", "x_launches", "x_tag", "x_form", "x_tile", "x_gx", "x_gy", "x_block", "x_lds", "x_splitk", "x_kchunk",
            "x_tiles_n", "x_cvec", "x_slab", "x_gn", "x_gtotal", "x_gsk", "x_reduce_gx")


def _envs():
    """Every per-call switch setting of the sweep ("+sk": a stream-K scratch is bound to the stream), and the (layout,
    epilogue, batch) combinations each runs over."""
    wide = [(1, 1, "plain", 1), (1, 1, "plain", 16), (1, 0, "plain", 1), (1, 1, "acc_ws", 1), (0, 0, "acc", 1),
            (1, 1, "masked_colsum", 1), (1, 1, "bias_resid", 1)]
    narrow = [(1, 1, "plain", 1), (1, 1, "acc_ws", 1), (0, 0, "acc", 1)]
    out = []
    for t in TILES:
        out.append(({"S2ST_GEMM_TILE": t}, wide))
    for v in ("0", "1", "2"):
        out.append(({"S2ST_GEMM_W4": v}, wide))
    for v in ("0", "1"):
        out.append(({"S2ST_GEMM_P4": v}, wide))
    for v in ("0", "2", "3"):
        out.append(({"S2ST_GEMM_PERSIST": v}, wide))
    out.append(({"S2ST_GEMM_FAST_EPI": "0"}, wide))
    out.append(({"S2ST_GEMM_STREAMK": "1", "+sk": "1"}, wide))
    out.append(({"S2ST_GEMM_STREAMK": "1"}, narrow))
    out.append(({"S2ST_GEMM_STREAMK": "0", "+sk": "1"}, narrow))
    out.append(({"+sk": "1"}, narrow))
    out.append(({"S2ST_GEMM_STREAMK": "1", "S2ST_STREAMK_MIN_STEPS": "2", "+sk": "1"}, narrow))
    out.append(({"S2ST_GEMM_STREAMK": "1", "S2ST_GEMM_TILE": "128x128", "+sk": "1"}, narrow))
    out.append(({"S2ST_GEMM_PERSIST": "3", "S2ST_GEMM_TILE": "128x64"}, narrow))
    out.append(({"S2ST_GEMM_PERSIST": "2", "S2ST_GEMM_TILE": "128x128"}, narrow))
    for t in TILES:
        for v in ("0", "1", "2"):
            out.append(({"S2ST_GEMM_TILE": t, "S2ST_GEMM_W4": v}, narrow))
        for v in ("0", "1"):
            out.append(({"S2ST_GEMM_TILE": t, "S2ST_GEMM_P4": v}, narrow))
    return out


def sweep():
    """(env list, rows): rows are tuples in IN_COLS order, env an index into the env list."""
    envs, rows = [{}], []

    def env_id(e):
        if e not in envs:
            envs.append(e)
        return envs.index(e)

    for proc, (penv, ncu) in enumerate(PROCS):
        full = not any(k in penv for k in ("S2ST_GEMM_DMA", "S2ST_SPLITK_TARGET"))
        ms, ns, ks = (MS, NS, KS) if full else (MS_R, NS_R, KS_R)
        # defaults: every shape x every layout (plain), every epilogue (K-contiguous operands; the accumulating ones also in
        # the weight-gradient layout), batch 16 for the plain, bf16-only and accumulating ones
        for M in ms:
            for N in ns:
                for K in ks:
                    for batch in (1, 16):
                        for akm, bkm in LAYOUTS:
                            rows.append((proc, ncu, 0, 0, -1, M, N, K, batch, akm, bkm, 0, 0, 0))
                        for e, name in enumerate(EPILOGUES):
                            if e == 0 or (batch == 16 and name not in ("h_only", "acc_ws", "acc")):
                                continue
                            rows.append((proc, ncu, 0, 0, -1, M, N, K, batch, 1, 1, 0, 0, e))
                            if name.startswith("acc"):
                                rows.append((proc, ncu, 0, 0, -1, M, N, K, batch, 0, 0, 0, 0, e))
        # operands: misaligned base (1), misaligned ld (2), misaligned output (4); a split row stride on the rows-contiguous one
        for M in MS_R:
            for N in NS_R:
                for K in KS_R:
                    for akm, bkm in LAYOUTS:
                        for mis in (1, 2, 4):
                            rows.append((proc, ncu, 0, 0, -1, M, N, K, 1, akm, bkm, 0, mis, 0))
                        if not (akm and bkm):
                            for e in (0, 6):
                                rows.append((proc, ncu, 0, 0, -1, M, N, K, 1, akm, bkm, 64, 0, e))
        if full:
            for env, combos in _envs():
                ei, sk = env_id(env), 1 if "+sk" in env else 0
                for M in MS_R:
                    for N in NS_R:
                        for K in KS_R:
                            for akm, bkm, name, batch in combos:
                                rows.append((proc, ncu, ei, sk, -1, M, N, K, batch, akm, bkm, 0, 0, EPILOGUES.index(name)))
        for gi in range(len(GROUPS)):
            for env in GROUP_ENVS:
                rows.append((proc, ncu, env_id(env), 1 if "+sk" in env else 0, gi, 0, 0, 0, 1, 0, 0, 0, 0, 6))
    return envs, rows


# ---- a row -> the call's arguments (fake addresses) ---------------------------------------------------------------------
def _bd():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    return importlib.import_module("speech-to-speech-translation_amd.runtime.binding")


def _up(x, m):
    return (x + m - 1) // m * m


def single_args(bd, M, N, K, batch, akm, bkm, per, mis, epi):
    g = bd.GemmArgs()
    name = EPILOGUES[epi]
    for op, base, rows, km in ((g.A, 0x10000000, M, akm), (g.B, 0x20000000, N, bkm)):
        op.p = base + (4 if mis & 1 else 0)
        op.kmajor, op.dtype = km, 1
        ld = _up(K if km else rows, 8) + (4 if mis & 2 else 0)
        op.sp = bd.make_split(ld, per if not km else 0, 64 * ld if (per and not km) else 0)
        op.zo, op.zi = (ld * (rows if km else K) if batch > 1 else 0), 0
    ldc = N + (2 if mis & 4 else 0)
    want_p, want_h = name not in ("h_only", "masked_colsum"), name in ("h_only", "both", "masked_colsum", "both_bias_gelu")
    g.C = bd.GemmOut(0x30000000 if want_p else None, bd.make_split(ldc), M * ldc if batch > 1 else 0, 0,
                     0x40000000 if want_h else None)
    ep = g.ep
    ep.alpha, ep.mask_scale = 1.0, 1.0
    if name in ("bias_relu_drop", "bias_resid", "acc_bias", "both_bias_gelu"):
        ep.bias = 0x50000000
    if name == "bias_relu_drop":
        ep.act, ep.drop_p, ep.seed = 1, 0.1, 5
    if name == "both_bias_gelu":
        ep.act = 2
    if name == "bias_resid":
        ep.resid = 0x60000000
    if name.startswith("acc"):
        ep.accumulate = 1
    if name == "acc_ws":
        g.ws, g.ws_floats = 0x70000000, WS_FLOATS
    if name == "masked_colsum":
        ep.mask_y, ep.colsum, ep.mask_scale = 0x48000000, 0x58000000, 1.0 / 0.9
    g.M, g.N, g.K, g.batch, g.zdiv, g.precise = M, N, K, batch, 1, 0
    return g


def group_args(bd, gi):
    probs = []
    spec = GROUPS[gi]
    mixed = spec == "mixed"
    for i, (n_out, k_in, t) in enumerate(GROUPS[0] if mixed else spec):
        g = bd.GemmArgs()
        km = 1 if (mixed and i == 2) else 0
        g.A = bd.GemmOperand(0x10000000 + (i << 24), km, 1, bd.make_split(_up(t, 8) if km else n_out), 0, 0)
        g.B = bd.GemmOperand(0x20000000 + (i << 24), 0, 1, bd.make_split(k_in), 0, 0)
        g.C = bd.GemmOut(0x30000000 + (i << 24), bd.make_split(k_in), 0, 0, None)
        g.ep.alpha, g.ep.mask_scale, g.ep.accumulate = 1.0, 1.0, 1
        g.M, g.N, g.K, g.batch, g.zdiv, g.precise = n_out, k_in, t, 1, 1, 0
        probs.append(g)
    return probs


class Switches:
    """Sets a row's per-call switches in os.environ (and binds / unbinds the fake stream-K scratch) only when they change."""
    KEYS = ("S2ST_GEMM_TILE", "S2ST_GEMM_W4", "S2ST_GEMM_P4", "S2ST_GEMM_PERSIST", "S2ST_GEMM_STREAMK", "S2ST_STREAMK_MIN_STEPS",
            "S2ST_GEMM_FAST_EPI", "S2ST_GROUP_TILE", "S2ST_GROUP_ONESHOT")

    def __init__(self, lib=None):
        self.lib, self.cur, self.saved = lib, None, {k: os.environ.get(k) for k in self.KEYS}

    def set(self, env):
        if env is self.cur:
            return
        self.cur = env
        for k in self.KEYS:
            if k in env:
                os.environ[k] = env[k]
            else:
                os.environ.pop(k, None)
        if self.lib is not None:  # (the recorded launcher looks for a scratch bound to the stream; the plan query is told)
            n = self.lib.s2st_gemm_streamk_scratch_floats()
            self.lib.s2st_gemm_streamk_scratch(C.c_void_p(0x78000000 if "+sk" in env else None), C.c_int64(n), None)

    def restore(self):
        for k, v in self.saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        if self.lib is not None:
            self.lib.s2st_gemm_streamk_scratch(None, C.c_int64(0), None)


def load():
    """The committed table: (envs, tags, {column: array})."""
    z = np.load(GOLDEN)
    return json.loads(str(z["envs"])), [str(t) for t in z["tags"]], {c: z[c] for c in IN_COLS + OUT_COLS}


def form_of(tag, kind_group):
    """The launcher's form from the recorded kernel name."""
    k = tag.split("<")[0]
    if k == "gemm_bf16_kernel":
        return "STAGED"
    if k == "gemm_bf16_p4_kernel":
        return "P4"
    if k == "gemm_bf16_w4_kernel":
        return "W4"
    if k == "gemm_bf16_w4_group_kernel":
        return "GROUP_W4"
    if k == "gemm_bf16_dma_group_kernel":
        return "GROUP_RING"
    if k == "gemm_bf16_dma_kernel":
        return "RING_256x128" if tag.startswith("gemm_bf16_dma_kernel<256,") else "RING"
    if k == "gemm_bf16_dma_persistent_kernel":
        if not kind_group:
            return "PERSISTENT"
        return "GROUP_PERSISTENT_256" if "<256," in tag else "GROUP_PERSISTENT"
    raise ValueError(tag)


# ---- recording (run against the recorder build of the parent commit) -----------------------------------------------------
def record_proc(lib_path, proc, out_path):
    bd = _bd()
    lib = bd.load_library(lib_path, emulator=True)
    lib.s2st_rec_get.argtypes = [C.c_int, C.c_char_p, C.c_void_p]
    envs, rows = sweep()
    sw = Switches(lib)
    tagbuf, v = C.create_string_buffer(128), (C.c_int32 * 16)()
    out = []
    for r in rows:
        if r[0] != proc:
            continue
        (_, ncu, ei, sk, gi, M, N, K, batch, akm, bkm, per, mis, epi) = r
        sw.set(envs[ei])
        lib.s2st_rec_clear()
        tile = C.c_int32(0)
        if gi >= 0:
            probs = group_args(bd, gi)
            arr = (bd.GemmArgs * len(probs))(*probs)
            rc = lib.s2st_gemm_group_f32(arr, len(probs), None)
        else:
            g = single_args(bd, M, N, K, batch, akm, bkm, per, mis, epi)
            rc = lib.s2st_gemm_tile_f32(C.byref(g), C.byref(tile), None)
        n = lib.s2st_rec_count()
        x = {"rc": rc, "launches": n, "tag": "", "form": -1, "tile": tile.value, "reduce_gx": 0}
        if n:
            lib.s2st_rec_get(0, tagbuf, v)
            x["tag"] = tagbuf.value.decode()
            x["form"] = FORMS.index(form_of(x["tag"], gi >= 0))
            x.update(gx=v[0], gy=v[1], block=v[3], lds=v[4], splitk=v[6], kchunk=v[7], tiles_n=v[8], cvec=v[9], slab=v[10],
                     gn=v[11], gtotal=v[12], gsk=v[13])
            assert v[2] == 1 and v[5] == (2 if gi >= 0 or x["form"] == FORMS.index("PERSISTENT") else 1), (r, list(v))
        if n > 1:
            assert n == 2
            lib.s2st_rec_get(1, tagbuf, v)
            assert tagbuf.value == b"splitk_reduce_kernel" and v[1] == batch, (r, tagbuf.value)
            x["reduce_gx"] = v[0]
        out.append(x)
    sw.restore()
    json.dump(out, open(out_path, "w"))


def record(lib_path):
    envs, rows = sweep()
    recs = []
    for proc, (penv, _) in enumerate(PROCS):
        tmp = GOLDEN + ".proc%d.json" % proc
        env = {k: v for k, v in os.environ.items() if not k.startswith("S2ST_")}
        env.update(penv)
        subprocess.check_call([sys.executable, os.path.abspath(__file__), "--record-proc", str(proc), lib_path, tmp], env=env)
        recs += json.load(open(tmp))
        os.remove(tmp)
    assert len(recs) == len(rows)
    tags = sorted({x["tag"] for x in recs})
    cols = {c: np.array([r[i] for r in rows], dtype=np.int32) for i, c in enumerate(IN_COLS)}
    for c in OUT_COLS:
        k = c[2:]
        cols[c] = np.array([tags.index(x["tag"]) if k == "tag" else x.get(k, 0) for x in recs], dtype=np.int32)
    np.savez_compressed(GOLDEN, envs=np.array(json.dumps(envs)), tags=np.array(tags), **cols)
    print(len(rows), "rows,", len(tags), "tags,", os.path.getsize(GOLDEN), "bytes ->", GOLDEN)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--record", metavar="LIB", help="the recorder build's libs2st_emu.so")
    ap.add_argument("--record-proc", nargs=3, metavar=("PROC", "LIB", "OUT"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.record_proc:
        record_proc(a.record_proc[1], int(a.record_proc[0]), a.record_proc[2])
    elif a.record:
        record(os.path.abspath(a.record))
    else:
        envs, rows = sweep()
        print(len(rows), "rows,", len(envs), "switch settings")
