"""What the bf16 GEMM dispatcher decides (csrc/gemm_bf16_plan.h through s2st_gemm_plan_f32 / binding.gemm_plan), against
tests/golden/gemm_dispatch.npz: the launches the launcher made BEFORE the decision became one function, recorded over a sweep
of shapes, layouts, alignments, epilogues, switches and CU counts (tools/gen_golden_gemm_dispatch.py has the procedure).
Host-only: the query launches nothing, so the decisions for a 256-CU chip are checked on the emulator build.

Rows recorded under a switch that the library reads once per process (S2ST_GEMM_DMA, S2ST_SPLITK_TARGET) are compared in a
child process started with that switch; everything else runs here."""
import ctypes as C
import importlib
import json
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
import gen_golden_gemm_dispatch as G  # noqa: E402

EMU_SLOTS160 = 2  # workgroups of the 160 x 128 form per CU by the LDS arithmetic the host build (and the recording) uses


def compare(bd, procs):
    """Every row of the given recorder processes: (rows compared, list of mismatches)."""
    envs, tags, c = G.load()
    cols = [c[k].tolist() for k in G.IN_COLS + G.OUT_COLS]
    sw = G.Switches()
    cache, bad, n = {}, [], 0
    try:
        for row in zip(*cols):
            (proc, ncu, ei, sk, gi, M, N, K, batch, akm, bkm, per, mis, epi,
             x_rc, x_launches, x_tag, x_form, x_tile, x_gx, x_gy, x_block, x_lds, x_splitk, x_kchunk, x_tiles_n, x_cvec, x_slab,
             x_gn, x_gtotal, x_gsk, x_reduce_gx) = row
            if proc not in procs:
                continue
            n += 1
            sw.set(envs[ei])
            key = (gi, M, N, K, batch, akm, bkm, per, mis, epi)
            args = cache.get(key)
            if args is None:
                args = cache[key] = G.group_args(bd, gi) if gi >= 0 else G.single_args(bd, M, N, K, batch, akm, bkm, per, mis, epi)
            p = bd.gemm_plan(args, ncu=ncu, slots160=EMU_SLOTS160, sk_bound=bool(sk))
            if x_rc != 0 or p.error != 0:
                if p.error != x_rc:
                    bad.append((row[:14], "error code", p.error, x_rc))
                continue
            if gi >= 0:
                cvec = sum(v << (4 * i) for i, v in enumerate(p.cvec_of))
                want_total = (x_gn, x_gtotal, bool(x_gsk))
            else:
                cvec = p.cvec
                persistent = G.FORMS[x_form] == "PERSISTENT"
                want_total = (1, x_gtotal, bool(x_gsk)) if persistent else (0, 0, False)
            got = (p.form, p.tag, p.bm * 1000 + p.bn if gi < 0 else None, p.splitk, p.kchunk, p.tiles_n, cvec, int(p.use_slab), p.grid,
                   (p.n, p.total, p.sk))
            want = (G.FORMS[x_form], tags[x_tag], x_tile if gi < 0 else None, x_splitk, x_kchunk, x_tiles_n, x_cvec,
                    x_slab, (x_gx, x_gy), want_total)
            if got != want:
                bad.append((row[:14], envs[ei], got, want))
            if (x_reduce_gx > 0) != p.use_slab or x_launches != 1 + int(p.use_slab):  # the split-K combine follows slabs only
                bad.append((row[:14], "reduce launch", x_reduce_gx, p.use_slab))
    finally:
        sw.restore()
    return n, bad


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call([os.path.join(ROOT, "tests", "hipemu", "build_emu.sh")], stdout=subprocess.DEVNULL)
    bd = importlib.import_module("speech-to-speech-translation_amd.runtime.binding")
    bd.load_library(os.path.join(ROOT, "tests", "hipemu", "_build", "libs2st_emu.so"), emulator=True)
    return bd


def test_table_covers_the_sweep():
    """The committed table is the sweep the tool defines, row for row (nothing dropped on either side)."""
    envs, rows = G.sweep()
    genvs, _, c = G.load()
    assert genvs == envs
    assert len(rows) == len(c["M"])
    assert rows == list(zip(*[c[k].tolist() for k in G.IN_COLS]))
    assert set(c["x_form"].tolist()) - {-1} == set(range(len(G.FORMS)))  # every form was met


def test_plan_equals_the_recorded_launches(emu):
    """Default process switches, 8 and 256 CUs: every recorded row, every field."""
    n, bad = compare(emu, (0, 1))
    print(n, "rows compared")
    assert n > 100000 and not bad, (len(bad), bad[:5])


@pytest.mark.parametrize("procs", [(2, 3), (4, 5)])
def test_plan_equals_the_recorded_launches_process_switches(emu, procs):
    """S2ST_GEMM_DMA=0 and S2ST_SPLITK_TARGET=64 are read once per process: their rows in a child started with them."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("S2ST_")}
    env.update({k: v for k, v in G.PROCS[procs[0]][0].items() if k != "S2ST_GEMM_PERSIST_WGS"})
    out = subprocess.run([sys.executable, os.path.abspath(__file__)] + [str(p) for p in procs], env=env, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    n, bad = json.loads(out.stdout.strip().splitlines()[-1])
    print(n, "rows compared")
    assert n > 5000 and not bad, (len(bad), bad[:5])


def _bf(x):
    return x.to(torch.bfloat16)


LAUNCHES = {  # form -> (switches, M, N, K): the emulator-sized shapes test_gemm.py runs that form on
    "RING": ({"S2ST_GEMM_W4": "0", "S2ST_GEMM_PERSIST": "0", "S2ST_GEMM_TILE": "128x128"}, 384, 256, 200),
    "W4": ({"S2ST_GEMM_W4": "1", "S2ST_GEMM_PERSIST": "0", "S2ST_GEMM_TILE": "128x64"}, 384, 256, 200),
    "P4": ({"S2ST_GEMM_PERSIST": "0", "S2ST_GEMM_TILE": "256x256"}, 300, 520, 200),
    "STAGED": ({}, 33, 21, 50),  # ld 50: the guarded scalar loader
    "PERSISTENT": ({"S2ST_GEMM_PERSIST": "2", "S2ST_GEMM_TILE": "128x128"}, 640, 256, 200),
    "GROUP_RING": ({"S2ST_GROUP_ONESHOT": "1", "S2ST_GEMM_W4": "0"}, 0, 0, 0),
}


@pytest.mark.parametrize("form", sorted(LAUNCHES))
def test_launch_carries_the_plans_tag(emu, monkeypatch, form):
    """One real launch per form with the profile registry on: the tag it reports is the plan's (the query describes what
    the launcher does), and the result is the product."""
    bd, lib = emu, emu.lib()
    env, M, N, K = LAUNCHES[form]
    for k in G.Switches.KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    g = torch.Generator().manual_seed(3)
    keep, refs = [], []
    if form == "GROUP_RING":
        args = []
        for (n_out, k_in, t) in G.GROUPS[0]:
            dY, X, dW = _bf(torch.randn(t, n_out, generator=g)), _bf(torch.randn(t, k_in, generator=g)), torch.zeros(n_out, k_in)
            keep += [dY, X]
            args.append(bd.gemm_args_bf16(dY, X, dW, n_out, k_in, t, a_kmajor=False, a_ld=n_out, b_kmajor=False, b_ld=k_in, accumulate=True))
            refs.append((dW, dY.double().t() @ X.double()))
    else:
        A, B, Cm = _bf(torch.randn(M, K, generator=g)), _bf(torch.randn(N, K, generator=g)), torch.zeros(M, N)
        keep += [A, B]
        args = bd.gemm_args_bf16(A, B, Cm, M, N, K)
        refs.append((Cm, A.double() @ B.double().t()))
    plan = bd.gemm_plan(args)
    assert plan.error == 0 and plan.form == form, plan
    lib.s2st_profile_enable(1)
    try:
        if form == "GROUP_RING":
            bd.gemm_group(args)
        else:
            bd.check(lib.s2st_gemm_f32(C.byref(args), None), "s2st_gemm_f32")
    finally:
        lib.s2st_profile_enable(0)
    buf = C.create_string_buffer(1 << 16)
    n = lib.s2st_profile_report(buf, len(buf))
    assert n > 0
    reported = [line.split("\t")[0] for line in buf.raw[:n].decode().splitlines() if line]
    assert reported == [plan.tag], (reported, plan.tag)
    for got, ref in refs:
        assert ((got.double() - ref).abs().max() / ref.abs().max()).item() < 2e-6


if __name__ == "__main__":  # the child of test_plan_equals_the_recorded_launches_process_switches
    _bd = importlib.import_module("speech-to-speech-translation_amd.runtime.binding")
    _bd.load_library(os.path.join(ROOT, "tests", "hipemu", "_build", "libs2st_emu.so"), emulator=True)
    print(json.dumps(compare(_bd, tuple(int(a) for a in sys.argv[1:]))))
