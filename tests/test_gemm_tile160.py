"""The 160-row GEMM tiles (K-contiguous A): 160 x 128 on the 4-wave early-release form (gemm_bf16_w4.hip) and 160 x 64 on
the 8-wave LDS-DMA ring form (gemm_bf16.hip, A image padded to 192 rows of DMA pieces).

Per output element the K order and the MFMA shape are those of the 128-row tiles and dropout masks are indexed by
element, so the criterion is not a tolerance: C (fp32 and bf16) of a launch forced to a 160-row tile equals the same
call forced to the 128-row tile of the same width bit for bit.  Only the column sums of the masked epilogue regroup
(wave rows of 80 instead of 64 rows); their bound is derived in _colsum_bound()."""
import ctypes

import pytest
import torch

MS = (81, 159, 160, 161, 323)  # wave-row boundary at 80 | one row short | one full tile | a second tile of one row | clamped rows inside a piece
NS = (64, 72, 128, 192)
KS = (64, 192, 200, 512)       # one K-step | fewer steps than the 8-wave ring holds | a K tail | steady state
MMAX, NMAX, KMAX = max(MS), max(NS), max(KS)
FORMS = {"160x128": "128x128", "160x64": "128x64"}  # forced tile -> the 128-row tile it is compared with
EPILOGUES = ("plain", "h_bias_relu_drop", "bias_resid", "accumulate", "masked")


@pytest.fixture(scope="module")
def operands():
    """One set of host operands for every case (cases slice it): A [MMAX][KMAX] K-contiguous, B in both layouts."""
    g = torch.Generator().manual_seed(160)
    A = torch.randn(MMAX, KMAX, generator=g).to(torch.bfloat16)
    B = (torch.randn(NMAX, KMAX, generator=g) / KMAX ** 0.5).to(torch.bfloat16)
    o = {"A": A, "B": B, "Bt": B.t().contiguous(), "bias": torch.randn(NMAX, generator=g),
         "resid": torch.randn(MMAX, NMAX, generator=g), "old": torch.randn(MMAX, NMAX, generator=g)}
    y = torch.relu(torch.randn(MMAX, NMAX, generator=g))  # a ReLU + dropout layer's output: about half zeros
    y[torch.rand(MMAX, NMAX, generator=g) < 0.1] = 0.0
    o["y"] = y.to(torch.bfloat16)
    return o


_dev = {}


def _on(backend, operands):
    if backend.kind not in _dev:
        _dev[backend.kind] = {k: v.to(backend.device) for k, v in operands.items()}
    return _dev[backend.kind]


def _colsum_bound(v_abs_sum, rows):
    """|colsum - sum_m float64(bf16(v[m]))| for one column.  The kernel adds the fp32 values v before they are rounded to the
    stored bf16: each differs from its stored value by at most half a bf16 ulp, 2^-9 |v|; the fp32 additions (16 rows in
    a lane, a 16-lane tree, one atomic per wave row: `rows` terms in any grouping) add at most rows * 2^-24 * sum |v|
    (first order).  Both are bounded with the stored values' sum of magnitudes, itself within 2^-9 of the exact one."""
    return v_abs_sum * (2.0 ** -9 + rows * 2.0 ** -24) * (1 + 2.0 ** -8)


def _run(backend, dv, tile, epi, M, N, K, bkm, zero_bias=False):
    """One launch under S2ST_GEMM_TILE=tile (the caller set it); returns (tile, fp32 C or None, bf16 C or None, colsum)."""
    d = backend.device
    kw = dict(a_kmajor=True, a_ld=KMAX, b_kmajor=bkm, b_ld=KMAX if bkm else NMAX, return_tile=True)
    B = dv["B"] if bkm else dv["Bt"]
    C = Ch = cs = None
    if epi == "plain":
        C = torch.full((M, N), 7.0, device=d)
        t = backend.bd.gemm(dv["A"], B, C, M, N, K, **kw)
    elif epi == "h_bias_relu_drop":
        Ch = torch.full((M, N), 7.0, dtype=torch.bfloat16, device=d)
        t = backend.bd.gemm(dv["A"], B, None, M, N, K, c_bf16=Ch, bias=dv["bias"][:N].contiguous(), act=1, drop_p=0.1, seed=5, **kw)
    elif epi == "bias_resid":
        C = torch.full((M, N), 7.0, device=d)
        t = backend.bd.gemm(dv["A"], B, C, M, N, K, bias=dv["bias"][:N].contiguous(), resid=dv["resid"][:M, :N].contiguous(), **kw)
    elif epi == "accumulate":
        C = dv["old"][:M, :N].contiguous()
        bias = torch.zeros(N, device=d) if zero_bias else None
        t = backend.bd.gemm(dv["A"], B, C, M, N, K, accumulate=True, bias=bias, **kw)
    else:
        Ch = torch.full((M, N), 7.0, dtype=torch.bfloat16, device=d)
        cs = torch.zeros(N, device=d)
        t = backend.bd.gemm(dv["A"], B, None, M, N, K, c_bf16=Ch, mask_y=dv["y"][:M, :N].contiguous(), mask_scale=1.0 / 0.9,
                            colsum=cs, **kw)
    backend.sync()
    return t, C, Ch, cs


@pytest.mark.parametrize("epi", EPILOGUES)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("bkm", [True, False])
@pytest.mark.parametrize("tile", sorted(FORMS))
def test_tile160_equals_128_row_tile(backend, monkeypatch, operands, tile, bkm, K, epi):
    """Every (M, N) of the lists above for one (form, B layout, K, epilogue): the forced launch reports the 160-row tile
    (a silent fallback fails here) and its outputs equal the 128-row launch's bit for bit."""
    dv = _on(backend, operands)
    monkeypatch.setenv("S2ST_GEMM_PERSIST", "0")
    bn = int(tile.split("x")[1])
    for M in MS:
        for N in NS:
            monkeypatch.setenv("S2ST_GEMM_W4", "-1")
            monkeypatch.setenv("S2ST_GEMM_TILE", tile)
            t, C, Ch, cs = _run(backend, dv, tile, epi, M, N, K, bkm)
            assert t == (160, bn), (M, N, t)
            # the reference launch: the 128-row tile of the same width on the same form (S2ST_GEMM_W4=1 puts a forced
            # 128 x 128 tile on the 4-wave form; 0 keeps 128 x 64 on the 8-wave ring).  An accumulating fp32 product with
            # K >= 512 and few tiles splits K under a 128-row tile (atomics: another summation order, by design) -- a zero
            # bias vector keeps that one launch unsplit and adds +0.0 to every element.
            monkeypatch.setenv("S2ST_GEMM_W4", "1" if tile == "160x128" else "0")
            monkeypatch.setenv("S2ST_GEMM_TILE", FORMS[tile])
            t2, C2, Ch2, cs2 = _run(backend, dv, FORMS[tile], epi, M, N, K, bkm, zero_bias=(epi == "accumulate" and K >= 512))
            assert t2 == (128, bn), (M, N, t2)
            if C is not None:
                assert torch.equal(C, C2), (M, N)
            if Ch is not None:
                assert torch.equal(Ch, Ch2), (M, N)
            if cs is not None:
                v = Ch.double().cpu()
                ref, mag = v.sum(0), v.abs().sum(0)
                err = (cs.double().cpu() - ref).abs()
                bound = _colsum_bound(mag, M)
                print(f"colsum M {M} N {N} K {K}: max err {err.max().item():.3e}  min bound {bound.min().item():.3e}")
                assert bool((err <= bound).all()), (M, N, (err - bound).max().item())
                assert bool((Ch.cpu()[dv["y"][:M, :N].cpu() == 0] == 0).all())  # (the mask itself: zero where y is +-0)


def test_plain_against_float64(backend, monkeypatch, operands):
    """The bit-equality above is against another tile of the same kernels; this anchors one shape per form to float64."""
    dv = _on(backend, operands)
    monkeypatch.setenv("S2ST_GEMM_PERSIST", "0")
    M, N, K = 323, 192, 200
    R = operands["A"][:M, :K].double() @ operands["B"][:N, :K].double().t()
    for tile in sorted(FORMS):
        monkeypatch.setenv("S2ST_GEMM_TILE", tile)
        t, C, _, _ = _run(backend, dv, tile, "plain", M, N, K, True)
        assert t == (160, int(tile.split("x")[1]))
        # exact products of bf16 values, fp32 accumulation (the bound test_gemm.py uses for this quantity)
        assert ((C.double().cpu() - R).norm() / R.norm()).item() < 2e-6


@pytest.mark.gpu
def test_unforced_pick_at_the_step_shapes(monkeypatch):
    """On the chip (256 CUs): the encoder's products just past M = 4096 take a 160-row tile by the rounds-of-slots rule, and
    at M = 4096 the pick is what it was (128 x 128 on the 4-wave form for N = 2048, 128 x 64 on the ring for N = 512)."""
    import importlib
    bd = importlib.import_module("speech-to-speech-translation_amd.runtime.binding")
    if bd.is_emulator():
        bd.load_library(bd.DEFAULT_LIB, emulator=False)
    for k in ("S2ST_GEMM_TILE", "S2ST_GEMM_W4", "S2ST_GEMM_PERSIST", "S2ST_GEMM_P4"):
        monkeypatch.delenv(k, raising=False)
    d = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    for (M, N, K), want in (((4584, 2048, 512), (160, 128)), ((4584, 512, 2048), (160, 64)), ((4584, 512, 512), (160, 64)),
                            ((5120, 2048, 512), (160, 128)), ((5120, 512, 2048), (160, 64)),
                            ((4096, 2048, 512), (128, 128)), ((4096, 512, 2048), (128, 64)), ((4584, 1536, 512), (128, 128))):
        A = torch.randn(M, K, generator=g).to(torch.bfloat16).to(d)
        B = (torch.randn(N, K, generator=g) / K ** 0.5).to(torch.bfloat16).to(d)
        C = torch.zeros(M, N, device=d)
        plan = bd.gemm_plan(bd.gemm_args_bf16(A, B, C, M, N, K))  # (ncu = 0: this chip's) the query names the same launch
        bd.lib().s2st_profile_enable(1)
        t = bd.gemm(A, B, C, M, N, K, return_tile=True)
        torch.cuda.synchronize()
        bd.lib().s2st_profile_enable(0)
        assert t == want, ((M, N, K), t)
        buf = ctypes.create_string_buffer(1 << 16)
        n = bd.lib().s2st_profile_report(buf, len(buf))
        assert (plan.bm, plan.bn) == want and [ln.split("\t")[0] for ln in buf.raw[:max(n, 0)].decode().splitlines()] == [plan.tag], plan
        monkeypatch.setenv("S2ST_GEMM_TILE", "128x128")
        C2 = torch.zeros(M, N, device=d)
        bd.gemm(A, B, C2, M, N, K)
        torch.cuda.synchronize()
        monkeypatch.delenv("S2ST_GEMM_TILE")
        assert torch.equal(C, C2), (M, N, K)
