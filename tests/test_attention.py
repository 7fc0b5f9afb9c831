"""Fused attention kernels (attention.hip, through the C ABI) against a float64 restatement of
fairseq MultiheadAttention's core (multihead_attention.py:224-367): masks, softmax, P*V and its
autograd.  Inputs are bf16-rounded; probabilities / score gradients pass through bf16 inside the
kernels, hence the 1-2 % tolerances."""
import pytest
import torch

from attention_ref import dropout_keep, reference, rel, rounding_model


@pytest.mark.parametrize("dh,H", [(64, 2), (128, 1)])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("bf16_o", [False, True], ids=["dvec_kernel", "d_in_kernel"])
def test_flash_attention_fwd_bwd(backend, dh, H, causal, bf16_o):
    B, T, S = 2, 37, 37 if causal else 45
    Cm = H * dh
    g = torch.Generator().manual_seed(dh + 7 * causal)
    q = torch.randn(B, T, Cm, generator=g).to(torch.bfloat16)
    k = torch.randn(B, S, Cm, generator=g).to(torch.bfloat16)
    v = torch.randn(B, S, Cm, generator=g).to(torch.bfloat16)
    dO = torch.randn(B, T, Cm, generator=g)
    klen = torch.tensor([S, S - 9], dtype=torch.int32)
    d = backend.device
    o, lse, dq, dk, dv = backend.bd.flash_attention(q.to(d), k.to(d), v.to(d), H, klen=klen.to(d), causal=causal,
                                                    dO=dO.to(d), bf16_o=bf16_o)
    backend.sync()
    ro, rl, rq, rk, rv = reference(q.float(), k.float(), v.float(), H, klen.long(), causal,
                                   dO.to(torch.bfloat16).float())
    assert rel(o, ro) < 1e-2
    assert rel(lse, rl) < 1e-4
    assert rel(dq, rq) < 2e-2 and rel(dk, rk) < 2e-2 and rel(dv, rv) < 2e-2
    # keys beyond klen get no gradient
    assert float(dk[1, S - 9:].abs().max()) == 0.0 and float(dv[1, S - 9:].abs().max()) == 0.0
    # bf16 gradient copies + fused bias-gradient column sums
    _, _, dq2, dk2, dv2, (dqh, dkh, dvh, dbq, dbk, dbv) = backend.bd.flash_attention(
        q.to(d), k.to(d), v.to(d), H, klen=klen.to(d), causal=causal, dO=dO.to(d), bf16_grads=True, bf16_o=bf16_o)
    backend.sync()
    for full, half, db in ((dq2, dqh, dbq), (dk2, dkh, dbk), (dv2, dvh, dbv)):
        assert torch.equal(half.cpu(), full.cpu().to(torch.bfloat16))
        ref_db = full.cpu().double().sum(dim=(0, 1))
        assert float((db.cpu().double() - ref_db).abs().max()) < 1e-4 * float(ref_db.abs().max() + 1e-6)


def test_flash_attention_xcd_block_order(backend):
    """Ten (batch, head) pairs: one full group of 8 (whose blocks are re-dealt so that a pair's blocks share an XCD) and two
    pairs in launch order; forward, backward and the bias-gradient partial sums against the reference."""
    B, H, dh, T, S = 5, 2, 64, 70, 83
    Cm = H * dh
    g = torch.Generator().manual_seed(3)
    q = torch.randn(B, T, Cm, generator=g).to(torch.bfloat16)
    k = torch.randn(B, S, Cm, generator=g).to(torch.bfloat16)
    v = torch.randn(B, S, Cm, generator=g).to(torch.bfloat16)
    dO = torch.randn(B, T, Cm, generator=g)
    klen = torch.tensor([S, S - 9, 40, S, 64], dtype=torch.int32)
    d = backend.device
    o, lse, dq, dk, dv, (dqh, dkh, dvh, dbq, dbk, dbv) = backend.bd.flash_attention(
        q.to(d), k.to(d), v.to(d), H, klen=klen.to(d), dO=dO.to(d), bf16_grads=True, bf16_o=True)
    backend.sync()
    ro, rl, rq, rk, rv = reference(q.float(), k.float(), v.float(), H, klen.long(), False, dO.to(torch.bfloat16).float())
    assert rel(o, ro) < 1e-2 and rel(lse, rl) < 1e-4
    assert rel(dq, rq) < 2e-2 and rel(dk, rk) < 2e-2 and rel(dv, rv) < 2e-2
    for full, db in ((dq, dbq), (dk, dbk), (dv, dbv)):
        ref_db = full.cpu().double().sum(dim=(0, 1))
        assert float((db.cpu().double() - ref_db).abs().max()) < 1e-4 * float(ref_db.abs().max() + 1e-6)


def test_flash_attention_dropout_matches_unfused_mask(backend):
    """Same (seed, element) -> same keep decision as the unfused softmax kernel: o_fused == dropout(p) v."""
    B, H, T, S, dh = 1, 1, 20, 24, 64
    g = torch.Generator().manual_seed(3)
    q = torch.randn(B, T, dh, generator=g).to(torch.bfloat16)
    k = torch.randn(B, S, dh, generator=g).to(torch.bfloat16)
    v = torch.randn(B, S, dh, generator=g).to(torch.bfloat16)
    d = backend.device
    o, _ = backend.bd.flash_attention(q.to(d), k.to(d), v.to(d), H, drop_p=0.3, seed=99)
    sc = (q.float() @ k.float().transpose(1, 2)) * dh ** -0.5
    ld = 24
    s_buf = sc.view(1, 1, T, S).contiguous().to(d)
    p = torch.zeros(1, 1, T, ld, device=d)
    pd = torch.zeros(1, 1, T, ld, device=d)
    backend.bd.call("s2st_softmax_fwd_f32", s_buf, p, pd, None, 1, 1, T, S, ld, 0, 0.3, 99)
    backend.sync()
    ref = pd[0, 0, :, :S].cpu().double() @ v[0].double()
    assert rel(o[0], ref) < 1e-2


# the BENCH's head geometry (dh 128 x H 4) at the lengths its batches really have -- one partial
# tile (31), exact tile edges (32, 64, 128), one past them (33, 129), several key blocks (213 = the 16 x 850 batch's encoder
# length, 349 = the longest timed batch), the corpus maximum (750 encoder positions, s2st_transformer.py max-source-positions
# 3000 / 4) -- self-attention with and without the causal mask (causal tile skipping needs T > 128) and cross-attention
# rectangles (decoder steps x encoder length of the timed batches); key lengths exactly ON the 32 / 64 / 128 boundaries and
# klen = 1; 16 (batch, head) pairs so that the XCD re-deal of the blocks engages at dh 128.
# Reference semantics: multihead_attention.py:332-367, s2st_transformer.py:465-477 (future mask).
BENCH_GEOMS = [(31, 31), (32, 32), (33, 33), (64, 64), (127, 127), (128, 128), (129, 129), (213, 213), (349, 349),
               (750, 750), (72, 108), (140, 213), (219, 349)]


def _boundary_klens(S):
    edges = [e for e in (128, 64, 32) if e < S]
    ks = [S] + edges[:2]
    while len(ks) < 3:
        ks.append(max(S - 1, 1))
    return ks + [1]


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("T,S", BENCH_GEOMS, ids=[f"{t}x{s}" for t, s in BENCH_GEOMS])
def test_flash_attention_bench_head_geometry(backend, T, S, causal):
    if causal and T != S:
        pytest.skip("the causal mask belongs to self-attention (T == S)")
    if backend.kind == "emu" and (T, S) not in ((31, 31), (33, 33), (129, 129)):
        pytest.skip("the emulator runs three small geometries; the sweep runs on the GPU (the CPU suite's time budget)")
    H, dh = 4, 128
    klen = torch.tensor(_boundary_klens(S), dtype=torch.int32)
    B = klen.numel()
    if backend.kind == "emu":
        B, klen = 2, klen[[1, 3]] if S > 32 else klen[[0, 3]]
    Cm = H * dh
    g = torch.Generator().manual_seed(1000 * T + S + causal)
    q = torch.randn(B, T, Cm, generator=g).to(torch.bfloat16)
    k = torch.randn(B, S, Cm, generator=g).to(torch.bfloat16)
    v = torch.randn(B, S, Cm, generator=g).to(torch.bfloat16)
    dO = torch.randn(B, T, Cm, generator=g)
    d = backend.device
    o, lse, dq, dk, dv, (dqh, dkh, dvh, dbq, dbk, dbv) = backend.bd.flash_attention(
        q.to(d), k.to(d), v.to(d), H, klen=klen.to(d), causal=causal, dO=dO.to(d), bf16_grads=True, bf16_o=True)
    backend.sync()
    ro, rl, rq, rk, rv = reference(q.float(), k.float(), v.float(), H, klen.long(), causal, dO.to(torch.bfloat16).float())
    assert rel(o, ro) < 1e-2, rel(o, ro)
    assert rel(lse, rl) < 1e-4
    assert rel(dq, rq) < 2e-2 and rel(dk, rk) < 2e-2 and rel(dv, rv) < 2e-2, (rel(dq, rq), rel(dk, rk), rel(dv, rv))
    for b in range(B):  # keys beyond klen get no gradient, and nothing leaks into them
        kl = int(klen[b])
        if kl < S:
            assert float(dk[b, kl:].abs().max()) == 0.0 and float(dv[b, kl:].abs().max()) == 0.0, b
    for full, half, db in ((dq, dqh, dbq), (dk, dkh, dbk), (dv, dvh, dbv)):
        assert torch.equal(half.cpu(), full.cpu().to(torch.bfloat16))
        ref_db = full.cpu().double().sum(dim=(0, 1))
        assert float((db.cpu().double() - ref_db).abs().max()) < 1e-4 * float(ref_db.abs().max() + 1e-6)


# ------------------------------------------------------------------------------------------------------------------------
# The kernels as the training step calls them (engine_ops.cpp: attention(), self_attn_block, cross_attn_block): q / k / v are
# column blocks of a packed projection ([K|V|Q] with ld = 3C for self-attention, dense q + [K|V] with ld = 2C for
# cross-attention), only the bf16 copies of O and of the gradients are stored, the bias gradients leave as per-(block, wave)
# partial sums, and attention dropout is on -- its mask recomputed in every backward body.
# ------------------------------------------------------------------------------------------------------------------------
HEADS = [(64, 3, 5), (128, 2, 5)]  # (dh, H, B): 15 pairs = one re-dealt XCD group of 8 + 7 in launch order; 10 pairs
# (T, S, causal): the kernel each one reaches is named in _kernel_of
ENGINE_GEOMS = [(33, 33, False), (33, 33, True), (64, 64, False), (64, 64, True),   # short, 4 waves
                (40, 100, False), (100, 40, False), (100, 100, False),             # short, 8 waves: T <= 64 < S, S <= 64 < T
                (128, 128, False), (128, 128, True),                               # short, 8 waves, the exact edge
                (129, 129, False), (129, 129, True),                               # streaming, one past the edge
                (70, 140, False), (70, 200, False), (200, 70, False),              # streaming, one side short
                (200, 200, True)]                                                  # streaming, causal tile skipping
# what the emulator runs (the CPU suite's time budget); everything runs on the GPU
EMU_CASES = {(64, 40, 100, False, 0.0), (128, 100, 40, False, 0.3), (64, 33, 33, True, 0.3), (64, 129, 129, True, 0.3),
             (128, 70, 140, False, 0.0), (64, 100, 100, False, 0.0)}
PAD = 8
S2ST_ERR_ARG = -4  # include/s2st_hip.h
O_TOL, LSE_TOL, G_TOL = 1e-2, 1e-4, 2e-2  # the bounds of the tests above


def _engine_klens(S, drop):
    """key lengths of the 5 batch elements: full, ragged, ON a 64 / 32 tile edge, one short row, full.  Under dropout the
    short row has 17 keys instead of 1: with a single key the forward's bf16 O is v itself or 0 and D = rowsum(dO * O) formed
    from it is off by bf16's rounding of O times |dO|, which alone costs 2.4e-2 .. 1.5e-1 on dk (rounding_model) -- the
    kernels' documented precision, not a defect, and no input for a 2e-2 bound."""
    edge = 64 if S > 64 else 32
    return [S, S - 9, min(S, edge), min(17, S) if drop else 1, S]


def _inputs(B, T, S, Cm, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, T, Cm, generator=g).to(torch.bfloat16)
    k = torch.randn(B, S, Cm, generator=g).to(torch.bfloat16)
    v = torch.randn(B, S, Cm, generator=g).to(torch.bfloat16)
    dO = torch.randn(B, T, Cm, generator=g)
    return q, k, v, dO


def _no_sentinel(bd, t):
    """every element was written: no NaN (fp32 buffers start as NaN) and no bf16 sentinel"""
    t = t.float().cpu()
    return not bool(torch.isnan(t).any()) and not bool((t == bd.BF16_SENTINEL).any())


def _pads_untouched(bd, r, pad):
    """the pad columns of every packed buffer the call was given still hold what the binding put there"""
    for name, buf in r.bufs.items():
        if pad == 0:
            continue
        tail = buf[..., -pad:].float().cpu()
        if name.startswith("g32_"):
            assert bool(torch.isnan(tail).all()), name
        else:
            assert bool((tail == bd.BF16_SENTINEL).all()), name


def _bits_equal(x, y):
    """bit-identical, NaN / -inf included"""
    x, y = x.cpu().contiguous(), y.cpu().contiguous()
    it = {2: torch.int16, 4: torch.int32}[x.element_size()]
    return x.dtype == y.dtype and torch.equal(x.view(it), y.view(it))


def _check_against_reference(r, ref, tag=""):
    ro, rl, rq, rk, rv = ref
    errs = dict(o=rel(r.oh.float(), ro), dq=rel(r.dqh.float(), rq), dk=rel(r.dkh.float(), rk), dv=rel(r.dvh.float(), rv))
    fin = torch.isfinite(rl)
    assert torch.equal(torch.isfinite(r.lse.cpu()), fin), tag
    errs["lse"] = rel(r.lse.cpu()[fin], rl[fin])
    print(tag, "kernel vs float64:", {k: "%.2e" % e for k, e in errs.items()})
    assert errs["o"] < O_TOL and errs["lse"] < LSE_TOL, (tag, errs)
    assert errs["dq"] < G_TOL and errs["dk"] < G_TOL and errs["dv"] < G_TOL, (tag, errs)


def _check_input_condition(model, ref, tag=""):
    """bf16 arithmetic alone (rounding_model, no kernel involved) stays within HALF of each bound on these inputs"""
    errs = dict(o=rel(model[0], ref[0]), dq=rel(model[2], ref[2]), dk=rel(model[3], ref[3]), dv=rel(model[4], ref[4]))
    print(tag, "rounding model vs float64:", {k: "%.2e" % e for k, e in errs.items()})
    assert errs["o"] < O_TOL / 2 and max(errs["dq"], errs["dk"], errs["dv"]) < G_TOL / 2, (tag, errs)


def _engine_ids():
    out = []
    for dh, H, B in HEADS:
        for T, S, causal in ENGINE_GEOMS:
            for p in (0.0, 0.3):
                for forced in ((False, True) if max(T, S) <= 128 else (False,)):
                    name = f"dh{dh}-{T}x{S}-{'causal' if causal else 'full'}-p{p}" + ("-streaming_forced" if forced else "")
                    out.append(pytest.param(dh, H, B, T, S, causal, p, forced, id=name))
    return out


@pytest.mark.parametrize("dh,H,B,T,S,causal,drop_p,forced", _engine_ids())
def test_flash_attention_engine_convention(backend, monkeypatch, dh, H, B, T, S, causal, drop_p, forced):
    """Packed layouts with pad columns, bf16-only O and gradients, partial-sum bias gradients, dropout in forward and
    backward: against the float64 reference with the call's own keep mask injected, at this file's bounds; nothing
    written outside the blocks and nothing left unwritten; a dense twin call with every fp32 output agrees bit for bit
    (strides and null pointers change no arithmetic); the partial rows sum to the fp32 gradients' column sums within
    fp32's worst-case summation error; a second call repeats bit for bit.  ``forced``: S2ST_ATTN_SHORT=0 sends the short
    lengths through the streaming kernels (same slots, same numbers within the same bounds)."""
    if backend.kind == "emu" and ((dh, T, S, causal, drop_p) not in EMU_CASES or forced):
        pytest.skip("the emulator runs six geometries; the sweep runs on the GPU (the CPU suite's time budget)")
    bd, d = backend.bd, backend.device
    if forced:
        monkeypatch.setenv("S2ST_ATTN_SHORT", "0")  # (read per call)
    Cm = H * dh
    tag = f"[dh{dh} {T}x{S} causal={causal} p={drop_p} forced={forced}]"
    klen = torch.tensor(_engine_klens(S, drop_p > 0), dtype=torch.int32)
    q, k, v, dO = _inputs(B, T, S, Cm, 7919 * T + 31 * S + dh + causal)
    seed, ld_drop = 4242 + T, (S + 7) // 8 * 8
    layout = "self" if T == S else "cross"
    kw = dict(klen=klen.to(d), causal=causal, drop_p=drop_p, seed=seed, dO=dO.to(d), bf16_o=True, bf16_grads=True, full=True)

    def engine_call():
        r = bd.flash_attention(q.to(d), k.to(d), v.to(d), H, layout=layout, pad=PAD, f32_o=False, f32_grads=False,
                               db="parts", **kw)
        backend.sync()
        return r

    r = engine_call()
    assert r.o is None and r.dq is None and r.dk is None and r.dv is None
    assert r.bufs["in_kvq" if layout == "self" else "in_kv"].stride(1) == (3 if layout == "self" else 2) * Cm + PAD

    # 1. the exact reference, the call's keep mask injected
    keep = dropout_keep(backend, B, H, T, S, ld_drop, drop_p, seed)
    dOh = dO.to(torch.bfloat16).float()
    ref = reference(q.float(), k.float(), v.float(), H, klen, causal, dOh, keep=keep)
    _check_against_reference(r, ref, tag)
    # 2. the inputs leave the kernels room: bf16 arithmetic alone is within half of every bound
    _check_input_condition(rounding_model(q.float(), k.float(), v.float(), H, klen, causal, dOh, keep=keep), ref, tag)

    # 3. no stray writes, nothing unwritten
    _pads_untouched(bd, r, PAD)
    for name in ("oh", "lse", "dqh", "dkh", "dvh", "db_part"):
        assert _no_sentinel(bd, getattr(r, name)), (tag, name)
    for b in range(B):
        kl = int(klen[b])
        if kl < S:
            assert float(r.dkh[b, kl:].float().abs().max()) == 0.0 and float(r.dvh[b, kl:].float().abs().max()) == 0.0, (tag, b)
    for name in ("dbq", "dbk", "dbv"):
        assert bool((getattr(r, name).cpu() == bd.DB_SENTINEL).all()), (tag, name)
    nblk = lambda n: (n + 63) // 64 * 4  # blocks of 64 columns, 4 waves each
    assert (r.slots_q, r.slots_k) == (B * nblk(T), B * nblk(S))
    assert r.dbq_part.shape == (r.slots_q, Cm) and r.dbk_part.shape == r.dbv_part.shape == (r.slots_k, Cm)

    # 4. the dense twin with fp32 O and fp32 gradients as well, bias gradients in the atomic form
    t = bd.flash_attention(q.to(d), k.to(d), v.to(d), H, db="atomic", **kw)
    backend.sync()
    for name in ("oh", "lse", "dqh", "dkh", "dvh"):
        assert _bits_equal(getattr(r, name), getattr(t, name)), (tag, name)
    for full, half in ((t.o, t.oh), (t.dq, t.dqh), (t.dk, t.dkh), (t.dv, t.dvh)):
        assert _bits_equal(full.to(torch.bfloat16), half), tag

    # 5. bias gradients: |sum of the partial rows - sum of the fp32 gradient| <= n 2^-24 sum|terms| (any order of fp32
    # additions of n terms is within (n - 1) u sum|terms| of the exact sum, u = 2^-24); the atomic form likewise
    for full, part, atomic, name in ((t.dq, r.dbq_part, t.dbq, "dbq"), (t.dk, r.dbk_part, t.dbk, "dbk"), (t.dv, r.dbv_part, t.dbv, "dbv")):
        g64 = full.cpu().double()
        exact, mag = g64.sum(dim=(0, 1)), g64.abs().sum(dim=(0, 1))
        bound = g64.shape[0] * g64.shape[1] * 2.0 ** -24 * mag
        e_part = (part.cpu().double().sum(dim=0) - exact).abs()
        e_atom = (atomic.cpu().double() - exact).abs()
        print(tag, name, "worst error / bound: parts %.3f atomic %.3f" % (float((e_part / bound).max()), float((e_atom / bound).max())))
        assert bool((e_part <= bound).all()), (tag, name, "partial sums")
        assert bool((e_atom <= bound).all()), (tag, name, "atomic")

    # 6. no atomics on the engine's path: a second call repeats bit for bit
    r2 = engine_call()
    for name in ("oh", "lse", "dqh", "dkh", "dvh", "db_part"):
        assert _bits_equal(getattr(r, name), getattr(r2, name)), (tag, name)


EDGE_GEOMS = [(40, 100), (129, 140)]  # one short, one streaming
EDGE_HEADS = [(64, 2), (128, 1)]


def _edge_call(backend, q, k, v, dO, H, **kw):
    """cross-packed, bf16-only outputs, partial sums: the engine's cross-attention call"""
    d = backend.device
    klen = kw.pop("klen", None)
    r = backend.bd.flash_attention(q.to(d), k.to(d), v.to(d), H, klen=None if klen is None else klen.to(d), dO=dO.to(d),
                                   layout="cross", pad=PAD, bf16_o=True, bf16_grads=True, f32_o=False, f32_grads=False,
                                   db="parts", full=True, **kw)
    backend.sync()
    return r


@pytest.mark.parametrize("T,S", EDGE_GEOMS, ids=[f"{t}x{s}" for t, s in EDGE_GEOMS])
@pytest.mark.parametrize("dh,H", EDGE_HEADS)
def test_flash_attention_key_length_edges(backend, dh, H, T, S):
    """klen = 0: O rows zero, lse = -inf, zero gradients and no NaN anywhere (the reference treats that element apart:
    the softmax of an empty row is NaN); klen = 1; klen > S is klen = S, bit for bit; klen = NULL is klen = S."""
    if backend.kind == "emu" and (dh, T) != (64, 40):
        pytest.skip("the emulator runs one geometry (the CPU suite's time budget)")
    bd = backend.bd
    Cm = H * dh
    q, k, v, dO = _inputs(4, T, S, Cm, 100 * T + dh)
    dOh = dO.to(torch.bfloat16).float()
    klen = torch.tensor([0, 1, S + 5, S], dtype=torch.int32)
    r = _edge_call(backend, q, k, v, dO, H, klen=klen)
    ref = reference(q.float(), k.float(), v.float(), H, klen, False, dOh)
    _check_against_reference(r, ref)
    _check_input_condition(rounding_model(q.float(), k.float(), v.float(), H, klen, False, dOh), ref)
    _pads_untouched(bd, r, PAD)
    for name in ("oh", "dqh", "dkh", "dvh", "db_part"):
        assert _no_sentinel(bd, getattr(r, name)), name
    assert not bool(torch.isnan(r.lse.cpu()).any())
    assert bool((r.lse[0].cpu() == float("-inf")).all()) and bool(torch.isfinite(r.lse[1:].cpu()).all())
    for name in ("oh", "dqh", "dkh", "dvh"):
        assert float(getattr(r, name)[0].float().abs().max()) == 0.0, name
    assert float(r.dkh[1, 1:].float().abs().max()) == 0.0 and float(r.dvh[1, 1:].float().abs().max()) == 0.0
    clipped = _edge_call(backend, q, k, v, dO, H, klen=torch.tensor([0, 1, S, S], dtype=torch.int32))
    for name in ("oh", "lse", "dqh", "dkh", "dvh", "db_part"):
        assert _bits_equal(getattr(r, name), getattr(clipped, name)), name
    none = _edge_call(backend, q, k, v, dO, H)
    full = _edge_call(backend, q, k, v, dO, H, klen=torch.full((4,), S, dtype=torch.int32))
    _check_against_reference(none, reference(q.float(), k.float(), v.float(), H, None, False, dOh))
    for name in ("oh", "lse", "dqh", "dkh", "dvh", "db_part"):
        assert _bits_equal(none.__dict__[name], full.__dict__[name]), name


@pytest.mark.parametrize("dh,H", EDGE_HEADS)
def test_flash_attention_one_query(backend, dh, H):
    """T = 1, S = 100: one query row in a 16-row wave tile"""
    q, k, v, dO = _inputs(3, 1, 100, H * dh, dh + 1)
    dOh = dO.to(torch.bfloat16).float()
    klen = torch.tensor([100, 91, 64], dtype=torch.int32)
    r = _edge_call(backend, q, k, v, dO, H, klen=klen)
    ref = reference(q.float(), k.float(), v.float(), H, klen, False, dOh)
    _check_against_reference(r, ref)
    _check_input_condition(rounding_model(q.float(), k.float(), v.float(), H, klen, False, dOh), ref)
    _pads_untouched(backend.bd, r, PAD)
    for name in ("oh", "lse", "dqh", "dkh", "dvh", "db_part"):
        assert _no_sentinel(backend.bd, getattr(r, name)), name


@pytest.mark.parametrize("dh,H", EDGE_HEADS)
def test_flash_attention_one_key(backend, dh, H):
    """S = 1, T = 40: P = 1, so O = v and dv = sum of dO; dS = P (dP - D) is zero in exact arithmetic (D = dO . O = dP), so dq
    and dk are pure rounding residue and are bounded absolutely: dP and D are both fp32 sums of the SAME dh products of
    bf16 values (O = v exactly here) in different orders, so |dP - D| <= 2 dh 2^-24 sum|dO_i v_i|; dq = scale dS k,
    dk = scale sum_t dS_t q_t."""
    T, S = 40, 1
    q, k, v, dO = _inputs(3, T, S, H * dh, dh + 2)
    dOh = dO.to(torch.bfloat16).float()
    r = _edge_call(backend, q, k, v, dO, H)
    ro, rl, rq, rk, rv = reference(q.float(), k.float(), v.float(), H, None, False, dOh)
    assert rel(r.oh.float(), ro) < O_TOL and rel(r.lse, rl) < LSE_TOL and rel(r.dvh.float(), rv) < G_TOL
    scale = dh ** -0.5
    ds_max = 2 * dh * 2.0 ** -24 * float((dOh.double().abs().view(3, T, H, dh) * v.double().abs().view(3, 1, H, dh)).sum(-1).max())
    slack = 1 + 2.0 ** -7  # dS and the stored gradients are rounded to bf16
    assert float(r.dqh.float().abs().max()) <= slack * scale * ds_max * float(k.float().abs().max())
    assert float(r.dkh.float().abs().max()) <= slack * scale * ds_max * T * float(q.float().abs().max())
    _pads_untouched(backend.bd, r, PAD)
    for name in ("oh", "lse", "dqh", "dkh", "dvh", "db_part"):
        assert _no_sentinel(backend.bd, getattr(r, name)), name


@pytest.mark.parametrize("T,S", EDGE_GEOMS, ids=[f"{t}x{s}" for t, s in EDGE_GEOMS])
@pytest.mark.parametrize("dh,H", EDGE_HEADS)
def test_flash_attention_explicit_scale(backend, dh, H, T, S):
    """scale = 0.2 instead of dh^-0.5: forward scores and both places of the backward (dK and dQ accumulators)"""
    if backend.kind == "emu" and (dh, T) != (128, 40):
        pytest.skip("the emulator runs one geometry (the CPU suite's time budget)")
    q, k, v, dO = _inputs(2, T, S, H * dh, 10 * T + dh)
    dOh = dO.to(torch.bfloat16).float()
    klen = torch.tensor([S, S - 9], dtype=torch.int32)
    r = _edge_call(backend, q, k, v, dO, H, klen=klen, scale=0.2)
    ref = reference(q.float(), k.float(), v.float(), H, klen, False, dOh, scale=0.2)
    _check_against_reference(r, ref)
    _check_input_condition(rounding_model(q.float(), k.float(), v.float(), H, klen, False, dOh, scale=0.2), ref)
    assert rel(reference(q.float(), k.float(), v.float(), H, klen, False)[0], ref[0]) > 10 * O_TOL  # the scale matters here


@pytest.mark.parametrize("T", [40, 129], ids=["short", "streaming"])
@pytest.mark.parametrize("dh,H", EDGE_HEADS)
def test_flash_attention_dropout_index_space(backend, dh, H, T):
    """p 0.3, S = 45, ld_drop = 64: the mask of element (b, h, t, s) is drop(seed, ((b H + h) T + t) ld_drop + s) in forward
    and backward -- the row stride of the index space is ld_drop, not S and not S rounded up to 8"""
    if backend.kind == "emu" and (dh, T) != (64, 40):
        pytest.skip("the emulator runs one geometry (the CPU suite's time budget)")
    B, S, ld_drop, p, seed = 2, 45, 64, 0.3, 77
    q, k, v, dO = _inputs(B, T, S, H * dh, 3 * T + dh)
    dOh = dO.to(torch.bfloat16).float()
    klen = torch.tensor([S, S - 9], dtype=torch.int32)
    r = _edge_call(backend, q, k, v, dO, H, klen=klen, drop_p=p, seed=seed, ld_drop=ld_drop)
    keep = dropout_keep(backend, B, H, T, S, ld_drop, p, seed)
    ref = reference(q.float(), k.float(), v.float(), H, klen, False, dOh, keep=keep)
    _check_against_reference(r, ref)
    _check_input_condition(rounding_model(q.float(), k.float(), v.float(), H, klen, False, dOh, keep=keep), ref)
    wrong = reference(q.float(), k.float(), v.float(), H, klen, False, dOh, keep=dropout_keep(backend, B, H, T, S, 48, p, seed))
    assert rel(wrong[0], ref[0]) > 10 * O_TOL  # the two index spaces give different masks


def _refusal_cases():
    off = lambda a: a.q + 2  # one bf16 element
    return [
        pytest.param(dict(dh=32), id="dh32"),
        pytest.param(dict(dh=96), id="dh96"),
        pytest.param(dict(override={"ldq": lambda a: a.ldq + 4}), id="ldq_not_multiple_of_8"),
        pytest.param(dict(override={"q": off}), id="q_offset_by_one_element"),
        pytest.param(dict(override={"lse": None}), id="no_lse"),
        pytest.param(dict(override={"o": None, "oh": None}), id="no_o_at_all"),
        pytest.param(dict(override_bwd={"doh": None}), id="bwd_without_doh"),
        pytest.param(dict(override_bwd={"dO": None}, bf16_o=False), id="bwd_without_bf16_o_and_dO"),
    ]


@pytest.mark.parametrize("case", _refusal_cases())
def test_flash_attention_refusals(backend, case):
    """What the launchers refuse (S2ST_ERR_ARG) they refuse before launching anything: every output keeps its sentinel"""
    bd, d = backend.bd, backend.device
    case = dict(case)
    dh = case.pop("dh", 64)
    H, B, T, S = 2, 2, 40, 48
    q, k, v, dO = _inputs(B, T, S, H * dh, dh)
    kw = dict(dO=dO.to(d), bf16_o=True, bf16_grads=True, db="parts", full=True)
    kw.update(case)
    with pytest.raises(bd.S2STHipError, match="code %d$" % S2ST_ERR_ARG) as ei:
        bd.flash_attention(q.to(d), k.to(d), v.to(d), H, **kw)
    backend.sync()
    r = ei.value.outputs
    in_bwd = "override_bwd" in case
    assert ("bwd" in str(ei.value)) == in_bwd

    def untouched(t, fill):
        t = t.float().cpu()
        return bool(torch.isnan(t).all()) if fill != fill else bool((t == fill).all())

    nan = float("nan")
    if not in_bwd:
        assert untouched(r.o, nan) and untouched(r.lse, nan) and (r.oh is None or untouched(r.oh, bd.BF16_SENTINEL))
        return
    for name in ("dq", "dk", "dv"):
        assert untouched(getattr(r, name), nan) and untouched(getattr(r, name + "h"), bd.BF16_SENTINEL), name
    for name in ("dbq", "dbk", "dbv"):
        assert untouched(getattr(r, name), bd.DB_SENTINEL), name
    assert untouched(r.db_part, nan)
