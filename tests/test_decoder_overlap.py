"""S2ST_DEC_OVERLAP (csrc/engine.h, engine_step.cpp): mel-decoder work that does not depend on the encoder -- the prenet,
the positions, layer 0's self-attention block and cross-attention query projection in the forward; everything of layer 0
below its cross-attention's dK|dV in the backward -- is issued on the engine's second stream, beside the encoder.  The same kernels run with the same arguments; only the stream and the place in the
enqueue order differ.  So a step with the overlap (mask 3, the default; 1 / 2 = its two pieces alone) must be the
step without it (mask 0) BIT FOR BIT: every loss term, every forward output, the whole gradient arena, the BatchNorm
running statistics, the dropout-site log (names, seeds, geometry, order) and the segment ranges the gradient exchange
reads.  On the emulator every launch is synchronous, so what is checked there is the re-ordered issue (site numbers,
tape, marks, accumulation order); the races a wrong event would leave are what the GPU tests are for.  Every step also
asserts which pieces the engine reports as engaged (``dec_overlap_active``): the mask asked for in the bf16-operand mode,
none for mask 0 -- so the equalities are about the new path and not about a switch that quietly stayed off.

The bf16x3 ("precise") mode owns no second stream, so both settings issue the identical launch sequence there (the
engine reports nothing engaged, which is asserted: the mode's cases check the fallback, not the overlap).  Its
gradient arena does not repeat ITSELF bit for bit (the fp32-operand GEMM splits K with atomics: two runs with the overlap
off differ by 5.0e-6 of the arena's norm on the emulator, 904732 of 1350144 elements), so in that mode the arena is held
to the 2e-5 that tests/test_full_size.py uses for the same reason; everything else is compared bit for bit there too."""
import importlib

import numpy as np
import pytest
import torch

import s2st_oracle as O
from configs import CONFIGS, golden_sample
from test_engine import DATA, ENG, MICRO, MICRO_POSTLN, NANO, make_engine, nano_batches

RECIPE_DROP = dict(dropout=0.1, attention_dropout=0.1, activation_dropout=0.01, prenet_dropout=0.5, postnet_dropout=0.5)


def _sites(e):
    return [(name, int(r.seed), int(r.kind), float(r.p), tuple(int(d) for d in r.dims))
            for name, r in e.dropout_sites().items()]


def _step(backend, e, sample, mask, monkeypatch, seed=9):
    """One training step under S2ST_DEC_OVERLAP=mask (read per call) -> everything the step leaves behind."""
    monkeypatch.setenv("S2ST_DEC_OVERLAP", str(mask))
    e.buffers.copy_(e._buf0)
    e.site_log(True)
    o = e.forward(sample, training=True, want_attn=True, seed=seed)
    e.zero_grad()
    e.backward(1.0)
    backend.sync()
    assert e.dec_overlap_active() == (0 if e.cfg.precise else mask), (mask, e.dec_overlap_active())
    outs = {k: v.clone() for k, v in o.items() if torch.is_tensor(v)}
    segs = [e.segment_range(i) for i in range(e.num_segments())]
    return outs, e.grads.clone(), e.buffers.clone(), _sites(e), segs


def _same_step(a, b, tag, precise=False):
    (oa, ga, ba, sa, ra), (ob, gb, bb, sb, rb) = a, b
    assert set(oa) == set(ob)
    assert torch.equal(oa["stats"], ob["stats"]), (tag, oa["stats"], ob["stats"])  # every loss term
    for k in oa:
        assert torch.equal(oa[k], ob[k]), (tag, k)
    if precise:  # (split-K atomics of the fp32-operand GEMM: see the module's docstring)
        assert float((ga - gb).norm()) <= 2e-5 * float(gb.norm()), (tag, float((ga - gb).norm()) / float(gb.norm()))
    else:
        assert torch.equal(ga, gb), (tag, int((ga != gb).sum()), float((ga - gb).norm()) / float(gb.norm()))
    assert torch.equal(ba, bb), tag  # BatchNorm running statistics
    assert sa == sb, (tag, [x for x, y in zip(sa, sb) if x != y][:4], len(sa), len(sb))
    assert ra == rb, (tag, ra, rb)


def _engine(backend, cfg, precise):
    a, e = make_engine(backend, cfg, precise)
    e._buf0 = e.buffers.clone()
    if not precise:  # (the bf16-operand mode owns a second stream, on the emulator as a label: the schedules do differ)
        assert e.lib.s2st_engine_side_stream(e.h), "no second stream: the comparison would be of a schedule with itself"
    return e


def _micro_sample():
    D = importlib.import_module(DATA)
    c = D.SyntheticFisherCorpus(n_utts=4, seed=3, max_src=64, median_src=50, min_src=30)
    return c.collate_batch(range(4))


@pytest.mark.parametrize("precise", [False, True], ids=["bf16", "bf16x3"])
@pytest.mark.parametrize("name", ["micro", "micro_postln", "tiny"])
def test_step_with_overlap_is_the_step_without(backend, name, precise, monkeypatch):
    """Micro (pre-LN with aux heads, post-LN) and tiny size, recipe dropouts on, both GEMM modes: overlap on against off,
    and each of its two pieces alone."""
    cfg = {"micro": MICRO, "micro_postln": MICRO_POSTLN, "tiny": CONFIGS["tiny"]}[name]
    sample = golden_sample("tiny", 0) if name == "tiny" else _micro_sample()
    e = _engine(backend, dict(cfg, **RECIPE_DROP), precise)
    off = _step(backend, e, sample, 0, monkeypatch)
    assert len(off[3]) > 10 and torch.isfinite(off[1]).all() and float(off[1].norm()) > 0
    for mask in ((3, 1, 2) if name == "micro" and not precise else (3,)):
        _same_step(_step(backend, e, sample, mask, monkeypatch), off, (name, precise, mask), precise)


def test_three_updates_with_overlap_end_on_the_same_parameters(backend, monkeypatch):
    """Three consecutive ``train_step``s with the overlapped optimizer update (its chunks sit on the second stream ahead of
    the decoder's front): bit-identical parameters and Adam moments with the overlap on and off."""
    PKG = ENG.rsplit(".runtime", 1)[0]
    tasks = importlib.import_module(PKG + ".tasks")
    tr = importlib.import_module(PKG + ".trainer")
    from synth_weights import load_synth
    if backend.kind == "hip":
        D = importlib.import_module(DATA)
        corpus = D.SyntheticFisherCorpus(n_utts=4096, seed=1234)
        bs = corpus.batches(max_tokens=20000, bsz_mult=8)
        order = np.random.RandomState(7).permutation(len(bs))
        cfg, batches = CONFIGS["base_recipe"], [corpus.collate_batch(bs[order[i]]) for i in range(3)]
    else:
        cfg, batches = dict(NANO, **RECIPE_DROP), nano_batches()
    runs = []
    for mask in (0, 3):
        monkeypatch.setenv("S2ST_DEC_OVERLAP", str(mask))
        a = O.make_args(**cfg)
        a.precise_gemm, a.lr, a.warmup_updates, a.clip_norm = False, 1e-3, 2, 0.05
        task = tasks.S2ST_TranslationTask.setup_task(a, device=backend.device)
        model = task.build_model(a)
        load_synth(model, 0)
        t = tr.Trainer(a, task, model, task.build_criterion(a))
        for u in range(3):
            t.train_step([batches[u % len(batches)]], overlap_optimizer=True)
        t.wait_optimizer()
        backend.sync()
        runs.append((model.engine.params.clone(), t.exp_avg.clone(), t.exp_avg_sq.clone(), int(t.skipped)))
        del t, model, task
    (p0, m0, v0, s0), (p1, m1, v1, s1) = runs
    assert s0 == s1 == 0 and torch.isfinite(p0).all()
    assert torch.equal(p0, p1), int((p0 != p1).sum())
    assert torch.equal(m0, m1) and torch.equal(v0, v1)


@pytest.fixture(scope="module")
def bench_batch():
    """One max-tokens batch of the bench corpus (the first of bench.py's shuffled order: 16 x 850 frames)."""
    D = importlib.import_module(DATA)
    corpus = D.SyntheticFisherCorpus(n_utts=4096, seed=1234)
    bs = corpus.batches(max_tokens=20000, bsz_mult=8)
    order = np.random.RandomState(7).permutation(len(bs))
    return corpus.collate_batch(bs[order[0]])


@pytest.mark.gpu
@pytest.mark.parametrize("precise", [False, True], ids=["bf16", "bf16x3"])
def test_base_size_step_with_overlap_is_the_step_without(backend, bench_batch, precise, monkeypatch):
    if backend.kind != "hip":
        pytest.skip("base size runs on the GPU")
    e = _engine(backend, CONFIGS["base_recipe"], precise)
    off = _step(backend, e, bench_batch, 0, monkeypatch, seed=11)
    assert torch.isfinite(off[1]).all()
    for mask in ((3, 1, 2) if not precise else (3,)):
        _same_step(_step(backend, e, bench_batch, mask, monkeypatch, seed=11), off, ("base", precise, mask), precise)


@pytest.mark.gpu
def test_twenty_repeats_of_a_base_size_step_give_the_same_gradients(backend, bench_batch, monkeypatch):
    """No race between the moved work and its consumers: 20 steps of the same batch from the same state, the overlap on,
    leave the same outputs and the same gradient arena each time."""
    if backend.kind != "hip":
        pytest.skip("base size runs on the GPU")
    e = _engine(backend, CONFIGS["base_recipe"], False)
    first = _step(backend, e, bench_batch, 3, monkeypatch, seed=11)
    for r in range(19):
        _same_step(_step(backend, e, bench_batch, 3, monkeypatch, seed=11), first, ("repeat", r))
