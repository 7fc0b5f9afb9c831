"""Host logic: C-ABI exports, plugin registry surface, trainer arithmetic vs the oracle and the
reference goldens (through the emulator build on CPU, the product library on GPU)."""
import ctypes
import importlib
import math
import os

import numpy as np
import pytest
import torch

import s2st_oracle as O
from configs import CONFIGS, golden_sample
from synth_weights import load_synth
from test_engine import MICRO, NANO, nano_batches

PKG = "speech-to-speech-translation_amd"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_c_abi_exports_every_declared_symbol():
    """The product .so loads on a CPU-only host and exports every symbol include/s2st_hip.h
    declares (no compute calls without a GPU)."""
    bd = importlib.import_module(PKG + ".runtime.binding")
    assert os.path.exists(bd.DEFAULT_LIB), "run __graft_entry__.build() first"
    lib = ctypes.CDLL(bd.DEFAULT_LIB)
    protos = bd.header_prototypes()
    assert len(protos) >= 40
    for name in protos:
        assert hasattr(lib, name), name
    assert lib.s2st_version() >= 100


def test_engine_header_compiles_alone_and_no_struct_fragments(tmp_path):
    """csrc/engine.h is a real header: a unit that includes nothing else passes the emulator build's compiler
    (tests/hipemu/build_emu.sh: its compiler, its include paths and defines) with -fsyntax-only.  And no file of csrc/
    is pasted into a struct body again: an indented ``#include "..."`` of a project file is what that looked like."""
    import re
    import subprocess
    csrc = os.path.join(ROOT, PKG, "csrc")
    here = os.path.join(ROOT, "tests", "hipemu")
    script = open(os.path.join(here, "build_emu.sh")).read()
    m_cxx = re.search(r"^CXX=(\S+)$", script, re.M)
    m_flags = re.search(r'^FLAGS="([^"]*)"$', script, re.M)
    assert m_cxx and m_flags, "build_emu.sh no longer has one-line CXX= / FLAGS=\"...\": teach this test its new form"
    cxx = m_cxx.group(1)
    flags = m_flags.group(1).replace("$HERE", here).replace("$SRC", csrc).replace("$ROOT", ROOT).split()
    assert any(f.startswith("-I") for f in flags)
    probe = tmp_path / "engine_h_alone.cpp"
    probe.write_text('#include "engine.h"\nint main() { return 0; }\n')
    r = subprocess.run([cxx] + flags + ["-x", "c++", "-fsyntax-only", str(probe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    # (deliberately strict: an include of a project file indented inside an #if block is rejected too -- csrc/ keeps its
    #  includes at column 0, and a scan that tracked braces would be more machinery than the rule is worth)
    pasted = []
    for f in sorted(os.listdir(csrc)):
        path = os.path.join(csrc, f)
        if os.path.isfile(path) and f.endswith((".h", ".cpp", ".hip")):
            for n, line in enumerate(open(path, errors="replace"), 1):
                if re.match(r'\s+#include "', line):
                    pasted.append("%s:%d" % (f, n))
    assert not pasted, pasted


@pytest.mark.parametrize("backend", ["emu"], indirect=True)
def test_every_called_entry_point_is_declared_and_bound(backend):
    """The package reaches the library only through names include/s2st_hip.h declares (``lib.<name>``,
    ``bd.call("<name>")``), and load_library gives every exported declared function its header signature."""
    import re
    bd = backend.bd
    protos = bd.header_prototypes()
    called = set()
    for dirpath, _, files in os.walk(os.path.join(ROOT, PKG)):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                called |= set(re.findall(r"\blib(?:\(\))?\.(s2st_\w+)", src))
                called |= set(re.findall(r"\b(?:call|_bind)\(\s*\"(s2st_\w+)\"", src))
    assert len(called) >= 60 and "s2st_engine_side_stream" in called
    assert not called - set(protos), sorted(called - set(protos))
    prev = (bd._lib, bd._lib_is_emulator)
    try:
        lib = bd.load_library(os.path.join(ROOT, "tests", "hipemu", "_build", "libs2st_emu.so"), emulator=True)
        exported = [n for n in protos if hasattr(lib, n)]
        assert len(exported) >= 100
        for name in exported:
            ret, args = protos[name]
            fn = getattr(lib, name)
            assert fn.argtypes == [t for t, _ in args] and fn.restype is ret, name
    finally:
        bd._lib, bd._lib_is_emulator = prev


def test_no_cpu_fallback():
    """Product binding refuses CPU tensors (only the test-suite may load the emulator build)."""
    bd = importlib.import_module(PKG + ".runtime.binding")
    prev = (bd._lib, bd._lib_is_emulator)
    try:
        bd.load_library(bd.DEFAULT_LIB, emulator=False)
        x = torch.zeros(4, 4)
        with pytest.raises(bd.S2STHipError):
            bd.call("s2st_layernorm_fwd_f32", x, x, x, x, x, x, 4, 4, 1e-5)
    finally:
        bd._lib, bd._lib_is_emulator = prev


def test_registry_names():
    reg = importlib.import_module(PKG + ".registry")
    importlib.import_module(PKG + ".tasks")
    importlib.import_module(PKG + ".models")
    importlib.import_module(PKG + ".criterions")
    assert "s2s_translation" in reg.TASKS
    assert "s2st_transformer" in reg.MODELS and "s2st_transformer" in reg.ARCHS
    assert "s2st_loss" in reg.CRITERIA
    assert reg.CRITERIA["s2st_loss"].logging_outputs_can_be_summed() is False


def test_base_architecture_defaults():
    import argparse
    models = importlib.import_module(PKG + ".models")
    a = models.base_architecture(argparse.Namespace(conv_channels=512))
    ref = O.make_args()
    for k in ("dropout", "encoder_transformer_layers", "encoder_embed_dim", "encoder_ffn_embed_dim",
              "decoder_transformer_layers", "prenet_dim", "postnet_conv_dim", "asr_decoder_embed_dim",
              "conv_kernel_sizes", "middle_layers", "decoder_normalize_before", "encoder_normalize_before"):
        assert getattr(a, k) == getattr(ref, k), k
    assert a.conv_channels == 1024  # reference quirk: --conv-channels is ignored


def _build(backend, cfg, **extra):
    tasks = importlib.import_module(PKG + ".tasks")
    tr = importlib.import_module(PKG + ".trainer")
    a = O.make_args(**cfg)
    a.precise_gemm = True
    a.report_accuracy = True
    for k, v in extra.items():
        setattr(a, k, v)
    task = tasks.S2ST_TranslationTask.setup_task(a, device=backend.device)
    model = task.build_model(a)
    load_synth(model, 0)
    crit = task.build_criterion(a)
    return a, task, model, crit, tr.Trainer(a, task, model, crit)


def test_model_state_dict_and_forward_structure(backend):
    a, task, model, crit, trainer = _build(backend, NANO)
    m = O.S2STModel(a)
    assert set(model.state_dict().keys()) == set(m.state_dict().keys())
    for k, v in m.state_dict().items():
        assert tuple(model.state_dict()[k].shape) == tuple(v.shape), k
    s = nano_batches()[0]
    ni = s["net_input"]
    model.eval()
    out = model(ni["src_speech"], ni["src_speech_lens"], None, None, ni["prev_output_tokens"],
                target_lengths=s["target_lengths"], prev_src_text_tokens=ni["prev_src_text_tokens"],
                prev_tgt_text_tokens=ni["prev_tgt_text_tokens"])
    (post, eos, extra), asr, st = out
    B, Dm = ni["prev_output_tokens"].shape[:2]
    assert post.shape == (B, Dm, 320) and eos.shape == (B, Dm, 1)
    assert extra["feature_out"].shape == post.shape and extra["attn"].shape[0] == B
    assert asr[0].shape == (B, ni["prev_src_text_tokens"].shape[1], a.src_vocab_size) and asr[1] is None
    assert st[0].shape[-1] == a.tgt_vocab_size
    # eval mode = BatchNorm running stats, dropouts off: compare with the oracle in eval mode
    load_synth(m, 0)
    m.eval()
    (rp, re_, rx), rasr, rst, _ = m(ni["src_speech"], ni["src_speech_lens"], ni["prev_output_tokens"],
                                    s["target_lengths"], ni["prev_src_text_tokens"], ni["prev_tgt_text_tokens"])
    backend.sync()
    for x, y in ((post, rp), (eos, re_), (extra["feature_out"], rx["feature_out"]), (asr[0], rasr)):
        assert float((x.cpu() - y).abs().max()) < 3e-4 * float(y.abs().max())


@pytest.mark.parametrize("fast", [True, False])
def test_train_steps_match_oracle(backend, fast):
    """fwd, bwd, grads * 1/sample_size, clip, fairseq-Adam, inverse-sqrt LR over 3 updates; the
    `fast=False` leg goes through task.train_step / loss.backward() like fairseq would."""
    a, task, model, crit, trainer = _build(backend, NANO, lr=1e-3, warmup_updates=2, clip_norm=0.02)
    m = O.S2STModel(a)
    load_synth(m, 0)
    opt = O.FairseqAdam(m.parameters())
    batches = nano_batches()
    for u in range(3):
        s = batches[u % 2]
        r = trainer.train_step([s], fast=fast)
        lo, gn, lr, log, _ = O.train_step(m, opt, s, u, 1e-3, 2, 0.02)
        backend.sync()
        assert abs(float(r["logs"][0]["loss"]) - float(lo)) < 3e-5 * float(lo)
        assert abs(float(r["gnorm"]) - float(gn)) < 2e-3 * float(gn)
        assert abs(r["lr"] - lr) < 1e-12
        assert r["logs"][0]["asr_total"] == log["asr_total"]
    named = dict(m.named_parameters())
    for n, p in model.named_parameters():
        ref = named[n].detach()
        assert float((p.detach().cpu() - ref).abs().max()) < 2e-4 * (float(ref.abs().max()) + 1e-6), n
    red = crit.reduce_metrics([dict(r["logs"][0].items())])
    assert abs(red["loss"] - float(r["logs"][0]["loss"])) < 1e-6 and "asr_accuracy" in red


@pytest.mark.gpu
def test_tiny_golden_train_steps(backend, golden_dir):
    """3 updates of BASELINE configs[0] against numbers produced by the reference's own
    Adam / clip_grad_norm_ (tests/golden/s2st_tiny.npz)."""
    if backend.kind != "hip":
        pytest.skip("golden-size config runs on the GPU")
    z = np.load(os.path.join(golden_dir, "s2st_tiny.npz"))
    LR, WARM, CLIP, N = z["train.hparams"].tolist()
    a, task, model, crit, trainer = _build(backend, CONFIGS["tiny"], lr=LR, warmup_updates=int(WARM), clip_norm=CLIP)
    for u in range(int(N)):
        r = trainer.train_step([golden_sample("tiny", u % 2)])
        backend.sync()
        np.testing.assert_allclose(float(r["logs"][0]["loss"]), z["train.loss"][u], rtol=1e-4)
        np.testing.assert_allclose(float(r["gnorm"]), z["train.gnorm"][u], rtol=1e-2)
        np.testing.assert_allclose(r["lr"], z["train.lr"][u], rtol=1e-12)
    pn = dict(zip(z["train.param_norm_names"].tolist(), z["train.param_norms"].tolist()))
    for n, p in model.named_parameters():
        np.testing.assert_allclose(float(p.detach().norm()), pn[n], rtol=1e-4, err_msg=n)


def test_use_hubert_front_end_feeds_the_encoder(backend):
    """Config 4 wiring (s2st_transformer.py:245-252): with --use-hubert the model runs the frozen HuBERT
    front end on the collated audio, and the encoder (first conv now hubert_hidden wide) consumes its
    features with the frame-level lengths.  Compared with oracle HuBERT -> oracle S2ST model."""
    import hubert_oracle as HO
    geo = dict(HO.TINY)
    cfg = dict(NANO, use_hubert="true", hubert_hidden=geo["embed"])
    a, task, model, crit, trainer = _build(backend, cfg, hubert_geometry=geo)
    assert model.hubert is not None and model.engine.cfg.in_dim == geo["embed"]
    model.hubert.load_state_dict(HO.synth_state(geo))
    a2 = O.make_args(**cfg)
    a2._hubert_input = True
    m = O.S2STModel(a2)
    load_synth(m, 0)
    m.eval()
    model.eval()
    wave, pad, _ = HO.synth_audio(2, 9000, 5)
    s = nano_batches()[0]
    ni = s["net_input"]
    out = model(None, None, wave, pad, ni["prev_output_tokens"], target_lengths=s["target_lengths"],
                prev_src_text_tokens=ni["prev_src_text_tokens"], prev_tgt_text_tokens=ni["prev_tgt_text_tokens"])
    backend.sync()
    feats, fpm = HO.extract_features(HO.synth_state(geo), geo, wave, pad)
    lens = (~fpm).long().sum(-1)
    (rp, re_, rx), rasr, rst, _ = m(feats, lens, ni["prev_output_tokens"], s["target_lengths"],
                                    ni["prev_src_text_tokens"], ni["prev_tgt_text_tokens"])
    (post, eos, extra), asr, st = out
    for x, y in ((post, rp), (eos, re_), (asr[0], rasr)):
        assert float((x.cpu() - y).abs().max()) < 5e-4 * float(y.abs().max())


def test_prefetched_batches_train_like_inline_ones(backend):
    """runtime/prefetch.DevicePrefetcher (background thread + its own stream for Engine.prepare) feeds the trainer
    the same batches: identical losses and parameters as feeding the collated samples directly; an empty padding
    batch passes through to the trainer's dummy-batch handling."""
    P = importlib.import_module(PKG + ".runtime.prefetch")
    res = []
    for mode in ("inline", "prefetch"):
        a, task, model, crit, trainer = _build(backend, NANO, lr=1e-3, warmup_updates=2, clip_norm=0.02,
                                               dropout=0.1, attention_dropout=0.1)
        feed = nano_batches() + [nano_batches()[0]]
        src = iter(feed) if mode == "inline" else P.DevicePrefetcher(feed, model.engine, depth=2)
        losses = []
        for s in src:
            r = trainer.train_step([s])
            losses.append(float(r["logs"][0]["loss"]))
        backend.sync()
        res.append((losses, {n: p.detach().clone() for n, p in model.named_parameters()}))
    # (identical up to the summation-order noise of the atomics in the loss / bias-gradient reductions; parameters
    # with a mathematically zero gradient follow that noise through Adam's normalisation and are left out)
    assert all(abs(x - y) <= 1e-6 * abs(x) for x, y in zip(res[0][0], res[1][0]))
    for n, p in res[0][1].items():
        if not (n.endswith("k_proj.bias") or (".postnet.convolutions." in n and n.endswith(".0.bias"))):
            assert float((p - res[1][1][n]).abs().max()) <= 1e-6, n
    assert list(P.DevicePrefetcher([{}], None.__class__ and type("E", (), {"device": torch.device("cpu"), "prepare": None})()))[0] == {}


def _hubert_nano_setup(backend, **extra):
    import hubert_oracle as HO
    geo = dict(HO.TINY)
    cfg = dict(NANO, use_hubert="true", hubert_hidden=geo["embed"], ctc_weight=0.0)
    cfg.update(extra)
    a, task, model, crit, trainer = _build(backend, cfg, hubert_geometry=geo, lr=1e-3, warmup_updates=2,
                                           clip_norm=0.02)
    model.hubert.load_state_dict(HO.synth_state(geo))
    D = importlib.import_module(PKG + ".data")
    c = D.SyntheticFisherCorpus(n_utts=4, seed=3, max_src=64, median_src=50, min_src=40, with_audio=True)
    batches = []
    for ix in (range(2), range(2, 4)):
        s = c.collate_batch(ix)
        s["net_input"]["src_speech"] = None  # HuBERT mode: the collater hands over audio only
        batches.append(s)
    return geo, cfg, a, task, model, crit, trainer, batches


def _oracle_hubert_sample(geo, s):
    """What the reference encoder's HuBERT branch feeds its subsampler (oracle front end)."""
    import hubert_oracle as HO
    ni = s["net_input"]
    feats, fpm = HO.extract_features(HO.synth_state(geo), geo, ni["collated_audios_orig"], ni["padding_mask"])
    out = dict(s)
    out["net_input"] = dict(ni, src_speech=feats, src_speech_lens=(~fpm).long().sum(-1))
    return out


def test_use_hubert_training_steps_against_oracle(backend):
    """BASELINE.json configs[3] composed as a TRAINING step at nano size: frozen HuBERT front end -> encoder ->
    mel decoder + aux ASR/ST heads -> s2st_loss -> backward -> clip -> Adam, two updates, against oracle HuBERT ->
    oracle model / criterion / optimizer (s2st_transformer.py:245-252, s2st_loss.py:179-292)."""
    geo, cfg, a, task, model, crit, trainer, batches = _hubert_nano_setup(backend)
    a2 = O.make_args(**cfg)
    a2._hubert_input = True
    m = O.S2STModel(a2)
    load_synth(m, 0)
    m.train()
    opt = O.FairseqAdam(m.parameters())
    for u, s in enumerate(batches):
        r = trainer.train_step([s])
        backend.sync()
        loss, gn, lr, log, _ = O.train_step(m, opt, _oracle_hubert_sample(geo, s), u, 1e-3, 2, 0.02)
        assert abs(float(r["logs"][0]["loss"]) - float(loss)) < 1e-4 * abs(float(loss))
        assert abs(float(r["gnorm"]) - float(gn)) < 2e-3 * float(gn)
    ref = dict(m.named_parameters())
    for n, p in model.named_parameters():
        assert float((p.detach().cpu() - ref[n].detach()).abs().max()) < 2e-3 * float(ref[n].abs().max()) + 1e-5, n
    # the front end is frozen: no trainable parameter of the model belongs to it
    assert not any("hubert" in n for n, _ in model.named_parameters())
    # through the criterion / autograd node as fairseq would drive it
    loss, ss, log = crit(model, batches[0])
    assert ss == batches[0]["ntokens"] and math.isfinite(float(log["loss"]))


def test_hubert_front_end_ahead_of_the_step_gives_the_same_updates(backend):
    """--use-hubert: the frozen front end of batch i + 1 launched beside step i (model.front_end_ahead: second stream, the
    step only waits for an event; DevicePrefetcher does it with one batch of look-ahead) == the front end inside each step:
    same losses, same parameters -- HuBERT does not depend on the update.  On the CPU emulator the call is a pass-through
    (nothing to overlap: skipped there); on the GPU the three loops differ."""
    if backend.kind == "emu":
        pytest.skip("no second stream on the emulator: front_end_ahead is a pass-through")
    P = importlib.import_module(PKG + ".runtime.prefetch")
    res = []
    for mode in ("inline", "ahead", "prefetcher"):
        geo, cfg, a, task, model, crit, trainer, batches = _hubert_nano_setup(backend)
        feed = batches + [batches[0], batches[1]]
        losses = []
        if mode == "prefetcher":
            for s in P.DevicePrefetcher(feed, model.engine, depth=2, model=model):
                losses.append(float(trainer.train_step([s])["logs"][0]["loss"]))
        else:
            prepared = [model.prepare_sample(s, training=True) for s in feed]
            for i, pb in enumerate(prepared):
                if mode == "ahead" and i + 1 < len(prepared):
                    model.front_end_ahead(prepared[i + 1])
                    if backend.kind == "hip":
                        assert prepared[i + 1].fe_ready is not None
                losses.append(float(trainer.train_step([pb])["logs"][0]["loss"]))
                assert getattr(pb, "fe_ready", None) is None  # (consumed by the step)
        backend.sync()
        res.append((losses, {n: p.detach().clone() for n, p in model.named_parameters()}))
    for other in res[1:]:
        assert all(abs(x - y) <= 1e-6 * abs(x) for x, y in zip(res[0][0], other[0])), (res[0][0], other[0])
        for n, p in res[0][1].items():
            if not (n.endswith("k_proj.bias") or (".postnet.convolutions." in n and n.endswith(".0.bias"))):
                assert float((p - other[1][n]).abs().max()) <= 1e-6, n


def test_use_hubert_with_ctc_fails_like_the_reference(backend):
    """s2st_loss.py:231-232 derives the CTC input lengths from the fbank lengths (100 fps) although the
    encoder ran on HuBERT frames (50 fps); F.ctc_loss then raises 'Expected input_lengths to have value at most E'
    in the reference (reproduced with the reference itself, oracle/gen_golden_hubert_train.py).  Same error here."""
    geo, cfg, a, task, model, crit, trainer, batches = _hubert_nano_setup(backend, ctc_weight=0.3)
    with pytest.raises(RuntimeError, match="Expected input_lengths to have value at most"):
        trainer.train_step([batches[0]])
