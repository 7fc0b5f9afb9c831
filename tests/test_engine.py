"""Whole-path parity: HIP engine (forward + s2st_loss + backward) against the CPU oracle and
the golden vectors captured from the reference.

* emulator backend (CPU, `-m "not gpu"`): a micro config, engine vs oracle -- checks the
  schedule / tape / layouts without a GPU.
* hip backend (`-m gpu`): BASELINE.json configs[0] (tiny) and configs[1] (base) against
  tests/golden/s2st_{tiny,tiny_postln,base}.npz and the oracle, in precise (bf16x3) mode with
  tight tolerances and in bf16 mode with the north-star tolerance (loss parity 1e-3).
"""
import importlib
import math
import os

import numpy as np
import pytest
import torch

import s2st_oracle as O
from configs import CONFIGS, golden_sample
from synth_weights import load_synth, synth_tensor

ENG = "speech-to-speech-translation_amd.runtime.engine"
DATA = "speech-to-speech-translation_amd.data"

MICRO = dict(
    encoder_transformer_layers=2, decoder_transformer_layers=2, encoder_embed_dim=64,
    decoder_embed_dim=64, encoder_ffn_embed_dim=128, decoder_ffn_embed_dim=128,
    encoder_attention_heads=4, decoder_attention_heads=4, encoder_normalize_before=True,
    decoder_normalize_before=True, prenet_dim=32, postnet_conv_dim=64, middle_layers="0,1",
    asr_decoder_layers=1, st_decoder_layers=1, asr_decoder_embed_dim=32, st_decoder_embed_dim=32,
    ctc_weight=0.3, asr_ce_weight=0.3, st_ce_weight=0.3, dropout=0.0, attention_dropout=0.0,
    activation_dropout=0.0, prenet_dropout=0.0, postnet_dropout=0.0)
MICRO_POSTLN = dict(MICRO, decoder_normalize_before=False, ctc_weight=0.0, asr_ce_weight=0.0,
                    st_ce_weight=0.0, middle_layers="0")

# smallest geometry that still exercises every op (host / distributed tests on the emulator)
NANO = dict(MICRO, encoder_transformer_layers=2, decoder_transformer_layers=1, encoder_embed_dim=32,
            decoder_embed_dim=32, encoder_ffn_embed_dim=64, decoder_ffn_embed_dim=64,
            encoder_attention_heads=2, decoder_attention_heads=2, prenet_dim=16, postnet_conv_dim=32,
            middle_layers="0,1", asr_decoder_embed_dim=16, st_decoder_embed_dim=16, postnet_layers=2)


def nano_batches():
    D = importlib.import_module(DATA)
    c = D.SyntheticFisherCorpus(n_utts=4, seed=3, max_src=44, median_src=40, min_src=30)
    return [c.collate_batch(range(2)), c.collate_batch(range(2, 4))]


LOSS_KEYS = [("loss", 16), ("l1_loss", 17), ("mse_loss", 18), ("eos_loss", 19), ("ctc_loss", 20),
             ("aux_asr_loss", 21), ("aux_st_loss", 22)]
SUB = 61


def _sub(x):
    x = np.asarray(x)
    return x if x.size <= 40000 else x.reshape(-1)[::SUB]


GRAD_STRIDE = 127


def gsub(x):
    """Sampling rule of the ``gsub.*`` golden entries (oracle/gen_golden.py): tensors up to 4096 elements whole,
    larger ones as flat[::127]."""
    x = np.asarray(x)
    return x.astype(np.float64) if x.size <= 4096 else x.reshape(-1)[::GRAD_STRIDE].astype(np.float64)


def bf16_tensor_bounds(golden_dir, fname="s2st_base_autocast.npz"):
    """Gradient-error bounds of the benchmarked bf16 mode at base size: not "what this path was measured
    at plus head-room" but what the REFERENCE's own mixed precision does to the same gradients.
    oracle/gen_golden_autocast.py runs the reference model + criterion on the golden batch under ``torch.autocast("cpu",
    bfloat16)`` and records, per tensor, the same Frobenius-relative error against the fp32 golden that
    check_gradient_direction computes (base batch: whole gradient 1.6e-2, worst tensors 8e-2 ... 1.1e-1, median 3.2e-2).
    The HIP path keeps fp32 results, residual stream and softmax where autocast rounds to bf16, so it is held to 1.5 x the
    reference-autocast figures:
      * the whole gradient, the median and the maximum over the tensors: 1.5 x the autocast run's;
      * every tensor: 1.5 x max(its own autocast error, the 90th percentile of the autocast errors).  A tensor's autocast
        error is ONE realisation of rounding noise, not a constant of the tensor -- the same tensor (first decoder layer's
        cross-attention k_proj.weight) measures 8.0e-2 on the base batch and 2.6e-2 on the HuBERT batch, while this path
        measures 4.9e-2 / 5.7e-2 on the two -- so a tensor is allowed what autocast does to its typically-worst tensors;
      * the floor is the bf16x3 (fp32-accurate) mode's own bound, 5e-3.
    Returns (per-tensor bound, whole-gradient bound, the per-tensor autocast errors)."""
    z = np.load(os.path.join(golden_dir, fname))
    ac = dict(zip(z["names"].tolist(), z["err"].tolist()))
    p90 = float(np.quantile(z["err"], 0.9))
    return (lambda n: max(1.5 * max(ac[n], p90), 5e-3)), 1.5 * float(z["whole"]), ac


def check_gradient_direction(named_grads, z, per_tensor_tol, whole_tol, tag="", yardstick=None):
    """Every gradient tensor against the reference's sampled gradient (``gsub.<name>``): Frobenius-relative
    difference of the samples per tensor (a gradient with the right norm and the wrong direction fails), and of the
    concatenation of all samples.  The floor (1e-3 of the largest tensor norm, spread over the sample) covers
    tensors whose gradient is mathematically zero (k_proj biases: softmax shift invariance)."""
    names = [k[5:] for k in z.files if k.startswith("gsub.")]
    assert len(names) > 100 or tag == "tiny"
    gmax = max(float(np.linalg.norm(z["gsub." + n])) for n in names)
    num = den = 0.0
    worst = []
    for n in names:
        ref = z["gsub." + n].astype(np.float64).reshape(-1)
        mine = gsub(named_grads[n].detach().cpu().numpy()).reshape(-1)
        d = float(np.linalg.norm(mine - ref))
        r = float(np.linalg.norm(ref))
        num += d * d
        den += r * r
        worst.append((d / (r + 1e-3 * gmax), n))
    worst.sort(reverse=True)
    whole = math.sqrt(num / den)
    print(f"[gradient direction {tag}] whole {whole:.2e}; worst tensors " +
          ", ".join(f"{n} {v:.2e}" for v, n in worst[:4]))
    if yardstick is not None:  # error relative to the reference-autocast error of the same tensor
        ratios = sorted(((v / max(yardstick[n], 1e-12), v, yardstick[n], n) for v, n in worst), reverse=True)
        mine_v, ac_v = np.asarray([v for v, _ in worst]), np.asarray([yardstick[n] for _, n in worst])
        print(f"[gradient direction {tag}] error / reference-autocast error: " +
              ", ".join(f"{n} {r:.2f} ({v:.1e} vs {y:.1e})" for r, v, y, n in ratios[:6]) +
              f"; median ratio {ratios[len(ratios) // 2][0]:.2f}; median {np.median(mine_v):.2e} vs {np.median(ac_v):.2e}, "
              f"max {mine_v.max():.2e} vs {ac_v.max():.2e}")
        assert np.median(mine_v) <= 1.5 * np.median(ac_v), (tag, "median tensor error vs reference autocast")
        assert mine_v.max() <= 1.5 * ac_v.max(), (tag, "worst tensor error vs reference autocast")
    tol_of = per_tensor_tol if callable(per_tensor_tol) else (lambda n: per_tensor_tol)
    bad = [(v, n) for v, n in worst if v >= tol_of(n)]
    assert not bad, (tag, "per-tensor gradient direction", bad[:5])
    assert whole < whole_tol, (tag, "whole-gradient", whole)
    return worst[0], whole


def make_engine(backend, cfg, precise):
    eng = importlib.import_module(ENG)
    a = O.make_args(**cfg)
    e = eng.Engine(a, backend.device, precise=precise)
    for name, pv, gv, isb in e.named_views():
        pv.copy_(torch.from_numpy(synth_tensor(name, tuple(pv.shape), 0)))
    return a, e


def make_oracle(cfg):
    a = O.make_args(**cfg)
    m = O.S2STModel(a)
    load_synth(m, 0)
    m.train()
    return a, m


def rel(x, y):
    x, y = x.detach().double().cpu(), y.detach().double().cpu()
    return float((x - y).abs().max() / (y.abs().max() + 1e-12))


def check_against_oracle(backend, e, m, sample, out_tol, grad_tol, loss_tol, global_grad_tol=None):
    loss, ss, log, outs = O.criterion_forward(m, sample)
    loss.backward()
    o = e.forward(sample, training=True, want_attn=True, seed=1)
    e.zero_grad()
    e.backward(1.0)
    backend.sync()
    pairs = [("encoder_out", outs["encoder_out"].transpose(0, 1)), ("feature_out", outs["feature_out"]),
             ("eos_out", outs["eos_out"]), ("post_feat_out", outs["post_feat_out"]), ("attn", outs["attn"])]
    if outs["asr_logits"] is not None:
        pairs += [("asr_logits", outs["asr_logits"]), ("st_logits", outs["st_logits"])]
    if outs["ctc_lprobs"] is not None:
        pairs += [("ctc_lprobs", outs["ctc_lprobs"].transpose(0, 1))]
    for k, ref in pairs:
        assert rel(o[k], ref) < out_tol, (k, rel(o[k], ref))
    st = o["stats"].cpu()
    for k, i in LOSS_KEYS:
        assert abs(float(st[i]) - float(log[k])) < loss_tol * max(1.0, abs(float(log[k]))), k
    if "asr_n_correct" in log:
        assert int(st[5]) == log["asr_n_correct"] and int(st[6]) == log["asr_total"]
        assert int(st[9]) == log["st_n_correct"] and int(st[10]) == log["st_total"]
    # integer outputs (bit-exact): CTC greedy path, stop indices, encoder lengths
    if outs["ctc_lprobs"] is not None and out_tol < 1e-3:
        il = O.ctc_input_lengths(sample["net_input"]["src_speech_lens"], [5, 5])
        mine = O.ctc_greedy_path(o["ctc_lprobs"].cpu().transpose(0, 1), il)
        assert torch.equal(mine, O.ctc_greedy_path(outs["ctc_lprobs"], il))
    if out_tol < 1e-3:
        assert torch.equal(O.stop_indices(o["eos_out"].cpu()), O.stop_indices(outs["eos_out"]))
    assert torch.equal(o["encoder_lens"].cpu().long(), outs["encoder_lens"])
    named = dict(m.named_parameters())
    gmax = max(float(p.grad.abs().max()) for p in named.values() if p.grad is not None)
    err2 = ref2 = 0.0
    for name, pv, gv, isb in e.named_views():
        if isb:
            continue
        rg = named[name].grad
        rg = torch.zeros_like(named[name]) if rg is None else rg
        # Frobenius-relative error (robust to a ReLU flipping sign on a near-zero pre-activation,
        # which moves single elements by a full dy*x term) plus a looser element-wise bound; the
        # floor covers mathematically-zero gradients (k_proj biases: softmax shift invariance;
        # conv biases in front of BatchNorm)
        d = (gv.cpu() - rg).double()
        fro = float(d.norm()) / (float(rg.double().norm()) + 1e-3 * gmax * math.sqrt(rg.numel()))
        if rg.numel() == 1 and global_grad_tol is not None:
            # a scalar that is a heavily cancelling sum (pos_emb_alpha): judged by the global check
            err2 += float(d.norm()) ** 2
            ref2 += float(rg.double().norm()) ** 2
            continue
        assert fro < grad_tol, (name, fro)
        assert float(d.abs().max()) < 10 * grad_tol * (float(rg.abs().max()) + 1e-3 * gmax), name
        err2 += float(d.norm()) ** 2
        ref2 += float(rg.double().norm()) ** 2
    if global_grad_tol is not None:  # whole-gradient relative error (what the optimizer sees)
        assert math.sqrt(err2 / ref2) < global_grad_tol, math.sqrt(err2 / ref2)
    return o, outs, log


@pytest.mark.parametrize("cfg", [MICRO, MICRO_POSTLN], ids=["preln_aux", "postln"])
def test_micro_engine_vs_oracle(backend, cfg):
    D = importlib.import_module(DATA)
    a, e = make_engine(backend, cfg, precise=True)
    _, m = make_oracle(cfg)
    c = D.SyntheticFisherCorpus(n_utts=4, seed=3, max_src=64, median_src=50, min_src=30)
    s = c.collate_batch(range(4))
    check_against_oracle(backend, e, m, s, out_tol=2e-4, grad_tol=2e-3, loss_tol=2e-5)


def test_state_dict_contract(backend, golden_dir):
    """Parameter / buffer names and shapes equal the reference's."""
    z = np.load(os.path.join(golden_dir, "s2st_tiny.npz"))
    a, e = make_engine(backend, CONFIGS["tiny"], precise=True)
    ref = dict(zip(z["sd_names"].tolist(), z["sd_shapes"].tolist()))
    mine = {n: ",".join(str(int(s)) for s in pv.shape) for n, pv, _, _ in e.named_views()}
    for n, shp in mine.items():
        assert ref[n] == shp, n
    extra = set(ref) - set(mine)
    # the rest are non-arithmetic bookkeeping buffers the host module adds back
    assert all(k.endswith(("_float_tensor", "version", "num_batches_tracked")) for k in extra), extra


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tiny", "tiny_postln"])
def test_tiny_golden_precise(backend, golden_dir, name):
    if backend.kind != "hip":
        pytest.skip("golden-size configs run on the GPU")
    z = np.load(os.path.join(golden_dir, f"s2st_{name}.npz"))
    a, e = make_engine(backend, CONFIGS[name], precise=True)
    _, m = make_oracle(CONFIGS[name])
    s = golden_sample(name, 0)
    # gradient tolerance: the fp32 oracle's own gradients move by up to 8e-3 (Frobenius-relative)
    # when its input is perturbed by 1e-5 -- ReLU units with near-zero pre-activations flip -- so
    # 1.5e-2 is the resolution of this comparison, not of the kernels (micro config: 2e-3).
    o, outs, log = check_against_oracle(backend, e, m, s, out_tol=3e-4, grad_tol=1.5e-2, loss_tol=3e-5)
    # and directly against the reference's own numbers
    st = o["stats"].cpu()
    for k, i in LOSS_KEYS:
        np.testing.assert_allclose(float(st[i]), float(z[f"log.{k}"]), rtol=5e-5, atol=5e-5, err_msg=k)
    for k, mine in [("post_feat_out", o["post_feat_out"]), ("feature_out", o["feature_out"]),
                    ("eos_out", o["eos_out"]), ("attn", o["attn"]),
                    ("encoder_out", o["encoder_out"].transpose(0, 1))]:
        ref = torch.from_numpy(z[f"out.{k}"])
        assert rel(mine, ref) < 3e-4, k
    if "int.ctc_greedy" in z.files:
        il = torch.from_numpy(z["int.ctc_input_lens"])
        assert np.array_equal(O.ctc_greedy_path(o["ctc_lprobs"].cpu().transpose(0, 1), il).numpy(), z["int.ctc_greedy"])
    assert np.array_equal(O.stop_indices(o["eos_out"].cpu()).numpy(), z["int.stop_idx"])
    gn = dict(zip(z["grad_norm_names"].tolist(), z["grad_norms"].tolist()))
    gmax = max(gn.values())
    for n, pv, gv, isb in e.named_views():
        if not isb and n in gn:
            assert abs(float(gv.norm()) - gn[n]) < 1.5e-2 * (gn[n] + 1e-3 * gmax), n
    for k in z.files:
        if k.startswith("grad."):
            g = dict((n, gv) for n, _, gv, b in e.named_views() if not b)[k[5:]]
            ref = z[k].astype(np.float64)
            d = _sub(g.cpu().numpy()).astype(np.float64) - ref
            assert np.linalg.norm(d) < 1.5e-2 * (np.linalg.norm(ref) + 1e-3 * gmax * math.sqrt(ref.size)), k
    # BatchNorm running statistics after one training forward
    bufs = dict((n, pv) for n, pv, _, b in e.named_views() if b)
    for k in z.files:
        if k.startswith("buf.") and not k.endswith("num_batches_tracked"):
            np.testing.assert_allclose(bufs[k[4:]].cpu().numpy(), z[k], rtol=2e-4, atol=2e-5, err_msg=k)


@pytest.mark.gpu
def test_base_golden(backend, golden_dir):
    """BASELINE.json configs[1] geometry (12/6, d512): checksums from the reference."""
    if backend.kind != "hip":
        pytest.skip("base config runs on the GPU")
    z = np.load(os.path.join(golden_dir, "s2st_base.npz"))
    s = golden_sample("base", 0)
    for precise, ltol, otol, gtol in [(True, 5e-5, 5e-4, 5e-3), (False, 1e-3, 3e-2, 1e-1)]:
        a, e = make_engine(backend, CONFIGS["base"], precise=precise)
        o = e.forward(s, training=True, seed=1)
        e.zero_grad()
        e.backward(1.0)
        backend.sync()
        st = o["stats"].cpu()
        for k, i in LOSS_KEYS:
            ref = float(z[f"log.{k}"])
            assert abs(float(st[i]) - ref) < ltol * max(1.0, abs(ref)), (precise, k, float(st[i]), ref)
        for k, mine in [("post_feat_out", o["post_feat_out"]), ("feature_out", o["feature_out"]),
                        ("eos_out", o["eos_out"]), ("encoder_out", o["encoder_out"].transpose(0, 1)),
                        ("asr_logits", o["asr_logits"]), ("st_logits", o["st_logits"])]:
            t = mine.detach().cpu().double().contiguous()
            ref = z[f"sum.{k}"]
            assert abs(float(t.abs().sum()) - ref[1]) < otol * ref[1], (precise, k)
            assert abs(float((t ** 2).sum().sqrt()) - ref[2]) < otol * ref[2], (precise, k)
            # the reference's first 256 values of the tensor (its own layout), element by element -- not only checksums
            head = z[f"head.{k}"].astype(np.float64)
            err = float(np.abs(t.reshape(-1)[:256].numpy() - head).max())
            assert err < otol * max(float(np.abs(head).max()), 1e-2 * float(t.abs().max())), (precise, k, err)
        gn = dict(zip(z["grad_norm_names"].tolist(), z["grad_norms"].tolist()))
        gmax = max(gn.values())
        for n, pv, gv, isb in e.named_views():
            if not isb and n in gn:
                assert abs(float(gv.norm()) - gn[n]) < gtol * (gn[n] + 1e-3 * gmax), (precise, n)
        # gradient DIRECTION of every tensor against the reference's sampled gradients: the
        # benchmarked bf16 mode is held to 5e-2 per tensor / 2e-2 for the whole gradient
        grads = {n: gv for n, pv, gv, isb in e.named_views() if not isb}
        tol_of, whole_tol, ac = bf16_tensor_bounds(golden_dir)
        w, whole = check_gradient_direction(grads, z, 5e-3 if precise else tol_of, 2e-3 if precise else whole_tol,
                                            tag="bf16x3" if precise else "bf16", yardstick=None if precise else ac)
        print(f"[base golden {'bf16x3' if precise else 'bf16'}] worst tensor {w[1]} {w[0]:.2e}, whole gradient {whole:.2e}")
        if precise:
            assert np.array_equal(O.stop_indices(o["eos_out"].cpu()).numpy(), z["int.stop_idx"])
        del e


def test_dropout_training_runs_and_is_seeded(backend):
    """Recipe dropouts (0.1/0.1/0.01, pre/post-net 0.5): same seed -> identical step,
    different seed -> different loss; gradients finite."""
    D = importlib.import_module(DATA)
    cfg = dict(MICRO, dropout=0.1, attention_dropout=0.1, activation_dropout=0.01, prenet_dropout=0.5,
               postnet_dropout=0.5)
    a, e = make_engine(backend, cfg, precise=False)
    c = D.SyntheticFisherCorpus(n_utts=4, seed=3, max_src=64, median_src=50, min_src=30)
    s = c.collate_batch(range(4))
    losses = []
    for seed in (5, 5, 6):
        o = e.forward(s, training=True, seed=seed)
        e.zero_grad()
        e.backward(1.0)
        backend.sync()
        losses.append(float(o["stats"][16]))
        assert torch.isfinite(e.grads).all()
    # same seed -> same dropout masks (sums differ only by atomic ordering); new seed -> new masks
    assert abs(losses[0] - losses[1]) < 1e-4 and abs(losses[0] - losses[2]) > 1e-3


@pytest.mark.parametrize("cfg", [MICRO, MICRO_POSTLN], ids=["preln_aux", "postln"])
@pytest.mark.parametrize("switch", ["S2ST_NO_LN_FUSE", "S2ST_NO_KV_HOIST", "S2ST_NO_ACT_FUSE", "S2ST_ATTN_GFUSE=0", "S2ST_ATTN_GFUSE=2", "S2ST_ATTN_GFUSE=3",
                                    "S2ST_NO_WGRAD_GROUP", "S2ST_GEMM_PERSIST=0", "S2ST_ORDERED_BIAS_SUMS=0", "S2ST_LN_BWD_SPLIT",
                                    "S2ST_GEMM_W4=2", "S2ST_ATTN_SHORT=0"])
def test_fused_backward_paths_equal_the_unfused_ones(backend, cfg, switch, monkeypatch):
    """The oracle cannot reproduce the dropout masks, so fusions that only exist with dropout on are checked
    against the engine's own unfused schedule (A/B switch) with the same seed: the layer-norm backward that also
    emits the preceding linear layer's dropout-backward operand + bias gradient, the hoisted cross-attention
    K|V projections, the ReLU-dropout backward in the data-gradient GEMM epilogue.  Same masks, same bf16
    operands: the gradients agree to fp32 summation order."""
    # (the emulator runs the switches that change kernels' ARITHMETIC paths; pure launch-structure switches are left to
    # the GPU run, where every combination executes: the CPU suite stays within minutes)
    if backend.kind == "emu" and switch not in ("S2ST_NO_LN_FUSE", "S2ST_NO_ACT_FUSE", "S2ST_ATTN_GFUSE=0", "S2ST_ATTN_GFUSE=3",
                                                "S2ST_LN_BWD_SPLIT", "S2ST_NO_WGRAD_GROUP", "S2ST_ORDERED_BIAS_SUMS=0",
                                                "S2ST_ATTN_SHORT=0"):
        pytest.skip("launch-structure switch: covered by the GPU run")
    if backend.kind == "emu" and cfg is MICRO_POSTLN and switch not in ("S2ST_NO_LN_FUSE", "S2ST_LN_BWD_SPLIT"):
        pytest.skip("post-LN layers differ from pre-LN ones in where the layer norms sit: their two switches run here, "
                    "the others on the pre-LN model (and all of them on the GPU)")
    D = importlib.import_module(DATA)
    cfg = dict(cfg, dropout=0.1, attention_dropout=0.1, activation_dropout=0.05, prenet_dropout=0.5, postnet_dropout=0.5)
    c = D.SyntheticFisherCorpus(n_utts=4, seed=3, max_src=64, median_src=50, min_src=30)
    s = c.collate_batch(range(4))
    res = []
    for off in (False, True):
        if off:
            monkeypatch.setenv(*(switch.split("=") if "=" in switch else (switch, "1")))
        a, e = make_engine(backend, cfg, precise=False)
        o = e.forward(s, training=True, seed=9)
        e.zero_grad()
        e.backward(1.0)
        backend.sync()
        res.append((o["stats"].clone(), e.grads.clone(), {n: gv.clone() for n, pv, gv, isb in e.named_views() if not isb}))
        del e
    (s0, g0, v0), (s1, g1, v1) = res
    assert torch.allclose(s0, s1, rtol=1e-5, atol=1e-6)
    # (the attention backward's bf16 projection gradients are the same bits as the cast pass makes; only the q/k/v
    # bias gradients are then summed from the rounded values instead of the fp32 ones)
    # (likewise the layer-norm backward's fused form: the bias gradient of the producing linear layer is the column sum
    # of the bf16 operand it emitted, not of the fp32 values)
    # (and the one-kernel layer-norm backward: on hardware its dx differs from the split kernel's in the last fp32 bit --
    # the compiler contracts the two kernels' multiply-adds differently, the emulator build does not -- and ONE bf16
    # operand of the 64-wide micro model rounding the other way moves the gradients behind it by ~5e-4:
    # tools/debug_lnsplit3.py, profiles/r03_e_ln_schedules_dump_compare.txt)
    # (and D = rowsum(dO * O) of the attention backward from the bf16 copies inside the kernels vs the fp32 row kernel)
    # (and the short-sequence attention forms against the streaming / two-pass kernels: dQ summed in another order, dS
    # rounded to bf16 before instead of after the dQ product's operand fetch)
    tol = 50.0 if switch.startswith(("S2ST_ATTN_GFUSE", "S2ST_NO_LN_FUSE", "S2ST_LN_BWD_SPLIT", "S2ST_ATTN_SHORT")) else 1.0
    worst = sorted(((float((v0[n] - v1[n]).norm()), float(v0[n].norm()), n) for n in v0), reverse=True)[:5]
    assert float((g0 - g1).norm()) <= tol * 2e-5 * float(g0.norm()), worst
    gmax = max(float(v.norm()) for v in v0.values())
    for n in v0:
        assert float((v0[n] - v1[n]).norm()) <= tol * 1e-4 * (float(v0[n].norm()) + 1e-2 * gmax), n


@pytest.mark.parametrize("switch", ["S2ST_NO_WGRAD_GROUP", "S2ST_GEMM_PERSIST=0", "S2ST_GEMM_PERSIST=2", "S2ST_WGRAD_GROUP=8"])
def test_grouped_weight_gradients_equal_single_launches(backend, switch, monkeypatch):
    """128-wide layers, so that the weight-gradient products qualify for the grouped persistent launch (one launch
    per <= 4 products, K = tokens unsplit) and the larger forward products for the persistent kernel: same
    gradients as one split-K launch (+ slab combine) per product / the one-shot kernels."""
    cfg = dict(MICRO, encoder_embed_dim=128, decoder_embed_dim=128, encoder_ffn_embed_dim=256, decoder_ffn_embed_dim=256,
               encoder_attention_heads=2, decoder_attention_heads=2, prenet_dim=128, postnet_conv_dim=128)
    test_fused_backward_paths_equal_the_unfused_ones(backend, cfg, switch, monkeypatch)


def test_removed_two_chain_schedule_is_refused(backend, monkeypatch):
    """S2ST_CHAINS=2 (the step's layers as two utterance-half chains) was measured neutral and removed
    (profiles/r05_chains_ab.txt).  Asked for and not available is loud: creating a bf16-operand engine fails with the
    binding's argument error (S2ST_ERR_ARG, -4) instead of silently running the one schedule there is; 1 is accepted."""
    eng = importlib.import_module(ENG)
    a = O.make_args(**MICRO)
    monkeypatch.setenv("S2ST_CHAINS", "2")
    with pytest.raises(backend.bd.S2STHipError, match=r"s2st_engine_create failed with code -4$"):
        eng.Engine(a, backend.device, precise=False)
    monkeypatch.setenv("S2ST_CHAINS", "1")
    e = eng.Engine(a, backend.device, precise=False)
    assert e.n_params > 0


@pytest.mark.parametrize("cfg", [MICRO, MICRO_POSTLN], ids=["preln_aux", "postln"])
def test_micro_engine_fast_mode_vs_oracle(backend, cfg):
    """Fast mode (bf16 copies of every GEMM operand, gemm_bf16.hip) against the fp32 oracle.
    Tolerances are bf16's: 8-bit mantissas on the operands, fp32 accumulation; the loss stays
    within the north-star 1e-3."""
    D = importlib.import_module(DATA)
    a, e = make_engine(backend, cfg, precise=False)
    _, m = make_oracle(cfg)
    c = D.SyntheticFisherCorpus(n_utts=4, seed=3, max_src=64, median_src=50, min_src=30)
    s = c.collate_batch(range(4))
    # gradients: bf16 rounding noise grows with depth on these 32/64-wide layers (the first prenet
    # layer, at the end of the longest backward path, moves by ~25 %); the whole gradient by ~6 %
    check_against_oracle(backend, e, m, s, out_tol=2e-2, grad_tol=0.35, loss_tol=1e-3, global_grad_tol=0.1)


def test_micro_engine_fused_attention_vs_oracle(backend):
    """Head width 64 (encoder / decoder dim 128, 2 heads): the fast mode takes the fused attention
    kernels (attention.hip) for self- and cross-attention, forward and backward; the last decoder
    layer's cross-attention stays unfused (its head-averaged map is an output)."""
    D = importlib.import_module(DATA)
    cfg = dict(MICRO, encoder_embed_dim=128, decoder_embed_dim=128, encoder_attention_heads=2,
               decoder_attention_heads=2)
    a, e = make_engine(backend, cfg, precise=False)
    _, m = make_oracle(cfg)
    c = D.SyntheticFisherCorpus(n_utts=4, seed=3, max_src=64, median_src=50, min_src=30)
    s = c.collate_batch(range(4))
    check_against_oracle(backend, e, m, s, out_tol=2e-2, grad_tol=0.35, loss_tol=1e-3, global_grad_tol=0.1)


@pytest.mark.parametrize("precise", [True, False], ids=["bf16x3", "bf16"])
def test_ragged_and_minimal_batches(backend, precise):
    """Edge geometries through the whole path: a single shortest-allowed utterance (encoder length 10,
    one or two decoder steps' worth of frames), and a ragged batch of 3 (not a multiple of 8) whose
    lengths differ by 3x -- padded rows, key masks and BatchNorm-over-padding must all match the oracle."""
    D = importlib.import_module(DATA)
    cfg = dict(MICRO, encoder_embed_dim=128, decoder_embed_dim=128, encoder_attention_heads=2,
               decoder_attention_heads=2) if not precise else MICRO
    a, e = make_engine(backend, cfg, precise=precise)
    _, m = make_oracle(cfg)
    c1 = D.SyntheticFisherCorpus(n_utts=2, seed=5, max_src=41, median_src=40, min_src=40)
    c2 = D.SyntheticFisherCorpus(n_utts=6, seed=6, max_src=130, median_src=70, min_src=40)
    tol = dict(out_tol=3e-4, grad_tol=1e-2, loss_tol=3e-5) if precise else \
        dict(out_tol=6e-2, grad_tol=0.5, loss_tol=2e-3, global_grad_tol=0.2)  # BatchNorm statistics over 5 rows
    # (the single-utterance batch) amplify the bf16 operand rounding; the bf16x3 leg pins the arithmetic
    for s in (c1.collate_batch([0]), c2.collate_batch([0, 3, 5])):
        m.zero_grad()
        check_against_oracle(backend, e, m, s, **tol)


def test_prepared_batches_survive_table_growth_and_later_forwards(backend):
    """(a) a batch prepared BEFORE the positional table had to grow still points at valid rows;
    (b) the stats of a forward are not overwritten by the next forward (LazyLog reads them later)."""
    a, e = make_engine(backend, NANO, precise=True)
    D = importlib.import_module(DATA)
    c = D.SyntheticFisherCorpus(n_utts=4, seed=3, max_src=44, median_src=40, min_src=30)
    short = c.collate_batch(range(2))
    long_c = D.SyntheticFisherCorpus(n_utts=2, seed=5, max_src=400, median_src=380, min_src=360)
    long_b = long_c.collate_batch(range(2))
    # start from tables that only just cover the short batch, as round 1's cache did
    e._pe, e._pe_rows = {}, 0
    ref = e.forward(short, training=False, seed=1)
    backend.sync()
    ref_post, ref_stats = ref["post_feat_out"].clone(), ref["stats"].clone()
    e._pe, e._pe_rows = {}, 0
    p_short = e.prepare(short, training=False, seed=1)  # pointers into the small tables
    rows_before = {d: t.shape[0] for d, t in e._pe.items()}
    e.reserve([p_short, e.prepare(long_b, training=False, seed=1)], training=False)
    p_long = e.prepare(long_b, training=False, seed=1)
    assert any(e._pe[d].shape[0] > n for d, n in rows_before.items()), "the long batch must have grown a table"
    # churn the allocator the way a training loop would: a released table would be reused here
    junk = [torch.full((t.numel(),), 7.0, device=backend.device) for t in e._pe_retired]
    o_short = e.forward(p_short, training=False, seed=1)
    backend.sync()
    stats_short, snap = o_short["stats"], o_short["stats"].clone()
    assert torch.equal(o_short["post_feat_out"], ref_post)
    assert rel(snap, ref_stats) < 1e-6  # (loss sums use atomics: last-bit differences between runs)
    o_long = e.forward(p_long, training=False, seed=1)
    backend.sync()
    assert torch.equal(stats_short, snap), "stats of an earlier forward were overwritten"
    assert not torch.equal(o_long["stats"], snap)
    del junk
