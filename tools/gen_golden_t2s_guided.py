#!/usr/bin/env python3
"""Golden vectors of ``--use-guided-attention-loss`` from the REFERENCE's own classes, on the CPU (build container only):

    python tools/gen_golden_t2s_guided.py        # writes tests/golden/s2st_tiny_t2s_guided.npz

TEST INFRASTRUCTURE: needs the reference checkout.  ``T2STransformerModel`` through its own ``build_model`` (oracle/
gen_golden_t2s.build) and examples/s2s_trans/criterions/t2s_loss.py's criterion with the flag ON, sigma 0.4, on the seeded
tiny batch -- the one variant in which the reference's term runs: its source lengths are the text lengths, which are the
encoder's own (t2s_loss.py:114-133); ``s2st_loss`` passes fbank lengths against the ``[B, E, D]`` map and raises.

Stored:
  * ``log.*``, ``out.attn``, ``gsub.*`` / ``grad_norms`` / ``grad_norm_names``: the step with every term on, in the form of
    s2st_tiny_t2s.npz.  The guided term moves that gradient by 1e-3 relative, far inside any direction bound, so it pins
    nothing about the term -- hence:
  * ``gattn.<name>`` (the ``gsub`` sample) and ``gattn_norms``: the gradient of the guided term ALONE,
    ``crit.guided_attn(extra["attn"], src_lens, tgt_lens).backward()`` on a fresh forward, for EVERY parameter (``None`` is
    stored as zeros: 36 of the 131 tensors cannot be reached by the term);
  * ``gattn_ac_err`` / ``gattn_ac_whole``: the same gradient formed under ``torch.autocast("cpu", dtype=torch.bfloat16)``,
    compared with the fp32 one by check_gradient_direction's measure (per tensor: ||d|| / (||ref|| + 1e-3 max ||ref||) on the
    samples) -- what the reference's own mixed precision does to this gradient, the yardstick of the bf16 mode;
  * ``kern.*``: on the seeded kernel-test input of tests/guided_attn_synth.py (fingerprint stored), the reference
    ``GuidedAttentionLoss``'s fp32 value, a float64 restatement of it, the relative difference of the two (the reference's
    own rounding error: the forward-kernel test's bound is a multiple of it) and the cell count.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.argv = [sys.argv[0]]
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import gen_golden_t2s as GT  # noqa: E402  (sets up the reference import path + its stand-ins)
import gen_golden as GG  # noqa: E402
import guided_attn_synth as GS  # noqa: E402
import s2st_oracle as O  # noqa: E402
from configs import CONFIGS, golden_sample  # noqa: E402
from examples.s2s_trans.criterions.t2s_loss import GuidedAttentionLoss  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "s2st_tiny_t2s_guided.npz")
SIGMA = GS.SIGMA


def guided_only_grads(a, task, sample, autocast):
    """{name: gradient of the guided term alone} on a fresh model; a parameter the term cannot reach gets zeros."""
    model, _ = GT.build(a)
    crit = GT.T2SCriterion(task, False, a.n_frames_per_step, True, SIGMA, a.bce_pos_weight, 0.0)
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
        _, _, extra = model(src_tokens=sample["src_text"], src_lengths=sample["src_text_len"],
                            prev_output_tokens=sample["net_input"]["prev_output_tokens"], incremental_state=None,
                            target_lengths=sample["target_lengths"], speaker=None)
        loss = crit.guided_attn(extra["attn"], sample["src_text_len"], sample["target_lengths"])
    loss.backward()
    return float(loss), {n: (GG.to_np(p.grad).astype(np.float32) if p.grad is not None else np.zeros(tuple(p.shape), np.float32))
                         for n, p in model.named_parameters()}, sum(p.grad is None for p in model.parameters())


def main():
    a = O.make_args(**CONFIGS["tiny_t2s"])
    model, task = GT.build(a)
    crit = GT.T2SCriterion(task, False, a.n_frames_per_step, True, SIGMA, a.bce_pos_weight, 0.0)
    sample = dict(golden_sample("tiny", 0), speaker=None)
    out = {"sigma": np.asarray(SIGMA)}
    loss, ss, log = crit(model, sample)
    for k, v in log.items():
        out[f"log.{k}"] = np.asarray(float(v))
    loss.backward()
    named = dict(model.named_parameters())
    gn = {n: float(p.grad.norm()) for n, p in named.items() if p.grad is not None}
    out["grad_norm_names"] = np.array(sorted(gn))
    out["grad_norms"] = np.array([gn[k] for k in sorted(gn)], dtype=np.float64)
    for n in sorted(gn):
        out[f"gsub.{n}"] = GG.gsub(GG.to_np(named[n].grad))
    out["src_lens"] = GG.to_np(sample["src_text_len"]).astype(np.int64)
    out["tgt_lens"] = GG.to_np(sample["target_lengths"]).astype(np.int64)
    model2, _ = GT.build(a)
    with torch.no_grad():
        _, _, extra = model2(src_tokens=sample["src_text"], src_lengths=sample["src_text_len"],
                             prev_output_tokens=sample["net_input"]["prev_output_tokens"], incremental_state=None,
                             target_lengths=sample["target_lengths"], speaker=None)
    out["out.attn"] = GG.to_np(extra["attn"]).astype(np.float32)

    # ---- the guided term alone, fp32 and under autocast ---------------------------------------------------------
    v32, g32, none32 = guided_only_grads(a, task, sample, False)
    vac, gac, _ = guided_only_grads(a, task, sample, True)
    names = sorted(g32)
    out["gattn_value"] = np.asarray(v32)
    out["gattn_names"] = np.array(names)
    out["gattn_norms"] = np.array([float(np.linalg.norm(g32[n].astype(np.float64))) for n in names])
    out["gattn_unreached"] = np.asarray(none32)
    for n in names:
        out[f"gattn.{n}"] = GG.gsub(g32[n])
    gmax = max(float(np.linalg.norm(GG.gsub(g32[n]).astype(np.float64))) for n in names)
    errs, num, den = [], 0.0, 0.0
    for n in names:
        r = GG.gsub(g32[n]).astype(np.float64).reshape(-1)
        d = float(np.linalg.norm(GG.gsub(gac[n]).astype(np.float64).reshape(-1) - r))
        errs.append(d / (float(np.linalg.norm(r)) + 1e-3 * gmax))
        num += d * d
        den += float(np.linalg.norm(r)) ** 2
    out["gattn_ac_err"] = np.array(errs)
    out["gattn_ac_whole"] = np.asarray(np.sqrt(num / den))
    out["gattn_ac_value"] = np.asarray(vac)

    # ---- the kernel-test input: reference module in fp32 against a float64 restatement -----------------------------
    attn, src, tgt = GS.fwd_input()
    ref32 = float(GuidedAttentionLoss(SIGMA)(torch.from_numpy(attn), torch.from_numpy(src).long(), torch.from_numpy(tgt).long()))
    tot, n = GS.guided_sum_f64(attn, src, tgt, SIGMA)
    out["kern.fingerprint"] = GS.fingerprint(attn)
    out["kern.ref_f32"] = np.asarray(ref32, dtype=np.float64)
    out["kern.sum_f64"] = np.asarray(tot)
    out["kern.value_f64"] = np.asarray(tot / n)
    out["kern.n_cells"] = np.asarray(n, dtype=np.int64)
    out["kern.ref_f64_err"] = np.asarray(abs(ref32 - tot / n) / abs(tot / n))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(path := OUT), {k: float(v) for k, v in log.items()})
    print("guided alone", v32, "autocast", vac, "unreached", none32, "autocast whole err", float(out["gattn_ac_whole"]),
          "worst", sorted(zip(errs, names), reverse=True)[:5])
    print("kernel input: ref fp32", ref32, "f64", tot / n, "rel err", float(out["kern.ref_f64_err"]), "N", n)


if __name__ == "__main__":
    main()
