#!/usr/bin/env python3
"""Golden vectors of the wav2vec 2.0 CTC recogniser from ``transformers.Wav2Vec2ForCTC``, on the CPU:

    python tools/gen_golden_w2v_ctc.py

writes tests/golden/w2v_ctc.npz.  TEST INFRASTRUCTURE: needs ``transformers`` (5.15 here); nothing on the GPU machine does.
For the tiny and the large geometry of tests/w2v_ctc_synth.py the library's model (feat_extract_norm "layer",
do_stable_layer_norm, conv_bias) is loaded with the seeded synthetic state and run on the geometry's ragged utterances as ONE
padded batch -- ``Wav2Vec2FeatureExtractor`` (zero-mean / unit-variance, attention mask), the model, ``torch.argmax``,
``Wav2Vec2CTCTokenizer`` -- in fp32 and under ``torch.autocast("cpu", dtype=torch.bfloat16)``.
Stored per geometry: each tensor's bit-pattern checksum and first values (the tests regenerate the weights from the recipe and fail if
they differ) and the library's frame counts; per head ("rich" and "peaked", w2v_ctc_synth's docstring): the fp32 logits at
the valid frames, the autocast error (max |autocast - fp32| over the valid frames: the fast-mode bound is twice that), the
library's own fp32 error against the float64 restatement, the collapsed ids of the valid frames, their text as the
tokenizer's ``batch_decode`` writes it (given each utterance's valid frames), and the share of frames whose top-1 / top-2
margin does not exceed twice the fast-mode bound.
Asserted here: the float64 restatement of w2v_ctc_synth equals the library, the transcripts are not trivial, the host
mapping of w2v_ctc_synth equals ``batch_decode``, the word delimiter occurs inside a transcript and at an utterance's edge,
and -- peaked head -- at most 10 % of the frames are below the margin and one multi-frame utterance is wholly above it.
"""
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import w2v_ctc_synth as WS  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "w2v_ctc.npz")


def library_state(sd, model):
    """The synthetic state under the names this version of the library uses for the positional conv's weight norm."""
    keys = set(model.state_dict().keys())
    out = {}
    for k, v in sd.items():
        if k.endswith("weight_g") and k not in keys:
            k = WS.POS + ".parametrizations.weight.original0"
        elif k.endswith("weight_v") and k not in keys:
            k = WS.POS + ".parametrizations.weight.original1"
        out[k] = v
    return out


def _split(flat, lens):
    out, o = [], 0
    for n in lens:
        out.append(flat[o:o + n])
        o += n
    return out


def main():
    from transformers import Wav2Vec2Config, Wav2Vec2CTCTokenizer, Wav2Vec2FeatureExtractor, Wav2Vec2ForCTC
    torch.manual_seed(0)
    tmp = tempfile.mkdtemp()
    with open(os.path.join(tmp, "vocab.json"), "w") as f:
        json.dump(WS.VOCAB, f)
    tok = Wav2Vec2CTCTokenizer(os.path.join(tmp, "vocab.json"), unk_token="<unk>", pad_token="<pad>", word_delimiter_token="|")
    fe = Wav2Vec2FeatureExtractor(feature_size=1, sampling_rate=16000, padding_value=0.0, do_normalize=True,
                                  return_attention_mask=True)
    rec = {}
    for name, cfg in WS.CONFIGS.items():
        hc = {k: v for k, v in WS.hf_config(cfg).items() if k not in ("model_type", "architectures")}
        model = Wav2Vec2ForCTC(Wav2Vec2Config(**hc)).eval()
        sd = WS.synth_state(cfg)
        res = model.load_state_dict(library_state(sd, model), strict=False)
        assert not res.unexpected_keys and set(res.missing_keys) <= {"wav2vec2.masked_spec_embed"}, res
        waves = [WS.synth_audio(n, seed) for n, seed in WS.UTTS[name]]
        inp = fe([w.numpy() for w in waves], sampling_rate=16000, return_tensors="pt", padding="longest")
        flens = model._get_feat_extract_output_lengths(inp.attention_mask.sum(-1)).tolist()
        assert flens == [WS.frame_count(cfg, n) for n, _ in WS.UTTS[name]], flens
        nfr = sum(flens)
        sums, first = WS.fingerprints(sd)
        rec[f"{name}.sd_sums"], rec[f"{name}.sd_first"] = sums, first
        rec[f"{name}.frame_lens"] = np.array(flens, np.int32)
        for head in WS.HEADS:
            sdh = WS.with_head(sd, name, head)
            with torch.no_grad():
                model.lm_head.weight.copy_(sdh["lm_head.weight"])
                model.lm_head.bias.copy_(sdh["lm_head.bias"])
                logits = model(inp.input_values, attention_mask=inp.attention_mask).logits
                with torch.autocast("cpu", dtype=torch.bfloat16):
                    logits_ac = model(inp.input_values, attention_mask=inp.attention_mask).logits.float()
            valid = [logits[b, :T] for b, T in enumerate(flens)]
            ac_err = max(float((logits_ac[b, :T] - logits[b, :T]).abs().max()) for b, T in enumerate(flens))
            scale = max(float(v.abs().max()) for v in valid)
            # the float64 restatement against the library (= the library's own fp32 error against float64)
            r_err = 0.0
            for w, v in zip(waves, valid):
                y64 = WS.restated_forward(sdh, cfg, w)
                assert tuple(y64.shape) == tuple(v.shape)
                r_err = max(r_err, float((y64 - v.double()).abs().max()))
            frame_ids = [v.argmax(-1) for v in valid]
            ids = [WS.collapse(a.tolist()) for a in frame_ids]
            texts = tok.batch_decode([a.tolist() for a in frame_ids])
            assert texts == [WS.ids_to_text(i) for i in ids], (texts, [WS.ids_to_text(i) for i in ids])
            top2 = torch.cat(valid).topk(2, dim=-1).values
            margin = top2[:, 0] - top2[:, 1]
            low = float((margin <= 2.0 * (2.0 * ac_err)).float().mean())
            print(f"{name}/{head}: frames {flens} max|logit| {scale:.3f} restatement-vs-library {r_err:.3e} autocast err "
                  f"{ac_err:.3e} frames under the margin {100 * low:.1f}% tokens {[len(i) for i in ids]} of {nfr} frames")
            print("   ", texts)
            assert r_err < 1e-4 * max(1.0, scale), (name, head, r_err)
            sure = _split(margin > 2.0 * (2.0 * ac_err), flens)
            if head == "peaked":
                assert low <= 0.10, (name, low)  # the fast-mode token check's condition
                # ... and its whole-utterance comparison has something to compare
                assert any(T > 1 and bool(s.all()) for s, T in zip(sure, flens)), (name, "no multi-frame utterance above the margin")
            # the word delimiter is emitted: inside a transcript, and at an utterance's start or end (the text is stripped)
            assert any(4 in i for i in ids) and any(" " in t for t in texts), (name, head, texts)
            assert any(len(i) > 1 and 4 in (i[0], i[-1]) for i in ids), (name, head, ids)
            assert sum(len(i) for i in ids) >= 6 and any(len(i) < T for i, T in zip(ids, flens) if T > 1), "trivial transcripts"
            k = f"{name}.{head}"
            rec[k + ".logits"] = torch.cat(valid).numpy().astype(np.float32)
            rec[k + ".autocast_err"] = np.float64(ac_err)
            rec[k + ".restatement_err"] = np.float64(r_err)
            rec[k + ".low_margin_share"] = np.float64(low)
            rec[k + ".ids"] = np.array([i for u in ids for i in u], np.int32)
            rec[k + ".counts"] = np.array([len(u) for u in ids], np.int32)
            rec[k + ".texts"] = np.array(texts)
    np.savez_compressed(OUT, **rec)
    print(f"wrote {OUT} ({os.path.getsize(OUT) / 1e6:.3f} MB)")


if __name__ == "__main__":
    main()
