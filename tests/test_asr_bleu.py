"""ASR-BLEU scoring of generated speech (stage 8 of the recipes, examples/s2s_trans/evalute_s2s_bleu.py): the wav2vec 2.0
CTC recogniser on the HIP path (s2st_w2v_ctc_*) against golden logits / tokens of ``transformers.Wav2Vec2ForCTC``
(tools/gen_golden_w2v_ctc.py), its kernels alone against float64 numpy, the resampler, the BLEU scorer, the checkpoint
loader and the script end to end."""
import importlib
import json
import math
import os
import struct
from collections import Counter
from fractions import Fraction

import numpy as np
import pytest
import torch

import w2v_ctc_synth as WS

PKG = "speech-to-speech-translation_amd"
W2V = PKG + ".models.wav2vec2_ctc"


def _golden(golden_dir):
    return np.load(os.path.join(golden_dir, "w2v_ctc.npz"))


_states = {}


def _state(z, name):
    """The geometry's seeded state, regenerated and proven equal to what the golden's generator loaded."""
    if name not in _states:
        sd = WS.synth_state(WS.CONFIGS[name])
        sums, first = WS.fingerprints(sd)
        assert np.array_equal(sums, z[f"{name}.sd_sums"]), f"{name}: the seeded weight recipe no longer reproduces the golden's"
        np.testing.assert_array_equal(first, z[f"{name}.sd_first"])
        _states[name] = sd
    return _states[name]


def _waves(name):
    return [WS.synth_audio(n, seed) for n, seed in WS.UTTS[name]]


def _net(backend, name, precise, sd=None):
    M = importlib.import_module(W2V)
    net = M.Wav2Vec2CTC(backend.device, precise=precise, vocab_map=WS.VOCAB, **WS.CONFIGS[name])
    net.load_state_dict(sd if sd is not None else WS.synth_state(WS.CONFIGS[name]))
    return net


def _set_head(net, sd, name, head):
    h = WS.with_head(sd, name, head)
    net._view("lm_head.weight").copy_(h["lm_head.weight"])
    net._view("lm_head.bias").copy_(h["lm_head.bias"])
    net.invalidate_bf16()


def _split(flat, lens):
    out, o = [], 0
    for n in lens:
        out.append(flat[o:o + n])
        o += n
    return out


def _run(backend, net, waves):
    logits, flens, ids, counts = net(waves)
    backend.sync()
    logits, ids, counts = logits.cpu(), ids.cpu().numpy(), counts.cpu().numpy()
    return [logits[b, :T] for b, T in enumerate(flens)], flens, [ids[b, :counts[b]].tolist() for b in range(len(waves))]


# ---- 1. the restatement is pinned by the library ------------------------------------------------------------------------
@pytest.mark.parametrize("head", WS.HEADS)
def test_restatement_matches_library_golden(golden_dir, head):
    """CPU: the float64 restatement equals the fp32 logits of Wav2Vec2ForCTC on the tiny geometry, on ragged utterances at
    their valid frames (the library ran them as one padded batch with an attention mask); frame counts are the library's.
    Bound: the library's own fp32 rounding, 1e-4 of the logit scale (measured by the generator: 1.2e-5 at |logit| <= 10.8)."""
    z = _golden(golden_dir)
    sd = WS.with_head(_state(z, "tiny"), "tiny", head)
    flens = [int(t) for t in z["tiny.frame_lens"]]
    assert flens == [WS.frame_count(WS.TINY, n) for n, _ in WS.UTTS["tiny"]]
    refs = _split(z[f"tiny.{head}.logits"], flens)
    for w, ref in zip(_waves("tiny"), refs):
        y = WS.restated_forward(sd, WS.TINY, w)
        assert tuple(y.shape) == ref.shape
        assert float(np.abs(y.numpy() - ref).max()) < 1e-4 * max(1.0, float(np.abs(z[f"tiny.{head}.logits"]).max()))


# ---- 2 - 4. logits and tokens against the library --------------------------------------------------------------------------
def _check_geometry(backend, golden_dir, name, precise):
    z = _golden(golden_dir)
    sd = _state(z, name)
    net = _net(backend, name, precise, sd)
    waves = _waves(name)
    flens_ref = [int(t) for t in z[f"{name}.frame_lens"]]
    for head in WS.HEADS:
        _set_head(net, sd, name, head)
        k = f"{name}.{head}"
        ref_all = z[k + ".logits"]
        refs = _split(ref_all, flens_ref)
        got, flens, ids = _run(backend, net, waves)
        assert flens == flens_ref
        # precise: 2e-4 of the output scale, the family's bound (tests/test_hubert.py); fast: twice the library's own
        # error under torch.autocast(bfloat16), stored by the generator
        bound = 2e-4 * max(1.0, float(np.abs(ref_all).max())) if precise else 2.0 * float(z[k + ".autocast_err"])
        err = max(float(np.abs(g.numpy() - r).max()) for g, r in zip(got, refs))
        print(f"{k} precise={precise}: max |logit error| {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (k, precise, err, bound)
        # tokens: the device's collapse of its own logits, always
        for g, i in zip(got, ids):
            assert i == WS.collapse(g.argmax(-1).tolist())
        ref_ids = _split(z[k + ".ids"].tolist(), [int(c) for c in z[k + ".counts"]])
        texts = [str(t) for t in z[k + ".texts"]]
        if precise:  # exact: ids, counts and text as the library's argmax + Wav2Vec2CTCTokenizer give them
            assert ids == ref_ids, k
            assert [net.decode(i) for i in ids] == texts
        elif head == "peaked":
            # fast mode: exact on the frames whose reference top-1 / top-2 margin exceeds twice the fast-mode bound; the
            # generator asserted that at most 10 % of the frames are excluded, and so does this
            ref_t = torch.from_numpy(ref_all)
            top2 = ref_t.topk(2, dim=-1).values
            sure = (top2[:, 0] - top2[:, 1]) > 2.0 * bound
            assert float((~sure).float().mean()) <= 0.10
            got_am = torch.cat(got).argmax(-1)
            assert bool((got_am[sure] == ref_t.argmax(-1)[sure]).all()), k
            whole = 0
            for u, (s, i) in enumerate(zip(_split(sure, flens), ids)):
                if bool(s.all()):  # an utterance wholly above the margin: collapsed ids, count and text as the library's
                    assert i == ref_ids[u] and net.decode(i) == texts[u]
                    whole += flens[u] > 1
            assert whole >= 1  # (the generator asserted that a multi-frame one exists)
        if name == "large":
            # the shapes the claim "a transcript does not depend on the batch" is made for: M = 147 rows against 49 / 27 / 71
            # alone, 1024-wide products (other tile forms than the tiny geometry's)
            for b, w in enumerate(waves):
                g1, f1, i1 = _run(backend, net, [w])
                assert f1[0] == flens[b] and i1[0] == ids[b] and torch.equal(g1[0], got[b]), (k, b)


@pytest.mark.parametrize("precise", [True, False], ids=["bf16x3", "bf16"])
def test_tiny_vs_library_golden(backend, golden_dir, precise):
    """Tiny geometry (conv 7 x 32, embed 64, 3 layers, 4 heads, FFN 128, pos conv 16 / 4, vocabulary 32), four ragged
    utterances incl. a one-frame one, both heads: logits at the valid frames, collapsed ids, counts and text."""
    _check_geometry(backend, golden_dir, "tiny", precise)


@pytest.mark.gpu
@pytest.mark.parametrize("backend", ["hip"], indirect=True)
@pytest.mark.parametrize("precise", [True, False], ids=["bf16x3", "bf16"])
def test_large_vs_library_golden(backend, golden_dir, precise):
    """wav2vec2-large-960h-lv60-self geometry (7 x 512 convs, 24 x 1024, 16 heads, FFN 4096, pos conv 128 / 16) with the
    seeded weights (regenerated; the golden's checksums and first values prove them), the library's logits computed on the
    CPU.  Same two bounds as the tiny geometry, and the batch of three equals each utterance alone bit for bit.  (The library's fp32 logits are within 8.7e-6 of the float64 restatement at
    24 layers, |logit| <= 8.4: the precise bound 2e-4 * 8.4 = 1.7e-3 has room.)"""
    _check_geometry(backend, golden_dir, "large", precise)


# ---- 5. batch independence ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precise", [True, False], ids=["bf16x3", "bf16"])
def test_batch_is_bit_identical_to_one_at_a_time(backend, precise):
    """A ragged batch gives, bit for bit, the logits at valid frames, the ids and the counts that each utterance alone
    gives; samples behind an utterance's end (NaN here) never reach its logits or its transcript."""
    net = _net(backend, "tiny", precise)
    waves = _waves("tiny")
    alone = [_run(backend, net, [w]) for w in waves]
    got, flens, ids = _run(backend, net, waves)
    for b, (lg, fl, i) in enumerate(alone):
        assert fl[0] == flens[b] and i[0] == ids[b]
        assert torch.equal(lg[0], got[b]), b
    lens = [int(w.numel()) for w in waves]
    x = torch.full((len(waves), max(lens) + 37), float("nan"))
    for b, w in enumerate(waves):
        x[b, :lens[b]] = w
    logits, fl2, ids2, counts2 = net.forward_padded(x, lens)
    backend.sync()
    assert fl2 == flens
    for b in range(len(waves)):
        assert torch.equal(logits[b, :flens[b]].cpu(), got[b])
        assert ids2[b, :int(counts2[b])].tolist() == ids[b]
        assert bool((ids2[b, int(counts2[b]):] == -1).all())
    assert net.transcribe(waves) == [net.decode(i) for i in ids]


# ---- 6. the kernels alone, through the C ABI, against float64 numpy -------------------------------------------------------
def _gelu64(z):
    return 0.5 * z * (1.0 + np.vectorize(math.erf)(z / np.sqrt(2.0)))


def test_wave_norm_kernel(backend):
    """(x - mean) / sqrt(var + 1e-7) over each utterance's valid samples, zeros behind them whatever was there; one with a
    large offset (fp32 rounding of the mean is the error: |x| 2^-24 / std), a one-sample one (variance 0), an empty one;
    the same bits on every run."""
    rs = np.random.RandomState(3)
    lens = [5000, 1, 777, 0, 2049]
    N = 5000
    x = (rs.randn(len(lens), N) * np.array([1.0, 1.0, 0.01, 1.0, 3.0])[:, None] +
         np.array([0.0, 2.0, 40.0, 0.0, -3.0])[:, None]).astype(np.float32)
    ref = np.zeros_like(x, dtype=np.float64)
    for b, n in enumerate(lens):
        if n:
            v = x[b, :n].astype(np.float64)
            ref[b, :n] = (v - v.mean()) / np.sqrt(v.var() + 1e-7)
    xin = x.copy()
    for b, n in enumerate(lens):
        xin[b, n:] = np.nan
    dev = backend.device
    outs = []
    for _ in range(2):
        y = torch.full((len(lens), N), 7.0, device=dev)
        backend.bd.call("s2st_w2v_wave_norm_f32", torch.from_numpy(xin).to(dev), torch.tensor(lens, dtype=torch.int32).to(dev),
                        y, len(lens), N, 1e-7)
        backend.sync()
        outs.append(y.cpu())
    assert torch.equal(outs[0], outs[1])
    got = outs[0].numpy()
    # (utterance 2: offset 40 at std 0.01 -- the fp32 mean is off by up to 40 * 2^-24, i.e. 2.4e-4 standard deviations)
    tol = np.array([1e-5, 1e-5, 1e-3, 1e-5, 1e-5])[:, None]
    assert bool((np.abs(got - ref) <= tol * np.maximum(1.0, np.abs(ref))).all())
    for b, n in enumerate(lens):
        assert bool((got[b, n:] == 0.0).all())


@pytest.mark.parametrize("k,stride,C,T", [(10, 5, 512, 70), (10, 5, 32, 130), (7, 3, 8, 65), (3, 1, 64, 1), (16, 2, 200, 5)])
def test_conv0_ln_gelu_kernel(backend, k, stride, C, T):
    """Conv1d(1, C, k, stride, bias) -> LayerNorm(C) -> GELU (Wav2Vec2LayerNormConvLayer, layer 0) against float64 numpy:
    the 10-tap form and the general one, one and eight channels per lane, channel counts that do not fill the lanes,
    frame counts across the 64-frame blocks, a single frame; fp32 and bf16 outputs."""
    rs = np.random.RandomState(k * 100 + C)
    B = 3
    N = (T - 1) * stride + k + 3
    wave = (rs.randn(B, N) + np.array([0.0, 4.0, -3.0])[:, None]).astype(np.float32)
    w = (rs.randn(C, k) / np.sqrt(k)).astype(np.float32)
    bias, g, b_ = (0.3 * rs.randn(C)).astype(np.float32), (1.0 + 0.2 * rs.randn(C)).astype(np.float32), (0.1 * rs.randn(C)).astype(np.float32)
    idx = np.arange(T)[:, None] * stride + np.arange(k)[None, :]
    conv = np.einsum("btk,ck->btc", wave.astype(np.float64)[:, idx], w.astype(np.float64)) + bias
    z = (conv - conv.mean(-1, keepdims=True)) / np.sqrt(conv.var(-1, keepdims=True) + 1e-5) * g + b_
    ref = _gelu64(z)
    dev = backend.device
    y = torch.empty(B, T, C, device=dev)
    yh = torch.empty(B, T, C, dtype=torch.bfloat16, device=dev)
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    backend.bd.call("s2st_w2v_conv0_ln_gelu_f32", t(wave), t(w), t(bias), t(g), t(b_), y, yh, B, N, T, C, k, stride, 1e-5)
    backend.sync()
    scale = max(1.0, float(np.abs(ref).max()))
    assert float(np.abs(y.cpu().numpy() - ref).max()) < 2e-4 * scale
    assert float(np.abs(yh.float().cpu().numpy() - ref).max()) < 1e-2 * scale
    only = torch.empty(B, T, C, dtype=torch.bfloat16, device=dev)  # fast mode's call: the bf16 copy alone
    backend.bd.call("s2st_w2v_conv0_ln_gelu_f32", t(wave), t(w), t(bias), t(g), t(b_), None, only, B, N, T, C, k, stride, 1e-5)
    backend.sync()
    assert torch.equal(only.cpu(), yh.cpu())


@pytest.mark.parametrize("rows,C", [(1, 32), (7, 512), (130, 100), (5, 1024)])
def test_ln_gelu_rows_kernel(backend, rows, C):
    """GELU(LayerNorm(x)) per row against float64 numpy: fp32 and bf16 copies, each alone and both, in place."""
    rs = np.random.RandomState(rows + C)
    x = (rs.randn(rows, C) * 2.0 + 0.5).astype(np.float32)
    g, b_ = (1.0 + 0.2 * rs.randn(C)).astype(np.float32), (0.1 * rs.randn(C)).astype(np.float32)
    xd = x.astype(np.float64)
    ref = _gelu64((xd - xd.mean(-1, keepdims=True)) / np.sqrt(xd.var(-1, keepdims=True) + 1e-5) * g + b_)
    dev = backend.device
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    y = torch.empty(rows, C, device=dev)
    yh = torch.empty(rows, C, dtype=torch.bfloat16, device=dev)
    backend.bd.call("s2st_w2v_ln_gelu_rows_f32", t(x), t(g), t(b_), y, yh, rows, C, 1e-5)
    y1, yh1 = torch.empty_like(y), torch.empty_like(yh)
    backend.bd.call("s2st_w2v_ln_gelu_rows_f32", t(x), t(g), t(b_), y1, None, rows, C, 1e-5)
    backend.bd.call("s2st_w2v_ln_gelu_rows_f32", t(x), t(g), t(b_), None, yh1, rows, C, 1e-5)
    xin = t(x.copy())
    backend.bd.call("s2st_w2v_ln_gelu_rows_f32", xin, t(g), t(b_), xin, None, rows, C, 1e-5)
    backend.sync()
    scale = max(1.0, float(np.abs(ref).max()))
    assert float(np.abs(y.cpu().numpy() - ref).max()) < 2e-5 * scale
    assert float(np.abs(yh.float().cpu().numpy() - ref).max()) < 1e-2 * scale
    assert torch.equal(y1.cpu(), y.cpu()) and torch.equal(yh1.cpu(), yh.cpu()) and torch.equal(xin.cpu(), y.cpu())


def test_ctc_greedy_kernel(backend):
    """Argmax + collapse on the device against the host rule (numpy's argmax: the first maximum): an all-blank row, a
    one-frame row, a row of one repeated token, argmax ties (two equal maxima, and a frame of equal logits: the lowest id,
    the blank), a long row whose repeats and blanks straddle the 256-frame chunks, and garbage behind every length."""
    rs = np.random.RandomState(11)
    T, V, blank = 600, 32, 0
    lens = [600, 1, 300, 40, 600, 257]
    B = len(lens)
    lg = rs.randn(B, T, V).astype(np.float32)
    lg[0, :, blank] = 50.0                       # all blank
    lg[2, :, 9] = 50.0                           # one repeated token
    lg[3, :, :] = rs.randint(0, 3, (T, V)).astype(np.float32)  # many exact ties
    lg[3, 5, :] = 1.0                            # a frame of equal logits
    seg = np.repeat(rs.randint(0, 6, 80), 8)[:T]  # runs of 8 frames over a few ids incl. the blank: boundaries at 256, 512
    lg[4, np.arange(T), seg] = 50.0
    lg[5, 250:257, 7] = 50.0                     # a run across the first chunk boundary, ending at the row's last frame
    for b, n in enumerate(lens):
        lg[b, n:] = np.nan
    dev = backend.device
    res = torch.full((B * T + B,), -7, dtype=torch.int32, device=dev)
    ids, counts = res[:B * T].view(B, T), res[B * T:]
    backend.bd.call("s2st_w2v_ctc_greedy_i32", torch.from_numpy(lg).to(dev), torch.tensor(lens, dtype=torch.int32).to(dev), ids,
                    counts, B, T, V, blank)
    backend.sync()
    ids, counts = ids.cpu().numpy(), counts.cpu().numpy()
    for b, n in enumerate(lens):
        ref = WS.collapse(np.argmax(lg[b, :n], axis=-1).tolist(), blank)
        assert counts[b] == len(ref) and ids[b, :counts[b]].tolist() == ref, b
        assert bool((ids[b, counts[b]:] == -1).all())
    assert counts[0] == 0 and counts[2] == 1 and ids[2, 0] == 9


# ---- 7. the resampler ------------------------------------------------------------------------------------------------------
def _resample_direct(x, sr_from, sr_to):
    """float64 evaluation of the same published filter, written as resampy's interpolation loop (time register, left and
    right wing per output sample)."""
    M = importlib.import_module(W2V)
    win, nb = M.kaiser_best_window()
    ratio = sr_to / sr_from
    if ratio < 1:
        win = win * ratio
    delta = np.append(np.diff(win), 0.0)
    scale = min(1.0, ratio)
    step = int(scale * nb)
    n_in = x.shape[0]
    n_out = -(-n_in * sr_to // sr_from)
    y = np.zeros(n_out)
    x = x.astype(np.float64)
    for t in range(n_out):
        time = Fraction(t * sr_from, sr_to)
        n = int(time)
        frac = scale * float(time - n)
        for sign, f in ((-1, frac), (1, scale - frac)):
            idx = f * nb
            off = int(idx)
            eta = idx - off
            cnt = (win.shape[0] - off) // step
            cnt = min(cnt, n + 1) if sign < 0 else min(cnt, n_in - n - 1)
            if cnt <= 0:
                continue
            pos = off + step * np.arange(cnt)
            src = n - np.arange(cnt) if sign < 0 else n + 1 + np.arange(cnt)
            y[t] += float(np.dot(win[pos] + eta * delta[pos], x[src]))
    return y


@pytest.mark.parametrize("sr_from", [24000, 22050, 8000])
def test_resampler(backend, sr_from):
    """s2st_resample_sinc_f32 to 16 kHz: output lengths ceil(n * to / from); against the float64 direct evaluation of the
    same filter to fp32 rounding (~200 taps of magnitude <= 1 on samples <= 1: 1e-5); a ragged batch equals one at a time
    bit for bit; against scipy.signal.resample_poly on band-limited tones below 7 kHz, away from the ends.
    The gap to scipy's default filter (Kaiser beta 5, 10 zero crossings -- a wider transition band than kaiser_best's) was
    measured once on the 64-sample-trimmed interior of signals of peak <= 1: 24000 -> 16000 Hz 5.2e-4, 22050 -> 16000 Hz
    8.1e-4, 8000 -> 16000 Hz (tones below 3.5 kHz) 9.2e-4; asserted at twice that.  PARITY UNPINNED against librosa."""
    M = importlib.import_module(W2V)
    from scipy.signal import resample_poly
    rs = np.random.RandomState(sr_from)
    lens = [3000, 1, 1234, 777]
    top = min(7000.0, 0.44 * sr_from)
    waves = []
    for n in lens:
        t = np.arange(n) / sr_from
        f, ph, a = rs.uniform(100.0, top, 4), rs.uniform(0, 6.28, 4), rs.uniform(0.1, 0.25, 4)
        waves.append((a[:, None] * np.sin(2 * np.pi * f[:, None] * t[None] + ph[:, None])).sum(0).astype(np.float32))
    ys = M.resample([torch.from_numpy(w) for w in waves], sr_from, 16000, backend.device)
    backend.sync()
    g = math.gcd(sr_from, 16000)
    gaps = []
    for w, y, n in zip(waves, ys, lens):
        assert y.numel() == -(-n * 16000 // sr_from)
        ref = _resample_direct(w, sr_from, 16000)
        assert float(np.abs(y.cpu().numpy() - ref).max()) < 1e-5
        one = M.resample([torch.from_numpy(w)], sr_from, 16000, backend.device)[0]
        assert torch.equal(one.cpu(), y.cpu())
        if n >= 1000:
            sp = resample_poly(w.astype(np.float64), 16000 // g, sr_from // g)
            m = min(sp.shape[0], y.numel())
            gaps.append(float(np.abs(sp[64:m - 64] - y.cpu().numpy()[64:m - 64]).max()))
    print(f"{sr_from} -> 16000 Hz: max gap to scipy.signal.resample_poly {max(gaps):.3e}")
    measured = {24000: 5.2e-4, 22050: 8.1e-4, 8000: 9.2e-4}[sr_from]
    assert max(gaps) <= 2.0 * measured


def test_resample_equal_rates_and_table():
    M = importlib.import_module(W2V)
    table, L, Mm, KL = M.polyphase_table(24000, 16000)
    assert (L, Mm) == (2, 3) and table.dtype == np.float32 and table.shape[0] == 2
    # phase 0 of a 2 / 3 down-sampler: the filter's peak (rolloff * ratio) sits on the input sample itself
    assert abs(float(table[0, KL - 1]) - 0.9475937167399596 * 2 / 3) < 1e-6
    assert abs(float(table.sum(1)[0]) - 1.0) < 2e-3 and abs(float(table.sum(1)[1]) - 1.0) < 2e-3  # unit DC gain


# ---- 8. BLEU ------------------------------------------------------------------------------------------------------------------
def _bleu_by_hand(hyps, refs):
    """An independent computation with exact fractions: clipped n-gram matches and totals of orders 1 - 4 over the corpus,
    exp smoothing, brevity penalty; returns (score, precisions, bp, hyp_len, ref_len)."""
    match, total = [0] * 4, [0] * 4
    hl = rl = 0
    for h, r in zip(hyps, refs):
        h, r = h.split(), r.split()
        hl, rl = hl + len(h), rl + len(r)
        for n in range(1, 5):
            hg = Counter(tuple(h[i:i + n]) for i in range(len(h) - n + 1))
            rg = Counter(tuple(r[i:i + n]) for i in range(len(r) - n + 1))
            total[n - 1] += sum(hg.values())
            match[n - 1] += sum(min(c, rg[g]) for g, c in hg.items())
    if not any(match):  # no match of any order: zero outright, nothing is smoothed (sacrebleu's early return)
        return 0.0, [0.0] * 4, 0.0, hl, rl
    prec, k = [], 0
    for m, t in zip(match, total):
        if t == 0:
            prec.append(Fraction(0))
        elif m == 0:
            k += 1
            prec.append(Fraction(100, 2 ** k * t))
        else:
            prec.append(Fraction(100 * m, t))
    bp = 1.0 if hl >= rl else (math.exp(1 - Fraction(rl, hl)) if hl else 0.0)
    score = 0.0 if any(p == 0 for p in prec) else bp * math.exp(sum(math.log(p) for p in prec) / 4)
    return score, [float(p) for p in prec], bp, hl, rl


def _line(score, prec, bp, hl, rl):
    return (f"BLEU = {score:.2f} " + "/".join(f"{p:.1f}" for p in prec) +
            f" (BP = {bp:.3f} ratio = {(hl / rl if rl else 0.0):.3f} hyp_len = {hl} ref_len = {rl})")


BLEU_CASES = {
    "perfect": (["the cat sat on the mat", "hello there general kenobi"], ["the cat sat on the mat", "hello there general kenobi"]),
    "no_4gram": (["the cat sat in the mat"], ["the cat sat on the mat"]),        # 5/6, 3/5, 1/4 and no 4-gram: smoothed
    "no_3gram": (["a cat b sat c on"], ["a cat sat on the mat"]),                # bigram "a cat" only: orders 3 and 4 smoothed
    "short": (["the cat sat"], ["the cat sat on the mat today"]),                # brevity penalty exp(1 - 7 / 3); no 4-gram
    "empty": ([""], ["the cat sat on the mat"]),
    "no_match": (["x y z w v"], ["the cat sat on the mat"]),                     # words, but no match of any order
    "clipping": (["the the the the the", "a b c d e f"], ["the cat", "a b c d e f"]),  # "the" counts once of five
}


@pytest.mark.parametrize("case", sorted(BLEU_CASES))
def test_sacrebleu_scorer_by_hand(case):
    """corpus BLEU against the by-hand computation, and the formatted line.  PARITY UNPINNED against sacrebleu itself."""
    S = importlib.import_module(PKG + ".scoring")
    hyps, refs = BLEU_CASES[case]
    sc = S.build_scorer("sacrebleu", None, cfg={"sacrebleu_tokenizer": "none"})
    for h, r in zip(hyps, refs):
        sc.add_string(r, h)
    score, prec, bp, hl, rl = _bleu_by_hand(hyps, refs)
    assert abs(sc.score() - score) < 1e-9
    assert sc.result_string(4) == _line(score, prec, bp, hl, rl)
    if case == "perfect":
        assert sc.result_string().startswith("BLEU = 100.00 100.0/100.0/100.0/100.0 (BP = 1.000 ratio = 1.000 hyp_len = 10 ")
    if case == "no_4gram":  # 5/6, 3/5, 1/4 and the smoothed 1 / (2 * 3)
        assert prec == [100 * 5 / 6, 60.0, 25.0, 100 / 6] and abs(score - 100 * (5 / 6 * 0.6 * 0.25 / 6) ** 0.25) < 1e-9
    if case == "no_3gram":
        assert prec[2:] == [100 / (2 * 4), 100 / (4 * 3)]
    if case == "short":
        assert abs(bp - math.exp(1 - 7 / 3)) < 1e-12 and sc.result_string().endswith("hyp_len = 3 ref_len = 7)")
    if case == "empty":
        assert score == 0.0 and sc.result_string() == "BLEU = 0.00 0.0/0.0/0.0/0.0 (BP = 0.000 ratio = 0.000 hyp_len = 0 ref_len = 6)"
    if case == "no_match":
        assert sc.result_string() == "BLEU = 0.00 0.0/0.0/0.0/0.0 (BP = 0.000 ratio = 0.833 hyp_len = 5 ref_len = 6)"
    if case == "clipping":
        assert prec[0] == 100 * 7 / 11


def test_build_scorer_choices():
    S = importlib.import_module(PKG + ".scoring")
    sc = S.build_scorer("sacrebleu")
    assert isinstance(sc, S.SacrebleuScorer) and sc.tokenizer.tokenizer_type == "13a" and not sc.tokenizer.lowercase
    sc.add_string("Hello, world.", "Hello, world.")  # 13a splits the punctuation off: 4 tokens
    assert sc.result_string().endswith("hyp_len = 4 ref_len = 4)")
    lc = S.build_scorer("sacrebleu", None, cfg={"sacrebleu_lowercase": True, "sacrebleu_char_level": True})
    lc.add_string("AB", "ab")
    assert lc.pred == ["a b"] and lc.ref == ["a b"]
    with pytest.raises(NotImplementedError):
        sc.result_string(2)
    assert isinstance(S.build_scorer("wer"), S.WerScorer)
    with pytest.raises(ValueError):
        S.build_scorer("bleu")


# ---- 9. the loader -------------------------------------------------------------------------------------------------------------
def _write_safetensors(path, sd):
    index, blobs, off = {"__metadata__": {"format": "pt"}}, [], 0
    for k, v in sd.items():
        raw = v.detach().contiguous().numpy().astype("<f4").tobytes()
        index[k] = {"dtype": "F32", "shape": list(v.shape), "data_offsets": [off, off + len(raw)]}
        blobs.append(raw)
        off += len(raw)
    head = json.dumps(index).encode("utf-8")
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(head)))
        f.write(head)
        for b in blobs:
            f.write(b)


def _model_dir(path, sd, fmt="bin", spelling="g_v"):
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(WS.hf_config(WS.TINY), f)
    with open(os.path.join(path, "vocab.json"), "w") as f:
        json.dump(WS.VOCAB, f)
    sd = dict(sd)
    sd["wav2vec2.masked_spec_embed"] = torch.zeros(WS.TINY["embed"])  # (a tensor the forward does not read)
    if spelling == "parametrizations":
        sd[WS.POS + ".parametrizations.weight.original0"] = sd.pop(WS.POS + ".weight_g")
        sd[WS.POS + ".parametrizations.weight.original1"] = sd.pop(WS.POS + ".weight_v")
    if fmt == "bin":
        torch.save(sd, os.path.join(path, "pytorch_model.bin"))
    else:
        _write_safetensors(os.path.join(path, "model.safetensors"), sd)
    return str(path)


def test_loader_formats_and_spellings(backend, tmp_path):
    """The same tiny state from pytorch_model.bin and from a hand-written model.safetensors, under both spellings of the
    positional conv's weight norm: identical arenas, equal to load_state_dict's; the weight norm is folded (g != ||v||);
    a missing directory is an error that names the reference's model; the group-norm variant is refused."""
    M = importlib.import_module(W2V)
    sd = WS.synth_state(WS.TINY)
    base = _net(backend, "tiny", True, sd)
    arenas = []
    for fmt in ("bin", "safetensors"):
        for spelling in ("g_v", "parametrizations"):
            d = _model_dir(tmp_path / f"{fmt}_{spelling}", sd, fmt, spelling)
            net = M.Wav2Vec2CTC.from_pretrained(d, backend.device, precise=True)
            assert net.conv == WS.TINY["conv"] and (net.embed, net.layers, net.vocab) == (64, 3, 32)
            assert net.id_to_token[4] == "|" and net.pad_token_id == 0
            arenas.append(net.params.cpu().clone())
    for a in arenas:
        assert torch.equal(a, base.params.cpu())
    G, Eg, kp = 4, 16, 16
    w = base._view(M.POS_W).cpu().permute(0, 1, 3, 2).reshape(64, Eg, kp)
    assert float((w.double() - WS.fold_pos(sd)).abs().max()) < 1e-6
    assert float((w - sd[WS.POS + ".weight_v"]).abs().max()) > 0.1
    with pytest.raises(FileNotFoundError, match="facebook/wav2vec2-large-960h-lv60-self"):
        M.Wav2Vec2CTC.from_pretrained(str(tmp_path / "nowhere"), backend.device)
    cfg = dict(WS.hf_config(WS.TINY), feat_extract_norm="group", do_stable_layer_norm=False, conv_bias=False)
    with pytest.raises(ValueError):
        M.Wav2Vec2CTC.from_config(cfg, WS.VOCAB, backend.device)


# ---- 10. the script end to end --------------------------------------------------------------------------------------------------
def test_cli_end_to_end(backend, tmp_path, capsys):
    """A tiny model directory, 24 kHz wavs from the seeded recipe, a manifest in the reference's column layout: one
    ``hyp<TAB>ref`` line per manifest row in manifest order, then ``Total Sentences: N, Sacrebleu: BLEU = ...``;
    --batch_size 1 (every utterance alone) and 10^9 (one batch) write identical files."""
    EV = importlib.import_module(PKG + ".evaluate_s2s_bleu")
    GW = importlib.import_module(PKG + ".generate_waveform")
    M = importlib.import_module(W2V)
    sd = WS.with_head(WS.synth_state(WS.TINY), "tiny", "rich")
    model_dir = _model_dir(tmp_path / "model", sd)
    wav_dir = tmp_path / "out" / "wav_24000hz_griffin_lim"
    os.makedirs(wav_dir)
    # (utt_e: 300 samples at 24 kHz, one mel frame of an immediate EOS -- 200 at 16 kHz, shorter than the conv stack's
    #  receptive field: an empty hypothesis, not an error)
    utts = [("utt_c", 9000, 31, "Hello, world !"), ("utt_a", 2000, 32, "eve"), ("utt_e", 300, 35, "gone"), ("utt_d", 14000, 33, "A B"),
            ("utt_b", 5000, 34, "be")]
    with open(tmp_path / "test.tsv", "w") as f:
        f.write("id\tsrc_audio\tsrc_n_frames\ttgt_audio\ttgt_n_frames\tsrc_text\ttgt_text\tspeaker\n")
        for uid, n, seed, text in utts:
            GW.write_wav(str(wav_dir / f"{uid}.wav"), WS.synth_audio(n, seed, rate=24000).numpy(), 24000)
            f.write(f"{uid}\tx\t1\ty\t1\tsrc\t{text}\tspk\n")
    outs = []
    for bs in ("1", "1000000000"):
        out = tmp_path / f"res_{bs}.txt"
        sc = EV.main(["--audio_manifest_file", str(tmp_path / "test.tsv"), "--decode_save_path", str(tmp_path / "out"),
                      "--out_result_file", str(out), "--scoring", "sacrebleu", "--batch_size", bs, "--model_path", model_dir,
                      "--precise"], device=backend.device)
        backend.sync()
        printed = capsys.readouterr().out.strip().splitlines()
        assert printed[-1] == f"Total Sentences: 5, Sacrebleu: {sc.result_string(4)}"
        assert printed[-1].startswith("Total Sentences: 5, Sacrebleu: BLEU = ")
        outs.append(open(out).read())
    assert outs[0] == outs[1]
    lines = outs[0].split("\n")
    assert lines[-1] == "" and len(lines) == 6
    assert lines[2] == "\tgone"
    assert [l.split("\t")[1] for l in lines[:5]] == ["hello, world", "eve", "gone", "a b", "be"]  # manifest order; the punctuation-only token is gone
    # the hypotheses: what the recogniser gives for each file alone (16-bit PCM read back, resampled on the device)
    net = M.Wav2Vec2CTC.from_pretrained(model_dir, backend.device, precise=True)
    S = importlib.import_module(PKG + ".scoring")
    for (uid, n, seed, _), line in zip(utts, lines):
        from scipy.io import wavfile
        sr, pcm = wavfile.read(str(wav_dir / f"{uid}.wav"))
        assert sr == 24000 and pcm.dtype == np.int16 and pcm.shape == (n,)
        w16 = M.resample([torch.from_numpy(pcm.astype(np.float32) / 32768.0)], 24000, 16000, backend.device)
        hyp = S.remove_punctuation(net.transcribe(w16)[0]).lower()
        assert line.split("\t")[0] == hyp and "\t" in line
    assert all(l.split("\t")[0] == l.split("\t")[0].lower() for l in lines[:5])
    assert any(" " in l.split("\t")[0] for l in lines[:5])  # (word boundaries reach the scored text)
    assert [b for b in EV.length_batches([5, 1, 9, 3], 10)] == [[1, 3], [0], [2]]
    assert EV.length_batches([5, 1, 9, 3], 10 ** 12) == [[1, 3, 0, 2]] and EV.MAX_BATCH_SAMPLES <= 16000000
