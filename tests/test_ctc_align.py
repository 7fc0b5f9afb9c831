"""CTC forced alignment (csrc/ctc_align.hip, ctc_align.py, align.py, Wav2Vec2CTC.align): the definition against the
enumeration of every labeling, the device form against the host form bit for bit at the shapes where the kernel takes
another path, ties, consistency with the greedy path and with the loss kernel's sum over all paths, the CLI and the
recogniser.  PARITY UNPINNED: the reference computes no alignment and torchaudio is absent; the definition is the one in
include/s2st_hip.h."""
import ctypes
import functools
import importlib
import math
import os

import numpy as np
import pytest
import torch

from ctc_align_cases import collapse, enumerate_best, frame_labels, log_softmax, random_target, repeats

PKG = "speech-to-speech-translation_amd"
NEG = np.float32(-np.inf)


def _ca():
    return importlib.import_module(PKG + ".ctc_align")


def _same(dev, host, what=""):
    """integers equal, floats =="""
    assert np.array_equal(dev.frame_tok, host.frame_tok), what
    assert np.array_equal(dev.spans, host.spans), what
    assert dev.tok_scores.dtype == np.float32 and host.tok_scores.dtype == np.float32
    assert np.array_equal(dev.tok_scores, host.tok_scores), what
    assert np.float32(dev.score) == np.float32(host.score), what


def _check_shape_of_result(a, target, n_frames, E):
    """What every alignment satisfies whatever produced it."""
    L = len(target)
    assert a.frame_tok.shape == (E,) and a.spans.shape == (L, 2) and a.tok_scores.shape == (L,)
    if not a.score > NEG:
        assert np.all(a.frame_tok == -2) and np.all(a.spans == -1) and np.all(a.tok_scores == 0)
        return
    assert np.all(a.frame_tok[n_frames:] == -2) and np.all(a.frame_tok[:n_frames] >= -1)
    prev_end = 0
    for i in range(L):
        s, e = a.spans[i]
        assert prev_end <= s < e <= n_frames
        assert np.all(a.frame_tok[s:e] == i)
        prev_end = e
    assert int((a.frame_tok[:n_frames] >= 0).sum()) == int((a.spans[:, 1] - a.spans[:, 0]).sum())


# ---- 1. the definition against enumeration (CPU, host form) -----------------------------------------------------------------
def test_host_form_against_enumeration_of_all_labelings():
    CA = _ca()
    rng = np.random.default_rng(0)
    feasible = infeasible = skipped = 0
    for case in range(300):
        T, V, L = int(rng.integers(1, 8)), int(rng.integers(2, 5)), int(rng.integers(0, 4))
        lp = log_softmax(rng.standard_normal((T, V)))
        target = [int(v) for v in rng.integers(1, V, size=L)]
        a = CA.host_forced_align(lp, target, blank=0)
        best_lab, best, second = enumerate_best(lp, target, 0)
        if best_lab is None:
            assert a.score == NEG and np.all(a.frame_tok == -2), case
            infeasible += 1
            continue
        feasible += 1
        assert abs(float(a.score) - best) <= 1e-4, case
        _check_shape_of_result(a, target, T, T)
        if best - second <= 1e-5:
            skipped += 1
            continue
        assert np.array_equal(frame_labels(a, target, 0, T), best_lab), case
    assert feasible + infeasible == 300 and feasible > 200 and infeasible > 20
    assert skipped <= 0.05 * 300


# ---- 2. device against host, bit for bit ----------------------------------------------------------------------------------------
# (L of the longest target, E, V, blank, layout, route 1 fits): S = 2 L + 1 on both sides of each states-per-thread boundary
# (256, 512, 1024) and the limit (2049); the last one is the recogniser's geometry
CASES = [(0, 6, 5, 0, "BTV", True), (1, 5, 5, 3, "TBV", True), (127, 258, 41, 0, "BTV", True), (128, 262, 5, 3, "TBV", True),
         (255, 520, 515, 0, "BTV", True), (256, 750, 41, 3, "TBV", True), (511, 1030, 5, 0, "BTV", False),
         (512, 1030, 5, 3, "BTV", False), (1024, 2056, 5, 0, "BTV", False), (500, 1500, 32, 0, "BTV", False)]


@functools.lru_cache(maxsize=None)
def _case(k):
    """lp (numpy, in the case's layout), targets, in_lens, the rows' roles, and the host form's alignments -- once."""
    L, E, V, blank, layout, _ = CASES[k]
    rng = np.random.default_rng(100 + k)
    full = random_target(rng, L, V, blank)
    need = L + repeats(full)
    rows = [(full, E, "full"), (full, need, "single path"), (full, max(need - 1, 0), "one frame short"),
            (full, min(2 * L + 1, E), "2L+1"), (full[:min(L, 1)], 1, "one frame")]
    if L >= 1:
        half = random_target(rng, max(L // 2, 1), V, blank, p_repeat=0.7)
        rows += [(half, E - 1, "-inf entries and a NaN"), (random_target(rng, max(L // 3, 1), V, blank), E, "blocked by -inf")]
    if L == 500:
        rows = rows[:1] + rows[5:6] + rows[1:2]
    B = len(rows)
    lp = log_softmax(rng.standard_normal((B, E, V)))
    for b, (t, n, role) in enumerate(rows):
        if role.startswith("-inf"):
            hit = rng.random((E, V)) < 0.1
            hit[:, blank] = False  # (the blank stays open so that most of these rows keep a path)
            lp[b][hit] = NEG
            lp[b, E // 2, t[len(t) // 2]] = np.nan
        if role.startswith("blocked"):
            lp[b, :, t[len(t) // 2]] = NEG
    if layout == "TBV":
        lp = np.ascontiguousarray(lp.transpose(1, 0, 2))
    CA = _ca()
    host = [CA.host_forced_align(lp[b] if layout == "BTV" else lp[:, b], t, blank, n) for b, (t, n, _) in enumerate(rows)]
    lp.setflags(write=False)
    return lp, [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], host


@pytest.mark.parametrize("k", range(len(CASES)), ids=[f"L{c[0]}-E{c[1]}-V{c[2]}-{c[4]}" for c in CASES])
def test_device_equals_host_bit_for_bit(backend, k):
    CA = _ca()
    L, E, V, blank, layout, fits1 = CASES[k]
    lp, targets, in_lens, roles, host = _case(k)
    assert any(n < E for n in in_lens)
    for b, role in enumerate(roles):  # the cases are what they claim to be
        _check_shape_of_result(host[b], targets[b], in_lens[b], E)
        if role in ("full", "single path", "2L+1"):
            assert host[b].score > NEG or (L == 0 and in_lens[b] == 0), role
        if role in ("one frame short", "blocked by -inf"):
            assert host[b].score == NEG, role
        if role == "single path" and in_lens[b] > 0:  # blanks only between repeated labels
            assert int((host[b].frame_tok[:in_lens[b]] == -1).sum()) == repeats(targets[b])
    x = torch.tensor(lp).to(backend.device)  # (a copy: the shared array stays read-only)
    got = {}
    for route in (0, 1, 2):
        if route == 1 and not fits1:
            with pytest.raises(backend.bd.S2STHipError, match='aligner="host"'):
                CA.forced_align(x, targets, in_lens, blank=blank, layout=layout, route=1)
            continue
        got[route] = CA.forced_align(x, targets, in_lens, blank=blank, layout=layout, route=route)
        backend.sync()
        for b in range(len(targets)):
            _same(got[route][b], host[b], (route, roles[b]))
    if 1 in got:  # the two routes against each other
        for b in range(len(targets)):
            _same(got[1][b], got[2][b], roles[b])
            _same(got[0][b], got[1][b], roles[b])
    # the host form through the public entry: the same alignments from the device's copy of the log-probabilities
    if k < 4:
        again = CA.forced_align(x, targets, in_lens, blank=blank, layout=layout, aligner="host")
        for b in range(len(targets)):
            _same(again[b], host[b], roles[b])


def test_strided_views_are_read_in_place(backend):
    """ld_b / ld_t: a [B][E][V] slice of a wider buffer (row stride > V) and its transposed view give the same result."""
    CA = _ca()
    rng = np.random.default_rng(7)
    B, E, V, pad = 3, 19, 6, 4
    wide = torch.from_numpy(log_softmax(rng.standard_normal((B, E, V + pad)))).to(backend.device)
    view = wide[:, :, :V]
    targets = [random_target(rng, n, V, 0) for n in (4, 0, 7)]
    lens = [19, 5, 15]
    a = CA.forced_align(view, targets, lens)
    t = CA.forced_align(view.transpose(0, 1), targets, lens, layout="TBV")
    h = CA.forced_align(view, targets, lens, aligner="host")
    backend.sync()
    for b in range(B):
        _same(a[b], h[b])
        _same(t[b], h[b])


def _raw_call(bd, dev, B, E, V, Lmax, route, ws_bytes, blank=0):
    """s2st_ctc_align_f32 on well-formed buffers, returning its code: the launcher's checks return before any launch."""
    lp = torch.zeros(B, E, V, device=dev)
    tg = torch.ones(B, max(Lmax, 1), dtype=torch.int64, device=dev)
    il = torch.full((B,), E, dtype=torch.int32, device=dev)
    tl = torch.full((B,), Lmax, dtype=torch.int32, device=dev)
    ft = torch.empty(B, E, dtype=torch.int32, device=dev)
    ts, te = (torch.empty(B, max(Lmax, 1), dtype=torch.int32, device=dev) for _ in range(2))
    tsc = torch.empty(B, max(Lmax, 1), device=dev)
    sc = torch.empty(B, device=dev)
    ws = torch.empty(max(ws_bytes, 4), dtype=torch.uint8, device=dev)
    return bd.lib().s2st_ctc_align_f32(lp.data_ptr(), E * V, V, tg.data_ptr(), Lmax, il.data_ptr(), tl.data_ptr(), B, E, V, blank,
                                       route, ft.data_ptr(), ts.data_ptr(), te.data_ptr(), tsc.data_ptr(), sc.data_ptr(),
                                       ws.data_ptr() if ws_bytes else None, ws_bytes, ctypes.c_void_p(bd.stream_ptr()))


def test_launcher_refusals(backend):
    """Argument checks only (they return before any launch): the state limit, a route that does not fit, a short
    workspace, an unknown route, a blank outside the vocabulary."""
    CA = _ca()
    bd, dev = backend.bd, backend.device
    SHAPE, ARG = -2, -4
    assert _raw_call(bd, dev, 1, 4, 3, 1025, 0, 0) == SHAPE
    assert _raw_call(bd, dev, 1, 4, 3, 1025, 2, 1 << 20) == SHAPE
    assert _raw_call(bd, dev, 1, 1500, 3, 500, 1, 0) == SHAPE  # the recogniser's geometry does not fit LDS
    need = bd.lib().s2st_ctc_align_workspace(2, 1500, 500)
    assert need == 2 * ((1500 + 15) // 16) * 1001 * 4
    assert _raw_call(bd, dev, 2, 1500, 3, 500, 2, need - 4) == ARG
    assert _raw_call(bd, dev, 2, 1500, 3, 500, 0, 0) == ARG  # route 0 picks the workspace form there
    assert _raw_call(bd, dev, 1, 4, 3, 1, 3, 0) == ARG
    assert _raw_call(bd, dev, 1, 4, 3, 1, 0, 0, blank=3) == ARG
    x = torch.zeros(1, 4, 3, device=dev)
    with pytest.raises(bd.S2STHipError, match='aligner="host"'):
        CA.forced_align(x, [[1] * 1025], [4])
    with pytest.raises(ValueError, match="outside the vocabulary"):
        CA.forced_align(x, [[3]], [4])
    # the host form has no such limit
    lp = torch.from_numpy(log_softmax(np.random.default_rng(3).standard_normal((1, 2060, 3)))).to(dev)
    a = CA.forced_align(lp, [[1, 2] * 513], [2060], aligner="host")[0]
    assert a.score > NEG and a.spans.shape == (1026, 2)


# ---- 3. ties -----------------------------------------------------------------------------------------------------------------
TIES = [([1, 1, 2, 2, 2, 3], 9), ([1, 1, 2, 2, 2, 3], 8), ([1, 2, 3], 3), ([1, 2, 3], 7), ([1, 1], 3), ([1, 1], 5), ([2], 4),
        ([], 3), ([1, 2, 1, 2], 10), ([3, 3, 3], 10), ([1], 1)]


def test_ties_go_to_the_smaller_jump(backend):
    CA = _ca()
    E, V = 10, 4
    lp = np.full((len(TIES), E, V), np.float32(math.log(0.25)), np.float32)
    targets, lens = [t for t, _ in TIES], [n for _, n in TIES]
    host = [CA.host_forced_align(lp[b], targets[b], 0, lens[b]) for b in range(len(TIES))]
    # [1,1,2,2,2,3] in 9 frames: state path 1 2 3 5 6 7 8 9 11; in 8 frames no path exists
    assert host[0].frame_tok[:9].tolist() == [0, -1, 1, 2, -1, 3, -1, 4, 5] and host[0].frame_tok[9] == -2
    assert host[1].score == NEG
    # stay wins: the path ends in the token's state (the last blank is entered only when strictly better) and, walking
    # back, stays there -- a lone token with frames to spare takes all of them
    assert host[6].frame_tok[:4].tolist() == [0, 0, 0, 0] and host[6].spans.tolist() == [[0, 4]]
    q = np.float32(math.log(0.25))
    assert host[6].tok_scores[0] == np.float32(np.float32(np.float32(q + q) + q) + q) / np.float32(4)
    assert host[7].frame_tok[:3].tolist() == [-1, -1, -1] and host[7].score == np.float32(np.float32(q + q) + q)
    for b in range(len(TIES)):
        _check_shape_of_result(host[b], targets[b], lens[b], E)
    x = torch.from_numpy(lp).to(backend.device)
    for route in (1, 2):
        dev = CA.forced_align(x, targets, lens, route=route)
        backend.sync()
        for b in range(len(TIES)):
            _same(dev[b], host[b], (route, TIES[b]))


# ---- 4. greedy consistency ----------------------------------------------------------------------------------------------------
def _greedy_case(lp, T):
    am = lp[:T].argmax(-1)
    acc = np.float32(0.0)
    for t in range(T):
        acc = np.float32(acc + lp[t, am[t]])
    return am, collapse(am, 0), acc


def test_aligning_the_greedy_transcript_reproduces_the_greedy_path(backend):
    CA = _ca()
    rng = np.random.default_rng(1)
    for case in range(100):  # the host form, T and V varying
        T, V = int(rng.integers(1, 81)), int(rng.integers(2, 15))
        lp = log_softmax(rng.standard_normal((T, V)))
        am, target, acc = _greedy_case(lp, T)
        a = CA.host_forced_align(lp, target, 0)
        assert np.array_equal(frame_labels(a, target, 0, T), am), case
        assert a.score == acc, case
    B, E, V = 12, 80, 14  # the device form, one ragged batch
    lp = log_softmax(rng.standard_normal((B, E, V)))
    lens = [int(v) for v in rng.integers(1, E + 1, size=B)]
    lens[0] = E
    cases = [_greedy_case(lp[b], lens[b]) for b in range(B)]
    dev = CA.forced_align(torch.from_numpy(lp).to(backend.device), [c[1] for c in cases], lens)
    backend.sync()
    for b, (am, target, acc) in enumerate(cases):
        assert np.array_equal(frame_labels(dev[b], target, 0, lens[b]), am), b
        assert dev[b].score == acc, b


def test_greedy_consistency_through_the_models_own_head(backend):
    """The nano engine with synthetic weights: forward_encoder -> get_normalized_probs (ctc_proj over tap 0) -> align to the
    collapse of the per-frame arg-max: the arg-max comes back on every valid frame, the score is its in-order fp32 sum."""
    import s2st_oracle as O
    from synth_weights import load_synth
    from test_engine import NANO, nano_batches
    CA = _ca()
    tasks = importlib.import_module(PKG + ".tasks")
    a = O.make_args(**NANO)
    a.precise_gemm = True
    task = tasks.S2ST_TranslationTask.setup_task(a, device=backend.device)
    model = task.build_model(a)
    load_synth(model, 0)
    model.eval()
    ni = nano_batches()[0]["net_input"]
    with torch.no_grad():
        enc = model.forward_encoder(ni["src_speech"], ni["src_speech_lens"])
        lprobs = model.get_normalized_probs((None, None, enc), log_probs=True)
    backend.sync()
    B, E, V = lprobs.shape
    pad = enc["encoder_padding_mask"]
    lens = (E - pad[0].sum(1)).tolist() if pad else [E] * B
    lp = lprobs.cpu().numpy()
    cases = [_greedy_case(lp[b], lens[b]) for b in range(B)]
    for aligner in ("device", "host"):
        al = CA.forced_align(lprobs, [c[1] for c in cases], lens, aligner=aligner)
        backend.sync()
        for b, (am, target, acc) in enumerate(cases):
            assert np.array_equal(frame_labels(al[b], target, 0, lens[b]), am), (aligner, b)
            assert al[b].score == acc, (aligner, b)


# ---- 5. against the loss kernel ---------------------------------------------------------------------------------------------
def test_best_path_never_beats_the_sum_over_all_paths(backend, golden_dir):
    """The tiny configuration's golden sample: the CTC head's log-probabilities (out.ctc_lprobs of the golden, [E][B][V]),
    the criterion's targets src_text[:src_text_len] and input lengths.  s2st_ctc_f32 reports loss_per_utt = -ll / max(L, 1)
    (0 when infeasible); with the normalisation undone, score[b] <= ll + E * 2^-23 * |ll|: the best path is one term of
    the sum, and fp32 rounding of a sum of E terms is all that may separate them."""
    from configs import golden_sample
    CA = _ca()
    z = np.load(os.path.join(golden_dir, "s2st_tiny.npz"))
    s = golden_sample("tiny", 0)
    lp_tbv = np.ascontiguousarray(z["out.ctc_lprobs"])
    E, B, V = lp_tbv.shape
    il = [int(v) for v in z["int.ctc_input_lens"]]
    tl = [int(v) for v in s["src_text_len"]]
    targets = [s["src_text"][b, :tl[b]].tolist() for b in range(B)]
    Lmax = max(tl)
    dev = backend.device
    logits = torch.tensor(lp_tbv.transpose(1, 0, 2)).contiguous().to(dev)
    tg = torch.zeros(B, Lmax, dtype=torch.int64)
    for b in range(B):
        tg[b, :tl[b]] = torch.tensor(targets[b])
    lpo = torch.zeros(B, E, V, device=dev)
    per = torch.zeros(B, device=dev)
    ws = torch.zeros(backend.bd._bind("s2st_ctc_workspace")(B, E, Lmax), device=dev)
    backend.bd.call("s2st_ctc_f32", logits, tg.to(dev), Lmax, torch.tensor(il, dtype=torch.int32).to(dev),
                    torch.tensor(tl, dtype=torch.int32).to(dev), B, E, V, lpo, per, None, 0.0, ws)
    al = CA.forced_align(lpo, targets, il)
    backend.sync()
    per = per.cpu().numpy()
    n = 0
    for b in range(B):
        if not al[b].score > NEG:
            assert per[b] == 0.0  # zero_infinity
            continue
        ll = -float(per[b]) * max(tl[b], 1)
        bound = E * 2.0 ** -23 * abs(ll)
        print(f"utt {b}: best path {float(al[b].score):.6f}  all paths {ll:.6f}  bound {bound:.3e}")
        assert float(al[b].score) <= ll + bound, b
        n += 1
    assert n >= B // 2


# ---- 6. CLI ----------------------------------------------------------------------------------------------------------------------
def test_align_cli_end_to_end(backend, tmp_path):
    """``python -m s2st_amd.align`` on the miniature corpus with a synthetic checkpoint: both aligners write the same
    bytes, one line per utterance in manifest order plus the closing line; the two refusals."""
    from test_generate_text import _checkpoint
    A = importlib.import_module(PKG + ".align")
    corpus, ckpt = _checkpoint(backend, tmp_path)
    subset = "dev_tiny"
    common = [corpus, "--config-yaml", "config.yaml", "--gen-subset", subset, "--path", ckpt, "--max-tokens", "100",
              "--precise-gemm"]
    raw = {}
    for aligner in ("device", "host"):
        out = tmp_path / aligner
        res = A.main(common + ["--aligner", aligner, "--results-path", str(out)], device=backend.device)
        backend.sync()
        assert res["utterances"] == 4
        with open(out / f"align-{subset}.txt", "rb") as f:
            raw[aligner] = f.read()
    assert raw["device"] == raw["host"]
    lines = raw["device"].decode("utf-8").split("\n")
    assert lines[-1] == "" and lines[-2].startswith("Aligned ")
    body = lines[:-2]
    assert len(body) == 4 and [l.split("\t")[0] for l in body] == ["utt2", "utt3", "utt4", "utt5"]  # dev_tiny: manifest order
    with open(os.path.join(corpus, f"{subset}.tsv")) as f:
        words = [r.split("\t")[5].split(" ") for r in f.read().strip().split("\n")[1:]]
    n_inf = 0
    for l, w in zip(body, words):
        f = l.split("\t")
        n_frames, n_tok = int(f[1]), int(f[2])
        assert n_tok == len(w) + 1  # eos included
        if f[3] == "-inf":
            assert f[4] == "-inf" and len(f) == 5
            n_inf += 1
            continue
        assert len(f) == 5 + n_tok and float(f[3]) < 0 and float(f[4]) == float(A.f32(np.float32(float(f[3])) / np.float32(n_frames)))
        prev = 0
        for tok, want in zip(f[5:], [x if x in ("hola", "que", "tal", "bien", "gracias", "adios", "si", "no") else "<unk>"
                                      for x in w] + ["</s>"]):
            sym, s, e, q = tok.rsplit(":", 3)
            assert sym == want and prev <= int(s) < int(e) <= n_frames and float(q) <= 0
            prev = int(e)
    assert f"({n_inf} without a path)" in lines[-2] and f"Aligned {4 - n_inf} of 4 utterances" in lines[-2]
    # refusal: a split without src_text
    with open(os.path.join(corpus, f"{subset}.tsv")) as f:
        rows = [r.split("\t") for r in f.read().strip().split("\n")]
    with open(os.path.join(corpus, "dev_notext.tsv"), "w") as f:
        for r in rows:
            f.write("\t".join(r[:5] + r[6:]) + "\n")
    with pytest.raises(SystemExit, match="no src_text column"):
        A.main(common[:3] + ["--gen-subset", "dev_notext"] + common[5:] + ["--results-path", str(tmp_path / "x")],
               device=backend.device)
    # refusal: a model without a CTC head
    state = torch.load(ckpt, map_location="cpu", weights_only=False)
    margs = state["cfg"]["model"]
    if isinstance(margs, dict):
        margs["ctc_weight"] = 0.0
    else:
        margs.ctc_weight = 0.0
    state["model"] = {k: v for k, v in state["model"].items() if ".ctc_proj." not in k}
    noctc = str(tmp_path / "noctc.pt")
    torch.save(state, noctc)
    with pytest.raises(SystemExit, match="no CTC head"):
        A.main([corpus, "--config-yaml", "config.yaml", "--gen-subset", subset, "--path", noctc, "--results-path",
                str(tmp_path / "y")], device=backend.device)


# ---- 7. recogniser ---------------------------------------------------------------------------------------------------------------
def test_recogniser_aligns_its_own_transcript(backend):
    """tests/w2v_ctc_synth.py weights with the peaked head: aligning each utterance's own greedy transcript returns word
    spans that cover exactly its non-blank greedy frames outside the word delimiter; a character outside the vocabulary
    is refused by name."""
    import w2v_ctc_synth as WS
    M = importlib.import_module(PKG + ".models.wav2vec2_ctc")
    net = M.Wav2Vec2CTC(backend.device, precise=True, vocab_map=WS.VOCAB, **WS.CONFIGS["tiny"])
    net.load_state_dict(WS.with_head(WS.synth_state(WS.CONFIGS["tiny"]), "tiny", "peaked"))
    waves = [WS.synth_audio(n, seed) for n, seed in WS.UTTS["tiny"]]
    logits, frame_lens, ids, counts = net.forward(waves)
    backend.sync()
    greedy = [logits[b, :frame_lens[b]].cpu().numpy().argmax(-1) for b in range(len(waves))]
    delim = WS.VOCAB["|"]
    inv = {i: t for t, i in WS.VOCAB.items()}
    ids, counts = ids.cpu().numpy(), counts.cpu().numpy()
    # the transcript with EVERY delimiter kept as a space (decode() strips those at the ends): its spelling is the collapsed
    # greedy ids exactly
    texts = ["".join(" " if i == delim else inv[int(i)] for i in ids[b, :counts[b]]) for b in range(len(waves))]
    assert [t.strip() for t in texts] == net.transcribe(waves)
    assert [net.encode_text(t) for t in texts] == [ids[b, :counts[b]].tolist() for b in range(len(waves))]
    checked = 0
    for aligner in ("device", "host"):
        words = net.align(waves, texts, aligner=aligner)
        backend.sync()
        for b, text in enumerate(texts):
            assert [w.text for w in words[b]] == text.split(), (aligner, b)
            al = net.last_alignments[b]
            assert al.score > NEG
            assert np.array_equal(frame_labels(al, net.encode_text(text), net.pad_token_id, frame_lens[b]), greedy[b])
            if not text.strip():  # (nothing but blanks and delimiters: no words)
                continue
            covered = np.zeros(frame_lens[b], bool)
            for w in words[b]:
                s, e = int(round(w.start / 0.02)), int(round(w.end / 0.02))
                assert 0 <= s < e <= frame_lens[b] and w.score <= 0
                covered[s:e] = True
            # the transcript is the collapse of the greedy path, so the alignment IS the greedy path; inside a word the
            # blank frames between two letters lie within the span, outside the words nothing but blanks and delimiters
            want = (greedy[b] != net.pad_token_id) & (greedy[b] != delim)
            assert not np.any(want & ~covered), (aligner, b)
            assert np.all((greedy[b][~covered] == net.pad_token_id) | (greedy[b][~covered] == delim)), (aligner, b)
            first_last = np.nonzero(want)[0]
            assert covered[first_last[0]] and covered[first_last[-1]]
            assert int(round(words[b][0].start / 0.02)) == first_last[0] and int(round(words[b][-1].end / 0.02)) == first_last[-1] + 1
            checked += 1
    assert checked >= 2
    with pytest.raises(ValueError, match="'#'"):
        net.align(waves[:1], ["A#B"])


def test_segments_merge_token_spans_into_words():
    CA = _ca()
    ft = np.array([-1, 0, 0, 1, -1, 2, 3, 3, -1, 4, -2], np.int32)
    spans = np.array([[1, 3], [3, 4], [5, 6], [6, 8], [9, 10]], np.int32)
    sc = np.array([-1.0, -2.0, -0.5, -3.0, -4.0], np.float32)
    al = CA.Alignment(ft, spans, sc, np.float32(-20.0))
    words = CA.segments(al, ["A", "B", "|", "C", "D"], sep="|")
    assert [(w.text, w.start, w.end) for w in words] == [("AB", 1, 4), ("CD", 6, 10)]
    assert words[0].score == pytest.approx((-1.0 * 2 + -2.0 * 1) / 3) and words[1].score == pytest.approx((-3.0 * 2 - 4.0) / 3)
    assert [(w.text, w.start, w.end) for w in CA.segments(al, list("ABXCD"))] == \
        [("A", 1, 3), ("B", 3, 4), ("X", 5, 6), ("C", 6, 8), ("D", 9, 10)]
    assert CA.segments(al, ["|", "A", "|", "|", "B"], sep="|")[0].text == "A"  # separators at the edge / in a row: no empty words
    assert CA.segments(CA.Alignment(ft, spans, sc, NEG), list("ABXCD")) == []
    with pytest.raises(ValueError):
        CA.segments(al, ["A"])
