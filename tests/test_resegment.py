"""Minimum-error re-segmentation (csrc/reseg.hip, resegment.py, evaluate_s2s_bleu --doc_column): the host form against the
definition restated as plain loops and against the enumeration of all cuts on small cases full of ties, what the definition
implies, the device form against the host form bit for bit on ragged batches around every size at which the kernel takes
another path, the launcher's refusals, and both command-line tools end to end.  Every comparison is exact.  PARITY UNPINNED:
the reference has no re-segmentation and no mwerSegmenter was at hand; the definition is the one in include/s2st_hip.h."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import resegment_cases as RC  # noqa: E402
import w2v_ctc_synth as WS  # noqa: E402

PKG = "speech-to-speech-translation_amd"
GPU_ONLY = pytest.mark.parametrize("backend", [pytest.param("hip", marks=pytest.mark.gpu)], indirect=True)


def _rs():
    return importlib.import_module(PKG + ".resegment")


def _sc():
    return importlib.import_module(PKG + ".scoring")


def _arr(x):
    return np.asarray(x, np.int32)


# ---- 1. the host form against the definition (CPU) -------------------------------------------------------------------------------
def test_host_form_against_the_definition_and_the_enumeration():
    M, S = _rs(), _sc()
    cases = RC.small_cases(420)
    no_hyp = no_ref = empty_sentence = at_zero = tied = 0
    for h, sentences, ends in cases:
        r = [t for s in sentences for t in s]
        want_cuts, want_seg, want_dist, D = RC.scalar_resegment(h, r, ends)
        cuts, seg, dist = M.host_resegment(h, r, ends)
        assert cuts.dtype == np.int32 and seg.dtype == np.int32
        assert cuts.tolist() == want_cuts and seg.tolist() == want_seg and dist == want_dist, (h, sentences, cuts, want_cuts)
        # non-decreasing cuts that end at n; the distances add up; each is the piece's own Levenshtein distance; no other
        # cuts do better
        at = [0] + cuts.tolist()
        assert all(a <= b for a, b in zip(at, at[1:])) and at[-1] == len(h)
        assert int(seg.sum()) == dist == S.edit_distance(h, r)
        for a, b, sen, d in zip(at, at[1:], sentences, seg.tolist()):
            assert d == S.edit_distance(h[a:b], sen), (h, sentences, cuts)
        assert dist == RC.best_cut_sum(h, sentences, S.edit_distance), (h, sentences)
        no_hyp += len(h) == 0
        no_ref += len(r) == 0
        empty_sentence += any(len(s) == 0 for s in sentences)
        at_zero += len(r) > 0 and len(sentences[0]) == 0
        n, m = len(h), len(r)
        tied += any((D[i][j] == D[i - 1][j - 1] + (h[i - 1] != r[j - 1])) + (D[i][j] == D[i - 1][j] + 1) + (D[i][j] == D[i][j - 1] + 1) > 1
                    for i in range(1, n + 1) for j in range(1, m + 1))
    assert len(cases) >= 400 and no_hyp >= 20 and no_ref >= 20 and empty_sentence >= 100 and at_zero >= 30 and tied >= 250, \
        (no_hyp, no_ref, empty_sentence, at_zero, tied)


# ---- 2. what the definition implies (CPU) ----------------------------------------------------------------------------------------
def test_properties():
    M = _rs()
    rng = np.random.RandomState(1)
    sentences = [[f"w{int(v)}" for v in rng.randint(0, 9, n)] for n in (5, 0, 7, 1, 12)]
    flat = [t for s in sentences for t in s]
    ends = np.cumsum([len(s) for s in sentences])
    # the reference itself: cut where the sentences end, nothing to pay, the reference lines back
    same, = M.resegment([flat], [sentences], backend="host")
    assert same.cuts.tolist() == ends.tolist() and same.dist == 0 and not same.seg_dist.any() and same.pieces == sentences
    # no hypothesis: every sentence is missing whole
    none, = M.resegment([[]], [sentences], backend="host")
    assert none.cuts.tolist() == [0] * 5 and none.seg_dist.tolist() == [5, 0, 7, 1, 12] and none.dist == 25
    assert none.pieces == [[]] * 5
    # the tie rule by hand: an extra word between two sentences fits either at no difference in cost; it goes to the earlier one
    tie, = M.resegment(["a b x c d".split()], [["a b".split(), "c d".split()]], backend="host")
    assert tie.pieces == [["a", "b", "x"], ["c", "d"]] and tie.cuts.tolist() == [3, 5] and tie.seg_dist.tolist() == [1, 0]
    # ... and so do words behind the last sentence's end and in front of the first one's start
    edge, = M.resegment(["x a b c y".split()], [["a".split(), "b c".split()]], backend="host")
    assert edge.pieces == [["x", "a"], ["b", "c", "y"]] and edge.dist == 2
    # the clamping: out of order, negative, beyond m; the last end is m
    assert M.clamp_ends([12, 5, -3, 40, 20, 7], 30).tolist() == [12, 12, 12, 30, 30, 30]
    assert M.clamp_ends([-5, 2], 9).tolist() == [0, 9]
    with pytest.raises(ValueError, match="at least one reference sentence"):
        M.resegment([["a"]], [[]], backend="host")
    with pytest.raises(ValueError, match="backend"):
        M.resegment([["a"]], [[["a"]]], backend="cpu")


# ---- 3. device equals host, bit for bit (both backends) --------------------------------------------------------------------------
_host = {}


def _host_of(key, make):
    """The host form's answers for a batch, computed once and shared by the tests that compare against them."""
    if key not in _host:
        batch = make()
        _host[key] = (batch, [_rs().host_resegment(h, r, e) for _, h, r, e in batch])
    return _host[key]


def _small_batch():
    h, r, e = RC.medium_case()
    return RC.ragged_batch() + [("150 x 200", h, r, e)]


def _device(backend, batch):
    got = _rs().device_resegment([_arr(h) for _, h, _, _ in batch], [_arr(r) for _, _, r, _ in batch],
                                 [_arr(e) for _, _, _, e in batch], backend.device)
    backend.sync()
    return got


def _same(got, want, names):
    for name, (c, s, d), (hc, hs, hd) in zip(names, got, want):
        assert c.dtype == np.int32 and s.dtype == np.int32
        assert np.array_equal(c, hc) and np.array_equal(s, hs) and d == hd, (name, c[:8], hc[:8], s[:8], hs[:8], d, hd)


@pytest.mark.parametrize("threads", ["256", "1024"])
def test_device_equals_host_on_the_ragged_batch(backend, monkeypatch, threads):
    """Both widths of the wavefront (the library reads S2ST_RESEG_THREADS at every call; unset: the one it chose)."""
    monkeypatch.setenv("S2ST_RESEG_THREADS", threads)
    batch, want = _host_of("small", _small_batch)
    names = [b[0] for b in batch]
    assert len(set(names)) == len(names) and want[names.index("150 x 200")][2] > 20
    got = _device(backend, batch)
    _same(got, want, names)
    # a document alone gives what it gives inside the batch; a second call gives the same bytes
    for name in ("65 strips", "a pass and five columns", "every column a boundary", "ends out of order", "m0 n2"):
        b = names.index(name)
        _same(_device(backend, [batch[b]]), [got[b]], [name])
    again = _device(backend, batch)
    assert all(a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2] for a, b in zip(got, again))


def test_a_reference_wider_than_a_pass_of_the_wide_wavefront(backend, monkeypatch):
    """1024 threads cover 8192 columns a pass: one strip more than that, and a hypothesis that ends in the second pass."""
    monkeypatch.setenv("S2ST_RESEG_THREADS", "1024")
    rng = np.random.RandomState(4)
    r = [int(v) for v in rng.randint(0, 4, 8192 + RC.STRIP)]
    batch = [("8200", r[8180:] + [1, 2], r, [8191, 8192, 8193, 8200]), ("8193", [0, 1, 2], r[:8193], [4000, 8193])]
    _same(_device(backend, batch), [_rs().host_resegment(h, rr, e) for _, h, rr, e in batch], ["8200", "8193"])


@GPU_ONLY
@pytest.mark.parametrize("threads", ["256", "1024"])
def test_device_equals_host_on_a_talk(backend, monkeypatch, threads):
    """About 3000 x 2500 tokens, 120 sentences: two passes of the narrow wavefront, one of the wide."""
    monkeypatch.setenv("S2ST_RESEG_THREADS", threads)
    batch, want = _host_of("talk", lambda: [("talk",) + RC.large_case(), ("150 x 200",) + RC.medium_case()])
    assert len(batch[0][1]) > 2900 and len(batch[0][2]) == 2500 and want[0][2] > 500
    got = _device(backend, batch)
    _same(got, want, ["talk", "150 x 200"])
    _same(_device(backend, batch[:1]), got[:1], ["talk alone"])


# ---- 4. the launcher's refusals --------------------------------------------------------------------------------------------------
def test_the_library_refuses_bad_arguments(backend):
    lib, dev = backend.bd.lib(), backend.device
    tok = torch.tensor([1, 2, 3, 1, 2, 4, 2, 3], dtype=torch.int32).to(dev)  # h = 1 2 3, r = 1 2 4, ends = 2 3
    off = torch.tensor([[0, 3], [0, 3], [0, 2]], dtype=torch.int64).to(dev)
    out = torch.full((5,), 77, dtype=torch.int32, device=dev)
    need = int(lib.s2st_reseg_workspace(1, 3, 3, 2))
    assert need == 4 * ((2 + 1) * (3 + 1) + 3 + 1 + 2) and int(lib.s2st_reseg_workspace(0, 3, 3, 2)) == 0
    ws = torch.zeros(need // 4, dtype=torch.int32, device=dev)

    def call(B=1, Nmax=3, Mmax=3, Kmax=2, ws_bytes=need, cuts=out.data_ptr()):
        return lib.s2st_reseg_i32(tok.data_ptr(), off[0].data_ptr(), tok[3:].data_ptr(), off[1].data_ptr(), tok[6:].data_ptr(),
                                  off[2].data_ptr(), B, Nmax, Mmax, Kmax, cuts, out[2:].data_ptr(), out[4:].data_ptr(),
                                  ws.data_ptr(), ws_bytes, None)

    for kw in (dict(B=-1), dict(Nmax=-1), dict(Mmax=-1), dict(Kmax=-1), dict(ws_bytes=need - 4), dict(ws_bytes=0), dict(cuts=None)):
        assert call(**kw) == -4, kw
    for kw in (dict(Nmax=32768), dict(Mmax=32768), dict(Nmax=1 << 30)):
        assert call(**kw) == -2, kw
    assert call(B=0) == 0 and call(B=0, ws_bytes=0) == 0
    backend.sync()
    assert bool((out == 77).all())           # nothing was launched
    assert call() == 0
    backend.sync()
    assert out.cpu().tolist() == [2, 3, 0, 1, 1]   # cuts, seg_dist, dist
    assert _rs().MAX_TOKENS == 32767 >= 16384


# ---- 5. the K = 1 convenience ------------------------------------------------------------------------------------------------------
def test_levenshtein_on_sentence_pairs(backend):
    M, S = _rs(), _sc()
    rng = np.random.RandomState(2)
    words = "the a cat dog sat ran on under mat tree".split()
    pairs = [([words[int(v)] for v in rng.randint(0, 10, rng.randint(0, 14))], [words[int(v)] for v in rng.randint(0, 10, rng.randint(0, 14))])
             for _ in range(200)]
    want = [S.edit_distance(a, b) for a, b in pairs]
    assert M.levenshtein(pairs, device=backend.device) == want and M.levenshtein(pairs, backend="host") == want
    assert M.levenshtein([], device=backend.device) == [] and max(want) >= 8 and any(len(a) == 0 or len(b) == 0 for a, b in pairs)


# ---- 6. the resegment CLI ----------------------------------------------------------------------------------------------------------
REF_ROWS = [("talk_a", "Hello there, world !"), ("talk_b", "One two three."), ("talk_a", "This is the second sentence ."),
            ("talk_a", "And a THIRD one"), ("talk_b", "four five")]
HYP = {"talk_a": "hello world this is , the the second sentence and third one more", "talk_b": "One two four FIVE"}


def _write_cli_files(tmp_path, rows=REF_ROWS, hyp=HYP, hyp_lines=None):
    with open(tmp_path / "ref.tsv", "w", encoding="utf-8") as f:
        f.write("doc\ttext\n")
        for d, t in rows:
            f.write(f"{d}\t{t}\n")
    with open(tmp_path / "st.txt", "w", encoding="utf-8") as f:
        for line in hyp_lines if hyp_lines is not None else [f"{d}\t{t}" for d, t in hyp.items()]:
            f.write(line + "\n")
    return ["--hyp", str(tmp_path / "st.txt"), "--ref", str(tmp_path / "ref.tsv")]


@pytest.mark.parametrize("scoring", ["sacrebleu", "wer"])
def test_resegment_cli(backend, tmp_path, capsys, scoring):
    M, S = _rs(), _sc()
    base = _write_cli_files(tmp_path)
    outs = []
    for which in ("device", "host"):
        out = tmp_path / f"{which}.txt"
        r = M.main(base + ["--out", str(out), "--scoring", scoring, "--resegmenter", which], device=backend.device)
        backend.sync()
        printed = capsys.readouterr().out.strip().splitlines()
        outs.append(open(out, "rb").read())
        assert r["documents"] == 2 and r["sentences"] == 5
        lines = [l.split("\t") for l in outs[-1].decode().split("\n")[:-1]]
        scorer = S.build_scorer(scoring, None)
        for hyp, ref in lines:
            scorer.add_string(ref, hyp)
        result = scorer.result_string(4) if scoring == "sacrebleu" else scorer.result_string()
        assert printed[-1] == f"Total Sentences: 5, Sacrebleu: {result}" and r["result"] == result
    assert outs[0] == outs[1]
    # one line per reference row in reference order; punctuation-only tokens gone, lower-cased; the pieces tile the hypothesis
    assert [ref for _, ref in lines] == ["hello there, world", "one two three.", "this is the second sentence", "and a third one",
                                         "four five"]
    assert " ".join(lines[i][0] for i in (0, 2, 3)).split() == "hello world this is the the second sentence and third one more".split()
    assert [lines[i][0] for i in (1, 4)] == ["one two", "four five"]
    assert lines[0][0] == "hello world" and lines[3][0] == "and third one more"
    # the preparation can be switched off
    raw = tmp_path / "raw.txt"
    M.main(base + ["--out", str(raw), "--punctuation-removal", "false", "--lowercase", "false", "--resegmenter", "host"])
    assert capsys.readouterr().out == ""  # (no --scoring: nothing printed)
    assert open(raw).read().split("\n")[1] == "One two\tOne two three."


def test_resegment_cli_char_level_and_refusals(backend, tmp_path, capsys):
    M, S = _rs(), _sc()
    rows = [("d", "今日は 晴れです"), ("d", "明日は雨")]
    base = _write_cli_files(tmp_path, rows, {"d": "今日 は晴れでした明日雨"})
    out = tmp_path / "char.txt"
    r = M.main(base + ["--out", str(out), "--char-level", "--scoring", "sacrebleu"], device=backend.device)
    lines = [l.split("\t") for l in open(out, encoding="utf-8").read().split("\n")[:-1]]
    assert lines == [["今日は晴れでした", "今日は晴れです"],
                     ["明日雨", "明日は雨"]]
    scorer = S.build_scorer("sacrebleu", None, {"sacrebleu_char_level": True})
    for hyp, ref in lines:
        scorer.add_string(ref, hyp)
    assert capsys.readouterr().out.strip().splitlines()[-1] == f"Total Sentences: 2, Sacrebleu: {scorer.result_string(4)}"
    assert r["result"].startswith("BLEU = ") and scorer.score() > 30
    # every refusal names the document
    host = ["--out", str(tmp_path / "no.txt"), "--resegmenter", "host"]
    for kw, why in ((dict(hyp={"talk_a": "x"}), "'talk_b' has reference rows but no hypothesis"),
                    (dict(hyp=dict(HYP, talk_c="y")), "'talk_c' has a hypothesis but no reference rows"),
                    (dict(hyp_lines=["talk_a\tx", "talk_b\ty", "talk_a\tz"]), "'talk_a' appears twice"),
                    (dict(rows=[]), "no reference rows")):
        with pytest.raises(SystemExit, match=why):
            M.main(_write_cli_files(tmp_path, **kw) + host)
    with pytest.raises(ValueError, match="'e' has no reference rows"):
        M.resegment_documents({"e": "x"}, {"e": []}, backend="host")
    assert not os.path.exists(tmp_path / "no.txt")


# ---- 7. evaluate_s2s_bleu --doc_column -------------------------------------------------------------------------------------------
def _talk(utts, pause=7200):
    """Utterances of the seeded speech-like signal at 24 kHz joined by pauses (a faint noise floor, 0.3 s)."""
    parts = []
    for k, (n, seed) in enumerate(utts):
        if k:
            parts.append(1e-4 * torch.randn(pause, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).float())
        parts.append(WS.synth_audio(n, seed, rate=24000).float())
    return torch.cat(parts).numpy()


def test_evaluate_s2s_bleu_on_documents(backend, tmp_path, capsys):
    import test_asr_bleu as TA
    EV = importlib.import_module(PKG + ".evaluate_s2s_bleu")
    GW = importlib.import_module(PKG + ".generate_waveform")
    W = importlib.import_module(PKG + ".models.wav2vec2_ctc")
    SG = importlib.import_module(PKG + ".segmentation")
    AU = importlib.import_module(PKG + ".data.audio_utils")
    M, S = _rs(), _sc()
    model_dir = TA._model_dir(tmp_path / "model", WS.with_head(WS.synth_state(WS.TINY), "tiny", "rich"))
    wav_dir = tmp_path / "out" / "wav_24000hz_griffin_lim"
    os.makedirs(wav_dir)
    talks = {"talk_a": [(19000, 41), (21000, 42), (17000, 43)], "talk_b": [(9000, 44)]}
    for name, utts in talks.items():
        GW.write_wav(str(wav_dir / f"{name}.wav"), _talk(utts), 24000)
    rows = [("s1", "talk_a", "H E"), ("s2", "talk_b", "the only one ."), ("s3", "talk_a", "second , sentence"), ("s4", "talk_a", "A")]
    with open(tmp_path / "test.tsv", "w") as f:
        f.write("id\tsrc_audio\tsrc_n_frames\ttgt_audio\ttgt_n_frames\tsrc_text\ttgt_text\tspeaker\n")
        for uid, doc, text in rows:
            f.write(f"{uid}\tx\t1\ty\t1\tsrc\t{text}\t{doc}\n")
    common = ["--audio_manifest_file", str(tmp_path / "test.tsv"), "--decode_save_path", str(tmp_path / "out"), "--scoring",
              "sacrebleu", "--model_path", model_dir, "--precise"]
    net = W.Wav2Vec2CTC.from_pretrained(model_dir, backend.device, precise=True)
    outs = []
    for which in ("device", "host"):
        out = tmp_path / f"doc_{which}.txt"
        sc = EV.main(common + ["--out_result_file", str(out), "--doc_column", "7", "--max_piece_s", "2", "--resegmenter", which],
                     device=backend.device, recogniser=net)
        backend.sync()
        assert capsys.readouterr().out.strip().splitlines()[-1] == f"Total Sentences: 4, Sacrebleu: {sc.result_string(4)}"
        outs.append(open(out).read())
    assert outs[0] == outs[1]
    lines = [l.split("\t") for l in outs[0].split("\n")[:-1]]
    assert [ref for _, ref in lines] == ["h e", "the only one", "second sentence", "a"]
    # what the pieces of segmentation.segment give when each is transcribed alone, joined per document ...
    joined = {}
    for name in talks:
        wave, rate = AU.get_waveform(str(wav_dir / f"{name}.wav"), mono=True, always_2d=False)
        seg, = SG.segment([SG.host_pcm16(wave)], rate, 100, 200, SG.SMOOTH_FRAMES, SG.SILENCE_DB, SG.CUT_PENALTY_DB, 10,
                          segmenter="host")
        spans = [tuple(int(v) for v in seg.trim_samples[k]) for k in range(len(seg)) if not seg.dropped[k]]
        texts = [net.transcribe(W.resample([torch.from_numpy(wave[a:b])], rate, 16000, backend.device))[0] for a, b in spans]
        joined[name] = S.remove_punctuation(" ".join(texts)).lower()
        assert len(spans) == (2 if name == "talk_a" else 1), (name, spans)
    by_doc = {"talk_a": [0, 2, 3], "talk_b": [1]}
    for name, ii in by_doc.items():
        assert " ".join(lines[i][0] for i in ii).split() == joined[name].split() and joined[name].split(), name
    # ... and its lines are resegment's pieces of that
    want = M.resegment_documents(joined, {d: [lines[i][1] for i in ii] for d, ii in by_doc.items()}, backend="host")
    assert {d: [lines[i][0] for i in ii] for d, ii in by_doc.items()} == want

    # without the flag nothing changes: one wav per row, each transcribed whole
    for k, (uid, _, _) in enumerate(rows):
        GW.write_wav(str(wav_dir / f"{uid}.wav"), WS.synth_audio(3000 + 2500 * k, 50 + k, rate=24000).numpy(), 24000)
    out = tmp_path / "plain.txt"
    sc = EV.main(common + ["--out_result_file", str(out)], device=backend.device, recogniser=net)
    backend.sync()
    scorer = S.build_scorer("sacrebleu", None)
    text = ""
    for uid, _, ref in rows:
        wave, rate = AU.get_waveform(str(wav_dir / f"{uid}.wav"), mono=True, always_2d=False)
        hyp = net.transcribe(W.resample([torch.from_numpy(wave)], rate, 16000, backend.device))[0]
        hyp, ref = S.remove_punctuation(hyp).lower(), S.remove_punctuation(ref).lower()
        text += f"{hyp}\t{ref}\n"
        scorer.add_string(ref, hyp)
    assert open(out).read() == text
    assert capsys.readouterr().out.strip().splitlines()[-1] == f"Total Sentences: 4, Sacrebleu: {scorer.result_string(4)}"
    args = EV.make_parser().parse_args(common + ["--out_result_file", "x"])
    assert args.doc_column is None and args.max_piece_s == 30.0 and args.resegmenter == "device"
