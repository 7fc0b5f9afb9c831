"""Pause-seeking segmentation of long recordings (csrc/segment.hip, segmentation.py, segment.py, translate --segment long):
the search against the enumeration of every admissible cut set, the device form against the host form bit for bit at the
lengths where the kernels take another path and at the recipes' geometry, ``translate --segment long`` against the same spans
fed as independent inputs, and the ``segment`` CLI.  Every comparison is exact: integers equal, bytes equal.  PARITY UNPINNED:
the reference has no segmentation; the definition is the one in include/s2st_hip.h."""
import csv
import importlib
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import segment_cases as SC  # noqa: E402
import test_feature_extraction as TF  # noqa: E402
import test_translate as TT  # noqa: E402
from test_translate import world  # noqa: E402,F401  (the fixture: corpus, stage 3 and a one-update checkpoint per backend)

PKG = "speech-to-speech-translation_amd"
FIELDS = ("start", "end", "trim_start", "trim_end", "dropped", "samples", "trim_samples")


def _sg():
    return importlib.import_module(PKG + ".segmentation")


def _same(dev, host, what=""):
    for f in ("n_samples", "rate", "win", "hop", "n_frames", "cost"):
        assert getattr(dev, f) == getattr(host, f), (what, f, getattr(dev, f), getattr(host, f))
    for f in FIELDS:
        a, b = getattr(dev, f), getattr(host, f)
        assert a.dtype == b.dtype and np.array_equal(a, b), (what, f, a, b)


def _check_shape_of_result(s, min_len, max_len, pad):
    """What every segmentation satisfies whatever produced it."""
    K, T = len(s), s.n_frames
    assert K >= 1 and s.start[0] == 0 and s.end[-1] == T and np.array_equal(s.start[1:], s.end[:-1])
    length = s.end - s.start
    assert np.all(length <= max_len) and (T < min_len or np.all(length >= min_len))
    assert s.samples[0, 0] == 0 and s.samples[-1, 1] == s.n_samples and np.array_equal(s.samples[1:, 0], s.samples[:-1, 1])
    for k in range(K):
        if s.dropped[k]:
            assert s.trim_start[k] == s.trim_end[k] == s.start[k] and s.trim_samples[k, 0] == s.trim_samples[k, 1]
        else:
            assert s.start[k] <= s.trim_start[k] < s.trim_end[k] <= s.end[k]
            a, b = s.trim_samples[k]
            assert s.samples[k, 0] <= a < b <= s.samples[k, 1]
            assert SC_frames(b - a, s.win, s.hop) <= s.trim_end[k] - s.trim_start[k] <= max_len  # it fits the model


def SC_frames(n, win, hop):
    return 0 if n < win else 1 + (n - win) // hop


# ---- 1. the definition against enumeration (CPU, host form) -----------------------------------------------------------------
def test_host_search_against_enumeration_of_all_cut_sets():
    SG = _sg()
    cases = SC.small_search_cases(400)
    several = ties = 0
    for S, lam, min_len, max_len in cases:
        want_cost, want_cuts = SC.enumerate_best(S, lam, min_len, max_len)
        cost, cuts = SG.host_search(S, lam, min_len, max_len)
        assert cost == want_cost and cuts == want_cuts, (S.tolist(), lam, min_len, max_len, cost, cuts, want_cost, want_cuts)
        several += len(cuts) > 2
        ties += len(S) > max_len and lam == 0 and not S.any()
    assert len(cases) == 400 and several >= 100 and ties >= 1  # none is skipped; forced cuts and all-equal costs occur


def test_bad_arguments():
    SG = _sg()
    S = np.zeros(10, np.int64)
    for min_len, max_len in ((0, 4), (-1, 4), (3, 5), (1, 1)):
        with pytest.raises(ValueError, match="min_len"):
            SG.host_search(S, 0, min_len, max_len)
        with pytest.raises(ValueError, match="min_len"):
            SG.host_segment(np.zeros(4000, np.int16), 16000, min_len, max_len)
    with pytest.raises(ValueError):
        SG.host_segment(np.zeros(4000, np.int16), 16000, 2, 4, w=-1)
    with pytest.raises(ValueError):
        SG.host_segment(np.zeros(4000, np.int16), 16000, 2, 4, silence_db=float("nan"))


def test_the_library_refuses_bad_arguments(backend):
    """S2ST_ERR_ARG (-4) from the entry point itself, S2ST_ERR_SHAPE (-2) beyond the ring; nothing is launched."""
    lib = backend.bd.lib()
    dev = backend.device
    pcm = torch.zeros(4000, dtype=torch.int16, device=dev)
    soff = torch.tensor([0, 4000], dtype=torch.int64).to(dev)
    T = 23
    o = [torch.zeros(64, dtype=torch.int32, device=dev) for _ in range(6)]
    cost = torch.zeros(1, dtype=torch.int64, device=dev)
    ws = torch.zeros(1 << 16, dtype=torch.int64, device=dev)

    def call(min_len=2, max_len=4, w=3, pad=1, pf=1e-4, sf=1e-4, Kcap=64, ws_bytes=ws.numel() * 8, B=1):
        return lib.s2st_segment_pcm16(pcm.data_ptr(), soff.data_ptr(), B, T, 400, 160, w, min_len, max_len, pad, pf, sf, Kcap,
                                      *(x.data_ptr() for x in o), cost.data_ptr(), ws.data_ptr(), ws_bytes, None)

    assert call() == 0
    backend.sync()
    for kw in (dict(min_len=0), dict(min_len=3, max_len=5), dict(w=-1), dict(w=65), dict(pad=-1), dict(pf=-1.0),
               dict(sf=float("nan")), dict(pf=float("inf")), dict(Kcap=5), dict(ws_bytes=64), dict(B=-1)):
        assert call(**kw) == -4, kw
    assert call(min_len=100, max_len=7100) == -2
    assert lib.s2st_segment_workspace(1, T, 2) > 0 and lib.s2st_segment_workspace(0, T, 2) == 0
    with pytest.raises(backend.bd.S2STHipError, match="host"):
        _sg().segment([np.zeros(4000, np.int16)], 16000, 100, 7100, device=dev)


# ---- 2. device equals host, bit for bit ---------------------------------------------------------------------------------------
def test_device_equals_host_on_the_ragged_batch(backend):
    SG = _sg()
    rec = SC.ragged_batch()
    kw = dict(w=SC.SMOOTH, silence_db=30.0, cut_penalty_db=25.0, pad=SC.PAD)
    dev, raw = SG.segment([x for _, x in rec], SC.RATE, SC.MIN_LEN, SC.MAX_LEN, device=backend.device, return_energy=True,
                          raw=True, **kw)
    backend.sync()
    seen = set()
    for b, ((name, x), d) in enumerate(zip(rec, dev)):
        h = SG.host_segment(x, SC.RATE, SC.MIN_LEN, SC.MAX_LEN, **kw)
        _same(d, h, name)
        assert np.array_equal(d.E, h.E) and np.array_equal(d.S, h.S), name
        _check_shape_of_result(d, SC.MIN_LEN, SC.MAX_LEN, SC.PAD)
        K = len(h)
        assert raw["nseg"][b] == K and raw["cost"][b] == h.cost
        assert np.all(raw["out"][:4, b, K:] == -1) and not raw["out"][4, b, K:].any(), name  # every element is written
        seen.add((h.n_frames, K))
    by = {name: d for (name, _), d in zip(rec, dev)}
    assert by["n<win"].n_frames == 0 and by["empty"].n_frames == 0 and by["T=1"].n_frames == 1
    assert len(by["T=max_len"]) == 1 and len(by["T=max_len+1"]) == 2 and len(by["T=min_len-1"]) == 1
    assert by["zeros"].dropped.all() and by["zeros"].cost == 0 and len(by["zeros"]) == 3  # the fewest cuts
    assert not by["all -32768"].dropped.any() and by["all -32768"].E.max() == 400 << 30
    assert not by["white noise"].dropped.any() and len(by["white noise"]) >= 300 // SC.MAX_LEN + 1  # forced cuts
    assert (by["bursts"].trim_end - by["bursts"].trim_start < by["bursts"].end - by["bursts"].start).any()
    # a float waveform is rounded by the s2st_wave_to_pcm16 rule first; a recording alone is what it is in the batch
    x = dict(rec)["bursts"]
    f = (x.astype(np.float32) / np.float32(32768) + np.float32(1e-5)).astype(np.float32)
    _same(SG.segment([f], SC.RATE, SC.MIN_LEN, SC.MAX_LEN, device=backend.device, **kw)[0],
          SG.host_segment(f, SC.RATE, SC.MIN_LEN, SC.MAX_LEN, **kw), "float")
    _same(SG.segment([x], SC.RATE, SC.MIN_LEN, SC.MAX_LEN, device=backend.device, **kw)[0], by["bursts"], "alone")


def test_device_equals_host_at_the_recipes_geometry(backend):
    """max_len 3000, min_len 100, T about 7000, the default smoothing (several energy tiles, many chunks, 70 steps)."""
    SG = _sg()
    x = SC.burst_pause(7003, 21, burst=260, pause=35)
    d = SG.segment([x, SC.white_noise(3001, 22)], SC.RATE, 100, 3000, device=backend.device, return_energy=True)
    backend.sync()
    for got, y in zip(d, (x, SC.white_noise(3001, 22))):
        h = SG.host_segment(y, SC.RATE, 100, 3000)
        _same(got, h)
        assert np.array_equal(got.E, h.E) and np.array_equal(got.S, h.S)
        _check_shape_of_result(got, 100, 3000, 10)
    assert d[0].n_frames == 7003 and len(d[0]) == 3 and len(d[1]) == 2


# ---- 3. translate --segment long ----------------------------------------------------------------------------------------------
LIMIT = 60  # the tiny model's max_source_positions in these tests
SEG_FLAGS = ["--min-segment-s", "0.1", "--segment-pad-ms", "20"]
SEG_OPTS = dict(min_segment_s=0.1, segment_pad_ms=20.0)
TEXT = ["--text", "both", "--beam", "2", "--max-len-b", "5"]


def _long_recording(world):
    """About 2.5 x LIMIT frames: the corpus' utterances with stretches of faint noise between them."""
    rs = np.random.RandomState(9)
    parts = []
    for k in (0, 1, 0, 1, 0):
        parts += [world.pcm(k)[0][:4000], rs.randint(-3, 4, 12 * SC.HOP).astype(np.int16)]
    x = np.concatenate(parts)[:SC.samples_for(150, 40)]
    assert SC_frames(len(x), SC.WIN, SC.HOP) == 150
    return x


def _setup(world):
    if not hasattr(world, "seg"):
        d = world.root / "segment"
        d.mkdir()
        ckpt = TT._edited_checkpoint(world, "short_source.pt", max_source_positions=LIMIT)
        long_ = _long_recording(world)
        open(d / "long.wav", "wb").write(TF._wav_bytes(long_, 16000))
        open(d / "silence.wav", "wb").write(TF._wav_bytes(np.zeros(len(long_), np.int16), 16000))
        world.seg = dict(dir=d, ckpt=ckpt, long=long_, files=[world.files[0], str(d / "long.wav"), world.files[1]], runs={})
    return world.seg


def _cli(world, tag, files, extra):
    s = _setup(world)
    if tag not in s["runs"]:
        out = s["dir"] / ("out_" + tag)
        argv = [str(world.data), "--config-yaml", "config.yaml", "--path", s["ckpt"], "--results-path", str(out), "--inputs"] + \
            list(files) + ["--max-tokens", "400", "--dump-features", "--dump-eos-probs"] + TT.GEN_FLAGS + TEXT + list(extra)
        np.random.seed(TT.PHASE_SEED)
        r = TT._mod("translate").main(argv, device=world.backend.device)
        world.backend.sync()
        s["runs"][tag] = (out, r)
    return s["runs"][tag]


def _tsv(path):
    with open(path) as f:
        return list(csv.DictReader(f, delimiter="\t", quoting=csv.QUOTE_NONE))


def _tree(root):
    return {os.path.relpath(os.path.join(d, f), root): open(os.path.join(d, f), "rb").read() for d, _, fs in os.walk(root) for f in fs}


def test_without_the_flag_a_long_input_is_skipped_as_before(backend, world):
    s = _setup(world)
    out, r = _cli(world, "off", s["files"], [])
    assert r["utterances"] == 2 and r["skipped"] == ["long"]
    assert r["skipped_reasons"]["long"] == f"150 frames exceed max_source_positions {LIMIT}"
    assert sorted(os.listdir(out / "wav_24000hz_griffin_lim")) == ["src4.wav", "src5.wav"] and not os.path.exists(out / "segments.tsv")


def test_translate_segment_long_equals_its_segments_as_independent_inputs(backend, world):
    s = _setup(world)
    out, r = _cli(world, "long", s["files"], ["--segment", "long"] + SEG_FLAGS)
    assert r["utterances"] == 3 and r["skipped"] == []
    rows = _tsv(out / "segments.tsv")
    assert list(rows[0]) == ["id", "k", "src_start_s", "src_end_s", "trim_start_s", "trim_end_s", "dropped", "out_start_s",
                             "out_end_s", "asr", "st"]
    assert [r_["id"] for r_ in rows] == ["long"] * len(rows) and [int(r_["k"]) for r_ in rows] == list(range(len(rows)))
    smp = lambda v: int(round(float(v) * 16000))  # noqa: E731
    assert smp(rows[0]["src_start_s"]) == 0 and smp(rows[-1]["src_end_s"]) == len(s["long"])
    assert all(smp(a["src_end_s"]) == smp(b["src_start_s"]) for a, b in zip(rows, rows[1:]))
    live = [r_ for r_ in rows if r_["dropped"] == "0"]
    assert len(live) >= 3 and all(smp(r_["src_end_s"]) - smp(r_["src_start_s"]) <= LIMIT * SC.HOP + SC.WIN for r_ in rows)
    spans = [(smp(r_["trim_start_s"]), smp(r_["trim_end_s"])) for r_ in live]
    assert any(b - a < smp(r_["src_end_s"]) - smp(r_["src_start_s"]) for (a, b), r_ in zip(spans, live))  # trimmed at the pauses

    # the spans the TSV reports, cut from the same samples, as independent inputs in the same call
    utt0, utt1 = world.pcm(4 - 4), world.pcm(5 - 4)
    tr = world.translator(ckpt=s["ckpt"], max_tokens=400, text="both", beam=2, max_len_b=5, **SEG_OPTS)
    ids = ["src4"] + [f"long#{r_['k']}" for r_ in live] + ["src5"]
    np.random.seed(TT.PHASE_SEED)
    alone = tr.translate([utt0] + [(s["long"][a:b], 16000) for a, b in spans] + [utt1], ids=ids)
    backend.sync()
    assert tr.skipped == [] and [h["id"] for h in alone] == ids
    np.random.seed(TT.PHASE_SEED)
    whole = tr.translate([utt0, (s["long"], 16000), utt1], ids=["src4", "long", "src5"], segment="long")
    backend.sync()
    assert tr.skipped == [] and whole[1]["segment_ids"] == [int(r_["k"]) for r_ in live]
    pairs = list(zip(whole[1]["segments"], alone[1:-1])) + [(whole[0], alone[0]), (whole[2], alone[-1])]
    for a, b in pairs:
        for key in ("src_feature", "feature", "eos_prob"):
            x, y = a[key].cpu().numpy(), b[key].cpu().numpy()
            assert x.shape == y.shape and np.array_equal(TT._bits(x), TT._bits(y)), (a["id"], key)
        assert a["id"] == b["id"] and np.array_equal(a["pcm"], b["pcm"]) and a["asr"] == b["asr"] and a["st"] == b["st"]
        assert a["src_feature"].shape[0] <= LIMIT and len(a["asr"].split()) == 5
        # ... and the CLI dumped these very features under id#k
        assert np.array_equal(TT._bits(np.load(out / "feat" / f"{a['id']}.npy")), TT._bits(a["feature"].cpu().numpy()))
    # the written wav: the segments' PCM in order, a pause of min(source gap in output samples, max pause) between neighbours
    pieces = [alone[1]["pcm"]]
    for (_, prev_end), (start, _), h in zip(spans, spans[1:], alone[2:-1]):
        pieces += [np.zeros(min((start - prev_end) * 24000 // 16000, 24000), np.int16), h["pcm"]]
    want = np.concatenate(pieces)
    rate, got = TT._wav(out / "wav_24000hz_griffin_lim" / "long.wav")
    assert rate == 24000 and np.array_equal(got, want) and np.array_equal(whole[1]["pcm"], want)
    at = 0
    for j, (r_, h) in enumerate(zip(live, alone[1:-1])):
        at += len(pieces[2 * j - 1]) if j else 0
        assert (int(round(float(r_["out_start_s"]) * 24000)), int(round(float(r_["out_end_s"]) * 24000))) == (at, at + len(h["pcm"]))
        at += len(h["pcm"])
        assert r_["asr"] == h["asr"] and r_["st"] == h["st"]
    for which in ("asr", "st"):
        lines = open(out / f"{which}.txt", encoding="utf-8").read().split("\n")
        assert lines == [f"src4\t{alone[0][which]}", "long\t" + " ".join(h[which] for h in alone[1:-1]),
                         f"src5\t{alone[-1][which]}", ""]
    assert sorted(os.listdir(out / "wav_24000hz_griffin_lim")) == ["long.wav", "src4.wav", "src5.wav"]
    # a shorter pause limit only shortens the pauses
    tr.max_pause_ms = 10.0
    short = tr._join("long", {"seg": whole[1]["segmentation"]}, dict(zip(whole[1]["segment_ids"], whole[1]["segments"])), 16000)
    pauses = [min((b[0] - a[1]) * 24000 // 16000, 240) for a, b in zip(spans, spans[1:])]
    assert len(short["pcm"]) == sum(len(h["pcm"]) for h in alone[1:-1]) + sum(pauses) < len(want)


def test_a_long_input_at_another_rate_is_resampled_once_and_then_segmented(backend, world):
    """Segmentation runs at the source rate: the segments of an 8 kHz copy are those of its resampled samples, fed at 16 kHz."""
    s = _setup(world)
    W, SG = TT._mod("models.wav2vec2_ctc"), _sg()
    x8 = np.ascontiguousarray(s["long"][::2])
    tr = world.translator(ckpt=s["ckpt"], max_tokens=400, src_sample_rate=16000, segment="long", **SEG_OPTS)
    np.random.seed(TT.PHASE_SEED)
    whole = tr.translate([(x8, 8000)], ids=["slow"])[0]
    y = W.resample([x8.astype(np.float32) / np.float32(32768)], 8000, 16000, device=backend.device)[0].cpu().numpy()
    seg = SG.host_segment(y, 16000, 10, LIMIT, pad=2)
    _same(whole["segmentation"], seg)
    live = [k for k in range(len(seg)) if not seg.dropped[k]]
    assert whole["segment_ids"] == live and len(live) >= 3 and tr.skipped == []
    np.random.seed(TT.PHASE_SEED)
    alone = tr.translate([(y[a:b], 16000) for a, b in seg.trim_samples[live]], ids=[f"slow#{k}" for k in live])
    for a, b in zip(whole["segments"], alone):
        assert a["id"] == b["id"] and np.array_equal(a["pcm"], b["pcm"])
        assert np.array_equal(TT._bits(a["src_feature"].cpu().numpy()), TT._bits(b["src_feature"].cpu().numpy()))


def test_the_host_segmenter_writes_the_same_files(backend, world):
    s = _setup(world)
    dev, _ = _cli(world, "long", s["files"], ["--segment", "long"] + SEG_FLAGS)
    host, r = _cli(world, "long_host", s["files"], ["--segment", "long", "--segmenter", "host"] + SEG_FLAGS)
    a, b = _tree(dev), _tree(host)
    assert sorted(a) == sorted(b) and "segments.tsv" in a and r["skipped"] == []
    for name in a:
        assert a[name] == b[name], name


def test_pure_silence_is_skipped(backend, world):
    s = _setup(world)
    out, r = _cli(world, "silence", [world.files[0], str(s["dir"] / "silence.wav")], ["--segment", "long"] + SEG_FLAGS)
    assert r["utterances"] == 1 and r["skipped"] == ["silence"] and "no speech" in r["skipped_reasons"]["silence"]
    assert os.listdir(out / "wav_24000hz_griffin_lim") == ["src4.wav"]
    rows = _tsv(out / "segments.tsv")
    assert len(rows) == 3 and all(r_["id"] == "silence" and r_["dropped"] == "1" and r_["out_start_s"] == "" for r_ in rows)


# ---- 4. the segment CLI ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("segmenter", ["device", "host"])
def test_segment_cli(backend, tmp_path, segmenter):
    SEG = TT._mod("segment")
    x, y = SC.burst_pause(500, 31, burst=40, pause=8), SC.white_noise(90, 32)
    open(tmp_path / "talk.wav", "wb").write(TF._wav_bytes(x, 16000))
    open(tmp_path / "short.wav", "wb").write(TF._wav_bytes(y, 16000))
    out = tmp_path / "out"
    r = SEG.main([str(tmp_path / "talk.wav"), str(tmp_path / "short.wav"), "--results-path", str(out), "--max-segment-s", "1.2",
                  "--min-segment-s", "0.3", "--segment-pad-ms", "30", "--segmenter", segmenter, "--write-wavs"],
                 device=backend.device)
    rows = _tsv(out / "segments.tsv")
    assert list(rows[0]) == ["id", "k", "src_start_s", "src_end_s", "trim_start_s", "trim_end_s", "dropped"]
    assert r["recordings"] == 2 and r["segments"] == len(rows)
    smp = lambda v: int(round(float(v) * 16000))  # noqa: E731
    for name, sig in (("talk", x), ("short", y)):
        mine = [r_ for r_ in rows if r_["id"] == name]
        assert [int(r_["k"]) for r_ in mine] == list(range(len(mine)))
        assert smp(mine[0]["src_start_s"]) == 0 and smp(mine[-1]["src_end_s"]) == len(sig)  # the rows tile [0, n) ..
        assert all(smp(a["src_end_s"]) == smp(b["src_start_s"]) for a, b in zip(mine, mine[1:]))  # .. without gaps
        h = _sg().host_segment(sig, 16000, 30, 120, pad=3)
        assert len(mine) == len(h)
        for k, r_ in enumerate(mine):
            assert (smp(r_["src_start_s"]), smp(r_["src_end_s"])) == tuple(h.samples[k]) and int(r_["dropped"]) == h.dropped[k]
            n = smp(r_["src_end_s"]) - smp(r_["src_start_s"])
            assert SC_frames(n, SC.WIN, SC.HOP) <= 120  # every segment is at most the limit
            if not h.dropped[k]:
                a, b = smp(r_["trim_start_s"]), smp(r_["trim_end_s"])
                assert (a, b) == tuple(h.trim_samples[k])
                rate, w = TT._wav(out / "wav" / f"{name}#{k}.wav")
                assert rate == 16000 and np.array_equal(w, sig[a:b])
    assert len([r_ for r_ in rows if r_["id"] == "talk"]) >= 5 and len([r_ for r_ in rows if r_["id"] == "short"]) == 1
    with pytest.raises(SystemExit, match="twice"):
        SEG.main([str(tmp_path / "talk.wav"), "--results-path", str(out), "--max-segment-s", "1", "--min-segment-s", "0.6",
                  "--segmenter", "host"])
