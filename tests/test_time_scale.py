"""Time-scale modification of 16-bit PCM (csrc/time_scale.hip, time_scale.py, translate --tempo / --timeline source): the host
form against a scalar restatement on small cases full of ties, the consequences of the definition, the placement rule on
numbers written out here, the device form against the host form bit for bit (outputs and positions) on ragged batches at three
geometries, and ``translate`` end to end.  Every comparison is exact.  PARITY UNPINNED: the reference has no time-scale
modification; the definition is the one in include/s2st_hip.h."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import time_scale_cases as TC  # noqa: E402
import test_segment as TS  # noqa: E402
import test_translate as TT  # noqa: E402
from test_translate import world  # noqa: E402,F401  (the fixture: corpus, stage 3 and a one-update checkpoint per backend)

PKG = "speech-to-speech-translation_amd"
GPU_ONLY = pytest.mark.parametrize("backend", [pytest.param("hip", marks=pytest.mark.gpu)], indirect=True)


def _ts():
    return importlib.import_module(PKG + ".time_scale")


# ---- 1. the host form against the scalar restatement (CPU) ------------------------------------------------------------------------
def test_host_form_against_the_scalar_restatement():
    M = _ts()
    cases = TC.small_cases(320)
    tied = short_in = short_out = ragged_out = 0
    for x, m, N, D in cases:
        want, want_pos, ties = TC.scalar_time_scale(x, m, N, D)
        got, pos = M.host_time_scale(x, m, N, D)
        assert got.dtype == np.int16 and pos.dtype == np.int32
        assert np.array_equal(got, want) and np.array_equal(pos, want_pos), (x.tolist(), m, N, D, got, want, pos, want_pos)
        tied += ties > 0
        short_in += len(x) < N
        short_out += m < N // 2
        ragged_out += m % (N // 2) != 0
    # no case is skipped; equal costs abound; the short and the ragged lengths occur
    assert len(cases) >= 300 and tied >= 100 and short_in >= 10 and short_out >= 5 and ragged_out >= 50, \
        (tied, short_in, short_out, ragged_out)


# ---- 2. what the definition implies (CPU) ------------------------------------------------------------------------------------------
def test_the_same_length_returns_the_input():
    M = _ts()
    for seed, (n, N, D) in enumerate(((0, 8, 3), (1, 8, 3), (5, 16, 0), (333, 64, 16), (1000, 64, 5), (2000, 960, 240))):
        x = np.random.RandomState(seed).randint(-32768, 32768, n).astype(np.int16)
        y, pos = M.host_time_scale(x, n, N, D)
        assert np.array_equal(y, x) and np.array_equal(pos, np.arange(len(pos)) * (N // 2))


@pytest.mark.parametrize("n,m", [(1200, 1200), (1200, 960), (1200, 601), (1200, 777), (700, 701), (700, 875), (700, 1050),
                                 (700, 1400)])
def test_a_periodic_signal_stays_the_same_periodic_signal(n, m):
    """Exact period P <= D, Hs >= P.  Compressed (m <= n): all m samples.  Stretched: a hop costs nothing and copies its
    template while the template lies inside the recording, and p_{j-1} <= a_{j-1} + D always, so every hop j with
    a_{j-1} + D + 2 Hs <= n is exact whatever the ratio -- asserted for every stretch here.  The tighter "all but the last Hs +
    D samples" is asserted at the ratios 701/700, 1.25 and 1.5; at a ratio of 2 it does not follow from the definition (the
    scalar restatement agrees): the first sample that differs lies 63 (N 64, D 16, P 7) and 128 (N 128, D 20, P 11) before the
    end, where Hs + D is 48 and 84."""
    M = _ts()
    for N, D, P in ((64, 16, 7), (64, 16, 16), (32, 16, 16), (64, 40, 32), (128, 20, 11)):
        Hs = N // 2
        x = TC.periodic(n, P, seed=P)
        y, pos = M.host_time_scale(x, m, N, D)
        want = TC.periodic(m, P, seed=P)
        a = np.arange(len(pos), dtype=np.int64) * Hs * n // m
        assert np.all(np.abs(pos - a) <= D)
        if m <= n:
            assert np.array_equal(y, want), (N, D, P)
            continue
        exact = 1 + max(j for j in range(1, len(pos)) if a[j - 1] + D + 2 * Hs <= n)  # hops 0 .. exact - 1
        assert np.array_equal(y[:exact * Hs], want[:exact * Hs]), (N, D, P)
        if m * 2 <= n * 3:
            assert np.array_equal(y[:m - (Hs + D)], want[:m - (Hs + D)]), (N, D, P)


def test_positions_stay_within_the_search_radius():
    M = _ts()
    for seed, (n, m, N, D) in enumerate(((500, 400, 64, 16), (500, 1000, 64, 0), (300, 150, 16, 9), (2400, 1920, 960, 240),
                                         (40, 3000, 64, 16), (3000, 40, 64, 16))):  # (the last two: far outside any tempo)
        x = TC.noise_tone(n, seed)
        y, pos = M.host_time_scale(x, m, N, D)
        Hs = N // 2
        a = np.arange(len(pos), dtype=np.int64) * Hs * n // m
        assert len(y) == m and len(pos) == -(-m // Hs) and pos[0] == 0 and np.all(np.abs(pos[1:] - a[1:]) <= D)


def test_geometry_and_refusals():
    M = _ts()
    assert M.geometry(24000) == (960, 240) and M.geometry(16000) == (640, 160) and M.geometry(8000) == (320, 80)
    x = np.zeros(100, np.int16)
    for N, D in ((0, 1), (3, 1), (4098, 1), (8, -1), (8, 2049)):
        with pytest.raises(ValueError, match="frame length"):
            M.host_time_scale(x, 100, N, D)
        with pytest.raises(ValueError, match="frame length"):
            M.time_scale([x], [100], N=N, D=D, scaler="host")
    for m in (49, 201, 0):  # a tempo outside [1/2, 2]: refused with a message; the definition itself is total
        with pytest.raises(ValueError, match="outside"):
            M.time_scale([x], [m], N=8, D=2, scaler="host")
        assert len(M.host_time_scale(x, m, 8, 2)[0]) == m
    assert [len(y) for y, _ in M.time_scale([x, x, x[:0]], [50, 200, 0], N=8, D=2, scaler="host")] == [50, 200, 0]
    with pytest.raises(ValueError, match="rate"):
        M.time_scale([x], [100], scaler="host")
    with pytest.raises(ValueError, match="int16"):
        M.time_scale([x.astype(np.float32)], [100], rate=24000, scaler="host")
    with pytest.raises(ValueError, match="scaler"):
        M.time_scale([x], [100], rate=24000, scaler="sox")
    assert M.scaled_len(1000, 1250) == 800 and M.scaled_len(1001, 1250) == 801 and M.scaled_len(7, 1000) == 7


# ---- 3. the placement rule on numbers written out here (CPU) ---------------------------------------------------------------------
def test_place():
    place = _ts().place
    # everything fits: starts are the source's, lengths the natural ones
    assert place([100, 1000, 2500], [500, 1200, 300], 3000, 1000, 1250) == ([100, 1000, 2500], [500, 1200, 300])
    # one segment compressed exactly to its slot: 1100 samples into the 1000 up to the next start (1.1 <= 1.25)
    assert place([0, 1000, 2500], [1100, 800, 100], 3000, 1000, 1250) == ([0, 1000, 2500], [1000, 800, 100])
    # capped by the limit: 2000 samples cannot go below ceil(2000 / 1.25) = 1600 > 1000; it overruns to 1600, the follower (room
    # 2000 - 1600 = 400 for its 600: least 480) goes to 480 and ends at 2080, which pushes the third (room 3000 - 2080 = 920 >= 300)
    assert place([0, 1000, 2000], [2000, 600, 300], 3000, 1000, 1250) == ([0, 1600, 2080], [1600, 480, 300])
    # the last one runs past the source's end: 900 into 500 is capped at 720
    assert place([0, 2500], [100, 900], 3000, 1000, 1250) == ([0, 2500], [100, 720])
    # a single segment; one of no samples; none at all
    assert place([40], [100], 1000, 1000, 1250) == ([40], [100])
    assert place([40], [0], 1000) == ([40], [0])
    assert place([], [], 1000) == ([], [])
    # a tempo of its own: want = ceil(n / 1.1); never slower than that; the limit still counts from the natural length
    assert place([0, 1000], [1000, 1001], 3000, 1100, 1250) == ([0, 1000], [910, 910])
    assert place([0, 500], [1000, 100], 3000, 1100, 1250) == ([0, 800], [800, 91])
    assert place([0, 1000], [880, 10], 3000, 800, 1250) == ([0, 1000], [1000, 13])  # 1100 wanted, 1000 there, 704 the least
    # max tempo == tempo: nothing is compressed beyond the tempo
    assert place([0, 100], [1000, 10], 3000, 1000, 1000) == ([0, 1000], [1000, 10])
    for bad in (dict(starts=[0, 1], natural=[1]), dict(starts=[5, 4], natural=[1, 1]), dict(starts=[-1], natural=[1]),
                dict(starts=[0], natural=[-1]), dict(starts=[0], natural=[1], total=-1),
                dict(starts=[0], natural=[1], tempo_milli=0), dict(starts=[0], natural=[1], tempo_milli=1300, max_tempo_milli=1250)):
        kw = dict(dict(total=10, tempo_milli=1000, max_tempo_milli=1250), **bad)
        with pytest.raises(ValueError):
            place(**kw)


# ---- 4. - 6. device equals host, bit for bit (both backends at the small geometry) ----------------------------------------------
def _compare_batch(backend, N, D, max_hops, period):
    M = _ts()
    rec = TC.ragged_batch(N, D, max_hops, period)
    got = M.time_scale([x for _, x, _ in rec], [m for _, _, m in rec], N=N, D=D, device=backend.device)
    backend.sync()
    want = M.time_scale([x for _, x, _ in rec], [m for _, _, m in rec], N=N, D=D, scaler="host")
    Hs = N // 2
    for (name, x, m), (y, pos), (hy, hpos) in zip(rec, got, want):
        assert y.dtype == np.int16 and pos.dtype == np.int32 and len(y) == m and len(pos) == -(-m // Hs), name
        assert np.array_equal(pos, hpos), (name, pos, hpos)
        assert np.array_equal(y, hy), (name, np.flatnonzero(y != hy)[:8])
    by = {name: (x, m, y, pos) for (name, x, m), (y, pos) in zip(rec, got)}
    assert np.array_equal(by["ratio 1"][2], by["ratio 1"][0])                     # the same length: the input
    assert not by["zeros"][2].any() and np.all(by["all -32768"][2] == -32768)
    full = by["all 32767"]
    assert np.all(full[2][:max(0, len(full[0]) - Hs - D)] == 32767)
    x, m, y, pos = by["odd period"]
    if len(pos) >= 12:  # (the four hops of the largest geometry are compared with the host form only)
        assert np.array_equal(y, TC.periodic(m, period, 10))                      # compressed: the same periodic signal
        k = pos[1:] - (np.arange(1, len(pos), dtype=np.int64) * Hs * len(x) // m) + D  # the chosen candidates' offsets in the region
        assert (k % 2 == 1).any() and (k % 2 == 0).any() and (k % 4 == 3).any()
    return rec, got


@pytest.mark.parametrize("odd", ["funnel", "image"])
def test_device_equals_host_on_the_ragged_batch(backend, monkeypatch, odd):
    """Both forms of the candidates at odd offsets (the library reads S2ST_TS_ODD at every call; unset: the one it chose)."""
    monkeypatch.setenv("S2ST_TS_ODD", odd)
    rec, got = _compare_batch(backend, 64, 16, 22, 7)
    # a recording alone gives the bytes it gives inside the batch
    M = _ts()
    for b in (9, 11, 16, 5):
        name, x, m = rec[b]
        (y, pos), = M.time_scale([x], [m], N=64, D=16, device=backend.device)
        assert np.array_equal(y, got[b][0]) and np.array_equal(pos, got[b][1]), name


def test_the_kernel_is_total(backend):
    """Far outside any tempo (the Python entry's guard off), the smallest frame, no search at all, a frame of odd half-length."""
    M = _ts()
    cases = [(TC.noise_tone(300, 1), 7, 64, 16), (TC.noise_tone(5, 2), 300, 64, 16), (np.zeros(0, np.int16), 40, 64, 16),
             (TC.noise_tone(90, 3), 70, 2, 0), (TC.noise_tone(90, 4), 111, 2, 5), (TC.noise_tone(200, 5), 170, 6, 3),
             (TC.noise_tone(200, 6), 260, 14, 1), (TC.noise_tone(200, 7), 150, 64, 0), (TC.noise_tone(150, 8), 200, 10, 40)]
    for x, m, N, D in cases:
        (y, pos), = M.time_scale([x], [m], N=N, D=D, device=backend.device, guard=False)
        hy, hpos = M.host_time_scale(x, m, N, D)
        assert np.array_equal(pos, hpos) and np.array_equal(y, hy), (len(x), m, N, D)


@GPU_ONLY
@pytest.mark.parametrize("odd", ["funnel", "image"])
@pytest.mark.parametrize("N,D,max_hops,period", [(960, 240, 40, 237), (4096, 2048, 4, 2047)], ids=["960-240", "4096-2048"])
def test_device_equals_host_at_the_larger_geometries(backend, monkeypatch, N, D, max_hops, period, odd):
    """The default geometry at 24 kHz (0.8 s at most per recording) and the largest the entry point takes (four hops)."""
    monkeypatch.setenv("S2ST_TS_ODD", odd)
    _compare_batch(backend, N, D, max_hops, period)


def test_the_library_refuses_bad_arguments(backend):
    """S2ST_ERR_ARG (-4) from the entry point itself; nothing is launched (the outputs keep their sentinel)."""
    lib, dev = backend.bd.lib(), backend.device
    pcm = torch.zeros(400, dtype=torch.int16, device=dev)
    off = torch.tensor([0, 400], dtype=torch.int64).to(dev)
    poff = torch.tensor([0, 13], dtype=torch.int64).to(dev)
    out = torch.full((400,), 77, dtype=torch.int16, device=dev)
    pos = torch.full((13,), 77, dtype=torch.int32, device=dev)

    def call(N=64, D=16, B=1):
        return lib.s2st_time_scale_pcm16(pcm.data_ptr(), off.data_ptr(), off.data_ptr(), B, N, D, out.data_ptr(), pos.data_ptr(),
                                         poff.data_ptr(), None)

    for kw in (dict(N=63), dict(N=4098), dict(N=0), dict(N=1), dict(D=-1), dict(D=2049), dict(B=-1)):
        assert call(**kw) == -4, kw
    assert call(B=0) == 0
    backend.sync()
    assert bool((out == 77).all()) and bool((pos == 77).all())
    assert call() == 0 and call(N=4096, D=2048) == 0 and call(N=2, D=0) == 0
    backend.sync()
    assert not bool(out.any())


# ---- 7. - 9. translate end to end (GPU) ---------------------------------------------------------------------------------------
SHORT = ["--segment", "long", "--max-segment-s", "0.3", "--min-segment-s", "0.1", "--segment-pad-ms", "20"]
SHORT_OPTS = dict(max_segment_s=0.3, min_segment_s=0.1, segment_pad_ms=20.0)


def _placed(world, hyp):
    """What ``--timeline source`` has to make of a cut recording's hypothesis: (pcm, spans, lengths, tempo strings)."""
    M = _ts()
    seg, ks = hyp["segmentation"], hyp["segment_ids"]
    natural = [len(h["pcm"]) for h in hyp["segments"]]
    starts = [int(seg.trim_samples[k][0]) * 24000 // 16000 for k in ks]
    L = -(-seg.n_samples * 24000 // 16000)
    at, lens = M.place(starts, natural, L, 1000, 1250)
    want = np.zeros(max([L] + [a + m for a, m in zip(at, lens)]), np.int16)
    for a, m, h in zip(at, lens, hyp["segments"]):
        want[a:a + m] = M.host_time_scale(h["pcm"], m, 960, 240)[0]
    return want, at, lens, natural, L


def _files(world):
    """A cut of dev utterance 0 short enough to stay whole under SHORT, and the long recording of tests/test_segment.py."""
    import test_feature_extraction as TF
    s = TS._setup(world)
    tiny = s["dir"] / "tiny.wav"
    if not tiny.exists():
        open(tiny, "wb").write(TF._wav_bytes(world.pcm(0)[0][:4000], 16000))
    return s, [str(tiny), str(s["dir"] / "long.wav")]


@GPU_ONLY
def test_translate_on_the_source_time_line(backend, world):
    s, files = _files(world)
    tr = world.translator(ckpt=s["ckpt"], max_tokens=400, text="both", beam=2, max_len_b=5, segment="long", **SHORT_OPTS)
    np.random.seed(TT.PHASE_SEED)
    whole = tr.translate([(world.pcm(0)[0][:4000], 16000), (s["long"], 16000)], ids=["tiny", "long"], timeline="source")
    backend.sync()
    hyp = whole[1]
    want, at, lens, natural, L = _placed(world, hyp)
    assert tr.skipped == [] and len(hyp["segment_ids"]) >= 4 and L == len(s["long"]) * 3 // 2
    assert any(m < n for m, n in zip(lens, natural)) and any(a > int(hyp["segmentation"].trim_samples[k][0]) * 3 // 2
                                                             for a, k in zip(at, hyp["segment_ids"]))  # compressed; pushed
    assert len(hyp["pcm"]) == max(L, at[-1] + lens[-1]) and np.array_equal(hyp["pcm"], want)
    assert hyp["out_spans"] == {k: (a, a + m) for k, a, m in zip(hyp["segment_ids"], at, lens)}
    covered = np.zeros(len(want), bool)
    for a, m in zip(at, lens):
        covered[a:a + m] = True
    assert not hyp["pcm"][~covered].any() and (~covered).any()  # zeros wherever no segment lies
    assert "out_spans" not in whole[0] and len(whole[0]["pcm"]) == len(hyp["segments"][0]["pcm"])  # not cut: as before

    # the CLI writes that wav, the spans and the tempo column; the host scaler writes the same files
    flags = SHORT + ["--timeline", "source"]
    out, r = TS._cli(world, "source", files, flags)
    assert r["utterances"] == 2 and r["skipped"] == []
    rate, got = TT._wav(out / "wav_24000hz_griffin_lim" / "long.wav")
    assert rate == 24000 and np.array_equal(got, want)
    rows = TS._tsv(out / "segments.tsv")
    assert list(rows[0]) == ["id", "k", "src_start_s", "src_end_s", "trim_start_s", "trim_end_s", "dropped", "out_start_s",
                             "out_end_s", "asr", "st", "tempo"]
    live = [r_ for r_ in rows if r_["dropped"] == "0"]
    assert [int(r_["k"]) for r_ in live] == hyp["segment_ids"]
    for r_, a, m, n in zip(live, at, lens, natural):
        assert (int(round(float(r_["out_start_s"]) * 24000)), int(round(float(r_["out_end_s"]) * 24000))) == (a, a + m)
        assert r_["tempo"] == f"{n / m:.6f}"
    assert all(r_["tempo"] == "" for r_ in rows if r_["dropped"] == "1")
    host, _ = TS._cli(world, "source_host", files, flags + ["--time-scaler", "host"])
    a, b = TS._tree(out), TS._tree(host)
    assert sorted(a) == sorted(b) and all(a[name] == b[name] for name in a)
    # the input of that call that was not cut: the file of a call without the flag
    c = TS._tree(TS._cli(world, "short", files, SHORT)[0])
    wav = lambda name: os.path.join("wav_24000hz_griffin_lim", name)  # noqa: E731
    assert a[wav("tiny.wav")] == c[wav("tiny.wav")] and a[wav("long.wav")] != c[wav("long.wav")]
    assert [r_["id"] for r_ in rows] == ["long"] * len(rows)


@GPU_ONLY
def test_the_default_flags_write_what_a_call_without_them_writes(backend, world):
    s, files = _files(world)
    plain, _ = TS._cli(world, "short", files, SHORT)
    same, r = TS._cli(world, "short_defaults", files, SHORT + ["--timeline", "joined", "--tempo", "1.0"])
    a, b = TS._tree(plain), TS._tree(same)
    assert sorted(a) == sorted(b) and "segments.tsv" in a and r["skipped"] == []
    for name in a:
        assert a[name] == b[name], name
    T = TT._mod("translate")
    for extra, why in ((["--timeline", "source"], "--segment long"), (["--tempo", "2.5"], "outside"),
                       (["--tempo", "1.3", "--max-tempo", "1.25"], "at least")):
        with pytest.raises(SystemExit, match=why):
            T.main([str(world.data), "--path", s["ckpt"], "--results-path", str(s["dir"] / "refused"), "--inputs"] + s["files"][:1] +
                   extra, device=backend.device)


@GPU_ONLY
def test_tempo_on_uncut_inputs(backend, world):
    M = _ts()
    batching = ("--max-tokens", "400")
    plain, _ = world.translate("stems", batching, ["--inputs"] + world.files)
    fast, r = world.translate("stems_tempo", batching, ["--inputs"] + world.files, ["--tempo", "1.25"])
    assert r["utterances"] == len(world.files) and r["skipped"] == []
    for f in world.files:
        name = os.path.splitext(os.path.basename(f))[0] + ".wav"
        rate, x = TT._wav(plain / "wav_24000hz_griffin_lim" / name)
        rate2, y = TT._wav(fast / "wav_24000hz_griffin_lim" / name)
        assert rate == rate2 == 24000 and len(y) == -(-len(x) * 1000 // 1250) and len(x) > 960
        assert np.array_equal(y, M.host_time_scale(x, len(y), 960, 240)[0]), name


# ---- the time_scale CLI ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scaler", ["device", "host"])
def test_time_scale_cli(backend, tmp_path, scaler):
    import test_feature_extraction as TF
    M = _ts()
    x, y = TC.noise_tone(1600, 1), TC.noise_tone(700, 2)
    open(tmp_path / "a.wav", "wb").write(TF._wav_bytes(x, 1600))
    open(tmp_path / "b.wav", "wb").write(TF._wav_bytes(y, 3200))
    out = tmp_path / "out"
    r = M.main([str(tmp_path / "a.wav"), str(tmp_path / "b.wav"), "--results-path", str(out), "--tempo", "0.8", "--time-scaler",
                scaler], device=backend.device)
    assert r["recordings"] == 2 and r["tempo_milli"] == 800
    for name, sig, rate in (("a", x, 1600), ("b", y, 3200)):
        got_rate, w = TT._wav(out / f"{name}.wav")
        N, D = M.geometry(rate)
        assert got_rate == rate and len(w) == -(-len(sig) * 1000 // 800) and (N, D) == (2 * rate // 50, rate // 100)
        assert np.array_equal(w, M.host_time_scale(sig, len(w), N, D)[0])
    with pytest.raises(SystemExit, match="outside"):
        M.main([str(tmp_path / "a.wav"), "--results-path", str(out), "--tempo", "3", "--time-scaler", "host"])
