"""``inference_common.drive``: the one pipelined loop behind ``generate_waveform`` and ``translate``, driven with a fake
generator that records its calls -- the order in which groups are enqueued and finished, grouping, the ``max_batches``
cut, skipping.  No device and no native library."""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
PKG = "speech-to-speech-translation_amd"
MODEL = object()


def _drive(*a, **k):
    return importlib.import_module(PKG + ".inference_common").drive(*a, **k)


class _One:
    """Records ("generate", [tag]) and returns the tagged list a real generator's hypothesis list stands for."""

    def __init__(self, log):
        self.log = log

    def generate(self, model, sample, has_targ=False, defer_vocoder=False):
        assert model is MODEL
        self.log.append(("generate", [sample["tag"]], has_targ, defer_vocoder))
        return ["hyp", sample["tag"]]


class _Many(_One):
    def generate_many(self, model, samples, has_targ=False, defer_vocoder=False):
        assert model is MODEL
        self.log.append(("generate_many", [s["tag"] for s in samples], has_targ, defer_vocoder))
        return (["hyp", s["tag"]] for s in samples)


def _run(gen_cls, tags, **kw):
    log = []

    def finish(sample, hypos):
        assert hypos == ["hyp", sample["tag"]]
        log.append(("finish", [sample["tag"]]))

    samples = (None if t is None else {} if t == "empty" else {"tag": t} for t in tags)
    seconds = _drive(gen_cls(log), MODEL, samples, finish, **kw)
    assert isinstance(seconds, float) and seconds >= 0.0
    return log


def _where(log, kind, tag):
    return next(n for n, e in enumerate(log) if e[0] == kind and tag in e[1])


def test_deferred_finish_follows_the_next_enqueue():
    log = _run(_Many, range(5), chains=1, defer=True)
    assert [e[0] for e in log].count("generate") == 5 and not any(e[0] == "generate_many" for e in log)
    assert all(e[3] is True for e in log if e[0] == "generate")  # defer_vocoder is handed on
    for k in range(5):
        f = _where(log, "finish", k)
        if k + 1 < 5:
            assert _where(log, "generate", k + 1) < f
        if k + 2 < 5:
            assert f < _where(log, "generate", k + 2)
    # drain: the last sample is finished at the end, after every generate
    assert log[-1] == ("finish", [4])
    assert [e[1][0] for e in log if e[0] == "finish"] == list(range(5))


def test_undeferred_finish_precedes_the_next_generate():
    log = _run(_Many, range(4), chains=1, defer=False)
    assert [(e[0], e[1]) for e in log] == [(kind, [k]) for k in range(4) for kind in ("generate", "finish")]
    assert all(e[3] is False for e in log if e[0] == "generate")


def test_grouping_three_chains_over_seven():
    log = _run(_Many, range(7), chains=3, defer=True, has_targ=True)
    calls = [(e[0], e[1]) for e in log if e[0] != "finish"]
    assert calls == [("generate_many", [0, 1, 2]), ("generate_many", [3, 4, 5]), ("generate", [6])]
    assert all(e[2] is True for e in log if e[0] != "finish")  # has_targ reaches both forms
    assert [e[1][0] for e in log if e[0] == "finish"] == list(range(7))
    # a group is finished after the next one has been enqueued
    assert _where(log, "generate_many", 3) < _where(log, "finish", 0) and _where(log, "finish", 2) < _where(log, "generate", 6)
    assert _where(log, "generate", 6) < _where(log, "finish", 3)


def test_max_batches_cuts_the_stream():
    consumed = []

    def stream():
        for t in range(7):
            consumed.append(t)
            yield {"tag": t}

    log = []
    _drive(_Many(log), MODEL, stream(), lambda s, h: log.append(("finish", [s["tag"]])), chains=3, defer=True, max_batches=4)
    assert [(e[0], e[1]) for e in log if e[0] != "finish"] == [("generate_many", [0, 1, 2]), ("generate", [3])]
    assert [e[1][0] for e in log if e[0] == "finish"] == [0, 1, 2, 3]
    assert consumed == [0, 1, 2, 3]  # nothing past the fourth sample is even fetched


def test_skipping_and_a_generator_without_generate_many():
    log = _run(_One, [0, None, "empty", 1, 2, None, 3], chains=3, defer=True)
    assert [(e[0], e[1]) for e in log if e[0] != "finish"] == [("generate", [k]) for k in range(4)]
    assert [e[1][0] for e in log if e[0] == "finish"] == list(range(4))
    # ... and skipped samples do not count as batches
    log = _run(_Many, [None, 0, "empty", 1, 2], chains=2, defer=False, max_batches=2)
    assert [(e[0], e[1]) for e in log] == [("generate_many", [0, 1]), ("finish", [0]), ("finish", [1])]


def test_generate_one_takes_the_single_batches():
    log, own = [], []

    def one(model, sample, has_targ=False, defer_vocoder=False):
        own.append((sample["tag"], has_targ, defer_vocoder))
        return ["hyp", sample["tag"]]

    _drive(_Many(log), MODEL, [{"tag": 0}, {"tag": 1}], lambda s, h: log.append(("finish", [s["tag"]])), chains=1, defer=True,
           generate_one=one, has_targ=True)
    assert own == [(0, True, True), (1, True, True)] and log == [("finish", [0]), ("finish", [1])]
