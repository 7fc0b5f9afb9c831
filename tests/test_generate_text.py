"""``python -m s2st_amd.generate_text`` (stages 10 / 11 of the recipes, fairseq_cli/generate_for_s2st.py) end to end on the
miniature on-disk corpus, and the scorer options of ``--scoring wer`` (fairseq/scoring/wer.py + tokenizer.py)."""
import argparse
import importlib
import os
import re

import pytest

PKG = "speech-to-speech-translation_amd"


def _checkpoint(backend, tmp_path):
    from data_corpus import make_corpus
    from synth_weights import load_synth
    from test_resume import NANO_FLAGS
    T = importlib.import_module(PKG + ".train")
    corpus = make_corpus(str(tmp_path / "corpus"))
    argv = [corpus, "--config-yaml", "config.yaml", "--train-subset", "train_tiny", "--valid-subset", "dev_tiny",
            "--max-tokens", "120", "--required-batch-size-multiple", "2", "--max-update", "1", "--lr", "1e-3",
            "--warmup-updates", "2", "--seed", "3", "--precise-gemm", "--save-dir", str(tmp_path / "ckpt"),
            "--disable-validation", "--log-interval", "1"] + NANO_FLAGS
    import torch
    threads = torch.get_num_threads()
    try:
        T.main(argv, device=backend.device, on_model_built=lambda m: load_synth(m, 0))
    finally:
        torch.set_num_threads(threads)  # (train.main pins the process to one intra-op thread; later tests' sums depend on it)
    ckpt = str(tmp_path / "ckpt" / "checkpoint_last.pt")
    assert os.path.isfile(ckpt)
    return corpus, ckpt


def _lines(path):
    with open(path, encoding="utf-8") as f:
        return f.read().split("\n")


def _without_timing(lines):
    """The throughput line carries wall-clock figures; its counts are compared, its seconds and rates are not."""
    out = []
    for l in lines:
        m = re.fullmatch(r"(Translated [\d,]+ sentences \([\d,]+ tokens\)) in .*", l)
        out.append(m.group(1) if m else l)
    return out


def test_generate_text_end_to_end(backend, tmp_path):
    GT = importlib.import_module(PKG + ".generate_text")
    GW = importlib.import_module(PKG + ".generate_waveform")
    S = importlib.import_module(PKG + ".scoring")
    corpus, ckpt = _checkpoint(backend, tmp_path)
    nbest, beam, subset = 2, 3, "dev_tiny"
    common = [corpus, "--config-yaml", "config.yaml", "--gen-subset", subset, "--path", ckpt, "--max-tokens", "400", "--beam",
              str(beam), "--nbest", str(nbest), "--max-len-b", "6", "--precise-gemm"]
    files, scorers = {}, {}
    for tag, extra in (("device", ["--scoring", "wer", "--search", "device"]), ("host", ["--scoring", "wer", "--search", "host"]),
                       ("st", ["--scoring", "sacrebleu"])):
        out = tmp_path / tag
        scorers[tag] = GT.main(common + extra + ["--results-path", str(out)], device=backend.device)
        backend.sync()
        files[tag] = _lines(out / f"generate-{subset}.txt")
    n_utt = 4  # dev_tiny: utt2 .. utt5
    for tag in ("device", "host", "st"):
        L = files[tag]
        assert L[-1] == "" and L[-2].startswith(f"Generate {subset} with beam={beam}: "), tag
        assert L[-3].startswith(f"Translated {n_utt} sentences ("), tag
        ids = [l.split("\t")[0][2:] for l in L if l.startswith("T-")]
        assert sorted(ids) == sorted(str(i) for i in range(n_utt)), tag
        for i in ids:  # per utterance: T, then nbest x (H, D, P), in that order
            k = L.index(next(l for l in L if l.startswith(f"T-{i}\t")))
            block = L[k + 1:k + 1 + 3 * nbest]
            assert [b.split("\t")[0] for b in block] == [f"H-{i}", f"D-{i}", f"P-{i}"] * nbest, (tag, i)
            for j in range(nbest):
                h, d, p = (b.split("\t") for b in block[3 * j:3 * j + 3])
                assert h[1] == d[1] and h[2] == d[2] and float(h[1]) < 0
                assert len(p[1].split(" ")) >= len(h[2].split()) + 1  # a score per token, EOS (and any <s>, not printed) included
                assert all(re.fullmatch(r"-?\d+\.\d{4}|-inf", x) for x in p[1].split(" "))
        assert sum(l.startswith("H-") for l in L) == n_utt * nbest and not any(l.startswith("S-") for l in L), tag
    # the two search forms write the same file (apart from the wall-clock figures of the throughput line)
    assert _without_timing(files["device"]) == _without_timing(files["host"])
    assert scorers["st"] is None and "BLEU is not computed here" in files["st"][-2]
    assert isinstance(scorers["device"], S.WerScorer)

    # the H- strings are Dictionary.string of what AuxSequenceGenerator returns for the same batches; the closing line's WER
    # is WerScorer fed the (T, D) pairs of the first hypotheses
    args = GT.make_parser().parse_args(common + ["--scoring", "wer", "--search", "host", "--results-path", str(tmp_path / "x")])
    for which, tag in (("asr", "host"), ("st", "st")):
        task, model, margs, dataset = GW.load_task_model_dataset(args, backend.device)
        args.aux_decoder = which
        gen = task.build_generator([model], args)
        assert gen.which == which and gen.tgt_dict is (task.src_dict if which == "asr" else task.tgt_dict)
        want = {}
        for sample in GW.batch_iterator(task, dataset, args):
            hypos = gen.generate([model], sample)
            for i, sid in enumerate(sample["id"].tolist()):
                want[str(sid)] = [gen.tgt_dict.string(h["tokens"]) for h in hypos[i][:nbest]]
        backend.sync()
        got = {}
        for l in files[tag]:
            if l.startswith("H-"):
                sid, _, s = l.split("\t")
                got.setdefault(sid[2:], []).append(s)
        assert got == want, which
    w = S.WerScorer()
    L = files["device"]
    for k, l in enumerate(L):
        if l.startswith("T-"):
            w.add_string(l.split("\t")[1], L[k + 2].split("\t")[2])
    assert w.ref_length > 0
    assert L[-2] == f"Generate {subset} with beam={beam}: {w.result_string()}"
    assert scorers["device"].score() == scorers["host"].score() == w.score()


# ---- scorer options (CPU) ----------------------------------------------------------------------------------------------------
def _tok(**kw):
    S = importlib.import_module(PKG + ".scoring")
    return S.EvaluationTokenizer(**kw)


def test_scorer_option_stages_and_their_order():
    """Expected values from fairseq/scoring/tokenizer.py read line by line: remove_punctuation drops the SPACE-separated
    tokens made only of category-P characters (:45-51); character tokenisation replaces spaces by U+2581 and puts a space
    between all characters (:59-62); lowercasing comes last (:64-65)."""
    S = importlib.import_module(PKG + ".scoring")
    assert S.remove_punctuation("hello , world !") == "hello world"
    assert S.remove_punctuation("hello, world!") == "hello, world!"  # (punctuation glued to a word is not a token of its own)
    assert S.remove_punctuation("¿ qué ? — sí … «ok» +") == "qué sí «ok» +"  # (P* is Unicode-wide; '+' is Sm, not P)
    assert S.remove_punctuation("a  , b") == "a b"  # (split on single spaces: the empty token counts as all-punctuation)
    assert _tok(character_tokenization=True).tokenize("ab c") == "a b ▁ c"
    assert _tok(lowercase=True).tokenize("Hello WORLD") == "hello world"
    assert _tok().tokenize("  Keep  As , Is. ") == "  Keep  As , Is. "  # the defaults: identity
    # the order: tokenizer -> punctuation -> characters -> lowercase.  Punctuation removal sees the 13a tokens (so the comma
    # glued to "Hi" goes), the character stage sees the text without them, lowercasing the characters
    t = _tok(tokenizer_type="13a", lowercase=True, punctuation_removal=True, character_tokenization=True)
    assert t.tokenize("Hi, YOU!") == "h i ▁ y o u"
    # (were punctuation removed BEFORE the tokenizer, "Hi," would keep its comma; were characters split before the removal,
    #  every "," would be a token of its own and go, and the U+2581 marks next to it would stay)
    assert _tok(tokenizer_type="none", punctuation_removal=True, character_tokenization=True).tokenize("Hi, YOU !") == \
        "H i , ▁ Y O U"
    for name in ("intl", "zh", "ja-mecab"):
        with pytest.raises(NotImplementedError, match=name):
            _tok(tokenizer_type=name)
    with pytest.raises(ValueError):
        _tok(tokenizer_type="moses")


def test_wer_scorer_honours_its_options():
    S = importlib.import_module(PKG + ".scoring")
    plain = S.WerScorer()
    plain.add_string("Hello , world", "hello world")
    assert (plain.distance, plain.ref_length) == (2, 3)  # today's defaults: split on whitespace, nothing else
    cfg = argparse.Namespace(wer_tokenizer="none", wer_lowercase=True, wer_remove_punct=True, wer_char_level=False)
    w = S.WerScorer(cfg)
    w.add_string("Hello , world", "hello world")
    assert (w.distance, w.ref_length) == (0, 2) and w.result_string() == "WER: 0.00"
    c = S.WerScorer({"wer_char_level": True})
    c.add_string("ab c", "ab d")
    assert (c.distance, c.ref_length) == (1, 4)  # a b U+2581 c
    assert S.build_scorer("wer", None, cfg=cfg).tokenizer.lowercase is True
    with pytest.raises(NotImplementedError):
        S.WerScorer(argparse.Namespace(wer_tokenizer="zh"))


def test_13a_tokenizer_rules_parity_unpinned():
    """PARITY UNPINNED: sacrebleu is not installed, these are the cases the published rule list of mteval-v13a defines."""
    S = importlib.import_module(PKG + ".scoring")
    t = S.tokenize_13a
    assert t('Hello, world! "Quoted" (text); a/b') == 'Hello , world ! " Quoted " ( text ) ; a / b'
    assert t("It costs 1,000 dollars or 3.14 euros") == "It costs 1,000 dollars or 3.14 euros"  # digits keep , and .
    assert t("The end.") == "The end ."  # a trailing period is split
    assert t("AT&amp;T said &quot;no&quot; &lt;b&gt;") == 'AT & T said " no " < b >'
    assert t("pages 5-6 of a well-known book") == "pages 5 - 6 of a well-known book"  # a dash after a digit only
    assert t("  many   spaces\nand a line ") == "many spaces and a line"
    assert t("x <skipped> y") == "x y"
