"""Scorers the generation scripts report (``fairseq/scoring``): word error rate and sacrebleu's corpus BLEU.

``WerScorer`` mirrors fairseq/scoring/wer.py:28-61 with its default configuration (tokenizer "none", no lowercasing, no
punctuation removal, word level): both strings are split on whitespace, the edit distance of the two token lists is
accumulated, ``score() = 100 * distance / reference length``.  The reference delegates the distance to the third-party
``editdistance`` package (un-pinned, absent from this image): ``editdistance.eval`` is the Levenshtein distance --
unit-cost insertions, deletions and substitutions -- restated here as the textbook two-row dynamic programme.

``WerScorer(cfg)`` honours the scorer's four options (fairseq/scoring/wer.py:13-24, ``--wer-tokenizer --wer-lowercase
--wer-remove-punct --wer-char-level``) through ``EvaluationTokenizer`` (fairseq/scoring/tokenizer.py:53-67), in its order:
tokenizer, punctuation removal by Unicode category ``P*``, character tokenisation with U+2581 for spaces, lowercasing.
The reference takes the tokenizers from sacrebleu, which is absent from this image.  ``none`` is the identity.  ``13a``
(``tokenize_13a``) is a restatement of the published rules of mteval-v13a as sacrebleu states them -- **parity unpinned**:
no sacrebleu was at hand to compare against.  ``intl``, ``zh`` and ``ja-mecab`` are refused by name.

``SacrebleuScorer`` mirrors fairseq/scoring/bleu.py:46-71: both strings go through ``EvaluationTokenizer``
(``sacrebleu_tokenizer``, default ``13a``; ``sacrebleu_lowercase``; ``sacrebleu_char_level``) and the score is sacrebleu's
``corpus_bleu(pred, [ref], tokenize="none")``, restated in ``corpus_bleu`` below from its published definition: clipped
n-gram counts of orders 1 - 4 summed over the corpus, the default ``exp`` smoothing (the k-th order without a match counts
as 1 / 2^k of a match; a corpus without any match at all scores 0.0 before smoothing), the brevity penalty ``exp(1 - ref_len / hyp_len)`` for a short system output, the geometric mean of
the four precisions, and the line sacrebleu's ``.format()`` prints -- **parity unpinned**, for the same reason.  fairseq's
token-id ``bleu`` scorer (its C extension) stays out of this path.
"""
from __future__ import annotations

import re
import unicodedata
import math
from collections import Counter
from typing import List, Sequence

SPACE, SPACE_ESCAPE = chr(32), chr(9601)
TOKENIZERS = ("none", "13a")
REFUSED_TOKENIZERS = ("intl", "zh", "ja-mecab")

_13A_RULES = (
    (re.compile(r"([\{-\~\[-\` -\&\(-\+\:-\@\/])"), r" \1 "),  # punctuation other than . , - becomes a token
    (re.compile(r"([^0-9])([\.,])"), r"\1 \2 "),                   # a period / comma not preceded by a digit
    (re.compile(r"([\.,])([^0-9])"), r" \1 \2"),                   # ... or not followed by one
    (re.compile(r"([0-9])(-)"), r"\1 \2 "),                        # a dash after a digit
)


def tokenize_13a(line: str) -> str:
    """mteval-v13a's tokenisation (sacrebleu's default tokenizer).  Parity unpinned: restated from its published rules."""
    line = line.replace("<skipped>", "").replace("-\n", "").replace("\n", " ")
    if "&" in line:
        line = line.replace("&quot;", '"').replace("&amp;", "&").replace("&lt;", "<").replace("&gt;", ">")
    line = " " + line + " "
    for rx, sub in _13A_RULES:
        line = rx.sub(sub, line)
    return " ".join(line.split())


def remove_punctuation(sent: str) -> str:
    """Drop the space-separated tokens made of punctuation only (Unicode categories P*)."""
    return SPACE.join(t for t in sent.split(SPACE) if not all(unicodedata.category(c)[0] == "P" for c in t))


class EvaluationTokenizer:
    def __init__(self, tokenizer_type: str = "none", lowercase: bool = False, punctuation_removal: bool = False,
                 character_tokenization: bool = False):
        if tokenizer_type in REFUSED_TOKENIZERS:
            raise NotImplementedError(f"--wer-tokenizer {tokenizer_type}: sacrebleu's {tokenizer_type!r} tokenizer is not "
                                      "restated here (available: none, 13a)")
        if tokenizer_type not in TOKENIZERS:
            raise ValueError(f"unknown tokenizer {tokenizer_type!r} (available: none, 13a)")
        self.tokenizer_type, self.lowercase = tokenizer_type, bool(lowercase)
        self.punctuation_removal, self.character_tokenization = bool(punctuation_removal), bool(character_tokenization)

    def tokenize(self, sent: str) -> str:
        out = tokenize_13a(sent) if self.tokenizer_type == "13a" else sent
        if self.punctuation_removal:
            out = remove_punctuation(out)
        if self.character_tokenization:
            out = SPACE.join(list(out.replace(SPACE, SPACE_ESCAPE)))
        if self.lowercase:
            out = out.lower()
        return out


def edit_distance(a: Sequence, b: Sequence) -> int:
    """Levenshtein distance of two sequences (what ``editdistance.eval(a, b)`` returns)."""
    if len(a) < len(b):
        a, b = b, a
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i] + [0] * len(b)
        for j, y in enumerate(b, 1):
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (x != y))
        prev = cur
    return prev[len(b)]


class WerScorer:
    def __init__(self, cfg=None):
        self.cfg = cfg
        opt = (lambda k, d: cfg.get(k, d)) if isinstance(cfg, dict) else (lambda k, d: getattr(cfg, k, d))
        self.tokenizer = EvaluationTokenizer(tokenizer_type=opt("wer_tokenizer", "none") or "none",
                                             lowercase=opt("wer_lowercase", False),
                                             punctuation_removal=opt("wer_remove_punct", False),
                                             character_tokenization=opt("wer_char_level", False))
        self.reset()

    def reset(self):
        self.distance = 0
        self.ref_length = 0

    def add_string(self, ref: str, pred: str):
        ref_items, pred_items = self.tokenizer.tokenize(ref).split(), self.tokenizer.tokenize(pred).split()
        self.distance += edit_distance(ref_items, pred_items)
        self.ref_length += len(ref_items)

    def result_string(self) -> str:
        return f"WER: {self.score():.2f}"

    def score(self) -> float:
        return 100.0 * self.distance / self.ref_length if self.ref_length > 0 else 0


class BleuScore:
    """What sacrebleu's ``corpus_bleu`` returns, as far as this path reads it: ``score``, the parts, ``format()``."""

    def __init__(self, score, counts, totals, precisions, bp, sys_len, ref_len):
        self.score, self.counts, self.totals, self.precisions = score, counts, totals, precisions
        self.bp, self.sys_len, self.ref_len = bp, sys_len, ref_len
        self.ratio = sys_len / ref_len if ref_len else 0.0

    def format(self) -> str:
        prec = "/".join(f"{p:.1f}" for p in self.precisions)
        return (f"BLEU = {self.score:.2f} {prec} (BP = {self.bp:.3f} ratio = {self.ratio:.3f} hyp_len = {self.sys_len:d} "
                f"ref_len = {self.ref_len:d})")

    __str__ = format


def _ngrams(tokens: Sequence[str], max_order: int) -> Counter:
    c: Counter = Counter()
    for n in range(1, max_order + 1):
        for i in range(len(tokens) - n + 1):
            c[tuple(tokens[i:i + n])] += 1
    return c


def corpus_bleu(hyps: Sequence[str], refs: Sequence[str], max_order: int = 4) -> BleuScore:
    """sacrebleu's corpus BLEU of whitespace-tokenised lines against ONE reference each (``tokenize="none"``, smoothing
    ``exp``, no effective order).  Parity unpinned: restated from the published definition."""
    if len(hyps) != len(refs):
        raise ValueError("one reference per hypothesis")
    counts, totals = [0] * max_order, [0] * max_order
    sys_len = ref_len = 0
    for h, r in zip(hyps, refs):
        ht, rt = h.split(), r.split()
        sys_len += len(ht)
        ref_len += len(rt)
        hn, rn = _ngrams(ht, max_order), _ngrams(rt, max_order)
        for g, c in hn.items():
            totals[len(g) - 1] += c
            counts[len(g) - 1] += min(c, rn.get(g, 0))
    precisions = [0.0] * max_order
    if not any(counts):  # no n-gram of any order matches: 0.0 outright, before any smoothing (as sacrebleu does)
        return BleuScore(0.0, counts, totals, precisions, 0.0, sys_len, ref_len)
    smooth = 1.0
    for n in range(max_order):
        if totals[n] == 0:
            break
        if counts[n] == 0:
            smooth *= 2.0
            precisions[n] = 100.0 / (smooth * totals[n])
        else:
            precisions[n] = 100.0 * counts[n] / totals[n]
    if sys_len < ref_len:
        bp = math.exp(1.0 - ref_len / sys_len) if sys_len > 0 else 0.0
    else:
        bp = 1.0
    log = lambda p: math.log(p) if p > 0.0 else -9999999999.0  # noqa: E731  (a precision of zero: a score of zero)
    score = bp * math.exp(sum(log(p) for p in precisions) / max_order)
    return BleuScore(score, counts, totals, precisions, bp, sys_len, ref_len)


class SacrebleuScorer:
    def __init__(self, cfg=None):
        self.cfg = cfg
        opt = (lambda k, d: cfg.get(k, d)) if isinstance(cfg, dict) else (lambda k, d: getattr(cfg, k, d))
        self.tokenizer = EvaluationTokenizer(tokenizer_type=opt("sacrebleu_tokenizer", "13a") or "13a",
                                             lowercase=opt("sacrebleu_lowercase", False),
                                             character_tokenization=opt("sacrebleu_char_level", False))
        self.reset()

    def reset(self):
        self.ref: List[str] = []
        self.pred: List[str] = []

    def add_string(self, ref: str, pred: str):
        self.ref.append(self.tokenizer.tokenize(ref))
        self.pred.append(self.tokenizer.tokenize(pred))

    def corpus(self, order: int = 4) -> BleuScore:
        if order != 4:
            raise NotImplementedError
        return corpus_bleu(self.pred, self.ref)  # (tokenisation and lowercasing were done by self.tokenizer)

    def score(self, order: int = 4) -> float:
        return self.corpus(order).score

    def result_string(self, order: int = 4) -> str:
        return self.corpus(order).format()


def build_scorer(choice, tgt_dict=None, cfg=None):
    """fairseq/scoring/__init__.py:39-48 for the scorers this path uses; ``cfg`` carries the ``wer_*`` / ``sacrebleu_*``
    options."""
    name = getattr(choice, "_name", choice)
    if name == "sacrebleu":
        return SacrebleuScorer(cfg)
    if name != "wer":
        raise ValueError(f"scorer {name!r} is not part of this path (available: 'wer', 'sacrebleu')")
    return WerScorer(cfg)
