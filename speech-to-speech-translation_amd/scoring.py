"""Scorers the generation scripts report (``fairseq/scoring``): word error rate.

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
"""
from __future__ import annotations

import re
import unicodedata
from typing import Sequence

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


def build_scorer(choice, tgt_dict=None, cfg=None):
    """fairseq/scoring/__init__.py:39-48 for the scorer this path uses; ``cfg`` carries the ``wer_*`` options."""
    name = getattr(choice, "_name", choice)
    if name != "wer":
        raise ValueError(f"scorer {name!r} is not part of this path (the mtl generator scores with 'wer')")
    return WerScorer(cfg)
