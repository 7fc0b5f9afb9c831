"""Inputs shared by tests/test_ctc_align.py: seeded log-probabilities, targets with runs of repeated labels, and the
enumeration of every labeling of a tiny case (the definition the host form is checked against)."""
import itertools

import numpy as np


def log_softmax(x):
    x = x - x.max(-1, keepdims=True)
    return (x - np.log(np.exp(x).sum(-1, keepdims=True))).astype(np.float32)


def random_target(rng, L, V, blank, p_repeat=0.4):
    """L labels != blank; each repeats its predecessor with probability p_repeat (runs of repeated labels)."""
    labels = [v for v in range(V) if v != blank]
    out = []
    for i in range(L):
        if i and (len(labels) == 1 or rng.random() < p_repeat):
            out.append(out[-1])
        else:
            out.append(int(labels[rng.integers(len(labels))]))
    return out


def repeats(target):
    return sum(1 for a, b in zip(target, target[1:]) if a == b)


def enumerate_best(lp, target, blank=0):
    """All V^T labelings of lp [T][V]; among those that collapse to ``target`` the best and second-best sums (float64)
    and the best labeling.  (None, -inf, -inf) when no labeling collapses to it."""
    T, V = lp.shape
    lab = np.array(list(itertools.product(range(V), repeat=T)), dtype=np.int64).reshape(-1, T)  # [V^T][T]
    prev = np.concatenate([np.full((len(lab), 1), -1), lab[:, :-1]], axis=1)
    keep = (lab != blank) & (lab != prev)
    idx = np.cumsum(keep, axis=1) - 1
    L = len(target)
    tg = np.asarray(list(target) + [-1], dtype=np.int64)  # (index L: never equal to a label)
    ok = (keep.sum(1) == L) & np.all(~keep | (lab == tg[np.clip(idx, 0, L)]), axis=1)
    if not ok.any():
        return None, -np.inf, -np.inf
    sums = lp.astype(np.float64)[np.arange(T)[None, :], lab[ok]].sum(1)
    order = np.argsort(-sums, kind="stable")
    best = sums[order[0]]
    second = sums[order[1]] if len(order) > 1 else -np.inf
    return lab[ok][order[0]], best, second


def frame_labels(alignment, target, blank, n_frames):
    """frame_tok (target indices) -> vocabulary ids per frame."""
    ft = alignment.frame_tok[:n_frames]
    return np.array([blank if i < 0 else target[i] for i in ft], dtype=np.int64)


def collapse(path, blank):
    out, prev = [], None
    for v in path:
        v = int(v)
        if v != prev and v != blank:
            out.append(v)
        prev = v
    return out
