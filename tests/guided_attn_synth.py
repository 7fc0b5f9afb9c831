"""Seeded inputs of the guided-attention kernel tests (tests/test_guided_attention.py) -- shared with
tools/gen_golden_t2s_guided.py, which records the reference module's value and a float64 restatement on the same input, so
that test and golden cannot drift apart (the golden stores the input's fingerprint)."""
import numpy as np

# forward kernel: wave and workgroup edges on both sides, length 1 on either side, a full-size utterance
FWD_B, FWD_S, FWD_T = 5, 70, 131
FWD_LENS = ((70, 131), (1, 1), (64, 64), (65, 1), (1, 130))  # (source positions, decoder steps)
SIGMA = 0.4


def fwd_input():
    """attn [B][S][T] fp32, src_lens, tgt_lens: every valid decoder step holds a random probability row over the valid
    source positions (non-negative, sums to 1); every cell outside a length holds NaN-free garbage (7.5 ... 8.5) that a
    kernel reading past a length would add to its sum."""
    rng = np.random.RandomState(20240607)
    attn = (7.5 + rng.rand(FWD_B, FWD_S, FWD_T)).astype(np.float32)
    for b, (sl, tl) in enumerate(FWD_LENS):
        rows = rng.rand(sl, tl) ** 3 + 1e-3  # peaky rows
        attn[b, :sl, :tl] = (rows / rows.sum(0, keepdims=True)).astype(np.float32)
    src = np.array([l[0] for l in FWD_LENS], dtype=np.int32)
    tgt = np.array([l[1] for l in FWD_LENS], dtype=np.int32)
    return attn, src, tgt


def fingerprint(x):
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1).astype(np.float64)
    return np.array([x.sum(), np.abs(x).sum(), (x * np.arange(1, x.size + 1)).sum() / x.size])


def guided_weight_f64(sl, tl, sigma):
    """W [tl][sl] of one utterance in float64 (criterions/t2s_loss.py:60-67)."""
    t = np.arange(tl, dtype=np.float64)[:, None]
    s = np.arange(sl, dtype=np.float64)[None, :]
    return 1.0 - np.exp(-((s / sl - t / tl) ** 2) / (2.0 * sigma ** 2))


def guided_sum_f64(attn, src, tgt, sigma):
    """(sum over the valid cells of W * attn, cell count N) in float64; attn [B][S][T]."""
    tot, n = 0.0, 0
    for b in range(attn.shape[0]):
        sl, tl = int(src[b]), int(tgt[b])
        tot += float((guided_weight_f64(sl, tl, sigma) * attn[b, :sl, :tl].astype(np.float64).T).sum())
        n += sl * tl
    return tot, n
