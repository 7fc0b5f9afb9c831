"""The fused attention path without the fp32 stores nobody reads (default) against S2ST_ATTN_KEEP_F32=1, which also stores
O in fp32 out of the forward kernels and dO in fp32 out of the out-projection's data-gradient GEMM.  Every reader takes
the bf16 copies either way, so losses, outputs and the whole gradient arena are the same bits on both backends.

The model is the micro model at head width 64 (the variant of test_micro_engine_fused_attention_vs_oracle): at the micro
model's own head width of 16 the engine takes the unfused attention path and neither form would run.  The workspace is
poisoned with NaNs, so a read of the never-written fp32 tensors would spread into the results."""
import importlib

import pytest
import torch

from test_engine import DATA, MICRO, make_engine

CFG = dict(MICRO, encoder_embed_dim=128, decoder_embed_dim=128, encoder_attention_heads=2, decoder_attention_heads=2,
           dropout=0.1, attention_dropout=0.1, activation_dropout=0.05, prenet_dropout=0.5, postnet_dropout=0.5)
OUTS = ("post_feat_out", "feature_out", "eos_out", "encoder_out")


def bits_equal(a, b, what):
    a, b = a.cpu().view(torch.int32), b.cpu().view(torch.int32)
    assert torch.equal(a, b), f"{what}: {int((a != b).sum())} of {a.numel()} elements differ"


def step(backend, monkeypatch, env, sample):
    env = dict(env, S2ST_POISON_WORKSPACE="1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    a, e = make_engine(backend, CFG, precise=False)
    o = e.forward(sample, training=True, seed=9)
    e.zero_grad()
    e.backward(1.0)
    backend.sync()
    res = (o["stats"].clone(), e.grads.clone())
    del e
    for k in env:
        monkeypatch.delenv(k)
    return res


@pytest.fixture(scope="module")
def sample():
    D = importlib.import_module(DATA)
    c = D.SyntheticFisherCorpus(n_utts=4, seed=3, max_src=64, median_src=50, min_src=30)
    return c.collate_batch(range(4))


@pytest.mark.parametrize("split", ["", "1"], ids=["default", "S2ST_ATTN_BWD_SPLIT"])
def test_training_step_without_fp32_o_and_do(backend, monkeypatch, sample, split):
    base = {"S2ST_ATTN_BWD_SPLIT": split} if split else {}
    s0, g0 = step(backend, monkeypatch, base, sample)
    s1, g1 = step(backend, monkeypatch, dict(base, S2ST_ATTN_KEEP_F32="1"), sample)
    assert torch.isfinite(s0).all() and torch.isfinite(g0).all() and float(g0.norm()) > 0
    bits_equal(s0, s1, "stats")
    bits_equal(g0, g1, "gradient arena")


@pytest.mark.parametrize("max_src", [64, 600], ids=["short", "long"])
def test_inference_forward_without_fp32_o(backend, monkeypatch, max_src):
    """training=False: no reader of fp32 O either.  short: T, S <= 128 (the one-workgroup-per-head forward kernel); long:
    encoder length > 128 (the streaming forward kernel) -- both with o = null"""
    D = importlib.import_module(DATA)
    c = D.SyntheticFisherCorpus(n_utts=2, seed=4, max_src=max_src, median_src=max_src - 10, min_src=max_src - 30)
    s = c.collate_batch(range(2))
    res = []
    for keep in (False, True):
        monkeypatch.setenv("S2ST_POISON_WORKSPACE", "1")
        if keep:
            monkeypatch.setenv("S2ST_ATTN_KEEP_F32", "1")
        a, e = make_engine(backend, CFG, precise=False)
        o = e.forward(s, training=False, with_loss=False)
        backend.sync()
        res.append({k: o[k].clone() for k in OUTS})
        E = o["encoder_out"].shape[1]
        del e
    monkeypatch.delenv("S2ST_ATTN_KEEP_F32")
    assert (E > 128) == (max_src > 128), E
    for k in OUTS:
        assert torch.isfinite(res[0][k]).all(), k
        bits_equal(res[0][k], res[1][k], k)
