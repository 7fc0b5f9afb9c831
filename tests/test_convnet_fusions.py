"""The convolutional sub-networks' fused launches against the launches they replace (S2ST_CONVNET_FUSE):

* BatchNorm forward with the statistics' finalize inside the apply kernel (s2st_bn_stats_apply[_img]_f32) against
  s2st_bn_stats_f32 + s2st_bn_apply[_img]_f32;
* BatchNorm backward with the sums' fold inside the dx kernel and the convolution's bf16 halo image out of the same
  kernel (s2st_bn_bwd_fused_f32) against s2st_bn_bwd_twin_f32 + s2st_halo_image_bf16_f32;
* GLU written as bf16 operand images (s2st_glu_fwd_img_f32 / s2st_glu_bwd_img_f32) against s2st_glu_fwd_f32 +
  s2st_cast_bf16_halo_f32 / s2st_glu_bwd_twin_f32 + s2st_halo_image_bf16_f32;
* the mel loss' gradients with the post-net residual added inside (s2st_mel_loss_resid_f32) against s2st_mel_loss_f32 +
  s2st_dropout_f32 used as an accumulating copy;
* one training step of the micro model with the fused forms against S2ST_CONVNET_FUSE=0.

The fused kernels do the same arithmetic in the same order: every comparison with the unfused launches is exact (bit
patterns) on the emulator and on the GPU.  That needed one expression pinned: left to the compiler, the one-element dx kernel
fused both multiply-adds of `du - s0 / n - xhat * s1 / n` while the four-column fused body kept a packed multiply, 98 ulp
apart where the terms cancel; `bn_bwd_dx_value` now spells out the fused forms the old kernel always had.  The fused results
also meet the torch references at the tolerances of tests/test_ops.py::test_batchnorm_train on both backends."""
import importlib

import pytest
import torch
import torch.nn.functional as F

from test_engine import DATA, MICRO, make_engine

EPS = 1e-5
NAN16 = 0x7FC1  # a bf16 NaN: an image element the kernel missed shows up


def dev(b, *ts):
    return [t.to(b.device) if t is not None else None for t in ts]


def close(a, b, rtol, atol, msg=""):
    torch.testing.assert_close(a.detach().cpu().double(), b.detach().cpu().double(), rtol=rtol, atol=atol, msg=msg or None)


def same(a, b, what):
    a, b = a.cpu(), b.cpu()
    if a.is_floating_point():  # bit patterns: -0 / +0 and NaNs count
        a, b = a.view(torch.int32), b.view(torch.int32)
    assert torch.equal(a, b), f"{what}: {int((a != b).sum())} of {a.numel()} elements differ"


def same_elementwise(backend, new, old, names, derived, what):
    """fp32 element results of a fused body (`names`) and the bf16 tensors made of them (`derived`) against the launches
    they replace: the same bits on both backends"""
    for k in list(names) + list(derived):
        same(new[k], old[k], f"{k} {what}")


def nan_image(b, *shape):
    return torch.full(shape, NAN16, dtype=torch.int16, device=b.device)


def bf16_bits(x):
    """fp32 -> bf16 (round to nearest even) as int16 bit patterns"""
    return x.detach().cpu().to(torch.bfloat16).view(torch.int16)


def halo_ref(rows_bits, B, T, pad, C, stride=1, Th=None):
    """[B * T][C] int16 -> [B][Th][C] with the rows at pad + stride * t, zeros elsewhere"""
    Th = Th if Th is not None else T + 2 * pad
    img = torch.zeros(B, Th, C, dtype=torch.int16)
    img[:, pad:pad + stride * T:stride][:, :T] = rows_bits.view(B, T, C)
    return img


def bn_inputs(rows, C, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, C, generator=g) * 1.5 + 0.3
    gam, bet = torch.randn(C, generator=g), torch.randn(C, generator=g)
    dy, res = torch.randn(rows, C, generator=g), torch.randn(rows, C, generator=g)
    return x, gam, bet, dy, res


def act(u, tanh_):
    return torch.tanh(u) if tanh_ == 1 else (torch.relu(u) if tanh_ == 2 else u)


def bn_reference(x, gam, bet, dy, res, tanh_):
    """torch BatchNorm1d in training mode (+ activation, + residual) and its backward, as in test_batchnorm_train"""
    C = x.shape[1]
    bn = torch.nn.BatchNorm1d(C)
    with torch.no_grad():
        bn.weight.copy_(gam)
        bn.bias.copy_(bet)
    bn.train()
    xr = x.clone().requires_grad_()
    y = act(bn(xr), tanh_)
    y.backward(dy)
    return dict(y=y.detach() + (res if res is not None else 0), rm=bn.running_mean, rv=bn.running_var, dx=xr.grad,
                dg=bn.weight.grad, db=bn.bias.grad)


def stat_bufs(b, C):
    z = lambda v: torch.full((C,), v, device=b.device)
    # mean, var, running mean, running var, scratch (S2ST_BN_TMP_FLOATS(C), poisoned)
    return z(0.0), z(0.0), z(0.25), z(1.5), torch.full((130 * C,), float("nan"), device=b.device)


# (rows, C): one slab; 6 slabs; 62 slabs with a 2-row last one (not a multiple of the 16-slab load batch); columns that
# are no multiple of 64 in every case, more than one column block in the last two.  B * T = rows for the image forms
SHAPES = [(1, 5, 40), (3, 32, 40), (4, 275, 72), (3, 32, 320)]
ACT_DROP = [(t, p) for t in (0, 1, 2) for p in (0.0, 0.5)]


@pytest.mark.parametrize("B,T,C", SHAPES, ids=lambda v: str(v))
def test_batchnorm_forward_plain(backend, B, T, C):
    rows = B * T
    x, gam, bet, dy, res = bn_inputs(rows, C, 3 + rows + C)
    xd, gd, bd_, resd = dev(backend, x, gam, bet, res)
    sp = backend.bd.make_split(C)
    for tanh_, p in ACT_DROP:
        seed = 77 if p > 0 else 0
        out = []
        for fused in (False, True):
            mean, var, rm, rv, tmp = stat_bufs(backend, C)
            y = torch.full_like(xd, float("nan"))
            if fused:
                backend.bd.call("s2st_bn_stats_apply_f32", xd, rows, C, mean, var, rm, rv, 0.1, tmp, gd, bd_, y, sp, resd, EPS,
                                tanh_, p, seed)
            else:
                backend.bd.call("s2st_bn_stats_f32", xd, rows, C, mean, var, rm, rv, 0.1, tmp)
                backend.bd.call("s2st_bn_apply_f32", xd, mean, var, gd, bd_, y, sp, resd, rows, C, EPS, tanh_, p, seed)
            backend.sync()
            out.append(dict(y=y, mean=mean, var=var, rm=rm, rv=rv))
        for k in ("mean", "var", "rm", "rv"):
            same(out[1][k], out[0][k], f"{k} tanh={tanh_} p={p}")
        same_elementwise(backend, out[1], out[0], ["y"], [], f"tanh={tanh_} p={p}")
        if p == 0.0 and rows > 1:
            ref = bn_reference(x, gam, bet, dy, res, tanh_)
            close(out[1]["y"], ref["y"], 1e-5, 1e-5)
            close(out[1]["rm"], 0.9 * 0.25 + ref["rm"], 1e-5, 1e-6)          # (torch's buffers start at 0 / 1)
            close(out[1]["rv"], 0.9 * 1.5 + (ref["rv"] - 0.9), 1e-5, 1e-6)


@pytest.mark.parametrize("B,T,C", [(3, 7, 40)] + SHAPES, ids=lambda v: str(v))
def test_batchnorm_forward_image(backend, B, T, C):
    rows, pad = B * T, 2
    x, gam, bet, dy, _ = bn_inputs(rows, C, 5 + rows + C)
    xd, gd, bd_ = dev(backend, x, gam, bet)
    for tanh_, p in ACT_DROP:
        seed = 1234567 if p > 0 else 0
        out = []
        for fused in (False, True):
            mean, var, rm, rv, tmp = stat_bufs(backend, C)
            y = torch.full_like(xd, float("nan"))
            img = nan_image(backend, B, T + 2 * pad, C)
            if fused:
                backend.bd.call("s2st_bn_stats_apply_img_f32", xd, B, T, pad, C, mean, var, rm, rv, 0.1, tmp, gd, bd_, y, img, EPS,
                                tanh_, p, seed)
            else:
                backend.bd.call("s2st_bn_stats_f32", xd, rows, C, mean, var, rm, rv, 0.1, tmp)
                backend.bd.call("s2st_bn_apply_img_f32", xd, mean, var, gd, bd_, y, img, B, T, pad, C, EPS, tanh_, p, seed)
            backend.sync()
            out.append(dict(y=y, img=img, mean=mean, var=var, rm=rm, rv=rv))
        for k in ("mean", "var", "rm", "rv"):
            same(out[1][k], out[0][k], f"{k} tanh={tanh_} p={p}")
        same_elementwise(backend, out[1], out[0], ["y"], ["img"], f"tanh={tanh_} p={p}")
        # the image is the bf16 rounding of y between zero halos
        same(out[1]["img"], halo_ref(bf16_bits(out[1]["y"]), B, T, pad, C), "image of y")
        if p == 0.0:
            ref = bn_reference(x, gam, bet, dy, None, tanh_)
            close(out[1]["y"], ref["y"], 1e-5, 1e-5)
    # without the fp32 rows (what the engine asks for)
    mean, var, rm, rv, tmp = stat_bufs(backend, C)
    img = nan_image(backend, B, T + 2 * pad, C)
    backend.bd.call("s2st_bn_stats_apply_img_f32", xd, B, T, pad, C, mean, var, rm, rv, 0.1, tmp, gd, bd_, None, img, EPS, tanh_, p,
                    seed)
    backend.sync()
    same(img, out[1]["img"], "image without y")


@pytest.mark.parametrize("B,T,C", [(3, 7, 40)] + SHAPES, ids=lambda v: str(v))
def test_batchnorm_backward(backend, B, T, C):
    rows, pad = B * T, 2
    x, gam, bet, dy, _ = bn_inputs(rows, C, 7 + rows + C)
    xd, gd, bd_, dyd = dev(backend, x, gam, bet, dy)
    sp = backend.bd.make_split(C)
    mean, var, rm, rv, tmp = stat_bufs(backend, C)
    backend.bd.call("s2st_bn_stats_f32", xd, rows, C, mean, var, rm, rv, 0.1, tmp)
    for tanh_, p in ACT_DROP:
        seed = 99 if p > 0 else 0
        out = []
        for fused in (False, True):
            tmp.fill_(float("nan"))
            dx = torch.full_like(xd, float("nan"))
            dxh = nan_image(backend, rows, C)
            img = nan_image(backend, B, T + 2 * pad, C)
            dg = torch.full((C,), 0.5, device=backend.device)   # the parameter gradients are accumulated into
            db = torch.full((C,), -0.25, device=backend.device)
            if fused:
                backend.bd.call("s2st_bn_bwd_fused_f32", dyd, sp, xd, mean, var, gd, bd_, dx, sp, dg, db, tmp, B, T, pad, C, EPS,
                                tanh_, p, seed, dxh, C, img)
            else:
                backend.bd.call("s2st_bn_bwd_twin_f32", dyd, sp, xd, mean, var, gd, bd_, dx, sp, dg, db, tmp, rows, C, EPS, tanh_, p,
                                seed, dxh, C)
                backend.bd.call("s2st_halo_image_bf16_f32", dxh, C, img, B, T, T + 2 * pad, C, pad, 1)
            backend.sync()
            out.append(dict(dx=dx, dxh=dxh, img=img, dg=dg, db=db))
        for k in ("dg", "db"):
            same(out[1][k], out[0][k], f"{k} tanh={tanh_} p={p}")
        same_elementwise(backend, out[1], out[0], ["dx"], ["dxh", "img"], f"tanh={tanh_} p={p}")
        same(out[1]["dxh"], bf16_bits(out[1]["dx"]), "twin of dx")
        same(out[1]["img"], halo_ref(out[1]["dxh"].cpu(), B, T, pad, C), "image of the twin")
        if p == 0.0 and rows > 1:
            ref = bn_reference(x, gam, bet, dy, None, tanh_)
            close(out[1]["dx"], ref["dx"], 1e-4, 1e-5)
            close(out[1]["dg"], ref["dg"] + 0.5, 1e-4, 1e-4)
            close(out[1]["db"], ref["db"] - 0.25, 1e-4, 1e-4)
    # without an image (a convolution whose input needs no gradient): pad is ignored
    dx = torch.full_like(xd, float("nan"))
    dxh = nan_image(backend, rows, C)
    dg, db = torch.full((C,), 0.5, device=backend.device), torch.full((C,), -0.25, device=backend.device)
    backend.bd.call("s2st_bn_bwd_fused_f32", dyd, sp, xd, mean, var, gd, bd_, dx, sp, dg, db, tmp, B, T, pad, C, EPS, tanh_, p, seed,
                    dxh, C, None)
    backend.sync()
    for k, v in dict(dx=dx, dxh=dxh, dg=dg, db=db).items():
        same(v, out[1][k], f"{k} without image")


@pytest.mark.parametrize("C", [8, 72])
def test_glu_forward_image(backend, C):
    B, T, pad = 3, 5, 2
    Th = T + 2 * pad
    a = torch.randn(B * T, 2 * C, generator=torch.Generator().manual_seed(C))
    ad, = dev(backend, a)
    yimg = torch.full((B, Th, C), float("nan"), device=backend.device)  # (fast mode never clears the fp32 image's halos)
    backend.bd.call("s2st_glu_fwd_f32", ad, yimg.view(-1)[pad * C:], backend.bd.make_split(C, T, Th * C), B * T, C)
    ref = nan_image(backend, B, Th, C)
    backend.bd.call("s2st_cast_bf16_halo_f32", yimg, ref, B, T, pad, C, 0)
    img = nan_image(backend, B, Th, C)
    backend.bd.call("s2st_glu_fwd_img_f32", ad, img, B, T, pad, C)
    backend.sync()
    same(img, ref, "GLU image")
    close(yimg[:, pad:pad + T].reshape(B * T, C), F.glu(a, dim=1), 1e-5, 1e-6)


@pytest.mark.parametrize("Tin", [9, 10])
@pytest.mark.parametrize("C", [8, 72])
def test_glu_backward_image(backend, C, Tin):
    """the stride-2 convolution's zero-stuffed operand: Tout = 5 for both Tin; with Tin = 10 the last image row before the
    halo is a stuffed one"""
    B, pad, stride, Kw = 3, 2, 2, 5
    Tout, Th = (Tin + 2 * pad - Kw) // stride + 1, Tin + 2 * pad
    assert Tout == 5
    rows = B * Tout
    g = torch.Generator().manual_seed(C + Tin)
    a, dy = torch.randn(rows, 2 * C, generator=g), torch.randn(rows, C, generator=g)
    ad, dyd = dev(backend, a, dy)
    ds, das = backend.bd.make_split(C), backend.bd.make_split(2 * C)
    out = []
    for fused in (False, True):
        da = torch.full_like(ad, float("nan"))
        dah = nan_image(backend, rows, 2 * C)
        img = nan_image(backend, B, Th, 2 * C)
        if fused:
            backend.bd.call("s2st_glu_bwd_img_f32", ad, dyd, ds, da, das, B, Tout, Th, pad, stride, C, dah, 2 * C, img)
        else:
            backend.bd.call("s2st_glu_bwd_twin_f32", ad, dyd, ds, da, das, rows, C, dah, 2 * C)
            backend.bd.call("s2st_halo_image_bf16_f32", dah, 2 * C, img, B, Tout, Th, 2 * C, pad, stride)
        backend.sync()
        out.append(dict(da=da, dah=dah, img=img))
    for k in out[0]:
        same(out[1][k], out[0][k], k)
    same(out[1]["dah"], bf16_bits(out[1]["da"]), "twin of da")
    same(out[1]["img"], halo_ref(out[1]["dah"].cpu(), B, Tout, pad, 2 * C, stride, Th), "stuffed image of the twin")
    ar = a.clone().requires_grad_()
    F.glu(ar, dim=1).backward(dy)
    close(out[1]["da"], ar.grad, 1e-5, 1e-6)


def test_mel_loss_backward_adds_the_residual(backend):
    B, D, Fd = 2, 5, 20
    g = torch.Generator().manual_seed(1)
    feat, post, tgt = (torch.randn(B, D, Fd, generator=g) for _ in range(3))
    eos = torch.randn(B, D, generator=g) * 2
    lens = torch.tensor([5, 3], dtype=torch.int32)  # the second utterance is shorter than D
    fd, pd, td, ed, ld = dev(backend, feat, post, tgt, eos, lens)
    c = (0.013, 0.027, 0.4)
    out = []
    for fused in (False, True):
        df, dp = torch.full_like(fd, float("nan")), torch.full_like(fd, float("nan"))
        de = torch.full_like(ed, float("nan"))
        if fused:
            backend.bd.call("s2st_mel_loss_resid_f32", fd, pd, ed, td, ld, B, D, Fd, 1.0, *c, df, dp, de)
        else:
            backend.bd.call("s2st_mel_loss_f32", fd, pd, ed, td, ld, B, D, Fd, 1.0, None, *c, df, dp, de)
            backend.bd.call("s2st_dropout_f32", dp, df, df.numel(), 1.0, 0.0, 0, 1)  # df += dp: the post-net's residual pass
        backend.sync()
        out.append(dict(dfeat=df, dpost=dp, deos=de))
    for k in out[0]:
        same(out[1][k], out[0][k], k)
    assert float(out[1]["dfeat"][1, 3:].abs().max()) == 0.0 and float(out[1]["dfeat"][1, :3].abs().min()) > 0.0


def run_step(backend, cfg, monkeypatch, env):
    D = importlib.import_module(DATA)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    c = D.SyntheticFisherCorpus(n_utts=4, seed=3, max_src=64, median_src=50, min_src=30)
    s = c.collate_batch(range(4))
    a, e = make_engine(backend, cfg, precise=False)
    o = e.forward(s, training=True, seed=9)
    e.zero_grad()
    e.backward(1.0)
    backend.sync()
    res = (o["stats"].clone(), e.grads.clone(), e.buffers.clone(),
           {n: gv.clone() for n, pv, gv, isb in e.named_views() if not isb},
           {k: o[k].clone() for k in ("post_feat_out", "feature_out", "eos_out", "encoder_out")})
    del e
    for k in env:
        monkeypatch.delenv(k)
    return res


def test_training_step_equals_the_unfused_launches(backend, monkeypatch):
    """The micro model of test_fused_backward_paths_equal_the_unfused_ones with its dropouts on: one forward + backward with
    the fused forms (default) and one with S2ST_CONVNET_FUSE=0, same seed, the workspace poisoned with NaNs (an element of an
    operand image that no kernel wrote would spread).  Emulator: the same bits.  GPU: that test's bounds at its tol = 1.0."""
    cfg = dict(MICRO, dropout=0.1, attention_dropout=0.1, activation_dropout=0.05, prenet_dropout=0.5, postnet_dropout=0.5)
    s0, g0, b0, v0, o0 = run_step(backend, cfg, monkeypatch, {"S2ST_POISON_WORKSPACE": "1"})
    s1, g1, b1, v1, o1 = run_step(backend, cfg, monkeypatch, {"S2ST_POISON_WORKSPACE": "1", "S2ST_CONVNET_FUSE": "0"})
    assert torch.isfinite(g0).all() and torch.isfinite(s0).all() and float(g0.norm()) > 0
    if backend.kind == "emu":
        same(s0, s1, "stats")
        same(g0, g1, "gradient arena")
        same(b0, b1, "BatchNorm buffers")
        for k in o0:
            same(o0[k], o1[k], k)
        return
    assert torch.allclose(s0, s1, rtol=1e-5, atol=1e-6)
    print("hip: |g0 - g1| / |g0| =", float((g0 - g1).norm()) / float(g0.norm()), "buffers equal:", torch.equal(b0, b1))
    assert float((g0 - g1).norm()) <= 2e-5 * float(g0.norm())
    gmax = max(float(v.norm()) for v in v0.values())
    for n in v0:
        assert float((v0[n] - v1[n]).norm()) <= 1e-4 * (float(v0[n].norm()) + 1e-2 * gmax), n
    close(b0, b1, 1e-5, 1e-6)
