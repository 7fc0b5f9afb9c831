"""References for the fused attention kernels (attention.hip), shared by the tests that drive them.

* ``reference``: a float64 restatement of fairseq MultiheadAttention's core (multihead_attention.py:224-367): q scaling,
  key-padding / causal masks, softmax, dropout on the probabilities (an INJECTED keep mask: ``P * mask`` after the softmax
  and before P*V, :360-367), P*V, and autograd for the backward.  This is what the kernels are compared with.
* ``rounding_model``: the same computation in float64 with the kernels' bf16 rounding points put in by hand.  It is never
  compared with a kernel: a test runs it on its own inputs to show that the precision the kernels work at leaves room
  under the test's bounds (an input on which bf16 arithmetic alone uses up the bound would test nothing).
* ``dropout_keep``: the keep mask of a call, regenerated through the C ABI the way tests/test_dropout_parity.py does.
"""
import torch


def rel(x, y):
    return float((x.double().cpu() - y).abs().max() / (y.abs().max() + 1e-12))


def _heads(x, H):
    B, L, Cm = x.shape
    return x.view(B, L, H, Cm // H).permute(0, 2, 1, 3)


def _masks(B, T, S, klen, causal):
    """(masked [B,1,T,S] bool, alive [B] bool): an element with no valid key (klen = 0) is `not alive` -- its softmax is
    over an empty set; the kernels define O = 0, lse = -inf and zero gradients there, and so do the references."""
    masked = torch.zeros(B, 1, T, S, dtype=torch.bool)
    alive = torch.ones(B, dtype=torch.bool)
    if klen is not None:
        kl = klen.long().clamp(max=S)  # a length past the end is the whole row
        masked |= (torch.arange(S)[None, :] >= kl[:, None])[:, None, None, :]
        alive = kl > 0
        masked[~alive] = False  # computed unmasked, zeroed below: no NaN enters autograd
    if causal:
        masked |= (torch.arange(S)[None, :] > torch.arange(T)[:, None])[None, None]
    return masked, alive


def reference(q, k, v, H, klen, causal, dO=None, keep=None, scale=None):
    """float64.  keep: [B, H, T, S] multiplier of the probabilities (0 or 1 / (1 - p)), or None."""
    B, T, Cm = q.shape
    S = k.shape[1]
    dh = Cm // H
    scale = dh ** -0.5 if scale is None else scale
    q, k, v = (x.double().requires_grad_(True) for x in (q, k, v))
    s = (_heads(q, H) * scale) @ _heads(k, H).transpose(-1, -2)
    masked, alive = _masks(B, T, S, klen, causal)
    s = s.masked_fill(masked, float("-inf"))
    p = torch.softmax(s, -1)
    if keep is not None:
        p = p * keep.double()
    live = alive.double()[:, None, None, None]
    o = ((p @ _heads(v, H)) * live).permute(0, 2, 1, 3).reshape(B, T, Cm)
    lse = torch.logsumexp(s, -1).masked_fill(~alive[:, None, None], float("-inf"))
    if dO is None:
        return o.detach(), lse.detach()
    o.backward(dO.double())
    return o.detach(), lse.detach(), q.grad, k.grad, v.grad


def _bf16(x):
    return x.float().to(torch.bfloat16).double()


def rounding_model(q, k, v, H, klen, causal, dO, keep=None, scale=None, bf16_out=True):
    """The kernels' arithmetic in float64 with their bf16 rounding points (attention.hip):

    * forward (flash_fwd_kernel / flash_fwd_short_kernel): p = exp(s - max) is summed into l unrounded, then multiplied
      by the keep factor and packed to bf16 (``pack_frag(p)``) as the operand of P*V; O = acc / l;
    * O is stored as bf16 (``pack_bf16x4`` into oh) and the backward forms D = rowsum(dO * O) from the bf16 copies of both
      (``tile_rowdots`` / ``dot_bf16x8``: the no-fp32-O form the training step uses);
    * backward (flash_bwd_kv_body, flash_bwd_q_body, flash_bwd_short_kernel): P = exp(s - lse); Pd = P * keep and
      dS = P * (keep * dP - D) are packed to bf16 (``pack_frag(pd)``, ``pack_frag(ds)``) as the operands of dV = Pd^T dO,
      dK = dS^T Q and dQ = dS K; the accumulators are scaled in fp32;
    * ``bf16_out``: O and the gradients leave through ``pack_bf16x4`` only (no fp32 copy is requested).

    Products and sums are exact here (the kernels accumulate in fp32: ~1e-7, far below bf16's 4e-3)."""
    B, T, Cm = q.shape
    S = k.shape[1]
    dh = Cm // H
    scale = dh ** -0.5 if scale is None else scale
    qh, kh, vh, doh = (_heads(x.double(), H) for x in (q, k, v, _bf16(dO)))
    masked, alive = _masks(B, T, S, klen, causal)
    live = alive.double()[:, None, None, None]
    s = ((qh @ kh.transpose(-1, -2)) * scale).masked_fill(masked, float("-inf"))
    keep = torch.ones_like(s) if keep is None else keep.double()
    m = s.max(-1, keepdim=True).values
    pu = torch.exp(s - m)
    l = pu.sum(-1, keepdim=True)
    o = (_bf16(pu * keep) @ vh) / l * live
    lse = (m + torch.log(l)).squeeze(-1).masked_fill(~alive[:, None, None], float("-inf"))
    o_seen = _bf16(o)
    D = (doh * o_seen).sum(-1, keepdim=True)
    p = torch.exp(s - (m + torch.log(l))) * live
    pd = _bf16(p * keep)
    ds = _bf16(p * (keep * (doh @ vh.transpose(-1, -2)) - D))
    dv = pd.transpose(-1, -2) @ doh
    dk = (ds.transpose(-1, -2) @ qh) * scale
    dq = (ds @ kh) * scale
    out = [x.permute(0, 2, 1, 3).reshape(B, -1, Cm) for x in (o, dq, dk, dv)]
    if bf16_out:
        out = [_bf16(x) for x in out]
    return out[0], lse, out[1], out[2], out[3]


def dropout_keep(backend, B, H, T, S, ld_drop, p, seed):
    """[B, H, T, S] float64 keep factors (0 or 1 / (1 - p)) of an attention call: s2st_dropout_f32 over ones in the call's
    index space ((b * H + h) * T + t) * ld_drop + s -- the same (seed, element) hash the kernels evaluate."""
    if p <= 0:
        return None
    n = B * H * T * ld_drop
    ones = torch.ones(n, device=backend.device)
    y = torch.zeros(n, device=backend.device)
    backend.bd.call("s2st_dropout_f32", ones, y, n, 1.0, p, seed, 0)
    backend.sync()
    return y.cpu().double().view(B, H, T, ld_drop)[..., :S].contiguous()
