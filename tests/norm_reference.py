"""Plain torch references of the UNet row kernels (csrc/norm.hip), written from the formulas alone.

Every function computes in the dtype of its inputs: the tests call them with fp64 tensors for the reference and with fp32 tensors for
the "same formula in single precision" whose distance to the fp64 result scales the tests' bounds.  Gradients come from autograd of the
forward written here, never from a hand-derived backward.  Activations are (B, L, C) channels-last, as the kernels see them.
tests/test_norm_reference_cpu.py checks these functions against torch.nn.functional and the UNet oracle.
"""
from __future__ import annotations

import torch

EPS = 1e-5


def cast(dtype, *ts):
    """CPU copies of tensors (None passes through) in `dtype`."""
    return [None if t is None else t.detach().to("cpu", dtype) for t in ts]


def gn_stats(y):
    """GroupNorm(1, C) statistics per sample over L x C: (B, 2) = (mean, rstd), biased variance, eps 1e-5."""
    mean = y.mean((1, 2))
    var = ((y - mean[:, None, None]) ** 2).mean((1, 2))
    return torch.stack([mean, 1.0 / torch.sqrt(var + EPS)], 1)


def gn_film_silu(y, gamma, beta, ss=None, identity_norm=False):
    """h = silu((xhat * gamma + beta) * (1 + scale) + shift); ss = (B, 2C) holding scale | shift, or None.
    identity_norm: Block(norm=False) -- xhat = y, no gamma / beta.  -> (h, mean_rstd (B, 2) or None)."""
    C = y.shape[-1]
    if identity_norm:
        u, mr = y, None
    else:
        mr = gn_stats(y)
        u = (y - mr[:, 0, None, None]) * mr[:, 1, None, None] * gamma + beta
    if ss is not None:
        u = u * (1 + ss[:, None, :C]) + ss[:, None, C:]
    return u * torch.sigmoid(u), mr


def gn_grads(y, gamma, beta, ss, dh, identity_norm=False):
    """Autograd of gn_film_silu under the cotangent dh -> dict of dy, dgamma, dbeta, dss (B, 2C), and the two column sums the backward
    kernel also emits: dbias = sum_{b,l} dy (gradient of the bias of the convolution that produced y) and dyy = sum_{b,l} dy * y."""
    y = y.clone().requires_grad_()
    gamma, beta = gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    ss = ss.clone().requires_grad_() if ss is not None else None
    h, _ = gn_film_silu(y, gamma, beta, ss, identity_norm)
    h.backward(dh)
    dy = y.grad
    return {"dy": dy, "dgamma": None if identity_norm else gamma.grad, "dbeta": None if identity_norm else beta.grad,
            "dss": ss.grad if ss is not None else None, "dbias": dy.sum((0, 1)), "dyy": (dy * y.detach()).sum((0, 1))}


def layer_norm(x, gamma, beta):
    """LayerNorm over the last dim, eps 1e-5 -> (out, mean_rstd (..., 2))."""
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + EPS)
    return (x - mean) * rstd * gamma + beta, torch.cat([mean, rstd], -1)


def ln_grads(x, gamma, beta, dy):
    x, gamma, beta = x.clone().requires_grad_(), gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    out, _ = layer_norm(x, gamma, beta)
    out.backward(dy)
    return {"dx": x.grad, "dgamma": gamma.grad, "dbeta": beta.grad}


def gca_pool(h, wk, bk=None):
    """GlobalContext pooling: p = softmax_l(h . wk + bk) (B, L), pooled = sum_l p h (B, C)."""
    logit = h @ wk
    if bk is not None:
        logit = logit + bk
    p = torch.softmax(logit, 1)
    return p, torch.einsum("bl,blc->bc", p, h)


def gate_residual(h, gate, res=None):
    out = h * gate[:, None, :]
    return out if res is None else out + res


def gca_grads(dout, h, gate, dpooled, wk, bk):
    """What osuf_gca_bwd_apply computes, restated from its caller (functional.GCAPoolFn._backward): h feeds out = h * gate + res and the
    pooling whose result makes the gate.  The kernel receives the cotangent of out (dout), the gate as a constant (B, C) and the
    cotangent of pooled (dpooled, already taken through the gate MLP), so its outputs are the autograd gradients of
        dout . (h * gate)  +  dpooled . pooled(h, wk, bk)
    with gate held fixed: dh, dlogit (of the pooling logits), dwk and dbk.  dbk = sum dlogit is zero analytically (softmax is
    shift invariant); it is returned as computed."""
    h, wk, bk = h.clone().requires_grad_(), wk.clone().requires_grad_(), bk.clone().requires_grad_()
    logit = h @ wk + bk
    logit.retain_grad()
    p = torch.softmax(logit, 1)
    pooled = torch.einsum("bl,blc->bc", p, h)
    ((dout * gate_residual(h, gate)).sum() + (dpooled * pooled).sum()).backward()
    return {"dh": h.grad, "dlogit": logit.grad, "dwk": wk.grad, "dbk": bk.grad,
            "p": p.detach(), "pooled": pooled.detach(), "sdot": (pooled.detach() * dpooled).sum(1)}


def wcolsum(a, bmul, w):
    """out[b][c] = sum_l w[b][l] * a[b][l][c] * bmul[b][l][c]   (w, bmul optional -> 1)."""
    t = a if bmul is None else a * bmul
    return t.sum(1) if w is None else torch.einsum("bl,blc->bc", w, t)
