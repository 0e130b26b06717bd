"""The hand-written fp64 references of tests/norm_reference.py against torch.nn.functional and the UNet oracle (CPU only).

tests/test_norm_rows_gpu.py measures the HIP kernels against these functions, so a slip in one of them would either hide a kernel bug
or report one that is not there."""
import torch
import torch.nn.functional as F

from oracle import unet_oracle as O
from tests import norm_reference as R
from tests.test_poisoned_memory import relmax, rnd

TOL = 1e-12                                                # fp64 against fp64: a few hundred ulps of headroom


def _d(tag, shape, scale=1.0):
    return rnd(tag, shape, scale).double()


def test_gn_film_silu_vs_functional():
    B, L, C = 3, 37, 24
    y = _d("y", (B, L, C), 2.0) + 0.7
    gamma, beta = 1 + 0.3 * _d("g", (C,)), 0.2 * _d("b", (C,))
    ss = 0.4 * _d("ss", (B, 2 * C))
    dh = _d("dh", (B, L, C)) + 0.3
    for use_ss in (False, True):
        yr, gr, br = y.clone().requires_grad_(), gamma.clone().requires_grad_(), beta.clone().requires_grad_()
        sr = ss.clone().requires_grad_() if use_ss else None
        u = F.group_norm(yr.transpose(1, 2), 1, gr, br, eps=1e-5).transpose(1, 2)
        if use_ss:
            u = u * (1 + sr[:, None, :C]) + sr[:, None, C:]
        want = F.silu(u)
        want.backward(dh)
        h, mr = R.gn_film_silu(y, gamma, beta, ss if use_ss else None)
        assert relmax(h, want) < TOL
        assert relmax(mr[:, 0], y.mean((1, 2))) < TOL
        assert relmax(mr[:, 1], 1 / torch.sqrt(y.var((1, 2), unbiased=False) + 1e-5)) < TOL
        g = R.gn_grads(y, gamma, beta, ss if use_ss else None, dh)
        assert relmax(g["dy"], yr.grad) < TOL and relmax(g["dgamma"], gr.grad) < TOL and relmax(g["dbeta"], br.grad) < TOL
        assert relmax(g["dbias"], yr.grad.sum((0, 1))) < TOL and relmax(g["dyy"], (yr.grad * y).sum((0, 1))) < TOL
        if use_ss:
            assert relmax(g["dss"], sr.grad) < TOL
        else:
            assert g["dss"] is None


def test_identity_norm_matches_closed_form():
    """Block(norm=False): dy = (1 + scale) * dh * silu'(u) with u = y * (1 + scale) + shift."""
    B, L, C = 2, 19, 16
    y, dh, ss = _d("y", (B, L, C)), _d("dh", (B, L, C)) + 0.3, 0.4 * _d("ss", (B, 2 * C))
    g = R.gn_grads(y, torch.ones(C).double(), torch.zeros(C).double(), ss, dh, identity_norm=True)
    k = 1 + ss[:, None, :C]
    u = y * k + ss[:, None, C:]
    s = torch.sigmoid(u)
    assert relmax(g["dy"], k * dh * s * (1 + u * (1 - s))) < TOL
    assert g["dgamma"] is None and g["dbeta"] is None
    assert relmax(g["dss"][:, C:], (dh * s * (1 + u * (1 - s))).sum(1)) < TOL


def test_layer_norm_vs_functional():
    M, C = 29, 40
    x = _d("x", (M, C), 1.5) - 0.4
    gamma, beta, dy = 1 + 0.3 * _d("g", (C,)), 0.2 * _d("b", (C,)), _d("dy", (M, C)) + 0.2
    xr, gr, br = x.clone().requires_grad_(), gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    want = F.layer_norm(xr, (C,), gr, br, eps=1e-5)
    want.backward(dy)
    out, mr = R.layer_norm(x, gamma, beta)
    assert relmax(out, want) < TOL
    assert relmax(mr[:, 0], x.mean(1)) < TOL and relmax(mr[:, 1], 1 / torch.sqrt(x.var(1, unbiased=False) + 1e-5)) < TOL
    g = R.ln_grads(x, gamma, beta, dy)
    assert relmax(g["dx"], xr.grad) < TOL and relmax(g["dgamma"], gr.grad) < TOL and relmax(g["dbeta"], br.grad) < TOL


def test_block_vs_oracle():
    """oracle.unet_oracle.block = conv3 -> GroupNorm(1, C) -> FiLM -> SiLU on (B, C, N): the reference applied to the oracle's own conv
    output gives the same h, and the same gradients for the norm's parameters, scale / shift, the conv output and the conv bias."""
    B, Cin, C, N = 2, 8, 16, 21
    p = {"b.proj.weight": _d("w", (C, Cin, 3), 0.2), "b.proj.bias": 0.1 * _d("pb", (C,)),
         "b.norm.weight": 1 + 0.3 * _d("g", (C,)), "b.norm.bias": 0.2 * _d("b", (C,))}
    p = {k: v.requires_grad_() for k, v in p.items()}
    x = _d("x", (B, Cin, N))
    scale, shift = (0.4 * _d("sc", (B, C, 1))).requires_grad_(), (0.4 * _d("sh", (B, C, 1))).requires_grad_()
    dh = _d("dh", (B, C, N)) + 0.3
    want = O.block(p, "b", x, (scale, shift), O.Numerics("fp32"))
    want.backward(dh)
    y = F.conv1d(x, p["b.proj.weight"], p["b.proj.bias"], padding=1).detach().transpose(1, 2).contiguous()      # (B, N, C)
    ss = torch.cat([scale.detach()[..., 0], shift.detach()[..., 0]], 1)
    gamma, beta = p["b.norm.weight"].detach(), p["b.norm.bias"].detach()
    h, _ = R.gn_film_silu(y, gamma, beta, ss)
    assert relmax(h.transpose(1, 2), want) < TOL
    g = R.gn_grads(y, gamma, beta, ss, dh.transpose(1, 2).contiguous())
    assert relmax(g["dgamma"], p["b.norm.weight"].grad) < TOL and relmax(g["dbeta"], p["b.norm.bias"].grad) < TOL
    assert relmax(g["dss"][:, :C], scale.grad[..., 0]) < TOL and relmax(g["dss"][:, C:], shift.grad[..., 0]) < TOL
    assert relmax(g["dbias"], p["b.proj.bias"].grad) < TOL


def test_global_context_vs_oracle():
    """oracle.unet_oracle.global_context on (B, C, N): the same pooled vector and gate, and -- through out = h * gate(h) -- the same
    dh, dwk and dbk as full autograd once the gate MLP's cotangent of pooled is handed to the reference as the kernel's caller does."""
    B, C, Ci, N = 2, 16, 8, 23
    p = {"g.to_k.weight": _d("wk", (1, C, 1), 0.5), "g.to_k.bias": _d("bk", (1,), 0.3),
         "g.layers.0.weight": _d("w0", (Ci, C, 1), 0.3), "g.layers.0.bias": 0.1 * _d("b0", (Ci,)),
         "g.layers.2.weight": _d("w2", (C, Ci, 1), 0.3), "g.layers.2.bias": 0.1 * _d("b2", (C,))}
    p = {k: v.requires_grad_() for k, v in p.items()}
    nm = O.Numerics("fp32")
    hc = _d("h", (B, C, N)).requires_grad_()
    dout = _d("dout", (B, C, N)) + 0.2
    gate = O.global_context(p, "g", hc, nm)                                          # (B, C, 1)
    (hc * gate).backward(dout)
    h = hc.detach().transpose(1, 2).contiguous()                                     # (B, N, C)
    wk, bk = p["g.to_k.weight"].detach().reshape(C), p["g.to_k.bias"].detach()
    prob, pooled = R.gca_pool(h, wk, bk)
    assert relmax(prob.sum(1), torch.ones(B).double()) < TOL
    pl = pooled.clone().requires_grad_()
    q = {k: v.detach() for k, v in p.items()}
    g1 = nm.lin(pl, q["g.layers.0.weight"], q["g.layers.0.bias"])
    gate2 = torch.sigmoid(nm.lin(F.silu(g1), q["g.layers.2.weight"], q["g.layers.2.bias"]))
    assert relmax(gate2, gate[..., 0]) < TOL
    do = dout.transpose(1, 2).contiguous()
    gate2.backward((do * h).sum(1))                                                  # d/dgate of dout . (h * gate)
    g = R.gca_grads(do, h, gate2.detach(), pl.grad, wk, bk)
    assert relmax(g["dh"].transpose(1, 2), hc.grad) < TOL
    assert relmax(g["dwk"], p["g.to_k.weight"].grad.reshape(C)) < TOL
    assert abs(g["dbk"].item() - p["g.to_k.bias"].grad.item()) < TOL * g["dlogit"].abs().sum().item()
    assert relmax(R.gate_residual(h, gate2.detach(), do), h * gate2.detach()[:, None] + do) < TOL
