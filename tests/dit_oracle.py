"""A plain-torch restatement of the DiT (osu_fusion/modules/dit.py), written from its equations, over a state dict.  The GPU tests
compare the HIP module's output and gradients against it (run in fp64 on the same parameters); tests/test_dit_cpu.py pins it to the
reference's recorded fixtures.

    x0   = stem(cat(x, a))                         sum of Conv1d(102, d_i, k_i, pad k_i // 2), concatenated on channels
    h_a  = [mean_l a | std_l a] (unbiased)         fe(h_a) -> mlp_audio
    c    = where(keep, mlp_cond(c), null_cond) + mlp_time(sinusoid(t)) + mlp_audio(fe(h_a))
    per block, (s1, g1, a1, s2, g2, a2) = Linear(silu(c)) split in six (shift, scale, gate, shift, scale, gate):
        x = x + a1 * attn(LN(x) (1 + g1) + s1),   x = x + a2 * W2 silu(W1 (LN(x) (1 + g2) + s2) + b1) + b2
        attn(h) = per head softmax(qn kn^T / sqrt(D)) v with q | k | v = h Wqkv^T and qn = q / max(|q|, 1e-12) * gamma_q * sqrt(D)
    final: Linear(LN(x) (1 + g) + s); out = postprocess (1x1 conv, no bias)
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, Tuple

import torch
import torch.nn.functional as F  # noqa: N812


@dataclass
class DiTConfig:
    dim_in_x: int = 6
    dim_in_a: int = 96
    dim_in_c: int = 5
    dim_h: int = 512
    dim_h_mult: int = 4
    depth: int = 12
    kernel_sizes: Tuple[int, ...] = (3, 7, 15)
    heads: int = 8
    dim_head: int = 64
    qk_norm: bool = True


def _ln(x: torch.Tensor) -> torch.Tensor:
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + 1e-6)


def _silu(x: torch.Tensor) -> torch.Tensor:
    return x * torch.sigmoid(x)


def _lin(x, p, name, bias=True):
    y = x @ p[name + ".weight"].t()
    return y + p[name + ".bias"] if bias else y


def _sinusoid(t: torch.Tensor, dim: int, dtype) -> torch.Tensor:
    half = dim // 2
    f = torch.exp(torch.arange(half, dtype=dtype, device=t.device) * (-math.log(10000) / (half - 1)))
    ang = t.to(dtype)[:, None] * f[None, :]
    return torch.cat([ang.sin(), ang.cos()], dim=-1)


def _qk_normed(q: torch.Tensor, gamma: torch.Tensor, D: int) -> torch.Tensor:
    n = torch.sqrt((q * q).sum(-1, keepdim=True)).clamp_min(1e-12)
    return q / n * gamma * math.sqrt(D)


class _Bf16Round(torch.autograd.Function):
    """x.to(bfloat16).to(x.dtype) forward and backward: the two casts around Attend's kernel (its output's gradient arrives in bf16)."""

    @staticmethod
    def forward(ctx, x):
        return x.to(torch.bfloat16).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.bfloat16).to(g.dtype)


def attend_exact(q, k, v):
    """softmax(q k^T / sqrt(D)) v in the inputs' dtype, with Attend's bf16 roundings of q, k, v, of the output and of its gradient."""
    q, k, v = (z.to(torch.bfloat16).to(z.dtype) for z in (q, k, v))
    return _Bf16Round.apply(torch.softmax((q @ k.transpose(-1, -2)) / math.sqrt(q.shape[-1]), -1) @ v)


def attend_sdpa_bf16(q, k, v):
    """What the reference's Attend computes on a CPU host with the bf16 configuration: SDPA on bf16 copies, cast back."""
    dt = v.dtype
    q, k, v = (z.to(torch.bfloat16).contiguous() for z in (q, k, v))
    return F.scaled_dot_product_attention(q, k, v).to(dt)


def dit_forward(p: Dict[str, torch.Tensor], cfg: DiTConfig, x, a, t, c, keep=None, attend=attend_exact) -> torch.Tensor:
    """x (B, dim_in_x, L), a (B, dim_in_a, L), t (B,), c (B, dim_in_c) -> (B, dim_in_x, L) in p's dtype.  keep: bool (B,) of the kept
    conditions (None = all)."""
    dt = next(iter(p.values())).dtype
    x, a, c = x.to(dt), a.to(dt), c.to(dt)
    xa = torch.cat([x, a], 1)
    ks = sorted(cfg.kernel_sizes)
    x0 = torch.cat([F.conv1d(xa, p[f"preprocess.convs.{i}.weight"], p[f"preprocess.convs.{i}.bias"], padding=k // 2) for i, k in enumerate(ks)], 1)
    h = x0.transpose(1, 2)                                               # (B, L, C)
    B, L, C = h.shape
    h_a = torch.cat([a.mean(-1), a.std(-1)], 1)
    h_a = _lin(h_a, p, "feature_extractor_a")
    e = _lin(_silu(_lin(c, p, "mlp_cond.0")), p, "mlp_cond.2")
    keep = torch.ones(B, dtype=torch.bool) if keep is None else keep
    e = torch.where(keep.to(e.device)[:, None], e, p["null_cond"][None, :].expand(B, -1))
    te = _lin(_silu(_lin(_sinusoid(t, C, dt), p, "mlp_time.1", False)), p, "mlp_time.3", False)
    ae = _lin(_silu(_lin(h_a, p, "mlp_audio.0")), p, "mlp_audio.2")
    cv = e + te + ae
    H, D = cfg.heads, cfg.dim_head
    for i in range(cfg.depth):
        pre = f"blocks.{i}."
        s1, g1, a1, s2, g2, a2 = _lin(_silu(cv), p, pre + "modulation.1").chunk(6, 1)
        u = _ln(h) * (1 + g1[:, None]) + s1[:, None]
        q, k, v = (z.reshape(B, L, H, D).transpose(1, 2) for z in (u @ p[pre + "attn.to_qkv.weight"].t()).chunk(3, -1))
        if cfg.qk_norm:
            q = _qk_normed(q, p[pre + "attn.q_norm.gamma"], D)
            k = _qk_normed(k, p[pre + "attn.k_norm.gamma"], D)
        o = attend(q, k, v).transpose(1, 2).reshape(B, L, H * D)
        h = h + a1[:, None] * o
        u = _ln(h) * (1 + g2[:, None]) + s2[:, None]
        f = _lin(_silu(_lin(u, p, pre + "ff.0")), p, pre + "ff.2")
        h = h + a2[:, None] * f
    sf, gf = _lin(_silu(cv), p, "final.modulation.1").chunk(2, 1)
    h = _lin(_ln(h) * (1 + gf[:, None]) + sf[:, None], p, "final.linear")
    return F.conv1d(h.transpose(1, 2), p["postprocess.weight"])
