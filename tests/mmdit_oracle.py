"""A plain-torch restatement of the MMDiT (osu_fusion/modules/mmdit.py), written from its equations, over a flat state dict; it runs in
the dtype of the parameters it is given (fp32 or fp64).  The GPU tests compare the HIP modules' outputs and gradients against it;
tests/test_mmdit_cpu.py pins it to the reference's recorded fixtures.

    stats = [mean_l a | std_l a] (unbiased) of the audio BEFORE it is padded
    x, a right-padded to a multiple of the patch size p with -1 / -23, then per stream s: s0 = Conv1d(kernel = stride = p)(s)  (B, L / p, dim_h)
    c = where(keep, ff_cond(lin_cond(c)), null_cond) + ff_time(sinusoid(t)) + ff_a(fe(stats)),   ff(u) = W2 silu(W1 u + b1) + b2
    per block and stream s in (x, a), (s1, g1, a1, s2, g2, a2) = Linear_s(silu(c)) split in six:
        u_s = LN(s) (1 + g1) + s1;   (o_x, o_a) = joint(u_x, u_a);   s = s + a1 * Wout_s o_s;   s = s + a2 * ff_s(LN(s) (1 + g2) + s2)
    joint(u_x, u_a): q_s (H heads), k_s, v_s (G heads) = u_s Wq_s^T, ..; q, k QK-normed per stream; over the sequence [audio; map] query
        head j attends with K/V head j mod G:  softmax(q_j k_{j mod G}^T / sqrt(D)) v_{j mod G}
    final: Linear(LN(x) (1 + g) + s) -> (B, N, p dim_h) -> rows (B, N p, dim_h) -> 1x1 conv with bias -> cropped to L
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict

import torch
import torch.nn.functional as F  # noqa: N812

from tests.dit_oracle import _sinusoid, attend_exact, attend_sdpa_bf16  # noqa: F401

# Attend rounds q, k, v to bf16, so the network is not continuous in its fp32 arithmetic: a last-bit difference ahead of the attention
# flips a rounding and shows as ~1e-5 of the output (the reference run in fp64 is 1.6e-5 .. 3.0e-5 away from itself in fp32 on the
# fixtures' cases).  The pieces below therefore go through the same torch primitives as the reference's layers (F.linear, F.layer_norm,
# F.silu, F.normalize), which keeps the fp32 restatement within 1e-5 of the recorded fixtures.


def _ln(x: torch.Tensor) -> torch.Tensor:
    return F.layer_norm(x, x.shape[-1:], eps=1e-6)


def _silu(x: torch.Tensor) -> torch.Tensor:
    return F.silu(x)


def _lin(x, p, name, bias=True):
    return F.linear(x, p[name + ".weight"], p[name + ".bias"] if bias else None)


def _qk_normed(q: torch.Tensor, gamma: torch.Tensor, D: int) -> torch.Tensor:
    return F.normalize(q, dim=-1) * gamma * D ** 0.5                                    # x / max(|x|, 1e-12) * gamma * sqrt(D)


def _mod(x, shift, scale):
    return x * (1 + scale[:, None]) + shift[:, None]


@dataclass
class MMDiTConfig:
    dim_in_x: int = 6
    dim_in_a: int = 96
    dim_in_c: int = 5
    dim_h: int = 512
    depth: int = 12
    patch_size: int = 4
    heads: int = 8
    kv_heads: int = 2
    dim_head: int = 64
    qk_norm: bool = True


def _ff(u, p, name):
    return _lin(_silu(_lin(u, p, name + ".0")), p, name + ".2")


def joint_attention(p: Dict[str, torch.Tensor], pre: str, x, a, H: int, G: int, D: int, qk_norm: bool, attend=attend_exact):
    """x (B, Nx, dim), a (B, Na, dim) -> (out_x (B, Nx, H D), out_a (B, Na, H D)); p[pre + "to_q_x.weight"] etc."""
    B, Nx, Na = x.shape[0], x.shape[1], a.shape[1]
    qkv = {}
    for s, u in (("a", a), ("x", x)):
        q = _lin(u, p, f"{pre}to_q_{s}", False).reshape(B, -1, H, D).transpose(1, 2)
        k = _lin(u, p, f"{pre}to_k_{s}", False).reshape(B, -1, G, D).transpose(1, 2)
        v = _lin(u, p, f"{pre}to_v_{s}", False).reshape(B, -1, G, D).transpose(1, 2)
        if qk_norm:
            q = _qk_normed(q, p[f"{pre}q_{s}_norm.gamma"], D)
            k = _qk_normed(k, p[f"{pre}k_{s}_norm.gamma"], D)
        qkv[s] = (q, k, v)
    q, k, v = (torch.cat([qkv["a"][i], qkv["x"][i]], dim=2) for i in range(3))     # audio rows first
    kv_of = torch.arange(H) % G                                                    # query head j reads K/V head j mod G
    o = attend(q, k[:, kv_of], v[:, kv_of]).transpose(1, 2).reshape(B, Na + Nx, H * D)
    return o[:, Na:], o[:, :Na]


def mmdit_forward(p: Dict[str, torch.Tensor], cfg: MMDiTConfig, x, a, t, c, keep=None, attend=attend_exact) -> torch.Tensor:
    """x (B, dim_in_x, L), a (B, dim_in_a, L), t (B,), c (B, dim_in_c) -> (B, dim_in_x, L) in p's dtype.  keep: bool (B,) of the kept
    conditions (None = all)."""
    dt = next(iter(p.values())).dtype
    x, a, c = x.to(dt), a.to(dt), c.to(dt)
    B, _, L = x.shape
    ps, C = cfg.patch_size, cfg.dim_h
    stats = torch.cat([a.mean(-1), a.std(-1)], 1)
    pad = (ps - L % ps) % ps
    x, a = F.pad(x, (0, pad), value=-1.0), F.pad(a, (0, pad), value=-23.0)
    hx = F.conv1d(x, p["emb_x.proj.weight"], p["emb_x.proj.bias"], stride=ps).transpose(1, 2)
    ha = F.conv1d(a, p["emb_a.proj.weight"], p["emb_a.proj.bias"], stride=ps).transpose(1, 2)
    e = _ff(_lin(c, p, "mlp_cond.0"), p, "mlp_cond.1")
    keep = torch.ones(B, dtype=torch.bool) if keep is None else keep
    e = torch.where(keep.to(e.device)[:, None], e, p["null_cond"][None, :].expand(B, -1))
    cv = e + _ff(_sinusoid(t, C, dt), p, "mlp_time.1") + _ff(_lin(stats, p, "feature_extractor_a"), p, "mlp_a")
    H, G, D = cfg.heads, cfg.kv_heads, cfg.dim_head
    for i in range(cfg.depth):
        pre = f"blocks.{i}."
        mx = _lin(_silu(cv), p, pre + "modulation_x.1").chunk(6, 1)
        ma = _lin(_silu(cv), p, pre + "modulation_a.1").chunk(6, 1)
        ux, ua = _mod(_ln(hx), mx[0], mx[1]), _mod(_ln(ha), ma[0], ma[1])
        ox, oa = joint_attention(p, pre + "attn.", ux, ua, H, G, D, cfg.qk_norm, attend)
        streams = []
        for s, h, o, m in (("x", hx, ox, mx), ("a", ha, oa, ma)):
            h = h + m[2][:, None] * _lin(o, p, f"{pre}attn_out_{s}", False)
            streams.append(h + m[5][:, None] * _ff(_mod(_ln(h), m[3], m[4]), p, f"{pre}mlp_{s}"))
        hx, ha = streams
    sf, gf = _lin(_silu(cv), p, "final_layer.modulation.1").chunk(2, 1)
    h = _lin(_mod(_ln(hx), sf, gf), p, "final_layer.linear")                            # (B, N, p dim_h)
    h = h.reshape(B, -1, C)                                                             # (B, N p, dim_h)
    return F.conv1d(h.transpose(1, 2), p["out.weight"], p["out.bias"])[:, :, :L]
