"""Autograd for the stand-alone ``Attend`` and ``RotaryPositionEmbedding`` modules (modules/attention.py).

In the reference both are differentiable (SDPA and torch arithmetic, attention.py:15-101), and its DiT / MMDiT blocks train through them.
Here the forward runs the same HIP kernels with or without autograd; under grad mode the functions below keep what the backward needs:
  * attend: the dispatch.  A call with a mask, or with k / v of another length than q, is cross_attend.py's (the generic kernels: any
    query count, any key count, mask or none, the bias gradient of a floating-point mask).  What stays here is the unmasked same-length
    call on the tuned kernels.
  * AttendFn: that path's autograd.  It keeps the bf16 q|k|v rows, the output rows and the log-sum-exp of its one launch; the backward is
    ops.mqa_bwd (the tuned fused sweep at head dim 64).
  * RopeFn: the forward's bf16 rounding is kept (the next op casts to bf16 anyway); the backward is the transposed rotation
    (osuf_rope_bwd) in fp32, the rounding taken as identity.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import cross_attend as Xa
from . import ops
from .cross_attend import _heads, _rows


def attend_forward(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor):
    """The unmasked same-length launch -> (output (B, H, N, D) in v.dtype, state).  state = (G, collapsed, qkv rows, o rows, lse2): G = the
    K/V heads the kernel ran with, collapsed = k / v came with H identical heads and ran as one."""
    B, H, N, D = q.shape
    G = k.shape[1]
    collapsed = False
    if G != 1 and torch.equal(k[:, :1].expand_as(k), k) and torch.equal(v[:, :1].expand_as(v), v):
        G, k, v, collapsed = 1, k[:, :1], v[:, :1], True    # one K/V head repeated (what the UNet's Attention hands over): one launch
    qkv = torch.cat([_rows(q), _rows(k), _rows(v)], dim=-1).to(torch.bfloat16).contiguous()
    o, lse = ops.mqa_fwd(qkv, B, N, H, D, torch.bfloat16, D ** -0.5, kv_heads=G)   # G = H: every query head has its own K/V head
    return o.view(B, N, H, D).permute(0, 2, 1, 3).to(v.dtype), (G, collapsed, qkv, o, lse)


class AttendFn(torch.autograd.Function):
    """softmax(q k^T / sqrt(D)) v on bf16 copies of q, k, v of one length (attention.py:84-101), differentiable in q, k, v."""

    @staticmethod
    def forward(ctx, q, k, v):
        out, (G, collapsed, qkv, o, lse) = attend_forward(q, k, v)
        ctx.geom = (tuple(q.shape), G, collapsed, q.dtype, k.dtype, v.dtype)
        ctx.save_for_backward(qkv, o, lse)
        return out

    @staticmethod
    def backward(ctx, go):
        (B, H, N, D), G, collapsed, qdt, kdt, vdt = ctx.geom
        qkv, o, lse = ctx.saved_tensors
        do = _rows(go, torch.bfloat16)                       # the reference's out.to(dtype) hands SDPA a bf16 gradient
        if collapsed:
            # k / v came with H identical heads: one dK / dV per head is still owed, so the backward runs with G = H on the single
            # head repeated, with the saved output and lse2 (laid out [G][B][H/G][N] for grouped launches)
            G = H
            kc, vc = qkv[..., H * D:(H + 1) * D], qkv[..., (H + 1) * D:]
            qkv = torch.cat([qkv[..., :H * D], kc.repeat(1, 1, H), vc.repeat(1, 1, H)], dim=-1)
            lse = lse.transpose(0, 1).unsqueeze(2).contiguous()
        dqkv = ops.mqa_bwd(qkv, o, do, lse, B, N, H, D, D ** -0.5, torch.float32, variant=ops.ATTN_BWD_DEFAULT, kv_heads=G)
        dq, dk, dv = dqkv[..., :H * D], dqkv[..., H * D:(H + G) * D], dqkv[..., (H + G) * D:]
        need = ctx.needs_input_grad
        return (_heads(dq, B, N, D).to(qdt) if need[0] else None, _heads(dk, B, N, D).to(kdt) if need[1] else None,
                _heads(dv, B, N, D).to(vdt) if need[2] else None)


def attend(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, attn_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """With a mask, or k / v of another length than q: cross_attend.py.  Else AttendFn when autograd has something to differentiate, or
    the bare launch (nothing kept)."""
    if attn_mask is not None or k.shape[2] != q.shape[2]:
        return Xa.cross_attend(q, k, v, attn_mask)
    if torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad):
        return AttendFn.apply(q, k, v)
    return attend_forward(q, k, v)[0]


# ---------------------------------------------------------------------------------------------------------
# RoPE
# ---------------------------------------------------------------------------------------------------------
def rope_bhnd(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    """attention.py:52-58 on (B, H, N, D): rotated, rounded to bf16 (as Attend would cast it next), returned in x.dtype."""
    B, H, N, D = x.shape
    rows = x.permute(0, 2, 1, 3).reshape(B, N, H * D).contiguous()
    if rows.dtype not in (torch.float32, torch.bfloat16):
        rows = rows.float()
    out = ops.rope_cast(rows, cos, sin, N, H, H, D)
    return out.view(B, N, H, D).permute(0, 2, 1, 3).to(x.dtype)


class RopeFn(torch.autograd.Function):
    """rope_bhnd with its transpose as the backward (fp32; the bf16 rounding of the forward passes the gradient unchanged)."""

    @staticmethod
    def forward(ctx, x, cos, sin):
        ctx.save_for_backward(cos, sin)
        ctx.dtype = x.dtype
        return rope_bhnd(x, cos, sin)

    @staticmethod
    def backward(ctx, g):
        cos, sin = ctx.saved_tensors
        B, H, N, D = g.shape
        rows = _rows(g, torch.float32)
        dx = ops.rope_bwd(rows, torch.float32, cos, sin, N, H, H, D)
        return _heads(dx, B, N, D).to(ctx.dtype), None, None


def rope(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    if torch.is_grad_enabled() and x.requires_grad:
        return RopeFn.apply(x, cos, sin)
    return rope_bhnd(x, cos, sin)
