"""Autograd for the stand-alone ``Attend`` and ``RotaryPositionEmbedding`` modules (modules/attention.py).

In the reference both are differentiable (SDPA and torch arithmetic, attention.py:15-101), and its DiT / MMDiT blocks train through them.
Here the forward runs the same HIP kernels with or without autograd; under grad mode the functions below keep what the backward needs:
  * AttendFn: the bf16 q|k|v rows, the output rows and the log-sum-exp of every launch.  Without a mask the backward is ops.mqa_bwd
    (the tuned fused sweep at head dim 64); with one it is osuf_mqa_bwd_masked, which restarts the scores from the bf16 bias exactly as
    the forward did and, when a floating-point mask requires grad, also stores dL/d(bias).
  * RopeFn: the forward's bf16 rounding is kept (the next op casts to bf16 anyway); the backward is the transposed rotation
    (osuf_rope_bwd) in fp32, the rounding taken as identity.
Rows whose every key is masked with -inf are NaN in the forward (as in SDPA) and therefore in the backward.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import cross_attend as Xa
from . import ops

# ---------------------------------------------------------------------------------------------------------
# allocating wrappers (one C-ABI launch each)
# ---------------------------------------------------------------------------------------------------------


def mqa_fwd_masked(qkv: torch.Tensor, mask4: torch.Tensor, B: int, N: int, H: int, D: int, out_dtype: torch.dtype, scale: float):
    """ops.mqa_fwd_masked that also returns the log-sum-exp: (o rows [B][N][H*D], lse2 [B][H][N]).  One K/V head."""
    M, W, ld = ops._rows(qkv)
    assert qkv.dtype == torch.bfloat16 and W == (H + 2) * D and mask4.dtype == torch.bfloat16 and tuple(mask4.shape) == (B, H, N, N)
    o = torch.empty((B, N, H * D), dtype=out_dtype, device=qkv.device)
    lse = torch.empty((B, H, N), dtype=torch.float32, device=qkv.device)
    base = qkv.data_ptr()
    sb, sh, sq, sk = mask4.stride()
    ops.call("osuf_mqa_fwd_masked", base, ld, base + 2 * H * D, ld, base + 2 * (H + 1) * D, ld, o.data_ptr(), H * D, ops._DT[out_dtype],
             lse.data_ptr(), mask4.data_ptr(), sb, sh, sq, sk, B, H, N, D, scale, ops._stream())
    return o, lse


def mqa_bwd_masked(qkv: torch.Tensor, mask4: torch.Tensor, o: torch.Tensor, do: torch.Tensor, lse: torch.Tensor, B: int, N: int, H: int, D: int,
                   scale: float, want_dbias: bool = False):
    """Backward of mqa_fwd_masked: fp32 gradients laid out like qkv, [B][N][(H+2)*D] (of the rotated q / k as they entered), and, when
    want_dbias, the dense fp32 gradient of the bias [B][H][N][N] (else None).  do: bf16 rows [B][N][H*D]; lse: the forward's lse2."""
    M, W, ld = ops._rows(qkv)
    _, _, ldo_ = ops._rows(do)
    _, _, ldo2 = ops._rows(o)
    assert qkv.dtype == torch.bfloat16 and W == (H + 2) * D and do.dtype == torch.bfloat16 and tuple(mask4.shape) == (B, H, N, N)
    assert mask4.dtype == torch.bfloat16 and lse.dtype == torch.float32 and lse.is_contiguous() and lse.numel() == B * H * N
    dev = qkv.device
    delta = torch.empty((B, H, N), dtype=torch.float32, device=dev)
    ops.call("osuf_attn_delta", do.data_ptr(), ldo_, o.data_ptr(), ldo2, ops._DT[o.dtype], delta.data_ptr(), B, H, N, D, ops._stream())
    dqkv = torch.empty((B, N, W), dtype=torch.float32, device=dev)
    dbias = torch.empty((B, H, N, N), dtype=torch.float32, device=dev) if want_dbias else None
    base, gb = qkv.data_ptr(), dqkv.data_ptr()
    sb, sh, sq, sk = mask4.stride()
    ops.call("osuf_mqa_bwd_masked", base, ld, base + 2 * H * D, ld, base + 2 * (H + 1) * D, ld, do.data_ptr(), ldo_, lse.data_ptr(), delta.data_ptr(),
             mask4.data_ptr(), sb, sh, sq, sk, gb, W, gb + 4 * H * D, gb + 4 * (H + 1) * D, W, B, H, N, D, scale, ops.F32, ops._p(dbias), ops._stream())
    return dqkv, dbias


# ---------------------------------------------------------------------------------------------------------
# Attend
# ---------------------------------------------------------------------------------------------------------
def _rows(t: torch.Tensor) -> torch.Tensor:
    """(B, h, N, D) -> (B, N, h * D) (a copy unless h == 1)."""
    B, h, N, D = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, N, h * D)


def _mask4(attn_mask: torch.Tensor, B: int, H: int, N: int) -> torch.Tensor:
    # attention.py:90-98: the mask is cast to the q/k/v dtype (bf16) and goes to SDPA as an ADDITIVE bias, whatever its dtype was
    m4 = attn_mask.to(torch.bfloat16)
    while m4.dim() < 4:
        m4 = m4.unsqueeze(0)
    return m4.expand(B, H, N, N)                         # a view: broadcast dimensions keep stride 0


def attend_forward(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, attn_mask: Optional[torch.Tensor]):
    """Attend's kernel launches -> (output (B, H, N, D) in v.dtype, state).  state = (G, collapsed, m4, parts): G = the K/V heads the
    kernels ran with, collapsed = k / v came with H identical heads and ran as one, parts = (qkv rows, o rows, lse2) per launch."""
    B, H, N, D = q.shape
    G = k.shape[1]
    if attn_mask is not None:
        m4 = _mask4(attn_mask, B, H, N)
        outs, parts = [], []
        for g in range(G):                               # per K/V head: its query heads are g, g + G, ... only when G == H or 1 here
            qs = q if G == 1 else q[:, g:g + 1]
            ms = m4 if G == 1 else m4[:, g:g + 1]
            Hq = qs.shape[1]
            qkv = torch.cat([_rows(qs), _rows(k[:, g:g + 1]), _rows(v[:, g:g + 1])], dim=-1).to(torch.bfloat16).contiguous()
            o, lse = mqa_fwd_masked(qkv, ms, B, N, Hq, D, torch.bfloat16, D ** -0.5)
            outs.append(o.view(B, N, Hq, D))
            parts.append((qkv, o, lse))
        return torch.cat(outs, dim=2).permute(0, 2, 1, 3).to(v.dtype), (G, False, m4, parts)
    collapsed = False
    if G != 1 and torch.equal(k[:, :1].expand_as(k), k) and torch.equal(v[:, :1].expand_as(v), v):
        G, k, v, collapsed = 1, k[:, :1], v[:, :1], True    # one K/V head repeated (what the UNet's Attention hands over): one launch
    qkv = torch.cat([_rows(q), _rows(k), _rows(v)], dim=-1).to(torch.bfloat16).contiguous()
    o, lse = ops.mqa_fwd(qkv, B, N, H, D, torch.bfloat16, D ** -0.5, kv_heads=G)   # G = H: every query head has its own K/V head
    return o.view(B, N, H, D).permute(0, 2, 1, 3).to(v.dtype), (G, collapsed, None, [(qkv, o, lse)])


def _heads(rows: torch.Tensor, B: int, N: int, D: int) -> torch.Tensor:
    """(B, N, h * D) -> (B, h, N, D)"""
    return rows.reshape(B, N, -1, D).permute(0, 2, 1, 3)


class AttendFn(torch.autograd.Function):
    """softmax(q k^T / sqrt(D) + mask.to(bf16)) v on bf16 copies of q, k, v (attention.py:84-101), differentiable in q, k, v and a
    floating-point mask."""

    @staticmethod
    def forward(ctx, q, k, v, attn_mask):
        out, (G, collapsed, m4, parts) = attend_forward(q, k, v, attn_mask)
        ctx.geom = (tuple(q.shape), G, collapsed, k.shape[1], q.dtype, k.dtype, v.dtype)
        ctx.mask_meta = None if attn_mask is None else (tuple(attn_mask.shape), attn_mask.dtype, attn_mask.is_floating_point())
        ctx.n_parts = len(parts)
        ctx.save_for_backward(*[t for p in parts for t in p], *([] if m4 is None else [m4]))
        return out

    @staticmethod
    def backward(ctx, go):
        (B, H, N, D), G, collapsed, Gin, qdt, kdt, vdt = ctx.geom
        saved = ctx.saved_tensors
        parts = [saved[3 * i:3 * i + 3] for i in range(ctx.n_parts)]
        scale = D ** -0.5
        do = _rows(go).to(torch.bfloat16).contiguous()       # the reference's out.to(dtype) hands SDPA a bf16 gradient
        want_dbias = ctx.mask_meta is not None and ctx.mask_meta[2] and ctx.needs_input_grad[3]
        dmask = None
        if ctx.mask_meta is not None:
            m4 = saved[-1]
            dq, dk, dv, db = [], [], [], []
            for g, (qkv, o, lse) in enumerate(parts):
                Hq = H if G == 1 else 1
                do_g = do if G == 1 else do[..., g * D:(g + 1) * D]
                ms = m4 if G == 1 else m4[:, g:g + 1]
                dqkv, dbias = mqa_bwd_masked(qkv, ms, o, do_g, lse, B, N, Hq, D, scale, want_dbias)
                dq.append(dqkv[..., :Hq * D])
                dk.append(dqkv[..., Hq * D:(Hq + 1) * D])
                dv.append(dqkv[..., (Hq + 1) * D:])
                db.append(dbias)
            dq, dk, dv = (torch.cat(t, dim=-1) if len(t) > 1 else t[0] for t in (dq, dk, dv))
            if want_dbias:
                shape, dtype, _ = ctx.mask_meta
                full = torch.cat(db, dim=1) if len(db) > 1 else db[0]
                shape4 = (1,) * (4 - len(shape)) + shape
                dmask = full.sum_to_size(shape4).reshape(shape).to(dtype)     # broadcast dims of the mask sum their gradients
        else:
            qkv, o, lse = parts[0]
            if collapsed:
                # k / v came with H identical heads: one dK / dV per head is still owed, so the backward runs with G = H on the single
                # head repeated, with the saved output and lse2 (laid out [G][B][H/G][N] for grouped launches)
                G = H
                kc, vc = qkv[..., H * D:(H + 1) * D], qkv[..., (H + 1) * D:]
                qkv = torch.cat([qkv[..., :H * D], kc.repeat(1, 1, H), vc.repeat(1, 1, H)], dim=-1)
                lse = lse.transpose(0, 1).unsqueeze(2).contiguous()
            dqkv = ops.mqa_bwd(qkv, o, do, lse, B, N, H, D, scale, torch.float32, variant=ops.ATTN_BWD_DEFAULT, kv_heads=G)
            dq, dk, dv = dqkv[..., :H * D], dqkv[..., H * D:(H + G) * D], dqkv[..., (H + G) * D:]
        need = ctx.needs_input_grad
        return (_heads(dq, B, N, D).to(qdt) if need[0] else None, _heads(dk, B, N, D).to(kdt) if need[1] else None,
                _heads(dv, B, N, D).to(vdt) if need[2] else None, dmask)


def attend(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, attn_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """AttendFn when autograd has something to differentiate, else the bare launches (nothing kept).  k / v of another length than q:
    cross_attend.py (the generic kernels with their own key count)."""
    if k.shape[2] != q.shape[2]:
        return Xa.cross_attend(q, k, v, attn_mask)
    if torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad or (attn_mask is not None and attn_mask.requires_grad)):
        return AttendFn.apply(q, k, v, attn_mask)
    return attend_forward(q, k, v, attn_mask)[0]


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
        rows = _rows(g).float().contiguous()
        dx = ops.rope_bwd(rows, torch.float32, cos, sin, N, H, H, D)
        return _heads(dx, B, N, D).to(ctx.dtype), None, None


def rope(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    if torch.is_grad_enabled() and x.requires_grad:
        return RopeFn.apply(x, cos, sin)
    return rope_bhnd(x, cos, sin)
