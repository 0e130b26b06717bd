"""The generic path of the stand-alone ``Attend`` module (modules/attention.py): any query count, any key count, mask or none.

The reference's Attend is F.scaled_dot_product_attention on bf16 copies (attention.py:61-101): q (B, H, Nq, D), k / v (B, 1|H, Nk, D), an
optional additive mask broadcastable to (B, H, Nq, Nk).  attend.py keeps the unmasked Nk == Nq call (the tuned kernels at head dim 64); a
call with a mask -- masked self-attention included -- or with another key count comes here and runs osuf_xattn_fwd / osuf_xattn_bwd: the
generic kernels of csrc/attn_generic.hpp, one K/V head per launch, every head dim; q, k, v may be column views of one row image.
  * check_shapes: what Attend.forward validates before anything is launched (pure, callable on CPU tensors).
  * xattn_fwd / xattn_bwd: the allocating wrappers, one C-ABI launch (plus osuf_attn_delta in the backward) each.
  * CrossAttendFn / cross_attend: Attend's contract -- bf16-cast inputs, output in v.dtype, gradients in each input's dtype, a k / v with
    one head gets its gradient summed over the query heads (by the dK/dV kernel itself), a floating-point mask that requires grad gets the
    dense bias gradient summed to its own shape.  Under no_grad the bare launches keep nothing.
Rows whose every key is masked with -inf are NaN in the forward (as in SDPA) and therefore in the backward.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import ops


def check_shapes(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, attn_mask: Optional[torch.Tensor] = None) -> Tuple[int, int, int, int, int, int]:
    """-> (B, H, Nq, Nk, D, G); ValueError for what SDPA would refuse (or silently broadcast where the kernels cannot)."""
    if q.dim() != 4 or k.dim() != 4 or v.dim() != 4:
        raise ValueError(f"q, k and v must be (B, heads, N, D) tensors (got {q.dim()}, {k.dim()} and {v.dim()} dimensions)")
    B, H, Nq, D = q.shape
    G, Nk = k.shape[1], k.shape[2]
    if k.shape[0] != B or v.shape[0] != B or k.shape[3] != D or v.shape[3] != D:
        raise ValueError(f"k / v must share q's batch size {B} and head dim {D} (got k {tuple(k.shape)}, v {tuple(v.shape)})")
    if v.shape[2] != Nk:
        raise ValueError(f"k and v must have the same length (got {Nk} keys and {v.shape[2]} values)")
    if G not in (1, H) or v.shape[1] != G:
        raise ValueError(f"k / v must carry 1 or {H} heads (got {G} / {v.shape[1]})")
    if Nk == 0:
        raise ValueError("k / v are empty: attention needs at least one key")
    if attn_mask is not None:
        ms = tuple(attn_mask.shape)
        want = (B, H, Nq, Nk)
        if len(ms) > 4 or any(m not in (1, w) for m, w in zip(reversed(ms), reversed(want))):
            raise ValueError(f"attn_mask of shape {ms} does not broadcast to (B, H, Nq, Nk) = {want}")
    return B, H, Nq, Nk, D, G


# ---------------------------------------------------------------------------------------------------------
# allocating wrappers (one C-ABI launch each)
# ---------------------------------------------------------------------------------------------------------
def _mask_args(mask4: Optional[torch.Tensor], B: int, H: int, Nq: int, Nk: int):
    if mask4 is None:
        return None, 0, 0, 0, 0
    assert mask4.dtype == torch.bfloat16 and tuple(mask4.shape) == (B, H, Nq, Nk)
    return (mask4.data_ptr(), *mask4.stride())


def xattn_fwd(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, mask4: Optional[torch.Tensor], B: int, Nq: int, Nk: int, H: int, D: int,
              out_dtype: torch.dtype, scale: float):
    """q: bf16 rows [B][Nq][H*D]; k, v: bf16 rows [B][Nk][D] (one K/V head); mask4: None or the bf16 mask expanded (as a view) to
    (B, H, Nq, Nk).  -> (o rows [B][Nq][H*D] in out_dtype, lse2 [B][H][Nq])."""
    (Mq, Wq, ldq), (Mk, Wk, ldk), (Mv, Wv, ldv) = ops._rows(q), ops._rows(k), ops._rows(v)
    assert q.dtype == k.dtype == v.dtype == torch.bfloat16 and (Mq, Wq) == (B * Nq, H * D) and (Mk, Wk) == (Mv, Wv) == (B * Nk, D)
    o = torch.empty((B, Nq, H * D), dtype=out_dtype, device=q.device)
    lse = torch.empty((B, H, Nq), dtype=torch.float32, device=q.device)
    ops.call("osuf_xattn_fwd", q.data_ptr(), ldq, k.data_ptr(), ldk, v.data_ptr(), ldv, o.data_ptr(), H * D, ops._DT[out_dtype], lse.data_ptr(),
             *_mask_args(mask4, B, H, Nq, Nk), B, H, Nq, Nk, D, scale, ops._stream())
    return o, lse


def xattn_bwd(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, mask4: Optional[torch.Tensor], o: torch.Tensor, do: torch.Tensor,
              lse: torch.Tensor, B: int, Nq: int, Nk: int, H: int, D: int, scale: float, want_dbias: bool = False):
    """Backward of xattn_fwd -> (dq rows [B][Nq][H*D], dk rows [B][Nk][D], dv rows [B][Nk][D], all fp32; dbias fp32 [B][H][Nq][Nk] when
    want_dbias (needs a mask), else None).  do: bf16 rows [B][Nq][H*D]; o, lse: the forward's."""
    (Mq, Wq, ldq), (Mk, Wk, ldk), (Mv, Wv, ldv) = ops._rows(q), ops._rows(k), ops._rows(v)
    _, Wd, lddo = ops._rows(do)
    _, Wo, ldo = ops._rows(o)
    assert q.dtype == k.dtype == v.dtype == do.dtype == torch.bfloat16 and (Mq, Wq) == (B * Nq, H * D) and (Mk, Wk) == (Mv, Wv) == (B * Nk, D)
    assert Wd == Wo == H * D and lse.dtype == torch.float32 and lse.is_contiguous() and lse.numel() == B * H * Nq
    assert not want_dbias or mask4 is not None
    dev = q.device
    delta = torch.empty((B, H, Nq), dtype=torch.float32, device=dev)
    ops.call("osuf_attn_delta", do.data_ptr(), lddo, o.data_ptr(), ldo, ops._DT[o.dtype], delta.data_ptr(), B, H, Nq, D, ops._stream())
    dq = torch.empty((B, Nq, H * D), dtype=torch.float32, device=dev)
    dk = torch.empty((B, Nk, D), dtype=torch.float32, device=dev)
    dv = torch.empty((B, Nk, D), dtype=torch.float32, device=dev)
    dbias = torch.empty((B, H, Nq, Nk), dtype=torch.float32, device=dev) if want_dbias else None
    ops.call("osuf_xattn_bwd", q.data_ptr(), ldq, k.data_ptr(), ldk, v.data_ptr(), ldv, do.data_ptr(), lddo, lse.data_ptr(), delta.data_ptr(),
             *_mask_args(mask4, B, H, Nq, Nk), dq.data_ptr(), H * D, dk.data_ptr(), dv.data_ptr(), D, B, H, Nq, Nk, D, scale, ops.F32,
             ops._p(dbias), ops._stream())
    return dq, dk, dv, dbias


# ---------------------------------------------------------------------------------------------------------
# Attend with a mask or with Nk != Nq
# ---------------------------------------------------------------------------------------------------------
def _rows(t: torch.Tensor, dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """(B, h, N, D) -> rows (B, N, h * D): as they come (a copy unless h == 1) or, with a dtype, cast to it and contiguous"""
    rows = t.permute(0, 2, 1, 3).reshape(t.shape[0], t.shape[2], -1)
    return rows if dtype is None else rows.to(dtype).contiguous()


def _heads(rows: torch.Tensor, B: int, N: int, D: int) -> torch.Tensor:
    """(B, N, h * D) -> (B, h, N, D)"""
    return rows.reshape(B, N, -1, D).permute(0, 2, 1, 3)


def _mask4(attn_mask: torch.Tensor, B: int, H: int, Nq: int, Nk: int) -> torch.Tensor:
    # attention.py:90-98: the mask is cast to bf16 and goes to SDPA as an ADDITIVE bias, whatever its dtype was
    m4 = attn_mask.to(torch.bfloat16)
    while m4.dim() < 4:
        m4 = m4.unsqueeze(0)
    return m4.expand(B, H, Nq, Nk)                       # a view: broadcast dimensions keep stride 0


def cross_attend_forward(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, attn_mask: Optional[torch.Tensor]):
    """The launches -> (output (B, H, Nq, D) in v.dtype, state).  state = (m4, parts), parts = (q rows, k rows, v rows, o rows, lse2) per
    launch: one launch over all query heads when k / v carry one head, else one per head with a single query head."""
    B, H, Nq, Nk, D, G = check_shapes(q, k, v, attn_mask)
    m4 = None if attn_mask is None else _mask4(attn_mask, B, H, Nq, Nk)
    outs, parts = [], []
    for g in range(G):
        qs = q if G == 1 else q[:, g:g + 1]
        ms = m4 if (G == 1 or m4 is None) else m4[:, g:g + 1]
        Hq = qs.shape[1]
        qr, kr, vr = (_rows(t, torch.bfloat16) for t in (qs, k[:, g:g + 1], v[:, g:g + 1]))
        o, lse = xattn_fwd(qr, kr, vr, ms, B, Nq, Nk, Hq, D, torch.bfloat16, D ** -0.5)
        outs.append(o.view(B, Nq, Hq, D))
        parts.append((qr, kr, vr, o, lse))
    out = outs[0] if G == 1 else torch.cat(outs, dim=2)
    return out.permute(0, 2, 1, 3).to(v.dtype), (m4, parts)


class CrossAttendFn(torch.autograd.Function):
    """softmax(q k^T / sqrt(D) + mask.to(bf16)) v on bf16 copies of q (Nq rows) and k, v (Nk rows), differentiable in q, k, v and a
    floating-point mask."""

    @staticmethod
    def forward(ctx, q, k, v, attn_mask):
        out, (m4, parts) = cross_attend_forward(q, k, v, attn_mask)
        ctx.geom = (tuple(q.shape), k.shape[1], k.shape[2], q.dtype, k.dtype, v.dtype)
        ctx.mask_meta = None if attn_mask is None else (tuple(attn_mask.shape), attn_mask.dtype, attn_mask.is_floating_point())
        ctx.n_parts = len(parts)
        ctx.save_for_backward(*[t for p in parts for t in p], *([] if m4 is None else [m4]))
        return out

    @staticmethod
    def backward(ctx, go):
        (B, H, Nq, D), G, Nk, qdt, kdt, vdt = ctx.geom
        saved = ctx.saved_tensors
        parts = [saved[5 * i:5 * i + 5] for i in range(ctx.n_parts)]
        m4 = saved[-1] if ctx.mask_meta is not None else None
        do = _rows(go, torch.bfloat16)                       # the reference's out.to(dtype) hands SDPA a bf16 gradient
        want_dbias = ctx.mask_meta is not None and ctx.mask_meta[2] and ctx.needs_input_grad[3]
        Hq = H if G == 1 else 1
        dq, dk, dv, db = [], [], [], []
        for g, (qr, kr, vr, o, lse) in enumerate(parts):
            do_g = do if G == 1 else do[..., g * D:(g + 1) * D]
            ms = m4 if (G == 1 or m4 is None) else m4[:, g:g + 1]
            r = xattn_bwd(qr, kr, vr, ms, o, do_g, lse, B, Nq, Nk, Hq, D, D ** -0.5, want_dbias)
            for acc, t in zip((dq, dk, dv, db), r):
                acc.append(t)
        dq, dk, dv = (torch.cat(t, dim=-1) if len(t) > 1 else t[0] for t in (dq, dk, dv))
        dmask = None
        if want_dbias:
            shape, dtype, _ = ctx.mask_meta
            full = torch.cat(db, dim=1) if len(db) > 1 else db[0]
            shape4 = (1,) * (4 - len(shape)) + shape
            dmask = full.sum_to_size(shape4).reshape(shape).to(dtype)     # broadcast dims of the mask sum their gradients
        need = ctx.needs_input_grad
        return (_heads(dq, B, Nq, D).to(qdt) if need[0] else None, _heads(dk, B, Nk, D).to(kdt) if need[1] else None,
                _heads(dv, B, Nk, D).to(vdt) if need[2] else None, dmask)


def cross_attend(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, attn_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """CrossAttendFn when autograd has something to differentiate, else the bare launches (nothing kept)."""
    if torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad or (attn_mask is not None and attn_mask.requires_grad)):
        return CrossAttendFn.apply(q, k, v, attn_mask)
    return cross_attend_forward(q, k, v, attn_mask)[0]
