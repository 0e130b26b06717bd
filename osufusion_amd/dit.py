"""Kernels and autograd of the DiT backbone (modules/dit.py, a mirror of osu_fusion/modules/dit.py).

Rows are channels-last (B, L, C) in the compute dtype, as everywhere else in the package.  The pieces of a DiTBlock:
  * AdaLNFn: modulate(LayerNorm(x), shift, scale) (dit.py:14-15,149-152) by osuf_adaln_fwd / osuf_adaln_bwd.  shift / scale are column
    blocks of the fp32 (B, 6C) modulation output, read in place, and their gradients are stored in place into the same blocks of that
    output's gradient; the backward also takes the residual stream's gradient (parked by the
    gated residual through a functional.ResLink) and adds it into dx in the same pass.
  * DiTAttentionFn: to_qkv GEMM -> osuf_joint_qknorm_fwd with one stream and G = H (F.normalize * gamma * sqrt(D) of the q and k heads,
    one bf16 rounding: the rows Attend casts to) -> ops.mqa_fwd with one K/V head per query head (kv_heads = H).  Backward: ops.mqa_bwd,
    osuf_joint_qknorm_bwd, then the dgrad / wgrad GEMMs of to_qkv.
  * DiTFeedForwardFn: W2 silu(W1 x + b1) + b2, SiLU in the first GEMM's epilogue (the residual is gated, so it stays out of the GEMM).
  * the gated residual x + gate[b] * f(x) is functional.GateResFn.
  * stat_pool: cat(a.mean(-1), a.std(-1)) of the audio (dit.py:275-277), forward only.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib
from . import functional as Fn
from . import ops

LN_EPS = 1e-6                                              # nn.LayerNorm(dim_h, elementwise_affine=False, eps=1e-6) (dit.py:76,135,143)


# ---------------------------------------------------------------------------------------------------------
# allocating wrappers (one C-ABI entry point each)
# ---------------------------------------------------------------------------------------------------------
def _cols(t: torch.Tensor):
    """(B, C) fp32 column block of a wider (B, W) tensor -> its row stride (the kernels read it in place)."""
    assert t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1 and t.data_ptr() % 16 == 0 and t.stride(0) % 4 == 0
    return t.stride(0)


def adaln_fwd(x: torch.Tensor, shift: torch.Tensor, scale: torch.Tensor, eps: float = LN_EPS):
    """x rows (B, L, C) -> (LN(x) * (1 + scale[b]) + shift[b] in x.dtype, mr (B*L, 2) fp32 = mean | rstd).  shift / scale: fp32 (B, C),
    possibly column blocks of one wider tensor with the same row stride."""
    M, C, ld = ops._rows(x)
    B, L = x.shape[0], x.shape[1]
    ldm = _cols(shift)
    assert _cols(scale) == ldm and tuple(shift.shape) == tuple(scale.shape) == (B, C)
    out = torch.empty((B, L, C), dtype=x.dtype, device=x.device)
    mr = torch.empty((M, 2), dtype=torch.float32, device=x.device)
    ops.call("osuf_adaln_fwd", ops.dt_of(x), x.data_ptr(), ld, out.data_ptr(), C, mr.data_ptr(), shift.data_ptr(), scale.data_ptr(), ldm,
             M, C, L, float(eps), ops._stream())
    return out, mr


def adaln_bwd(dy: torch.Tensor, x: torch.Tensor, mr: torch.Tensor, scale: torch.Tensor, dres: Optional[torch.Tensor] = None,
              dshift: Optional[torch.Tensor] = None, dscale: Optional[torch.Tensor] = None):
    """-> (dx rows in x.dtype (+ dres), dshift, dscale).  dshift / dscale: fp32 (B, C) outputs, possibly column blocks of one wider tensor
    with the same row stride (the (B, 6C) gradient of the modulation output): the kernel stores into them in place.  Not given: both
    are column blocks of a fresh (B, 2C) tensor."""
    M, C, ld = ops._rows(x)
    B, L = x.shape[0], x.shape[1]
    assert dy.dtype == x.dtype and (dres is None or dres.dtype == x.dtype) and mr.is_contiguous() and mr.numel() == 2 * M
    ldm = _cols(scale)
    dev = x.device
    dx = torch.empty((B, L, C), dtype=x.dtype, device=dev)
    if dshift is None:
        dss = torch.empty((B, 2 * C), dtype=torch.float32, device=dev)
        dshift, dscale = dss[:, :C], dss[:, C:]
    ldd = _cols(dshift)
    off2 = (dscale.data_ptr() - dshift.data_ptr()) // 4
    assert _cols(dscale) == ldd and tuple(dshift.shape) == tuple(dscale.shape) == (B, C) and dscale.data_ptr() - dshift.data_ptr() == 4 * off2
    need = _lib.load().osuf_adaln_bwd_workspace_bytes(M, C, L)
    assert need > 0, "osuf_adaln_bwd: unsupported shape"
    ws = torch.empty(need // 4, dtype=torch.float32, device=dev)
    ops.call("osuf_adaln_bwd", ops.dt_of(x), dy.data_ptr(), ops._rows(dy)[2], x.data_ptr(), ld, ops._p(dres), ops._rows(dres)[2] if dres is not None else 0,
             dx.data_ptr(), C, mr.data_ptr(), scale.data_ptr(), ldm, dshift.data_ptr(), ldd, off2, ws.data_ptr(), need, M, C, L, ops._stream())
    return dx, dshift, dscale


def qknorm_fwd(raw: torch.Tensor, gamma_q: torch.Tensor, gamma_k: torch.Tensor, H: int, D: int):
    """raw q|k|v projection rows (B, L, 3 H D) -> (bf16 rows for the attention kernels, inv norms (B*L, 2H) fp32).  The joint kernel with
    one stream (Ns = Nj = L, off = 0) and G = H: its row and head permutations are then the identity."""
    M, W, ld = ops._rows(raw)
    L = raw.shape[1]
    assert W == 3 * H * D and gamma_q.dtype == gamma_k.dtype == torch.float32 and gamma_q.is_contiguous() and gamma_k.is_contiguous()
    assert gamma_q.numel() == gamma_k.numel() == H * D
    y = torch.empty(raw.shape, dtype=torch.bfloat16, device=raw.device)
    inv = torch.empty((M, 2 * H), dtype=torch.float32, device=raw.device)
    ops.call("osuf_joint_qknorm_fwd", ops.dt_of(raw), raw.data_ptr(), ld, y.data_ptr(), W, inv.data_ptr(), gamma_q.data_ptr(), gamma_k.data_ptr(),
             M, L, L, 0, H, H, D, ops._stream())
    return y, inv


def qknorm_bwd(dqkv: torch.Tensor, raw: torch.Tensor, inv: torch.Tensor, gamma_q: torch.Tensor, gamma_k: torch.Tensor, H: int, D: int):
    """fp32 dq|dk|dv rows (ops.mqa_bwd) -> (gradient of the raw projections in raw.dtype, dgamma (2, H, D) fp32 = q | k)."""
    M, W, ld = ops._rows(raw)
    Mg, Wg, ldg = ops._rows(dqkv)
    L = raw.shape[1]
    assert dqkv.dtype == torch.float32 and Mg == M and Wg == W == 3 * H * D and inv.is_contiguous() and inv.numel() == 2 * H * M
    dev = raw.device
    dx = torch.empty(raw.shape, dtype=raw.dtype, device=dev)
    dgamma = torch.empty((2, H, D), dtype=torch.float32, device=dev)
    need = _lib.load().osuf_joint_qknorm_bwd_workspace_bytes(M, H, H, D)
    ws = torch.empty(max(need // 4, 1), dtype=torch.float32, device=dev)
    ops.call("osuf_joint_qknorm_bwd", ops.dt_of(raw), dqkv.data_ptr(), ldg, raw.data_ptr(), ld, inv.data_ptr(), gamma_q.data_ptr(),
             gamma_k.data_ptr(), dx.data_ptr(), W, dgamma.data_ptr(), ws.data_ptr(), need, M, L, L, 0, H, H, D, ops._stream())
    return dx, dgamma


def stat_pool(a: torch.Tensor) -> torch.Tensor:
    """fp32 (B, C, L) -> (B, 2C) = cat(a.mean(-1), a.std(-1)) (unbiased)."""
    assert a.is_cuda and a.dim() == 3, "stat_pool: (B, C, L) on the GPU"
    a = a.float().contiguous()
    B, C, L = a.shape
    out = torch.empty((B, 2 * C), dtype=torch.float32, device=a.device)
    ops.call("osuf_stat_pool", a.data_ptr(), out.data_ptr(), B, C, L, ops._stream())
    return out


# ---------------------------------------------------------------------------------------------------------
# autograd
# ---------------------------------------------------------------------------------------------------------
class AdaLNFn(torch.autograd.Function):
    """modulate(LayerNorm(x), shift, scale) on rows, shift / scale = column blocks i_shift / i_scale (C wide) of the fp32 modulation
    output `mod`, read in place.  The backward stores dshift / dscale straight into those blocks of mod's gradient (the other blocks
    zero).  link (functional.ResLink, optional): the gated residual that also reads x parks its gradient of x there, and this backward
    adds it into dx (the residual stream's gradient is never summed by a separate pass)."""

    @staticmethod
    def forward(ctx, x, mod, i_shift, i_scale, link=None):
        C = x.shape[-1]
        out, mr = adaln_fwd(x, mod[:, i_shift * C:(i_shift + 1) * C], mod[:, i_scale * C:(i_scale + 1) * C])
        ctx.save_for_backward(x, mr, mod)
        ctx.cols, ctx.link = (i_shift, i_scale), link
        return out

    @staticmethod
    def backward(ctx, dy):
        x, mr, mod = ctx.saved_tensors
        (i_shift, i_scale), link = ctx.cols, ctx.link
        C = x.shape[-1]
        dres = None
        if link is not None and link.dx is not None:
            dres, link.dx = Fn._rc(link.dx), None
        dmod = ops.zeros(mod.shape, torch.float32, mod.device)
        dx, _, _ = adaln_bwd(Fn._rc(dy), x, mr, mod[:, i_scale * C:(i_scale + 1) * C], dres,
                             dmod[:, i_shift * C:(i_shift + 1) * C], dmod[:, i_scale * C:(i_scale + 1) * C])
        return dx, dmod, None, None, None


def adaln(x: torch.Tensor, mod: torch.Tensor, i_shift: int, i_scale: int, link=None) -> torch.Tensor:
    """modulate(LayerNorm(x), shift, scale) with shift / scale the C-wide column blocks i_shift / i_scale of mod (fp32 (B, k C))."""
    if torch.is_grad_enabled() and (x.requires_grad or mod.requires_grad):
        return AdaLNFn.apply(x, mod, i_shift, i_scale, link)
    C = x.shape[-1]
    return adaln_fwd(x, mod[:, i_shift * C:(i_shift + 1) * C], mod[:, i_scale * C:(i_scale + 1) * C])[0]


def _attn_rows(x, w, gq, gk, cache, H: int, D: int, one_launch: bool = False):
    """-> (raw projections, bf16 q|k|v rows, inv norms or None, o (bf16), lse2).  one_launch (inference): all H heads in one osuf_gqa_fwd
    launch instead of one osuf_mqa_fwd launch per head; the same bits."""
    B, L, _ = x.shape
    raw = Fn.conv_forward(x, w, None, cache, "same")
    if gq is not None:
        qkv, inv = qknorm_fwd(raw, gq, gk, H, D)
    else:
        qkv, inv = ops.cast_rows(raw, torch.bfloat16), None
    fwd = ops.gqa_fwd if one_launch else ops.mqa_fwd
    o, lse = fwd(qkv, B, L, H, D, torch.bfloat16, D ** -0.5, kv_heads=H)
    return raw, qkv, inv, o, lse


class DiTAttentionFn(torch.autograd.Function):
    """DiTAttention (dit.py:108-116) on rows: softmax(qn kn^T / sqrt(D)) v per head on the bf16 rows, qn / kn the QK-normed heads.
    The output is Attend's bf16 result in the compute dtype.  gq / gk None: attn_qk_norm=False."""

    @staticmethod
    def forward(ctx, x, w, gq, gk, cache, H, D):
        raw, qkv, inv, o, lse = _attn_rows(x, w, gq, gk, cache, H, D)
        ctx.save_for_backward(x, w, raw, qkv, o, lse, *((inv, gq, gk) if gq is not None else ()))
        ctx.cache, ctx.hd, ctx.norm = cache, (H, D), gq is not None
        return ops.cast_rows(o, x.dtype)

    @staticmethod
    def backward(ctx, go):
        x, w, raw, qkv, o, lse, *nrm = ctx.saved_tensors
        H, D = ctx.hd
        B, L, _ = x.shape
        do = ops.cast_rows(Fn._rc(go), torch.bfloat16)       # Attend hands SDPA its gradient in bf16
        dqkv = ops.mqa_bwd(qkv, o, do, lse, B, L, H, D, D ** -0.5, torch.float32, variant=ops.ATTN_BWD_DEFAULT, kv_heads=H)
        dgq = dgk = None
        if ctx.norm:
            inv, gq, gk = nrm
            draw, dgamma = qknorm_bwd(dqkv, raw, inv, gq, gk, H, D)
            dgq, dgk = dgamma[0].view(gq.shape), dgamma[1].view(gk.shape)
        else:
            draw = ops.cast_rows(dqkv, x.dtype)
        need = ctx.needs_input_grad
        dx = Fn.conv_dgrad(draw, w, ctx.cache, "same", L) if need[0] else None
        dw = Fn.conv_wgrad(draw, x, w, "same") if need[1] else None
        return dx, dw, dgq, dgk, None, None, None


def dit_attention(x, w, gq, gk, cache, H: int, D: int) -> torch.Tensor:
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, w, gq, gk)):
        return DiTAttentionFn.apply(x, w, gq, gk, cache, H, D)
    return ops.cast_rows(_attn_rows(x, w, gq, gk, cache, H, D, one_launch=ops.one_launch_attention_on())[3], x.dtype)      # nothing kept


class DiTFeedForwardFn(torch.autograd.Function):
    """FeedForward (dit.py:53-60): W2 silu(W1 x + b1) + b2 on rows, SiLU in the first GEMM's epilogue."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, cache):
        h, pre = Fn.conv_forward(x, w1, b1, cache, "same", None, act=1, want_pre=True)
        wp2 = cache.packs(("p2", x.dtype), (w2,), w2, "same", x.dtype)[0]
        out = ops.gemm_nt(h, wp2, b2, out_shape=x.shape)
        ctx.save_for_backward(x, w1, w2, h, pre)
        ctx.cache, ctx.b1, ctx.b2 = cache, b1, b2
        return out

    @staticmethod
    def backward(ctx, dout):
        x, w1, w2, h, pre = ctx.saved_tensors
        dout = Fn._rc(dout)
        cache = ctx.cache
        wd2 = cache.packs(("p2", x.dtype), (w2,), w2, "same", x.dtype)[1]
        dpre = ops.gemm_nt(dout, wd2, None, dact=pre, out_shape=pre.shape)          # (dout W2) * silu'(pre)
        need = ctx.needs_input_grad
        dw2, db2 = Fn.conv_wgrad_bias(dout, h, w2, "same", ctx.b2, need[3], need[4])
        dw1, db1 = Fn.conv_wgrad_bias(dpre, x, w1, "same", ctx.b1, need[1], need[2])
        dx = None
        if need[0]:
            wd1 = cache.packs(("p", "same", x.dtype, ""), (w1,), w1, "same", x.dtype)[1]
            dx = ops.gemm_nt(dpre, wd1, None, out_shape=x.shape)
        return dx, dw1, db1, dw2, db2, None
