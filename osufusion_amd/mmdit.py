"""Kernels and autograd of the MMDiT's joint attention (modules/mmdit.py, a mirror of osu_fusion/modules/mmdit.py).

JointAttention (mmdit.py:94-127) attends over the concatenated sequence [audio; map] with H query heads on G K/V heads.  Here the two
streams stay separate rows (B, Ns, dim) up to the projections; one bf16 buffer (B, Nj = Na + Nx, (H + 2G) D) then holds the packed
q | k | v rows the attention kernels read:
  * rows: sample b's Na audio rows, then its Nx map rows (pack([.._a, .._x], "b h * d"));
  * columns: H query heads GROUP-MAJOR, G key heads, G value heads (what ops.mqa_fwd(kv_heads=G) documents).  The reference repeats
    K/V as "b h n d -> b (r h) n d", so natural query head j reads K/V head j % G and goes to column block (j % G) * (H / G) + j / G.
The row kernels of csrc/dit.hip do the packing, the QK-norm and their transposes, one call per stream (the other stream's joint rows
are never touched); the attention itself is ops.mqa_fwd / ops.mqa_bwd at N = Nj.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib
from . import functional as Fn
from . import ops


# ---------------------------------------------------------------------------------------------------------
# wrappers (one C-ABI entry point each).  `joint`: the (B, Nj, W) bf16 buffer both streams write into; off: the stream's row offset
# ---------------------------------------------------------------------------------------------------------
def _geom(rows: torch.Tensor, joint: torch.Tensor, off: int):
    B, Ns = rows.shape[0], rows.shape[1]
    Nj = joint.shape[1]
    assert joint.shape[0] == B and joint.is_contiguous() and 0 <= off and off + Ns <= Nj
    return B * Ns, Ns, Nj


def joint_buffer(B: int, Nj: int, W: int, device, dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    return torch.empty((B, Nj, W), dtype=dtype, device=device)


def joint_qknorm_fwd(raw: torch.Tensor, joint: torch.Tensor, off: int, gamma_q: Optional[torch.Tensor], gamma_k: Optional[torch.Tensor],
                     H: int, G: int, D: int) -> Optional[torch.Tensor]:
    """One stream's raw q|k|v projection rows (B, Ns, (H + 2G) D) -> its rows of the bf16 joint buffer; -> inv norms (B*Ns, H + G) fp32
    (None without gammas: cast and permute only)."""
    M, W, ld = ops._rows(raw)
    _, Ns, Nj = _geom(raw, joint, off)
    assert W == (H + 2 * G) * D and joint.dtype == torch.bfloat16 and joint.shape[2] == W
    inv = None
    if gamma_q is not None:
        assert gamma_q.dtype == gamma_k.dtype == torch.float32 and gamma_q.is_contiguous() and gamma_k.is_contiguous()
        assert gamma_q.numel() == H * D and gamma_k.numel() == G * D
        inv = torch.empty((M, H + G), dtype=torch.float32, device=raw.device)
    ops.call("osuf_joint_qknorm_fwd", ops.dt_of(raw), raw.data_ptr(), ld, joint.data_ptr(), W, ops._p(inv), ops._p(gamma_q), ops._p(gamma_k),
             M, Ns, Nj, off, H, G, D, ops._stream())
    return inv


def joint_pack(rows: torch.Tensor, joint: torch.Tensor, off: int, H: int, G: int, D: int) -> torch.Tensor:
    """One stream's rows (B, Ns, H D), natural head order -> its rows of the bf16 joint buffer (B, Nj, H D), group-major."""
    M, W, ld = ops._rows(rows)
    _, Ns, Nj = _geom(rows, joint, off)
    assert W == H * D and joint.dtype == torch.bfloat16 and joint.shape[2] == W
    ops.call("osuf_joint_pack", ops.dt_of(rows), rows.data_ptr(), ld, joint.data_ptr(), W, M, Ns, Nj, off, H, G, D, ops._stream())
    return joint


def joint_unpack(joint: torch.Tensor, Ns: int, off: int, dtype: torch.dtype, H: int, G: int, D: int) -> torch.Tensor:
    """The transpose of joint_pack: -> the stream's rows (B, Ns, H D) in `dtype`, heads in natural order."""
    B, Nj, W = joint.shape
    assert W == H * D and joint.dtype == torch.bfloat16 and joint.is_contiguous() and 0 <= off and off + Ns <= Nj
    out = torch.empty((B, Ns, W), dtype=dtype, device=joint.device)
    ops.call("osuf_joint_unpack", ops.dt_of(out), joint.data_ptr(), W, out.data_ptr(), W, B * Ns, Ns, Nj, off, H, G, D, ops._stream())
    return out


def joint_qknorm_bwd(dqkv: torch.Tensor, raw: torch.Tensor, off: int, inv: Optional[torch.Tensor], gamma_q: Optional[torch.Tensor],
                     gamma_k: Optional[torch.Tensor], H: int, G: int, D: int):
    """fp32 dq|dk|dv joint rows (ops.mqa_bwd) -> (gradient of the stream's raw projections in raw.dtype, dgamma (H + G, D) fp32 = q | k,
    or None without gammas)."""
    M, W, ld = ops._rows(raw)
    _, Ns, Nj = _geom(raw, dqkv, off)
    assert dqkv.dtype == torch.float32 and dqkv.shape[2] == W == (H + 2 * G) * D
    dev = raw.device
    dx = torch.empty(raw.shape, dtype=raw.dtype, device=dev)
    dgamma = ws = None
    need = 0
    if gamma_q is not None:
        assert inv is not None and inv.is_contiguous() and inv.numel() == (H + G) * M
        dgamma = torch.empty((H + G, D), dtype=torch.float32, device=dev)
        need = _lib.load().osuf_joint_qknorm_bwd_workspace_bytes(M, H, G, D)
        assert need > 0, "osuf_joint_qknorm_bwd: unsupported shape"
        ws = torch.empty(need // 4, dtype=torch.float32, device=dev)
    ops.call("osuf_joint_qknorm_bwd", ops.dt_of(raw), dqkv.data_ptr(), W, raw.data_ptr(), ld, ops._p(inv), ops._p(gamma_q), ops._p(gamma_k),
             dx.data_ptr(), W, ops._p(dgamma), ops._p(ws), need, M, Ns, Nj, off, H, G, D, ops._stream())
    return dx, dgamma


# ---------------------------------------------------------------------------------------------------------
# autograd
# ---------------------------------------------------------------------------------------------------------
def _qkv_packs(cache, dt, tag: str, wq, wk, wv):
    """(forward, dgrad) operands of to_q | to_k | to_v stacked along the output dim: the three parameters run as one GEMM."""
    return cache.packs(("qkv", tag, dt), (wq, wk, wv), (wq, wk, wv), "same", dt)


def _joint_rows(x, a, wx, wa, gx, ga, cache, H: int, G: int, D: int, one_launch: bool = False):
    """-> (raw_x, raw_a, bf16 joint q|k|v rows, inv_x, inv_a, joint o (bf16), lse2).  Audio rows first.  one_launch (inference): the G groups
    in one osuf_gqa_fwd launch instead of one osuf_mqa_fwd launch each; the same bits."""
    B, Nx, _ = x.shape
    Na = a.shape[1]
    W = (H + 2 * G) * D
    dt = x.dtype
    raw_x = ops.gemm_nt(x, _qkv_packs(cache, dt, "x", *wx)[0], None, out_shape=(B, Nx, W))
    raw_a = ops.gemm_nt(a, _qkv_packs(cache, dt, "a", *wa)[0], None, out_shape=(B, Na, W))
    qkv = joint_buffer(B, Na + Nx, W, x.device)
    inv_a = joint_qknorm_fwd(raw_a, qkv, 0, ga[0], ga[1], H, G, D)
    inv_x = joint_qknorm_fwd(raw_x, qkv, Na, gx[0], gx[1], H, G, D)
    fwd = ops.gqa_fwd if one_launch else ops.mqa_fwd
    o, lse = fwd(qkv, B, Na + Nx, H, D, torch.bfloat16, D ** -0.5, kv_heads=G)
    return raw_x, raw_a, qkv, inv_x, inv_a, o, lse


class JointAttentionFn(torch.autograd.Function):
    """JointAttention (mmdit.py:94-127) on rows: x (B, Nx, dim), a (B, Na, dim) -> (out_x (B, Nx, H D), out_a (B, Na, H D)), Attend's
    bf16 result in the compute dtype.  Forward: one q|k|v GEMM per stream, osuf_joint_qknorm_fwd per stream, ops.mqa_fwd at
    N = Na + Nx with G K/V heads, osuf_joint_unpack per stream.  Backward: osuf_joint_pack of dO per stream, ops.mqa_bwd,
    osuf_joint_qknorm_bwd per stream, then the dgrad / wgrad GEMMs.  gq_* / gk_* None: qk_norm=False."""

    @staticmethod
    def forward(ctx, x, a, wq_x, wk_x, wv_x, wq_a, wk_a, wv_a, gq_x, gk_x, gq_a, gk_a, cache, H, G, D):
        raw_x, raw_a, qkv, inv_x, inv_a, o, lse = _joint_rows(x, a, (wq_x, wk_x, wv_x), (wq_a, wk_a, wv_a), (gq_x, gk_x), (gq_a, gk_a),
                                                              cache, H, G, D)
        norm = gq_x is not None
        ctx.save_for_backward(x, a, wq_x, wk_x, wv_x, wq_a, wk_a, wv_a, qkv, o, lse,
                              *((raw_x, raw_a, inv_x, inv_a, gq_x, gk_x, gq_a, gk_a) if norm else ()))
        ctx.cache, ctx.geom, ctx.norm = cache, (H, G, D), norm
        Nx, Na = x.shape[1], a.shape[1]
        return joint_unpack(o, Nx, Na, x.dtype, H, G, D), joint_unpack(o, Na, 0, a.dtype, H, G, D)

    @staticmethod
    def backward(ctx, go_x, go_a):
        x, a, wq_x, wk_x, wv_x, wq_a, wk_a, wv_a, qkv, o, lse, *nrm = ctx.saved_tensors
        H, G, D = ctx.geom
        B, Nx, _ = x.shape
        Na = a.shape[1]
        Nj, HD = Na + Nx, H * D
        dt = x.dtype
        do = joint_buffer(B, Nj, HD, x.device)               # Attend hands SDPA its gradient in bf16
        joint_pack(Fn._rc(go_a), do, 0, H, G, D)
        joint_pack(Fn._rc(go_x), do, Na, H, G, D)
        dqkv = ops.mqa_bwd(qkv, o, do, lse, B, Nj, H, D, D ** -0.5, torch.float32, variant=ops.ATTN_BWD_DEFAULT, kv_heads=G)
        if ctx.norm:
            raw_x, raw_a, inv_x, inv_a, gq_x, gk_x, gq_a, gk_a = nrm
        else:
            raw_x = raw_a = inv_x = inv_a = gq_x = gk_x = gq_a = gk_a = None
        need = ctx.needs_input_grad
        grads = {}
        for tag, inp, raw, off, inv, gq, gk, ws, i_in, i_w, i_g in (
                ("x", x, raw_x, Na, inv_x, gq_x, gk_x, (wq_x, wk_x, wv_x), 0, 2, 8),
                ("a", a, raw_a, 0, inv_a, gq_a, gk_a, (wq_a, wk_a, wv_a), 1, 5, 10)):
            draw, dgamma = _stream_bwd(dqkv, raw, inp, off, inv, gq, gk, H, G, D, ctx.norm)
            if dgamma is not None:
                grads[i_g], grads[i_g + 1] = dgamma[:H].view(gq.shape), dgamma[H:].view(gk.shape)
            cols = (0, HD, HD + G * D, HD + 2 * G * D)
            for k, w in enumerate(ws):
                if need[i_w + k]:
                    grads[i_w + k] = Fn.conv_wgrad(draw[..., cols[k]:cols[k + 1]], inp, w, "same")
            if need[i_in]:
                grads[i_in] = ops.gemm_nt(draw, _qkv_packs(ctx.cache, dt, tag, *ws)[1], None, out_shape=inp.shape)
        return (*[grads.get(i) for i in range(12)], None, None, None, None)


def _stream_bwd(dqkv, raw, inp, off, inv, gq, gk, H, G, D, norm):
    if norm:
        return joint_qknorm_bwd(dqkv, raw, off, inv, gq, gk, H, G, D)
    return joint_unnorm_bwd(dqkv, inp, off, H, G, D), None


def joint_unnorm_bwd(dqkv: torch.Tensor, inp: torch.Tensor, off: int, H: int, G: int, D: int) -> torch.Tensor:
    """qk_norm=False: the stream's rows of the fp32 joint gradient, permuted back and cast to inp.dtype (osuf_joint_qknorm_bwd without
    gammas; the raw projections are not read)."""
    B, Ns = inp.shape[0], inp.shape[1]
    Nj, W = dqkv.shape[1], dqkv.shape[2]
    assert dqkv.dtype == torch.float32 and dqkv.is_contiguous() and W == (H + 2 * G) * D and off + Ns <= Nj
    dx = torch.empty((B, Ns, W), dtype=inp.dtype, device=inp.device)
    ops.call("osuf_joint_qknorm_bwd", ops.dt_of(dx), dqkv.data_ptr(), W, None, W, None, None, None, dx.data_ptr(), W, None, None, 0,
             B * Ns, Ns, Nj, off, H, G, D, ops._stream())
    return dx


def joint_attention(x, a, wx, wa, gx, ga, cache, H: int, G: int, D: int):
    """wx / wa: (to_q, to_k, to_v) weights of the map / audio stream; gx / ga: (gamma_q, gamma_k) or (None, None)."""
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, a, *wx, *wa, *gx, *ga)):
        return JointAttentionFn.apply(x, a, *wx, *wa, *gx, *ga, cache, H, G, D)
    o = _joint_rows(x, a, wx, wa, gx, ga, cache, H, G, D, one_launch=ops.one_launch_attention_on())[5]    # nothing kept
    return joint_unpack(o, x.shape[1], a.shape[1], x.dtype, H, G, D), joint_unpack(o, a.shape[1], 0, a.dtype, H, G, D)
