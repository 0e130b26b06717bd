"""HIP-backed mirror of osu_fusion/modules/attention.py.

``RotaryPositionEmbedding`` and ``Attend`` keep the reference's call signatures on (B, H, N, D) tensors; the UNet's
own Attention block does not go through them (it uses the fused LN -> QKV -> RoPE -> flash path of functional.py),
they exist so code written against the reference's attention.py keeps working on the HIP kernels.  Both are
differentiable, as in the reference (osufusion_amd/attend.py): with nothing to differentiate, or under no_grad /
inference_mode, they run the bare kernel launches and keep nothing.
"""
from typing import Optional, Tuple

import torch
import torch.nn as nn

from .. import attend as At
from .. import cross_attend as Xa
from .. import functional as Fn
from .. import runtime as rt


class RotaryPositionEmbedding(nn.Module):
    """attention.py:15-58: positions rescaled by scale_base / seq_len, half-split rotation.  Outputs are rounded to bf16 (what Attend
    casts them to next) and returned in the input dtype; the gradient is the exact transpose of the rotation."""

    def __init__(self, dim: int, theta: int = 10000, scale_base: int = 4096) -> None:
        super().__init__()
        self.dim, self.theta, self.scale_base = dim, theta, scale_base
        inv_freq = 1.0 / (theta ** (torch.arange(0, dim, 2).float() / dim))
        self.register_buffer("inv_freq", inv_freq, persistent=False)

    def forward(self, q: torch.Tensor, k: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        rt.require_gpu(q)
        if self.dim % 16:
            raise NotImplementedError("the HIP RoPE kernel rotates head dims that are multiples of 16")
        cos, sin = Fn.rope_tables(q.shape[-2], self.dim, self.scale_base, q.device, float(self.theta))
        return At.rope(q, cos, sin), At.rope(k, cos, sin)


class Attend(nn.Module):
    """attention.py:61-101: q, k, v -> bf16, softmax(q k^T / sqrt(d) + attn_mask.to(bf16)) v, back to the input dtype.  k / v carry 1 or
    H heads and may be of another length than q.  A call with a mask or with another key count runs the generic kernels
    (osufusion_amd/cross_attend.py), the unmasked same-length call the tuned ones (osufusion_amd/attend.py).  Differentiable in q, k, v and a
    floating-point attn_mask (a k / v with one head gets the gradient summed over the query heads).  Rows whose every key is masked with
    -inf are NaN, as in SDPA."""

    def forward(self, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, attn_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        rt.require_gpu(q)
        D = Xa.check_shapes(q, k, v, attn_mask)[4]
        if D not in (16, 32, 64, 128):
            raise NotImplementedError("the HIP attention kernels cover head dims 16, 32, 64 and 128")
        return At.attend(q, k, v, attn_mask)
