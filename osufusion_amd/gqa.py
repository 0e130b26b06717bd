"""The grouped-query attention forward with every K/V group in one launch (osuf_gqa_fwd, csrc/attn.hip); reached as ops.gqa_fwd."""
from __future__ import annotations

import torch

from . import ops


def gqa_fwd(qkv: torch.Tensor, B: int, N: int, H: int, D: int, out_dtype: torch.dtype, scale: float, kv_heads: int = 1):
    """qkv: bf16 rows [B*N][(H+2G)*D] (H query heads GROUP-MAJOR | G k heads | G v heads), as ops.mqa_fwd(kv_heads=G) takes them.
    Returns o rows [B*N][H*D] and lse2 ([B][H][N] for G == 1, else [G][B][H/G][N])."""
    M, W, ld = ops._rows(qkv)
    G = kv_heads
    assert qkv.dtype == torch.bfloat16 and W == (H + 2 * G) * D and H % G == 0
    o = torch.empty((B, N, H * D), dtype=out_dtype, device=qkv.device)
    lse = torch.empty((B, H, N) if G == 1 else (G, B, H // G, N), dtype=torch.float32, device=qkv.device)
    base = qkv.data_ptr()
    ops.call("osuf_gqa_fwd", base, ld, base + 2 * H * D, ld, base + 2 * (H + G) * D, ld, o.data_ptr(), H * D, ops._DT[out_dtype], lse.data_ptr(),
             B, H, G, N, D, scale, ops._stream(), meta=ops.LaunchSize(N, B))
    return o, lse
