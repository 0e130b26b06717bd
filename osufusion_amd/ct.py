"""Continuous-time Gaussian diffusion on the device (osuf_ct_schedule, osuf_ct_step, csrc/elementwise.hip); reached as ops.ct_schedule /
ops.ct_step.  The allocating wrappers live here, as osufusion_amd/gqa.py's does; their guarded-memory cases are in
tests/test_scheduler_gpu.py."""
from __future__ import annotations

from typing import Optional

import torch

from . import ops

KINDS = {"linear": 0, "cosine": 1}
# columns of a schedule row (include/osufusion_hip.h)
LOG_SNR, ALPHA, SIGMA, LOG_SNR_NEXT, ALPHA_NEXT, SIGMA_NEXT, C, POST_VAR, POST_LOG_VAR, INV_ALPHA, K_X, K_X0, NOISE_GAIN = range(13)
COLS_T, COLS = 3, 13


def _times(t: torch.Tensor) -> torch.Tensor:
    assert t.dim() == 1, "times are one value per sample"
    return t.float().contiguous()


def ct_schedule(t: torch.Tensor, t_next: Optional[torch.Tensor] = None, kind: int = 0) -> torch.Tensor:
    """t (B,), t_next (B,) or None -> fp32 (B, 3) = log_snr, alpha, sigma, or (B, 13) with the posterior and step columns."""
    t = _times(t)
    if t_next is not None:
        t_next = _times(t_next)
        assert t_next.shape == t.shape and t_next.device == t.device
    out = torch.empty((t.shape[0], COLS if t_next is not None else COLS_T), dtype=torch.float32, device=t.device)
    ops.call("osuf_ct_schedule", ops._p(t), ops._p(t_next), int(kind), ops._p(out), t.shape[0], ops._stream())
    return out


def ct_step(x: torch.Tensor, cond: torch.Tensor, null: Optional[torch.Tensor], cond_scale: float, coef: torch.Tensor,
            noise: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One ancestral step over (B, ...) fp32 contiguous tensors; coef = ct_schedule(t, t_next, kind), (B, 13)."""
    for v in (x, cond, null, noise):
        assert v is None or (v.dtype == torch.float32 and v.is_contiguous() and v.shape == x.shape)
    assert coef.dtype == torch.float32 and coef.is_contiguous() and coef.shape == (x.shape[0], COLS)
    out = torch.empty_like(x)
    ops.call("osuf_ct_step", ops._p(x), ops._p(cond), ops._p(null), float(cond_scale), ops._p(coef), ops._p(noise), ops._p(out),
             x.shape[0], x[0].numel(), ops._stream())
    return out
