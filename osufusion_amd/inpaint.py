"""Masked generation: keep the known parts of a beatmap while a sampler draws the rest (osuf_inpaint_blend, csrc/sampling.hip; reached as
ops.inpaint_blend).  The method is replacement conditioning: before an iterate goes to the denoiser its known region is overwritten by the
known signal noised to the iterate's own level, a known + s noise -- fresh noise per blend in the stochastic samplers (RePaint), one
fixed tensor in the deterministic ones, whose known region then follows the trajectory the sampler itself would take for that x_0.  The
allocating wrapper and the mask helpers live here, as ct.py's do; `Blender` is what the sampling loops of osufusion_amd/models share.
The guarded-memory cases are in tests/test_inpaint_gpu.py."""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch

from . import ops
from .audio import HOP_LENGTH, SR


def frame_times_ms(n: int) -> torch.Tensor:
    """fp64 (n,): frame l sits at l * 176 / 22050 * 1000 ms (audio.HOP_LENGTH, audio.SR), evaluated in that order."""
    return torch.arange(int(n), dtype=torch.float64) * HOP_LENGTH / SR * 1000.0


def frame_mask(n: int, spans_ms: Sequence[Tuple[float, float]], feather_ms: float = 0.0) -> torch.Tensor:
    """Spans [start, end] in milliseconds -> fp32 (n,) mask over frames, on the host: m[l] = max over spans of
    clamp(1 - d / feather_ms, 0, 1), d the distance in ms from frame l's time to the span (0 inside it).  feather_ms = 0: a hard 0/1 mask."""
    n, feather_ms = int(n), float(feather_ms)
    if n < 1:
        raise ValueError(f"a mask over {n} frames")
    if feather_ms < 0.0:
        raise ValueError(f"feather_ms must be >= 0 (got {feather_ms})")
    t = frame_times_ms(n)
    m = torch.zeros(n, dtype=torch.float64)
    for start, end in spans_ms:
        start, end = float(start), float(end)
        if end < start:
            raise ValueError(f"span ends before it starts: ({start}, {end})")
        d = torch.clamp(torch.maximum(start - t, t - end), min=0.0)
        w = (d == 0.0).double() if feather_ms == 0.0 else torch.clamp(1.0 - d / feather_ms, 0.0, 1.0)
        m = torch.maximum(m, w)
    return m.float()


def as_mask(known_mask: torch.Tensor, B: int, n: int, device) -> torch.Tensor:
    """A (n,), (B, n) or (B, 1, n) mask, bool or floating (1 / True = keep) -> fp32 contiguous rows on `device`: (n,) for a shared mask, else
    (B, n).  Values are expected in [0, 1]; they are not checked (a check would cost a host sync)."""
    if not isinstance(known_mask, torch.Tensor):
        raise ValueError(f"known_mask must be a tensor (got {type(known_mask).__name__})")
    if not (known_mask.dtype == torch.bool or known_mask.dtype.is_floating_point):
        raise ValueError(f"known_mask must be bool or floating (got {known_mask.dtype})")
    shape = tuple(known_mask.shape)
    if shape == (B, 1, n):
        known_mask = known_mask.reshape(B, n)
    elif shape not in ((n,), (B, n)):
        raise ValueError(f"known_mask must have shape ({n},), ({B}, {n}) or ({B}, 1, {n}) (got {shape})")
    return known_mask.to(device=device, dtype=torch.float32).contiguous()


def check_pair(known, known_mask) -> bool:
    """The both-or-neither rule of every sample(); -> whether a known region is given."""
    if (known is None) != (known_mask is None):
        raise ValueError("known and known_mask go together: give both (a masked sample) or neither")
    return known is not None


def inpaint_blend(x: torch.Tensor, known: torch.Tensor, mask: torch.Tensor, coef: Optional[torch.Tensor] = None, col_a: int = 0, col_s: int = 1,
                  noise: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = x where mask == 0, tgt where mask == 1, x + mask (tgt - x) between, with tgt = a known + s noise at the per-sample levels
    a = coef[b, col_a], s = coef[b, col_s] (rows of ct_schedule / ct_solver_schedule or the DDIM loop's 4-column rows, any row stride);
    noise None: tgt = a known; coef None: tgt = known, bit for bit.  x, known, noise, out: fp32 contiguous (B, Dch, L); mask (L,) (shared) or
    (B, L), fp32 in [0, 1] or bool (converted once here); out may be x.  One launch."""
    assert x.dim() == 3 and x.dtype == torch.float32 and x.is_contiguous(), "x is fp32 contiguous (B, Dch, L)"
    B, Dch, L = x.shape
    for v in (known, noise, out):
        assert v is None or (v.dtype == torch.float32 and v.is_contiguous() and v.shape == x.shape and v.device == x.device)
    if mask.dtype == torch.bool:
        mask = mask.float()
    assert mask.dtype == torch.float32 and mask.device == x.device and mask.stride(-1) == 1 and mask.shape in ((L,), (B, L))
    mask_ld = 0 if mask.dim() == 1 else (mask.stride(0) if B > 1 else L)
    assert mask_ld >= 0
    coef_ld = 0
    if coef is not None:
        assert coef.dtype == torch.float32 and coef.device == x.device and coef.dim() == 2 and coef.shape[0] == B and coef.stride(1) == 1
        assert 0 <= col_a < coef.shape[1] and 0 <= col_s < coef.shape[1]
        coef_ld = coef.stride(0) if B > 1 else coef.shape[1]
        assert coef_ld >= 1
    if out is None:
        out = torch.empty_like(x)
    ops.call("osuf_inpaint_blend", ops._p(x), ops._p(known), ops._p(noise), ops._p(mask), mask_ld, ops._p(coef), coef_ld, int(col_a), int(col_s),
             ops._p(out), B, Dch, L, ops._stream())
    return out


class Blender:
    """The known region of one sample() call.  `fixed`: the deterministic loops' one noise tensor, a clone of the start iterate taken before
    the first blend; None draws a fresh torch.randn of the iterate's shape per level blend (the stochastic loops).  The exact blend draws
    nothing."""

    def __init__(self, known: torch.Tensor, known_mask: torch.Tensor, x: torch.Tensor, fresh: bool) -> None:
        if not isinstance(known, torch.Tensor) or tuple(known.shape) != tuple(x.shape):
            raise ValueError(f"known must have the iterate's shape {tuple(x.shape)} (got {tuple(getattr(known, 'shape', ()))})")
        self.known = known.to(device=x.device, dtype=torch.float32).contiguous()
        self.mask = as_mask(known_mask, x.shape[0], x.shape[-1], x.device)
        self.fixed = None if fresh else x.clone()

    def level(self, x: torch.Tensor, coef: torch.Tensor, col_a: int, col_s: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        noise = torch.randn(x.shape, device=x.device) if self.fixed is None else self.fixed
        return inpaint_blend(x, self.known, self.mask, coef, col_a, col_s, noise, out)

    def exact(self, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        return inpaint_blend(x, self.known, self.mask, out=out)
