"""Windowed sampling: generate a song longer than the trained context by fused-window denoising (MultiDiffusion).  At every step the
iterate is cut into overlapping windows of the trained length (osuf_window_gather), the denoiser runs on all windows as one batch, and
the window predictions are fused back into one full-length prediction by a tapered, normalised overlap-add (osuf_window_fuse, both in
csrc/sampling.hip; reached as ops.window_gather / ops.window_fuse).  The step kernels then work on the full-length tensors as they do
without windows.  The window layout, the taper, the allocating wrappers and the argument rules of every sample() live here, as
inpaint.py's do; the closure the sampling loops (models/base._OsuFusion._run, ode.ode_loop) call is
_TransformerOsuFusion._windowed_denoiser (models/transformer_diffusion.py); the UNet family has no windowed closure yet.  The
guarded-memory cases are in tests/test_windowed_gpu.py."""
from __future__ import annotations

from typing import List, NamedTuple, Optional

import numpy as np
import torch

from . import ops

TAPERS = ("trapezoid", "flat")


def _check_layout(n: int, window: int, stride: int) -> None:
    if window < 1:
        raise ValueError(f"window must be >= 1 (got {window})")
    if not 1 <= stride <= window:
        raise ValueError(f"the window stride must be in [1, window = {window}] (got {stride})")
    if n < 1:
        raise ValueError(f"windows over {n} frames")


def window_starts(n: int, window: int, stride: int) -> List[int]:
    """The starts of the windows over n frames, every window exactly `window` frames long: [0] for n <= window, else
    W = ceil((n - window) / stride) + 1 starts s_j = min(j * stride, n - window).  Only the last start is clamped, so the last window may
    overlap its predecessor by more than window - stride."""
    n, window, stride = int(n), int(window), int(stride)
    _check_layout(n, window, stride)
    if n <= window:
        return [0]
    W = -(-(n - window) // stride) + 1
    return [min(j * stride, n - window) for j in range(W)]


def window_weight(window: int, stride: int, taper: str = "trapezoid") -> torch.Tensor:
    """fp32 (window,) on the host, every weight strictly positive (a song's first and last frames are covered by one window only).
    "trapezoid": with r = window - stride, w[i] = min(1, (i + 1) / (r + 1), (window - i) / (r + 1)), evaluated in fp64 and rounded once;
    the smallest weight is 1 / (r + 1).  "flat": all ones (a plain mean over the covering windows)."""
    window, stride = int(window), int(stride)
    _check_layout(window, window, stride)
    if taper not in TAPERS:
        raise ValueError(f"Unknown window taper: {taper!r} (one of {list(TAPERS)})")
    if taper == "flat":
        return torch.ones(window, dtype=torch.float32)
    r = window - stride
    i = np.arange(window, dtype=np.float64)
    w = np.minimum(1.0, np.minimum((i + 1.0) / (r + 1.0), (window - i) / (r + 1.0)))
    return torch.from_numpy(w.astype(np.float32))


class WindowPlan(NamedTuple):
    """What sample(window=...) resolved to: the window length, the stride, the taper's name and the rows per denoiser call (None: all)."""
    window: int
    stride: int
    taper: str
    batch: Optional[int]


def plan(window, window_stride, window_taper, window_batch, patch_size: int = 1) -> Optional[WindowPlan]:
    """The window keywords of every sample() -> a WindowPlan, or None when no window is asked for.  window_stride defaults to
    window * 3 // 4 rounded down to a multiple of patch_size.  ValueError: window < 1; a stride outside [1, window]; an unknown taper;
    window_batch < 1; window or the stride not a multiple of patch_size; any other window keyword given while window is None."""
    if window is None:
        if window_stride is not None or window_batch is not None or window_taper != "trapezoid":
            raise ValueError("window_stride, window_taper and window_batch need window= (windowed sampling is off while window is None)")
        return None
    window, p = int(window), int(patch_size)
    if window < 1:
        raise ValueError(f"window must be >= 1 (got {window})")
    if window % p:
        raise ValueError(f"window must be a multiple of the backbone's patch size {p} (got {window})")
    stride = (window * 3 // 4) // p * p if window_stride is None else int(window_stride)
    if not 1 <= stride <= window:
        raise ValueError(f"window_stride must be in [1, window = {window}] (got {stride})")
    if stride % p:
        raise ValueError(f"window_stride must be a multiple of the backbone's patch size {p} (got {stride})")
    if window_taper not in TAPERS:
        raise ValueError(f"Unknown window taper: {window_taper!r} (one of {list(TAPERS)})")
    if window_batch is not None:
        window_batch = int(window_batch)
        if window_batch < 1:
            raise ValueError(f"window_batch must be >= 1 (got {window_batch})")
    return WindowPlan(window, stride, window_taper, window_batch)


def check_length(n: int, wp: WindowPlan, patch_size: int = 1) -> bool:
    """-> whether a sequence of n frames is windowed under `wp` (n > window); then n must be a multiple of patch_size."""
    if n <= wp.window:
        return False
    if n % int(patch_size):
        raise ValueError(f"a windowed sample needs a length that is a multiple of the backbone's patch size {patch_size} (got {n})")
    return True


def _fp32_3d(t: torch.Tensor, what: str) -> None:
    assert t.dim() == 3 and t.dtype == torch.float32 and t.is_contiguous() and t.is_cuda, f"{what} is fp32 contiguous (rows, D, length) on the GPU"


def window_gather(src: torch.Tensor, window: int, stride: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """src fp32 contiguous (R, D, n), n >= window -> (R * W, D, window), out[r * W + j, d, i] = src[r, d, s_j + i] with
    s = window_starts(n, window, stride): a copy of bits.  out must not overlap src.  One launch."""
    _fp32_3d(src, "src")
    R, D, n = src.shape
    window, stride = int(window), int(stride)
    _check_layout(n, window, stride)
    assert n >= window, "window_gather needs n >= window"
    W = len(window_starts(n, window, stride))
    if out is None:
        out = torch.empty((R * W, D, window), dtype=torch.float32, device=src.device)
    else:
        _fp32_3d(out, "out")
        assert tuple(out.shape) == (R * W, D, window) and out.device == src.device
    ops.call("osuf_window_gather", ops._p(src), ops._p(out), R, W, D, n, window, stride, ops._stream())
    return out


def window_fuse(pred: torch.Tensor, weight: torch.Tensor, n: int, stride: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """pred fp32 contiguous (R * W, D, window), the windows of window_starts(n, window, stride) row by row; weight fp32 (window,), every
    weight > 0 (window_weight's are; not checked here) -> (R, D, n).  A frame that one window covers takes that window's value bit for bit;
    elsewhere sum_j w pred / sum_j w over the covering windows in ascending j, fp32, products rounded before their adds, one division.
    out must not overlap pred.  One launch; every element is written by one lane, so the result is deterministic."""
    _fp32_3d(pred, "pred")
    RW, D, window = pred.shape
    n, stride = int(n), int(stride)
    _check_layout(n, window, stride)
    assert n >= window, "window_fuse needs n >= window"
    W = len(window_starts(n, window, stride))
    assert RW % W == 0, f"pred holds {RW} windows, not a multiple of the {W} windows of one sequence"
    R = RW // W
    assert weight.dtype == torch.float32 and weight.is_contiguous() and tuple(weight.shape) == (window,) and weight.device == pred.device
    if out is None:
        out = torch.empty((R, D, n), dtype=torch.float32, device=pred.device)
    else:
        _fp32_3d(out, "out")
        assert tuple(out.shape) == (R, D, n) and out.device == pred.device
    ops.call("osuf_window_fuse", ops._p(pred), ops._p(weight), ops._p(out), R, W, D, n, window, stride, ops._stream())
    return out
