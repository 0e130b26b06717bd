"""An np.float32 restatement of windowed sampling's layout and kernels (osufusion_amd/windowed.py, osuf_window_gather / osuf_window_fuse;
the reference has no such feature, the definition is the project's own): `starts`, `weight`, `gather` and `fuse32`, the fuse rule applied
literally, frame by frame -- a single covering window is a select, otherwise ascending-j fp32 sums that start from the first term, every
product rounded before its add, one division.  Bit-comparable with the kernels.  A helper module, imported by tests/test_windowed_*.py."""
from __future__ import annotations

from typing import List

import numpy as np

f32 = np.float32


def starts(n: int, window: int, stride: int) -> List[int]:
    assert 1 <= stride <= window and n >= 1
    if n <= window:
        return [0]
    W = -(-(n - window) // stride) + 1
    return [min(j * stride, n - window) for j in range(W)]


def weight(window: int, stride: int, taper: str = "trapezoid") -> np.ndarray:
    assert 1 <= stride <= window
    if taper == "flat":
        return np.ones(window, f32)
    assert taper == "trapezoid"
    r = window - stride
    w = [min(1.0, (i + 1) / (r + 1), (window - i) / (r + 1)) for i in range(window)]       # python floats: fp64, rounded once below
    return np.array(w, np.float64).astype(f32)


def gather(src: np.ndarray, window: int, stride: int) -> np.ndarray:
    """(R, D, n) -> (R * W, D, window)."""
    R, D, n = src.shape
    assert n >= window
    s = starts(n, window, stride)
    return np.stack([src[r, :, sj:sj + window] for r in range(R) for sj in s]).astype(src.dtype, copy=False).reshape(R * len(s), D, window)


def cover(n: int, window: int, stride: int) -> List[List[int]]:
    """Per frame, the windows that cover it, in ascending j (by search over the starts, not by the kernel's closed form)."""
    s = starts(n, window, stride)
    return [[j for j, sj in enumerate(s) if sj <= l < sj + window] for l in range(n)]


def fuse32(pred: np.ndarray, w: np.ndarray, n: int, stride: int) -> np.ndarray:
    """(R * W, D, window), (window,) -> (R, D, n) in np.float32, one rounding per operation."""
    pred, w = np.asarray(pred, f32), np.asarray(w, f32)
    RW, D, window = pred.shape
    s = starts(n, window, stride)
    W = len(s)
    assert RW % W == 0 and n >= window
    p = pred.reshape(RW // W, W, D, window)
    out = np.empty((RW // W, D, n), f32)
    with np.errstate(all="ignore"):
        for l, J in enumerate(cover(n, window, stride)):
            if len(J) == 1:
                out[:, :, l] = p[:, J[0], :, l - s[J[0]]]
                continue
            num = den = None
            for j in J:
                wj = w[l - s[j]]
                wp = (wj * p[:, j, :, l - s[j]]).astype(f32)
                num = wp if num is None else (num + wp).astype(f32)
                den = wj if den is None else f32(den + wj)
            out[:, :, l] = (num / den).astype(f32)
    return out
