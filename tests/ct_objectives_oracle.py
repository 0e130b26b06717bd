"""An fp64 numpy restatement of the continuous-time scheduler's prediction objectives (noise, x_start, v), dynamic thresholding and
min-SNR-gamma weighting: what osuf_ct_x0_quantile, osuf_ct_step_ex, osuf_ct_qsample and osuf_mse_w compute.  A helper module, imported by
tests/test_ct_objectives_*.py.

The reference has no code for any of this (its scheduler predicts noise, clamps statically and weights nothing): the formulas are those
of the issue that asked for the feature -- Imagen's dynamic thresholding (section 2.3), v = alpha noise - sigma x_0 (Salimans & Ho),
min-SNR-gamma (Hang et al.) -- and torch.quantile's / np.quantile's linear interpolation.  Schedule rows are taken as given (the
kernel's own fp32 row, columns as tests/scheduler_oracle.COLUMNS), so only the arithmetic downstream of the row is restated."""
from __future__ import annotations

import math
from typing import Optional, Tuple

import numpy as np

OBJECTIVES = ("noise", "x_start", "v")
ALPHA, SIGMA, INV_ALPHA, K_X, K_X0, NOISE_GAIN = 1, 2, 9, 10, 11, 12


def f64(v) -> np.ndarray:
    return np.asarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v, dtype=np.float64)


def _col(row: np.ndarray, j: int, like: np.ndarray) -> np.ndarray:
    return f64(row)[:, j].reshape((-1,) + (1,) * (like.ndim - 1))


def guided(cond, null, cond_scale: float) -> np.ndarray:
    cond = f64(cond)
    return cond if null is None else f64(null) + (cond - f64(null)) * cond_scale


def start_from(x, p, row, objective: str) -> np.ndarray:
    """The unclamped start prediction from the (guided) prediction p."""
    x, p = f64(x), f64(p)
    if objective == "noise":
        return (x - _col(row, SIGMA, x) * p) * _col(row, INV_ALPHA, x)
    if objective == "x_start":
        return p
    if objective == "v":
        return _col(row, ALPHA, x) * x - _col(row, SIGMA, x) * p
    raise ValueError(objective)


def quantile_rank(q: float, n: int) -> Tuple[int, float]:
    pos = float(q) * (n - 1)
    k_lo = min(int(math.floor(pos)), n - 1)
    return k_lo, pos - k_lo


def threshold(x0, q: float) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Per sample: the order statistics of |x0| at ranks k_lo and min(k_lo + 1, n - 1), and s = max(1, lo + (hi - lo) frac)."""
    a = np.sort(np.abs(f64(x0)).reshape(len(x0), -1), axis=1)
    n = a.shape[1]
    k_lo, frac = quantile_rank(q, n)
    lo, hi = a[:, k_lo], a[:, min(k_lo + 1, n - 1)]
    return lo, hi, np.maximum(1.0, lo + (hi - lo) * frac)


def dynamic_threshold(x0, q: float) -> np.ndarray:
    x0 = f64(x0)
    s = threshold(x0, q)[2].reshape((-1,) + (1,) * (x0.ndim - 1))
    return np.clip(x0, -s, s) / s


def step(x, cond, null, cond_scale: float, row, noise, objective: str, s=None):
    """osuf_ct_step_ex -> (out, the largest |term| per element of the sums and products it forms)."""
    x = f64(x)
    p = guided(cond, null, cond_scale)
    raw = start_from(x, p, row, objective)
    if s is None:
        x0 = np.clip(raw, -1.0, 1.0)
    else:
        sv = f64(s).reshape((-1,) + (1,) * (x.ndim - 1))
        x0 = np.clip(raw, -sv, sv) / sv
    kx, kx0, gain = _col(row, K_X, x), _col(row, K_X0, x), _col(row, NOISE_GAIN, x)
    out = kx * x + kx0 * x0
    terms = [np.abs(x), np.abs(p), np.abs(_col(row, SIGMA, x) * p), np.abs(_col(row, ALPHA, x) * x), np.abs(raw), np.abs(kx * x),
             np.abs(kx0 * x0), np.abs(out)]
    if null is not None:
        terms += [np.abs(f64(null)), np.abs((f64(cond) - f64(null)) * cond_scale)]
    if noise is not None:
        add = np.where(gain != 0, gain * f64(noise), 0.0)
        out = out + add
        terms += [np.abs(add), np.abs(out)]
    return out, np.max(np.stack([np.broadcast_to(t, out.shape) for t in terms]), axis=0)


def q_sample(x_0, noise, alpha, sigma) -> np.ndarray:
    x_0 = f64(x_0)
    a, s = (f64(v).reshape((-1,) + (1,) * (x_0.ndim - 1)) for v in (alpha, sigma))
    return a * x_0 + s * f64(noise)


def calculate_v(x_0, noise, alpha, sigma) -> np.ndarray:
    x_0 = f64(x_0)
    a, s = (f64(v).reshape((-1,) + (1,) * (x_0.ndim - 1)) for v in (alpha, sigma))
    return a * f64(noise) - s * x_0


def predict_start_from_v(x_t, v, alpha, sigma) -> np.ndarray:
    x_t = f64(x_t)
    a, s = (f64(v_).reshape((-1,) + (1,) * (x_t.ndim - 1)) for v_ in (alpha, sigma))
    return a * x_t - s * f64(v)


def predict_start_from_noise(x_t, noise, alpha, sigma) -> np.ndarray:
    x_t = f64(x_t)
    a, s = (f64(v).reshape((-1,) + (1,) * (x_t.ndim - 1)) for v in (alpha, sigma))
    return (x_t - s * f64(noise)) / np.maximum(a, 1e-8)


def target_of(x_0, noise, alpha, sigma, objective: str) -> np.ndarray:
    return {"noise": lambda: f64(noise), "x_start": lambda: f64(x_0), "v": lambda: calculate_v(x_0, noise, alpha, sigma)}[objective]()


def posterior_mean(x_t, x_0, alpha, alpha_next, c) -> np.ndarray:
    x_t = f64(x_t)
    a, an, cc = (f64(v).reshape((-1,) + (1,) * (x_t.ndim - 1)) for v in (alpha, alpha_next, c))
    return an * (x_t * (1 - cc) / a + cc * f64(x_0))


def loss_weight(log_snr, objective: str, gamma: Optional[float]) -> Optional[np.ndarray]:
    if gamma is None:
        return None
    snr = np.exp(f64(log_snr))
    c = np.minimum(snr, gamma)
    return {"noise": c / snr, "x_start": c, "v": c / (snr + 1)}[objective]


def mse_w(pred, target, orig_len, w) -> float:
    """sum_b w_b sum_{d, l < len_b} (pred - target)^2 / sum_b D len_b   (w None: ones; orig_len None: full length)."""
    pred, target = f64(pred), f64(target)
    B, D, L = pred.shape
    lens = np.full(B, L) if orig_len is None else np.minimum(np.asarray(orig_len, dtype=np.int64), L)
    mask = (np.arange(L)[None, :] < lens[:, None]).astype(np.float64)[:, None, :]
    wv = np.ones(B) if w is None else f64(w)
    return float((wv[:, None, None] * mask * (pred - target) ** 2).sum() / (D * lens.sum()))
