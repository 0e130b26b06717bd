"""An fp64 numpy restatement of the continuous-time solvers on a log-SNR grid -- DDIM(eta) and DPM-Solver++(2M), data prediction: what
osuf_ct_solver_schedule and osuf_ct_solver_step compute -- with a whole-loop driver for any denoiser and the Gaussian toy problem whose
optimal denoiser and probability-flow solution are closed forms.  A helper module, imported by tests/test_ct_solver_*.py.

The reference has no code for either sampler (its scheduler samples ancestrally); the formulas are those of the issue that asked for the
feature: DDIM (Song et al.) with eta interpolating to the ancestral sampler, and DPM-Solver++(2M) (Lu et al., algorithm 2) with
lambda = log_snr / 2.  Both are  x_next = k_x x + k_0 x0 + k_p x0_prev + gain z  with x0 the clamped start prediction."""
from __future__ import annotations

from typing import Callable, Optional, Sequence, Tuple

import numpy as np

from tests import ct_objectives_oracle as CO

SAMPLERS = ("ddim", "dpmpp_2m")
K_X, K_0, K_P, GAIN = range(4)
f64 = CO.f64


def alpha_sigma(ls) -> Tuple[np.ndarray, np.ndarray]:
    ls = f64(ls)
    return np.sqrt(1.0 / (1.0 + np.exp(-ls))), np.sqrt(1.0 / (1.0 + np.exp(ls)))


def rows(grid) -> np.ndarray:
    """(S, 13): the schedule row of every step of the grid (S + 1 log-SNR values), columns as tests/scheduler_oracle.COLUMNS; the noise gain
    (column 12) of the last step is zero, as the ancestral sampler's at t_next = 0."""
    grid = f64(grid)
    ls, lsn = grid[:-1], grid[1:]
    (a, s), (an, sn) = alpha_sigma(ls), alpha_sigma(lsn)
    c = -np.expm1(ls - lsn)
    var = sn ** 2 * c
    logvar = np.log(np.maximum(var, 1e-20))
    gain = np.exp(0.5 * logvar)
    gain[-1] = 0.0
    return np.stack([ls, a, s, lsn, an, sn, c, var, logvar, 1.0 / np.maximum(a, 1e-8), an * ((1 - c) / a), an * c, gain], axis=1)


def factors(grid, sampler: str, eta: float = 0.0) -> Tuple[np.ndarray, np.ndarray]:
    """-> ((S, 4) = k_x, k_0, k_p, gain per step, (S,) = max(1, |k_d| (1 + 1 / (2 r))), the scale of the absolute bound on k_0 and k_p; one
    for DDIM, whose k_0 is a difference of two values of at most one)."""
    grid = f64(grid)
    ls, lsn = grid[:-1], grid[1:]
    (a, s), (an, sn) = alpha_sigma(ls), alpha_sigma(lsn)
    h = (lsn - ls) / 2
    out = np.zeros((len(ls), 4))
    scale = np.ones(len(ls))
    if sampler == "ddim":
        # sigma_eta^2 = eta^2 (sigma_n^2 / sigma^2) (1 - alpha^2 / alpha_n^2) = eta^2 sigma_n^2 (-expm1(ls - ls_n)), as alpha^2 / sigma^2 = exp(ls),
        # and k_eps^2 = sigma_n^2 - sigma_eta^2 = sigma_n^2 ((1 - eta^2) + eta^2 exp(ls - ls_n)).  The right-hand sides are evaluated: the
        # differences on the left cancel in fp64 too (the first step of the cosine time grid has exp(ls - ls_n) = 2.5e-13, so that at eta = 1
        # sigma_n^2 - sigma_eta^2 keeps 3 digits).  tests/test_ct_solver_cpu.py holds the two forms together where neither cancels.
        d = ls - lsn
        s_eta = eta * np.sqrt(sn ** 2 * -np.expm1(d))
        k_eps = sn * np.sqrt((1 - eta ** 2) + eta ** 2 * np.exp(d))
        out[:, K_X], out[:, K_0], out[:, GAIN] = k_eps / s, an - k_eps * a / s, s_eta
    elif sampler == "dpmpp_2m":
        k_d = -an * np.expm1(-h)
        out[:, K_X] = sn / s
        out[0, K_0] = k_d[0]
        r = h[:-1] / h[1:]
        out[1:, K_0] = k_d[1:] * (1 + 1 / (2 * r))
        out[1:, K_P] = -k_d[1:] / (2 * r)
        scale[0] = max(1.0, abs(k_d[0]))
        scale[1:] = np.maximum(1.0, np.abs(k_d[1:]) * (1 + 1 / (2 * r)))
    else:
        raise ValueError(sampler)
    return out, scale


def step(x, cond, null, cond_scale: float, row, fac, x0_prev, noise, objective: str, s=None):
    """osuf_ct_solver_step -> (x_next, x0, the largest |term| per element of the sums and products it forms).  row (B, 13) and fac (4,) as
    given (the kernel's own fp32 values in the GPU tests)."""
    x = f64(x)
    p = CO.guided(cond, null, cond_scale)
    raw = CO.start_from(x, p, row, objective)
    if s is None:
        x0 = np.clip(raw, -1.0, 1.0)
    else:
        sv = f64(s).reshape((-1,) + (1,) * (x.ndim - 1))
        x0 = np.clip(raw, -sv, sv) / sv
    k_x, k_0, k_p, gain = (float(v) for v in f64(fac))
    out = k_x * x + k_0 * x0
    terms = [np.abs(x), np.abs(p), np.abs(CO._col(row, CO.SIGMA, x) * p), np.abs(CO._col(row, CO.ALPHA, x) * x), np.abs(raw), np.abs(k_x * x),
             np.abs(k_0 * x0), np.abs(out)]
    if null is not None:
        terms += [np.abs(f64(null)), np.abs((f64(cond) - f64(null)) * cond_scale)]
    if x0_prev is not None and k_p != 0:
        out = out + k_p * f64(x0_prev)
        terms += [np.abs(k_p * f64(x0_prev)), np.abs(out)]
    if noise is not None and gain != 0:
        out = out + gain * f64(noise)
        terms += [np.abs(gain * f64(noise)), np.abs(out)]
    return out, x0, np.max(np.stack([np.broadcast_to(t, out.shape) for t in terms]), axis=0)


def loop(denoiser: Callable[[np.ndarray, float], np.ndarray], x, grid, sampler: str, eta: float = 0.0, objective: str = "x_start",
         noises: Optional[Sequence] = None, schedule_rows=None, fac=None) -> np.ndarray:
    """The whole sampler: per step one denoiser(x, log_snr) -> the prediction for `objective`, one step().  noises: one array per step for
    DDIM with eta > 0.  schedule_rows / fac: the kernel's own values instead of the restatement's."""
    x = f64(x)
    R = rows(grid) if schedule_rows is None else f64(schedule_rows)
    Fc = factors(grid, sampler, eta)[0] if fac is None else f64(fac)
    prev = None
    for i in range(len(R)):
        row = np.broadcast_to(R[i], (x.shape[0], 13))
        pred = denoiser(x, float(f64(grid)[i]))
        x, prev, _ = step(x, pred, None, 1.0, row, Fc[i], prev, None if noises is None else noises[i], objective)
    return x


# ---- the toy problem: data N(mean, std^2) per element ------------------------------------------------------------------------------------
TOY_MEAN, TOY_STD = 0.2, 0.1


def toy_denoiser(x, log_snr: float) -> np.ndarray:
    """E[x_0 | x_t] for x_t = alpha x_0 + sigma eps: the optimal x_start prediction."""
    a, s = alpha_sigma(log_snr)
    return TOY_MEAN + a * TOY_STD ** 2 / (a ** 2 * TOY_STD ** 2 + s ** 2) * (f64(x) - a * TOY_MEAN)


def toy_exact(x_start, ls_start: float, ls_end: float) -> np.ndarray:
    """The probability-flow ODE's solution: the marginals are N(alpha mean, alpha^2 std^2 + sigma^2) and the flow keeps the quantile."""
    (a0, s0), (a1, s1) = alpha_sigma(ls_start), alpha_sigma(ls_end)
    sd0, sd1 = np.sqrt(a0 ** 2 * TOY_STD ** 2 + s0 ** 2), np.sqrt(a1 ** 2 * TOY_STD ** 2 + s1 ** 2)
    return a1 * TOY_MEAN + sd1 / sd0 * (f64(x_start) - a0 * TOY_MEAN)


def rms(a, b) -> float:
    return float(np.sqrt(np.mean((f64(a) - f64(b)) ** 2)))
