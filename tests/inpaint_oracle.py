"""A numpy restatement of masked generation by replacement conditioning (osufusion_amd/inpaint.py; the reference has no such feature, the
definition is the project's own).  Two parts: the blend of osuf_inpaint_blend in np.float32 with the kernel's roundings, bit-comparable;
and the masked sampling loops in fp64 around a denoiser passed in as a callable -- the DDIM loop (UNet and DiT), the midpoint flow loop
(UNet and DiT) and the continuous-time "ddpm", "ddim" and "dpmpp_2m" loops, with RePaint resampling on the ancestral one.  A helper module,
imported by tests/test_inpaint_*.py."""
from __future__ import annotations

from typing import Callable, List, Optional

import numpy as np

from tests import ct_solver_oracle as SV

f32 = np.float32


def _mask_like(mask, x, dtype):
    m = np.asarray(mask, dtype=dtype)
    m = m[None, None, :] if m.ndim == 1 else m[:, None, :]
    return np.broadcast_to(m, x.shape)


def blend32(x, known, mask, coef=None, col_a: int = 0, col_s: int = 1, noise=None) -> np.ndarray:
    """osuf_inpaint_blend on (B, Dch, L) arrays: every product and sum is one np.float32 operation, i.e. one rounding, in the kernel's
    order; the two ends of the mask are selects.  mask (L,) or (B, L); coef (B, ncols) or None."""
    x, known = np.asarray(x, f32), np.asarray(known, f32)
    m = _mask_like(mask, x, f32)
    with np.errstate(all="ignore"):
        if coef is None:
            tgt = known
        else:
            coef = np.asarray(coef, f32)
            tgt = coef[:, col_a][:, None, None] * known
            if noise is not None:
                sz = coef[:, col_s][:, None, None] * np.asarray(noise, f32)
                tgt = tgt + sz
        d = tgt - x
        md = m * d
        mid = x + md
    return np.where(m == 0, x, np.where(m == 1, tgt, mid)).astype(f32)


def blend64(x, known, mask, a=None, s=None, noise=None) -> np.ndarray:
    """The same rule in fp64 at scalar levels (a, s); a None is the exact blend."""
    x, known = np.asarray(x, np.float64), np.asarray(known, np.float64)
    m = _mask_like(mask, x, np.float64)
    tgt = known if a is None else a * known + s * np.asarray(noise, np.float64)
    return np.where(m == 0, x, np.where(m == 1, tgt, x + m * (tgt - x)))


class _Region:
    """known, mask and the noise rule of one loop: `fixed` (the deterministic loops' clone of the start iterate) or draws from `draw`."""

    def __init__(self, known, mask, fixed=None, draw: Optional[Callable[[], np.ndarray]] = None, trace: Optional[List] = None) -> None:
        self.known, self.mask, self.fixed, self.draw, self.trace = known, mask, fixed, draw, trace

    def level(self, x, a, s):
        out = blend64(x, self.known, self.mask, a, s, self.fixed if self.fixed is not None else self.draw())
        if self.trace is not None:
            self.trace.append((float(a), float(s), out.copy()))
        return out

    def exact(self, x):
        return blend64(x, self.known, self.mask)


def ddim_loop(den, x, coefs, known=None, mask=None, total: Optional[int] = None, trace=None) -> np.ndarray:
    """The DDIM loop of models/diffusion.py and DiffusionOsuFusionDiT: den(x, i) -> the noise prediction; coefs (steps, 4) =
    sqrt(1 - a_t), sqrt(a_t), sqrt(a_prev), sqrt(1 - a_prev); total = the steps of a full run (len(coefs) unless the run is cut short).
    trace collects (a, s, iterate) of every level blend, i.e. of every iterate handed to den."""
    x = np.asarray(x, np.float64)
    coefs = np.asarray(coefs, np.float64)
    total = len(coefs) if total is None else total
    reg = _Region(known, mask, fixed=x.copy(), trace=trace) if known is not None else None
    if reg is not None and len(coefs):
        x = reg.level(x, coefs[0][1], coefs[0][0])
    for i, c in enumerate(coefs):
        eps = den(x, i)
        x0 = np.clip((x - c[0] * eps) / c[1], -1.0, 1.0)
        x = c[2] * x0 + c[3] * eps
        if reg is not None:
            x = reg.exact(x) if i == total - 1 else reg.level(x, c[2], c[3])
    return x


def flow_loop(vel, x, times, known=None, mask=None, trace=None) -> np.ndarray:
    """The fixed-grid midpoint loop of both flow samplers: vel(t, y) -> the flow; the state at ODE time t is t x_0 + (1 - t) noise."""
    x = np.asarray(x, np.float64)
    reg = _Region(known, mask, fixed=x.copy(), trace=trace) if known is not None else None
    if reg is not None:
        x = reg.level(x, times[0], 1.0 - times[0])
    last = len(times) - 2
    for j, (t0, t1) in enumerate(zip(times[:-1], times[1:])):
        dt = t1 - t0
        k1 = vel(t0, x)
        mid = x + 0.5 * dt * k1
        if reg is not None:
            tm = t0 + 0.5 * dt
            mid = reg.level(mid, tm, 1.0 - tm)
        k2 = vel(t0 + 0.5 * dt, mid)
        x = x + dt * k2
        if reg is not None:
            x = reg.exact(x) if j == last else reg.level(x, t1, 1.0 - t1)
    return x


def renoise_factors(rows):
    """(k_r, k_g) per step of RePaint's way back from a step's level to the level it left: x = k_r x + k_g z with k_r = alpha / alpha_next and
    k_g = sigma sqrt(c), the exact forward transition (k_r^2 sigma_next^2 + k_g^2 = sigma^2)."""
    rows = np.asarray(rows, np.float64)
    return rows[:, 1] / rows[:, 4], rows[:, 2] * np.sqrt(rows[:, 6])


def ct_loop(den, x, grid, sampler: str, eta: float = 0.0, known=None, mask=None, draw: Optional[Callable[[], np.ndarray]] = None,
            stop_after: Optional[int] = None, resample: int = 1, trace=None, calls: Optional[List] = None) -> np.ndarray:
    """The continuous-time loops of ContinuousDiffusionOsuFusionDiT over a rising log-SNR grid (S + 1,): den(x, i) -> the start prediction
    (objective "x_start"), clamped to [-1, 1]; "ddpm" is the ancestral step on the grid's schedule rows, "ddim" / "dpmpp_2m" the solver
    steps of tests/ct_solver_oracle.py.  draw() -> the next noise array, called in the documented order: (the start blend's), then per
    pass the step's own, the level blend's, the way back's."""
    x = np.asarray(x, np.float64)
    R = SV.rows(grid)
    total = len(R)
    steps = total if stop_after is None else min(stop_after, total)
    fresh = sampler == "ddpm" or (sampler == "ddim" and eta > 0)
    Fc = None if sampler == "ddpm" else SV.factors(grid, sampler, eta)[0]
    k_r, k_g = renoise_factors(R)
    reg = None
    if known is not None:
        reg = _Region(known, mask, fixed=None if fresh else x.copy(), draw=draw, trace=trace)
        if steps:
            x = reg.level(x, R[0][1], R[0][2])
    assert resample == 1 or (sampler == "ddpm" and reg is not None)
    prev = None
    for i in range(steps):
        passes = resample if i < total - 1 else 1
        for u in range(passes):
            x0 = np.clip(den(x, i), -1.0, 1.0)
            if calls is not None:
                calls.append(i)
            if sampler == "ddpm":
                x = R[i][10] * x + R[i][11] * x0
                if i < total - 1:
                    x = x + R[i][12] * draw()
            else:
                k_x, k_0, k_p, gain = Fc[i]
                nxt = k_x * x + k_0 * x0
                if prev is not None and k_p != 0:
                    nxt = nxt + k_p * prev
                if fresh:
                    nxt = nxt + gain * draw()
                x, prev = nxt, x0
            if reg is not None:
                x = reg.exact(x) if i == total - 1 else reg.level(x, R[i][4], R[i][5])
            if u < passes - 1:
                x = k_r[i] * x + k_g[i] * draw()
    return x
