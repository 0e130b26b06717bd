"""fp64 numpy restatement of osufusion_amd/ode.py's loops for any f(t, y) (a plain helper module, imported by tests/test_ode_cpu.py and
tests/test_ode_gpu.py).  It shares the policy with the code under test -- the tableaus (ode.TABLEAUS), the controller (ode.step_factor,
ode.batch_ratio) and the clipping of the last step (ode.clip_step), which tests/test_ode_cpu.py checks against rationals and hand-computed
values -- and restates the arithmetic: stage states, the solution, the error norm (osuf_rk_error as include/osufusion_hip.h states it) and the
toy problem with its closed form."""
import math

import numpy as np

from osufusion_amd import ode


def error_ratio(y0, y1, ks, e, dt, atol, rtol):
    """(B,) fp64: sqrt(mean_i ((dt sum_j e_j k_j) / (atol + rtol max(|y0|, |y1|)))^2) per sample; a stage under a zero weight is not read
    and a term whose error is exactly 0 is 0."""
    B = y0.shape[0]
    y0, y1 = y0.reshape(B, -1).astype(np.float64), y1.reshape(B, -1).astype(np.float64)
    a = np.zeros_like(y0)
    for w, k in zip(e, ks):
        if w != 0.0:
            a = a + w * k.reshape(B, -1).astype(np.float64)
    err = dt * a
    with np.errstate(all="ignore"):
        m0, m1 = np.abs(y0), np.abs(y1)
        tol = atol + rtol * np.where((m0 > m1) | np.isnan(m0), m0, m1)
        term = np.where(err == 0.0, 0.0, (err / tol) ** 2)
        return np.sqrt(term.sum(axis=1) / y0.shape[1])


def _combine(y, ks, weights, dt):
    out = y.copy()
    for w, k in zip(weights, ks):
        if w != 0.0:
            out = out + (dt * w) * k
    return out


def fixed_grid(f, y, times, method):
    """One step of `method` per interval of `times` -> (y at times[-1], stats)."""
    tab = ode.TABLEAUS[method]
    co = tab.floats()
    y = np.asarray(y, dtype=np.float64)
    evals = 0
    for t0, t1 in zip(times[:-1], times[1:]):
        dt = t1 - t0
        ks = [f(t0, y)]
        for i in range(1, tab.stages):
            ks.append(f(t0 + co.c[i] * dt, _combine(y, ks, co.a[i], dt)))
        evals += tab.stages
        y = _combine(y, ks, co.b, dt)
    return y, {"evals": evals, "accepted": len(times) - 1, "rejected": 0, "times": list(times[1:])}


def adaptive(f, y, t0, t_end, method, rtol, atol, first_step, max_steps=1000):
    """The embedded pair from t0 to t_end -> (y, stats); stats also holds every attempted step's batch ratio (`ratios`) and its decision
    (`decisions`, True = accepted), in order."""
    tab = ode.TABLEAUS[method]
    co = tab.floats()
    y = np.asarray(y, dtype=np.float64)
    t, dt = float(t0), float(first_step)
    stats = {"evals": 1, "accepted": 0, "rejected": 0, "times": [], "ratios": [], "decisions": []}
    k1 = f(t, y)
    while t < t_end:
        if len(stats["decisions"]) >= max_steps:
            raise RuntimeError("max_steps")
        t_new, h = ode.clip_step(t, dt, t_end)
        ks = [k1]
        for i in range(1, tab.stages):
            y1 = _combine(y, ks, co.a[i], h)
            ks.append(f(t_new if i == tab.stages - 1 else t + co.c[i] * h, y1))
        stats["evals"] += tab.stages - 1
        ratio = ode.batch_ratio(error_ratio(y, y1, ks, co.e, h, atol, rtol).tolist())
        accepted, factor = ode.step_factor(ratio, tab.order)
        stats["ratios"].append(ratio)
        stats["decisions"].append(accepted)
        if accepted:
            t, y, k1 = t_new, y1, ks[-1]
            stats["accepted"] += 1
            stats["times"].append(t)
        else:
            stats["rejected"] += 1
        dt = h * factor
    return y, stats


def solve(f, y, times, method, rtol=1e-5, atol=1e-5, first_step=None, max_steps=1000):
    if ode.TABLEAUS[method].adaptive:
        return adaptive(f, y, times[0], times[-1], method, rtol, atol, times[1] - times[0] if first_step is None else first_step, max_steps)
    return fixed_grid(f, y, times, method)


# ---- the toy problem: y' = omega J y on channel pairs (2c, 2c + 1), a rotation by omega t ------------------------------------------------------
def rotation_f(omega):
    def f(t, y):
        k = np.empty_like(y)
        k[:, 0::2] = -omega * y[:, 1::2]
        k[:, 1::2] = omega * y[:, 0::2]
        return k
    return f


def rotation_exact(y0, omega, t):
    y0 = np.asarray(y0, dtype=np.float64)
    out = np.empty_like(y0)
    c, s = math.cos(omega * t), math.sin(omega * t)
    out[:, 0::2] = c * y0[:, 0::2] - s * y0[:, 1::2]
    out[:, 1::2] = s * y0[:, 0::2] + c * y0[:, 1::2]
    return out


def linspace(steps):
    """The sampler's grid: torch.linspace(0, 1, steps) in fp32, as python floats."""
    import torch
    return torch.linspace(0.0, 1.0, steps).tolist()
