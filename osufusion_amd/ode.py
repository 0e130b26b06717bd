"""ODE solvers of the rectified-flow samplers: the reference's ``odeint(ode_fn, x, times, method=..., rtol=..., atol=...)`` with the method
and the tolerances honoured.  Fixed-grid Euler, midpoint and RK4 (the 3/8 rule) over the sampler's grid, and the adaptive embedded pairs
Bogacki-Shampine 3(2) ("bosh3") and Dormand-Prince 5(4) ("dopri5") with torchdiffeq's step controller.

This module is host policy: tableaus as plain data, the controller, the clipping of the last step and the loops.  It imports and tests without
a GPU.  The work on the device is three things: the flow function f(t, y) the sampler passes in (a full denoiser call; guidance, windows and
masks live inside it), ops.lincomb for every stage state and solution (y + dt sum_j w_j k_j as one fp64 fma chain rounded once, zero weights
skipped) and ops.rk_error (osuf_rk_error, csrc/sampling.hip) for the per-sample scaled error norm; its allocating wrapper is here.

Synchronisation: an adaptive loop reads B doubles (the per-sample ratios) from the device once per attempted step -- the step size is a host
decision -- and that is its only synchronisation.  The fixed-grid loops have none.

torchdiffeq is not installed where this was written: the tableaus are the published ones (checked against their order conditions in exact
rationals, tests/test_ode_cpu.py) and the controller restates torchdiffeq 0.2.4's rule from its documentation, but parity with torchdiffeq
itself -- its fixed-grid "rk4" is, to our recollection, the 3/8 rule used here -- is unpinned.

Not covered: adaptive methods with a known region (a blend between steps invalidates the reused first-same-as-last stage and the error
estimate: ValueError), per-sample step sizes (one step size serves the batch: the largest per-sample ratio decides), dense output (only
the state at the last time is returned) and hipGraph capture of an adaptive loop (its length is decided on the host)."""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass
from fractions import Fraction as Fr
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib, inpaint, ops


@dataclass(frozen=True)
class Tableau:
    """An explicit Runge-Kutta method in exact rationals: stage i is f(t + c[i] dt, y + dt sum_j a[i][j] k_j), the solution
    y + dt sum_j b[j] k_j.  b_star: the embedded lower-order weights of an adaptive pair (None: fixed grid); order: the order of b, which is
    also the controller's exponent.  Both pairs are first-same-as-last: the last row of a is b, so the last stage state is the solution and
    its derivative is the next step's first stage."""
    name: str
    c: Tuple[Fr, ...]
    a: Tuple[Tuple[Fr, ...], ...]
    b: Tuple[Fr, ...]
    order: int
    b_star: Optional[Tuple[Fr, ...]] = None

    @property
    def stages(self) -> int:
        return len(self.b)

    @property
    def adaptive(self) -> bool:
        return self.b_star is not None

    @property
    def e(self) -> Tuple[Fr, ...]:
        """The error weights b_j - b*_j."""
        return tuple(x - y for x, y in zip(self.b, self.b_star))

    def floats(self) -> "Coefficients":
        return Coefficients([float(v) for v in self.c], [[float(v) for v in row] for row in self.a], [float(v) for v in self.b],
                            [float(v) for v in self.e] if self.adaptive else None)


@dataclass(frozen=True)
class Coefficients:
    """A tableau as python floats, each the correctly rounded value of its rational."""
    c: List[float]
    a: List[List[float]]
    b: List[float]
    e: Optional[List[float]]


def _rows(*rows) -> Tuple[Tuple[Fr, ...], ...]:
    return tuple(tuple(Fr(v) for v in row) for row in rows)


def _vec(*vals) -> Tuple[Fr, ...]:
    return tuple(Fr(v) for v in vals)


TABLEAUS: Dict[str, Tableau] = {
    "euler": Tableau("euler", _vec(0), _rows(()), _vec(1), 1),
    "midpoint": Tableau("midpoint", _vec(0, "1/2"), _rows((), ("1/2",)), _vec(0, 1), 2),
    "rk4": Tableau("rk4", _vec(0, "1/3", "2/3", 1), _rows((), ("1/3",), ("-1/3", 1), (1, -1, 1)), _vec("1/8", "3/8", "3/8", "1/8"), 4),
    "bosh3": Tableau("bosh3", _vec(0, "1/2", "3/4", 1), _rows((), ("1/2",), (0, "3/4"), ("2/9", "1/3", "4/9")),
                     _vec("2/9", "1/3", "4/9", 0), 3, _vec("7/24", "1/4", "1/3", "1/8")),
    "dopri5": Tableau("dopri5", _vec(0, "1/5", "3/10", "4/5", "8/9", 1, 1),
                      _rows((), ("1/5",), ("3/40", "9/40"), ("44/45", "-56/15", "32/9"),
                            ("19372/6561", "-25360/2187", "64448/6561", "-212/729"),
                            ("9017/3168", "-355/33", "46732/5247", "49/176", "-5103/18656"),
                            ("35/384", 0, "500/1113", "125/192", "-2187/6784", "11/84")),
                      _vec("35/384", 0, "500/1113", "125/192", "-2187/6784", "11/84", 0), 5,
                      _vec("5179/57600", 0, "7571/16695", "393/640", "-92097/339200", "187/2100", "1/40")),
}
METHODS = tuple(TABLEAUS)
SAFETY, MAX_FACTOR, REJECT_FACTOR = 0.9, 10.0, 0.2


# ---- the step controller (torchdiffeq's rule) ----------------------------------------------------------------------------------------------------
def batch_ratio(ratios: Sequence[float]) -> float:
    """One ratio for the batch: the largest per-sample ratio (for B = 1 torchdiffeq's RMS norm); NaN if any sample's is not finite."""
    ratios = [float(r) for r in ratios]
    return max(ratios) if all(math.isfinite(r) for r in ratios) else math.nan


def step_factor(ratio: float, order: int) -> Tuple[bool, float]:
    """(accepted, factor): the step is accepted when ratio <= 1 and the next attempt's step is factor times this one's.
    factor = min(10, max(0.9 ratio^(-1 / order), dfactor)), dfactor = 1 after an accepted step and 0.2 after a rejected one; 10 where
    ratio == 0.  A ratio that is not finite is a rejection with factor 0.2."""
    if not math.isfinite(ratio):
        return False, REJECT_FACTOR
    accepted = ratio <= 1.0
    if ratio == 0.0:
        return True, MAX_FACTOR
    dfactor = 1.0 if accepted else REJECT_FACTOR
    return accepted, min(MAX_FACTOR, max(SAFETY * ratio ** (-1.0 / order), dfactor))


def clip_step(t: float, dt: float, t_end: float) -> Tuple[float, float]:
    """(end of the step, its length): a step that would reach or pass t_end ends exactly there, as a select (t + (t_end - t) need not
    round to t_end)."""
    if t + dt >= t_end:
        return t_end, t_end - t
    return t + dt, dt


def check_options(method: str, rtol: float, atol: float, first_step: Optional[float], max_steps: int) -> Tableau:
    if method not in TABLEAUS:
        raise ValueError(f"method must be one of {METHODS} (got {method!r})")
    tab = TABLEAUS[method]
    if tab.adaptive:
        rtol, atol = float(rtol), float(atol)
        if not (math.isfinite(rtol) and math.isfinite(atol) and rtol >= 0.0 and atol >= 0.0 and (rtol > 0.0 or atol > 0.0)):
            raise ValueError(f"rtol and atol must be finite, not negative and not both zero (got rtol={rtol}, atol={atol})")
        if first_step is not None and not (math.isfinite(float(first_step)) and float(first_step) > 0.0):
            raise ValueError(f"first_step must be positive and finite or None (got {first_step})")
        if int(max_steps) < 1:
            raise ValueError(f"max_steps must be at least 1 (got {max_steps})")
    return tab


# ---- the device side -------------------------------------------------------------------------------------------------------------------------------
def rk_error(y0: torch.Tensor, y1: torch.Tensor, ks, e, dt: float, atol: float, rtol: float) -> torch.Tensor:
    """y0, y1 (B, ...) fp32 contiguous, ks the stage derivatives of that shape (None allowed under a zero weight), e the error weights
    -> ratio (B,) fp64 (osuf_rk_error, include/osufusion_hip.h).  Two launches, no atomics, no synchronisation; the workspace is a torch.empty
    per call, served by the caching allocator as cfg_rescale's is."""
    S = len(ks)
    assert S == len(e) and 1 <= S <= 7
    for v in [y0, y1] + [k for k in ks if k is not None]:
        assert v.dtype == torch.float32 and v.is_contiguous() and v.shape == y0.shape and v.device == y0.device and v.is_cuda
    B, n = y0.shape[0], y0[0].numel()
    ratio = torch.empty((B,), dtype=torch.float64, device=y0.device)
    ws = torch.empty(_lib.load().osuf_rk_error_workspace_bytes(B, n) // 8, dtype=torch.float64, device=y0.device)
    ptrs = (ctypes.c_void_p * S)(*[None if k is None else k.data_ptr() for k in ks])
    we = (ctypes.c_double * S)(*[float(w) for w in e])
    step = (ctypes.c_double * 3)(float(dt), float(atol), float(rtol))
    ops.call("osuf_rk_error", ops._p(y0), ops._p(y1), ctypes.cast(ptrs, ctypes.c_void_p), ctypes.cast(we, ctypes.c_void_p), S,
             ctypes.cast(step, ctypes.c_void_p), ops._p(ws), ops._p(ratio), B, n, ops._stream())
    return ratio


def _combine(y: torch.Tensor, ks: List[torch.Tensor], weights: Sequence[float], dt: float) -> torch.Tensor:
    """y + dt sum_j weights[j] ks[j]: one ops.lincomb, an fp64 fma chain rounded to fp32 once."""
    out = torch.empty_like(y)
    ops.lincomb([y] + ks[:len(weights)], [1.0] + [dt * w for w in weights], out=out)
    return out


def _levels(ts: Sequence[float], b: int, device) -> torch.Tensor:
    """(len(ts), b, 2) fp32 = (t, 1 - t) per sample: the levels a masked loop blends at; t and 1 - t are python floats rounded to fp32."""
    return torch.tensor([[[t, 1.0 - t]] * b for t in ts], dtype=torch.float32, device=device)


def flow_levels(times, b: int, device) -> torch.Tensor:
    """The levels a masked midpoint loop over `times` blends at, (1 + 2 (S - 1), b, 2): row 0 the start (times[0]), then per interval its
    midpoint t0 + dt / 2 and its end t1.  Built once per call."""
    ts = [times[0]]
    for t0, t1 in zip(times[:-1], times[1:]):
        ts += [t0 + 0.5 * (t1 - t0), t1]
    return _levels(ts, b, device)


def midpoint_loop(f, x: torch.Tensor, times, ones: torch.Tensor, keep_region=None) -> torch.Tensor:
    """The reference's sampler, torchdiffeq==0.2.4's fixed-grid ``odeint(..., method="midpoint")`` restated: per interval of `times`
    ``k1 = f(t0, y); k2 = f(t0 + dt/2, y + dt/2 * k1); y += dt * k2``, each update one ops.axpby_rows (its own rounding, which is why this is
    not fixed_grid_loop over the midpoint tableau: ops.lincomb rounds differently).  keep_region = (known, known_mask): every state
    handed to f is blended at its own time, the end of the last interval exactly; None issues the unmasked loop's launches and nothing else."""
    blender = None
    if keep_region is not None:
        blender = inpaint.Blender(*keep_region, x, fresh=False)
        levels = flow_levels(times, x.shape[0], x.device)
        x = blender.level(x, levels[0], 0, 1)
    last = len(times) - 2
    for j, (t0, t1) in enumerate(zip(times[:-1], times[1:])):
        dt = t1 - t0
        k1 = f(t0, x)
        mid = ops.axpby_rows(x, k1, ones, ones * (0.5 * dt))
        if blender is not None:
            mid = blender.level(mid, levels[1 + 2 * j], 0, 1)
        k2 = f(t0 + 0.5 * dt, mid)
        x = ops.axpby_rows(x, k2, ones, ones * dt)
        if blender is not None:
            x = blender.exact(x) if j == last else blender.level(x, levels[2 + 2 * j], 0, 1)
    return x


def fixed_grid_loop(f: Callable, x: torch.Tensor, times: Sequence[float], tab: Tableau, keep_region=None) -> torch.Tensor:
    """One step of `tab` per interval of `times`.  keep_region = (known, known_mask): every state handed to f is blended at its own time
    t0 + c_i dt, the end of an interval at t1 and the end of the last interval exactly, as midpoint_loop does."""
    co = tab.floats()
    blender = None
    if keep_region is not None:
        blender = inpaint.Blender(*keep_region, x, fresh=False)
        ts = [times[0]]
        for t0, t1 in zip(times[:-1], times[1:]):
            ts += [t0 + c * (t1 - t0) for c in co.c[1:]] + [t1]
        levels = _levels(ts, x.shape[0], x.device)
        x = blender.level(x, levels[0], 0, 1)
    per, last = tab.stages, len(times) - 2                 # levels per interval: stages - 1 stage states and the end
    for j, (t0, t1) in enumerate(zip(times[:-1], times[1:])):
        dt = t1 - t0
        ks = [f(t0, x)]
        for i in range(1, tab.stages):
            yi = _combine(x, ks, co.a[i], dt)
            if blender is not None:
                yi = blender.level(yi, levels[per * j + i], 0, 1)
            ks.append(f(t0 + co.c[i] * dt, yi))
        x = _combine(x, ks, co.b, dt)
        if blender is not None:
            x = blender.exact(x) if j == last else blender.level(x, levels[per * (j + 1)], 0, 1)
    return x


def adaptive_loop(f: Callable, x: torch.Tensor, t0: float, t_end: float, tab: Tableau, rtol: float, atol: float, first_step: float,
                  max_steps: int, stats: dict) -> torch.Tensor:
    """The embedded pair `tab` from t0 to t_end, one step size for the batch.  Per attempted step: stages - 1 evaluations of f (the first
    stage is the last one of the step before: first-same-as-last), one ops.rk_error, one read of B doubles."""
    co = tab.floats()
    t, dt = float(t0), float(first_step)
    k1 = f(t, x)
    attempts = 0
    while t < t_end:
        attempts += 1
        if attempts > max_steps:
            raise RuntimeError(f"{tab.name}: more than max_steps = {max_steps} attempted steps (t = {t}, dt = {dt}, rtol = {rtol}, atol = {atol})")
        t_new, h = clip_step(t, dt, t_end)
        ks = [k1]
        for i in range(1, tab.stages):
            y1 = _combine(x, ks, co.a[i], h)                # the last row of a is b: the last stage state is the solution
            ks.append(f(t_new if i == tab.stages - 1 else t + co.c[i] * h, y1))
        ratio = batch_ratio(rk_error(x, y1, ks, co.e, h, atol, rtol).tolist())
        accepted, factor = step_factor(ratio, tab.order)
        if accepted:
            t, x, k1 = t_new, y1, ks[-1]
            stats["accepted"] += 1
            stats["times"].append(t)
        else:
            stats["rejected"] += 1
        dt = h * factor
    return x


def ode_loop(f: Callable, x: torch.Tensor, times: Sequence[float], ones: torch.Tensor, method: str = "midpoint", rtol: float = 1e-5,
             atol: float = 1e-5, first_step: Optional[float] = None, max_steps: int = 1000, keep_region=None) -> Tuple[torch.Tensor, dict]:
    """The flow f(t, y) integrated over `times` (the sampler's linspace(0, 1, S)) -> (the state at times[-1], stats).  stats: evals (calls
    of f), accepted, rejected, times (the ends of the accepted steps).  "midpoint" is midpoint_loop itself, launches and
    bits unchanged; "euler" and "rk4" step once per interval of the grid and ignore the tolerances, as torchdiffeq's fixed-grid solvers do;
    "bosh3" and "dopri5" choose their own steps from rtol / atol, starting at first_step (None: the grid's first interval) and ending
    exactly at times[-1].  keep_region with an adaptive method: ValueError (see the module docstring).  RuntimeError after max_steps
    attempted steps."""
    tab = check_options(method, rtol, atol, first_step, max_steps)
    if tab.adaptive and keep_region is not None:
        raise ValueError(f"method={method!r} does not take known / known_mask: a blend between steps invalidates the reused stage and the "
                         "error estimate; use a fixed-grid method (euler, midpoint, rk4)")
    stats = {"method": method, "evals": 0, "accepted": 0, "rejected": 0, "times": []}

    def counted(t, y):
        stats["evals"] += 1
        return f(t, y)
    if not tab.adaptive:
        x = midpoint_loop(counted, x, times, ones, keep_region) if method == "midpoint" else fixed_grid_loop(counted, x, times, tab, keep_region)
        stats["accepted"], stats["times"] = len(times) - 1, list(times[1:])
        return x, stats
    if len(times) < 2:                                     # a one-point grid: nothing to integrate, as the fixed-grid loops find
        return x, stats
    first = times[1] - times[0] if first_step is None else float(first_step)
    x = adaptive_loop(counted, x, times[0], times[-1], tab, float(rtol), float(atol), first, int(max_steps), stats)
    return x, stats
