"""Continuous-time Gaussian diffusion on the device (osuf_ct_schedule, osuf_ct_step, csrc/sampling.hip); reached as ops.ct_schedule /
ops.ct_step.  The allocating wrappers live here, as osufusion_amd/gqa.py's does; their guarded-memory cases are in
tests/test_scheduler_gpu.py.  Prediction objectives and dynamic thresholding (osuf_ct_step_ex, osuf_ct_x0_quantile, osuf_ct_qsample;
ops.ct_step_ex / ops.ct_x0_quantile / ops.ct_qsample) follow, guarded in tests/test_ct_objectives_gpu.py; then the DDIM / DPM-Solver++(2M)
solvers on a log-SNR grid (osuf_ct_solver_schedule, osuf_ct_solver_step; ops.ct_solver_schedule / ops.ct_solver_step), guarded in
tests/test_ct_solver_gpu.py."""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch

from . import _lib, ops

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


def _step_args(x, cond, null, noise, coef) -> None:
    for v in (x, cond, null, noise):
        assert v is None or (v.dtype == torch.float32 and v.is_contiguous() and v.shape == x.shape)
    assert coef.dtype == torch.float32 and coef.is_contiguous() and coef.shape == (x.shape[0], COLS)


def ct_step(x: torch.Tensor, cond: torch.Tensor, null: Optional[torch.Tensor], cond_scale: float, coef: torch.Tensor,
            noise: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One ancestral step over (B, ...) fp32 contiguous tensors; coef = ct_schedule(t, t_next, kind), (B, 13)."""
    _step_args(x, cond, null, noise, coef)
    out = torch.empty_like(x)
    ops.call("osuf_ct_step", ops._p(x), ops._p(cond), ops._p(null), float(cond_scale), ops._p(coef), ops._p(noise), ops._p(out),
             x.shape[0], x[0].numel(), ops._stream())
    return out


# what the network predicts (include/osufusion_hip.h: OSUF_CT_OBJ_*)
OBJECTIVES = {name: _lib.CONSTS["OSUF_CT_OBJ_" + name.upper()] for name in ("noise", "x_start", "v")}


def objective_code(objective) -> int:
    if objective in OBJECTIVES:
        return OBJECTIVES[objective]
    if objective in OBJECTIVES.values() and not isinstance(objective, bool):
        return int(objective)
    raise ValueError(f"Unknown prediction objective: {objective!r} (one of {sorted(OBJECTIVES)})")


def quantile_rank(q: float, n: int) -> Tuple[int, float]:
    """(k_lo, frac) of torch.quantile's linear interpolation over n sorted values, in fp64: q (n - 1) = k_lo + frac, 0 <= frac < 1 (q = 1:
    k_lo = n - 1, frac = 0).  The value is v[k_lo] + (v[min(k_lo + 1, n - 1)] - v[k_lo]) frac."""
    q, n = float(q), int(n)
    if not 0.0 <= q <= 1.0:
        raise ValueError(f"quantile must be in [0, 1] (got {q})")
    if n < 1:
        raise ValueError(f"quantile of {n} values")
    pos = q * (n - 1)
    k_lo = min(int(math.floor(pos)), n - 1)
    return k_lo, pos - k_lo


def ct_step_ex(x: torch.Tensor, cond: torch.Tensor, null: Optional[torch.Tensor], cond_scale: float, coef: torch.Tensor,
               noise: Optional[torch.Tensor] = None, objective="noise", s: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ct_step for a noise / x_start / v prediction; s (B,) fp32 (any stride: a column of ct_x0_quantile's rows is read in place) is the
    per-sample dynamic threshold, None the static clamp to [-1, 1]."""
    _step_args(x, cond, null, noise, coef)
    assert s is None or (s.dtype == torch.float32 and s.shape == (x.shape[0],) and s.device == x.device and (s.stride(0) >= 1 or x.shape[0] == 1))
    out = torch.empty_like(x)
    ops.call("osuf_ct_step_ex", ops._p(x), ops._p(cond), ops._p(null), float(cond_scale), ops._p(coef), ops._p(noise), objective_code(objective),
             ops._p(s), max(s.stride(0), 1) if s is not None else 0, ops._p(out), x.shape[0], x[0].numel(), ops._stream())
    return out


def ct_x0_quantile(x: torch.Tensor, cond: torch.Tensor, null: Optional[torch.Tensor], cond_scale: float, coef: torch.Tensor,
                   objective="noise", q: float = 0.95) -> torch.Tensor:
    """-> (B, 3) fp32 = per sample the two order statistics of |x0| that bracket its q-quantile (exact) and s = max(1, the quantile);
    x0 = the unclamped start prediction of ct_step_ex on the same arguments."""
    _step_args(x, cond, null, None, coef)
    B, n = x.shape[0], x[0].numel()
    k_lo, frac = quantile_rank(q, n)
    out = torch.empty((B, 3), dtype=torch.float32, device=x.device)
    ws = torch.empty(_lib.load().osuf_ct_x0_quantile_workspace_bytes(B) // 4, dtype=torch.int32, device=x.device)
    ops.call("osuf_ct_x0_quantile", ops._p(x), ops._p(cond), ops._p(null), float(cond_scale), ops._p(coef), objective_code(objective), k_lo,
             frac, ops._p(out), ops._p(ws), B, n, ops._stream())
    return out


# solvers on a log-SNR grid (include/osufusion_hip.h: OSUF_CT_SAMPLER_*); "ddpm" is the ancestral path and has no code here
SAMPLERS = {name: _lib.CONSTS["OSUF_CT_SAMPLER_" + name.upper()] for name in ("ddim", "dpmpp_2m")}
FAC_K_X, FAC_K_0, FAC_K_P, FAC_GAIN = range(4)


def sampler_code(sampler) -> int:
    if sampler in SAMPLERS:
        return SAMPLERS[sampler]
    if sampler in SAMPLERS.values() and not isinstance(sampler, bool):
        return int(sampler)
    raise ValueError(f"Unknown solver: {sampler!r} (one of {sorted(SAMPLERS)})")


def ct_solver_schedule(log_snr: torch.Tensor, sampler="dpmpp_2m", eta: float = 0.0, batch: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
    """log_snr (S + 1,) fp32, rising -> (rows (S, batch, 13) fp32: step i's schedule row, once per sample, rows[i] being the coef of
    ct_x0_quantile / ct_solver_step; fac (S, 4) fp32 = k_x, k_0, k_p, gain of x_next = k_x x + k_0 x0 + k_p x0_prev + gain z).  One launch, no
    host sync."""
    assert log_snr.dim() == 1 and log_snr.shape[0] >= 2, "the grid is S + 1 log-SNR values"
    if not 0.0 <= float(eta) <= 1.0:
        raise ValueError(f"eta must be in [0, 1] (got {eta})")
    code = sampler_code(sampler)
    log_snr = log_snr.float().contiguous()
    steps, batch = log_snr.shape[0] - 1, int(batch)
    assert batch >= 1
    rows = torch.empty((steps, batch, COLS), dtype=torch.float32, device=log_snr.device)
    fac = torch.empty((steps, 4), dtype=torch.float32, device=log_snr.device)
    ops.call("osuf_ct_solver_schedule", ops._p(log_snr), steps, code, float(eta), ops._p(rows), ops._p(fac), batch, ops._stream())
    return rows, fac


def ct_solver_step(x: torch.Tensor, cond: torch.Tensor, null: Optional[torch.Tensor], cond_scale: float, coef: torch.Tensor, fac: torch.Tensor,
                   x0_prev: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None, objective="noise",
                   s: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """One DDIM / DPM-Solver++(2M) step over (B, ...) fp32 contiguous tensors -> (x_next, x0): coef (B, 13) and fac (4,) = rows[i] and fac[i]
    of ct_solver_schedule; x0 is the clamped (s None) or thresholded start prediction, the x0_prev of the next 2M step.  x0_prev is read
    only when fac's k_p is non-zero, noise only when its gain is."""
    _step_args(x, cond, null, noise, coef)
    assert x0_prev is None or (x0_prev.dtype == torch.float32 and x0_prev.is_contiguous() and x0_prev.shape == x.shape)
    assert fac.dtype == torch.float32 and fac.is_contiguous() and fac.shape == (4,) and fac.device == x.device
    assert s is None or (s.dtype == torch.float32 and s.shape == (x.shape[0],) and s.device == x.device and (s.stride(0) >= 1 or x.shape[0] == 1))
    x_next, x0 = torch.empty_like(x), torch.empty_like(x)
    ops.call("osuf_ct_solver_step", ops._p(x), ops._p(cond), ops._p(null), float(cond_scale), ops._p(coef), ops._p(fac), ops._p(x0_prev),
             ops._p(noise), objective_code(objective), ops._p(s), max(s.stride(0), 1) if s is not None else 0, ops._p(x_next), ops._p(x0),
             x.shape[0], x[0].numel(), ops._stream())
    return x_next, x0


def ct_qsample(x_0: torch.Tensor, noise: torch.Tensor, sched: torch.Tensor, objective="noise",
               want_target: bool = True) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """-> (alpha x_0 + sigma noise, the objective's training target: noise, x_0 or v = alpha noise - sigma x_0), one pass; sched = ct_schedule's
    rows at the samples' times, (B, 3) or (B, 13)."""
    assert x_0.dtype == torch.float32 and x_0.is_contiguous() and noise.dtype == torch.float32 and noise.is_contiguous() and noise.shape == x_0.shape
    assert sched.dtype == torch.float32 and sched.is_contiguous() and sched.dim() == 2 and sched.shape[0] == x_0.shape[0] and sched.shape[1] in (COLS_T, COLS)
    x_t = torch.empty_like(x_0)
    target = torch.empty_like(x_0) if want_target else None
    ops.call("osuf_ct_qsample", ops._p(x_0), ops._p(noise), ops._p(sched), sched.shape[1], objective_code(objective), ops._p(x_t), ops._p(target),
             x_0.shape[0], x_0[0].numel(), ops._stream())
    return x_t, target
