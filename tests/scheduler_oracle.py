"""A restatement of the continuous-time Gaussian diffusion schedule (modules/scheduler.py of the reference) in plain torch, in the
precision asked for: fp32 in the reference's order of operations (what tests/golden/scheduler_cases.npz records and what the network is
conditioned on) and fp64 (the yardstick of the elementwise kernels).  A helper module, imported by tests/test_scheduler_*.py.

`nudge` moves the one intermediate whose rounding a different libm may change -- cos(.) of the cosine schedule, expm1(.) of the linear
one -- by that many ulps (torch.nextafter); perturbation_bound() turns it into the tolerance of a comparison across two libms."""
from __future__ import annotations

import math
from typing import Callable, Dict, Optional

import torch

SCHEDULES = ("linear", "cosine")
GOLDEN_TIMES = (0.0, 1e-3, 0.25, 0.5, 0.999, 1.0)
COLUMNS = ("log_snr", "alpha", "sigma", "log_snr_next", "alpha_next", "sigma_next", "c", "posterior_variance", "posterior_log_variance",
           "inv_alpha", "k_x", "k_x0", "noise_gain")                      # the row of osuf_ct_schedule, in its order


def _nudged(v: torch.Tensor, k: int) -> torch.Tensor:
    toward = torch.full_like(v, math.inf if k > 0 else -math.inf)
    for _ in range(abs(k)):
        v = torch.nextafter(v, toward)
    return v


def _fn(f: Callable[[torch.Tensor], torch.Tensor], x: torch.Tensor) -> torch.Tensor:
    """A function of x in x's precision.  For fp32 it is evaluated in fp64 and rounded once, i.e. correctly rounded: torch's own fp32
    cos / log / exp / expm1 -- and its fp32 sqrt on AVX-512 hosts -- are vector routines whose last bit depends on the CPU they run on,
    and a restatement that moved with the machine could not be held against a recording.  (+, -, *, / are IEEE everywhere.)"""
    return f(x.double()).to(x.dtype)


def _sigmoid(x: torch.Tensor) -> torch.Tensor:
    return 1 / (1 + _fn(torch.exp, -x))                                   # as torch evaluates sigmoid on fp32 tensors


def log_snr(t: torch.Tensor, schedule: str, dtype: torch.dtype = torch.float32, nudge: int = 0) -> torch.Tensor:
    t = t.to(dtype)
    if schedule == "linear":
        return -_fn(torch.log, _nudged(_fn(torch.expm1, 1e-4 + 10 * (t ** 2)), nudge))
    if schedule == "cosine":
        s = 0.008
        res = (_nudged(_fn(torch.cos, (t + s) / (1 + s) * math.pi * 0.5), nudge) ** -2) - 1
        return -_fn(torch.log, res.clamp(min=1e-8))
    raise ValueError(f"Unknown noise schedule: {schedule}")


def alpha_sigma(ls: torch.Tensor):
    return _fn(torch.sqrt, _sigmoid(ls)), _fn(torch.sqrt, _sigmoid(-ls))


def schedule_row(t: torch.Tensor, t_next: Optional[torch.Tensor], schedule: str, dtype: torch.dtype = torch.float32, nudge: int = 0,
                 nudge_next: int = 0) -> Dict[str, torch.Tensor]:
    """Every column of osuf_ct_schedule, by name.  Columns 0-8 are the reference's q_posterior intermediates; 9-12 fold them for the step."""
    ls = log_snr(t, schedule, dtype, nudge)
    alpha, sigma = alpha_sigma(ls)
    row = dict(log_snr=ls, alpha=alpha, sigma=sigma)
    if t_next is None:
        return row
    lsn = log_snr(t_next, schedule, dtype, nudge_next)
    alpha_n, sigma_n = alpha_sigma(lsn)
    c = -_fn(torch.expm1, ls - lsn)
    var = (sigma_n ** 2) * c
    logvar = _fn(torch.log, var.clamp(min=1e-20))
    gain = torch.where(t_next.to(dtype) > 0, _fn(torch.exp, 0.5 * logvar), torch.zeros_like(logvar))
    row.update(log_snr_next=lsn, alpha_next=alpha_n, sigma_next=sigma_n, c=c, posterior_variance=var, posterior_log_variance=logvar,
               inv_alpha=1.0 / alpha.clamp(min=1e-8), k_x=alpha_n * ((1 - c) / alpha), k_x0=alpha_n * c, noise_gain=gain)
    return row


def _pad(x: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    return v.reshape(v.shape + (1,) * (x.dim() - v.dim()))


def q_sample(x_0, t, noise, schedule, dtype=torch.float32, nudge=0):
    ls = log_snr(t, schedule, dtype, nudge)
    alpha, sigma = alpha_sigma(_pad(x_0, ls))
    return alpha * x_0.to(dtype) + sigma * noise.to(dtype), ls, alpha, sigma


def predict_start_from_noise(x_t, t, noise, schedule, dtype=torch.float32, nudge=0):
    alpha, sigma = alpha_sigma(_pad(x_t, log_snr(t, schedule, dtype, nudge)))
    return (x_t.to(dtype) - sigma * noise.to(dtype)) / alpha.clamp(min=1e-8)


def q_posterior(x_0, x_t, t, t_next, schedule, dtype=torch.float32, nudge=0, nudge_next=0):
    ls = _pad(x_t, log_snr(t, schedule, dtype, nudge))
    lsn = _pad(x_t, log_snr(t_next, schedule, dtype, nudge_next))
    alpha, _ = alpha_sigma(ls)
    alpha_n, sigma_n = alpha_sigma(lsn)
    c = -_fn(torch.expm1, ls - lsn)
    mean = alpha_n * (x_t.to(dtype) * (1 - c) / alpha + c * x_0.to(dtype))
    var = (sigma_n ** 2) * c
    return mean, var, _fn(torch.log, var.clamp(min=1e-20))


def sampling_timesteps(timesteps: int, batch_size: int) -> torch.Tensor:
    """get_sampling_timesteps stacked: (timesteps, 2, B) fp32."""
    times = torch.linspace(1.0, 0.0, timesteps + 1, dtype=torch.float32)[None, :].expand(batch_size, -1)
    return torch.stack((times[:, :-1], times[:, 1:]), dim=0).permute(2, 0, 1).contiguous()


def ct_step(x, cond, null, cond_scale, row, noise, dtype=torch.float64):
    """osuf_ct_step's formula on a coefficient row (B, 13) as given (the kernel's fp32 row, or schedule_row's columns stacked), in `dtype`.
    -> (out, the largest |term| per element of the sums it forms)."""
    k = [_pad(x, row[:, i].to(dtype)) for i in range(13)]
    x, cond = x.to(dtype), cond.to(dtype)
    eps = cond if null is None else null.to(dtype) + (cond - null.to(dtype)) * cond_scale
    raw = (x - k[2] * eps) * k[9]
    x0 = raw.clamp(-1, 1)
    out = k[10] * x + k[11] * x0
    terms = [x.abs(), eps.abs(), (k[2] * eps).abs(), raw.abs(), (k[10] * x).abs(), (k[11] * x0).abs(), out.abs()]
    if null is not None:
        terms += [null.abs().to(dtype), ((cond - null.to(dtype)) * cond_scale).abs()]
    if noise is not None:
        add = torch.where(k[12] != 0, k[12] * noise.to(dtype), torch.zeros_like(out))
        out = out + add
        terms += [add.abs(), out.abs()]
    return out, torch.stack([t.expand_as(out) for t in terms]).amax(0), (raw.abs() > 1)


def stack_row(row: Dict[str, torch.Tensor]) -> torch.Tensor:
    return torch.stack([row[k] for k in COLUMNS if k in row], dim=-1)


def perturbation_bound(fn: Callable[..., torch.Tensor], two_times: bool) -> torch.Tensor:
    """|fn(nudge...) - fn(0...)| elementwise, the largest over the intermediate moved by +-2 ulps (at t, at t_next, or both)."""
    base = fn(0, 0) if two_times else fn(0)
    moves = [(a, b) for a in (-2, 0, 2) for b in (-2, 0, 2) if (a, b) != (0, 0)] if two_times else [(-2,), (2,)]
    bound = torch.zeros_like(base)
    for m in moves:
        bound = torch.maximum(bound, (fn(*m) - base).abs())
    return bound
