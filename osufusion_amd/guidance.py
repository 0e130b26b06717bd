"""Control of classifier-free guidance in the transformer samplers: the guidance interval (Kynkaanniemi et al. 2024: guide only while the
noise level lies in a band of log-SNR) and the CFG rescale (Lin et al. 2024, sec. 3.4: osuf_cfg_rescale, csrc/sampling.hip; reached as
ops.cfg_rescale).  The allocating wrapper lives here, as osufusion_amd/windowed.py's do; its guarded-memory cases are in
tests/test_guidance_gpu.py.  Everything but cfg_rescale is host arithmetic on python floats: the per-call log-SNR of each loop and the
guided / unguided decision, made once per sample() call, before the loop."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import torch

from . import _lib, ops


@dataclass(frozen=True)
class Guidance:
    """What sample()'s guidance_rescale / guidance_interval ask for.  bounded: an interval was given (the decision list is needed)."""
    phi: float = 0.0
    lo: float = -math.inf
    hi: float = math.inf
    bounded: bool = False

    def contains(self, log_snr: float) -> bool:
        return self.lo <= log_snr <= self.hi


def check_phi(phi) -> float:
    phi = float(phi)
    if not 0.0 <= phi <= 1.0:                               # a NaN fails both comparisons
        raise ValueError(f"guidance_rescale must be in [0, 1] (got {phi})")
    return phi


def plan(guidance_rescale=0.0, guidance_interval=None) -> Optional[Guidance]:
    """The two keywords checked -> None at their defaults (the sampler's loop then runs as it did before them), else a Guidance.
    guidance_interval = (lo, hi) in log-SNR, both ends inclusive, None at an end = unbounded.  ValueError: phi outside [0, 1]; an interval
    that is not a pair; lo > hi; a NaN end."""
    phi = check_phi(guidance_rescale)
    if guidance_interval is None:
        return Guidance(phi) if phi > 0.0 else None
    if isinstance(guidance_interval, (str, bytes)) or not isinstance(guidance_interval, (tuple, list)) or len(guidance_interval) != 2:
        raise ValueError(f"guidance_interval must be a pair (lo, hi) of log-SNR values or None (got {guidance_interval!r})")
    lo, hi = (None if v is None else float(v) for v in guidance_interval)
    if any(v is not None and math.isnan(v) for v in (lo, hi)):
        raise ValueError(f"guidance_interval has a NaN end (got {guidance_interval!r})")
    lo, hi = -math.inf if lo is None else lo, math.inf if hi is None else hi
    if lo > hi:
        raise ValueError(f"guidance_interval must have lo <= hi (got {guidance_interval!r})")
    if lo == -math.inf and hi == math.inf:                  # unbounded at both ends: every call is guided, nothing to decide
        return Guidance(phi) if phi > 0.0 else None
    return Guidance(phi, lo, hi, True)


def guided_calls(log_snr: Sequence[float], g: Optional[Guidance], cond_scale: float) -> List[bool]:
    """Per denoiser call: guided (2B rows) iff cond_scale != 1 and the call's log-SNR lies in the interval."""
    on = cond_scale != 1.0
    return [on and (g is None or g.contains(float(v))) for v in log_snr]


def ddim_log_snr(alphas_cumprod: torch.Tensor, timesteps: Sequence[int]) -> List[float]:
    """Discrete DDIM: log(abar_t / (1 - abar_t)) of the scheduler's cumulative alphas at the sampling timesteps, in fp64."""
    acp = alphas_cumprod.detach().cpu().double().tolist()
    return [math.log(acp[t] / (1.0 - acp[t])) for t in timesteps]


def flow_log_snr(t: float) -> float:
    """Rectified flow, x_t = t x_1 + (1 - t) noise: 2 log(t / (1 - t)) in fp64; -inf at t = 0 (pure noise), +inf at t = 1."""
    t = float(t)
    if t <= 0.0:
        return -math.inf
    if t >= 1.0:
        return math.inf
    return 2.0 * math.log(t / (1.0 - t))


def midpoint_eval_times(times: Sequence[float]) -> List[float]:
    """The evaluation times of ode.midpoint_loop over the grid `times`, in call order: t0 and t0 + dt / 2 per interval."""
    out: List[float] = []
    for t0, t1 in zip(times[:-1], times[1:]):
        out += [t0, t0 + 0.5 * (t1 - t0)]
    return out


def cfg_rescale(cond: torch.Tensor, null: torch.Tensor, cond_scale: float, phi: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """cond, null (B, ...) fp32 contiguous -> (out = f_b g (the shape of cond), factor (B,) fp32 = f_b): the guided prediction
    g = null + (cond - null) cond_scale rescaled to the conditional prediction's per-sample standard deviation and mixed back by phi,
    f_b = phi std_b(cond) / std_b(g) + (1 - phi).  Two launches, no atomics, deterministic; the workspace is a torch.empty per call, served
    by the caching allocator as ct_x0_quantile's is."""
    phi = check_phi(phi)
    for v in (cond, null):
        assert v.dtype == torch.float32 and v.is_contiguous() and v.shape == cond.shape and v.device == cond.device
    B, n = cond.shape[0], cond[0].numel()
    out = torch.empty_like(cond)
    factor = torch.empty((B,), dtype=torch.float32, device=cond.device)
    ws = torch.empty(_lib.load().osuf_cfg_rescale_workspace_bytes(B, n) // 8, dtype=torch.float64, device=cond.device)
    ops.call("osuf_cfg_rescale", ops._p(cond), ops._p(null), float(cond_scale), phi, ops._p(ws), ops._p(factor), ops._p(out), B, n, ops._stream())
    return out, factor
