"""The project's own restatement of the guidance controls (a plain helper module, imported by tests/test_guidance_cpu.py and
tests/test_guidance_gpu.py; numpy and math only).

CFG rescale (Lin et al. 2024, sec. 3.4), as include/osufusion_hip.h states osuf_cfg_rescale:
  g    in np.float32, one rounding per operation, in the kernel's order: (cond - null), times cond_scale, plus null;
  sums of c, c^2, g, g^2 per sample exactly (math.fsum over fp64 values; the square of an fp32 value is exact in fp64);
  f    = phi sqrt(var(cond) / var(g)) + (1 - phi) in fp64 with var = sum x^2 - (sum x)^2 / n (the normalisation cancels), rounded once to
         fp32; 1 where n < 2 or var(g) <= 0; a negative rounding residue in var(cond) counts as 0; NaN where the sample holds a NaN or Inf;
  out  = np.float32(f) * g.
cond_scale and phi enter as the fp32 values the C entry point receives.  The kernel differs from this in the order of its fp64 additions
alone.

The guidance interval: the per-call log-SNR lists of the five sampling loops and the guided / unguided decision."""
import math
from typing import List, Optional, Sequence, Tuple

import numpy as np


def guide32(cond: np.ndarray, null: np.ndarray, cond_scale: float) -> np.ndarray:
    cond, null = np.asarray(cond, np.float32), np.asarray(null, np.float32)
    with np.errstate(all="ignore"):
        d = cond - null
        m = d * np.float32(cond_scale)
        return (null + m).astype(np.float32)


def _sums(v: np.ndarray) -> Tuple[float, float]:
    v64 = v.astype(np.float64).ravel()
    return math.fsum(v64.tolist()), math.fsum((v64 * v64).tolist())


def factor64(cond_b: np.ndarray, g_b: np.ndarray, phi: float) -> float:
    """f_b of one sample, in fp64."""
    n = cond_b.size
    if n < 2:
        return 1.0
    if not (np.isfinite(cond_b).all() and np.isfinite(g_b).all()):
        return math.nan
    (c1, c2), (g1, g2) = _sums(cond_b), _sums(g_b)
    vc, vg = c2 - c1 * c1 / n, g2 - g1 * g1 / n
    if vg <= 0.0:
        return 1.0
    vc = max(vc, 0.0)
    p = float(np.float32(phi))
    return p * math.sqrt(vc / vg) + (1.0 - p)


def rescale(cond: np.ndarray, null: np.ndarray, cond_scale: float, phi: float) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """-> (out (B, ...) fp32, factor (B,) fp32, g (B, ...) fp32)."""
    g = guide32(cond, null, cond_scale)
    f = np.array([factor64(np.asarray(cond[b], np.float32), g[b], phi) for b in range(g.shape[0])], dtype=np.float64).astype(np.float32)
    return apply32(f, g), f, g


def apply32(factor: np.ndarray, g: np.ndarray) -> np.ndarray:
    """out = np.float32(factor[b]) * g[b], one fp32 multiply per element."""
    with np.errstate(all="ignore"):
        return (np.asarray(factor, np.float32).reshape((-1,) + (1,) * (g.ndim - 1)) * g).astype(np.float32)


def ulps32(a, b) -> np.ndarray:
    """Distance in fp32 units in the last place between positive finite fp32 values."""
    ia, ib = np.asarray(a, np.float32).view(np.int32).astype(np.int64), np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


# ---- the log-SNR of every denoiser call, per loop ------------------------------------------------------------------------------------------
def ddim_timesteps(train_timesteps: int, steps: int) -> List[int]:
    return [i * (train_timesteps // steps) for i in range(steps)][::-1]


def ddim_log_snr(alphas_cumprod: Sequence[float], train_timesteps: int, steps: int) -> List[float]:
    """Discrete DDIM: log(abar_t / (1 - abar_t)) at the sampling timesteps, fp64, from the scheduler's cumulative alphas as given."""
    return [math.log(float(alphas_cumprod[t]) / (1.0 - float(alphas_cumprod[t]))) for t in ddim_timesteps(train_timesteps, steps)]


def ct_log_snr(denoiser_inputs: Sequence[float]) -> List[float]:
    """Continuous time, every sampler: the fp32 log-SNR the denoiser is given for the call, as a host float."""
    return [float(np.float32(v)) for v in denoiser_inputs]


def flow_eval_times(times: Sequence[float]) -> List[float]:
    """The midpoint loop over the grid `times`: t0 and t0 + dt / 2 per interval, in call order."""
    out: List[float] = []
    for t0, t1 in zip(times[:-1], times[1:]):
        out += [t0, t0 + 0.5 * (t1 - t0)]
    return out


def flow_log_snr(times: Sequence[float]) -> List[float]:
    """Flow: 2 log(t / (1 - t)) of every evaluation time, fp64, -inf at t = 0."""
    return [-math.inf if t <= 0.0 else math.inf if t >= 1.0 else 2.0 * math.log(t / (1.0 - t)) for t in flow_eval_times(times)]


def decide(log_snr: Sequence[float], interval: Optional[Tuple[Optional[float], Optional[float]]], cond_scale: float) -> List[bool]:
    """A call is guided iff cond_scale != 1 and lo <= its log-SNR <= hi (None at an end: unbounded; no interval: every call)."""
    lo, hi = (None, None) if interval is None else interval
    lo, hi = -math.inf if lo is None else float(lo), math.inf if hi is None else float(hi)
    return [cond_scale != 1.0 and lo <= v <= hi for v in log_snr]


def rows_per_call(guided: Sequence[bool], batch: int) -> List[int]:
    return [2 * batch if g else batch for g in guided]
