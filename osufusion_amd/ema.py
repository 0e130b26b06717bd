"""Decay schedules of the exponential moving average (EMA) of the weights that train.FusedAdamW keeps in its optimizer pass.

Host only.  An `EMAConfig` describes one track; `ema_beta(cfg, k)` is the decay that optimizer step k (k = 1 is the first step) applies,
`ema_d(cfg, k)` the fp32 step size d = 1 - beta the kernel receives:  e <- e + d * (p_new - e).

  constant  beta_k = beta.
  warmup    ema_pytorch / diffusers EMAModel:  j = k - update_after_step - 1;  beta_k = 0 for j <= 0 (the track is a copy of the weights),
            else clamp(1 - (1 + j / inv_gamma) ** -power, min_beta, beta).
  power     EDM2 (Karras et al. 2024, "Analyzing and Improving the Training Dynamics of Diffusion Models", section 3.1):
            beta_k = (1 - 1/k) ** (gamma + 1); gamma directly, or from the profile's relative standard deviation sigma_rel.
"""
from __future__ import annotations

from dataclasses import asdict, dataclass
from typing import Optional, Sequence, Tuple, Union

import numpy as np

KINDS = ("constant", "warmup", "power")
MAX_TRACKS = 4                                             # what one osuf_adamw_ema launch carries


def sigma_rel_to_gamma(sigma_rel: float) -> float:
    """The exponent gamma of the power-function profile whose relative standard deviation is sigma_rel: the largest real root of
    g^3 + 7 g^2 + (16 - s^-2) g + (12 - s^-2)   (EDM2, algorithm 2)."""
    if not sigma_rel > 0.0:
        raise ValueError(f"sigma_rel must be positive, got {sigma_rel}")
    t = float(sigma_rel) ** -2
    roots = np.roots([1.0, 7.0, 16.0 - t, 12.0 - t])
    return float(roots[np.abs(roots.imag) < 1e-9].real.max())


@dataclass(frozen=True)
class EMAConfig:
    kind: str = "constant"
    beta: float = 0.9999                                   # constant: the decay; warmup: its upper clamp
    inv_gamma: float = 1.0                                 # warmup
    power: float = 2.0 / 3.0                               # warmup
    min_beta: float = 0.0                                  # warmup: lower clamp
    update_after_step: int = 0                             # warmup: the track stays a copy of the weights for this many steps more
    gamma: Optional[float] = None                          # power: the exponent, or
    sigma_rel: Optional[float] = None                      # power: the profile width it is derived from

    def __post_init__(self) -> None:
        if self.kind not in KINDS:
            raise ValueError(f"unknown EMA kind {self.kind!r}: one of {KINDS}")
        for name in ("beta", "min_beta"):
            v = getattr(self, name)
            if not 0.0 <= v <= 1.0:
                raise ValueError(f"EMA {name} must lie in [0, 1], got {v}")
        if self.kind == "warmup" and not (self.inv_gamma > 0.0 and self.update_after_step >= 0):
            raise ValueError("EMA warmup needs inv_gamma > 0 and update_after_step >= 0")
        if self.kind == "power":
            if (self.gamma is None) == (self.sigma_rel is None):
                raise ValueError("EMA kind 'power' takes exactly one of gamma and sigma_rel")
            if self.power_gamma() < 0.0:
                raise ValueError(f"EMA power exponent must be >= 0, got {self.power_gamma()}")

    def power_gamma(self) -> float:
        return float(self.gamma) if self.gamma is not None else sigma_rel_to_gamma(self.sigma_rel)

    def as_dict(self) -> dict:
        return asdict(self)


def ema_beta(cfg: EMAConfig, k: int) -> float:
    """The decay of optimizer step k >= 1."""
    if k < 1:
        raise ValueError(f"optimizer steps count from 1, got {k}")
    if cfg.kind == "constant":
        return float(cfg.beta)
    if cfg.kind == "warmup":
        j = k - cfg.update_after_step - 1
        if j <= 0:
            return 0.0
        return float(min(max(1.0 - (1.0 + j / cfg.inv_gamma) ** -cfg.power, cfg.min_beta), cfg.beta))
    return float((1.0 - 1.0 / k) ** (cfg.power_gamma() + 1.0))


def ema_d(cfg: EMAConfig, k: int) -> float:
    """1 - beta_k rounded to fp32, as a Python float: the value the kernel computes with (0 leaves the track alone, 1 copies)."""
    return float(np.float32(1.0 - ema_beta(cfg, k)))


def as_tracks(ema: Union[None, EMAConfig, Sequence[EMAConfig]]) -> Tuple[EMAConfig, ...]:
    """Trainer's `ema` argument as a tuple of at most MAX_TRACKS configs."""
    if ema is None:
        return ()
    tracks = (ema,) if isinstance(ema, EMAConfig) else tuple(ema)
    if not all(isinstance(c, EMAConfig) for c in tracks):
        raise ValueError("ema takes an EMAConfig or a sequence of them")
    if len(tracks) > MAX_TRACKS:
        raise ValueError(f"at most {MAX_TRACKS} EMA tracks, got {len(tracks)}")
    return tracks
