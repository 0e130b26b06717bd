"""scheduler.py: GaussianDiffusionContinuousTimes, the linear / cosine log-SNR schedule in continuous time.  Method names, argument
orders, return tuples and the error are the reference's.  Every per-sample value (log_snr, alpha, sigma, the posterior's c, variance and
log-variance) comes from one osuf_ct_schedule launch, which evaluates the schedule in fp32 in the reference's order of operations; the
full-size arithmetic is osuf_axpby_rows.  Tensors must be on the GPU; the time grids (get_times, get_sampling_timesteps) are plain
constructors and take any device."""
from typing import Optional, Tuple, Union

import torch
import torch.nn as nn

from .. import ct
from .. import ops
from .. import runtime as rt


def _pad_to(x: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """utils.right_pad_dims_to: (B,) -> (B, 1, ..., 1) with x's number of dims."""
    return v.reshape(v.shape + (1,) * (x.dim() - v.dim()))


class GaussianDiffusionContinuousTimes(nn.Module):
    def __init__(self, noise_schedule: str = "linear", timesteps: int = 1000) -> None:
        super().__init__()
        if noise_schedule not in ct.KINDS:
            msg = f"Unknown noise schedule: {noise_schedule}"
            raise ValueError(msg)
        self.noise_schedule = noise_schedule
        self.kind = ct.KINDS[noise_schedule]
        self.timesteps = timesteps
        self._log_snr_ends: Optional[Tuple[float, float]] = None    # (log_snr(1), log_snr(0)) as the kernel gives them, for solver_log_snr_grid

    def coefficients(self, t: torch.Tensor, t_next: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The schedule rows of ops.ct_schedule at t (and t_next), (B, 3) or (B, 13) fp32: what a sampler hands to ops.ct_step."""
        rt.require_gpu(t)
        return ops.ct_schedule(t, t_next, self.kind)

    def log_snr(self, t: torch.Tensor) -> torch.Tensor:
        rt.require_gpu(t)
        return ops.ct_schedule(t.reshape(-1), None, self.kind)[:, ct.LOG_SNR].reshape(t.shape)

    def get_times(self, batch_size: int, noise_level: float, device: torch.device) -> torch.Tensor:
        return torch.full((batch_size,), noise_level, device=device, dtype=torch.float32)

    def sample_random_times(self, batch_size: int, device: torch.device) -> torch.Tensor:
        return torch.zeros((batch_size,), device=device, dtype=torch.float32).uniform_(0, 1)

    def get_condition(self, t: torch.Tensor) -> torch.Tensor:
        return self.log_snr(t)

    def get_sampling_timesteps(self, batch_size: int, device: torch.device) -> Tuple[torch.Tensor, ...]:
        """`timesteps` tensors (2, B): row 0 the step's time, row 1 the next one, from 1 down to 0."""
        times = torch.linspace(1.0, 0.0, self.timesteps + 1, device=device, dtype=torch.float32)
        times = times[None, :].expand(batch_size, -1)
        times = torch.stack((times[:, :-1], times[:, 1:]), dim=0)
        return times.unbind(dim=-1)

    # ---- DDIM / DPM-Solver++(2M) on a log-SNR grid (the reference samples ancestrally only) ----
    def solver_log_snr_grid(self, steps: int, spacing: str = "logsnr", logsnr_min: float = -15.0,
                            device: Union[torch.device, str] = "cuda") -> torch.Tensor:
        """The solvers' grid, (steps + 1,) fp32 log-SNR values rising from noise to data.  "time": the kernel's log_snr at
        linspace(1, 0, steps + 1), the ancestral sampler's grid.  "logsnr": torch.linspace from max(log_snr(1), logsnr_min) to log_snr(0),
        the two ends from osuf_ct_schedule -- the backbone is conditioned on log_snr, so no inverse of the schedule is needed.  At the default
        logsnr_min = -15 alpha is 5.5e-4: a standard-normal start iterate is the marginal there to within that."""
        if spacing not in ("logsnr", "time"):
            raise ValueError(f"Unknown solver spacing: {spacing!r} (one of ['logsnr', 'time'])")
        if steps < 1:
            raise ValueError(f"steps must be at least 1 (got {steps})")
        if spacing == "time":
            return self.log_snr(torch.linspace(1.0, 0.0, steps + 1, device=device, dtype=torch.float32))
        if self._log_snr_ends is None:                                              # two constants of the schedule: read back once
            self._log_snr_ends = tuple(self.log_snr(torch.tensor([1.0, 0.0], device=device, dtype=torch.float32)).tolist())
        lo, hi = self._log_snr_ends
        return torch.linspace(max(lo, float(logsnr_min)), hi, steps + 1, device=device, dtype=torch.float32)

    def solver_coefficients(self, grid: torch.Tensor, sampler: str = "dpmpp_2m", eta: float = 0.0,
                            batch: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
        """ops.ct_solver_schedule on a grid of solver_log_snr_grid: (rows (S, batch, 13), fac (S, 4)), what a sampler hands to
        ops.ct_x0_quantile and ops.ct_solver_step step by step."""
        rt.require_gpu(grid)
        return ops.ct_solver_schedule(grid, sampler, eta, batch)

    def q_posterior(self, x_0: torch.Tensor, x_t: torch.Tensor, t: torch.Tensor,
                    t_next: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        rt.require_gpu(x_t)
        if t_next is None:
            t_next = (t - 1.0 / self.timesteps).clamp(min=0.0)
        k = self.coefficients(t, t_next)
        mean = ops.axpby_rows(x_t.float().contiguous(), x_0.float().contiguous(), k[:, ct.K_X].contiguous(), k[:, ct.K_X0].contiguous())
        return mean, _pad_to(x_t, k[:, ct.POST_VAR]), _pad_to(x_t, k[:, ct.POST_LOG_VAR])

    def q_sample(self, x_0: torch.Tensor, t: Union[torch.Tensor, float],
                 noise: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        rt.require_gpu(x_0)
        if isinstance(t, float):
            t = torch.full((x_0.shape[0],), t, dtype=torch.float32, device=x_0.device)
        noise = torch.randn_like(x_0) if noise is None else noise
        k = self.coefficients(t)
        alpha, sigma = k[:, ct.ALPHA].contiguous(), k[:, ct.SIGMA].contiguous()
        x_t = ops.axpby_rows(x_0.float().contiguous(), noise.float().contiguous(), alpha, sigma)
        return x_t, k[:, ct.LOG_SNR], _pad_to(x_0, alpha), _pad_to(x_0, sigma)

    def predict_start_from_noise(self, x_t: torch.Tensor, t: torch.Tensor, noise: torch.Tensor) -> torch.Tensor:
        rt.require_gpu(x_t)
        k = self.coefficients(t)
        inv_alpha = 1.0 / k[:, ct.ALPHA].clamp(min=1e-8)
        return ops.axpby_rows(x_t.float().contiguous(), noise.float().contiguous(), inv_alpha, -(k[:, ct.SIGMA] * inv_alpha))

    # ---- v / x_start objectives, min-SNR-gamma, dynamic thresholding (imagen-pytorch's formulas; the reference has none of them) ----
    def predict_start_from_v(self, x_t: torch.Tensor, t: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
        """x_0 = alpha x_t - sigma v."""
        rt.require_gpu(x_t)
        k = self.coefficients(t)
        return ops.axpby_rows(x_t.float().contiguous(), v.float().contiguous(), k[:, ct.ALPHA].contiguous(), -k[:, ct.SIGMA])

    def calculate_v(self, x_0: torch.Tensor, t: torch.Tensor, noise: torch.Tensor) -> torch.Tensor:
        """v = alpha noise - sigma x_0."""
        rt.require_gpu(x_0)
        k = self.coefficients(t)
        return ops.axpby_rows(noise.float().contiguous(), x_0.float().contiguous(), k[:, ct.ALPHA].contiguous(), -k[:, ct.SIGMA])

    @staticmethod
    def loss_weight(log_snr: torch.Tensor, objective: str = "noise", min_snr_gamma: Optional[float] = None) -> Optional[torch.Tensor]:
        """Min-SNR-gamma weights of the per-sample MSE: with snr = exp(log_snr) and c = min(snr, gamma), c / snr for a noise prediction, c for
        x_start, c / (snr + 1) for v; None (unweighted) when gamma is None.  Plain torch, any device."""
        if objective not in ct.OBJECTIVES:
            raise ValueError(f"Unknown prediction objective: {objective!r} (one of {sorted(ct.OBJECTIVES)})")
        if min_snr_gamma is None:
            return None
        snr = log_snr.exp()
        c = snr.clamp(max=min_snr_gamma)
        return {"noise": c / snr, "x_start": c, "v": c / (snr + 1)}[objective]

    @staticmethod
    def dynamic_threshold(x_0: torch.Tensor, percentile: float = 0.95) -> torch.Tensor:
        """Imagen 2.3 in plain torch (any device): s = max(1, the per-sample `percentile` quantile of |x_0|), x_0.clamp(-s, s) / s.  What
        ops.ct_x0_quantile + ops.ct_step_ex do inside the sampler's step without forming x_0."""
        s = torch.quantile(x_0.abs().reshape(x_0.shape[0], -1), percentile, dim=-1).clamp(min=1.0)
        s = _pad_to(x_0, s)
        return x_0.clamp(-s, s) / s
