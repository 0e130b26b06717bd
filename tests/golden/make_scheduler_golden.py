#!/usr/bin/env python3
"""Golden vectors of the continuous-time scheduler.  Runs ONLY in the build container, next to the reference:

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=/path/to/reference:. python3 tests/golden/make_scheduler_golden.py

It imports the reference's osu_fusion.modules.scheduler (nothing is copied) and records, on the CPU in fp32, for both noise schedules
(keys prefixed `linear/` and `cosine/`): log_snr, alpha and sigma at the times `t`; q_sample, predict_start_from_noise and q_posterior
(explicit t_next = max(t - 1/8, 0), and the default of a timesteps = 8 scheduler, which is the same times) on seeded (6, 6, 37) inputs,
one time per sample; and, shared, the get_sampling_timesteps(2) grid for timesteps = 8 and 1 and one get_times row.  A few KB.
"""
from __future__ import annotations

from pathlib import Path

import numpy as np
import torch

from osu_fusion.modules.scheduler import GaussianDiffusionContinuousTimes, log_snr_to_alpha_sigma  # reference, PYTHONPATH

HERE = Path(__file__).resolve().parent
TIMES = (0.0, 1e-3, 0.25, 0.5, 0.999, 1.0)
TIMESTEPS = 8


def main() -> None:
    g = torch.Generator().manual_seed(20240607)
    t = torch.tensor(TIMES, dtype=torch.float32)
    t_next = (t - 1.0 / TIMESTEPS).clamp(min=0.0)
    x_0 = torch.randn((len(TIMES), 6, 37), generator=g).clamp(-1, 1)
    noise = torch.randn((len(TIMES), 6, 37), generator=g)
    arrays = dict(t=t, t_next=t_next, x_0=x_0, noise=noise)
    for schedule in ("linear", "cosine"):
        sch = GaussianDiffusionContinuousTimes(noise_schedule=schedule, timesteps=TIMESTEPS)
        log_snr = sch.get_condition(t)
        alpha, sigma = log_snr_to_alpha_sigma(log_snr)
        x_t, qs_log_snr, qs_alpha, qs_sigma = sch.q_sample(x_0, t, noise)
        start = sch.predict_start_from_noise(x_t, t, noise)
        mean, var, logvar = sch.q_posterior(x_0, x_t, t, t_next)
        mean_d, var_d, logvar_d = sch.q_posterior(x_0, x_t, t)
        x_half = sch.q_sample(x_0, 0.5, noise)[0]                                        # a float t
        case = dict(log_snr=log_snr, alpha=alpha, sigma=sigma, x_t=x_t, qs_log_snr=qs_log_snr, qs_alpha=qs_alpha, qs_sigma=qs_sigma,
                    start=start, post_mean=mean, post_var=var, post_logvar=logvar, post_mean_default=mean_d, post_var_default=var_d,
                    post_logvar_default=logvar_d, x_half=x_half)
        for k, v in case.items():
            assert torch.isfinite(v).all(), (schedule, k)
            arrays[f"{schedule}/{k}"] = v
    for n in (TIMESTEPS, 1):
        pairs = GaussianDiffusionContinuousTimes(timesteps=n).get_sampling_timesteps(2, torch.device("cpu"))
        arrays[f"grid{n}"] = torch.stack(list(pairs))                                     # (n, 2, B)
    arrays["get_times"] = GaussianDiffusionContinuousTimes().get_times(3, 0.25, torch.device("cpu"))
    fn = HERE / "scheduler_cases.npz"
    np.savez_compressed(fn, **{k: v.numpy() for k, v in arrays.items()})
    print(f"wrote {fn.name} ({fn.stat().st_size / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
