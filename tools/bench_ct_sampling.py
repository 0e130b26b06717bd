"""Ancestral-sampling steps/s of ContinuousDiffusionOsuFusionDiT.sample against the same loop with the step composed from torch ops.

    python tools/bench_ct_sampling.py [--out profiles/ct_sampling.json] [--B 16] [--L 8192] [--cfg 7.0] [--steps 4] [--rounds 5]
                                      [--backbones dit,mmdit] [--depth 12]

Both backbones at their default widths (dim_h 512), bf16 compute, cosine schedule.  Rows:
  * composed: the same once-per-call denoiser (2B rows per step with guidance), the schedule as the dozen B-sized torch kernels of the
    reference's scheduler.py per step, and the step (guidance, start prediction, clamp, posterior mean, noise) as torch elementwise ops
    with per-sample broadcasts;
  * sample: `ContinuousDiffusionOsuFusionDiT.sample` (one osuf_ct_schedule per call, one osuf_ct_step per step).
The two loops run in ONE process on the same weights and inputs, interleaved round by round after a warm-up of each; a row is the median
over the rounds of (host clock around `steps` steps ending in a device synchronise) and the spread.  `step_ms` is the step alone (schedule
+ elementwise work, no denoiser), timed the same way on recorded predictions.  A timing tool, not a gate."""
import argparse
import json
import math
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

from osufusion_amd import ops  # noqa: E402
from osufusion_amd.models import ContinuousDiffusionOsuFusionDiT  # noqa: E402

DEV = "cuda"


def cosine_log_snr(t, s=0.008):
    return -torch.log(((torch.cos((t + s) / (1 + s) * math.pi * 0.5) ** -2) - 1).clamp(min=1e-8))


def composed_step(x, pred, b, cfg, cond_scale, t, t_next, noise):
    """scheduler.py's predict_start_from_noise + q_posterior + the noise term, in torch."""
    eps = pred[b:] + (pred[:b] - pred[b:]) * cond_scale if cfg else pred
    log_snr, log_snr_next = cosine_log_snr(t)[:, None, None], cosine_log_snr(t_next)[:, None, None]
    alpha, sigma = torch.sqrt(torch.sigmoid(log_snr)), torch.sqrt(torch.sigmoid(-log_snr))
    alpha_next, sigma_next = torch.sqrt(torch.sigmoid(log_snr_next)), torch.sqrt(torch.sigmoid(-log_snr_next))
    x0 = ((x - sigma * eps) / alpha.clamp(min=1e-8)).clamp(-1.0, 1.0)
    c = -torch.expm1(log_snr - log_snr_next)
    mean = alpha_next * (x * (1 - c) / alpha + c * x0)
    if noise is None:
        return mean
    log_var = torch.log(((sigma_next ** 2) * c).clamp(min=1e-20))
    return mean + torch.exp(0.5 * log_var) * noise


def composed_loop(model, a, c, x, steps, cond_scale):
    b = a.shape[0]
    cfg = cond_scale != 1.0
    total = model.scheduler.timesteps
    x = x.float().contiguous()
    with torch.inference_mode(), ops.reproducible_mode(True), ops.one_launch_attention(True), model._dtype_ctx():
        pairs = model.scheduler.get_sampling_timesteps(b, torch.device(DEV))
        f = model._denoiser(a, c, cfg)
        for i in range(steps):
            t, t_next = pairs[i][0], pairs[i][1]
            pred = f(x, cosine_log_snr(t).repeat(2 if cfg else 1))
            noise = torch.randn(x.shape, device=DEV) if i < total - 1 else None
            x = composed_step(x, pred, b, cfg, cond_scale, t, t_next, noise)
    return x


def wall(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--L", type=int, default=8192)
    ap.add_argument("--cfg", type=float, default=7.0)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--backbones", default="dit,mmdit")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ct_sampling.py needs an MI355X"
    B, L, S = args.B, args.L, args.steps
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "B": B, "L": L, "cfg": args.cfg, "dtype": "bf16",
           "steps_per_window": S, "rounds": args.rounds, "rows": []}
    for backbone in args.backbones.split(","):
        torch.manual_seed(0)
        model = ContinuousDiffusionOsuFusionDiT(512, backbone=backbone, depth=args.depth, sampling_timesteps=35).to(DEV)
        with torch.no_grad():                                # the reference zero-inits the adaLN modulations and the output: use live weights
            for p in model.parameters():
                if not p.any():
                    p.normal_(0, 0.02)
        model.set_full_bf16()
        model.stop_after = S
        a = torch.rand(B, 96, L, device=DEV) * 10 - 15
        c = torch.rand(B, 5, device=DEV) * 2 - 1
        x = torch.randn(B, 6, L, device=DEV)
        cfg = args.cfg != 1.0

        def sample():
            torch.manual_seed(1)
            return model.sample(a, c, x, cond_scale=args.cfg)

        def composed():
            torch.manual_seed(1)
            return composed_loop(model, a, c, x, S, args.cfg)

        # the step alone, on a recorded prediction
        pred = torch.randn((2 * B if cfg else B, 6, L), device=DEV)
        noise = torch.randn_like(x)
        pair = model.scheduler.get_sampling_timesteps(B, torch.device(DEV))[3]
        t, t_next = pair[0].contiguous(), pair[1].contiguous()

        def step_kernel():
            for _ in range(S):
                ops.ct_step(x, pred[:B], pred[B:] if cfg else None, args.cfg, model.scheduler.coefficients(t, t_next), noise)

        def step_composed():
            for _ in range(S):
                composed_step(x, pred, B, cfg, args.cfg, t, t_next, noise)

        loops = {"composed": composed, "sample": sample}
        outs = {}
        for name, fn in loops.items():                       # warm-up (pack caches, code objects)
            fn()
            outs[name] = fn()
        step_kernel(), step_composed()
        diff = ((outs["sample"] - outs["composed"]).norm() / outs["composed"].norm()).item()
        times = {name: [] for name in loops}
        step_times = {"composed": [], "sample": []}
        for _ in range(args.rounds):                         # interleaved: composed, sample, composed, sample, ...
            for name, fn in loops.items():
                times[name].append(wall(fn))
            step_times["composed"].append(wall(step_composed))
            step_times["sample"].append(wall(step_kernel))
        for name in loops:
            med = statistics.median(times[name])
            row = {"backbone": backbone, "loop": name, "steps_per_s": round(S / med, 3), "ms_per_step": round(med / S * 1e3, 2),
                   "ms_per_step_min_max": [round(min(times[name]) / S * 1e3, 2), round(max(times[name]) / S * 1e3, 2)],
                   "step_ms": round(statistics.median(step_times[name]) / S * 1e3, 3),
                   "rel_l2_vs_composed_after_window": diff if name == "sample" else 0.0}
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
        del model
        torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
