"""The solver step kernel against its neighbours, and seconds per sample() for the three samplers of ContinuousDiffusionOsuFusionDiT.

    python tools/bench_ct_solvers.py [--out profiles/ct_solvers.json] [--B 16] [--L 8192] [--cfg 7.0] [--rounds 3] [--iters 20]
                                     [--backbones dit,mmdit] [--depth 12] [--skip-sample]

Step rows (fp32, (B, 6, L), guidance on, noise objective, static clamp), each the median over `rounds` of (host clock around `iters` launches
ending in a device synchronise) / iters, after a warm-up:
  * copy: x.clone() -- the measured rate of one read and one write stream, the yardstick for the memory-bound kernels below;
  * ct_step_ex: the ancestral step, 4 streams read (x, cond, null, noise), 1 written;
  * solver_step 2m: osuf_ct_solver_step on a later 2M step, 4 read (x, cond, null, x0_prev), 2 written;
  * solver_step ddim_eta: the same with noise in place of x0_prev; solver_step ddim0: 3 read, 2 written;
  * composed 2m: the 2M update from torch elementwise ops with the factors read from the same device rows.
GB/s = (streams read + written) * 4 B * elements / time.
Sample rows: seconds per sample() (median, min, max over the rounds; interleaved round by round) for ddpm at 35 steps, ddim at 35 and
dpmpp_2m at 16 and 20, bf16 compute, both backbones at their default widths.  A timing tool, not a gate."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

from osufusion_amd import ops  # noqa: E402
from osufusion_amd.models import ContinuousDiffusionOsuFusionDiT  # noqa: E402
from osufusion_amd.modules import GaussianDiffusionContinuousTimes  # noqa: E402

DEV = "cuda"
SAMPLE_CASES = (("ddpm", 35), ("ddim", 35), ("dpmpp_2m", 16), ("dpmpp_2m", 20))


def wall(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def composed_2m(x, cond, null, cond_scale, row, fac, prev):
    """The later 2M step in torch: guidance, start prediction from the noise prediction, clamp, three-term update."""
    eps = null + (cond - null) * cond_scale
    sigma, inv_alpha = row[:, 2, None, None], row[:, 9, None, None]
    x0 = ((x - sigma * eps) * inv_alpha).clamp(-1.0, 1.0)
    return fac[0] * x + fac[1] * x0 + fac[2] * prev, x0


def step_rows(B, L, cond_scale, rounds, iters):
    sch = GaussianDiffusionContinuousTimes("cosine")
    grid = sch.solver_log_snr_grid(16, device=DEV)
    n = B * 6 * L
    x, cond, noise = (torch.randn(B, 6, L, device=DEV) for _ in range(3))
    null = cond + 0.05 * torch.randn_like(cond)
    prev = torch.tanh(torch.randn_like(x))
    rows, fac = {}, {}
    for name, sampler, eta in (("2m", "dpmpp_2m", 0.0), ("ddim0", "ddim", 0.0), ("ddim_eta", "ddim", 0.5)):
        r, f = ops.ct_solver_schedule(grid, sampler, eta, B)
        rows[name], fac[name] = r[8], f[8]
    cases = {
        "copy": (2, lambda: x.clone()),
        "ct_step_ex": (5, lambda: ops.ct_step_ex(x, cond, null, cond_scale, rows["2m"], noise, "noise", None)),
        "solver_step 2m": (6, lambda: ops.ct_solver_step(x, cond, null, cond_scale, rows["2m"], fac["2m"], prev, None, "noise")),
        "solver_step ddim_eta": (6, lambda: ops.ct_solver_step(x, cond, null, cond_scale, rows["ddim_eta"], fac["ddim_eta"], None, noise, "noise")),
        "solver_step ddim0": (5, lambda: ops.ct_solver_step(x, cond, null, cond_scale, rows["ddim0"], fac["ddim0"], None, None, "noise")),
        "composed 2m": (6, lambda: composed_2m(x, cond, null, cond_scale, rows["2m"], fac["2m"], prev)),
    }
    out = []
    times = {k: [] for k in cases}
    for _, fn in cases.values():
        fn()
    for _ in range(rounds):
        for name, (_, fn) in cases.items():
            times[name].append(wall(lambda: [fn() for _ in range(iters)]) / iters)
    for name, (streams, _) in cases.items():
        med = statistics.median(times[name])
        row = {"kind": "step", "name": name, "us": round(med * 1e6, 1), "us_min_max": [round(min(times[name]) * 1e6, 1), round(max(times[name]) * 1e6, 1)],
               "streams": streams, "GBps": round(streams * 4 * n / med / 1e9, 1)}
        out.append(row)
        print(json.dumps(row), flush=True)
    return out


def sample_rows(backbone, B, L, cond_scale, rounds, depth):
    a = torch.rand(B, 96, L, device=DEV) * 10 - 15
    c = torch.rand(B, 5, device=DEV) * 2 - 1
    x = torch.randn(B, 6, L, device=DEV)
    torch.manual_seed(0)
    model = ContinuousDiffusionOsuFusionDiT(512, backbone=backbone, depth=depth).to(DEV)
    with torch.no_grad():                                    # the reference zero-inits the adaLN modulations and the output: use live weights
        for p in model.parameters():
            if not p.any():
                p.normal_(0, 0.02)
    model.set_full_bf16()

    def run(sampler, steps):
        model.sampler = sampler
        model.sampling_timesteps = model.scheduler.timesteps = steps
        torch.manual_seed(1)
        return model.sample(a, c, x, cond_scale=cond_scale)

    model.stop_after = 2
    for sampler, steps in SAMPLE_CASES:                      # warm-up (pack caches, code objects): two steps of each
        run(sampler, steps)
    model.stop_after = None
    times = {case: [] for case in SAMPLE_CASES}
    for _ in range(rounds):
        for case in SAMPLE_CASES:
            times[case].append(wall(lambda: run(*case)))
    out = []
    for (sampler, steps), ts in times.items():
        med = statistics.median(ts)
        row = {"kind": "sample", "backbone": backbone, "sampler": sampler, "steps": steps, "s_per_sample": round(med, 3),
               "s_min_max": [round(min(ts), 3), round(max(ts), 3)], "ms_per_step": round(med / steps * 1e3, 2)}
        out.append(row)
        print(json.dumps(row), flush=True)
    del model
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--L", type=int, default=8192)
    ap.add_argument("--cfg", type=float, default=7.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--backbones", default="dit,mmdit")
    ap.add_argument("--skip-sample", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ct_solvers.py needs an MI355X"
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "B": args.B, "L": args.L, "cfg": args.cfg, "rounds": args.rounds,
           "iters": args.iters, "rows": step_rows(args.B, args.L, args.cfg, args.rounds, args.iters)}
    if not args.skip_sample:
        for backbone in args.backbones.split(","):
            res["rows"] += sample_rows(backbone, args.B, args.L, args.cfg, args.rounds, args.depth)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
