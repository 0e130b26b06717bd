"""Dynamic thresholding's cost: osuf_ct_x0_quantile + osuf_ct_step_ex against the same step composed from torch ops, and the whole
ContinuousDiffusionOsuFusionDiT.sample with and without thresholding.

    python tools/bench_ct_objectives.py [--out profiles/ct_objectives.md] [--B 16] [--L 8192,65536] [--cfg 7.0] [--q 0.95]
                                        [--iters 10] [--rounds 7] [--steps 4] [--depth 12] [--backbone dit]

Kernel timing, per L: one thresholded ancestral step on recorded predictions (guidance 7, noise objective, cosine schedule),
  * kernels: ops.ct_x0_quantile + ops.ct_step_ex (two entry points: a memset, three counting launches, a finish, the step);
  * composed: guidance, x0, |x0|, torch.quantile per sample, clamp(-s, s), divide, posterior mean, noise, as torch elementwise ops on the
    same schedule row.
Whole sampler, at the first L: `steps` steps of sample() (bf16 backbone at its default width) with dynamic_thresholding on and off, on
the same weights and inputs; the difference per step is the cost thresholding adds to a step of the same build.
Everything runs in ONE process, interleaved round by round after a warm-up of each; a figure is the median over the rounds of (host
clock around the window, ending in a device synchronise), with the spread.  A timing tool, not a gate."""
import argparse
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

from osufusion_amd import ct, ops  # noqa: E402
from osufusion_amd.models import ContinuousDiffusionOsuFusionDiT  # noqa: E402

DEV = "cuda"


def composed_step(x, cond, null, cond_scale, row, noise, q):
    k = [row[:, j].reshape(-1, 1, 1) for j in range(13)]
    p = null + (cond - null) * cond_scale
    x0 = (x - k[2] * p) * k[9]
    s = torch.quantile(x0.abs().flatten(1), q, dim=1).clamp(min=1.0).reshape(-1, 1, 1)
    x0 = x0.clamp(-s, s) / s
    return k[10] * x + k[11] * x0 + k[12] * noise


def wall(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def med(v, per):
    return statistics.median(v) / per * 1e3, min(v) / per * 1e3, max(v) / per * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--L", default="8192,65536")
    ap.add_argument("--cfg", type=float, default=7.0)
    ap.add_argument("--q", type=float, default=0.95)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--backbone", default="dit")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ct_objectives.py needs an MI355X"
    B, Ls = args.B, [int(v) for v in args.L.split(",")]
    lines = ["# Dynamic thresholding: timings", "",
             f"`tools/bench_ct_objectives.py` on {torch.cuda.get_device_name(0)}, torch {torch.__version__}: B = {B}, guidance {args.cfg}, q = {args.q}, "
             f"median of {args.rounds} interleaved rounds (min .. max).", "",
             "## One thresholded step on recorded predictions", "",
             "| L | values per sample | kernels: quantile + step (ms) | of which quantile (ms) | torch composition (ms) | composition / kernels | max abs diff of the step |",
             "|---|---|---|---|---|---|---|"]
    for L in Ls:
        torch.manual_seed(0)
        x, cond, noise = (torch.randn((B, 6, L), device=DEV) for _ in range(3))
        null = cond + 0.05 * torch.randn_like(cond)
        t = torch.full((B,), 0.5, device=DEV)
        row = ops.ct_schedule(t, t - 1.0 / 35, ct.KINDS["cosine"])

        def kernels():
            for _ in range(args.iters):
                s = ops.ct_x0_quantile(x, cond, null, args.cfg, row, "noise", args.q)[:, 2]
                out = ops.ct_step_ex(x, cond, null, args.cfg, row, noise, "noise", s)
            return out

        def quantile_only():
            for _ in range(args.iters):
                ops.ct_x0_quantile(x, cond, null, args.cfg, row, "noise", args.q)

        def composed():
            for _ in range(args.iters):
                out = composed_step(x, cond, null, args.cfg, row, noise, args.q)
            return out

        diff = (kernels() - composed()).abs().max().item()                 # also the warm-up
        quantile_only()
        tk, tq, tc = [], [], []
        for _ in range(args.rounds):
            tc.append(wall(composed))
            tk.append(wall(kernels))
            tq.append(wall(quantile_only))
        k, qo, c = med(tk, args.iters), med(tq, args.iters), med(tc, args.iters)
        lines.append(f"| {L} | {6 * L} | {k[0]:.3f} ({k[1]:.3f} .. {k[2]:.3f}) | {qo[0]:.3f} ({qo[1]:.3f} .. {qo[2]:.3f}) | {c[0]:.3f} ({c[1]:.3f} .. {c[2]:.3f}) | "
                     f"{c[0] / k[0]:.2f}x | {diff:.2e} |")
        print(lines[-1], flush=True)
        del x, cond, noise, null
        torch.cuda.empty_cache()

    L, S = Ls[0], args.steps
    torch.manual_seed(0)
    models = {}
    for name, thr in (("static clamp", False), ("dynamic thresholding", True)):
        torch.manual_seed(0)
        m = ContinuousDiffusionOsuFusionDiT(512, backbone=args.backbone, depth=args.depth, sampling_timesteps=35, dynamic_thresholding=thr,
                                            dynamic_thresholding_percentile=args.q).to(DEV)
        with torch.no_grad():                                # the reference zero-inits the adaLN modulations and the output: use live weights
            gen = torch.Generator(device=DEV).manual_seed(1)
            for p in m.parameters():
                if not p.any():
                    p.normal_(0, 0.02, generator=gen)
        m.set_full_bf16()
        m.stop_after = S
        models[name] = m
    a = torch.rand(B, 96, L, device=DEV) * 10 - 15
    c = torch.rand(B, 5, device=DEV) * 2 - 1
    x = torch.randn(B, 6, L, device=DEV)

    def run(m):
        torch.manual_seed(1)
        return m.sample(a, c, x, cond_scale=args.cfg)

    for m in models.values():
        run(m), run(m)
    times = {name: [] for name in models}
    for _ in range(args.rounds):
        for name, m in models.items():
            times[name].append(wall(lambda: run(m)))
    res = {name: med(v, S) for name, v in times.items()}
    added = res["dynamic thresholding"][0] - res["static clamp"][0]
    lines += ["", f"## Whole sampler: {args.backbone}, dim_h 512, depth {args.depth}, bf16, B = {B}, L = {L}, {S} steps per window", "",
              "| sampler | ms per step |", "|---|---|"]
    lines += [f"| {name} | {r[0]:.2f} ({r[1]:.2f} .. {r[2]:.2f}) |" for name, r in res.items()]
    lines += ["", f"Thresholding adds {added:.3f} ms per step ({100 * added / res['static clamp'][0]:.2f} % of the unthresholded step of the same build)."]
    print("\n".join(lines[-6:]), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
