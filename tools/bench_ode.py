"""What the ODE solvers of the flow samplers cost, on the build under test: osuf_rk_error beside the same quantity composed from torch
operations, and every method of RectifiedFlowOsuFusionDiT.sample in evaluations and seconds.

    python tools/bench_ode.py [--out profiles/ode_solvers.md] [--B 16] [--L 8192] [--cfg 2.0] [--steps 16] [--rounds 3] [--iters 50]
                              [--depth 12] [--backbones dit,mmdit] [--rtol 1e-2] [--atol 1e-2] [--max-steps 60]

The kernel: fp32 (B, 6, L), S = 7 stages with Dormand-Prince's weights (one of them zero: six stages and the two states are read, 8 streams
of 4 bytes), the median over `rounds` of (host clock around `iters` calls ending in a device synchronise) / iters after a warm-up, against
an fp64 torch composition of the same ratio, and the GB/s the byte count gives.  The toy problem: y' = omega J y on the channel pairs in
fp64 numpy (tests/ode_oracle.py's restatement, no GPU work), evaluations and distance to the closed form per method.  The backbones
(dim_h 512, bf16 compute, random live weights, so the flow is not a trained one and the adaptive methods' step counts say nothing about a
trained model): evaluations, accepted and rejected steps and seconds per sample() call, interleaved round by round.  The tables are
written as markdown to --out; where that file already has the "## Measured" section only that section is replaced.  A timing tool, not a gate."""
import argparse
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from osufusion_amd import ode, ops  # noqa: E402
from osufusion_amd.models import RectifiedFlowOsuFusionDiT  # noqa: E402
from tests import ode_oracle as OO  # noqa: E402

DEV = "cuda"
METHODS = ("euler", "midpoint", "rk4", "bosh3", "dopri5")


def wall(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def kernel_rows(B, L, rounds, iters):
    y0, y1 = torch.randn(B, 6, L, device=DEV), torch.randn(B, 6, L, device=DEV)
    ks = [torch.randn(B, 6, L, device=DEV) for _ in range(7)]
    e = ode.TABLEAUS["dopri5"].floats().e
    dt, atol, rtol = 0.1, 1e-5, 1e-5

    def composed():
        a = torch.zeros(B, 6, L, dtype=torch.float64, device=DEV)
        for w, k in zip(e, ks):
            if w != 0.0:
                a = a + w * k.double()
        q = dt * a / (atol + rtol * torch.maximum(y0.abs(), y1.abs()).double())
        return (q * q).mean(dim=(1, 2)).sqrt()
    cases = {"copy (x.clone(), 2 streams)": (2.0, lambda: y0.clone()), "torch composition, fp64": (8.0, composed),
             "osuf_rk_error (8 streams read)": (8.0, lambda: ops.rk_error(y0, y1, ks, e, dt, atol, rtol))}
    times = {k: [] for k in cases}
    for _, fn in cases.values():
        fn()
    for _ in range(rounds):
        for name, (_, fn) in cases.items():
            times[name].append(wall(lambda: [fn() for _ in range(iters)]) / iters)
    diff = ((ops.rk_error(y0, y1, ks, e, dt, atol, rtol) - composed()).abs() / composed()).max().item()
    n = B * 6 * L
    lines = ["| fp32 (%d, 6, %d), S = 7 | bytes the algorithm needs | us (median) | us (min .. max) | GB/s |" % (B, L), "|---|---|---|---|---|"]
    for name, (streams, _) in cases.items():
        med = statistics.median(times[name])
        lines.append("| %s | %.2f MB | %.1f | %.1f .. %.1f | %.0f |" % (name, streams * 4 * n / 1e6, med * 1e6, min(times[name]) * 1e6, max(times[name]) * 1e6,
                                                                   streams * 4 * n / med / 1e9))
    return lines + ["", "Largest relative difference between the kernel's ratios and the composition's: %.2e." % diff, ""]


def toy_rows(steps, rtol, atol, omega=6.0):
    y0 = np.random.default_rng(0).standard_normal((2, 6, 64))
    exact = OO.rotation_exact(y0, omega, 1.0)
    times = OO.linspace(steps)
    lines = ["| y' = %g J y to t = 1, fp64 restatement, grid of %d points, rtol = atol = %g | evaluations | accepted | rejected | max distance to the closed form |"
             % (omega, steps, rtol), "|---|---|---|---|---|"]
    for method in METHODS:
        y, st = OO.solve(OO.rotation_f(omega), y0, times, method, rtol=rtol, atol=atol)
        lines.append("| %s | %d | %d | %d | %.3e |" % (method, st["evals"], st["accepted"], st["rejected"], np.abs(y - exact).max()))
    return lines + [""]


def sample_rows(backbone, B, L, cond_scale, steps, rounds, depth, rtol, atol, max_steps):
    a = torch.rand(B, 96, L, device=DEV) * 10 - 15
    c = torch.rand(B, 5, device=DEV) * 2 - 1
    x = torch.randn(B, 6, L, device=DEV)
    torch.manual_seed(0)
    model = RectifiedFlowOsuFusionDiT(512, backbone=backbone, depth=depth, sampling_timesteps=steps).to(DEV)
    with torch.no_grad():                                    # the reference zero-inits the adaLN modulations and the output: use live weights
        for p in model.parameters():
            if not p.any():
                p.normal_(0, 0.02)
    model.set_full_bf16()

    def run(method):
        return model.sample(a, c, x, cond_scale=cond_scale, method=method, rtol=rtol, atol=atol, max_steps=max_steps)
    stats, times = {}, {m: [] for m in METHODS}
    for m in METHODS:                                        # warm-up (pack caches, code objects) and the counts
        try:
            run(m)
            stats[m] = dict(model.last_ode_stats)
        except RuntimeError as err:                          # an adaptive method that does not get there in max_steps: recorded, not timed
            if "max_steps" not in str(err):
                raise
            stats[m] = None
    for _ in range(rounds):
        for m in METHODS:
            if stats[m] is not None:
                times[m].append(wall(lambda: run(m)))
    lines = ["| %s depth %d, bf16, (%d, 6, %d), guidance %g, grid of %d points, rtol = atol = %g | evaluations | accepted | rejected | s per sample() (median) | "
             "s (min .. max) | ms per evaluation |" % (backbone, depth, B, L, cond_scale, steps, rtol), "|---|---|---|---|---|---|---|"]
    for m in METHODS:
        if stats[m] is None:
            lines.append("| %s | more than %d attempted steps | | | | | |" % (m, max_steps))
            continue
        med, st = statistics.median(times[m]), stats[m]
        lines.append("| %s | %d | %d | %d | %.3f | %.3f .. %.3f | %.1f |" % (m, st["evals"], st["accepted"], st["rejected"], med, min(times[m]), max(times[m]),
                                                                         1e3 * med / st["evals"]))
    return lines + [""]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/ode_solvers.md")
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--L", type=int, default=8192)
    ap.add_argument("--cfg", type=float, default=2.0)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--backbones", default="dit,mmdit")
    ap.add_argument("--rtol", type=float, default=1e-2)
    ap.add_argument("--atol", type=float, default=1e-2)
    ap.add_argument("--max-steps", type=int, default=60)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ode.py needs an MI355X"
    lines = ["## Measured (tools/bench_ode.py)", "", "%s, torch %s, rounds %d, iters %d." % (torch.cuda.get_device_name(0), torch.__version__, args.rounds, args.iters), ""]
    lines += kernel_rows(args.B, args.L, args.rounds, args.iters)
    lines += toy_rows(args.steps, 1e-5, 1e-5)
    for backbone in args.backbones.split(","):
        lines += sample_rows(backbone, args.B, args.L, args.cfg, args.steps, args.rounds, args.depth, args.rtol, args.atol, args.max_steps)
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    old = out.read_text() if out.exists() else ""
    start = old.find(lines[0])
    if start >= 0:                                           # a document around the table: replace this section only
        end = old.find("\n## ", start + 1)
        text = old[:start] + text + (old[end:] if end >= 0 else "")
    out.write_text(text)


if __name__ == "__main__":
    main()
