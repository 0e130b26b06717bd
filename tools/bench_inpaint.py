"""What masked generation costs, on the build under test: the blend alone, a masked against an unmasked sample(), and RePaint resampling.

    python tools/bench_inpaint.py [--out profiles/inpaint.md] [--B 16] [--L 8192] [--cfg 2.0] [--rounds 3] [--iters 50] [--backbone mmdit]
                                  [--depth 12]

Blend rows (fp32 (B, 6, L), half-length per-sample mask), each the median over `rounds` of (host clock around `iters` launches ending in a
device synchronise) / iters, after a warm-up: copy (x.clone(), one stream read and one written: the yardstick), the level blend (x, known,
noise and the mask read, one stream written), the exact blend (x, known, mask read), and the level blend in place.  GB/s = (streams read +
written) * 4 B * elements / time, the mask counted as 1 / 6 of a stream.
Sample rows: seconds per sample() of ContinuousDiffusionOsuFusionDiT in bf16 compute (median, min, max over the rounds, interleaved round
by round): "dpmpp_2m" at 16 steps without and with the mask, "ddpm" at 35 steps with the mask at resample 1 and 3, and the denoiser calls
each makes.  The tables are written as markdown to --out; where that file already has the "## Measured" section (profiles/inpaint.md, with
its reading of the numbers around it) only that section is replaced.  A timing tool, not a gate."""
import argparse
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
# name, sampler, steps, masked, resample
SAMPLE_CASES = (("2m unmasked", "dpmpp_2m", 16, False, 1), ("2m masked", "dpmpp_2m", 16, True, 1), ("ddpm masked r=1", "ddpm", 35, True, 1),
                ("ddpm masked r=3", "ddpm", 35, True, 3))


def wall(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def half_mask(B, L):
    keep = torch.zeros(B, L, dtype=torch.bool, device=DEV)
    keep[:, : L // 2] = True
    return keep


def blend_rows(B, L, rounds, iters):
    n = B * 6 * L
    x, known, noise = (torch.randn(B, 6, L, device=DEV) for _ in range(3))
    mask = half_mask(B, L).float()
    coef = torch.rand(B, 13, device=DEV)
    scratch = x.clone()
    cases = {
        "copy": (2.0, lambda: x.clone()),
        "level blend": (4.0 + 1 / 6, lambda: ops.inpaint_blend(x, known, mask, coef, 4, 5, noise)),
        "exact blend": (3.0 + 1 / 6, lambda: ops.inpaint_blend(x, known, mask)),
        "level blend in place": (4.0 + 1 / 6, lambda: ops.inpaint_blend(scratch, known, mask, coef, 4, 5, noise, out=scratch)),
    }
    times = {k: [] for k in cases}
    for _, fn in cases.values():
        fn()
    for _ in range(rounds):
        for name, (_, fn) in cases.items():
            times[name].append(wall(lambda: [fn() for _ in range(iters)]) / iters)
    lines = ["| blend, fp32 (%d, 6, %d) | us (median) | us (min .. max) | GB/s |" % (B, L), "|---|---|---|---|"]
    for name, (streams, _) in cases.items():
        med = statistics.median(times[name])
        lines.append("| %s | %.1f | %.1f .. %.1f | %.0f |" % (name, med * 1e6, min(times[name]) * 1e6, max(times[name]) * 1e6, streams * 4 * n / med / 1e9))
    lines.append("")
    lines.append("One operand is %.2f MB; the launches are timed back to back from the host, so a time near the copy's is launch-bound." % (4 * n / 1e6))
    return lines


def sample_rows(backbone, B, L, cond_scale, rounds, depth):
    a = torch.rand(B, 96, L, device=DEV) * 10 - 15
    c = torch.rand(B, 5, device=DEV) * 2 - 1
    x = torch.randn(B, 6, L, device=DEV)
    known = torch.tanh(torch.randn(B, 6, L, device=DEV))
    keep = half_mask(B, L)
    torch.manual_seed(0)
    model = ContinuousDiffusionOsuFusionDiT(512, backbone=backbone, depth=depth).to(DEV)
    with torch.no_grad():                                    # the reference zero-inits the adaLN modulations and the output: use live weights
        for p in model.parameters():
            if not p.any():
                p.normal_(0, 0.02)
    model.set_full_bf16()
    calls = []
    denoiser = model._denoiser

    def counting(a_, c_, cfg):
        f = denoiser(a_, c_, cfg)

        def g(x_, t_):
            calls.append(1)
            return f(x_, t_)
        return g
    model._denoiser = counting

    def run(_, sampler, steps, masked, resample):
        model.sampler = sampler
        model.sampling_timesteps = model.scheduler.timesteps = steps
        torch.manual_seed(1)
        kw = dict(known=known, known_mask=keep, resample=resample) if masked else {}
        return model.sample(a, c, x, cond_scale=cond_scale, **kw)

    model.stop_after = 2
    for case in SAMPLE_CASES:                                # warm-up (pack caches, code objects): two steps of each
        run(*case)
    model.stop_after = None
    times = {case: [] for case in SAMPLE_CASES}
    ncalls = {}
    for _ in range(rounds):
        for case in SAMPLE_CASES:
            calls.clear()
            times[case].append(wall(lambda: run(*case)))
            ncalls[case] = len(calls)
    lines = ["| sample(), %s depth %d, bf16, (%d, 6, %d), guidance %g | steps | denoiser calls | s (median) | s (min .. max) | ms per call |"
             % (backbone, depth, B, L, cond_scale), "|---|---|---|---|---|---|"]
    for case, ts in times.items():
        med = statistics.median(ts)
        lines.append("| %s | %d | %d | %.3f | %.3f .. %.3f | %.2f |" % (case[0], case[2], ncalls[case], med, min(ts), max(ts), med / ncalls[case] * 1e3))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/inpaint.md")
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--L", type=int, default=8192)
    ap.add_argument("--cfg", type=float, default=2.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--backbone", default="mmdit")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_inpaint.py needs an MI355X"
    lines = ["## Measured (tools/bench_inpaint.py)", "", "%s, torch %s, rounds %d, iters %d." % (torch.cuda.get_device_name(0), torch.__version__, args.rounds, args.iters), ""]
    lines += blend_rows(args.B, args.L, args.rounds, args.iters) + [""]
    lines += sample_rows(args.backbone, args.B, args.L, args.cfg, args.rounds, args.depth)
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
