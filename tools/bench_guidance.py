"""What the guidance controls cost and save, on the build under test: one ops.cfg_rescale beside one denoiser call, and DDIM steps per second
with full guidance against a guidance interval that guides half the calls.

    python tools/bench_guidance.py [--out profiles/guidance.md] [--B 16] [--L 8192] [--cfg 2.0] [--steps 16] [--rounds 3] [--iters 50]
                                   [--depth 12] [--backbones dit,mmdit]

Per backbone (DiffusionOsuFusionDiT, dim_h 512, bf16 compute, live weights): the rescale as the median over `rounds` of (host clock around
`iters` launches ending in a device synchronise) / iters after a warm-up, with its byte count 5 B per_sample 4 (cond and null read twice,
out written once) and the GB/s that gives; one denoiser call on 2B rows and on B rows; and sample() at the defaults -- the path of the
commit before the keywords -- against guidance_interval set to the middle half of the steps' log-SNR and against guidance_rescale = 0.7, as
steps per second (median, min .. max over the rounds, interleaved round by round).  The tables are written as markdown to --out; where that
file already has the "## Measured" section only that section is replaced.  A timing tool, not a gate."""
import argparse
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

from osufusion_amd import guidance, ops  # noqa: E402
from osufusion_amd.models import DiffusionOsuFusionDiT  # noqa: E402

DEV = "cuda"


def wall(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def rescale_rows(B, L, cond_scale, rounds, iters):
    cond, null = torch.randn(B, 6, L, device=DEV), torch.randn(B, 6, L, device=DEV)
    cases = {"copy (x.clone(), 2 streams)": (2.0, lambda: cond.clone()), "cfg_rescale (5 streams)": (5.0, lambda: ops.cfg_rescale(cond, null, cond_scale, 0.7))}
    times = {k: [] for k in cases}
    for _, fn in cases.values():
        fn()
    for _ in range(rounds):
        for name, (_, fn) in cases.items():
            times[name].append(wall(lambda: [fn() for _ in range(iters)]) / iters)
    n = B * 6 * L
    lines = ["| fp32 (%d, 6, %d) | bytes | us (median) | us (min .. max) | GB/s |" % (B, L), "|---|---|---|---|---|"]
    for name, (streams, _) in cases.items():
        med = statistics.median(times[name])
        lines.append("| %s | %.2f MB | %.1f | %.1f .. %.1f | %.0f |" % (name, streams * 4 * n / 1e6, med * 1e6, min(times[name]) * 1e6, max(times[name]) * 1e6,
                                                                   streams * 4 * n / med / 1e9))
    return lines, statistics.median(times["cfg_rescale (5 streams)"])


def sample_rows(backbone, B, L, cond_scale, steps, rounds, depth, rescale_s):
    a = torch.rand(B, 96, L, device=DEV) * 10 - 15
    c = torch.rand(B, 5, device=DEV) * 2 - 1
    x = torch.randn(B, 6, L, device=DEV)
    torch.manual_seed(0)
    model = DiffusionOsuFusionDiT(512, backbone=backbone, depth=depth, sampling_timesteps=steps).to(DEV)
    with torch.no_grad():                                    # the reference zero-inits the adaLN modulations and the output: use live weights
        for p in model.parameters():
            if not p.any():
                p.normal_(0, 0.02)
    model.set_full_bf16()
    model.scheduler.set_timesteps(steps)
    ls = guidance.ddim_log_snr(model.scheduler.alphas_cumprod, model.scheduler.timesteps.tolist())
    half = (ls[steps // 4], ls[steps // 4 + steps // 2 - 1])                        # the middle half of the steps
    cases = {"full guidance (defaults)": {}, "interval, %d of %d calls guided" % (steps // 2, steps): dict(guidance_interval=half),
             "full guidance, rescale 0.7": dict(guidance_rescale=0.7)}

    def run(kw):
        torch.manual_seed(1)
        return model.sample(a, c, x, cond_scale=cond_scale, **kw)
    model.stop_after = 2
    for kw in cases.values():                                # warm-up (pack caches, code objects)
        run(kw)
    run(dict(guidance_interval=(ls[1], ls[1])))              # ... and the B-row form of the denoiser
    model.stop_after = None
    with torch.inference_mode(), ops.reproducible_mode(True), ops.one_launch_attention(True), model._dtype_ctx():
        den = model._denoiser(a, c, True)
        t = torch.full((2 * B,), 500, dtype=torch.int64, device=DEV)
        calls = {}
        for name, guided in (("2B rows", True), ("B rows", False)):
            den(x, t, guided)
            calls[name] = statistics.median(wall(lambda: den(x, t, guided)) for _ in range(rounds))
    times = {k: [] for k in cases}
    for _ in range(rounds):
        for name, kw in cases.items():
            times[name].append(wall(lambda: run(kw)))
    lines = ["| %s depth %d, bf16, (%d, 6, %d), guidance %g | ms |" % (backbone, depth, B, L, cond_scale), "|---|---|"]
    lines += ["| one denoiser call, %s | %.2f |" % (k, v * 1e3) for k, v in calls.items()]
    lines += ["| one ops.cfg_rescale | %.3f (%.2f %% of the 2B-row call) |" % (rescale_s * 1e3, 100 * rescale_s / calls["2B rows"]), ""]
    lines += ["| DDIM sample(), %d steps | steps/s (median) | steps/s (min .. max) | s per sample() |" % steps, "|---|---|---|---|"]
    for name, ts in times.items():
        med = statistics.median(ts)
        lines.append("| %s | %.2f | %.2f .. %.2f | %.3f |" % (name, steps / med, steps / max(ts), steps / min(ts), med))
    return lines + [""]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/guidance.md")
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--L", type=int, default=8192)
    ap.add_argument("--cfg", type=float, default=2.0)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--backbones", default="dit,mmdit")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_guidance.py needs an MI355X"
    lines = ["## Measured (tools/bench_guidance.py)", "", "%s, torch %s, rounds %d, iters %d." % (torch.cuda.get_device_name(0), torch.__version__, args.rounds, args.iters), ""]
    rows, rescale_s = rescale_rows(args.B, args.L, args.cfg, args.rounds, args.iters)
    lines += rows + [""]
    for backbone in args.backbones.split(","):
        lines += sample_rows(backbone, args.B, args.L, args.cfg, args.steps, args.rounds, args.depth, rescale_s)
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
