"""What windowed sampling costs against handing the whole song to the backbone, on the build under test.

    python tools/bench_windowed.py [--out profiles/windowed.md] [--B 1] [--L 32768] [--window 4096] [--stride 3072] [--cfg 2.0] [--steps 4]
                                   [--rounds 5] [--iters 50] [--backbones dit,mmdit] [--depth 12] [--window-batch N]

Step rows: both backbones at the sizes of tools/bench_dit_sampling.py (dim_h 512: DiT 8 x 64 heads, MMDiT 8 x 64 heads on 2 K/V heads, patch
4; depth 12, bf16 compute), DiffusionOsuFusionDiT.sample cut to `steps` steps, once with window=None (the whole song as one sequence: the
sampler as it was before the window keywords, launch for launch) and once with window / window_stride.  The two run in one process on the
same weights and inputs, interleaved round by round after a warm-up of each; a row is the median over the rounds of (host clock around
`steps` steps ending in a device synchronise) / steps and the spread (min .. max).  Both include their once-per-call set-up, amortised
over `steps`.  Kernel rows: ops.window_gather of the iterate (D = 6) and of the audio (D = 96) and ops.window_fuse of the guided
prediction (R = 2 B), each the median over `rounds` of (host clock around `iters` launches ending in a synchronise) / iters, next to a
copy of the output's size; GB/s counts the bytes read and written.  The tables are written as markdown to --out; where that file already
has the "## Measured" section only that section is replaced.  A timing tool, not a gate: it fixes no number."""
import argparse
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

from osufusion_amd import ops, windowed  # noqa: E402
from osufusion_amd.models import DiffusionOsuFusionDiT  # noqa: E402

DEV = "cuda"


def wall(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def kernel_rows(B, L, window, stride, rounds, iters):
    W = len(windowed.window_starts(L, window, stride))
    x, a = torch.randn(B, 6, L, device=DEV), torch.randn(B, 96, L, device=DEV)
    pred = torch.randn(2 * B * W, 6, window, device=DEV)
    weight = windowed.window_weight(window, stride).to(DEV)
    x_w, a_w, fused = ops.window_gather(x, window, stride), ops.window_gather(a, window, stride), ops.window_fuse(pred, weight, L, stride)
    # name -> (bytes read + written, launch)
    cases = {
        "copy of the iterate's windows": (2 * x_w.numel() * 4, lambda: x_w.clone()),
        "window_gather, iterate (D = 6)": (2 * x_w.numel() * 4, lambda: ops.window_gather(x, window, stride, out=x_w)),
        "window_gather, audio (D = 96)": (2 * a_w.numel() * 4, lambda: ops.window_gather(a, window, stride, out=a_w)),
        "window_fuse, guided prediction (R = 2 B)": ((pred.numel() + fused.numel()) * 4, lambda: ops.window_fuse(pred, weight, L, stride, out=fused)),
    }
    times = {k: [] for k in cases}
    for _, fn in cases.values():
        fn()
    for _ in range(rounds):
        for name, (_, fn) in cases.items():
            times[name].append(wall(lambda: [fn() for _ in range(iters)]) / iters)
    lines = ["| kernel, B = %d, n = %d, window %d, stride %d (%d windows) | MB moved | us (median) | us (min .. max) | GB/s |" % (B, L, window, stride, W),
             "|---|---|---|---|---|"]
    for name, (nbytes, _) in cases.items():
        med = statistics.median(times[name])
        lines.append("| %s | %.2f | %.1f | %.1f .. %.1f | %.0f |" % (name, nbytes / 1e6, med * 1e6, min(times[name]) * 1e6, max(times[name]) * 1e6, nbytes / med / 1e9))
    lines += ["", "The launches are timed back to back from the host, so a time near the copy's is launch-bound."]
    return lines


def step_rows(backbone, B, L, window, stride, window_batch, cond_scale, steps, rounds, depth):
    torch.manual_seed(0)
    model = DiffusionOsuFusionDiT(512, backbone=backbone, depth=depth, sampling_timesteps=35).to(DEV)
    with torch.no_grad():                                    # the reference zero-inits the adaLN modulations and the output: use live weights
        for p in model.parameters():
            if not p.any():
                p.normal_(0, 0.02)
    model.set_full_bf16()
    model.stop_after = steps
    a = torch.rand(B, 96, L, device=DEV) * 10 - 15
    c = torch.rand(B, 5, device=DEV) * 2 - 1
    x = torch.randn(B, 6, L, device=DEV)
    loops = {"whole song": lambda: model.sample(a, c, x, cond_scale=cond_scale),
             "windowed": lambda: model.sample(a, c, x, cond_scale=cond_scale, window=window, window_stride=stride, window_batch=window_batch)}
    for fn in loops.values():                                # warm-up (pack caches, code objects) of every shape the timed rounds use
        assert torch.isfinite(fn()).all()
    times = {name: [] for name in loops}
    for _ in range(rounds):                                  # interleaved: whole, windowed, whole, windowed, ...
        for name, fn in loops.items():
            times[name].append(wall(fn))
    lines = []
    for name, ts in times.items():
        med = statistics.median(ts)
        lines.append("| %s depth %d | %s | %.2f | %.2f .. %.2f |" % (backbone, depth, name, med / steps * 1e3, min(ts) / steps * 1e3, max(ts) / steps * 1e3))
    del model
    torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/windowed.md")
    ap.add_argument("--B", type=int, default=1)
    ap.add_argument("--L", type=int, default=32768)
    ap.add_argument("--window", type=int, default=4096)
    ap.add_argument("--stride", type=int, default=3072)
    ap.add_argument("--window-batch", type=int, default=None)
    ap.add_argument("--cfg", type=float, default=2.0)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--backbones", default="dit,mmdit")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_windowed.py needs an MI355X"
    lines = ["## Measured (tools/bench_windowed.py)", "",
             "%s, torch %s, rounds %d, %d steps per round, iters %d." % (torch.cuda.get_device_name(0), torch.__version__, args.rounds, args.steps, args.iters), ""]
    lines += kernel_rows(args.B, args.L, args.window, args.stride, args.rounds, args.iters) + [""]
    lines += ["| DiffusionOsuFusionDiT.sample, bf16, (%d, 6, %d), guidance %g, window %d, stride %d, window_batch %s | loop | ms per step (median) | ms per step (min .. max) |"
              % (args.B, args.L, args.cfg, args.window, args.stride, args.window_batch), "|---|---|---|---|"]
    for backbone in args.backbones.split(","):
        lines += step_rows(backbone, args.B, args.L, args.window, args.stride, args.window_batch, args.cfg, args.steps, args.rounds, args.depth)
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
