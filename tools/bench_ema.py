"""What an EMA track costs inside the AdamW pass, against keeping it with a pass of its own, on the build under test.

    python tools/bench_ema.py [--out profiles/ema.md] [--n N] [--rounds 12] [--iters 5]

At the flat parameter length of the full-size UNet (dim_h = 256: the model is built on the meta device and laid out as
train.FlatParameters does, 64-element alignment) it times, over the same buffers:
  * osuf_adamw alone (28 B per parameter: p, g, m, v in; p, m, v out),
  * osuf_adamw_ema with 1, 2 and 4 tracks (8 B more per track: the track in and out),
  * the unfused baseline: osuf_adamw followed by one torch.Tensor.lerp_ per track (12 B more per track: p is read again).
Every variant is warmed up, then the variants run interleaved round by round; a round times `iters` back-to-back calls of one variant
between two device events.  A row is the median over the rounds, with min .. max.  The margin of the byte-ratio check is the largest
relative spread (max - min) / median any variant showed in this very session: a difference inside it is not a difference.
Writes the whole of --out.  A timing tool: the suite fixes no number from it."""
import argparse
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

from osufusion_amd import ops  # noqa: E402

DEV = "cuda"
HYPER = dict(lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, wd=1e-2, step=10)
D = [0.1, 0.01, 0.001, 0.0001]
TRACKS = (1, 2, 4)


def full_size_flat_length(align: int = 64) -> int:
    from osufusion_amd.models.diffusion import OsuFusion
    with torch.device("meta"):
        model = OsuFusion(256)
    return sum((p.numel() + align - 1) // align * align for p in model.parameters() if p.requires_grad)


def timed(fn, iters: int) -> float:
    """ms per call: device events around `iters` calls."""
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/ema.md")
    ap.add_argument("--n", type=int, default=None)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--iters", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ema.py needs an MI355X"
    n = args.n or full_size_flat_length()
    torch.manual_seed(0)
    p, g = torch.randn(n, device=DEV) * 0.05, torch.randn(n, device=DEV) * 1e-3
    m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    coef = torch.ones(1, device=DEV)
    ema = p.unsqueeze(0).repeat(4, 1)

    def plain():
        ops.adamw(p, g, m, v, gscale=coef, **HYPER)

    def fused(t):
        return lambda: ops.adamw_ema(p, g, m, v, gscale=coef, ema=ema[:t], d=D[:t], **HYPER)

    def unfused(t):
        def run():
            ops.adamw(p, g, m, v, gscale=coef, **HYPER)
            for j in range(t):
                ema[j].lerp_(p, D[j])
        return run

    variants = {"osuf_adamw": (28, plain)}
    for t in TRACKS:
        variants[f"osuf_adamw_ema, {t} track{'s' if t > 1 else ''}"] = (28 + 8 * t, fused(t))
    for t in TRACKS:
        variants[f"osuf_adamw + {t} x lerp_"] = (28 + 12 * t, unfused(t))
    for _, fn in variants.values():                          # warm-up of every variant: code objects, allocator
        timed(fn, 2)
    times = {k: [] for k in variants}
    for _ in range(args.rounds):                             # interleaved: every variant once per round
        for name, (_, fn) in variants.items():
            times[name].append(timed(fn, args.iters))
    assert torch.isfinite(p).all() and torch.isfinite(ema).all()

    med = {k: statistics.median(ts) for k, ts in times.items()}
    spread = {k: (max(ts) - min(ts)) / med[k] for k, ts in times.items()}
    margin = max(spread.values())
    lines = ["# EMA tracks in the AdamW pass: cost (tools/bench_ema.py)", "",
             "%s, torch %s.  n = %d fp32 parameters (the full-size UNet's flat buffer), %d rounds of %d calls per variant, interleaved; device events."
             % (torch.cuda.get_device_name(0), torch.__version__, n, args.rounds, args.iters), "",
             "Bytes per parameter: AdamW reads p, g, m, v and writes p, m, v (28 B); a fused track is read and written (8 B); an unfused track",
             "costs a second read of p as well (12 B).  A track with d = 0 would cost nothing and one with d = 1 only its write; the tracks timed",
             "here all blend.", "",
             "| variant | B / parameter | ms (median) | ms (min .. max) | spread | TB/s | time / osuf_adamw | bytes / osuf_adamw |", "|---|---|---|---|---|---|---|---|"]
    base = med["osuf_adamw"]
    for name, (nbytes, _) in variants.items():
        ts = times[name]
        lines.append("| %s | %d | %.3f | %.3f .. %.3f | %.1f %% | %.2f | %.3f | %.3f |"
                     % (name, nbytes, med[name], min(ts), max(ts), 100 * spread[name], nbytes * n / med[name] / 1e9, med[name] / base, nbytes / 28))
    lines += ["", "Margin: %.1f %%, the largest (max - min) / median over the rounds of any variant above: two medians closer than that are not told" % (100 * margin),
              "apart by this run.", "",
              "| tracks | fused <= unfused (medians) | fused / osuf_adamw <= byte ratio x (1 + margin) |", "|---|---|---|"]
    ok = True
    for t in TRACKS:
        f, u = med[f"osuf_adamw_ema, {t} track{'s' if t > 1 else ''}"], med[f"osuf_adamw + {t} x lerp_"]
        ratio, allowed = f / base, (28 + 8 * t) / 28 * (1 + margin)
        a, b = f <= u, ratio <= allowed
        ok = ok and a and b
        lines.append("| %d | %s: %.3f vs %.3f ms (%.2fx) | %s: %.3f vs %.3f |" % (t, "yes" if a else "NO", f, u, u / f, "yes" if b else "NO", ratio, allowed))
    lines += ["", "Both conditions hold for every track count." if ok else "A condition above does NOT hold."]
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(text)


if __name__ == "__main__":
    main()
