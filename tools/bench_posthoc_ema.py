"""What the post-hoc EMA sum costs on the GPU, and what the fp64 oracle says about its quality (osufusion_amd/posthoc_ema.py).

    python tools/bench_posthoc_ema.py [--out profiles/posthoc_ema.md] [--n N] [--rounds 12] [--iters 3]

At the flat parameter length of the full-size UNet it times osuf_lincomb with K = 8 sources in its two forms,
  * accumulate: eight fp32 sources into the fp64 accumulator that is carried on (read and written):   4 K + 8 + 8 bytes per element,
  * final:      eight fp32 sources, the accumulator read, the fp32 result written (the accumulator too: the form reconstruct() launches,
                4 K + 8 + 8 + 4 bytes; and without the accumulator write, 4 K + 8 + 4),
against the same sum as a chain of torch `acc.add_(src, alpha=w)` on an fp64 buffer (per source: the source read, the accumulator read
and written, 20 bytes if torch converts on the fly) followed by one `.float()`.  Every variant is warmed up, then the variants run
interleaved round by round in this one process; a round times `iters` calls between two device events; a row is the median over the rounds
with min .. max.  The host-side section repeats the oracle's end-to-end condition (tests/posthoc_ema_oracle.py) and records its ratio.
Writes the whole of --out.  A timing tool: the suite fixes no number from it."""
import argparse
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from osufusion_amd import ops  # noqa: E402
from osufusion_amd.ema import sigma_rel_to_gamma  # noqa: E402
from osufusion_amd.posthoc_ema import solve_weights  # noqa: E402

DEV = "cuda"
K = 8


def full_size_flat_length(align: int = 64) -> int:
    from osufusion_amd.models.diffusion import OsuFusion
    with torch.device("meta"):
        model = OsuFusion(256)
    return sum((p.numel() + align - 1) // align * align for p in model.parameters() if p.requires_grad)


def timed(fn, iters: int) -> float:
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / iters


def oracle_lines():
    from tests import posthoc_ema_oracle as O
    g_stored = [sigma_rel_to_gamma(s) for s in O.SIGMA_STORED]
    g_target = sigma_rel_to_gamma(O.SIGMA_TARGET)
    _, snaps, target = O.end_to_end(g_stored, g_target)
    steps = sorted(snaps)
    x = solve_weights(np.repeat(steps, 2), np.tile(g_stored, len(steps)), O.T, g_target)
    recon = x @ np.concatenate([snaps[s] for s in steps])
    d = np.linalg.norm(recon - target)
    dt = [np.linalg.norm(snaps[O.T][g] - target) for g in range(2)]
    return ["## Reconstruction quality on the fp64 oracle (host only)", "",
            "Random walk in %d dimensions, %d steps, seed %d; tracks at sigma_rel %s stored every %d steps; target sigma_rel %s at step %d,"
            % (O.DIM, O.T, O.SEED, " and ".join(map(str, O.SIGMA_STORED)), O.EVERY, O.SIGMA_TARGET, O.T),
            "computed directly by the recurrence.  Distances are Euclidean, to the direct target.", "",
            "| | distance |", "|---|---|", "| reconstruction from %d stored tracks | %.4e |" % (len(x), d),
            "| stored track sigma_rel %s at step %d | %.4e |" % (O.SIGMA_STORED[0], O.T, dt[0]),
            "| stored track sigma_rel %s at step %d | %.4e |" % (O.SIGMA_STORED[1], O.T, dt[1]), "",
            "Ratio of the reconstruction's distance to the nearer stored track's: %.4e.  Weights %+.4f .. %+.4f, sum %.6f."
            % (d / min(dt), x.min(), x.max(), x.sum()), ""]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/posthoc_ema.md")
    ap.add_argument("--n", type=int, default=None)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--iters", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_posthoc_ema.py needs an MI355X"
    n = args.n or full_size_flat_length()
    torch.manual_seed(0)
    srcs = [torch.randn(n, device=DEV) * 0.05 for _ in range(K)]
    w = [(-1.0) ** k * (0.3 + 0.4 * k) for k in range(K)]             # alternating sign, beyond 1 in magnitude
    acc = torch.zeros(n, dtype=torch.float64, device=DEV)
    out = torch.empty(n, device=DEV)
    acc_t = torch.zeros(n, dtype=torch.float64, device=DEV)

    def torch_chain():
        acc_t.zero_()
        for s, wk in zip(srcs, w):
            acc_t.add_(s, alpha=wk)
        return acc_t.float()

    variants = {
        "osuf_lincomb K=8, accumulate (acc in, acc out)": (4 * K + 16, lambda: ops.lincomb(srcs, w, acc=acc, cont=True)),
        "osuf_lincomb K=8, final (acc in, acc and out written)": (4 * K + 20, lambda: ops.lincomb(srcs, w, acc=acc, out=out, cont=True)),
        "osuf_lincomb K=8, first (acc out only)": (4 * K + 8, lambda: ops.lincomb(srcs, w, acc=acc)),
        "osuf_lincomb K=8, single launch (out only)": (4 * K + 4, lambda: ops.lincomb(srcs, w, out=out)),
        "torch: zero_, 8 x add_(src, alpha=w) on fp64, .float()": (8 + 20 * K + 12, torch_chain),
    }
    for _, fn in variants.values():
        timed(fn, 2)
    # the same numbers from both, before any is timed: one launch from zero against the torch chain
    ops.lincomb(srcs, w, acc=acc, out=out)
    ref = torch_chain()
    gap = (out.double() - ref.double()).abs().max().item()
    acc.zero_()
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for name, (_, fn) in variants.items():
            times[name].append(timed(fn, args.iters))
        acc.zero_()                                                   # the accumulate form would otherwise grow without bound
    med = {k: statistics.median(ts) for k, ts in times.items()}
    base = med["torch: zero_, 8 x add_(src, alpha=w) on fp64, .float()"]
    lines = ["# Post-hoc EMA: the cost of the sum and the quality of the reconstruction (tools/bench_posthoc_ema.py)", "",
             "%s, torch %s.  n = %d fp32 elements per source (the full-size UNet's flat buffer), K = %d sources, %d rounds of %d calls per"
             % (torch.cuda.get_device_name(0), torch.__version__, n, K, args.rounds, args.iters),
             "variant, interleaved in one process; device events.  Largest difference between the fp32 results of one launch and of the torch",
             "chain on the same inputs: %.3e." % gap, "",
             "| variant | B / element | ms (median) | ms (min .. max) | GB/s | time / torch chain |", "|---|---|---|---|---|---|"]
    for name, (nbytes, _) in variants.items():
        ts = times[name]
        lines.append("| %s | %d | %.3f | %.3f .. %.3f | %.0f | %.3f |" % (name, nbytes, med[name], min(ts), max(ts), nbytes * n / med[name] / 1e6, med[name] / base))
    a = med["osuf_lincomb K=8, accumulate (acc in, acc out)"]
    lines += ["", "Expectation stated before any run: one pass over K sources costs about the bytes of K + 4 fp32 buffers (4 K + 16 B per element),",
              "the torch chain about 5 K (20 K B).  Byte ratio (4 K + 16) / (8 + 20 K + 12) = %.3f; measured time ratio, accumulate form against the"
              % ((4 * K + 16) / (8 + 20 * K + 12)),
              "torch chain: %.3f." % (a / base), ""]
    lines += oracle_lines()
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    out_path = Path(args.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(text)


if __name__ == "__main__":
    main()
