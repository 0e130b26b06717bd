"""DDIM steps/s of the DiT / MMDiT samplers (osufusion_amd/models/transformer_diffusion.py) against the loop a user writes without them.

    python tools/bench_dit_sampling.py [--out profiles/dit_sampling.json] [--B 16] [--L 8192] [--cfg 2.0] [--steps 4] [--rounds 5]
                                       [--backbones dit,mmdit] [--depth 12]

Both backbones at their default widths (dim_h 512: DiT 8 x 64 heads, MMDiT 8 x 64 heads on 2 K/V heads, patch 4), bf16 compute.  Rows:
  * plain: `unet.forward_with_cond_scale` (two batch-B forwards, every embedding recomputed) + `ops.ddim_step`, attention in one launch
    per K/V group -- what the tree offered before the model wrappers;
  * sample: `DiffusionOsuFusionDiT.sample` (step-independent embeddings once per call, one 2B-batched forward per step, guidance in the
    DDIM-step kernel, one attention launch per block).
The two loops run in ONE process on the same weights and inputs, interleaved round by round after a warm-up of each; a row is the median over
the rounds of (host clock around `steps` steps ending in a device synchronise) and the spread (min .. max).  `sample` includes its once-per-call
set-up, amortised over `steps`.  Launch counts per step come from ops.call (every C-ABI launch goes through it).  A timing tool, not a gate."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

from osufusion_amd import forced_compute_dtype, ops  # noqa: E402
from osufusion_amd.models import DiffusionOsuFusionDiT  # noqa: E402
from osufusion_amd.models.diffusion import DDIMSchedule  # noqa: E402

DEV = "cuda"


def plain_loop(model, a, c, x, steps, cond_scale):
    b = a.shape[0]
    sch = DDIMSchedule()
    sch.set_timesteps(model.sampling_timesteps)
    x = x.float().contiguous()
    with torch.inference_mode(), forced_compute_dtype(torch.bfloat16):
        for t in sch.timesteps.tolist()[:steps]:
            tb = torch.full((b,), t, dtype=torch.int64, device=DEV)
            pred = model.unet.forward_with_cond_scale(x, a, tb, c, cond_scale=cond_scale).contiguous()
            coef = torch.tensor([sch.step_coefficients(t)] * b, dtype=torch.float32, device=DEV)
            x = ops.ddim_step(x, pred, None, 1.0, coef)
    return x


class LaunchCounter:
    """Counts the C-ABI launches by name while active (wraps ops.call)."""

    def __enter__(self):
        self.counts, self._orig = {}, ops.call

        def counting(name, *args, **kw):
            self.counts[name] = self.counts.get(name, 0) + 1
            return self._orig(name, *args, **kw)
        ops.call = counting
        return self

    def __exit__(self, *exc):
        ops.call = self._orig
        return False


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
    ap.add_argument("--cfg", type=float, default=2.0)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--backbones", default="dit,mmdit")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_dit_sampling.py needs an MI355X"
    B, L, S = args.B, args.L, args.steps
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "B": B, "L": L, "cfg": args.cfg, "dtype": "bf16",
           "steps_per_window": S, "rounds": args.rounds, "rows": []}
    for backbone in args.backbones.split(","):
        torch.manual_seed(0)
        model = DiffusionOsuFusionDiT(512, backbone=backbone, depth=args.depth, sampling_timesteps=35).to(DEV)
        with torch.no_grad():                                # the reference zero-inits the adaLN modulations and the output: use live weights
            for p in model.parameters():
                if not p.any():
                    p.normal_(0, 0.02)
        model.set_full_bf16()
        model.stop_after = S
        a = torch.rand(B, 96, L, device=DEV) * 10 - 15
        c = torch.rand(B, 5, device=DEV) * 2 - 1
        x = torch.randn(B, 6, L, device=DEV)
        loops = {"plain": lambda: plain_loop(model, a, c, x, S, args.cfg), "sample": lambda: model.sample(a, c, x, cond_scale=args.cfg)}
        outs, launches = {}, {}
        for name, fn in loops.items():                       # warm-up (pack caches, code objects) + launch counts of one window
            fn()
            with LaunchCounter() as lc:
                outs[name] = fn()
            launches[name] = lc.counts
        diff = ((outs["sample"] - outs["plain"]).norm() / outs["plain"].norm()).item()
        times = {name: [] for name in loops}
        for _ in range(args.rounds):                         # interleaved: plain, sample, plain, sample, ...
            for name, fn in loops.items():
                times[name].append(wall(fn))
        for name in loops:
            med = statistics.median(times[name])
            n = launches[name]
            row = {"backbone": backbone, "loop": name, "steps_per_s": round(S / med, 3), "ms_per_step": round(med / S * 1e3, 2),
                   "ms_per_step_min_max": [round(min(times[name]) / S * 1e3, 2), round(max(times[name]) / S * 1e3, 2)],
                   "launches_per_step": round(sum(n.values()) / S, 1),
                   "attention_fwd_launches_per_step": round((n.get("osuf_mqa_fwd", 0) + n.get("osuf_gqa_fwd", 0)) / S, 1),
                   "rel_l2_vs_plain_after_window": diff if name == "sample" else 0.0}
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
        del model
        torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
