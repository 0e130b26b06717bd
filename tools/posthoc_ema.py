"""Post-hoc EMA from a snapshot directory to a model file.

    python tools/posthoc_ema.py --dir SNAPSHOTS --sigma-rel 0.075 [--at-step K] --out ema.safetensors [--base model.safetensors]

Reconstructs the power-function average of relative width --sigma-rel (or exponent --gamma) as it would stand after optimizer step
--at-step (default: the last snapshot) from the snapshots a Trainer(ema_snapshots=...) run left in --dir (osufusion_amd/posthoc_ema.py),
on the GPU, and writes it under the stored parameter names: a `.safetensors` file, or a torch file for any other suffix, which
data.load_model_sd loads (strict=False when the model has buffers or frozen parameters and no --base is given).  --base: a model file
whose entries the output starts from (buffers, frozen parameters); the reconstructed parameters replace theirs."""
import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

from osufusion_amd.posthoc_ema import SnapshotStore, reconstruct  # noqa: E402


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--dir", required=True)
    which = ap.add_mutually_exclusive_group(required=True)
    which.add_argument("--sigma-rel", type=float)
    which.add_argument("--gamma", type=float)
    ap.add_argument("--at-step", type=int, default=None)
    ap.add_argument("--out", required=True)
    ap.add_argument("--base", default=None)
    ap.add_argument("--profile", choices=("discrete", "continuous"), default="discrete")
    ap.add_argument("--max-resident", type=int, default=8)
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "the reconstruction runs on the GPU (osuf_lincomb)"
    store = SnapshotStore(args.dir)
    named, w = reconstruct(store, sigma_rel=args.sigma_rel, gamma=args.gamma, at_step=args.at_step, device="cuda", profile=args.profile,
                           max_resident=args.max_resident)
    sd = {}
    if args.base:
        if Path(args.base).suffix == ".safetensors":
            from safetensors.torch import load_file
            sd = load_file(args.base)
        else:
            sd = torch.load(args.base, map_location="cpu", weights_only=True)
            sd = sd.get("model_state_dict", sd)
        missing = [k for k in named if k not in sd]
        if missing:
            raise SystemExit(f"--base does not hold {len(missing)} of the stored parameters, e.g. {missing[0]}")
    sd.update({k: v.detach().cpu().contiguous().clone() for k, v in named.items()})
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    if out.suffix == ".safetensors":
        from safetensors.torch import save_file
        save_file(sd, str(out))
    else:
        torch.save(sd, out)
    steps = store.list()
    print(f"{out}: {len(named)} parameters from {len(w)} stored tracks (steps {steps[0]} .. {args.at_step or steps[-1]}); "
          f"weights {w.min():+.4g} .. {w.max():+.4g}, sum {w.sum():.6f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
