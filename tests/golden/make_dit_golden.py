#!/usr/bin/env python3
"""Golden vectors of the DiT backbone.  Runs ONLY in the build container, next to the reference:

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=/path/to/reference:. python3 tests/golden/make_dit_golden.py

It imports the reference's osu_fusion.modules.dit (nothing is copied), applies make_golden's Attend shim, fills every parameter with
osufusion_amd.pattern.param_pattern (the reference zero-inits the adaLN / final modulation and the postprocess, which would zero every
gradient) and stores, per config, dit_<name>.npz (fp32) and dit_<name>_autocast.npz (torch.autocast("cpu", bfloat16)):
y_cond, y_null (cond_drop_prob=1), the MSE loss against the synthetic noise, per-parameter gradient norms and the first 16 values of
every gradient, plus the autocast run's distances from the fp32 one.  Also state_dict_dit.json: names and shapes at the defaults.
"""
from __future__ import annotations

import contextlib
import json
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))

from osufusion_amd.pattern import param_pattern, synth_inputs  # noqa: E402
from tests.golden.make_golden import shim_attend  # noqa: E402

from osu_fusion.modules import dit as ref_dit  # noqa: E402  (reference, PYTHONPATH)

torch.manual_seed(0)

# (the stem splits its output as 102 // 2, 102 // 4 and the rest (dit.py:40-41), so dim_h must exceed 76: the smallest config is 96 wide)
CASES = {
    "dit_h96": dict(dim_h=96, attn_heads=6, attn_dim_head=16, depth=2, attn_qk_norm=True, B=2, L=200),
    "dit_h128": dict(dim_h=128, attn_heads=2, attn_dim_head=64, depth=2, attn_qk_norm=True, B=2, L=1000),
    "dit_h256_nonorm": dict(dim_h=256, attn_heads=8, attn_dim_head=32, depth=2, attn_qk_norm=False, B=2, L=96),
}


def build(cfg):
    kw = {k: v for k, v in cfg.items() if k not in ("B", "L", "dim_h")}
    net = shim_attend(ref_dit.DiT(6, 96, 5, cfg["dim_h"], **kw))
    sd = net.state_dict()
    net.load_state_dict({k: torch.from_numpy(param_pattern(k, tuple(v.shape)).copy()) for k, v in sd.items()})
    return net


def outputs(net, name, B, L, autocast: bool):
    x, a, c, t, noise = (torch.from_numpy(v) for v in synth_inputs(name, B, L))
    ctx = (lambda: torch.autocast("cpu", dtype=torch.bfloat16)) if autocast else contextlib.nullcontext
    net.zero_grad(set_to_none=True)
    with ctx():
        y = net(x, a, t, c, cond_drop_prob=0.0)
        loss = torch.nn.functional.mse_loss(y.float(), noise)
    loss.backward()
    with ctx(), torch.no_grad():                           # (its own autocast region: a weight cast cached under no_grad has no graph)
        y_null = net(x, a, t, c, cond_drop_prob=1.0).float()
    grads = {k: p.grad.detach().float().clone() for k, p in net.named_parameters()}
    return y.detach().float(), y_null, loss.detach(), grads


def rel(a, b):
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def main() -> None:
    meta = {}
    for name, cfg in CASES.items():
        net = build(cfg)
        B, L = cfg["B"], cfg["L"]
        names = [k for k, _ in net.named_parameters()]
        res = {}
        for ac in (False, True):
            y, yn, loss, g = outputs(net, name, B, L, ac)
            res[ac] = (y, yn, loss, g)
            arrays = dict(y_cond=y.numpy(), y_null=yn.numpy(), loss=loss.numpy(),
                          grad_norm=np.array([g[k].norm().item() for k in names], dtype=np.float64),
                          grad_head=np.stack([np.pad(g[k].flatten()[:16].numpy(), (0, max(0, 16 - g[k].numel()))) for k in names]))
            if ac:
                y32, yn32, l32, g32 = res[False]
                arrays.update(out_dist=rel(y, y32), null_dist=rel(yn, yn32), loss_fp32=l32.numpy(),
                              grad_dist=np.array([rel(g[k], g32[k]) for k in names], dtype=np.float64),
                              flat_grad_dist=rel(torch.cat([g[k].flatten() for k in names]), torch.cat([g32[k].flatten() for k in names])))
            fn = HERE / f"{name}{'_autocast' if ac else ''}.npz"
            np.savez_compressed(fn, **arrays)
            print(f"  wrote {fn.name} ({fn.stat().st_size / 1024:.1f} KiB)")
        meta[name] = dict(cfg, param_names=names)
    (HERE / "dit_cases.json").write_text(json.dumps(meta, indent=1) + "\n")
    sd = ref_dit.DiT(6, 96, 5, 512).state_dict()
    (HERE / "state_dict_dit.json").write_text(json.dumps({k: list(v.shape) for k, v in sd.items()}, indent=0) + "\n")


if __name__ == "__main__":
    main()
