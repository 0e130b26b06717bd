#!/usr/bin/env python3
"""Golden vectors of the MMDiT backbone.  Runs ONLY in the build container, next to the reference:

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=/path/to/reference:. python3 tests/golden/make_mmdit_golden.py

It imports the reference's osu_fusion.modules.mmdit (nothing is copied), applies make_golden's Attend shim, fills every parameter with
osufusion_amd.pattern.param_pattern (the reference zero-inits the adaLN modulations, the final layer and the output convolution, which
would zero every gradient) and stores, per config, mmdit_<name>.npz (fp32) and mmdit_<name>_autocast.npz
(torch.autocast("cpu", bfloat16)) with the fields of the DiT fixtures: y_cond, y_null (cond_drop_prob=1), the MSE loss against the
synthetic noise, per-parameter gradient norms and the first 16 values of every gradient, plus the autocast run's distances from the
fp32 one.  Also mmdit_cases.json (the configs and parameter order), state_dict_mmdit.json (names and shapes at the defaults) and
mod_joint_attention.npz: one JointAttention with Na != Nx, its outputs and every input and parameter gradient.
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

from osufusion_amd.pattern import param_pattern, synth_inputs, uniform_pm  # noqa: E402
from tests.golden.make_golden import shim_attend  # noqa: E402

from osu_fusion.modules import mmdit as ref_mmdit  # noqa: E402  (reference, PYTHONPATH)

torch.manual_seed(0)

# (the reference only runs when attn_heads * attn_dim_head == dim_h: attn_out_* is Linear(dim_h, dim_h))
CASES = {
    "mmdit_h96": dict(dim_h=96, attn_heads=6, attn_kv_heads=2, attn_dim_head=16, depth=2, patch_size=4, attn_qk_norm=True, B=2, L=203),
    "mmdit_h128_mqa": dict(dim_h=128, attn_heads=2, attn_kv_heads=1, attn_dim_head=64, depth=2, patch_size=4, attn_qk_norm=True, B=2, L=512),
    "mmdit_h128_nonorm": dict(dim_h=128, attn_heads=4, attn_kv_heads=4, attn_dim_head=32, depth=1, patch_size=2, attn_qk_norm=False, B=2, L=96),
}
JOINT = dict(dim=96, dim_head=16, heads=6, kv_heads=2, B=2, Nx=40, Na=23)


def fill(net):
    sd = net.state_dict()
    net.load_state_dict({k: torch.from_numpy(param_pattern(k, tuple(v.shape)).copy()) for k, v in sd.items()})
    return net


def build(cfg):
    kw = {k: v for k, v in cfg.items() if k not in ("B", "L", "dim_h")}
    return fill(shim_attend(ref_mmdit.MMDiT(6, 96, 5, cfg["dim_h"], **kw)))


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
    # (the last block's audio stream feeds nothing: its attn_out_a / mlp_a and half of modulation_a get no gradient, recorded as zeros)
    grads = {k: (p.grad.detach().float().clone() if p.grad is not None else torch.zeros_like(p)) for k, p in net.named_parameters()}
    return y.detach().float(), y_null, loss.detach(), grads


def rel(a, b):
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def joint_attention_case() -> None:
    j = JOINT
    net = fill(shim_attend(ref_mmdit.JointAttention(j["dim"], j["dim_head"], j["heads"], j["kv_heads"])))
    x = torch.from_numpy(uniform_pm("joint/x", (j["B"], j["Nx"], j["dim"]), 1.0)).requires_grad_()
    a = torch.from_numpy(uniform_pm("joint/a", (j["B"], j["Na"], j["dim"]), 1.0)).requires_grad_()
    gx = torch.from_numpy(uniform_pm("joint/gx", (j["B"], j["Nx"], j["dim_head"] * j["heads"]), 1.0))
    ga = torch.from_numpy(uniform_pm("joint/ga", (j["B"], j["Na"], j["dim_head"] * j["heads"]), 1.0))
    out_x, out_a = net(x, a)
    ((out_x * gx).sum() + (out_a * ga).sum()).backward()
    arrays = dict(out_x=out_x.detach().numpy(), out_a=out_a.detach().numpy(), dx=x.grad.numpy(), da=a.grad.numpy())
    arrays.update({"grad/" + k: p.grad.numpy() for k, p in net.named_parameters()})
    fn = HERE / "mod_joint_attention.npz"
    np.savez_compressed(fn, **arrays)
    print(f"  wrote {fn.name} ({fn.stat().st_size / 1024:.1f} KiB)")


def main() -> None:
    meta = {"joint_attention": JOINT}
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
    (HERE / "mmdit_cases.json").write_text(json.dumps(meta, indent=1) + "\n")
    sd = ref_mmdit.MMDiT(6, 96, 5, 512).state_dict()
    (HERE / "state_dict_mmdit.json").write_text(json.dumps({k: list(v.shape) for k, v in sd.items()}, indent=0) + "\n")
    joint_attention_case()


if __name__ == "__main__":
    main()
