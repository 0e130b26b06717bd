#!/usr/bin/env python3
"""The sampling step kernels and the three transformer diffusion samplers, bit for bit: the record that a refactor of either is held to.

    PYTHONPATH=/path/to/a/build/of/the/recorded/commit:. python3 tests/golden/make_sampling_bits_golden.py

Run once on the MI355X against a build of the commit whose bits are to be kept (the parent of the commit that folded the two step kernels
and the three sampling loops into one); it writes tests/golden/sampling_bits.npz.  Only API that both sides of that fold have is used:
ops.ct_schedule, ops.ct_solver_schedule, ops.ct_step, ops.ct_step_ex, ops.ct_solver_step and the three models' sample().
tests/test_sampling_bits_gpu.py recomputes every case through the functions below and compares the integer views.

Kernel cases.  Inputs come from a seeded CPU generator and are copied to the device; the predictions are 3 N(0, 1) and the guidance scale
is 7, so the start prediction lies far outside [-1, 1] for most elements and inside for some: the static clamp and the threshold clamp
both act and both pass values through.  Shapes, the smallest at which the step kernel's skeleton can still go wrong:
  * straddle: B = 3, per_sample = 54 = 6 x 9 -- the group of four at elements 52..55 holds two samples, total = 162 leaves a tail of 2;
  * vec:      B = 2, per_sample = 64 -- no straddle, no tail;
  * scalar:   the straddle shape with every input a view one float into its buffer, so that the scalar path runs.
Ancestral step: objective x {s None, s a strided column of a (B, 3) tensor} x {null None, null given} x {noise None, noise given with a
non-zero gain column, noise given with the gain column zero (t_next = 0 rows)}; objective "noise" without s goes through ops.ct_step, the
rest through ops.ct_step_ex.  Solver step, per objective and s / no s, null given: DDIM at eta = 0; DDIM at eta = 0.5 with noise; the
first 2M step (x0_prev None); a later 2M step with x0_prev; a later DDIM(0) step handed an x0_prev (k_p == 0).  Both outputs are recorded.
The schedule rows and factors that feed them are recorded too (the solver's once, at B = 3).

Loop cases, per backbone (the smallest DiT and MMDiT of tests/test_ct_solver_gpu.py, weights from pattern.param_pattern), B = 2, n = 32,
three sampling steps, each after torch.manual_seed(SEED): DiffusionOsuFusionDiT.sample; ContinuousDiffusionOsuFusionDiT.sample for ddpm,
ddim at eta = 0.5 and dpmpp_2m; a thresholded v-objective ddpm run; a masked ddpm run with resample = 2; a dpmpp_2m run cut by
stop_after = 2.

File: `names` (newline-joined, as bytes), `sizes` (elements per name) and `bits` (every output's fp32 bits as int32, concatenated).
"""
from __future__ import annotations

from pathlib import Path

import numpy as np
import torch

from osufusion_amd import ops
from osufusion_amd.models import ContinuousDiffusionOsuFusionDiT, DiffusionOsuFusionDiT
from osufusion_amd.pattern import param_pattern, synth_inputs

PATH = Path(__file__).resolve().parent / "sampling_bits.npz"
SEED = 20260417
CFG = 7.0
OBJECTIVES = ("noise", "x_start", "v")
SHAPES = {"straddle": (3, 54, False), "vec": (2, 64, False), "scalar": (3, 54, True)}            # B, per_sample, misaligned
TIMES, TIMES_NEXT = (0.5, 0.625, 0.125), (0.375, 0.5, 0.03125)
THRESHOLDS = (1.0, 1.75, 2.5)
GRID = (-8.0, -3.0, 0.5, 3.0, 6.5)
# name: (sampler, eta, step of the grid, x0_prev given, noise given)
SOLVER_MODES = {"ddim0": ("ddim", 0.0, 1, False, False), "ddim_eta": ("ddim", 0.5, 1, False, True), "2m_first": ("dpmpp_2m", 0.0, 0, False, False),
                "2m_later": ("dpmpp_2m", 0.0, 2, True, False), "ddim0_prev": ("ddim", 0.0, 2, True, False)}
BACKBONE_KW = {"dit": dict(backbone="dit", dim_h=96, depth=2, attn_heads=6, attn_dim_head=16),
               "mmdit": dict(backbone="mmdit", dim_h=64, depth=2, attn_heads=4, attn_kv_heads=2, attn_dim_head=16)}
LOOP_B, LOOP_N, LOOP_STEPS = 2, 32, 3


def _misaligned(t: torch.Tensor) -> torch.Tensor:
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    buf[1:].copy_(t.flatten())
    return buf[1:].view(t.shape)


def _inputs(shape: str, dev):
    """x, cond, null, noise, prev (B, per_sample) and the threshold column s (B,), stride 3."""
    B, per, misalign = SHAPES[shape]
    g = torch.Generator().manual_seed(SEED + per)
    x, cond, dn, noise, prev = (torch.randn((B, per), generator=g) for _ in range(5))
    put = (lambda v: _misaligned(v.to(dev))) if misalign else (lambda v: v.to(dev))
    s3 = torch.zeros((B, 3))
    s3[:, 2] = torch.tensor(THRESHOLDS[:B])
    return put(x), put(3.0 * cond), put(3.0 * cond + 0.3 * dn), put(noise), put(torch.tanh(prev)), s3.to(dev)[:, 2]


def step_cases(dev):
    """-> (name, tensor) of the ancestral step kernel and its schedule rows."""
    for shape, (B, _, _) in SHAPES.items():
        x, cond, null, noise, _, s = _inputs(shape, dev)
        t = torch.tensor(TIMES[:B], device=dev)
        rows = {"gain": ops.ct_schedule(t, torch.tensor(TIMES_NEXT[:B], device=dev), 1), "last": ops.ct_schedule(t, torch.zeros_like(t), 1)}
        for key, row in rows.items():
            yield f"schedule/{shape}/{key}", row
        for objective in OBJECTIVES:
            for thr in (False, True):
                for guided in (False, True):
                    for nz in ("none", "gain", "last"):
                        row = rows["last" if nz == "last" else "gain"]
                        args = (x, cond, null if guided else None, CFG if guided else 1.0, row, None if nz == "none" else noise)
                        if objective == "noise" and not thr:
                            out = ops.ct_step(*args)
                        else:
                            out = ops.ct_step_ex(*args, objective, s if thr else None)
                        yield f"step/{shape}/{objective}/thr{int(thr)}/null{int(guided)}/noise_{nz}", out


def solver_cases(dev):
    """-> (name, tensor) of the solver step kernel (x_next and x0) and its schedules."""
    grid = torch.tensor(GRID, device=dev)
    for shape, (B, _, _) in SHAPES.items():
        x, cond, null, noise, prev, s = _inputs(shape, dev)
        sched = {}
        for mode, (sampler, eta, i, with_prev, with_noise) in SOLVER_MODES.items():
            if (sampler, eta) not in sched:
                sched[sampler, eta] = ops.ct_solver_schedule(grid, sampler, eta, B)
                if shape == "straddle":
                    yield f"solver_schedule/{sampler}_{eta}/rows", sched[sampler, eta][0]
                    yield f"solver_schedule/{sampler}_{eta}/fac", sched[sampler, eta][1]
            rows, fac = sched[sampler, eta]
            for objective in OBJECTIVES:
                for thr in (False, True):
                    x_next, x0 = ops.ct_solver_step(x, cond, null, CFG, rows[i], fac[i], prev if with_prev else None,
                                                    noise if with_noise else None, objective, s if thr else None)
                    yield f"solver/{shape}/{mode}/{objective}/thr{int(thr)}/x_next", x_next
                    yield f"solver/{shape}/{mode}/{objective}/thr{int(thr)}/x0", x0


def _model(cls, backbone: str, dev, **kw):
    model = cls(**BACKBONE_KW[backbone], sampling_timesteps=LOOP_STEPS, **kw)
    model.load_state_dict({k: torch.from_numpy(param_pattern(k[len("unet."):], tuple(v.shape)).copy()) for k, v in model.state_dict().items()})
    return model.to(dev)


def loop_cases(dev, backbone: str):
    """-> (name, tensor) of the samplers' results; every run draws its start iterate on the device after torch.manual_seed(SEED)."""
    known, a, c, _, _ = (torch.from_numpy(v).to(dev) for v in synth_inputs("sampling_bits_" + backbone, LOOP_B, LOOP_N))
    mask = torch.zeros(LOOP_N)
    mask[:12], mask[12:16] = 1.0, 0.5
    runs = {
        "discrete_ddim": (DiffusionOsuFusionDiT, {}, {}, None),
        "ddpm": (ContinuousDiffusionOsuFusionDiT, dict(sampler="ddpm"), {}, None),
        "ddim_eta": (ContinuousDiffusionOsuFusionDiT, dict(sampler="ddim", ddim_eta=0.5), {}, None),
        "dpmpp_2m": (ContinuousDiffusionOsuFusionDiT, dict(sampler="dpmpp_2m"), {}, None),
        "ddpm_v_thresholded": (ContinuousDiffusionOsuFusionDiT, dict(sampler="ddpm", pred_objective="v", dynamic_thresholding=True), {}, None),
        "ddpm_masked_resample2": (ContinuousDiffusionOsuFusionDiT, dict(sampler="ddpm"), dict(known=known, known_mask=mask.to(dev), resample=2), None),
        "dpmpp_2m_stop2": (ContinuousDiffusionOsuFusionDiT, dict(sampler="dpmpp_2m"), {}, 2),
    }
    for name, (cls, model_kw, sample_kw, stop_after) in runs.items():
        model = _model(cls, backbone, dev, **model_kw)
        model.stop_after = stop_after
        torch.manual_seed(SEED)
        yield f"loop/{backbone}/{name}", model.sample(a, c, **sample_kw)


def bits(t: torch.Tensor) -> torch.Tensor:
    assert t.dtype == torch.float32
    return t.contiguous().view(torch.int32).flatten().cpu()


def load():
    """-> {name: int32 array}, the recorded fixture."""
    z = np.load(PATH)
    names = bytes(z["names"]).decode().split("\n")
    ends = np.cumsum(z["sizes"])
    return {n: z["bits"][e - s:e] for n, s, e in zip(names, z["sizes"], ends)}


def main() -> None:
    assert torch.cuda.is_available(), "the recording is made on the MI355X"
    dev = "cuda"
    cases = list(step_cases(dev)) + list(solver_cases(dev)) + [c for b in BACKBONE_KW for c in loop_cases(dev, b)]
    names = [n for n, _ in cases]
    assert len(set(names)) == len(names)
    arrays = [bits(t).numpy() for _, t in cases]
    np.savez_compressed(PATH, names=np.frombuffer("\n".join(names).encode(), dtype=np.uint8), sizes=np.array([a.size for a in arrays], dtype=np.int32),
                        bits=np.concatenate(arrays))
    size = PATH.stat().st_size
    print(f"{PATH.name}: {len(names)} outputs, {sum(a.size for a in arrays)} values, {size} bytes")
    assert size < 100_000, size


if __name__ == "__main__":
    main()
