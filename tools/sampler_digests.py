"""Bits and launches of the samplers over a fixed list of small cases: per case the SHA-256 of the output bytes, the count of osuf_* calls by
name (a wrapper on ops.call) and, on the flow models, the counts of last_ode_stats.  Run on the commit before a change to the models layer and
again after it, the two files must be equal; tests/test_sampler_digests_gpu.py holds the tree to tests/golden/sampler_parent_digests.json.
    python tools/sampler_digests.py --out digests.json
Models are built as tests/test_inpaint_gpu.py builds them (the deterministic non-zero weight pattern: a zero-initialised output layer would
make every denoiser trivial, so each case first asserts that the backbone's prediction at the start iterate is not all zero).  Inputs come
from a seeded CPU generator; the stochastic samplers draw from the global generator, seeded per case."""
import argparse
import gc
import hashlib
import json
import sys
from collections import Counter
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch  # noqa: E402

from osufusion_amd import forced_compute_dtype, ops  # noqa: E402
from osufusion_amd.models import ContinuousDiffusionOsuFusionDiT, DiffusionOsuFusionDiT, RectifiedFlowOsuFusionDiT  # noqa: E402
from osufusion_amd.models.diffusion import OsuFusion  # noqa: E402
from osufusion_amd.models.rectified_flow import OsuFusion as FlowOsuFusion  # noqa: E402
from osufusion_amd.pattern import param_pattern  # noqa: E402

DEV = "cuda"
STEPS, B, N_TRANSFORMER = 3, 2, 96
UNET_KW = dict(dim_h_mult=(1, 2), num_layer_blocks=(1, 1), num_middle_transformers=1, cross_embed_kernel_sizes=(3,), attn_dim_head=64, attn_heads=2,
               attn_kv_heads=1, attn_context_len=256)
BACKBONE_KW = {"dit": dict(backbone="dit", dim_h=96, depth=2, attn_heads=6, attn_dim_head=16),
               "mmdit": dict(backbone="mmdit", dim_h=64, depth=2, attn_heads=4, attn_kv_heads=2, attn_dim_head=16)}
KINDS = ["unet_ddim", "unet_flow", "dit_ddim", "dit_flow", "ct_ddpm", "ct_2m"]
DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}


def build_model(kind):
    if kind == "unet_ddim":
        model = OsuFusion(32, sampling_timesteps=STEPS, **UNET_KW)
    elif kind == "unet_flow":
        model = FlowOsuFusion(32, sampling_timesteps=STEPS, **UNET_KW)
    elif kind == "dit_ddim":
        model = DiffusionOsuFusionDiT(sampling_timesteps=STEPS, **BACKBONE_KW["mmdit"])
    elif kind == "dit_flow":
        model = RectifiedFlowOsuFusionDiT(sampling_timesteps=STEPS, **BACKBONE_KW["dit"])
    else:
        model = ContinuousDiffusionOsuFusionDiT(sampling_timesteps=STEPS, sampler={"ct_ddpm": "ddpm", "ct_2m": "dpmpp_2m"}[kind], **BACKBONE_KW["mmdit"])
    model.load_state_dict({k: torch.from_numpy(param_pattern(k[len("unet."):], tuple(v.shape)).copy()) for k, v in model.state_dict().items()})
    return model.to(DEV)


def cases(kind):
    """-> [(case id, n, cond_scale, dtype name, masked, extra)]; extra: stop_after (the DDIM UNet) or method (the flow UNet)."""
    if not kind.startswith("unet"):
        return [(f"{kind}/n{N_TRANSFORMER}/cs2.0/bf16/masked", N_TRANSFORMER, 2.0, "bf16", True, {})]
    out = [(f"{kind}/n{n}/cs{cs}/{dt}/{'masked' if masked else 'plain'}", n, cs, dt, masked, {})
           for n in (256, 250) for cs in (1.0, 2.0) for dt in DTYPES for masked in (False, True)]
    if kind == "unet_ddim":
        out += [(f"{kind}/n250/cs2.0/bf16/plain/stop{s}", 250, 2.0, "bf16", False, dict(stop_after=s)) for s in (1, 0)]
    else:
        out += [(f"{kind}/n250/cs2.0/bf16/plain/{m}", 250, 2.0, "bf16", False, dict(method=m)) for m in ("euler", "rk4", "dopri5")]
    return out


def inputs(case_id, n):
    g = torch.Generator().manual_seed(int.from_bytes(hashlib.sha256(case_id.encode()).digest()[:4], "little"))
    a = (torch.randn(B, 96, n, generator=g) * 3 - 10).to(DEV)
    c = (torch.rand(B, 5, generator=g) * 2 - 1).to(DEV)
    x0 = torch.randn(B, 6, n, generator=g).to(DEV)
    known = (torch.rand(B, 6, n, generator=g) * 2 - 1).to(DEV)
    keep = torch.zeros(B, n, dtype=torch.bool, device=DEV)
    keep[:, : n // 2] = True
    return a, c, x0, known, keep


def first_prediction(kind, model, a, c, x0):
    """The backbone at the start iterate and the sampler's first time input, outside the counted call."""
    if kind.endswith("ddim"):
        model.scheduler.set_timesteps(STEPS)
        t = torch.full((B,), model.scheduler.timesteps.tolist()[0], dtype=torch.int64, device=DEV)
    elif kind.endswith("flow"):
        t = torch.zeros(B, dtype=torch.float32, device=DEV)
    else:
        t = model.scheduler.log_snr(torch.ones(B, dtype=torch.float32, device=DEV))
    with torch.inference_mode():
        return model.unet(x0, a, t, c, cond_drop_prob=0.0)


def run_case(kind, model, case):
    case_id, n, cond_scale, dt, masked, extra = case
    a, c, x0, known, keep = inputs(case_id, n)
    kw = dict(known=known, known_mask=keep) if masked else {}
    method = extra.get("method")
    if method is not None:
        kw.update(method=method, rtol=1e-3, atol=1e-3, max_steps=200)
    entry = getattr(model, "sample_masked", model.sample) if kw else model.sample
    counts = Counter()
    plain_call = ops.call

    def counting(name, *args, **kwargs):
        counts[name] += 1
        return plain_call(name, *args, **kwargs)
    with forced_compute_dtype(DTYPES[dt]):
        assert first_prediction(kind, model, a, c, x0).abs().max().item() > 0.0, f"{case_id}: the first prediction is all zero"
        torch.manual_seed(1234)
        if "stop_after" in extra:
            model.stop_after = extra["stop_after"]
        ops.call = counting
        try:
            out = entry(a, c, x0.clone(), cond_scale=cond_scale, **kw)
        finally:
            ops.call = plain_call
            if "stop_after" in extra:
                model.stop_after = None
    assert out.shape == x0.shape and out.dtype == torch.float32 and torch.isfinite(out).all(), case_id
    if extra.get("stop_after") == 0:
        assert torch.equal(out, x0), f"{case_id}: stop_after = 0 returns the start iterate's values"
    rec = dict(sha256=hashlib.sha256(out.contiguous().cpu().numpy().tobytes()).hexdigest(), calls=dict(sorted(counts.items())))
    if kind.endswith("flow"):
        rec["ode"] = {k: model.last_ode_stats[k] for k in ("evals", "accepted", "rejected")}
    return rec


def run_kind(kind):
    """-> {case id: record}.  A case that raises a host-side IndexError / ValueError is recorded as {"error": ...} instead of ending the run, so
    that a tree which cannot run a case still records the others."""
    model = build_model(kind)
    out = {}
    try:
        for case in cases(kind):
            try:
                out[case[0]] = run_case(kind, model, case)
            except (IndexError, ValueError) as e:
                out[case[0]] = dict(error=f"{type(e).__name__}: {e}")
        return out
    finally:
        del model
        gc.collect()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    result = {}
    for kind in KINDS:
        result.update(run_kind(kind))
        print(f"[digests] {kind}: {len(cases(kind))} cases", file=sys.stderr, flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1, sort_keys=True) + "\n")
