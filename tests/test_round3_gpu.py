"""GPU tests added in round 3 (run with -m gpu on an MI355X), all through the C ABI:
  * cached GEMM operand packs never go stale across optimizer steps when derived weights were packed under no_grad
    (reentrant activation checkpointing, trainer.py:229; a sample() between two train steps, trainer.py:344-356);
  * a ResidualBlock applied twice in one forward (residual.py:118-137) completes its FiLM gradient once, after both uses.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import osufusion_amd as oa
    from osufusion_amd import functional as Fn
    from osufusion_amd import ops

from tests.test_hip_parity import DEV, T, forcing, load_pattern, rell2, report  # noqa: F401  (forcing: a fixture)

_TINY = dict(dim_h_mult=(1, 2), num_layer_blocks=(2, 2), num_middle_transformers=1, cross_embed_kernel_sizes=(3,), attn_dim_head=64,
             attn_context_len=512)


def _fresh_copy(model, kw):
    """A new model object (empty pack caches) holding the same parameter values."""
    from osufusion_amd.models.diffusion import OsuFusion
    twin = OsuFusion(32, **kw).to(DEV)
    twin.load_state_dict({k: v.detach().clone() for k, v in model.state_dict().items()})
    return twin


@pytest.mark.parametrize("heads,kv_heads", [(2, 1), (4, 2)])
@pytest.mark.parametrize("scenario", ["checkpointing", "sample_between_steps"])
def test_packs_follow_the_weights_after_no_grad_forwards(heads, kv_heads, scenario):
    """under no_grad every tensor DERIVED from parameters (merged CrossEmbed stem, Parallel's c3 + pad(c1), the
    padded final_conv, the GQA-permuted to_q / to_out views) is a leaf, so `is_leaf` let the grouped refresh register a job on such a
    temporary copy and re-pack from it after the next optimizer step: forward / dgrad then ran on pre-step weights for good.
    Here: train steps with (a) reentrant checkpointing, (b) a no_grad sample() in between; afterwards every registered job reads a
    real nn.Parameter, and the model's forward equals that of a fresh model (empty caches) holding the same weights -- bit for bit
    in the reproducible sampling mode."""
    from osufusion_amd.models.diffusion import OsuFusion
    from osufusion_amd.pattern import synth_inputs
    from osufusion_amd.train import Trainer
    kw = dict(_TINY, attn_heads=heads, attn_kv_heads=kv_heads)
    model = OsuFusion(32, **kw).to(DEV)
    load_pattern(model.unet)
    x, a, c, t, noise = (T(v) for v in synth_inputs(f"r3packs{heads}{kv_heads}", 2, 256))
    try:
        if scenario == "checkpointing":
            model.unet.set_gradient_checkpointing(True)
        tr = Trainer(model, lr=3e-3, compute_dtype=torch.bfloat16)
        model.sampling_timesteps = 2
        for step in range(3):
            tr.step(x, a, c, noise, t)
            if scenario == "sample_between_steps":
                with torch.no_grad():
                    model.sample(a, c, x=noise.clone(), cond_scale=2.0)          # rebuilds stale stem / head / GQA packs under no_grad
        params = {id(p) for p in model.parameters()}
        jobs = [j for j in Fn._PACK_JOBS.values() if j.cache() is not None]
        assert len(jobs) >= 20
        for j in jobs:
            assert all(isinstance(w, torch.nn.Parameter) and id(w) in params for w in j.ws), j.key
        # one more optimizer step: the grouped refresh now marks its entries valid for the NEW weights
        tr.step(x, a, c, noise, t)
        twin = _fresh_copy(model, kw)
        with torch.no_grad(), ops.reproducible_mode(True), oa.forced_compute_dtype(torch.bfloat16):
            got = model.unet(x, a, t, c)
            ref = twin.unet(x, a, t, c)
        report(f"packs_after_no_grad/{scenario}/h{heads}kv{kv_heads}", rel_l2=rell2(got, ref))
        assert torch.equal(got, ref), f"cached operand packs differ from the current weights: rel-L2 {rell2(got, ref):.3e}"
    finally:
        Fn.enable_direct_grads(False)


def test_resblock_applied_twice_reports_film_gradient_once(golden_dir):
    """a ResidualBlock used twice in one forward takes two taps of the grouped FiLM output; its `mlp.1` parameters
    are reported complete ONCE (after both uses) and carry the sum of both uses' gradients."""
    from osufusion_amd.modules.residual import ResidualBlock
    from osufusion_amd import runtime as rt
    from osufusion_amd.train import FlatParameters, GradReducer
    torch.manual_seed(5)
    blk = ResidualBlock(32, 32, dim_time=64, dim_cond=64).to(DEV)
    for p in blk.parameters():
        p.data.normal_(0, 0.2)
    x = torch.randn(2, 32, 64, device=DEV)
    te, ce = torch.randn(2, 64, device=DEV, requires_grad=True), torch.randn(2, 64, device=DEV)   # (in the UNet: time_mlp's output)

    def run(group):
        for p in blk.parameters():
            p.grad = None
        rt.clear_shared_cat()
        with oa.forced_compute_dtype(torch.float32):
            rows = rt.to_rows(x, torch.float32)
            if group:
                emb = rt.shared_cat(te, ce)
                assert rt.film_prepare(emb, [blk.mlp[1]])
            y = blk.forward_rows(blk.forward_rows(rows, te, ce), te, ce)
            y.float().square().mean().backward()
        rt.clear_shared_cat()
        return {k: p.grad.detach().clone() for k, p in blk.named_parameters()}

    ref = run(False)
    flat = FlatParameters(blk)
    red = GradReducer(flat)
    Fn.enable_direct_grads(True, red.param_ready, red.param_complete)
    try:
        flat.zero_grad()
        red.begin()
        rt.clear_shared_cat()
        with oa.forced_compute_dtype(torch.float32):
            rows = rt.to_rows(x, torch.float32)
            emb = rt.shared_cat(te, ce)
            assert rt.film_prepare(emb, [blk.mlp[1]])
            blk.forward_rows(blk.forward_rows(rows, te, ce), te, ce).float().square().mean().backward()
        red.finish()
        rt.clear_shared_cat()
        assert red.duplicate_reports == 0
        assert sorted(red.order_log) == list(range(len(flat.params))), "every parameter exactly once"
        got = {k: p.grad.detach().clone() for k, p in blk.named_parameters()}
    finally:
        Fn.enable_direct_grads(False)
    gmax = max(v.abs().max().item() for v in ref.values())
    for k in ref:
        e = (got[k] - ref[k]).abs().max().item() / (ref[k].abs().max().item() + 1e-4 * gmax)
        assert e < 2e-2, (k, e)


def test_sampler_error_growth_vs_oracle(golden_dir):
    """k-step error growth of the DDIM sampler against the oracle (diffusion.py:59-77), tiny golden model, 50-step schedule, fp32
    mode: after k = 1, 2, 5, 10, 20, 35, 50 steps the HIP iterate is compared with the oracle's, and next to it the ORACLE'S OWN
    sensitivity -- the same oracle loop started from x0 perturbed by 3e-4 (relative), the size of one HIP step's error.  The
    network's weights are a fixed pattern, not a trained denoiser, so errors are amplified step by step; what is asserted is that
    the HIP path grows no faster than the oracle's own perturbation does ('matches the reference' must not remain a
    per-step claim without this curve)."""
    import json
    from oracle import diffusion_oracle as DO
    from oracle import unet_oracle as O
    from osufusion_amd.pattern import synth_inputs
    from tests.test_hip_parity import _build_model
    meta, cfgd, model = _build_model("unet_tiny", golden_dir)
    cfg = O.UNetConfig(**cfgd)
    p = O.make_params(cfg, prefix="unet.")
    S, ks = 50, (1, 2, 5, 10, 20, 35, 50)
    x, a, c, t, noise = (torch.from_numpy(v) for v in synth_inputs("growth", 2, 256))
    acp = DO.ddim_alphas_cumprod()
    steps = DO.ddim_timesteps(S).tolist()

    def oracle_traj(x0, cond_scale, kmax):
        xs, out = x0.clone(), {}
        with torch.no_grad():
            for i, tt in enumerate(steps[:kmax]):
                tb = torch.full((x0.shape[0],), tt, dtype=torch.int64)
                pred = O.unet_forward(p, cfg, xs, a, tb, c, cond_drop_prob=0.0, prefix="unet.")
                if cond_scale != 1.0:
                    null = O.unet_forward(p, cfg, xs, a, tb, c, cond_drop_prob=1.0, prefix="unet.")
                    pred = null + (pred - null) * cond_scale
                xs = DO.ddim_step(pred, tt, xs, acp, S)
                if i + 1 in ks:
                    out[i + 1] = xs.clone()
        return out

    model.sampling_timesteps = S
    rows = []
    try:
        for cs, kmax in ((1.0, 50), (2.0, 20)):                       # (guided: two oracle forwards per step -- followed for 20 steps)
            ref = oracle_traj(noise, cs, kmax)
            g = torch.Generator().manual_seed(17)
            pert = noise + 3e-4 * noise.norm() / noise.numel() ** 0.5 * torch.randn(noise.shape, generator=g)
            ref_p = oracle_traj(pert, cs, kmax)
            for k in [k for k in ks if k <= kmax]:
                model.stop_after = k
                with oa.forced_compute_dtype(torch.float32):
                    got = model.sample(a.to(DEV), c.to(DEV), noise.to(DEV), cond_scale=cs).cpu()
                e_hip = rell2(got, ref[k])
                e_orc = rell2(ref_p[k], ref[k])
                rows.append(dict(cond_scale=cs, k=k, hip_vs_oracle=e_hip, oracle_perturbed_3e4_vs_oracle=e_orc))
                report(f"sampler_error_growth/cs{cs}/k{k}", hip_vs_oracle=e_hip, oracle_perturbed_vs_oracle=e_orc)
    finally:
        model.stop_after = None
        model.sampling_timesteps = 35
    import os
    os.makedirs("gpurun_out", exist_ok=True)
    with open("gpurun_out/r03_sampler_error_growth.json", "w") as f:
        json.dump(dict(model="unet_tiny (tests/golden pattern weights)", schedule=f"DDIM {S} steps, eta 0", mode="fp32 compute mode",
                       note="oracle_perturbed = the oracle's own loop from x0 + 3e-4 (rel) noise: its sensitivity to one HIP-step-sized error",
                       rows=rows), f, indent=1)
    for r in rows:
        if r["k"] == 1:
            assert r["hip_vs_oracle"] < 1e-3 * (2 * r["cond_scale"] - 1), r
        # growth: never more than 4x what the oracle itself does to a 3e-4 perturbation (and never below the 1-step bound's scale)
        assert r["hip_vs_oracle"] < max(4.0 * r["oracle_perturbed_3e4_vs_oracle"], 3e-3), r


def _attn_case_d(Bn, N, H, D):
    import torch.nn.functional as F
    qkv = (torch.randn(Bn, N, (H + 2) * D, device=DEV) * (64 / D) ** 0.25).to(torch.bfloat16)
    do = torch.randn(Bn, N, H * D).to(torch.bfloat16)
    qkv32 = qkv.float().cpu().requires_grad_()
    q = qkv32[..., : H * D].view(Bn, N, H, D).permute(0, 2, 1, 3)
    k = qkv32[..., H * D: (H + 1) * D][:, None]
    v = qkv32[..., (H + 1) * D:][:, None]
    s = (q @ k.transpose(-1, -2)) * D ** -0.5
    o_ref = (s.softmax(-1) @ v).permute(0, 2, 1, 3).reshape(Bn, N, H * D)
    o_ref.backward(do.float())
    return qkv, do.to(DEV), o_ref.detach(), qkv32.grad


@pytest.mark.parametrize("D", [16, 32, 128])
@pytest.mark.parametrize("N", [200, 512])
def test_attention_head_dims_other_than_64(D, N):
    """attn_dim_head is a free constructor argument of the reference (unet.py:105-123, diffusion.py:16-30): forward, dQ and dK/dV of the
    generic-head-dim kernels (csrc/attn_generic.hpp; D = 16 runs zero-padded to 32) against autograd of the fp32 formula
    (attention.py:87-101), ragged and whole-block lengths, with and without the RoPE transpose pass."""
    H, Bn = 3, 2
    qkv, do, o_ref, g_ref = _attn_case_d(Bn, N, H, D)
    o, lse = ops.mqa_fwd(qkv, Bn, N, H, D, torch.bfloat16, D ** -0.5)
    e_fwd = rell2(o.float(), o_ref)
    assert e_fwd < 5e-3, e_fwd
    ref_lse = torch.logsumexp((qkv.float()[..., : H * D].view(Bn, N, H, D).permute(0, 2, 1, 3) @
                               qkv.float()[..., H * D: (H + 1) * D][:, None].transpose(-1, -2)) * D ** -0.5, dim=-1) * 1.4426950408889634
    assert (lse - ref_lse).abs().max().item() < 2e-2
    dqkv = ops.mqa_bwd(qkv, o, do, lse, Bn, N, H, D, D ** -0.5)
    for part, sl in (("dq", slice(0, H * D)), ("dk", slice(H * D, (H + 1) * D)), ("dv", slice((H + 1) * D, (H + 2) * D))):
        e = rell2(dqkv[..., sl], g_ref[..., sl])
        report(f"attn_generic/D{D}/N{N}/{part}", rel_l2=e)
        assert e < 1e-2, (part, e)
    # bf16 output == the rounded fp32 output; the RoPE transpose pass == rotating the raw gradients by hand (attention.py:52-58 transposed)
    d16 = ops.mqa_bwd(qkv, o, do, lse, Bn, N, H, D, D ** -0.5, torch.bfloat16)
    assert relmax_(d16.float(), dqkv) < 8e-3
    cos, sin = Fn.rope_tables(N, D, 2 * N, DEV)
    got = ops.mqa_bwd(qkv, o, do, lse, Bn, N, H, D, D ** -0.5, torch.float32, cos, sin)
    want = dqkv.clone()
    for h in range(H + 1):                                               # q heads and the k head; v untouched
        y1, y2 = dqkv[..., h * D: h * D + D // 2], dqkv[..., h * D + D // 2: (h + 1) * D]
        want[..., h * D: h * D + D // 2] = y1 * cos + y2 * sin
        want[..., h * D + D // 2: (h + 1) * D] = y2 * cos - y1 * sin
    assert relmax_(got, want) < 1e-5
    # and the forward rotation + cast
    rot = ops.rope_cast(qkv, cos, sin, N, H + 1, H + 2, D).float()
    x = qkv.float()
    for h in range(H + 1):
        x1, x2 = x[..., h * D: h * D + D // 2], x[..., h * D + D // 2: (h + 1) * D]
        assert relmax_(rot[..., h * D: h * D + D // 2], (x1 * cos - x2 * sin).to(torch.bfloat16).float()) < 4e-3      # one bf16 ulp (fma contraction)
        assert relmax_(rot[..., h * D + D // 2: (h + 1) * D], (x2 * cos + x1 * sin).to(torch.bfloat16).float()) < 4e-3
    assert torch.equal(rot[..., (H + 1) * D:], x[..., (H + 1) * D:])


def relmax_(a, b):
    return ((a.float().cpu() - b.float().cpu()).abs().max() / b.float().abs().max().clamp_min(1e-30)).item()


@pytest.mark.parametrize("D,heads,kv_heads", [(16, 4, 1), (32, 4, 2), (128, 2, 1)])
def test_attention_module_head_dims_vs_oracle(D, heads, kv_heads):
    """The UNet's Attention block (unet.py:104-146) with 16- / 32- / 128-wide heads, forward and every gradient against the oracle's
    autograd (fp32 mode; bf16 only where the reference casts)."""
    from oracle import unet_oracle as O
    from osufusion_amd.modules.unet import Attention
    torch.manual_seed(11)
    C, N, Bn = 64, 96, 2
    m = Attention(C, D, heads, kv_heads, context_len=192).to(DEV)
    for p_ in m.parameters():
        p_.data.normal_(0, 0.15)
    m.norm.weight.data.add_(1.0)
    x = torch.randn(Bn, N, C, device=DEV)
    cfg = O.UNetConfig(attn_dim_head=D, attn_heads=heads, attn_kv_heads=kv_heads)
    p = {f"a.{k}": v.detach().cpu().clone().requires_grad_() for k, v in m.state_dict().items()}
    xr = x.cpu().clone().requires_grad_()
    ref = O.attention(p, "a", xr, cfg, 192, O.Numerics("fp32"))
    xg = x.clone().requires_grad_()
    with oa.forced_compute_dtype(torch.float32):
        got = m(xg)
    g = torch.randn_like(got)
    got.backward(g)
    ref.backward(g.cpu())
    assert rell2(got, ref) < 5e-3
    assert rell2(xg.grad, xr.grad) < 2e-2
    for k, q in m.named_parameters():
        assert rell2(q.grad, p[f"a.{k}"].grad) < 3e-2, k


@pytest.mark.parametrize("big", [False, True])
@pytest.mark.parametrize("M,N,K,taps", [(1024, 256, 256, 3), (520, 96, 40, 1), (2048, 768, 512, 1)])
def test_f32x3_gemms_keep_seventeen_bits(forcing, M, N, K, taps, big):
    """OSUF_DT_F32X3 (fp32 storage, three bf16 MFMAs on split operands) for the conv / linear GEMMs and their weight gradients against an
    fp64 product: an order of magnitude and a half inside north_star's 1e-3, two orders better than bf16 operands (residual.py:70,115,
    unet.py:118-123,149-156 in an fp32 run).  big: the 256x256 LDS-DMA kernels' x3 paths forced onto these small ragged shapes."""
    if big:
        forcing(gemm_big=1)
    torch.manual_seed(1)
    L = M // 2
    a = torch.randn(M, K, device=DEV)
    w = torch.randn(taps, N, K, device=DEV) / (K * taps) ** 0.5
    dy = torch.randn(M, N, device=DEV)
    kw = dict(taps=taps, lin=L, lout=L, stride=1, pad=taps // 2, mode=0)

    def ref_fwd():
        ad, wd = a.double().view(2, L, K), w.double()
        out = torch.zeros(2, L, N, dtype=torch.float64, device=DEV)
        for t in range(taps):
            sh = t - taps // 2
            src = torch.zeros_like(ad)
            if sh >= 0:
                src[:, : L - sh] = ad[:, sh:]
            else:
                src[:, -sh:] = ad[:, : L + sh]
            out += src @ wd[t].T
        return out.view(M, N)

    want = ref_fwd()
    errs = {}
    for mode in ("exact", "x3"):
        prev = ops.set_f32_matmul(mode)
        try:
            got = ops.gemm_nt(a, w, None, **kw)
            gw = ops.gemm_tn(dy, a, **kw)
        finally:
            ops.set_f32_matmul(prev)
        errs[mode] = (rell2(got, want), gw)
    gw_ref = errs["exact"][1].double()
    e_w = rell2(errs["x3"][1], gw_ref)
    bf = ops.gemm_nt(a.to(torch.bfloat16), w.to(torch.bfloat16), None, **kw)
    e_bf = rell2(bf.float(), want)
    report(f"f32x3/M{M}N{N}K{K}t{taps}{'/big' if big else ''}", exact=errs["exact"][0], x3=errs["x3"][0], bf16=e_bf, wgrad_x3_vs_exact=e_w)
    assert errs["exact"][0] < 2e-6
    assert errs["x3"][0] < 3e-5 and e_w < 3e-5, (errs["x3"][0], e_w)
    assert e_bf > 30 * errs["x3"][0]
    # the x3 weight gradient with a split plan goes through partial tiles in a workspace + the fixed-order reduce (ops.gemm_tn asks for the
    # workspace with the launch's dtype code since round 4; with dt_of() it got none and fell back to fp32 atomics): bit-reproducible
    from osufusion_amd import _lib
    need = _lib.load().osuf_gemm_tn_workspace_bytes(ops.F32X3, M, N, K, taps)
    report(f"f32x3_wgrad_workspace/M{M}N{N}K{K}t{taps}{'/big' if big else ''}", workspace_bytes=need)
    if need > 0:
        prev = ops.set_f32_matmul("x3")
        try:
            g1 = ops.gemm_tn(dy, a, **kw)
            g2 = ops.gemm_tn(dy, a, **kw)
        finally:
            ops.set_f32_matmul(prev)
        assert torch.equal(g1, g2) and torch.equal(g1, errs["x3"][1])


def test_f32x3_mode_unet_vs_golden(golden_dir):
    """The whole UNet in the fp32 compute mode with x3 GEMMs against the reference's golden (north_star: 1e-3), next to the exact mode."""
    from osufusion_amd.pattern import synth_inputs
    from tests.test_hip_parity import G, _build_model
    meta, cfgd, model = _build_model("unet_mid", golden_dir)
    g = G(golden_dir, "unet_mid")
    x, a, c, t, noise = (T(v) for v in synth_inputs("unet_mid", meta["B"], meta["L"]))
    out = {}
    for mode in ("exact", "x3"):
        prev = ops.set_f32_matmul(mode)
        try:
            with torch.no_grad(), oa.forced_compute_dtype(torch.float32):
                out[mode] = rell2(model.unet(x, a, t, c, cond_drop_prob=0.0), g["y_cond"])
            for q in model.parameters():
                q.grad = None
            with oa.forced_compute_dtype(torch.float32):
                loss = model.loss_with(x, a, c, noise, t, cond_drop_prob=0.0)
                loss.backward()
            out[mode + "_loss"] = abs(loss.item() - float(g["loss"])) / abs(float(g["loss"]))
            params = dict(model.unet.named_parameters())
            import numpy as np
            gn = np.array([params[k].grad.norm().item() for k in meta["param_names"]])
            ref = g["grad_norms"]
            out[mode + "_gn"] = float((np.abs(gn - ref) / (ref + 1e-3 * ref.max())).max())
        finally:
            ops.set_f32_matmul(prev)
    report("f32x3/unet_mid_vs_golden", **out)
    assert out["x3"] < 1e-3 and out["exact"] < 1e-3
    assert out["x3_loss"] < 1e-3 and out["x3_gn"] < 2e-2


@pytest.mark.parametrize("D,H,G", [(64, 4, 1), (16, 2, 2), (32, 3, 1), (128, 2, 1)])
def test_attend_with_mask_matches_reference_semantics(D, H, G):
    """Attend(q, k, v, attn_mask) (attention.py:77-99): the reference casts the mask to bf16 and passes it to SDPA, i.e. it is an ADDITIVE
    bias of the scaled scores whatever its dtype was (a bool mask adds 1.0 / 0.0).  Checked against that formula in fp32 on the
    bf16-cast inputs: a float bias incl. -inf blocks (broadcast over batch and heads), a per-head bias, and a bool mask."""
    from osufusion_amd.modules.attention import Attend
    torch.manual_seed(4)
    B, N = 2, 200
    q = torch.randn(B, H, N, D, device=DEV)
    k = torch.randn(B, G, N, D, device=DEV)
    v = torch.randn(B, G, N, D, device=DEV)
    att = Attend()

    def ref(mask):
        qb, kb, vb = (t.to(torch.bfloat16).float() for t in (q, k, v))
        if G != H:
            kb, vb = kb.expand(B, H, N, D), vb.expand(B, H, N, D)
        sc = (qb @ kb.transpose(-1, -2)) * D ** -0.5 + mask.to(torch.bfloat16).float()
        return sc.softmax(-1) @ vb

    causal = torch.zeros(N, N, device=DEV).masked_fill(torch.triu(torch.ones(N, N, device=DEV, dtype=torch.bool), 1), float("-inf"))
    per_head = torch.randn(1, H, N, N, device=DEV) * 2
    boolean = torch.rand(B, 1, N, N, device=DEV) > 0.5
    for name, m in (("causal -inf", causal), ("per-head float", per_head), ("bool", boolean)):
        got = att(q, k, v, attn_mask=m)
        want = ref(m)
        e = rell2(got, want)
        report(f"attend_mask/D{D}/{name}", rel_l2=e)
        assert torch.isfinite(got).all() and e < 6e-3, (name, e)
    assert rell2(att(q, k, v), ref(torch.zeros(1, device=DEV))) < 6e-3


@pytest.mark.parametrize("D", [16, 32, 64, 128])
@pytest.mark.parametrize("N", [64, 200, 1000])
def test_masked_forward_op_random_bias(D, N):
    """The masked forward on its own (osuf_xattn_fwd with Nk = N, on the column views of the q|k|v image): a dense random bf16 bias with a band of -inf key columns, every key tile (the second 32-key half of
    a 64-key tile included -- a first version of the kernel got exactly that half wrong) and a ragged last tile."""
    from osufusion_amd import cross_attend as Xa
    torch.manual_seed(D + N)
    B, H = 2, 3
    qkv = torch.randn(B, N, (H + 2) * D, device=DEV).to(torch.bfloat16)
    qc, kc, vc = qkv[..., :H * D], qkv[..., H * D:(H + 1) * D], qkv[..., (H + 1) * D:]
    x = qkv.float()
    q = x[..., :H * D].view(B, N, H, D).permute(0, 2, 1, 3)
    k, v = x[..., H * D:(H + 1) * D][:, None], x[..., (H + 1) * D:][:, None]
    bias = torch.randn(B, H, N, N, device=DEV).to(torch.bfloat16)
    bias[:, :, :, N // 2:N // 2 + 7] = float("-inf")
    want = (((q @ k.transpose(-1, -2)) * D ** -0.5 + bias.float()).softmax(-1) @ v).permute(0, 2, 1, 3).reshape(B, N, H * D)
    got = Xa.xattn_fwd(qc, kc, vc, bias, B, N, N, H, D, torch.bfloat16, D ** -0.5)[0]
    e = rell2(got, want)
    report(f"attend_mask/op/D{D}/N{N}", rel_l2=e)
    assert e < 4e-3
    # a one-hot row of the bias selects exactly that key's value row
    hot = torch.full((B, H, N, N), -1e4, device=DEV, dtype=torch.bfloat16)
    key = min(N - 1, 33)
    hot[..., key] = 0
    got = Xa.xattn_fwd(qc, kc, vc, hot, B, N, N, H, D, torch.float32, D ** -0.5)[0]
    assert torch.equal(got.view(B, N, H, D), v[:, 0, key][:, None, None, :].expand(B, N, H, D))


@pytest.mark.parametrize("Cin,Cout,L,Bq", [(128, 328, 512, 3), (64, 256, 256, 4), (192, 72, 768, 2)])
def test_halo_shared_k3_conv_kernel(forcing, Cin, Cout, L, Bq):
    """gemm_nt_big_halo3_kernel (k = 3 'same' convs and their input gradients with L % 256 == 0: one activation panel per K-step shared by
    the three taps) forced onto small shapes: against the plain 256x256 kernel (same products, K-step-major instead of tap-major fp32
    sums) and against conv1d on the bf16-rounded operands -- sample edges (halo rows from the zero page), N tail, every epilogue
    option, residual.py:70."""
    import torch.nn.functional as F
    from tests.test_hip_parity import relmax
    torch.manual_seed(Cin + L)
    forcing(gemm_big=1, wgrad_f32_partials=True)               # pins the kernels' products (round 4's bf16-pair partial tiles: tests/test_round4_gpu.py)
    x = torch.randn(Bq, L, Cin, device=DEV).to(torch.bfloat16)
    w = torch.randn(Cout, Cin, 3, device=DEV) / (Cin * 3) ** 0.5
    bias = torch.randn(Cout, device=DEV)
    res = torch.randn(Bq, L, Cout, device=DEV).to(torch.bfloat16)
    rscale = torch.rand(Bq, Cout, device=DEV)
    outs = []
    for nohalo in (True, False):
        with ops.force(nohalo=nohalo):
            stats = torch.zeros(Bq, 2, dtype=torch.float64, device=DEV)
            y, pre = Fn.conv_forward(x, w, bias, Fn.PackCache(), "same", None, act=1, residual=res, rscale=rscale, stats=stats, want_pre=True)
            dx = Fn.conv_dgrad(y, w, Fn.PackCache(), "same", L, residual=x)
            dw = Fn.conv_wgrad(res, x, w, "same")              # gemm_tn_taps3_kernel (three taps per workgroup, one X panel) when not "nohalo"
        outs.append((y.float(), pre.float(), stats.clone(), dx.float(), dw.float()))
    (y0, p0, s0, d0, w0), (y1, p1, s1, d1, w1) = outs
    assert relmax(w1, w0) < 1e-5                               # same bf16 products, different fp32 summation order
    xs = F.pad(x.float(), (0, 0, 1, 1))                        # zero rows at the sample edges
    want = torch.stack([torch.einsum("blo,bli->oi", res.float(), xs[:, t:t + L]) for t in range(3)], dim=-1)
    assert relmax(w1.reshape(want.shape), want) < 1e-4
    for u, v in ((p0, p1), (y0, y1), (d0, d1)):       # different fp32 summation order: a bf16 ulp on a few elements at most
        assert torch.allclose(u, v, rtol=2.0 ** -7, atol=2e-3) and (u != v).float().mean().item() < 2e-2
    assert torch.allclose(s0, s1, rtol=1e-5)
    ref = F.conv1d(x.float().permute(0, 2, 1), w.to(torch.bfloat16).float(), bias, padding=1)
    assert relmax(p1.permute(0, 2, 1), ref) < 1e-2
    # a sample's first and last rows see zeros, not the neighbouring sample's rows
    assert relmax(p1[:, [0, L - 1]].permute(0, 2, 1), ref[:, :, [0, L - 1]]) < 1e-2


@pytest.mark.parametrize("M,N1,N2,taps,force_big", [(1024, 328, 128, 3, True), (2048, 256, 64, 1, True), (4096, 1152, 256, 1, True),
                                                     (520, 96, 40, 1, False), (1024, 328, 128, 3, False)])
@pytest.mark.parametrize("dtype", ["bf16", "x3"])
def test_bias_gradient_rides_the_weight_gradient(forcing, M, N1, N2, taps, force_big, dtype):
    """osuf_gemm_tn_bias: the layer's bias gradient (column sums of dy) from the weight gradient's own pass over dy -- the merged-taps and
    256x256 bf16 kernels sum the dY fragments they hold, every other path (small shapes, the fp32 modes) runs osuf_colsum inside the entry
    point.  Against dy.sum(0) in fp64 and against osuf_gemm_tn + osuf_colsum (residual.py:70,115, unet.py:118-123,149-156)."""
    if force_big:
        forcing(gemm_big=1)
    torch.manual_seed(M + N1)
    L = M // 2
    dt = torch.bfloat16 if dtype == "bf16" else torch.float32
    dy = torch.randn(M, N1, device=DEV).to(dt)
    x = torch.randn(M, N2, device=DEV).to(dt)
    kw = dict(taps=taps, lin=L, lout=L, stride=1, pad=taps // 2, mode=0)
    prev = ops.set_f32_matmul("x3")
    try:
        db = torch.full((N1,), 0.5, device=DEV)                      # accumulated into, not overwritten
        gw = ops.gemm_tn(dy, x, bias_out=db, **kw)
        gw0 = ops.gemm_tn(dy, x, **kw)
    finally:
        ops.set_f32_matmul(prev)
    want = dy.double().sum(0) + 0.5
    assert rell2(db, want) < 2e-6
    assert torch.allclose(gw, gw0, rtol=1e-5, atol=1e-5 * gw0.abs().max().item())
    assert rell2(ops.colsum(dy, N1) + 0.5, want) < 2e-6
    # every row of m counted exactly once: indicator rows (a first version counted rows 0, 1 of each group of four twice and rows 2, 3 never,
    # which random data and all-ones both let through at the magnitude level)
    for r in (2, 3, 7, 13):
        ind = (torch.arange(M, device=DEV) % 16 == r).to(dt)[:, None].expand(M, N1).contiguous()
        db = torch.zeros(N1, device=DEV)
        prev = ops.set_f32_matmul("x3")
        try:
            ops.gemm_tn(ind, x, bias_out=db, **kw)
        finally:
            ops.set_f32_matmul(prev)
        assert torch.equal(db, ind.float().sum(0)), r
