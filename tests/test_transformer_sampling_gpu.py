"""DiffusionOsuFusionDiT / RectifiedFlowOsuFusionDiT on the GPU (osufusion_amd/models/transformer_diffusion.py): the restructured samplers
against the loop a user writes from the public pieces, one DDIM step against the fp64 restatements (tests/dit_oracle.py,
tests/mmdit_oracle.py), the training losses, repeatability and the attention launch count.  Weights are the deterministic non-zero pattern
the fixtures of tests/golden/{dit,mmdit}_cases.json were recorded with (a freshly initialised adaLN-Zero model outputs zeros).  The measured
distances are recorded in profiles/dit_sampling.md."""
import json
from pathlib import Path

import pytest
import torch

from oracle import diffusion_oracle as DO
from osufusion_amd import forced_compute_dtype, ops
from osufusion_amd.models import DiffusionOsuFusionDiT, RectifiedFlowOsuFusionDiT
from osufusion_amd.models.diffusion import DDIMSchedule, _MSEFn
from osufusion_amd.models.rectified_flow import cosmap
from osufusion_amd.pattern import param_pattern, synth_inputs
from tests import dit_oracle, mmdit_oracle
from tests.test_attend_autograd_gpu import RL2
from tests.test_poisoned_memory import relmax, rell2

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = Path(__file__).resolve().parent / "golden"
META = {**json.loads((GOLD / "mmdit_cases.json").read_text()), **json.loads((GOLD / "dit_cases.json").read_text())}
NAMES = ["mmdit_h96", "mmdit_h128_mqa", "mmdit_h128_nonorm", "dit_h96", "dit_h128"]
STEPS = 4

# Restructured sampler vs the plain loop: the two differ by batching (2B rows per launch), by the order of the three-term sum of the
# conditioning vector, by the fused guidance combine and, on the DiT, by the stem's audio channels being summed apart from the map's: fp32
# last-bit differences, which the bf16 rounding of the attention operands turns into occasional 2^-9 steps and every further step of these
# untrained weights amplifies (1 step: <= 2.5e-5 rel-L2; 3 steps: <= 3.1e-4).  Measured over every DDIM and flow case below (fp32 compute,
# profiles/dit_sampling.md): largest rel-L2 3.055e-4, largest relmax 2.129e-3, both at mmdit_h128_nonorm / 3 steps / guidance 2.  The bounds
# are 4 x those maxima, and never above the fp32-mode RL2 of tests/test_mmdit_gpu.py.
MEASURED_RL2, MEASURED_RMAX = 3.055e-4, 2.129e-3
PLAIN_RL2, PLAIN_RMAX = min(4 * MEASURED_RL2, RL2), min(4 * MEASURED_RMAX, RL2)
RESTATEMENT_RL2 = 1e-3                 # test_mmdit_fp32_vs_restatement / test_dit_fp32_vs_restatement: the output against fp64


def _backbone_kwargs(name):
    m = META[name]
    kw = dict(dim_h=m["dim_h"], depth=m["depth"], attn_dim_head=m["attn_dim_head"], attn_heads=m["attn_heads"], attn_qk_norm=m["attn_qk_norm"])
    if name.startswith("mmdit"):
        kw.update(backbone="mmdit", patch_size=m["patch_size"], attn_kv_heads=m["attn_kv_heads"])
    else:
        kw.update(backbone="dit")
    return kw


def _model(cls, name, **kw):
    model = cls(**_backbone_kwargs(name), **kw)
    model.load_state_dict({k: torch.from_numpy(param_pattern(k[len("unet."):], tuple(v.shape)).copy()) for k, v in model.state_dict().items()})
    return model.to(DEV)


def _inputs(name, dev=DEV):
    m = META[name]
    return [torch.from_numpy(v).to(dev) for v in synth_inputs(name, m["B"], m["L"])]          # x, a, c, t, noise


def _plain_ddim(model, a, c, x, stop_after, cond_scale):
    """The loop a user writes from the public pieces: forward_with_cond_scale (two batch-B forwards) + DDIMSchedule + ops.ddim_step."""
    b = a.shape[0]
    sch = DDIMSchedule()
    sch.set_timesteps(STEPS)
    x = x.float().contiguous()
    with torch.inference_mode(), forced_compute_dtype(torch.float32):
        for t in sch.timesteps.tolist()[:stop_after]:
            tb = torch.full((b,), t, dtype=torch.int64, device=DEV)
            pred = model.unet.forward_with_cond_scale(x, a, tb, c, cond_scale=cond_scale).contiguous()
            coef = torch.tensor([sch.step_coefficients(t)] * b, dtype=torch.float32, device=DEV)
            x = ops.ddim_step(x, pred, None, 1.0, coef)
    return x


def _plain_flow(model, a, c, x, cond_scale):
    b = a.shape[0]
    ones = torch.ones(b, dtype=torch.float32, device=DEV)
    x = x.float().contiguous()
    with torch.inference_mode(), forced_compute_dtype(torch.float32):
        def f(t, y):
            tb = torch.full((b,), t, dtype=torch.float32, device=DEV)
            return model.unet.forward_with_cond_scale(y, a, tb, c, cond_scale=cond_scale).contiguous()
        times = torch.linspace(0.0, 1.0, model.sample_timesteps).tolist()
        for t0, t1 in zip(times[:-1], times[1:]):
            dt = t1 - t0
            k1 = f(t0, x)
            k2 = f(t0 + 0.5 * dt, ops.axpby_rows(x, k1, ones, ones * (0.5 * dt)))
            x = ops.axpby_rows(x, k2, ones, ones * dt)
    return x


def _assert_near_plain(tag, got, want):
    e2, em = rell2(got, want), relmax(got, want)
    print(f"dit_sampling {tag}: rel_l2={e2:.3e} relmax={em:.3e}")
    assert torch.isfinite(got).all(), tag
    assert e2 < PLAIN_RL2 and em < PLAIN_RMAX, (tag, e2, em)


@pytest.mark.parametrize("cond_scale", [1.0, 2.0])
@pytest.mark.parametrize("stop_after", [1, 3])
@pytest.mark.parametrize("name", NAMES)
def test_ddim_sampler_equals_the_plain_loop(name, stop_after, cond_scale):
    model = _model(DiffusionOsuFusionDiT, name, sampling_timesteps=STEPS)
    _, a, c, _, x = _inputs(name)
    model.stop_after = stop_after
    with forced_compute_dtype(torch.float32):
        got = model.sample(a, c, x, cond_scale=cond_scale)
    assert got.shape == x.shape and got.dtype == torch.float32
    _assert_near_plain(f"ddim/{name}/stop{stop_after}/cfg{cond_scale}", got, _plain_ddim(model, a, c, x, stop_after, cond_scale))


@pytest.mark.parametrize("cond_scale", [1.0, 2.0])
@pytest.mark.parametrize("name", NAMES)
def test_flow_sampler_equals_the_plain_loop(name, cond_scale):
    """sampling_timesteps = 3: two midpoint intervals, four evaluations of the backbone."""
    model = _model(RectifiedFlowOsuFusionDiT, name, sampling_timesteps=3)
    _, a, c, _, x = _inputs(name)
    with forced_compute_dtype(torch.float32):
        got = model.sample(a, c, x, cond_scale=cond_scale)
    _assert_near_plain(f"flow/{name}/cfg{cond_scale}", got, _plain_flow(model, a, c, x, cond_scale))


_ORACLE = {}


def _oracle_preds(name, model, x, a, c, t):
    """fp64 noise predictions of the restatement for keep = 1 and keep = 0, computed once per case."""
    if name not in _ORACLE:
        m = META[name]
        p = {k[len("unet."):]: v.detach().cpu().double() for k, v in model.state_dict().items()}
        b = a.shape[0]
        tb = torch.full((b,), t, dtype=torch.int64)
        if name.startswith("mmdit"):
            cfg = mmdit_oracle.MMDiTConfig(dim_h=m["dim_h"], depth=m["depth"], patch_size=m["patch_size"], heads=m["attn_heads"],
                                           kv_heads=m["attn_kv_heads"], dim_head=m["attn_dim_head"], qk_norm=m["attn_qk_norm"])
            fwd = lambda keep: mmdit_oracle.mmdit_forward(p, cfg, x.cpu(), a.cpu(), tb, c.cpu(), keep=keep)
        else:
            cfg = dit_oracle.DiTConfig(dim_h=m["dim_h"], depth=m["depth"], heads=m["attn_heads"], dim_head=m["attn_dim_head"], qk_norm=m["attn_qk_norm"])
            fwd = lambda keep: dit_oracle.dit_forward(p, cfg, x.cpu(), a.cpu(), tb, c.cpu(), keep=keep)
        with torch.no_grad():
            _ORACLE[name] = (fwd(torch.ones(b, dtype=torch.bool)).double(), fwd(torch.zeros(b, dtype=torch.bool)).double())
    return _ORACLE[name]


@pytest.mark.parametrize("name", NAMES)
def test_one_ddim_step_vs_fp64_restatement(name):
    """x1 of the first step (t = 750 of 4) against oracle.diffusion_oracle.ddim_step on the guided fp64 prediction.  The bound is the
    restatement tests' 1e-3 on the prediction, so the prediction is recovered from x1: x1 = pa * clamp((x - s1 eps) / sa) + p1 eps is
    affine in eps on each side of the clamp (slope p1 - pa s1 / sa inside, p1 where x0 is clamped to +-1), inverted per element on the
    side the reference is on."""
    cond_scale = 2.0
    model = _model(DiffusionOsuFusionDiT, name, sampling_timesteps=STEPS)
    _, a, c, _, x = _inputs(name)
    model.stop_after = 1
    with forced_compute_dtype(torch.float32):
        x1 = model.sample(a, c, x, cond_scale=cond_scale).double().cpu()
    t = DO.ddim_timesteps(STEPS)[0].item()
    cond, null = _oracle_preds(name, model, x, a, c, t)
    eps = null + (cond - null) * cond_scale
    acp = DO.ddim_alphas_cumprod().double()
    xd = x.double().cpu()
    ref_x1 = DO.ddim_step(eps, t, xd, acp, STEPS)
    a_t, a_prev = acp[t], acp[t - 1000 // STEPS]
    s1, sa, pa, p1 = (1 - a_t).sqrt(), a_t.sqrt(), a_prev.sqrt(), (1 - a_prev).sqrt()
    x0 = (xd - s1 * eps) / sa
    inside = x0.abs() <= 1.0
    got_eps = torch.where(inside, (x1 - pa / sa * xd) / (p1 - pa * s1 / sa), (x1 - pa * x0.sign()) / p1)
    e_x1, e_eps = rell2(x1, ref_x1), rell2(got_eps, eps)
    print(f"dit_sampling step_vs_fp64/{name}: x1 rel_l2={e_x1:.3e} recovered prediction rel_l2={e_eps:.3e} clamped={1 - inside.double().mean().item():.3f}")
    assert e_eps < RESTATEMENT_RL2, (e_eps, e_x1)


@pytest.mark.parametrize("name", ["mmdit_h96", "dit_h96"])
@pytest.mark.parametrize("cls", [DiffusionOsuFusionDiT, RectifiedFlowOsuFusionDiT], ids=lambda c: c.__name__)
def test_loss_with_is_the_mse_of_the_backbones_forward(cls, name):
    model = _model(cls, name)
    x, a, c, t, noise = _inputs(name)
    b = x.shape[0]
    orig_len = torch.tensor([x.shape[-1], x.shape[-1] - 17])
    if cls is DiffusionOsuFusionDiT:
        draws = t
        x_noisy, target = model.scheduler.add_noise(x, noise, t), noise.float()
    else:
        draws = torch.linspace(0.2, 0.7, b, device=DEV)
        tt = cosmap(draws)
        ones = torch.ones_like(tt)
        x_noisy = ops.axpby_rows(x.float().contiguous(), noise.float().contiguous(), tt.contiguous(), (1 - tt).contiguous())
        target = ops.axpby_rows(x.float().contiguous(), noise.float().contiguous(), ones, -ones)
    torch.manual_seed(11)
    got = model.loss_with(x, a, c, noise, draws, orig_len)
    torch.manual_seed(11)                                   # the same condition-drop mask
    want = _MSEFn.apply(model.unet(x_noisy, a, draws if cls is DiffusionOsuFusionDiT else draws.float(), c, cond_drop_prob=model.cond_drop_prob),
                        target, orig_len)
    assert got.grad_fn is not None and torch.isfinite(got).item() and got.item() > 0
    assert torch.equal(got.detach(), want.detach())


@pytest.mark.parametrize("cls,name", [(DiffusionOsuFusionDiT, "mmdit_h96"), (RectifiedFlowOsuFusionDiT, "dit_h96")], ids=["ddim_mmdit", "flow_dit"])
def test_bf16_loss_backward_under_memguard(cls, name):
    from tests.memguard import guard
    model = _model(cls, name)
    model.set_full_bf16()
    x, a, c, t, noise = _inputs(name)
    draws = t if cls is DiffusionOsuFusionDiT else torch.linspace(0.2, 0.7, x.shape[0], device=DEV)
    with guard(0xFF) as g:
        loss = model.loss_with(x, a, c, noise, draws)
        loss.backward()
        torch.cuda.synchronize()
        g.check()
        assert torch.isfinite(loss).item()
        for k, p in model.named_parameters():
            assert p.grad is None or torch.isfinite(p.grad).all(), k
        first_attn = next(p for k, p in model.named_parameters() if k.startswith('unet.blocks.0.attn.to_q'))
        assert model.unet.null_cond.grad is not None and first_attn.grad is not None
        g.release()


@pytest.mark.parametrize("cls,name", [(DiffusionOsuFusionDiT, "mmdit_h96"), (DiffusionOsuFusionDiT, "dit_h96"), (RectifiedFlowOsuFusionDiT, "mmdit_h128_mqa")],
                         ids=["ddim_mmdit", "ddim_dit", "flow_mmdit"])
def test_sampling_is_repeatable_bit_for_bit(cls, name):
    model = _model(cls, name, sampling_timesteps=3)
    _, a, c, _, x = _inputs(name)
    outs = [model.sample(a, c, x, cond_scale=2.0) for _ in range(2)]
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])
    model.set_full_bf16()
    outs = [model.sample(a, c, x, cond_scale=2.0) for _ in range(2)]
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("name,per_step", [("mmdit_h96", 2), ("dit_h96", 2)])
def test_sampler_step_issues_one_attention_launch_per_block(name, per_step):
    """depth = 2 blocks, G = 2 (MMDiT) / G = H = 6 (DiT) K/V groups: one osuf_gqa_fwd launch per block and step, none of the per-group
    osuf_mqa_fwd launches the plain forward issues."""
    model = _model(DiffusionOsuFusionDiT, name, sampling_timesteps=STEPS)
    assert len(model.unet.blocks) == per_step
    _, a, c, _, x = _inputs(name)
    for stop_after in (1, 2):
        model.stop_after = stop_after
        timer = ops.KernelTimer(["osuf_gqa_fwd", "osuf_mqa_fwd"])
        ops.set_kernel_timer(timer)
        try:
            model.sample(a, c, x, cond_scale=2.0)
        finally:
            ops.set_kernel_timer(None)
        got = {k: v["launches"] for k, v in timer.summary().items()}
        assert got == {"osuf_gqa_fwd": per_step * stop_after}, got
    G = META[name].get("attn_kv_heads", META[name]["attn_heads"])
    timer = ops.KernelTimer(["osuf_gqa_fwd", "osuf_mqa_fwd"])
    ops.set_kernel_timer(timer)
    try:
        with torch.no_grad():
            model.unet(x, a, torch.zeros(x.shape[0], dtype=torch.int64, device=DEV), c)
    finally:
        ops.set_kernel_timer(None)
    assert {k: v["launches"] for k, v in timer.summary().items()} == {"osuf_mqa_fwd": per_step * G}     # the plain forward keeps its launches
