"""The continuous-time scheduler on the GPU: osuf_ct_schedule against the reference's recorded fp32 values, osuf_ct_step against an fp64
evaluation of its own formula, GaussianDiffusionContinuousTimes' methods against the fixture, and ContinuousDiffusionOsuFusionDiT
(sampler against the plain loop and the fp64 restatement, loss, repeatability, launch count).  Outputs are allocated poisoned and
canary-guarded (tests/memguard.py).  Bounds and measured distances: profiles/ct_scheduler_parity.md."""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

from osufusion_amd import ct, forced_compute_dtype, ops
from osufusion_amd.models import ContinuousDiffusionOsuFusionDiT
from osufusion_amd.models.diffusion import _MSEFn
from osufusion_amd.modules import GaussianDiffusionContinuousTimes
from osufusion_amd.pattern import param_pattern, synth_inputs
from tests import dit_oracle, mmdit_oracle
from tests import scheduler_oracle as SO
from tests.memguard import guard

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD_DIR = Path(__file__).resolve().parent / "golden"
GOLD = np.load(GOLD_DIR / "scheduler_cases.npz")
META = {**json.loads((GOLD_DIR / "mmdit_cases.json").read_text()), **json.loads((GOLD_DIR / "dit_cases.json").read_text())}
NAMES = ["mmdit_h96", "dit_h96"]                       # B = 2, L = 203: no multiple of the MMDiT's patch size 4
# tests/test_transformer_sampling_gpu.py's bounds (restated: importing that module would collect its tests a second time)
RL2 = 2e-3                                             # tests/test_attend_autograd_gpu.py
MEASURED_RL2, MEASURED_RMAX = 3.055e-4, 2.129e-3
PLAIN_RL2, PLAIN_RMAX = min(4 * MEASURED_RL2, RL2), min(4 * MEASURED_RMAX, RL2)
RESTATEMENT_RL2 = 1e-3


def gold(key):
    return torch.from_numpy(GOLD[key])


def rell2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def relmax(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


# ---- osuf_ct_schedule ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_next", [False, True], ids=["t", "t_and_next"])
@pytest.mark.parametrize("schedule", SO.SCHEDULES)
def test_ct_schedule_against_the_recorded_reference(schedule, with_next):
    """The bound: how far the fp32 restatement moves when its cos(.) / expm1(.) moves by +-2 ulps (a different libm), times 2 for the
    second libm between the recording and the device.  Computed on the CPU from the restatement, never from the kernel.

    Measured (MI355X, profiles/ct_scheduler_parity.md): every column of both schedules equals the recording bit for bit except cosine
    posterior_variance / posterior_log_variance at t = 0.25 (5.59e-08 / 1.91e-06 against bounds of 2.5e-07 / 8.1e-06)."""
    t, t_next = gold("t"), gold("t_next") if with_next else None
    want = SO.stack_row(SO.schedule_row(t, t_next, schedule))
    if with_next:
        bound = 2 * SO.perturbation_bound(lambda a, b: SO.stack_row(SO.schedule_row(t, t_next, schedule, nudge=a, nudge_next=b)), True)
    else:
        bound = 2 * SO.perturbation_bound(lambda a: SO.stack_row(SO.schedule_row(t, None, schedule, nudge=a)), False)
    recorded = {"log_snr": "log_snr", "alpha": "alpha", "sigma": "sigma", "posterior_variance": "post_var", "posterior_log_variance": "post_logvar"}
    for col, key in recorded.items():                                     # the recording where there is one, else the fp32 restatement
        if col in SO.COLUMNS[:want.shape[1]]:
            want[:, SO.COLUMNS.index(col)] = gold(f"{schedule}/{key}").flatten()
    with guard(0xFF) as g:
        got = ops.ct_schedule(g.place(t.to(DEV)), g.place(t_next.to(DEV)) if with_next else None, ct.KINDS[schedule])
        g.check()
        got = got.cpu()
        g.release()
    assert got.shape == want.shape == (6, ct.COLS if with_next else ct.COLS_T) and got.dtype == torch.float32
    assert torch.isfinite(got).all(), got                                  # t = 0 and t = 1 included; an unwritten element is NaN
    err = (got - want).abs()
    for j in range(want.shape[1]):
        print(f"ct_scheduler ct_schedule/{schedule}/{SO.COLUMNS[j]}: dist per t = {[f'{v:.2e}' for v in err[:, j].tolist()]} "
              f"bound = {[f'{v:.2e}' for v in bound[:, j].tolist()]}")
    assert (err <= bound).all(), [(SO.COLUMNS[j], i, err[i, j].item(), bound[i, j].item()) for i, j in (err > bound).nonzero().tolist()]


# ---- osuf_ct_step -------------------------------------------------------------------------------------------------------------------
def step_inputs(B, per_sample, seed=5):
    """N(0, 1) iterates and predictions; the null prediction lies near the conditional one, so that guidance 7 keeps eps at N(0, 1)'s scale."""
    g = torch.Generator().manual_seed(seed)
    x, cond, noise = (torch.randn((B, per_sample), generator=g) for _ in range(3))
    null = cond + 0.05 * torch.randn((B, per_sample), generator=g)
    return x, cond, null, noise


STEP_TIMES = ([0.5, 0.625, 0.125], [0.375, 0.5, 0.0])                      # three (t, t_next); the last sample's t_next is 0
STEP_SHAPES = {
    "B3_222": (3, 6 * 37, False),                                          # no multiple of 4: rows start unaligned, two tail elements
    "vec_second_pass": (3, 699052, False),                                 # 2,097,156 elements: 2048 x 256 lanes x 4, and one more group
    "scalar_second_pass": (3, 174764, True),                               # buffers off 16-byte alignment: 524,292 > 2048 x 256 lanes
}


def _misaligned(t):
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    buf[1:].copy_(t.flatten())
    return buf[1:].view(t.shape)


@pytest.mark.parametrize("with_noise", [False, True], ids=["mean", "noise"])
@pytest.mark.parametrize("with_null", [False, True], ids=["cond", "guided"])
@pytest.mark.parametrize("shape", list(STEP_SHAPES))
def test_ct_step_against_fp64_of_its_formula(shape, with_null, with_noise):
    """Fed the kernel's own fp32 coefficient row, so only the elementwise rounding is under test: a handful of fp32 roundings,
    16 * 2^-24 * max(1, largest |term| of the element)."""
    B, per, misalign = STEP_SHAPES[shape]
    x, cond, null, noise = step_inputs(B, per)
    cond_scale = 7.0 if with_null else 1.0
    with guard(0xFF) as g:
        put = (lambda v: _misaligned(v.to(DEV))) if misalign else (lambda v: g.place(v.to(DEV)))
        row = ops.ct_schedule(torch.tensor(STEP_TIMES[0], device=DEV), torch.tensor(STEP_TIMES[1], device=DEV), ct.KINDS["cosine"])
        xd, cd = put(x), put(cond)
        nd, zd = (put(null) if with_null else None), (put(noise) if with_noise else None)
        assert (xd.data_ptr() % 16 != 0) == misalign
        got = ops.ct_step(xd, cd, nd, cond_scale, row, zd)
        poisoned = ops.ct_step(xd, cd, nd, cond_scale, row, put(torch.full_like(noise, float("nan"))))
        again = ops.ct_step(xd, cd, nd, cond_scale, row, zd)
        g.check()
        got, poisoned, again, row = got.cpu(), poisoned.cpu(), again.cpu(), row.cpu()
        g.release()
    want, terms, clamped = SO.ct_step(x, cond, null if with_null else None, cond_scale, row, noise if with_noise else None)
    frac = clamped.double().mean().item()
    bound = 16 * 2.0 ** -24 * terms.clamp(min=1.0)
    err = (got.double() - want).abs()
    print(f"ct_scheduler ct_step/{shape}/null{int(with_null)}/noise{int(with_noise)}: max err/bound = {(err / bound).max().item():.3f} "
          f"max|term| = {terms.max().item():.2f} clamped = {frac:.3f}")
    assert 0.10 <= frac <= 0.60, frac
    assert torch.isfinite(got).all()
    assert (err <= bound).all(), (err / bound).max().item()
    assert torch.equal(got, again)                                                        # bit-repeatable
    # t_next == 0: the posterior mean, bit for bit, whatever the noise buffer holds
    mean_only, _, _ = SO.ct_step(x, cond, null if with_null else None, cond_scale, row, None)
    assert torch.equal(poisoned[2], got[2]) and torch.isfinite(poisoned[2]).all()
    assert ((got[2].double() - mean_only[2]).abs() <= bound[2]).all()
    assert torch.isnan(poisoned[:2]).all()                                                # the other samples do read their noise


def test_ct_step_without_noise_is_the_mean_of_the_noised_step():
    """gain * noise is the only difference: with a zero noise buffer the two forms agree bit for bit on every sample."""
    x, cond, null, noise = (v.to(DEV) for v in step_inputs(3, 222))
    row = ops.ct_schedule(torch.tensor(STEP_TIMES[0], device=DEV), torch.tensor(STEP_TIMES[1], device=DEV), 1)
    assert torch.equal(ops.ct_step(x, cond, null, 7.0, row, None), ops.ct_step(x, cond, null, 7.0, row, torch.zeros_like(noise)))


# ---- GaussianDiffusionContinuousTimes -------------------------------------------------------------------------------------------------
def _per_sample_bound(ref32, ref64):
    """4 x the largest distance, per sample, between the reference's fp32 evaluation (the recording) and the fp64 evaluation of the same
    call: the reference's own rounding is the scale."""
    d = (ref32.double() - ref64).abs().reshape(ref32.shape[0], -1).amax(1)
    return 4 * d, d


@pytest.mark.parametrize("schedule", SO.SCHEDULES)
def test_module_methods_against_the_recorded_reference(schedule):
    """Bound: 4 x the distance, per sample, between the reference's fp32 evaluation (the recording) and the fp64 evaluation of the same call."""
    t, t_next, x_0, noise = gold("t"), gold("t_next"), gold("x_0"), gold("noise")
    rec = {k: gold(f"{schedule}/{k}") for k in ("x_t", "qs_log_snr", "qs_alpha", "qs_sigma", "start", "post_mean", "post_var", "post_logvar",
                                                 "post_mean_default", "post_var_default", "post_logvar_default", "x_half", "log_snr")}
    f64 = torch.float64
    o_xt, o_ls, o_alpha, o_sigma = SO.q_sample(x_0, t, noise, schedule, f64)
    o_mean, o_var, o_logvar = SO.q_posterior(x_0, rec["x_t"], t, t_next, schedule, f64)
    ref64 = dict(x_t=o_xt, qs_log_snr=o_ls, qs_alpha=o_alpha, qs_sigma=o_sigma, log_snr=o_ls,
                 start=SO.predict_start_from_noise(rec["x_t"], t, noise, schedule, f64), post_mean=o_mean, post_var=o_var, post_logvar=o_logvar,
                 post_mean_default=o_mean, post_var_default=o_var, post_logvar_default=o_logvar,
                 x_half=SO.q_sample(x_0, torch.full((6,), 0.5), noise, schedule, f64)[0])
    sch = GaussianDiffusionContinuousTimes(noise_schedule=schedule, timesteps=8)
    td, tnd, x0d, nzd, xtd = (v.to(DEV) for v in (t, t_next, x_0, noise, rec["x_t"]))
    with guard(0xFF) as g:
        x_t, ls, alpha, sigma = sch.q_sample(x0d, td, nzd)
        mean, var, logvar = sch.q_posterior(x0d, xtd, td, tnd)
        mean_d, var_d, logvar_d = sch.q_posterior(x0d, xtd, td)
        got = dict(x_t=x_t, qs_log_snr=ls, qs_alpha=alpha, qs_sigma=sigma, log_snr=sch.get_condition(td), start=sch.predict_start_from_noise(xtd, td, nzd),
                   post_mean=mean, post_var=var, post_logvar=logvar, post_mean_default=mean_d, post_var_default=var_d, post_logvar_default=logvar_d,
                   x_half=sch.q_sample(x0d, 0.5, nzd)[0])
        g.check()
        got = {k: v.cpu() for k, v in got.items()}
        g.release()
    failures = []
    for k, v in got.items():
        assert v.shape == rec[k].shape and v.dtype == torch.float32 and torch.isfinite(v).all(), k
        bound, d = _per_sample_bound(rec[k], ref64[k])
        err = (v.double() - rec[k].double()).abs().reshape(6, -1)
        worst = err.amax(1)
        print(f"ct_scheduler module/{schedule}/{k}: dist per t = {[f'{e:.2e}' for e in worst.tolist()]} "
              f"reference fp32-fp64 per t = {[f'{e:.2e}' for e in d.tolist()]}")
        if not (err <= bound.reshape(6, 1)).all():
            failures.append(k)
    assert not failures, failures


# ---- ContinuousDiffusionOsuFusionDiT -------------------------------------------------------------------------------------------------
def _backbone_kwargs(name):
    m = META[name]
    kw = dict(dim_h=m["dim_h"], depth=m["depth"], attn_dim_head=m["attn_dim_head"], attn_heads=m["attn_heads"], attn_qk_norm=m["attn_qk_norm"])
    if name.startswith("mmdit"):
        kw.update(backbone="mmdit", patch_size=m["patch_size"], attn_kv_heads=m["attn_kv_heads"])
    else:
        kw.update(backbone="dit")
    return kw


def _model(name, **kw):
    model = ContinuousDiffusionOsuFusionDiT(**_backbone_kwargs(name), **kw)
    model.load_state_dict({k: torch.from_numpy(param_pattern(k[len("unet."):], tuple(v.shape)).copy()) for k, v in model.state_dict().items()})
    return model.to(DEV)


def _inputs(name):
    m = META[name]
    return [torch.from_numpy(v).to(DEV) for v in synth_inputs(name, m["B"], m["L"])]          # x, a, c, t, noise


def _plain_loop(model, a, c, x, cond_scale, schedule):
    """What a user writes from the public pieces: get_sampling_timesteps, get_condition, forward_with_cond_scale (two batch-B forwards),
    and the step's formula in plain torch (the fp32 restatement), drawing noise as sample()'s docstring says."""
    b = a.shape[0]
    pairs = model.scheduler.get_sampling_timesteps(b, torch.device(DEV))
    x = x.float().contiguous()
    with torch.inference_mode(), forced_compute_dtype(torch.float32):
        for i, pair in enumerate(pairs):
            t, t_next = pair[0].contiguous(), pair[1].contiguous()
            pred = model.unet.forward_with_cond_scale(x, a, model.scheduler.get_condition(t), c, cond_scale=cond_scale)
            noise = torch.randn(x.shape, device=DEV) if i < len(pairs) - 1 else None
            row = SO.stack_row(SO.schedule_row(t.cpu(), t_next.cpu(), schedule)).to(DEV)
            x = SO.ct_step(x, pred, None, 1.0, row, noise, dtype=torch.float32)[0]
    return x


@pytest.mark.parametrize("cond_scale", [1.0, 7.0])
@pytest.mark.parametrize("name", NAMES)
def test_sampler_equals_the_plain_loop(name, cond_scale):
    """Three steps (the last one has t_next = 0 and no noise), held to the bound of the DDIM sampler's comparison
    (tests/test_transformer_sampling_gpu.py::_assert_near_plain): the step adds fp32 elementwise work to the same backbone calls."""
    model = _model(name, sampling_timesteps=3)
    _, a, c, _, x = _inputs(name)
    torch.manual_seed(1234)
    with forced_compute_dtype(torch.float32):
        got = model.sample(a, c, x, cond_scale=cond_scale)
    torch.manual_seed(1234)
    want = _plain_loop(model, a, c, x, cond_scale, "cosine")
    e2, em = rell2(got, want), relmax(got, want)
    print(f"ct_scheduler sample_vs_plain/{name}/cfg{cond_scale}: rel_l2={e2:.3e} relmax={em:.3e}")
    assert got.shape == x.shape and got.dtype == torch.float32 and torch.isfinite(got).all()
    assert e2 < PLAIN_RL2 and em < PLAIN_RMAX, (e2, em)


@pytest.mark.parametrize("name", NAMES)
def test_one_step_vs_fp64_restatement(name):
    """x1 of the first step of a linear schedule (t = 1 -> 2/3) against the fp64 backbone restatement (tests/dit_oracle.py,
    tests/mmdit_oracle.py) conditioned on the same fp32 log_snr, and the fp64 step; the bound is the restatement tests' 1e-3, on x1 and on
    the prediction recovered from x1 where the start prediction is not clamped (x1 is affine in eps there)."""
    cond_scale = 2.0
    model = _model(name, sampling_timesteps=3, noise_schedule="linear")
    _, a, c, _, x = _inputs(name)
    model.stop_after = 1
    torch.manual_seed(77)
    with forced_compute_dtype(torch.float32):
        x1 = model.sample(a, c, x, cond_scale=cond_scale).double().cpu()
    torch.manual_seed(77)
    noise = torch.randn(x.shape, device=DEV).cpu()
    b = a.shape[0]
    pair = model.scheduler.get_sampling_timesteps(b, torch.device(DEV))[0]
    row = ops.ct_schedule(pair[0].contiguous(), pair[1].contiguous(), ct.KINDS["linear"]).cpu()
    m = META[name]
    p = {k[len("unet."):]: v.detach().cpu().double() for k, v in model.state_dict().items()}
    tb = row[:, ct.LOG_SNR].double()
    if name.startswith("mmdit"):
        cfg = mmdit_oracle.MMDiTConfig(dim_h=m["dim_h"], depth=m["depth"], patch_size=m["patch_size"], heads=m["attn_heads"],
                                       kv_heads=m["attn_kv_heads"], dim_head=m["attn_dim_head"], qk_norm=m["attn_qk_norm"])
        fwd = lambda keep: mmdit_oracle.mmdit_forward(p, cfg, x.cpu(), a.cpu(), tb, c.cpu(), keep=keep)
    else:
        cfg = dit_oracle.DiTConfig(dim_h=m["dim_h"], depth=m["depth"], heads=m["attn_heads"], dim_head=m["attn_dim_head"], qk_norm=m["attn_qk_norm"])
        fwd = lambda keep: dit_oracle.dit_forward(p, cfg, x.cpu(), a.cpu(), tb, c.cpu(), keep=keep)
    with torch.no_grad():
        cond, null = fwd(torch.ones(b, dtype=torch.bool)).double(), fwd(torch.zeros(b, dtype=torch.bool)).double()
    eps = null + (cond - null) * cond_scale
    ref_x1, _, clamped = SO.ct_step(x.cpu(), eps, None, 1.0, row, noise)
    k = [row[:, i].double().reshape(-1, 1, 1) for i in range(13)]
    xd = x.double().cpu()
    inside = ~clamped
    got_eps = (xd - (x1 - k[10] * xd - k[12] * noise.double()) / (k[11] * k[9])) / k[2]
    e_x1, e_eps = rell2(x1, ref_x1), rell2(got_eps[inside], eps[inside])
    print(f"ct_scheduler step_vs_fp64/{name}: x1 rel_l2={e_x1:.3e} recovered prediction rel_l2={e_eps:.3e} ({int(inside.sum())} unclamped of {inside.numel()})")
    assert inside.sum() >= 8
    assert e_x1 < RESTATEMENT_RL2 and e_eps < RESTATEMENT_RL2, (e_x1, e_eps)


@pytest.mark.parametrize("name", NAMES)
def test_loss_with_is_the_mse_of_the_backbones_forward_at_log_snr(name):
    model = _model(name)
    x, a, c, _, noise = _inputs(name)
    times = torch.linspace(0.2, 0.7, x.shape[0], device=DEV)
    orig_len = torch.tensor([x.shape[-1], x.shape[-1] - 17])
    x_t, log_snr, _, _ = model.scheduler.q_sample(x, times, noise)
    assert torch.equal(log_snr, model.scheduler.get_condition(times))
    torch.manual_seed(11)
    got = model.loss_with(x, a, c, noise, times, orig_len)
    torch.manual_seed(11)                                   # the same condition-drop mask
    want = _MSEFn.apply(model.unet(x_t, a, log_snr.contiguous(), c, cond_drop_prob=model.cond_drop_prob), noise.float(), orig_len)
    assert got.grad_fn is not None and torch.isfinite(got).item() and got.item() > 0
    assert torch.equal(got.detach(), want.detach())
    torch.manual_seed(3)
    assert torch.isfinite(model(x, a, c, orig_len)).item()                                  # forward(): its own draws


@pytest.mark.parametrize("name", NAMES)
def test_bf16_loss_backward_under_memguard(name):
    model = _model(name)
    model.set_full_bf16()
    x, a, c, _, noise = _inputs(name)
    times = torch.linspace(0.2, 0.7, x.shape[0], device=DEV)
    with guard(0xFF) as g:
        loss = model.loss_with(x, a, c, noise, times)
        loss.backward()
        torch.cuda.synchronize()
        g.check()
        assert torch.isfinite(loss).item()
        for k, p in model.named_parameters():
            assert p.grad is None or torch.isfinite(p.grad).all(), k
        first_attn = next(p for k, p in model.named_parameters() if k.startswith("unet.blocks.0.attn.to_q"))
        assert model.unet.null_cond.grad is not None and first_attn.grad is not None
        g.release()


@pytest.mark.parametrize("name", NAMES)
def test_sampling_is_repeatable_bit_for_bit(name):
    model = _model(name, sampling_timesteps=3)
    _, a, c, _, x = _inputs(name)

    def run(start):
        torch.manual_seed(99)
        return model.sample(a, c, start, cond_scale=7.0)
    for start in (x, None):                                 # a given start iterate, and one drawn from the seed
        outs = [run(start) for _ in range(2)]
        assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])
    model.set_full_bf16()
    outs = [run(x) for _ in range(2)]
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("name,per_step", [("mmdit_h96", 2), ("dit_h96", 2)])
def test_sampler_step_issues_one_attention_launch_per_block_and_one_ct_step(name, per_step):
    model = _model(name, sampling_timesteps=4)
    assert len(model.unet.blocks) == per_step
    _, a, c, _, x = _inputs(name)
    for stop_after in (1, 2):
        model.stop_after = stop_after
        timer = ops.KernelTimer(["osuf_gqa_fwd", "osuf_mqa_fwd", "osuf_ct_step", "osuf_ct_schedule"])
        ops.set_kernel_timer(timer)
        try:
            model.sample(a, c, x, cond_scale=7.0)
        finally:
            ops.set_kernel_timer(None)
        got = {k: v["launches"] for k, v in timer.summary().items()}
        assert got == {"osuf_gqa_fwd": per_step * stop_after, "osuf_ct_step": stop_after, "osuf_ct_schedule": 1}, got
