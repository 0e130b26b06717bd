"""DDIM(eta) and DPM-Solver++(2M) on the GPU: osuf_ct_solver_schedule against ops.ct_schedule (bits) and the fp64 restatement (factors),
osuf_ct_solver_step against fp64 of its own formula on the kernel's fp32 rows, the identities between the two samplers and with
osuf_ct_step_ex, the whole loop on the Gaussian toy problem, and ContinuousDiffusionOsuFusionDiT(sampler=...) against the loop written out.
The yardstick is tests/ct_solver_oracle.py.  Inputs and outputs are poisoned and canary-guarded (tests/memguard.py)."""
import numpy as np
import pytest
import torch

from osufusion_amd import ct, ops
from osufusion_amd.models import ContinuousDiffusionOsuFusionDiT
from osufusion_amd.modules import GaussianDiffusionContinuousTimes
from osufusion_amd.pattern import param_pattern, synth_inputs
from tests import ct_solver_oracle as SV
from tests.memguard import guard

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 2.0 ** -24
OBJECTIVES = ("noise", "x_start", "v")
SOLVERS = (("ddim", 0.0), ("ddim", 0.5), ("ddim", 1.0), ("dpmpp_2m", 0.0))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _grid(schedule, spacing, steps, logsnr_min=-15.0):
    return GaussianDiffusionContinuousTimes(schedule).solver_log_snr_grid(steps, spacing, logsnr_min, device=DEV)


# ---- osuf_ct_solver_schedule -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spacing", ["logsnr", "time"])
@pytest.mark.parametrize("schedule", ["linear", "cosine"])
def test_schedule_rows_are_ct_schedule_rows(schedule, spacing):
    """S = 7, B = 3.  The rows do not depend on the sampler and are the same for every sample; columns 3-5 of step i are columns 0-2 of step
    i + 1, bit for bit.  On the time grid a step is a (t, t_next) pair of ops.ct_schedule: all 13 columns are bit-equal to its row (the last
    step has t_next = 0, gain 0).  On the log-SNR grid only the two ends are a log_snr(t): columns 0 and 3 are the grid itself, the ends'
    alpha and sigma are ops.ct_schedule's bit for bit, and alpha, sigma, 1 / alpha in between are held to fp64 at 4 * 2^-24 relative (exp, +, /
    and sqrt: 2.5 roundings; the reciprocal one more)."""
    S, B = 7, 3
    sch = GaussianDiffusionContinuousTimes(schedule)
    with guard(0xFF) as g:
        grid = g.place(_grid(schedule, spacing, S))
        rows, _ = ops.ct_solver_schedule(grid, "ddim", 0.0, B)
        rows_2m, _ = ops.ct_solver_schedule(grid, "dpmpp_2m", 0.0, B)
        g.check()
        rows, rows_2m, grid = rows.cpu(), rows_2m.cpu(), grid.cpu()
        g.release()
    assert rows.shape == (S, B, 13) and rows.dtype == torch.float32 and torch.isfinite(rows).all()
    assert torch.equal(_bits(rows), _bits(rows_2m))
    assert all(torch.equal(_bits(rows[:, b]), _bits(rows[:, 0])) for b in range(B))
    r = rows[:, 0]
    assert torch.equal(_bits(r[:, 0]), _bits(grid[:-1])) and torch.equal(_bits(r[:, 3]), _bits(grid[1:]))
    assert torch.equal(_bits(r[:-1, 3:6]), _bits(r[1:, 0:3]))
    assert (grid[1:] > grid[:-1]).all() and (r[:-1, 12] > 0).all() and r[-1, 12] == 0
    if spacing == "time":
        t = torch.linspace(1.0, 0.0, S + 1, device=DEV)
        want = sch.coefficients(t[:-1], t[1:]).cpu()
        assert torch.equal(_bits(r), _bits(want))
    else:
        ends = sch.coefficients(torch.tensor([1.0, 0.0], device=DEV)).cpu()
        assert grid[0] == max(ends[0, 0].item(), -15.0) and grid[-1] == ends[1, 0]
        assert torch.equal(_bits(r[-1, 3:6]), _bits(ends[1]))
        if ends[0, 0] >= -15.0:                                                            # linear: log_snr(1) = -10, not clamped
            assert torch.equal(_bits(r[0, 0:3]), _bits(ends[0]))
        want = SV.rows(grid)
        for j in (1, 2, 4, 5, 9):
            err = np.abs(r[:, j].double().numpy() - want[:, j]) / want[:, j]
            assert err.max() <= 4 * EPS, (j, err.max() / EPS)


@pytest.mark.parametrize("sampler,eta", SOLVERS, ids=[f"{s}-{e}" for s, e in SOLVERS])
@pytest.mark.parametrize("steps", [7, 300], ids=["S7", "S300"])
@pytest.mark.parametrize("spacing", ["logsnr", "time"])
@pytest.mark.parametrize("schedule", ["linear", "cosine"])
def test_schedule_factors_against_fp64(schedule, spacing, steps, sampler, eta):
    """k_x, k_0, k_p, gain against the restatement fed the kernel's own fp32 grid.  The bound is the issue's: 8 * 2^-24 relative on k_x and
    gain, and 8 * 2^-24 * max(1, |k_d| (1 + 1 / (2r))) absolute on k_0 and k_p.  S = 300 is two workgroups of the one-thread-per-step kernel."""
    with guard(0xFF) as g:
        grid = g.place(_grid(schedule, spacing, steps))
        _, fac = ops.ct_solver_schedule(grid, sampler, eta, 2)
        _, again = ops.ct_solver_schedule(grid, sampler, eta, 1)
        g.check()
        fac, again, grid = fac.cpu(), again.cpu(), grid.cpu()
        g.release()
    assert fac.shape == (steps, 4) and torch.isfinite(fac).all() and torch.equal(_bits(fac), _bits(again))
    want, scale = SV.factors(grid, sampler, float(np.float32(eta)))
    got = fac.double().numpy()
    bound = 8 * EPS
    rel = {j: np.abs(got[:, j] - want[:, j]) / np.where(want[:, j] != 0, np.abs(want[:, j]), 1.0) / bound for j in (SV.K_X, SV.GAIN)}
    ab = {j: np.abs(got[:, j] - want[:, j]) / (bound * scale) for j in (SV.K_0, SV.K_P)}
    print(f"ct_solver factors/{schedule}/{spacing}/S{steps}/{sampler}/{eta}: max err / bound  k_x {rel[SV.K_X].max():.3f}  k_0 {ab[SV.K_0].max():.3f}  "
          f"k_p {ab[SV.K_P].max():.3f}  gain {rel[SV.GAIN].max():.3f}")
    for j, v in {**rel, **ab}.items():
        assert v.max() <= 1.0, (j, int(v.argmax()), got[int(v.argmax())], want[int(v.argmax())])
    if sampler == "ddim":
        assert (fac[:, SV.K_P] == 0).all() and ((fac[:, SV.GAIN] == 0).all() if eta == 0 else (fac[:, SV.GAIN] > 0).all())
    else:
        assert fac[0, SV.K_P] == 0 and (fac[1:, SV.K_P] < 0).all() and (fac[:, SV.GAIN] == 0).all()


# ---- osuf_ct_solver_step -----------------------------------------------------------------------------------------------------------------
def step_inputs(B, per_sample, seed=5):
    """N(0, 1) iterates and predictions; the null prediction lies near the conditional one, so that guidance 7 keeps p at N(0, 1)'s scale;
    a previous start prediction inside [-1, 1]."""
    g = torch.Generator().manual_seed(seed)
    x, cond, noise = (torch.randn((B, per_sample), generator=g) for _ in range(3))
    null = cond + 0.05 * torch.randn((B, per_sample), generator=g)
    prev = torch.tanh(torch.randn((B, per_sample), generator=g))
    return x, cond, null, noise, prev


def _misaligned(t):
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    buf[1:].copy_(t.flatten())
    return buf[1:].view(t.shape)


# (sampler, eta, step of the S = 7 grid, noise enters, x0_prev enters)
MODES = {"ddim0": ("ddim", 0.0, 3, False, False), "ddim_eta": ("ddim", 0.5, 3, True, False), "2m_first": ("dpmpp_2m", 0.0, 0, False, False),
         "2m_later": ("dpmpp_2m", 0.0, 3, False, True)}


@pytest.mark.parametrize("misalign", [False, True], ids=["vec", "scalar"])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("thresholded", [False, True], ids=["clamp", "threshold"])
@pytest.mark.parametrize("with_null", [False, True], ids=["cond", "guided"])
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_solver_step_against_fp64_of_its_formula(objective, with_null, thresholded, mode, misalign):
    """Both outputs against fp64 of the kernel's formula fed the kernel's own fp32 rows, factors and threshold, at the bound osuf_ct_step_ex is
    held to: 16 * 2^-24 * max(1, largest |term| of the element).  B = 3, per_sample = 222 (no multiple of 4: four-wide groups straddle two
    samples), 16-byte aligned and off by one float (the scalar path).  The operand that does not enter (noise at gain 0, x0_prev at k_p 0)
    is handed over NaN-filled: a finite result equal to the call without it shows that it is not read."""
    sampler, eta, i, z_in, prev_in = MODES[mode]
    B, per = 3, 6 * 37
    x, cond, null, noise, prev = step_inputs(B, per)
    null = null if with_null else None
    scale = 7.0 if with_null else 1.0
    nan = torch.full_like(x, float("nan"))
    with guard(0xFF) as g:
        put = (lambda v: _misaligned(v.to(DEV))) if misalign else (lambda v: g.place(v.to(DEV)))
        rows, fac = ops.ct_solver_schedule(_grid("cosine", "logsnr", 7), sampler, eta, B)
        row, f = rows[i], fac[i]
        xd, cd = put(x), put(cond)
        nd = put(null) if with_null else None
        zd, pd = put(noise if z_in else nan), put(prev if prev_in else nan)
        s = ops.ct_x0_quantile(xd, cd, nd, scale, row, objective, 0.9)[:, 2] if thresholded else None
        got, got0 = ops.ct_solver_step(xd, cd, nd, scale, row, f, pd, zd, objective, s)
        again, again0 = ops.ct_solver_step(xd, cd, nd, scale, row, f, pd, zd, objective, s)
        bare, bare0 = ops.ct_solver_step(xd, cd, nd, scale, row, f, pd if prev_in else None, zd if z_in else None, objective, s)
        g.check()
        got, got0, again, again0, bare, bare0, row_c, f_c = (v.cpu() for v in (got, got0, again, again0, bare, bare0, row, f))
        s_c = s.cpu() if thresholded else None
        g.release()
    want, want0, terms = SV.step(x, cond, null, scale, row_c, f_c, prev if prev_in else None, noise if z_in else None, objective, s_c)
    bound = 16 * EPS * np.maximum(terms, 1.0)
    err, err0 = np.abs(got.double().numpy() - want), np.abs(got0.double().numpy() - want0)
    print(f"ct_solver step/{objective}/null{int(with_null)}/thr{int(thresholded)}/{mode}/{'scalar' if misalign else 'vec'}: max err/bound x_next = "
          f"{(err / bound).max():.3f}  x0 = {(err0 / bound).max():.3f}  fac = {f_c.tolist()}" + (f"  s = {s_c.tolist()}" if thresholded else ""))
    assert torch.isfinite(got).all() and torch.isfinite(got0).all()
    assert (err <= bound).all(), (err / bound).max()
    assert (err0 <= bound).all(), (err0 / bound).max()
    assert torch.equal(_bits(got), _bits(again)) and torch.equal(_bits(got0), _bits(again0))
    assert torch.equal(_bits(got), _bits(bare)) and torch.equal(_bits(got0), _bits(bare0))
    assert (f_c[SV.GAIN] != 0) == z_in and (f_c[SV.K_P] != 0) == prev_in
    assert np.abs(want0).max() <= 1.0
    if thresholded:
        assert (s_c > 1.0).any()


@pytest.mark.parametrize("misalign", [False, True], ids=["vec", "scalar"])
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_first_2m_step_is_ddim0_on_the_device(objective, misalign):
    """The schedule kernel does NOT form the two by the same expressions -- 2M's k_0 is -alpha_n expm1(-h), DDIM's alpha_n - k_eps exp(ls / 2),
    equal in exact arithmetic only (k_x = sigma_n / sigma is the same expression, and is bit-equal) -- so x_next agrees within the step
    bound, 16 * 2^-24 * max(1, largest |term|), and x0, which does not see the factors, bit for bit.  Every step of the S = 7 grid is taken as
    a first step."""
    B, per = 3, 6 * 37
    x, cond, null, _, _ = step_inputs(B, per, seed=9)
    put = (lambda v: _misaligned(v.to(DEV))) if misalign else (lambda v: v.to(DEV))
    xd, cd, nd = put(x), put(cond), put(null)
    grid = _grid("cosine", "logsnr", 7)
    rows, fac = ops.ct_solver_schedule(grid, "ddim", 0.0, B)
    for i in range(7):
        rows_2m, fac_2m = ops.ct_solver_schedule(grid[i:i + 2], "dpmpp_2m", 0.0, B)
        assert torch.equal(_bits(rows_2m[0, :, :12]), _bits(rows[i, :, :12]))                # (column 12 is zero on a last step)
        assert torch.equal(_bits(fac_2m[0, SV.K_X]), _bits(fac[i, SV.K_X]))
        a, a0 = ops.ct_solver_step(xd, cd, nd, 2.0, rows[i], fac[i], None, None, objective)
        b, b0 = ops.ct_solver_step(xd, cd, nd, 2.0, rows_2m[0], fac_2m[0], None, None, objective)
        _, _, terms = SV.step(x, cond, null, 2.0, rows[i].cpu(), fac[i].cpu(), None, None, objective)
        d = (a.double() - b.double()).abs().cpu().numpy()
        assert (d <= 16 * EPS * np.maximum(terms, 1.0)).all(), (i, d.max())
        assert torch.equal(_bits(a0), _bits(b0))


@pytest.mark.parametrize("thresholded", [False, True], ids=["clamp", "threshold"])
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_x0_output_is_the_start_prediction_of_ct_step_ex(objective, thresholded):
    """osuf_ct_step_ex with the row's mean factors set to (0, 1) and its gain to 0 returns 0 x + 1 x0 = its clamped start prediction; the
    solver step's second output equals it (the two kernels share ct_start and the clamp)."""
    B, per = 3, 6 * 37
    x, cond, null, _, _ = step_inputs(B, per, seed=11)
    xd, cd, nd = x.to(DEV), cond.to(DEV), null.to(DEV)
    rows, fac = ops.ct_solver_schedule(_grid("linear", "logsnr", 7), "dpmpp_2m", 0.0, B)
    for i in (0, 3, 6):
        row = rows[i]
        s = ops.ct_x0_quantile(xd, cd, nd, 7.0, row, objective, 0.9)[:, 2] if thresholded else None
        ident = row.clone()
        ident[:, ct.K_X], ident[:, ct.K_X0], ident[:, ct.NOISE_GAIN] = 0.0, 1.0, 0.0
        want = ops.ct_step_ex(xd, cd, nd, 7.0, ident, None, objective, s)
        _, got = ops.ct_solver_step(xd, cd, nd, 7.0, row, fac[i], None, None, objective, s)
        assert torch.equal(got, want) and got.abs().max() <= 1.0


@pytest.mark.parametrize("per_sample", [1, 257, 6 * 40])
def test_solver_entry_points_between_canaries(per_sample):
    """Poisoned, canary-guarded outputs: every output element is written, nothing behind an allocation is (S = 1 and B * per_sample < 4
    included)."""
    B = 3
    x, cond, null, noise, prev = step_inputs(B, per_sample, seed=per_sample)
    with guard(0xFF) as g:
        outs = []
        for steps, sampler, eta in ((1, "dpmpp_2m", 0.0), (2, "dpmpp_2m", 0.0), (5, "ddim", 1.0)):
            rows, fac = ops.ct_solver_schedule(g.place(_grid("cosine", "logsnr", steps)), sampler, eta, B)
            outs += [rows, fac]
            xd, cd, nd, zd, pd = (g.place(v.to(DEV)) for v in (x, cond, null, noise, prev))
            for objective in OBJECTIVES:
                q = ops.ct_x0_quantile(xd, cd, nd, 7.0, rows[-1], objective, 0.95)
                outs += list(ops.ct_solver_step(xd, cd, nd, 7.0, rows[-1], fac[-1], pd, zd, objective, q[:, 2]))
                outs += list(ops.ct_solver_step(xd, cd, None, 1.0, rows[-1], fac[-1], None, None, objective, None))
        g.check()
        for o in outs:
            assert torch.isfinite(o).all()
        g.release()


# ---- the loop on the device: the Gaussian toy problem ------------------------------------------------------------------------------------
def _toy_denoiser_torch(x, log_snr):
    """tests/ct_solver_oracle.toy_denoiser in fp64 torch on the device, rounded to fp32."""
    ls = log_snr.double()
    a, s = torch.sigmoid(ls).sqrt(), torch.sigmoid(-ls).sqrt()
    return (SV.TOY_MEAN + a * SV.TOY_STD ** 2 / (a ** 2 * SV.TOY_STD ** 2 + s ** 2) * (x.double() - a * SV.TOY_MEAN)).float()


def _device_loop(x, grid, sampler):
    rows, fac = ops.ct_solver_schedule(grid, sampler, 0.0, x.shape[0])
    prev = None
    for i in range(grid.shape[0] - 1):
        x, prev = ops.ct_solver_step(x, _toy_denoiser_torch(x, grid[i]), None, 1.0, rows[i], fac[i], prev, None, "x_start")
    return x


@pytest.mark.parametrize("schedule", ["linear", "cosine"])
def test_toy_problem_loop_on_the_device(schedule):
    """B = 2, 6 x 341, S = 16 on the log-SNR grid.  The kernels' 2M iterate is within 1e-4 (absolute) of the fp64 restatement's loop on the
    same fp32 grid -- 16 steps of about 1e-6 each, and the problem is contractive -- and meets the CPU convergence condition against the exact
    probability-flow solution: 2M's RMS error is at most a quarter of DDIM(0)'s."""
    x = torch.randn((2, 6 * 341), generator=torch.Generator().manual_seed(0))
    grid = _grid(schedule, "logsnr", 16)
    got = {s: _device_loop(x.to(DEV), grid, s).cpu() for s in SV.SAMPLERS}
    g64 = grid.double().cpu().numpy()
    want = SV.loop(SV.toy_denoiser, x, g64, "dpmpp_2m")
    exact = SV.toy_exact(x, g64[0], g64[-1])
    d = np.abs(got["dpmpp_2m"].double().numpy() - want).max()
    e_2m, e_ddim = SV.rms(got["dpmpp_2m"], exact), SV.rms(got["ddim"], exact)
    print(f"ct_solver toy_device/{schedule}: |kernels - fp64 loop| = {d:.3e}  rms vs exact: 2m {e_2m:.3e} ddim {e_ddim:.3e} ratio {e_ddim / e_2m:.1f}")
    assert d <= 1e-4, d
    assert e_2m <= e_ddim / 4, (e_2m, e_ddim)


# ---- ContinuousDiffusionOsuFusionDiT(sampler=...) ----------------------------------------------------------------------------------------
# dim_h = 64 for the MMDiT.  The DiT's stem (CrossEmbedLayer over the 102 input channels, kernel sizes 3 / 7 / 15) gives its widest kernel
# dim_h - 51 - 25 channels, so a DiT narrower than 77 cannot be built: it runs at 96, the width of the smallest DiT fixture.
BACKBONE_KW = {"dit": dict(backbone="dit", dim_h=96, depth=2, attn_heads=6, attn_dim_head=16),
               "mmdit": dict(backbone="mmdit", dim_h=64, depth=2, attn_heads=4, attn_kv_heads=2, attn_dim_head=16)}
STEPS = 4
# sampler, ddim_eta, spacing, pred_objective, dynamic_thresholding
MODEL_CASES = {"ddim0": ("ddim", 0.0, "logsnr", "noise", False), "ddim_eta": ("ddim", 0.5, "time", "noise", False),
               "2m": ("dpmpp_2m", 0.0, "logsnr", "noise", False), "2m_v_thr": ("dpmpp_2m", 0.0, "logsnr", "v", True)}
TIMED = ["osuf_ct_solver_schedule", "osuf_ct_solver_step", "osuf_ct_x0_quantile", "osuf_ct_step", "osuf_ct_step_ex"]


def _model(backbone, **kw):
    model = ContinuousDiffusionOsuFusionDiT(**BACKBONE_KW[backbone], sampling_timesteps=STEPS, **kw)
    model.load_state_dict({k: torch.from_numpy(param_pattern(k[len("unet."):], tuple(v.shape)).copy()) for k, v in model.state_dict().items()})
    return model.to(DEV)


def _inputs(backbone):
    x, a, c, _, noise = (torch.from_numpy(v).to(DEV) for v in synth_inputs("ct_solver_" + backbone, 2, 256))
    return a, c, noise


def _solver_loop(model, a, c, x, cond_scale, seen=None):
    """sample() for the two solvers written out over ops calls; draws as its docstring says."""
    b = a.shape[0]
    cfg = cond_scale != 1.0
    x = x.float().contiguous()
    with torch.inference_mode(), ops.reproducible_mode(True), ops.one_launch_attention(True), model._dtype_ctx():
        grid = model.scheduler.solver_log_snr_grid(model.scheduler.timesteps, model.solver_spacing, model.solver_logsnr_min, device=DEV)
        rows, fac = ops.ct_solver_schedule(grid, model.sampler, model.ddim_eta, b)
        f = model._denoiser(a, c, cfg)
        prev = None
        for i in range(model.scheduler.timesteps):
            pred = f(x, grid[i].repeat(2 * b if cfg else b))
            noise = torch.randn(x.shape, device=DEV) if model.sampler == "ddim" and model.ddim_eta > 0 else None
            cond, null = pred[:b], pred[b:] if cfg else None
            s = None
            if model.dynamic_thresholding:
                s = ops.ct_x0_quantile(x, cond, null, cond_scale, rows[i], model.pred_objective, model.dynamic_thresholding_percentile)[:, 2]
                if seen is not None:
                    seen.append(s)
            x, prev = ops.ct_solver_step(x, cond, null, cond_scale, rows[i], fac[i], prev, noise, model.pred_objective, s)
    return x


@pytest.mark.parametrize("case", list(MODEL_CASES))
@pytest.mark.parametrize("backbone", ["dit", "mmdit"])
def test_model_sample_is_the_loop_written_out(backbone, case):
    """B = 2, n = 256, cond_scale 2, four steps: sample() against the loop over ops calls drawing the same way from the same seed, bit for bit
    and twice; the launches are one schedule and S steps (S quantiles more with thresholding), none of the ancestral step; the deterministic
    samplers leave both generators where they were."""
    sampler, eta, spacing, objective, thresholded = MODEL_CASES[case]
    model = _model(backbone, sampler=sampler, ddim_eta=eta, solver_spacing=spacing, pred_objective=objective, dynamic_thresholding=thresholded)
    a, c, x = _inputs(backbone)
    timer = ops.KernelTimer(TIMED)
    ops.set_kernel_timer(timer)
    try:
        torch.manual_seed(77)
        before = (torch.get_rng_state(), torch.cuda.get_rng_state())
        got = model.sample(a, c, x, cond_scale=2.0)
        after = (torch.get_rng_state(), torch.cuda.get_rng_state())
    finally:
        ops.set_kernel_timer(None)
    launches = {k: v["launches"] for k, v in timer.summary().items()}
    want_launches = {"osuf_ct_solver_schedule": 1, "osuf_ct_solver_step": STEPS}
    if thresholded:
        want_launches["osuf_ct_x0_quantile"] = STEPS
    assert launches == want_launches
    drew = not (torch.equal(before[0], after[0]) and torch.equal(before[1], after[1]))
    assert drew == (eta > 0)
    torch.manual_seed(77)
    again = model.sample(a, c, x, cond_scale=2.0)
    seen = []
    torch.manual_seed(77)
    want = _solver_loop(model, a, c, x, 2.0, seen)
    assert got.shape == x.shape and torch.isfinite(got).all()
    assert torch.equal(_bits(got), _bits(again)) and torch.equal(_bits(got), _bits(want))
    if thresholded:
        assert (torch.stack(seen) >= 1.0).all()
    torch.manual_seed(78)
    unguided = model.sample(a, c, x, cond_scale=1.0)                                        # no null branch: B rows through the backbone
    torch.manual_seed(78)
    want_unguided = _solver_loop(model, a, c, x, 1.0)
    assert torch.isfinite(unguided).all() and torch.equal(_bits(unguided), _bits(want_unguided)) and not torch.equal(unguided, got)
    model.stop_after = 2
    early = model.sample(a, c, x, cond_scale=2.0)
    model.stop_after = None
    assert torch.isfinite(early).all() and not torch.equal(early, got)


@pytest.mark.parametrize("backbone", ["dit", "mmdit"])
def test_start_iterate_is_the_only_draw_without_x(backbone):
    """x = None: the start iterate is torch.randn((B, 6, n)) from the global generator, and 2M draws nothing else."""
    model = _model(backbone, sampler="dpmpp_2m")
    a, c, _ = _inputs(backbone)
    torch.manual_seed(5)
    got = model.sample(a, c, cond_scale=2.0)
    torch.manual_seed(5)
    start = torch.randn((2, 6, 256), device=DEV)
    state = torch.cuda.get_rng_state()
    assert torch.equal(_bits(got), _bits(model.sample(a, c, start, cond_scale=2.0))) and torch.equal(state, torch.cuda.get_rng_state())


@pytest.mark.parametrize("backbone", ["dit", "mmdit"])
def test_default_sampler_is_the_ancestral_path(backbone):
    """sampler = "ddpm" (the default): sample() against ops.ct_step composed by hand over the time grid, bit for bit, and no solver launch."""
    model = _model(backbone)
    explicit = _model(backbone, sampler="ddpm", ddim_eta=1.0, solver_spacing="time")        # the solver keywords do not reach the ancestral path
    a, c, x = _inputs(backbone)
    b = a.shape[0]
    timer = ops.KernelTimer(TIMED)
    ops.set_kernel_timer(timer)
    try:
        torch.manual_seed(3)
        got = model.sample(a, c, x, cond_scale=2.0)
    finally:
        ops.set_kernel_timer(None)
    assert {k: v["launches"] for k, v in timer.summary().items()} == {"osuf_ct_step": STEPS}
    torch.manual_seed(3)
    same = explicit.sample(a, c, x, cond_scale=2.0)
    torch.manual_seed(3)
    with torch.inference_mode(), ops.reproducible_mode(True), ops.one_launch_attention(True), model._dtype_ctx():
        times = torch.linspace(1.0, 0.0, STEPS + 1, device=DEV, dtype=torch.float32)
        coef = model.scheduler.coefficients(times[:-1].repeat_interleave(b), times[1:].repeat_interleave(b)).view(STEPS, b, -1)
        log_snr = coef[:, :, 0].repeat(1, 2).contiguous()
        f = model._denoiser(a, c, True)
        want = x.float().contiguous()
        for i in range(STEPS):
            pred = f(want, log_snr[i])
            noise = torch.randn(want.shape, device=DEV) if i < STEPS - 1 else None
            want = ops.ct_step(want, pred[:b], pred[b:], 2.0, coef[i], noise)
    assert torch.isfinite(got).all() and torch.equal(_bits(got), _bits(want)) and torch.equal(_bits(got), _bits(same))
