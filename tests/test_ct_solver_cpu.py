"""CPU checks of the DDIM / DPM-Solver++(2M) samplers on the continuous-time log-SNR parameterisation: the algebra of the fp64 restatement
(tests/ct_solver_oracle.py) against the reference scheduler's posterior (tests/scheduler_oracle.py), the convergence conditions on the
Gaussian toy problem, the C ABI of the two new entry points and the constructor's new keywords."""
import inspect

import numpy as np
import pytest
import torch

from osufusion_amd import _lib, ct
from osufusion_amd.models import ContinuousDiffusionOsuFusionDiT
from osufusion_amd.modules import GaussianDiffusionContinuousTimes
from tests import ct_solver_oracle as SV
from tests import scheduler_oracle as SO

SMALL = {"mmdit": dict(dim_h=32, depth=2, attn_heads=2, attn_kv_heads=1, attn_dim_head=16), "dit": dict(dim_h=96, depth=2, attn_heads=6, attn_dim_head=16)}


def grid_of(schedule: str, spacing: str, steps: int, logsnr_min: float = -15.0) -> np.ndarray:
    """What GaussianDiffusionContinuousTimes.solver_log_snr_grid returns, from the fp32 restatement of the schedule."""
    if spacing == "time":
        return SO.log_snr(torch.linspace(1.0, 0.0, steps + 1), schedule).double().numpy()
    ends = SO.log_snr(torch.tensor([1.0, 0.0]), schedule)
    return torch.linspace(max(ends[0].item(), logsnr_min), ends[1].item(), steps + 1, dtype=torch.float32).double().numpy()


def textbook_ddim(grid, eta):
    """DDIM(eta)'s factors as the issue writes them.  sigma_n^2 - sigma_eta^2 and 1 - alpha^2 / alpha_n^2 cancel (at eta = 1 over a long step,
    and over a short step), which is why the restatement evaluates the equivalent sums; the two are compared where neither cancels much."""
    ls, lsn = grid[:-1], grid[1:]
    (a, s), (an, sn) = SV.alpha_sigma(ls), SV.alpha_sigma(lsn)
    s_eta = eta * np.sqrt(np.maximum((sn ** 2 / s ** 2) * (1 - a ** 2 / an ** 2), 0.0))
    k_eps = np.sqrt(np.maximum(sn ** 2 - s_eta ** 2, 0.0))
    return np.stack([k_eps / s, an - k_eps * a / s, np.zeros_like(s), s_eta], axis=1)


# ---- oracle algebra ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", SO.SCHEDULES)
@pytest.mark.parametrize("eta", [0.0, 0.5, 1.0])
def test_restated_ddim_factors_are_the_textbook_ones(schedule, eta):
    """On the log-SNR grid (steps of about 1.5 in log-SNR: no cancellation beyond a few digits) the restatement's sums equal the issue's
    differences to 1e-12 relative (k_0: absolute, it is a difference of two values of at most one in both forms)."""
    grid = grid_of(schedule, "logsnr", 16)
    got, want = SV.factors(grid, "ddim", eta)[0], textbook_ddim(grid, eta)
    for j in (SV.K_X, SV.GAIN):
        assert np.abs(got[:, j] - want[:, j]).max() <= 1e-12 * np.abs(want[:, j]).max()
        assert (np.abs(got[:, j] - want[:, j]) <= 1e-12 * np.abs(want[:, j])).all()
    assert np.abs(got[:, SV.K_0] - want[:, SV.K_0]).max() <= 1e-12
    assert (got[:, SV.K_P] == 0).all() and ((got[:, SV.GAIN] == 0).all() if eta == 0 else (got[:, SV.GAIN] > 0).all())


@pytest.mark.parametrize("spacing", ["logsnr", "time"])
@pytest.mark.parametrize("schedule", SO.SCHEDULES)
def test_ddim0_is_the_first_2m_step(schedule, spacing):
    """sigma_n / sigma and alpha_n - sigma_n alpha / sigma against -alpha_n expm1(-h): every step of the grid taken as a first step."""
    grid = grid_of(schedule, spacing, 16)
    ddim = SV.factors(grid, "ddim", 0.0)[0]
    for i in range(16):
        first = SV.factors(grid[i:i + 2], "dpmpp_2m")[0][0]
        assert first[SV.K_P] == 0 and first[SV.GAIN] == 0 and ddim[i, SV.GAIN] == 0
        assert abs(ddim[i, SV.K_X] - first[SV.K_X]) <= 1e-12 * first[SV.K_X]
        assert abs(ddim[i, SV.K_0] - first[SV.K_0]) <= 1e-12 * max(first[SV.K_0], 1.0), (i, ddim[i, SV.K_0], first[SV.K_0])
    later = SV.factors(grid, "dpmpp_2m")[0][1:]
    assert (later[:, SV.K_P] < 0).all() and (later[:, SV.K_0] > 0).all()                    # second order from the second step on


@pytest.mark.parametrize("spacing", ["logsnr", "time"])
@pytest.mark.parametrize("schedule", SO.SCHEDULES)
def test_ddim1_is_the_reference_posterior(schedule, spacing):
    """gain^2 = the posterior variance sigma_n^2 (-expm1(ls - ls_n)) and, for a given x0, the DDIM(1) mean = q_posterior's mean, in fp64
    against the restatement of the reference scheduler on the same times (tests/scheduler_oracle.py)."""
    steps = 16
    if spacing == "time":
        t = torch.linspace(1.0, 0.0, steps + 1, dtype=torch.float64)[1:-1]                  # without t = 1: q_posterior divides by alpha(t)
        t_next = t - 1.0 / steps
        ls, lsn = SO.log_snr(t, schedule, torch.float64).numpy(), SO.log_snr(t_next, schedule, torch.float64).numpy()
    else:
        grid = grid_of(schedule, "logsnr", steps)
        ls, lsn = grid[:-1], grid[1:]
        t = t_next = None
    rng = np.random.default_rng(4)
    x0, x_t = np.tanh(rng.standard_normal((len(ls), 6, 11))), rng.standard_normal((len(ls), 6, 11))
    for i in range(len(ls)):
        fac = SV.factors(np.array([ls[i], lsn[i]]), "ddim", 1.0)[0][0]
        _, sn = SV.alpha_sigma(lsn[i])
        var = sn ** 2 * -np.expm1(ls[i] - lsn[i])
        assert abs(fac[SV.GAIN] ** 2 - var) <= 1e-12 * var
        mean = fac[SV.K_X] * x_t[i] + fac[SV.K_0] * x0[i]
        row = SV.rows(np.array([ls[i], lsn[i]]))[0]
        want = row[10] * x_t[i] + row[11] * x0[i]                                           # the ancestral columns of the solver's own row
        assert np.abs(mean - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
        if t is not None:
            ref_mean, ref_var, _ = SO.q_posterior(torch.from_numpy(x0[i:i + 1]), torch.from_numpy(x_t[i:i + 1]), t[i:i + 1], t_next[i:i + 1], schedule,
                                                  torch.float64)
            assert np.abs(mean - ref_mean[0].numpy()).max() <= 1e-12 * max(1.0, ref_mean.abs().max().item())
            assert abs(fac[SV.GAIN] ** 2 - ref_var.item()) <= 1e-12 * ref_var.item()


def test_oracle_step_terms_and_unread_operands():
    rng = np.random.default_rng(1)
    x, cond, prev, z = (rng.standard_normal((3, 6, 5)) for _ in range(4))
    row = np.broadcast_to(SV.rows(np.array([-1.0, 0.5]))[0], (3, 13))
    fac = np.array([0.7, 0.4, 0.0, 0.0])
    nan = np.full_like(x, np.nan)
    out, x0, terms = SV.step(x, cond, None, 1.0, row, fac, nan, nan, "x_start")
    assert np.isfinite(out).all() and (x0 == np.clip(cond, -1, 1)).all() and (terms >= np.abs(out)).all()
    out2, _, _ = SV.step(x, cond, None, 1.0, row, np.array([0.7, 0.4, -0.2, 0.3]), prev, z, "x_start")
    np.testing.assert_allclose(out2, out - 0.2 * prev + 0.3 * z, rtol=1e-14)


# ---- convergence on the toy problem ------------------------------------------------------------------------------------------------------
def _toy_errors(schedule, steps, spacing="logsnr"):
    x = torch.randn(4096, generator=torch.Generator().manual_seed(0), dtype=torch.float64).numpy().reshape(1, -1)
    grid = grid_of(schedule, spacing, steps)
    exact = SV.toy_exact(x, grid[0], grid[-1])
    return {s: SV.rms(SV.loop(SV.toy_denoiser, x, grid, s), exact) for s in SV.SAMPLERS}


@pytest.mark.parametrize("schedule", SO.SCHEDULES)
def test_2m_converges_at_second_order_on_the_toy_problem(schedule):
    """Gaussian data N(0.2, 0.1^2) per element, 4096 standard-normal starts (seed 0), the log-SNR grid with logsnr_min = -15, fp64: the RMS
    distance to the exact probability-flow solution.  2M is at most 1/4 of DDIM(0) at S = 16 and 35 (measured ratios 9.6 to 18), and 2M at
    16 steps is below DDIM(0) at 40."""
    err = {s: _toy_errors(schedule, s) for s in (16, 35, 40)}
    print(f"ct_solver toy/{schedule}: " + "  ".join(f"S={s}: ddim {e['ddim']:.3e} 2m {e['dpmpp_2m']:.3e}" for s, e in err.items()))
    for s in (16, 35):
        assert err[s]["dpmpp_2m"] <= err[s]["ddim"] / 4, (s, err[s])
    assert err[16]["dpmpp_2m"] < err[40]["ddim"]
    assert err[35]["ddim"] < err[16]["ddim"] and err[35]["dpmpp_2m"] < err[16]["dpmpp_2m"]


def test_toy_exact_solution_is_the_limit_of_ddim():
    """The closed form against the solver itself: DDIM(0)'s error falls as 1 / S (a first-order method) towards it."""
    e = [_toy_errors("cosine", s)["ddim"] for s in (100, 200)]
    assert 1.8 < e[0] / e[1] < 2.2, e


# ---- C ABI -------------------------------------------------------------------------------------------------------------------------------
def test_capi_solver_entry_points_are_declared_and_bound():
    decls, consts = _lib.read_header()
    want = {
        "osuf_ct_solver_schedule": ["log_snr", "steps", "sampler", "eta", "rows", "fac", "B", "stream"],
        "osuf_ct_solver_step": ["x", "cond", "nullp", "cond_scale", "coef", "fac", "x0_prev", "noise", "objective", "s", "s_ld", "x_next", "x0", "B",
                                "per_sample", "stream"],
    }
    for name, names in want.items():
        assert name in decls, f"{name} is not declared in include/osufusion_hip.h"
        assert decls[name][0] == "int" and [p.split()[-1].lstrip("*") for p in decls[name][1]] == names
        assert len(_lib.SIGNATURES[name]) == len(names)
        assert hasattr(_lib.load(), name)
    for j, name in enumerate(("DDIM", "DPMPP_2M")):
        assert consts[f"OSUF_CT_SAMPLER_{name}"] == j
    assert ct.SAMPLERS == {"ddim": 0, "dpmpp_2m": 1}
    from osufusion_amd import ops
    assert all(callable(getattr(ops, n)) for n in ("ct_solver_schedule", "ct_solver_step"))


def test_capi_solver_entry_points_validate_on_the_host():
    """Every call returns before a launch (the "pointers" are never dereferenced): -1 invalid argument, -2 unknown sampler."""
    lib = _lib.load()
    buf = 4096

    def schedule(**kw):
        a = dict(log_snr=buf, steps=7, sampler=0, eta=0.5, rows=buf, fac=buf, B=2)
        a.update(kw)
        return lib.osuf_ct_solver_schedule(a["log_snr"], a["steps"], a["sampler"], a["eta"], a["rows"], a["fac"], a["B"], None)

    for kw in (dict(steps=0), dict(steps=-1), dict(B=0), dict(log_snr=None), dict(rows=None), dict(fac=None), dict(eta=-0.1), dict(eta=1.5),
               dict(eta=float("nan"))):
        assert schedule(**kw) == -1, kw
    assert schedule(sampler=2) == -2 and schedule(sampler=-1) == -2

    def step(**kw):
        a = dict(x=buf, cond=buf, nullp=None, coef=buf, fac=buf, prev=None, noise=None, objective=0, s=None, s_ld=0, x_next=buf, x0=2 * buf, B=2, per=24)
        a.update(kw)
        return lib.osuf_ct_solver_step(a["x"], a["cond"], a["nullp"], 1.0, a["coef"], a["fac"], a["prev"], a["noise"], a["objective"], a["s"], a["s_ld"],
                                       a["x_next"], a["x0"], a["B"], a["per"], None)

    for kw in (dict(B=0), dict(per=0), dict(x=None), dict(cond=None), dict(coef=None), dict(fac=None), dict(x_next=None), dict(x0=None),
               dict(x0=buf), dict(objective=3), dict(objective=-1), dict(s=buf, s_ld=0)):
        assert step(**kw) == -1, kw


# ---- the model's keywords ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backbone", ["mmdit", "dit"])
def test_constructor_sampler_keywords_and_validation(backbone):
    sig = inspect.signature(ContinuousDiffusionOsuFusionDiT.__init__)
    got = {k: sig.parameters[k].default for k in ("sampler", "ddim_eta", "solver_spacing", "solver_logsnr_min")}
    assert got == {"sampler": "ddpm", "ddim_eta": 0.0, "solver_spacing": "logsnr", "solver_logsnr_min": -15.0}
    kw = SMALL[backbone]
    plain = ContinuousDiffusionOsuFusionDiT(backbone=backbone, **kw)
    explicit = ContinuousDiffusionOsuFusionDiT(backbone=backbone, sampler="ddpm", **kw)
    new = {"sampler", "ddim_eta", "solver_spacing", "solver_logsnr_min"}
    scalars = lambda m: {k: v for k, v in vars(m).items() if not k.startswith("_") and k not in new}
    assert scalars(plain) == scalars(explicit)
    assert (plain.sampler, plain.ddim_eta, plain.solver_spacing, plain.solver_logsnr_min) == ("ddpm", 0.0, "logsnr", -15.0)
    assert (plain.pred_objective, plain.dynamic_thresholding, plain.sampling_timesteps, plain.scheduler.timesteps, plain.stop_after) == \
        ("noise", False, 35, 35, None)
    m = ContinuousDiffusionOsuFusionDiT(backbone=backbone, sampler="dpmpp_2m", sampling_timesteps=16, solver_spacing="time", solver_logsnr_min=-12.0, **kw)
    assert (m.sampler, m.solver_spacing, m.solver_logsnr_min, m.scheduler.timesteps) == ("dpmpp_2m", "time", -12.0, 16)
    assert ContinuousDiffusionOsuFusionDiT(backbone=backbone, sampler="ddim", ddim_eta=1.0, **kw).ddim_eta == 1.0
    assert list(m.state_dict()) == list(plain.state_dict())                    # no new parameters or buffers
    with pytest.raises(ValueError, match="sampler"):
        ContinuousDiffusionOsuFusionDiT(backbone=backbone, sampler="euler", **kw)
    with pytest.raises(ValueError, match="spacing"):
        ContinuousDiffusionOsuFusionDiT(backbone=backbone, solver_spacing="karras", **kw)
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError, match="eta"):
            ContinuousDiffusionOsuFusionDiT(backbone=backbone, ddim_eta=bad, **kw)


def test_scheduler_solver_methods_validate_and_refuse_cpu_tensors():
    sch = GaussianDiffusionContinuousTimes("cosine")
    with pytest.raises(ValueError, match="spacing"):
        sch.solver_log_snr_grid(8, "karras")
    with pytest.raises(ValueError, match="steps"):
        sch.solver_log_snr_grid(0)
    with pytest.raises(RuntimeError, match="MI355X only"):
        sch.solver_coefficients(torch.linspace(-15.0, 9.0, 8))
    with pytest.raises(ValueError, match="solver"):
        ct.sampler_code("ddpm")
    assert ct.sampler_code("ddim") == 0 and ct.sampler_code(1) == 1
