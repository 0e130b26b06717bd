"""CPU checks of the continuous-time scheduler: the restatement (tests/scheduler_oracle.py) against the reference's recorded values
(tests/golden/scheduler_cases.npz), the time grids, the error text, the exports, the model's constructor and the C ABI of the two entry
points.  The bounds are written down in profiles/ct_scheduler_parity.md."""
import inspect
from ctypes import c_float, c_int, c_long, c_void_p
from pathlib import Path

import numpy as np
import pytest
import torch

from osufusion_amd import _lib
from tests import scheduler_oracle as SO

ROOT = Path(__file__).resolve().parent.parent
GOLD = np.load(ROOT / "tests" / "golden" / "scheduler_cases.npz")
SMALL = {"mmdit": dict(dim_h=32, depth=2, attn_heads=2, attn_kv_heads=1, attn_dim_head=16), "dit": dict(dim_h=96, depth=2, attn_heads=6, attn_dim_head=16)}


def gold(key):
    return torch.from_numpy(GOLD[key])


def oracle_arrays(schedule, dtype=torch.float32, nudge=0, nudge_next=0):
    """Every per-schedule array of the fixture from the restatement.  x_t is the recorded one downstream of q_sample (as the fixture's
    own calls had it), so each entry restates one call of the reference."""
    t, t_next, x_0, noise = gold("t"), gold("t_next"), gold("x_0"), gold("noise")
    x_t, ls, alpha, sigma = SO.q_sample(x_0, t, noise, schedule, dtype, nudge)
    rec_x_t = gold(f"{schedule}/x_t")
    mean, var, logvar = SO.q_posterior(x_0, rec_x_t, t, t_next, schedule, dtype, nudge, nudge_next)
    a1, s1 = SO.alpha_sigma(SO.log_snr(t, schedule, dtype, nudge))
    return dict(log_snr=ls, alpha=a1, sigma=s1, x_t=x_t, qs_log_snr=ls, qs_alpha=alpha, qs_sigma=sigma,
                start=SO.predict_start_from_noise(rec_x_t, t, noise, schedule, dtype, nudge),
                post_mean=mean, post_var=var, post_logvar=logvar, post_mean_default=mean, post_var_default=var, post_logvar_default=logvar,
                x_half=SO.q_sample(x_0, torch.full((x_0.shape[0],), 0.5), noise, schedule, dtype, nudge)[0])


def libm_bounds(schedule):
    """Per array and element: how far the fp32 restatement moves when cos(.) (cosine) / expm1(.) (linear) moves by +-2 ulps, at t, at
    t_next, or at both.  It stands for a different libm; it is computed from the reference formula alone."""
    base = oracle_arrays(schedule)
    bound = {k: torch.zeros_like(v) for k, v in base.items()}
    for a in (-2, 0, 2):
        for b in (-2, 0, 2):
            if (a, b) != (0, 0):
                for k, v in oracle_arrays(schedule, nudge=a, nudge_next=b).items():
                    bound[k] = torch.maximum(bound[k], (v - base[k]).abs())
    return base, bound


@pytest.mark.parametrize("schedule", SO.SCHEDULES)
def test_fp32_restatement_reproduces_the_recorded_reference(schedule):
    """The restatement rounds every function once from fp64, so it does not move with the CPU it runs on; against the recording it is
    bit-equal for the linear schedule and within the bound for the cosine one (post_mean 8.94e-07, post_var 5.59e-08, post_logvar 1.91e-06)."""
    base, bound = libm_bounds(schedule)
    assert set(base) == {k.split("/", 1)[1] for k in GOLD.files if k.startswith(schedule + "/")}
    for k, got in base.items():
        want = gold(f"{schedule}/{k}")
        assert got.dtype == torch.float32 and got.shape == want.shape, k
        assert torch.isfinite(want).all(), k
        err = (got - want).abs()
        print(f"ct_scheduler oracle/{schedule}/{k}: max|diff|={err.max().item():.3e} largest bound={bound[k].max().item():.3e}")
        assert (err <= bound[k]).all(), (k, err.max().item())


def test_the_recorded_fp32_values_are_not_the_fp64_ones():
    """The two numbers the fp32-order decision rests on: the network is conditioned on the fp32 value."""
    t = gold("t")
    ls32, ls64 = gold("cosine/log_snr"), SO.log_snr(t, "cosine", torch.float64)
    assert abs(ls32[5].item() + 33.8913) < 1e-3 and abs(ls64[5].item() + 74.66) < 1e-2
    assert abs(ls32[0].item() - 8.76919) < 1e-5 and abs(ls64[0].item() - 8.76929) < 1e-5
    assert abs(gold("cosine/alpha")[5].item() - 4.37e-8) < 1e-10


def test_time_grids_are_bit_equal():
    from osufusion_amd.modules import GaussianDiffusionContinuousTimes
    for n in (1, 8):
        sch = GaussianDiffusionContinuousTimes(timesteps=n)
        pairs = sch.get_sampling_timesteps(2, torch.device("cpu"))
        assert isinstance(pairs, tuple) and len(pairs) == n and all(p.shape == (2, 2) and p.dtype == torch.float32 for p in pairs)
        assert torch.equal(torch.stack(list(pairs)), gold(f"grid{n}"))
        assert torch.equal(SO.sampling_timesteps(n, 2), gold(f"grid{n}"))
        assert pairs[0][0].tolist() == [1.0, 1.0] and pairs[-1][1].tolist() == [0.0, 0.0]
    got = GaussianDiffusionContinuousTimes().get_times(3, 0.25, torch.device("cpu"))
    assert got.dtype == torch.float32 and torch.equal(got, gold("get_times"))
    r = GaussianDiffusionContinuousTimes().sample_random_times(5, torch.device("cpu"))
    assert r.shape == (5,) and r.dtype == torch.float32 and ((r >= 0) & (r <= 1)).all()


def test_unknown_schedule_raises_the_references_error():
    from osufusion_amd.modules.scheduler import GaussianDiffusionContinuousTimes
    with pytest.raises(ValueError, match=r"^Unknown noise schedule: sigmoid$"):
        GaussianDiffusionContinuousTimes(noise_schedule="sigmoid")
    sig = inspect.signature(GaussianDiffusionContinuousTimes.__init__)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [("noise_schedule", "linear"), ("timesteps", 1000)]
    sch = GaussianDiffusionContinuousTimes()
    assert (sch.noise_schedule, sch.timesteps) == ("linear", 1000) and not list(sch.parameters())


def test_methods_refuse_cpu_tensors():
    from osufusion_amd.modules import GaussianDiffusionContinuousTimes
    sch = GaussianDiffusionContinuousTimes("cosine")
    x = torch.zeros(2, 6, 8)
    for call in (lambda: sch.get_condition(torch.zeros(2)), lambda: sch.q_sample(x, 0.5), lambda: sch.predict_start_from_noise(x, torch.zeros(2), x),
                 lambda: sch.q_posterior(x, x, torch.ones(2))):
        with pytest.raises(RuntimeError, match="MI355X only"):
            call()


def test_exports():
    import osufusion_amd.models as models
    import osufusion_amd.modules as modules
    from osufusion_amd.models.transformer_diffusion import ContinuousDiffusionOsuFusionDiT, _TransformerOsuFusion
    from osufusion_amd.modules.scheduler import GaussianDiffusionContinuousTimes
    assert modules.GaussianDiffusionContinuousTimes is GaussianDiffusionContinuousTimes
    assert models.ContinuousDiffusionOsuFusionDiT is ContinuousDiffusionOsuFusionDiT
    assert issubclass(ContinuousDiffusionOsuFusionDiT, _TransformerOsuFusion)


@pytest.mark.parametrize("backbone", ["mmdit", "dit"])
def test_model_constructor(backbone):
    from osufusion_amd.models import ContinuousDiffusionOsuFusionDiT
    from osufusion_amd.modules import GaussianDiffusionContinuousTimes
    from osufusion_amd.modules.dit import DiT
    from osufusion_amd.modules.mmdit import MMDiT
    sig = inspect.signature(ContinuousDiffusionOsuFusionDiT.__init__)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:6]] == [
        ("dim_h", inspect.Parameter.empty), ("backbone", "mmdit"), ("cond_drop_prob", 0.5), ("noise_schedule", "cosine"), ("sampling_timesteps", 35)]
    m = ContinuousDiffusionOsuFusionDiT(backbone=backbone, **SMALL[backbone])
    assert hasattr(m, "unet") and isinstance(m.unet, {"mmdit": MMDiT, "dit": DiT}[backbone])
    assert isinstance(m.scheduler, GaussianDiffusionContinuousTimes)
    assert (m.scheduler.noise_schedule, m.scheduler.timesteps, m.sampling_timesteps, m.cond_drop_prob, m.stop_after) == ("cosine", 35, 35, 0.5, None)
    assert all(k.startswith("unet.") for k in m.state_dict())
    lin = ContinuousDiffusionOsuFusionDiT(backbone=backbone, noise_schedule="linear", sampling_timesteps=4, **SMALL[backbone])
    assert (lin.scheduler.noise_schedule, lin.scheduler.timesteps) == ("linear", 4)
    with pytest.raises(ValueError, match="Unknown noise schedule: foo"):
        ContinuousDiffusionOsuFusionDiT(backbone=backbone, noise_schedule="foo", **SMALL[backbone])
    with pytest.raises(ValueError, match="backbone"):
        ContinuousDiffusionOsuFusionDiT(32, backbone="unet")
    assert "t_next == 0" in ContinuousDiffusionOsuFusionDiT.sample.__doc__ and "step order" in ContinuousDiffusionOsuFusionDiT.sample.__doc__


def test_capi_ct_entry_points_are_declared_and_bound():
    decls = _lib.read_header()[0]
    P, L, I, F = c_void_p, c_long, c_int, c_float
    kinds = {"*": P, "hipStream_t": P, "long": L, "int": I, "float": F}
    want_names = {
        "osuf_ct_schedule": ["t", "t_next", "kind", "out", "B", "stream"],
        "osuf_ct_step": ["x", "cond", "nullp", "cond_scale", "coef", "noise", "out", "B", "per_sample", "stream"],
    }
    for name, names in want_names.items():
        assert name in decls, f"{name} is not declared in include/osufusion_hip.h"
        ret, params = decls[name]
        assert ret == "int" and [p.split()[-1].lstrip("*") for p in params] == names
        assert _lib.SIGNATURES[name] == [kinds["*" if "*" in p else p.split()[0]] for p in params], name
        assert hasattr(_lib.load(), name)
    from osufusion_amd import ct, ops
    assert callable(ops.ct_schedule) and callable(ops.ct_step)
    assert len(SO.COLUMNS) == ct.COLS == 13 and SO.COLUMNS.index("noise_gain") == ct.NOISE_GAIN and SO.COLUMNS.index("k_x") == ct.K_X
