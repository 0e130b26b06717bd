"""CPU checks of the v / x_start objectives, min-SNR-gamma weights and dynamic thresholding: the algebra of the fp64 restatement
(tests/ct_objectives_oracle.py; the two fp64 algebra tests check the yardstick against itself), GaussianDiffusionContinuousTimes.loss_weight / .dynamic_threshold (plain torch, any device), the host
side of the quantile (ct.quantile_rank), the constructor's validation and the C ABI of the new entry points."""
import inspect

import numpy as np
import pytest
import torch

from osufusion_amd import _lib, ct
from osufusion_amd.models import ContinuousDiffusionOsuFusionDiT
from osufusion_amd.modules import GaussianDiffusionContinuousTimes
from tests import ct_objectives_oracle as CO
from tests import scheduler_oracle as SO

SMALL = {"mmdit": dict(dim_h=32, depth=2, attn_heads=2, attn_kv_heads=1, attn_dim_head=16), "dit": dict(dim_h=96, depth=2, attn_heads=6, attn_dim_head=16)}
TIMES = torch.tensor([1e-3, 0.25, 0.5, 0.75, 0.999], dtype=torch.float64)


def _pair(seed=0, shape=(5, 6, 37)):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape), rng.standard_normal(shape)


@pytest.mark.parametrize("schedule", SO.SCHEDULES)
def test_v_algebra_round_trip_in_fp64(schedule):
    """A self-check of the restatement (tests/ct_objectives_oracle.py), not of the package: predict_start_from_v(q_sample(x0), t,
    calculate_v(x0, t, noise)) == x0, because alpha^2 + sigma^2 = 1.  The scheduler's own methods run on the GPU only and are held to this
    restatement in tests/test_ct_objectives_gpu.py::test_scheduler_v_methods_against_fp64_and_round_trip."""
    x0, noise = _pair()
    alpha, sigma = SO.alpha_sigma(SO.log_snr(TIMES, schedule, torch.float64))
    x_t = CO.q_sample(x0, noise, alpha, sigma)
    v = CO.calculate_v(x0, noise, alpha, sigma)
    back = CO.predict_start_from_v(x_t, v, alpha, sigma)
    assert np.abs(back - x0).max() < 1e-13, np.abs(back - x0).max()
    assert np.abs(CO.f64(alpha) ** 2 + CO.f64(sigma) ** 2 - 1).max() < 1e-14


@pytest.mark.parametrize("schedule", SO.SCHEDULES)
def test_three_objectives_give_one_posterior_mean_in_fp64(schedule):
    """A self-check of the restatement, as above (the kernels are held to it in tests/test_ct_objectives_gpu.py).
    The exact noise, x_start and v of one (x0, noise) pair recover the same start prediction, and so the same posterior mean; through
    step() (no clamp active: x0 scaled into [-1, 1]) too."""
    x0, noise = _pair(1)
    x0 = np.tanh(x0) * 0.9
    t_next = (TIMES - 0.2).clamp(min=0.0)
    row = SO.stack_row(SO.schedule_row(TIMES, t_next, schedule, torch.float64)).numpy()
    alpha, sigma = row[:, 1], row[:, 2]
    x_t = CO.q_sample(x0, noise, alpha, sigma)
    preds = {k: CO.target_of(x0, noise, alpha, sigma, k) for k in CO.OBJECTIVES}
    starts = {k: CO.start_from(x_t, preds[k], row, k) for k in CO.OBJECTIVES}
    means = {k: CO.posterior_mean(x_t, starts[k], alpha, row[:, 4], row[:, 6]) for k in CO.OBJECTIVES}
    stepped = {k: CO.step(x_t, preds[k], None, 1.0, row, None, k)[0] for k in CO.OBJECTIVES}
    scale = 1.0 / alpha.min()                                                  # the noise form divides by alpha
    for k in CO.OBJECTIVES:
        assert np.abs(starts[k] - x0).max() < 1e-13 * scale, (k, np.abs(starts[k] - x0).max())
        assert np.abs(means[k] - means["x_start"]).max() < 1e-12 * scale, k
        assert np.abs(stepped[k] - means["x_start"]).max() < 1e-12 * scale, k


def test_loss_weights_below_at_and_above_gamma():
    gamma = 5.0
    snr = torch.tensor([0.25, 5.0, 80.0], dtype=torch.float64)                  # snr < gamma, = gamma, > gamma
    log_snr = snr.log()
    want = {"noise": [1.0, 1.0, 5.0 / 80.0], "x_start": [0.25, 5.0, 5.0], "v": [0.25 / 1.25, 5.0 / 6.0, 5.0 / 81.0]}
    for objective, w in want.items():
        got = GaussianDiffusionContinuousTimes.loss_weight(log_snr, objective, gamma)
        assert got.shape == snr.shape
        np.testing.assert_allclose(got.numpy(), np.array(w), rtol=1e-14)
        np.testing.assert_allclose(got.numpy(), CO.loss_weight(log_snr, objective, gamma), rtol=1e-14)
        assert GaussianDiffusionContinuousTimes.loss_weight(log_snr, objective, None) is None
        assert CO.loss_weight(log_snr, objective, None) is None
    sch = GaussianDiffusionContinuousTimes("cosine")
    assert torch.equal(sch.loss_weight(log_snr, "v", gamma), GaussianDiffusionContinuousTimes.loss_weight(log_snr, "v", gamma))
    with pytest.raises(ValueError, match="objective"):
        GaussianDiffusionContinuousTimes.loss_weight(log_snr, "eps", gamma)


@pytest.mark.parametrize("q", [0.5, 0.95, 0.999, 1.0])
def test_dynamic_threshold_against_numpy_quantile(q):
    rng = np.random.default_rng(3)
    x0 = torch.from_numpy(rng.standard_normal((4, 6, 40)) * np.array([0.2, 1.0, 3.0, 10.0])[:, None, None])
    got = GaussianDiffusionContinuousTimes.dynamic_threshold(x0, q).numpy()
    s = np.maximum(1.0, np.quantile(np.abs(x0.numpy()).reshape(4, -1), q, axis=1, method="linear"))
    want = np.clip(x0.numpy(), -s[:, None, None], s[:, None, None]) / s[:, None, None]
    np.testing.assert_allclose(got, want, rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(CO.threshold(x0, q)[2], s, rtol=1e-14)
    np.testing.assert_allclose(CO.dynamic_threshold(x0, q), want, rtol=1e-13, atol=1e-15)
    assert np.abs(got).max() <= 1.0
    if q < 1.0:
        assert (s[2:] > 1.0).all()                                              # the wide samples are rescaled, not just clamped


def test_dynamic_threshold_inside_the_range_is_the_static_clamp():
    """Every value inside [-1, 1]: s = 1 and the output is x0.clamp(-1, 1) = x0, bit for bit (fp32 too)."""
    g = torch.Generator().manual_seed(0)
    for dtype in (torch.float64, torch.float32):
        x0 = (torch.rand((3, 6, 17), generator=g, dtype=dtype) * 2 - 1)
        got = GaussianDiffusionContinuousTimes.dynamic_threshold(x0, 0.95)
        assert torch.equal(got, x0.clamp(-1.0, 1.0)) and torch.equal(got, x0)
        assert (CO.threshold(x0, 0.95)[2] == 1.0).all()
    # one sample outside: only the static clamp differs there
    x0 = torch.tensor([[0.5, -0.25, 4.0, -2.0]], dtype=torch.float64)
    assert torch.equal(GaussianDiffusionContinuousTimes.dynamic_threshold(x0, 1.0), x0 / 4.0)


@pytest.mark.parametrize("n", [1, 2, 240, 257])
@pytest.mark.parametrize("q", [0.5, 0.95, 0.999, 1.0])
def test_host_quantile_rank(n, q):
    k_lo, frac = ct.quantile_rank(q, n)
    assert isinstance(k_lo, int) and 0 <= k_lo <= n - 1 and 0.0 <= frac < 1.0
    assert k_lo == int(np.floor(q * (n - 1))) and frac == q * (n - 1) - k_lo
    assert (k_lo, frac) == CO.quantile_rank(q, n)
    if q == 1.0:
        assert (k_lo, frac) == (n - 1, 0.0)
    v = np.sort(np.random.default_rng(n).standard_normal(n))
    mine = v[k_lo] + (v[min(k_lo + 1, n - 1)] - v[k_lo]) * frac
    np.testing.assert_allclose(mine, np.quantile(v, q, method="linear"), rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(mine, torch.quantile(torch.from_numpy(v), q).item(), rtol=1e-13, atol=1e-15)


def test_host_quantile_rank_refuses_bad_arguments():
    for q in (-0.1, 1.5):
        with pytest.raises(ValueError):
            ct.quantile_rank(q, 10)
    with pytest.raises(ValueError):
        ct.quantile_rank(0.5, 0)
    assert ct.OBJECTIVES == {"noise": 0, "x_start": 1, "v": 2}
    with pytest.raises(ValueError, match="objective"):
        ct.objective_code("epsilon")


@pytest.mark.parametrize("backbone", ["mmdit", "dit"])
def test_constructor_keywords_and_validation(backbone):
    sig = inspect.signature(ContinuousDiffusionOsuFusionDiT.__init__)
    got = {k: sig.parameters[k].default for k in ("pred_objective", "dynamic_thresholding", "dynamic_thresholding_percentile", "min_snr_gamma")}
    assert got == {"pred_objective": "noise", "dynamic_thresholding": False, "dynamic_thresholding_percentile": 0.95, "min_snr_gamma": None}
    kw = SMALL[backbone]
    plain = ContinuousDiffusionOsuFusionDiT(backbone=backbone, **kw)
    assert (plain.pred_objective, plain.dynamic_thresholding, plain.dynamic_thresholding_percentile, plain.min_snr_gamma) == ("noise", False, 0.95, None)
    m = ContinuousDiffusionOsuFusionDiT(backbone=backbone, pred_objective="v", dynamic_thresholding=True, dynamic_thresholding_percentile=0.9,
                                        min_snr_gamma=5.0, **kw)
    assert (m.pred_objective, m.dynamic_thresholding, m.dynamic_thresholding_percentile, m.min_snr_gamma) == ("v", True, 0.9, 5.0)
    assert list(m.state_dict()) == list(plain.state_dict())                    # no new parameters or buffers
    ContinuousDiffusionOsuFusionDiT(backbone=backbone, pred_objective="x_start", dynamic_thresholding_percentile=1.0, **kw)
    with pytest.raises(ValueError, match="objective"):
        ContinuousDiffusionOsuFusionDiT(backbone=backbone, pred_objective="eps", **kw)
    for bad in (0.0, -0.5, 1.01):
        with pytest.raises(ValueError, match="percentile"):
            ContinuousDiffusionOsuFusionDiT(backbone=backbone, dynamic_thresholding_percentile=bad, **kw)


def test_new_methods_refuse_cpu_tensors():
    sch = GaussianDiffusionContinuousTimes("cosine")
    x = torch.zeros(2, 6, 8)
    for call in (lambda: sch.predict_start_from_v(x, torch.zeros(2), x), lambda: sch.calculate_v(x, torch.zeros(2), x)):
        with pytest.raises(RuntimeError, match="MI355X only"):
            call()


def test_capi_new_entry_points_are_declared_and_bound():
    decls, consts = _lib.read_header()
    want = {
        "osuf_ct_step_ex": ["x", "cond", "nullp", "cond_scale", "coef", "noise", "objective", "s", "s_ld", "out", "B", "per_sample", "stream"],
        "osuf_ct_x0_quantile": ["x", "cond", "nullp", "cond_scale", "coef", "objective", "k_lo", "frac", "out", "workspace", "B", "per_sample", "stream"],
        "osuf_ct_qsample": ["x0", "noise", "sched", "sched_ld", "objective", "x_noisy", "target", "B", "per_sample", "stream"],
        "osuf_mse_w": ["pred", "target", "orig_len", "w", "grad", "loss_sum", "B", "Dch", "L", "stream"],
    }
    for name, names in want.items():
        assert name in decls, f"{name} is not declared in include/osufusion_hip.h"
        assert decls[name][0] == "int" and [p.split()[-1].lstrip("*") for p in decls[name][1]] == names
        assert len(_lib.SIGNATURES[name]) == len(names)
        assert hasattr(_lib.load(), name)
    for j, obj in enumerate(("NOISE", "X_START", "V")):
        assert consts[f"OSUF_CT_OBJ_{obj}"] == j
    lib = _lib.load()
    assert lib.osuf_ct_x0_quantile_workspace_bytes(3) == 3 * (5 * 2048 + 8) * 4 and lib.osuf_ct_x0_quantile_workspace_bytes(0) == 0
    from osufusion_amd import ops
    assert all(callable(getattr(ops, n)) for n in ("ct_step_ex", "ct_x0_quantile", "ct_qsample"))
    assert "weight" in inspect.signature(ops.mse).parameters
