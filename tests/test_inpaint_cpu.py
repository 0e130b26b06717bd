"""Masked generation without a GPU: the host helpers of osufusion_amd/inpaint.py (frame_mask, as_mask), the argument validation of every
sample(), and the properties of the masked loops as tests/inpaint_oracle.py restates them in fp64."""
import numpy as np
import pytest
import torch

from osufusion_amd import inpaint
from osufusion_amd.models import ContinuousDiffusionOsuFusionDiT, DiffusionOsuFusionDiT, RectifiedFlowOsuFusionDiT
from osufusion_amd.models.diffusion import DDIMSchedule, OsuFusion
from osufusion_amd.models.rectified_flow import OsuFusion as FlowOsuFusion
from tests import inpaint_oracle as IO
from tests import scheduler_oracle as SO

MS = 176 / 22050 * 1000                      # one frame, about 7.98 ms


# ---- frame_mask --------------------------------------------------------------------------------------------------------------------------
def test_frame_times_are_hop_over_rate():
    t = inpaint.frame_times_ms(2000)
    assert t.dtype == torch.float64 and t[0].item() == 0.0
    want = [l * 176 / 22050 * 1000 for l in range(2000)]             # plain python arithmetic, no audio library
    assert t.tolist() == want
    assert abs(t[1250].item() - 9977.32426303855) < 1e-9              # 1250 * 176 samples = 9.977324... s


def test_hard_spans():
    t = inpaint.frame_times_ms(100)
    m = inpaint.frame_mask(100, [(t[10].item(), t[20].item())])
    assert m.dtype == torch.float32 and m.shape == (100,)
    want = torch.zeros(100)
    want[10:21] = 1.0                                                # both ends are frame times: the span is closed
    assert torch.equal(m, want)
    m = inpaint.frame_mask(100, [(10.5 * MS, 19.5 * MS)])
    want = torch.zeros(100)
    want[11:20] = 1.0
    assert torch.equal(m, want)
    assert torch.equal(inpaint.frame_mask(50, []), torch.zeros(50))
    assert torch.equal(inpaint.frame_mask(50, [(-5.0, 1e9)]), torch.ones(50))
    head_and_tail = inpaint.frame_mask(64, [(0.0, 7.5 * MS), (56.5 * MS, 1e9)])
    assert head_and_tail.tolist() == [1.0] * 8 + [0.0] * 49 + [1.0] * 7


def test_overlapping_spans_take_the_maximum():
    a, b = (10.5 * MS, 30.5 * MS), (25.5 * MS, 40.5 * MS)
    both = inpaint.frame_mask(64, [a, b])
    want = torch.zeros(64)
    want[11:41] = 1.0
    assert torch.equal(both, want)
    fa, fb = inpaint.frame_mask(64, [a], 40.0), inpaint.frame_mask(64, [b], 40.0)
    assert torch.equal(inpaint.frame_mask(64, [a, b], 40.0), torch.maximum(fa, fb))
    assert torch.equal(inpaint.frame_mask(64, [b, a], 40.0), torch.maximum(fa, fb))


def test_feathered_edge():
    feather = 10 * MS
    m = inpaint.frame_mask(100, [(40 * MS, 60 * MS)], feather)
    assert (m[40:61] == 1.0).all()                                   # exactly one inside
    assert (m[:30] == 0.0).all() and (m[71:] == 0.0).all()           # exactly zero beyond feather_ms (frames 30 and 70 sit at d = feather_ms)
    assert m[30].item() < 1e-6 and m[70].item() < 1e-6
    up, down = m[30:41], m[60:71]
    assert (up[1:] > up[:-1]).all() and (down[1:] < down[:-1]).all()  # strictly monotone across the edge
    assert ((m >= 0) & (m <= 1)).all()
    t = inpaint.frame_times_ms(100)
    want = torch.clamp(1.0 - torch.clamp(torch.maximum(40 * MS - t, t - 60 * MS), min=0.0) / feather, 0.0, 1.0).float()
    assert torch.equal(m, want)
    assert abs(m[35].item() - 0.5) < 1e-6


def test_frame_mask_rejects_bad_arguments():
    with pytest.raises(ValueError):
        inpaint.frame_mask(0, [])
    with pytest.raises(ValueError):
        inpaint.frame_mask(10, [(5.0, 1.0)])
    with pytest.raises(ValueError):
        inpaint.frame_mask(10, [(1.0, 5.0)], feather_ms=-1.0)


# ---- as_mask -----------------------------------------------------------------------------------------------------------------------------
def test_as_mask_shapes_and_dtypes():
    B, n = 3, 10
    shared = torch.arange(n) % 2 == 0
    got = inpaint.as_mask(shared, B, n, "cpu")
    assert got.dtype == torch.float32 and got.shape == (n,) and got.is_contiguous() and torch.equal(got, shared.float())
    rows = torch.rand(B, n, dtype=torch.float64)
    got = inpaint.as_mask(rows, B, n, "cpu")
    assert got.dtype == torch.float32 and got.shape == (B, n) and torch.equal(got, rows.float())
    got = inpaint.as_mask(rows.half().reshape(B, 1, n), B, n, "cpu")
    assert got.dtype == torch.float32 and got.shape == (B, n) and got.is_contiguous()
    strided = torch.rand(B, 2 * n)[:, ::2]
    got = inpaint.as_mask(strided, B, n, "cpu")
    assert got.is_contiguous() and torch.equal(got, strided)
    f32 = torch.rand(B, n)
    assert inpaint.as_mask(f32, B, n, "cpu").data_ptr() == f32.data_ptr()          # already as wanted: no copy


@pytest.mark.parametrize("bad", [torch.ones(9), torch.ones(2, 10), torch.ones(3, 2, 10), torch.ones(3, 10, 1), torch.ones(()),
                                 torch.ones(3, 10, dtype=torch.int64), [1.0] * 10])
def test_as_mask_errors(bad):
    with pytest.raises(ValueError):
        inpaint.as_mask(bad, 3, 10, "cpu")


# ---- argument validation, raised before any GPU requirement --------------------------------------------------------------------------------
UNET_KW = dict(dim_h_mult=(1, 2), num_layer_blocks=(1, 1), num_middle_transformers=1, cross_embed_kernel_sizes=(3,), attn_dim_head=64, attn_heads=2,
               attn_kv_heads=1, attn_context_len=256)
DIT_KW = dict(dim_h=32, depth=2, attn_heads=2, attn_kv_heads=1, attn_dim_head=16)
MODELS = {"unet_ddim": lambda: OsuFusion(32, **UNET_KW), "unet_flow": lambda: FlowOsuFusion(32, **UNET_KW),
          "dit_ddim": lambda: DiffusionOsuFusionDiT(**DIT_KW), "dit_flow": lambda: RectifiedFlowOsuFusionDiT(**DIT_KW),
          "ct_ddpm": lambda: ContinuousDiffusionOsuFusionDiT(**DIT_KW), "ct_ddim": lambda: ContinuousDiffusionOsuFusionDiT(sampler="ddim", **DIT_KW),
          "ct_2m": lambda: ContinuousDiffusionOsuFusionDiT(sampler="dpmpp_2m", **DIT_KW)}


def _entry(model):
    """The call that takes known / known_mask: sample() on the transformer models; sample_masked() on the two UNet models, whose sample()
    keeps the reference's signature (tests/test_host_logic.py)."""
    return getattr(model, "sample_masked", model.sample)


@pytest.mark.parametrize("name", list(MODELS))
def test_known_and_mask_go_together(name):
    model = MODELS[name]()
    a, c = torch.zeros(2, 96, 64), torch.zeros(2, 5)
    known, mask = torch.zeros(2, 6, 64), torch.ones(64)
    with pytest.raises(ValueError, match="known"):
        _entry(model)(a, c, known=known)
    with pytest.raises(ValueError, match="known"):
        _entry(model)(a, c, known_mask=mask)
    with pytest.raises(RuntimeError, match="MI355X"):                 # both given: past the check, at the GPU-only guard
        _entry(model)(a, c, known=known, known_mask=mask)


def test_resample_validation():
    a, c = torch.zeros(2, 96, 64), torch.zeros(2, 5)
    known, mask = torch.zeros(2, 6, 64), torch.ones(64)
    for name in ("ct_ddim", "ct_2m"):
        with pytest.raises(ValueError, match="resample"):
            MODELS[name]().sample(a, c, known=known, known_mask=mask, resample=3)
    ddpm = MODELS["ct_ddpm"]()
    with pytest.raises(ValueError, match="resample"):
        ddpm.sample(a, c, resample=3)                                  # no known region
    with pytest.raises(ValueError, match="resample"):
        ddpm.sample(a, c, known=known, known_mask=mask, resample=0)
    with pytest.raises(RuntimeError, match="MI355X"):
        ddpm.sample(a, c, known=known, known_mask=mask, resample=3)


# ---- properties of the loops, in the fp64 restatement ---------------------------------------------------------------------------------------
B, D, N = 2, 6, 24
RNG = np.random.default_rng(20240)
X_STAR = RNG.uniform(-0.9, 0.9, (B, D, N))
START = RNG.standard_normal((B, D, N))
HARD = (np.arange(N) % 5 < 2).astype(np.float64)
SOFT = np.stack([HARD, np.clip(np.linspace(-0.5, 1.5, N), 0.0, 1.0)])
# A rising log-SNR grid that ends at 80: sigma there is e^-40 = 4e-18, below the round-off of any comparison, so the final level is the
# data itself (the product's grids end at the schedule's log_snr(0), sigma about 1e-4: there the property holds to that sigma only).
GRID = np.array([-12.0, -6.0, -2.5, 0.0, 2.0, 5.0, 9.0, 80.0])
TOL = 5e-12                                                           # fp64 round-off through 7 steps with factors up to about 20


def _ddim_coefs(steps):
    sch = DDIMSchedule()
    sch.set_timesteps(steps)
    return np.array([sch.step_coefficients(t) for t in sch.timesteps.tolist()], dtype=np.float64)


def _draws(seed=5):
    rng = np.random.default_rng(seed)
    return lambda: rng.standard_normal((B, D, N))


def _perfect_eps(coefs):
    return lambda x, i: (x - coefs[i][1] * X_STAR) / coefs[i][0]


def _perfect_flow(t, y):
    return (X_STAR - y) / (1.0 - t)


@pytest.mark.parametrize("mask", [HARD, SOFT], ids=["hard", "soft_per_sample"])
def test_perfect_denoiser_returns_the_point_mass(mask):
    """The data distribution is the point mass at x*, the denoiser is exact for it, known = x* on the mask: nothing the blend puts in
    contradicts the denoiser, and every loop ends on x* over the whole signal."""
    coefs = _ddim_coefs(7)
    got = IO.ddim_loop(_perfect_eps(coefs), START, coefs, X_STAR, mask)
    assert np.abs(got - X_STAR).max() < TOL
    got = IO.flow_loop(_perfect_flow, START, np.linspace(0.0, 1.0, 8).tolist(), X_STAR, mask)
    assert np.abs(got - X_STAR).max() < TOL
    for sampler, eta, resample in (("ddpm", 0.0, 1), ("ddpm", 0.0, 3), ("ddim", 0.0, 1), ("ddim", 0.7, 1), ("dpmpp_2m", 0.0, 1)):
        got = IO.ct_loop(lambda x, i: X_STAR, START, GRID, sampler, eta, X_STAR, mask, _draws(), resample=resample)
        assert np.abs(got - X_STAR).max() < TOL, (sampler, eta, resample)


def test_known_region_sits_at_every_level_in_the_deterministic_loops():
    """Every iterate handed to the denoiser holds a known + s eps where the mask is 1, eps the start iterate: exactly (it is a select)."""
    known = RNG.uniform(-1, 1, (B, D, N))
    on = np.broadcast_to(HARD[None, None, :] == 1, START.shape)
    den = lambda x, i: np.tanh(x + i)                                 # any denoiser
    coefs = _ddim_coefs(5)
    traces = {"ddim": [], "flow": [], "ct_ddim": [], "ct_2m": []}
    IO.ddim_loop(den, START, coefs, known, HARD, trace=traces["ddim"])
    IO.flow_loop(lambda t, y: np.tanh(y - t), START, np.linspace(0.0, 1.0, 5).tolist(), known, HARD, trace=traces["flow"])
    IO.ct_loop(den, START, GRID, "ddim", 0.0, known, HARD, trace=traces["ct_ddim"])
    IO.ct_loop(den, START, GRID, "dpmpp_2m", 0.0, known, HARD, trace=traces["ct_2m"])
    assert [len(v) for v in traces.values()] == [5, 1 + 2 * 4 - 1, 7, 7]      # one per denoiser call
    for name, trace in traces.items():
        for a, s, x in trace:
            assert np.array_equal(x[on], (a * known + s * START)[on]), name
    assert traces["ddim"][0][:2] == (coefs[0][1], coefs[0][0]) and traces["ddim"][-1][:2] == (coefs[3][2], coefs[3][3])
    assert [t[:2] for t in traces["flow"][:3]] == [(0.0, 1.0), (0.125, 0.875), (0.25, 0.75)]
    rows = IO.SV.rows(GRID)
    assert traces["ct_2m"][0][:2] == (rows[0][1], rows[0][2]) and traces["ct_2m"][-1][:2] == (rows[5][4], rows[5][5])


def test_all_zero_mask_is_the_unmasked_loop():
    known = np.full((B, D, N), np.nan)                                # never read into the result
    zero = np.zeros(N)
    den = lambda x, i: np.tanh(x + i)
    coefs = _ddim_coefs(5)
    assert np.array_equal(IO.ddim_loop(den, START, coefs, known, zero), IO.ddim_loop(den, START, coefs))
    vel, times = (lambda t, y: np.tanh(y - t)), np.linspace(0.0, 1.0, 5).tolist()
    assert np.array_equal(IO.flow_loop(vel, START, times, known, zero), IO.flow_loop(vel, START, times))
    for sampler, eta in (("ddim", 0.0), ("dpmpp_2m", 0.0)):
        assert np.array_equal(IO.ct_loop(den, START, GRID, sampler, eta, known, zero), IO.ct_loop(den, START, GRID, sampler, eta))
    # the stochastic loops: the blends still draw, so the unmasked loop sees every other draw of the masked one's sequence
    for sampler, eta in (("ddpm", 0.0), ("ddim", 0.5)):
        seq = [np.random.default_rng(100 + k).standard_normal((B, D, N)) for k in range(2 * len(GRID))]
        it = iter(seq)
        masked = IO.ct_loop(den, START, GRID, sampler, eta, known, zero, lambda: next(it))
        # masked order: start blend, then (step, blend) per step; "ddpm" draws no step noise on the last step and the exact blend none at all
        it2 = iter([seq[1 + 2 * i] for i in range(len(GRID) - 1)])
        assert np.array_equal(masked, IO.ct_loop(den, START, GRID, sampler, eta, draw=lambda: next(it2))), sampler


def test_resample_counts_and_stop_after():
    calls = []
    IO.ct_loop(lambda x, i: X_STAR, START, GRID, "ddpm", 0.0, X_STAR, HARD, _draws(), resample=3, calls=calls)
    S = len(GRID) - 1
    assert len(calls) == 3 * (S - 1) + 1 and calls == [i for i in range(S - 1) for _ in range(3)] + [S - 1]
    trace = []
    early = IO.ct_loop(lambda x, i: np.tanh(x), START, GRID, "dpmpp_2m", 0.0, X_STAR, HARD, stop_after=2, trace=trace)
    assert len(trace) == 3 and np.array_equal(early, trace[-1][2])   # a run cut short ends on its level blend


# ---- the way back of RePaint's resampling ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("steps", [7, 300])
@pytest.mark.parametrize("schedule", SO.SCHEDULES)
def test_renoise_is_the_forward_transition(schedule, steps):
    """k_r^2 sigma_next^2 + k_g^2 = sigma_t^2 on the sampler's time grid, in fp64.  Both sides are sums of positive terms; what separates them
    is the rounding of d = log_snr - log_snr_next (|log_snr| <= 37: 2 * 37 * 2^-53 = 8e-15 relative in exp(d)) and a few ulps: 5e-14."""
    times = torch.linspace(1.0, 0.0, steps + 1, dtype=torch.float64)
    row = SO.stack_row(SO.schedule_row(times[:-1], times[1:], schedule, torch.float64)).numpy()
    k_r, k_g = IO.renoise_factors(row)
    lhs, rhs = k_r ** 2 * row[:, 5] ** 2 + k_g ** 2, row[:, 2] ** 2
    assert np.isfinite(lhs).all() and (k_g >= 0).all() and (k_r > 0).all() and (k_r <= 1 + 1e-15).all()
    assert np.abs(lhs / rhs - 1).max() < 5e-14
