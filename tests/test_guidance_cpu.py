"""Guidance interval and CFG rescale, the host side: the keywords' errors, the per-call log-SNR lists and guided / unguided decisions of the
five sampling loops against hand-written expectations (the package's osufusion_amd/guidance.py and the restatement tests/guidance_oracle.py
side by side), and the C surface of osuf_cfg_rescale: declared, bound, exported, and refusing bad arguments before any launch."""
import math
from ctypes import c_float, c_int, c_long, c_void_p

import numpy as np
import pytest
import torch

from osufusion_amd import _lib, guidance
from osufusion_amd.models import ContinuousDiffusionOsuFusionDiT, DiffusionOsuFusionDiT, RectifiedFlowOsuFusionDiT
from osufusion_amd.models.diffusion import DDIMSchedule
from tests import guidance_oracle as GO

INF = math.inf


# ---- the keywords ------------------------------------------------------------------------------------------------------------------------
BAD = [dict(guidance_rescale=-0.1), dict(guidance_rescale=1.5), dict(guidance_rescale=math.nan), dict(guidance_interval=3.0),
       dict(guidance_interval=(1.0,)), dict(guidance_interval=(0.0, 1.0, 2.0)), dict(guidance_interval="ab"), dict(guidance_interval=(2.0, 1.0)),
       dict(guidance_interval=(math.nan, 1.0)), dict(guidance_interval=(None, math.nan))]


@pytest.mark.parametrize("kw", BAD, ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_plan_refuses(kw):
    with pytest.raises(ValueError):
        guidance.plan(**kw)


def test_plan_accepts():
    G = guidance.Guidance
    assert guidance.plan() is None and guidance.plan(0.0, None) is None
    assert guidance.plan(0.0, (None, None)) is None                      # unbounded at both ends: nothing to decide
    assert guidance.plan(0.7) == G(0.7) and guidance.plan(1.0, (None, None)) == G(1.0)
    assert guidance.plan(0.0, (-2.0, 3.0)) == G(0.0, -2.0, 3.0, True)
    assert guidance.plan(0.5, [None, 3]) == G(0.5, -INF, 3.0, True) and guidance.plan(0.0, (1.5, None)) == G(0.0, 1.5, INF, True)
    assert guidance.plan(0.0, (2.0, 2.0)) == G(0.0, 2.0, 2.0, True)      # lo == hi is a (one-point) interval
    assert guidance.plan(0.0, (-INF, 0.0)).contains(-INF)               # the flow loop's t = 0 lies in an interval unbounded below


@pytest.mark.parametrize("cls", [DiffusionOsuFusionDiT, ContinuousDiffusionOsuFusionDiT, RectifiedFlowOsuFusionDiT])
def test_sample_raises_before_it_touches_a_device(cls):
    """The three sample() methods check the keywords first: a CPU call gets the ValueError, not the no-GPU error."""
    model = cls(dim_h=96, backbone="dit", depth=1, attn_heads=6, attn_dim_head=16, sampling_timesteps=2)
    a, c = torch.zeros(1, 96, 16), torch.zeros(1, 5)
    for kw in (BAD[0], BAD[1], BAD[3], BAD[4], BAD[7], BAD[8]):
        with pytest.raises(ValueError, match="guidance_"):
            model.sample(a, c, **kw)


# ---- which calls are guided ---------------------------------------------------------------------------------------------------------------
def _both(log_snr, interval, cond_scale):
    """The package's decision and the restatement's, which must agree."""
    got = guidance.guided_calls(log_snr, guidance.plan(0.0, interval), cond_scale)
    assert got == GO.decide(log_snr, interval, cond_scale)
    return got


def test_discrete_ddim_decisions():
    """T = 1000, S = 4: timesteps 750, 500, 250, 0, log-SNR rising from about -5.7 to about 9.2."""
    sch = DDIMSchedule(num_train_timesteps=1000)
    sch.set_timesteps(4)
    assert sch.timesteps.tolist() == GO.ddim_timesteps(1000, 4) == [750, 500, 250, 0]
    ls = guidance.ddim_log_snr(sch.alphas_cumprod, sch.timesteps.tolist())
    assert ls == GO.ddim_log_snr(sch.alphas_cumprod.tolist(), 1000, 4)
    acp = sch.alphas_cumprod.double()
    assert ls == pytest.approx([math.log(acp[t] / (1 - acp[t])) for t in (750, 500, 250, 0)], rel=1e-15)
    assert ls == pytest.approx([-5.71, -2.47, 0.086, 9.21], abs=0.01) and ls == sorted(ls)
    assert _both(ls, None, 2.0) == [True, True, True, True]
    assert _both(ls, (-3.0, 1.0), 2.0) == [False, True, True, False]
    assert _both(ls, (ls[1], ls[2]), 2.0) == [False, True, True, False]            # both ends exactly on a call: inclusive
    assert _both(ls, (math.nextafter(ls[1], INF), math.nextafter(ls[2], -INF)), 2.0) == [False, False, False, False]
    assert _both(ls, (None, 0.0), 2.0) == [True, True, False, False]
    assert _both(ls, (0.0, None), 2.0) == [False, False, True, True]
    assert _both(ls, (-100.0, 100.0), 2.0) == [True] * 4
    assert _both(ls, (-3.0, 1.0), 1.0) == [False] * 4                               # cond_scale == 1: nothing is guided
    assert GO.rows_per_call(_both(ls, (-3.0, 1.0), 2.0), 2) == [2, 4, 4, 2]


def test_continuous_time_decisions():
    """The denoiser's fp32 log-SNR inputs as host floats, the same rule under "ddpm", "ddim" and "dpmpp_2m": a grid of fp32 values that are
    not fp64-round numbers, the interval's ends exactly on two of them."""
    grid = np.linspace(-15.0, 9.2, 5, dtype=np.float32)[:-1]                        # -15, -8.95, -2.9, 3.15 (fp32)
    ls = GO.ct_log_snr(grid)
    assert ls == [float(v) for v in grid] and ls == pytest.approx([-15.0, -8.95, -2.9, 3.15], abs=1e-5)
    assert _both(ls, (ls[1], ls[2]), 7.0) == [False, True, True, False]
    assert _both(ls, (math.nextafter(ls[1], INF), ls[2]), 7.0) == [False, False, True, False]   # one fp64 ulp inside the call: no tolerance
    assert _both(ls, (None, ls[0]), 7.0) == [True, False, False, False]
    assert _both(ls, (ls[3], ls[3]), 7.0) == [False, False, False, True]
    assert _both(ls, None, 1.0) == [False] * 4


def test_flow_decisions():
    """S = 4 grid points: three midpoint steps, six evaluations at t = 0, 1/6, 1/3, 1/2, 2/3, 5/6; each decides for itself."""
    times = torch.linspace(0.0, 1.0, 4).tolist()
    ev = guidance.midpoint_eval_times(times)
    assert ev == GO.flow_eval_times(times) and ev == pytest.approx([0, 1 / 6, 1 / 3, 1 / 2, 2 / 3, 5 / 6], abs=1e-7)
    ls = [guidance.flow_log_snr(t) for t in ev]
    assert ls == GO.flow_log_snr(times)
    assert ls[0] == -INF and ls[1:] == pytest.approx([2 * math.log(0.2), 2 * math.log(0.5), 0.0, 2 * math.log(2.0), 2 * math.log(5.0)], abs=1e-6)
    assert guidance.flow_log_snr(1.0) == INF
    assert _both(ls, None, 2.0) == [True] * 6
    assert _both(ls, (-2.0, 2.0), 2.0) == [False, False, True, True, True, False]
    assert _both(ls, (None, 0.5), 2.0) == [True, True, True, True, False, False]   # t = 0, log-SNR -inf, lies in an interval unbounded below
    assert _both(ls, (-INF, -INF), 2.0) == [True, False, False, False, False, False]
    assert _both(ls, (-1e30, 0.5), 2.0) == [False, True, True, True, False, False]  # ... and in no interval with a finite lower end
    assert _both(ls, (ls[2], ls[4]), 2.0) == [False, False, True, True, True, False]   # ends exactly on the first evaluation of steps 2 and 3
    assert _both(ls, (ls[3], ls[3]), 2.0) == [False, False, False, True, False, False]  # one midpoint evaluation alone
    assert _both(ls, (-2.0, 2.0), 1.0) == [False] * 6


# ---- the restatement itself ------------------------------------------------------------------------------------------------------------------
def test_oracle_rescale_by_hand():
    """Two samples of four values with exact arithmetic: cond = (0, 2, 0, 2), null = 0 and cond_scale 3 -> g = 3 cond, std ratio 1 / 3."""
    cond = np.array([[0, 2, 0, 2], [1, 1, 1, 1]], np.float32)
    null = np.zeros_like(cond)
    out, f, g = GO.rescale(cond, null, 3.0, 1.0)
    assert np.array_equal(g, 3 * cond) and f.tolist() == [np.float32(1 / 3), 1.0]   # sample 1 has no spread: the select
    assert np.array_equal(out[0], np.float32(1 / 3) * g[0]) and np.array_equal(out[1], g[1])
    assert GO.rescale(cond, null, 3.0, 0.0)[1].tolist() == [1.0, 1.0]
    assert GO.rescale(cond, null, 3.0, 0.5)[1][0] == np.float32(0.5 / 3 + 0.5)
    assert GO.rescale(cond[:, :1], null[:, :1], 3.0, 1.0)[1].tolist() == [1.0, 1.0]  # per_sample < 2
    cond[1, 2] = np.nan
    f = GO.rescale(cond, null, 3.0, 1.0)[1]
    assert f[0] == np.float32(1 / 3) and np.isnan(f[1])


# ---- the C surface -----------------------------------------------------------------------------------------------------------------------------
def test_capi_cfg_rescale_is_declared_bound_and_exported():
    decls = _lib.read_header()[0]
    P, L, I, F = c_void_p, c_long, c_int, c_float
    assert "osuf_cfg_rescale" in decls, "osuf_cfg_rescale is not declared in include/osufusion_hip.h"
    ret, params = decls["osuf_cfg_rescale"]
    assert ret == "int"
    assert [p.split()[-1].lstrip("*") for p in params] == ["cond", "nullp", "cond_scale", "phi", "ws", "factor", "out", "B", "per_sample", "stream"]
    assert _lib.SIGNATURES["osuf_cfg_rescale"] == [P, P, F, F, P, P, P, I, L, P]
    ws = decls.get("osuf_cfg_rescale_workspace_bytes")
    assert ws and ws[0] == "long" and [p.split()[-1] for p in ws[1]] == ["B", "per_sample"]
    assert _lib.SIGNATURES["osuf_cfg_rescale_workspace_bytes"] == [I, L]
    lib = _lib.load()
    assert hasattr(lib, "osuf_cfg_rescale") and lib.osuf_cfg_rescale_workspace_bytes.restype is c_long


def test_capi_cfg_rescale_workspace_bytes():
    """Four fp64 sums per 4096-element chunk per sample; the chunking depends on per_sample alone."""
    ws = _lib.load().osuf_cfg_rescale_workspace_bytes
    assert ws(1, 1) == 32 and ws(1, 4096) == 32 and ws(1, 4097) == 64 and ws(3, 6 * 16388) == 3 * 25 * 32
    assert ws(16, 6 * 8192) == 16 * 12 * 32 and ws(0, 10) == 0 and ws(2, 0) == 0 and ws(-1, 10) == 0
    assert ws(2, 3 << 31) == 2 * ((3 << 31) // 4096) * 32                          # beyond an int


def test_capi_cfg_rescale_validates_its_arguments_on_the_host():
    """Every call returns -1 before a launch: the "pointers" are never dereferenced."""
    lib = _lib.load()
    buf = 4096

    def call(**kw):
        a = dict(cond=buf, nullp=buf, cs=2.0, phi=0.5, ws=buf, factor=buf, out=buf, B=2, n=54)
        a.update(kw)
        return lib.osuf_cfg_rescale(a["cond"], a["nullp"], a["cs"], a["phi"], a["ws"], a["factor"], a["out"], a["B"], a["n"], None)
    for kw in (dict(cond=None), dict(nullp=None), dict(ws=None), dict(factor=None), dict(out=None), dict(B=0), dict(B=-3), dict(n=0), dict(n=-1),
               dict(phi=-0.25), dict(phi=1.0001), dict(phi=math.nan), dict(phi=math.inf), dict(phi=-math.inf), dict(ws=buf + 4)):
        assert call(**kw) == -1, kw
