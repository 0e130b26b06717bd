"""Guidance interval and CFG rescale on the GPU: osuf_cfg_rescale against its restatement (tests/guidance_oracle.py) on poisoned and
canary-guarded memory (tests/memguard.py), and the five transformer sampling loops with guidance_rescale / guidance_interval against the same
loops written out over the public ops and a denoiser called guided (2B rows) or unguided (B rows), bit for bit.

The tolerance on the factor, 4 fp32 ulps, is derived: the kernel and the restatement differ only in the order of fp64 additions.  With
N <= 1e5 values, mean / spread <= 100, the sums carry a relative error below N 2^-53 = 1e-11 and the variance, which cancels by
(mean / spread)^2 = 1e4, below 1e-7 -- under one fp32 ulp of the square root; the final rounding to fp32 adds at most one more.
out = factor * g is one fp32 multiply of values both sides hold exactly: bit for bit."""
import contextlib

import numpy as np
import pytest
import torch

from osufusion_amd import _lib, inpaint, ops, windowed
from osufusion_amd.models import ContinuousDiffusionOsuFusionDiT, DiffusionOsuFusionDiT, RectifiedFlowOsuFusionDiT
from osufusion_amd.pattern import param_pattern, synth_inputs
from tests import guidance_oracle as GO
from tests.memguard import guard

pytestmark = pytest.mark.gpu
DEV = "cuda"
EINVAL = -1
ULPS = 4


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(got: torch.Tensor, want: np.ndarray) -> bool:
    return np.array_equal(got.detach().cpu().numpy().view(np.uint32), np.ascontiguousarray(want, dtype=np.float32).view(np.uint32))


# ---- the kernel pair --------------------------------------------------------------------------------------------------------------------------
# (B, 6, n): n = 9, 54 values: the scalar path, less than one workgroup; 5000: the four-wide path, eight chunks, the last one ragged; 4099: the
# scalar path (6 * 4099 is no multiple of 4) over seven chunks; 16388: 25 chunks, the last one of 24 values.
NS = [9, 5000, 4099, 16388]
BK, CSK, PHI = 3, 7.0, 0.7
_DATA = {}


def _data(n):
    """cond, null and the restatement's (out, factor, g) at (CSK, PHI), computed once per shape and left unchanged."""
    if n not in _DATA:
        rng = np.random.default_rng(n)
        cond = (0.2 + 1.3 * rng.standard_normal((BK, 6, n))).astype(np.float32)
        null = rng.standard_normal((BK, 6, n)).astype(np.float32)
        _DATA[n] = (cond, null) + GO.rescale(cond, null, CSK, PHI)
    return _DATA[n]


def _put(g, v, offset=False):
    """A test operand at the front of a guarded allocation, or (offset) one float into it: off 16-byte alignment."""
    t = torch.from_numpy(np.ascontiguousarray(v))
    if not offset:
        return g.place(t.to(DEV))
    buf = g.place(torch.cat([torch.zeros(1), t.reshape(-1)]).to(DEV))
    return buf[1:].view(t.shape)


def _rescale(g, cond, null, cond_scale, phi, offset=False):
    """ops.cfg_rescale on guarded operands; offset: every operand, the outputs too, one float into its buffer, through the C entry point."""
    c, u = _put(g, cond, offset), _put(g, null, offset)
    if not offset:
        out, factor = ops.cfg_rescale(c, u, cond_scale, phi)
    else:
        B, per = c.shape[0], c[0].numel()
        obuf, fbuf = torch.empty(c.numel() + 1, dtype=torch.float32, device=DEV), torch.empty(B + 1, dtype=torch.float32, device=DEV)
        ws = torch.empty(_lib.load().osuf_cfg_rescale_workspace_bytes(B, per) // 8, dtype=torch.float64, device=DEV)
        out, factor = obuf[1:].view(c.shape), fbuf[1:]
        ops.call("osuf_cfg_rescale", c.data_ptr(), u.data_ptr(), cond_scale, phi, ws.data_ptr(), factor.data_ptr(), out.data_ptr(), B, per, ops._stream())
        g.check()
        assert torch.isnan(obuf[0]).item() and torch.isnan(fbuf[0]).item()          # the floats in front keep their poison
    g.check()
    assert out.shape == c.shape and tuple(factor.shape) == (c.shape[0],)
    return out, factor.cpu().numpy()


def _check(out, factor, want_factor, g32):
    ulps = GO.ulps32(factor, want_factor)
    print("factor", factor.tolist(), "oracle", want_factor.tolist(), "ulps", ulps.tolist())
    assert _same_bits(out, GO.apply32(factor, g32))                                # with the factor as the kernel returned it
    assert (ulps <= ULPS).all()


@pytest.mark.parametrize("offset", [False, True], ids=["aligned", "offset"])
@pytest.mark.parametrize("n", NS)
def test_rescale_against_the_restatement(n, offset):
    cond, null, _, want_factor, g32 = _data(n)
    assert np.isfinite(want_factor).all() and (want_factor < 0.9).all()            # guidance 7 widens the spread: there is something to rescale
    with guard(0xFF) as g:
        out, factor = _rescale(g, cond, null, CSK, PHI, offset)
    _check(out, factor, want_factor, g32)


def test_a_mean_of_a_hundred_spreads():
    """cond = 100 + N(0, 1): sum x^2 - (sum x)^2 / n keeps 1e-4 of its terms.  The kernel's fp64 sums hold the bound; the same formula on
    fp32 sums, shown here for the record, does not."""
    rng = np.random.default_rng(100)
    cond = (100.0 + rng.standard_normal((BK, 6, 5000))).astype(np.float32)
    null = (100.0 + 0.5 * rng.standard_normal((BK, 6, 5000))).astype(np.float32)
    _, want_factor, g32 = GO.rescale(cond, null, 2.0, 1.0)
    with guard(0xFF) as g:
        for offset in (False, True):
            out, factor = _rescale(g, cond, null, 2.0, 1.0, offset)
            _check(out, factor, want_factor, g32)

    def var32(v):
        v = v.reshape(BK, -1)
        return (v * v).sum(1, dtype=np.float32) - v.sum(1, dtype=np.float32) ** 2 / np.float32(v.shape[1])
    with np.errstate(all="ignore"):
        naive = np.sqrt(var32(cond) / var32(g32)).astype(np.float32)
    assert not (GO.ulps32(np.abs(naive), want_factor) <= ULPS).all()


def test_phi_zero_is_the_guided_prediction():
    cond, null, _, _, g32 = _data(5000)
    with guard(0xFF) as g:
        for offset in (False, True):
            out, factor = _rescale(g, cond, null, CSK, 0.0, offset)
            assert (factor == 1.0).all() and _same_bits(out, g32)


def test_scale_one_and_phi_one_is_factor_one():
    """Operands on a grid of 2^-8 in [-4, 4]: null + (cond - null) * 1 is exact, g == cond, and the two variances are the same sums."""
    rng = np.random.default_rng(8)
    cond, null = (rng.integers(-1024, 1025, (2, BK, 6, 4099)) / 256.0).astype(np.float32)
    with guard(0xFF) as g:
        out, factor = _rescale(g, cond, null, 1.0, 1.0)
    assert (factor == 1.0).all() and _same_bits(out, cond)


def test_all_zero_predictions():
    """An untrained adaLN-Zero model predicts exact zeros: no spread, the factor is 1 by a select, not 0 / 0."""
    zero = np.zeros((BK, 6, 5000), np.float32)
    with guard(0xFF) as g:
        for offset in (False, True):
            out, factor = _rescale(g, zero, zero, CSK, PHI, offset)
            assert (factor == 1.0).all() and _same_bits(out, zero)
        out, factor = _rescale(g, zero[:, :1, :1], zero[:, :1, :1] + 1, CSK, 1.0)   # per_sample < 2
        assert (factor == 1.0).all() and _same_bits(out, GO.guide32(zero[:, :1, :1], zero[:, :1, :1] + 1, CSK))


@pytest.mark.parametrize("bad", [np.nan, np.inf], ids=["nan", "inf"])
@pytest.mark.parametrize("n", [9, 16388])
def test_a_non_finite_value_stays_in_its_sample(n, bad):
    cond, null, _, _, _ = _data(n)
    cond = cond.copy()
    cond[1, 3, n - 2] = bad
    with guard(0xFF) as g:
        out, factor = _rescale(g, cond, null, CSK, PHI)
    out = out.cpu().numpy()
    assert np.isnan(factor[1]) and np.isnan(out[1]).all()
    clean_out, clean_factor = _rescale_clean(n)
    for b in (0, 2):
        assert factor[b] == clean_factor[b] and np.array_equal(out[b].view(np.uint32), clean_out[b].view(np.uint32))


def _rescale_clean(n):
    cond, null, _, _, _ = _data(n)
    with guard(0xFF) as g:
        out, factor = _rescale(g, cond, null, CSK, PHI)
    return out.cpu().numpy(), factor


@pytest.mark.parametrize("n", [9, 16388])
def test_a_sample_does_not_depend_on_its_batch(n):
    cond, null, _, _, _ = _data(n)
    out3, factor3 = _rescale_clean(n)
    with guard(0xFF) as g:
        for b in range(BK):
            out1, factor1 = _rescale(g, cond[b:b + 1], null[b:b + 1], CSK, PHI)
            assert factor1[0] == factor3[b] and np.array_equal(out1.cpu().numpy().view(np.uint32)[0], out3[b].view(np.uint32))


def test_argument_errors_leave_the_outputs_untouched():
    lib = _lib.load()
    cond, null, want_out, want_factor, _ = _data(9)
    with guard(0xFF) as g:
        c, u = _put(g, cond), _put(g, null)
        out, factor = torch.empty_like(c), torch.empty(BK, dtype=torch.float32, device=DEV)
        ws = torch.empty(lib.osuf_cfg_rescale_workspace_bytes(BK, 54) // 8, dtype=torch.float64, device=DEV)
        out.fill_(7.0), factor.fill_(7.0)
        good = dict(cond=c.data_ptr(), nullp=u.data_ptr(), cs=CSK, phi=PHI, ws=ws.data_ptr(), factor=factor.data_ptr(), out=out.data_ptr(), B=BK, n=54)
        bad = [dict(cond=None), dict(nullp=None), dict(ws=None), dict(factor=None), dict(out=None), dict(B=0), dict(B=-1), dict(n=0), dict(n=-54),
               dict(phi=-0.5), dict(phi=1.5), dict(phi=float("nan")), dict(phi=float("inf")), dict(ws=ws.data_ptr() + 4)]
        for change in bad:
            assert lib.osuf_cfg_rescale(*{**good, **change}.values(), ops._stream()) == EINVAL, change
        g.check()
        assert (out == 7.0).all() and (factor == 7.0).all()
        with pytest.raises(ValueError):
            ops.cfg_rescale(c, u, CSK, 1.5)
        assert lib.osuf_cfg_rescale(*good.values(), ops._stream()) == 0
        g.check()
    assert _same_bits(out, GO.apply32(factor.cpu().numpy(), GO.guide32(cond, null, CSK))) and (GO.ulps32(factor.cpu().numpy(), want_factor) <= ULPS).all()


def test_the_two_launches_are_graph_capturable():
    """One linear capture on one stream; the replay writes the eager call's bits."""
    cond, null, _, _, _ = _data(5000)
    c, u = torch.from_numpy(cond).to(DEV), torch.from_numpy(null).to(DEV)
    want_out, want_factor = ops.cfg_rescale(c, u, CSK, PHI)
    out, factor = torch.empty_like(c), torch.empty(BK, dtype=torch.float32, device=DEV)
    ws = torch.empty(_lib.load().osuf_cfg_rescale_workspace_bytes(BK, 6 * 5000) // 8, dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.call("osuf_cfg_rescale", c.data_ptr(), u.data_ptr(), CSK, PHI, ws.data_ptr(), factor.data_ptr(), out.data_ptr(), BK, 6 * 5000, ops._stream())
    out.zero_(), factor.zero_(), ws.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(want_out)) and torch.equal(_bits(factor), _bits(want_factor))


# ---- the samplers ------------------------------------------------------------------------------------------------------------------------
B, N, STEPS, CS = 2, 96, 4, 2.0
LONG, WIN, STRIDE = 336, 96, 72                              # the windowed case: five windows, the last one clamped
BACKBONE_KW = {"dit": dict(backbone="dit", dim_h=96, depth=2, attn_heads=6, attn_dim_head=16),
               "mmdit": dict(backbone="mmdit", dim_h=64, depth=2, attn_heads=4, attn_kv_heads=2, attn_dim_head=16)}
KINDS = ["dit_ddim", "dit_flow", "ct_ddpm", "ct_ddim0", "ct_ddim_eta", "ct_2m"]
_CACHE = {}


def _model(kind, **extra):
    """A fresh model per test (a model kept alive across tests keeps its weight-pack jobs registered, see tests/test_inpaint_gpu.py)."""
    if kind == "dit_ddim":
        model = DiffusionOsuFusionDiT(sampling_timesteps=STEPS, **BACKBONE_KW["mmdit"])
    elif kind == "dit_flow":
        model = RectifiedFlowOsuFusionDiT(sampling_timesteps=STEPS, **BACKBONE_KW["dit"])
    else:
        sampler, eta = {"ct_ddpm": ("ddpm", 0.0), "ct_ddim0": ("ddim", 0.0), "ct_ddim_eta": ("ddim", 0.5), "ct_2m": ("dpmpp_2m", 0.0)}[kind]
        model = ContinuousDiffusionOsuFusionDiT(sampling_timesteps=STEPS, sampler=sampler, ddim_eta=eta, **extra, **BACKBONE_KW["mmdit"])
    model.load_state_dict({k: torch.from_numpy(param_pattern(k[len("unet."):], tuple(v.shape)).copy()) for k, v in model.state_dict().items()})
    return model.to(DEV)


def _inputs(n=N):
    if n not in _CACHE:
        x, a, c, _, noise = (torch.from_numpy(v).to(DEV) for v in synth_inputs("guidance", B, n))
        keep = torch.zeros(B, n, dtype=torch.bool, device=DEV)
        keep[0, :n // 3] = True
        keep[1, n // 2:(5 * n) // 6] = True
        _CACHE[n] = (a, c, noise.float().contiguous(), x.float().contiguous().clamp(-1, 1), keep)
    return _CACHE[n]


def _contexts(model):
    st = contextlib.ExitStack()
    for ctx in (torch.inference_mode(), ops.reproducible_mode(True), ops.one_launch_attention(True), model._dtype_ctx()):
        st.enter_context(ctx)
    return st


def _log_snr(kind, model):
    """The restatement's log-SNR of every denoiser call of a full run of `kind`, in call order (one entry per step; per evaluation for flow)."""
    if kind == "dit_ddim":
        return GO.ddim_log_snr(model.scheduler.alphas_cumprod.tolist(), model.train_timesteps, STEPS)
    if kind == "dit_flow":
        return GO.flow_log_snr(torch.linspace(0.0, 1.0, STEPS).tolist())
    if model.sampler == "ddpm":
        return GO.ct_log_snr(model.scheduler.log_snr(torch.linspace(1.0, 0.0, STEPS + 1, device=DEV)[:-1]).tolist())
    return GO.ct_log_snr(model.scheduler.solver_log_snr_grid(STEPS, model.solver_spacing, model.solver_logsnr_min, device=DEV)[:-1].tolist())


def _interval(kind, model):
    """Both ends exactly on a call's log-SNR, calls on either side: steps 1 and 2 of four; evaluations 2 to 4 of the flow loop's six."""
    ls = _log_snr(kind, model)
    assert ls == sorted(ls)
    return (ls[2], ls[4]) if kind == "dit_flow" else (ls[1], ls[2])


def _plain_f(model, a, c):
    """f(x, t, guided): the cfg = True / cfg = False forms of one denoiser."""
    den = model._denoiser(a, c, True)
    return lambda x, t, guided: den(x, t, guided)


def _windowed_f(model, a, c, batch):
    """The windowed denoiser written out (tests/test_windowed_gpu.py), every chunk's inner denoiser called guided or unguided."""
    b, n = a.shape[0], a.shape[-1]
    W = len(windowed.window_starts(n, WIN, STRIDE))
    rows = b * W
    a_w, c_w = ops.window_gather(a, WIN, STRIDE), c.repeat_interleave(W, 0)
    chunks = [(lo, min(lo + batch, rows)) for lo in range(0, rows, batch)]
    inner = [model._denoiser(a_w[lo:hi], c_w[lo:hi], True) for lo, hi in chunks]
    weight = windowed.window_weight(WIN, STRIDE, "trapezoid").to(DEV)

    def f(x, t, guided):
        g = 2 if guided else 1
        x_w = ops.window_gather(x, WIN, STRIDE)
        parts = [den(x_w[lo:hi], t[:1].repeat(g * (hi - lo)), guided).view(g, hi - lo, 6, WIN) for (lo, hi), den in zip(chunks, inner)]
        return ops.window_fuse(torch.cat(parts, 1).contiguous().view(g * rows, 6, WIN), weight, n, STRIDE)
    return f


def _written_out(kind, model, a, c, x, phi, guided, region=None, resample=1, window_batch=None):
    """The loop of `kind` over the public ops; guided[k]: whether denoiser call k of a full run (RePaint passes share their step's entry) runs
    2B rows.  A guided call with phi > 0: one ops.cfg_rescale, and the step (and the quantile) take (out, None)."""
    b = a.shape[0]
    x = x.float().contiguous()
    blend = None
    if region is not None:
        known, mask = region[0], inpaint.as_mask(region[1], b, x.shape[-1], DEV)
        blend = lambda v, coef=None, ca=0, cs=1, z=None: ops.inpaint_blend(v, known, mask, coef, ca, cs, z)  # noqa: E731
    draw = lambda: torch.randn(x.shape, device=DEV)  # noqa: E731
    with _contexts(model):
        f = _plain_f(model, a, c) if window_batch is None else _windowed_f(model, a, c, window_batch)

        def predict(xx, t, on, flow=False):
            if not on:
                return f(xx, t, False), None
            pred = f(xx, t, True)
            if phi > 0:
                return ops.cfg_rescale(pred[:b], pred[b:], CS, phi)[0], None
            return pred[:b], pred[b:]

        if kind == "dit_ddim":
            sch = model.scheduler
            sch.set_timesteps(STEPS)
            ts = sch.timesteps.tolist()
            coef = torch.tensor([[sch.step_coefficients(t)] * b for t in ts], dtype=torch.float32, device=DEV)
            eps = x.clone()
            if blend:
                x = blend(x, coef[0], 1, 0, eps)
            for i in range(STEPS):
                cond, null = predict(x, torch.full((2 * b,), ts[i], dtype=torch.int64, device=DEV), guided[i])
                x = ops.ddim_step(x, cond, null, CS, coef[i])
                if blend:
                    x = blend(x) if i == STEPS - 1 else blend(x, coef[i], 2, 3, eps)
            return x
        if kind == "dit_flow":
            ones = torch.ones(b, dtype=torch.float32, device=DEV)
            calls = iter(guided)

            def flow(t, y):
                cond, null = predict(y, torch.full((2 * b,), t, dtype=torch.float32, device=DEV), next(calls))
                return cond if null is None else ops.axpby_rows(null.contiguous(), cond.contiguous(), ones * (1.0 - CS), ones * CS)
            level = lambda t: torch.tensor([[t, 1.0 - t]] * b, dtype=torch.float32, device=DEV)  # noqa: E731
            times = torch.linspace(0.0, 1.0, STEPS).tolist()
            eps = x.clone()
            if blend:
                x = blend(x, level(times[0]), 0, 1, eps)
            for j, (t0, t1) in enumerate(zip(times[:-1], times[1:])):
                dt = t1 - t0
                mid = ops.axpby_rows(x, flow(t0, x), ones, ones * (0.5 * dt))
                if blend:
                    mid = blend(mid, level(t0 + 0.5 * dt), 0, 1, eps)
                x = ops.axpby_rows(x, flow(t0 + 0.5 * dt, mid), ones, ones * dt)
                if blend:
                    x = blend(x) if j == STEPS - 2 else blend(x, level(t1), 0, 1, eps)
            return x
        obj, q = model.pred_objective, model.dynamic_thresholding_percentile
        thr = lambda xx, cond, null, row: ops.ct_x0_quantile(xx, cond, null, CS, row, obj, q)[:, 2] if model.dynamic_thresholding else None  # noqa: E731
        if model.sampler == "ddpm":
            times = torch.linspace(1.0, 0.0, STEPS + 1, device=DEV, dtype=torch.float32)
            coef = model.scheduler.coefficients(times[:-1].repeat_interleave(b), times[1:].repeat_interleave(b)).view(STEPS, b, -1)
            log_snr = coef[:, :, 0].repeat(1, 2).contiguous()
            k_r, k_g = (coef[:, :, 1] / coef[:, :, 4]).contiguous(), (coef[:, :, 2] * torch.sqrt(coef[:, :, 6])).contiguous()
            if blend:
                x = blend(x, coef[0], 1, 2, draw())
            for i in range(STEPS):
                passes = resample if i < STEPS - 1 else 1
                for u in range(passes):
                    cond, null = predict(x, log_snr[i], guided[i])
                    noise = draw() if i < STEPS - 1 else None
                    if obj == "noise" and not model.dynamic_thresholding:
                        x = ops.ct_step(x, cond, null, CS, coef[i], noise)
                    else:
                        x = ops.ct_step_ex(x, cond, null, CS, coef[i], noise, obj, thr(x, cond, null, coef[i]))
                    if blend:
                        x = blend(x) if i == STEPS - 1 else blend(x, coef[i], 4, 5, draw())
                    if u < passes - 1:
                        x = ops.axpby_rows(x, draw(), k_r[i], k_g[i])
            return x
        grid = model.scheduler.solver_log_snr_grid(STEPS, model.solver_spacing, model.solver_logsnr_min, device=DEV)
        rows, fac = ops.ct_solver_schedule(grid, model.sampler, model.ddim_eta, b)
        fresh = model.sampler == "ddim" and model.ddim_eta > 0
        eps = None if fresh else x.clone()
        if blend:
            x = blend(x, rows[0], 1, 2, draw() if fresh else eps)
        prev = None
        for i in range(STEPS):
            cond, null = predict(x, grid[i].repeat(2 * b), guided[i])
            noise = draw() if fresh else None
            x, prev = ops.ct_solver_step(x, cond, null, CS, rows[i], fac[i], prev, noise, obj, thr(x, cond, null, rows[i]))
            if blend:
                x = blend(x) if i == STEPS - 1 else blend(x, rows[i], 4, 5, draw() if fresh else eps)
        return x


def _sample(model, a, c, x, seed=1234, cond_scale=CS, **kw):
    torch.manual_seed(seed)
    return model.sample(a, c, x, cond_scale=cond_scale, **kw)


@contextlib.contextmanager
def _counting(model):
    """model._denoiser wrapped so that every call of the closure it returns records the rows of its prediction."""
    calls, orig = [], model._denoiser

    def counting(a_, c_, cfg):
        f = orig(a_, c_, cfg)

        def g(*args):
            pred = f(*args)
            calls.append(pred.shape[0])
            return pred
        return g
    model._denoiser = counting
    try:
        yield calls
    finally:
        del model._denoiser


@contextlib.contextmanager
def _recording():
    names, orig = [], ops.call
    ops.call = lambda name, *args, **kw: (names.append(name), orig(name, *args, **kw))[1]
    try:
        yield names
    finally:
        ops.call = orig


MODES = {"both": (0.7, True), "rescale": (0.7, False), "interval": (0.0, True)}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", KINDS)
def test_sample_is_the_loop_written_out(kind, mode):
    """Bit-equal to the written-out loop from the same seed; 2B rows per denoiser call inside the interval and B outside, as the restatement's
    decision list says; one osuf_cfg_rescale per guided call with phi > 0 and none otherwise."""
    phi, bounded = MODES[mode]
    model = _model(kind)
    a, c, x, _, _ = _inputs()
    interval = _interval(kind, model) if bounded else None
    guided = GO.decide(_log_snr(kind, model), interval, CS)
    assert guided == (([False, False, True, True, True, False] if kind == "dit_flow" else [False, True, True, False]) if bounded else [True] * len(guided))
    with _counting(model) as calls, _recording() as names:
        got = _sample(model, a, c, x, guidance_rescale=phi, guidance_interval=interval)
    assert calls == GO.rows_per_call(guided, B)
    assert names.count("osuf_cfg_rescale") == (sum(guided) if phi > 0 else 0)
    torch.manual_seed(1234)
    want = _written_out(kind, model, a, c, x, phi, guided)
    assert got.shape == x.shape and torch.isfinite(got).all() and torch.equal(_bits(got), _bits(want))
    assert torch.equal(_bits(got), _bits(_sample(model, a, c, x, guidance_rescale=phi, guidance_interval=interval)))
    assert not torch.equal(got, _sample(model, a, c, x))                            # the keywords change the result


@pytest.mark.parametrize("kind", ["ct_ddpm", "ct_2m"])
def test_with_dynamic_thresholding(kind):
    """A v-prediction model with dynamic thresholding: the quantile of a rescaled step is taken of (out, None), of an unguided step of
    (cond, None)."""
    model = _model(kind, pred_objective="v", dynamic_thresholding=True, dynamic_thresholding_percentile=0.9)
    a, c, x, _, _ = _inputs()
    interval = _interval(kind, model)
    guided = GO.decide(_log_snr(kind, model), interval, CS)
    with _counting(model) as calls, _recording() as names:
        got = _sample(model, a, c, x, guidance_rescale=0.7, guidance_interval=interval)
    assert calls == GO.rows_per_call(guided, B) and names.count("osuf_cfg_rescale") == 2 and names.count("osuf_ct_x0_quantile") == STEPS
    torch.manual_seed(1234)
    assert torch.isfinite(got).all() and torch.equal(_bits(got), _bits(_written_out(kind, model, a, c, x, 0.7, guided)))


def test_with_a_known_region_and_resampling():
    """known / known_mask and resample = 2 on the ancestral sampler: the two passes of a step share its decision, the draws keep their order."""
    model = _model("ct_ddpm")
    a, c, x, known, keep = _inputs()
    interval = _interval("ct_ddpm", model)
    guided = GO.decide(_log_snr("ct_ddpm", model), interval, CS)
    per_call = [g for i, g in enumerate(guided) for _ in range(2 if i < STEPS - 1 else 1)]
    with _counting(model) as calls:
        got = _sample(model, a, c, x, known=known, known_mask=keep, resample=2, guidance_rescale=0.7, guidance_interval=interval)
    assert calls == GO.rows_per_call(per_call, B) == [2, 2, 4, 4, 4, 4, 2]
    torch.manual_seed(1234)
    want = _written_out("ct_ddpm", model, a, c, x, 0.7, guided, region=(known, keep), resample=2)
    on = keep[:, None, :].expand_as(got)
    assert torch.isfinite(got).all() and torch.equal(_bits(got), _bits(want)) and torch.equal(_bits(got[on]), _bits(known[on]))


@pytest.mark.parametrize("kind", ["dit_ddim", "ct_2m"])
def test_windowed_with_window_batch(kind):
    """n = 336 in windows of 96: the ten window rows go to the backbone in chunks of 4, 4 and 2, guided (twice the rows) or not, and the
    rescale sees the fused full-length prediction."""
    model = _model(kind)
    a, c, x, _, _ = _inputs(LONG)
    interval = _interval(kind, model)
    guided = GO.decide(_log_snr(kind, model), interval, CS)
    with _counting(model) as calls, _recording() as names:
        got = _sample(model, a, c, x, window=WIN, window_stride=STRIDE, window_batch=4, guidance_rescale=0.7, guidance_interval=interval)
    assert calls == [r * (2 if g else 1) for g in guided for r in (4, 4, 2)] and names.count("osuf_cfg_rescale") == 2
    torch.manual_seed(1234)
    want = _written_out(kind, model, a, c, x, 0.7, guided, window_batch=4)
    assert got.shape == x.shape and torch.isfinite(got).all() and torch.equal(_bits(got), _bits(want))


@pytest.mark.parametrize("kind", KINDS)
def test_defaults_and_an_all_containing_interval_are_the_positional_call(kind):
    """sample() through the signature it had before the keywords, against the keywords at their defaults and against an interval that
    contains every call at phi = 0: the same launches by name, in order, and the same bits."""
    model = _model(kind)
    a, c, x, _, _ = _inputs()
    model.sample(a, c, x, CS)                                                       # the first call packs the weights: not part of the comparison
    torch.manual_seed(9)
    with _recording() as old_names:
        old = model.sample(a, c, x, CS)
    assert torch.isfinite(old).all() and "osuf_cfg_rescale" not in old_names
    for kw in (dict(guidance_rescale=0.0, guidance_interval=None), dict(guidance_interval=(None, None)), dict(guidance_interval=(-1e30, 1e30)),
               dict(guidance_rescale=0.0, guidance_interval=(None, 1e30))):
        torch.manual_seed(9)
        with _counting(model) as calls, _recording() as names:
            new = model.sample(a, c, x, cond_scale=CS, **kw)
        finite_lo = kw.get("guidance_interval") == (-1e30, 1e30) and kind == "dit_flow"     # the flow loop's t = 0 is at -inf: outside
        if finite_lo:
            assert calls == [B] + [2 * B] * 5
        else:
            assert names == old_names and torch.equal(_bits(old), _bits(new)) and set(calls) == {2 * B}, kw


@pytest.mark.parametrize("kind", ["dit_ddim", "dit_flow", "ct_2m"])
def test_cond_scale_one_accepts_both_and_changes_nothing(kind):
    model = _model(kind)
    a, c, x, _, _ = _inputs()
    _sample(model, a, c, x, cond_scale=1.0)                                         # packs the weights
    with _recording() as old_names:
        old = _sample(model, a, c, x, cond_scale=1.0)
    with _counting(model) as calls, _recording() as names:
        new = _sample(model, a, c, x, cond_scale=1.0, guidance_rescale=0.7, guidance_interval=(-1.0, 1.0))
    assert names == old_names and set(calls) == {B} and torch.equal(_bits(old), _bits(new))
