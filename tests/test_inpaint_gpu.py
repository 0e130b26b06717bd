"""Masked generation on the GPU: osuf_inpaint_blend against its np.float32 restatement (tests/inpaint_oracle.blend32), bit for bit, on
poisoned and canary-guarded memory (tests/memguard.py), and the five masked sampling loops against the same loops written out over ops
calls with the documented draw order."""
import contextlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F  # noqa: N812

from osufusion_amd import _lib, ct, inpaint, ops
from osufusion_amd import runtime as rt
from osufusion_amd.models import ContinuousDiffusionOsuFusionDiT, DiffusionOsuFusionDiT, RectifiedFlowOsuFusionDiT
from osufusion_amd.models.diffusion import OsuFusion
from osufusion_amd.models.rectified_flow import OsuFusion as FlowOsuFusion
from osufusion_amd.pattern import param_pattern, synth_inputs
from tests import inpaint_oracle as IO
from tests.memguard import guard

pytestmark = pytest.mark.gpu
DEV = "cuda"
EINVAL = -1
BELOW_ONE = float(np.nextafter(np.float32(1.0), np.float32(0.0)))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(got: torch.Tensor, want: np.ndarray) -> bool:
    return np.array_equal(got.detach().cpu().numpy().view(np.uint32), np.ascontiguousarray(want, dtype=np.float32).view(np.uint32))


# ---- the kernel --------------------------------------------------------------------------------------------------------------------------
# (1, 1, 1) and (3, 6, 5): the scalar path; (2, 6, 8): the four-wide path; (3, 1, 1027): a scalar row longer than one workgroup's 256 lanes
# with a tail; (2, 6, 4100): 6150 groups of four, more than one workgroup per sample, the last one partly idle.
SHAPES = [(1, 1, 1), (3, 6, 5), (2, 6, 8), (3, 1, 1027), (2, 6, 4100)]


def _masks(rng, B, L):
    hard = (rng.random((B, L)) < 0.5).astype(np.float32)
    soft = rng.random((B, L)).astype(np.float32)
    pick = rng.integers(0, 5, (B, L))
    soft = np.where(pick == 0, 0.0, np.where(pick == 1, 1.0, np.where(pick == 2, 0.5, np.where(pick == 3, BELOW_ONE, soft)))).astype(np.float32)
    return {"hard_shared": hard[0], "hard_rows": hard, "soft_shared": soft[0], "soft_rows": soft}


def _operands(rng, shape):
    B = shape[0]
    x, known, noise = (rng.standard_normal(shape).astype(np.float32) for _ in range(3))
    coef13 = rng.uniform(0.05, 1.0, (B, 13)).astype(np.float32)
    coef4 = rng.uniform(0.05, 1.0, (B, 4)).astype(np.float32)
    return x, known, noise, coef13, coef4


def _run(g, x, known, mask, coef=None, col_a=0, col_s=1, noise=None, in_place=False, offset=False):
    """The operands placed in guarded allocations (offset: every (B, Dch, L) operand and the mask one float into its buffer) -> the output."""
    def put(v):
        if v is None:
            return None
        t = torch.from_numpy(np.ascontiguousarray(v))
        if not offset:
            return g.place(t.to(DEV))
        buf = g.place(torch.cat([torch.zeros(1), t.reshape(-1)]).to(DEV))
        return buf[1:].view(t.shape)
    xd, kd, nd, md, cd = put(x), put(known), put(noise), put(mask), (None if coef is None else g.place(torch.from_numpy(coef).to(DEV)))
    if in_place:
        got = ops.inpaint_blend(xd, kd, md, cd, col_a, col_s, nd, out=xd)
        assert got.data_ptr() == xd.data_ptr()
    elif offset:
        ob = torch.empty(xd.numel() + 1, dtype=torch.float32, device=DEV)
        got = ops.inpaint_blend(xd, kd, md, cd, col_a, col_s, nd, out=ob[1:].view(xd.shape))
        assert torch.isnan(ob[0]).item()                              # the float in front of the output keeps its poison
    else:
        got = ops.inpaint_blend(xd, kd, md, cd, col_a, col_s, nd)
    g.check()
    return got


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_blend_bits(shape):
    """Every mask kind x every operand variant, out of place, in place and one float off alignment: the restatement's bits."""
    rng = np.random.default_rng(sum(shape))
    x, known, noise, coef13, coef4 = _operands(rng, shape)
    variants = {"rows13": dict(coef=coef13, col_a=ct.ALPHA_NEXT, col_s=ct.SIGMA_NEXT, noise=noise), "rows4": dict(coef=coef4, col_a=1, col_s=0, noise=noise),
                "no_noise": dict(coef=coef13, col_a=ct.ALPHA, col_s=ct.SIGMA, noise=None), "exact": dict()}
    with guard(0xFF) as g:
        for mname, mask in _masks(rng, shape[0], shape[2]).items():
            for vname, kw in variants.items():
                want = IO.blend32(x, known, mask, kw.get("coef"), kw.get("col_a", 0), kw.get("col_s", 1), kw.get("noise"))
                assert np.isfinite(want).all()
                for how in (dict(), dict(in_place=True), dict(offset=True)):
                    got = _run(g, x, known, mask, **kw, **how)
                    assert _same_bits(got, want), (mname, vname, how)
            g.release()
        noisy_exact = _run(g, x, known, mask, None, 0, 1, np.full(shape, np.nan, np.float32))       # coef NULL: the noise given is not read
        assert _same_bits(noisy_exact, IO.blend32(x, known, mask))


def test_bool_mask_and_strided_rows():
    """A bool mask is converted once; coef and mask rows may be column / row slices of wider tensors (their strides are the leading dims)."""
    rng = np.random.default_rng(3)
    shape = (3, 6, 8)
    x, known, noise, coef13, _ = _operands(rng, shape)
    keep = rng.random((3, 8)) < 0.5
    wide_mask = torch.zeros(3, 24, device=DEV)
    wide_mask[:, 8:16] = torch.from_numpy(keep).float().to(DEV)
    wide_coef = torch.from_numpy(np.concatenate([coef13, coef13 + 1], 1)).to(DEV)
    want = IO.blend32(x, known, keep.astype(np.float32), coef13, 4, 5, noise)
    xd, kd, nd = (torch.from_numpy(v).to(DEV) for v in (x, known, noise))
    with guard(0xFF) as g:
        assert _same_bits(ops.inpaint_blend(xd, kd, torch.from_numpy(keep).to(DEV), torch.from_numpy(coef13).to(DEV), 4, 5, nd), want)
        assert _same_bits(ops.inpaint_blend(xd, kd, wide_mask[:, 8:16], wide_coef[:, :13], 4, 5, nd), want)
        assert _same_bits(ops.inpaint_blend(xd, kd, wide_mask[:, 8:16], wide_coef[:, 13:], 4, 5, nd),
                          IO.blend32(x, known, keep.astype(np.float32), coef13 + 1, 4, 5, noise))
        g.check()


@pytest.mark.parametrize("shape", [(3, 6, 5), (2, 6, 8)], ids=["scalar", "vec"])
def test_selects_do_not_leak_what_lies_under_them(shape):
    """NaN in known and noise wherever m == 0 and in x wherever m == 1: the output is finite and has the bits of the clean operands'."""
    rng = np.random.default_rng(11)
    x, known, noise, coef13, _ = _operands(rng, shape)
    masks = _masks(rng, shape[0], shape[2])
    with guard(0xFF) as g:
        for mname in ("hard_rows", "soft_shared"):
            mask = masks[mname]
            m = np.broadcast_to(mask[None, None, :] if mask.ndim == 1 else mask[:, None, :], shape)
            xp, kp, zp = np.where(m == 1, np.nan, x), np.where(m == 0, np.nan, known), np.where(m == 0, np.nan, noise)
            want = IO.blend32(x, known, mask, coef13, 1, 2, noise)
            for kw in (dict(), dict(in_place=True)):
                got = _run(g, xp.astype(np.float32), kp.astype(np.float32), mask, coef13, 1, 2, zp.astype(np.float32), **kw)
                assert torch.isfinite(got).all() and _same_bits(got, want), (mname, kw)
            got = _run(g, xp.astype(np.float32), kp.astype(np.float32), mask)
            assert torch.isfinite(got).all() and _same_bits(got, IO.blend32(x, known, mask))


def test_negative_zero_survives_the_exact_blend():
    x = np.ones((2, 6, 8), np.float32)
    known = np.full((2, 6, 8), -0.0, np.float32)
    mask = np.array([1, 0, 1, 1, 0, 1, 0, 1], np.float32)
    x[:, :, 1] = -0.0
    with guard(0xFF) as g:
        for kw in (dict(), dict(offset=True)):
            got = _run(g, x, known, mask, **kw).cpu().numpy()
            assert np.signbit(got[:, :, mask == 1]).all() and (got[:, :, mask == 1] == 0).all()
            assert np.signbit(got[:, :, 1]).all() and (got[:, :, [4, 6]] == 1).all()


def test_argument_errors_leave_the_output_untouched():
    lib = _lib.load()
    B, D, L = 2, 6, 8
    t = {k: torch.randn(B, D, L, device=DEV) for k in ("x", "known", "noise")}
    mask, coef = torch.ones(B, L, device=DEV), torch.rand(B, 13, device=DEV)
    out = torch.full((B, D, L), 7.0, device=DEV)
    good = dict(x=t["x"].data_ptr(), known=t["known"].data_ptr(), noise=t["noise"].data_ptr(), mask=mask.data_ptr(), mask_ld=L, coef=coef.data_ptr(),
                coef_ld=13, col_a=1, col_s=2, out=out.data_ptr(), B=B, Dch=D, L=L)
    order = list(good)
    bad = [dict(x=None), dict(known=None), dict(mask=None), dict(B=0), dict(Dch=0), dict(L=0), dict(B=-1), dict(mask_ld=-1), dict(coef_ld=0),
           dict(col_a=-1), dict(col_s=-1)]
    for change in bad:
        args = {**good, **change}
        assert lib.osuf_inpaint_blend(*[args[k] for k in order], ops._stream()) == EINVAL, change
    assert lib.osuf_inpaint_blend(*[{**good, "out": None}[k] for k in order], ops._stream()) == EINVAL
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    # without coef the leading dimension and the columns are not looked at
    assert lib.osuf_inpaint_blend(*[{**good, "coef": None, "coef_ld": 0, "col_a": -1, "col_s": -1}[k] for k in order], ops._stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(t["known"]))


def test_blend_is_graph_capturable():
    x, known, noise = (torch.randn(2, 6, 96, device=DEV) for _ in range(3))
    mask, coef = (torch.rand(2, 96, device=DEV) < 0.5).float(), torch.rand(2, 13, device=DEV)
    out = torch.empty_like(x)
    want = ops.inpaint_blend(x, known, mask, coef, 1, 2, noise)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.inpaint_blend(x, known, mask, coef, 1, 2, noise, out=out)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(want))


# ---- the five loops --------------------------------------------------------------------------------------------------------------------------
N, STEPS, CS = 96, 4, 2.0
UNET_KW = dict(dim_h_mult=(1, 2), num_layer_blocks=(1, 1), num_middle_transformers=1, cross_embed_kernel_sizes=(3,), attn_dim_head=64, attn_heads=2,
               attn_kv_heads=1, attn_context_len=256)
BACKBONE_KW = {"dit": dict(backbone="dit", dim_h=96, depth=2, attn_heads=6, attn_dim_head=16),
               "mmdit": dict(backbone="mmdit", dim_h=64, depth=2, attn_heads=4, attn_kv_heads=2, attn_dim_head=16)}
_CACHE = {}


def _patterned(model, prefix=""):
    model.load_state_dict({k: torch.from_numpy(param_pattern(k[len(prefix):], tuple(v.shape)).copy()) for k, v in model.state_dict().items()})
    return model.to(DEV)


def _model(kind):
    """A fresh model per test: a model kept alive across tests keeps its weight-pack jobs registered (functional._PACK_JOBS), which the
    pack tests of tests/test_round2_gpu.py and tests/test_round3_gpu.py walk."""
    if kind == "unet_ddim":
        return _patterned(OsuFusion(32, sampling_timesteps=STEPS, **UNET_KW), "unet.")
    if kind == "unet_flow":
        return _patterned(FlowOsuFusion(32, sampling_timesteps=STEPS, **UNET_KW), "unet.")
    if kind == "dit_ddim":
        return _patterned(DiffusionOsuFusionDiT(sampling_timesteps=STEPS, **BACKBONE_KW["mmdit"]), "unet.")
    if kind == "dit_flow":
        return _patterned(RectifiedFlowOsuFusionDiT(sampling_timesteps=STEPS, **BACKBONE_KW["dit"]), "unet.")
    sampler, eta = {"ct_ddpm": ("ddpm", 0.0), "ct_ddim0": ("ddim", 0.0), "ct_ddim_eta": ("ddim", 0.5), "ct_2m": ("dpmpp_2m", 0.0)}[kind]
    return _patterned(ContinuousDiffusionOsuFusionDiT(sampling_timesteps=STEPS, sampler=sampler, ddim_eta=eta, **BACKBONE_KW["mmdit"]), "unet.")


KINDS = ["unet_ddim", "unet_flow", "dit_ddim", "dit_flow", "ct_ddpm", "ct_ddim0", "ct_ddim_eta", "ct_2m"]
STOCHASTIC = ("ct_ddpm", "ct_ddim_eta")


def _inputs():
    if "inputs" not in _CACHE:
        x, a, c, _, noise = (torch.from_numpy(v).to(DEV) for v in synth_inputs("inpaint", 2, N))
        keep = torch.zeros(2, N, dtype=torch.bool, device=DEV)
        keep[0, :40] = True
        keep[1, 30:70] = True
        _CACHE["inputs"] = (a, c, noise.float().contiguous(), x.float().contiguous().clamp(-1, 1), keep)
    return _CACHE["inputs"]


def _contexts(model):
    if isinstance(model, (OsuFusion, FlowOsuFusion)):
        reproducible = getattr(model, "reproducible_sampling", True)
        return lambda: _stack(torch.inference_mode(), ops.reproducible_mode(reproducible), model._dtype_ctx())
    return lambda: _stack(torch.inference_mode(), ops.reproducible_mode(True), ops.one_launch_attention(True), model._dtype_ctx())


def _stack(*ctxs):
    st = contextlib.ExitStack()
    for c in ctxs:
        st.enter_context(c)
    return st


def _denoiser(model, a, c, counter=None):
    """f(x, t (2B,)) -> the prediction (2B, 6, n) with guidance rows, as the samplers call the backbone; the UNet's written out from its parts."""
    b, n = a.shape[0], a.shape[-1]
    if not isinstance(model, (OsuFusion, FlowOsuFusion)):
        f = model._denoiser(a, c, True)
    else:
        unet = model.unet
        depth = len(unet.down_layers)
        pad_len = (2 ** depth - (n % (2 ** depth))) % (2 ** depth)
        dtype = rt.compute_dtype(unet.final_conv.weight.dtype)
        a_rows = unet.encode_audio(a, pad_len, dtype)
        a_rows = torch.cat([a_rows, a_rows], 0)
        keep = torch.ones(b, dtype=torch.bool, device=DEV)
        ce = unet.embed_cond(torch.cat([c, c], 0), torch.cat([keep, ~keep], 0))

        def f(x, t):
            x_rows = unet.init_x.forward_rows(F.pad(torch.cat([x, x], 0), (0, pad_len), value=-1.0), dtype)
            return unet.denoise_rows(x_rows, a_rows, unet.embed_time(t), ce)[:, :, :n].contiguous()
    if counter is None:
        return f

    def counted(x, t):
        counter.append(1)
        return f(x, t)
    return counted


def _written_out(kind, model, a, c, x, known, keep, stop_after=None, resample=1, counter=None):
    """The masked loop of `kind` over ops calls: the rule of the docstrings, the draws in their documented order."""
    b = a.shape[0]
    x = x.float().contiguous()
    mask = inpaint.as_mask(keep, b, x.shape[-1], DEV)
    blend = lambda v, coef=None, ca=0, cs=1, z=None: ops.inpaint_blend(v, known, mask, coef, ca, cs, z)
    with _contexts(model)():
        if kind.endswith("ddim") and not kind.startswith("ct"):
            sch = model.scheduler
            sch.set_timesteps(STEPS)
            ts = sch.timesteps.tolist()
            coef = torch.tensor([[sch.step_coefficients(t)] * b for t in ts], dtype=torch.float32, device=DEV)
            f = _denoiser(model, a, c, counter)
            eps = x.clone()
            x = blend(x, coef[0], 1, 0, eps)
            for i in range(STEPS if stop_after is None else stop_after):
                pred = f(x, torch.full((2 * b,), ts[i], dtype=torch.int64, device=DEV))
                x = ops.ddim_step(x, pred[:b], pred[b:], CS, coef[i])
                x = blend(x) if i == STEPS - 1 else blend(x, coef[i], 2, 3, eps)
            return x
        if kind.endswith("flow"):
            ones = torch.ones(b, dtype=torch.float32, device=DEV)
            den = _denoiser(model, a, c, counter)

            def f(t, y):
                out = den(y, torch.full((2 * b,), t, dtype=torch.float32, device=DEV))
                return ops.axpby_rows(out[b:].contiguous(), out[:b].contiguous(), ones * (1.0 - CS), ones * CS)
            level = lambda t: torch.tensor([[t, 1.0 - t]] * b, dtype=torch.float32, device=DEV)
            times = torch.linspace(0.0, 1.0, STEPS).tolist()
            eps = x.clone()
            x = blend(x, level(times[0]), 0, 1, eps)
            for j, (t0, t1) in enumerate(zip(times[:-1], times[1:])):
                dt = t1 - t0
                k1 = f(t0, x)
                mid = blend(ops.axpby_rows(x, k1, ones, ones * (0.5 * dt)), level(t0 + 0.5 * dt), 0, 1, eps)
                k2 = f(t0 + 0.5 * dt, mid)
                x = ops.axpby_rows(x, k2, ones, ones * dt)
                x = blend(x) if j == STEPS - 2 else blend(x, level(t1), 0, 1, eps)
            return x
        steps = STEPS if stop_after is None else stop_after
        draw = lambda: torch.randn(x.shape, device=DEV)
        if model.sampler == "ddpm":
            times = torch.linspace(1.0, 0.0, STEPS + 1, device=DEV, dtype=torch.float32)
            coef = model.scheduler.coefficients(times[:-1].repeat_interleave(b), times[1:].repeat_interleave(b)).view(STEPS, b, -1)
            log_snr = coef[:, :, 0].repeat(1, 2).contiguous()
            f = _denoiser(model, a, c, counter)
            x = blend(x, coef[0], 1, 2, draw())
            for i in range(steps):
                for u in range(resample if i < STEPS - 1 else 1):
                    pred = f(x, log_snr[i])
                    x = ops.ct_step(x, pred[:b], pred[b:], CS, coef[i], draw() if i < STEPS - 1 else None)
                    x = blend(x) if i == STEPS - 1 else blend(x, coef[i], 4, 5, draw())
                    if u < resample - 1 and i < STEPS - 1:
                        k_r = (coef[i][:, 1] / coef[i][:, 4]).contiguous()
                        k_g = (coef[i][:, 2] * torch.sqrt(coef[i][:, 6])).contiguous()
                        x = ops.axpby_rows(x, draw(), k_r, k_g)
            return x
        grid = model.scheduler.solver_log_snr_grid(STEPS, model.solver_spacing, model.solver_logsnr_min, device=DEV)
        rows, fac = ops.ct_solver_schedule(grid, model.sampler, model.ddim_eta, b)
        f = _denoiser(model, a, c, counter)
        fresh = model.sampler == "ddim" and model.ddim_eta > 0
        eps = None if fresh else x.clone()
        x = blend(x, rows[0], 1, 2, draw() if fresh else eps)
        prev = None
        for i in range(steps):
            pred = f(x, grid[i].repeat(2 * b))
            x, prev = ops.ct_solver_step(x, pred[:b], pred[b:], CS, rows[i], fac[i], prev, draw() if fresh else None, model.pred_objective, None)
            x = blend(x) if i == STEPS - 1 else blend(x, rows[i], 4, 5, draw() if fresh else eps)
        return x


def _sample(model, a, c, x, seed=1234, **kw):
    """sample() on the transformer models; the two UNet models keep the reference's signature there and take known / known_mask through
    sample_masked()."""
    torch.manual_seed(seed)
    return getattr(model, "sample_masked", model.sample)(a, c, x, cond_scale=CS, **kw)


@pytest.mark.parametrize("kind", KINDS)
def test_masked_sample_is_the_loop_written_out(kind):
    """Bit-equal to the written-out loop from the same seed, and again on a second call; where the mask is 1 the full run returns `known`
    bit for bit; the start iterate passed in is not written."""
    model = _model(kind)
    a, c, x, known, keep = _inputs()
    x_before = x.clone()
    got = _sample(model, a, c, x, known=known, known_mask=keep)
    again = _sample(model, a, c, x, known=known, known_mask=keep)
    torch.manual_seed(1234)
    want = _written_out(kind, model, a, c, x, known, keep)
    assert got.shape == x.shape and got.dtype == torch.float32 and torch.isfinite(got).all()
    assert torch.equal(_bits(got), _bits(again)) and torch.equal(_bits(got), _bits(want))
    on = keep[:, None, :].expand_as(got)
    assert torch.equal(_bits(got[on]), _bits(known[on]))
    assert not torch.equal(got[~on], known[~on]) and torch.equal(x, x_before)
    unmasked = _sample(model, a, c, x)
    assert not torch.equal(got, unmasked)
    # a float mask of the same values, shaped (B, 1, n), is the same call
    assert torch.equal(_bits(got), _bits(_sample(model, a, c, x, known=known, known_mask=keep.float()[:, None, :])))


@pytest.mark.parametrize("kind", KINDS)
def test_all_zero_mask_is_the_unmasked_sample(kind):
    model = _model(kind)
    a, c, x, known, keep = _inputs()
    zero = torch.zeros(N, dtype=torch.bool, device=DEV)
    poisoned = torch.full_like(known, float("nan"))                   # under m == 0 nothing of `known` is read into the result
    got = _sample(model, a, c, x, known=poisoned, known_mask=zero)
    assert torch.isfinite(got).all()
    if kind in STOCHASTIC:                                             # the blends still draw: the written-out loop is the yardstick
        torch.manual_seed(1234)
        assert torch.equal(_bits(got), _bits(_written_out(kind, model, a, c, x, poisoned, zero)))
    else:
        assert torch.equal(_bits(got), _bits(_sample(model, a, c, x)))


@pytest.mark.parametrize("kind", ["unet_ddim", "dit_ddim", "ct_ddpm", "ct_ddim0", "ct_ddim_eta", "ct_2m"])
def test_stop_after_one_returns_the_level_blended_iterate(kind):
    model = _model(kind)
    a, c, x, known, keep = _inputs()
    model.stop_after = 1
    try:
        got = _sample(model, a, c, x, known=known, known_mask=keep)
    finally:
        model.stop_after = None
    torch.manual_seed(1234)
    want = _written_out(kind, model, a, c, x, known, keep, stop_after=1)
    assert torch.equal(_bits(got), _bits(want))
    on = keep[:, None, :].expand_as(got)
    assert not torch.equal(got[on], known[on])                         # a level blend, not the exact one
    if kind not in STOCHASTIC:                                         # a known + s eps at the level the first step arrived at
        if kind.startswith("ct"):
            grid = model.scheduler.solver_log_snr_grid(STEPS, model.solver_spacing, model.solver_logsnr_min, device=DEV)
            coef, cols = ops.ct_solver_schedule(grid, model.sampler, model.ddim_eta, 2)[0][0], (4, 5)
        else:
            model.scheduler.set_timesteps(STEPS)
            coef = torch.tensor([model.scheduler.step_coefficients(model.scheduler.timesteps.tolist()[0])] * 2, dtype=torch.float32, device=DEV)
            cols = (2, 3)
        level = IO.blend32(np.zeros(x.shape, np.float32), known.cpu().numpy(), np.ones(N, np.float32), coef.cpu().numpy(), *cols, x.cpu().numpy())
        assert torch.equal(_bits(got[on]), _bits(torch.from_numpy(level).to(DEV)[on]))


def test_unet_graph_replay_equals_eager_at_three_steps():
    model = _model("unet_ddim")
    a, c, x, known, keep = _inputs()
    model.sampling_timesteps = 3
    try:
        eager = _sample(model, a, c, x, known=known, known_mask=keep)
        model.use_hip_graph = True
        replayed = _sample(model, a, c, x, known=known, known_mask=keep)
    finally:
        model.use_hip_graph = False
        model.sampling_timesteps = STEPS
    on = keep[:, None, :].expand_as(eager)
    assert torch.isfinite(eager).all() and torch.equal(_bits(eager), _bits(replayed)) and torch.equal(_bits(eager[on]), _bits(known[on]))


def test_resample_three_on_the_ancestral_sampler():
    model = _model("ct_ddpm")
    a, c, x, known, keep = _inputs()
    calls = []
    orig = model._denoiser

    def counting(a_, c_, cfg):
        f = orig(a_, c_, cfg)

        def g(x_, t_):
            calls.append(1)
            return f(x_, t_)
        return g
    model._denoiser = counting
    try:
        got = _sample(model, a, c, x, known=known, known_mask=keep, resample=3)
    finally:
        del model._denoiser
    assert len(calls) == 3 * (STEPS - 1) + 1
    written = []
    torch.manual_seed(1234)
    want = _written_out("ct_ddpm", model, a, c, x, known, keep, resample=3, counter=written)
    assert len(written) == 3 * (STEPS - 1) + 1
    on = keep[:, None, :].expand_as(got)
    assert torch.isfinite(got).all() and torch.equal(_bits(got), _bits(want)) and torch.equal(_bits(got[on]), _bits(known[on]))
    assert not torch.equal(got, _sample(model, a, c, x, known=known, known_mask=keep))


@pytest.mark.parametrize("kind", KINDS)
def test_defaults_are_the_positional_call(kind):
    """sample() without the new arguments against the call through the signature it had before them."""
    model = _model(kind)
    a, c, x, _, _ = _inputs()
    torch.manual_seed(9)
    old = model.sample(a, c, x, CS)
    torch.manual_seed(9)
    entry = getattr(model, "sample_masked", model.sample)
    new = entry(a, c, x, cond_scale=CS, known=None, known_mask=None, **({"resample": 1} if kind.startswith("ct") else {}))
    assert torch.isfinite(old).all() and torch.equal(_bits(old), _bits(new))
