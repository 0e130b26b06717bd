"""Windowed sampling on the GPU: osuf_window_gather / osuf_window_fuse against their np.float32 restatement (tests/windowed_oracle.py), bit for
bit, on poisoned and canary-guarded memory (tests/memguard.py), and the windowed transformer sampling loops against the same loops written
out over ops calls -- gather, model._denoiser on the window batch, fuse -- with the documented draw order."""
import contextlib

import numpy as np
import pytest
import torch

from osufusion_amd import _lib, inpaint, ops, windowed
from osufusion_amd.models import ContinuousDiffusionOsuFusionDiT, DiffusionOsuFusionDiT, RectifiedFlowOsuFusionDiT
from osufusion_amd.pattern import param_pattern, synth_inputs
from tests import windowed_oracle as WO
from tests.memguard import guard

pytestmark = pytest.mark.gpu
DEV = "cuda"
EINVAL = -1
TAPERS = ("trapezoid", "flat")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(got: torch.Tensor, want: np.ndarray) -> bool:
    return np.array_equal(got.detach().cpu().numpy().view(np.uint32), np.ascontiguousarray(want, dtype=np.float32).view(np.uint32))


# ---- the kernels -------------------------------------------------------------------------------------------------------------------------
# (R, D, n, window, stride).  (1, 1, 5, 4, 4): the scalar path, a clamped last window; (3, 6, 9, 4, 3); (2, 6, 11, 4, 1): four windows per
# frame; (2, 6, 24, 8, 4): the four-wide path, an exact fit; (2, 6, 28, 8, 8): four-wide, stride = window, a clamped last window;
# (3, 1, 1027, 256, 192): scalar rows longer than a workgroup, with a tail; (2, 6, 4100, 1024, 768): more than one workgroup per row.
SHAPES = [(1, 1, 5, 4, 4), (3, 6, 9, 4, 3), (2, 6, 11, 4, 1), (2, 6, 24, 8, 4), (2, 6, 28, 8, 8), (3, 1, 1027, 256, 192), (2, 6, 4100, 1024, 768)]
IDS = lambda s: "x".join(map(str, s))  # noqa: E731


def _put(g, v, offset=False):
    """A test operand at the front of a guarded allocation, or (offset) one float into it: off 16-byte alignment."""
    t = torch.from_numpy(np.ascontiguousarray(v))
    if not offset:
        return g.place(t.to(DEV))
    buf = g.place(torch.cat([torch.zeros(1), t.reshape(-1)]).to(DEV))
    return buf[1:].view(t.shape)


def _out(shape, offset):
    """None (the wrapper allocates) or an output one float into a (guarded, poisoned) buffer, with that buffer."""
    if not offset:
        return None, None
    buf = torch.empty(int(np.prod(shape)) + 1, dtype=torch.float32, device=DEV)
    return buf[1:].view(shape), buf


def _gather(g, src, window, stride, offset=False):
    R, D, n = src.shape
    W = len(WO.starts(n, window, stride))
    out, buf = _out((R * W, D, window), offset)
    got = ops.window_gather(_put(g, src, offset), window, stride, out=out)
    g.check()
    assert tuple(got.shape) == (R * W, D, window) and (buf is None or torch.isnan(buf[0]).item())   # the float in front keeps its poison
    return got


def _fuse(g, pred, w, n, stride, offset=False):
    RW, D, window = pred.shape
    R = RW // len(WO.starts(n, window, stride))
    out, buf = _out((R, D, n), offset)
    got = ops.window_fuse(_put(g, pred, offset), _put(g, w, offset), n, stride, out=out)
    g.check()
    assert tuple(got.shape) == (R, D, n) and (buf is None or torch.isnan(buf[0]).item())
    return got


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_gather_and_fuse_bits(shape):
    """Both kernels, out of place and with every operand one float off alignment, both tapers: the restatement's bits, canaries intact."""
    R, D, n, window, stride = shape
    rng = np.random.default_rng(sum(shape))
    src = rng.standard_normal((R, D, n)).astype(np.float32)
    W = len(WO.starts(n, window, stride))
    pred = rng.standard_normal((R * W, D, window)).astype(np.float32)
    want_gather = WO.gather(src, window, stride)
    with guard(0xFF) as g:
        for offset in (False, True):
            assert _same_bits(_gather(g, src, window, stride, offset), want_gather), offset
        for taper in TAPERS:
            w = WO.weight(window, stride, taper)
            want = WO.fuse32(pred, w, n, stride)
            assert np.isfinite(want).all()
            for offset in (False, True):
                assert _same_bits(_fuse(g, pred, w, n, stride, offset), want), (taper, offset)
            # the round trip on the device: the windows of src fuse back to src, bit for bit where one window covers the frame
            back = _fuse(g, want_gather, w, n, stride)
            assert _same_bits(back, WO.fuse32(want_gather, w, n, stride))
            single = torch.tensor([len(c) == 1 for c in WO.cover(n, window, stride)], device=DEV)
            assert torch.equal(_bits(back[:, :, single]), _bits(torch.from_numpy(src).to(DEV)[:, :, single]))
            g.release()


def test_wrapper_weights_are_the_oracles_on_the_device():
    for taper in TAPERS:
        assert _same_bits(windowed.window_weight(96, 72, taper).to(DEV), WO.weight(96, 72, taper))


@pytest.mark.parametrize("shape", [(3, 6, 9, 4, 3), (2, 6, 28, 8, 8), (2, 6, 24, 8, 4)], ids=["scalar", "vec_clamped", "vec_fit"])
def test_a_nan_window_reaches_exactly_the_frames_it_covers(shape):
    R, D, n, window, stride = shape
    rng = np.random.default_rng(5)
    s = WO.starts(n, window, stride)
    W = len(s)
    w = WO.weight(window, stride)
    with guard(0xFF) as g:
        for r, j in [(0, 0), (R - 1, W - 1), (R - 1, W - 2), (0, W // 2)]:
            pred = rng.standard_normal((R * W, D, window)).astype(np.float32)
            pred[r * W + j] = np.nan
            got = _fuse(g, pred, w, n, stride).cpu().numpy()
            want = np.zeros((R, D, n), bool)
            want[r, :, s[j]:s[j] + window] = True
            assert np.array_equal(np.isnan(got), want), (r, j)
            g.release()


@pytest.mark.parametrize("shape", [(3, 6, 9, 4, 3), (2, 6, 28, 8, 8)], ids=["scalar", "vec"])
def test_negative_zero_survives_on_singly_covered_frames(shape):
    R, D, n, window, stride = shape
    W = len(WO.starts(n, window, stride))
    single = np.array([len(c) == 1 for c in WO.cover(n, window, stride)])
    assert single.any() and not single.all()
    pred = np.full((R * W, D, window), -0.0, np.float32)
    with guard(0xFF) as g:
        for taper in TAPERS:
            for offset in (False, True):
                got = _fuse(g, pred, WO.weight(window, stride, taper), n, stride, offset).cpu().numpy()
                assert (got == 0).all() and np.signbit(got[:, :, single]).all()


def test_argument_errors_leave_the_output_untouched():
    lib = _lib.load()
    R, D, n, window, stride = 2, 6, 28, 8, 8
    W = 4
    src, pred, weight = torch.randn(R, D, n, device=DEV), torch.randn(R * W, D, window, device=DEV), torch.ones(window, device=DEV)
    out_g, out_f = torch.full((R * W, D, window), 7.0, device=DEV), torch.full((R, D, n), 7.0, device=DEV)
    bad = [dict(R=0), dict(R=-1), dict(W=0), dict(D=0), dict(n=0), dict(window=0), dict(stride=0), dict(stride=-8), dict(stride=9), dict(n=7),
           dict(W=3), dict(W=5), dict(n=24), dict(window=4), dict(stride=4)]        # the last three: W is not that layout's window count
    good_g = dict(src=src.data_ptr(), out=out_g.data_ptr(), R=R, W=W, D=D, n=n, window=window, stride=stride)
    good_f = dict(pred=pred.data_ptr(), weight=weight.data_ptr(), out=out_f.data_ptr(), R=R, W=W, D=D, n=n, window=window, stride=stride)
    for fn, good, nulls in ((lib.osuf_window_gather, good_g, ("src", "out")), (lib.osuf_window_fuse, good_f, ("pred", "weight", "out"))):
        order = list(good)
        for change in bad + [{k: None} for k in nulls]:
            args = {**good, **change}
            assert fn(*[args[k] for k in order], ops._stream()) == EINVAL, change
    torch.cuda.synchronize()
    assert (out_g == 7.0).all() and (out_f == 7.0).all()
    assert lib.osuf_window_gather(*good_g.values(), ops._stream()) == 0 and lib.osuf_window_fuse(*good_f.values(), ops._stream()) == 0
    torch.cuda.synchronize()
    assert _same_bits(out_g, WO.gather(src.cpu().numpy(), window, stride))
    assert _same_bits(out_f, WO.fuse32(pred.cpu().numpy(), np.ones(window, np.float32), n, stride))


def test_kernels_are_graph_capturable():
    n, window, stride = 336, 96, 72
    src, weight = torch.randn(4, 6, n, device=DEV), windowed.window_weight(window, stride).to(DEV)
    want_g = ops.window_gather(src, window, stride)
    pred = torch.randn_like(want_g)
    want_f = ops.window_fuse(pred, weight, n, stride)
    out_g, out_f = torch.empty_like(want_g), torch.empty_like(want_f)
    torch.cuda.synchronize()
    for launch, out, want in ((lambda: ops.window_gather(src, window, stride, out=out_g), out_g, want_g),
                              (lambda: ops.window_fuse(pred, weight, n, stride, out=out_f), out_f, want_f)):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            launch()
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(out), _bits(want))


# ---- the samplers ------------------------------------------------------------------------------------------------------------------------
# B = 2, n = 336, window 96, stride 72: five windows at 0, 72, 144, 216, 240 (the last one clamped), each of the length 96 that
# tests/test_inpaint_gpu.py runs these models at.
B, N, WIN, STRIDE, STEPS, CS = 2, 336, 96, 72, 4, 2.0
BACKBONE_KW = {"dit": dict(backbone="dit", dim_h=96, depth=2, attn_heads=6, attn_dim_head=16),
               "mmdit": dict(backbone="mmdit", dim_h=64, depth=2, attn_heads=4, attn_kv_heads=2, attn_dim_head=16)}
KINDS = ["dit_ddim", "dit_flow", "ct_ddpm", "ct_ddim0", "ct_ddim_eta", "ct_2m"]
_CACHE = {}


def _model(kind):
    """A fresh model per test (a model kept alive across tests keeps its weight-pack jobs registered, see tests/test_inpaint_gpu.py)."""
    if kind == "dit_ddim":
        model = DiffusionOsuFusionDiT(sampling_timesteps=STEPS, **BACKBONE_KW["mmdit"])
    elif kind == "dit_flow":
        model = RectifiedFlowOsuFusionDiT(sampling_timesteps=STEPS, **BACKBONE_KW["dit"])
    else:
        sampler, eta = {"ct_ddpm": ("ddpm", 0.0), "ct_ddim0": ("ddim", 0.0), "ct_ddim_eta": ("ddim", 0.5), "ct_2m": ("dpmpp_2m", 0.0)}[kind]
        model = ContinuousDiffusionOsuFusionDiT(sampling_timesteps=STEPS, sampler=sampler, ddim_eta=eta, **BACKBONE_KW["mmdit"])
    model.load_state_dict({k: torch.from_numpy(param_pattern(k[len("unet."):], tuple(v.shape)).copy()) for k, v in model.state_dict().items()})
    return model.to(DEV)


def _inputs(n=N):
    if n not in _CACHE:
        x, a, c, _, noise = (torch.from_numpy(v).to(DEV) for v in synth_inputs("windowed", B, n))
        keep = torch.zeros(B, n, dtype=torch.bool, device=DEV)
        keep[0, :n // 3] = True                                          # spans that cross window borders and overlaps
        keep[1, n // 2:(5 * n) // 6] = True
        _CACHE[n] = (a, c, noise.float().contiguous(), x.float().contiguous().clamp(-1, 1), keep)
    return _CACHE[n]


def _contexts(model):
    st = contextlib.ExitStack()
    for ctx in (torch.inference_mode(), ops.reproducible_mode(True), ops.one_launch_attention(True), model._dtype_ctx()):
        st.enter_context(ctx)
    return st


def _windowed_f(model, a, c, taper="trapezoid", batch=None, counter=None):
    """f(x (b, 6, n), t (2b,), one value) -> (2b, 6, n) written out: gather, model._denoiser on the window rows (in chunks of `batch`),
    the [cond; null] halves of every chunk side by side, fuse."""
    b, n = a.shape[0], a.shape[-1]
    W = len(WO.starts(n, WIN, STRIDE))
    rows = b * W
    a_w = ops.window_gather(a, WIN, STRIDE)
    c_w = c.repeat_interleave(W, 0)
    step = rows if batch is None else batch
    chunks = [(lo, min(lo + step, rows)) for lo in range(0, rows, step)]
    inner = [model._denoiser(a_w[lo:hi], c_w[lo:hi], True) for lo, hi in chunks]
    weight = torch.from_numpy(WO.weight(WIN, STRIDE, taper)).to(DEV)

    def f(x, t):
        x_w = ops.window_gather(x, WIN, STRIDE)
        parts = []
        for (lo, hi), den in zip(chunks, inner):
            if counter is not None:
                counter.append(1)
            parts.append(den(x_w[lo:hi], t[:1].repeat(2 * (hi - lo))).view(2, hi - lo, 6, WIN))
        return ops.window_fuse(torch.cat(parts, 1).contiguous().view(2 * rows, 6, WIN), weight, n, STRIDE)
    return f


def _written_out(kind, model, a, c, x, region=None, stop_after=None, **fkw):
    """The loop of `kind` over ops calls around the written-out windowed f; region = (known, keep): the masked loop, the draws in their
    documented order."""
    b = a.shape[0]
    x = x.float().contiguous()
    blend = None
    if region is not None:
        known, mask = region[0], inpaint.as_mask(region[1], b, x.shape[-1], DEV)
        blend = lambda v, coef=None, ca=0, cs=1, z=None: ops.inpaint_blend(v, known, mask, coef, ca, cs, z)  # noqa: E731
    draw = lambda: torch.randn(x.shape, device=DEV)  # noqa: E731
    with _contexts(model):
        if kind == "dit_ddim":
            sch = model.scheduler
            sch.set_timesteps(STEPS)
            ts = sch.timesteps.tolist()
            coef = torch.tensor([[sch.step_coefficients(t)] * b for t in ts], dtype=torch.float32, device=DEV)
            f = _windowed_f(model, a, c, **fkw)
            eps = x.clone()
            if blend:
                x = blend(x, coef[0], 1, 0, eps)
            for i in range(STEPS if stop_after is None else stop_after):
                pred = f(x, torch.full((2 * b,), ts[i], dtype=torch.int64, device=DEV))
                x = ops.ddim_step(x, pred[:b], pred[b:], CS, coef[i])
                if blend:
                    x = blend(x) if i == STEPS - 1 else blend(x, coef[i], 2, 3, eps)
            return x
        if kind == "dit_flow":
            ones = torch.ones(b, dtype=torch.float32, device=DEV)
            den = _windowed_f(model, a, c, **fkw)

            def f(t, y):
                out = den(y, torch.full((2 * b,), t, dtype=torch.float32, device=DEV))
                return ops.axpby_rows(out[b:].contiguous(), out[:b].contiguous(), ones * (1.0 - CS), ones * CS)
            level = lambda t: torch.tensor([[t, 1.0 - t]] * b, dtype=torch.float32, device=DEV)  # noqa: E731
            times = torch.linspace(0.0, 1.0, STEPS).tolist()
            eps = x.clone()
            if blend:
                x = blend(x, level(times[0]), 0, 1, eps)
            for j, (t0, t1) in enumerate(zip(times[:-1], times[1:])):
                dt = t1 - t0
                mid = ops.axpby_rows(x, f(t0, x), ones, ones * (0.5 * dt))
                if blend:
                    mid = blend(mid, level(t0 + 0.5 * dt), 0, 1, eps)
                x = ops.axpby_rows(x, f(t0 + 0.5 * dt, mid), ones, ones * dt)
                if blend:
                    x = blend(x) if j == STEPS - 2 else blend(x, level(t1), 0, 1, eps)
            return x
        steps = STEPS if stop_after is None else stop_after
        if model.sampler == "ddpm":
            times = torch.linspace(1.0, 0.0, STEPS + 1, device=DEV, dtype=torch.float32)
            coef = model.scheduler.coefficients(times[:-1].repeat_interleave(b), times[1:].repeat_interleave(b)).view(STEPS, b, -1)
            log_snr = coef[:, :, 0].repeat(1, 2).contiguous()
            if blend:
                x = blend(x, coef[0], 1, 2, draw())
            f = _windowed_f(model, a, c, **fkw)
            for i in range(steps):
                pred = f(x, log_snr[i])
                x = ops.ct_step(x, pred[:b], pred[b:], CS, coef[i], draw() if i < STEPS - 1 else None)
                if blend:
                    x = blend(x) if i == STEPS - 1 else blend(x, coef[i], 4, 5, draw())
            return x
        grid = model.scheduler.solver_log_snr_grid(STEPS, model.solver_spacing, model.solver_logsnr_min, device=DEV)
        rows, fac = ops.ct_solver_schedule(grid, model.sampler, model.ddim_eta, b)
        fresh = model.sampler == "ddim" and model.ddim_eta > 0
        eps = None if fresh else x.clone()
        if blend:
            x = blend(x, rows[0], 1, 2, draw() if fresh else eps)
        f = _windowed_f(model, a, c, **fkw)
        prev = None
        for i in range(steps):
            pred = f(x, grid[i].repeat(2 * b))
            x, prev = ops.ct_solver_step(x, pred[:b], pred[b:], CS, rows[i], fac[i], prev, draw() if fresh else None, model.pred_objective, None)
            if blend:
                x = blend(x) if i == STEPS - 1 else blend(x, rows[i], 4, 5, draw() if fresh else eps)
        return x


def _sample(model, a, c, x, seed=1234, **kw):
    torch.manual_seed(seed)
    return model.sample(a, c, x, cond_scale=CS, **kw)


def _counting(model, calls):
    """model._denoiser wrapped so that every call of the closure it returns is counted."""
    orig = model._denoiser

    def counting(a_, c_, cfg):
        f = orig(a_, c_, cfg)

        def g(x_, t_):
            calls.append(x_.shape[0])
            return f(x_, t_)
        return g
    model._denoiser = counting


@pytest.mark.parametrize("kind", KINDS)
def test_windowed_sample_is_the_loop_written_out(kind):
    """Bit-equal to the written-out loop from the same seed, and again on a second call; the start iterate passed in is not written."""
    model = _model(kind)
    a, c, x, _, _ = _inputs()
    x_before = x.clone()
    got = _sample(model, a, c, x, window=WIN, window_stride=STRIDE)
    again = _sample(model, a, c, x, window=WIN, window_stride=STRIDE)
    torch.manual_seed(1234)
    want = _written_out(kind, model, a, c, x)
    assert got.shape == x.shape and got.dtype == torch.float32 and torch.isfinite(got).all()
    assert torch.equal(_bits(got), _bits(again)) and torch.equal(_bits(got), _bits(want))
    assert torch.equal(x, x_before)
    assert not torch.equal(got, _sample(model, a, c, x))               # the whole-sequence sampler computes something else
    # the stride's default, window * 3 // 4 = 72, and the taper's are this call; the other taper is another result
    assert torch.equal(_bits(got), _bits(_sample(model, a, c, x, window=WIN, window_taper="trapezoid")))
    flat = _sample(model, a, c, x, window=WIN, window_stride=STRIDE, window_taper="flat")
    torch.manual_seed(1234)
    assert not torch.equal(got, flat) and torch.equal(_bits(flat), _bits(_written_out(kind, model, a, c, x, taper="flat")))


@pytest.mark.parametrize("kind", ["ct_2m", "ct_ddpm"])
def test_window_batch_chunks_the_window_rows(kind):
    """window_batch = 4 on both sides: the ten window rows go to the backbone as chunks of 4, 4 and 2, three inner calls per step."""
    model = _model(kind)
    a, c, x, _, _ = _inputs()
    calls, written = [], []
    _counting(model, calls)
    try:
        got = _sample(model, a, c, x, window=WIN, window_stride=STRIDE, window_batch=4)
    finally:
        del model._denoiser
    torch.manual_seed(1234)
    want = _written_out(kind, model, a, c, x, batch=4, counter=written)
    assert calls == [4, 4, 2] * STEPS and len(written) == 3 * STEPS
    assert torch.isfinite(got).all() and torch.equal(_bits(got), _bits(want))
    one = []
    _counting(model, one)
    try:
        _sample(model, a, c, x, window=WIN, window_stride=STRIDE, window_batch=64)      # more than there are rows: one chunk
    finally:
        del model._denoiser
    assert one == [10] * STEPS


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [96, 80])
def test_a_sequence_that_fits_one_window_is_the_plain_sample(kind, n):
    model = _model(kind)
    a, c, x, _, _ = _inputs(n)
    plain = _sample(model, a, c, x)
    assert torch.isfinite(plain).all() and torch.equal(_bits(plain), _bits(_sample(model, a, c, x, window=WIN, window_stride=STRIDE, window_batch=1)))


@pytest.mark.parametrize("kind", KINDS)
def test_defaults_are_the_positional_call(kind):
    """sample() without the new keywords against the call through the signature it had before them."""
    model = _model(kind)
    a, c, x, _, _ = _inputs(96)
    torch.manual_seed(9)
    old = model.sample(a, c, x, CS)
    torch.manual_seed(9)
    new = model.sample(a, c, x, cond_scale=CS, known=None, known_mask=None, window=None, window_stride=None, window_taper="trapezoid",
                       window_batch=None, **({"resample": 1} if kind.startswith("ct") else {}))
    assert torch.isfinite(old).all() and torch.equal(_bits(old), _bits(new))


@pytest.mark.parametrize("kind", KINDS)
def test_masked_windowed_sample(kind):
    """known / known_mask compose with the windows: `known` bit for bit where the mask is 1, and the written-out masked, windowed loop."""
    model = _model(kind)
    a, c, x, known, keep = _inputs()
    got = _sample(model, a, c, x, known=known, known_mask=keep, window=WIN, window_stride=STRIDE)
    torch.manual_seed(1234)
    want = _written_out(kind, model, a, c, x, region=(known, keep))
    on = keep[:, None, :].expand_as(got)
    assert torch.isfinite(got).all() and torch.equal(_bits(got), _bits(want))
    assert torch.equal(_bits(got[on]), _bits(known[on])) and not torch.equal(got[~on], known[~on])
    assert not torch.equal(got, _sample(model, a, c, x, window=WIN, window_stride=STRIDE))


@pytest.mark.parametrize("kind", ["dit_ddim", "ct_2m"])
def test_windows_keep_the_denoiser_local(kind):
    """What the feature is for.  After one step, changing the audio at frames >= 240 leaves the windowed result bit-identical on frames
    < 216: those are covered only by the windows at 0, 72 and 144, which end at frame 239.  The whole-sequence sampler attends over all
    frames and changes there."""
    model = _model(kind)
    a, c, x, _, _ = _inputs()
    a2 = a.clone()
    a2[:, :, 240:] = a2[:, :, 240:].flip(-1) + 1.0
    model.stop_after = 1
    try:
        near, far = (_sample(model, v, c, x, window=WIN, window_stride=STRIDE) for v in (a, a2))
        whole_near, whole_far = (_sample(model, v, c, x) for v in (a, a2))
    finally:
        model.stop_after = None
    torch.manual_seed(1234)
    assert torch.equal(_bits(near), _bits(_written_out(kind, model, a, c, x, stop_after=1)))
    assert torch.equal(_bits(near[:, :, :216]), _bits(far[:, :, :216])) and not torch.equal(near[:, :, 216:], far[:, :, 216:])
    assert not torch.equal(whole_near[:, :, :216], whole_far[:, :, :216])
