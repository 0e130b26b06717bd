"""The ODE solvers of the flow samplers on the GPU: osuf_rk_error against an extended-precision restatement on poisoned, canary-guarded memory
(tests/memguard.py), ode.ode_loop on a rotation with a closed form against the fp64 restatement (tests/ode_oracle.py), and the solver keywords
of the flow models' samplers.

The bound on a ratio is computed per case from the inputs and the summation lengths, u = 2^-53:
  a = sum_j e_j k_j as an fma chain: |da| <= S u A, A = sum_j |e_j k_j| (each step rounds once, by at most u of a partial sum below A);
  q = (dt a) / (atol + rtol m): one rounding for the product, two for the tolerance, one for the division: dq / q <= S u A / |a| + 4 u;
  term = q^2: d term / term <= 2 S u A / |a| + 9 u;
  the sum of the (non-negative) terms: a lane adds at most 4096 / 256 = 16 of them, the wave adds over 6 shuffle levels, the workgroup over
  3 more additions, the second launch over the G chunks: every term passes through at most 16 + 6 + 3 + G additions, each rounding by u of
  a partial sum below the total: d sum / sum <= (25 + G) u;
  ratio = sqrt(sum / n): the root halves the relative error, the division and the root round once each.
The restatement is evaluated in numpy's extended precision (2^-64 where the platform has it), far below these bounds."""
import ctypes
import math

import numpy as np
import pytest
import torch

from osufusion_amd import _lib, ode, ops
from osufusion_amd.models import RectifiedFlowOsuFusionDiT
from osufusion_amd.models.rectified_flow import OsuFusion as FlowOsuFusion
from osufusion_amd.pattern import param_pattern, synth_inputs
from tests import ode_oracle as OO
from tests.memguard import guard

pytestmark = pytest.mark.gpu
DEV = "cuda"
EINVAL = -1
U = 2.0 ** -53
DT, ATOL, RTOL = 0.1, 1e-3, 1e-2
WEIGHTS = {1: [0.5], 4: ode.TABLEAUS["bosh3"].floats().e, 7: ode.TABLEAUS["dopri5"].floats().e}     # S = 7 has the zero weight (stage 1)
PERS = [1, 3, 4095, 4096, 4097, 8192 + 4]
_DATA = {}


def _bits64(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


def _data(per, B=3):
    """y0, y1 and seven stages (B, per), computed once per shape and left unchanged; the stage under dopri5's zero weight is all NaN."""
    if (per, B) not in _DATA:
        rng = np.random.default_rng(7 * per + B)
        y0, y1 = (rng.standard_normal((2, B, per)) * 2.0).astype(np.float32)
        ks = [rng.standard_normal((B, per)).astype(np.float32) for _ in range(7)]
        _DATA[(per, B)] = (y0, y1, ks)
    return _DATA[(per, B)]


def _reference(y0, y1, ks, e, dt=DT, atol=ATOL, rtol=RTOL):
    """(ratio, bound), (B,) each, the ratio in extended precision and the bound of the module docstring."""
    ld = np.longdouble
    S, n = len(e), y0.shape[1]
    G = -(-n // 4096)
    a, A = np.zeros(y0.shape, ld), np.zeros(y0.shape, np.float64)
    for w, k in zip(e, ks):
        if w != 0.0:
            a = a + ld(w) * k.astype(ld)
            A = A + np.abs(w * k.astype(np.float64))
    err = ld(dt) * a
    tol = ld(atol) + ld(rtol) * np.maximum(np.abs(y0), np.abs(y1)).astype(ld)
    with np.errstate(all="ignore"):
        term = np.where(err == 0, ld(0), (err / tol) ** 2)
        rel = np.where(err == 0, 0.0, 2 * S * U * A / np.abs(a.astype(np.float64)) + 9 * U)
    total = term.sum(axis=1)
    ratio = np.sqrt(total / ld(n))
    d_sum = (term.astype(np.float64) * rel).sum(axis=1) / np.maximum(total.astype(np.float64), 1e-300) + (25 + G) * U
    return ratio, ratio.astype(np.float64) * (0.5 * d_sum + 2 * U)


def _put(g, v, offset=False):
    """A test operand at the front of a guarded allocation, or (offset) one element into it: off 16-byte alignment."""
    t = torch.from_numpy(np.ascontiguousarray(v))
    if not offset:
        return g.place(t.to(DEV))
    buf = g.place(torch.cat([torch.zeros(1, dtype=t.dtype), t.reshape(-1)]).to(DEV))
    return buf[1:].view(t.shape)


def _raw(y0, y1, ks, e, step, ws, ratio, B, per, S=None):
    """The C entry point; tensors, integers or None for the pointers."""
    def ptr(v):
        return v.data_ptr() if isinstance(v, torch.Tensor) else v
    kp = None if ks is None else ctypes.cast((ctypes.c_void_p * 7)(*[ptr(k) for k in ks]), ctypes.c_void_p)
    ep = None if e is None else ctypes.cast((ctypes.c_double * 7)(*e), ctypes.c_void_p)
    sp = None if step is None else ctypes.cast((ctypes.c_double * 3)(*step), ctypes.c_void_p)
    return _lib.load().osuf_rk_error(ptr(y0), ptr(y1), kp, ep, len(e) if S is None else S, sp, ptr(ws), ptr(ratio), B, per, ops._stream())


def _run(g, y0, y1, ks, e, offset=False, dt=DT, atol=ATOL, rtol=RTOL):
    """ops.rk_error on guarded operands (ks entries may be None) -> (B,) fp64 numpy; offset: every operand and the output one element into its
    buffer, through the C entry point."""
    d0, d1 = _put(g, y0, offset), _put(g, y1, offset)
    dk = [None if k is None else _put(g, k, offset) for k in ks]
    if not offset:
        ratio = ops.rk_error(d0, d1, dk, e, dt, atol, rtol)
    else:
        B, per = y0.shape
        rbuf = torch.empty(B + 1, dtype=torch.float64, device=DEV)
        ws = torch.empty(_lib.load().osuf_rk_error_workspace_bytes(B, per) // 8, dtype=torch.float64, device=DEV)
        ratio = rbuf[1:]
        assert _raw(d0, d1, dk, e, (dt, atol, rtol), ws, ratio, B, per) == 0
        g.check()
        assert torch.isnan(rbuf[0]).item()                                        # the double in front keeps its poison
    g.check()
    assert ratio.dtype == torch.float64 and tuple(ratio.shape) == (y0.shape[0],)
    return ratio.cpu().numpy()


# ---- the kernel pair --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [False, True], ids=["aligned", "offset"])
@pytest.mark.parametrize("S", [1, 4, 7])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("per", PERS)
def test_rk_error_against_extended_precision(per, B, S, offset):
    y0, y1, ks = _data(per, B)
    e = WEIGHTS[S]
    want, bound = _reference(y0, y1, ks[:S], e)
    assert np.isfinite(want.astype(np.float64)).all() and (want > 0).all()
    with guard(0xFF) as g:
        got = _run(g, y0, y1, ks[:S], e, offset)
    err = np.abs((got.astype(np.longdouble) - want).astype(np.float64))
    print(f"rk_error per={per} B={B} S={S} {'offset' if offset else 'aligned'}: ratio {got.tolist()} worst error / bound = {(err / bound).max():.3f}")
    assert (err <= bound).all()


@pytest.mark.parametrize("per", [3, 8196])
def test_a_zero_weight_skips_its_stage(per):
    """dopri5's stage 1: NaN-filled and NULL give the bits of the six-stage call."""
    y0, y1, ks = _data(per)
    e = WEIGHTS[7]
    assert e[1] == 0.0
    nan = np.full_like(ks[1], np.nan)
    with guard(0xFF) as g:
        want = _run(g, y0, y1, ks[:1] + ks[2:], e[:1] + e[2:])
        for offset in (False, True):
            if not offset:
                assert np.array_equal(_bits64(_run(g, y0, y1, [ks[0], nan] + ks[2:], e)), _bits64(want))
                assert np.array_equal(_bits64(_run(g, y0, y1, [ks[0], None] + ks[2:], e)), _bits64(want))
            else:
                got = _run(g, y0, y1, [ks[0], None] + ks[2:], e, offset=True)
                assert np.isfinite(got).all() and np.allclose(got, want, rtol=1e-12)
        assert (_run(g, y0, y1, [None, None], [0.0, -0.0]) == 0.0).all()          # no stage at all: no error


def test_no_error_and_no_tolerance_is_zero():
    """atol = 0 and both states 0: tol == 0.  Where the error is 0 too the term is 0 by a select; one element with an error gives inf."""
    B, per = 3, 4100
    zero = np.zeros((B, per), np.float32)
    k = zero.copy()
    k[1, 4097] = 1.0
    with guard(0xFF) as g:
        for offset in (False, True):
            got = _run(g, zero, zero, [k], [0.5], offset, atol=0.0, rtol=1e-3)
            assert got[0] == 0.0 and got[2] == 0.0 and np.isinf(got[1])
            assert (_run(g, zero, zero, [zero], [0.5], offset, atol=0.0, rtol=1e-3) == 0.0).all()


def _clean(per):
    y0, y1, ks = _data(per)
    with guard(0xFF) as g:
        return _run(g, y0, y1, ks, WEIGHTS[7])


@pytest.mark.parametrize("where", ["stage", "y0", "y1"])
@pytest.mark.parametrize("bad", [np.nan, np.inf], ids=["nan", "inf"])
@pytest.mark.parametrize("per", [3, 8196])
def test_a_non_finite_value_stays_in_its_sample(per, bad, where):
    y0, y1, ks = _data(per)
    y0, y1, ks = y0.copy(), y1.copy(), [k.copy() for k in ks]
    {"stage": ks[4], "y0": y0, "y1": y1}[where][1, per - 2] = bad
    with guard(0xFF) as g:
        got = _run(g, y0, y1, ks, WEIGHTS[7])
    clean = _clean(per)
    assert np.array_equal(_bits64(got[[0, 2]]), _bits64(clean[[0, 2]]))
    if where == "stage" or math.isnan(bad):
        assert not np.isfinite(got[1])                                             # an infinite state makes an infinite tolerance: a finite ratio
    else:
        assert np.isfinite(got[1]) and got[1] <= clean[1]


def test_a_nan_state_under_a_zero_error_is_absorbed():
    """The select on err == 0 comes first, as the header states it: a NaN state at an element whose error is exactly 0 contributes 0, the
    same NaN at an element with an error makes the sample's ratio NaN."""
    per = 8196
    y0, y1, ks = _data(per)
    y0, ks = y0.copy(), [k.copy() for k in ks]
    for k in ks:
        k[1, 4100] = 0.0                                     # the element's error is exactly 0
    with guard(0xFF) as g:
        for offset in (False, True):
            base = _run(g, y0, y1, ks, WEIGHTS[7], offset)
            y0[1, 4100] = np.nan
            assert np.array_equal(_bits64(_run(g, y0, y1, ks, WEIGHTS[7], offset)), _bits64(base))
            y0[1, 4100], y0[1, 4101] = 1.0, np.nan
            got = _run(g, y0, y1, ks, WEIGHTS[7], offset)
            assert np.isnan(got[1]) and np.array_equal(_bits64(got[[0, 2]]), _bits64(base[[0, 2]]))
            y0[1, 4101] = 1.0


@pytest.mark.parametrize("per", [3, 4097, 8196])
def test_a_sample_does_not_depend_on_its_batch_and_runs_repeat(per):
    y0, y1, ks = _data(per)
    three = _clean(per)
    assert np.array_equal(_bits64(_clean(per)), _bits64(three))                    # two runs: the same bits
    with guard(0xFF) as g:
        for b in range(3):
            alone = _run(g, y0[b:b + 1], y1[b:b + 1], [k[b:b + 1] for k in ks], WEIGHTS[7])
            assert np.array_equal(_bits64(alone), _bits64(three[b:b + 1]))


def test_argument_errors_leave_the_ratio_poisoned():
    lib = _lib.load()
    B, per = 3, 54
    y0, y1, ks = _data(per)
    e = WEIGHTS[4]
    nan, inf = math.nan, math.inf
    with guard(0xFF) as g:
        d0, d1, dk = _put(g, y0), _put(g, y1), [_put(g, k) for k in ks[:4]]
        ratio = torch.empty(B, dtype=torch.float64, device=DEV)
        ws = torch.empty(lib.osuf_rk_error_workspace_bytes(B, per) // 8, dtype=torch.float64, device=DEV)
        good = dict(y0=d0, y1=d1, ks=dk, e=e, step=(DT, ATOL, RTOL), ws=ws, ratio=ratio, B=B, per=per, S=4)
        bad = [dict(y0=None), dict(y1=None), dict(ks=None), dict(e=None), dict(step=None), dict(ws=None), dict(ratio=None),
               dict(ks=[dk[0], None, dk[2], dk[3]]), dict(S=0), dict(S=8), dict(S=-1), dict(B=0), dict(B=-1), dict(per=0), dict(per=-54),
               dict(e=[e[0], nan, e[2], e[3]]), dict(step=(nan, ATOL, RTOL)), dict(step=(inf, ATOL, RTOL)), dict(step=(DT, nan, RTOL)),
               dict(step=(DT, inf, RTOL)), dict(step=(DT, ATOL, nan)), dict(step=(DT, ATOL, inf)), dict(step=(DT, -ATOL, RTOL)),
               dict(step=(DT, ATOL, -RTOL)), dict(step=(DT, 0.0, 0.0)), dict(ws=ws.data_ptr() + 4)]
        for change in bad:
            assert _raw(**{**good, **change}) == EINVAL, change
        g.check()
        assert bool((ratio.view(torch.uint8) == 0xFF).all())
        assert _raw(**{**good, "ks": [dk[0], None, dk[2], dk[3]], "e": [e[0], 0.0, e[2], e[3]]}) == 0       # NULL under a zero weight is fine
        assert _raw(**good) == 0
        g.check()
        want, bound = _reference(y0, y1, ks[:4], e)
        assert (np.abs(ratio.cpu().numpy() - want.astype(np.float64)) <= bound).all()


def test_the_two_launches_are_graph_capturable():
    y0, y1, ks = _data(8196)
    d0, d1 = (torch.from_numpy(v).to(DEV) for v in (y0, y1))
    dk = [torch.from_numpy(k).to(DEV) for k in ks]
    want = ops.rk_error(d0, d1, dk, WEIGHTS[7], DT, ATOL, RTOL)
    ratio = torch.empty(3, dtype=torch.float64, device=DEV)
    ws = torch.empty(_lib.load().osuf_rk_error_workspace_bytes(3, 8196) // 8, dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert _raw(d0, d1, dk, WEIGHTS[7], (DT, ATOL, RTOL), ws, ratio, 3, 8196) == 0
    ratio.zero_(), ws.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(ratio.view(torch.int64), want.view(torch.int64))


# ---- ode_loop on a rotation ---------------------------------------------------------------------------------------------------------------------
# y' = omega J y on the channel pairs, f in torch fp32.  The inputs were fixed on a CPU-only run of both sides (the device calls replaced by
# torch, as tests/test_ode_cpu.py does): the restatement's distance to the closed form is 1e-3 .. 6e-2 for the adaptive cases and 1e-3 .. 1 for the
# fixed grids, against fp32 deviations of 1e-6, and no ratio of the restatement's run lies within 5 % of 1 (the closest: 0.73 and 0.64).
#
# The state bound.  Per evaluation the device rounds twice: omega * y in fp32 (2^-24 of |k| <= omega Y) and the stage state or the solution,
# one rounding of ops.lincomb's fp64 chain (2^-24 Y).  A rounding made in a stage reaches the step's end through at most two more
# applications of h omega: a factor (1 + h omega)^2.  The propagator of these methods on a rotation has norm |R(i h omega)|, which is what
# carries Y_0 to the final Y, so with Y = max(|y_0|, |y_end|) taken from the restatement the roundings of earlier steps are not amplified
# beyond those of Y itself.  Hence |device - restatement| <= steps * stages * 2^-24 * Y * (1 + h omega)^2.
#
# The step times.  They are fp64 host decisions, but functions of the device's ratios, which differ from the restatement's with the fp32
# states, so they are compared in three parts.  (1) The decisions, the counts and the final time 1.0 equal the restatement's exactly; no
# ratio of the restatement's lies within 5 % of 1 (asserted first), and every device ratio is required to lie within 5 % of the restatement's,
# so no decision is left to rounding.  (2) The controller replayed on the host over the ratios the device returned gives the loop's times
# bit for bit: the times are host arithmetic and nothing else.  (3) A ratio r enters the next step size as r^(-1 / order), so a relative
# difference rho_i between the two sides' ratios moves every later step size by rho_i / order to first order; the step sizes add up to
# t_end - t_0 = 1, so the two sides' times differ by at most the sum of rho_i / order, doubled here for the higher-order terms.
FIXED = {"euler": (2.0, 5), "midpoint": (2.0, 5), "rk4": (2.0, 5)}
ADAPTIVE = {"bosh3": (6.0, 5, 1e-3), "dopri5": (10.0, 3, 1e-4)}
SHAPE = (2, 6, 700)                                            # 4200 values per sample: two chunks, the four-wide path


def _rotation_start():
    y0 = np.random.default_rng(11).standard_normal(SHAPE).astype(np.float32)
    y0[1] *= 0.25                                            # the two samples' ratios differ: the batch ratio is sample 0's
    return y0


def _f32(omega):
    def f(t, y):
        k = torch.empty_like(y)
        k[:, 0::2] = -omega * y[:, 1::2]
        k[:, 1::2] = omega * y[:, 0::2]
        return k
    return f


def _state_bound(steps, stages, h, omega, y0, y_end):
    return steps * stages * 2.0 ** -24 * max(np.abs(y0).max(), np.abs(y_end).max()) * (1.0 + h * omega) ** 2


@pytest.mark.parametrize("method", list(FIXED))
def test_fixed_grid_methods_against_the_restatement(method):
    omega, S = FIXED[method]
    y0, times = _rotation_start(), OO.linspace(S)
    want, ws = OO.solve(OO.rotation_f(omega), y0, times, method)
    stages = ode.TABLEAUS[method].stages
    bound = _state_bound(S - 1, stages, 1.0 / (S - 1), omega, y0, want)
    truncation = np.abs(want - OO.rotation_exact(y0, omega, 1.0)).max()
    assert truncation > 10 * bound                           # the method's own error sits well above fp32 rounding
    with guard(0xFF) as g:
        got, gs = ode.ode_loop(_f32(omega), g.place(torch.from_numpy(y0).to(DEV)), times, torch.ones(2, device=DEV), method=method)
        g.check()
    err = np.abs(got.cpu().numpy() - want).max()
    print(f"{method}: |device - restatement| = {err:.3e}, bound {bound:.3e}, truncation {truncation:.3e}")
    assert gs["evals"] == ws["evals"] == stages * (S - 1) and gs["accepted"] == S - 1 and gs["rejected"] == 0 and gs["times"] == times[1:]
    assert err <= bound


@pytest.mark.parametrize("method", list(ADAPTIVE))
def test_adaptive_methods_against_the_restatement(method, monkeypatch):
    omega, S, tol = ADAPTIVE[method]
    tab = ode.TABLEAUS[method]
    y0, times = _rotation_start(), OO.linspace(S)
    want, ws = OO.solve(OO.rotation_f(omega), y0, times, method, rtol=tol, atol=tol)
    assert all(abs(r - 1.0) > 0.05 for r in ws["ratios"])     # no decision of the restatement's run is close: a flipped one is a bug, not noise
    assert ws["rejected"] >= 1 and ws["accepted"] >= 5
    attempts = len(ws["decisions"])
    h = max(b - a for a, b in zip([0.0] + ws["times"][:-1], ws["times"]))
    bound = _state_bound(attempts, tab.stages, h, omega, y0, want)
    truncation = np.abs(want - OO.rotation_exact(y0, omega, 1.0)).max()
    assert truncation > 10 * bound
    seen, kernel = [], ode.rk_error

    def recording(*args):
        seen.append(kernel(*args))
        return seen[-1]
    monkeypatch.setattr(ode, "rk_error", recording)
    with guard(0xFF) as g:
        got, gs = ode.ode_loop(_f32(omega), g.place(torch.from_numpy(y0).to(DEV)), times, None, method=method, rtol=tol, atol=tol)
        g.check()
    err = np.abs(got.cpu().numpy() - want).max()
    ratios = [ode.batch_ratio(r.tolist()) for r in seen]
    rho = [abs(a - b) / b for a, b in zip(ratios, ws["ratios"])]
    replayed, t, dt = [], 0.0, times[1] - times[0]
    for r in ratios:
        t_new, h_used = ode.clip_step(t, dt, 1.0)
        accepted, factor = ode.step_factor(r, tab.order)
        if accepted:
            t = t_new
            replayed.append(t)
        dt = h_used * factor
    t_bound = 2.0 * sum(rho) / tab.order
    t_err = max(abs(a - b) for a, b in zip(gs["times"], ws["times"])) if len(gs["times"]) == len(ws["times"]) else math.inf
    print(f"{method}: decisions {''.join('A' if d else 'R' for d in ws['decisions'])}, |device - restatement| = {err:.3e}, bound {bound:.3e}, "
          f"truncation {truncation:.3e}; largest relative ratio difference {max(rho):.3e}; step times differ by {t_err:.3e}, bound {t_bound:.3e}")
    assert gs["evals"] == ws["evals"] == 1 + (tab.stages - 1) * attempts and len(ratios) == attempts
    assert (gs["accepted"], gs["rejected"]) == (ws["accepted"], ws["rejected"]) and len(gs["times"]) == len(ws["times"])
    assert gs["times"][-1] == 1.0 == ws["times"][-1]
    assert [ode.step_factor(r, tab.order)[0] for r in ratios] == ws["decisions"]                   # the accept / reject sequence itself
    assert max(rho) < 0.05
    assert gs["times"] == replayed
    assert t_err <= t_bound
    assert err <= bound


# ---- the models -------------------------------------------------------------------------------------------------------------------------------
B, N, STEPS, CS = 2, 96, 4, 2.0
LONG, WIN, STRIDE = 336, 96, 72
BACKBONE_KW = {"dit": dict(backbone="dit", dim_h=96, depth=2, attn_heads=6, attn_dim_head=16),
               "mmdit": dict(backbone="mmdit", dim_h=64, depth=2, attn_heads=4, attn_kv_heads=2, attn_dim_head=16)}
UNET_KW = dict(dim_h_mult=(1, 2), num_layer_blocks=(1, 1), num_middle_transformers=1, cross_embed_kernel_sizes=(3,), attn_dim_head=64, attn_heads=2,
               attn_kv_heads=1, attn_context_len=256)
_INPUTS = {}


def _patterned(model):
    """A fresh model per test (a model kept alive across tests keeps its weight-pack jobs registered, see tests/test_inpaint_gpu.py)."""
    model.load_state_dict({k: torch.from_numpy(param_pattern(k[len("unet."):], tuple(v.shape)).copy()) for k, v in model.state_dict().items()})
    return model.to(DEV)


def _flow(backbone):
    return _patterned(RectifiedFlowOsuFusionDiT(sampling_timesteps=STEPS, **BACKBONE_KW[backbone]))


def _inputs(n=N):
    if n not in _INPUTS:
        x, a, c, _, noise = (torch.from_numpy(v).to(DEV) for v in synth_inputs("ode", B, n))
        keep = torch.zeros(B, n, dtype=torch.bool, device=DEV)
        keep[0, :n // 3] = True
        keep[1, n // 2:(5 * n) // 6] = True
        _INPUTS[n] = (a, c, noise.float().contiguous(), x.float().contiguous().clamp(-1, 1), keep)
    return _INPUTS[n]


def _same(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("backbone", ["dit", "mmdit"])
def test_flow_sampler_methods(backbone):
    model = _flow(backbone)
    a, c, noise, _, _ = _inputs()
    base = model.sample(a, c, noise.clone(), cond_scale=CS)
    assert model.last_ode_stats["evals"] == 2 * (STEPS - 1) and model.last_ode_stats["method"] == "midpoint"
    assert _same(model.sample(a, c, noise.clone(), cond_scale=CS, method="midpoint"), base)
    for method, evals in (("euler", STEPS - 1), ("rk4", 4 * (STEPS - 1))):
        out = model.sample(a, c, noise.clone(), cond_scale=CS, method=method)
        st = model.last_ode_stats
        assert torch.isfinite(out).all() and not _same(out, base)
        assert st["evals"] == evals and st["accepted"] == STEPS - 1 and st["rejected"] == 0 and st["times"][-1] == 1.0
    outs = []
    for _ in range(2):
        outs.append(model.sample(a, c, noise.clone(), cond_scale=CS, method="dopri5", rtol=5e-2, atol=5e-2))
        st = model.last_ode_stats
        print(f"{backbone} dopri5 at 5e-2: {st['evals']} evaluations, {st['accepted']} accepted, {st['rejected']} rejected")
        assert st["evals"] == 1 + 6 * (st["accepted"] + st["rejected"]) and st["times"][-1] == 1.0 and len(st["times"]) == st["accepted"]
    assert torch.isfinite(outs[0]).all() and _same(outs[0], outs[1])
    with pytest.raises(ValueError):
        model.sample(a, c, noise.clone(), cond_scale=CS, method="heun")
    with pytest.raises(RuntimeError, match="max_steps"):
        model.sample(a, c, noise.clone(), cond_scale=CS, method="dopri5", rtol=0.0, atol=1e-30, max_steps=2)


def _written_out_rk4(f, x, times, ones, **_):
    """The 3/8 rule written out from its formula over torch fp64 combines (no tableau, no ops.lincomb), in ode_loop's place."""
    def comb(y, *terms):
        out = y.double()
        for w, k in terms:
            out = out + w * k.double()
        return out.float()
    y, third = x, 1.0 / 3.0
    for t0, t1 in zip(times[:-1], times[1:]):
        h = t1 - t0
        k1 = f(t0, y)
        k2 = f(t0 + third * h, comb(y, (h * third, k1)))
        k3 = f(t0 + 2.0 * third * h, comb(y, (-h * third, k1), (h, k2)))
        k4 = f(t0 + h, comb(y, (h, k1), (-h, k2), (h, k3)))
        y = comb(y, (h * 0.125, k1), (h * 0.375, k2), (h * 0.375, k3), (h * 0.125, k4))
    return y, {"evals": 4 * (len(times) - 1)}


@pytest.mark.parametrize("backbone", ["dit", "mmdit"])
def test_rk4_values_against_the_rule_written_out(backbone, monkeypatch):
    """sample(method="rk4") against the same sampler with its loop replaced by the rule written out over the same flow function.  The two
    differ only in how a combine is rounded -- one fp64 fma chain against fp64 adds, either rounded to fp32 once: the same bits but for
    rare ties, each one fp32 spacing of the state.  The bound allows every one of the 4 (S - 1) combines such a tie at the largest value,
    2^-23 of it each.  A wrong stage, weight or time, or a stage overwritten while it is still needed, is another method: even the
    nearest correct one, the midpoint rule on the same grid, must lie ten bounds away for the comparison to mean anything, which is
    asserted; the figures are printed."""
    model = _flow(backbone)
    a, c, noise, _, _ = _inputs()
    got = model.sample(a, c, noise.clone(), cond_scale=CS, method="rk4")
    mid = model.sample(a, c, noise.clone(), cond_scale=CS)
    monkeypatch.setattr(ode, "ode_loop", _written_out_rk4)
    want = model.sample(a, c, noise.clone(), cond_scale=CS, method="rk4")
    assert model.last_ode_stats == {"evals": 4 * (STEPS - 1)}                      # the written-out loop ran
    diff, scale = (got - want).abs().max().item(), want.abs().max().item()
    print(f"{backbone} rk4: |kernel loop - written out| = {diff:.3e} of {scale:.3e}; |rk4 - midpoint| = {(want - mid).abs().max().item():.3e}")
    bound = 4 * (STEPS - 1) * 2.0 ** -23 * scale
    assert (want - mid).abs().max().item() > 10 * bound
    assert diff <= bound


def test_known_region_with_a_fixed_grid_and_not_with_an_adaptive_method():
    model = _flow("dit")
    a, c, noise, known, keep = _inputs()
    out = model.sample(a, c, noise.clone(), cond_scale=CS, known=known, known_mask=keep, method="rk4")
    m = keep[:, None, :].expand_as(out)
    assert model.last_ode_stats["evals"] == 4 * (STEPS - 1) and torch.isfinite(out).all()
    assert _same(out[m], known[m]) and not _same(out[~m], known[~m])
    for method in ("bosh3", "dopri5"):
        with pytest.raises(ValueError, match="known"):
            model.sample(a, c, noise.clone(), cond_scale=CS, known=known, known_mask=keep, method=method)


def test_windows_and_guidance_controls_under_bosh3():
    model = _flow("mmdit")
    a, c, noise, _, _ = _inputs(LONG)
    kw = dict(cond_scale=CS, method="bosh3", rtol=5e-2, atol=5e-2)
    for extra in (dict(window=WIN, window_stride=STRIDE), dict(guidance_rescale=0.7, guidance_interval=(-2.0, 2.0)),
                  dict(window=WIN, window_stride=STRIDE, guidance_rescale=0.7)):
        out = model.sample(a, c, noise.clone(), **kw, **extra)
        st = model.last_ode_stats
        assert torch.isfinite(out).all() and st["evals"] == 1 + 3 * (st["accepted"] + st["rejected"]) and st["times"][-1] == 1.0


def test_unet_flow_model_sample_masked_with_rk4():
    model = _patterned(FlowOsuFusion(32, sampling_timesteps=STEPS, **UNET_KW))
    a, c, noise, known, keep = _inputs()
    base = model.sample(a, c, noise.clone(), cond_scale=CS)
    assert model.last_ode_stats["evals"] == 2 * (STEPS - 1)
    assert _same(model.sample_masked(a, c, noise.clone(), cond_scale=CS, method="midpoint"), base)
    out = model.sample_masked(a, c, noise.clone(), cond_scale=CS, method="rk4")
    assert torch.isfinite(out).all() and model.last_ode_stats["evals"] == 4 * (STEPS - 1) and not _same(out, base)
    out = model.sample_masked(a, c, noise.clone(), cond_scale=CS, known=known, known_mask=keep, method="rk4")
    m = keep[:, None, :].expand_as(out)
    assert _same(out[m], known[m])
    with pytest.raises(ValueError, match="known"):
        model.sample_masked(a, c, noise.clone(), cond_scale=CS, known=known, known_mask=keep, method="dopri5")
