"""The v / x_start objectives, dynamic thresholding and min-SNR-gamma weighting on the GPU: osuf_ct_x0_quantile (exact select against a CPU
sort; the fused start prediction against the fp64 restatement), osuf_ct_step_ex, osuf_ct_qsample, osuf_mse_w, and
ContinuousDiffusionOsuFusionDiT with the new keywords (defaults against the code path as it was, v + min-SNR loss, thresholded sampler).
The yardstick is tests/ct_objectives_oracle.py.  Outputs are allocated poisoned and canary-guarded (tests/memguard.py).  Measured
distances: profiles/ct_objectives.md."""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

from osufusion_amd import ct, forced_compute_dtype, ops
from osufusion_amd.models import ContinuousDiffusionOsuFusionDiT
from osufusion_amd.models.diffusion import _MSEFn
from osufusion_amd.pattern import param_pattern, synth_inputs
from tests import ct_objectives_oracle as CO
from tests.memguard import guard

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD_DIR = Path(__file__).resolve().parent / "golden"
META = {**json.loads((GOLD_DIR / "mmdit_cases.json").read_text()), **json.loads((GOLD_DIR / "dit_cases.json").read_text())}
NAMES = ["mmdit_h96", "dit_h96"]                       # the smallest fixtures: B = 2, L = 203
OBJECTIVES = ("noise", "x_start", "v")
QS = (0.5, 0.95, 0.999, 1.0)
STEP_TIMES = ([0.5, 0.625, 0.125], [0.375, 0.5, 0.0])  # three (t, t_next); the last sample's t_next is 0: gain 0


def _row(B, t=STEP_TIMES[0], t_next=STEP_TIMES[1]):
    reps = -(-B // len(t))
    return ops.ct_schedule(torch.tensor((list(t) * reps)[:B], device=DEV), torch.tensor((list(t_next) * reps)[:B], device=DEV), ct.KINDS["cosine"])


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- osuf_ct_x0_quantile: the select is exact ------------------------------------------------------------------------------------------
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 6 * 40, 6 * 1000, 6 * 8192)
KINDS = ("gaussian", "all_equal", "two_values", "zeros_and_subnormals", "low_mantissa_byte", "exponent_byte")


def select_data(kind, B, n, seed):
    """(B, n) fp32 with random signs.  Each kind exercises one part of the digit walk: a tie run that holds the rank, keys that part only
    in the last digit (low mantissa byte) or only in the first (exponent byte), and the keys at the bottom of the order (+-0, subnormals)."""
    g = torch.Generator().manual_seed(seed)
    if kind == "gaussian":
        v = torch.randn((B, n), generator=g)
    elif kind == "all_equal":
        v = torch.full((B, n), 0.37)
    elif kind == "two_values":                              # about 2/3 of the values are the larger: the ranks of q >= 0.5 lie in its run
        v = torch.where(torch.rand((B, n), generator=g) < 1 / 3, torch.tensor(0.75), torch.tensor(1.5))
    elif kind == "zeros_and_subnormals":                    # keys 0 .. 1023 (zero and subnormals), a few normal values on top
        bits = torch.randint(0, 1024, (B, n), generator=g, dtype=torch.int32)
        bits = torch.where(torch.rand((B, n), generator=g) < 0.25, torch.zeros_like(bits), bits)
        bits = torch.where(torch.rand((B, n), generator=g) < 0.1, torch.randint(0x00800000, 0x40000000, (B, n), generator=g, dtype=torch.int32), bits)
        v = bits.view(torch.float32)
    elif kind == "low_mantissa_byte":
        v = (0x3F9D7A00 + torch.randint(0, 256, (B, n), generator=g, dtype=torch.int32)).view(torch.float32)
    elif kind == "exponent_byte":
        v = ((torch.randint(1, 255, (B, n), generator=g, dtype=torch.int32) << 23) | 0x2AAAAB).view(torch.float32)
    else:
        raise ValueError(kind)
    sign = torch.where(torch.rand((B, n), generator=g) < 0.5, torch.tensor(-2 ** 31, dtype=torch.int32), torch.tensor(0, dtype=torch.int32))
    return (v.contiguous().view(torch.int32) ^ sign).view(torch.float32)      # the sign bit alone (-0.0 included), no arithmetic


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_quantile_order_statistics_equal_a_cpu_sort_bit_for_bit(n, kind):
    """Objective x_start, no guidance, cond = the data: x0 is the data, untouched.  out[:, 0:2] against torch.sort(|data|) on the CPU as bit
    patterns, s against the same fp32 expression on those two values, and a second run against the first."""
    for B in (1, 3):
        data = select_data(kind, B, n, seed=1000 * n + B)
        ref = torch.sort(data.abs(), dim=1).values
        assert torch.equal(_bits(ref), torch.sort(_bits(data) & 0x7FFFFFFF, dim=1).values)      # the host sorted subnormals as values too
        if kind == "two_values" and n >= 63:
            assert (ref[:, int(0.95 * (n - 1))] == ref[:, int(0.95 * (n - 1)) - 1]).all()       # the rank lies inside a tie run
        d = data.to(DEV)
        row = _row(B)
        for q in QS:
            k_lo, frac = ct.quantile_rank(q, n)
            k_hi = min(k_lo + 1, n - 1)
            got = ops.ct_x0_quantile(d, d, None, 1.0, row, "x_start", q)
            again = ops.ct_x0_quantile(d, d, None, 1.0, row, "x_start", q)
            assert got.shape == (B, 3) and got.dtype == torch.float32
            assert torch.equal(_bits(got), _bits(again))
            got = got.cpu()
            lo, hi = ref[:, k_lo], ref[:, k_hi]
            assert torch.equal(_bits(got[:, 0]), _bits(lo)), (B, q, got[:, 0], lo)
            assert torch.equal(_bits(got[:, 1]), _bits(hi)), (B, q, got[:, 1], hi)
            s = torch.clamp(lo + (hi - lo) * torch.tensor(frac, dtype=torch.float32), min=1.0)
            assert torch.equal(_bits(got[:, 2]), _bits(s)), (B, q, got[:, 2], s)


# ---- osuf_ct_x0_quantile: the fused start prediction --------------------------------------------------------------------------------
def step_inputs(B, per_sample, seed=5):
    """N(0, 1) iterates and predictions; the null prediction lies near the conditional one, so that guidance 7 keeps p at N(0, 1)'s scale."""
    g = torch.Generator().manual_seed(seed)
    x, cond, noise = (torch.randn((B, per_sample), generator=g) for _ in range(3))
    null = cond + 0.05 * torch.randn((B, per_sample), generator=g)
    return x, cond, null, noise


def composed_threshold(x, cond, null, cond_scale, row, objective, q):
    """The torch composition on the device, fp32: guidance, x0, |.|, torch.quantile, clamp(min=1)."""
    p = cond if null is None else null + (cond - null) * cond_scale
    k = [row[:, j].reshape(-1, 1) for j in range(13)]
    x0 = {"noise": lambda: (x - k[2] * p) * k[9], "x_start": lambda: p, "v": lambda: k[1] * x - k[2] * p}[objective]()
    return torch.quantile(x0.abs(), q, dim=1).clamp(min=1.0), x0


@pytest.mark.parametrize("cond_scale", [None, 2.0, 7.0], ids=["cond", "cfg2", "cfg7"])
@pytest.mark.parametrize("objective", OBJECTIVES)
@pytest.mark.parametrize("n", [6 * 40, 6 * 1000 + 2], ids=["n240", "n6002"])
def test_quantile_of_the_fused_start_prediction_against_fp64(n, objective, cond_scale):
    """s against the fp64 restatement.  The bound is 4 x the distance of the fp32 torch composition (guidance, x0, torch.quantile) from the
    same restatement on the same inputs, the largest over the case's 8 samples: the margin profiles/dit_sampling.md uses.  n = 6002 is two
    workgroups per sample on the scalar path (no multiple of 4), n = 240 one on the vector path.
    Measured (MI355X, profiles/ct_objectives.md): kernel within 4.8e-8 .. 3.7e-7 of the restatement over the 18 cases, the torch composition
    within 2.0e-7 .. 2.8e-6; the largest kernel / bound ratio is 0.17."""
    B, q = 8, 0.95
    x, cond, null, _ = step_inputs(B, n, seed=n)
    null = null if cond_scale is not None else None
    scale = cond_scale if cond_scale is not None else 1.0
    with guard(0xFF) as g:
        row = _row(B)
        xd, cd = g.place(x.to(DEV)), g.place(cond.to(DEV))
        nd = g.place(null.to(DEV)) if null is not None else None
        got = ops.ct_x0_quantile(xd, cd, nd, scale, row, objective, q)
        g.check()
        got, row_c = got.cpu(), row.cpu()
        g.release()
    torch_s, _ = composed_threshold(x.to(DEV), cond.to(DEV), null.to(DEV) if null is not None else None, scale, row, objective, q)
    lo, hi, want = CO.threshold(CO.start_from(x, CO.guided(cond, null, scale), row_c, objective), q)
    d_torch = np.abs(torch_s.double().cpu().numpy() - want).max()
    d_kernel = np.abs(got[:, 2].double().numpy() - want).max()
    print(f"ct_objectives fused_x0/n{n}/{objective}/cfg{cond_scale}: kernel |s - fp64| = {d_kernel:.3e}  torch composition = {d_torch:.3e}  "
          f"s = {want.min():.3f} .. {want.max():.3f}")
    assert torch.isfinite(got).all() and (want > 1.0).all()                                  # the threshold is live in every sample
    assert d_kernel <= 4 * d_torch, (d_kernel, d_torch)
    assert (got[:, 0] <= got[:, 1]).all()


# ---- osuf_ct_step_ex -----------------------------------------------------------------------------------------------------------------
def _misaligned(t):
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    buf[1:].copy_(t.flatten())
    return buf[1:].view(t.shape)


@pytest.mark.parametrize("misalign", [False, True], ids=["vec", "scalar"])
def test_step_ex_is_ct_step_for_noise_without_a_threshold_and_with_ones(misalign):
    x, cond, null, noise = step_inputs(3, 222)
    put = (lambda v: _misaligned(v.to(DEV))) if misalign else (lambda v: v.to(DEV))
    xd, cd, nd, zd = put(x), put(cond), put(null), put(noise)
    row = _row(3)
    ones = torch.ones(3, device=DEV)
    strided = torch.ones((3, 3), device=DEV)[:, 2]                                           # as a column of the quantile's rows
    for nu, scale in ((None, 1.0), (nd, 7.0)):
        for z in (None, zd):
            want = ops.ct_step(xd, cd, nu, scale, row, z)
            assert torch.equal(ops.ct_step_ex(xd, cd, nu, scale, row, z, "noise", None), want)
            assert torch.equal(ops.ct_step_ex(xd, cd, nu, scale, row, z, "noise", ones), want)
            assert torch.equal(ops.ct_step_ex(xd, cd, nu, scale, row, z, 0, strided), want)


@pytest.mark.parametrize("with_noise", [False, True], ids=["mean", "noise"])
@pytest.mark.parametrize("thresholded", [False, True], ids=["clamp", "threshold"])
@pytest.mark.parametrize("with_null", [False, True], ids=["cond", "guided"])
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_step_ex_against_fp64_of_its_formula(objective, with_null, thresholded, with_noise):
    """The bound tests/test_scheduler_gpu.py holds osuf_ct_step to: fed the kernel's own fp32 row (and the fp32 threshold), a handful of
    fp32 roundings, 16 * 2^-24 * max(1, largest |term| of the element).  Sample 2 has t_next = 0: gain 0, the mean whatever noise holds."""
    B, per = 3, 6 * 37
    x, cond, null, noise = step_inputs(B, per)
    null = null if with_null else None
    scale = 7.0 if with_null else 1.0
    with guard(0xFF) as g:
        row = _row(B)
        xd, cd = g.place(x.to(DEV)), g.place(cond.to(DEV))
        nd = g.place(null.to(DEV)) if with_null else None
        zd = g.place(noise.to(DEV)) if with_noise else None
        s_rows = ops.ct_x0_quantile(xd, cd, nd, scale, row, objective, 0.9) if thresholded else None
        s = s_rows[:, 2] if thresholded else None
        got = ops.ct_step_ex(xd, cd, nd, scale, row, zd, objective, s)
        again = ops.ct_step_ex(xd, cd, nd, scale, row, zd, objective, s)
        poisoned = ops.ct_step_ex(xd, cd, nd, scale, row, g.place(torch.full_like(noise, float("nan")).to(DEV)), objective, s)
        g.check()
        got, again, poisoned, row_c = got.cpu(), again.cpu(), poisoned.cpu(), row.cpu()
        s_c = s.cpu() if thresholded else None
        g.release()
    want, terms = CO.step(x, cond, null, scale, row_c, noise if with_noise else None, objective, s_c)
    bound = 16 * 2.0 ** -24 * np.maximum(terms, 1.0)
    err = np.abs(got.double().numpy() - want)
    print(f"ct_objectives step_ex/{objective}/null{int(with_null)}/thr{int(thresholded)}/noise{int(with_noise)}: max err/bound = {(err / bound).max():.3f}"
          + (f"  s = {s_c.tolist()}" if thresholded else ""))
    assert torch.isfinite(got).all()
    assert (err <= bound).all(), (err / bound).max()
    assert torch.equal(got, again)
    if thresholded:
        assert (s_c > 1.0).any()
    mean_only, _ = CO.step(x, cond, null, scale, row_c, None, objective, s_c)
    assert torch.isfinite(poisoned[2]).all() and (np.abs(poisoned[2].double().numpy() - mean_only[2]) <= bound[2]).all()
    assert torch.isnan(poisoned[:2]).all()


# ---- osuf_ct_qsample -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", [ct.COLS_T, ct.COLS])
@pytest.mark.parametrize("objective", OBJECTIVES)
def test_qsample_and_target_against_fp64(objective, cols):
    """Two products and a sum per output: 4 * 2^-24 * (|alpha x0| + |sigma noise|) (for v: |alpha noise| + |sigma x0|); the noise and x_start
    targets are copies."""
    g0 = torch.Generator().manual_seed(21)
    x0, noise = torch.randn((3, 6, 37), generator=g0), torch.randn((3, 6, 37), generator=g0)
    t = torch.tensor([0.05, 0.5, 0.95], device=DEV)
    with guard(0xFF) as g:
        sched = ops.ct_schedule(t, t - 0.04 if cols == ct.COLS else None, ct.KINDS["cosine"])
        x_t, target = ops.ct_qsample(g.place(x0.to(DEV)), g.place(noise.to(DEV)), sched, objective)
        only_x, none = ops.ct_qsample(g.place(x0.to(DEV)), g.place(noise.to(DEV)), sched, objective, want_target=False)
        g.check()
        x_t, target, only_x, sched = x_t.cpu(), target.cpu(), only_x.cpu(), sched.cpu()
        g.release()
    assert none is None and torch.equal(only_x, x_t) and sched.shape == (3, cols)
    alpha, sigma = sched[:, ct.ALPHA], sched[:, ct.SIGMA]
    a, s = CO.f64(alpha).reshape(-1, 1, 1), CO.f64(sigma).reshape(-1, 1, 1)
    want = CO.q_sample(x0, noise, alpha, sigma)
    bound = 4 * 2.0 ** -24 * (np.abs(a * CO.f64(x0)) + np.abs(s * CO.f64(noise)))
    assert (np.abs(x_t.double().numpy() - want) <= bound).all()
    if objective == "v":
        bound_v = 4 * 2.0 ** -24 * (np.abs(a * CO.f64(noise)) + np.abs(s * CO.f64(x0)))
        assert (np.abs(target.double().numpy() - CO.target_of(x0, noise, alpha, sigma, "v")) <= bound_v).all()
    else:
        assert torch.equal(target, noise if objective == "noise" else x0)


# ---- GaussianDiffusionContinuousTimes.calculate_v / predict_start_from_v ------------------------------------------------------------------
@pytest.mark.parametrize("schedule", ["linear", "cosine"])
def test_scheduler_v_methods_against_fp64_and_round_trip(schedule):
    """The two methods against the restatement on the kernel's own fp32 alpha and sigma: two products and a sum per element,
    4 * 2^-24 * (|a y| + |s z|).  The round trip predict_start_from_v(q_sample(x0), t, calculate_v(x0, t, noise)) through the methods: each of
    x_t and v carries such an error, and alpha x_t - sigma v adds one more, so 3 * 4 * 2^-24 * (|x0| + |noise|) (alpha, sigma <= 1 and
    alpha^2 + sigma^2 = 1 to fp32 rounding, which the restatement's own round trip on the fp32 row measures and the bound adds)."""
    from osufusion_amd.modules import GaussianDiffusionContinuousTimes
    g0 = torch.Generator().manual_seed(33)
    x0, noise = torch.randn((4, 6, 37), generator=g0), torch.randn((4, 6, 37), generator=g0)
    t = torch.tensor([0.02, 0.3, 0.6, 0.97], device=DEV)
    sch = GaussianDiffusionContinuousTimes(noise_schedule=schedule)
    with guard(0xFF) as g:
        x0d, nzd = g.place(x0.to(DEV)), g.place(noise.to(DEV))
        row = sch.coefficients(t)
        v = sch.calculate_v(x0d, t, nzd)
        x_t = sch.q_sample(x0d, t, nzd)[0]
        start = sch.predict_start_from_v(x_t, t, v)
        g.check()
        row, v, x_t, start = row.cpu(), v.cpu(), x_t.cpu(), start.cpu()
        g.release()
    alpha, sigma = row[:, ct.ALPHA], row[:, ct.SIGMA]
    a, s = CO.f64(alpha).reshape(-1, 1, 1), CO.f64(sigma).reshape(-1, 1, 1)
    X, N = CO.f64(x0), CO.f64(noise)
    eps = 4 * 2.0 ** -24
    assert v.shape == x0.shape and v.dtype == torch.float32
    assert (np.abs(v.double().numpy() - CO.calculate_v(x0, noise, alpha, sigma)) <= eps * (np.abs(a * N) + np.abs(s * X))).all()
    # predict_start_from_v on the method's own fp32 inputs (x_t, v)
    want = CO.predict_start_from_v(x_t, v, alpha, sigma)
    assert (np.abs(start.double().numpy() - want) <= eps * (np.abs(a * CO.f64(x_t)) + np.abs(s * CO.f64(v)))).all()
    # the round trip through the three methods
    exact = CO.predict_start_from_v(CO.q_sample(x0, noise, alpha, sigma), CO.calculate_v(x0, noise, alpha, sigma), alpha, sigma)      # (a^2 + s^2) x0
    bound = 3 * eps * (np.abs(X) + np.abs(N)) + np.abs(exact - X)
    err = np.abs(start.double().numpy() - X)
    print(f"ct_objectives v_round_trip/{schedule}: max err = {err.max():.3e} max err/bound = {(err / bound).max():.3f} "
          f"|a^2 + s^2 - 1| = {np.abs(a * a + s * s - 1).max():.2e}")
    assert (err <= bound).all(), (err / bound).max()
    assert np.abs(a * a + s * s - 1).max() <= 16 * 2.0 ** -24                                # the fp32 row: a unit vector to a few roundings


# ---- osuf_mse_w ----------------------------------------------------------------------------------------------------------------------
def _mse_inputs(B=3, D=6, L=203, seed=8):
    g = torch.Generator().manual_seed(seed)
    pred, target = torch.randn((B, D, L), generator=g), torch.randn((B, D, L), generator=g)
    w = torch.rand(B, generator=g) * 3 + 0.1
    return pred, target, w


@pytest.mark.parametrize("lens", [None, [203, 120, 7]], ids=["full", "masked"])       # len = L and 0 < len < L
def test_mse_w_against_fp64_and_finite_differences(lens):
    """Loss: fp32 sums of a few positive terms per lane, a wave reduction, four partials: 16 * 2^-24 relative.  Gradient: one product chain
    per element, 8 * 2^-24 relative, against the analytic gradient of the restatement, itself checked by central differences in fp64."""
    pred, target, w = _mse_inputs()
    orig_len = torch.tensor(lens) if lens is not None else None
    with guard(0xFF) as g:
        pd = g.place(pred.to(DEV)).requires_grad_(True)
        loss = _MSEFn.apply(pd, g.place(target.to(DEV)), orig_len, g.place(w.to(DEV)))
        loss.backward()
        g.check()
        got, grad = loss.item(), pd.grad.cpu()
        g.release()
    want = CO.mse_w(pred, target, lens, w)
    assert abs(got - want) <= 16 * 2.0 ** -24 * want + 2.0 ** -24 * want, (got, want)      # + the fp32 rounding of the returned scalar
    B, D, L = pred.shape
    ln = np.array(lens if lens is not None else [L] * B)
    mask = (np.arange(L)[None, :] < ln[:, None])[:, None, :]
    analytic = 2 * CO.f64(w)[:, None, None] * mask * (CO.f64(pred) - CO.f64(target)) / (D * ln.sum())
    rng = np.random.default_rng(0)
    for _ in range(12):                                                                      # the restatement's gradient by central differences
        b, d_, l = rng.integers(B), rng.integers(D), rng.integers(L)
        hp, hm = CO.f64(pred).copy(), CO.f64(pred).copy()
        hp[b, d_, l] += 1e-4
        hm[b, d_, l] -= 1e-4
        fd = (CO.mse_w(hp, target, lens, w) - CO.mse_w(hm, target, lens, w)) / 2e-4
        assert abs(fd - analytic[b, d_, l]) <= 1e-9, (fd, analytic[b, d_, l])
    assert (np.abs(grad.double().numpy() - analytic) <= 8 * 2.0 ** -24 * np.abs(analytic)).all()
    if lens is not None:
        assert (grad[1, :, 120:] == 0).all() and (grad[2, :, 7:] == 0).all() and torch.isfinite(grad).all()


@pytest.mark.parametrize("lens", [None, [203, 120, 7]], ids=["full", "masked"])
def test_mse_w_with_ones_is_mse(lens):
    pred, target, _ = _mse_inputs()
    pd, td = pred.to(DEV), target.to(DEV)
    orig_len = torch.tensor(lens) if lens is not None else None
    acc, grad = ops.mse(pd, td, orig_len, True)
    acc_w, grad_w = ops.mse(pd, td, orig_len, True, torch.ones(3, device=DEV))
    assert torch.equal(acc, acc_w) and torch.equal(grad, grad_w)
    assert torch.equal(ops.mse(pd, td, orig_len, False, torch.ones(3, device=DEV))[0], acc)


# ---- ContinuousDiffusionOsuFusionDiT ---------------------------------------------------------------------------------------------------
def _backbone_kwargs(name):
    m = META[name]
    kw = dict(dim_h=m["dim_h"], depth=m["depth"], attn_dim_head=m["attn_dim_head"], attn_heads=m["attn_heads"], attn_qk_norm=m["attn_qk_norm"])
    if name.startswith("mmdit"):
        kw.update(backbone="mmdit", patch_size=m["patch_size"], attn_kv_heads=m["attn_kv_heads"])
    else:
        kw.update(backbone="dit")
    return kw


def _model(name, **kw):
    model = ContinuousDiffusionOsuFusionDiT(**_backbone_kwargs(name), **kw)
    model.load_state_dict({k: torch.from_numpy(param_pattern(k[len("unet."):], tuple(v.shape)).copy()) for k, v in model.state_dict().items()})
    return model.to(DEV)


def _inputs(name):
    m = META[name]
    return [torch.from_numpy(v).to(DEV) for v in synth_inputs(name, m["B"], m["L"])]          # x, a, c, t, noise


def _loop(model, a, c, x, cond_scale, step):
    """The sampler's loop written out, the step left to `step(i, x, cond, null, coef_i, noise)`; draws as sample()'s docstring says."""
    b = a.shape[0]
    cfg = cond_scale != 1.0
    total = model.scheduler.timesteps
    x = x.float().contiguous()
    with torch.inference_mode(), ops.reproducible_mode(True), ops.one_launch_attention(True), model._dtype_ctx():
        times = torch.linspace(1.0, 0.0, total + 1, device=DEV, dtype=torch.float32)
        coef = model.scheduler.coefficients(times[:-1].repeat_interleave(b), times[1:].repeat_interleave(b)).view(total, b, -1)
        log_snr = coef[:, :, 0].repeat(1, 2 if cfg else 1).contiguous()
        f = model._denoiser(a, c, cfg)
        for i in range(total):
            pred = f(x, log_snr[i])
            noise = torch.randn(x.shape, device=DEV) if i < total - 1 else None
            x = step(i, x, pred[:b], pred[b:] if cfg else None, coef[i], noise)
    return x


@pytest.mark.parametrize("name", NAMES)
def test_defaults_give_the_results_of_the_code_path_as_it_was(name):
    """A model built with the defaults: sample() against the loop with ops.ct_step, loss_with against q_sample + the backbone + the
    unweighted MSE, both bit for bit, and the state_dict's keys unchanged."""
    model = _model(name, sampling_timesteps=3)
    explicit = _model(name, sampling_timesteps=3, pred_objective="noise", dynamic_thresholding=False, min_snr_gamma=None)
    assert list(model.state_dict()) == list(explicit.state_dict())
    x, a, c, _, noise = _inputs(name)
    for cond_scale in (1.0, 7.0):
        torch.manual_seed(1234)
        got = model.sample(a, c, noise, cond_scale=cond_scale)
        torch.manual_seed(1234)
        want = _loop(model, a, c, noise, cond_scale, lambda i, xi, cond, null, k, z: ops.ct_step(xi, cond, null, cond_scale, k, z))
        assert torch.isfinite(got).all() and torch.equal(got, want)
    times = torch.linspace(0.2, 0.7, x.shape[0], device=DEV)
    orig_len = torch.tensor([x.shape[-1], x.shape[-1] - 17])
    torch.manual_seed(11)
    got = model.loss_with(x, a, c, noise, times, orig_len)
    torch.manual_seed(11)
    x_t, log_snr, _, _ = model.scheduler.q_sample(x, times, noise)
    want = _MSEFn.apply(model.unet(x_t, a, log_snr.contiguous(), c, cond_drop_prob=model.cond_drop_prob), noise.float(), orig_len)
    assert torch.isfinite(got).item() and torch.equal(got.detach(), want.detach())


@pytest.mark.parametrize("name", NAMES)
def test_v_objective_min_snr_loss_matches_the_restatement_and_trains(name):
    """loss_with for pred_objective = v, min_snr_gamma = 5 against the restatement's weighted loss of the backbone's own output: the target's
    fp32 rounding (2^-24 |target| against differences of order one, twice in the square) and the 16 * 2^-24 of the sum: 64 * 2^-24."""
    model = _model(name, pred_objective="v", min_snr_gamma=5.0)
    x, a, c, _, noise = _inputs(name)
    times = torch.tensor([0.15, 0.8], device=DEV)                                           # snr above and below gamma
    orig_len = torch.tensor([x.shape[-1], x.shape[-1] - 17])
    torch.manual_seed(11)
    loss = model.loss_with(x, a, c, noise, times, orig_len)
    torch.manual_seed(11)
    sched = model.scheduler.coefficients(times)
    x_t, _ = ops.ct_qsample(x.float().contiguous(), noise.float().contiguous(), sched, "v")
    pred = model.unet(x_t, a, sched[:, ct.LOG_SNR].contiguous(), c, cond_drop_prob=model.cond_drop_prob).detach()      # the same (training) forward
    sched = sched.cpu()
    snr = np.exp(CO.f64(sched[:, ct.LOG_SNR]))
    assert snr[0] > 5.0 > snr[1]
    w = CO.loss_weight(sched[:, ct.LOG_SNR], "v", 5.0)
    want = CO.mse_w(pred, CO.target_of(x, noise, sched[:, ct.ALPHA], sched[:, ct.SIGMA], "v"), orig_len.tolist(), w)
    print(f"ct_objectives v_loss/{name}: loss = {loss.item():.6f} restatement = {want:.6f} rel = {abs(loss.item() - want) / want:.2e} weights = {w.tolist()}")
    assert abs(loss.item() - want) <= 64 * 2.0 ** -24 * want, (loss.item(), want)
    loss.backward()
    torch.cuda.synchronize()
    without = sorted(k for k, p in model.named_parameters() if p.grad is None)
    print(f"ct_objectives v_loss/{name}: parameters without a gradient = {without}")
    assert without == NO_GRADIENT[name], without
    for k, p in model.named_parameters():
        assert p.grad is None or torch.isfinite(p.grad).all(), k
    first_attn = next(p for k, p in model.named_parameters() if k.startswith("unet.blocks.0.attn.to_q"))
    assert model.unet.null_cond.grad is not None and first_attn.grad is not None and first_attn.grad.abs().max() > 0


# Parameters that the training loss does not reach, per fixture (every other parameter must receive a finite gradient).  The MMDiT's last
# block (depth 2: blocks.1) still updates its audio stream, which nothing reads after it: that stream's output projection and MLP.
NO_GRADIENT = {"mmdit_h96": ["unet.blocks.1.attn_out_a.weight", "unet.blocks.1.mlp_a.0.bias", "unet.blocks.1.mlp_a.0.weight",
                             "unet.blocks.1.mlp_a.2.bias", "unet.blocks.1.mlp_a.2.weight"],
               "dit_h96": []}


@pytest.mark.parametrize("objective", ["x_start", "v"])
@pytest.mark.parametrize("name", NAMES)
def test_objective_without_thresholding_samples_and_trains_through_the_model(name, objective):
    """The `s = None` branch of the sampler for a v / x_start model: three steps at cond_scale 7 against the loop of backbone call +
    ops.ct_step_ex(..., s=None), bit for bit; one launch per step.  And loss_with against the unweighted MSE of the backbone's forward on
    ops.ct_qsample's x_noisy and target (for x_start the target is x itself)."""
    model = _model(name, sampling_timesteps=3, pred_objective=objective)
    x, a, c, _, noise = _inputs(name)
    timer = ops.KernelTimer(["osuf_ct_x0_quantile", "osuf_ct_step_ex", "osuf_ct_step"])
    ops.set_kernel_timer(timer)
    try:
        torch.manual_seed(7)
        got = model.sample(a, c, noise, cond_scale=7.0)
    finally:
        ops.set_kernel_timer(None)
    assert {k: v["launches"] for k, v in timer.summary().items()} == {"osuf_ct_step_ex": 3}
    torch.manual_seed(7)
    want = _loop(model, a, c, noise, 7.0, lambda i, xi, cond, null, k, z: ops.ct_step_ex(xi, cond, null, 7.0, k, z, objective, None))
    assert torch.isfinite(got).all() and torch.equal(got, want)
    torch.manual_seed(7)
    as_noise = _loop(model, a, c, noise, 7.0, lambda i, xi, cond, null, k, z: ops.ct_step(xi, cond, null, 7.0, k, z))
    assert not torch.equal(got, as_noise)                                                    # the objective does reach the step
    times = torch.linspace(0.2, 0.7, x.shape[0], device=DEV)
    orig_len = torch.tensor([x.shape[-1], x.shape[-1] - 17])
    torch.manual_seed(11)
    loss = model.loss_with(x, a, c, noise, times, orig_len)
    torch.manual_seed(11)
    sched = model.scheduler.coefficients(times)
    x_t, target = ops.ct_qsample(x.float().contiguous(), noise.float().contiguous(), sched, objective)
    if objective == "x_start":
        assert torch.equal(target, x.float())
    want = _MSEFn.apply(model.unet(x_t, a, sched[:, ct.LOG_SNR].contiguous(), c, cond_drop_prob=model.cond_drop_prob), target, orig_len)
    assert loss.grad_fn is not None and torch.isfinite(loss).item() and torch.equal(loss.detach(), want.detach())


@pytest.mark.parametrize("objective", ["noise", "v"])
@pytest.mark.parametrize("name", NAMES)
def test_thresholded_sampler_equals_the_plain_loop_and_repeats(name, objective):
    """Three steps at cond_scale 7: sample() against the loop of backbone call + ops.ct_x0_quantile + ops.ct_step_ex, bit for bit and twice;
    two launches per step; for the noise objective the threshold is live (the first step divides by alpha(t = 1))."""
    model = _model(name, sampling_timesteps=3, pred_objective=objective, dynamic_thresholding=True, dynamic_thresholding_percentile=0.95)
    _, a, c, _, x = _inputs(name)
    seen = []

    def step(i, xi, cond, null, k, z):
        rows = ops.ct_x0_quantile(xi, cond, null, 7.0, k, objective, 0.95)
        seen.append(rows)
        return ops.ct_step_ex(xi, cond, null, 7.0, k, z, objective, rows[:, 2])

    timer = ops.KernelTimer(["osuf_ct_x0_quantile", "osuf_ct_step_ex", "osuf_ct_step"])
    ops.set_kernel_timer(timer)
    try:
        torch.manual_seed(99)
        got = model.sample(a, c, x, cond_scale=7.0)
    finally:
        ops.set_kernel_timer(None)
    assert {k: v["launches"] for k, v in timer.summary().items()} == {"osuf_ct_x0_quantile": 3, "osuf_ct_step_ex": 3}
    torch.manual_seed(99)
    again = model.sample(a, c, x, cond_scale=7.0)
    torch.manual_seed(99)
    want = _loop(model, a, c, x, 7.0, step)
    assert torch.isfinite(got).all() and torch.equal(got, again) and torch.equal(got, want)
    s = torch.stack(seen)[:, :, 2].cpu()
    print(f"ct_objectives thresholded_sampler/{name}/{objective}: s per step = {s.tolist()}")
    assert (s >= 1.0).all()
    assert (s[1:] > 1.0).any()                              # live after the first step too (noise: step 0 divides by alpha(t = 1), s ~ 5e7)
    if objective == "noise":
        torch.manual_seed(99)
        static = _model(name, sampling_timesteps=3).sample(a, c, x, cond_scale=7.0)
        assert not torch.equal(static, got)


# ---- guarded memory --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_sample", [1, 257, 6 * 40])
def test_new_entry_points_between_canaries(per_sample):
    """Each of the four entry points on poisoned, canary-guarded outputs (and the quantile's workspace): every output element is written,
    nothing behind an allocation is."""
    B = 3
    x, cond, null, noise = step_inputs(B, per_sample, seed=per_sample)
    with guard(0xFF) as g:
        row = _row(B)
        xd, cd, nd, zd = (g.place(v.to(DEV)) for v in (x, cond, null, noise))
        outs = []
        for objective in OBJECTIVES:
            rows = ops.ct_x0_quantile(xd, cd, nd, 7.0, row, objective, 0.95)
            outs += [rows, ops.ct_step_ex(xd, cd, nd, 7.0, row, zd, objective, rows[:, 2]), ops.ct_step_ex(xd, cd, None, 1.0, row, None, objective, None)]
            outs += list(ops.ct_qsample(xd, zd, row, objective))
        w = g.place(torch.tensor([0.5, 1.0, 2.0], device=DEV))
        p3, t3 = xd.view(B, 1, per_sample), cd.view(B, 1, per_sample)
        for lens in (None, torch.tensor([per_sample, max(per_sample // 2, 1), 1])):
            acc, grad = ops.mse(p3, t3, lens, True, w)
            outs += [acc, grad]
        g.check()
        for o in outs:
            assert torch.isfinite(o).all()
        g.release()
