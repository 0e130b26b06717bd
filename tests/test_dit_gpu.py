"""The DiT backbone on the GPU: its row kernels (adaLN, QK-norm, statistics pooling) against fp64 torch, and the module against the
torch restatement (tests/dit_oracle.py) and the reference's fixtures (tests/golden/dit_*.npz)."""
import copy
import hashlib
import json
from pathlib import Path

import numpy as np
import pytest
import torch

from osufusion_amd import dit as Dt
from osufusion_amd import forced_compute_dtype, ops
from osufusion_amd.pattern import param_pattern, synth_inputs
from tests import dit_oracle as O
from tests.test_poisoned_memory import relmax, rell2, rnd

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = Path(__file__).resolve().parent / "golden"
CASES = json.loads((GOLD / "dit_cases.json").read_text())


# ---------------------------------------------------------------------------------------------------------------------------------
# kernels vs fp64 torch
# ---------------------------------------------------------------------------------------------------------------------------------
def _adaln_ref(x, shift, scale):
    x = x.double()
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + 1e-6) * (1 + scale.double()[:, None]) + shift.double()[:, None]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("L", [1, 200, 1000])
@pytest.mark.parametrize("C", [64, 512, 1032])
@pytest.mark.parametrize("with_dres", [False, True])
def test_adaln_fwd_bwd_vs_fp64(C, L, dtype, with_dres):
    B = 2
    x = (rnd("x", (B, L, C)) * 2 + 0.5).to(DEV).to(dtype)
    mod = (rnd("mod", (B, 6 * C)) * 0.3).to(DEV)
    shift, scale = mod[:, 2 * C:3 * C], mod[:, 4 * C:5 * C]                         # column blocks read in place (row stride 6C)
    dy = rnd("dy", (B, L, C)).to(DEV).to(dtype)
    dres = rnd("dres", (B, L, C)).to(DEV).to(dtype) if with_dres else None
    out, mr = Dt.adaln_fwd(x, shift, scale)
    xr = x.double().cpu().requires_grad_()
    sh, sc = shift.double().cpu().requires_grad_(), scale.double().cpu().requires_grad_()
    ref = _adaln_ref(xr, sh, sc)
    tol = 2e-6 if dtype == torch.float32 else 1e-2
    assert relmax(out.cpu(), ref) < tol
    ref.backward(dy.double().cpu())
    dmod = torch.full((B, 6 * C), 7.0, device=DEV)                                  # stored into two of its blocks in place
    dx, dsh, dsc = Dt.adaln_bwd(dy, x, mr, scale, dres, dmod[:, C:2 * C], dmod[:, 5 * C:])
    want_dx = xr.grad + (dres.double().cpu() if with_dres else 0)
    assert rell2(dx.cpu(), want_dx) < (1e-5 if dtype == torch.float32 else 1e-2)
    gtol = 1e-5 if dtype == torch.float32 else 1e-2
    assert rell2(dmod[:, C:2 * C].cpu(), sh.grad) < gtol
    assert rell2(dmod[:, 5 * C:].cpu(), sc.grad) < gtol
    assert (dmod[:, :C] == 7).all() and (dmod[:, 2 * C:5 * C] == 7).all()             # the other blocks untouched
    dx2, dsh2, dsc2 = Dt.adaln_bwd(dy, x, mr, scale, dres)                            # fresh outputs: the same values
    assert torch.equal(dx2, dx) and torch.equal(dsh2, dmod[:, C:2 * C]) and torch.equal(dsc2, dmod[:, 5 * C:])


def _qknorm_ref(raw, gq, gk, H, D):
    M = raw.shape[0] * raw.shape[1]
    r = raw.double().reshape(M, 3, H, D)
    n = torch.linalg.vector_norm(r[:, :2], dim=-1, keepdim=True).clamp_min(1e-12)          # as F.normalize: zero gradient at a zero norm
    g = torch.stack([gq.double().reshape(H, D), gk.double().reshape(H, D)])
    qk = r[:, :2] / n * g * D ** 0.5
    return torch.cat([qk, r[:, 2:]], 1).reshape(raw.shape)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("H", [1, 2, 8])
@pytest.mark.parametrize("D", [16, 32, 64, 128])
def test_qknorm_fwd_bwd_vs_fp64(D, H, dtype):
    B, L = 2, 67
    raw = rnd("raw", (B, L, 3 * H * D)).to(dtype)
    raw[0, 3, :D] = 0                                                                # an all-zero q head: the clamp branch
    raw[1, 5, H * D:H * D + D] = 0                                                   # and an all-zero k head
    raw = raw.to(DEV)
    gq = (1 + 0.2 * rnd("gq", (H, 1, D))).to(DEV)
    gk = (1 + 0.2 * rnd("gk", (H, 1, D))).to(DEV)
    y, inv = Dt.qknorm_fwd(raw, gq, gk, H, D)
    rr = raw.double().cpu().requires_grad_()
    gqr, gkr = gq.double().cpu().requires_grad_(), gk.double().cpu().requires_grad_()
    ref = _qknorm_ref(rr, gqr, gkr, H, D)
    assert y.dtype == torch.bfloat16 and relmax(y.cpu(), ref) < 8e-3
    g = rnd("g", (B, L, 3 * H * D)).to(DEV)
    ref.backward(g.double().cpu())
    dx, dgamma = Dt.qknorm_bwd(g, raw, inv, gq, gk, H, D)
    tol = 1e-5 if dtype == torch.float32 else 1e-2
    # the two clamped heads' gradients are ~1e12 x the others' (the norm is held at 1e-12): each group is measured on its own, and the
    # regular rows per q / k / v block
    got, want = dx.cpu().double().reshape(B, L, 3, H, D), rr.grad.reshape(B, L, 3, H, D)
    clamped = torch.zeros(B, L, 3, H, dtype=torch.bool)
    clamped[0, 3, 0, 0] = clamped[1, 5, 1, 0] = True
    assert rell2(got[clamped], want[clamped]) < tol
    for blk in range(3):
        reg = ~clamped[:, :, blk]
        e = rell2(got[:, :, blk][reg], want[:, :, blk][reg])
        assert e < tol, ("qkv"[blk], e)
    assert rell2(dgamma[0].cpu(), gqr.grad.reshape(H, D)) < 1e-5
    assert rell2(dgamma[1].cpu(), gkr.grad.reshape(H, D)) < 1e-5


QKNORM_DIGESTS = json.loads((GOLD / "qknorm_parent_digests.json").read_text())


def _sha256(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("H,D", [(1, 128), (4, 64), (8, 64), (8, 128), (2, 16)])
def test_qknorm_bits_equal_the_single_stream_kernels(H, D, dtype):
    """dit.qknorm_fwd / _bwd ran on kernels of their own (qknorm_fwd_kernel / qknorm_bwd_kernel) before they became the one-stream, G = H
    call of the joint kernels.  tests/golden/qknorm_parent_digests.json holds the SHA-256 of what those kernels wrote on an MI355X for the
    inputs of test_qknorm_fwd_bwd_vs_fp64 (134 rows: not a multiple of 4, 9 backward workgroups; the two all-zero heads), one case per
    chunk-loop depth J = 1, 2, 4, 8 and per head width of 2, 8 and 16 lanes, for both raw dtypes: every output bit is still the same.
    The digest of the inputs is checked first, so a changed generator is told apart from a changed kernel."""
    B, L = 2, 67
    raw = rnd("raw", (B, L, 3 * H * D)).to(dtype)
    raw[0, 3, :D] = 0
    raw[1, 5, H * D:H * D + D] = 0
    gq, gk, g = 1 + 0.2 * rnd("gq", (H, 1, D)), 1 + 0.2 * rnd("gk", (H, 1, D)), rnd("g", (B, L, 3 * H * D))
    want = QKNORM_DIGESTS[f"H{H}_D{D}_{'f32' if dtype == torch.float32 else 'bf16'}"]
    assert _sha256(raw, gq, gk, g) == want["inputs"], "the generated inputs differ from the recorded ones"
    raw, gq, gk, g = (t.to(DEV) for t in (raw, gq, gk, g))
    y, inv = Dt.qknorm_fwd(raw, gq, gk, H, D)
    dx, dgamma = Dt.qknorm_bwd(g, raw, inv, gq, gk, H, D)
    assert y.dtype == torch.bfloat16 and tuple(inv.shape) == (B * L, 2 * H) and dx.dtype == dtype and tuple(dgamma.shape) == (2, H, D)
    got = {"y": _sha256(y), "inv": _sha256(inv), "dx": _sha256(dx), "dgamma": _sha256(dgamma)}
    assert got == {k: want[k] for k in got}


@pytest.mark.parametrize("L", [1, 7, 4096])
def test_stat_pool_vs_torch(L):
    a = (rnd("a", (3, 96, L)) * 5 - 10).to(DEV)
    got = Dt.stat_pool(a)
    want = torch.cat([a.double().mean(-1), a.double().std(-1)], 1)
    if L == 1:
        assert torch.allclose(got[:, :96].double(), want[:, :96]) and torch.isnan(got[:, 96:]).all()
    else:
        assert relmax(got, want) < 1e-5


def test_reductions_bit_identical_across_launches():
    B, L, C, H, D = 2, 1000, 512, 8, 64
    x = rnd("x", (B, L, C)).to(DEV).bfloat16()
    mod = rnd("mod", (B, 6 * C)).to(DEV) * 0.3
    dy = rnd("dy", (B, L, C)).to(DEV).bfloat16()
    raw = rnd("raw", (B, L, 3 * C)).to(DEV)
    gq, gk = torch.ones(H, 1, D, device=DEV), torch.ones(H, 1, D, device=DEV) * 1.5
    g = rnd("g", (B, L, 3 * C)).to(DEV)
    a = rnd("a", (B, 96, 4096)).to(DEV)

    def once():
        out, mr = Dt.adaln_fwd(x, mod[:, :C], mod[:, C:2 * C])
        _, dsh, dsc = Dt.adaln_bwd(dy, x, mr, mod[:, C:2 * C], None)
        _, inv = Dt.qknorm_fwd(raw, gq, gk, H, D)
        _, dgamma = Dt.qknorm_bwd(g, raw, inv, gq, gk, H, D)
        return [out, mr, dsh, dsc, inv, dgamma, Dt.stat_pool(a)]

    r1, r2 = once(), once()
    for u, v in zip(r1, r2):
        assert torch.equal(u, v)


# ---------------------------------------------------------------------------------------------------------------------------------
# poisoned-memory cases of every allocating function of osufusion_amd/dit.py (table checked by tests/test_dit_cpu.py)
# ---------------------------------------------------------------------------------------------------------------------------------
def adaln_case(C, L, dtype, dres):
    def run(c):
        B = 2
        x = c.inp(rnd("x", (B, L, C)), dtype)
        mod = c.inp(rnd("mod", (B, 6 * C)) * 0.3)
        dy = c.inp(rnd("dy", (B, L, C)), dtype)
        r = c.inp(rnd("r", (B, L, C)), dtype) if dres else None
        out, mr = Dt.adaln_fwd(x, mod[:, :C], mod[:, C:2 * C])
        dx, dsh, dsc = Dt.adaln_bwd(dy, x, mr, mod[:, C:2 * C], r)
        c.eq("out", out), c.eq("mr", mr), c.eq("dx", dx), c.eq("dshift", dsh), c.eq("dscale", dsc)
    return run


def qknorm_case(H, D, dtype):
    def run(c):
        B, L = 2, 33
        raw = c.inp(rnd("raw", (B, L, 3 * H * D)), dtype)
        gq, gk = c.inp(1 + 0.2 * rnd("gq", (H, 1, D))), c.inp(1 + 0.2 * rnd("gk", (H, 1, D)))
        g = c.inp(rnd("g", (B, L, 3 * H * D)))
        y, inv = Dt.qknorm_fwd(raw, gq, gk, H, D)
        dx, dgamma = Dt.qknorm_bwd(g, raw, inv, gq, gk, H, D)
        c.eq("y", y), c.eq("inv", inv), c.eq("dx", dx), c.eq("dgamma", dgamma)
    return run


def stat_pool_case(L):
    def run(c):
        a = c.inp(rnd("a", (2, 96, L)))
        c.eq("s", Dt.stat_pool(a))
    return run


POISON_CASES = {
    "adaln_fwd": [("C64_L200_f32", adaln_case(64, 200, torch.float32, False)), ("C1032_L37_bf16", adaln_case(1032, 37, torch.bfloat16, False))],
    "adaln_bwd": [("C512_L200_bf16_dres", adaln_case(512, 200, torch.bfloat16, True)), ("C1032_L37_f32", adaln_case(1032, 37, torch.float32, False))],
    "qknorm_fwd": [("H8_D64_bf16", qknorm_case(8, 64, torch.bfloat16)), ("H2_D16_f32", qknorm_case(2, 16, torch.float32))],
    "qknorm_bwd": [("H1_D128_bf16", qknorm_case(1, 128, torch.bfloat16)), ("H8_D32_f32", qknorm_case(8, 32, torch.float32))],
    "stat_pool": [("L200", stat_pool_case(200))],
}


@pytest.mark.parametrize("fn,case", [(k, c) for k, v in POISON_CASES.items() for c, _ in v])
def test_dit_kernels_on_poisoned_memory(fn, case):
    from tests.test_poisoned_memory import run_case
    run_case(dict(POISON_CASES[fn])[case])


# ---------------------------------------------------------------------------------------------------------------------------------
# the module
# ---------------------------------------------------------------------------------------------------------------------------------
def _model(name):
    from osufusion_amd.modules.dit import DiT
    m = CASES[name]
    net = DiT(6, 96, 5, m["dim_h"], depth=m["depth"], attn_heads=m["attn_heads"], attn_dim_head=m["attn_dim_head"], attn_qk_norm=m["attn_qk_norm"])
    net.load_state_dict({k: torch.from_numpy(param_pattern(k, tuple(v.shape)).copy()) for k, v in net.state_dict().items()})
    return net.to(DEV), m


def _inputs(name, m, dev=DEV):
    return [torch.from_numpy(v).to(dev) for v in synth_inputs(name, m["B"], m["L"])]


def _oracle(name, m, dtype=torch.float64):
    net, _ = _model(name)
    p = {k: v.detach().cpu().to(dtype).requires_grad_() for k, v in net.state_dict().items()}
    x, a, c, t, noise = _inputs(name, m, "cpu")
    cfg = O.DiTConfig(dim_h=m["dim_h"], depth=m["depth"], heads=m["attn_heads"], dim_head=m["attn_dim_head"], qk_norm=m["attn_qk_norm"])
    y = O.dit_forward(p, cfg, x, a, t, c)
    torch.nn.functional.mse_loss(y, noise.to(dtype)).backward()
    return y.detach(), {k: v.grad for k, v in p.items()}


@pytest.mark.parametrize("mode", ["exact", "x3"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_dit_fp32_vs_restatement(name, mode):
    """Output and every parameter gradient against the fp64 restatement (Attend's bf16 roundings included): < 1e-3 rel-L2.  The QK-norm
    gammas are the exception: their gradient sum_n g * u is the radial part of dq / dk, which the attention backward forms from bf16
    probabilities and score gradients with heavy cancellation; it is held to 0.3 here and to 1e-5 at the kernel level (exact inputs)."""
    net, m = _model(name)
    x, a, c, t, noise = _inputs(name, m)
    prev = ops.set_f32_matmul(mode)
    try:
        with forced_compute_dtype(torch.float32):
            y = net(x, a, t, c)
            torch.nn.functional.mse_loss(y, noise).backward()
    finally:
        ops.set_f32_matmul(prev)
    ry, rg = _oracle(name, m)
    errs = {"y": rell2(y.cpu(), ry)}
    for k, p in net.named_parameters():
        if rg[k].norm() > 0:
            errs[k] = rell2(p.grad.cpu(), rg[k])
    bad = {k: e for k, e in errs.items() if not e < (0.3 if k.endswith("norm.gamma") else 1e-3)}
    assert not bad, bad
    g = np.load(GOLD / f"{name}.npz")
    assert rell2(y.detach().cpu(), torch.from_numpy(g["y_cond"])) < 1e-3


@pytest.mark.parametrize("name", sorted(CASES))
def test_dit_bf16_vs_reference_autocast(name):
    """bf16 compute against the fp32 golden within 1.5 x the reference's own autocast distance (output, loss and flat gradient; the
    gradient's fp32 reference is the restatement, which tests/test_dit_cpu.py pins to the fixtures)."""
    net, m = _model(name)
    x, a, c, t, noise = _inputs(name, m)
    g32, g16 = np.load(GOLD / f"{name}.npz"), np.load(GOLD / f"{name}_autocast.npz")
    with forced_compute_dtype(torch.bfloat16):
        y = net(x, a, t, c)
        loss = torch.nn.functional.mse_loss(y, noise)
        loss.backward()
    e_out = rell2(y.detach().cpu(), torch.from_numpy(g32["y_cond"]))
    assert e_out < 1.5 * max(float(g16["out_dist"]), 2e-3), (e_out, float(g16["out_dist"]))
    e_loss = abs(loss.item() - float(g32["loss"])) / float(g32["loss"])
    ref_loss = abs(float(g16["loss"]) - float(g16["loss_fp32"])) / float(g16["loss_fp32"])
    assert e_loss < 1.5 * max(ref_loss, 1e-3), (e_loss, ref_loss)
    _, rg = _oracle(name, m, torch.float32)
    names = m["param_names"]
    params = dict(net.named_parameters())
    flat = torch.cat([params[k].grad.cpu().flatten() for k in names])
    flat_ref = torch.cat([rg[k].flatten() for k in names])
    e_flat = rell2(flat, flat_ref)
    assert e_flat < 1.5 * max(float(g16["flat_grad_dist"]), 2e-3), (e_flat, float(g16["flat_grad_dist"]))


def test_cond_drop_and_cond_scale_vs_goldens():
    name = "dit_h128"
    net, m = _model(name)
    x, a, c, t, _ = _inputs(name, m)
    g = np.load(GOLD / f"{name}.npz")
    yc, yn = torch.from_numpy(g["y_cond"]), torch.from_numpy(g["y_null"])
    with torch.no_grad(), forced_compute_dtype(torch.float32):
        null = net(x, a, t, c, cond_drop_prob=1.0).cpu()
        guided = net.forward_with_cond_scale(x, a, t, c, cond_scale=3.0).cpu()
        plain = net.forward_with_cond_scale(x, a, t, c, cond_scale=1.0).cpu()
    assert rell2(null, yn) < 1e-3
    assert rell2(guided, yn + (yc - yn) * 3.0) < 1e-3
    assert rell2(plain, yc) < 1e-3


def test_no_grad_keeps_nothing():
    net, m = _model("dit_h96")
    x, a, c, t, _ = _inputs("dit_h96", m)
    with torch.no_grad():
        y = net(x, a, t, c)
    assert y.grad_fn is None
    with torch.inference_mode():
        assert net(x, a, t, c).grad_fn is None


def test_checkpointed_equals_plain_gradients():
    name = "dit_h128"
    net, m = _model(name)
    net2 = copy.deepcopy(net)
    net2.set_gradient_checkpointing(True)
    net.train(), net2.train()
    x, a, c, t, noise = _inputs(name, m)
    grads = []
    for model in (net, net2):
        with forced_compute_dtype(torch.bfloat16):
            torch.nn.functional.mse_loss(model(x, a, t, c), noise).backward()
        grads.append({k: p.grad.detach().clone() for k, p in model.named_parameters()})
    for k in grads[0]:
        assert rell2(grads[1][k], grads[0][k]) < 1e-6 or grads[0][k].norm() == 0, k


class _LossWrapper(torch.nn.Module):
    """What a trainer drives: model(x, a, c, orig_len) -> loss (noise and timesteps fixed by the test)."""

    def __init__(self, dit, noise, t):
        super().__init__()
        self.dit, self.noise, self.t = dit, noise, t

    def forward(self, x, a, c, orig_len=None):
        return torch.nn.functional.mse_loss(self.dit(x, a, self.t, c), self.noise)


def test_trainer_step_then_fresh_module_agrees():
    from osufusion_amd.modules.dit import DiT
    from osufusion_amd.train import Trainer
    name = "dit_h128"
    net, m = _model(name)
    x, a, c, t, noise = _inputs(name, m)
    model = _LossWrapper(net, noise, t)
    trainer = Trainer(model, lr=1e-3, compute_dtype=torch.bfloat16)
    before = {k: v.detach().clone() for k, v in net.state_dict().items()}
    for _ in range(2):
        loss, norm = trainer.step(x, a, c)
        assert torch.isfinite(loss).item() and torch.isfinite(norm).item()
    sd = net.state_dict()
    assert any(not torch.equal(before[k], sd[k]) for k in sd)
    fresh = DiT(6, 96, 5, m["dim_h"], depth=m["depth"], attn_heads=m["attn_heads"], attn_dim_head=m["attn_dim_head"]).to(DEV)
    fresh.load_state_dict({k: v.detach().clone() for k, v in sd.items()})
    with torch.no_grad(), forced_compute_dtype(torch.bfloat16):
        y1, y2 = net(x, a, t, c), fresh(x, a, t, c)
    assert torch.equal(y1, y2)


def test_bf16_train_step_under_memguard():
    from tests.memguard import guard
    name = "dit_h96"
    net, m = _model(name)
    x, a, c, t, noise = _inputs(name, m)
    with guard(0xFF) as g:
        with forced_compute_dtype(torch.bfloat16):
            loss = torch.nn.functional.mse_loss(net(x, a, t, c), noise)
            loss.backward()
        torch.cuda.synchronize()
        g.check()
        assert torch.isfinite(loss).item()
        for k, p in net.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all(), k
        g.release()
