"""The MMDiT backbone on the GPU: the joint-attention row kernels (csrc/dit.hip) against fp64 torch, JointAttention against the reference's
module fixture and fp64 autograd of the restatement (tests/mmdit_oracle.py), and MMDiT against the reference's fixtures
(tests/golden/mmdit_*.npz).  The measured distances are recorded in profiles/mmdit_parity.md."""
import copy
import json
from pathlib import Path

import numpy as np
import pytest
import torch

from osufusion_amd import forced_compute_dtype, ops
from osufusion_amd import mmdit as Mm
from osufusion_amd.pattern import param_pattern, synth_inputs, uniform_pm
from tests import mmdit_oracle as O
from tests.test_attend_autograd_gpu import RL2, RMAX
from tests.test_poisoned_memory import relmax, rell2, rnd, run_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = Path(__file__).resolve().parent / "golden"
META = json.loads((GOLD / "mmdit_cases.json").read_text())
CASES = {k: v for k, v in META.items() if k.startswith("mmdit_")}

# (B, Na, Nx, H, G, D): G = 1, G = H, odd row counts on both sides of a 32-row block, every head dim
KERNEL_SHAPES = [(2, 5, 40, 6, 2, 16), (1, 33, 31, 4, 4, 32), (3, 64, 64, 2, 1, 64), (2, 7, 129, 8, 2, 128)]
SENTINEL = -1234.0                                                                  # exact in bf16


# ---------------------------------------------------------------------------------------------------------------------------------
# row kernels vs fp64 torch
# ---------------------------------------------------------------------------------------------------------------------------------
def _group_major(H, G):
    """perm[c] = the natural query head in column block c: natural head j sits in block (j % G) * (H / G) + j / G."""
    perm = [0] * H
    for j in range(H):
        perm[(j % G) * (H // G) + j // G] = j
    return perm


def _joint_ref(raw_a, raw_x, ga, gx, H, G, D):
    """fp64 joint q|k|v rows (B, Na + Nx, (H + 2G) D) from the two streams' raw rows (fp64 leaves); gammas (gq (H, 1, D), gk (G, 1, D)) or None."""
    rows = []
    for raw, gam in ((raw_a, ga), (raw_x, gx)):
        B, N, _ = raw.shape
        q, k, v = raw[..., :H * D].reshape(B, N, H, D), raw[..., H * D:(H + G) * D].reshape(B, N, G, D), raw[..., (H + G) * D:]
        if gam is not None:
            q = q / torch.linalg.vector_norm(q, dim=-1, keepdim=True).clamp_min(1e-12) * gam[0].reshape(H, D) * D ** 0.5
            k = k / torch.linalg.vector_norm(k, dim=-1, keepdim=True).clamp_min(1e-12) * gam[1].reshape(G, D) * D ** 0.5
        rows.append(torch.cat([q[:, :, _group_major(H, G)].reshape(B, N, H * D), k.reshape(B, N, G * D), v], -1))
    return torch.cat(rows, 1)


def _within_one_bf16_spacing(got, ref):
    """|got - ref| <= the bf16 spacing at ref: 2^(floor(log2 |ref|) - 7) (8 significand bits)."""
    ref = ref.double().cpu()
    spacing = torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -126))) - 7)
    return bool(((got.double().cpu() - ref).abs() <= spacing).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("gamma", [True, False], ids=["gamma", "cast"])
@pytest.mark.parametrize("shape", KERNEL_SHAPES, ids=lambda s: "B%d_Na%d_Nx%d_H%d_G%d_D%d" % s)
def test_joint_qknorm_fwd_bwd_vs_fp64(shape, gamma, dtype):
    """Forward: every bf16 output within one bf16 spacing of the fp64 value; inv within 1e-5 (fp32 sum of D <= 128 squares and one
    reciprocal: D 2^-24 < 1e-5).  Backward at the bounds tests/test_dit_gpu.py holds dit.qknorm_bwd to: the raw-projection gradient
    1e-5 (fp32 rows) / 1e-2 (bf16 rows) rel-L2 per q / k / v block, the clamped head on its own; dgamma 1e-5.  A stream's call leaves the
    other stream's joint rows untouched."""
    B, Na, Nx, H, G, D = shape
    W, Nj = (H + 2 * G) * D, Na + Nx
    raw_a, raw_x = rnd("raw_a", (B, Na, W)).to(dtype), rnd("raw_x", (B, Nx, W)).to(dtype)
    raw_x[0, 3, D:2 * D] = 0                                                        # an all-zero q head (natural head 1 or, H = 1.., the clamp branch)
    raw_a, raw_x = raw_a.to(DEV), raw_x.to(DEV)
    ga = gx = None
    if gamma:
        ga = ((1 + 0.2 * rnd("gqa", (H, 1, D))).to(DEV), (1 + 0.2 * rnd("gka", (G, 1, D))).to(DEV))
        gx = ((1 + 0.2 * rnd("gqx", (H, 1, D))).to(DEV), (1 + 0.2 * rnd("gkx", (G, 1, D))).to(DEV))
    joint = torch.full((B, Nj, W), SENTINEL, dtype=torch.bfloat16, device=DEV)
    inv_a = Mm.joint_qknorm_fwd(raw_a, joint, 0, *(ga or (None, None)), H, G, D)
    assert (joint[:, Na:] == SENTINEL).all() and not (joint[:, :Na] == SENTINEL).any()       # the map rows are not the audio call's
    inv_x = Mm.joint_qknorm_fwd(raw_x, joint, Na, *(gx or (None, None)), H, G, D)
    ra, rx = raw_a.double().cpu().requires_grad_(), raw_x.double().cpu().requires_grad_()
    gr = [tuple(t.double().cpu().requires_grad_() for t in gm) if gm is not None else None for gm in (ga, gx)]
    ref = _joint_ref(ra, rx, gr[0], gr[1], H, G, D)
    assert _within_one_bf16_spacing(joint, ref.detach())
    if not gamma:
        assert inv_a is None and inv_x is None
        if dtype == torch.bfloat16:
            assert torch.equal(joint.cpu().double(), ref.detach())                  # a pure permutation
    else:
        for inv, r in ((inv_a, ra), (inv_x, rx)):
            n = torch.linalg.vector_norm(r.detach()[..., :(H + G) * D].reshape(-1, H + G, D), dim=-1)
            reg = n > 0
            assert relmax(inv.cpu()[reg], (1 / n)[reg]) < 1e-5
            assert ((inv.cpu()[~reg] / 1e12 - 1).abs() < 1e-5).all()                 # 1 / max(0, 1e-12)
    g = rnd("g", (B, Nj, W)).to(DEV)
    ref.backward(g.double().cpu())
    tol = 1e-5 if dtype == torch.float32 else 1e-2
    for raw, r, off, inv, gm, grr in ((raw_a, ra, 0, inv_a, ga, gr[0]), (raw_x, rx, Na, inv_x, gx, gr[1])):
        if gamma:
            dx, dgamma = Mm.joint_qknorm_bwd(g, raw, off, inv, gm[0], gm[1], H, G, D)
            assert rell2(dgamma[:H].cpu(), grr[0].grad.reshape(H, D)) < 1e-5
            assert rell2(dgamma[H:].cpu(), grr[1].grad.reshape(G, D)) < 1e-5
        else:
            dx = Mm.joint_unnorm_bwd(g, raw, off, H, G, D)
        assert dx.dtype == dtype and dx.shape == raw.shape
        got, want = dx.cpu().double(), r.grad
        clamped = torch.zeros(got.shape, dtype=torch.bool)
        if gamma and off == Na:
            clamped[0, 3, D:2 * D] = True                                           # ~1e12 x the others (the norm is held at 1e-12): on its own
            assert rell2(got[clamped], want[clamped]) < tol
        for blk, (c0, c1) in zip("qkv", ((0, H * D), (H * D, (H + G) * D), ((H + G) * D, W))):
            m = ~clamped[..., c0:c1]
            e = rell2(got[..., c0:c1][m], want[..., c0:c1][m])
            assert e < tol, (blk, off, e)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", KERNEL_SHAPES, ids=lambda s: "B%d_Na%d_Nx%d_H%d_G%d_D%d" % s)
def test_joint_pack_unpack_round_trip(shape, dtype):
    B, Na, Nx, H, G, D = shape
    Nj, HD = Na + Nx, H * D
    for Ns, off, other in ((Na, 0, slice(Na, Nj)), (Nx, Na, slice(0, Na))):
        t = rnd("t", (B, Ns, HD)).to(torch.bfloat16).to(dtype).to(DEV)              # bf16 values: the bf16 joint buffer holds them exactly
        joint = torch.full((B, Nj, HD), SENTINEL, dtype=torch.bfloat16, device=DEV)
        Mm.joint_pack(t, joint, off, H, G, D)
        assert (joint[:, other] == SENTINEL).all()
        want = t.reshape(B, Ns, H, D)[:, :, _group_major(H, G)].reshape(B, Ns, HD)
        assert torch.equal(joint[:, off:off + Ns].to(dtype), want)
        back = Mm.joint_unpack(joint, Ns, off, dtype, H, G, D)
        assert back.dtype == dtype and torch.equal(back, t)


def test_joint_reductions_bit_identical_across_launches():
    B, Na, Nx, H, G, D = 2, 300, 213, 8, 2, 64
    W = (H + 2 * G) * D
    raw = rnd("raw", (B, Nx, W)).to(DEV)
    gq, gk = (1 + 0.2 * rnd("gq", (H, 1, D))).to(DEV), (1 + 0.2 * rnd("gk", (G, 1, D))).to(DEV)
    g = rnd("g", (B, Na + Nx, W)).to(DEV)
    joint = torch.zeros((B, Na + Nx, W), dtype=torch.bfloat16, device=DEV)
    inv = Mm.joint_qknorm_fwd(raw, joint, Na, gq, gk, H, G, D)
    r1, r2 = (Mm.joint_qknorm_bwd(g, raw, Na, inv, gq, gk, H, G, D) for _ in range(2))
    assert torch.equal(r1[0], r2[0]) and torch.equal(r1[1], r2[1])


def test_joint_norm_matches_the_single_stream_kernel_bit_for_bit():
    """G = H, one stream: the joint layout is the plain q|k|v rows, and dit.qknorm_fwd / _bwd are the joint kernels called that way (their
    Ns / off / G mapping and the inv / dgamma shapes).  The single-stream kernels these replaced are pinned by
    tests/golden/qknorm_parent_digests.json (tests/test_dit_gpu.py)."""
    from osufusion_amd import dit as Dt
    B, N, H, D = 2, 67, 4, 32
    raw = rnd("raw", (B, N, 3 * H * D)).to(DEV).bfloat16()
    gq, gk = (1 + 0.2 * rnd("gq", (H, 1, D))).to(DEV), (1 + 0.2 * rnd("gk", (H, 1, D))).to(DEV)
    g = rnd("g", (B, N, 3 * H * D)).to(DEV)
    y, inv = Dt.qknorm_fwd(raw, gq, gk, H, D)
    dx, dgamma = Dt.qknorm_bwd(g, raw, inv, gq, gk, H, D)
    joint = torch.empty_like(y)
    jinv = Mm.joint_qknorm_fwd(raw, joint, 0, gq, gk, H, H, D)
    jdx, jdgamma = Mm.joint_qknorm_bwd(g, raw, 0, jinv, gq, gk, H, H, D)
    assert torch.equal(joint, y) and torch.equal(jinv, inv) and torch.equal(jdx, dx) and torch.equal(jdgamma.view(2, H, D), dgamma)
    # the same stream at row offset 3 of a longer joint buffer: the forward kernel's general instance (row and head maps not compiled out)
    wide = torch.empty((B, N + 3, 3 * H * D), dtype=torch.bfloat16, device=DEV)
    winv = Mm.joint_qknorm_fwd(raw, wide, 3, gq, gk, H, H, D)
    assert torch.equal(wide[:, 3:], y) and torch.equal(winv, inv)


# ---------------------------------------------------------------------------------------------------------------------------------
# guarded allocations (tests/memguard.py through tests/test_poisoned_memory.run_case): the shapes above
# ---------------------------------------------------------------------------------------------------------------------------------
def joint_case(shape, dtype, gamma):
    def run(c):
        B, Na, Nx, H, G, D = shape
        W = (H + 2 * G) * D
        raws = [c.inp(rnd("raw_a", (B, Na, W)), dtype), c.inp(rnd("raw_x", (B, Nx, W)), dtype)]
        gam = [(c.inp(1 + 0.2 * rnd("gq" + s, (H, 1, D))), c.inp(1 + 0.2 * rnd("gk" + s, (G, 1, D)))) if gamma else (None, None) for s in "ax"]
        g = c.inp(rnd("g", (B, Na + Nx, W)))
        do = [c.inp(rnd("do_a", (B, Na, H * D)), dtype), c.inp(rnd("do_x", (B, Nx, H * D)), dtype)]
        joint = Mm.joint_buffer(B, Na + Nx, W, DEV)
        jdo = Mm.joint_buffer(B, Na + Nx, H * D, DEV)
        for s, (raw, off) in enumerate(zip(raws, (0, Na))):
            inv = Mm.joint_qknorm_fwd(raw, joint, off, *gam[s], H, G, D)
            Mm.joint_pack(do[s], jdo, off, H, G, D)
            if gamma:
                dx, dgamma = Mm.joint_qknorm_bwd(g, raw, off, inv, *gam[s], H, G, D)
                c.eq(f"inv{s}", inv), c.eq(f"dgamma{s}", dgamma)
            else:
                dx = Mm.joint_unnorm_bwd(g, raw, off, H, G, D)
            c.eq(f"dx{s}", dx)
        c.eq("joint", joint), c.eq("jdo", jdo)
        c.eq("o_a", Mm.joint_unpack(jdo, Na, 0, dtype, H, G, D)), c.eq("o_x", Mm.joint_unpack(jdo, Nx, Na, dtype, H, G, D))
    return run


POISON_CASES = [("%s_%s_%s" % ("B%d_Na%d_Nx%d_H%d_G%d_D%d" % s, "bf16" if dt == torch.bfloat16 else "f32", "gamma" if gm else "cast"), joint_case(s, dt, gm))
                for i, s in enumerate(KERNEL_SHAPES) for dt, gm in (((torch.bfloat16, True), (torch.float32, False)) if i % 2 == 0 else
                                                                    ((torch.float32, True), (torch.bfloat16, False)))]


@pytest.mark.parametrize("case", [c for c, _ in POISON_CASES])
def test_joint_kernels_on_poisoned_memory(case):
    run_case(dict(POISON_CASES)[case])


# ---------------------------------------------------------------------------------------------------------------------------------
# JointAttention
# ---------------------------------------------------------------------------------------------------------------------------------
def _check(name, got, want, rl2=RL2, rmax=RMAX):
    e2, em = rell2(got, want), relmax(got, want)
    print(f"mmdit_parity {name}: rel_l2={e2:.3e} relmax={em:.3e}")
    assert torch.isfinite(got).all(), name
    assert e2 < rl2 and em < rmax, (name, e2, em)


def _joint_inputs(j):
    x = torch.from_numpy(uniform_pm("joint/x", (j["B"], j["Nx"], j["dim"]), 1.0))
    a = torch.from_numpy(uniform_pm("joint/a", (j["B"], j["Na"], j["dim"]), 1.0))
    gx = torch.from_numpy(uniform_pm("joint/gx", (j["B"], j["Nx"], j["dim_head"] * j["heads"]), 1.0))
    ga = torch.from_numpy(uniform_pm("joint/ga", (j["B"], j["Na"], j["dim_head"] * j["heads"]), 1.0))
    return x, a, gx, ga


def _run_joint(net, x, a, gx, ga):
    x, a = x.to(DEV).requires_grad_(), a.to(DEV).requires_grad_()
    net.zero_grad(set_to_none=True)
    with forced_compute_dtype(torch.float32):
        ox, oa = net(x, a)
        ((ox * gx.to(DEV)).sum() + (oa * ga.to(DEV)).sum()).backward()
    return ox.detach(), oa.detach(), x.grad, a.grad


def test_joint_attention_vs_reference_fixture():
    """fp32 compute against the reference's recorded JointAttention (Na != Nx; its Attend is bf16 SDPA): outputs 6e-3 rel-L2 / 3e-2
    relmax, every input and parameter gradient 1e-2 / 3e-2 (the bounds of tests/test_cross_attend_gpu.py)."""
    from osufusion_amd.modules.mmdit import JointAttention
    j = META["joint_attention"]
    g = np.load(GOLD / "mod_joint_attention.npz")
    net = JointAttention(j["dim"], j["dim_head"], j["heads"], j["kv_heads"])
    net.load_state_dict({k: torch.from_numpy(param_pattern(k, tuple(v.shape)).copy()) for k, v in net.state_dict().items()})
    net.to(DEV)
    ox, oa, dx, da = _run_joint(net, *_joint_inputs(j))
    assert ox.shape == (j["B"], j["Nx"], j["heads"] * j["dim_head"]) and oa.shape == (j["B"], j["Na"], j["heads"] * j["dim_head"])
    _check("fixture/out_x", ox, torch.from_numpy(g["out_x"]), 6e-3), _check("fixture/out_a", oa, torch.from_numpy(g["out_a"]), 6e-3)
    _check("fixture/dx", dx, torch.from_numpy(g["dx"])), _check("fixture/da", da, torch.from_numpy(g["da"]))
    for k, p in net.named_parameters():
        _check("fixture/" + k, p.grad, torch.from_numpy(g["grad/" + k]))


@pytest.mark.parametrize("qk_norm", [True, False], ids=["qknorm", "nonorm"])
@pytest.mark.parametrize("H,G,D", [(4, 1, 32), (6, 2, 16), (2, 2, 64), (4, 2, 128)], ids=lambda v: str(v))
def test_joint_attention_vs_fp64_autograd(H, G, D, qk_norm):
    """fp32 compute against fp64 autograd of the reference formula with Attend's bf16 roundings (tests/mmdit_oracle.joint_attention), at
    the bounds of tests/test_cross_attend_gpu.py: outputs 6e-3 / 3e-2, gradients 1e-2 / 3e-2.  G = 1, 2 and H; Na != Nx."""
    from osufusion_amd.modules.mmdit import JointAttention
    j = dict(B=2, Nx=70, Na=45, dim=H * D, dim_head=D, heads=H)
    net = JointAttention(H * D, D, H, G, qk_norm=qk_norm)
    sd = {k: (1 + 0.2 * rnd(k, tuple(v.shape))) if k.endswith("gamma") else rnd(k, tuple(v.shape)) * v.shape[-1] ** -0.5 for k, v in net.state_dict().items()}
    net.load_state_dict(sd)
    net.to(DEV)
    x, a, gx, ga = _joint_inputs(j)
    gx, ga = gx.to(torch.bfloat16).float(), ga.to(torch.bfloat16).float()
    ox, oa, dx, da = _run_joint(net, x, a, gx, ga)
    p = {"attn." + k: v.double().requires_grad_() for k, v in sd.items()}
    xr, ar = x.double().requires_grad_(), a.double().requires_grad_()
    rox, roa = O.joint_attention(p, "attn.", xr, ar, H, G, D, qk_norm)
    ((rox * gx.double()).sum() + (roa * ga.double()).sum()).backward()
    tag = f"fp64/H{H}G{G}D{D}/{'qknorm' if qk_norm else 'nonorm'}/"
    _check(tag + "out_x", ox, rox.detach(), 6e-3), _check(tag + "out_a", oa, roa.detach(), 6e-3)
    _check(tag + "dx", dx, xr.grad), _check(tag + "da", da, ar.grad)
    for k, prm in net.named_parameters():
        _check(tag + k, prm.grad, p["attn." + k].grad)


# ---------------------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------------------
def _model(name):
    from osufusion_amd.modules.mmdit import MMDiT
    m = CASES[name]
    net = MMDiT(6, 96, 5, m["dim_h"], depth=m["depth"], patch_size=m["patch_size"], attn_dim_head=m["attn_dim_head"], attn_heads=m["attn_heads"],
                attn_kv_heads=m["attn_kv_heads"], attn_qk_norm=m["attn_qk_norm"])
    net.load_state_dict({k: torch.from_numpy(param_pattern(k, tuple(v.shape)).copy()) for k, v in net.state_dict().items()})
    return net.to(DEV), m


def _inputs(name, m, dev=DEV):
    return [torch.from_numpy(v).to(dev) for v in synth_inputs(name, m["B"], m["L"])]


def _grad(p):
    return p.grad if p.grad is not None else torch.zeros_like(p)                  # (the last block's audio tail feeds nothing)


_ORACLE = {}


def _oracle(name, m, dtype=torch.float64):
    """Output and gradients of the restatement, computed once per (case, dtype) and shared."""
    if (name, dtype) not in _ORACLE:
        net, _ = _model(name)
        p = {k: v.detach().cpu().to(dtype).requires_grad_() for k, v in net.state_dict().items()}
        x, a, c, t, noise = _inputs(name, m, "cpu")
        cfg = O.MMDiTConfig(dim_h=m["dim_h"], depth=m["depth"], patch_size=m["patch_size"], heads=m["attn_heads"], kv_heads=m["attn_kv_heads"],
                            dim_head=m["attn_dim_head"], qk_norm=m["attn_qk_norm"])
        y = O.mmdit_forward(p, cfg, x, a, t, c)
        torch.nn.functional.mse_loss(y, noise.to(dtype)).backward()
        _ORACLE[(name, dtype)] = (y.detach(), {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in p.items()})
    return _ORACLE[(name, dtype)]


@pytest.mark.parametrize("mode", ["exact", "x3"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_mmdit_fp32_vs_restatement(name, mode):
    """As tests/test_dit_gpu.py::test_dit_fp32_vs_restatement: output, null output and loss against the fp64 restatement (Attend's bf16
    roundings included) and the fp32 fixture: < 1e-3; the QK-norm gammas (the radial part of dq / dk, formed by the attention backward
    with heavy cancellation) 0.3 here and 1e-5 at the kernel level.
    The DiT's 1e-3 for every other parameter gradient does not transfer: on mmdit_h128_mqa (exact fp32 GEMMs) the gradients that pass
    through the joint attention measure 1.0e-3 .. 1.5e-3 (to_q_x 1.40e-3 / 1.48e-3 in blocks 0 / 1, to_k_x 1.01e-3, attn_out_a 1.04e-3,
    mlp_a.0.bias 1.03e-3; output 2.65e-4).  The attention kernels keep probabilities and score gradients in bf16 (they are held to 1e-2
    on their own, tests/test_cross_attend_gpu.py), the joint sequence is twice a stream's length and one K/V head collects the gradients of
    H / G query heads.  Each gradient is therefore held to 1.5 x the reference's own autocast-vs-fp32 distance of that parameter, recorded in
    the fixture (grad_dist, 3e-3 .. 1.8e-2): the project's usual allowance.  profiles/mmdit_parity.md keeps the measured values."""
    net, m = _model(name)
    x, a, c, t, noise = _inputs(name, m)
    g = np.load(GOLD / f"{name}.npz")
    prev = ops.set_f32_matmul(mode)
    try:
        with forced_compute_dtype(torch.float32):
            y = net(x, a, t, c)
            loss = torch.nn.functional.mse_loss(y, noise)
            loss.backward()
            with torch.no_grad():
                yn = net(x, a, t, c, cond_drop_prob=1.0)
    finally:
        ops.set_f32_matmul(prev)
    ry, rg = _oracle(name, m)
    errs = {"y": rell2(y.cpu(), ry)}
    for k, p in net.named_parameters():
        if rg[k].norm() > 0:
            errs[k] = rell2(_grad(p).cpu(), rg[k])
        else:
            assert _grad(p).norm() == 0, k
    print(f"mmdit_parity {name}/{mode}: y={errs['y']:.3e} worst grad={max((e, k) for k, e in errs.items() if not k.endswith('norm.gamma'))} "
          f"worst gamma={max([(e, k) for k, e in errs.items() if k.endswith('norm.gamma')] or [(0, '')])}")
    ref_dist = dict(zip(m["param_names"], np.load(GOLD / f"{name}_autocast.npz")["grad_dist"]))
    bound = lambda k: 1e-3 if k == "y" else 0.3 if k.endswith("norm.gamma") else 1.5 * float(ref_dist[k])
    bad = {k: (e, bound(k)) for k, e in errs.items() if not e < bound(k)}
    assert not bad, bad
    assert rell2(y.detach().cpu(), torch.from_numpy(g["y_cond"])) < 1e-3
    assert rell2(yn.cpu(), torch.from_numpy(g["y_null"])) < 1e-3
    assert abs(loss.item() - float(g["loss"])) / float(g["loss"]) < 1e-3


@pytest.mark.parametrize("name", sorted(CASES))
def test_mmdit_bf16_vs_reference_autocast(name):
    """As tests/test_dit_gpu.py::test_dit_bf16_vs_reference_autocast: bf16 compute against the fp32 golden within 1.5 x the reference's
    own autocast distance (output, null output, loss and flat gradient; the gradient's fp32 reference is the restatement, which
    tests/test_mmdit_cpu.py pins to the fixtures)."""
    net, m = _model(name)
    x, a, c, t, noise = _inputs(name, m)
    g32, g16 = np.load(GOLD / f"{name}.npz"), np.load(GOLD / f"{name}_autocast.npz")
    with forced_compute_dtype(torch.bfloat16):
        y = net(x, a, t, c)
        loss = torch.nn.functional.mse_loss(y, noise)
        loss.backward()
        with torch.no_grad():
            yn = net(x, a, t, c, cond_drop_prob=1.0)
    e_out = rell2(y.detach().cpu(), torch.from_numpy(g32["y_cond"]))
    e_null = rell2(yn.cpu(), torch.from_numpy(g32["y_null"]))
    e_loss = abs(loss.item() - float(g32["loss"])) / float(g32["loss"])
    ref_loss = abs(float(g16["loss"]) - float(g16["loss_fp32"])) / float(g16["loss_fp32"])
    _, rg = _oracle(name, m, torch.float32)
    names = m["param_names"]
    params = dict(net.named_parameters())
    flat = torch.cat([_grad(params[k]).cpu().flatten() for k in names])
    flat_ref = torch.cat([rg[k].flatten() for k in names])
    e_flat = rell2(flat, flat_ref)
    print(f"mmdit_parity {name}/bf16: out={e_out:.3e} (ref {float(g16['out_dist']):.3e}) null={e_null:.3e} (ref {float(g16['null_dist']):.3e}) "
          f"loss={e_loss:.3e} (ref {ref_loss:.3e}) flat_grad={e_flat:.3e} (ref {float(g16['flat_grad_dist']):.3e})")
    assert e_out < 1.5 * max(float(g16["out_dist"]), 2e-3), (e_out, float(g16["out_dist"]))
    assert e_null < 1.5 * max(float(g16["null_dist"]), 2e-3), (e_null, float(g16["null_dist"]))
    assert e_loss < 1.5 * max(ref_loss, 1e-3), (e_loss, ref_loss)
    assert e_flat < 1.5 * max(float(g16["flat_grad_dist"]), 2e-3), (e_flat, float(g16["flat_grad_dist"]))


def test_cond_scale_vs_goldens():
    name = "mmdit_h128_mqa"
    net, m = _model(name)
    x, a, c, t, _ = _inputs(name, m)
    g = np.load(GOLD / f"{name}.npz")
    yc, yn = torch.from_numpy(g["y_cond"]), torch.from_numpy(g["y_null"])
    with torch.no_grad(), forced_compute_dtype(torch.float32):
        guided = net.forward_with_cond_scale(x, a, t, c, cond_scale=3.0).cpu()
        plain = net.forward_with_cond_scale(x, a, t, c, cond_scale=1.0).cpu()
    assert rell2(guided, yn + (yc - yn) * 3.0) < 1e-3
    assert rell2(plain, yc) < 1e-3


def test_checkpointed_equals_plain_gradients():
    """gradient_checkpointing=True: the same loss and gradients (1e-6 rel-L2, the DiT's bound)."""
    name = "mmdit_h96"
    net, m = _model(name)
    net2 = copy.deepcopy(net)
    net2.set_gradient_checkpointing(True)
    assert all(b.gradient_checkpointing for b in net2.blocks) and not any(b.gradient_checkpointing for b in net.blocks)
    net.train(), net2.train()
    x, a, c, t, noise = _inputs(name, m)
    grads, losses = [], []
    for model in (net, net2):
        with forced_compute_dtype(torch.bfloat16):
            loss = torch.nn.functional.mse_loss(model(x, a, t, c), noise)
            loss.backward()
        losses.append(loss.item())
        grads.append({k: _grad(p).detach().clone() for k, p in model.named_parameters()})
    assert losses[0] == losses[1]
    for k in grads[0]:
        assert rell2(grads[1][k], grads[0][k]) < 1e-6 or grads[0][k].norm() == 0, k


def test_block_with_two_lengths_checkpointed():
    """MMDiTBlock through the reference's API with Na != Nx, plain and checkpointed: identical outputs, gradients within 1e-6."""
    from osufusion_amd.modules.mmdit import MMDiTBlock
    blk = MMDiTBlock(128, attn_dim_head=32, attn_heads=4, attn_kv_heads=2)
    blk.load_state_dict({k: torch.from_numpy(param_pattern(k, tuple(v.shape)).copy()) for k, v in blk.state_dict().items()})
    blk.to(DEV).train()
    x, a, c = rnd("x", (2, 37, 128)).to(DEV), rnd("a", (2, 50, 128)).to(DEV), rnd("c", (2, 128)).to(DEV)
    outs = []
    for ckpt in (False, True):
        blk.gradient_checkpointing = ckpt
        blk.zero_grad(set_to_none=True)
        xi, ai = x.clone().requires_grad_(), a.clone().requires_grad_()
        ox, oa = blk(xi, ai, c)
        assert ox.shape == x.shape and oa.shape == a.shape
        (ox.square().mean() + oa.square().mean()).backward()
        outs.append((ox.detach(), oa.detach(), xi.grad, ai.grad, {k: p.grad.clone() for k, p in blk.named_parameters()}))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert rell2(outs[1][2], outs[0][2]) < 1e-6 and rell2(outs[1][3], outs[0][3]) < 1e-6
    for k in outs[0][4]:
        assert torch.isfinite(outs[0][4][k]).all() and rell2(outs[1][4][k], outs[0][4][k]) < 1e-6, k


def test_no_grad_equals_training_forward_and_weight_updates_invalidate_packs():
    name = "mmdit_h96"
    net, m = _model(name)
    x, a, c, t, _ = _inputs(name, m)
    with forced_compute_dtype(torch.bfloat16):
        y = net(x, a, t, c)
        assert y.grad_fn is not None
        with torch.no_grad():
            y0 = net(x, a, t, c)
        with torch.inference_mode():
            y1 = net(x, a, t, c)
        assert y0.grad_fn is None and torch.equal(y0, y.detach()) and torch.equal(y1, y0)
        with torch.no_grad():
            for p in (net.blocks[0].attn.to_k_a.weight, net.blocks[1].attn_out_x.weight, net.emb_x.proj.weight):
                before = y0
                p.mul_(1.5)
                y0 = net(x, a, t, c)
                assert not torch.equal(y0, before)


def test_bf16_train_step_under_memguard():
    from tests.memguard import guard
    name = "mmdit_h96"
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
            assert p.grad is None or torch.isfinite(p.grad).all(), k
        g.release()
