"""GPU parity tests (run with -m gpu on an MI355X): HIP path vs the oracle / golden vectors, through the C ABI.

Tolerances (relative to the reference tensor's max-abs unless stated):
  fp32 mode : 1e-3  -- north_star's bound vs the reference's PyTorch-CPU outputs (goldens); most ops land at 1e-5..1e-4,
                       attention is bf16 inside the reference itself (attention.py:87-101), noise floor ~5e-4.
  bf16 mode : 3e-2 element-wise on single blocks vs the oracle's bf16 emulation, 2e-2 rel-L2 on whole-UNet outputs.
"""
import contextlib
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from osufusion_amd.pattern import param_pattern, synth_inputs, uniform_pm

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import osufusion_amd as oa
    from osufusion_amd import functional as Fn
    from osufusion_amd import ops
    from osufusion_amd.models.diffusion import OsuFusion
    from osufusion_amd.modules import residual as R
    from osufusion_amd.modules import unet as U

from oracle import diffusion_oracle as DO
from oracle import unet_oracle as O

DEV = "cuda"
B = 2


def T(a, dev=DEV):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def relmax(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu() if isinstance(b, torch.Tensor) else torch.from_numpy(np.asarray(b)).double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return ((a - b).abs().max() / (b.abs().max() + 1e-20)).item()


def rell2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu() if isinstance(b, torch.Tensor) else torch.from_numpy(np.asarray(b)).double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return ((a - b).norm() / (b.norm() + 1e-20)).item()


def report(name, **vals):
    """Append achieved errors to gpurun_out/parity_metrics.jsonl (quoted in DESIGN.md)."""
    import os
    os.makedirs("gpurun_out", exist_ok=True)
    with open("gpurun_out/parity_metrics.jsonl", "a") as f:
        f.write(json.dumps({"test": name, **{k: (v if isinstance(v, (list, str)) else float(v)) for k, v in vals.items()}}) + "\n")


@pytest.fixture()
def forcing():
    """forcing(**overrides): ops.force for the rest of the test."""
    with contextlib.ExitStack() as stack:
        yield lambda **kw: stack.enter_context(ops.force(**kw))


def load_pattern(module):
    sd = {k: T(param_pattern(k, tuple(v.shape))) for k, v in module.state_dict().items()}
    module.load_state_dict(sd, strict=True)
    return module


def G(golden_dir, name):
    return np.load(golden_dir / f"{name}.npz")


# --------------------------------------------------------------------------------------------------------
# raw kernels vs torch
# --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_mfma_layout_exact_integers(dtype):
    """A=I-style exactness check with asymmetric integer operands: every MFMA fragment map must be right."""
    M, N, K = 160, 136, 72
    a = torch.randint(-3, 4, (M, K), device=DEV).to(dtype)
    w = torch.randint(-3, 4, (N, K), device=DEV).to(dtype)
    want = a.double() @ w.double().t()
    got = ops.gemm_nt(a, w.unsqueeze(0).contiguous(), None)
    assert torch.equal(got.double(), want)
    dy = torch.randint(-2, 3, (M, N), device=DEV).to(dtype)
    gw = ops.gemm_tn(dy, a)[0]
    assert torch.equal(gw.double(), dy.double().t() @ a.double())


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 2e-5), (torch.bfloat16, 1e-2)])
@pytest.mark.parametrize("M,N,K,in_act,out_act", [(32, 128, 256, 0, 0), (32, 256, 128, 1, 2), (2, 64, 5, 0, 0), (48, 72, 200, 1, 0),
                                                  (64, 1024, 1024, 1, 2), (7, 33, 17, 0, 2), (32, 512, 2048, 1, 0), (5, 40, 24, 1, 2),
                                                  (33, 264, 136, 0, 2)])
def test_skinny_linear_kernels(dtype, tol, M, N, K, in_act, out_act):
    """osuf_skinny_fwd / _bwd (embedding-sized MLPs, fp32 masters read in place) vs torch: y, dx, dW, db; M not a multiple of 32,
    K not a multiple of 8 (cond_mlp.0 has K=5), fused input SiLU / output sigmoid and their derivatives."""
    x = T(uniform_pm("sk.x", (M, K), 1.5)).requires_grad_()
    w = T(uniform_pm("sk.w", (N, K), 1.0 / np.sqrt(K))).requires_grad_()
    b = T(uniform_pm("sk.b", (N,), 0.2)).requires_grad_()
    gy = T(uniform_pm("sk.g", (M, N), 1.0))
    xr, wr, br = (t.detach().double().requires_grad_() for t in (x, w, b))
    xin = F.silu(xr) if in_act else xr
    if dtype == torch.bfloat16:                              # the kernel rounds both MFMA operands to bf16 (fp32 accumulate)
        rnd = lambda t: t + (t.float().bfloat16().double() - t).detach()
        z = F.linear(rnd(xin), rnd(wr), br)
    else:
        z = F.linear(xin, wr, br)
    yr = torch.sigmoid(z) if out_act else z
    yr.backward(gy.double())
    y = Fn.SkinnyLinearFn.apply(x, w, b, dtype, in_act, out_act)
    y.backward(gy)
    assert relmax(y, yr) < tol
    assert relmax(x.grad, xr.grad) < tol * (1 if dtype == torch.float32 else 3)
    assert relmax(w.grad, wr.grad) < tol * (1 if dtype == torch.float32 else 3)
    assert relmax(b.grad, br.grad) < 1e-5
    # direct accumulation into an existing .grad (Trainer path): a second backward doubles it
    Fn.enable_direct_grads(True)
    try:
        g0 = w.grad.clone()
        y2 = Fn.SkinnyLinearFn.apply(x.detach(), w, b, dtype, in_act, out_act)
        y2.backward(gy)
        assert relmax(w.grad, 2 * g0) < 1e-5
    finally:
        Fn.enable_direct_grads(False)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("kind,O,I,k", [("same", 40, 72, 3), ("same", 33, 17, 1), ("same", 64, 96, 15), ("same", 8, 40, 7), ("down", 48, 40, 3),
                                        ("up", 24, 100, 3)])
def test_pack_weight_kernel_bit_exact(dtype, kind, O, I, k):
    """osuf_pack_weight vs its contract restated with torch ops: bit-exact (a cast at most, and for "up" one fp32 add)."""
    w = T(uniform_pm(f"pack.{kind}.{O}.{I}.{k}", (O, I, k), 1.0))
    if k == 1:
        w = w[:, :, 0].contiguous()
    fwd, dgr = ops.pack_weight(w, dtype, kind)
    w3 = w if w.dim() == 3 else w.unsqueeze(-1)
    ref_f = w3.permute(2, 0, 1).to(dtype)
    wt = w3.permute(2, 1, 0)
    if kind == "same":
        ref_d = wt.flip(0).to(dtype)
    elif kind == "down":
        ref_d = torch.cat([wt, wt[2:3]], 0).to(dtype)
    else:
        ref_d = torch.stack([wt[2], wt[1] + wt[2], wt[0] + wt[1], wt[0]], 0).to(dtype)
    assert torch.equal(fwd, ref_f.contiguous()) and torch.equal(dgr, ref_d.contiguous())
    # two weights stacked along O (fused q|kv projection operands)
    if k == 1:
        w2 = T(uniform_pm("pack.second", (24, I), 1.0))
        cache = Fn.PackCache()
        f2, d2 = cache.packs(("t", dtype), (w, w2), (w, w2), "same", dtype)
        cat = torch.cat([w, w2], 0)
        assert torch.equal(f2[0], cat.to(dtype)) and torch.equal(d2[0], cat.t().contiguous().to(dtype))


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 2e-5), (torch.bfloat16, 1e-2)])
@pytest.mark.parametrize("kind,k,L", [("same", 3, 96), ("same", 1, 64), ("same", 7, 40), ("same", 15, 200), ("down", 3, 96), ("up", 3, 56),
                                      ("same", 3, 8), ("down", 3, 300)])
def test_conv_fn_forward_backward(dtype, tol, kind, k, L):
    Cin, Cout = 48, 72
    x = torch.randn(B, Cin, L, device=DEV)
    w = (torch.randn(Cout, Cin, k, device=DEV) / (Cin * k) ** 0.5).requires_grad_()
    b = torch.randn(Cout, device=DEV).requires_grad_()
    xq = x.to(dtype).float().clone().requires_grad_()
    wq = w.detach().to(dtype).float().requires_grad_()
    bq = b.detach().clone()
    if kind == "same":
        ref = F.conv1d(xq, wq, bq, padding=k // 2)
    elif kind == "down":
        ref = F.conv1d(F.pad(xq, (0, 1), mode="reflect"), wq, bq, stride=2)
    else:
        ref = F.conv1d(F.interpolate(xq, scale_factor=2.0, mode="nearest"), wq, bq, padding=1)
    rows = x.detach().permute(0, 2, 1).contiguous().to(dtype).clone().requires_grad_()
    out = Fn.ConvFn.apply(rows, w, b, Fn.PackCache(), kind)
    assert relmax(out.float().permute(0, 2, 1), ref) < tol
    g = torch.randn_like(ref)
    gq = g.to(dtype).float()
    ref.backward(gq)
    out.backward(g.permute(0, 2, 1).contiguous().to(dtype))
    assert relmax(rows.grad.float().permute(0, 2, 1), xq.grad) < tol
    assert relmax(w.grad, wq.grad) < tol
    assert relmax(b.grad, gq.sum((0, 2))) < tol


@pytest.mark.parametrize("kind,k,L", [("same", 3, 200), ("same", 1, 520), ("down", 3, 96), ("up", 3, 56), ("same", 15, 64)])
def test_big_tile_gemm_kernel(kind, k, L):
    """The 256x256 8-wave LDS-DMA kernel is normally selected only for chip-filling shapes; force it on small ragged ones
    (M, N, K tails, every row-map mode, every epilogue option) and compare with the 128x128 kernel bit for bit."""
    Cin, Cout = 72, 328
    x = torch.randn(B, L, Cin, device=DEV).to(torch.bfloat16)
    w = (torch.randn(Cout, Cin, k, device=DEV) / (Cin * k) ** 0.5)
    bias = torch.randn(Cout, device=DEV)
    Lout = {"same": L, "down": L // 2, "up": 2 * L}[kind]
    res = torch.randn(B, Lout, Cout, device=DEV).to(torch.bfloat16)
    rscale = torch.rand(B, Cout, device=DEV)
    outs = []
    for big in (0, 1):                                           # fp32 partial tiles pin the kernel's products (the bf16-pair tiles of round 4 have
        with ops.force(gemm_big=big, wgrad_f32_partials=True):   # their own test, tests/test_round4_gpu.py)
            stats = torch.zeros(B, 2, dtype=torch.float64, device=DEV)
            y, pre = Fn.conv_forward(x, w, bias, Fn.PackCache(), kind, None, act=1, residual=res, rscale=rscale, stats=stats, want_pre=True)
            dx = Fn.conv_dgrad(y, w, Fn.PackCache(), kind, L, residual=x)
            dw = Fn.conv_wgrad(res, x, w, kind)                  # 256x256 LDS-DMA wgrad kernel when forced
        outs.append((y.float(), pre.float(), stats.clone(), dx.float(), dw.float()))
    (y0, p0, s0, d0, w0), (y1, p1, s1, d1, w1) = outs
    assert torch.equal(p0, p1)
    # y = silu(.)+res*rscale: the two kernels' epilogues are separate instantiations and may contract mul+add differently -- at most a
    # bf16 ulp on a handful of elements; d (the input gradient computed FROM y) inherits that
    for u, v in ((y0, y1), (d0, d1)):
        assert torch.allclose(u, v, rtol=2.0 ** -7, atol=1e-3) and (u != v).float().mean().item() < 1e-3
    assert torch.allclose(s0, s1, rtol=1e-6)
    assert relmax(w1, w0) < 1e-5                                 # fp32 atomics: same products, different summation order
    xq, wq = x.float(), w.to(torch.bfloat16).float()
    if kind == "same":
        ref = F.conv1d(xq.permute(0, 2, 1), wq, bias, padding=k // 2)
    elif kind == "down":
        ref = F.conv1d(F.pad(xq.permute(0, 2, 1), (0, 1), mode="reflect"), wq, bias, stride=2)
    else:
        ref = F.conv1d(F.interpolate(xq.permute(0, 2, 1), scale_factor=2.0, mode="nearest"), wq, bias, padding=1)
    assert relmax(p1.permute(0, 2, 1), ref) < 1e-2


@pytest.mark.parametrize("N,K,k,L", [(16, 256, 3, 2048), (32, 328, 1, 4100), (8, 64, 3, 1500), (32, 1024, 1, 2304)])
def test_skinny_n_gemm_kernel(N, K, k, L):
    """gemm_nt_skinny_kernel (N <= 32, M >= 4096: the rank-r LoRA products) vs torch conv1d on the same bf16-rounded operands:
    taps with zero padding at sample boundaries, K tail, M tail, N < 32."""
    Bq = 3
    x = torch.randn(Bq, L, K, device=DEV).to(torch.bfloat16)
    w = (torch.randn(N, K, k, device=DEV) / (K * k) ** 0.5).to(torch.bfloat16)
    wp = w.permute(2, 0, 1).contiguous()                                 # [k][N][K]
    y = ops.gemm_nt(x, wp, None, taps=k, lin=L, lout=L, stride=1, pad=k // 2, mode=0, out_shape=(Bq, L, N))
    ref = F.conv1d(x.float().permute(0, 2, 1), w.float(), None, padding=k // 2).permute(0, 2, 1)
    assert y.shape == ref.shape and relmax(y.float(), ref) < 1e-2


@pytest.mark.parametrize("N1,N2,k,L", [(256, 16, 1, 2048), (328, 32, 3, 1500), (1024, 8, 3, 1400), (40, 24, 1, 4100)])
def test_skinny_wgrad_kernel(N1, N2, k, L):
    """gemm_tn_skinny_kernel (N2 <= 32, M >= 4096: dB = dy^T u and dA^T = x^T du of the LoRA path) vs an fp64 reference on the same
    bf16-rounded operands: taps with zero padding at sample edges, N1 / N2 / M tails, split-over-m atomics."""
    Bq = 3
    dy = torch.randn(Bq, L, N1, device=DEV).to(torch.bfloat16)
    x = torch.randn(Bq, L, N2, device=DEV).to(torch.bfloat16)
    got = ops.gemm_tn(dy, x, taps=k, lin=L, lout=L, stride=1, pad=k // 2, mode=0, n1=N1)          # [k][N1][N2]
    ref = torch.zeros(k, N1, N2, dtype=torch.float64, device=DEV)
    xd, yd = x.double(), dy.double()
    for t in range(k):
        sh = t - k // 2                                                     # source row = m + sh inside the sample
        lo, hi = max(0, -sh), min(L, L - sh)
        ref[t] = torch.einsum("bmn,bmk->nk", yd[:, lo:hi], xd[:, lo + sh:hi + sh])
    assert got.shape == ref.shape and relmax(got, ref) < 1e-4


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 5e-5), (torch.bfloat16, 2e-2)])
@pytest.mark.parametrize("film", [False, True])
def test_block_fn(dtype, tol, film):
    Cin, C, L = 40, 64, 136
    x = torch.randn(B, Cin, L, device=DEV).to(dtype).float()
    blk = load_pattern(R.Block(Cin, C).to(DEV))
    ss = (torch.randn(B, 2 * C, device=DEV) * 0.3).requires_grad_() if film else None
    nm = O.Numerics("bf16" if dtype == torch.bfloat16 else "fp32")
    p = {"m." + k: v.detach().cpu().clone().requires_grad_() for k, v in blk.state_dict().items()}
    xr = x.cpu().clone().requires_grad_()
    ssr = ss.detach().cpu().clone().requires_grad_() if film else None
    ref = O.block(p, "m", xr, (ssr[:, :C, None], ssr[:, C:, None]) if film else None, nm)
    rows = x.detach().permute(0, 2, 1).contiguous().to(dtype).clone().requires_grad_()
    out = blk.forward_rows(rows, ss)
    assert relmax(out.float().permute(0, 2, 1), ref) < tol
    g = torch.randn(B, C, L).to(dtype).float()
    ref.backward(g)
    out.backward(g.to(DEV).permute(0, 2, 1).contiguous().to(dtype))
    assert relmax(rows.grad.float().permute(0, 2, 1), xr.grad) < 3 * tol
    assert relmax(blk.proj.weight.grad, p["m.proj.weight"].grad) < 3 * tol
    assert relmax(blk.proj.bias.grad, p["m.proj.bias"].grad) < 3 * tol
    assert relmax(blk.norm.weight.grad, p["m.norm.weight"].grad) < 3 * tol
    assert relmax(blk.norm.bias.grad, p["m.norm.bias"].grad) < 3 * tol
    if film:
        assert relmax(ss.grad, ssr.grad) < 3 * tol


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 5e-5), (torch.bfloat16, 2e-2)])
def test_global_context_and_gate(dtype, tol):
    C, L = 48, 200
    h = torch.randn(B, C, L, device=DEV).to(dtype).float()
    gc = load_pattern(R.GlobalContext(C, C).to(DEV))
    p = {"m." + k: v.detach().cpu().clone().requires_grad_() for k, v in gc.state_dict().items()}
    hr = h.cpu().clone().requires_grad_()
    ref_gate = O.global_context(p, "m", hr, O.Numerics("bf16" if dtype == torch.bfloat16 else "fp32"))
    res = torch.randn(B, C, L).to(dtype).float()
    ref = hr * ref_gate + res
    rows = h.detach().permute(0, 2, 1).contiguous().to(dtype).clone().requires_grad_()
    gate = gc.gate_from_rows(rows)
    assert relmax(gate, ref_gate[..., 0]) < tol
    out = Fn.GateResFn.apply(rows, gate, res.to(DEV).permute(0, 2, 1).contiguous().to(dtype))
    assert relmax(out.float().permute(0, 2, 1), ref) < tol
    g = torch.randn(B, C, L).to(dtype).float()
    ref.backward(g)
    out.backward(g.to(DEV).permute(0, 2, 1).contiguous().to(dtype))
    assert relmax(rows.grad.float().permute(0, 2, 1), hr.grad) < 3 * tol
    for k in ("to_k.weight", "layers.0.weight", "layers.0.bias", "layers.2.weight", "layers.2.bias"):
        assert relmax(dict(gc.named_parameters())[k].grad, p["m." + k].grad) < 5 * tol, k


@pytest.mark.parametrize("N", [8, 64, 200, 512])
def test_mqa_flash_vs_sdpa(N):
    H, D = 4, 64
    qkv = torch.randn(B, N, (H + 2) * D, device=DEV).to(torch.bfloat16)
    o, lse = ops.mqa_fwd(qkv, B, N, H, D, torch.bfloat16, D ** -0.5)
    q = qkv[..., : H * D].view(B, N, H, D).permute(0, 2, 1, 3).float().cpu()
    k = qkv[..., H * D: (H + 1) * D].float().cpu()[:, None].expand(B, H, N, D)
    v = qkv[..., (H + 1) * D:].float().cpu()[:, None].expand(B, H, N, D)
    s = (q @ k.transpose(-1, -2)) * D ** -0.5
    ref = (s.softmax(-1) @ v).permute(0, 2, 1, 3).reshape(B, N, H * D)
    assert relmax(o.float(), ref) < 1.5e-2                          # bf16 P and bf16 output rounding
    assert rell2(o.float(), ref) < 5e-3
    ref_lse2 = torch.logsumexp(s, -1) / np.log(2.0)
    assert (lse.cpu() - ref_lse2).abs().max() < 2e-3
    # backward vs autograd of the fp32 formula
    qkv32 = qkv.float().cpu().requires_grad_()
    q2 = qkv32[..., : H * D].view(B, N, H, D).permute(0, 2, 1, 3)
    k2 = qkv32[..., H * D: (H + 1) * D][:, None]
    v2 = qkv32[..., (H + 1) * D:][:, None]
    o2 = (((q2 @ k2.transpose(-1, -2)) * D ** -0.5).softmax(-1) @ v2).permute(0, 2, 1, 3).reshape(B, N, H * D)
    do = torch.randn(B, N, H * D).to(torch.bfloat16)
    o2.backward(do.float())
    dqkv = ops.mqa_bwd(qkv, o, do.to(DEV), lse, B, N, H, D, D ** -0.5)
    assert rell2(dqkv, qkv32.grad) < 1e-2
    assert relmax(dqkv, qkv32.grad) < 3e-2
    # fused epilogue: transpose of the RoPE rotation on dq / dk (not dv) + cast == the stand-alone rope_bwd kernel on the fp32 result
    cos, sin = Fn.rope_tables(N, D, 2 * N, DEV)
    for out_dt in (torch.float32, torch.bfloat16):
        ref_r = ops.rope_bwd(dqkv, out_dt, cos, sin, N, H + 1, H + 2, D)
        got_r = ops.mqa_bwd(qkv, o, do.to(DEV), lse, B, N, H, D, D ** -0.5, out_dt, cos, sin)
        assert got_r.dtype == out_dt and relmax(got_r.float(), ref_r.float()) < (1e-5 if out_dt == torch.float32 else 8e-3)


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-3), (torch.bfloat16, 3e-2)])
def test_transformer_block_vs_oracle(dtype, tol):
    C, N = 96, 136
    cfg = O.UNetConfig(dim_h=C, attn_dim_head=64, attn_heads=4, attn_kv_heads=1)
    blk = load_pattern(U.TransformerBlock(C, attn_dim_head=64, attn_heads=4, attn_kv_heads=1, attn_context_len=256).to(DEV))
    p = {"m." + k: v.detach().cpu().clone().requires_grad_() for k, v in blk.state_dict().items()}
    x = torch.randn(B, C, N).to(dtype).float()
    xr = x.clone().requires_grad_()
    ref = O.transformer_block(p, "m", xr, cfg, 256, O.Numerics("bf16" if dtype == torch.bfloat16 else "fp32"))
    rows = x.to(DEV).permute(0, 2, 1).contiguous().to(dtype).clone().requires_grad_()
    out = blk.forward_rows(rows)
    assert relmax(out.float().permute(0, 2, 1), ref) < tol
    g = torch.randn(B, C, N).to(dtype).float()
    ref.backward(g)
    out.backward(g.to(DEV).permute(0, 2, 1).contiguous().to(dtype))
    gtol = 2e-2 if dtype == torch.float32 else 6e-2                   # SDPA backward is bf16 on both sides
    assert rell2(rows.grad.float().permute(0, 2, 1), xr.grad) < gtol
    for k, v in blk.named_parameters():
        assert rell2(v.grad, p["m." + k].grad) < gtol, k


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 5e-3), (torch.bfloat16, 4e-2)])
@pytest.mark.parametrize("heads,kv_heads", [(4, 2), (4, 4), (6, 3)])
def test_grouped_query_attention_vs_oracle(dtype, tol, heads, kv_heads):
    """Attention with kv_heads > 1 (unet.py:132-135: query head j reads K/V head j mod kv_heads): forward and every gradient -- through
    the head-block permutation of to_q / to_out and one launch set per K/V head -- against the oracle's autograd; optimizer-style
    in-place weight updates must invalidate the packed operands of the permuted views."""
    C, N = 96, 136
    cfg = O.UNetConfig(dim_h=C, attn_dim_head=64, attn_heads=heads, attn_kv_heads=kv_heads)
    att = load_pattern(U.Attention(C, 64, heads, kv_heads, context_len=256).to(DEV))
    for rep in range(2):
        p = {"m." + k: v.detach().cpu().clone().requires_grad_() for k, v in att.state_dict().items()}
        x = torch.randn(B, N, C).to(dtype).float()
        xr = x.clone().requires_grad_()
        ref = O.attention(p, "m", xr, cfg, 256, O.Numerics("bf16" if dtype == torch.bfloat16 else "fp32"))
        rows = x.to(DEV).to(dtype).clone().requires_grad_()
        with oa.forced_compute_dtype(dtype):
            out = att(rows)
        assert relmax(out.float(), ref) < tol
        g = torch.randn(B, N, C).to(dtype).float()
        ref.backward(g)
        for v in att.parameters():
            v.grad = None
        out.backward(g.to(DEV).to(dtype))
        gtol = 2e-2 if dtype == torch.float32 else 6e-2                   # SDPA backward is bf16 on both sides
        assert rell2(rows.grad.float(), xr.grad) < gtol
        for k, v in att.named_parameters():
            assert rell2(v.grad, p["m." + k].grad) < gtol, k
        with torch.no_grad():                                             # what torch.optim does: the second pass must see new weights
            for v in att.parameters():
                v.add_(0.05 * torch.randn_like(v))


def test_scheduler_and_optimizer_kernels():
    x = torch.randn(4, 6, 100, device=DEV)
    n = torch.randn_like(x)
    t = torch.tensor([0, 17, 500, 999], device=DEV)
    from osufusion_amd.models.diffusion import DDIMSchedule
    sch = DDIMSchedule()
    acp = DO.ddim_alphas_cumprod()
    assert torch.allclose(sch.add_noise(x, n, t).cpu(), DO.add_noise(x.cpu(), n.cpu(), t.cpu(), acp), atol=1e-6)
    sch.set_timesteps(50)
    assert sch.timesteps.tolist() == DO.ddim_timesteps(50).tolist()
    for tt in (980, 500, 0):
        coef = torch.tensor([sch.step_coefficients(tt)] * 4, dtype=torch.float32, device=DEV)
        null = torch.randn_like(x)
        got = ops.ddim_step(x, n, null, 2.0, coef)
        eps = null.cpu() + (n.cpu() - null.cpu()) * 2.0
        assert torch.allclose(got.cpu(), DO.ddim_step(eps, tt, x.cpu(), acp, 50), atol=2e-6)
    # AdamW vs torch.optim.AdamW, 3 steps, odd length
    nel = 1027
    p0 = torch.randn(nel, device=DEV)
    pt = p0.clone().requires_grad_()
    opt = torch.optim.AdamW([pt], lr=1e-3, weight_decay=1e-2)
    p, m, v = p0.clone(), torch.zeros(nel, device=DEV), torch.zeros(nel, device=DEV)
    for step in range(1, 4):
        g = torch.randn(nel, device=DEV)
        pt.grad = g.clone()
        opt.step()
        ops.adamw(p, g, m, v, 1e-3, 0.9, 0.999, 1e-8, 1e-2, step)
    assert torch.allclose(p, pt.detach(), atol=1e-6)
    acc = torch.zeros(1, dtype=torch.float64, device=DEV)
    ops.sqnorm(g, acc)
    assert abs(acc.item() - (g.double() ** 2).sum().item()) < 1e-6 * acc.item()
    pred, tgt = torch.randn(3, 6, 50, device=DEV), torch.randn(3, 6, 50, device=DEV)
    ol = torch.tensor([50, 20, 35])
    acc, grad = ops.mse(pred, tgt, ol, True)
    mask = (torch.arange(50)[None] < ol[:, None]).float()[:, None].to(DEV)
    assert abs(acc.item() - (((pred - tgt) ** 2) * mask).sum().item()) < 1e-3


# --------------------------------------------------------------------------------------------------------
# modules vs golden vectors (fp32 mode; the reference's own outputs)
# --------------------------------------------------------------------------------------------------------
TOL = 1e-3


def test_modules_vs_golden(golden_dir):
    with oa.forced_compute_dtype(torch.float32):
        x = T(uniform_pm("mod/x48", (B, 48, 96), 1.0))
        t = T(uniform_pm("mod/t", (B, 64), 1.0))
        c = T(uniform_pm("mod/c", (B, 64), 1.0))
        g = G(golden_dir, "mod_block")
        m = load_pattern(R.Block(48, 80).to(DEV))
        ss = (T(uniform_pm("mod/scale", (B, 80, 1), 0.5)), T(uniform_pm("mod/shift", (B, 80, 1), 0.5)))
        assert relmax(m(x), g["y_plain"]) < TOL
        assert relmax(m(x, scale_shift=ss), g["y_film"]) < TOL
        m = load_pattern(R.GlobalContext(48, 48).to(DEV))
        assert relmax(m(x), G(golden_dir, "mod_global_context")["y"]) < TOL
        m = load_pattern(R.ResidualBlock(48, 80, 64, 64).to(DEV))
        assert relmax(m(x, t, c), G(golden_dir, "mod_resblock_film")["y"]) < TOL
        m = load_pattern(R.ResidualBlock(48, 48, None, None).to(DEV))
        assert relmax(m(x), G(golden_dir, "mod_resblock_plain")["y"]) < TOL
        m = load_pattern(R.Block(48, 80, norm=False).to(DEV))                 # nn.Identity instead of the GroupNorm (residual.py:71)
        g = G(golden_dir, "mod_block_nonorm")
        xg = x.clone().requires_grad_()
        ssg = tuple(v.clone().requires_grad_() for v in ss)
        assert relmax(m(x), g["y_plain"]) < TOL
        y = m(xg, scale_shift=ssg)
        assert relmax(y, g["y_film"]) < TOL
        y.backward(T(uniform_pm("mod/gy_nonorm", tuple(y.shape), 1.0)))
        for got, key in ((xg.grad, "dx"), (m.proj.weight.grad, "dw"), (m.proj.bias.grad, "db"), (ssg[0].grad, "dscale"), (ssg[1].grad, "dshift")):
            assert relmax(got, g[key]) < TOL, key
        m = load_pattern(R.SqueezeExcite(48, 48).to(DEV))                     # the use_gca=False gate (residual.py:40-59,116)
        assert relmax(m(x), G(golden_dir, "mod_squeeze_excite")["y"]) < TOL
        m = load_pattern(R.ResidualBlock(48, 80, 64, 64, use_gca=False).to(DEV))
        g = G(golden_dir, "mod_resblock_se")
        xg = x.clone().requires_grad_()
        y = m(xg, t, c)
        assert relmax(y, g["y"]) < TOL
        y.backward(T(uniform_pm("mod/gy_se", tuple(y.shape), 1.0)))
        assert relmax(xg.grad, g["dx"]) < TOL and relmax(m.se.layers[0].weight.grad, g["dw_se0"]) < TOL
        assert relmax(m.block1.proj.weight.grad, g["dw_proj1"]) < TOL
        m = load_pattern(U.Downsample(48, 80).to(DEV))
        assert relmax(m(x), G(golden_dir, "mod_downsample")["y"]) < TOL
        m = load_pattern(U.Upsample(48, 80).to(DEV))
        assert relmax(m(x), G(golden_dir, "mod_upsample")["y"]) < TOL
        m = load_pattern(U.Parallel(torch.nn.Conv1d(48, 80, 3, padding=1), torch.nn.Conv1d(48, 80, 1)).to(DEV))
        assert relmax(m(x), G(golden_dir, "mod_parallel")["y"]) < TOL
        m = load_pattern(U.CrossEmbedLayer(96, 128, (3, 7, 15)).to(DEV))
        assert relmax(m(T(uniform_pm("mod/xa", (B, 96, 64), 1.0))), G(golden_dir, "mod_cross_embed")["y"]) < TOL
        m = load_pattern(U.CrossEmbedLayer(6, 128, (3, 7, 15)).to(DEV))
        assert relmax(m(T(uniform_pm("mod/x6", (B, 6, 64), 1.0))), G(golden_dir, "mod_cross_embed6")["y"]) < TOL
        m = U.SinusoidalPositionEmbedding(128)
        assert relmax(m(torch.tensor([0, 1, 17, 500, 999], device=DEV)), G(golden_dir, "mod_sinusoidal")["y"]) < 1e-4
        m = load_pattern(U.Attention(96, 64, 4, 1, context_len=256).to(DEV))
        assert relmax(m(T(uniform_pm("mod/xt", (B, 128, 96), 1.0))), G(golden_dir, "mod_attention")["y"]) < TOL
        m = load_pattern(U.Attention(96, 64, 4, 2, context_len=256).to(DEV))               # grouped-query (kv_heads = 2)
        assert relmax(m(T(uniform_pm("mod/xt", (B, 128, 96), 1.0))), G(golden_dir, "mod_attention_gqa")["y"]) < TOL
        m = load_pattern(U.TransformerBlock(96, attn_dim_head=64, attn_heads=4, attn_kv_heads=1, attn_context_len=256).to(DEV))
        assert relmax(m(T(uniform_pm("mod/xc", (B, 96, 128), 1.0))), G(golden_dir, "mod_transformer")["y"]) < TOL
        te, ce = T(uniform_pm("mod/te", (B, 64), 1.0)), T(uniform_pm("mod/ce", (B, 64), 1.0))
        xb = T(uniform_pm("mod/xb", (B, 64, 64), 1.0))
        for name, li, down, xin, dout in (("mod_unetblock_down", 0, True, xb, 96), ("mod_unetblock_down_last", 1, True, xb, 96),
                                          ("mod_unetblock_up", 0, False, T(uniform_pm("mod/xu", (B, 112, 64), 1.0)), 48)):
            m = load_pattern(U.UNetBlock(64, dout, 64, 64, li, 2, 1, down, 64, 2, 1, 128).to(DEV))
            y, s = m(xin, te, ce)
            gg = G(golden_dir, name)
            assert relmax(y, gg["y"]) < TOL, name
            assert relmax(s, gg["skip"]) < TOL, name
        m = load_pattern(U.AudioEncoder(96, 96, dim_h_mult=(1, 2), num_layer_blocks=(1, 1), cross_embed_kernel_sizes=(3, 7, 15),
                                        attn_dim_head=64, attn_heads=2, attn_kv_heads=1).to(DEV))
        assert relmax(m(T(uniform_pm("mod/xae", (B, 96, 64), 1.0))), G(golden_dir, "mod_audio_encoder")["y"]) < TOL


def test_rope_and_attend_modules_vs_golden(golden_dir):
    from osufusion_amd.modules.attention import RotaryPositionEmbedding
    for n, sb in ((512, 512), (520, 256)):
        g = G(golden_dir, f"mod_rope_{n}_{sb}")
        r = RotaryPositionEmbedding(64, scale_base=sb)
        q, k = T(uniform_pm(f"mod/ropeq{n}", (1, 2, n, 64), 1.0)), T(uniform_pm(f"mod/ropek{n}", (1, 2, n, 64), 1.0))
        qo, ko = r(q, k)
        assert relmax(qo, g["q"]) < 5e-3 and relmax(ko, g["k"]) < 5e-3       # outputs are bf16 (the next op's cast)


def _build_model(case, golden_dir):
    meta = json.loads((golden_dir / "unet_cases.json").read_text())[case]
    cfgd = {k: (tuple(v) if isinstance(v, list) else v) for k, v in meta["cfg"].items()}
    kw = {k: v for k, v in cfgd.items() if not k.startswith("dim_in_")}
    model = OsuFusion(kw.pop("dim_h"), **kw).to(DEV)
    load_pattern(model.unet)
    return meta, cfgd, model


@pytest.mark.parametrize("case", ["unet_tiny", "unet_small16", "unet_mid"])      # small16: SURVEY 8c's tiny configuration, attn_dim_head = 16 (attn_generic.hpp)
def test_unet_vs_golden_fp32(golden_dir, case):
    meta, cfgd, model = _build_model(case, golden_dir)
    net = model.unet
    g = G(golden_dir, case)
    x, a, c, t, noise = (T(v) for v in synth_inputs(case, meta["B"], meta["L"]))
    with oa.forced_compute_dtype(torch.float32):
        with torch.no_grad():
            Lo = meta["L_odd"]
            e_cond = rell2(net(x, a, t, c, cond_drop_prob=0.0), g["y_cond"])
            e_null = rell2(net(x, a, t, c, cond_drop_prob=1.0), g["y_null"])
            e_odd = rell2(net(x[..., :Lo].contiguous(), a[..., :Lo].contiguous(), t, c), g["y_odd"])
            report(f"unet_fp32_fwd/{case}", cond=e_cond, null=e_null, odd=e_odd)
            assert max(e_cond, e_null, e_odd) < TOL
        loss = model.loss_with(x, a, c, noise, t, cond_drop_prob=0.0)
        report(f"unet_fp32_loss/{case}", rel=abs(loss.item() - float(g["loss"])) / abs(float(g["loss"])))
        assert abs(loss.item() - float(g["loss"])) < TOL * abs(float(g["loss"]))
        loss.backward()
    names = meta["param_names"]
    params = dict(net.named_parameters())
    gn = np.array([params[k].grad.norm().item() for k in names])
    ref = g["grad_norms"]
    rel = np.abs(gn - ref) / (ref + 1e-3 * ref.max())
    worst = 0.0
    for key in g.files:
        if key.startswith("g/"):
            got = params[key[2:]].grad.flatten()[:24]
            worst = max(worst, relmax(got, g[key]))
    report(f"unet_fp32_grads/{case}", grad_norm_max_rel=rel.max(), grad_norm_median_rel=float(np.median(rel)), grad_slice_max_rel=worst)
    assert rel.max() < 2e-2, f"grad-norm mismatch {rel.max():.3e} at {names[int(rel.argmax())]}"
    assert worst < 2e-2


@pytest.mark.parametrize("case", ["unet_tiny", "unet_mid"])
def test_unet_bf16_vs_oracle_emulation(golden_dir, case):
    meta, cfgd, model = _build_model(case, golden_dir)
    net = model.unet
    cfg = O.UNetConfig(**cfgd)
    p = O.make_params(cfg)
    x, a, c, t, noise = (torch.from_numpy(v) for v in synth_inputs(case, meta["B"], meta["L"]))
    with torch.no_grad():
        ref16 = O.unet_forward(p, cfg, x, a, t, c, mode="bf16")
        ref32 = O.unet_forward(p, cfg, x, a, t, c, mode="fp32")
    with oa.forced_compute_dtype(torch.bfloat16), torch.no_grad():
        got = net(x.to(DEV), a.to(DEV), t.to(DEV), c.to(DEV))
    e16, e32, floor = rell2(got, ref16), rell2(got, ref32), rell2(ref16, ref32)
    print(f"{case}: bf16 HIP vs oracle-bf16 {e16:.3e}; vs oracle-fp32 {e32:.3e}; oracle bf16-vs-fp32 {floor:.3e}")
    report(f"unet_bf16_fwd/{case}", hip_vs_oracle_bf16=e16, hip_vs_oracle_fp32=e32, oracle_bf16_vs_fp32=floor)
    assert e16 < 2e-2
    assert e32 < 3 * floor + 1e-2


@pytest.mark.parametrize("case", ["unet_tiny", "unet_mid"])
def test_unet_bf16_vs_reference_autocast(golden_dir, case):
    """The timed (bf16) mode against the REFERENCE's own bf16 arithmetic: `{case}_autocast.npz` holds the imported reference UNet run under
    torch.autocast("cpu", bfloat16) (trainer.py:295,374) on the fp32 fixtures' weights and inputs, and its distance from its own fp32
    run (unet_mid: output 1.08e-2, flat gradient 8.0e-3).  HIP-bf16 is held to the fp32 golden within 1.5 x that distance (output,
    prediction, flat gradient), and per parameter to 2.5 x / median 1.25 x of the reference-autocast distance on that parameter."""
    meta, cfgd, model = _build_model(case, golden_dir)
    net = model.unet
    g32, g16 = G(golden_dir, case), G(golden_dir, f"{case}_autocast")
    x, a, c, t, noise = (T(v) for v in synth_inputs(case, meta["B"], meta["L"]))
    cfg = O.UNetConfig(**cfgd)
    p = {k: v.requires_grad_() for k, v in O.make_params(cfg, prefix="unet.").items()}
    xs, as_, cs, ts, ns = (torch.from_numpy(v) for v in synth_inputs(case, meta["B"], meta["L"]))
    DO.training_loss(p, cfg, xs, as_, cs, ns, ts, cond_drop_prob=0.0).backward()          # oracle fp32 (pinned to the fp32 golden): full gradients
    with oa.forced_compute_dtype(torch.bfloat16):
        with torch.no_grad():
            y = net(x, a, t, c, cond_drop_prob=0.0)
        loss = model.loss_with(x, a, c, noise, t, cond_drop_prob=0.0)
        loss.backward()
    e_out, ref_out = rell2(y, g32["y_cond"]), float(g16["out_dist"])
    e_vs_autocast = rell2(y, g16["y_cond"])
    names = meta["param_names"]
    params = dict(net.named_parameters())
    got = {k: params[k].grad.detach().float().cpu() for k in names}
    ref = {k: p["unet." + k].grad for k in names}
    flat_got, flat_ref = torch.cat([got[k].flatten() for k in names]), torch.cat([ref[k].flatten() for k in names])
    e_flat, ref_flat = rell2(flat_got, flat_ref), float(g16["flat_grad_dist"])
    floor = 1e-4 * flat_ref.norm().item() / len(names) ** 0.5
    d_hip = np.array([(got[k] - ref[k]).norm().item() / max(ref[k].norm().item(), floor) for k in names])
    d_ref = np.maximum(g16["grad_dist"], 2e-3)
    ratio = d_hip / d_ref
    e_loss, ref_loss = abs(loss.item() - float(g32["loss"])) / float(g32["loss"]), abs(float(g16["loss"]) - float(g16["loss_fp32"])) / float(g16["loss_fp32"])
    iw = int(ratio.argmax())
    report(f"unet_bf16_vs_reference_autocast/{case}", hip_out_vs_fp32_golden=e_out, reference_autocast_out_vs_fp32=ref_out,
           hip_out_vs_reference_autocast=e_vs_autocast, hip_flat_grad_vs_fp32=e_flat, reference_autocast_flat_grad_vs_fp32=ref_flat,
           hip_loss_rel=e_loss, reference_autocast_loss_rel=ref_loss, per_param_ratio_max=ratio.max(), per_param_ratio_median=float(np.median(ratio)),
           worst_ratio_param=names[iw])
    assert e_out < 1.5 * ref_out, (e_out, ref_out)
    assert e_flat < 1.5 * ref_flat, (e_flat, ref_flat)
    assert e_vs_autocast < 2.0 * ref_out                        # two bf16 roundings of one fp32 function: ~sqrt(2) x apart
    assert e_loss < max(3 * ref_loss, 1e-3)
    assert ratio.max() < 2.5, (names[iw], d_hip[iw], d_ref[iw])
    assert float(np.median(ratio)) < 1.25


def test_masked_loss_ragged_batch_and_length_assert(golden_dir):
    """trainer.py:74-95 pads a batch to its longest sample and passes orig_len; diffusion.py:104-110 masks the loss with it and
    diffusion.py:86 raises AssertionError on a length mismatch (which trainer.py:296-299 catches to skip the batch)."""
    meta, cfgd, model = _build_model("unet_tiny", golden_dir)
    cfg = O.UNetConfig(**cfgd)
    p = O.make_params(cfg, prefix="unet.")
    B_, L = meta["B"], meta["L"]
    x, a, c, t, noise = (torch.from_numpy(v) for v in synth_inputs("ragged", B_, L))
    orig = torch.tensor([L, L // 2 - 5][:B_])
    for b in range(B_):                                                  # what collate_fn produces
        x[b, :, orig[b]:] = -1.0
        a[b, :, orig[b]:] = -23.0
    ref = DO.training_loss(p, cfg, x, a, c, noise, t, cond_drop_prob=0.0, orig_len=orig)
    ref_unmasked = DO.training_loss(p, cfg, x, a, c, noise, t, cond_drop_prob=0.0)
    with oa.forced_compute_dtype(torch.float32):
        loss = model.loss_with(x.to(DEV), a.to(DEV), c.to(DEV), noise.to(DEV), t.to(DEV), orig_len=orig.to(DEV), cond_drop_prob=0.0)
        loss.backward()
    assert abs(loss.item() - ref.item()) < TOL * abs(ref.item())
    assert abs(ref.item() - ref_unmasked.item()) > 3 * TOL * abs(ref.item())           # the mask matters in this fixture
    g = model.unet.final_conv.weight.grad
    assert g is not None and torch.isfinite(g).all() and g.abs().max() > 0
    with pytest.raises(AssertionError):
        model(x.to(DEV), a[..., : L - 16].contiguous().to(DEV), c.to(DEV))


def test_gradient_checkpointing_matches_plain_backward(golden_dir):
    """UNet.set_gradient_checkpointing (unet.py:452-456, reentrant checkpoint of every UNetBlock body, unet.py:260-261): same loss
    and gradients as the plain backward (fp32 compute; differences are summation order only)."""
    meta, cfgd, model = _build_model("unet_tiny", golden_dir)
    x, a, c, t, noise = (T(v) for v in synth_inputs("unet_tiny", meta["B"], meta["L"]))
    model.train()
    with oa.forced_compute_dtype(torch.float32):
        l0 = model.loss_with(x, a, c, noise, t, cond_drop_prob=0.0)
        l0.backward()
    ref = {k: q.grad.detach().clone() for k, q in model.named_parameters()}
    for q in model.parameters():
        q.grad = None
    model.unet.set_gradient_checkpointing(True)
    assert any(getattr(m, "gradient_checkpointing", False) for m in model.modules())
    with oa.forced_compute_dtype(torch.float32):
        l1 = model.loss_with(x, a, c, noise, t, cond_drop_prob=0.0)
        l1.backward()
    assert abs(l0.item() - l1.item()) < 1e-5 * abs(l0.item())
    gmax = max(v.abs().max().item() for v in ref.values())
    errs = {k: ((q.grad - ref[k]).abs().max() / (ref[k].abs().max() + 1e-4 * gmax)).item() for k, q in model.named_parameters()}
    worst_k = max(errs, key=errs.get)
    report("gradient_checkpointing_vs_plain", max_rel=errs[worst_k])
    assert errs[worst_k] < 2e-2, (worst_k, errs[worst_k], sorted(errs, key=errs.get)[-8:])   # noise floor as in the direct-accumulation test


def test_direct_grad_accumulation_matches_autograd(golden_dir):
    """Trainer path (kernels add straight into the flat .grad buffer, autograd sees None) == plain autograd gradients.
    fp32 compute so that only summation order differs; errors are measured against each tensor's own scale plus a floor at
    1e-4 of the largest gradient (se.to_k.bias gradients are mathematically zero: softmax is shift-invariant)."""
    from osufusion_amd.train import Trainer
    meta, cfgd, model = _build_model("unet_tiny", golden_dir)
    x, a, c, t, noise = (T(v) for v in synth_inputs("unet_tiny", meta["B"], meta["L"]))
    with oa.forced_compute_dtype(torch.float32):
        model.loss_with(x, a, c, noise, t, cond_drop_prob=0.0).backward()
    ref = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
    gmax = max(v.abs().max().item() for v in ref.values())
    try:
        trainer = Trainer(model, compute_dtype=torch.float32)           # re-homes params/grads, enables the direct path
        trainer.flat.zero_grad()
        with oa.forced_compute_dtype(torch.float32):
            model.loss_with(x, a, c, noise, t, cond_drop_prob=0.0).backward()
        torch.cuda.synchronize()
        worst, worst_k = 0.0, ""
        for k, p in model.named_parameters():
            assert trainer.flat.grad.data_ptr() <= p.grad.data_ptr() < trainer.flat.grad.data_ptr() + 4 * trainer.flat.numel
            e = ((p.grad - ref[k]).abs().max() / (ref[k].abs().max() + 1e-4 * gmax)).item()
            if e > worst:
                worst, worst_k = e, k
        report("direct_grad_vs_autograd", max_rel=worst)
        assert worst < 2e-2, worst_k                                      # noise floor (atomics order -> bf16 attention flips); a layout error is O(1)
        loss, gn = trainer.step(x, a, c, noise, t)                       # and one fused optimizer step on the flat buffers
        assert torch.isfinite(loss).item() and torch.isfinite(gn).item()
    finally:
        Fn.enable_direct_grads(False)


def test_rectified_flow_vs_oracle(golden_dir):
    """Rectified-flow wrapper (rectified_flow.py:57-111): training loss + gradients and the 2*(S-1)-evaluation midpoint sampler."""
    from oracle import rectified_flow_oracle as RO
    from osufusion_amd.models.rectified_flow import OsuFusion as RFOsuFusion
    meta = json.loads((golden_dir / "unet_cases.json").read_text())["unet_tiny"]
    cfgd = {k: (tuple(v) if isinstance(v, list) else v) for k, v in meta["cfg"].items()}
    kw = {k: v for k, v in cfgd.items() if not k.startswith("dim_in_")}
    model = RFOsuFusion(kw.pop("dim_h"), **kw).to(DEV)
    load_pattern(model.unet)
    assert model.sample_timesteps == 16 and model.cond_drop_prob == 0.5
    cfg = O.UNetConfig(**cfgd)
    p = {"unet." + k: v.requires_grad_() for k, v in O.make_params(cfg).items()}
    x, a, c, t, noise = (torch.from_numpy(v) for v in synth_inputs("rf", 2, 256))
    times = torch.tensor([0.3, 0.85])
    ref = RO.training_loss(p, cfg, x, a, c, noise, times, cond_drop_prob=0.0)
    ref.backward()
    with oa.forced_compute_dtype(torch.float32):
        got = model.loss_with(x.to(DEV), a.to(DEV), c.to(DEV), noise.to(DEV), times.to(DEV), cond_drop_prob=0.0)
        got.backward()
    assert abs(got.item() - ref.item()) < 1e-3 * abs(ref.item())
    gref = torch.stack([p["unet." + k].grad.norm() for k, _ in model.unet.named_parameters()])
    ggot = torch.stack([v.grad.norm().cpu() for _, v in model.unet.named_parameters()])
    assert ((ggot - gref).abs() / (gref + 1e-3 * gref.max())).max() < 2e-2
    model.sample_timesteps = 4
    with torch.no_grad():
        for cs in (1.0, 2.0):
            want = RO.sample({k: v.detach() for k, v in p.items()}, cfg, a, c, noise.clone(), sampling_steps=4, cond_scale=cs)
            with oa.forced_compute_dtype(torch.float32):
                have = model.sample(a.to(DEV), c.to(DEV), noise.to(DEV), cond_scale=cs)
            e = rell2(have, want)
            report(f"rf_midpoint_3step/cond_scale_{cs}", rel_l2=e)
            assert e < 1e-2, cs


def test_sampler_vs_oracle(golden_dir):
    meta, cfgd, model = _build_model("unet_tiny", golden_dir)
    cfg = O.UNetConfig(**cfgd)
    p = {"unet." + k: v for k, v in O.make_params(cfg).items()}
    model.sampling_timesteps = 5
    x, a, c, t, noise = (torch.from_numpy(v) for v in synth_inputs("sampler", 2, 256))
    for cs in (1.0, 2.0):
        ref = DO.sample(p, cfg, a, c, noise.clone(), sampling_steps=5, cond_scale=cs)
        with oa.forced_compute_dtype(torch.float32):
            got = model.sample(a.to(DEV), c.to(DEV), noise.to(DEV), cond_scale=cs)
        e = rell2(got, ref)
        report(f"ddim_5step/cond_scale_{cs}", rel_l2=e)
        # 5 chained steps with clip_sample: per-step eps errors sit at the reference's own bf16-attention noise floor and the
        # clamp amplifies them ~3x per late step, so the trajectory bound is looser than the single-forward bound
        assert e < 3e-2, cs
