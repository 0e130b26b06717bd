"""GPU parity tests added in round 2 (run with -m gpu on an MI355X), all through the C ABI:
  * every attention-backward kernel (plain / software-pipelined dQ, plain / pipelined / query-split dK/dV) FORCED on every
    shape, including the N = 2048 / 4096 shapes the benchmark runs, against autograd of the fp32 formula
    (attention.py:87-101, unet.py:125-141);
  * clip_grad_norm_ + AdamW of the train step (trainer.py:305-307) through osuf_sqnorm / osuf_clip_coef / osuf_adamw;
  * UNet.forward_with_cond_scale (unet.py:458-465), Attend (attention.py:84-101), OsuFusion.set_full_bf16 (diffusion.py:56-57);
  * the sampler is bit-reproducible, and a hipGraph-replayed step equals the eager one (diffusion.py:59-77).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import osufusion_amd as oa
    from osufusion_amd import functional as Fn
    from osufusion_amd import ops

from oracle import diffusion_oracle as DO
from oracle import unet_oracle as O
from tests.attn_reference import bwd_cases
from tests.test_hip_parity import DEV, _build_model, rell2, relmax, report


# ---- attention backward: every kernel on every shape ---------------------------------------------------------
def _attn_case(Bn, N, H, D=64):
    qkv = torch.randn(Bn, N, (H + 2) * D, device=DEV).to(torch.bfloat16)
    do = torch.randn(Bn, N, H * D).to(torch.bfloat16)
    qkv32 = qkv.float().cpu().requires_grad_()
    q = qkv32[..., : H * D].view(Bn, N, H, D).permute(0, 2, 1, 3)
    k = qkv32[..., H * D: (H + 1) * D][:, None]
    v = qkv32[..., (H + 1) * D:][:, None]
    s = (q @ k.transpose(-1, -2)) * D ** -0.5
    o_ref = (s.softmax(-1) @ v).permute(0, 2, 1, 3).reshape(Bn, N, H * D)
    o_ref.backward(do.float())
    return qkv, do.to(DEV), o_ref.detach(), qkv32.grad


def test_fused_attention_backward_beyond_eight_samples():
    """B = 9, H = 16, N = 512: the fused sweep places sample b = (qid / nkb) * 8 + xcd (attn.hip), so b >= 8 is a second pass of the
    block-index map that the B <= 2 cases never reach -- checked against autograd of the fp32 formula like the rest."""
    Bn, N, H, D = 9, 512, 16, 64
    qkv, do, o_ref, g_ref = _attn_case(Bn, N, H)
    o, lse = ops.mqa_fwd(qkv, Bn, N, H, D, torch.bfloat16, D ** -0.5)
    assert rell2(o.float(), o_ref) < 5e-3
    for name, variant, qsplit in (("fused", ops.ATTN_FUSED, 0), ("fused-split2", ops.ATTN_FUSED, 2), ("fused-slabs", ops.ATTN_FUSED_SLABS, 0),
                                  ("auto", ops.ATTN_AUTO, 0), ("fused512", ops.ATTN_FUSED512, 1), ("fused512-split4", ops.ATTN_FUSED512, 4),
                                  ("fused512a", ops.ATTN_FUSED512A, 1), ("fused512a-split4", ops.ATTN_FUSED512A, 4)):
        dqkv = ops.mqa_bwd(qkv, o, do, lse, Bn, N, H, D, D ** -0.5, variant=variant, qsplit=qsplit)
        for bi in range(Bn):                                               # per sample: a mis-placed sample is an O(1) error on it alone
            e = rell2(dqkv[bi], g_ref[bi])
            assert e < 1e-2, (name, bi, e)
        report(f"attn_bwd/B9_H16_N512/{name}", rel_l2=rell2(dqkv, g_ref))


@pytest.mark.parametrize("N", [200, 512, 2048, 4096])
def test_every_attention_backward_kernel_vs_fp32_autograd(N):
    """N = 2048 / 4096 are the shapes at which the train step picks mqa_bwd_dq_pipe_kernel and the unsplit
    mqa_bwd_dkv_pipe_kernel; N = 200 forces the pipelined kernels through a ragged last tile; qsplit forces the split path."""
    H, D = 4, 64
    Bn = 2 if N <= 512 else 1
    qkv, do, o_ref, g_ref = _attn_case(Bn, N, H)
    o, lse = ops.mqa_fwd(qkv, Bn, N, H, D, torch.bfloat16, D ** -0.5)
    assert rell2(o.float(), o_ref) < 5e-3                              # bf16 P and bf16 output rounding
    # the variant list is shared with tests/test_attn_exact_gpu.py: 9 kernels that take any N, the 4-wave 512-keys-per-workgroup sweep (round 3: whole
    # query blocks) and the same sweep with its generated, hand-placed loop (round 4: whole 512-key blocks)
    cases = bwd_cases(ops, N)
    outs = {}
    for name, variant, qsplit in cases:
        dqkv = ops.mqa_bwd(qkv, o, do, lse, Bn, N, H, D, D ** -0.5, variant=variant, qsplit=qsplit)
        e2, em = rell2(dqkv, g_ref), relmax(dqkv, g_ref)
        for part, sl in (("dq", slice(0, H * D)), ("dk", slice(H * D, (H + 1) * D)), ("dv", slice((H + 1) * D, (H + 2) * D))):
            ep = rell2(dqkv[..., sl], g_ref[..., sl])
            report(f"attn_bwd/N{N}/{name}/{part}", rel_l2=ep)
            assert ep < 1e-2, (name, part, ep)                         # bf16 P / dS operands, fp32 accumulation
        assert e2 < 1e-2 and em < 3e-2, (name, e2, em)
        outs[name] = dqkv
    # the kernels differ only in schedule / summation order
    assert rell2(outs["plain"], outs["pipe-unsplit"]) < 2e-3
    if "fused512a" in outs:
        # the hand-placed loop keeps every fragment map and the order of every accumulation of the compiled 512-key sweep: dK / dV bit for bit,
        # dQ up to the order of its float atomics
        for a_, b_ in (("fused512a", "fused512"), ("fused512a-split2", "fused512-split2")):
            assert torch.equal(outs[a_][..., H * D:], outs[b_][..., H * D:]), a_
            assert rell2(outs[a_][..., :H * D], outs[b_][..., :H * D]) < 1e-5, a_
    # the slab path adds the key blocks' partial dQ in a fixed order: bit-reproducible
    assert torch.equal(outs["fused-slabs"], ops.mqa_bwd(qkv, o, do, lse, Bn, N, H, D, D ** -0.5, variant=ops.ATTN_FUSED_SLABS))
    # fused RoPE-transpose epilogue of the pipelined kernels == the stand-alone rope_bwd kernel on their fp32 result
    cos, sin = Fn.rope_tables(N, D, 2 * N, DEV)
    for name, variant, qsplit in cases[2:4] + cases[5:]:
        ref_r = ops.rope_bwd(outs[name], torch.bfloat16, cos, sin, N, H + 1, H + 2, D)
        got_r = ops.mqa_bwd(qkv, o, do, lse, Bn, N, H, D, D ** -0.5, torch.bfloat16, cos, sin, variant=variant, qsplit=qsplit)
        assert relmax(got_r.float(), ref_r.float()) < 8e-3, name


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 2e-5), (torch.bfloat16, 1e-2)])
@pytest.mark.parametrize("Bn,L,H,K", [(2, 200, 2, 96), (3, 64, 1, 40), (4, 4096, 16, 256)])     # 128^2-tile path (ragged M) and the 256^2 path
def test_gemm_rowdot_epilogue(dtype, tol, Bn, L, H, K):
    """osuf_gemm_nt_rowdot == osuf_gemm_nt followed by osuf_attn_delta (the to_out input gradient + sum_d dO * O of unet.py:141 /
    attention.py:94-99's backward), from one epilogue."""
    a = (torch.randn(Bn * L, K, device=DEV) * 0.5).to(dtype)
    w = (torch.randn(1, H * 64, K, device=DEV) / K ** 0.5).to(dtype)
    o = torch.randn(Bn, L, H * 64, device=DEV).to(torch.bfloat16).to(dtype)          # attention outputs hold bf16-rounded values
    c_ref = ops.gemm_nt(a, w, None)
    c, delta = ops.gemm_nt_rowdot(a, w, o, L, H)
    assert torch.equal(c.view_as(c_ref), c_ref)
    want = (c_ref.to(torch.bfloat16).float().view(Bn, L, H, 64) * o.float().view(Bn, L, H, 64)).sum(-1).permute(0, 2, 1)
    assert delta.shape == (Bn, H, L) and relmax(delta, want) < 1e-5
    d2 = torch.empty_like(delta)                                                       # and the stand-alone kernel it replaces
    ops.call("osuf_attn_delta", c_ref.to(torch.bfloat16).data_ptr(), H * 64, o.data_ptr(), H * 64, ops._DT[o.dtype], d2.data_ptr(), Bn, H, L, 64,
             torch.cuda.current_stream().cuda_stream)
    assert relmax(delta, d2) < 1e-5


def test_attention_backward_rejects_unknown_variant():
    qkv = torch.zeros(1, 64, 6 * 64, device=DEV, dtype=torch.bfloat16)
    o, lse = ops.mqa_fwd(qkv, 1, 64, 4, 64, torch.bfloat16, 0.125)
    with pytest.raises(RuntimeError, match="invalid argument"):
        ops.mqa_bwd(qkv, o, o, lse, 1, 64, 4, 64, 0.125, variant=99)
    # dq_mode 4 was the no-atomics timing build of the 512-key sweep (since removed): the number stays refused, and sizes no workspace
    from osufusion_amd import _lib
    assert _lib.load().osuf_mqa_bwd_fused_workspace_bytes(1, 4, 64, 0, 0, 4) == 0
    dqkv, ws = torch.empty(1, 64, 6 * 64, device=DEV), torch.empty(1 << 16, device=DEV)
    delta = torch.zeros(1, 4, 64, device=DEV)
    q, st = qkv.data_ptr(), torch.cuda.current_stream().cuda_stream
    with pytest.raises(RuntimeError, match="invalid argument"):
        ops.call("osuf_mqa_bwd_fused", q, 384, q + 512, 384, q + 640, 384, o.data_ptr(), 256, lse.data_ptr(), delta.data_ptr(), dqkv.data_ptr(), 384,
                 dqkv.data_ptr() + 1024, dqkv.data_ptr() + 1280, 384, 1, 4, 64, 64, 0.125, 0, None, None, ws.data_ptr(), ws.numel() * 4, 0, 4, st)


# ---- clip + AdamW (trainer.py:305-307) -----------------------------------------------------------------------
@pytest.mark.parametrize("max_norm", [0.0, 0.05, 1e4])                 # no clipping / clipping active / threshold not reached
@pytest.mark.parametrize("world", [1, 4])
def test_clip_and_adamw_match_torch(max_norm, world):
    from osufusion_amd.train import FlatParameters, FusedAdamW
    torch.manual_seed(3)
    model = torch.nn.Sequential(torch.nn.Linear(37, 19), torch.nn.Linear(19, 5)).to(DEV)
    ref = torch.nn.Sequential(torch.nn.Linear(37, 19), torch.nn.Linear(19, 5)).to(DEV)
    ref.load_state_dict(model.state_dict())
    try:
        flat = FlatParameters(model, align=4)
        opt = FusedAdamW(flat, lr=1e-2, weight_decay=1e-2)
        topt = torch.optim.AdamW(ref.parameters(), lr=1e-2, weight_decay=1e-2)
        for step in range(3):
            gsum = [torch.randn_like(p) * (1.0 + step) for p in ref.parameters()]          # what a SUM all-reduce leaves behind
            for p, g in zip(model.parameters(), gsum):
                p.grad.copy_(g)
            for p, g in zip(ref.parameters(), gsum):
                p.grad = g / world                                                         # DDP's averaged gradient
            if max_norm > 0:
                tn_ref = torch.nn.utils.clip_grad_norm_(ref.parameters(), max_norm)
            else:
                tn_ref = torch.linalg.vector_norm(torch.stack([p.grad.norm() for p in ref.parameters()]))
            topt.step()
            tn = opt.step(grad_scale=1.0 / world, clip_grad_norm=max_norm)
            assert abs(tn.item() - tn_ref.item()) < 1e-5 * tn_ref.item()
            for p, q in zip(model.parameters(), ref.parameters()):
                assert torch.allclose(p, q, rtol=1e-5, atol=1e-6), (step, max_norm, world)
    finally:
        Fn.enable_direct_grads(False)


# ---- public API pieces without a test in round 1 --------------------------------------------------------------
def test_forward_with_cond_scale_vs_oracle(golden_dir):
    """unet.py:458-465: null + (cond - null) * s from two sequential forwards (the sampler batches them; this is the method)."""
    from osufusion_amd.pattern import synth_inputs
    meta, cfgd, model = _build_model("unet_tiny", golden_dir)
    cfg = O.UNetConfig(**cfgd)
    p = O.make_params(cfg)
    x, a, c, t, _ = (torch.from_numpy(v) for v in synth_inputs("cfg", 2, 256))
    with torch.no_grad():
        cond = O.unet_forward(p, cfg, x, a, t, c, cond_drop_prob=0.0)
        null = O.unet_forward(p, cfg, x, a, t, c, cond_drop_prob=1.0)
        for s in (1.0, 2.5):
            want = cond if s == 1.0 else null + (cond - null) * s
            with oa.forced_compute_dtype(torch.float32):
                got = model.unet.forward_with_cond_scale(x.to(DEV), a.to(DEV), t.to(DEV), c.to(DEV), cond_scale=s)
            e = rell2(got, want)
            report(f"forward_with_cond_scale/{s}", rel_l2=e)
            # each branch sits at the reference's own bf16-attention noise floor (3.8e-4 on this net); guidance
            # extrapolates: err(null + s (cond - null)) <= (s + |s - 1|) x the per-forward error relative to a similar norm
            assert e < (1e-3 if s == 1.0 else 1e-3 * (2 * s - 1)), (s, e)


@pytest.mark.parametrize("N", [96, 1000])
def test_attend_module_vs_sdpa(N):
    """attention.py:84-101: q, k, v -> bf16, SDPA, back to the input dtype (fp32 in, fp32 out); K/V repeated over heads."""
    from osufusion_amd.modules.attention import Attend
    Bn, H, D = 2, 4, 64
    q = torch.randn(Bn, H, N, D, device=DEV)
    k1, v1 = torch.randn(Bn, 1, N, D, device=DEV), torch.randn(Bn, 1, N, D, device=DEV)
    k, v = k1.expand(Bn, H, N, D).contiguous(), v1.expand(Bn, H, N, D).contiguous()      # the GQA repeat of unet.py:135
    got = Attend()(q, k, v)
    assert got.dtype == q.dtype and got.shape == q.shape
    qb, kb, vb = (t.to(torch.bfloat16).float().cpu() for t in (q, k, v))
    want = F.scaled_dot_product_attention(qb, kb, vb).to(torch.bfloat16).float()
    assert rell2(got, want) < 5e-3 and relmax(got, want) < 1.5e-2
    assert torch.equal(got, Attend()(q, k1, v1))                                         # un-repeated single K/V head: same kernel
    kh, vh = torch.randn(Bn, H, N, D, device=DEV), torch.randn(Bn, H, N, D, device=DEV)  # a K/V head of its own per query head
    got = Attend()(q, kh, vh)
    want = F.scaled_dot_product_attention(qb, kh.to(torch.bfloat16).float().cpu(), vh.to(torch.bfloat16).float().cpu()).to(torch.bfloat16).float()
    assert rell2(got, want) < 5e-3 and relmax(got, want) < 1.5e-2
    # attn_mask (round 3, tests/test_round3_gpu.py): the reference's cast-to-bf16-and-add semantics -- an all-True bool mask adds 1.0 to every
    # score, which the softmax ignores
    ones = Attend()(q, k1, v1, attn_mask=torch.ones(N, N, device=DEV, dtype=torch.bool))
    assert rell2(ones, Attend()(q, k1, v1)) < 5e-3


def test_set_full_bf16_switches_every_kernel_to_bf16(golden_dir):
    """diffusion.py:56-57 casts the UNet to bf16; here the masters stay fp32 and all kernels compute in bf16: the output is
    that of a forced-bf16 run bit for bit, stays within the bf16 bound of the fp32 run, and the parameters keep their dtype."""
    from osufusion_amd.pattern import synth_inputs
    meta, cfgd, model = _build_model("unet_tiny", golden_dir)
    x, a, c, t, noise = (torch.from_numpy(v).to(DEV) for v in synth_inputs("fullbf16", 2, 256))
    with torch.no_grad(), ops.reproducible_mode(True):                # fixed-order reductions: two bf16 runs agree bit for bit
        with oa.forced_compute_dtype(torch.float32):
            y32 = model.unet(x, a, t, c)
        with oa.forced_compute_dtype(torch.bfloat16):
            y16 = model.unet(x, a, t, c)
            l16 = model.loss_with(x, a, c, noise, t, cond_drop_prob=0.0)
        model.set_full_bf16()
        ybf = model.loss_with(x, a, c, noise, t, cond_drop_prob=0.0)
    assert torch.equal(ybf, l16)
    assert all(p.dtype == torch.float32 for p in model.parameters())
    assert 1e-5 < rell2(y16, y32) < 2e-2


# ---- sampler: reproducible, graph == eager (diffusion.py:59-77, inference_gradio.py:105,128) ------------------------
@pytest.mark.parametrize("cond_scale", [1.0, 2.0])
def test_sampler_is_bit_reproducible_and_graph_equals_eager(golden_dir, cond_scale):
    from osufusion_amd.pattern import synth_inputs
    meta, cfgd, model = _build_model("unet_tiny", golden_dir)
    model.sampling_timesteps = 6
    x, a, c, t, noise = (torch.from_numpy(v).to(DEV) for v in synth_inputs("repro", 3, 256))
    with oa.forced_compute_dtype(torch.bfloat16):                      # the mode the sampler benchmark runs in
        s1 = model.sample(a, c, noise.clone(), cond_scale=cond_scale)
        s2 = model.sample(a, c, noise.clone(), cond_scale=cond_scale)
        assert torch.isfinite(s1).all() and torch.equal(s1, s2), "two eager calls of sample() must agree bit for bit"
        model.use_hip_graph = True
        g1 = model.sample(a, c, noise.clone(), cond_scale=cond_scale)
        g2 = model.sample(a, c, noise.clone(), cond_scale=cond_scale)
        model.use_hip_graph = False
    assert torch.equal(g1, g2) and torch.equal(g1, s1), "hipGraph replay of the step must equal the eager step"
    # the reproducible kernels are the same arithmetic as the training kernels up to summation order
    model.reproducible_sampling = False
    with oa.forced_compute_dtype(torch.float32):
        model.stop_after = 1
        fast = model.sample(a, c, noise.clone(), cond_scale=cond_scale)
        model.reproducible_sampling = True
        slow = model.sample(a, c, noise.clone(), cond_scale=cond_scale)
        model.stop_after = None
    assert rell2(fast, slow) < 1e-3


def test_reproducible_reductions_vs_atomic_ones():
    """osuf_gn_stats (fixed-order) vs the statistics fused into the GEMM epilogue; osuf_wcolsum with / without the partial buffer."""
    Bn, L, C = 3, 520, 96
    y = torch.randn(Bn, L, C, device=DEV) * 2 + 0.3
    for dt in (torch.float32, torch.bfloat16):
        yy = y.to(dt)
        mr = ops.gn_stats(yy, L)
        mean = yy.float().mean(dim=(1, 2))
        rstd = (yy.float().var(dim=(1, 2), unbiased=False) + 1e-5).rsqrt()
        assert torch.allclose(mr[:, 0], mean, atol=1e-5) and torch.allclose(mr[:, 1], rstd, rtol=1e-5)
        assert torch.equal(mr, ops.gn_stats(yy, L))
        # round 5: the second stage inside the apply kernel (osuf_gn_stats_parts + osuf_gn_apply_fwd_parts, the sampler's path): same statistics
        # (another fixed summation order: equal to rounding), same output as the two-kernel form fed those statistics, identical bits on every call
        g, bt = torch.randn(C, device=DEV), torch.randn(C, device=DEV)
        ss = torch.randn(Bn, 2 * C, device=DEV) * 0.1
        for s_ in (ss, None):
            h2, mr2 = ops.gn_apply_reproducible(yy.reshape(Bn * L, C), g, bt, s_, L)
            assert torch.allclose(mr2, mr, rtol=1e-6, atol=1e-7)
            assert torch.equal(h2, ops.gn_apply(yy.reshape(Bn * L, C), mr2, g, bt, s_, L))
            h3, mr3 = ops.gn_apply_reproducible(yy.reshape(Bn * L, C), g, bt, s_, L)
            assert torch.equal(h2, h3) and torch.equal(mr2, mr3)
        w = torch.rand(Bn * L, device=DEV)
        want = (yy.float() * w.view(Bn, L, 1)).sum(1)
        atomic = ops.wcolsum(yy, None, w, Bn, L)
        with ops.reproducible_mode(True):
            det = ops.wcolsum(yy, None, w, Bn, L)
            assert torch.equal(det, ops.wcolsum(yy, None, w, Bn, L))
        assert relmax(det, want) < 1e-5 and relmax(atomic, want) < 1e-5


def test_trainer_gradient_accumulation_and_relayout(golden_dir):
    """trainer.py:293-309 with gradient_accumulation_steps = 2: two micro-batches of 2 give the gradient (and the clipped AdamW
    moments) of one batch of 4; the observed-order re-layout after the first optimizer step moves parameters, gradients and Adam
    moments together and makes the next backward complete its gradients in layout order."""
    from osufusion_amd.pattern import synth_inputs
    from osufusion_amd.train import Trainer
    x, a, c, t, noise = (torch.from_numpy(v).to(DEV) for v in synth_inputs("accum", 4, 256))

    def named(tr, buf):
        names = {id(p): n for n, p in tr.model.named_parameters()}
        return {names[id(p)]: buf[o:o + p.numel()].clone() for p, o in zip(tr.flat.params, tr.flat.offsets)}

    try:
        _, _, m1 = _build_model("unet_tiny", golden_dir)
        m1.cond_drop_prob = 0.0
        tr1 = Trainer(m1, lr=1e-3, clip_grad_norm=1.0, compute_dtype=torch.float32, reorder_buckets=False)
        _, n1 = tr1.step(x, a, c, noise, t)
        g1, m1st = named(tr1, tr1.flat.grad), named(tr1, tr1.opt.exp_avg)
        _, _, m2 = _build_model("unet_tiny", golden_dir)
        m2.cond_drop_prob = 0.0
        tr2 = Trainer(m2, lr=1e-3, clip_grad_norm=1.0, compute_dtype=torch.float32, gradient_accumulation_steps=2, reorder_buckets=True)
        first_layout = [id(p) for p in tr2.flat.params]
        _, n_a = tr2.step(x[:2], a[:2], c[:2], noise[:2], t[:2])
        assert n_a is None and tr2.opt.step_count == 0                 # accumulation-only micro-batch: no optimizer step
        _, n2 = tr2.step(x[2:], a[2:], c[2:], noise[2:], t[2:])
        assert tr2.opt.step_count == 1 and abs(n1.item() - n2.item()) < 2e-3 * n1.item()
        assert [id(p) for p in tr2.flat.params] != first_layout, "the completion order differs from reverse registration order"
        g2, m2st = named(tr2, tr2.flat.grad), named(tr2, tr2.opt.exp_avg)
        # tolerance: everything outside attention is exact fp32 here, but the reference's bf16 cast of q / k / v (attention.py:87-92)
        # turns last-bit differences of the projections (B = 4 vs 2 + 2 take different tile / split plans) into isolated 2^-9 jumps:
        # ~2e-4 rel-L2 run to run (noise floor).  Per parameter the error is taken relative to its largest element
        # or 1e-3 of the model's largest gradient element, whichever is larger (attention weights carry gradients 1e-4 of the rest)
        gmax = max(v.abs().max().item() for v in g1.values())
        mmax = max(v.abs().max().item() for v in m1st.values())
        for k in g1:
            assert (g2[k] / 2 - g1[k]).abs().max().item() <= 1e-2 * max(g1[k].abs().max().item(), 1e-3 * gmax), k   # 2 half-batch means = 2 x full mean
            assert (m2st[k] - m1st[k]).abs().max().item() <= 1e-2 * max(m1st[k].abs().max().item(), 1e-3 * mmax), k  # Adam moments moved along
        assert rell2(torch.cat([g2[k] / 2 for k in g1]), torch.cat([g1[k] for k in g1])) < 1e-3
        for p, o in zip(tr2.flat.params, tr2.flat.offsets):
            assert p.data_ptr() == tr2.flat.data.data_ptr() + 4 * o and p.grad.data_ptr() == tr2.flat.grad.data_ptr() + 4 * o
        tr2.step(x[:2], a[:2], c[:2], noise[:2], t[:2])
        tr2.step(x[2:], a[2:], c[2:], noise[2:], t[2:])
        assert tr2.reducer.order_log == list(range(len(tr2.flat.params))), "after the re-layout gradients complete in layout order"
        tr1.step(x, a, c, noise, t)
        e = rell2(torch.cat([v for v in named(tr2, tr2.flat.grad).values()]) / 2, torch.cat([named(tr1, tr1.flat.grad)[k] for k in named(tr2, tr2.flat.grad)]))
        assert e < 2e-2, e                                             # second step: same trajectory up to Adam's sign noise on ~0 gradients
    finally:
        Fn.enable_direct_grads(False)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
def test_grouped_weight_pack_equals_per_weight_pack(golden_dir, dt):
    """osuf_pack_weight_group (one launch for every plain master weight, run by Trainer.step after the optimizer) writes exactly
    what one osuf_pack_weight launch per weight writes, and leaves every refreshed cache entry valid for the updated parameters."""
    from osufusion_amd.pattern import synth_inputs
    from osufusion_amd.train import Trainer
    x, a, c, t, noise = (torch.from_numpy(v).to(DEV) for v in synth_inputs("packs", 2, 256))
    try:
        _, _, m = _build_model("unet_tiny", golden_dir)
        tr = Trainer(m, lr=1e-2, clip_grad_norm=1.0, compute_dtype=dt, reorder_buckets=False)
        tr.step(x, a, c, noise, t)                                     # registers the jobs (lazy packs) and ends with one grouped refresh
        jobs = [j for j in Fn._PACK_JOBS.values() if j.cache() is not None and j.dt == dt]
        assert len(jobs) >= 20
        before = {id(j): j.pair[0].clone() for j in jobs}
        calls = []
        orig = ops.call
        ops.call = lambda name, *args, **kw: (calls.append(name), orig(name, *args, **kw))[1]
        try:
            tr.step(x, a, c, noise, t)
        finally:
            ops.call = orig
        assert calls.count("osuf_pack_weight_group") == 1
        lazy = calls.count("osuf_pack_weight")
        assert lazy <= 8, f"{lazy} per-weight packs left in a steady-state step (derived weights only: merged stems, Parallel sum, head)"
        changed = 0
        for j in jobs:
            ent = j.cache()._d[j.key]
            assert ent[2] is j and ent[0][0] == Fn._WEIGHT_EPOCH            # valid for the parameters as they are now
            off = 0
            for w in j.ws:
                f, d = ops.pack_weight(w.detach(), dt, j.kind)
                O = w.shape[0]
                assert torch.equal(j.pair[0][:, off:off + O], f) and torch.equal(j.pair[1][:, :, off:off + O], d), j.key
                off += O
            changed += int(not torch.equal(before[id(j)], j.pair[0]))
        assert changed >= len(jobs) // 2                                # the optimizer did move the weights the table re-read
    finally:
        Fn.enable_direct_grads(False)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_linear_group_equals_per_linear_kernels(dt):
    """osuf_skinny_fwd_group / osuf_skinny_dx_group (the 35 FiLM projections of a UNet forward in one launch, residual.py:104-111)
    against the per-linear kernels: outputs bit-equal (same tile body), dx = the sum of the per-linear dx up to the order of the
    fp32 adds, weight / bias gradients through autograd equal to SkinnyLinearFn's."""
    torch.manual_seed(3)
    M, K = 32, 2048
    Ns = [512, 1536, 1024, 2048, 520, 8]
    x = (torch.randn(M, K, device=DEV) * 0.7).requires_grad_()
    lins = [torch.nn.Linear(K, N).to(DEV) for N in Ns]
    outs = Fn.film_group(x, lins, dt, ops.ACT_SILU)
    ys = [Fn.film_tap(outs[id(l.weight)]) for l in lins]
    gs = [torch.randn(M, N, device=DEV) for N in Ns]
    gs[4] = None                                                          # one output without a gradient
    torch.autograd.backward([y for y, g in zip(ys, gs) if g is not None], [g for g in gs if g is not None])
    dx_group, dws = x.grad.clone(), [l.weight.grad.clone() if l.weight.grad is not None else None for l in lins]
    dbs = [l.bias.grad.clone() if l.bias.grad is not None else None for l in lins]
    x.grad = None
    for l in lins:
        l.weight.grad = l.bias.grad = None
    refs = [Fn.SkinnyLinearFn.apply(x, l.weight, l.bias, dt, ops.ACT_SILU, 0) for l in lins]
    for y, r in zip(ys, refs):
        assert torch.equal(y, r)
    torch.autograd.backward([r for r, g in zip(refs, gs) if g is not None], [g for g in gs if g is not None])
    assert rell2(dx_group, x.grad) < 1e-6
    for i, l in enumerate(lins):
        if gs[i] is None:
            assert dws[i] is None and l.weight.grad is None
        else:
            assert torch.equal(dws[i], l.weight.grad) and torch.equal(dbs[i], l.bias.grad)


def test_grouped_film_weights_complete_with_their_blocks(golden_dir):
    """The grouped FiLM projections must not delay gradient completion (what the bucketed all-reduce overlaps with): each
    `mlp.1.weight` reports complete right after its own block's backward, not with the group node at the end of the backward."""
    from osufusion_amd.pattern import synth_inputs
    from osufusion_amd.train import Trainer
    x, a, c, t, noise = (torch.from_numpy(v).to(DEV) for v in synth_inputs("film", 2, 256))
    try:
        _, _, m = _build_model("unet_tiny", golden_dir)
        tr = Trainer(m, lr=1e-3, compute_dtype=torch.float32, reorder_buckets=False)
        calls = []
        orig = ops.call
        ops.call = lambda name, *args, **kw: (calls.append(name), orig(name, *args, **kw))[1]
        try:
            tr.step(x, a, c, noise, t)
        finally:
            ops.call = orig
        assert calls.count("osuf_skinny_fwd_group") == 1 and calls.count("osuf_skinny_dx_group") == 1
        names = {id(p): k for k, p in m.named_parameters()}
        order = [names[id(tr.flat.params[i])] for i in tr.reducer.order_log]
        assert len(order) == len(tr.flat.params) == len(set(order))          # every parameter reported exactly once
        ranks = [i for i, k in enumerate(order) if k.endswith(".mlp.1.weight")]
        assert len(ranks) >= 8
        assert ranks[0] < len(order) // 8 and ranks[len(ranks) // 2] < 3 * len(order) // 4, ranks
        # each FiLM weight completes right behind the first conv of its own block (block1's backward produces the FiLM gradient)
        for k in (k for k in order if k.endswith(".mlp.1.weight")):
            blk = k[: -len(".mlp.1.weight")]
            assert 0 < order.index(k) - order.index(blk + ".block1.proj.weight") <= 6, (k, order.index(k), order.index(blk + ".block1.proj.weight"))
    finally:
        Fn.enable_direct_grads(False)
