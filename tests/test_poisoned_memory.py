"""Every kernel's result must not depend on what its uninitialised memory held, and no kernel may write past the end of an allocation.

Each case below runs three times, under tests/memguard.py's guard with zero fill, with 0xFF (NaN) and with 0x7F (~3.4e38, finite) in every
torch.empty / torch.empty_like of the package (outputs, workspaces, operand packs; the module caches are dropped on entry so that they are
re-allocated poisoned), its own inputs placed at the front of guarded buffers too, and every allocation's tail slack checked afterwards:
  * deterministic outputs (forward kernels, packs, fixed-order reductions, split wgrads with partial tiles, the slab dQ sum) are bit-identical
    across the three runs;
  * outputs of atomic paths (fused dQ, GroupNorm / LayerNorm backward statistics, atomic wgrads) are finite and within the existing parity test's
    tolerance of a reference computed here.
Shapes are those of the parity tests (tests/test_hip_parity.py, test_round5_gpu.py): M / L off the tile, C a multiple of 8 but not of 64, small K
tails, N in {200, 512, 1024, 2048}.  The CPU test at the end requires a case (or a written exemption) for every allocating function of
osufusion_amd/ops.py and functional.py."""
import ast
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parent.parent
DEV = "cuda"
PATTERNS = (0x00, 0xFF, 0x7F)


def relmax(a, b):
    a, b = a.detach().double(), b.detach().double().to(a.device)
    assert a.shape == b.shape, (a.shape, b.shape)
    return ((a - b).abs().max() / (b.abs().max() + 1e-20)).item()


def rell2(a, b):
    a, b = a.detach().double(), b.detach().double().to(a.device)
    assert a.shape == b.shape, (a.shape, b.shape)
    return ((a - b).norm() / (b.norm() + 1e-20)).item()


def rnd(tag, shape, scale=1.0):
    """Deterministic CPU input (the same in all three runs)."""
    import zlib
    g = torch.Generator().manual_seed(zlib.crc32(f"{tag}{tuple(shape)}".encode()))
    return torch.randn(*shape, generator=g) * scale


class Case:
    """Collects what one run of a case produced: `bits` (compared bit for bit across the runs) and `near` (checked against a reference
    in every run).  Inputs come from `inp` (guarded placement on the GPU)."""

    def __init__(self, g) -> None:
        self.g, self.bits, self.near = g, {}, []

    def inp(self, t, dtype=None):
        return self.g.place(t.to(dtype) if dtype is not None else t)

    def eq(self, name, t):
        self.bits[name] = t

    def close(self, name, got, want, tol, metric=relmax):
        self.near.append((name, got, want, tol, metric))


_REFS = {}


def memo(key, fn):
    """A reference computed once per case (its inputs are the same in every run)."""
    if key not in _REFS:
        _REFS[key] = fn()
    return _REFS[key]


def run_case(fn):
    """The case under each pattern; every pattern's findings are reported (not only the first one's)."""
    from tests.memguard import guard
    runs, errors = {}, []
    for byte in PATTERNS:
        with guard(byte) as g:
            c = Case(g)
            fn(c)
            try:
                g.check()
                got = {k: v.detach().clone() for k, v in c.bits.items()}
                for name, t in got.items():
                    assert bool(torch.isfinite(t.float()).all()), f"pattern {byte:#04x}: {name} is not finite"
                for name, t, want, tol, metric in c.near:
                    assert bool(torch.isfinite(t.float()).all()), f"pattern {byte:#04x}: {name} is not finite"
                    e = metric(t, want)
                    assert e < tol, f"pattern {byte:#04x}: {name} off its reference by {e:.3e} (tolerance {tol:.1e})"
                runs[byte] = got
            except AssertionError as e:
                errors.append(str(e).split("\n")[0])
            g.release()
        torch.cuda.synchronize()
    first = next(iter(runs.values()), {})
    for byte, r in runs.items():
        for name in first:
            if not torch.equal(first[name], r[name]):
                errors.append(f"{name}: pattern {byte:#04x} changes the result (a read of uninitialised memory)")
    assert not errors, "; ".join(errors)


# ----------------------------------------------------------------------------------------------------------------------------------------
# GEMMs and packs
# ----------------------------------------------------------------------------------------------------------------------------------------
def conv_epilogue(kind, k, L, Cin, dtype, big=None):
    """conv_forward with every epilogue option (bias, SiLU, pre-activation copy, residual x per-sample scale, GroupNorm sums) and its input
    gradient with a residual -- the 128 x 128 kernel, or (big=1) the 256 x 256 ones forced onto the small shape."""
    def run(c):
        from osufusion_amd import functional as Fn, ops
        Cout, B = 328, 2
        Lout = {"same": L, "down": L // 2, "up": 2 * L}[kind]
        x = c.inp(rnd("x", (B, L, Cin)), dtype)
        w = c.inp(rnd("w", (Cout, Cin, k), (Cin * k) ** -0.5))
        bias = c.inp(rnd("b", (Cout,)))
        res = c.inp(rnd("r", (B, Lout, Cout)), dtype)
        rscale = c.inp(rnd("s", (B, Cout)).abs())
        with ops.force(**({} if big is None else {"gemm_big": big})):
            stats = torch.zeros(B, 2, dtype=torch.float64, device=DEV)
            y, pre = Fn.conv_forward(x, w, bias, Fn.PackCache(), kind, None, act=1, residual=res, rscale=rscale, stats=stats, want_pre=True)
            dx = Fn.conv_dgrad(y, w, Fn.PackCache(), kind, L, residual=x)
            y2 = Fn.conv_forward(x, w, None, Fn.PackCache(), kind, None)
        c.eq("y", y), c.eq("pre", pre), c.eq("dx", dx), c.eq("y_plain", y2)
        yd = y.double()                                                   # the sums are of the stored (rounded) outputs
        c.close("stats", stats, torch.stack([yd.sum((1, 2)), (yd * yd).sum((1, 2))], 1), 1e-5)
    return run


def plain_gemm(M, N, K, dtype, taps=1, slice_out=True):
    def run(c):
        from osufusion_amd import ops
        a = c.inp(rnd("a", (M, K)), dtype)
        w = c.inp(rnd("w", (taps, N, K), K ** -0.5), dtype)
        kw = dict(taps=taps, lin=M, lout=M, stride=1, pad=taps // 2) if taps > 1 else {}
        c.eq("c", ops.gemm_nt(a, w, None, **kw))
        if not slice_out:
            return
        out = torch.zeros(M, N + 24, dtype=dtype, device=DEV)            # a column slice of a wider buffer (row stride > width)
        ops.gemm_nt(a, w, c.inp(rnd("b", (N,))), out=out[:, :N], **kw)
        c.eq("c_slice", out)
    return run


def gemm_rowdot(c):
    from osufusion_amd import ops
    M, K, heads, L = 400, 136, 4, 200
    a = c.inp(rnd("a", (M, K)), torch.bfloat16)
    w = c.inp(rnd("w", (1, heads * 64, K), K ** -0.5), torch.bfloat16)
    o = c.inp(rnd("o", (M, heads * 64)), torch.bfloat16)
    out, delta = ops.gemm_nt_rowdot(a, w, o, L, heads)
    c.eq("out", out), c.eq("delta", delta)


def wgrad(B, L, N1, N2, k, dtype, with_bias=False, tol=1e-4):
    """gemm_tn (+ the fused bias column sums) vs fp64 on the same operands; bit-identical when the launch takes the fixed-order split plan
    (a workspace of partial tiles), to the tolerance of tests/test_hip_parity.py's wgrad checks on the atomic plans."""
    def run(c):
        from osufusion_amd import _lib, ops
        dy = c.inp(rnd("dy", (B, L, N1)), dtype)
        x = c.inp(rnd("x", (B, L, N2)), dtype)
        db = torch.zeros(N1, dtype=torch.float32, device=DEV) if with_bias else None
        got = ops.gemm_tn(dy, x, taps=k, lin=L, lout=L, stride=1, pad=k // 2, mode=0, n1=N1, bias_out=db)

        def ref():
            r = torch.zeros(k, N1, N2, dtype=torch.float64, device=DEV)
            xd, yd = x.double(), dy.double()
            for t in range(k):
                sh = t - k // 2
                lo, hi = max(0, -sh), min(L, L - sh)
                r[t] = torch.einsum("bmn,bmk->nk", yd[:, lo:hi], xd[:, lo + sh:hi + sh])
            return r, yd.sum((0, 1))
        want, wb = memo(("wgrad", B, L, N1, N2, k, dtype), ref)
        split = _lib.load().osuf_gemm_tn_workspace_bytes(ops.gemm_dt(dy), B * L, N1, N2, k) > 0
        if split and dtype == torch.bfloat16:                             # bf16-pair partial tiles: tests/test_round4_gpu.py's 3e-3 rel-L2
            c.close("dW", got, want, 3e-3, rell2)
        else:
            c.close("dW", got, want, tol)
        if with_bias:
            c.close("db", db, wb, 1e-5)
        if split and not with_bias:
            c.eq("dW", got)
    return run


def shared_workspace_reuse(c):
    """The split-wgrad workspace (ops._workspace: grown x5/4, shared, never cleared) first holds a smaller plan's partial tiles, then serves a larger one:
    the larger result must not depend on the stale tiles -- the "first call differs" shape of the sampler incident."""
    from osufusion_amd import _lib, ops
    shapes = ((2, 2048, 256, 256, 1), (2, 4096, 512, 256, 3))
    for i, (B, L, N1, N2, k) in enumerate(shapes):
        dy = c.inp(rnd(f"dy{i}", (B, L, N1)), torch.bfloat16)
        x = c.inp(rnd(f"x{i}", (B, L, N2)), torch.bfloat16)
        assert _lib.load().osuf_gemm_tn_workspace_bytes(ops.gemm_dt(dy), B * L, N1, N2, k) > 0
        c.eq(f"dW{i}", ops.gemm_tn(dy, x, taps=k, lin=L, lout=L, stride=1, pad=k // 2, mode=0, n1=N1))


def pack(kind, O, I, k, dtype):
    def run(c):
        from osufusion_amd import functional as Fn
        from osufusion_amd import ops
        w = c.inp(rnd("w", (O, I, k)))
        if k == 1:
            w = c.inp(w[:, :, 0].contiguous())
        fwd, dgr = ops.pack_weight(w, dtype, kind)
        c.eq("fwd", fwd), c.eq("dgrad", dgr)                               # ("down" / "up": the fourth dgrad tap comes from a k = 3 weight)
        if k == 1:
            w2 = c.inp(rnd("w2", (24, I)))
            f2, d2 = Fn.PackCache().packs(("t", dtype), (w, w2), (w, w2), "same", dtype)
            c.eq("fwd2", f2), c.eq("dgrad2", d2)
        # the grouped refresh writes the same bytes into existing destinations
        items = [(w, kind, fwd, dgr, 0)]
        tab, n, blocks = ops.pack_desc_table(items, dtype, DEV)
        fwd.zero_(), dgr.zero_()
        ops.pack_weight_group(tab, n, blocks, dtype)
        c.eq("fwd_group", fwd), c.eq("dgrad_group", dgr)
    return run


def adapted_pack(dora):
    def run(c):
        from osufusion_amd import ops
        O, I, k, r = 40, 72, 3, 8
        w = c.inp(rnd("w", (O, I, k), 0.1))
        a = c.inp(rnd("a", (r, I, k), 0.1))
        b = c.inp(rnd("b", (O, r, 1), 0.1))
        m = c.inp(rnd("m", (O,)).abs() + 0.5) if dora else None
        g, t32, t16 = ops.dora_gain(w, a, b, m, 0.5)
        weff, g2 = ops.dora_effective(w, a, b, m, 0.5)
        c.eq("g", g), c.eq("t32", t32), c.eq("t16", t16), c.eq("weff", weff), c.eq("g2", g2)
        fwd, dgr = ops.pack_weight(w, torch.bfloat16, "same", adapt=(a, b, g if dora else None, 0.5))
        c.eq("fwd", fwd), c.eq("dgrad", dgr)
    return run


# ----------------------------------------------------------------------------------------------------------------------------------------
# norms, pooling, gating
# ----------------------------------------------------------------------------------------------------------------------------------------
def gn_forward(B, L, C, dtype, film):
    def run(c):
        from osufusion_amd import ops
        y = c.inp(rnd("y", (B * L, C), 2.0) + 0.5, dtype)
        gamma = c.inp(rnd("g", (C,)) * 0.2 + 1)
        beta = c.inp(rnd("be", (C,)) * 0.2)
        ss = c.inp(rnd("ss", (B, 2 * C)) * 0.3) if film else None
        c.eq("mr_stats", ops.gn_stats(y, L))
        h, mr = ops.gn_apply_reproducible(y, gamma, beta, ss, L)
        c.eq("h_parts", h), c.eq("mr_parts", mr)
        c.eq("h", ops.gn_apply(y, mr, gamma, beta, ss, L))
        yd = y.double().view(B, L * C)
        st = c.inp(torch.stack([yd.sum(1), (yd * yd).sum(1)], 1).cpu())
        c.eq("mr_fin", ops.gn_finalize(st, L * C))
        h2, mr2 = ops.gn_apply_from_stats(y, st, gamma, beta, ss, L)
        c.eq("h_stats", h2), c.eq("mr_from_stats", mr2)
        c.close("mean", mr[:, 0], yd.mean(1), 1e-5)
    return run


def gn_backward(B, L, C, dtype, film, tol):
    """osuf_gn_bwd (atomic per-(b, c) sums) vs fp64 autograd of silu(GroupNorm(1, C)(y) * (1 + scale) + shift) (residual.py:75-84); the tolerance
    is tests/test_hip_parity.py::test_block_fn's."""
    def run(c):
        from osufusion_amd import ops
        y = c.inp(rnd("y", (B * L, C), 2.0) + 0.5, dtype)
        gamma = c.inp(rnd("g", (C,)) * 0.2 + 1)
        beta = c.inp(rnd("be", (C,)) * 0.2)
        ss = c.inp(rnd("ss", (B, 2 * C)) * 0.3) if film else None
        dh = c.inp(rnd("dh", (B * L, C)), dtype)
        mr = ops.gn_stats(y, L)
        dbias = torch.zeros(C, dtype=torch.float32, device=DEV)
        dy, dgamma, dbeta, dss = ops.gn_bwd(dh, y, mr, gamma, beta, ss, L, dbias_out=dbias)

        def ref():
            yd = y.double().view(B, L, C).requires_grad_()
            gd, bd = gamma.double().requires_grad_(), beta.double().requires_grad_()
            sd = ss.double().requires_grad_() if film else None
            z = F.group_norm(yd.transpose(1, 2), 1, gd, bd, eps=1e-5).transpose(1, 2)
            if film:
                z = z * (1 + sd[:, None, :C]) + sd[:, None, C:]
            F.silu(z).backward(dh.double().view(B, L, C))
            return yd.grad.view(B * L, C), gd.grad, bd.grad, (sd.grad if film else None), yd.grad.sum((0, 1))
        rdy, rg, rb, rss, rdb = memo(("gn_bwd", B, L, C, dtype, film), ref)
        c.close("dy", dy, rdy, tol), c.close("dgamma", dgamma, rg, tol), c.close("dbeta", dbeta, rb, tol), c.close("dbias", dbias, rdb, tol)
        if film:
            c.close("dss", dss, rss, tol)
    return run


def ln(M, C, dtype, tol):
    def run(c):
        from osufusion_amd import ops
        x = c.inp(rnd("x", (M, C), 2.0), dtype)
        gamma = c.inp(rnd("g", (C,)) * 0.2 + 1)
        beta = c.inp(rnd("be", (C,)) * 0.2)
        dy = c.inp(rnd("dy", (M, C)), dtype)
        out, mr = ops.ln_fwd(x, gamma, beta)
        c.eq("out", out), c.eq("mr", mr)
        dx, dgamma, dbeta = ops.ln_bwd(dy, x, mr, gamma)

        def ref():
            xd, gd, bd = x.double().requires_grad_(), gamma.double().requires_grad_(), beta.double().requires_grad_()
            F.layer_norm(xd, (C,), gd, bd, eps=1e-5).backward(dy.double())
            return xd.grad, gd.grad, bd.grad
        rx, rg, rb = memo(("ln", M, C, dtype), ref)
        c.close("dx", dx, rx, tol), c.close("dgamma", dgamma, rg, tol), c.close("dbeta", dbeta, rb, tol)
    return run


def pooling(B, L, C, dtype):
    def run(c):
        from osufusion_amd import ops
        h = c.inp(rnd("h", (B * L, C), 2.0), dtype)
        wk = c.inp(rnd("wk", (C,), 6.0 / C ** 0.5))
        bk = c.inp(rnd("bk", (1,)))
        pooled, p = ops.gca_pool(h, wk, bk, L)
        c.eq("pooled", pooled), c.eq("p", p)
        with ops.reproducible_mode(True):
            p2 = ops.rowdot(h, wk, bk, L)
            ops.softmax_rows_(p2, B, L)
            c.eq("p_rowdot", p2)
            c.eq("pooled_wcolsum", ops.wcolsum(h, None, p2, B, L))
            c.eq("wcolsum_bmul", ops.wcolsum(h, h, None, B, L))
        with ops.reproducible_mode(False):                                    # the training step's atomic column sums
            want = memo(("pool", B, L, C, dtype), lambda: (p2.double().view(B, L, 1) * h.double().view(B, L, C)).sum(1))
            c.close("wcolsum_atomic", ops.wcolsum(h, None, p2, B, L), want, 1e-4)
        gate = c.inp(torch.sigmoid(rnd("gate", (B, C))))
        res = c.inp(rnd("res", (B * L, C)), dtype)
        c.eq("gate_res", ops.gate_residual(h, gate, res, L)), c.eq("gate", ops.gate_residual(h, gate, None, L))
        c.eq("rowdot_ps", ops.rowdot(pooled, c.inp(rnd("dp", (B, C))), None, 1, per_sample=True))
    return run


def module_case(which, dtype, tol):
    """A residual-block Function end to end against the oracle's autograd, with tests/test_hip_parity.py's tolerances: the backward's atomic
    statistics and wgrads (BlockFn: gn_bwd, gemm_tn, colsum; GCAPoolFn + GateResFn: gca_bwd_apply, rowdot, gate_residual).  Nothing is compared
    bit for bit: the training forward's GroupNorm sums come from fp64 atomics in the GEMM epilogue, so even the output may differ in its last bit."""
    def run(c):
        from oracle import unet_oracle as O
        from osufusion_amd.modules import residual as R
        from tests.test_hip_parity import load_pattern
        torch.manual_seed(11)
        B = 2
        nm = O.Numerics("bf16" if dtype == torch.bfloat16 else "fp32")
        if which == "block":
            Cin, C, L = 40, 64, 136
            mod = load_pattern(R.Block(Cin, C).to(DEV))
            names = ("proj.weight", "proj.bias", "norm.weight", "norm.bias")
        else:
            Cin = C = 48
            L = 200
            mod = load_pattern(R.GlobalContext(C, C).to(DEV))
            names = ("to_k.weight", "layers.0.weight", "layers.0.bias", "layers.2.weight", "layers.2.bias")
        x = rnd("x", (B, Cin, L)).to(dtype).float()
        ss = rnd("ss", (B, 2 * C)) * 0.3
        g = rnd("g", (B, C, L)).to(dtype).float()
        res = rnd("res", (B, C, L)).to(dtype).float()

        def ref():
            p = {"m." + k: v.detach().cpu().clone().requires_grad_() for k, v in mod.state_dict().items()}
            xr, ssr = x.clone().requires_grad_(), ss.clone().requires_grad_()
            if which == "block":
                out = O.block(p, "m", xr, (ssr[:, :C, None], ssr[:, C:, None]), nm)
            else:
                out = xr * O.global_context(p, "m", xr, nm) + res
            out.backward(g)
            return out.detach(), xr.grad, ssr.grad, {k: p["m." + k].grad for k in names}
        rout, rx, rss, rp = memo(("module", which, dtype), ref)
        rows = c.inp(x.permute(0, 2, 1).contiguous(), dtype).requires_grad_()
        if which == "block":
            ssd = c.inp(ss).requires_grad_()
            out = mod.forward_rows(rows, ssd)
        else:
            from osufusion_amd import functional as Fn
            out = Fn.GateResFn.apply(rows, mod.gate_from_rows(rows), c.inp(res.permute(0, 2, 1).contiguous(), dtype))
        out.backward(c.inp(g.permute(0, 2, 1).contiguous(), dtype))
        c.close("out", out.detach().float().permute(0, 2, 1), rout, tol)
        c.close("dx", rows.grad.float().permute(0, 2, 1), rx, 3 * tol)
        if which == "block":
            c.close("dss", ssd.grad, rss, 3 * tol)
        for k, v in mod.named_parameters():
            if k in names:
                c.close(k, v.grad, rp[k], 5 * tol)
                v.grad = None
    return run


# ----------------------------------------------------------------------------------------------------------------------------------------
# attention
# ----------------------------------------------------------------------------------------------------------------------------------------
def _attn_ref(raw, do, B, N, H, G, D, cos=None, sin=None):
    """fp32 autograd of the attention formula on the same bf16 projections (RoPE half-split first when the tables are given): (o, dqkv)."""
    x = raw.float().cpu().requires_grad_()
    r = H // G

    def rot(t):
        if cos is None:
            return t
        c_, s_ = cos.cpu(), sin.cpu()
        h = D // 2
        t1, t2 = t[..., :h], t[..., h:]
        return torch.cat([t1 * c_[None, :, None] - t2 * s_[None, :, None], t2 * c_[None, :, None] + t1 * s_[None, :, None]], -1)
    q = rot(x[..., : H * D].view(B, N, H, D))
    k = rot(x[..., H * D:(H + G) * D].view(B, N, G, D))
    v = x[..., (H + G) * D:].view(B, N, G, D)
    outs = []
    for gi in range(G):
        sc = torch.einsum("bnhd,bmd->bhnm", q[:, :, gi * r:(gi + 1) * r], k[:, :, gi]) * D ** -0.5
        outs.append(torch.einsum("bhnm,bmd->bnhd", sc.softmax(-1), v[:, :, gi]).reshape(B, N, r * D))
    o = torch.cat(outs, -1)
    o.backward(do.float().cpu())
    return o.detach(), x.grad


def attention(B, N, H, G=1, D=64, variant=None, qsplit=0, qs=False, rope=False, out_dtype=torch.float32, zero_dq=None):
    """mqa_fwd (+ rope_cast) and mqa_bwd: forward bit-identical; dK / dV bit-identical on the fused sweeps and everything on the slab sweep
    (fixed-order dQ); dQ of the atomic sweeps and the dQ + dK/dV pair within the parity tests' 1e-2 rel-L2 of fp32 autograd.  zero_dq: "fwd" /
    "rope" -- the layer-private workspace cleared by the forward (mqa_fwd_zdq / mqa_fwd_rope) and handed to the backward."""
    def run(c):
        from osufusion_amd import functional as Fn
        from osufusion_amd import ops
        var = ops.ATTN_FUSED if variant is None else variant
        scale = D ** -0.5
        W = (H + 2 * G) * D
        raw = c.inp(rnd("raw", (B, N, W)), torch.bfloat16)
        do = c.inp(rnd("do", (B, N, H * D)), torch.bfloat16)
        cos = sin = None
        if rope or qs or zero_dq == "rope":
            cos, sin = Fn.rope_tables(N, D, 2 * N, DEV)
        ws = ops.fused_bwd_workspace(B, N, H, D, out_dtype, DEV, variant=var) if zero_dq else None
        assert (ws is not None) == bool(zero_dq)
        if zero_dq == "rope":
            qkv, o, lse = ops.mqa_fwd_rope(raw, cos, sin, B, N, H, D, torch.bfloat16, scale, write_q=True, zero_dq=ws)
            _, o2, lse2 = ops.mqa_fwd_rope(raw, cos, sin, B, N, H, D, torch.bfloat16, scale, write_q=False)
            c.eq("o_noq", o2), c.eq("lse_noq", lse2)
            qs_ = True
        else:
            if cos is not None:
                qkv = ops.rope_cast(raw, cos, sin, N, H + G, H + 2 * G, D, q_mul=scale * ops.LOG2E if qs else 1.0, n_q_heads=H)
            else:
                qkv = raw
            o, lse = ops.mqa_fwd(qkv, B, N, H, D, torch.bfloat16, scale, kv_heads=G, qs=qs, zero_dq=ws)
            qs_ = qs
        c.eq("qkv", qkv), c.eq("o", o), c.eq("lse", lse)
        dqkv = ops.mqa_bwd(qkv, o, do, lse, B, N, H, D, scale, out_dtype, cos, sin, variant=var, qsplit=qsplit, kv_heads=G, qs=qs_, workspace=ws)
        ro, rg = memo(("attn", B, N, H, G, D, bool(cos is not None)), lambda: _attn_ref(raw, do, B, N, H, G, D, cos, sin))
        c.close("o", o.float(), ro, 5e-3, rell2)
        dtol = 1e-2 if out_dtype == torch.float32 else 1.5e-2
        for nm, sl in (("dq", slice(0, H * D)), ("dk", slice(H * D, (H + G) * D)), ("dv", slice((H + G) * D, None))):
            c.close(nm, dqkv[..., sl].float(), rg[..., sl], dtol, rell2)
        fused = D == 64 and var in ops._FUSED_DQ_MODE
        if fused:
            c.eq("dkv", dqkv[..., H * D:])
            if var == ops.ATTN_FUSED_SLABS:
                c.eq("dq", dqkv[..., : H * D])
    return run


def rope_pair(c):
    from osufusion_amd import functional as Fn
    from osufusion_amd import ops
    B, N, H, D = 2, 200, 3, 64
    cos, sin = Fn.rope_tables(N, D, 2 * N, DEV)
    qkv32 = c.inp(rnd("q", (B * N, (H + 2) * D)))
    c.eq("cast", ops.rope_cast(qkv32, cos, sin, N, H + 1, H + 2, D))
    c.eq("cast_qs", ops.rope_cast(qkv32, cos, sin, N, H + 1, H + 2, D, q_mul=0.18, n_q_heads=H))
    for dt in (torch.float32, torch.bfloat16):
        c.eq(f"bwd_{dt}", ops.rope_bwd(qkv32, dt, cos, sin, N, H + 1, H + 2, D))


# ----------------------------------------------------------------------------------------------------------------------------------------
# layout, elementwise, scheduler, loss, small linears, audio
# ----------------------------------------------------------------------------------------------------------------------------------------
def layout(c):
    from osufusion_amd import ops
    B, C, L = 2, 72, 200
    x = c.inp(rnd("x", (B, C, L)))
    for dt in (torch.float32, torch.bfloat16):
        r = ops.ncl_to_rows(x, dt, 80)
        c.eq(f"rows_{dt}", r)                                              # all 80 columns: C..80 are zeroed by the kernel (the stem GEMM's K padding)
        c.eq(f"ncl_{dt}", ops.rows_to_ncl(r, C))
        c.eq(f"im2col_{dt}", ops.ncl_to_rows(x, dt, 3 * C, kt=3))
        rr = ops.cast_rows(r[..., :C], torch.bfloat16 if dt == torch.float32 else torch.float32)
        c.eq(f"cast_{dt}", rr)
        c.eq(f"add_{dt}", ops.add_rows(r, r))
        c.eq(f"copy_{dt}", ops.copy2d(r, torch.zeros(B, L, 96, dtype=dt, device=DEV), C))


def scheduler_and_loss(c):
    from osufusion_amd import ops
    x = c.inp(rnd("x", (4, 6, 100)))
    n = c.inp(rnd("n", (4, 6, 100)))
    null = c.inp(rnd("null", (4, 6, 100)))
    coef = c.inp(rnd("coef", (4, 4)).abs())
    c.eq("ddim", ops.ddim_step(x, n, null, 2.0, coef))
    c.eq("ddim_nocfg", ops.ddim_step(x, n, None, 1.0, coef))
    c.eq("axpby", ops.axpby_rows(x, n, coef[:, 0].contiguous(), coef[:, 1].contiguous()))
    ol = torch.tensor([100, 20, 35, 77], dtype=torch.int32)
    acc, grad = ops.mse(x, n, ol, True)
    c.eq("mse_grad", grad)
    mask = (torch.arange(100)[None] < ol[:, None].long()).double()[:, None].to(DEV)
    c.close("mse", acc, (((x.double() - n.double()) ** 2) * mask).sum().reshape(1), 1e-6)       # fp64 atomics of fp32 partial sums


def skinny(M, N, K, in_act, out_act, dtype, tol):
    """skinny_fwd / skinny_bwd through SkinnyLinearFn (dx, dW: fp32 atomics over K / M slices) vs fp64 autograd, test_skinny_linear_kernels' tolerances."""
    def run(c):
        from osufusion_amd import functional as Fn
        x = c.inp(rnd("x", (M, K)) * 1.5).requires_grad_()
        w = c.inp(rnd("w", (N, K), K ** -0.5)).requires_grad_()
        b = c.inp(rnd("b", (N,)) * 0.2).requires_grad_()
        gy = c.inp(rnd("g", (M, N)))
        y = Fn.SkinnyLinearFn.apply(x, w, b, dtype, in_act, out_act)
        y.backward(gy)
        c.eq("y", y.detach())

        def ref():
            xr, wr, br = (t.detach().double().requires_grad_() for t in (x, w, b))
            xin = F.silu(xr) if in_act else xr
            if dtype == torch.bfloat16:
                q = lambda t: t + (t.float().bfloat16().double() - t).detach()
                z = F.linear(q(xin), q(wr), br)
            else:
                z = F.linear(xin, wr, br)
            yr = torch.sigmoid(z) if out_act else z
            yr.backward(gy.double())
            return yr.detach(), xr.grad, wr.grad, br.grad
        ry, rx, rw, rb = memo(("skinny", M, N, K, in_act, out_act, dtype), ref)
        m = 1 if dtype == torch.float32 else 3
        c.close("y", y, ry, tol), c.close("dx", x.grad, rx, tol * m), c.close("dw", w.grad, rw, tol * m), c.close("db", b.grad, rb, 1e-5)
    return run


def linear_group(c):
    """FiLM projections as one group: skinny_fwd_group, and skinny_dx_group + per-linear skinny_bwd in LinearGroupFn.backward."""
    from osufusion_amd import functional as Fn
    M, K = 6, 96
    x = c.inp(rnd("x", (M, K))).requires_grad_()
    ws = [c.inp(rnd(f"w{i}", (n, K), K ** -0.5)).requires_grad_() for i, n in enumerate((128, 64, 256))]
    bs = [c.inp(rnd(f"b{i}", (w.shape[0],)) * 0.2).requires_grad_() for i, w in enumerate(ws)]
    ys = Fn.LinearGroupFn.apply(x, torch.float32, 1, False, *ws, *bs)
    gs = [c.inp(rnd(f"g{i}", tuple(y.shape))) for i, y in enumerate(ys)]
    torch.autograd.backward(ys, gs)

    def ref():
        xr = x.detach().double().requires_grad_()
        wr = [w.detach().double().requires_grad_() for w in ws]
        br = [b.detach().double().requires_grad_() for b in bs]
        yr = [F.linear(F.silu(xr), w, b) for w, b in zip(wr, br)]
        torch.autograd.backward(yr, [g.double() for g in gs])
        return [y.detach() for y in yr], xr.grad, [w.grad for w in wr], [b.grad for b in br]
    ry, rx, rw, rb = memo(("group",), ref)
    for i, y in enumerate(ys):
        c.eq(f"y{i}", y.detach())
        c.close(f"y{i}", y, ry[i], 2e-5), c.close(f"dw{i}", ws[i].grad, rw[i], 2e-5), c.close(f"db{i}", bs[i].grad, rb[i], 1e-5)
    c.close("dx", x.grad, rx, 2e-5)


def adapter(c):
    """A DoRA conv (AdaptedConvFn) forward + backward: adapter_grads' dA / dB / dm (not direct: the fresh tensors) against fp64 autograd of
    conv(x, g (W + s B A)) with g = m / ||W + s B A|| (norm detached, as peft's DoRA)."""
    from osufusion_amd import functional as Fn
    B, L, Cin, O, k, r, s = 2, 136, 40, 64, 3, 8, 0.5
    x = c.inp(rnd("x", (B, L, Cin))).requires_grad_()
    w = c.inp(rnd("w", (O, Cin, k), (Cin * k) ** -0.5))
    bias = c.inp(rnd("bias", (O,)) * 0.1)
    la = c.inp(rnd("a", (r, Cin, k), 0.1)).requires_grad_()
    lb = c.inp(rnd("b", (O, r, 1), 0.1)).requires_grad_()
    lm = c.inp(rnd("m", (O, 1, 1)).abs() + 0.5).requires_grad_()
    ad = Fn.Adapter(w, la, lb, lm, s)
    y = Fn.AdaptedConvFn.apply(x, bias, Fn.PackCache(), "same", ad, la, lb, lm)
    dy = c.inp(rnd("dy", tuple(y.shape)))
    y.backward(dy)
    c.eq("y", y.detach())

    def ref():
        xr, ar, br, mr = (t.detach().double().requires_grad_() for t in (x, la, lb, lm))
        weff = w.double() + s * torch.einsum("or,rik->oik", br[:, :, 0], ar)
        weff = weff * (mr.view(O, 1, 1) / weff.norm(dim=(1, 2), keepdim=True).detach())    # the norm is detached (lora_layers.py:16-26)
        yr = F.conv1d(xr.permute(0, 2, 1), weff, bias.double(), padding=1).permute(0, 2, 1)
        yr.backward(dy.double())
        return xr.grad, ar.grad, br.grad, mr.grad
    rx, ra, rb, rm = memo(("adapter",), ref)
    c.close("dx", x.grad, rx, 2e-5), c.close("dA", la.grad, ra, 1e-4), c.close("dB", lb.grad, rb, 1e-4), c.close("dm", lm.grad, rm, 1e-4)


def audio(c):
    from osufusion_amd import ops
    sig = c.inp(rnd("sig", (4099,)))
    taps = c.inp(rnd("taps", (31,), 0.1))
    c.eq("fir", ops.fir_decimate2(sig, taps))
    c.eq("frames", ops.frame_rows(sig, 64, 256, 70))
    bins, K, hop = 12, 256, 64
    wave = c.inp(rnd("wave", (hop * 40 + K,)))
    bank = c.inp(rnd("bank", (2 * bins, K), 0.05))
    sc = c.inp(rnd("sc", (bins,)).abs() + 0.5)
    c.eq("vqt", ops.log_vqt(wave, bank, sc, hop, 41))


def cast(c):
    from osufusion_amd import ops
    src = c.inp(rnd("src", (1027,)))
    c.eq("bf16", ops.cast_f32_bf16(src, torch.empty(1027, dtype=torch.bfloat16, device=DEV)))


BF, F32 = torch.bfloat16, torch.float32
# ops / functional function -> [(variant, case)]
CASES = {
    "gemm_nt": [("conv_same_k3_bf16", conv_epilogue("same", 3, 200, 72, BF)), ("conv_same_k3_f32", conv_epilogue("same", 3, 200, 72, F32)),
                ("conv_down_bf16", conv_epilogue("down", 3, 96, 72, BF)), ("conv_up_f32", conv_epilogue("up", 3, 56, 72, F32)),
                ("conv_k15_bf16", conv_epilogue("same", 15, 64, 72, BF)),
                ("big256_same_k3", conv_epilogue("same", 3, 200, 64, BF, big=1)), ("big256_8phase_k1", conv_epilogue("same", 1, 264, 192, BF, big=1)),
                ("big256_down", conv_epilogue("down", 3, 96, 128, BF, big=1)), ("big256_up", conv_epilogue("up", 3, 56, 64, BF, big=1)),
                ("plain_ragged_bf16", plain_gemm(133, 200, 136, BF)), ("plain_ragged_f32", plain_gemm(133, 200, 136, F32)),
                ("skinny_n_taps", plain_gemm(4100, 16, 328, BF, taps=3, slice_out=False)), ("plain_k_tail", plain_gemm(70, 24, 48, F32))],
    "gemm_nt_rowdot": [("heads4_L200", gemm_rowdot)],
    "gemm_tn": [("split_bf16", wgrad(2, 4096, 512, 256, 3, BF)), ("split_bf16_k1", wgrad(2, 2048, 256, 256, 1, BF)),
                ("bias_bf16", wgrad(2, 2048, 256, 256, 1, BF, with_bias=True)),
                ("skinny_atomic", wgrad(3, 1500, 328, 32, 3, BF)), ("ragged_f32", wgrad(2, 200, 72, 40, 3, F32)),
                ("ragged_bf16_odd", wgrad(2, 136, 328, 72, 1, BF, tol=1e-4))],
    "_workspace": [("stale_partial_tiles", shared_workspace_reuse)],
    "_pack_geometry": [(f"{kind}_{O}x{I}x{k}_{str(dt)[6:]}", pack(kind, O, I, k, dt)) for kind, O, I, k in
                       (("same", 40, 72, 3), ("same", 33, 17, 1), ("down", 48, 40, 3), ("up", 24, 100, 3)) for dt in (F32, BF)],
    "PackCache.packs": [("stacked_qkv", pack("same", 33, 17, 1, BF))],
    "dora_gain": [("dora", adapted_pack(True)), ("lora", adapted_pack(False))],
    "dora_effective": [("dora", adapted_pack(True))],
    "adapter_grads": [("dora_conv_k3", adapter)],
    "gn_finalize": [("B2_L136_C64", gn_forward(2, 136, 64, F32, True))],
    "gn_stats": [("B3_L200_C48_bf16", gn_forward(3, 200, 48, BF, False))],
    "gn_apply_reproducible": [("film_f32", gn_forward(2, 136, 64, F32, True)), ("plain_bf16", gn_forward(3, 200, 48, BF, False)),
                              ("film_bf16_C72", gn_forward(2, 520, 72, BF, True))],
    "gn_apply_from_stats": [("film_bf16", gn_forward(2, 136, 64, BF, True))],
    "gn_apply": [("film_f32", gn_forward(3, 200, 48, F32, True))],
    "gn_bwd": [("film_f32", gn_backward(2, 136, 64, F32, True, 1.5e-4)), ("plain_bf16", gn_backward(3, 200, 48, BF, False, 6e-2)),
               ("block_f32", module_case("block", F32, 5e-5)), ("block_bf16", module_case("block", BF, 2e-2))],
    "ln_fwd": [("M272_C96_f32", ln(272, 96, F32, 1e-4)), ("M400_C256_bf16", ln(400, 256, BF, 3e-2))],
    "ln_bwd": [("M272_C96_f32", ln(272, 96, F32, 1e-4)), ("M1030_C72_f32", ln(1030, 72, F32, 1e-4))],
    "rowdot": [("pool_f32", pooling(3, 520, 96, F32))],
    "gca_pool": [("L520_C96_f32", pooling(3, 520, 96, F32)), ("L200_C48_bf16", pooling(2, 200, 48, BF)), ("L64_C2048_bf16", pooling(2, 64, 2048, BF)),
                 ("L1024_C256_f32", pooling(2, 1024, 256, F32))],
    "wcolsum": [("reproducible_and_atomic", pooling(2, 200, 48, BF))],
    "gate_residual": [("f32", pooling(3, 520, 96, F32))],
    "gca_bwd_apply": [("gc_f32", module_case("gc", F32, 5e-5)), ("gc_bf16", module_case("gc", BF, 2e-2))],
    "rope_cast": [("f32_ragged", rope_pair), ("qs", attention(2, 200, 3, qs=True))],
    "rope_bwd": [("f32_ragged", rope_pair), ("head_dim_32", attention(2, 136, 2, D=32, rope=True))],
}


def _attention_cases():
    from osufusion_amd import ops as o
    return {
        "mqa_fwd": [("N200", attention(2, 200, 4)), ("N512_qs", attention(1, 512, 2, qs=True)), ("N1024_gqa", attention(2, 1024, 4, G=2, qs=True)),
                    ("N200_D32", attention(2, 200, 2, D=32)), ("N2048_zdq", attention(1, 2048, 2, qs=True, rope=True, zero_dq="fwd"))],
        "fused_bwd_workspace": [("zdq_N200", attention(2, 200, 3, rope=True, zero_dq="fwd")), ("zdq_N1024_qs", attention(2, 1024, 4, qs=True, zero_dq="fwd")),
                                ("zdq_rope_N512", attention(1, 512, 2, zero_dq="rope"))],
        "mqa_fwd_rope": [("write_q_zdq_N200", attention(2, 200, 3, zero_dq="rope")), ("write_q_zdq_N2048", attention(1, 2048, 16, zero_dq="rope"))],
        "mqa_bwd": [("auto_N200", attention(2, 200, 4, variant=o.ATTN_AUTO)), ("auto_qsplit_N512_rope", attention(1, 512, 2, variant=o.ATTN_AUTO, qsplit=2, rope=True)),
                    ("plain_N200", attention(2, 200, 4, variant=o.ATTN_PLAIN)), ("pipe_N1024", attention(2, 1024, 2, variant=o.ATTN_PIPE)),
                    ("fused_N200_rope_bf16", attention(2, 200, 3, rope=True, out_dtype=BF)), ("fused_gqa_N1024", attention(2, 1024, 4, G=2, qs=True, rope=True)),
                    ("slabs_N512", attention(1, 512, 2, variant=o.ATTN_FUSED_SLABS, rope=True)), ("slabs_N200", attention(2, 200, 4, variant=o.ATTN_FUSED_SLABS)),
                    ("fused256_N1024_qs", attention(2, 1024, 2, variant=o.ATTN_FUSED256, qs=True, rope=True)),
                    ("fused512_N1024_qsplit", attention(2, 1024, 1, variant=o.ATTN_FUSED512, qsplit=2)),
                    ("fused512a_N2048_qs", attention(1, 2048, 2, variant=o.ATTN_FUSED512A, qs=True, rope=True)),
                    ("fused512a_N512_qsplit16", attention(1, 512, 2, variant=o.ATTN_FUSED512A, qsplit=16)),
                    ("generic_D32_rope", attention(2, 136, 2, D=32, rope=True)), ("generic_D128", attention(2, 200, 2, D=128))],
        "ncl_to_rows": [("C72_L200", layout)], "rows_to_ncl": [("C72_L200", layout)], "cast_rows": [("C72_L200", layout)],
        "add_rows": [("C72_L200", layout)],
        "axpby_rows": [("x4", scheduler_and_loss)], "ddim_step": [("x4", scheduler_and_loss)], "mse": [("ragged_len", scheduler_and_loss)],
        "skinny_fwd": [(f"{M}x{N}x{K}_{str(dt)[6:]}", skinny(M, N, K, ia, oa, dt, tol)) for M, N, K, ia, oa in ((32, 256, 128, 1, 2), (7, 33, 17, 0, 2), (64, 1024, 1024, 1, 2))
                       for dt, tol in ((F32, 2e-5), (BF, 1e-2))],
        "skinny_bwd": [("48x72x200", skinny(48, 72, 200, 1, 0, F32, 2e-5)), ("5x40x24", skinny(5, 40, 24, 1, 2, BF, 1e-2))],
        "SkinnyLinearFn.backward": [("33x264x136", skinny(33, 264, 136, 0, 2, F32, 2e-5))],
        "skinny_fwd_group": [("film3", linear_group)], "skinny_dx_group": [("film3", linear_group)], "LinearGroupFn.backward": [("film3", linear_group)],
        "fir_decimate2": [("odd_len", audio)], "frame_rows": [("tail", audio)], "log_vqt": [("bins12", audio)],
    }


# functions that allocate but need no case of their own
EXEMPT = {
    "_upload_table": "pinned host staging (passes through the guard); the device copy it feeds is exercised by skinny_fwd_group / skinny_dx_group",
    "ZeroArena.take": "torch.empty(0) on the host: an element-size probe, nothing is read",
}


def all_cases():
    d = {k: list(v) for k, v in CASES.items()}
    for k, v in _attention_cases().items():
        d.setdefault(k, []).extend(v)
    return d


def _ids():
    """Case ids without importing the package (collection on a CPU-only machine): the attention entries are listed by name."""
    try:
        cases = all_cases()
    except Exception:                                                    # noqa: BLE001 -- no built library: the GPU cases are not collected here
        return list((k, v) for k, vs in CASES.items() for v, _ in vs)
    return [(k, v) for k, vs in cases.items() for v, _ in vs]


@pytest.mark.gpu
@pytest.mark.parametrize("op,variant", _ids(), ids=lambda s: s)
def test_poisoned_memory(op, variant):
    fn = dict(all_cases()[op])[variant]
    run_case(fn)


# ----------------------------------------------------------------------------------------------------------------------------------------
# completeness (CPU)
# ----------------------------------------------------------------------------------------------------------------------------------------
def allocating_functions(path: Path):
    """Qualified names (Class.method or function) of every function in `path` that calls torch.empty / torch.empty_like (nested helpers
    count towards the function they are defined in)."""
    tree = ast.parse(path.read_text())
    found = set()

    def calls_empty(node):
        for n in ast.walk(node):
            if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and n.func.attr in ("empty", "empty_like", "new_empty", "empty_strided"):
                v = n.func.value
                if (isinstance(v, ast.Name) and v.id == "torch") or n.func.attr in ("new_empty",):
                    return True
        return False

    for top in tree.body:
        if isinstance(top, (ast.FunctionDef, ast.AsyncFunctionDef)) and calls_empty(top):
            found.add(top.name)
        elif isinstance(top, ast.ClassDef):
            for m in top.body:
                if isinstance(m, (ast.FunctionDef, ast.AsyncFunctionDef)) and calls_empty(m):
                    found.add(f"{top.name}.{m.name}")
    return found


def _table_keys():
    src = Path(__file__).read_text()
    tree = ast.parse(src)
    keys = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == "CASES" for t in node.targets):
            keys |= {k.value for k in node.value.keys}
        if isinstance(node, ast.FunctionDef) and node.name == "_attention_cases":
            for r in ast.walk(node):
                if isinstance(r, ast.Dict):
                    keys |= {k.value for k in r.keys if isinstance(k, ast.Constant)}
    return keys


def test_every_allocating_function_has_a_poisoned_memory_case():
    """A new torch.empty site in ops.py or functional.py fails the CPU suite until it has a case here (or a reason in EXEMPT)."""
    sites = allocating_functions(ROOT / "osufusion_amd" / "ops.py") | allocating_functions(ROOT / "osufusion_amd" / "functional.py")
    assert {"gemm_nt", "mqa_bwd", "PackCache.packs", "LinearGroupFn.backward"} <= sites        # the parser sees methods and functions
    keys = _table_keys()
    missing = sorted(s for s in sites if s not in keys and s not in EXEMPT)
    assert not missing, f"allocating functions without a poisoned-memory case or an exemption: {missing}"
    stale = sorted(k for k in set(EXEMPT) if k not in sites)
    assert not stale, f"EXEMPT names functions that no longer allocate: {stale}"
    for k, vs in CASES.items():
        assert vs, k


def test_completeness_check_sees_a_missing_entry(tmp_path):
    """Dropping one entry makes the check fail: the parser finds the function, the table no longer names it."""
    sites = allocating_functions(ROOT / "osufusion_amd" / "ops.py")
    assert "gn_apply" in sites and "gn_apply" in _table_keys()
    p = tmp_path / "m.py"
    p.write_text("import torch\n\ndef f(n):\n    return torch.empty(n)\n\nclass K:\n    def g(self, x):\n        return torch.empty_like(x)\n\ndef h():\n    return 1\n")
    assert allocating_functions(p) == {"f", "K.g"}


# ----------------------------------------------------------------------------------------------------------------------------------------
# model level: unet_mid (tests/golden) -- one Trainer step, and the two samplers
# ----------------------------------------------------------------------------------------------------------------------------------------
def _oracle_grads(golden_dir, case):
    """The oracle's fp32 gradients of the golden case (pinned to the reference's goldens), flattened in param_names order."""
    def ref():
        import json

        from oracle import diffusion_oracle as DO
        from oracle import unet_oracle as O
        from osufusion_amd.pattern import synth_inputs
        meta = json.loads((golden_dir / "unet_cases.json").read_text())[case]
        cfgd = {k: (tuple(v) if isinstance(v, list) else v) for k, v in meta["cfg"].items()}
        p = {k: v.requires_grad_() for k, v in O.make_params(O.UNetConfig(**cfgd), prefix="unet.").items()}
        xs, as_, cs, ts, ns = (torch.from_numpy(v) for v in synth_inputs(case, meta["B"], meta["L"]))
        DO.training_loss(p, O.UNetConfig(**cfgd), xs, as_, cs, ns, ts, cond_drop_prob=0.0).backward()
        return torch.cat([p["unet." + k].grad.flatten() for k in meta["param_names"]])
    return memo(("oracle_grads", case), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("byte", [0xFF, 0x7F])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_unet_mid_train_step_under_poison(golden_dir, dtype, byte):
    """One Trainer step (forward, backward with direct accumulation into the flat gradient, fused AdamW, grouped pack refresh) with every
    allocation poisoned: loss and flat gradient finite and within the golden tolerances of tests/test_hip_parity.py (fp32: 1e-3 loss,
    2e-2 per-parameter gradient norms; bf16: the reference-autocast bounds), every canary intact, and the step arena's memory behind its
    high-water mark still zero (a write past an arena accumulator would corrupt the next step's "pre-zeroed" memory)."""
    import numpy as np

    from osufusion_amd import functional as Fn
    from osufusion_amd.pattern import synth_inputs
    from osufusion_amd.train import Trainer
    from tests.memguard import guard
    from tests.test_hip_parity import G, T, _build_model
    case = "unet_mid"
    meta, _, model = _build_model(case, golden_dir)
    model.cond_drop_prob = 0.0
    g32, g16 = G(golden_dir, case), G(golden_dir, f"{case}_autocast")
    x, a, c, t, noise = (T(v) for v in synth_inputs(case, meta["B"], meta["L"]))
    names = meta["param_names"]
    try:
        with guard(byte) as g:
            trainer = Trainer(model, lr=1e-4, compute_dtype=dtype)
            params = dict(model.unet.named_parameters())
            loss, norm = trainer.step(x, a, c, noise, t)
            torch.cuda.synchronize()
            grads = {k: params[k].grad.detach().clone() for k in names}
            g.check()
            assert g.allocations > 200, g.allocations                     # the step's outputs, workspaces and packs all came through the guard
            arena = trainer.arena
            assert arena.dirty > 0 and not bool(arena.buf[arena.dirty:].any()), "memory behind the arena's high-water mark was written"
            g.release()
    finally:
        Fn.enable_direct_grads(False)
    assert torch.isfinite(loss).item() and torch.isfinite(norm).item()
    flat = torch.cat([grads[k].flatten() for k in names])
    assert bool(torch.isfinite(flat).all())
    e_loss = abs(loss.item() - float(g32["loss"])) / abs(float(g32["loss"]))
    if dtype == torch.float32:
        assert e_loss < 1e-3, e_loss
        gn = np.array([grads[k].norm().item() for k in names])
        ref = g32["grad_norms"]
        rel = np.abs(gn - ref) / (ref + 1e-3 * ref.max())
        assert rel.max() < 2e-2, (names[int(rel.argmax())], rel.max())
    else:
        ref_loss = abs(float(g16["loss"]) - float(g16["loss_fp32"])) / float(g16["loss_fp32"])
        assert e_loss < max(3 * ref_loss, 1e-3), (e_loss, ref_loss)
        e_flat = rell2(flat.cpu(), _oracle_grads(golden_dir, case))
        assert e_flat < 1.5 * float(g16["flat_grad_dist"]), e_flat


@pytest.mark.gpu
@pytest.mark.parametrize("sampler", ["ddim", "rectified_flow"])
def test_unet_mid_samplers_under_poison(golden_dir, sampler):
    """The bf16 samplers after an fp32-mode call (the order of the round-4 incident (a)): a sample with every allocation NaN-filled, one with
    every allocation ~3.4e38, and a clean one are bit-identical; no canary overwritten."""
    import json

    import osufusion_amd as oa
    from osufusion_amd.pattern import synth_inputs
    from tests.memguard import guard
    from tests.test_hip_parity import T, _build_model, load_pattern
    case = "unet_mid"
    if sampler == "ddim":
        meta, _, model = _build_model(case, golden_dir)
        model.sampling_timesteps = 4
    else:
        from osufusion_amd.models.rectified_flow import OsuFusion as RF
        meta = json.loads((golden_dir / "unet_cases.json").read_text())[case]
        kw = {k: (tuple(v) if isinstance(v, list) else v) for k, v in meta["cfg"].items() if not k.startswith("dim_in_")}
        model = RF(kw.pop("dim_h"), **kw).to(DEV)
        load_pattern(model.unet)
        model.sample_timesteps = 4
    model.eval()
    _, a, c, _, noise = (T(v) for v in synth_inputs(f"poison_{sampler}", meta["B"], meta["L"]))
    with oa.forced_compute_dtype(torch.float32):
        y32 = model.sample(a, c, noise.clone(), cond_scale=2.0)
    assert bool(torch.isfinite(y32).all())
    outs = []
    for byte in (0xFF, 0x7F):
        with guard(byte) as g, oa.forced_compute_dtype(torch.bfloat16):
            outs.append(model.sample(a, c, noise.clone(), cond_scale=2.0).clone())
            g.check()
            assert g.allocations > 100, g.allocations
            g.release()
    with oa.forced_compute_dtype(torch.bfloat16):
        outs.append(model.sample(a, c, noise.clone(), cond_scale=2.0))
    assert bool(torch.isfinite(outs[0]).all())
    assert torch.equal(outs[0], outs[1]), "0xFF vs 0x7F"
    assert torch.equal(outs[0], outs[2]), "poisoned vs clean"
