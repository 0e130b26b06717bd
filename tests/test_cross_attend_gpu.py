"""Cross-attention through the stand-alone Attend module (osufusion_amd/cross_attend.py): k / v of another length than q.

The yardstick is tests/test_attend_autograd_gpu.py's, generalised to (Nq, Nk): fp64 autograd of softmax(q k^T D^-0.5 + mask.to(bf16)) v on
the bf16-cast inputs (the reference Attend's arithmetic, attention.py:84-101), with that file's bounds: output rel-L2 < 6e-3, gradients
rel-L2 < 1e-2 and rel-max < 3e-2, everything finite.  Shapes: Nk = 77 (one full 64-key tile + a ragged 13-key one; one dK/dV workgroup with
idle waves), Nk = 130 (a second dK/dV workgroup with 2 live keys), Nq = 33 (a ragged second 32-query block), Nk = 5 (less than a tile),
Nk >> Nq and Nk << Nq (a swapped N / Nk in a batch stride or an index shows).  Masked self-attention rides the same path: its C entry points
against osuf_xattn_*, its dispatch from attend(), and its poisoned-memory cases on column views of one q|k|v image are here too."""
import itertools

import pytest
import torch
import torch.nn.functional as F

from tests.test_attend_autograd_gpu import HG, MASKS, RL2, RMAX, check
from tests.test_hip_parity import DEV, rell2, report
from tests.test_poisoned_memory import rnd, run_case

pytestmark = pytest.mark.gpu

B = 2
SHAPES = ((200, 77), (64, 1000), (33, 130), (1000, 64), (40, 5))


def make_mask(kind, H, Nq, Nk, dev=DEV):
    if kind == "none":
        return None
    if kind == "causal":                                   # (Nq, Nk) float, -inf where key > query * Nk / Nq (key 0 stays in every row)
        qi, ki = torch.arange(Nq, device=dev)[:, None], torch.arange(Nk, device=dev)[None, :]
        return torch.zeros(Nq, Nk, device=dev).masked_fill(ki * Nq > qi * Nk, float("-inf"))
    if kind == "per_head":                                 # (1, H, Nq, Nk) float
        return torch.randn(1, H, Nq, Nk, device=dev)
    if kind == "bool":                                     # (B, 1, Nq, Nk): adds 1.0 / 0.0 (the reference's bf16 cast of a bool mask)
        return torch.rand(B, 1, Nq, Nk, device=dev) > 0.5
    if kind == "dense":                                    # (B, H, Nq, Nk) bf16 with a band of -inf keys; every row keeps finite keys
        m = torch.randn(B, H, Nq, Nk, device=dev).to(torch.bfloat16)
        m[..., Nk // 4:Nk // 4 + max(Nk // 8, 1)] = float("-inf")
        return m
    raise ValueError(kind)


def ref_grads(q, k, v, mask, go):
    """fp64 autograd of softmax(q k^T D^-0.5 + mask.to(bf16)) v on bf16-cast q (Nq rows), k, v (Nk rows): (out, dq, dk, dv, dmask)."""
    H, D = q.shape[1], q.shape[3]
    qb, kb, vb = (t.detach().to(torch.bfloat16).double().requires_grad_() for t in (q, k, v))
    mb = None
    sc = qb @ kb.expand(-1, H, -1, -1).transpose(-1, -2) * D ** -0.5
    if mask is not None:
        mb = mask.detach().to(torch.bfloat16).double().requires_grad_(mask.is_floating_point())
        sc = sc + mb
    out = sc.softmax(-1) @ vb.expand(-1, H, -1, -1)
    out.backward(go.double())
    return out.detach(), qb.grad, kb.grad, vb.grad, (mb.grad if mb is not None and mb.requires_grad else None)


def leaves(H, G, Nq, Nk, D):
    return [torch.randn(B, h, n, D, device=DEV).requires_grad_() for h, n in ((H, Nq), (G, Nk), (G, Nk))]


# every mask kind meets every (H, G) pair and every shape across the D x shape grid (the (H, G) choice is shifted by one per block)
GRID = [(D, s, m, HG[(i + i // len(MASKS)) % len(HG)]) for i, (D, s, m) in enumerate(itertools.product((16, 32, 64, 128), SHAPES, MASKS))]


@pytest.mark.parametrize("D,shape,kind,hg", GRID, ids=[f"D{d}-Nq{s[0]}-Nk{s[1]}-{m}-H{h}G{g}" for d, s, m, (h, g) in GRID])
def test_cross_attend_gradients(D, shape, kind, hg):
    from osufusion_amd.modules.attention import Attend
    (Nq, Nk), (H, G) = shape, hg
    q, k, v = leaves(H, G, Nq, Nk, D)
    mask = make_mask(kind, H, Nq, Nk)
    go = torch.randn(B, H, Nq, D, device=DEV).to(torch.bfloat16).float()
    att = Attend()
    out = att(q, k, v, attn_mask=mask)
    assert out.grad_fn is not None and out.shape == (B, H, Nq, D) and out.dtype == v.dtype
    with torch.no_grad():
        assert torch.equal(out.detach(), att(q, k, v, attn_mask=mask))        # grad mode runs the very same launches
    out.backward(go)
    ro, rq, rk, rv, _ = ref_grads(q, k, v, mask, go)
    tag = f"D{D}/Nq{Nq}/Nk{Nk}/{kind}/H{H}G{G}"
    check(f"cross/{tag}/out", out.detach(), ro, 6e-3, RMAX)
    for nm, t, r in (("dq", q, rq), ("dk", k, rk), ("dv", v, rv)):
        assert t.grad.shape == t.shape and t.grad.dtype == t.dtype
        check(f"cross/{tag}/{nm}", t.grad, r)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("D,Nq,H,G,dtype", [(16, 40, 3, 1, torch.float32), (64, 200, 4, 4, torch.bfloat16), (128, 33, 2, 1, torch.float32),
                                                  (32, 70, 3, 1, torch.bfloat16)])
def test_single_key(D, Nq, H, G, dtype, masked):
    """Nk = 1: every softmax row is exactly 1, so the output is v's only row (rounded to bf16) for every query and head."""
    from osufusion_amd.modules.attention import Attend
    q, k, v = (t.detach().to(dtype).requires_grad_() for t in leaves(H, G, Nq, 1, D))
    mask = torch.randn(B, H, Nq, 1, device=DEV) if masked else None
    out = Attend()(q, k, v, attn_mask=mask)
    assert out.dtype == dtype
    assert torch.equal(out.detach(), v.detach().to(torch.bfloat16).to(dtype).expand(B, H, Nq, D))
    out.backward(torch.randn(B, H, Nq, D, device=DEV).to(dtype))
    for t in (q, k, v):
        assert t.grad.shape == t.shape and t.grad.dtype == dtype and torch.isfinite(t.grad).all()


@pytest.mark.parametrize("shape", ["1HNN", "BHNN"])
@pytest.mark.parametrize("G", ["1", "H"])
@pytest.mark.parametrize("D,nn,dtype", [(64, (200, 77), torch.float32), (32, (64, 1000), torch.float32), (128, (33, 130), torch.bfloat16)])
def test_cross_attend_bias_gradient(shape, G, D, nn, dtype):
    from osufusion_amd.modules.attention import Attend
    H, (Nq, Nk) = 3, nn
    q, k, v = leaves(H, 1 if G == "1" else H, Nq, Nk, D)
    m = torch.randn(1 if shape == "1HNN" else B, H, Nq, Nk, device=DEV)
    m[..., Nk // 3:Nk // 3 + 5] = float("-inf")
    m = m.to(dtype).requires_grad_()
    go = torch.randn(B, H, Nq, D, device=DEV).to(torch.bfloat16).float()
    Attend()(q, k, v, attn_mask=m).backward(go)
    _, rq, rk, rv, rm = ref_grads(q, k, v, m, go)
    assert m.grad is not None and m.grad.shape == m.shape and m.grad.dtype == dtype
    tag = f"cross_bias/{shape}/G{G}/D{D}/Nq{Nq}/Nk{Nk}"
    check(f"{tag}/dmask", m.grad, rm)
    for nm, t, r in (("dq", q, rq), ("dk", k, rk), ("dv", v, rv)):
        check(f"{tag}/{nm}", t.grad, r)


def test_bool_and_integer_masks_get_no_gradient():
    from osufusion_amd.modules.attention import Attend
    q, k, v = leaves(2, 1, 64, 77, 32)
    for m in (torch.rand(64, 77, device=DEV) > 0.3, torch.ones(1, 1, 64, 77, device=DEV, dtype=torch.int32)):
        out = Attend()(q, k, v, attn_mask=m)
        out.sum().backward()                                                   # (a gradient handed to a non-float input would raise here)
        assert m.grad is None
        for t in (q, k, v):
            assert t.grad is not None and t.grad.shape == t.shape and torch.isfinite(t.grad).all()
        q.grad = k.grad = v.grad = None


# ----------------------------------------------------------------------------------------------------------------------------------------
# osuf_mqa_fwd_masked / osuf_mqa_bwd_masked forward to osuf_xattn_* with Nk = N: called directly (no Python wrapper is left for them), they
# equal the generic path bit for bit
# ----------------------------------------------------------------------------------------------------------------------------------------
def _image(N, H, D):
    qkv = torch.randn(B, N, (H + 2) * D, device=DEV).to(torch.bfloat16)
    return qkv, qkv[..., :H * D], qkv[..., H * D:(H + 1) * D], qkv[..., (H + 1) * D:]


@pytest.mark.parametrize("N,H,D", [(200, 3, 64), (136, 2, 32), (200, 1, 128), (136, 3, 16)])
def test_same_length_equals_masked_self_attention(N, H, D):
    from osufusion_amd import cross_attend as Xa
    from osufusion_amd import ops
    scale = D ** -0.5
    qkv, q, k, v = _image(N, H, D)
    m = torch.randn(B, H, N, N, device=DEV)
    m[..., N // 4:N // 4 + 7] = float("-inf")
    m4 = m.to(torch.bfloat16)
    do = torch.randn(B, N, H * D, device=DEV).to(torch.bfloat16)
    # the self-attention side: the two C symbols on the [B][N][(H+2)D] image, outputs allocated here
    W = (H + 2) * D
    base, mstr, st = qkv.data_ptr(), m4.stride(), ops._stream()
    o = torch.empty(B, N, H * D, dtype=torch.bfloat16, device=DEV)
    lse, delta = (torch.empty(B, H, N, dtype=torch.float32, device=DEV) for _ in range(2))
    dqkv = torch.empty(B, N, W, dtype=torch.float32, device=DEV)
    dbias = torch.empty(B, H, N, N, dtype=torch.float32, device=DEV)
    gb = dqkv.data_ptr()
    ops.call("osuf_mqa_fwd_masked", base, W, base + 2 * H * D, W, base + 2 * (H + 1) * D, W, o.data_ptr(), H * D, ops.BF16, lse.data_ptr(),
             m4.data_ptr(), *mstr, B, H, N, D, scale, st)
    ops.call("osuf_attn_delta", do.data_ptr(), H * D, o.data_ptr(), H * D, ops.BF16, delta.data_ptr(), B, H, N, D, st)
    ops.call("osuf_mqa_bwd_masked", base, W, base + 2 * H * D, W, base + 2 * (H + 1) * D, W, do.data_ptr(), H * D, lse.data_ptr(), delta.data_ptr(),
             m4.data_ptr(), *mstr, gb, W, gb + 4 * H * D, gb + 4 * (H + 1) * D, W, B, H, N, D, scale, ops.F32, dbias.data_ptr(), st)
    xo, xlse = Xa.xattn_fwd(q, k, v, m4, B, N, N, H, D, torch.bfloat16, scale)
    assert torch.equal(xo, o) and torch.equal(xlse, lse)
    xdq, xdk, xdv, xdb = Xa.xattn_bwd(q, k, v, m4, xo, do, xlse, B, N, N, H, D, scale, True)
    assert torch.equal(xdq, dqkv[..., :H * D]) and torch.equal(xdk, dqkv[..., H * D:(H + 1) * D]) and torch.equal(xdv, dqkv[..., (H + 1) * D:])
    assert torch.equal(xdb, dbias)
    assert all(torch.isfinite(t).all() for t in (xo, xlse, xdq, xdk, xdv, xdb))


def test_null_lse2_is_an_invalid_argument():
    """lse2 = NULL: the kernel writes it unconditionally, so both forward entry points refuse the call before anything is launched."""
    from osufusion_amd import ops
    N, H, D = 32, 1, 32
    qkv, q, k, v = _image(N, H, D)
    qkv, q, k, v = qkv[:1], q[:1], k[:1], v[:1]
    W = (H + 2) * D
    m4 = torch.zeros(1, H, N, N, dtype=torch.bfloat16, device=DEV)
    o = torch.empty(1, N, H * D, dtype=torch.bfloat16, device=DEV)
    head = (q.data_ptr(), W, k.data_ptr(), W, v.data_ptr(), W, o.data_ptr(), H * D, ops.BF16, None, m4.data_ptr(), *m4.stride(), 1, H)
    for name, lengths in (("osuf_mqa_fwd_masked", (N,)), ("osuf_xattn_fwd", (N, N))):
        with pytest.raises(RuntimeError, match=name + " failed: invalid argument"):
            ops.call(name, *head, *lengths, D, D ** -0.5, ops._stream())


@pytest.mark.parametrize("grad_mask", [False, True])
def test_masked_self_attention_dispatches_to_the_generic_path(grad_mask):
    """attend() with a mask at Nk == Nq: CrossAttendFn under grad mode, and the very same launches under no_grad."""
    from osufusion_amd import attend as At
    from osufusion_amd.cross_attend import CrossAttendFn
    N, H, D = 64, 2, 32
    q, k, v = leaves(H, 1, N, N, D)
    if grad_mask:
        q, k, v = (t.detach() for t in (q, k, v))                              # the mask alone asks for a gradient
    mask = make_mask("causal", H, N, N).requires_grad_(grad_mask)
    out = At.attend(q, k, v, mask)
    assert out.grad_fn is not None and type(out.grad_fn).__name__ == CrossAttendFn.__name__ + "Backward"
    with torch.no_grad():
        bare = At.attend(q, k, v, mask)
    assert bare.grad_fn is None and torch.equal(out.detach(), bare)


@pytest.mark.parametrize("N", [200, 136])
def test_same_length_unmasked_equals_generic_forward(N):
    """mask = NULL at head dim 32: the very kernel ops.mqa_fwd launches."""
    from osufusion_amd import cross_attend as Xa
    from osufusion_amd import ops
    H, D = 3, 32
    qkv, q, k, v = _image(N, H, D)
    o, lse = ops.mqa_fwd(qkv, B, N, H, D, torch.bfloat16, D ** -0.5)
    xo, xlse = Xa.xattn_fwd(q, k, v, None, B, N, N, H, D, torch.bfloat16, D ** -0.5)
    assert torch.equal(xo, o) and torch.equal(xlse, lse) and torch.isfinite(xo.float()).all()


# ----------------------------------------------------------------------------------------------------------------------------------------
# poisoned memory (tests/memguard.py): the kernels have no atomics, so every output is bit-identical across the three fills
# ----------------------------------------------------------------------------------------------------------------------------------------
def cross_pair(Nq, Nk, H, D, bias_shape, want_dbias, image=False):
    """image: q, k, v are column views of one guarded [B][N][(H+2)D] q|k|v image (Nk == Nq; the row stride is not the row width)."""
    def run(c):
        from osufusion_amd import cross_attend as Xa
        scale = D ** -0.5
        if image:
            assert Nk == Nq
            qkv = c.inp(rnd("qkv", (B, Nq, (H + 2) * D)), torch.bfloat16)
            q, k, v = qkv[..., :H * D], qkv[..., H * D:(H + 1) * D], qkv[..., (H + 1) * D:]
        else:
            q = c.inp(rnd("q", (B, Nq, H * D)), torch.bfloat16)
            k = c.inp(rnd("k", (B, Nk, D)), torch.bfloat16)
            v = c.inp(rnd("v", (B, Nk, D)), torch.bfloat16)
        do = c.inp(rnd("do", (B, Nq, H * D)), torch.bfloat16)
        mask4 = None
        if bias_shape is not None:
            m = rnd("m", bias_shape)
            m[..., Nk // 4:Nk // 4 + 7] = float("-inf")
            mask4 = c.inp(m, torch.bfloat16).expand(B, H, Nq, Nk)
        o, lse = Xa.xattn_fwd(q, k, v, mask4, B, Nq, Nk, H, D, torch.bfloat16, scale)
        dq, dk, dv, dbias = Xa.xattn_bwd(q, k, v, mask4, o, do, lse, B, Nq, Nk, H, D, scale, want_dbias)
        c.eq("o", o), c.eq("lse", lse), c.eq("dq", dq), c.eq("dk", dk), c.eq("dv", dv)
        if want_dbias:
            c.eq("dbias", dbias)
        else:
            assert dbias is None
        heads = lambda t, n: t.view(B, n, -1, D).permute(0, 2, 1, 3)
        ro, rq, rk, rv, rm = ref_grads(heads(q, Nq), heads(k, Nk), heads(v, Nk), mask4, heads(do, Nq).float())
        rows = lambda t: t.permute(0, 2, 1, 3).reshape(B, t.shape[2], -1).float()
        c.close("o", o, rows(ro), 6e-3, rell2)
        c.close("dq", dq, rows(rq), RL2, rell2)
        c.close("dk", dk, rows(rk), RL2, rell2)
        c.close("dv", dv, rows(rv), RL2, rell2)
        if want_dbias:
            c.close("dbias", dbias, rm.float(), RL2, rell2)                    # rm: the gradient of the expanded (B, H, Nq, Nk) bias
    return run


# allocating function of osufusion_amd/cross_attend.py -> its cases (tests/test_cross_attend_cpu.py requires one for every torch.empty site)
def masked_pair(N, H, D, bias_shape, want_dbias):
    """Masked self-attention as Attend's callers lay it out: one q|k|v row image, Nk = Nq = N."""
    return cross_pair(N, N, H, D, bias_shape, want_dbias, image=True)


def attention_masked(c):
    """A key-padding bias (B, 1, 1, N) of 0 / -1e4 on the q|k|v image: the forward alone."""
    from osufusion_amd import cross_attend as Xa
    N, H, D = 200, 2, 64
    qkv = c.inp(rnd("qkv", (B, N, (H + 2) * D)), torch.bfloat16)
    m = (rnd("m", (B, 1, 1, N)) > -1.0).to(torch.bfloat16)
    mask4 = c.inp(torch.where(m > 0, 0.0, -1e4).to(torch.bfloat16)).expand(B, H, N, N)
    o, lse = Xa.xattn_fwd(qkv[..., :H * D], qkv[..., H * D:(H + 1) * D], qkv[..., (H + 1) * D:], mask4, B, N, N, H, D, torch.bfloat16, D ** -0.5)
    c.eq("o", o), c.eq("lse", lse)


POISON_CASES = {
    "xattn_fwd": [("Nq200_Nk77_D64_broadcast", cross_pair(200, 77, 3, 64, (1, 1, 200, 77), False)),
                  ("Nq64_Nk200_D128_unmasked", cross_pair(64, 200, 2, 128, None, False)),
                  ("image_N200_D64_broadcast", masked_pair(200, 3, 64, (1, 1, 200, 200), False)),
                  ("image_N200_D64_key_padding", attention_masked)],
    "xattn_bwd": [("Nq200_Nk77_D64_broadcast", cross_pair(200, 77, 3, 64, (1, 1, 200, 77), False)),
                  ("Nq33_Nk130_D32_dbias", cross_pair(33, 130, 2, 32, (B, 2, 33, 130), True)),
                  ("Nq64_Nk200_D128_unmasked", cross_pair(64, 200, 2, 128, None, False)),
                  ("image_N200_D64_broadcast", masked_pair(200, 3, 64, (1, 1, 200, 200), False)),
                  ("image_N200_D64_dbias", masked_pair(200, 3, 64, (B, 3, 200, 200), True)),
                  ("image_N136_D32_dbias", masked_pair(136, 2, 32, (B, 2, 136, 136), True)),
                  ("image_N100_D128_dbias", masked_pair(100, 1, 128, (B, 1, 100, 100), True))],
}


@pytest.mark.parametrize("fn,case", [(k, c) for k, v in POISON_CASES.items() for c, _ in v])
def test_cross_attention_on_poisoned_memory(fn, case):
    run_case(dict(POISON_CASES[fn])[case])


# ----------------------------------------------------------------------------------------------------------------------------------------
def test_toy_cross_block_end_to_end():
    """Linear -> Attend(q from x, k / v from a context of another length, its padded tail masked) -> Linear, loss, backward: every
    parameter gradient within rel-L2 1e-2 of the same block on torch SDPA in fp32."""
    from osufusion_amd.modules.attention import Attend
    C, Cc, H, D, Nq, Nk = 96, 48, 2, 64, 200, 77
    to_q, to_kv, to_out = torch.nn.Linear(C, H * D).to(DEV), torch.nn.Linear(Cc, 2 * H * D).to(DEV), torch.nn.Linear(H * D, C).to(DEV)
    att = Attend()
    x, ctx, target = torch.randn(B, Nq, C, device=DEV), torch.randn(B, Nk, Cc, device=DEV), torch.randn(B, Nq, C, device=DEV)
    pad = torch.zeros(1, 1, 1, Nk, device=DEV)
    pad[..., Nk - 7:] = float("-inf")

    def block(attend_fn):
        q = to_q(x).view(B, Nq, H, D).permute(0, 2, 1, 3)
        k, v = to_kv(ctx).view(B, Nk, 2, H, D).permute(2, 0, 3, 1, 4)
        o = attend_fn(q, k, v)
        return F.mse_loss(to_out(o.permute(0, 2, 1, 3).reshape(B, Nq, H * D)), target)

    params = list(to_q.parameters()) + list(to_kv.parameters()) + list(to_out.parameters())
    got = torch.autograd.grad(block(lambda q, k, v: att(q, k, v, attn_mask=pad)), params)
    want = torch.autograd.grad(block(lambda q, k, v: F.scaled_dot_product_attention(q, k, v, attn_mask=pad)), params)
    for name, g, w in zip(("q.weight", "q.bias", "kv.weight", "kv.bias", "out.weight", "out.bias"), got, want):
        e = rell2(g, w)
        report(f"toy_cross_block/{name}", rel_l2=e)
        assert torch.isfinite(g).all() and e < 1e-2, (name, e)
