"""Training through the stand-alone Attend and RotaryPositionEmbedding modules (osufusion_amd/attend.py): their gradients against fp64
autograd of the reference's formulas (attention.py:15-101) on the bf16-cast inputs, the bias gradient of a floating-point mask, K/V heads
given repeated, and a toy block end to end.  (The masked calls run cross_attend.py's generic path; their poisoned-memory cases are in
tests/test_cross_attend_gpu.py.)"""
import itertools

import pytest
import torch
import torch.nn.functional as F

from tests.test_hip_parity import DEV, rell2, relmax, report

pytestmark = pytest.mark.gpu

RL2, RMAX = 1e-2, 3e-2          # the bounds of test_hip_parity.py::test_mqa_flash_vs_sdpa
B = 2
MASKS = ("none", "causal", "per_head", "bool", "dense")
HG = ((1, 1), (3, 1), (3, 3), (4, 1), (4, 4))


def make_mask(kind, H, N, dev=DEV):
    if kind == "none":
        return None
    if kind == "causal":                                   # (N, N) float, -inf above the diagonal
        return torch.zeros(N, N, device=dev).masked_fill(torch.ones(N, N, device=dev, dtype=torch.bool).triu(1), float("-inf"))
    if kind == "per_head":                                 # (1, H, N, N) float
        return torch.randn(1, H, N, N, device=dev)
    if kind == "bool":                                     # (B, 1, N, N): adds 1.0 / 0.0 (the reference's bf16 cast of a bool mask)
        return torch.rand(B, 1, N, N, device=dev) > 0.5
    if kind == "dense":                                    # (B, H, N, N) bf16 with a band of -inf keys; every row keeps finite keys
        m = torch.randn(B, H, N, N, device=dev).to(torch.bfloat16)
        m[..., N // 4:N // 4 + max(N // 8, 1)] = float("-inf")
        return m
    raise ValueError(kind)


def ref_grads(q, k, v, mask, go):
    """fp64 autograd of softmax(q k^T D^-0.5 + mask.to(bf16)) v on bf16-cast q, k, v: (out, dq, dk, dv, dmask)."""
    H, N, D = q.shape[1], q.shape[2], q.shape[3]
    qb, kb, vb = (t.detach().to(torch.bfloat16).double().requires_grad_() for t in (q, k, v))
    mb = None
    sc = qb @ kb.expand(-1, H, -1, -1).transpose(-1, -2) * D ** -0.5
    if mask is not None:
        mb = mask.detach().to(torch.bfloat16).double().requires_grad_(mask.is_floating_point())
        sc = sc + mb
    out = sc.softmax(-1) @ vb.expand(-1, H, -1, -1)
    out.backward(go.double())
    return out.detach(), qb.grad, kb.grad, vb.grad, (mb.grad if mb is not None and mb.requires_grad else None)


def leaves(H, G, N, D):
    return [torch.randn(B, h, N, D, device=DEV).requires_grad_() for h in (H, G, G)]


def check(name, got, want, rl2=RL2, rmax=RMAX):
    e2, em = rell2(got, want), relmax(got, want)
    report(f"attend_autograd/{name}", rel_l2=e2, relmax=em)
    assert torch.isfinite(got).all(), name
    assert e2 < rl2 and em < rmax, (name, e2, em)


# every mask kind meets every (H, G) pair across the D x N grid (the (H, G) choice is shifted by one per (D, N) block)
GRID = [(D, N, m, HG[(i + i // len(MASKS)) % len(HG)]) for i, (D, N, m) in enumerate(itertools.product((16, 32, 64, 128), (64, 200, 1000), MASKS))]


@pytest.mark.parametrize("D,N,kind,hg", GRID, ids=[f"D{d}-N{n}-{m}-H{h}G{g}" for d, n, m, (h, g) in GRID])
def test_attend_gradients(D, N, kind, hg):
    from osufusion_amd.modules.attention import Attend
    H, G = hg
    q, k, v = leaves(H, G, N, D)
    mask = make_mask(kind, H, N)
    go = torch.randn(B, H, N, D, device=DEV).to(torch.bfloat16).float()
    att = Attend()
    out = att(q, k, v, attn_mask=mask)
    assert out.grad_fn is not None
    with torch.no_grad():
        assert torch.equal(out.detach(), att(q, k, v, attn_mask=mask))        # grad mode runs the very same launches
    out.backward(go)
    ro, rq, rk, rv, _ = ref_grads(q, k, v, mask, go)
    tag = f"D{D}/N{N}/{kind}/H{H}G{G}"
    check(f"{tag}/out", out.detach(), ro, 6e-3, RMAX)
    for nm, t, r in (("dq", q, rq), ("dk", k, rk), ("dv", v, rv)):
        assert t.grad.shape == t.shape and t.grad.dtype == t.dtype
        check(f"{tag}/{nm}", t.grad, r)


@pytest.mark.parametrize("shape", ["1HNN", "BHNN"])
@pytest.mark.parametrize("G", ["1", "H"])
@pytest.mark.parametrize("D,N,dtype", [(64, 200, torch.float32), (32, 1000, torch.float32), (128, 64, torch.bfloat16)])
def test_attend_bias_gradient(shape, G, D, N, dtype):
    from osufusion_amd.modules.attention import Attend
    H = 3
    q, k, v = leaves(H, 1 if G == "1" else H, N, D)
    m = torch.randn(1 if shape == "1HNN" else B, H, N, N, device=DEV)
    m[..., :, N // 3:N // 3 + 5] = float("-inf")
    m = m.to(dtype).requires_grad_()
    go = torch.randn(B, H, N, D, device=DEV).to(torch.bfloat16).float()
    Attend()(q, k, v, attn_mask=m).backward(go)
    _, rq, rk, rv, rm = ref_grads(q, k, v, m, go)
    assert m.grad is not None and m.grad.shape == m.shape and m.grad.dtype == dtype
    tag = f"bias/{shape}/G{G}/D{D}/N{N}"
    check(f"{tag}/dmask", m.grad, rm)
    for nm, t, r in (("dq", q, rq), ("dk", k, rk), ("dv", v, rv)):
        check(f"{tag}/{nm}", t.grad, r)


def test_attend_bool_and_integer_masks_get_no_gradient():
    from osufusion_amd.modules.attention import Attend
    q, k, v = leaves(2, 1, 64, 32)
    for m in (torch.rand(64, 64, device=DEV) > 0.3, torch.ones(1, 1, 64, 64, device=DEV, dtype=torch.int32)):
        out = Attend()(q, k, v, attn_mask=m)
        out.sum().backward()
        assert q.grad is not None and torch.isfinite(q.grad).all()
        q.grad = k.grad = v.grad = None


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("D,N", [(64, 200), (32, 1000)])
def test_attend_repeated_kv_heads(kind, D, N):
    """k / v given with H identical heads (the unmasked forward runs them as one): one dK / dV per head, equal to the G = H reference."""
    from osufusion_amd.modules.attention import Attend
    H = 4
    k1, v1 = torch.randn(B, 1, N, D, device=DEV), torch.randn(B, 1, N, D, device=DEV)
    q = torch.randn(B, H, N, D, device=DEV).requires_grad_()
    k = k1.repeat(1, H, 1, 1).requires_grad_()
    v = v1.repeat(1, H, 1, 1).requires_grad_()
    mask = make_mask(kind, H, N)
    go = torch.randn(B, H, N, D, device=DEV).to(torch.bfloat16).float()
    att = Attend()
    out = att(q, k, v, attn_mask=mask)
    with torch.no_grad():
        assert torch.equal(out.detach(), att(q, k, v, attn_mask=mask))
    with torch.inference_mode():
        assert torch.equal(out.detach(), att(q, k, v, attn_mask=mask))
    out.backward(go)
    _, rq, rk, rv, _ = ref_grads(q, k, v, mask, go)
    for nm, t, r in (("dq", q, rq), ("dk", k, rk), ("dv", v, rv)):
        assert t.grad.shape == (B, H, N, D)
        check(f"repeated/{kind}/D{D}/N{N}/{nm}", t.grad, r)


def _ref_tables(N, dim, scale_base, theta=10000):
    """attention.py:33-47 on the GPU in fp32: positions scaled by scale_base / seq_len, emb = cat(freqs, freqs)."""
    inv_freq = 1.0 / (theta ** (torch.arange(0, dim, 2).float() / dim))
    t = torch.arange(N, dtype=torch.float32, device=DEV)
    t *= scale_base / N
    freqs = torch.einsum("i , j -> i j", t, inv_freq.to(DEV))
    emb = torch.cat([freqs, freqs], dim=-1)
    return emb.cos()[None, None], emb.sin()[None, None]


@pytest.mark.parametrize("N", [512, 520])
def test_rope_gradients(N):
    from osufusion_amd import functional as Fn
    from osufusion_amd.modules.attention import RotaryPositionEmbedding
    from osufusion_amd.modules.utils import apply_rotary_pos_emb
    D, H, sb = 64, 3, 4096
    rope = RotaryPositionEmbedding(D, scale_base=sb)
    q = torch.randn(B, H, N, D, device=DEV).requires_grad_()
    k = torch.randn(B, 1, N, D, device=DEV).requires_grad_()
    qo, ko = rope(q, k)
    assert qo.grad_fn is not None and ko.grad_fn is not None and qo.dtype == torch.float32
    with torch.no_grad():
        qn, kn = rope(q, k)
    assert torch.equal(qo.detach(), qn) and torch.equal(ko.detach(), kn)
    gq, gk = torch.randn_like(qo), torch.randn_like(ko)
    torch.autograd.backward([qo, ko], [gq, gk])
    c, s = Fn.rope_tables(N, D, sb, DEV)
    own = (torch.cat([c, c], -1)[None, None], torch.cat([s, s], -1)[None, None])
    for tables, tol, name in ((own, 1e-5, "own"), (_ref_tables(N, D, sb), 1e-3, "reference")):
        for x, g in ((q, gq), (k, gk)):
            xr = x.detach().clone().requires_grad_()
            apply_rotary_pos_emb(xr, *tables).backward(g)
            e = relmax(x.grad, xr.grad)
            report(f"rope_grad/N{N}/{name}", relmax=e)
            assert e < tol, (name, e)


def test_toy_block_end_to_end():
    """Linear -> RoPE -> Attend (causal) -> Linear, loss, backward: every parameter gradient within rel-L2 1e-2 of the same block in fp32 torch."""
    from osufusion_amd.modules.attention import Attend, RotaryPositionEmbedding
    from osufusion_amd.modules.utils import apply_rotary_pos_emb
    C, H, D, N = 96, 2, 64, 200
    to_qkv, to_out = torch.nn.Linear(C, 3 * H * D).to(DEV), torch.nn.Linear(H * D, C).to(DEV)
    rope, att = RotaryPositionEmbedding(D, scale_base=N), Attend()
    x = torch.randn(B, N, C, device=DEV)
    target = torch.randn(B, N, C, device=DEV)
    causal = make_mask("causal", H, N)

    def block(rope_fn, attend_fn):
        q, k, v = to_qkv(x).view(B, N, 3, H, D).permute(2, 0, 3, 1, 4)
        q, k = rope_fn(q, k)
        o = attend_fn(q, k, v)
        return F.mse_loss(to_out(o.permute(0, 2, 1, 3).reshape(B, N, H * D)), target)

    params = list(to_qkv.parameters()) + list(to_out.parameters())
    got = torch.autograd.grad(block(rope, lambda q, k, v: att(q, k, v, attn_mask=causal)), params)
    cos, sin = _ref_tables(N, D, N)
    want = torch.autograd.grad(block(lambda q, k: (apply_rotary_pos_emb(q, cos, sin), apply_rotary_pos_emb(k, cos, sin)),
                                     lambda q, k, v: F.scaled_dot_product_attention(q, k, v, attn_mask=causal)), params)
    for name, g, w in zip(("qkv.weight", "qkv.bias", "out.weight", "out.bias"), got, want):
        e = rell2(g, w)
        report(f"toy_block/{name}", rel_l2=e)
        assert e < 1e-2, (name, e)
