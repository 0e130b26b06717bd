"""tests/attn_reference.py against itself (no GPU): the fp64 reference against torch.autograd of the textbook formula, and the conditions
that keep tests/test_attn_exact_gpu.py from passing vacuously -- every operand of every case survives bf16, the general reference
reproduces the closed forms, every 32-query block reaches the first and the last key tile and the last valid key, and the shifted cases
push lse2 beyond +-128 on every row."""
import pytest
import torch

from tests import attn_reference as R

F64 = torch.float64
SHAPES = sorted({(D, N) for D in R.HEAD_DIMS for N in R.LENGTHS} | {(64, N) for N in R.LENGTHS_512})     # every (D, N) of the GPU file


def _relmax(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


@pytest.mark.parametrize("G,Nq,Nk,masked", [(1, 37, 37, False), (2, 33, 70, True), (4, 5, 129, True), (1, 64, 9, False)])
def test_reference_vs_fp64_autograd(G, Nq, Nk, masked):
    B, H, D = 2, 4, 16
    q = torch.randn(B, H, Nq, D, dtype=F64, requires_grad=True)
    k = torch.randn(B, G, Nk, D, dtype=F64, requires_grad=True)
    v = torch.randn(B, G, Nk, D, dtype=F64, requires_grad=True)
    bias = torch.randn(B, 1, Nq, Nk, dtype=F64, requires_grad=True) if masked else None
    do = torch.randn(B, H, Nq, D, dtype=F64)
    r = H // G
    s = (q @ k.repeat_interleave(r, 1).transpose(-1, -2)) * 0.3 + (bias if masked else 0.0)
    o = s.softmax(-1) @ v.repeat_interleave(r, 1)
    o.backward(do)
    got = R.attention_fp64(q.detach(), k.detach(), v.detach(), do, 0.3, None if bias is None else bias.detach())
    assert _relmax(got["o"], o.detach()) < 1e-13
    assert _relmax(got["lse2"], torch.logsumexp(s.detach(), -1) * R.LOG2E) < 1e-13
    assert _relmax(got["dq"], q.grad) < 1e-12 and _relmax(got["dk"], k.grad) < 1e-12 and _relmax(got["dv"], v.grad) < 1e-12
    assert _relmax(got["delta"], (do * o.detach()).sum(-1)) < 1e-13
    if masked:
        assert _relmax(got["dbias"].sum(1, keepdim=True), bias.grad) < 1e-12


def _check_closed(c, ref):
    cl = c.closed
    assert (ref["o"] - cl["o"]).abs().max() <= 1e-12
    assert (ref["lse2"] - cl["lse2"]).abs().max() <= 1e-12 * max(1.0, cl["lse2"].abs().max().item())
    zs = c.zero_scale * c.s                                            # what cancels in dq / dk (see the GPU sweep's zero bound)
    for key in ("dq", "dk", "dv"):
        top = cl[key].abs().max().item()                               # a quantity that is exactly zero: relative to what cancels in it
        assert (ref[key] - cl[key]).abs().max() <= 1e-12 * (max(1.0, top) if top > 0 else zs), key
    assert (ref["dbias"] - R.closed_dbias(c)).abs().max() <= 1e-12 * c.zero_scale


@pytest.mark.parametrize("kind,D,N", [(kind, D, N) for kind in ("selector", "tie") for D, N in SHAPES if kind == "selector" or N >= 2])   # a tie needs two keys
def test_constructions(kind, D, N):
    for shift in (0, -1, 1):
        H, G = (4, 2) if N <= 257 else (2, 1)
        c = R.make_case(kind, 1 if N > 513 else 2, N, N, H, G, D, shift=shift, seed=3)
        for name in ("q", "k", "v", "do"):
            assert R.is_bf16(getattr(c, name)), name
        if D == 64:                                                    # the pre-scaled-query kernels: scores leave the MFMA chain as exponents
            assert (c.q.abs().unique().numel() <= 2 + (shift != 0))    # 0, one magnitude (+ the shift column): a tie survives any rounding of it
        for b in range(c.B):
            for h in range(c.H):
                assert not R.map_conditions(c.pa[b, h], N), (b, h)
        assert not R.map_coverage([c.pa[b, h] for b in range(c.B) for h in range(c.H)], N)     # tail blocks: between the heads
        ref = R.attention_fp64(c.q, c.k, c.v, c.do, c.scale)
        _check_closed(c, ref)
        if kind == "tie":                                              # both weights 1/2, dS a multiple of 1/2 of magnitude <= 2: exact in bf16
            ds = ref["dbias"]
            top2 = torch.softmax((c.q @ c.k.repeat_interleave(c.H // c.G, 1).transpose(-1, -2)) * c.scale, -1).topk(2, -1).values
            assert (top2 - 0.5).abs().max() == 0.0
            big = ds.abs() > 1e-9
            assert ((ds[big] * 2).round() == ds[big] * 2).all() and ds.abs().max() <= 2.0 and big.any()
            assert ref["dq"].abs().max() > 0 and ref["dk"].abs().max() > 0
        else:
            assert torch.equal(c.closed["o"], torch.gather(c.v.repeat_interleave(c.H // c.G, 1), 2, c.pa[..., None].expand(-1, -1, -1, D)))
        if shift < 0:
            assert ref["lse2"].max() < -128 and ref["lse2"].min() > -1000
        if shift > 0:
            assert ref["lse2"].min() > 128


@pytest.mark.parametrize("Nq,Nk", R.CROSS_LENGTHS)
@pytest.mark.parametrize("D", R.HEAD_DIMS)
def test_cross_constructions(D, Nq, Nk):
    for kind in ("selector",) + (("tie",) if Nk >= 2 else ()):
        for shift in (0, -1):
            c = R.make_case(kind, 2, Nq, Nk, 2, 1, D, shift=shift, seed=5)
            assert all(R.is_bf16(getattr(c, n)) for n in ("q", "k", "v", "do"))
            assert all(not R.map_conditions(c.pa[b, h], Nk) for b in range(2) for h in range(2))
            assert not R.map_coverage([c.pa[b, h] for b in range(2) for h in range(2)], Nk)
            ref = R.attention_fp64(c.q, c.k, c.v, c.do, c.scale)
            _check_closed(c, ref)
            assert shift == 0 or ref["lse2"].max() < -128


@pytest.mark.parametrize("form", R.BIAS_FORMS)
@pytest.mark.parametrize("kind", ["selector", "tie", "bool"])
def test_bias_constructions(kind, form):
    for D, (Nq, Nk) in [(D, L) for D in R.HEAD_DIMS for L in R.CROSS_LENGTHS if kind == "selector" or L[1] >= 2]:   # the GPU file's masked table
        c = R.make_bias_case(kind, 2, Nq, Nk, 3, D, form, seed=1)
        assert all(R.is_bf16(getattr(c, n)) for n in ("q", "k", "v", "do", "bias"))
        assert tuple(c.bias.shape) == (2 if "b" in form else 1, 3 if "h" in form else 1, Nq if "q" in form else 1, Nk)
        ref = R.attention_fp64(c.q, c.k, c.v, c.do, c.scale, c.bias)
        assert (ref["o"] - c.closed["o"]).abs().max() <= 1e-12 and (ref["lse2"] - c.closed["lse2"]).abs().max() <= 1e-12
        assert (ref["dbias"] - R.closed_dbias(c)).abs().max() <= 1e-12 * c.zero_scale
        assert ref["dk"].abs().max() == 0.0                            # q = 0
        if kind != "selector":
            assert ref["dbias"].abs().max() > 0 and ref["dq"].abs().max() > 0


@pytest.mark.parametrize("D", R.HEAD_DIMS)
def test_quarter_turn_tables(D):
    N = 257
    cos, sin = R.quarter_tables(N, D)
    assert cos.shape == sin.shape == (N, D // 2) and ((cos.abs() + sin.abs()) == 1).all() and (cos * sin == 0).all()
    turns = (cos == 1) * 0 + (sin == 1) * 1 + (cos == -1) * 2 + (sin == -1) * 3
    assert all((turns == t).sum() > N * D // 2 // 8 for t in range(4))            # every turn is used, and
    assert (turns[1:] != turns[:-1]).any(1).all()                                 # every position differs from its neighbour
    x = torch.randint(-7, 8, (2, N, D)).to(F64)
    y = R.rope(x, cos, sin)
    assert torch.equal(R.rope(y, cos, sin, inverse=True), x) and torch.equal(y.abs().sort(-1).values, x.abs().sort(-1).values)
    g = torch.randn(2, N, D, dtype=F64)                                           # the inverse is the transpose: <R x, g> = <x, R^T g>
    assert abs((y * g).sum() - (x * R.rope(g, cos, sin, inverse=True)).sum()) < 1e-9
