"""The hand-written references of tests/gemm_reference.py against torch.nn.functional, fp64 autograd and the per-row emulation of
tests/test_host_logic.py (CPU only), and the guard of the GPU file's caps.

tests/test_gemm_rows_gpu.py measures the HIP GEMMs against these functions, so a slip in one of them would either hide a kernel bug
or report one that is not there."""
import pytest
import torch
import torch.nn.functional as F

from tests import gemm_reference as G
from tests.bound_check import FLOOR
from tests.test_host_logic import emu_gemm_nt, emu_gemm_tn, emu_pack_weight, map_row
from tests.test_poisoned_memory import relmax, rell2

TOL = 1e-12                                                # fp64 against fp64
F64 = torch.float64


def _d(tag, shape, scale=1.0):
    return G.rnd(tag, shape, scale).double()


def _conv(kind, x, w, b=None):
    if kind == "same":
        return F.conv1d(x, w, b, padding=w.shape[2] // 2)
    if kind == "down":
        return F.conv1d(F.pad(x, (0, 1), mode="reflect"), w, b, stride=2)
    return F.conv1d(F.interpolate(x, scale_factor=2.0, mode="nearest"), w, b, padding=1)


def _rows(t):
    return t.detach().permute(0, 2, 1).reshape(-1, t.shape[1])


@pytest.mark.parametrize("mode,Lin,Lout,stride,pad,taps", [(0, 9, 9, 1, 1, 3), (0, 7, 7, 1, 7, 15), (0, 14, 7, 2, 1, 4), (1, 12, 6, 2, 0, 3),
                                                           (1, 2, 1, 2, 0, 3), (2, 7, 14, 1, 1, 3), (2, 14, 7, 2, 1, 4), (3, 6, 12, 1, 0, 4),
                                                           (3, 1, 2, 1, 0, 4)])
def test_rowmap_matches_the_scalar_form(mode, Lin, Lout, stride, pad, taps):
    want = torch.tensor([[map_row(i, t, Lin, Lout, stride, pad, mode) for i in range(Lout)] for t in range(taps)])
    assert torch.equal(G.rowmap(Lin, Lout, stride, pad, mode, taps), want)


@pytest.mark.parametrize("kind,k,L", [("same", 1, 9), ("same", 3, 12), ("same", 7, 10), ("same", 15, 20), ("down", 3, 12), ("down", 3, 2),
                                      ("up", 3, 7), ("up", 3, 1)])
def test_forward_and_gradients_vs_conv1d_autograd(kind, k, L):
    B, Cin, Cout = 3, 5, 4
    x, w, b = _d("x", (B, Cin, L)).requires_grad_(), _d("w", (Cout, Cin, k)).requires_grad_(), _d("b", (Cout,))
    want = _conv(kind, x, w, b)
    dy = _d("dy", tuple(want.shape))
    want.backward(dy)
    fwd, dgrad = G.geom(kind, k, L)
    wf, wd = emu_pack_weight(w.detach(), F64, kind)
    out, pre = G.epilogue(G.gemm_nt(_rows(x), wf, **fwd), b)
    assert out is pre and relmax(out, _rows(want)) < TOL
    assert relmax(G.gemm_nt(_rows(dy), wd, **dgrad), _rows(x.grad)) < TOL                  # modes 3 (down) and 0 with stride 2 (up)
    assert relmax(G.gemm_tn(_rows(dy), _rows(x), conv_layout=True, **fwd), w.grad) < TOL
    assert relmax(G.gemm_tn(_rows(dy), _rows(x), **fwd), w.grad.permute(2, 0, 1)) < TOL
    base = _d("base", (Cout, Cin, k))
    assert relmax(G.gemm_tn(_rows(dy), _rows(x), conv_layout=True, out=base, accumulate=True, **fwd), w.grad + base) < TOL


@pytest.mark.parametrize("kind,k,L", [("same", 3, 6), ("down", 3, 8), ("up", 3, 5)])
def test_against_the_per_row_emulation(kind, k, L):
    B, Cin, Cout = 2, 4, 3
    fwd, dgrad = G.geom(kind, k, L)
    a, dy = _d("a", (B * L, Cin)), _d("dy", (B * fwd["lout"], Cout))
    w, wd = _d("w", (fwd["taps"], Cout, Cin)), _d("wd", (dgrad["taps"], Cin, Cout))
    assert relmax(G.gemm_nt(a, w, **fwd), emu_gemm_nt(a, w, **fwd)) < 1e-6               # the emulation returns fp32
    assert relmax(G.gemm_nt(dy, wd, **dgrad), emu_gemm_nt(dy, wd, **dgrad)) < 1e-6
    assert relmax(G.gemm_tn(dy, a, **fwd), emu_gemm_tn(dy, a, **fwd)) < 1e-6
    assert relmax(G.gemm_tn(dy, a, conv_layout=True, **fwd), emu_gemm_tn(dy, a, conv_layout=True, **fwd)) < 1e-6
    assert relmax(G.gemm_nt(a, w, n_out=2, **fwd), emu_gemm_nt(a, w, **fwd)[:, :2]) < 1e-6


def test_epilogue_vs_functional():
    B, L, N = 3, 7, 8
    acc, bias = _d("acc", (B * L, N), 2.0), _d("bias", (N,))
    U, R, rs = _d("U", (B * L, N), 1.5).requires_grad_(), _d("R", (B * L, N)), 1 + 0.3 * _d("rs", (B, N))
    F.silu(U).sum().backward()                                                          # autograd's silu'
    gU, U = U.grad, U.detach()
    assert relmax(G.silu_grad(U), gU) < TOL
    out, pre = G.epilogue(acc, bias, 1)
    assert relmax(pre, acc + bias) < TOL and relmax(out, F.silu(acc + bias)) < TOL
    assert relmax(G.epilogue(acc, bias, 2)[0], torch.sigmoid(acc + bias)) < TOL
    assert relmax(G.epilogue(acc, None, 0, U=U)[0], acc * gU) < TOL
    want = F.silu(acc + bias) * gU + R * rs[:, None, :].expand(B, L, N).reshape(B * L, N)
    assert relmax(G.epilogue(acc, bias, 1, U, R, rs, L)[0], want) < TOL
    assert relmax(G.epilogue(acc, None, 0, None, R)[0], acc + R) < TOL


def test_colsum_and_rowdot_delta():
    Y, out = _d("Y", (37, 16)), _d("o", (16,))
    assert relmax(G.colsum(Y, out), torch.einsum("mn->n", Y) + out) < TOL
    B, L, heads = 2, 5, 3
    C, O = _d("C", (B * L, heads * 64)), _d("O", (B * L, heads * 64))
    want = torch.zeros(B, heads, L, dtype=F64)
    cb = C.bfloat16().double()
    for b in range(B):
        for h in range(heads):
            for l in range(L):
                want[b, h, l] = (cb[b * L + l, h * 64:(h + 1) * 64] * O[b * L + l, h * 64:(h + 1) * 64]).sum()
    assert relmax(G.rowdot_delta(C, O, L, heads), want) < TOL


def test_split_x3_and_its_product():
    t = _d("t", (64, 48)).float()
    hi, lo = G.split_x3(t)
    assert torch.equal(hi, t.bfloat16().float()) and torch.equal(lo, (t - hi).bfloat16().float())
    assert ((t - hi - lo).abs() <= 2.0 ** -16 * t.abs()).all()                         # two bf16 roundings: 2^-8 * 2^-8
    a, b = _d("a", (40, 64)).float().double(), _d("b", (24, 64)).float().double()
    mul = lambda p, q: p @ q.T
    got = G.x3_product(mul, a, b)
    (ah, al), (bh, bl) = G.split_x3(a), G.split_x3(b)
    assert relmax(got, (ah + al) @ (bh + bl).T - al @ bl.T) < TOL                        # everything but a_lo b_lo
    assert rell2(got, a @ b.T) < G.X3_L2
    ai = G.ints("ai", (8, 16), 3).double()
    assert torch.equal(G.x3_product(mul, ai, ai), ai @ ai.T)                            # integers: lo = 0


def test_named_kernels_follow_the_launchers():
    """The kernel each table entry names is the one the restated dispatch picks for it, and together they are every branch."""
    seen = set()
    for gid, kind, k, L, K, dg in G.GEOMETRIES:
        g = G.geom(kind, k, L)[1 if dg else 0]
        for mode, big in G.GEO_MODES:
            seen.add(G.nt_kernel(mode, G.GEO_B * g["lout"], G.GEO_N, K, g, big))
    for mode, L, K, no8p in G.HALO:
        seen.add(G.nt_kernel(mode, G.GEO_B * L, G.GEO_N, K, G.geom("same", 3, L)[0], True, no8p=no8p))
    for k, B, L in G.K8256:
        seen.add(G.nt_kernel("bf16", B * L, 256, 8256, G.geom("same", k, L)[0], True))
    for N, K, k, B, L in G.SKINNY_NT:
        seen.add(G.nt_kernel("bf16", B * L, N, K, G.geom("same", k, L)[0], False))
    assert seen == {"gemm_nt_glds_kernel<bf16>", "gemm_nt_glds_kernel<float>", "gemm_nt_glds_kernel<float, true>", "gemm_nt_big_kernel<bf16>",
                    "gemm_nt_big_kernel<float, true>", "gemm_nt_big8_kernel", "gemm_nt_big_halo3_kernel<bf16>", "gemm_nt_big_halo3_kernel<float>",
                    "gemm_nt_big8_halo3_kernel", "gemm_nt_skinny_kernel"}
    assert G.nt_kernel("bf16", 264, 256, 8256, G.geom("same", 1, 264)[0], True) == "gemm_nt_big_kernel<bf16>"
    assert G.nt_kernel("bf16", 256, 256, 8256, G.geom("same", 3, 256)[0], True) == "gemm_nt_big_halo3_kernel<bf16>"
    reduces = set()
    for cid, mode, B, L, N1, N2, kind, k, conv, acc, env, kernel, red in G.WGRAD_EXACT:
        M = B * G.geom(kind, k, L)[0]["lout"]
        if red is not None:
            assert G.reduce_kernel(kernel, M, N1, N2, k, conv, False) == red, cid
            reduces.add(red)
    for cid, B, L, N1, N2, k, conv, acc, kernel, red in G.WGRAD_PK:
        assert G.reduce_kernel(kernel, B * L, N1, N2, k, conv, True) == red, cid
        reduces.add(red)
    assert reduces == ({f"wgrad_reduce_kernel<{l}>" for l in (0, 1)} | {f"wgrad_reduce4_kernel<{l}>" for l in (0, 1)} |
                       {"wgrad_reduce_pk_kernel<1, 3>", "wgrad_reduce_pk_kernel<1, 1>", "wgrad_reduce_pk_kernel<0, 1>"})
    assert {c[11] for c in G.WGRAD_EXACT} == {"gemm_tn_kernel<bf16>", "gemm_tn_kernel<float>", "gemm_tn_kernel<float, true>", "gemm_tn_big_kernel",
                                              "gemm_tn_big_x3_kernel", "gemm_tn_taps3_kernel", "gemm_tn_taps3_x3_kernel", "gemm_tn_skinny_kernel"}


def test_exact_cases_stay_exact_in_fp32():
    """Section A relies on every partial sum being an integer below 2^24: |A| <= 3, |W| <= 2 (|dY| <= 3, |X| <= 2 for the weight gradients)."""
    worst = max([K * G.geom(kind, k, L)[1 if dg else 0]["taps"] for _, kind, k, L, K, dg in G.GEOMETRIES] + [8256 * 3] +
                [K * k for _, K, k, _, _ in G.SKINNY_NT] + [B * G.geom(kind, k, L)[0]["lout"] for _, _, B, L, _, _, kind, k, *_ in G.WGRAD_EXACT])
    assert worst * 6 < 2 ** 24


# ---------------------------------------------------------------------------------------------------------------------------------
# the caps never bind below fp32's own noise
# ---------------------------------------------------------------------------------------------------------------------------------
def _guard(e32, cap, what):
    assert 16 * e32 < cap, (what, e32, cap)
    assert FLOOR < cap


@pytest.mark.parametrize("name,mode,shape", list(G.epi_cases()), ids=lambda v: v if isinstance(v, str) else f"B{v['B']}L{v['L']}")
def test_caps_hold_sixteen_times_fp32_noise_epilogue(name, mode, shape):
    inp = G.epi_inputs(name, mode, **shape)
    x3 = mode == "x3"
    o64, p64 = G.epi_refs(inp, F64, x3)
    o32, p32 = G.epi_refs(inp, torch.float32, x3)
    _guard(relmax(o32, o64), G.OUT_CAP, "out")
    _guard(relmax(p32, p64), G.OUT_CAP, "pre")
    if name == "product" and mode == "f32":
        _guard(rell2(o32, o64), G.PROD_CAP_L2, "product")
    if x3:
        assert rell2(o64, G.epi_refs(inp, F64, False)[0]) < G.X3_L2 / 4                 # the split itself leaves room under the project's 3e-5


@pytest.mark.parametrize("mode", ["bf16", "f32", "x3"])
def test_caps_hold_sixteen_times_fp32_noise_rowdot_colsum(mode):
    r = G.rowdot_inputs(mode)
    mul = lambda a, w: G.gemm_nt(a, w)
    for dt in (F64, torch.float32):
        A, W, O = r["A"].to(dt), r["W"].to(dt), r["O"].to(dt)
        c = G.x3_product(mul, A, W) if mode == "x3" else mul(A, W)
        d = G.rowdot_delta(c.double(), O, G.ROWDOT["L"], G.ROWDOT["heads"])            # delta is taken from the SAME stored C in both precisions
        if dt == F64:
            c64, d64 = c, d
    _guard(relmax(c, c64), G.OUT_CAP, "rowdot C")
    d32 = G.rowdot_delta(c64, r["O"].float(), G.ROWDOT["L"], G.ROWDOT["heads"])
    _guard(relmax(d32, d64), G.OUT_CAP, "delta")
    if mode != "x3":
        for M in G.COLSUM_M:
            for N in G.COLSUM_N:
                y, out = G.colsum_inputs(M, N, mode)
                _guard(rell2(G.colsum(y[:, :N], out), G.colsum(y[:, :N].double(), out.double())), G.OUT_CAP, ("colsum", M, N))
