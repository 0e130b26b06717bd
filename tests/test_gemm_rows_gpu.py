"""The tap-GEMMs of csrc/gemm.hip and their epilogues against plain fp64 references, on every branch gemm_nt_launch, gemm_tn_launch,
launch_wgrad_reduce and osuf_colsum pick from.  Every launch is checked on inputs of its own; none consumes another kernel's output.

References and case tables: tests/gemm_reference.py (checked on the CPU by tests/test_gemm_reference_cpu.py, which also holds every cap
used here above 16 x the fp32 evaluation's own noise).  Kernels are forced with the switches the suite already uses
(ops.force(gemm_big=, no8p=, wgrad_f32_partials=), ops.set_f32_matmul); the kernel each case reaches is named in its
table entry (gemm_reference.nt_kernel / the WGRAD tables) and listed from a kernel trace in profiles/gemm_sweep.md.

A. Geometry, exact: operands are small integers (|A| <= 3, |W| <= 2), so every partial sum is an integer below 2^24, exact in fp32 in any
   order and through atomics, and the x3 split has lo = 0: torch.equal against the fp64 result cast once to the storage dtype.
B. Epilogue, real-valued, bounded (tests/bound_check.py): an fp32 result within 16 x e32 of the fp64 reference evaluated on the inputs the
   kernel saw, e32 being the fp32 CPU evaluation's own distance, floored at 1e-6 and capped at 2e-5 (relmax; 2e-6 rel-L2 for the exact-f32
   product); a bf16-stored result within 2^-7 |ref| + bound * max|ref| element by element; silu / sigmoid add FAST = 2^-21, silu'(U) adds
   FAST * (1 + max|U|).  x3 is held to the fp64 sum of the three products mfma_x3 issues, and that to 3e-5 rel-L2 of the unsplit product.
   GroupNorm sums are referenced from the kernel's own stored output (1e-5), delta from bf16(C as stored) . O.
"""
import contextlib

import pytest
import torch

from osufusion_amd import _lib, ops
from tests import bound_check
from tests import gemm_reference as G
from tests.test_poisoned_memory import relmax, rell2

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
SENT = 777.0


EPI_IDS = lambda v: v if isinstance(v, str) else ("big" if v else "128")


class Check(bound_check.Check):
    prefix = "gemm_rows"


def sdt(mode):
    return BF16 if mode == "bf16" else F32


def dev(t, mode):
    return None if t is None else t.to(sdt(mode)).to(DEV)


@pytest.fixture()
def force():
    """force(mode, big=None|bool, no8p, env=ops.force keywords): sets the compute mode and the dispatch overrides for the test, all others at their default."""
    with contextlib.ExitStack() as stack:
        def set_(mode, big=None, no8p=False, env=None):
            stack.enter_context(ops.force(gemm_big=None if big is None else int(big), no8p=no8p, nohalo=None, wgrad_f32_partials=None))
            stack.enter_context(ops.force(**(env or {})))
            stack.callback(ops.set_f32_matmul, ops.set_f32_matmul("x3" if mode == "x3" else "exact"))

        yield set_


# ---------------------------------------------------------------------------------------------------------------------------------
# A. geometry, exact
# ---------------------------------------------------------------------------------------------------------------------------------
def exact_nt(mode, B, N, K, g):
    """Integer operands through ops.gemm_nt against the fp64 product cast once to the storage dtype: equal, no tolerance."""
    A, W = G.ints("A", (B * g["lin"], K), 3), G.ints("W", (g["taps"], N, K), 2)
    got = ops.gemm_nt(dev(A, mode), dev(W, mode), None, **g)
    want = G.gemm_nt(A.double(), W.double(), **g).to(sdt(mode))
    assert got.shape == want.shape
    bad = (got.cpu() != want).nonzero()
    assert torch.equal(got.cpu(), want), (len(bad), bad[:8].tolist())


@pytest.mark.parametrize("mode,big", G.GEO_MODES, ids=EPI_IDS)
@pytest.mark.parametrize("gid,kind,k,L,K,dgrad", [pytest.param(*c, id=c[0]) for c in G.GEOMETRIES])
def test_geometry_exact(force, gid, kind, k, L, K, dgrad, mode, big):
    force(mode, big)
    exact_nt(mode, G.GEO_B, G.GEO_N, K, G.geom(kind, k, L)[1 if dgrad else 0])


@pytest.mark.parametrize("mode,L,K,no8p", [pytest.param(*c, id=f"{c[0]}_L{c[1]}_K{c[2]}_{'1barrier' if c[3] else 'default'}") for c in G.HALO])
def test_shared_panel_k3_exact(force, mode, L, K, no8p):
    g = G.geom("same", 3, L)[0]
    assert "halo3" in G.nt_kernel(mode, G.GEO_B * L, G.GEO_N, K, g, True, no8p=no8p)
    force(mode, True, no8p)
    exact_nt(mode, G.GEO_B, G.GEO_N, K, g)


@pytest.mark.parametrize("k,B,L", G.K8256)
def test_k_above_8192_falls_back_exact(force, k, B, L):
    """K = 8256 > 8192 without ops.force(no8p=True): gemm_nt_big8_kernel / gemm_nt_big8_halo3_kernel hand over to the one-barrier loops."""
    force("bf16", True)
    exact_nt("bf16", B, 256, 8256, G.geom("same", k, L)[0])


@pytest.mark.parametrize("N,K,k,B,L", G.SKINNY_NT)
def test_skinny_n_exact(force, N, K, k, B, L):
    g = G.geom("same", k, L)[0]
    assert G.nt_kernel("bf16", B * L, N, K, g, False) == "gemm_nt_skinny_kernel"
    force("bf16")
    exact_nt("bf16", B, N, K, g)


@pytest.mark.parametrize("cid,mode,B,L,N1,N2,kind,k,conv,acc,env,kernel,red", [pytest.param(*c, id=c[0]) for c in G.WGRAD_EXACT])
def test_wgrad_exact(force, cid, mode, B, L, N1, N2, kind, k, conv, acc, env, kernel, red):
    force(mode, env=env)
    g = G.geom(kind, k, L)[0]
    dY, X = G.ints("dY", (B * g["lout"], N1), 3), G.ints("X", (B * L, N2), 2)
    base = G.ints("base", (N1, N2, k) if conv else (k, N1, N2), 5)
    got = ops.gemm_tn(dev(dY, mode), dev(X, mode), conv_layout=conv, accumulate=acc, out=base.to(DEV) if acc else None, **g)
    want = G.gemm_tn(dY.double(), X.double(), conv_layout=conv, accumulate=acc, out=base.double(), **g).float()
    assert torch.equal(got.cpu(), want), (got.cpu() != want).nonzero()[:8].tolist()


def test_wgrad_256_tile_atomics_without_workspace(force):
    """osuf_gemm_tn with workspace = NULL: the 256^2 kernel adds its partial tiles into dW with fp32 atomics (the path the header documents
    and ops.gemm_tn, which always brings a workspace, never takes)."""
    force("bf16")
    M, N1, N2 = 2048, 256, 64
    assert _lib.load().osuf_gemm_tn_workspace_bytes(ops.BF16, M, N1, N2, 1) > 0          # the 256^2 plan applies to this shape
    dY, X = G.ints("dY", (M, N1), 3), G.ints("X", (M, N2), 2)
    dy, x = dev(dY, "bf16"), dev(X, "bf16")
    want = G.gemm_tn(dY.double(), X.double()).float()
    for acc in (0, 1):
        out = torch.full((1, N1, N2), 3.0 if acc else SENT, device=DEV)
        ops.call("osuf_gemm_tn", ops.BF16, dy.data_ptr(), N1, x.data_ptr(), N2, out.data_ptr(), N2, N1 * N2, M, N1, N2, 1, M, M, 1, 0, 0, 0, 0, acc,
                 None, 0, torch.cuda.current_stream().cuda_stream)
        assert torch.equal(out.cpu(), want + 3.0 if acc else want)


@pytest.mark.parametrize("cid,B,L,N1,N2,k,conv,acc,kernel,red", [pytest.param(*c, id=c[0]) for c in G.WGRAD_PK])
def test_wgrad_bf16_pair_partials(force, cid, B, L, N1, N2, k, conv, acc, kernel, red):
    """The bf16-pair partial tiles round once per split, so they cannot be exact: real-valued operands, 3e-3 rel-L2 against fp64."""
    force("bf16")
    g = G.geom("same", k, L)[0]
    dY, X = G.wgrad_pk_inputs(B, L, N1, N2)
    base = G.rnd("pk_base", (N1, N2, k) if conv else (k, N1, N2))
    got = ops.gemm_tn(dev(dY, "bf16"), dev(X, "bf16"), conv_layout=conv, accumulate=acc, out=base.to(DEV) if acc else None, **g)
    want = G.gemm_tn(dY.double(), X.double(), conv_layout=conv, **g)
    ck = Check("wgrad_pk", "bf16", case=cid)
    ck.fixed("dw", rell2(got.cpu().double() - (base.double() if acc else 0), want), G.PK_L2)
    ck.done()


# ---------------------------------------------------------------------------------------------------------------------------------
# B. epilogue, real-valued, bounded
# ---------------------------------------------------------------------------------------------------------------------------------
def stats_err(stats, stored, B):
    y = stored.double().cpu().reshape(B, -1)
    want = torch.stack([y.sum(1), (y * y).sum(1)], 1)
    return ((stats.cpu() - want).abs() / want.abs().clamp_min(1e-30)).max().item()


def epi_case(name, mode, B, L, K, N, k, tagname="epilogue", **where):
    inp = G.epi_inputs(name, mode, B, L, K, N, k)
    o = G.EPI[name]
    x3 = mode == "x3"
    stats = torch.zeros(B, 2, dtype=F64, device=DEV) if o.get("stats") else None
    res = ops.gemm_nt(dev(inp["A"], mode), dev(inp["W"], mode), None if inp["bias"] is None else inp["bias"].to(DEV), act=inp["act"],
                      residual=dev(inp["R"], mode), dact=dev(inp["U"], mode), rscale=None if inp["rscale"] is None else inp["rscale"].to(DEV),
                      stats=stats, want_pre=bool(o.get("want_pre")), **inp["g"])
    out, pre = res if o.get("want_pre") else (res, None)
    o64, p64 = G.epi_refs(inp, F64, x3)
    o32, p32 = G.epi_refs(inp, F32, x3)
    ck = Check(tagname, mode, case=name, B=B, L=L, **where)
    ck.out("out", out, o64, o32, G.OUT_CAP, G.epi_extra(inp))
    if pre is not None:
        ck.out("pre", pre, p64, p32, G.OUT_CAP)
    if name == "product" and mode == "f32":
        ck.f32("product_l2", out, o64, o32, rell2, G.PROD_CAP_L2)
    if x3:
        ck.fixed("x3_vs_unsplit", rell2(o64, G.epi_refs(inp, F64, False)[0]), G.X3_L2)
        ck.fixed("got_vs_unsplit", rell2(out.cpu(), G.epi_refs(inp, F64, False)[0]), G.X3_L2)
    if stats is not None:
        ck.fixed("stats", stats_err(stats, out, B), 1e-5)
    ck.done()


@pytest.mark.parametrize("mode,big", G.EPI_MODES, ids=EPI_IDS)
@pytest.mark.parametrize("name", list(G.EPI))
def test_epilogue(force, name, mode, big):
    force(mode, big)
    epi_case(name, mode, **G.EPI_SHAPE, big=int(big))


@pytest.mark.parametrize("mode,big", G.EPI_MODES, ids=EPI_IDS)
@pytest.mark.parametrize("B,L", G.BOUNDARY)
@pytest.mark.parametrize("name", G.BOUNDARY_EPI)
def test_epilogue_sample_boundaries(force, name, B, L, mode, big):
    """Several samples per tile (L = 40) and per 8-row pass of the 256^2 epilogue (L = 12): the per-lane sample tracking of stats and rscale."""
    force(mode, big)
    epi_case(name, mode, **dict(G.EPI_SHAPE, B=B, L=L), tagname="epilogue_boundary", big=int(big))


@pytest.mark.parametrize("mode,big", G.EPI_MODES, ids=EPI_IDS)
def test_rowdot(force, mode, big):
    force(mode, big)
    L, heads = G.ROWDOT["L"], G.ROWDOT["heads"]
    r = G.rowdot_inputs(mode)
    C, delta = ops.gemm_nt_rowdot(dev(r["A"], mode), dev(r["W"], mode), dev(r["O"], mode), L, heads)
    mul = lambda a, w: G.gemm_nt(a, w)
    ref = lambda dt: (G.x3_product if mode == "x3" else (lambda m, a, w: m(a, w)))(mul, r["A"].to(dt), r["W"].to(dt))
    ck = Check("rowdot", mode, big=int(big))
    ck.out("C", C, ref(F64), ref(F32), G.OUT_CAP)
    if mode == "f32":
        ck.f32("C_l2", C, ref(F64), ref(F32), rell2, G.OUT_CAP)
    stored_c = C.cpu().double()                                  # a rounding flip in C does not count against delta
    ck.f32("delta", delta, G.rowdot_delta(stored_c, r["O"].double(), L, heads), G.rowdot_delta(stored_c, r["O"], L, heads), relmax, G.OUT_CAP)
    ck.done()


@pytest.mark.parametrize("name,big,mode", [(n, b, m) for n, b in G.STRIDED for m in ("bf16", "f32", "x3") if not (b and m == "f32")], ids=EPI_IDS)
def test_strided_operands(force, name, big, mode):
    """A, C, R and U are column slices of wider buffers (ld > width), n_out is smaller than W's row count, and the slack columns of C hold
    a sentinel that must survive.  (The pre-activation copy is a dense tensor of its own: its row stride differs from C's.)"""
    force(mode, big)
    B, L, K, N, Nw = 2, 200, 64, 328, 344
    inp = G.epi_inputs(name, mode, B, L, K, Nw, 1)
    inp["bias"] = 0.5 * G.rnd("sbias", (N,))
    wide = lambda t, pad, fill=0.0: None if t is None else torch.cat([torch.full((t.shape[0], 8), fill), t, torch.full((t.shape[0], pad), fill)], 1)
    a = dev(wide(inp["A"], 16), mode)[:, 8:8 + K]
    r = None if inp["R"] is None else dev(wide(inp["R"][:, :N], 24), mode)[:, 8:8 + N]
    u = None if inp["U"] is None else dev(wide(inp["U"][:, :N], 40), mode)[:, 8:8 + N]
    cbuf = torch.full((B * L, N + 32), SENT, dtype=sdt(mode), device=DEV)
    out, pre = ops.gemm_nt(a, dev(inp["W"], mode), inp["bias"].to(DEV), n_out=N, residual=r, dact=u, out=cbuf[:, 8:8 + N], want_pre=True, **inp["g"])
    assert pre.shape == (B * L, N)
    keep = torch.ones(N + 32, dtype=torch.bool)
    keep[8:8 + N] = False
    assert (cbuf.cpu()[:, keep] == SENT).all()
    x3 = mode == "x3"
    ref_in = dict(inp, W=inp["W"][:, :N], R=None if inp["R"] is None else inp["R"][:, :N], U=None if inp["U"] is None else inp["U"][:, :N])
    o64, p64 = G.epi_refs(ref_in, F64, x3)
    o32, p32 = G.epi_refs(ref_in, F32, x3)
    ck = Check("strided", mode, case=name, big=int(big))
    ck.out("out", out.contiguous(), o64, o32, G.OUT_CAP, G.epi_extra(ref_in))
    ck.out("pre", pre, p64, p32, G.OUT_CAP)
    ck.done()


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("N", G.COLSUM_N)
@pytest.mark.parametrize("M", G.COLSUM_M)
def test_colsum(M, N, mode):
    """ld = N + 8 > N, into a non-zero out."""
    y, out0 = G.colsum_inputs(M, N, mode)
    got = ops.colsum(dev(y, mode)[:, :N], N, out0.clone().to(DEV))
    ck = Check("colsum", mode, M=M, N=N)
    ck.f32("sum", got, G.colsum(y[:, :N].double(), out0.double()), G.colsum(y[:, :N], out0), rell2, G.OUT_CAP)
    ck.done()
