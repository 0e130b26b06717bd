"""The UNet row kernels of csrc/norm.hip against plain fp64 references, on every branch their launchers pick from C, L and M.

References: tests/norm_reference.py (checked on the CPU by tests/test_norm_reference_cpu.py), evaluated in fp64 on the inputs the kernel
saw (in bf16 mode the bf16-rounded ones).  Bounds are not taken from the kernels: for an output of fp32 arithmetic the same reference is
also evaluated in fp32 torch on the CPU, e32 is its distance to the fp64 result in the same metric (relmax for elementwise outputs, rell2
for reduced ones) and the bound is 16 * e32 (a different summation order, atomics), at least 1e-6 and never above what the suite already
asks of the quantity (5e-5 forward, 1.5e-4 gradients).  A bf16-stored output must lie within one bf16 spacing of the reference plus that
fp32 term: |got - ref| <= 2^-7 |ref| + bound * max|ref|.  Every achieved figure goes to the suite's parity metrics file (report()).
"""
import pytest
import torch

from osufusion_amd import ops
from tests import bound_check
from tests import norm_reference as R
from tests.test_hip_parity import report
from tests.test_poisoned_memory import relmax, rell2, rnd

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = torch.float32, torch.float64
DTYPES = [torch.float32, torch.bfloat16]
FWD_CAP, GRAD_CAP, FLOOR = 5e-5, 1.5e-4, 1e-6
# sigmoid_f = v_rcp_f32(1 + __expf(-u)) and the softmax kernels' __expf: v_exp_f32 and v_rcp_f32 are documented at 1 ulp each, and
# __expf's argument product u * log2(e) adds |u| * 2^-24 to the exponent, which reaches the result weighted by |u| e^-|u| <= 0.37.  With
# the add and the final multiply that is under 4 ulp of the result = 4 * 2^-23 = 2^-21, the term added where a kernel uses them.
FAST = 2.0 ** -21
SENT = 777.0

ROW_C = [8, 24, 96, 512, 520, 1024, 1032, 1536, 1544, 2048]      # G = 1 | 4, one lane masked | anchor | nch 1 full | 2, 2 full | 3, 3 full | 4, 4 full
COL_C = [8, 40, 264, 1024, 1032, 2048]                           # rp = 256 | 51 (1 idle) | 7 (25 idle) | 2 | 1 (127 idle) | 1
# the row-skeleton cases run M = 129 rows (B = 3, L = 43 where a kernel has samples): odd, so no multiple of the 64 / G rows of a wave
# for any G < 64, and 129 = 2 * 64 + 1 leaves a tail of exactly one row at every G (2 * 67 would leave six at G = 1)
RB, RL = 3, 43


def dev(t, dtype=F32):
    return t.to(dtype).to(DEV)


def tag(dtype):
    return "f32" if dtype == F32 else "bf16"


class Check(bound_check.Check):
    prefix = "norm_rows"


def affine(C):
    return dev(1 + 0.3 * rnd("gamma", (C,))), dev(0.2 * rnd("beta", (C,)))


# ---------------------------------------------------------------------------------------------------------------------------------
# row skeleton: LayerNorm, rowdot
# ---------------------------------------------------------------------------------------------------------------------------------
def ln_case(M, C, dtype, fwd=True, bwd=True):
    x = dev(rnd("x", (M, C)) * 1.5 + 0.5, dtype)
    dy = dev(rnd("dy", (M, C)) + 0.3, dtype)
    gamma, beta = affine(C)
    ck = Check("ln", dtype, C=C, M=M)
    a64, a32 = R.cast(F64, x, gamma, beta), R.cast(F32, x, gamma, beta)
    o64, mr64 = R.layer_norm(*a64)
    o32, mr32 = R.layer_norm(*a32)
    if fwd:
        out, mr = ops.ln_fwd(x, gamma, beta)
        ck.out("out", out, o64, o32, FWD_CAP)
        ck.f32("mean", mr[:, 0], mr64[:, 0], mr32[:, 0], relmax, FWD_CAP)
        ck.f32("rstd", mr[:, 1], mr64[:, 1], mr32[:, 1], relmax, FWD_CAP)
    if bwd:
        g64, g32 = R.ln_grads(*a64, dy.double().cpu()), R.ln_grads(*a32, dy.float().cpu())
        dx, dg, db = ops.ln_bwd(dy, x, dev(mr64), gamma)
        ck.out("dx", dx, g64["dx"], g32["dx"], GRAD_CAP)
        ck.f32("dgamma", dg, g64["dgamma"], g32["dgamma"], rell2, GRAD_CAP)
        ck.f32("dbeta", db, g64["dbeta"], g32["dbeta"], rell2, GRAD_CAP)
    ck.done()


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("C", ROW_C)
def test_ln_fwd_bwd(C, dtype):
    ln_case(RB * RL, C, dtype)


# osuf_ln_bwd: blocks of nt / 64 waves x 64 / G rows, capped at 256 (512 for nt = 256): one row more than the cap covers, so that the
# grid-stride loop takes a second trip in one wave and every other wave runs it once
@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("C,M", [(8, 256 * 1024 + 1), (512, 256 * 16 + 1), (1024, 256 * 8 + 1), (2048, 512 * 4 + 1)])
def test_ln_bwd_above_block_cap(C, M, dtype):
    ln_case(M, C, dtype, fwd=False)


def rowdot_case(B, L, C, dtype):
    h = dev(rnd("h", (B, L, C)), dtype)
    w, ws, bias = dev(rnd("w", (C,)) / C ** 0.5), dev(rnd("ws", (B, C)) / C ** 0.5), dev(rnd("bias", (1,)))
    ck = Check("rowdot", dtype, C=C, M=B * L)
    for key, wv, bv, per in (("shared", w, bias, False), ("per_sample", ws, None, True)):
        def ref(dt):
            hh, ww, bb = R.cast(dt, h, wv, bv)
            r = torch.einsum("blc,bc->bl", hh, ww) if per else hh @ ww
            return (r if bb is None else r + bb).reshape(-1)
        ck.f32(key, ops.rowdot(h, wv, bv, L, per_sample=per), ref(F64), ref(F32), rell2, FWD_CAP)
    ck.done()


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("C", ROW_C)
def test_rowdot(C, dtype):
    rowdot_case(RB, RL, C, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
def test_ln_fwd_rowdot_above_block_cap(dtype):
    """row_grid: 4 waves x 64 / G rows per block, capped at 4096 blocks -- C = 512 (one row per wave), one row above the cap."""
    M = 4096 * 4 + 1
    ln_case(M, 512, dtype, bwd=False)
    rowdot_case(1, M, 512, dtype)


# ---------------------------------------------------------------------------------------------------------------------------------
# GlobalContext: pooling, gate / residual, backward
# ---------------------------------------------------------------------------------------------------------------------------------
def gca_inputs(B, L, C, dtype):
    h = dev(rnd("h", (B, L, C)), dtype)
    return h, dev(2 * rnd("wk", (C,)) / C ** 0.5), dev(rnd("bk", (1,)))


def pool_case(B, L, C, dtype):
    h, wk, bk = gca_inputs(B, L, C, dtype)
    p64, pooled64 = R.gca_pool(*R.cast(F64, h, wk, bk))
    p32, pooled32 = R.gca_pool(*R.cast(F32, h, wk, bk))
    pooled, p = ops.gca_pool(h, wk, bk, L)
    ck = Check("gca_pool", dtype, C=C, L=L, B=B)
    ck.f32("p", p.view(B, L), p64, p32, relmax, FWD_CAP, FAST)
    ck.f32("pooled", pooled, pooled64, pooled32, rell2, FWD_CAP, FAST)
    ck.done()


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("C", ROW_C)
def test_gca_pool(C, dtype):
    pool_case(RB, RL, C, dtype)


# 32 rows per workgroup (M < 65536): a single row, one short of / one past a workgroup, several workgroups with a ragged last one --
# at 64 rows per wave (C = 8), several rows per wave (96) and one row per wave with the NCH = 4 template (1032)
@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("L", [1, 31, 33, 200])
@pytest.mark.parametrize("C", [8, 96, 1032])
def test_gca_pool_row_blocks(C, L, dtype):
    pool_case(2, L, C, dtype)


# gca_pool_rows_per_block: 64 rows from M = 65536, 128 from M = 131072 (the workspace stays sized for 32); L no multiple of 128
@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("L", [32800, 65570])
def test_gca_pool_wide_row_blocks(L, dtype):
    pool_case(2, L, 8, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("C", ROW_C)
def test_gate_residual(C, dtype):
    B, L = RB, RL
    h, res = dev(rnd("h", (B, L, C)), dtype), dev(rnd("res", (B, L, C)), dtype)
    gate = dev(torch.sigmoid(rnd("gate", (B, C))))
    ck = Check("gate_residual", dtype, C=C)
    for key, r in (("gated", None), ("gated_res", res)):
        ck.out(key, ops.gate_residual(h, gate, r, L), R.gate_residual(*R.cast(F64, h, gate, r)), R.gate_residual(*R.cast(F32, h, gate, r)),
               FWD_CAP)
    ck.done()


def gca_bwd_raw(dout, h, p, gate, dpooled, sdot, wk, L, dwk, dbk, ws):
    """osuf_gca_bwd_apply with the workspace chosen by the caller (None: the atomic path)."""
    M, C, ld = ops._rows(h)
    dh, dlogit = torch.empty_like(h), torch.empty(M, dtype=F32, device=DEV)
    ops.call("osuf_gca_bwd_apply", ops.dt_of(h), dout.data_ptr(), ops._rows(dout)[2], h.data_ptr(), ld, dh.data_ptr(), C, p.data_ptr(),
             gate.data_ptr(), dpooled.data_ptr(), sdot.data_ptr(), wk.data_ptr(), dlogit.data_ptr(), M, C, L, ops._p(dwk), ops._p(dbk),
             ops._p(ws), 0 if ws is None else ws.numel() * 4, ops._stream())
    return dh, dlogit


def gca_bwd_case(B, L, C, dtype, modes):
    """dh, dlogit, dwk, dbk against autograd of the fp64 chain dout . (h * gate) + dpooled . pooled(h, wk, bk) (norm_reference.gca_grads:
    what GCAPoolFn._backward feeds the kernel).  dbk is a sum that cancels to zero, so it is measured against sum |dlogit|."""
    h, wk, bk = gca_inputs(B, L, C, dtype)
    dout = dev(rnd("dout", (B, L, C)) + 0.2, dtype)
    gate, dpooled = dev(torch.sigmoid(rnd("gate", (B, C)))), dev(rnd("dpooled", (B, C)))
    g64 = R.gca_grads(*R.cast(F64, dout, h, gate, dpooled, wk, bk))
    g32 = R.gca_grads(*R.cast(F32, dout, h, gate, dpooled, wk, bk))
    p, sdot = dev(g64["p"].reshape(-1)), dev(g64["sdot"])
    denom = g64["dlogit"].abs().sum().item()

    def cancel(a, b):
        return (a.double().cpu() - b.double()).abs().sum().item() / denom
    ck = Check("gca_bwd_apply", dtype, C=C, M=B * L)
    prev_w, prev_b = rnd("prev_w", (C,)), torch.tensor([0.25])

    def check_dh(key, dh, dlogit):
        ck.out(f"dh_{key}", dh, g64["dh"], g32["dh"], GRAD_CAP)
        ck.f32(f"dlogit_{key}", dlogit.view(B, L), g64["dlogit"], g32["dlogit"], relmax, GRAD_CAP)

    def check_dw(key, dwk, dbk, pw=0.0, pb=0.0):
        ck.f32(f"dwk_{key}", dwk, g64["dwk"] + pw, g32["dwk"] + pw, rell2, GRAD_CAP)
        if dbk is not None:
            ck.f32(f"dbk_{key}", dbk, g64["dbk"] + pb, g32["dbk"] + pb, cancel, GRAD_CAP)
    if "none" in modes:
        check_dh("none", *ops.gca_bwd_apply(dout, h, p, gate, dpooled, sdot, wk, L))
    if "ws" in modes:                                      # slab + reduce, through the wrapper
        dwk, dbk = torch.zeros(C, device=DEV), torch.zeros(1, device=DEV)
        check_dh("ws", *ops.gca_bwd_apply(dout, h, p, gate, dpooled, sdot, wk, L, dwk, dbk))
        check_dw("ws", dwk, dbk)
    if "acc" in modes:                                     # accumulation: previous + gradient
        dwk, dbk = dev(prev_w), dev(prev_b)
        ops.gca_bwd_apply(dout, h, p, gate, dpooled, sdot, wk, L, dwk, dbk)
        check_dw("acc", dwk, dbk, prev_w, prev_b)
    if "atomic" in modes:                                  # workspace = NULL on a zeroed dwk
        dwk, dbk = torch.zeros(C, device=DEV), torch.zeros(1, device=DEV)
        check_dh("atomic", *gca_bwd_raw(dout, h, p, gate, dpooled, sdot, wk, L, dwk, dbk, None))
        check_dw("atomic", dwk, dbk)
        dwk = dev(prev_w)                                  # dwk alone (no dbk), accumulating
        gca_bwd_raw(dout, h, p, gate, dpooled, sdot, wk, L, dwk, None, None)
        check_dw("atomic_acc", dwk, None, prev_w)
    ck.done()


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("C", ROW_C)
def test_gca_bwd_apply(C, dtype):
    gca_bwd_case(RB, RL, C, dtype, ("none", "ws", "acc", "atomic"))


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
def test_gca_bwd_apply_above_block_cap(dtype):
    """With dwk the grid is capped at 2048 blocks of 4 waves x 64 rows (C = 8): M = 2048 * 256 + 1 = 3 * 174763."""
    gca_bwd_case(3, 174763, 8, dtype, ("ws",))


@pytest.mark.parametrize("L", [1, 255, 257, 1000])
def test_softmax_rows(L):
    B = 3
    logit = rnd("logit", (B, L)) * 3
    logit[1] += 80                                         # exp(80 + x) overflows fp32 unless the row maximum is subtracted
    p = ops.softmax_rows_(dev(logit).clone(), B, L)
    ck = Check("softmax_rows", F32, L=L)
    ck.f32("p", p.view(B, L), torch.softmax(logit.double(), 1), torch.softmax(logit, 1), relmax, FWD_CAP, FAST)
    ck.done()


# ---------------------------------------------------------------------------------------------------------------------------------
# column geometry: GroupNorm(1, C) + FiLM + SiLU forward / backward, wcolsum
# ---------------------------------------------------------------------------------------------------------------------------------
def rp8(C):
    """rows of one workgroup of gn_stats / gn_apply_fwd / gn_bwd_apply (rp row lanes x 8 rows per thread), plus one."""
    return (256 // (C // 8)) * 8 + 1


def raw_sums(y):
    y64 = y.double().cpu()
    return torch.stack([y64.sum((1, 2)), (y64 * y64).sum((1, 2))], 1).to(DEV)


def gn_fwd_case(B, L, C, dtype, y, name="gn_fwd"):
    gamma, beta = affine(C)
    ss = dev(0.3 * rnd("ss", (B, 2 * C)))
    ck = Check(name, dtype, C=C, L=L)
    for sk, s in (("", None), ("_ss", ss)):
        h64, mr64 = R.gn_film_silu(*R.cast(F64, y, gamma, beta, s))
        h32, mr32 = R.gn_film_silu(*R.cast(F32, y, gamma, beta, s))
        mr_a = ops.gn_stats(y, L)
        runs = {"stats": (ops.gn_apply(y, mr_a, gamma, beta, s, L), mr_a),
                "sums": ops.gn_apply_from_stats(y, raw_sums(y), gamma, beta, s, L),
                "parts": ops.gn_apply_reproducible(y, gamma, beta, s, L)}
        for key, (h, mr) in runs.items():
            ck.out(f"h_{key}{sk}", h, h64, h32, FWD_CAP, FAST)
            ck.f32(f"mean_{key}{sk}", mr[:, 0], mr64[:, 0], mr32[:, 0], relmax, FWD_CAP)
            ck.f32(f"rstd_{key}{sk}", mr[:, 1], mr64[:, 1], mr32[:, 1], relmax, FWD_CAP)
    ck.done()


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("C,L", [(C, L) for C in COL_C for L in (1, rp8(C))])
def test_gn_fwd(C, L, dtype):
    gn_fwd_case(2, L, C, dtype, dev(rnd("y", (2, L, C)) * 1.5 + 0.5, dtype))


@pytest.mark.parametrize("C", [40, 1032])
def test_gn_fwd_large_mean(C):
    """y = 30 + randn: E[y^2] - mean^2 loses three digits, so statistics accumulated in single precision show here."""
    L = rp8(C)
    gn_fwd_case(2, L, C, F32, dev(30 + rnd("y", (2, L, C))), name="gn_fwd_large_mean")


# gn_bwd_reduce: 64-row blocks walked 4 * rp rows per trip (clamped loads, masked surplus); gn_bwd_apply: rp * 8-row blocks
GN_BWD_CL = [(8, 1), (8, 65), (8, rp8(8)), (40, 63), (40, 200), (40, rp8(40)), (264, 1), (264, 63), (264, 65), (264, rp8(264)), (264, 200),
             (1024, 65), (1024, rp8(1024)), (1032, 1), (1032, 63), (1032, 65), (1032, 200), (1032, rp8(1032)), (2048, 65), (2048, rp8(2048))]


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("C,L", GN_BWD_CL)
def test_gn_bwd(C, L, dtype):
    B = 2
    y = dev(rnd("y", (B, L, C)) * 1.5 + 0.5, dtype)
    dh = dev(rnd("dh", (B, L, C)) + 0.3, dtype)            # non-zero mean: dbias and dyy are sums of substance, not noise around zero
    gamma, beta = affine(C)
    ss = dev(0.3 * rnd("ss", (B, 2 * C)))
    prev = {k: rnd("prev_" + k, (C,)) for k in ("dgamma", "dbeta", "dbias", "dyy")}
    ck = Check("gn_bwd", dtype, C=C, L=L)
    for sk, s in (("", None), ("_ss", ss)):
        g64 = R.gn_grads(*R.cast(F64, y, gamma, beta, s, dh))
        g32 = R.gn_grads(*R.cast(F32, y, gamma, beta, s, dh))
        mr = dev(R.gn_stats(y.double().cpu()))
        for pk, pre in (("", False), ("_acc", True)):      # fresh (zeroed) side outputs, then accumulation into pre-filled ones
            side = {k: dev(v) if pre else torch.zeros(C, device=DEV) for k, v in prev.items()}
            dy, dg, db, dss = ops.gn_bwd(dh, y, mr, gamma, beta, s, L, side["dgamma"], side["dbeta"], side["dbias"], side["dyy"])
            assert dg is side["dgamma"] and db is side["dbeta"]
            if not pre:
                ck.out(f"dy{sk}", dy, g64["dy"], g32["dy"], GRAD_CAP, FAST)
                if s is not None:
                    ck.f32("dss", dss, g64["dss"], g32["dss"], rell2, GRAD_CAP, FAST)
                else:
                    assert dss is None
            for k in prev:
                add = prev[k] if pre else 0.0
                ck.f32(f"{k}{sk}{pk}", side[k], g64[k] + add, g32[k] + add, rell2, GRAD_CAP, FAST)
    ck.done()


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("C,L", [(40, 65), (1032, 65)])
def test_gn_bwd_identity_norm(C, L, dtype):
    """Block(norm=False): dgamma == NULL, mean 0, rstd 1, gamma 1, beta 0 -> dy = (1 + scale) * dh * silu'(u), no statistics terms."""
    B = 2
    y = dev(rnd("y", (B, L, C)) * 1.5 + 0.5, dtype)
    dh = dev(rnd("dh", (B, L, C)) + 0.3, dtype)
    gamma, beta = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    mr = torch.tensor([[0.0, 1.0]] * B, device=DEV)
    ss = dev(0.3 * rnd("ss", (B, 2 * C)))
    ck = Check("gn_bwd_identity", dtype, C=C, L=L)
    for sk, s in (("", None), ("_ss", ss)):
        g64 = R.gn_grads(*R.cast(F64, y, gamma, beta, s, dh), identity_norm=True)
        g32 = R.gn_grads(*R.cast(F32, y, gamma, beta, s, dh), identity_norm=True)
        dbias, dyy = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
        dy, dg, db, dss = ops.gn_bwd(dh, y, mr, gamma, beta, s, L, None, None, dbias, dyy, identity_norm=True)
        assert dg is None and db is None
        ck.out(f"dy{sk}", dy, g64["dy"], g32["dy"], GRAD_CAP, FAST)
        if s is not None:
            ck.f32("dss", dss, g64["dss"], g32["dss"], rell2, GRAD_CAP, FAST)
        ck.f32(f"dbias{sk}", dbias, g64["dbias"], g32["dbias"], rell2, GRAD_CAP, FAST)
        ck.f32(f"dyy{sk}", dyy, g64["dyy"], g32["dyy"], rell2, GRAD_CAP, FAST)
    ck.done()


WCOL_CL = [(8, 65), (40, 63), (40, 200), (264, 1), (264, 63), (264, 65), (264, 200), (1024, 65), (1032, 1), (1032, 63), (1032, 65),
           (1032, 200), (2048, 65)]


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("C,L", WCOL_CL)
def test_wcolsum(C, L, dtype):
    B = 2
    a, bm = dev(rnd("a", (B, L, C)) + 0.2, dtype), dev(rnd("bm", (B, L, C)) + 0.2, dtype)
    w = dev(rnd("w", (B * L,)) + 0.3)
    ck = Check("wcolsum", dtype, C=C, L=L)
    for bk, b_ in (("", None), ("_bmul", bm)):
        for wk_, w_ in (("", None), ("_w", w)):
            r64, r32 = (R.wcolsum(*R.cast(dt, a, b_, None if w_ is None else w_.view(B, L))) for dt in (F64, F32))
            ck.f32(f"atomic{bk}{wk_}", ops.wcolsum(a, b_, w_, B, L), r64, r32, rell2, FWD_CAP)
            with ops.reproducible_mode():
                ck.f32(f"repro{bk}{wk_}", ops.wcolsum(a, b_, w_, B, L), r64, r32, rell2, FWD_CAP)
    ck.done()


# ---------------------------------------------------------------------------------------------------------------------------------
# row strides: every operand a column block [8 : 8 + C] of a buffer C + 24 wide
# ---------------------------------------------------------------------------------------------------------------------------------
def wide(t):
    """t as a column slice of a wider, sentinel-filled buffer."""
    buf = torch.full((*t.shape[:-1], t.shape[-1] + 24), SENT, dtype=t.dtype, device=t.device)
    v = buf[..., 8:8 + t.shape[-1]]
    v.copy_(t)
    return v


def wide_out(shape, dtype):
    buf = torch.full((*shape[:-1], shape[-1] + 24), SENT, dtype=dtype, device=DEV)
    return buf, buf[..., 8:8 + shape[-1]]


def untouched(buf, C):
    return bool((buf[..., :8] == SENT).all() and (buf[..., 8 + C:] == SENT).all())


def near(a, b):
    """The strided run against the dense one where fp32 atomics meet (gn_bwd's per-sample sums, dgamma / dbeta): only the order of a few
    hundred additions differs -- 1e-6 of the largest value, plus one bf16 spacing for a bf16-stored result."""
    lim = (2.0 ** -7 if a.dtype == torch.bfloat16 else 0.0)
    a, b = a.double(), b.double()
    return bool(((a - b).abs() <= lim * b.abs() + 1e-6 * b.abs().max()).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("C", [96, 1032])
def test_row_kernels_strided(C, dtype):
    B, L = RB, RL
    M, ld, dt, st = B * L, C + 24, ops._DT[dtype], ops._stream()
    x, dy = dev(rnd("x", (B, L, C)) * 1.5 + 0.5, dtype), dev(rnd("dy", (B, L, C)) + 0.3, dtype)
    gamma, beta = affine(C)
    xw, dyw = wide(x), wide(dy)
    # LayerNorm
    out, mr = ops.ln_fwd(x, gamma, beta)
    out2, mr2 = ops.ln_fwd(xw, gamma, beta)
    assert torch.equal(out2, out) and torch.equal(mr2, mr)
    buf, v = wide_out((B, L, C), dtype)
    mr3 = torch.empty_like(mr)
    ops.call("osuf_ln_fwd", dt, xw.data_ptr(), ld, v.data_ptr(), ld, mr3.data_ptr(), gamma.data_ptr(), beta.data_ptr(), M, C, st)
    assert torch.equal(v, out) and torch.equal(mr3, mr) and untouched(buf, C)
    dx, dg, db = ops.ln_bwd(dy, x, mr, gamma)
    buf, v = wide_out((B, L, C), dtype)
    dgb = torch.zeros(2, C, device=DEV)
    ops.call("osuf_ln_bwd", dt, dyw.data_ptr(), ld, xw.data_ptr(), ld, v.data_ptr(), ld, mr.data_ptr(), gamma.data_ptr(), dgb[0].data_ptr(),
             dgb[1].data_ptr(), M, C, st)
    assert torch.equal(v, dx) and untouched(buf, C) and near(dgb[0], dg) and near(dgb[1], db)
    # rowdot, pooling (both without atomics)
    h, wk, bk = gca_inputs(B, L, C, dtype)
    hw = wide(h)
    assert torch.equal(ops.rowdot(hw, wk, bk, L), ops.rowdot(h, wk, bk, L))
    pooled, p = ops.gca_pool(h, wk, bk, L)
    pooled2, p2 = ops.gca_pool(hw, wk, bk, L)
    assert torch.equal(pooled2, pooled) and torch.equal(p2, p)
    # gate / residual
    gate = dev(torch.sigmoid(rnd("gate", (B, C))))
    res = dev(rnd("res", (B, L, C)), dtype)
    o = ops.gate_residual(h, gate, res, L)
    resw = wide(res)
    assert torch.equal(ops.gate_residual(hw, gate, resw, L), o)
    buf, v = wide_out((B, L, C), dtype)
    ops.call("osuf_gate_residual", dt, hw.data_ptr(), ld, gate.data_ptr(), resw.data_ptr(), ld, v.data_ptr(), ld, M, C, L, st)
    assert torch.equal(v, o) and untouched(buf, C)
    # GlobalContext backward (no dwk: dh and dlogit have a fixed order)
    dpooled = dev(rnd("dpooled", (B, C)))
    sdot = ops.rowdot(pooled, dpooled, None, 1, per_sample=True)
    dh, dlogit = ops.gca_bwd_apply(dy, h, p, gate, dpooled, sdot, wk, L)
    buf, v = wide_out((B, L, C), dtype)
    dl2 = torch.empty_like(dlogit)
    ops.call("osuf_gca_bwd_apply", dt, dyw.data_ptr(), ld, hw.data_ptr(), ld, v.data_ptr(), ld, p.data_ptr(), gate.data_ptr(),
             dpooled.data_ptr(), sdot.data_ptr(), wk.data_ptr(), dl2.data_ptr(), M, C, L, None, None, None, 0, st)
    assert torch.equal(v, dh) and torch.equal(dl2, dlogit) and untouched(buf, C)


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("C", [40, 1032])
def test_column_kernels_strided(C, dtype):
    B, L = 2, 65
    M, ld, dt, st = B * L, C + 24, ops._DT[dtype], ops._stream()
    y, dh = dev(rnd("y", (B, L, C)) * 1.5 + 0.5, dtype), dev(rnd("dh", (B, L, C)) + 0.3, dtype)
    gamma, beta = affine(C)
    ss = dev(0.3 * rnd("ss", (B, 2 * C)))
    yw, dhw = wide(y), wide(dh)
    mr = ops.gn_stats(y, L)
    assert torch.equal(ops.gn_stats(yw, L), mr)
    h = ops.gn_apply(y, mr, gamma, beta, ss, L)
    assert torch.equal(ops.gn_apply(yw, mr, gamma, beta, ss, L), h)
    h2, mr2 = ops.gn_apply_from_stats(y, raw_sums(y), gamma, beta, ss, L)
    h3, mr3 = ops.gn_apply_from_stats(yw, raw_sums(y), gamma, beta, ss, L)
    assert torch.equal(h3, h2) and torch.equal(mr3, mr2)
    h2, mr2 = ops.gn_apply_reproducible(y, gamma, beta, ss, L)
    h3, mr3 = ops.gn_apply_reproducible(yw, gamma, beta, ss, L)
    assert torch.equal(h3, h2) and torch.equal(mr3, mr2)
    buf, v = wide_out((B, L, C), dtype)
    ops.call("osuf_gn_apply_fwd", dt, yw.data_ptr(), ld, v.data_ptr(), ld, mr.data_ptr(), gamma.data_ptr(), beta.data_ptr(), ss.data_ptr(),
             M, C, L, st)
    assert torch.equal(v, h) and untouched(buf, C)
    # backward: dy depends on sums that meet by atomics
    side = [torch.zeros(C, device=DEV) for _ in range(4)]
    dy, dg, db, dss = ops.gn_bwd(dh, y, mr, gamma, beta, ss, L, *side)
    buf, v = wide_out((B, L, C), dtype)
    side2 = [torch.zeros(C, device=DEV) for _ in range(4)]
    T, S, dss2 = torch.zeros(B, 4, C, device=DEV), torch.empty(B, 2, device=DEV), torch.empty(B, 2 * C, device=DEV)
    ops.call("osuf_gn_bwd", dt, dhw.data_ptr(), ld, yw.data_ptr(), ld, v.data_ptr(), ld, mr.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
             ss.data_ptr(), T.data_ptr(), S.data_ptr(), dss2.data_ptr(), *[t.data_ptr() for t in side2], M, C, L, st)
    assert near(v, dy) and untouched(buf, C) and near(dss2, dss)
    for a, b in zip(side2, side):
        assert near(a, b)
    # wcolsum, fixed-order form
    with ops.reproducible_mode():
        assert torch.equal(ops.wcolsum(yw, dhw, None, B, L), ops.wcolsum(y, dh, None, B, L))
    assert near(ops.wcolsum(yw, dhw, None, B, L), ops.wcolsum(y, dh, None, B, L))


# ---------------------------------------------------------------------------------------------------------------------------------
# argument checks (host side: nothing is launched)
# ---------------------------------------------------------------------------------------------------------------------------------
def _launchers():
    """name -> f(dt, inp, out, M, C, ld, L, stream): every kernel reads `inp` and writes `out` only."""
    def P(t):
        return t.data_ptr()
    return {
        "osuf_gn_stats": (lambda dt, i, o, M, C, ld, L, st: ops.call("osuf_gn_stats", dt, P(i), ld, P(o), P(o), M, C, L, st)),
        "osuf_gn_apply_fwd": (lambda dt, i, o, M, C, ld, L, st: ops.call("osuf_gn_apply_fwd", dt, P(i), ld, P(o), ld, P(i), P(i), P(i), None, M, C, L, st)),
        "osuf_gn_bwd": (lambda dt, i, o, M, C, ld, L, st: ops.call("osuf_gn_bwd", dt, P(i), ld, P(i), ld, P(o), ld, P(i), P(i), P(i), None, P(o), P(o),
                                                                          None, P(o), P(o), P(o), P(o), M, C, L, st)),
        "osuf_ln_fwd": (lambda dt, i, o, M, C, ld, L, st: ops.call("osuf_ln_fwd", dt, P(i), ld, P(o), ld, P(o), P(i), P(i), M, C, st)),
        "osuf_ln_bwd": (lambda dt, i, o, M, C, ld, L, st: ops.call("osuf_ln_bwd", dt, P(i), ld, P(i), ld, P(o), ld, P(i), P(i), P(o), P(o), M, C, st)),
        "osuf_rowdot": (lambda dt, i, o, M, C, ld, L, st: ops.call("osuf_rowdot", dt, P(i), ld, P(i), 0, None, P(o), M, C, L, st)),
        "osuf_gca_pool": (lambda dt, i, o, M, C, ld, L, st: ops.call("osuf_gca_pool", dt, P(i), ld, P(i), None, P(o), P(o), P(o), M, C, L, st)),
        "osuf_wcolsum": (lambda dt, i, o, M, C, ld, L, st: ops.call("osuf_wcolsum", dt, P(i), ld, None, 0, None, P(o), M // L, C, L, None, st)),
        "osuf_gate_residual": (lambda dt, i, o, M, C, ld, L, st: ops.call("osuf_gate_residual", dt, P(i), ld, P(i), None, 0, P(o), ld, M, C, L, st)),
        "osuf_gca_bwd_apply": (lambda dt, i, o, M, C, ld, L, st: ops.call("osuf_gca_bwd_apply", dt, P(i), ld, P(i), ld, P(o), ld, P(i), P(i), P(i), P(i),
                                                                                 P(i), P(o), M, C, L, None, None, None, 0, st)),
    }


BAD = {"C12": (6, 12, 16, 3), "C2056": (6, 2056, 2056, 3), "ld_odd": (6, 16, 28, 3), "M_mod_L": (7, 16, 16, 3)}      # M, C, ld, L


TAKES_L = {"osuf_gn_stats": True, "osuf_gn_apply_fwd": True, "osuf_gn_bwd": True, "osuf_ln_fwd": False, "osuf_ln_bwd": False, "osuf_rowdot": False,
           "osuf_gca_pool": True, "osuf_wcolsum": False, "osuf_gate_residual": True, "osuf_gca_bwd_apply": True}


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("name,bad", [(n, b) for n, l in TAKES_L.items() for b in BAD if l or b != "M_mod_L"])     # M % L: where M and L are both given
def test_bad_arguments_refused(name, bad, dtype):
    fn = _launchers()[name]
    M, C, ld, L = BAD[bad]
    inp = torch.zeros(1 << 16, device=DEV)                 # large enough for every operand, should a launch slip through
    out = torch.full((1 << 16,), SENT, device=DEV)
    with pytest.raises(RuntimeError, match="invalid argument"):
        fn(ops._DT[dtype], inp, out, M, C, ld, L, ops._stream())
    torch.cuda.synchronize()
    assert bool((out == SENT).all())


def test_wrappers_raise_on_bad_shapes():
    g = torch.ones(2056, device=DEV)
    for C in (12, 2056):
        with pytest.raises(RuntimeError, match="invalid argument"):
            ops.ln_fwd(torch.zeros(6, C, device=DEV), g, g)
    with pytest.raises(RuntimeError, match="invalid argument"):
        ops.ln_fwd(torch.zeros(6, 28, device=DEV)[:, 4:20], g, g)                   # row stride 28
    with pytest.raises(RuntimeError, match="invalid argument"):
        ops.gn_apply(torch.zeros(7, 16, device=DEV), torch.zeros(2, 2, device=DEV), g, g, None, 3)      # M % L != 0
