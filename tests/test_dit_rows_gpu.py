"""The DiT row kernels (csrc/dit.hip: adaLN forward / backward, the joint QK RMS-norm forward / backward, pack / unpack,
rowpart_finish_kernel behind both backwards, stat_pool) against plain fp64 references, on every branch the kernels and their launchers
take.  Launches go through ops.call on the raw entry points, so that strides, offsets, NULLs and alignment are the test's to choose.  No
launch consumes another kernel's output: mean | rstd and the inverse norms of the backward cases are the fp64 reference's, rounded to
fp32; one chained forward-to-backward case per kernel pair shows the real hand-over.

References, input generators, case tables and caps: tests/dit_rows_reference.py (checked on the CPU by
tests/test_dit_rows_reference_cpu.py, which derives the branch each case reaches from the launcher arithmetic).  The branch goes to the
parity metrics file with the achieved figures (dit_rows::*); profiles/dit_sweep.md holds the worst of them.

Every output, the workspaces included, is a slice of a buffer filled with a NaN bit pattern: 8 cells before the first row, the columns
between the width and the row stride, a spare row after the last, and for the joint buffers the other stream's rows.  Every cell outside
the slice must still hold the pattern, and a cell inside that was not written shows as a NaN.  The padding columns of strided inputs
hold NaNs too.

Bounds (tests/bound_check.py): an fp32 output within 16 x e32 of the fp64 reference, floored at 1e-6 and capped as R.*_CAP state; a
bf16 output within one bf16 spacing of the reference plus that term; moves and casts exact; the reduction outputs of two launches
bit-equal.  adaLN rows with an offset (kinds c and d) add the term R.adaln_extra derives: the kernel forms the mean as sum * (1 / C),
which costs up to 2^-23 |offset| when C is no power of two, and the output carries that times rstd (1 + max|scale|) <= ~2000; the cap
moves by the same term, since 2e-6 is what the suite asks of rows whose rstd is of order one.
"""
import functools

import numpy as np
import pytest
import torch

from osufusion_amd import _lib, ops
from tests import bound_check
from tests import dit_rows_reference as R
from tests import elementwise_reference as E
from tests.test_poisoned_memory import relmax, rell2

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
DT = {"f32": F32, "bf16": BF16}
CODE = {"f32": ops.F32, "bf16": ops.BF16}
SENT = {F32: 0x7FC00123, BF16: 0x7FC1}                                                  # NaN bit patterns
INT = {F32: torch.int32, BF16: torch.int16}
UINT = {F32: np.uint32, BF16: np.uint16}
LEAD = 8
ID0 = lambda v: v[0] if isinstance(v, tuple) else None


class Check(bound_check.Check):
    prefix = "dit_rows"


def stream():
    return torch.cuda.current_stream().cuda_stream


def p(t, col=0):
    return None if t is None else t.data_ptr() + col * t.element_size()


def dev(t, dtype=F32, ld=None):
    """CPU values (M, W) -> a device tensor (M, ld) in `dtype` (the values are held exactly) whose padding columns are NaN."""
    if t is None:
        return None
    M, W = t.shape
    out = torch.full((M, W if ld is None else ld), float("nan"), dtype=dtype, device=DEV)
    out[:, :W] = t.to(DEV).to(dtype)
    assert out.data_ptr() % 16 == 0
    return out


class Frame:
    """M rows at row stride ld inside a sentinel-filled flat buffer: LEAD cells before, a spare row and LEAD cells after.  The kernel may
    write the column blocks [(col0, width), ...] of the rows `rows` (default: all M) and nothing else."""

    def __init__(self, M, ld, dtype, blocks, rows=None):
        self.M, self.ld, self.dtype, self.blocks = M, ld, dtype, blocks
        self.rows = np.arange(M) if rows is None else np.asarray(rows)
        self.buf = torch.empty(LEAD + (M + 1) * ld + LEAD, dtype=dtype, device=DEV)
        self.buf.view(INT[dtype]).fill_(SENT[dtype])
        self.base = self.buf[LEAD:]
        assert all(0 <= c and c + w <= ld for c, w in blocks) and self.rows.max() < M

    def ptr(self, col=0):
        return p(self.base, col)

    def bits(self):
        return self.buf.cpu().view(INT[self.dtype]).numpy().view(UINT[self.dtype])

    def grid(self, b):
        return b[LEAD:LEAD + self.M * self.ld].reshape(self.M, self.ld)

    def intact(self):
        b = self.bits()
        keep = np.ones(b.shape, dtype=bool)
        inside = np.zeros((self.M, self.ld), dtype=bool)
        for c, w in self.blocks:
            inside[self.rows[:, None], np.arange(c, c + w)[None, :]] = True
        self.grid(keep)[inside] = False
        bad = np.nonzero(keep & (b != SENT[self.dtype]))[0]
        assert len(bad) == 0, (len(bad), "cells outside the slice were written, first flat indices:", bad[:8].tolist())

    def untouched(self):
        return bool((self.bits() == SENT[self.dtype]).all())

    def got(self, i=0):
        """Block i's bits, (len(rows), width)."""
        c, w = self.blocks[i]
        return self.grid(self.bits())[self.rows][:, c:c + w]

    def values(self, i=0):
        c, w = self.blocks[i]
        return self.grid(self.buf.cpu())[torch.from_numpy(self.rows)][:, c:c + w].contiguous()


def flat(n, dtype=F32):
    return Frame(1, n, dtype, [(0, n)])


def mismatches(ck, key, got_bits, want32, dtype):
    """Exact: the count of cells whose bits differ from the expected ones goes to the metrics with bound 0."""
    want = E.expect_bits(want32, dtype)
    bad = np.argwhere(E.bits_differ(got_bits, want, dtype))
    if len(bad):
        print(key, len(bad), "first (row, col), got, want:", [(tuple(i), hex(got_bits[tuple(i)]), hex(want[tuple(i)])) for i in bad[:6]])
    ck.fixed(key + "_mismatches", len(bad), 0)


def dbl(t):
    return None if t is None else t.double()


# ---------------------------------------------------------------------------------------------------------------------------------
# adaLN
# ---------------------------------------------------------------------------------------------------------------------------------
def adaln_strides(C, strides):
    return strides or dict(ldx=C, ldo=C, lddy=C, ldr=C, lddx=C, ldm=C, ldd=2 * C, off2=C)


@functools.lru_cache(maxsize=None)
def adaln_refs(cid, B, L, C, dt, kind):
    """(inputs, fp64 forward, fp32 forward, mean | rstd as the backward receives them: the fp64 forward's, rounded to fp32)."""
    inp = R.adaln_inputs(cid, B, L, C, dt, kind)
    f64 = R.adaln_fwd(inp["x"].double(), inp["shift"].double(), inp["scale"].double(), L)
    f32 = R.adaln_fwd(inp["x"], inp["shift"], inp["scale"], L)
    return inp, f64, f32, (f64[1].to(F32), f64[2].to(F32))


def launch_adaln_fwd(inp, B, L, C, dt, st, with_mr=True):
    M = B * L
    out, mr = Frame(M, st["ldo"], DT[dt], [(0, C)]), Frame(M, 2, F32, [(0, 2)])
    x, sh, sc = dev(inp["x"], DT[dt], st["ldx"]), dev(inp["shift"], F32, st["ldm"]), dev(inp["scale"], F32, st["ldm"])
    ops.call("osuf_adaln_fwd", CODE[dt], p(x), st["ldx"], out.ptr(), st["ldo"], mr.ptr() if with_mr else None, p(sh), p(sc), st["ldm"],
             M, C, L, R.LN_EPS, stream())
    torch.cuda.synchronize()
    out.intact(), mr.intact()
    return out, mr


def launch_adaln_bwd(inp, mean_rstd, B, L, C, dt, st, with_dres):
    """-> (dx frame, dmod frame: block 0 dshift, block 1 dscale)."""
    M = B * L
    need = _lib.load().osuf_adaln_bwd_workspace_bytes(M, C, L)
    assert need == B * R.adaln_bwd_blocks(B, L) * 2 * C * 4
    dx, ws = Frame(M, st["lddx"], DT[dt], [(0, C)]), flat(need // 4)
    c_shift = max(0, -st["off2"])
    dmod = Frame(B, st["ldd"], F32, [(c_shift, C), (c_shift + st["off2"], C)])
    dy, x = dev(inp["dy"], DT[dt], st["lddy"]), dev(inp["x"], DT[dt], st["ldx"])
    dres = dev(inp["dres"], DT[dt], st["ldr"]) if with_dres else None
    mr = mean_rstd if isinstance(mean_rstd, torch.Tensor) else torch.stack(mean_rstd, 1).contiguous().to(DEV)
    sc = dev(inp["scale"], F32, st["ldm"])
    ops.call("osuf_adaln_bwd", CODE[dt], p(dy), st["lddy"], p(x), st["ldx"], p(dres), st["ldr"] if with_dres else 0, dx.ptr(), st["lddx"], p(mr), p(sc),
             st["ldm"], dmod.ptr(c_shift), st["ldd"], st["off2"], ws.ptr(), need, M, C, L, stream())
    torch.cuda.synchronize()
    dx.intact(), dmod.intact(), ws.intact()
    return dx, dmod


def adaln_kinds(dt, dirs):
    return [k for k in R.ADALN_KINDS if not (k == "c" and dt == "bf16")] if dirs != "bwd" else []


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("case", [c for c in R.ADALN if c[5] != "bwd"], ids=ID0)
def test_adaln_fwd(case, dt):
    """out, mean, rstd for every input kind: a (eps invisible), b (var = 2^-20 ~ eps: a dropped or wrong eps is 0.1 .. 0.46 away),
    c and d (rows with an offset; the derived term of the module docstring).  Kind a of the first case also runs with mr = NULL."""
    cid, B, L, C, strides, dirs, named = case
    st = adaln_strides(C, strides)
    for kind in adaln_kinds(dt, dirs):
        inp, f64, f32, _ = adaln_refs(cid, B, L, C, dt, kind)
        out, mr = launch_adaln_fwd(inp, B, L, C, dt, st)
        extra = R.adaln_extra(kind, inp["scale"], f64[0])
        ck = Check("adaln_fwd", dt, case=cid, kind=kind, branch=",".join(sorted(R.adaln_branches(B, L, C, strides, dirs))))
        ck.out("out", out.values(), f64[0], f32[0], R.OUT_CAP + extra, extra)
        ck.f32("mean", mr.values()[:, 0], f64[1], f32[1], relmax, R.OUT_CAP)
        ck.f32("rstd", mr.values()[:, 1], f64[2], f32[2], relmax, R.OUT_CAP)
        ck.done()


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_adaln_fwd_without_mr(dt):
    """mr == NULL: the same output bits, and nothing else is written."""
    cid, B, L, C = "C520_L5", 2, 5, 520
    inp = adaln_refs(cid, B, L, C, dt, "a")[0]
    st = adaln_strides(C, None)
    with_mr, _ = launch_adaln_fwd(inp, B, L, C, dt, st)
    without, mr = launch_adaln_fwd(inp, B, L, C, dt, st, with_mr=False)
    assert mr.untouched() and np.array_equal(with_mr.got(), without.got()) and not torch.isnan(without.values().float()).any()


@pytest.mark.parametrize("with_dres", [False, True], ids=["nores", "dres"])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("case", [c for c in R.ADALN if c[5] != "fwd"], ids=ID0)
def test_adaln_bwd(case, dt, with_dres):
    """dx, dshift, dscale from given mean | rstd; two launches store bit-equal dshift | dscale."""
    cid, B, L, C, strides, dirs, named = case
    st = adaln_strides(C, strides)
    inp, f64, _, mean_rstd = adaln_refs(cid, B, L, C, dt, "a")
    mean, rstd = mean_rstd
    dres = inp["dres"] if with_dres else None
    b64 = R.adaln_bwd(inp["dy"].double(), inp["x"].double(), mean.double(), rstd.double(), inp["scale"].double(), L, dbl(dres))
    b32 = R.adaln_bwd(inp["dy"], inp["x"], mean, rstd, inp["scale"], L, dres)
    dx, dmod = launch_adaln_bwd(inp, mean_rstd, B, L, C, dt, st, with_dres)
    dx2, dmod2 = launch_adaln_bwd(inp, mean_rstd, B, L, C, dt, st, with_dres)
    ck = Check("adaln_bwd", dt, case=cid, dres=int(with_dres), branch=",".join(sorted(R.adaln_branches(B, L, C, strides, dirs))))
    ck.out("dx", dx.values(), b64[0], b32[0], R.GRAD_CAP)
    ck.f32("dshift", dmod.values(0), b64[1], b32[1], rell2, R.GRAD_CAP)
    ck.f32("dscale", dmod.values(1), b64[2], b32[2], rell2, R.GRAD_CAP)
    ck.fixed("relaunch_mismatches", int((dmod.bits() != dmod2.bits()).sum() + (dx.bits() != dx2.bits()).sum()), 0)
    ck.done()


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_adaln_chained(dt):
    """The backward on the forward kernel's own mean | rstd, against the fp64 chain."""
    cid, B, L, C = "C520_L67", 2, 67, 520
    st = adaln_strides(C, None)
    inp, f64, f32, _ = adaln_refs(cid, B, L, C, dt, "a")
    _, mr = launch_adaln_fwd(inp, B, L, C, dt, st)
    dx, dmod = launch_adaln_bwd(inp, mr.values().contiguous().to(DEV), B, L, C, dt, st, True)
    b64 = R.adaln_bwd(inp["dy"].double(), inp["x"].double(), f64[1], f64[2], inp["scale"].double(), L, inp["dres"].double())
    b32 = R.adaln_bwd(inp["dy"], inp["x"], f32[1], f32[2], inp["scale"], L, inp["dres"])
    ck = Check("adaln_chain", dt, case=cid, branch="fwd->bwd")
    ck.out("dx", dx.values(), b64[0], b32[0], R.GRAD_CAP)
    ck.f32("dshift", dmod.values(0), b64[1], b32[1], rell2, R.GRAD_CAP)
    ck.f32("dscale", dmod.values(1), b64[2], b32[2], rell2, R.GRAD_CAP)
    ck.done()


# ---------------------------------------------------------------------------------------------------------------------------------
# joint QK-norm
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def joint_refs(cid, B, Ns, Nj, off, H, G, D, dt, sp, gamma):
    inp = R.joint_inputs(cid, B, Ns, Nj, H, G, D, dt, sp)
    gq, gk = (inp["gq"], inp["gk"]) if gamma else (None, None)
    y64, inv64 = R.qknorm_fwd(inp["x"].double(), dbl(gq), dbl(gk), H, G, D)
    y32, inv32 = R.qknorm_fwd(inp["x"], gq, gk, H, G, D)
    masks = R.special_mask(B, Ns, H, G, D, inp["specials"] if gamma else [])
    groups = {"regular": ~(masks["zero"] | masks["tiny"] | masks["near"]), "clamped": masks["zero"] | masks["tiny"], "near": masks["near"]}
    groups["regular"][:, (H + G) * D:] = False                                          # the v columns are checked bit for bit
    if not gamma:
        groups["regular"][:] = False
    return inp, (y64, inv64), (y32, inv32), {k: m for k, m in groups.items() if m.any()}


def joint_args(case):
    cid, B, Ns, Nj, off, H, G, D, strided, sp, dirs, named = case
    W = (H + 2 * G) * D
    return cid, B, Ns, Nj, off, H, G, D, sp, W, R.joint_strides(W, strided), ",".join(sorted(R.joint_branches(B, Ns, Nj, off, H, G, D, strided, dirs)))


def launch_qknorm_fwd(inp, B, Ns, Nj, off, H, G, D, dt, st, gamma):
    M, W = B * Ns, (H + 2 * G) * D
    y = Frame(B * Nj, st["ldy"], BF16, [(0, W)], R.joint_rows(B, Ns, Nj, off).numpy())
    inv = Frame(M, H + G, F32, [(0, H + G)])
    x = dev(inp["x"], DT[dt], st["ldx"])
    gq, gk = (dev(inp["gq"]), dev(inp["gk"])) if gamma else (None, None)
    ops.call("osuf_joint_qknorm_fwd", CODE[dt], p(x), st["ldx"], y.ptr(), st["ldy"], inv.ptr() if gamma else None, p(gq), p(gk), M, Ns, Nj, off, H, G, D,
             stream())
    torch.cuda.synchronize()
    y.intact(), inv.intact()
    assert gamma or inv.untouched()
    return y, inv


def launch_qknorm_bwd(inp, inv, B, Ns, Nj, off, H, G, D, dt, st, gamma):
    M, W, QK = B * Ns, (H + 2 * G) * D, (H + G) * D
    need = _lib.load().osuf_joint_qknorm_bwd_workspace_bytes(M, H, G, D)
    assert need == R.qknorm_bwd_blocks(M) * QK * 4
    dx, dgamma, ws = Frame(M, st["lddx"], DT[dt], [(0, W)]), flat(QK), flat(need // 4)
    g = dev(inp["g"], F32, st["ldg"])
    if gamma:
        x, gq, gk, iv = dev(inp["x"], DT[dt], st["ldx"]), dev(inp["gq"]), dev(inp["gk"]), inv.contiguous().to(DEV)
        ops.call("osuf_joint_qknorm_bwd", CODE[dt], p(g), st["ldg"], p(x), st["ldx"], p(iv), p(gq), p(gk), dx.ptr(), st["lddx"], dgamma.ptr(), ws.ptr(), need,
                 M, Ns, Nj, off, H, G, D, stream())
    else:
        ops.call("osuf_joint_qknorm_bwd", CODE[dt], p(g), st["ldg"], None, W, None, None, None, dx.ptr(), st["lddx"], None, None, 0,
                 M, Ns, Nj, off, H, G, D, stream())
    torch.cuda.synchronize()
    dx.intact(), dgamma.intact(), ws.intact()
    assert gamma or (dgamma.untouched() and ws.untouched())
    return dx, dgamma


@pytest.mark.parametrize("gamma", [True, False], ids=["gamma", "cast"])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("case", [c for c in R.JOINT if c[10] != "bwd"], ids=ID0)
def test_joint_qknorm_fwd(case, dt, gamma):
    """The stream's joint rows: the normed heads bounded (regular heads, the clamped ones and the ones just above the clamp each on their
    own), the v columns -- and in cast mode every column -- bit for bit; the other stream's rows keep the pattern (Frame.intact)."""
    cid, B, Ns, Nj, off, H, G, D, sp, W, st, branch = joint_args(case)
    inp, r64, r32, groups = joint_refs(cid, B, Ns, Nj, off, H, G, D, dt, sp, gamma)
    y, inv = launch_qknorm_fwd(inp, B, Ns, Nj, off, H, G, D, dt, st, gamma)
    ck = Check("joint_qknorm_fwd", dt, case=cid, gamma=int(gamma), branch=branch)
    cols = R.joint_cols(H, G, D, H + 2 * G)
    got = y.values()[:, cols]                                                           # natural order
    exact = torch.ones(B * Ns, W, dtype=torch.bool)
    for name, m in groups.items():
        exact &= ~m
        ck.out("y_" + name, got[m], r64[0][:, cols][m], r32[0][:, cols][m], R.Y_CAP)
    ej = torch.empty_like(exact)
    ej[:, cols] = exact                                                                 # the same cells in joint order
    ej = ej.numpy()
    bad = np.argwhere(E.bits_differ(np.where(ej, y.got(), 0), np.where(ej, E.expect_bits(r32[0], BF16), 0), BF16))   # moves and casts of the input values
    ck.fixed("moved_mismatches", len(bad), 0)
    if gamma:
        special = torch.zeros(B * Ns, H + G, dtype=torch.bool)
        for b, n, head, kind in inp["specials"]:
            special[b * Ns + n, head] = True
        iv = inv.values()
        ck.f32("inv", iv[~special], r64[1][~special], r32[1][~special], relmax, R.INV_CAP)
        if special.any():
            ck.f32("inv_special", iv[special], r64[1][special], r32[1][special], relmax, R.INV_CAP)
    ck.done()


@pytest.mark.parametrize("gamma", [True, False], ids=["gamma", "cast"])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("case", [c for c in R.JOINT if c[10] != "fwd"], ids=ID0)
def test_joint_qknorm_bwd(case, dt, gamma):
    """dx per group of heads, the v columns (cast mode: every column) bit for bit, dgamma against the fp64 sum; two launches store
    bit-equal dgamma."""
    cid, B, Ns, Nj, off, H, G, D, sp, W, st, branch = joint_args(case)
    inp, r64, r32, groups = joint_refs(cid, B, Ns, Nj, off, H, G, D, dt, sp, gamma)
    gq, gk = (inp["gq"], inp["gk"]) if gamma else (None, None)
    g = inp["g"][R.joint_rows(B, Ns, Nj, off)]
    inv = r64[1].to(F32) if gamma else None
    b64 = R.qknorm_bwd(g.double(), inp["x"].double(), dbl(inv), dbl(gq), dbl(gk), H, G, D)
    b32 = R.qknorm_bwd(g, inp["x"], inv, gq, gk, H, G, D)
    dx, dgamma = launch_qknorm_bwd(inp, inv, B, Ns, Nj, off, H, G, D, dt, st, gamma)
    dx2, dgamma2 = launch_qknorm_bwd(inp, inv, B, Ns, Nj, off, H, G, D, dt, st, gamma)
    ck = Check("joint_qknorm_bwd", dt, case=cid, gamma=int(gamma), branch=branch)
    got = dx.values()
    exact = torch.ones(B * Ns, W, dtype=torch.bool)
    for name, m in groups.items():
        exact &= ~m
        ck.out("dx_" + name, got[m], b64[0][m], b32[0][m], R.GRAD_CAP)
    e = exact.numpy()
    bad = np.argwhere(E.bits_differ(np.where(e, dx.got(), 0), np.where(e, E.expect_bits(b32[0], DT[dt]), 0), DT[dt]))
    ck.fixed("moved_mismatches", len(bad), 0)
    if gamma:
        ck.f32("dgamma", dgamma.values().view(H + G, D), b64[1], b32[1], rell2, R.GRAD_CAP)
    ck.fixed("relaunch_mismatches", int((dgamma.bits() != dgamma2.bits()).sum() + (dx.bits() != dx2.bits()).sum()), 0)
    ck.done()


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_joint_qknorm_chained(dt):
    """The backward on the forward kernel's own inverse norms, against the fp64 chain."""
    case = next(c for c in R.JOINT if c[0] == "j2c_x")
    cid, B, Ns, Nj, off, H, G, D, sp, W, st, branch = joint_args(case)
    inp, r64, r32, groups = joint_refs(cid, B, Ns, Nj, off, H, G, D, dt, sp, True)
    _, inv = launch_qknorm_fwd(inp, B, Ns, Nj, off, H, G, D, dt, st, True)
    dx, dgamma = launch_qknorm_bwd(inp, inv.values(), B, Ns, Nj, off, H, G, D, dt, st, True)
    g = inp["g"][R.joint_rows(B, Ns, Nj, off)]
    b64 = R.qknorm_bwd(g.double(), inp["x"].double(), r64[1], inp["gq"].double(), inp["gk"].double(), H, G, D)
    b32 = R.qknorm_bwd(g, inp["x"], r32[1], inp["gq"], inp["gk"], H, G, D)
    ck = Check("joint_qknorm_chain", dt, case=cid, branch="fwd->bwd")
    for name, m in groups.items():
        ck.out("dx_" + name, dx.values()[m], b64[0][m], b32[0][m], R.GRAD_CAP)
    ck.f32("dgamma", dgamma.values().view(H + G, D), b64[1], b32[1], rell2, R.GRAD_CAP)
    ck.done()


# ---------------------------------------------------------------------------------------------------------------------------------
# pack / unpack: the permuted layout itself
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("case", R.PERM, ids=ID0)
def test_joint_pack_and_unpack(case, dt):
    cid, B, Ns, Nj, off, H, G, D, lds, ldj, branch = case
    M, HD = B * Ns, H * D
    jr = R.joint_rows(B, Ns, Nj, off)
    rows = R.stored(R.rnd(f"pk.{cid}", (M, HD)), BF16)                                  # bf16 values: the joint buffer holds them exactly
    joint = Frame(B * Nj, ldj, BF16, [(0, HD)], jr.numpy())
    d_rows = dev(rows, DT[dt], lds)
    ops.call("osuf_joint_pack", CODE[dt], p(d_rows), lds, joint.ptr(), ldj, M, Ns, Nj, off, H, G, D, stream())
    torch.cuda.synchronize()
    joint.intact()
    ck = Check("joint_pack", dt, case=cid, branch=branch)
    mismatches(ck, "joint", joint.got(), R.pack(rows, H, G, D), BF16)
    src = R.stored(R.rnd(f"upk.{cid}", (B * Nj, HD)), BF16)
    out = Frame(M, lds, DT[dt], [(0, HD)])
    d_src = dev(src, BF16, ldj)
    ops.call("osuf_joint_unpack", CODE[dt], p(d_src), ldj, out.ptr(), lds, M, Ns, Nj, off, H, G, D, stream())
    torch.cuda.synchronize()
    out.intact()
    mismatches(ck, "rows", out.got(), R.unpack(src[jr], H, G, D), DT[dt])
    ck.done()


# ---------------------------------------------------------------------------------------------------------------------------------
# stat_pool
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.STAT_KINDS)
@pytest.mark.parametrize("C", R.STAT_C)
@pytest.mark.parametrize("L", R.STAT_L)
def test_stat_pool(L, C, kind):
    """[mean | std] at relmax as tests/test_dit_gpu.py measures it; for the plain input the two halves also on their own."""
    B = R.STAT_B
    a = R.stat_input(kind, B, C, L)
    out = Frame(B, 2 * C, F32, [(0, 2 * C)])
    d_a = a.to(DEV)
    ops.call("osuf_stat_pool", p(d_a), out.ptr(), B, C, L, stream())
    torch.cuda.synchronize()
    out.intact()
    r64, r32, got = R.stat_pool(a.double()), R.stat_pool(a), out.values()
    ck = Check("stat_pool", "f32", kind=kind, C=C, L=L, branch=f"trips={(L + 255) // 256},tail={L % 256}")
    ck.f32("out", got, r64, r32, relmax, R.STAT_CAP)
    if kind == "plain":
        ck.f32("mean", got[:, :C], r64[:, :C], r32[:, :C], relmax, R.STAT_CAP)
        ck.f32("std", got[:, C:], r64[:, C:], r32[:, C:], relmax, R.STAT_CAP)
    ck.done()


# ---------------------------------------------------------------------------------------------------------------------------------
# contract
# ---------------------------------------------------------------------------------------------------------------------------------
def good_calls():
    """entry point -> (ordered {argument: value} of a call that would succeed, the frames it would write).  Pointer arguments hold a device
    tensor or a frame."""
    z = lambda *shape, dtype=F32: torch.zeros(*shape, dtype=dtype, device=DEV)
    a, j = R.GOOD_ADALN, R.GOOD_JOINT
    B, L, C, ld, ldm = a["B"], a["L"], a["C"], a["ld"], a["ldm"]
    M = B * L
    good = {}
    out, mr = Frame(M, ld, F32, [(0, C)]), Frame(M, 2, F32, [(0, 2)])
    good["osuf_adaln_fwd"] = (dict(dtype=ops.F32, x=z(M, ld), ldx=ld, out=out, ldo=ld, mr=mr, shift=z(B, ldm), scale=z(B, ldm), ldm=ldm, M=M, C=C, L=L,
                                   eps=R.LN_EPS), [out, mr])
    good["osuf_adaln_bwd_workspace_bytes"] = (dict(M=M, C=C, L=L), [])
    dx, dmod, ws = Frame(M, ld, F32, [(0, C)]), Frame(B, ldm, F32, [(0, C), (C, C)]), flat(B * 2 * C)
    good["osuf_adaln_bwd"] = (dict(dtype=ops.F32, dy=z(M, ld), lddy=ld, x=z(M, ld), ldx=ld, dres=z(M, ld), ldr=ld, dx=dx, lddx=ld, mr=z(M, 2), scale=z(B, ldm),
                                   ldm=ldm, dmod=dmod, ldd=ldm, off2=C, workspace=ws, workspace_bytes=B * 2 * C * 4, M=M, C=C, L=L), [dx, dmod, ws])
    o = flat(3 * 12)
    good["osuf_stat_pool"] = (dict(a=z(3, 6, 40), out=o, B=3, C=6, L=40), [o])
    B, Ns, Nj, off, H, G, D, ld, ldp = (j[k] for k in ("B", "Ns", "Nj", "off", "H", "G", "D", "ld", "ldp"))
    M, W, QK, HD = B * Ns, (H + 2 * G) * D, (H + G) * D, H * D
    shape = dict(M=M, Ns=Ns, Nj=Nj, off=off, H=H, G=G, D=D)
    y, inv = Frame(B * Nj, ld, BF16, [(0, W)]), Frame(M, H + G, F32, [(0, H + G)])
    good["osuf_joint_qknorm_fwd"] = (dict(dtype=ops.F32, x=torch.ones(M, ld, device=DEV), ldx=ld, y=y, ldy=ld, inv=inv, gamma_q=z(H, D), gamma_k=z(G, D), **shape),
                                     [y, inv])
    jt = Frame(B * Nj, ldp, BF16, [(0, HD)])
    good["osuf_joint_pack"] = (dict(dtype=ops.F32, s=z(M, ldp), lds=ldp, joint=jt, ldj=ldp, **shape), [jt])
    s = Frame(M, ldp, F32, [(0, HD)])
    good["osuf_joint_unpack"] = (dict(dtype=ops.F32, joint=z(B * Nj, ldp, dtype=BF16), ldj=ldp, s=s, lds=ldp, **shape), [s])
    good["osuf_joint_qknorm_bwd_workspace_bytes"] = (dict(M=M, H=H, G=G, D=D), [])
    dx, dg, ws = Frame(M, ld, F32, [(0, W)]), flat(QK), flat(QK)
    good["osuf_joint_qknorm_bwd"] = (dict(dtype=ops.F32, g=z(B * Nj, ld), ldg=ld, x=torch.ones(M, ld, device=DEV), ldx=ld, inv=torch.ones(M, H + G, device=DEV),
                                          gamma_q=z(H, D), gamma_k=z(G, D), dx=dx, lddx=ld, dgamma=dg, workspace=ws, workspace_bytes=QK * 4, **shape),
                                     [dx, dg, ws])
    return good


def pointer(v, how=None):
    if how == "null":
        return None
    ptr = v.ptr() if isinstance(v, Frame) else v.data_ptr()
    return ptr + (4 if how == "off4" else 0)


def marshal(args, over, with_stream):
    call = []
    for name, v in args.items():
        o = over.get(name)
        if isinstance(v, (Frame, torch.Tensor)):
            assert o in (None, "null", "off4"), (name, o)
            call.append(pointer(v, o))
        else:
            call.append(v if o is None else o)
    return call + ([stream()] if with_stream else [])


def test_good_calls_succeed():
    """The calls the contract table alters one argument of are themselves accepted (status 0, the workspace sizes as restated)."""
    lib = _lib.load()
    for entry, (args, outs) in good_calls().items():
        ws = entry.endswith("_workspace_bytes")
        status = getattr(lib, entry)(*marshal(args, {}, not ws))
        assert (status > 0) if ws else (status == 0), (entry, status)
    torch.cuda.synchronize()
    assert lib.osuf_adaln_bwd_workspace_bytes(10, 64, 5) == 2 * 2 * 64 * 4 and lib.osuf_joint_qknorm_bwd_workspace_bytes(10, 6, 2, 16) == 128 * 4
    assert lib.osuf_adaln_bwd_workspace_bytes(65535, 8, 1) == 65535 * 2 * 8 * 4


def test_bad_arguments_are_refused():
    """Every line of R.DIT_BAD: the status it names (a workspace size of 0), before any launch -- every output and workspace frame still
    holds its sentinel in every cell."""
    lib = _lib.load()
    good = good_calls()
    assert set(good) == set(R.DIT_ENTRIES) == {e for e, _, _ in R.DIT_BAD}
    for entry, kind, over in R.DIT_BAD:
        args, _ = good[entry]
        assert set(over) <= set(args), (entry, over)
        got = getattr(lib, entry)(*marshal(args, over, not entry.endswith("_workspace_bytes")))
        assert got == R.bad_status(entry, kind), (entry, kind, over, got)
    torch.cuda.synchronize()
    for entry, (_, outs) in good.items():
        for o in outs:
            assert o.untouched(), (entry, "an output was written by a refused call")
