"""The layout, loss, optimizer and DDPM / DDIM kernels (the head of csrc/elementwise.hip: ncl_to_rows, rows_to_ncl, copy2d, add2d, mse,
sqnorm, adamw, clip_coef, cast_flat; the top of csrc/sampling.hip: axpby_rows, ddim_step) against plain references, on every branch the
kernels and ew_grid take.  Launches go through ops.call on the raw entry points, so that strides, offsets and alignment are the test's to
choose; no launch consumes another kernel's output.

References, input generators, case tables and caps: tests/elementwise_reference.py (checked on the CPU by
tests/test_elementwise_reference_cpu.py, which also shows that the fp32 evaluation keeps every cap used here).  The branch each case
reaches is named in its table entry and goes to the parity metrics file with the achieved figures (elementwise_rows::*).

Every output is a slice of a buffer filled with a NaN bit pattern: 8 cells before the first row, the columns between the width and the
row stride, a spare row after the last.  Every cell outside the slice must still hold the pattern, and a cell inside that was not
written shows as a NaN.

A. Moves, exact: the stored bits equal the reference's (for bf16, the fp32 value rounded once by rne_bf16).
B. Rounding, exact: the packed conversion (store8: the body of cast_flat, copy2d, ncl_to_rows) and the scalar one (the tail of cast_flat)
   on 393 216 fp32 patterns / about 200 boundary patterns against rne_bf16; bits where a number is expected, NaN-ness where a NaN is.
C. Arithmetic, bounded (tests/bound_check.py): within 16 x e32 of the fp64 reference, floored at 1e-6 and capped as E.*_CAP state; mse's
   grad, the integer sums and clip_coef's pass-through values are exact.
D. Contract: every line of E.EW_BAD is refused with its status before any launch, and nothing is written.
"""
import functools

import numpy as np
import pytest
import torch

from osufusion_amd import _lib, ops
from tests import bound_check
from tests import elementwise_reference as E
from tests.test_poisoned_memory import relmax

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
DT = {"f32": F32, "bf16": BF16}
CODE = {"f32": ops.F32, "bf16": ops.BF16}
SENT = {F32: 0x7FC00123, BF16: 0x7FC1, F64: 0x7FF8000000000123}                          # NaN bit patterns
INT = {F32: torch.int32, BF16: torch.int16, F64: torch.int64}
LEAD = 8
ID0 = lambda v: v[0] if isinstance(v, tuple) else None


class Check(bound_check.Check):
    prefix = "elementwise_rows"


def stream():
    return torch.cuda.current_stream().cuda_stream


def p(t):
    return None if t is None else t.data_ptr()


_ALIVE = []


@pytest.fixture(autouse=True)
def _inputs_outlive_the_launch():
    """dev() is called inside argument lists: its tensors are kept until the test ends, so that no two of them share an address."""
    yield
    _ALIVE.clear()


def dev(t, dtype=None):
    """A CPU tensor of values -> a device tensor of its own (16-byte aligned), in `dtype` (bf16: the values are held exactly)."""
    if t is None:
        return None
    t = t.to(DEV)
    t = t if dtype is None or t.dtype == dtype else t.to(dtype)
    _ALIVE.append(t)
    return t


class Frame:
    """M rows of `width` cells at row stride ld inside a sentinel-filled flat buffer: LEAD cells before, a spare row and LEAD cells after.
    .view is what the kernel is given (16-byte aligned when ld % 8 == 0)."""

    def __init__(self, M, width, ld=None, dtype=F32):
        ld = width if ld is None else ld
        self.M, self.width, self.ld, self.dtype = M, width, ld, dtype
        self.buf = torch.empty(LEAD + (M + 1) * ld + LEAD, dtype=dtype, device=DEV)
        self.buf.view(INT[dtype]).fill_(SENT[dtype])
        self.view = self.buf[LEAD:LEAD + M * ld].view(M, ld)[:, :width]
        assert self.view.data_ptr() % 16 == 0 or ld % 8

    def bits(self):
        b = self.buf.cpu().view(INT[self.dtype]).numpy()
        return b.view({F32: np.uint32, BF16: np.uint16, F64: np.uint64}[self.dtype])

    def intact(self):
        b = self.bits()
        keep = np.ones(b.shape, dtype=bool)
        keep[LEAD:LEAD + self.M * self.ld].reshape(self.M, self.ld)[:, :self.width] = False
        bad = np.nonzero(keep & (b != SENT[self.dtype]))[0]
        assert len(bad) == 0, (len(bad), "cells outside the slice were written, first flat indices:", bad[:8].tolist())

    def got(self):
        """The slice's bits, (M, width)."""
        return self.bits()[LEAD:LEAD + self.M * self.ld].reshape(self.M, self.ld)[:, :self.width]

    def values(self):
        return self.view.cpu()


def same_bits(ck, key, frame, want32):
    """Exact: the count of differing cells goes to the metrics (bound 0); the assertion names the first of them.  want32: the fp32 values
    the reference gives, (M, width); the frame's dtype says how they are stored."""
    frame.intact()
    got, want = frame.got(), E.expect_bits(want32.reshape(frame.M, frame.width), frame.dtype)
    bad = np.argwhere(E.bits_differ(got, want, frame.dtype))
    ck.fixed(key + "_mismatches", len(bad), 0)
    if len(bad):
        print(key, len(bad), "first (row, col), got, want:", [(tuple(i), hex(got[tuple(i)]), hex(want[tuple(i)])) for i in bad[:6]])
    ck.done()


# ---------------------------------------------------------------------------------------------------------------------------------
# A. moves, exact
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("case", E.NCL, ids=ID0)
def test_ncl_to_rows(case, dt):
    cid, B, C, L, KT, width, ld, branch = case
    x = E.ncl_input(f"ncl.{cid}", B, C, L)
    out = Frame(B * L, width, ld, DT[dt])
    ops.call("osuf_ncl_to_rows", CODE[dt], p(dev(x)), p(out.view), ld, width, B, C, L, KT, stream())
    same_bits(Check("ncl_to_rows", dt, case=cid, branch=branch), "rows", out, E.ncl_to_rows(x, C, L, KT, width))


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("case", E.R2N, ids=ID0)
def test_rows_to_ncl(case, dt):
    cid, B, C, L, ld, branch = case
    rows = E.rows_input(f"r2n.{cid}", B * L, ld, DT[dt])
    out = Frame(1, B * C * L)
    ops.call("osuf_rows_to_ncl", CODE[dt], p(dev(rows, DT[dt])), ld, p(out.view), B, C, L, stream())
    same_bits(Check("rows_to_ncl", dt, case=cid, branch=branch), "ncl", out, E.rows_to_ncl(rows, B, C, L))


@pytest.mark.parametrize("sdt,ddt", E.DT_PAIRS)
@pytest.mark.parametrize("case", E.COPY, ids=ID0)
def test_copy2d(case, sdt, ddt):
    cid, M, cols, lds, ldd, branch = case
    src = E.rows_input(f"cp.{cid}", M, lds, DT[sdt])
    out = Frame(M, cols, ldd, DT[ddt])
    ops.call("osuf_copy2d", CODE[sdt], p(dev(src, DT[sdt])), lds, CODE[ddt], p(out.view), ldd, M, cols, stream())
    same_bits(Check("copy2d", f"{sdt}->{ddt}", case=cid, branch=branch), "dst", out, E.copy2d(src, cols))


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("case", E.ADD, ids=ID0)
def test_add2d(case, dt):
    """f32: the bits of the torch fp32 add; bf16: rne_bf16(float(a) + float(b))."""
    cid, M, cols, lda, ldb, ldd, branch = case
    a, b = E.rows_input(f"add.a.{cid}", M, lda, DT[dt]), E.rows_input(f"add.b.{cid}", M, ldb, DT[dt])
    out = Frame(M, cols, ldd, DT[dt])
    ops.call("osuf_add2d", CODE[dt], p(dev(a, DT[dt])), lda, p(dev(b, DT[dt])), ldb, p(out.view), ldd, M, cols, stream())
    want = E.add2d(a, b, cols)
    assert want.dtype == F32 and torch.equal(want, a[:, :cols] + b[:, :cols])
    same_bits(Check("add2d", dt, case=cid, branch=branch), "dst", out, want)


# ---------------------------------------------------------------------------------------------------------------------------------
# B. rounding, exact
# ---------------------------------------------------------------------------------------------------------------------------------
def cast_flat(bits):
    """osuf_cast_f32_bf16 over the given fp32 patterns -> (frame, expected bf16 bits)."""
    n = len(bits)
    out = Frame(1, n, None, BF16)
    src = E.f32_from_bits(bits).to(DEV)
    assert np.array_equal(E.f32_bits(src), bits)                                         # the patterns reach the device as they are
    ops.call("osuf_cast_f32_bf16", p(src), p(out.view), n, stream())
    return out, E.rne_bf16(bits)[None, :]


def rounding_mismatches(out, want):
    out.intact()
    got = out.got()
    bad = np.argwhere(E.bits_differ(got, want, BF16))
    return bad, [(tuple(i), hex(got[tuple(i)]), hex(want[tuple(i)])) for i in bad[:6]]


def test_cast_vector_body_on_the_pattern_table():
    bits = E.pattern_table()
    out, want = cast_flat(bits)
    bad, first = rounding_mismatches(out, want)
    ck = Check("cast_f32_bf16", "bf16", case="table", branch="body")
    ck.fixed("mismatches", len(bad), 0)
    ck.done()
    assert len(bad) == 0, (len(bad), "first (0, index), got, want:", first, "source patterns:", [hex(bits[i[1]]) for i in bad[:6]])


@pytest.mark.parametrize("n", range(1, 16))
def test_cast_tails_of_every_length(n):
    """n < 8: the tail alone; n = 8: the body alone; otherwise one vector and n - 8 scalar conversions."""
    bits = np.roll(E.special_patterns(), -7 * n)[:n]
    out, want = cast_flat(bits)
    bad, first = rounding_mismatches(out, want)
    ck = Check("cast_f32_bf16", "bf16", case=f"n{n}", branch=f"body={n // 8},tail={n % 8}")
    ck.fixed("mismatches", len(bad), 0)
    ck.done()
    assert len(bad) == 0, (first, [hex(bits[i[1]]) for i in bad[:6]])


def test_cast_scalar_tail_on_the_special_patterns():
    """n = 7 over consecutive sevens of the special patterns: every one goes through the scalar conversion."""
    s = E.special_patterns()
    s = np.concatenate([s, s[:(-len(s)) % 7]])
    total, firsts = 0, []
    for i in range(0, len(s), 7):
        out, want = cast_flat(s[i:i + 7])
        bad, first = rounding_mismatches(out, want)
        total += len(bad)
        firsts += [(hex(s[i + j[1]]), g, w) for j, (_, g, w) in zip(bad, first)]
    ck = Check("cast_f32_bf16", "bf16", case="specials", branch="tail")
    ck.fixed("mismatches", total, 0)
    ck.done()
    assert total == 0, (total, "(source, got, want):", firsts[:8])


def test_copy2d_and_ncl_to_rows_round_the_pattern_table():
    """The packed conversion behind the other two kernels that store bf16 from fp32: the table as (8192, 48) rows / as (1, 48, 8192)."""
    bits = E.pattern_table()
    M, cols = 8192, 48
    assert M * cols == len(bits)
    src = E.f32_from_bits(bits).view(M, cols)
    want = E.rne_bf16(bits).reshape(M, cols)
    out = Frame(M, cols, cols + 8, BF16)
    ops.call("osuf_copy2d", ops.F32, p(dev(src)), cols, ops.BF16, p(out.view), cols + 8, M, cols, stream())
    bad_c, first_c = rounding_mismatches(out, want)
    x = src.t().contiguous().view(1, cols, M)                                            # x[0][ci][n] = src[n][ci]
    out2 = Frame(M, cols, cols, BF16)
    ops.call("osuf_ncl_to_rows", ops.BF16, p(dev(x)), p(out2.view), cols, cols, 1, cols, M, 1, stream())
    bad_n, first_n = rounding_mismatches(out2, want)
    ck = Check("store8_rounding", "bf16", case="table", branch="copy2d,ncl_to_rows")
    ck.fixed("copy2d_mismatches", len(bad_c), 0)
    ck.fixed("ncl_to_rows_mismatches", len(bad_n), 0)
    ck.done()
    assert len(bad_c) == 0 and len(bad_n) == 0, (first_c, first_n)


# ---------------------------------------------------------------------------------------------------------------------------------
# C. arithmetic, bounded
# ---------------------------------------------------------------------------------------------------------------------------------
PRELOAD = 3.25                                             # loss_sum / out before the launch: the kernels add, they do not store


@pytest.mark.parametrize("has_len,has_wt,has_grad", E.MSE_OPTS)
@pytest.mark.parametrize("case", E.MSE, ids=ID0)
def test_mse(case, has_len, has_wt, has_grad):
    cid, B, Dch, L, branch = case
    inp = E.mse_inputs(cid, B, Dch, L, has_len, has_wt)
    grad = Frame(1, B * Dch * L) if has_grad else None
    acc = torch.full((1,), PRELOAD, dtype=F64, device=DEV)
    args = (p(dev(inp["pred"])), p(dev(inp["target"])), p(dev(inp["orig_len"])))
    tail = (p(grad.view) if has_grad else None, p(acc), B, Dch, L, stream())
    if has_wt:
        ops.call("osuf_mse_w", *args, p(dev(inp["wt"])), *tail)
    else:
        ops.call("osuf_mse", *args, *tail)
    s64, _ = E.mse(inp["pred"].double(), inp["target"].double(), inp["orig_len"], inp["wt"])
    s32, g32 = E.mse(inp["pred"], inp["target"], inp["orig_len"], inp["wt"])
    ck = Check("mse_w" if has_wt else "mse", "f32", case=cid, branch=branch, orig_len=int(has_len), grad=int(has_grad))
    ck.fixed("sum", E.rel1(acc.item() - PRELOAD, s64), ck.bound(s32.reshape(1), s64.reshape(1), relmax, E.SUM_CAP))
    if has_grad:
        grad.intact()
        g = grad.values().view(B, Dch, L)
        ck.fixed("grad_mismatches", (g != g32).sum().item(), 0)
    ck.done()
    assert not has_grad or torch.equal(g, g32)                                           # (2 w) (pred - target): one subtraction, one product


@pytest.mark.parametrize("n", E.FLAT_N)
def test_sqnorm(n):
    ck = Check("sqnorm", "f32", n=n, branch=",".join(sorted(E.branches_flat(n))))
    gi = E.ints("sq.i", (n,), 3)
    acc = torch.full((1,), PRELOAD, dtype=F64, device=DEV)
    ops.call("osuf_sqnorm", p(dev(gi)), n, p(acc), stream())
    want = E.sqnorm(gi.double()) + PRELOAD
    ck.fixed("int_sum_off", abs(acc.item() - want.item()), 0)                            # every partial sum is a small integer: exact
    g = E.uni("sq.g", (n,), 3.0)
    acc2 = torch.full((1,), PRELOAD, dtype=F64, device=DEV)
    ops.call("osuf_sqnorm", p(dev(g)), n, p(acc2), stream())
    s64, s32 = E.sqnorm(g.double()), E.sqnorm(g)
    ck.fixed("sum", E.rel1(acc2.item() - PRELOAD, s64), ck.bound(s32.reshape(1), s64.reshape(1), relmax, E.SUM_CAP))
    ck.done()
    assert torch.equal(acc.cpu(), want.reshape(1))


@functools.lru_cache(maxsize=None)
def adamw_state(n):
    return E.adamw_inputs(n)


def adamw_case(n, step, gs, wd):
    pt, g, m, v = adamw_state(n)
    hyper = E.HYPER + (wd,)
    fp, fm, fv = Frame(1, n), Frame(1, n), Frame(1, n)
    for f, t in ((fp, pt), (fm, m), (fv, v)):
        f.view.copy_(t.view(1, n))
    gsd = None if gs is None else torch.tensor([gs], dtype=F32, device=DEV)
    ops.call("osuf_adamw", p(fp.view), p(dev(g)), p(fm.view), p(fv.view), n, *hyper, step, p(gsd), stream())
    for f in (fp, fm, fv):
        f.intact()
    gsv = 1.0 if gs is None else gs
    r64 = E.adamw_step(pt.double(), g.double(), m.double(), v.double(), hyper, step, gsv)
    r32 = E.adamw_step(pt, g, m, v, hyper, step, gsv)
    ck = Check("adamw", "f32", n=n, step=step, gscale=-1.0 if gs is None else gs, wd=wd, branch=",".join(sorted(E.branches_flat(n))))
    ck.f32("m", fm.values().view(n), r64[1], r32[1], relmax, E.MOMENT_CAP)
    ck.f32("v", fv.values().view(n), r64[2], r32[2], relmax, E.MOMENT_CAP)
    ck.f32("update", fp.values().view(n), r64[0], r32[0], E.update_metric(pt), E.UPDATE_CAP)
    ck.done()


@pytest.mark.parametrize("wd", E.ADAMW_WD)
@pytest.mark.parametrize("gs", E.ADAMW_GSCALE)
@pytest.mark.parametrize("step", E.ADAMW_STEPS)
@pytest.mark.parametrize("n", E.FLAT_N)
def test_adamw(n, step, gs, wd):
    """One step from a given state: m', v' at relmax, and the update p' - p element by element beside p's own spacing.  The last n takes
    two trips of the four-wide body and block 0's tail."""
    adamw_case(n, step, gs, wd)


@pytest.mark.parametrize("has_tn", [False, True])
@pytest.mark.parametrize("sumsq,max_norm,base,branch", E.CLIP)
def test_clip_coef(sumsq, max_norm, base, branch, has_tn):
    ss = torch.tensor([sumsq], dtype=F64, device=DEV)
    coef, tn = Frame(1, 1), Frame(1, 1)
    ops.call("osuf_clip_coef", p(ss), max_norm, base, p(coef.view), p(tn.view) if has_tn else None, stream())
    coef.intact(), tn.intact()
    got, want = coef.values().item(), E.clip_coef(sumsq, max_norm, base)
    ck = Check("clip_coef", "f32", sumsq=sumsq, max_norm=max_norm, base=base, branch=branch, total_norm=int(has_tn))
    ck.fixed("coef", E.rel1(got, want), E.CLIP_TOL if branch == "active" else 0)
    if has_tn:
        ck.fixed("total_norm_off", abs(tn.values().item() - float(np.float32(np.sqrt(np.float64(sumsq))))), 0)
    else:
        assert (tn.bits() == SENT[F32]).all()
    ck.done()
    assert branch == "active" or got == base


@pytest.mark.parametrize("per", E.AXPBY)
def test_axpby_rows(per):
    B = E.STEP_B
    x, y = E.uni("ax.x", (B, per), 1.5), E.uni("ax.y", (B, per), 1.5)
    coef = E.ddim_coef().to(F32)
    ca, cb = coef[:, 1].contiguous(), coef[:, 0].contiguous()
    out = Frame(1, B * per)
    ops.call("osuf_axpby_rows", p(dev(x)), p(dev(y)), p(dev(ca)), p(dev(cb)), p(out.view), B, per, stream())
    out.intact()
    ck = Check("axpby_rows", "f32", per_sample=per, branch=E.passes(B * per))
    ck.out("out", out.values().view(B, per), E.axpby(x.double(), y.double(), ca.double(), cb.double()), E.axpby(x, y, ca, cb), E.STEP_CAP)
    ck.done()


@pytest.mark.parametrize("case", E.DDIM, ids=ID0)
def test_ddim_step(case):
    cid, per, has_null, cs, sn, span = case
    B = E.STEP_B
    inp = E.ddim_inputs(cid, B, per, has_null, cs, span)
    out = Frame(1, B * per)
    ops.call("osuf_ddim_step", p(dev(inp["x"])), p(dev(inp["cond"])), p(dev(inp["null"])), cs, p(dev(inp["coef"])), p(out.view), B, per, stream())
    out.intact()
    d = lambda t: None if t is None else t.double()
    r64 = E.ddim_step(d(inp["x"]), d(inp["cond"]), d(inp["null"]), cs, d(inp["coef"]))
    r32 = E.ddim_step(inp["x"], inp["cond"], inp["null"], cs, inp["coef"])
    ck = Check("ddim_step", "f32", case=cid, branch=f"{E.passes(B * per)},clamp={sn},null={int(has_null)}")
    ck.out("out", out.values().view(B, per), r64, r32, E.STEP_CAP)
    ck.done()


# ---------------------------------------------------------------------------------------------------------------------------------
# D. contract
# ---------------------------------------------------------------------------------------------------------------------------------
def good_calls():
    """entry point -> (ordered {argument: value} of a call that would succeed, the tensors it would write).  Pointer arguments hold the
    device tensor; outputs are sentinel-filled frames."""
    f = lambda n, dtype=F32: Frame(1, n, None, dtype)
    z = lambda *shape: torch.zeros(*shape, dtype=F32, device=DEV)
    g = {}
    o = f(40 * 3 * 96)
    g["osuf_ncl_to_rows"] = (dict(dtype=ops.F32, inp=z(3, 6, 40), out=o, ld=96, width=96, B=3, C=6, L=40, KT=15), [o])
    o = f(3 * 6 * 40)
    g["osuf_rows_to_ncl"] = (dict(dtype=ops.F32, inp=z(120, 8), ld=8, out=o, B=3, C=6, L=40), [o])
    o = f(5 * 40)
    g["osuf_copy2d"] = (dict(sdt=ops.F32, src=z(5, 32), lds=32, ddt=ops.F32, dst=o, ldd=40, M=5, cols=24), [o])
    o = f(5 * 48)
    g["osuf_add2d"] = (dict(dtype=ops.F32, a=z(5, 32), lda=32, b=z(5, 40), ldb=40, dst=o, ldd=48, M=5, cols=24), [o])
    o, s = f(3 * 6 * 50), f(1, F64)
    g["osuf_mse"] = (dict(pred=z(3, 6, 50), target=z(3, 6, 50), orig_len=None, grad=o, loss_sum=s, B=3, Dch=6, L=50), [o, s])
    o, s = f(3 * 6 * 50), f(1, F64)
    g["osuf_mse_w"] = (dict(pred=z(3, 6, 50), target=z(3, 6, 50), orig_len=None, w=z(3), grad=o, loss_sum=s, B=3, Dch=6, L=50), [o, s])
    s = f(1, F64)
    g["osuf_sqnorm"] = (dict(g=z(1032), n=1027, out=s), [s])
    fp, fm, fv = f(1032), f(1032), f(1032)
    lr, b1, b2, eps = E.HYPER
    g["osuf_adamw"] = (dict(p=fp, g=z(1032), m=fm, v=fv, n=1027, lr=lr, b1=b1, b2=b2, eps=eps, wd=0.0, step=1, gscale=None), [fp, fm, fv])
    c, t = f(1), f(1)
    g["osuf_clip_coef"] = (dict(sumsq=torch.ones(1, dtype=F64, device=DEV), max_norm=1.0, base=1.0, coef=c, total_norm=t), [c, t])
    o = f(1032, BF16)
    g["osuf_cast_f32_bf16"] = (dict(src=z(1032), dst=o, n=1027), [o])
    o = f(4 * 600)
    g["osuf_axpby_rows"] = (dict(x=z(4, 600), y=z(4, 600), ca=z(4), cb=z(4), out=o, B=4, per=600), [o])
    o = f(4 * 600)
    g["osuf_ddim_step"] = (dict(x=z(4, 600), cond=z(4, 600), null=None, cs=1.0, coef=torch.ones(4, 4, device=DEV), out=o, B=4, per=600), [o])
    return g


def pointer(v, how=None):
    if how == "null":
        return None
    t = v.view if isinstance(v, Frame) else v
    return None if t is None else t.data_ptr() + (4 if how == "off4" else 0)


def test_bad_arguments_are_refused():
    """Every line of E.EW_BAD: the status it names, before any launch -- every output frame still holds its sentinel in every cell."""
    lib = _lib.load()
    good = good_calls()
    assert set(good) == {e for e, _, _ in E.EW_BAD}
    for entry, kind, over in E.EW_BAD:
        args, _ = good[entry]
        assert set(over) <= set(args), (entry, over)
        call = []
        for name, v in args.items():
            o = over.get(name)
            if isinstance(v, (Frame, torch.Tensor)) or (v is None and o in ("null", "off4")):
                assert o in (None, "null", "off4"), (entry, name, o)
                call.append(pointer(v, o))
            else:
                call.append(v if o is None else o)
        assert getattr(lib, entry)(*call, stream()) == E.bad_status(kind), (entry, kind, over)
    torch.cuda.synchronize()
    for entry, (_, outs) in good.items():
        for o in outs:
            assert (o.bits() == SENT[o.dtype]).all(), (entry, "an output was written by a refused call")
