"""The embedding-sized linears of csrc/skinny.hip (skinny_fwd, skinny_fwd_group, skinny_dx, skinny_dx_group, skinny_dw) against plain fp64
references, on every branch osuf_skinny_fwd / osuf_skinny_bwd and the kernels pick from alignment, stride and size.  Launches go through
ops.call on the raw entry points, so that strides and alignment are the test's to choose; no launch consumes another kernel's output (the y
a backward launch reads is the fp64 forward rounded once to fp32).

References, input generators and case tables: tests/skinny_reference.py (checked on the CPU by tests/test_skinny_reference_cpu.py, which
also holds every cap used here above 16 x the fp32 evaluation's own noise).  The branch each case reaches is named in its table entry and
goes to the parity metrics file with the achieved figures (skinny_rows::*).

A. Geometry, exact: operands are small integers (|x|, |dy| <= 3, |W| <= 2, integer bias and bases), no activation, so every partial sum is
   an integer below 2^24, exact in fp32 in any order, through atomics and in both modes: torch.equal against the fp64 result.
B. Real-valued, bounded (tests/bound_check.py): within 16 x e32 of the fp64 reference evaluated on the operands the kernel saw, e32 being
   the fp32 CPU evaluation's own distance, floored at 1e-6 and capped at 2e-5 relmax (1e-5 for db) in BOTH modes -- the reference rounds
   the same operands to bf16, and the generators keep them clear of the rounding boundaries; an output sigmoid adds FAST = 2^-21, silu'(x)
   on dx adds FAST * (1 + max|x|).  Element by element, nothing is off by more than bound * max|ref| + 2^-20 |ref|.
C. Strided outputs keep their surroundings: y, dx and a group's y_i are columns [8, 8 + width) of sentinel-filled buffers 24 columns wider,
   with one spare row after the last; every cell outside the slice still holds the sentinel, and the values pass B.
D. Contract: every line of sk_bad / sk_group_bad returns OSUF_EINVAL and writes nothing; two launches of an atomic case agree within B's bound.
"""
import functools

import pytest
import torch

from osufusion_amd import _lib, ops
from tests import bound_check
from tests import skinny_reference as S
from tests.test_poisoned_memory import relmax

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = torch.float32, torch.float64
SENT = 777.0
MODE = {"f32": ops.F32, "bf16": ops.BF16}
EINVAL = -1
ID0 = lambda v: v[0] if isinstance(v, tuple) else None


class Check(bound_check.Check):
    prefix = "skinny_rows"


# ---------------------------------------------------------------------------------------------------------------------------------
# placement and launches
# ---------------------------------------------------------------------------------------------------------------------------------
def stream():
    return torch.cuda.current_stream().cuda_stream


def place(t, pad=0, off=0):
    """CPU (rows, cols) fp32 -> a device view of row stride cols + pad that starts `off` floats past a 16-byte boundary."""
    if t is None:
        return None
    if t.dim() == 1:
        return t.to(DEV)
    rows, cols = t.shape
    ld = cols + pad
    base = torch.zeros(off + rows * ld + 8, dtype=F32, device=DEV)
    v = base[off:off + rows * ld].view(rows, ld)[:, :cols]
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 * (off % 4) and (v.stride(0) == ld or rows == 1)
    return v


def dense(rows, cols, fill=SENT):
    return torch.full((rows, cols), fill, dtype=F32, device=DEV)


def framed(M, width):
    """(buffer, the slice the kernel is given): columns [8, 8 + width) of the first M rows of a sentinel-filled (M + 1, width + 24)."""
    buf = dense(M + 1, width + S.PAD_L + S.PAD_R)
    return buf, buf[:M, S.PAD_L:S.PAD_L + width]


def frame_intact(buf, M, width):
    keep = torch.ones(buf.shape, dtype=torch.bool)
    keep[:M, S.PAD_L:S.PAD_L + width] = False
    b = buf.cpu()
    bad = (keep & (b != SENT)).nonzero()
    assert len(bad) == 0, (len(bad), "cells outside the slice were written, first (row, col):", bad[:8].tolist())


def p(t):
    return None if t is None else t.data_ptr()


def ld(t, width):
    return width if t is None else (t.stride(0) if t.shape[0] > 1 else max(t.stride(0), width))


def k_fwd(mode, x, W, b, y, M, N, K, ia, oa):
    ops.call("osuf_skinny_fwd", MODE[mode], p(x), ld(x, K), p(W), p(b), p(y), ld(y, N), M, N, K, ia, oa, stream())


def bwd_args(mode, dy, y, x, W, dx, dW, db, M, N, K, ia, oa, acc, lddx=None):
    return (MODE[mode], p(dy), ld(dy, N), p(y), 0 if y is None else ld(y, N), p(x), ld(x, K), p(W), p(dx), ld(dx, K) if lddx is None else lddx,
            p(dW), p(db), M, N, K, ia, oa, acc, stream())


def k_bwd(*a, **k):
    ops.call("osuf_skinny_bwd", *bwd_args(*a, **k))


def table(rows, per):
    """Device osuf_linear_desc array of (W, bias, y, dy) device tensors, block0 = running sum of ceil(N / per) -> (table, n, total)."""
    import numpy as np
    tab = np.zeros(len(rows), dtype=ops.LINEAR_DESC)
    total = 0
    for j, (W, b, y, dy) in enumerate(rows):
        N = W.shape[0]
        tab[j] = (W.data_ptr(), p(b) or 0, p(y) or 0, p(dy) or 0, 0 if y is None else ld(y, N), 0 if dy is None else ld(dy, N), N, total)
        total += -(-N // per)
    return ops._upload_table(tab, torch.device(DEV)), len(rows), total


def k_fwd_group(mode, x, Ws, bs, ys, M, K, ia):
    tab, n, total = table([(W, b, y, None) for W, b, y in zip(Ws, bs, ys)], 32)
    ops.call("osuf_skinny_fwd_group", MODE[mode], p(x), ld(x, K), tab.data_ptr(), n, total, M, K, ia, stream())


def k_dx_group(mode, dys, Ws, x, dx, M, K, ia):
    tab, n, total = table([(W, None, None, dy) for W, dy in zip(Ws, dys) if dy is not None], 512)
    ops.call("osuf_skinny_dx_group", MODE[mode], tab.data_ptr(), n, total, p(x), ld(x, K), p(dx), ld(dx, K), M, K, ia, stream())


def same(ck, key, got, want64):
    """Exact: the count of differing elements goes to the metrics (bound 0); the assertion names the first of them."""
    got, want = got.cpu(), want64.to(F32)
    assert got.shape == want.shape
    bad = (got != want).nonzero()
    ck.fixed(key + "_mismatches", len(bad), 0)
    ck.done()
    assert torch.equal(got, want), (key, len(bad), "first bad indices:", bad[:8].tolist())


def near(ck, key, got, r64, r32, cap, extra=0.0):
    """Section B's two statements about one tensor."""
    ck.f32(key, got, r64, r32, relmax, cap, extra)
    ck.fixed(key + "_elem", S.elementwise_excess(got, r64, ck.bound(r32, r64, relmax, cap, extra)), 1.0)


def branch_fwd(e):
    return "vec" if e[7] else "nonvec"


def branch_dx(e):
    return f"{'vec' if e[6] else 'nonvec'},slices={e[7]},last={e[8]}"


def branch_dw(e):
    return f"tiles={S.dw_tiles(e[1], e[2])},acc={e[4]},db={int(e[5])}"


@functools.lru_cache(maxsize=None)
def real(cid, M, N, K, ia, oa, mode):
    """Inputs of a real-valued case and its (y, dx) in fp64 and fp32, computed once and left unchanged."""
    inp = S.linear_inputs(cid, M, N, K, ia, oa, mode)
    return inp, S.linear_refs(inp, F64)[:2], S.linear_refs(inp, F32)[:2]


def acts_of(geo):
    return [(1, 2)] if geo else S.ACTS


FWD_B = [pytest.param(e, M, ia, oa, id=f"{e[0]}_m{M}_a{ia}{oa}") for e, M in S.cases(S.FWD) for ia, oa in acts_of(e[6])]
DX_B = [pytest.param(e, M, ia, oa, id=f"{e[0]}_m{M}_a{ia}{oa}") for e, M in S.cases(S.DX) for ia, oa in acts_of(e[5])]
DW_B = [pytest.param(e, M, ia, oa, id=f"{e[0]}_m{M}_a{ia}{oa}") for e, M in S.cases(S.DW) for ia, oa in S.ACTS]
CASE_M = lambda t: [pytest.param(e, M, id=f"{e[0]}_m{M}") for e, M in S.cases(t)]


# ---------------------------------------------------------------------------------------------------------------------------------
# A. geometry, exact
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", S.MODES)
@pytest.mark.parametrize("e,M", CASE_M(S.FWD))
def test_fwd_exact(e, M, mode):
    cid, N, K, _, off, pad, _, _ = e
    x, W = S.ints("x", (M, K), 3), S.ints("W", (N, K), 2)
    b = S.ints("b", (N,), 5) if M == 33 else None                                        # the other M of every shape runs with bias = NULL
    y = dense(M, N)
    k_fwd(mode, place(x, pad, off), place(W), place(b), y, M, N, K, 0, 0)
    same(Check("fwd_exact", mode, case=cid, M=M, branch=branch_fwd(e)), "y", y, S.fwd(x.double(), W.double(), S.cast(b, F64), 0, 0))


@pytest.mark.parametrize("mode", S.MODES)
@pytest.mark.parametrize("e,M", CASE_M(S.DX))
def test_dx_exact(e, M, mode):
    cid, N, K, _, off, *_ = e
    dy, W, x = S.ints("dy", (M, N), 3), S.ints("W", (N, K), 2), S.ints("x", (M, K), 3)
    dx = dense(M, K)
    k_bwd(mode, place(dy, 0, off), None, place(x), place(W), dx, None, None, M, N, K, 0, 0, 0)
    same(Check("dx_exact", mode, case=cid, M=M, branch=branch_dx(e)), "dx", dx, S.dx(dy.double(), None, x.double(), W.double(), 0, 0))


@pytest.mark.parametrize("mode", S.MODES)
@pytest.mark.parametrize("e,M", CASE_M(S.DW))
def test_dw_exact(e, M, mode):
    cid, N, K, _, acc, has_db = e
    dy, x, W = S.ints("dy", (M, N), 3), S.ints("x", (M, K), 3), S.ints("W", (N, K), 2)
    bw, bb = S.ints("bw", (N, K), 5), S.ints("bb", (N,), 5)
    dW, db = bw.clone().to(DEV), bb.clone().to(DEV) if has_db else None
    k_bwd(mode, place(dy), None, place(x), place(W), None, dW, db, M, N, K, 0, 0, acc)
    w64, b64 = S.dw(dy.double(), None, x.double(), 0, 0, bw.double(), bb.double() if has_db else None, bool(acc))
    ck = Check("dw_exact", mode, case=cid, M=M, branch=branch_dw(e))
    if has_db:
        ck.fixed("db_mismatches", (db.cpu() != b64.float()).sum().item(), 0)
    same(ck, "dW", dW, w64)
    assert not has_db or torch.equal(db.cpu(), b64.float())


@pytest.mark.parametrize("mode", S.MODES)
def test_db_without_dw_is_left_alone(mode):
    """dW = NULL with db given ("db needs dW"): no launch, db keeps what it held."""
    M, N, K = 5, 40, 72
    dy, x, W = S.ints("dy", (M, N), 3), S.ints("x", (M, K), 3), S.ints("W", (N, K), 2)
    db = torch.full((N,), SENT, device=DEV)
    k_bwd(mode, place(dy), None, place(x), place(W), None, None, db, M, N, K, 0, 0, 1)
    assert (db.cpu() == SENT).all()


@pytest.mark.parametrize("mode", S.MODES)
@pytest.mark.parametrize("case", S.GROUP, ids=ID0)
def test_group_exact(case, mode):
    cid, M, K, Ns, nobias, nody = case
    x = S.ints("gx", (M, K), 3)
    Ws = [S.ints(f"gW{i}", (N, K), 2) for i, N in enumerate(Ns)]
    bs = [None if i == nobias else S.ints(f"gb{i}", (N,), 5) for i, N in enumerate(Ns)]
    dys = [None if i == nody else S.ints(f"gdy{i}", (M, N), 3) for i, N in enumerate(Ns)]
    xd, Wd = place(x), [place(W) for W in Ws]
    ys, dx = [dense(M, N) for N in Ns], dense(M, K)
    k_fwd_group(mode, xd, Wd, [place(b) for b in bs], ys, M, K, 0)
    k_dx_group(mode, [place(d) for d in dys], Wd, xd, dx, M, K, 0)
    y64, dx64 = S.group_refs(dict(x=x, Ws=Ws, bs=bs, dys=dys), F64, 0, "f32")
    ck = Check("group_exact", mode, case=cid, branch=f"n={len(Ns)},blocks={sum(-(-N // 32) for N in Ns)},slices={sum(-(-N // 512) for N, d in zip(Ns, dys) if d is not None)}")
    for i, (y, r) in enumerate(zip(ys, y64)):
        ck.fixed(f"y{i}_mismatches", (y.cpu() != r.float()).sum().item(), 0)
    same(ck, "dx", dx, dx64)
    for i, (y, r) in enumerate(zip(ys, y64)):
        bad = (y.cpu() != r.float()).nonzero()
        assert len(bad) == 0, (i, len(bad), "first bad indices:", bad[:8].tolist())


# ---------------------------------------------------------------------------------------------------------------------------------
# B. real-valued, bounded
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", S.MODES)
@pytest.mark.parametrize("e,M,ia,oa", FWD_B)
def test_fwd_bounded(e, M, ia, oa, mode):
    cid, N, K, _, off, pad, _, _ = e
    inp, r64, r32 = real(cid, M, N, K, ia, oa, mode)
    y = dense(M, N)
    k_fwd(mode, place(inp["x"], pad, off), place(inp["W"]), place(inp["b"]), y, M, N, K, ia, oa)
    ck = Check("fwd", mode, case=cid, M=M, in_act=ia, out_act=oa, branch=branch_fwd(e))
    near(ck, "y", y, r64[0], r32[0], S.OUT_CAP, S.extra_y(oa))
    ck.done()


@pytest.mark.parametrize("mode", S.MODES)
@pytest.mark.parametrize("e,M,ia,oa", DX_B)
def test_dx_bounded(e, M, ia, oa, mode):
    cid, N, K, _, off, *_ = e
    inp, r64, r32 = real(cid, M, N, K, ia, oa, mode)
    dx = dense(M, K)
    k_bwd(mode, place(inp["dy"], 0, off), place(inp["y"]) if oa else None, place(inp["x"]), place(inp["W"]), dx, None, None, M, N, K, ia, oa, 0)
    ck = Check("dx", mode, case=cid, M=M, in_act=ia, out_act=oa, branch=branch_dx(e))
    near(ck, "dx", dx, r64[1], r32[1], S.OUT_CAP, S.extra_dx(ia, inp["x"]))
    ck.done()


@pytest.mark.parametrize("mode", S.MODES)
@pytest.mark.parametrize("e,M,ia,oa", DW_B)
def test_dw_bounded(e, M, ia, oa, mode):
    """accumulate = 1 adds into a non-zero dW, accumulate = 0 overwrites one; db is always added into a non-zero db."""
    cid, N, K, _, acc, has_db = e
    inp = real(cid, M, N, K, ia, oa, mode)[0]
    bw, bb = S.dw_bases(cid, N, K)
    dW, db = bw.clone().to(DEV), bb.clone().to(DEV) if has_db else None
    k_bwd(mode, place(inp["dy"]), place(inp["y"]) if oa else None, place(inp["x"]), place(inp["W"]), None, dW, db, M, N, K, ia, oa, acc)
    ref = lambda dt: S.dw(*(S.cast(inp[k], dt) for k in ("dy", "y", "x")), ia, oa, S.cast(bw, dt), S.cast(bb, dt) if has_db else None, bool(acc), mode)
    (w64, b64), (w32, b32) = ref(F64), ref(F32)
    ck = Check("dw", mode, case=cid, M=M, in_act=ia, out_act=oa, branch=branch_dw(e))
    near(ck, "dW", dW, w64, w32, S.OUT_CAP)
    if has_db:
        ck.f32("db", db, b64, b32, relmax, S.DB_CAP)
    ck.done()


def group_case(case, mode, ia, strided):
    cid, M, K, Ns, nobias, nody = case
    inp = S.group_inputs(cid, M, K, Ns, nobias, nody)
    xd, Wd = place(inp["x"]), [place(W) for W in inp["Ws"]]
    frames = [framed(M, N) if strided else (None, dense(M, N)) for N in Ns]
    dxbuf, dx = framed(M, K) if strided else (None, dense(M, K))
    k_fwd_group(mode, xd, Wd, [place(b) for b in inp["bs"]], [v for _, v in frames], M, K, ia)
    k_dx_group(mode, [place(d) for d in inp["dys"]], Wd, xd, dx, M, K, ia)
    if strided:
        for (buf, _), N in zip(frames, Ns):
            frame_intact(buf, M, N)
        frame_intact(dxbuf, M, K)
    (y64, dx64), (y32, dx32) = S.group_refs(inp, F64, ia, mode), S.group_refs(inp, F32, ia, mode)
    ck = Check("group_strided" if strided else "group", mode, case=cid, in_act=ia, branch=f"n={len(Ns)},slices={sum(-(-N // 512) for N, d in zip(Ns, inp['dys']) if d is not None)}")
    for i, (_, y) in enumerate(frames):
        near(ck, f"y{i}", y, y64[i], y32[i], S.OUT_CAP)
    near(ck, "dx", dx, dx64, dx32, S.OUT_CAP, S.extra_dx(ia, inp["x"]))
    ck.done()


@pytest.mark.parametrize("mode", S.MODES)
@pytest.mark.parametrize("ia", S.GROUP_ACTS)
@pytest.mark.parametrize("case", S.GROUP, ids=ID0)
def test_group_bounded(case, ia, mode):
    group_case(case, mode, ia, False)


# ---------------------------------------------------------------------------------------------------------------------------------
# C. strided outputs keep their surroundings
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", S.MODES)
def test_strided_y_keeps_its_frame(mode):
    cid, N, K = S.STRIDED_FWD
    M, ia, oa = S.STRIDED_M, 1, 2
    inp, r64, r32 = real(cid + "_strided", M, N, K, ia, oa, mode)
    buf, y = framed(M, N)
    k_fwd(mode, place(inp["x"]), place(inp["W"]), place(inp["b"]), y, M, N, K, ia, oa)
    frame_intact(buf, M, N)
    ck = Check("fwd_strided", mode, case=cid, M=M, branch=f"vec,ldy={y.stride(0)}")
    near(ck, "y", y, r64[0], r32[0], S.OUT_CAP, S.extra_y(oa))
    ck.done()


@pytest.mark.parametrize("mode", S.MODES)
@pytest.mark.parametrize("cid,N,K", S.STRIDED_DX)
def test_strided_dx_keeps_its_frame(cid, N, K, mode):
    """One slice stores into the K columns; several slices zero them first -- and only them, at the pitch of dx -- and add with atomics."""
    M, ia, oa = S.STRIDED_M, 1, 2
    inp, r64, r32 = real(cid + "_strided", M, N, K, ia, oa, mode)
    buf, dx = framed(M, K)
    k_bwd(mode, place(inp["dy"]), place(inp["y"]), place(inp["x"]), place(inp["W"]), dx, None, None, M, N, K, ia, oa, 0)
    frame_intact(buf, M, K)
    ck = Check("dx_strided", mode, case=cid, M=M, branch=f"slices={S.bwd_split(N, K)[0]},lddx={dx.stride(0)}")
    near(ck, "dx", dx, r64[1], r32[1], S.OUT_CAP, S.extra_dx(ia, inp["x"]))
    ck.done()


@pytest.mark.parametrize("mode", S.MODES)
def test_strided_group_keeps_its_frames(mode):
    group_case(S.STRIDED_GROUP, mode, 1, True)


# ---------------------------------------------------------------------------------------------------------------------------------
# D. contract
# ---------------------------------------------------------------------------------------------------------------------------------
BAD = [(0, 40, 72, 0, 0), (5, 0, 72, 0, 0), (5, 40, 0, 0, 0), (-1, 40, 72, 0, 0), (5, -8, 72, 0, 0), (5, 40, -8, 0, 0),
       (5, 40, 72, 2, 0), (5, 40, 72, 3, 0), (5, 40, 72, -1, 0), (5, 40, 72, 0, 1), (5, 40, 72, 0, 3), (5, 40, 72, 1, -1)]


def untouched(*ts):
    return all((t.cpu() == SENT).all() for t in ts)


@pytest.mark.parametrize("M,N,K,ia,oa", BAD)
def test_bad_arguments_are_refused(M, N, K, ia, oa):
    """Every line of sk_bad, through both per-linear entry points: OSUF_EINVAL, and nothing is written."""
    lib = _lib.load()
    m, n, k = 5, 40, 72
    x, W, dy, yin = place(S.ints("x", (m, k), 3)), place(S.ints("W", (n, k), 2)), place(S.ints("dy", (m, n), 3)), dense(m, n, 0.5)
    y, dx, dW, db = dense(m, n), dense(m, k), dense(n, k), torch.full((n,), SENT, device=DEV)
    for mode in S.MODES:
        assert lib.osuf_skinny_fwd(MODE[mode], p(x), k, p(W), None, p(y), n, M, N, K, ia, oa, stream()) == EINVAL
        assert lib.osuf_skinny_bwd(MODE[mode], p(dy), n, p(yin), n, p(x), k, p(W), p(dx), k, p(dW), p(db), M, N, K, ia, oa, 1, stream()) == EINVAL
    assert untouched(y, dx, dW, db)


def test_bad_backward_arguments_are_refused():
    """out_act = 2 without y, and a dx narrower than its rows."""
    lib = _lib.load()
    m, n, k = 5, 40, 72
    x, W, dy, yin = place(S.ints("x", (m, k), 3)), place(S.ints("W", (n, k), 2)), place(S.ints("dy", (m, n), 3)), dense(m, n, 0.5)
    dx, dW, db = dense(m, k), dense(n, k), torch.full((n,), SENT, device=DEV)
    for mode in S.MODES:
        assert lib.osuf_skinny_bwd(MODE[mode], p(dy), n, None, 0, p(x), k, p(W), p(dx), k, p(dW), p(db), m, n, k, 0, 2, 0, stream()) == EINVAL
        assert lib.osuf_skinny_bwd(MODE[mode], p(dy), n, p(yin), n, p(x), k, p(W), p(dx), k - 8, p(dW), p(db), m, n, k, 0, 2, 0, stream()) == EINVAL
    assert untouched(dx, dW, db)


def test_bad_group_arguments_are_refused():
    """Every line of sk_group_bad and of the two group entry points' own checks."""
    lib = _lib.load()
    M, K, N = 5, 96, 40
    xbuf = place(S.ints("x", (M, K + 8), 3))
    x, x1 = xbuf[:, :K], xbuf.reshape(-1)[1:1 + M * K].view(M, K)                        # x1: one float off a 16-byte boundary
    W, dy = place(S.ints("W", (N, K), 2)), place(S.ints("dy", (M, N), 3))
    y, dx = dense(M, N), dense(M, K)
    ft, n, blocks = table([(W, None, y, None)], 32)
    dt, _, slices = table([(W, None, None, dy)], 512)
    ldx = x.stride(0)
    # (x, ldx, n, total, M, K, in_act, lddx)
    good = (x, ldx, n, 1, M, K, 0, K)
    bad = [(x, ldx, n, 1, M, 12, 0, 12), (x, ldx, n, 1, M, 100, 0, 100), (x, ldx + 2, n, 1, M, K, 0, K), (x1, K, n, 1, M, K, 0, K), (None, ldx, n, 1, M, K, 0, K),
           (x, ldx, 0, 1, M, K, 0, K), (x, ldx, -1, 1, M, K, 0, K), (x, ldx, n, 0, M, K, 0, K), (x, ldx, n, 1, 0, K, 0, K), (x, ldx, n, 1, -3, K, 0, K),
           (x, ldx, n, 1, M, 0, 0, K), (x, ldx, n, 1, M, K, 2, K), (x, ldx, n, 1, M, K, 3, K)]
    assert x1.data_ptr() % 16 == 4 and blocks == 2 and slices == 1
    for mode in S.MODES:
        for xx, l, nn, tot, m, k, ia, lddx in bad:
            assert lib.osuf_skinny_fwd_group(MODE[mode], p(xx), l, ft.data_ptr(), nn, tot * blocks, m, k, ia, stream()) == EINVAL, (xx is x, l, nn, tot, m, k, ia)
            assert lib.osuf_skinny_dx_group(MODE[mode], dt.data_ptr(), nn, tot, p(xx), l, p(dx), lddx, m, k, ia, stream()) == EINVAL, (xx is x, l, nn, tot, m, k, ia)
        xx, l, nn, tot, m, k, ia, lddx = good
        assert lib.osuf_skinny_fwd_group(MODE[mode], p(xx), l, None, nn, blocks, m, k, ia, stream()) == EINVAL
        assert lib.osuf_skinny_dx_group(MODE[mode], None, nn, tot, p(xx), l, p(dx), lddx, m, k, ia, stream()) == EINVAL
        assert lib.osuf_skinny_dx_group(MODE[mode], dt.data_ptr(), nn, tot, p(xx), l, None, lddx, m, k, ia, stream()) == EINVAL
        assert lib.osuf_skinny_dx_group(MODE[mode], dt.data_ptr(), nn, tot, p(xx), l, p(dx), k - 8, m, k, ia, stream()) == EINVAL     # lddx < K
    assert untouched(y, dx)


@pytest.mark.parametrize("mode", S.MODES)
def test_atomic_slices_repeat_within_the_bound(mode):
    """Two launches of the same three-slice case add their slices in whatever order the hardware takes them: each is within B's bound of the
    reference (test_dx_bounded), and they differ from each other by no more than that bound; they need not be bit-equal."""
    cid, N, K = "n264_k256", 264, 256
    M, ia, oa = 33, 1, 2
    assert S.bwd_split(N, K)[0] == 3
    inp, r64, r32 = real(cid, M, N, K, ia, oa, mode)
    args = [place(inp[k]) for k in ("dy", "y", "x", "W")]
    got = []
    for _ in range(2):
        dx = dense(M, K)
        k_bwd(mode, *args, dx, None, None, M, N, K, ia, oa, 0)
        got.append(dx.cpu())
    ck = Check("dx_repeat", mode, case=cid, M=M, branch="slices=3")
    b = ck.bound(r32[1], r64[1], relmax, S.OUT_CAP, S.extra_dx(ia, inp["x"]))
    ck.fixed("run_to_run", relmax(got[0], got[1].double()), b)
    ck.done()
