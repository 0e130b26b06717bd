"""The LoRA / DoRA adapter kernels of csrc/elementwise.hip (osuf_dora_effective, osuf_dora_gain, osuf_pack_weight_adapted,
osuf_adapter_finish) against plain fp64 references, on every branch their launchers pick from the row width, the rank and the tap count.
Launches go through ops.call on the raw entry points, so that strides, NULL arguments and destinations are the test's to choose; no launch
consumes another kernel's output (the gain a pack is handed is generated, not computed by osuf_dora_gain).

References, generators and case tables: tests/adapter_reference.py (checked on the CPU by tests/test_adapter_reference_cpu.py, which also
holds every cap used here at the smallest step above 16 x the fp32 evaluation's own noise).  The branch each case reaches is named in its
table entry and goes to the parity metrics file with the achieved figures (adapter_rows::*).  Rows differ in magnitude by factors of two in
every case and every metric is per element (relmax, Check.out), never a whole-tensor norm.

A. Exact: integer w (each value names its (o, i, t)), integer A and B, s and g powers of two; integer tb / gt and bases for the finish:
   torch.equal against the fp64 result, in f32 and, rounded once, in bf16.
B. Real-valued, bounded (tests/bound_check.py): 16 x e32, floored at 1e-6, capped as the tables say; bf16 outputs within one bf16 spacing.
C. Every output sits in a sentinel frame that stays intact; NULL outputs are honoured; refused launches return their code and write nothing.
"""
import functools

import pytest
import torch

from osufusion_amd import _lib, ops
from tests import adapter_reference as R
from tests import bound_check
from tests.test_poisoned_memory import relmax

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
SENT = -768.0                                              # exact in bf16
GUARD = 8
EINVAL, EUNSUPPORTED = _lib.CONSTS["OSUF_EINVAL"], _lib.CONSTS["OSUF_EUNSUPPORTED"]
DT = {"f32": (F32, ops.F32), "bf16": (BF16, ops.BF16)}
DKIND = {"same": 0, "down": 1, "up": 2}
ID0 = lambda v: v[0] if isinstance(v, tuple) else None


class Check(bound_check.Check):
    prefix = "adapter_rows"


def stream():
    return torch.cuda.current_stream().cuda_stream


def p(t):
    return None if t is None else t.data_ptr()


def dev(t):
    return None if t is None else t.contiguous().to(DEV)


def flat(n, dtype=F32, fill=SENT):
    """(buffer, the n elements the kernel is given) with GUARD sentinels on either side."""
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def flat_intact(buf, n, fill=SENT):
    b = buf.cpu().float()
    assert (b[:GUARD] == fill).all() and (b[GUARD + n:] == fill).all(), "written outside the output"


def untouched(*ts):
    return all((t.cpu().float() == SENT).all() for t in ts)


def same(ck, key, got, want64):
    """Exact: the count of differing elements goes to the metrics (bound 0); the assertion names the first of them."""
    got, want = got.cpu(), want64.to(F32).to(got.dtype)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = (got != want).nonzero()
    ck.fixed(key + "_mismatches", len(bad), 0)
    return lambda: (key, len(bad), "first bad indices:", bad[:8].tolist())


def finish_same(ck, fails):
    ck.done()
    for f in fails:
        assert f()[1] == 0, f()


# ---------------------------------------------------------------------------------------------------------------------------------
# osuf_dora_effective
# ---------------------------------------------------------------------------------------------------------------------------------
def effective_where(e):
    oc, attr, blocks, last = e[6]
    return dict(case=e[0], branch=f"OC={oc},attr={int(attr)},blocks={blocks},last={last},mag={int(e[4])},g={int(e[5])}")


@functools.lru_cache(maxsize=None)
def effective_real(cid, O, IK, r, mag):
    f32 = R.real_factors(cid, O, IK, 1, r, mag)
    return f32, R.effective(*R.cast(f32, F64), R.S), R.effective(*f32, R.S)


@pytest.mark.parametrize("e", R.EFFECTIVE, ids=ID0)
def test_dora_effective_bounded(e):
    cid, O, IK, r, mag, gout, _ = e
    (W, A, B, m), (w64, g64), (w32, g32) = effective_real(cid, O, IK, r, mag)
    wbuf, weff = flat(O * IK)
    gbuf, g = flat(O)
    Wd, Ad, Bd, md = (dev(t) for t in (W, A, B, m))                                      # held until the launch is queued
    ops.call("osuf_dora_effective", p(Wd), p(Ad), p(Bd), p(md), O, IK, r, R.S, p(weff), p(g) if gout else None, stream())
    flat_intact(wbuf, O * IK)
    flat_intact(gbuf, O)
    ck = Check("dora_effective", F32, **effective_where(e))
    ck.out("Weff", weff.view(O, IK), w64.reshape(O, IK), w32.reshape(O, IK), R.EFFECTIVE_CAP)
    if gout and mag:
        ck.out("g", g, g64, g32, R.G_CAP)
    ck.done()
    if not gout:
        assert untouched(g)
    elif not mag:
        assert torch.equal(g.cpu(), torch.ones(O)), "g must be exactly 1 without a magnitude"


def test_dora_effective_refusals_write_nothing():
    """A row of more than 150 KiB, NULL pointers and empty shapes: OSUF_EINVAL."""
    lib = _lib.load()
    O, IK = R.EFFECTIVE_EINVAL
    assert R.effective_branch(O, IK) == "einval"
    W, A, B, m = (torch.ones(n, device=DEV) for n in (O * IK, IK, O, O))
    wbuf, weff = flat(O * IK)
    gbuf, g = flat(O)
    assert lib.osuf_dora_effective(p(W), p(A), p(B), p(m), O, IK, 1, R.S, p(weff), p(g), stream()) == EINVAL
    good = [p(W), p(A), p(B), p(m), O, 16, 1, R.S, p(weff), p(g)]
    for i, v in [(0, None), (1, None), (2, None), (8, None), (4, 0), (4, -1), (5, 0), (5, -1), (6, 0), (6, -1)]:
        a = list(good)
        a[i] = v
        assert lib.osuf_dora_effective(*a, stream()) == EINVAL, (i, v)
    assert untouched(wbuf, gbuf)


# ---------------------------------------------------------------------------------------------------------------------------------
# osuf_dora_gain
# ---------------------------------------------------------------------------------------------------------------------------------
def adapt_where(e, br):
    kind, it, ot, chunks = br
    return dict(case=e[0], branch=f"lds={kind},i_tiles={it},o_tiles={ot},tap_chunks={chunks}")


@pytest.mark.parametrize("e", R.GAIN, ids=ID0)
def test_dora_gain_bounded(e):
    cid, O, I, k, r, mag, outs, br = e
    W, A, B, m = R.real_factors(cid, O, I, k, r, mag)
    g64 = R.gain(R.adapted(W.double(), A.double(), B.double(), R.S), m.double()) if mag else None
    g32 = R.gain(R.adapted(W, A, B, R.S), m) if mag else None
    t64, t32r = R.sgbt(B.double(), g64, R.S), R.sgbt(B, g32, R.S)
    gbuf, g = flat(O)
    b32, t32 = flat(r * O)
    b16, t16 = flat(r * O, BF16)
    pbuf, part = flat(-(-I // 32) * O)
    Wd, Ad, Bd, md = (dev(t) for t in (W, A, B, m))
    ops.call("osuf_dora_gain", p(Wd), p(Ad), p(Bd), p(md), O, I, k, r, R.S, p(part) if mag else None, p(g),
             p(t32) if outs != "16" else None, p(t16) if outs != "32" else None, stream())
    for buf, n in ((gbuf, O), (b32, r * O), (b16, r * O), (pbuf, part.numel())):
        flat_intact(buf, n)
    ck = Check("dora_gain", F32, **adapt_where(e, br), mag=int(mag), outs=outs)
    if mag:
        ck.out("g", g, g64, g32, R.G_CAP)
    if outs != "16":
        ck.out("sgbt32", t32.view(r, O), t64, t32r, R.SGBT_CAP)
    if outs != "32":
        ck.out("sgbt16", t16.view(r, O), t64, t32r, R.SGBT_CAP)
    if outs == "both":                                                                   # the bf16 operand is the f32 one rounded to nearest even
        ck.fixed("sgbt16_not_rne_of_sgbt32", (t16.cpu().view(torch.int16) != t32.cpu().to(BF16).view(torch.int16)).sum().item(), 0)
    ck.done()
    assert untouched(t32) or outs != "16"
    assert untouched(t16) or outs != "32"
    if not mag:
        assert torch.equal(g.cpu(), torch.ones(O)) and untouched(part)
        assert outs == "16" or torch.equal(t32.cpu().view(r, O), (R.S * B).T.contiguous())


def test_dora_gain_refusals_write_nothing():
    """More than 96 KiB of adapter slabs: OSUF_EUNSUPPORTED.  A magnitude without the partial workspace, NULL pointers, empty shapes: OSUF_EINVAL."""
    lib = _lib.load()
    r, k = R.ADAPT_UNSUPPORTED
    O, I = 3, 5
    W, A, B, m = (torch.ones(n, device=DEV) for n in (O * I * k, r * I * k, O * r, O))
    bufs = [flat(O), flat(r * O), flat(r * O, BF16), flat(O)]
    (_, g), (_, t32), (_, t16), (_, part) = bufs
    assert lib.osuf_dora_gain(p(W), p(A), p(B), p(m), O, I, k, r, R.S, p(part), p(g), p(t32), p(t16), stream()) == EUNSUPPORTED
    good = [p(W), p(A), p(B), p(m), O, I, k, 2, R.S, p(part), p(g), p(t32), p(t16)]
    for i, v in [(9, None), (0, None), (1, None), (2, None), (10, None), (4, 0), (5, 0), (6, 0), (7, 0), (4, -1), (7, -1)]:
        a = list(good)
        a[i] = v
        assert lib.osuf_dora_gain(*a, stream()) == EINVAL, (i, v)
    assert untouched(*(b for b, _ in bufs))


# ---------------------------------------------------------------------------------------------------------------------------------
# osuf_pack_weight_adapted
# ---------------------------------------------------------------------------------------------------------------------------------
def k_pack(W, A, B, g, r, O, I, k, mode, kind, outs, rows=None, row_offset=0):
    """One launch -> (F view [k][O][I] or None, D view [kd][I][O] or None): the destinations are [k][rows][I] / [kd][I][rows] operands
    (rows = O unless stacked) inside sentinel frames, this weight's rows at row_offset."""
    tdt, code = DT[mode]
    rows = O if rows is None else rows
    kd = k if kind == "same" else 4
    fbuf, Ff = flat(k * rows * I, tdt)
    dbuf, Df = flat(kd * I * rows, tdt)
    F3, D3 = Ff.view(k, rows, I), Df.view(kd, I, rows)
    wantF, wantD = "F" in outs, "D" in outs
    Wd, Ad, Bd, gd = (dev(t) for t in (W, A, B, g))
    ops.call("osuf_pack_weight_adapted", p(Wd), p(Ad), p(Bd), p(gd), R.S, r, O, I, k, code,
             p(F3[0, row_offset:]) if wantF else None, I, rows * I, p(D3[0, 0, row_offset:]) if wantD else None, rows, I * rows, DKIND[kind], stream())
    flat_intact(fbuf, Ff.numel())
    flat_intact(dbuf, Df.numel())
    inside = torch.zeros(rows, dtype=torch.bool)
    inside[row_offset:row_offset + O] = True
    assert (F3.cpu().float()[:, ~inside] == SENT).all() and (D3.cpu().float()[:, :, ~inside] == SENT).all(), "rows of another weight were written"
    assert wantF or untouched(Ff)
    assert wantD or untouched(Df)
    return (F3[:, row_offset:row_offset + O] if wantF else None), (D3[:, :, row_offset:row_offset + O] if wantD else None)


PACK_MODES = [pytest.param(e, mode, id=f"{e[0]}_{mode}") for e in R.PACK for mode in DT]


@pytest.mark.parametrize("e,mode", PACK_MODES)
def test_pack_adapted_exact(e, mode):
    cid, O, I, k, r, kind, hasg, outs, br = e
    W, A, B = R.exact_factors(cid, O, I, k, r)
    g = R.row_pow2(O) if hasg else None
    Fo, Do = k_pack(W, A, B, g, r, O, I, k, mode, kind, outs)
    We = R.scale_rows(R.adapted(W.double(), A.double(), B.double(), R.S), R.cast(g, F64))
    ck = Check("pack_adapted_exact", mode, **adapt_where(e, br), kind=kind, g=int(hasg), outs=outs)
    fails = []
    if Fo is not None:
        fails.append(same(ck, "F", Fo, R.fwd_layout(We)))
    if Do is not None:
        fails.append(same(ck, "D", Do, R.dgrad_layout(We, kind)))
    finish_same(ck, fails)


@functools.lru_cache(maxsize=None)
def pack_real(cid, O, I, k, r, hasg):
    W, A, B, _ = R.real_factors(cid, O, I, k, r, False)
    g = R.real_gain(cid, O) if hasg else None
    w64 = R.scale_rows(R.adapted(W.double(), A.double(), B.double(), R.S), R.cast(g, F64))
    return W, A, B, g, w64, R.scale_rows(R.adapted(W, A, B, R.S), g)


@pytest.mark.parametrize("e,mode", PACK_MODES)
def test_pack_adapted_bounded(e, mode):
    cid, O, I, k, r, kind, hasg, outs, br = e
    W, A, B, g, w64, w32 = pack_real(cid, O, I, k, r, hasg)
    Fo, Do = k_pack(W, A, B, g, r, O, I, k, mode, kind, outs)
    ck = Check("pack_adapted", mode, **adapt_where(e, br), kind=kind, g=int(hasg), outs=outs)
    if Fo is not None:
        ck.out("F", Fo, R.fwd_layout(w64), R.fwd_layout(w32), R.PACK_CAP)
    if Do is not None:
        ck.out("D", Do, R.dgrad_layout(w64, kind), R.dgrad_layout(w32, kind), R.PACK_CAP)
    ck.done()


@pytest.mark.parametrize("mode", DT)
@pytest.mark.parametrize("kind", R.KINDS)
def test_pack_adapted_into_a_stacked_operand(kind, mode):
    """This weight's rows at row_offset of a larger operand (the fused q|kv projection): the other rows keep their sentinels (k_pack), and
    the values are the exact case's."""
    cid, O, I, k, r, rows, off = R.STACKED
    W, A, B = R.exact_factors(cid, O, I, k, r)
    g = R.row_pow2(O)
    Fo, Do = k_pack(W, A, B, g, r, O, I, k, mode, kind, "FD", rows, off)
    We = R.scale_rows(R.adapted(W.double(), A.double(), B.double(), R.S), g.double())
    ck = Check("pack_adapted_stacked", mode, case=cid, branch=f"rows={rows},row_offset={off}", kind=kind)
    finish_same(ck, [same(ck, "F", Fo, R.fwd_layout(We)), same(ck, "D", Do, R.dgrad_layout(We, kind))])


@pytest.mark.parametrize("kind", R.KINDS)
def test_pack_adapted_agrees_with_the_plain_pack_of_the_effective_weight(kind):
    """The f32 adapted pack lies within the bound of osuf_pack_weight (a pure layout change) applied to the fp64 effective weight rounded
    once to fp32."""
    cid, O, I, k, r = "o33_i70_k3_consistency", 33, 70, 3, 8
    W, A, B, g, w64, w32 = pack_real(cid, O, I, k, r, True)
    Fo, Do = k_pack(W, A, B, g, r, O, I, k, "f32", kind, "FD")
    kd = 3 if kind == "same" else 4
    Fp, Dp = torch.empty(k, O, I, device=DEV), torch.empty(kd, I, O, device=DEV)
    wd = dev(w64.float())
    ops.call("osuf_pack_weight", p(wd), O, I, k, ops.F32, p(Fp), I, O * I, p(Dp), O, I * O, DKIND[kind], stream())
    ck = Check("pack_adapted_vs_plain", F32, case=cid, kind=kind)
    ck.f32("F", Fo.contiguous(), Fp.cpu().double(), R.fwd_layout(w32), relmax, R.PACK_CAP)
    ck.f32("D", Do.contiguous(), Dp.cpu().double(), R.dgrad_layout(w32, kind), relmax, R.PACK_CAP)
    ck.done()


def test_pack_adapted_refusals_write_nothing():
    """More than 96 KiB of adapter slabs: OSUF_EUNSUPPORTED.  down / up with k != 3, no destination, NULL factors, empty shapes: OSUF_EINVAL."""
    lib = _lib.load()
    r, k = R.ADAPT_UNSUPPORTED
    O, I = 3, 5
    W, A, B, g = (torch.ones(n, device=DEV) for n in (O * I * k, r * I * k, O * r, O))
    fbuf, Ff = flat(k * O * I)
    dbuf, Df = flat(k * I * O)
    for code in (ops.F32, ops.BF16):
        assert lib.osuf_pack_weight_adapted(p(W), p(A), p(B), p(g), R.S, r, O, I, k, code, p(Ff), I, O * I, p(Df), O, I * O, 0, stream()) == EUNSUPPORTED
    good = [p(W), p(A), p(B), p(g), R.S, 2, O, I, 3, ops.F32, p(Ff), I, O * I, p(Df), O, I * O, 0]
    bad = [(0, None), (1, None), (2, None), (5, 0), (5, -1), (6, 0), (7, 0), (8, 0), (16, 3), (16, -1), (9, 7)]
    for i, v in bad:
        a = list(good)
        a[i] = v
        assert lib.osuf_pack_weight_adapted(*a, stream()) == (EUNSUPPORTED if i == 9 else EINVAL), (i, v)
    for kk, dk in ((1, 1), (7, 2), (4, 1)):                                              # down / up are three-tap layouts
        a = list(good)
        a[8], a[16] = kk, dk
        assert lib.osuf_pack_weight_adapted(*a, stream()) == EINVAL, (kk, dk)
    a = list(good)
    a[10] = a[13] = None                                                                 # neither F nor D
    assert lib.osuf_pack_weight_adapted(*a, stream()) == EINVAL
    assert untouched(fbuf, dbuf)


# ---------------------------------------------------------------------------------------------------------------------------------
# osuf_adapter_finish
# ---------------------------------------------------------------------------------------------------------------------------------
def finish_where(e):
    return dict(case=e[0], branch=f"largest={e[8][0]},blocks={e[8][1]},acc={e[5]},dm={int(e[6])},bias={int(e[7])}")


def k_finish(e, inp):
    """One launch -> (dB, dA, dm views, their buffers): NaN-filled for accumulate = 0, the bases for accumulate = 1."""
    cid, O, I, k, r, acc, hasdm, hasbias, _ = e
    outs = []
    for n, base in zip((O * r, r * I * k, O), inp["bases"]):
        buf, v = flat(n)
        v.copy_(base.reshape(-1)) if acc else v.fill_(float("nan"))
        outs.append((buf, v))
    (_, dB), (_, dA), (_, dm) = outs
    d = {n: dev(inp[n]) for n in ("tb", "sg", "gt", "s0", "s1", "bias", "m")}             # held until the launch is queued
    ops.call("osuf_adapter_finish", p(d["tb"]), p(d["sg"]), p(dB), p(d["gt"]), p(dA), p(d["s0"]) if hasdm else None,
             p(d["s1"]) if hasdm and hasbias else None, p(d["bias"]) if hasdm and hasbias else None, p(d["m"]) if hasdm else None,
             p(dm) if hasdm else None, O, I, k, r, acc, stream())
    for buf, v in outs:
        flat_intact(buf, v.numel())
    return dB.view(O, r), dA.view(r, I, k), dm


def finish_ref(e, inp, dt):
    cid, O, I, k, r, acc, hasdm, hasbias, _ = e
    c = lambda n: R.cast(inp[n], dt)
    return R.finish(c("tb"), c("sg"), c("gt"), c("s0") if hasdm else None, c("s1") if hasdm and hasbias else None,
                    c("bias") if hasdm and hasbias else None, c("m") if hasdm else None, c("bases") if acc else None)


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "real"])
@pytest.mark.parametrize("e", R.FINISH, ids=ID0)
def test_adapter_finish(e, exact):
    """accumulate = 0 overwrites NaN-filled outputs, accumulate = 1 adds to the bases; dB and dA are exact on integers and bounded on real
    values, dm (a division) is bounded in both; without dm its buffer keeps what it held."""
    cid, O, I, k, r, acc, hasdm, hasbias, _ = e
    inp = R.finish_inputs(cid, O, I, k, r, exact)
    dB, dA, dm = k_finish(e, inp)
    (b64, a64, m64), (b32, a32, m32) = finish_ref(e, inp, F64), finish_ref(e, inp, F32)
    ck = Check("adapter_finish_exact" if exact else "adapter_finish", F32, **finish_where(e))
    if hasdm:
        ck.out("dm", dm, m64, m32, R.DM_CAP)
    else:
        held = dm.cpu()
        assert torch.equal(held, inp["bases"][2]) if acc else held.isnan().all(), "dm = NULL, yet its buffer changed"
    if exact:
        finish_same(ck, [same(ck, "dB", dB, b64), same(ck, "dA", dA, a64)])
    else:
        ck.out("dB", dB, b64, b32, R.DM_CAP)
        ck.out("dA", dA, a64, a32, R.DM_CAP)
        ck.done()


def test_adapter_finish_refusals_write_nothing():
    """Every invalid combination of the launcher's line: a NULL operand or output; dm without s0 or m; dm with bias but without s1; an empty
    shape."""
    lib = _lib.load()
    O, I, k, r = 5, 4, 3, 2
    tb, sg, gt, s0, s1, bias, m = (torch.ones(n, device=DEV) for n in (O * r, O, k * I * r, O, O, O, O))
    bufs = [flat(O * r), flat(r * I * k), flat(O)]
    (_, dB), (_, dA), (_, dm) = bufs
    # (tb, sg, dB, gt, dA, s0, s1, bias, m, dm, O, I, k, r, accumulate)
    good = [p(tb), p(sg), p(dB), p(gt), p(dA), p(s0), p(s1), p(bias), p(m), p(dm), O, I, k, r, 1]
    for i, v in [(0, None), (1, None), (2, None), (3, None), (4, None), (5, None), (8, None), (6, None), (10, 0), (11, 0), (12, 0), (13, 0),
                 (10, -1), (13, -1)]:
        a = list(good)
        a[i] = v
        assert lib.osuf_adapter_finish(*a, stream()) == EINVAL, (i, v)
    assert untouched(*(b for b, _ in bufs))
