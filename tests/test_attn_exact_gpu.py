"""Every attention kernel against the fp64 reference on inputs whose answer is exact (tests/attn_reference.py): selector, tie and
shifted cases, bias cases for the masked kernels, RoPE by quarter turns.  P and dS are exactly representable in bf16, so a dropped or
doubled key, a row constant of the wrong (batch, head, row), a skipped rescale or a wrong table entry is an O(1) error.

Bounds (they follow from the construction, not from the kernels): the one inexact step is exp2(score * c - lse2) next to an lse2 of
magnitude up to ~700, whose fp32 spacing 6.1e-5 puts a relative 2e-4 on P and dS.  So
  * a nonzero quantity: relmax <= REL = 2e-4 against fp64 (fp32 outputs, and bf16 outputs whose exact value is bf16-representable; other bf16
    outputs get one bf16 spacing on top, Check.out);
  * a quantity that is exactly zero (selector dQ, dK, dbias): max-abs <= REL * max|dO| max|v| D * s (dQ, dK) or without s (dbias);
  * lse2: 2 ulp of its magnitude + 1e-6.
Every figure goes to the parity metrics file under "attn_exact::".
"""
import pytest
import torch

from tests import attn_reference as R
from tests.bound_check import Check

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from osufusion_amd import cross_attend as X
    from osufusion_amd import ops

DEV = "cuda"
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
REL = 2e-4
DTYPES = [F32, BF16]


class Exact(Check):
    prefix = "attn_exact"

    def value(self, key, got, ref):
        """a nonzero quantity"""
        got, refd = got.detach(), ref.to(got.device)                 # (the figures are formed where the output lies)
        # is the exact value a bf16 number?  (the general reference carries the e^-40 weights of the other keys: 1e-9 of the largest value)
        if got.dtype == BF16 and (refd.to(BF16).double() - refd).abs().max() > 1e-9 * refd.abs().max():
            return self.out(key, got.cpu(), ref, ref, REL, extra=REL)
        self.fixed(key, ((got.double() - refd).abs().max() / refd.abs().max()).item(), REL)

    def zero(self, key, got, ref, scale):
        """a quantity whose exact value is zero: relative to the terms that cancel in it"""
        self.fixed(key + "_abs", (got.detach().double() - ref.to(got.device)).abs().max().item(), REL * scale)

    def grad(self, key, got, ref, is_zero, scale):
        self.zero(key, got, ref, scale) if is_zero else self.value(key, got, ref)

    def lse(self, got, ref):
        self.fixed("lse2", ((got.detach().cpu().double() - ref).abs() / (2 * R.ulp32(ref) + 1e-6)).max().item(), 1.0)

    def finite(self, **outs):
        for k, t in outs.items():
            assert torch.isfinite(t).all(), (self.kernel, self.where, k, "not finite")


def strided(x, dtype=BF16, left=8, right=24):
    """x as a column view of a wider row buffer (filled with a value no kernel may read or overwrite unnoticed)"""
    buf = torch.full((*x.shape[:-1], x.shape[-1] + left + right), 777.0, dtype=dtype, device=DEV)
    view = buf[..., left:left + x.shape[-1]]
    view.copy_(x)
    return view


def lse_layout(l, G):
    """reference lse2 / delta (B, H, N) -> the kernels' [G][B][H/G][N] for G > 1"""
    B, H, N = l.shape
    return l if G == 1 else l.view(B, G, H // G, N).permute(1, 0, 2, 3).contiguous()


def kinds_for(N, shifts):
    ks = [("selector", 0)] + ([("tie", 0)] if N >= 2 else [])
    if N in shifts:
        ks += [("selector", -1), ("selector", 1)] + ([("tie", -1)] if N >= 2 else [])
    return ks


def shape_for(N):
    """B, H per length: B = 9 at N = 512 (the b >= 8 pass of the key-stationary block map), H = 3 / 16 at one length each"""
    return {512: (9, 2), 65: (2, 3), 64: (1, 16), 1024: (1, 2), 2048: (1, 2), 1: (2, 1)}.get(N, (2, 2))


def ref_rows(ref, G=1):
    return {"o": R.rows(ref["o"]), "lse2": lse_layout(ref["lse2"], G), "dq": R.rows(ref["dq"]) if "dq" in ref else None,
            "dk": R.rows(ref["dk"]) if "dk" in ref else None, "dv": R.rows(ref["dv"]) if "dv" in ref else None}


# ---- forward, head dim 64 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", R.LENGTHS)
def test_mqa_fwd_64(N):
    """mqa_fwd_kernel: plain / WHOLE (N % 64 == 0), pre-scaled queries, rope in the kernel with and without write_q, zero_dq; osuf_rope_cast / _qs."""
    D = 64
    B, H = shape_for(N)
    cos, sin = R.quarter_tables(N, D)
    cosd, sind = cos.to(DEV), sin.to(DEV)
    cq = float(torch.tensor(D ** -0.5, dtype=F32) * torch.tensor(R.LOG2E, dtype=F32))
    for kind, shift in kinds_for(N, R.SHIFT_FWD):
        c = R.make_case(kind, B, N, N, H, 1, D, shift=shift, seed=N)
        where = dict(N=N, B=B, H=H, kind=kind, shift=shift)
        ref = ref_rows(R.attention_fp64(c.q, c.k, c.v, None, c.scale))
        rot = c.rows_qkv()
        raw = torch.cat([R.rows(R.rope(c.q, cos, sin, True)), R.rows(R.rope(c.k, cos, sin, True)), R.rows(c.v)], -1)
        qkv = strided(rot)
        outs = {}
        for dt in DTYPES:
            o, lse = ops.mqa_fwd(qkv, B, N, H, D, dt, c.scale)
            ck = Exact("mqa_fwd", dt, **where)
            ck.finite(o=o, lse=lse); ck.value("o", o, ref["o"]); ck.lse(lse, ref["lse2"]); ck.done()
            outs[dt] = o
        # zero_dq: the accumulator is cleared, o and lse2 are those of the plain launch
        ws = ops.fused_bwd_workspace(B, N, H, D, F32, DEV)
        ws.fill_(float("nan"))
        o, lse = ops.mqa_fwd(qkv, B, N, H, D, BF16, c.scale, zero_dq=ws)
        assert (ws[:B * N * H * D] == 0).all() and torch.equal(o, outs[BF16])
        ck = Exact("mqa_fwd_zdq", BF16, **where)
        ck.value("o", o, ref["o"]); ck.lse(lse, ref["lse2"]); ck.done()
        # osuf_rope_cast: the rotated operands come back exactly
        for dt in DTYPES:
            got = ops.rope_cast(strided(raw, dt), cosd, sind, N, H + 1, H + 2, D)
            ck = Exact("rope_cast", dt, **where)
            ck.value("qkv", got, rot); ck.done()
        # osuf_rope_cast_qs -> mqa_fwd(qs): the reference takes the queries as the kernel rounded them, scores are exponents (scale = ln 2)
        qr = ops.rope_cast(strided(raw, F32), cosd, sind, N, H + 1, H + 2, D, q_mul=cq, n_q_heads=H)
        want = rot.clone()
        want[..., :H * D] = (rot[..., :H * D].float() * cq).double()
        ck = Exact("rope_cast_qs", BF16, **where)
        ck.value("q", qr[..., :H * D], want[..., :H * D]); ck.value("kv", qr[..., H * D:], rot[..., H * D:]); ck.done()
        qeff = R.heads(qr[..., :H * D].cpu().double(), D)
        refq = ref_rows(R.attention_fp64(qeff, c.k, c.v, None, R.LN2))
        for dt in DTYPES:
            o, lse = ops.mqa_fwd(strided(qr), B, N, H, D, dt, c.scale, qs=True)
            ck = Exact("mqa_fwd_qs", dt, **where)
            ck.finite(o=o, lse=lse); ck.value("o", o, refq["o"]); ck.lse(lse, refq["lse2"]); ck.done()
        if N == 64 and kind == "tie":                                   # the override-gated fall-backs of the launcher: one case each
            for knob, qs_ in (("attn_fwd_nowhole", False), ("attn_fwd_noqsk", True)):
                with ops.force(**{knob: True}):
                    o, lse = ops.mqa_fwd(strided(qr) if qs_ else qkv, B, N, H, D, BF16, c.scale, qs=qs_)
                ck = Exact("mqa_fwd_" + knob.rsplit("_", 1)[1], BF16, **where)
                ck.value("o", o, (refq if qs_ else ref)["o"]); ck.lse(lse, (refq if qs_ else ref)["lse2"]); ck.done()
        # osuf_mqa_fwd_rope: un-rotated bf16 projections in, the kernel rotates / scales / rounds its queries
        for write_q in (True, False):
            for dt in DTYPES:
                ws.fill_(float("nan"))
                q_out, o, lse = ops.mqa_fwd_rope(strided(raw), cosd, sind, B, N, H, D, dt, c.scale, write_q=write_q, zero_dq=ws if write_q else None)
                ck = Exact("mqa_fwd_rope" + ("" if write_q else "_noq"), dt, **where)
                ck.finite(o=o, lse=lse); ck.value("o", o, refq["o"]); ck.lse(lse, refq["lse2"])
                ck.value("kv", q_out[..., H * D:], rot[..., H * D:])
                if write_q:
                    assert torch.equal(q_out[..., :H * D], qr[..., :H * D]) and (ws[:B * N * H * D] == 0).all()
                ck.done()


@pytest.mark.parametrize("G", [2, 3])
@pytest.mark.parametrize("D", R.HEAD_DIMS)
@pytest.mark.parametrize("N", R.LENGTHS)
def test_gqa_fwd(N, D, G):
    """osuf_gqa_fwd (GROUPS: the tuned kernel at head dim 64, the generic one elsewhere) and the per-group launches of mqa_fwd(kv_heads=G)."""
    B, H = 2, 2 * G
    for kind, shift in kinds_for(N, R.SHIFT_FWD):
        c = R.make_case(kind, B, N, N, H, G, D, shift=shift, seed=N + G)
        ref = ref_rows(R.attention_fp64(c.q, c.k, c.v, None, c.scale), G)
        qkv = strided(c.rows_qkv())
        for dt in DTYPES:
            for name, fn in (("gqa_fwd", ops.gqa_fwd), ("mqa_fwd_groups", ops.mqa_fwd)):
                o, lse = fn(qkv, B, N, H, D, dt, c.scale, kv_heads=G)
                ck = Exact(name, dt, N=N, D=D, G=G, kind=kind, shift=shift)
                ck.finite(o=o, lse=lse); ck.value("o", o, ref["o"]); ck.lse(lse, ref["lse2"]); ck.done()


@pytest.mark.parametrize("D", [16, 32, 128])
@pytest.mark.parametrize("N", R.LENGTHS)
def test_mqa_fwd_generic(N, D):
    """mqa_gen_fwd_kernel<DP 32 / 128> through ops.mqa_fwd."""
    B, H = (2, 3) if N == 65 else (2, 2)
    for kind, shift in kinds_for(N, R.SHIFT_FWD):
        c = R.make_case(kind, B, N, N, H, 1, D, shift=shift, seed=N)
        ref = ref_rows(R.attention_fp64(c.q, c.k, c.v, None, c.scale))
        qkv = strided(c.rows_qkv())
        for dt in DTYPES:
            o, lse = ops.mqa_fwd(qkv, B, N, H, D, dt, c.scale)
            ck = Exact("mqa_fwd_gen", dt, N=N, D=D, kind=kind, shift=shift)
            ck.finite(o=o, lse=lse); ck.value("o", o, ref["o"]); ck.lse(lse, ref["lse2"]); ck.done()


# ---- backward, head dim 64 ----------------------------------------------------------------------------------------------------
def _bwd_expect(c, ref, cos, sin, qscale=1.0):
    """gradient rows [B][N][(H + 2G) D] of the rotated operands and of the un-rotated ones (the RoPE transpose on dq / dk)"""
    dq = ref["dq"] * qscale
    plain = torch.cat([R.rows(dq), R.rows(ref["dk"]), R.rows(ref["dv"])], -1)
    unrot = torch.cat([R.rows(R.rope(dq, cos, sin, True)), R.rows(R.rope(ref["dk"], cos, sin, True)), R.rows(ref["dv"])], -1)
    return plain, unrot


def _check_bwd(ck, dqkv, want, c, H, G, D, zero_qk):
    zs = c.zero_scale * c.s
    ck.finite(dqkv=dqkv)
    ck.grad("dq", dqkv[..., :H * D], want[..., :H * D], zero_qk, zs)
    ck.grad("dk", dqkv[..., H * D:(H + G) * D], want[..., H * D:(H + G) * D], zero_qk, zs)
    ck.value("dv", dqkv[..., (H + G) * D:], want[..., (H + G) * D:])


@pytest.mark.parametrize("N", sorted(set(R.LENGTHS) | set(R.LENGTHS_512)))
def test_mqa_bwd_64(N):
    """Every head-dim-64 backward kernel (the variants of test_every_attention_backward_kernel_vs_fp32_autograd), fp32 and bf16 gradients, with
    and without the fused RoPE transpose, the fused sweeps also on pre-scaled queries.  o, lse2 are the reference's, delta the kernel's own."""
    D = 64
    B, H = shape_for(N)
    cos, sin = R.quarter_tables(N, D)
    cosd, sind = cos.to(DEV), sin.to(DEV)
    cq = float(torch.tensor(D ** -0.5, dtype=F32) * torch.tensor(R.LOG2E, dtype=F32))
    kinds = kinds_for(N, R.SHIFT_BWD)
    if N in (256, 2048):                                                # + one whole length per sweep (256-key / 512-key)
        kinds += [("selector", -1), ("tie", -1)]
    for kind, shift in kinds:
        c = R.make_case(kind, B, N, N, H, 1, D, shift=shift, seed=N)
        ref = R.attention_fp64(c.q, c.k, c.v, c.do, c.scale)
        rot = c.rows_qkv()
        qr = rot.clone()
        qr[..., :H * D] = (rot[..., :H * D].float() * cq).to(BF16).double()
        refq = R.attention_fp64(R.heads(qr[..., :H * D], D), c.k, c.v, c.do, R.LN2)
        want = {False: _bwd_expect(c, ref, cos, sin), True: _bwd_expect(c, refq, cos, sin, c.scale / R.LN2)}
        ops_in = {False: (strided(rot), ref), True: (strided(qr), refq)}
        do = strided(R.rows(c.do))
        zero_qk = kind == "selector"
        for name, variant, qsplit in R.bwd_cases(ops, N, ragged512_ok=False):
            for qs in (False, True) if variant in ops._FUSED_DQ_MODE else (False,):
                qkv, rf = ops_in[qs]
                for odt in DTYPES:                                      # the forward's o in both storage types feeds osuf_attn_delta
                    o = strided(R.rows(rf["o"]), odt)
                    lse = rf["lse2"].float().to(DEV)
                    for rope in (False, True):
                        dqkv = ops.mqa_bwd(qkv, o, do, lse, B, N, H, D, c.scale, odt, cosd if rope else None, sind if rope else None,
                                           variant=variant, qsplit=qsplit, qs=qs)
                        ck = Exact("mqa_bwd/" + name + ("/qs" if qs else "") + ("/rope" if rope else ""), odt, N=N, B=B, H=H, kind=kind, shift=shift)
                        _check_bwd(ck, dqkv, want[qs][rope], c, H, 1, D, zero_qk)
                        ck.done()


@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("D", [16, 32, 128])
@pytest.mark.parametrize("N", R.LENGTHS)
def test_mqa_bwd_generic(N, D, G):
    """mqa_gen_bwd_dq_kernel + mqa_gen_bwd_dkv_kernel through ops.mqa_bwd (per-group launches for G = 2), and osuf_rope_bwd behind them."""
    B, H = 2, 2 * G
    cos, sin = R.quarter_tables(N, D)
    for kind, shift in kinds_for(N, R.SHIFT_BWD + [64]):
        c = R.make_case(kind, B, N, N, H, G, D, shift=shift, seed=N + G)
        ref = R.attention_fp64(c.q, c.k, c.v, c.do, c.scale)
        want = _bwd_expect(c, ref, cos, sin)
        qkv, do = strided(c.rows_qkv()), strided(R.rows(c.do))
        lse = lse_layout(ref["lse2"], G).float().to(DEV)
        for odt in DTYPES:
            o = strided(R.rows(ref["o"]), odt)
            for rope in (False, True):
                dqkv = ops.mqa_bwd(qkv, o, do, lse, B, N, H, D, c.scale, odt, cos.to(DEV) if rope else None, sin.to(DEV) if rope else None, kv_heads=G)
                ck = Exact("mqa_bwd_gen" + ("/rope" if rope else ""), odt, N=N, D=D, G=G, kind=kind, shift=shift)
                _check_bwd(ck, dqkv, want[rope], c, H, G, D, kind == "selector")
                ck.done()


# ---- Attend's generic path: cross lengths, masks ---------------------------------------------------------------------------------
def _xattn(ck_name, c, bias, where, want_dbias):
    B, H, Nq, Nk, D = c.B, c.H, c.Nq, c.Nk, c.D
    ref = R.attention_fp64(c.q, c.k, c.v, c.do, c.scale, bias)
    q, k, v, do = strided(R.rows(c.q)), strided(R.rows(c.k)), strided(R.rows(c.v)), strided(R.rows(c.do))
    m4 = None if bias is None else bias.to(BF16).to(DEV).expand(B, H, Nq, Nk)             # broadcast dims keep stride 0
    sel = c.kind == "selector"
    q_zero = bool((c.q == 0).all())                                    # the bias-only cases: dK = dS^T q is exactly zero
    for dt in DTYPES:
        o, lse = X.xattn_fwd(q, k, v, m4, B, Nq, Nk, H, D, dt, c.scale)
        ck = Exact(ck_name + "_fwd", dt, **where)
        ck.finite(o=o, lse=lse); ck.value("o", o, R.rows(ref["o"])); ck.lse(lse, ref["lse2"]); ck.done()
        dq, dk, dv, db = X.xattn_bwd(q, k, v, m4, strided(R.rows(ref["o"]), dt), do, ref["lse2"].float().to(DEV), B, Nq, Nk, H, D, c.scale, want_dbias)
        ck = Exact(ck_name + "_bwd", dt, **where)
        ck.finite(dq=dq, dk=dk, dv=dv)
        zs = c.zero_scale * c.s
        ck.grad("dq", dq, R.rows(ref["dq"]), sel, zs)
        ck.grad("dk", dk, R.rows(ref["dk"]), sel or q_zero, zs)
        ck.value("dv", dv, R.rows(ref["dv"]))
        if want_dbias:
            ck.finite(dbias=db)
            ck.grad("dbias", db, ref["dbias"], sel, c.zero_scale)
        ck.done()


@pytest.mark.parametrize("D", R.HEAD_DIMS)
@pytest.mark.parametrize("Nq,Nk", R.CROSS_LENGTHS + [(200, 200)])
def test_xattn_unmasked(Nq, Nk, D):
    """mqa_gen_fwd / bwd kernels without a mask (head dim 64 included), keys and queries of their own lengths, shifted rows at every length."""
    for kind in ("selector",) + (("tie",) if Nk >= 2 else ()):
        for shift in (0, -1, 1):
            c = R.make_case(kind, 2, Nq, Nk, 2, 1, D, shift=shift, seed=Nq + Nk)
            _xattn("xattn", c, None, dict(Nq=Nq, Nk=Nk, D=D, kind=kind, shift=shift), False)


@pytest.mark.parametrize("form", R.BIAS_FORMS)
@pytest.mark.parametrize("D", R.HEAD_DIMS)
@pytest.mark.parametrize("Nq,Nk", R.CROSS_LENGTHS)
def test_xattn_masked(Nq, Nk, D, form):
    """The masked kernels: the bias alone selects (q = 0), through every stride pattern of the ABI, with dbias; and a bias on top of the
    selector / tie scores (all zero: the strides and the clamped reads of padded keys must not change anything)."""
    for kind in ("selector",) + (("tie", "bool") if Nk >= 2 else ()):
        c = R.make_bias_case(kind, 2, Nq, Nk, 3, D, form, seed=Nq)
        _xattn("xattn_masked", c, c.bias, dict(Nq=Nq, Nk=Nk, D=D, kind=kind, form=form), True)
    if form == "bhk" and Nk >= 2:
        for shift in (0, -1):
            c = R.make_case("tie", 2, Nq, Nk, 3, 1, D, shift=shift, seed=Nq)
            _xattn("xattn_masked", c, torch.zeros(2, 3, 1, Nk, dtype=F64), dict(Nq=Nq, Nk=Nk, D=D, kind="tie+0", form=form, shift=shift), True)


# ---- the elementwise companions -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [64, 32])
@pytest.mark.parametrize("odt", DTYPES, ids=["f32", "bf16"])
def test_attn_delta(D, odt):
    """osuf_attn_delta (both kernels, both o storage types) against sum_d dO O on integers: every (batch, head, row) has its own value."""
    B, H, N = 3, 5, 77
    gen = torch.Generator().manual_seed(11 + D)
    do = torch.randint(-3, 4, (B, N, H * D), generator=gen).to(F64)
    o = torch.randint(-7, 8, (B, N, H * D), generator=gen).to(F64)
    delta = torch.full((B, H, N), float("nan"), device=DEV)
    dod, od = strided(do), strided(o, odt)
    ops.call("osuf_attn_delta", dod.data_ptr(), dod.stride(1), od.data_ptr(), od.stride(1), ops._DT[odt], delta.data_ptr(), B, H, N, D, ops._stream())
    want = (do * o).view(B, N, H, D).sum(-1).permute(0, 2, 1)
    ck = Exact("attn_delta", odt, D=D)
    ck.value("delta", delta, want); ck.done()


@pytest.mark.parametrize("D", R.HEAD_DIMS)
@pytest.mark.parametrize("odt", DTYPES, ids=["f32", "bf16"])
def test_rope_bwd(D, odt):
    """osuf_rope_bwd (head dim 64 and the generic kernel): the transposed quarter turn of integer gradients, the v heads untouched."""
    B, N, nh = 2, 131, 5
    cos, sin = R.quarter_tables(N, D)
    g = torch.randint(-100, 101, (B, N, nh * D), generator=torch.Generator().manual_seed(12 + D)).to(F64)
    got = ops.rope_bwd(strided(g, F32), odt, cos.to(DEV), sin.to(DEV), N, 3, nh, D)
    want = torch.cat([R.rows(R.rope(R.heads(g[..., :3 * D], D), cos, sin, True)), g[..., 3 * D:]], -1)
    ck = Exact("rope_bwd", odt, D=D)
    ck.value("g", got, want); ck.done()


@pytest.mark.parametrize("D", [16, 32, 128])
@pytest.mark.parametrize("idt", DTYPES, ids=["f32", "bf16"])
def test_rope_cast_generic(D, idt):
    """osuf_rope_cast at the generic head dims (rope_gen_kernel, forward direction): the quarter turn of integer rows, the v heads copied."""
    B, N, nh = 2, 131, 5
    cos, sin = R.quarter_tables(N, D)
    x = torch.randint(-100, 101, (B, N, nh * D), generator=torch.Generator().manual_seed(13 + D)).to(F64)
    got = ops.rope_cast(strided(x, idt), cos.to(DEV), sin.to(DEV), N, 3, nh, D)
    want = torch.cat([R.rows(R.rope(R.heads(x[..., :3 * D], D), cos, sin)), x[..., 3 * D:]], -1)
    ck = Exact("rope_cast_gen", idt, D=D)
    ck.value("x", got, want); ck.done()
