"""The references of tests/dit_rows_reference.py against fp64 autograd of their forwards and independent restatements, the branch each
case-table entry names (from the launcher arithmetic of csrc/dit.hip restated there), the contract table against the source's checks, and
the guard of the caps tests/test_dit_rows_gpu.py uses (CPU only).

The GPU file measures the DiT row kernels against these functions, so a slip in one of them would either hide a kernel bug or report one
that is not there."""
from pathlib import Path

import pytest
import torch

from tests import dit_rows_reference as R
from tests.bound_check import FLOOR
from tests.test_poisoned_memory import relmax, rell2

TOL = 1e-12                                                # fp64 against fp64
F32, F64 = torch.float32, torch.float64
ID0 = lambda v: v[0] if isinstance(v, tuple) else None
SRC = (Path(__file__).resolve().parent.parent / "osufusion_amd" / "csrc" / "dit.hip").read_text()


def dbl(t):
    return None if t is None else t.double()


# ---------------------------------------------------------------------------------------------------------------------------------
# backwards against autograd, forwards against torch's own operators
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["a", "b"])
@pytest.mark.parametrize("C,L", [(8, 1), (520, 5), (1032, 7)])
def test_adaln_backward_equals_autograd(C, L, kind):
    B = 3
    inp = R.adaln_inputs("cpu", B, L, C, "f32", kind)
    x, sh, sc = (inp[k].double().requires_grad_() for k in ("x", "shift", "scale"))
    out, mean, rstd = R.adaln_fwd(x, sh, sc, L)
    ln = torch.nn.functional.layer_norm(x, (C,), eps=R.LN_EPS).view(B, L, C)
    assert relmax(out.detach(), (ln * (1 + sc[:, None]) + sh[:, None]).reshape(B * L, C).detach()) < TOL
    out.backward(inp["dy"].double())
    for dres in (None, inp["dres"].double()):
        dx, dsh, dsc = R.adaln_bwd(inp["dy"].double(), x.detach(), mean.detach(), rstd.detach(), sc.detach(), L, dres)
        assert rell2(dx, x.grad + (0 if dres is None else dres)) < TOL
        assert rell2(dsh, sh.grad) < TOL and rell2(dsc, sc.grad) < TOL


def _qknorm_autograd(x, gq, gk, H, G, D):
    """F.normalize semantics (clamp_min: zero gradient through a clamped norm), natural order."""
    M, QK = x.shape[0], (H + G) * D
    h = x[:, :QK].reshape(M, H + G, D)
    n = torch.linalg.vector_norm(h, dim=-1, keepdim=True).clamp_min(1e-12)
    qk = h / n * torch.cat([gq, gk], 0) * D ** 0.5
    return torch.cat([qk.reshape(M, QK), x[:, QK:]], 1)


def _group_major(H, G):
    perm = [0] * H
    for j in range(H):
        perm[(j % G) * (H // G) + j // G] = j
    return perm


@pytest.mark.parametrize("H,G,D", [(6, 2, 16), (8, 4, 64), (4, 4, 32), (2, 1, 128)])
def test_qknorm_backward_equals_autograd(H, G, D):
    B, Ns = 2, 12
    inp = R.joint_inputs("cpu", B, Ns, 17, H, G, D, "f32", True)
    x, gq, gk = (inp[k].double().requires_grad_() for k in ("x", "gq", "gk"))
    W, M = (H + 2 * G) * D, B * Ns
    nat = _qknorm_autograd(x, gq, gk, H, G, D)
    # the joint layout, restated: "b h n d -> b (r h) n d" makes natural query head j = r G + g read K/V head g: blocks ordered (g, r)
    q = nat[:, :H * D].reshape(M, H // G, G, D).transpose(1, 2).reshape(M, H * D)
    want = torch.cat([q, nat[:, H * D:]], 1)
    got, inv = R.qknorm_fwd(x.detach(), gq.detach(), gk.detach(), H, G, D)
    assert torch.equal(q.detach(), nat.detach()[:, :H * D].reshape(M, H, D)[:, _group_major(H, G)].reshape(M, H * D))
    assert relmax(got, want.detach()) < TOL
    g = inp["g"].double()[R.joint_rows(B, Ns, 17, 5)]
    want.backward(g)
    dx, dgamma = R.qknorm_bwd(g, x.detach(), inv, gq.detach(), gk.detach(), H, G, D)
    masks = R.special_mask(B, Ns, H, G, D, inp["specials"])
    special = masks["zero"] | masks["tiny"] | masks["near"]
    for name, m in (("regular", ~special), ("clamped", masks["zero"] | masks["tiny"]), ("near", masks["near"])):
        assert m.any() and rell2(dx[m], x.grad[m]) < TOL, name
    assert rell2(dgamma, torch.cat([gq.grad, gk.grad], 0)) < TOL
    # the three kinds take the branch they are there for; the tiny heads give dgamma a non-zero term
    n = (x.detach()[:, :(H + G) * D].reshape(M, H + G, D) ** 2).sum(-1).sqrt()
    for b, r, head, kind in inp["specials"]:
        nn = n[b * Ns + r, head].item()
        assert (nn == 0) if kind == "zero" else (0 < nn < 1e-12) if kind == "tiny" else (1e-12 < nn < 1e-10), (kind, nn)
    assert {k for *_, k in inp["specials"]} == set(R.SPECIAL_KINDS) and {h < H for _, _, h, _ in inp["specials"]} == {True, False}
    u_tiny = (x.detach() * 1e12)[masks["tiny"]]
    assert (u_tiny != 0).all() and (g[masks["tiny"][:, R.joint_cols(H, G, D, H + 2 * G).argsort()]] != 0).any()
    # cast-only mode: the permutation alone, in both directions
    y0, inv0 = R.qknorm_fwd(x.detach(), None, None, H, G, D)
    assert inv0 is None and torch.equal(y0[:, R.joint_cols(H, G, D, H + 2 * G)], x.detach())
    dx0, dg0 = R.qknorm_bwd(g, None, None, None, None, H, G, D)
    assert dg0 is None and torch.equal(dx0, g[:, R.joint_cols(H, G, D, H + 2 * G)])


def test_special_values_survive_bf16_and_fp32_squares():
    for v in R.SPECIAL_KINDS.values():
        t = torch.tensor([v], dtype=F32)
        assert R.stored(t, torch.bfloat16).item() == v and (t * t).item() == v * v       # 2^-100 and 2^-78 are normal fp32 numbers


@pytest.mark.parametrize("case", R.PERM, ids=ID0)
def test_pack_equals_the_reference_rearrangement(case):
    cid, B, Ns, Nj, off, H, G, D, lds, ldj, branch = case
    M = min(B * Ns, 40)
    rows = R.rnd(f"pk.{cid}", (M, H * D))
    want = rows.view(M, H // G, G, D).transpose(1, 2).reshape(M, H * D)
    assert torch.equal(R.pack(rows, H, G, D), want) and torch.equal(R.unpack(want, H, G, D), rows)
    jr = R.joint_rows(B, Ns, Nj, off).view(B, Ns)
    assert all(torch.equal(jr[b], torch.arange(b * Nj + off, b * Nj + off + Ns)) for b in range(B))
    assert branch in R.perm_branches(B, Ns, H, D)


def test_pack_table_has_a_real_permutation_and_the_cap():
    assert {c[-1] for c in R.PERM} == {"one_pass", "ew_grid_cap"}
    assert sum(_group_major(H, G) != list(range(H)) for _, _, _, _, _, H, G, *_ in R.PERM) >= 3
    cid, B, Ns, Nj, off, H, G, D, *_ = R.PERM[-1]
    assert (B * Ns, H, D) == (16400, 2, 128) and B * Ns * (H * D // 8) > R.GRID_CAP and R.ew_grid(B * Ns * (H * D // 8)) == 2048
    assert any(lds > H * D and ldj > H * D and lds != ldj for _, _, _, _, _, H, G, D, lds, ldj, _ in R.PERM)


@pytest.mark.parametrize("kind", R.STAT_KINDS)
def test_stat_pool_equals_torch(kind):
    for L in R.STAT_L:
        a = R.stat_input(kind, R.STAT_B, 96, L).double()
        assert relmax(R.stat_pool(a), torch.cat([a.mean(-1), a.std(-1)], 1)) < TOL
    # the offset input shows a one-pass variance: E[x^2] - mean^2 in fp32 keeps no digit of a 1e-4 variance beside 1e6
    a = R.stat_input("offset", R.STAT_B, 96, 1000)
    one_pass = ((a * a).sum(-1) / 1000 - (a.sum(-1) / 1000) ** 2).clamp_min(0) * (1000 / 999)
    want = R.stat_pool(a.double())
    assert relmax(torch.cat([a.sum(-1) / 1000, one_pass.sqrt()], 1), want) > 10 * R.STAT_CAP
    assert R.STAT_L == [2, 255, 256, 257, 1000] and R.STAT_C == [1, 96]                # both sides of the 256-thread stride


# ---------------------------------------------------------------------------------------------------------------------------------
# the launcher arithmetic is the source's, and each table reaches what it names
# ---------------------------------------------------------------------------------------------------------------------------------
def test_launcher_arithmetic_is_the_sources():
    for text in ("const int j = (chunks + 63) / 64; return j <= 1 ? 1 : j <= 2 ? 2 : j <= 4 ? 4 : j <= 8 ? 8 : 0;",
                 "int nblk = (L + 15) / 16;", "const int cap = 2048 / B > 1 ? 2048 / B : 1;", "return nblk < cap ? nblk : cap;",
                 "long b = ((long)M + 15) / 16; return (int)(b < 1024 ? b : 1024);", "long blocks = ((long)M + 3) / 4;",
                 "if (blocks > 4096) blocks = 4096;", "static constexpr int kFinCols = 64, kFinSlices = 16;",
                 "for (long n = 4L * k + wv; n < L; n += 4L * nblk)", "const int grid = ew_grid((long)M * (H * D / 8));",
                 "const size_t lds = (size_t)8 * C * sizeof(float);"):
        assert text in SRC, text
    common = (Path(__file__).resolve().parent.parent / "osufusion_amd" / "csrc" / "common.hpp").read_text()
    assert "if (blocks > 2048) blocks = 2048;" in common and R.GRID_CAP == 2048 * 256
    assert [R.chunk_iters(c) for c in (1, 64, 65, 128, 129, 256, 257, 512, 513)] == [1, 1, 2, 2, 4, 4, 8, 8, 0]
    assert (R.adaln_bwd_blocks(2, 67), R.adaln_bwd_blocks(256, 200), R.adaln_bwd_blocks(65535, 1), R.adaln_bwd_blocks(2, 300)) == (5, 8, 1, 19)
    assert (R.qknorm_bwd_blocks(24), R.qknorm_bwd_blocks(16400)) == (2, 1024) and R.fwd_trips(16384) == 1 and R.fwd_trips(16400) == 2


def test_adaln_table_reaches_its_branches():
    reached, ids = set(), set()
    for cid, B, L, C, strides, dirs, named in R.ADALN:
        got = R.adaln_branches(B, L, C, strides, dirs)
        assert set(named) <= got, (cid, named, got)
        reached |= got
        ids.add(cid)
        assert 8 * C * 4 <= 65536 and B <= 65535                                        # the backward's dynamic LDS, grid.y
        if strides:
            lds = [strides[k] for k in ("ldx", "ldo", "lddy", "ldr", "lddx")]
            assert len(set(lds)) == 5 and min(lds) > C and all(v % 8 == 0 for v in lds) and strides["ldm"] > C and strides["ldm"] % 4 == 0
            lo, hi = sorted((0, strides["off2"]))
            assert hi - lo >= C and hi + C <= strides["ldd"] + (strides["off2"] < 0) * hi   # the two blocks do not overlap, and fit a row
    assert len(ids) == len(R.ADALN) and R.ADALN_NAMED <= reached, R.ADALN_NAMED - reached
    by = {cid: R.adaln_branches(B, L, C, s, d) for cid, B, L, C, s, d, _ in R.ADALN}
    # J = 1, 2, 4, each with a full and a one-lane last pass
    for C, J, lanes in ((8, 1, "1"), (512, 1, "full"), (520, 2, "1"), (1024, 2, "full"), (1032, 4, "1"), (2048, 4, "full"), (504, 1, "63")):
        assert {f"J={J}", f"last_pass={lanes}"} <= by[f"C{C}_L5"], C
    assert {C for _, _, _, C, *_ in R.ADALN[:21]} == {8, 504, 512, 520, 1024, 1032, 2048} and {L for _, _, L, *_ in R.ADALN[:21]} == {1, 5, 67}
    assert 8 * 2048 * 4 == 65536                                                        # C = 2048: exactly the default dynamic-LDS limit
    assert "fwd_grid_cap" in by["fwd_stride"] and R.fwd_trips(4 * 4100) == 2 and 4 * 4100 == 16400
    assert {"bwd_cap", "bwd_trips=7", "finish:nblk<16"} <= by["bwd_cap"] and R.adaln_bwd_blocks(256, 200) == 8
    assert "grid.y=65535" in by["grid_y"] and "bwd_cap" not in by["grid_y"]
    assert "finish:nblk%16!=0" in by["L300"] and "finish:nblk<16" in by["C8_L67"]
    assert "off2<0" in by["off2_neg"] and "strided" in by["strided_520"] and "strided" in by["strided_1032"]


def test_joint_table_reaches_its_branches():
    reached = set()
    by = {}
    for cid, B, Ns, Nj, off, H, G, D, strided, sp, dirs, named in R.JOINT:
        got = R.joint_branches(B, Ns, Nj, off, H, G, D, strided, dirs)
        assert set(named) <= got, (cid, named, got)
        assert off + Ns <= Nj and H % G == 0 and (H + 2 * G) * D <= 4096 and 4 * (H + G) * D * 4 <= 65536
        assert not sp or Ns >= 7                                                        # the six special heads sit in rows of their own
        reached |= got
        by[cid] = got
    assert R.JOINT_NAMED <= reached, R.JOINT_NAMED - reached
    for J in (1, 2, 4, 8):
        assert any({f"J={J}", "joint"} <= b for b in by.values()), J
    for J in (2, 8):
        assert any({f"J={J}", "identity"} <= b for b in by.values()), J
    assert {"J=8", "joint", "width=4096", "last_pass=full"} <= by["j8f_x"] and {"J=8", "joint"} <= by["j8p_x"] and "width=4096" not in by["j8p_x"]
    assert {"fwd_grid_cap", "bwd_cap", "finish:nblk=1024", "joint", "J=1"} <= by["big"]
    assert not any(3 * H * D == 4096 for H in range(1, 257) for D in (16, 32, 64, 128))  # G = H never gives a 4096-wide row: id_j8 is 4080
    # a query head's permuted chunk lands in another 64-chunk pass than its source: J = 2 and J = 8, joint mode
    for cid in ("j2c_x", "j4_x", "j8p_x", "j8f_x"):
        _, B, Ns, Nj, off, H, G, D, *_ = next(c for c in R.JOINT if c[0] == cid)
        src = torch.arange(H * D)
        assert ((R.joint_cols(H, G, D, H) // 512) != (src // 512)).any(), cid


# ---------------------------------------------------------------------------------------------------------------------------------
# eps is visible in kind b; the derived term of kinds c and d
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [8, 504, 512, 520, 1024, 1032, 2048])
def test_eps_sensitive_rows(C):
    B, L = 2, 5
    inp = R.adaln_inputs(f"C{C}_L{L}", B, L, C, "bf16", "b")
    x = inp["x"]
    assert torch.equal(R.stored(x, torch.bfloat16), x) and (x.sum(-1) == 0).all() and ((x * x).sum(-1) / C == 2.0 ** -20).all()
    r64 = R.adaln_fwd(x.double(), inp["shift"].double(), inp["scale"].double(), L)[0]
    wrong = R.adaln_fwd(x.double(), inp["shift"].double(), inp["scale"].double(), L, eps=1e-5)[0]
    none = R.adaln_fwd(x.double(), inp["shift"].double(), inp["scale"].double(), L, eps=0.0)[0]
    r32 = R.adaln_fwd(x, inp["shift"], inp["scale"], L)[0]
    print(C, relmax(wrong, r64), relmax(none, r64), relmax(r32, r64))
    assert relmax(wrong, r64) > 0.3 and relmax(none, r64) > 0.1 and relmax(r32, r64) < 2e-7
    # kind a hides both
    xa = R.adaln_inputs(f"C{C}_L{L}", B, L, C, "f32", "a")["x"].double()
    assert relmax(R.adaln_fwd(xa, inp["shift"].double(), inp["scale"].double(), L, eps=1e-5)[0], R.adaln_fwd(xa, inp["shift"].double(), inp["scale"].double(), L)[0]) < 1e-5


def test_offset_rows_and_their_extra():
    for C in (504, 520, 2048):
        for kind in ("c", "d"):
            inp = R.adaln_inputs("cpu.off", 2, 5, C, "f32", kind)
            x = inp["x"]
            assert (x.sum(-1) == C * R.OFFSET[kind]).all()                              # the row sums are exact in fp32
            r64 = R.adaln_fwd(x.double(), inp["shift"].double(), inp["scale"].double(), 5)
            extra = R.adaln_extra(kind, inp["scale"], r64[0])
            assert 1e-5 < extra < 2e-3
            if kind == "d":
                assert relmax(r64[0], inp["shift"].double().repeat_interleave(5, 0)) == 0 and (r64[2] - 1 / R.LN_EPS ** 0.5).abs().max() < 1e-9
            # an output formed with a mean that is off by 2^-23 of the offset stays inside it
            b = torch.arange(10) // 5
            moved = (x.double() - R.OFFSET[kind] * (1 + 2.0 ** -23)) * r64[2][:, None] * (1 + inp["scale"].double()[b]) + inp["shift"].double()[b]
            assert 0.05 * extra < relmax(moved, r64[0]) <= extra * (1 + 1e-9)
    assert R.adaln_extra("a", None, None) == 0.0 and R.adaln_extra("b", None, None) == 0.0


# ---------------------------------------------------------------------------------------------------------------------------------
# caps: 16 e32 <= cap for every bounded quantity of every case, so no cap is ever the active bound by accident
# ---------------------------------------------------------------------------------------------------------------------------------
def _guard(e32, cap, what, factor=16):
    print(what, f"e32 = {e32:.3g}", f"cap = {cap:.3g}")
    assert factor * e32 <= cap, (what, e32, cap)
    assert FLOOR <= cap


def _mr32(mean, rstd):
    return mean.to(F32), rstd.to(F32)


@pytest.mark.parametrize("case", R.ADALN, ids=ID0)
def test_caps_adaln(case):
    """16 e32 <= cap for every quantity but the forward's on kind a.  OUT_CAP = 2e-6 is 16 fp32 spacings at the largest output, and the
    fp32 evaluation of 2 randn + 0.5 rows is itself one to two spacings away (e32 = 1.3e-7 ... 2.7e-7 over the table), so 16 e32 cannot
    stay under it: there the cap -- what tests/test_dit_gpu.py already asks of out -- is the active bound on purpose, and the guard is
    e32 <= cap.  Kinds b, c and d (exact sums) keep 16 e32 <= cap (e32 <= 1.1e-7)."""
    cid, B, L, C, strides, dirs, named = case
    for dt in ("f32", "bf16"):
        for kind in R.ADALN_KINDS:
            if kind == "c" and dt == "bf16" or (dirs == "bwd" and kind != "a"):
                continue
            inp = R.adaln_inputs(cid, B, L, C, dt, kind)
            f64 = R.adaln_fwd(inp["x"].double(), inp["shift"].double(), inp["scale"].double(), L)
            f32 = R.adaln_fwd(inp["x"], inp["shift"], inp["scale"], L)
            assert all(t.dtype == F32 for t in f32)
            if dirs != "bwd":
                for key, a, b in zip(("out", "mean", "rstd"), f32, f64):
                    _guard(relmax(a, b), R.OUT_CAP, (cid, dt, kind, key), factor=1 if kind == "a" else 16)
            if dirs == "fwd" or kind != "a":
                continue
            mean, rstd = _mr32(f64[1], f64[2])
            for dres in (None, inp["dres"]):
                b64 = R.adaln_bwd(inp["dy"].double(), inp["x"].double(), mean.double(), rstd.double(), inp["scale"].double(), L, dbl(dres))
                b32 = R.adaln_bwd(inp["dy"], inp["x"], mean, rstd, inp["scale"], L, dres)
                _guard(relmax(b32[0], b64[0]), R.GRAD_CAP, (cid, dt, "dx", dres is not None))
                _guard(rell2(b32[1], b64[1]), R.GRAD_CAP, (cid, dt, "dshift"))
                _guard(rell2(b32[2], b64[2]), R.GRAD_CAP, (cid, dt, "dscale"))


@pytest.mark.parametrize("case", R.JOINT, ids=ID0)
def test_caps_joint(case):
    cid, B, Ns, Nj, off, H, G, D, strided, sp, dirs, named = case
    for dt in ("f32", "bf16"):
        inp = R.joint_inputs(cid, B, Ns, Nj, H, G, D, dt, sp)
        x, gq, gk = inp["x"], inp["gq"], inp["gk"]
        y64, inv64 = R.qknorm_fwd(x.double(), gq.double(), gk.double(), H, G, D)
        y32, inv32 = R.qknorm_fwd(x, gq, gk, H, G, D)
        masks = R.special_mask(B, Ns, H, G, D, inp["specials"])
        cols = R.joint_cols(H, G, D, H + 2 * G)
        groups = {"regular": ~(masks["zero"] | masks["tiny"] | masks["near"]), "clamped": masks["zero"] | masks["tiny"], "near": masks["near"]}
        for name, m in groups.items():
            if m.any():
                _guard(relmax(y32[:, cols][m], y64[:, cols][m]), R.Y_CAP, (cid, dt, "y", name))
        _guard(relmax(inv32, inv64), R.INV_CAP, (cid, dt, "inv"))
        g = inp["g"][R.joint_rows(B, Ns, Nj, off)]
        inv = inv64.to(F32)
        d64, dg64 = R.qknorm_bwd(g.double(), x.double(), inv.double(), gq.double(), gk.double(), H, G, D)
        d32, dg32 = R.qknorm_bwd(g, x, inv, gq, gk, H, G, D)
        for name, m in groups.items():
            if m.any():
                _guard(relmax(d32[m], d64[m]), R.GRAD_CAP, (cid, dt, "dx", name))
        _guard(rell2(dg32, dg64), R.GRAD_CAP, (cid, dt, "dgamma"))


@pytest.mark.parametrize("kind", R.STAT_KINDS)
def test_caps_stat_pool(kind):
    for C in R.STAT_C:
        for L in R.STAT_L:
            a = R.stat_input(kind, R.STAT_B, C, L)
            _guard(relmax(R.stat_pool(a), R.stat_pool(a.double())), R.STAT_CAP, ("stat_pool", kind, C, L))


# ---------------------------------------------------------------------------------------------------------------------------------
# contract table
# ---------------------------------------------------------------------------------------------------------------------------------
def test_contract_table_walks_every_clause():
    for text in R.DIT_CLAUSES:
        assert text in SRC, text
    assert {e for e, _, _ in R.DIT_BAD} == set(R.DIT_ENTRIES)
    for entry in R.DIT_ENTRIES:
        assert f" {entry}(" in SRC, entry
    per = lambda entry: {(k, tuple(sorted(o))) for e, k, o in R.DIT_BAD if e == entry}
    # the new adaLN refusals
    for a in ("x", "out", "shift", "scale"):
        assert ("null", (a,)) in per("osuf_adaln_fwd") and ("al16", (a,)) in per("osuf_adaln_fwd")
    for a in ("ldx", "ldo", "ldm"):
        assert ("ld < C", (a,)) in per("osuf_adaln_fwd")
    for a in ("dy", "x", "dx", "scale", "mr", "dmod", "workspace"):
        assert ("null", (a,)) in per("osuf_adaln_bwd")
    for a in ("lddy", "ldx", "ldr", "lddx", "ldm", "ldd"):
        assert ("ld < C", (a,)) in per("osuf_adaln_bwd")
    # no line may reach a launch: a bad stride stays a multiple of what its own clause asks only where it tests the other clause
    g = R.GOOD_ADALN
    for e, kind, over in R.DIT_BAD:
        assert over, (e, kind)
        if e.startswith("osuf_adaln") and kind == "ld < C":
            (a, v), = over.items()
            assert v < g["C"] and (v % 8 == 0 or a in ("ldm", "ldd")), (e, over)
        if e.startswith("osuf_adaln") and kind in ("ld % 8", "ld % 4"):
            (a, v), = over.items()
            assert v >= g["C"] and v % (8 if kind == "ld % 8" else 4), (e, over)
        assert R.bad_status(e, kind) == (0 if e.endswith("_workspace_bytes") else R.EUNSUPPORTED if kind == "dtype" else R.EINVAL)
    j = R.GOOD_JOINT
    W = (j["H"] + 2 * j["G"]) * j["D"]
    assert W == 160 and j["ld"] >= W and j["ld"] % 8 == 0 and j["ldp"] >= j["H"] * j["D"] and j["off"] + j["Ns"] <= j["Nj"]
    for e, kind, over in R.DIT_BAD:
        if kind == "ld < W":
            (a, v), = over.items()
            assert v < (j["H"] * j["D"] if e in ("osuf_joint_pack", "osuf_joint_unpack") else W) and v % 8 in (0, 4), (e, over)
