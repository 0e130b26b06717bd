"""The references of tests/elementwise_reference.py against independent restatements (torch's own bf16 conversion, unfold / permute,
torch.optim.AdamW in fp64, the oracle's DDIM algebra and masked loss), the branch each case-table entry names, the contract table, and the
guard of the caps tests/test_elementwise_rows_gpu.py uses (CPU only).

The GPU file measures the layout, loss, optimizer and DDPM / DDIM kernels against these functions, so a slip in one of them would either
hide a kernel bug or report one that is not there."""
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import diffusion_oracle as DO
from tests import elementwise_reference as E
from tests.bound_check import FLOOR
from tests.test_poisoned_memory import relmax

TOL = 1e-12                                                # fp64 against fp64
F32, F64 = torch.float32, torch.float64
ID0 = lambda v: v[0] if isinstance(v, tuple) else None


# ---------------------------------------------------------------------------------------------------------------------------------
# bits
# ---------------------------------------------------------------------------------------------------------------------------------
def test_rne_bf16_equals_torch_on_the_pattern_table():
    for bits in (E.pattern_table(), E.special_patterns()):
        want = E.bf16_bits(E.f32_from_bits(bits).to(torch.bfloat16))
        got = E.rne_bf16(bits)
        nan = E.bf16_is_nan(got)
        assert np.array_equal(nan, E.bf16_is_nan(want)) and np.array_equal(nan, np.isnan(E.f32_from_bits(bits).numpy()))
        assert np.array_equal(got[~nan], want[~nan])
    assert len(E.pattern_table()) == 393216 and 190 <= len(E.special_patterns()) <= 220


def test_rne_bf16_known_answers():
    r = lambda b: int(E.rne_bf16(np.array([b], dtype=np.uint32))[0])
    assert r(0x3F808000) == 0x3F80 and r(0x3F818000) == 0x3F82                          # ties: to the even neighbour, down and up
    assert r(0x3F807FFF) == 0x3F80 and r(0x3F808001) == 0x3F81
    assert r(0x7F7FFFFF) == 0x7F80 and r(0xFF7F8000) == 0xFF80 and r(0x7F7F7FFF) == 0x7F7F   # the largest finite values round to inf
    assert r(0x00000001) == 0x0000 and r(0x00008000) == 0x0000 and r(0x00018000) == 0x0002 and r(0x00008001) == 0x0001   # subnormals are kept
    assert r(0x007FFFFF) == 0x0080                                                      # the largest subnormal rounds to the smallest normal
    assert r(0x80000000) == 0x8000 and r(0x80000001) == 0x8000                          # -0 stays -0
    assert r(0x7F800000) == 0x7F80 and r(0xFF800000) == 0xFF80
    assert E.bf16_is_nan(E.rne_bf16(np.array([0x7F800001, 0x7FC00000, 0xFFFFFFFF, 0x7F80FFFF], dtype=np.uint32))).all()
    d = E.bits_differ(np.array([0x7FC0, 0x3F80, 0x3F81], dtype=np.uint16), np.array([0xFFC1, 0x3F80, 0x3F80], dtype=np.uint16), torch.bfloat16)
    assert d.tolist() == [False, False, True]


def test_special_patterns_cover_the_boundaries():
    s = E.special_patterns()
    exps = set(((s >> 23) & 0xFF).tolist())
    assert {0, 1, 254, 255} <= exps and len(E.SPECIAL_EXPONENTS) == 12
    for e in E.SPECIAL_EXPONENTS:
        lo = set((s[((s >> 23) & 0xFF) == e] & 0xFFFF).tolist())
        assert {0x7FFF, 0x8000, 0x8001, 0xFFFF} <= lo
        assert {0, 1} <= set(((s[((s >> 23) & 0xFF) == e] >> 16) & 1).tolist())          # an even and an odd last kept bit


# ---------------------------------------------------------------------------------------------------------------------------------
# moves
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", E.NCL, ids=ID0)
def test_ncl_to_rows_equals_unfold(case):
    cid, B, C, L, KT, width, ld, branch = case
    x = E.ncl_input(f"ncl.{cid}", B, C, L)
    got = E.ncl_to_rows(x, C, L, KT, width)
    lo = KT // 2
    xp = F.pad(x, (lo, KT - 1 - lo))                                                    # taps n - KT/2 .. n + KT - 1 - KT/2
    cols = xp.unfold(2, KT, 1)                                                          # (B, C, L, KT)
    want = torch.zeros(B, L, width)
    want[:, :, :C * KT] = cols.permute(0, 2, 3, 1).reshape(B, L, KT * C)                # column t * C + ci
    assert torch.equal(got, want.view(B * L, width))
    assert (got[:, C * KT:] == 0).all()


def test_ncl_to_rows_reads_no_neighbouring_sample():
    """In the edge cases every non-zero value of row (b, n) lies within 1 of 8 (b + 1)."""
    for cid, B, C, L, KT, width, ld, branch in E.NCL[:6]:
        got = E.ncl_to_rows(E.ncl_input(f"ncl.{cid}", B, C, L), C, L, KT, width).view(B, L, width)
        for b in range(B):
            nz = got[b][got[b] != 0]
            assert ((nz - 8.0 * (b + 1)).abs() < 1).all(), cid
        assert B >= 2 or cid == "c1"


@pytest.mark.parametrize("case", E.R2N, ids=ID0)
def test_rows_to_ncl_equals_permute(case):
    cid, B, C, L, ld, branch = case
    rows = E.rows_input(f"r2n.{cid}", B * L, ld, F32)
    assert torch.equal(E.rows_to_ncl(rows, B, C, L), rows.view(B, L, ld)[:, :, :C].permute(0, 2, 1).contiguous())


def test_copy_and_add():
    a, b = E.rows_input("a", 5, 40, F32), E.rows_input("b", 5, 32, F32)
    assert torch.equal(E.copy2d(a, 24), a[:, :24]) and torch.equal(E.add2d(a, b, 24), a[:, :24] + b[:, :24])
    h = E.rows_input("h", 5, 16, torch.bfloat16)
    assert torch.equal(E.round_bf16(h).to(F32), h)                                      # bf16 inputs are held exactly


def test_move_tables_name_their_branches():
    for table, fn, names in ((E.NCL, E.branches_ncl, E.NCL_BRANCHES), (E.R2N, E.branches_r2n, E.R2N_BRANCHES), (E.COPY, E.branches_copy, E.COPY_BRANCHES)):
        reached = set()
        for cid, *shape, branch in table:
            assert branch in fn(*shape), (cid, branch, fn(*shape))
            reached |= fn(*shape)
        assert names <= reached, names - reached
        assert names - {"padding", "ld>width"} <= {e[-1] for e in table}
    assert "padding" in E.branches_ncl(*E.NCL[1][1:7]) and 6 * 15 == 90                 # the stem: padding columns 90..95
    assert {e[-1] for e in E.ADD} == E.ADD_BRANCHES and len({E.ADD[0][3], E.ADD[0][4], E.ADD[0][5]}) == 3
    assert E.passes(E.GRID_CAP) == "one_pass" and E.passes(2 * E.GRID_CAP) == "one_pass" and E.passes(E.GRID_CAP + 1) == "second_pass"
    assert len(E.DT_PAIRS) == 4


# ---------------------------------------------------------------------------------------------------------------------------------
# loss, optimizer
# ---------------------------------------------------------------------------------------------------------------------------------
def test_mse_equals_the_oracle_loss_and_autograd():
    """oracle/diffusion_oracle.py:63-68: (loss * mask).sum() with mask = arange(n) < orig_len; the weights multiply a sample's share."""
    B, Dch, L = 3, 6, 50
    inp = E.mse_inputs("oracle", B, Dch, L, True, True)
    pred, target = inp["pred"].double().requires_grad_(), inp["target"].double()
    loss = (pred - target) ** 2
    mask = (torch.arange(L)[None, :] < inp["orig_len"][:, None]).to(loss.dtype)[:, None, :].expand(B, Dch, L)
    assert abs(E.mse(pred.detach(), target, inp["orig_len"])[0] - (loss * mask).sum()) < TOL * loss.sum()
    want = (loss * mask * inp["wt"].double()[:, None, None]).sum()
    want.backward()
    s, g = E.mse(pred.detach(), target, inp["orig_len"], inp["wt"])
    assert abs(s - want) < TOL * want.abs() and relmax(g, pred.grad) < TOL
    s, g = E.mse(pred.detach(), target)
    assert abs(s - loss.sum()) < TOL * loss.sum() and relmax(g, 2 * (pred.detach() - target)) < TOL


def test_mse_inputs_hold_every_kind_of_length_and_weight():
    for cid, B, Dch, L, branch in E.MSE:
        inp = E.mse_inputs(cid, B, Dch, L, True, True)
        lens, wts = inp["orig_len"].tolist(), inp["wt"].tolist()
        if B == 4:
            assert set(lens) == {0, L, L + 5, max(L // 3, 1)} and set(wts) == set(E.MSE_WT)
        assert {0.0, 1.0} <= set(E.MSE_WT) and min(E.MSE_WT) < 0 and max(E.MSE_WT) >= 1000
        assert wts[0] == 1000.0 and lens[0] > 0                                         # the sum is dominated by one sample: no cancellation
        assert branch in E.branches_mse(B, Dch, L)
    assert {e[-1] for e in E.MSE} == E.MSE_BRANCHES and sum(B == 4 for _, B, *_ in E.MSE) >= 2
    assert len(set(E.MSE_OPTS)) == 8


def test_adamw_equals_torch_optim_in_fp64():
    """Three steps from zero state against torch.optim.AdamW in fp64; the single-step-from-given-state form composes to the same numbers."""
    lr, b1, b2, eps = E.HYPER
    for wd in E.ADAMW_WD:
        n = 37
        p0 = E.uni("aw.cpu.p", (n,), 2.0).double()
        pt = p0.clone().requires_grad_()
        opt = torch.optim.AdamW([pt], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
        p, m, v = p0.clone(), torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64)
        for step in range(1, 4):
            g = E.uni(f"aw.cpu.g{step}", (n,)).double()
            pt.grad = g.clone()
            opt.step()
            p, m, v = E.adamw_step(p, g, m, v, (lr, b1, b2, eps, wd), step)
            assert relmax(p, pt.detach()) < TOL
            st = opt.state[pt]
            assert relmax(m, st["exp_avg"]) < TOL and relmax(v, st["exp_avg_sq"]) < TOL
    p2, m2, v2 = E.adamw_step(p0, g, m, v, (lr, b1, b2, eps, 0.0), 7, 0.25)
    p3, m3, v3 = E.adamw_step(p0, g * 0.25, m, v, (lr, b1, b2, eps, 0.0), 7)
    assert relmax(p2, p3) < TOL and relmax(m2, m3) < TOL and relmax(v2, v3) < TOL      # gscale multiplies the gradient
    assert all(float(np.float32(h)) == h for h in E.HYPER + tuple(E.ADAMW_WD))          # what the entry point receives


def test_flat_table_names_its_branches():
    reached = set()
    for n in E.FLAT_N:
        reached |= E.branches_flat(n)
    assert reached == E.FLAT_BRANCHES
    assert E.branches_flat(E.FLAT_N[-1]) == {"body+tail", "second_pass"} and E.FLAT_N[-1] < 2.2e6
    p, g, m, v = E.adamw_inputs(1027)
    z = slice(1, 1 + E.ZERO_BLOCK)
    assert (g[z] == 0).all() and (v[z] == 0).all() and (m[z] != 0).all() and (v >= 0).all()
    upd = (E.adamw_step(p.double(), g.double(), m.double(), v.double(), E.HYPER + (0.0,), 1000)[0] - p.double()).abs()
    assert upd[z].max() < 10 * upd.max() and upd[z].max() * 10 > upd.median()           # the zero block neither drowns the rest nor vanishes
    assert E.ADAMW_STEPS == [1, 2, 1000, 100000] and E.ADAMW_GSCALE == [None, 0.25, 1.0, 0.0] and E.ADAMW_WD[0] == 0.0


def test_clip_table():
    assert {c[-1] for c in E.CLIP} == E.CLIP_BRANCHES
    for sumsq, max_norm, base, branch in E.CLIP:
        c = E.clip_coef(sumsq, max_norm, base)
        if branch == "active":
            assert max_norm > 0 and sumsq ** 0.5 + 1e-6 > max_norm and c < base
            tn = torch.tensor([sumsq], dtype=F64).sqrt()                               # torch.nn.utils.clip_grad_norm_: clamp(max_norm / (norm + 1e-6), max=1)
            assert abs(c - float(torch.clamp(max_norm / (tn + 1e-6), max=1.0)) * base) < TOL
        else:
            assert c == base
            assert (branch == "off") == (max_norm <= 0) and (branch == "zero") == (sumsq == 0 and max_norm > 0)
        assert float(np.float32(base)) == base and float(np.float32(max_norm)) == max_norm


# ---------------------------------------------------------------------------------------------------------------------------------
# DDPM / DDIM algebra
# ---------------------------------------------------------------------------------------------------------------------------------
def test_axpby_and_ddim_equal_the_oracle():
    ts, per = (980, 500, 20, 0), 33
    acp = torch.cumprod(1 - torch.linspace(1e-4, 0.02, 1000, dtype=F64), 0)
    assert relmax(acp.float(), DO.ddim_alphas_cumprod()) < 1e-6
    coef = E.ddim_coef(ts)
    x, cond, null = (E.uni(f"or.{k}", (4, per), 1.5).double() for k in "xcn")
    for scale, nu in ((1.0, None), (2.0, null), (7.0, null)):
        eps = cond if nu is None else nu + (cond - nu) * scale
        got = E.ddim_step(x, cond, nu, scale, coef)
        for b, t in enumerate(ts):
            assert relmax(got[b], DO.ddim_step(eps[b], t, x[b], acp, 50)) < TOL
    t = torch.tensor(ts)
    assert relmax(E.axpby(x, cond, acp[t].sqrt(), (1 - acp[t]).sqrt()), DO.add_noise(x, cond, t, acp)) < TOL
    assert len({tuple(r.tolist()) for r in coef}) == 4                                  # four different coefficient rows


def test_ddim_inputs_reach_both_sides_of_the_clamp():
    seen = set()
    for cid, per, hn, cs, sn, span in E.DDIM:
        inp = E.ddim_inputs(cid, E.STEP_B, per, hn, cs, span)
        x, cond, c = inp["x"].double(), inp["cond"].double(), inp["coef"].double()
        eps = cond if inp["null"] is None else inp["null"].double() + (cond - inp["null"].double()) * cs
        x0 = (x - c[:, 0:1] * eps) / c[:, 1:2]
        if sn == "inactive":
            assert x0.abs().max() < 0.9
        elif per >= 2:
            assert ((x0 > 1.5).any(1) & (x0 < -1.5).any(1)).all()                       # every sample saturates on both sides
        assert (inp["null"] is not None) == hn
        seen.add((per, hn, cs, sn))
    assert {(p, hn, cs, sn) for p in E.PER_SAMPLE for hn, cs in E.GUIDE for sn, _ in E.SPANS} <= seen
    assert E.passes(E.STEP_B * E.STEP_BIG) == "second_pass" and any(per == E.STEP_BIG for _, per, *_ in E.DDIM) and E.STEP_BIG in E.AXPBY
    assert {cs for _, cs in E.GUIDE if _} == {1.0, 2.0, 7.0} and E.PER_SAMPLE == [1, 257, 600]


# ---------------------------------------------------------------------------------------------------------------------------------
# caps: the fp32 evaluation of every bounded case stays inside the cap the GPU file names for it.  Measured e32 (worst case over the
# table) beside each: none needed raising.
# ---------------------------------------------------------------------------------------------------------------------------------
def _guard(e32, cap, what):
    print(what, f"e32 = {e32:.3g}", f"cap = {cap:.3g}")
    assert e32 <= cap, (what, e32, cap)
    assert FLOOR <= cap


@pytest.mark.parametrize("case", E.MSE, ids=ID0)
def test_caps_mse(case):
    """SUM_CAP = 1e-6; e32 <= 1.5e-7 (torch's pairwise fp32 sum)."""
    cid, B, Dch, L, branch = case
    for has_len, has_wt, _ in E.MSE_OPTS[::2]:
        inp = E.mse_inputs(cid, B, Dch, L, has_len, has_wt)
        s64, g64 = E.mse(inp["pred"].double(), inp["target"].double(), inp["orig_len"], inp["wt"])
        s32, g32 = E.mse(inp["pred"], inp["target"], inp["orig_len"], inp["wt"])
        assert s64.abs() > 0
        _guard(E.rel1(s32, s64), E.SUM_CAP, ("mse", cid, has_len, has_wt))
        w = E.mse_weight(inp["orig_len"], inp["wt"], B, L, F32)[:, None, :]
        assert torch.equal(g32, (2 * w) * (inp["pred"] - inp["target"])) and g32.dtype == F32


@pytest.mark.parametrize("n", E.FLAT_N)
def test_caps_sqnorm_and_adamw(n):
    """SUM_CAP = 1e-6 (e32 <= 1e-7); MOMENT_CAP = 2e-6 (e32 <= 1.2e-7: a handful of roundings); UPDATE_CAP = 2e-6 beside p's spacing
    (e32 <= 4e-7).  The integer sums of the exact part stay below 2^24 per fp32 partial sum: 9 per element, at most 2 * 4 elements per
    lane, 256 lanes."""
    g = E.uni("sq.g", (n,), 3.0)
    _guard(E.rel1(E.sqnorm(g), E.sqnorm(g.double())), E.SUM_CAP, ("sqnorm", n))
    assert 9 * 8 * 256 < 2 ** 24 and E.sqnorm(E.ints("sq.i", (n,), 3).double()) < 2 ** 53
    p, g, m, v = E.adamw_inputs(n)
    for step in E.ADAMW_STEPS:
        for gs in (1.0, 0.25, 0.0):
            for wd in E.ADAMW_WD:
                hyper = E.HYPER + (wd,)
                r64 = E.adamw_step(p.double(), g.double(), m.double(), v.double(), hyper, step, gs)
                r32 = E.adamw_step(p, g, m, v, hyper, step, gs)
                assert all(t.dtype == F32 for t in r32)
                _guard(relmax(r32[1], r64[1]), E.MOMENT_CAP, ("m", n, step, gs, wd))
                _guard(relmax(r32[2], r64[2]), E.MOMENT_CAP, ("v", n, step, gs, wd))
                _guard(E.update_metric(p)(r32[0], r64[0]), E.UPDATE_CAP, ("update", n, step, gs, wd))


def test_update_metric_sees_a_wrong_bias_correction():
    """p' alone at relmax would let a wrong bias correction through; the update does not."""
    p, g, m, v = (t.double() for t in E.adamw_inputs(1027))
    lr, b1, b2, eps = E.HYPER
    for step in (1, 2, 1000):
        good = E.adamw_step(p, g, m, v, E.HYPER + (0.0,), step)[0]
        bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
        m2, v2 = b1 * m + (1 - b1) * g, b2 * v + (1 - b2) * g * g
        swapped = p - (lr / bc2 ** 0.5) * m2 / (v2.sqrt() / bc1 + eps)
        assert E.update_metric(p.float())(swapped, good) > 100 * E.UPDATE_CAP


@pytest.mark.parametrize("case", E.DDIM, ids=ID0)
def test_caps_ddim(case):
    """STEP_CAP = 2e-6 relmax; e32 <= 2.5e-7."""
    cid, per, hn, cs, sn, span = case
    inp = E.ddim_inputs(cid, E.STEP_B, per, hn, cs, span)
    d = lambda t: None if t is None else t.double()
    r64 = E.ddim_step(d(inp["x"]), d(inp["cond"]), d(inp["null"]), cs, d(inp["coef"]))
    r32 = E.ddim_step(inp["x"], inp["cond"], inp["null"], cs, inp["coef"])
    assert r32.dtype == F32
    _guard(relmax(r32, r64), E.STEP_CAP, ("ddim", cid))


@pytest.mark.parametrize("per", E.AXPBY)
def test_caps_axpby(per):
    """STEP_CAP = 2e-6 relmax; e32 <= 1e-7."""
    x, y = E.uni("ax.x", (E.STEP_B, per), 1.5), E.uni("ax.y", (E.STEP_B, per), 1.5)
    coef = E.ddim_coef().to(F32)
    r64 = E.axpby(x.double(), y.double(), coef[:, 1].double(), coef[:, 0].double())
    _guard(relmax(E.axpby(x, y, coef[:, 1], coef[:, 0]), r64), E.STEP_CAP, ("axpby", per))


# ---------------------------------------------------------------------------------------------------------------------------------
# contract table
# ---------------------------------------------------------------------------------------------------------------------------------
def test_contract_table_names_every_condition():
    assert {kind for _, kind, _ in E.EW_BAD} == E.EW_BAD_KINDS
    csrc = Path(__file__).resolve().parent.parent / "osufusion_amd" / "csrc"
    src = (csrc / "elementwise.hip").read_text()
    for entry, kind, over in E.EW_BAD:
        assert over and f'extern "C" int {entry}(' in (csrc / ("sampling.hip" if entry in ("osuf_axpby_rows", "osuf_ddim_step") else "elementwise.hip")).read_text(), entry
        for arg, val in over.items():
            if val == "null":
                assert kind == "null" and arg in E.NULL_GUARDED[entry], (entry, arg)      # only where the source refuses it before the launch
            if val == "off4":
                assert kind == "al16" and arg in E.AL16_GUARDED[entry], (entry, arg)
        assert E.bad_status(kind) == (E.EUNSUPPORTED if kind == "dtype" else E.EINVAL)
    # every guard the source has for these entry points is in the table
    for table, marker in ((E.NULL_GUARDED, "null"), (E.AL16_GUARDED, "off4")):
        for entry, args in table.items():
            assert args == {a for e, _, over in E.EW_BAD if e == entry for a, v in over.items() if v == marker}, entry
    # the guards themselves, as the source spells them
    for text in ("!a || !b || !dst", "!al16(a) || !al16(b) || !al16(dst)", "!pred || !target || !loss_sum", "!sumsq || !coef", "!g || !out", "!in || !out", "!src || !dst"):
        assert text in src, text
