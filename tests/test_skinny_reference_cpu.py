"""The hand-written references of tests/skinny_reference.py against fp64 autograd, its restated slice plan against the branch each table
entry names, the band its generators keep clear around bf16 rounding boundaries, and the guard of the GPU file's caps (CPU only).

tests/test_skinny_rows_gpu.py measures the skinny-linear kernels against these functions, so a slip in one of them would either hide a
kernel bug or report one that is not there."""
import pytest
import torch
import torch.nn.functional as F

from tests import skinny_reference as S
from tests.bound_check import FLOOR
from tests.test_poisoned_memory import relmax

TOL = 1e-12                                                # fp64 against fp64
F32, F64 = torch.float32, torch.float64
IDS = lambda v: v[0] if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("in_act,out_act", S.ACTS)
def test_references_equal_autograd_in_f32_mode(in_act, out_act, bias):
    M, N, K = 7, 11, 13
    x, W = S.uni("x", (M, K), 1.5).double().requires_grad_(), S.uni("w", (N, K), 0.3).double().requires_grad_()
    b = S.uni("b", (N,), 0.2).double().requires_grad_() if bias else None
    z = F.linear(F.silu(x) if in_act else x, W, b)
    y = torch.sigmoid(z) if out_act else z
    dy = S.uni("dy", (M, N)).double()
    y.backward(dy)
    xd, Wd, yd = x.detach(), W.detach(), y.detach()
    assert relmax(S.fwd(xd, Wd, None if b is None else b.detach(), in_act, out_act), yd) < TOL
    assert relmax(S.dx(dy, yd, xd, Wd, in_act, out_act), x.grad) < TOL
    base_w, base_b = S.uni("bw", (N, K)).double(), S.uni("bb", (N,)).double()
    gw, gb = S.dw(dy, yd, xd, in_act, out_act, base_w, base_b, True)
    assert relmax(gw, W.grad + base_w) < TOL
    assert relmax(gb, (b.grad if bias else S.dz_of(dy, yd, out_act).sum(0)) + base_b) < TOL
    gw, gb = S.dw(dy, yd, xd, in_act, out_act, base_w, None, False)
    assert relmax(gw, W.grad) < TOL and gb is None


@pytest.mark.parametrize("in_act", S.GROUP_ACTS)
def test_group_references_equal_autograd(in_act):
    M, K, Ns = 5, 16, (8, 24, 40)
    inp = S.group_inputs("auto", M, K, Ns, 1, 2)
    x = inp["x"].double().requires_grad_()
    Ws, bs, dys = S.cast(inp["Ws"], F64), S.cast(inp["bs"], F64), S.cast(inp["dys"], F64)
    ys = [F.linear(F.silu(x) if in_act else x, W, b) for W, b in zip(Ws, bs)]
    sum((y * d).sum() for y, d in zip(ys, dys) if d is not None).backward()
    got_y, got_dx = S.group_refs(inp, F64, in_act, "f32")
    assert all(relmax(g, y.detach()) < TOL for g, y in zip(got_y, ys))
    assert relmax(got_dx, x.grad) < TOL


def test_bf16_mode_rounds_the_operands_and_nothing_else():
    x, W, dy = S.make_x("rx", 5, 24), S.make_w("rw", 9, 24), S.uni("rdy", (5, 9))
    b = S.make_b("rb", 9)
    bf = lambda t: t.bfloat16().double()
    xd, Wd = x.double(), W.double()
    y = S.fwd(xd, Wd, b.double(), 1, 2, "bf16")
    assert relmax(y, torch.sigmoid(bf(F.silu(xd).float()) @ bf(W).T + b.double())) < TOL
    d = dy.double() * y * (1 - y)
    assert relmax(S.dx(dy.double(), y, xd, Wd, 1, 2, "bf16"), (bf(d.float()) @ bf(W)) * S.silu_grad(xd)) < TOL
    gw, gb = S.dw(dy.double(), y, xd, 1, 2, None, torch.zeros(9, dtype=F64), False, "bf16")
    assert relmax(gw, bf(d.float()).T @ bf(F.silu(xd).float())) < TOL
    assert relmax(gb, d.sum(0)) < TOL                                                   # db: the unrounded dz


def test_slice_plan_and_branches_follow_the_table():
    """Each entry reaches the branch it names, and together the tables reach every branch of the host's choice."""
    for cid, N, K, Ms, off, pad, geo, vec in S.FWD:
        assert S.fwd_vec(K, K + pad, off) == vec, cid
    fwd = {(vec, K % 8 == 0, off % 4 == 0, pad % 4 == 0) for _, N, K, _, off, pad, _, vec in S.FWD}
    assert {(True, True, True, True), (False, False, True, True), (False, True, False, True), (False, True, True, False)} <= fwd
    assert any(vec and pad for *_, pad, _, vec in S.FWD)                                # vec at ldx > K
    assert {-(-K // 256) for _, _, K, _, _, _, _, vec in S.FWD if vec} >= {1, 2, 3}       # trips of the 256-wide k loop
    assert {(1, 64), (64, 1)} <= {(N, K) for _, N, K, *_ in S.FWD}
    for cid, N, K, Ms, off, geo, vec, slices, last in S.DX:
        assert S.dx_branch(N, K, off) == (vec, slices, last), (cid, S.dx_branch(N, K, off))
    assert S.bwd_split(256, 256) == (1, 256) and S.bwd_split(256, 257)[0] > 1            # N K = 65536 is the last single slice
    assert S.bwd_split(264, 256) == (3, 128) and S.bwd_split(2048, 40) == (16, 128) and S.bwd_split(136, 488) == (2, 128)
    dxs = {(vec, slices > 1, last) for *_, vec, slices, last in S.DX}
    assert {(True, False, 256), (True, True, 8), (False, True, 1), (False, False, 33), (False, True, 8)} <= dxs
    assert any(N % 8 == 0 and not vec for _, N, _, _, _, _, vec, *_ in S.DX)            # misaligned dy
    assert any(S.dw_tiles(N, K) % 4 for _, N, K, *_ in S.DW) and S.dw_tiles(40, 72) == 6
    assert {(a, d) for *_, a, d in S.DW} == {(0, False), (0, True), (1, False), (1, True)}
    assert {(N, K) for _, N, K, *_ in S.FWD[:7]} <= {(N, K) for _, N, K, *_ in S.DW}     # the forward's shape list is the weight gradient's
    for table in (S.FWD, S.DX, S.DW):
        Ms = [M for e in table for M in e[3]]
        assert all(33 in e[3] and len(e[3]) == 2 for e in table)
        assert all(Ms.count(M) >= 2 for M in (1, 5, 32, 33, 65)) and set(Ms) == {1, 5, 32, 33, 65}
    # group: slices of 512 + 8 rows, linears that are no multiple of 32 wide, one bias and one dy absent, one group of a single linear
    assert [-(-N // 512) for N in S.GROUP_N] == [1, 1, 2, 3, 1] and 520 - 512 == 8 and 1032 - 1024 == 8
    assert sum(N % 32 != 0 for N in S.GROUP_N[:2]) == 2 and all(N % 8 == 0 for N in S.GROUP_N)
    assert {(M, K) for _, M, K, *_ in S.GROUP[:4]} == {(M, K) for M in (5, 33) for K in (96, 264)} and len(S.GROUP[4][3]) == 1


def test_exact_cases_stay_exact_in_fp32():
    """Section A relies on every partial sum being an integer below 2^24: |x|, |dy| <= 3, |W| <= 2, |bias|, |base| <= 5."""
    depth = max([K for _, _, K, *_ in S.FWD] + [N for _, N, *_ in S.DX] + [65] + [sum(S.GROUP_N)])
    assert depth * 6 + 5 < 2 ** 24


def test_near_boundary():
    one = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -7, -(1.0 + 2.0 ** -8), 0.0, 3.0 * 2.0 ** -9 * (1 + 2.0 ** -8 / 1.5)], dtype=F64)
    assert S.near_boundary(one).tolist() == [False, True, False, True, False, True]
    mid = 1.0 + 2.0 ** -8
    assert S.near_boundary(torch.tensor([mid * (1 + 0.9 * S.BAND), mid * (1 - 0.9 * S.BAND)], dtype=F64)).all()
    assert not S.near_boundary(torch.tensor([mid * (1 + 1.2 * S.BAND), mid * (1 - 1.2 * S.BAND)], dtype=F64)).any()
    v = S.uni("nb", (4096,), 2.0).double()
    flips = v.float().bfloat16() != (v * (1 + S.BAND / 2)).float().bfloat16()
    flips |= v.float().bfloat16() != (v * (1 - S.BAND / 2)).float().bfloat16()
    assert (S.near_boundary(v) | ~flips).all()                                          # whatever half a band can flip is inside the band


def _operands(inp):
    xd, yd, dyd = inp["x"].double(), inp["y"].double(), inp["dy"].double()
    return [xd, S.silu(xd), inp["W"].double(), dyd, S.dz_of(dyd, yd, inp["out_act"])]


def _all_linear_cases():
    for table in (S.FWD, S.DX, S.DW):
        for e, M in S.cases(table):
            yield e[0], M, e[1], e[2]
    yield S.STRIDED_FWD[0] + "_strided", S.STRIDED_M, S.STRIDED_FWD[1], S.STRIDED_FWD[2]
    for cid, N, K in S.STRIDED_DX:
        yield cid + "_strided", S.STRIDED_M, N, K


LINEAR = sorted(set(_all_linear_cases()))


def _guard(e32, cap, what):
    assert 16 * e32 < cap, (what, e32, cap)
    assert FLOOR < cap


@pytest.mark.parametrize("mode", S.MODES)
@pytest.mark.parametrize("cid,M,N,K", LINEAR, ids=lambda v: str(v))
def test_band_and_caps_linear(cid, M, N, K, mode):
    """No generated operand sits inside the excluded band, the fp32 evaluation therefore rounds every operand as the fp64 one does, and
    every cap of the GPU file lies at or above 16 x the fp32 evaluation's own distance to fp64."""
    for ia, oa in S.ACTS:
        inp = S.linear_inputs(cid, M, N, K, ia, oa, mode)
        for o in _operands(inp):
            assert not S.near_boundary(o).any()
        x, dy, y = inp["x"], inp["dy"], inp["y"]
        assert torch.equal(S.rb(S.silu(x), "bf16").double(), S.rb(S.silu(x.double()), "bf16"))
        assert torch.equal(S.rb(S.dz_of(dy, y, oa), "bf16").double(), S.rb(S.dz_of(dy.double(), y.double(), oa), "bf16"))
        assert x.abs().max() <= 1.5 and inp["W"].abs().max() <= 1 / K ** 0.5 and dy.abs().max() <= 1
        bw, bb = S.dw_bases(cid, N, K)
        r64, r32 = S.linear_refs(inp, F64, bw, bb, True), S.linear_refs(inp, F32, bw, bb, True)
        for name, a, b, cap in zip(("y", "dx", "dW", "db"), r32, r64, (S.OUT_CAP, S.OUT_CAP, S.OUT_CAP, S.DB_CAP)):
            _guard(relmax(a, b), cap, (name, ia, oa))


@pytest.mark.parametrize("mode", S.MODES)
@pytest.mark.parametrize("case", S.GROUP, ids=IDS)
def test_band_and_caps_group(case, mode):
    inp = S.group_inputs(*case)
    xd = inp["x"].double()
    for o in [xd, S.silu(xd)] + S.cast(inp["Ws"], F64) + [d.double() for d in inp["dys"] if d is not None]:
        assert not S.near_boundary(o).any()
    assert sum(b is None for b in inp["bs"]) == (case[4] is not None) and sum(d is None for d in inp["dys"]) == (case[5] is not None)
    for ia in S.GROUP_ACTS:
        (y64, dx64), (y32, dx32) = S.group_refs(inp, F64, ia, mode), S.group_refs(inp, F32, ia, mode)
        for a, b in zip(y32 + [dx32], y64 + [dx64]):
            _guard(relmax(a, b), S.OUT_CAP, (case[0], ia))
