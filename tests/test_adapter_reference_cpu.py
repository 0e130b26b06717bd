"""The hand-written references of tests/adapter_reference.py against oracle/lora_oracle.py and fp64 autograd, its restated launcher
arithmetic against the branch each table entry names, the caps written next to the tables, and the inventory of the adapter entry points
(CPU only).

tests/test_adapter_rows_gpu.py measures the LoRA / DoRA kernels against these functions, so a slip in one of them would either hide a
kernel bug or report one that is not there."""
import re
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

from oracle import lora_oracle as LO
from tests import adapter_reference as R
from tests import gemm_reference as GR
from tests.bound_check import FLOOR
from tests.test_poisoned_memory import relmax

TOL = 1e-12                                                # fp64 against fp64
F32, F64 = torch.float32, torch.float64
ROOT = Path(__file__).resolve().parent.parent


def factors64(cid, O, I, k, r, mag=True):
    return R.cast(R.real_factors(cid, O, I, k, r, mag), F64)


# ---------------------------------------------------------------------------------------------------------------------------------
# references against the oracle and autograd
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("O,I,k,r,mag", [(5, 7, 3, 4, True), (5, 7, 3, 4, False), (9, 4, 1, 2, True), (3, 6, 7, 5, True)])
def test_effective_weight_equals_the_oracle(O, I, k, r, mag):
    W, A, B, m = factors64("or", O, I, k, r, mag)
    delta = LO.delta_weight(A, B.reshape(O, r, 1), W)
    assert relmax(R.adapted(W, A, B, R.S), W + R.S * delta) < TOL
    We, g = R.effective(W, A, B, m, R.S)
    assert relmax(We, LO.effective_weight(W, A, B.reshape(O, r, 1), m, R.S)) < TOL
    if mag:
        assert relmax(g, m / LO.weight_norm(W, delta, R.S)) < TOL
        assert relmax(R.sgbt(B, g, R.S), (R.S * g[:, None] * B).T) < TOL and R.sgbt(B, g, R.S).shape == (r, O)
    else:
        assert g is None and torch.equal(R.sgbt(B, None, R.S), (R.S * B).T)


def test_rows_differ_by_factors_of_two_and_a_wrong_row_shows():
    O, I, k, r = 6, 5, 3, 4
    W, A, B, m = factors64("rows", O, I, k, r)
    V = R.adapted(W, A, B, R.S)
    g = R.gain(V, m)
    assert (g.roll(1) / g - 1).abs().min() > 0.05                                        # no two neighbouring gains agree to 5 %
    assert relmax(R.scale_rows(V, g.roll(1)), R.scale_rows(V, g)) > 0.05                 # the neighbouring row's gain
    assert relmax(R.adapted(W, A, B.roll(1, 0), R.S), V) > 0.05                          # the neighbouring row's B
    assert relmax(R.gain(V, m), m / V.flatten(1).abs().sum(1)) > 0.05                    # an L1 norm


@pytest.mark.parametrize("k", [1, 3, 7])
@pytest.mark.parametrize("bias", [True, False])
def test_finish_formulas_equal_autograd(k, bias):
    """dA, dB and dm of sum(wgt * (conv1d(x, Weff) + bias)) from the factored form -- tb = dy^T u, gt = the swapped, tap-flipped x^T du,
    s0 = sum dy y, s1 = sum dy -- through R.finish equal fp64 autograd (the norm behind g detached, as in the reference)."""
    O, I, r, L, Bn, pad = 6, 5, 3, 11, 2, k // 2
    W, A, B, m = factors64(f"auto{k}", O, I, k, r)
    b = R.uni("auto.bias", (O,), 0.5).double() if bias else None
    x, dy = R.uni("auto.x", (Bn, I, L)).double(), R.uni("auto.dy", (Bn, O, L)).double()
    Ap, Bp, mp = A.clone().requires_grad_(), B.clone().requires_grad_(), m.clone().requires_grad_()
    g = mp * R.gain(R.adapted(W, Ap, Bp, R.S), torch.ones_like(m)).detach()             # m / ||V||, the norm a constant
    y = F.conv1d(x, R.scale_rows(R.adapted(W, Ap, Bp, R.S), g), b, padding=pad)
    (y * dy).sum().backward()
    gd, yd = g.detach(), y.detach()
    u = F.conv1d(x, A, padding=pad)                                                      # (Bn, r, L)
    du = torch.einsum("bol,oq->bql", dy, R.S * gd[:, None] * B)
    tb = torch.einsum("bol,bql->oq", dy, u)
    gt = torch.zeros(k, I, r, dtype=F64)
    for t in range(k):                                                                   # G[t'][i][q] = sum_m x[m][i] du[m + t' - (k-1-pad)][q]
        sh = t - (k - 1 - pad)
        lo, hi = max(0, -sh), min(L, L - sh)
        gt[t] = torch.einsum("bil,bql->iq", x[:, :, lo:hi], du[:, :, lo + sh:hi + sh])
    s0, s1 = (dy * yd).sum((0, 2)), dy.sum((0, 2))
    dB, dA, dm = R.finish(tb, R.S * gd, gt, s0, s1 if bias else None, b, m)
    assert relmax(dB, Bp.grad) < TOL and relmax(dA, Ap.grad) < TOL and relmax(dm, mp.grad) < TOL
    assert relmax(gt.permute(2, 1, 0), Ap.grad) > 1e-2 or k == 1                         # without the tap flip
    bases = [torch.ones(O, r, dtype=F64), torch.ones(r, I, k, dtype=F64), torch.ones(O, dtype=F64)]
    dB1, dA1, dm1 = R.finish(tb, R.S * gd, gt, s0, s1 if bias else None, b, m, bases)
    assert relmax(dB1, dB + 1) < TOL and relmax(dA1, dA + 1) < TOL and relmax(dm1, dm + 1) < TOL
    assert R.finish(tb, R.S * gd, gt)[2] is None


def test_layouts_equal_the_convolutions_they_serve():
    """fwd [k][O][I] and the three dgrad layouts, used as GEMM operands under the geometry of each kind (tests/gemm_reference.py), equal
    torch's convolutions with the plain weight and their input gradients: same padding; a stride-2 conv behind a right reflect pad of one;
    nearest x2 followed by a k3 conv."""
    O, I, L, Bn = 5, 4, 12, 2
    for kind, k in (("same", 3), ("same", 5), ("same", 4), ("same", 1), ("down", 3), ("up", 3)):
        w = R.uni(f"lay.{kind}{k}", (O, I, k)).double()
        x = R.uni(f"lay.x.{kind}{k}", (Bn, I, L)).double().requires_grad_()
        if kind == "same":
            y = F.conv1d(F.pad(x, (k // 2, k - 1 - k // 2)), w)
        elif kind == "down":
            y = F.conv1d(F.pad(x, (0, 1), mode="reflect"), w, stride=2)
        else:
            y = F.conv1d(x.repeat_interleave(2, dim=2), w, padding=1)
        dy = R.uni(f"lay.dy.{kind}{k}", tuple(y.shape)).double()
        (y * dy).sum().backward()
        fg, dg = GR.geom(kind, k, L)
        rows = lambda t: t.detach().permute(0, 2, 1).reshape(-1, t.shape[1])
        back = lambda t, n: t.reshape(Bn, n, -1).permute(0, 2, 1)
        assert relmax(back(GR.gemm_nt(rows(x), R.fwd_layout(w), **fg), y.shape[2]), y.detach()) < TOL, (kind, k)
        assert relmax(back(GR.gemm_nt(rows(dy), R.dgrad_layout(w, kind), **dg), L), x.grad) < TOL, (kind, k)
    w = R.uni("lay.slip", (O, I, 3)).double()
    assert not torch.equal(R.dgrad_layout(w, "same"), w.permute(2, 1, 0))                # without the tap flip
    assert not torch.equal(R.dgrad_layout(w, "down")[:3], R.dgrad_layout(w, "same"))     # down keeps the tap order


def test_exact_cases_stay_exact_in_fp32():
    for cid, O, I, k, r, *_ in R.PACK:
        W, A, B = R.exact_factors(cid, O, I, k, r)
        assert W.max() < 2 ** 16 and W.unique().numel() == W.numel() and 4 * r * R.S < 2 ** 16
        We = R.scale_rows(R.adapted(W.double(), A.double(), B.double(), R.S), R.row_pow2(O).double())
        for t in [R.fwd_layout(We)] + [R.dgrad_layout(We, kind) for kind in (R.KINDS if k == 3 else ("same",))]:
            assert torch.equal(t.float().double(), t)
    for cid, O, I, k, r, *_ in R.FINISH:
        inp = R.finish_inputs(cid, O, I, k, r, True)
        dB, dA, _ = R.finish(*(inp[n].double() for n in ("tb", "sg", "gt")), bases=R.cast(inp["bases"], F64))
        assert torch.equal(dB.float().double(), dB) and torch.equal(dA.float().double(), dA)


# ---------------------------------------------------------------------------------------------------------------------------------
# branches
# ---------------------------------------------------------------------------------------------------------------------------------
def test_every_table_entry_reaches_the_branch_it_names():
    for cid, O, IK, r, mag, gout, br in R.EFFECTIVE:
        assert br == R.effective_branch(O, IK), (cid, R.effective_branch(O, IK))
    assert {(e[1], e[2]) for e in R.EFFECTIVE} >= {(1, 1), (3, 200), (9, 3072), (5, 3073), (3, 6145), (2, 12289), (2, 38400)}
    assert {e[6][0] for e in R.EFFECTIVE} == {8, 4, 2, 1} and {e[3] for e in R.EFFECTIVE} == {1, 8, 17}
    assert {oc for _, O, _, _, _, _, (oc, *_) in R.EFFECTIVE if O % oc} >= {8, 4, 2}      # clamped duplicate rows under OC 8, 4 and 2
    assert sum(not e[4] for e in R.EFFECTIVE) == 1 and sum(not e[5] for e in R.EFFECTIVE) == 1
    assert R.effective_branch(2, 38400)[0] == 1 and R.effective_branch(*R.EFFECTIVE_EINVAL) == "einval" and 3072 * 4 * 8 == 96 * 1024
    assert [R.effective_branch(1, ik)[0] for ik in (3072, 3073, 6144, 6145, 12288, 12289)] == [8, 4, 4, 2, 2, 1]

    for cid, O, I, k, r, mag, outs, br in R.GAIN:
        assert br == R.adapt_branch(O, I, k, r), (cid, R.adapt_branch(O, I, k, r))
    assert {e[2] for e in R.GAIN} == {1, 31, 32, 33, 70} and {e[1] for e in R.GAIN} == {1, 33, 255, 256, 257} and {e[3] for e in R.GAIN} == {1, 3, 7}
    assert {e[7][1] for e in R.GAIN} == {1, 2, 3} and {e[6] for e in R.GAIN} == {"32", "16", "both"}
    assert sum(e[7][0] == "attr" for e in R.GAIN) == 1 and sum(not e[5] for e in R.GAIN) == 1
    r, k = R.ADAPT_UNSUPPORTED
    assert R.adapt_branch(1, 1, k, r)[0] == "unsupported" and R.adapt_lds(r, k) == 98432
    assert R.adapt_lds(64, 3) == R.adapt_lds(32, 7) == 32896 and R.adapt_branch(1, 1, 3, 63)[0] == "plain"

    for cid, O, I, k, r, kind, g, outs, br in R.PACK:
        assert br == R.adapt_branch(O, I, k, r) and (kind == "same" or k == 3), (cid, R.adapt_branch(O, I, k, r))
    assert {e[1] for e in R.PACK} == {e[2] for e in R.PACK} == {1, 31, 32, 33, 70} and {e[3] for e in R.PACK} == {1, 3, 4, 5, 7}
    assert {e[5] for e in R.PACK} == set(R.KINDS) and {e[7] for e in R.PACK} == {"FD", "F", "D"} and {e[6] for e in R.PACK} == {True, False}
    assert any(e[3] == 7 and e[6] for e in R.PACK) and sum(e[8][0] == "attr" for e in R.PACK) >= 1
    assert {(e[3], e[4]) for e in R.PACK if e[8][0] == "attr"} == {(3, 64), (7, 32)}

    for cid, O, I, k, r, acc, dm, bias, br in R.FINISH:
        assert br == R.finish_branch(O, I, k, r), (cid, R.finish_branch(O, I, k, r))
    assert {e[8][0] for e in R.FINISH} == {"O*r", "r*I*k"} and {e[3] for e in R.FINISH} == {1, 3, 7} and {e[5] for e in R.FINISH} == {0, 1}
    assert any(not e[6] for e in R.FINISH) and any(e[6] and not e[7] for e in R.FINISH) and max(e[8][1] for e in R.FINISH) > 1
    assert ("o300_i2_k1_r3", 300, 2, 1, 3) == R.FINISH[0][:5]


# ---------------------------------------------------------------------------------------------------------------------------------
# caps
# ---------------------------------------------------------------------------------------------------------------------------------
def test_caps_effective_and_gain():
    worst_w = worst_g = worst_t = 0.0
    for cid, O, IK, r, mag, *_ in R.EFFECTIVE:
        f32 = R.real_factors(cid, O, IK, 1, r, mag)
        (w64, g64), (w32, g32) = R.effective(*R.cast(f32, F64), R.S), R.effective(*f32, R.S)
        worst_w = max(worst_w, 16 * relmax(w32, w64))
        worst_g = max(worst_g, 16 * relmax(g32, g64)) if mag else worst_g
    for cid, O, I, k, r, mag, *_ in R.GAIN:
        W, A, B, m = R.real_factors(cid, O, I, k, r, mag)
        if mag:
            g64, g32 = R.gain(R.adapted(W.double(), A.double(), B.double(), R.S), m.double()), R.gain(R.adapted(W, A, B, R.S), m)
            worst_g = max(worst_g, 16 * relmax(g32, g64))
            worst_t = max(worst_t, 16 * relmax(R.sgbt(B, g32, R.S), R.sgbt(B.double(), g64, R.S)))
    assert FLOOR < R.EFFECTIVE_CAP == R.smallest_cap(worst_w), worst_w
    assert FLOOR < R.G_CAP == R.smallest_cap(worst_g), worst_g
    assert FLOOR < R.SGBT_CAP == R.smallest_cap(worst_t), worst_t


def test_caps_pack_and_finish():
    worst = 0.0
    for cid, O, I, k, r, kind, g, *_ in R.PACK:
        W, A, B, _ = R.real_factors(cid, O, I, k, r, False)
        gv = R.real_gain(cid, O) if g else None
        w64 = R.scale_rows(R.adapted(W.double(), A.double(), B.double(), R.S), R.cast(gv, F64))
        w32 = R.scale_rows(R.adapted(W, A, B, R.S), gv)
        worst = max(worst, 16 * relmax(R.fwd_layout(w32), R.fwd_layout(w64)), 16 * relmax(R.dgrad_layout(w32, kind), R.dgrad_layout(w64, kind)))
    assert FLOOR < R.PACK_CAP == R.smallest_cap(worst), worst
    worst = 0.0
    for cid, O, I, k, r, acc, dm, bias, _ in R.FINISH:
        inp = R.finish_inputs(cid, O, I, k, r, False)
        args = lambda dt: [R.cast(inp[n], dt) for n in ("tb", "sg", "gt", "s0", "s1", "bias", "m", "bases")]
        worst = max([worst] + [16 * relmax(a, b) for a, b in zip(R.finish(*args(F32)), R.finish(*args(F64)))])
    assert FLOOR < R.DM_CAP == R.smallest_cap(worst), worst


# ---------------------------------------------------------------------------------------------------------------------------------
# inventory
# ---------------------------------------------------------------------------------------------------------------------------------
def test_every_adapter_entry_point_has_a_case_table():
    src = (ROOT / "osufusion_amd" / "csrc" / "elementwise.hip").read_text()
    defined = set(re.findall(r'extern "C"\s+\w+\s+(osuf_\w+)\s*\([^)]*\)\s*\{', src))
    adapter = {n for n in defined if re.search(r"dora|adapt", n)}
    assert adapter == set(R.KERNELS), adapter ^ set(R.KERNELS)
    gpu = (ROOT / "tests" / "test_adapter_rows_gpu.py").read_text()
    for name, tables in R.KERNELS.items():
        assert all(len(R.TABLES[t]) > 0 for t in tables) and f'"{name}"' in gpu, name
        assert all(f"R.{t}" in gpu for t in tables), name
