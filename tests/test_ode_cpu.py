"""The ODE solvers of the flow samplers, host side (osufusion_amd/ode.py): every tableau against its order conditions in exact rationals, the
step controller and the clipping of the last step against hand-computed values, the adaptive loop's bookkeeping with the two device calls
replaced by torch on the CPU, the public keywords, and the C surface of osuf_rk_error: declared, bound, exported, and refusing bad arguments
before any launch.  The convergence slopes of the restatement (tests/ode_oracle.py) are printed for the record, not asserted: the order
conditions are the proof."""
import ctypes
import inspect
import math
from ctypes import c_int, c_long, c_void_p
from fractions import Fraction as Fr

import numpy as np
import pytest
import torch

from osufusion_amd import _lib, ode
from osufusion_amd.models import RectifiedFlowOsuFusionDiT
from osufusion_amd.models.rectified_flow import OsuFusion as FlowOsuFusion
from tests import ode_oracle as OO


# ---- order conditions ----------------------------------------------------------------------------------------------------------------------------
# A rooted tree is the sorted tuple of its root's subtrees; the leaf is ().  For a tree t with subtrees t_1 .. t_m:
#   order |t| = 1 + sum |t_k|,  density gamma(t) = |t| prod gamma(t_k),  elementary weights Phi_i(t) = prod_k sum_j a_ij Phi_j(t_k), Phi_i(leaf) = 1.
# A method has order p iff sum_i b_i Phi_i(t) = 1 / gamma(t) for every tree of order <= p (Butcher; Hairer, Norsett & Wanner II.2).
def _trees(n, _memo={1: [()]}):
    if n not in _memo:
        out = set()

        def forests(left, smallest):                        # multisets of trees with `left` vertices in total, orders ascending
            if left == 0:
                yield ()
                return
            for k in range(smallest, left + 1):
                for t in _trees(k):
                    for rest in forests(left - k, k):
                        yield (t,) + rest
        for forest in forests(n - 1, 1):
            out.add(tuple(sorted(forest)))
        _memo[n] = sorted(out)
    return _memo[n]


def _order(t):
    return 1 + sum(_order(s) for s in t)


def _gamma(t):
    g = _order(t)
    for s in t:
        g *= _gamma(s)
    return g


def _phi(t, a):
    """[Phi_i(t)] over the stages."""
    out = [Fr(1)] * len(a)
    for s in t:
        inner = _phi(s, a)
        out = [o * sum((aij * inner[j] for j, aij in enumerate(row)), Fr(0)) for o, row in zip(out, a)]
    return out


def _holds(weights, a, p):
    return all(sum((w * ph for w, ph in zip(weights, _phi(t, a))), Fr(0)) == Fr(1, _gamma(t)) for n in range(1, p + 1) for t in _trees(n))


def test_the_tree_generator_counts_the_rooted_trees():
    assert [len(_trees(n)) for n in range(1, 7)] == [1, 1, 2, 4, 9, 20]
    assert _gamma(((), ())) == 3 and _gamma((((),),)) == 6 and _gamma((((), ()),)) == 12


@pytest.mark.parametrize("name", ode.METHODS)
def test_tableau_satisfies_its_order_conditions_exactly(name):
    tab = ode.TABLEAUS[name]
    s = tab.stages
    assert len(tab.c) == len(tab.a) == s and all(len(row) == i for i, row in enumerate(tab.a))     # explicit: row i has i entries
    assert all(isinstance(v, Fr) for row in tab.a for v in row) and all(isinstance(v, Fr) for v in tab.b + tab.c)
    a = [list(row) + [Fr(0)] * (s - len(row)) for row in tab.a]
    assert all(ci == sum(row, Fr(0)) for ci, row in zip(tab.c, a))
    assert sum(tab.b, Fr(0)) == 1
    assert _holds(tab.b, a, tab.order) and not _holds(tab.b, a, tab.order + 1)                      # its order and no higher
    assert tab.adaptive == (name in ("bosh3", "dopri5"))
    if tab.adaptive:
        assert sum(tab.e, Fr(0)) == 0 and tab.e == tuple(x - y for x, y in zip(tab.b, tab.b_star))
        assert _holds(tab.b_star, a, tab.order - 1) and not _holds(tab.b_star, a, tab.order)
        assert tuple(a[-1]) == tab.b and tab.c[-1] == 1 and tab.b[-1] == 0                          # first same as last
    co = tab.floats()
    assert co.b == [float(v) for v in tab.b] and co.a[-1] == [float(v) for v in tab.a[-1]]
    assert (co.e is None) == (not tab.adaptive)


def test_the_orders_and_the_skipped_stage():
    assert {n: (t.stages, t.order) for n, t in ode.TABLEAUS.items()} == {"euler": (1, 1), "midpoint": (2, 2), "rk4": (4, 4), "bosh3": (4, 3),
                                                                          "dopri5": (7, 5)}
    assert ode.TABLEAUS["rk4"].b == (Fr(1, 8), Fr(3, 8), Fr(3, 8), Fr(1, 8))                        # the 3/8 rule
    assert ode.TABLEAUS["dopri5"].floats().e[1] == 0.0                                              # the stage osuf_rk_error never reads
    assert ode.TABLEAUS["bosh3"].e == (Fr(-5, 72), Fr(1, 12), Fr(1, 9), Fr(-1, 8))


# ---- the controller ------------------------------------------------------------------------------------------------------------------------------
def test_step_factor_against_hand_computed_values():
    assert ode.step_factor(0.0, 5) == (True, 10.0) and ode.step_factor(0.0, 3) == (True, 10.0)
    # ratio < 1: 0.9 * ratio^(-1 / order): (1 / 32)^(-1 / 5) = 2 and (1 / 8)^(-1 / 3) = 2, so 1.8 (pow rounds: to 1e-14)
    assert ode.step_factor(1.0 / 32.0, 5) == (True, pytest.approx(1.8, rel=1e-14))
    assert ode.step_factor(1.0 / 8.0, 3) == (True, pytest.approx(1.8, rel=1e-14))
    assert ode.step_factor(1.0, 5) == (True, 1.0)                                                   # 0.9 < dfactor = 1: an accepted step never shrinks
    assert ode.step_factor(0.9, 5) == (True, 1.0)                                                   # 0.9 * 0.9^-0.2 = 0.919 < 1
    assert ode.step_factor(1e-12, 5) == (True, 10.0)                                                # 0.9 * 251 capped at 10
    # ratio > 1: rejected, 0.9 * ratio^(-1 / order) but at least 0.2
    assert ode.step_factor(32.0, 5) == (False, pytest.approx(0.45, rel=1e-14))
    assert ode.step_factor(8.0, 3) == (False, pytest.approx(0.45, rel=1e-14))
    assert ode.step_factor(1.0 + 2.0 ** -52, 5)[0] is False
    assert ode.step_factor(1e6, 5) == (False, 0.2) and ode.step_factor(1e300, 3) == (False, 0.2)
    for bad in (math.nan, math.inf, -math.inf):
        assert ode.step_factor(bad, 5) == (False, 0.2)


def test_batch_ratio_is_the_largest_and_keeps_a_non_finite_sample():
    assert ode.batch_ratio([0.25]) == 0.25 and ode.batch_ratio([0.25, 3.0, 1.0]) == 3.0 and ode.batch_ratio([0.0, 0.0]) == 0.0
    assert math.isnan(ode.batch_ratio([0.1, math.nan])) and math.isnan(ode.batch_ratio([math.inf, 0.1]))


def test_clip_step_ends_exactly_at_the_end():
    assert ode.clip_step(0.25, 0.5, 1.0) == (0.75, 0.5)
    assert ode.clip_step(0.25, 0.75, 1.0) == (1.0, 0.75) and ode.clip_step(0.25, 2.0, 1.0) == (1.0, 0.75)
    t = 0.7                                                                                         # whatever t + (1 - t) rounds to,
    end, h = ode.clip_step(t, 0.31, 1.0)
    assert end == 1.0 and h == 1.0 - t                                                              # the end is 1.0 itself, a select
    t = 1.0 - 2.0 ** -53
    assert ode.clip_step(t, 1e-3, 1.0) == (1.0, 2.0 ** -53)


def test_check_options():
    assert ode.check_options("midpoint", 1e-5, 1e-5, None, 1000) is ode.TABLEAUS["midpoint"]
    assert ode.check_options("euler", -1.0, math.nan, -2.0, 0).name == "euler"                      # fixed grid: the tolerances are ignored
    with pytest.raises(ValueError):
        ode.check_options("heun", 1e-5, 1e-5, None, 1000)
    for kw in (dict(rtol=-1e-5), dict(atol=-1.0), dict(rtol=0.0, atol=0.0), dict(rtol=math.nan), dict(atol=math.inf), dict(first_step=0.0),
               dict(first_step=-0.1), dict(first_step=math.nan), dict(max_steps=0)):
        with pytest.raises(ValueError):
            ode.check_options(**{**dict(method="dopri5", rtol=1e-5, atol=1e-5, first_step=None, max_steps=1000), **kw})
    assert ode.check_options("bosh3", 0.0, 1e-3, 0.5, 1).name == "bosh3"


# ---- the loops with the two device calls on the CPU -----------------------------------------------------------------------------------------------
OMEGA, SHAPE = 3.0, (2, 6, 5)


def _cpu_device_calls(monkeypatch):
    def combine(y, ks, weights, dt):
        out = y.double()
        for w, k in zip(weights, ks):
            if w != 0.0:
                out = out + (dt * w) * k.double()
        return out.float()

    def rk_error(y0, y1, ks, e, dt, atol, rtol):
        return torch.from_numpy(OO.error_ratio(y0.numpy(), y1.numpy(), [None if k is None else k.numpy() for k in ks], e, dt, atol, rtol))
    monkeypatch.setattr(ode, "_combine", combine)
    monkeypatch.setattr(ode, "rk_error", rk_error)


def _f32(t, y):
    k = torch.empty_like(y)
    k[:, 0::2] = -OMEGA * y[:, 1::2]
    k[:, 1::2] = OMEGA * y[:, 0::2]
    return k


def _start():
    return np.random.default_rng(5).standard_normal(SHAPE).astype(np.float32)


@pytest.mark.parametrize("method", ["euler", "rk4", "bosh3", "dopri5"])
def test_ode_loop_bookkeeping_matches_the_restatement(method, monkeypatch):
    _cpu_device_calls(monkeypatch)
    times, y0 = OO.linspace(6), _start()
    want, ws = OO.solve(OO.rotation_f(OMEGA), y0, times, method, rtol=1e-4, atol=1e-4)
    got, gs = ode.ode_loop(_f32, torch.from_numpy(y0), times, None, method=method, rtol=1e-4, atol=1e-4)
    assert gs["evals"] == ws["evals"] and gs["accepted"] == ws["accepted"] and gs["rejected"] == ws["rejected"]
    stages = ode.TABLEAUS[method].stages
    if ode.TABLEAUS[method].adaptive:
        assert gs["evals"] == 1 + (stages - 1) * (gs["accepted"] + gs["rejected"]) and gs["times"][-1] == 1.0
        assert len(gs["times"]) == gs["accepted"] and gs["times"] == sorted(gs["times"])
        assert np.allclose(gs["times"], ws["times"], rtol=1e-3)
    else:
        assert gs["evals"] == stages * 5 and gs["times"] == times[1:]
    assert np.abs(got.numpy() - want).max() < 1e-5


def test_max_steps_raises(monkeypatch):
    """From first_step = 1e-3 with tolerances nothing meets the first four attempts are rejected (0.2 each): max_steps = 4 raises at the fifth."""
    _cpu_device_calls(monkeypatch)
    calls = []

    def f(t, y):
        calls.append(t)
        return _f32(t, y)
    with pytest.raises(RuntimeError, match="max_steps = 4"):
        ode.ode_loop(f, torch.from_numpy(_start()), [0.0, 1.0], None, method="dopri5", rtol=0.0, atol=1e-300, first_step=1e-3, max_steps=4)
    assert len(calls) == 1 + 6 * 4


def test_a_non_finite_ratio_is_a_rejection(monkeypatch):
    """f returns NaN beyond t = 0.5: the steps that reach past it are rejected and shrink by 0.2 until max_steps."""
    _cpu_device_calls(monkeypatch)

    def f(t, y):
        return _f32(t, y) * (math.nan if t > 0.5 else 1.0)
    with pytest.raises(RuntimeError):
        ode.ode_loop(f, torch.from_numpy(_start()), [0.0, 1.0], None, method="bosh3", rtol=1e-2, atol=1e-2, first_step=0.25, max_steps=40)


def test_adaptive_methods_refuse_a_known_region():
    x = torch.zeros(SHAPE)
    for method in ("bosh3", "dopri5"):
        with pytest.raises(ValueError, match="known"):
            ode.ode_loop(_f32, x, [0.0, 1.0], None, method=method, keep_region=(x, torch.ones(5)))


def test_convergence_slopes_of_the_restatement_are_printed():
    y0, omega = _start(), 2.0
    exact = OO.rotation_exact(y0, omega, 1.0)
    for method in ("euler", "midpoint", "rk4", "bosh3", "dopri5"):
        errs = []
        for n in (8, 16, 32):
            times = [i / n for i in range(n + 1)]
            if ode.TABLEAUS[method].adaptive:                # the pair's higher-order solution on the fixed grid
                y = OO.fixed_grid(OO.rotation_f(omega), y0, times, method)[0]
            else:
                y = OO.solve(OO.rotation_f(omega), y0, times, method)[0]
            errs.append(np.abs(y - exact).max())
        slopes = [math.log2(errs[i] / errs[i + 1]) for i in range(2)]
        print(f"{method}: max error at 8, 16, 32 steps = {errs[0]:.3e}, {errs[1]:.3e}, {errs[2]:.3e}; slopes {slopes[0]:.2f}, {slopes[1]:.2f} "
              f"(order {ode.TABLEAUS[method].order})")


# ---- the public keywords -------------------------------------------------------------------------------------------------------------------------
SOLVER_KW = [("method", "midpoint"), ("rtol", 1e-5), ("atol", 1e-5), ("first_step", None), ("max_steps", 1000)]


def test_the_samplers_take_the_solver_keywords():
    for fn in (RectifiedFlowOsuFusionDiT.sample, FlowOsuFusion.sample_masked):
        params = inspect.signature(fn).parameters
        assert [(k, params[k].default) for k, _ in SOLVER_KW] == SOLVER_KW and list(params)[-5:] == [k for k, _ in SOLVER_KW]
    assert list(inspect.signature(FlowOsuFusion.sample).parameters)[1:] == ["a", "c", "x", "cond_scale"]       # the reference's signature stays
    sig = inspect.signature(ode.ode_loop)
    assert list(sig.parameters) == ["f", "x", "times", "ones", "method", "rtol", "atol", "first_step", "max_steps", "keep_region"]


# ---- the C surface -------------------------------------------------------------------------------------------------------------------------------
def test_capi_rk_error_is_declared_bound_and_exported():
    decls = _lib.read_header()[0]
    P, L, I = c_void_p, c_long, c_int
    assert "osuf_rk_error" in decls, "osuf_rk_error is not declared in include/osufusion_hip.h"
    ret, params = decls["osuf_rk_error"]
    assert ret == "int" and [p.split()[-1].lstrip("*") for p in params] == ["y0", "y1", "k", "e", "S", "step", "ws", "ratio", "B", "per_sample", "stream"]
    assert _lib.SIGNATURES["osuf_rk_error"] == [P, P, P, P, I, P, P, P, I, L, P]
    assert _lib.SIGNATURES["osuf_rk_error_workspace_bytes"] == [I, L]
    lib = _lib.load()
    assert hasattr(lib, "osuf_rk_error") and lib.osuf_rk_error_workspace_bytes.restype is c_long


def test_capi_rk_error_workspace_bytes():
    """One fp64 sum per 4096-element chunk per sample."""
    ws = _lib.load().osuf_rk_error_workspace_bytes
    assert ws(1, 1) == 8 and ws(1, 4096) == 8 and ws(1, 4097) == 16 and ws(3, 8196) == 3 * 3 * 8 and ws(16, 6 * 8192) == 16 * 12 * 8
    assert ws(0, 10) == 0 and ws(2, 0) == 0 and ws(-1, 10) == 0 and ws(2, 3 << 31) == 2 * ((3 << 31) // 4096) * 8


def test_capi_rk_error_validates_its_arguments_on_the_host():
    """Every call returns -1 before a launch: the device "pointers" are never dereferenced."""
    lib = _lib.load()
    buf = 4096

    def call(S=3, k=(buf, buf, buf), e=(0.5, -0.25, -0.25), step=(0.1, 1e-5, 1e-5), **kw):
        a = dict(y0=buf, y1=buf, ws=buf, ratio=buf, B=2, n=54)
        a.update(kw)
        ks = (ctypes.c_void_p * 7)(*k) if k is not None else None
        es = (ctypes.c_double * 7)(*e) if e is not None else None
        st = (ctypes.c_double * 3)(*step) if step is not None else None
        return lib.osuf_rk_error(a["y0"], a["y1"], ks, es, S, st, a["ws"], a["ratio"], a["B"], a["n"], None)
    nan, inf = math.nan, math.inf
    for kw in (dict(y0=None), dict(y1=None), dict(k=None), dict(e=None), dict(step=None), dict(ws=None), dict(ratio=None), dict(S=0), dict(S=8),
               dict(S=-1), dict(B=0), dict(B=-2), dict(n=0), dict(n=-1), dict(k=(buf, None, buf)), dict(e=(0.5, nan, 0.0)),
               dict(step=(nan, 1e-5, 1e-5)), dict(step=(inf, 1e-5, 1e-5)), dict(step=(0.1, nan, 1e-5)), dict(step=(0.1, 1e-5, inf)),
               dict(step=(0.1, -1e-5, 1e-5)), dict(step=(0.1, 1e-5, -1e-5)), dict(step=(0.1, 0.0, 0.0)), dict(ws=buf + 4)):
        assert call(**kw) == -1, kw


def test_a_one_point_grid_integrates_nothing():
    """sampling_timesteps = 1: linspace(0, 1, 1) = [0].  The fixed-grid loops take no step; the adaptive ones return the state too, without
    an evaluation."""
    x = torch.from_numpy(_start())
    for method in ("euler", "rk4", "bosh3", "dopri5"):
        out, st = ode.ode_loop(_f32, x, OO.linspace(1), None, method=method)
        assert out is x and st["evals"] == 0 and st["accepted"] == 0 and st["rejected"] == 0 and st["times"] == []
