"""Post-hoc EMA, host side (osufusion_amd/posthoc_ema.py): profile coefficients, Gram matrices, least-squares weights and the snapshot
files, against the fp64 recurrence oracle (tests/posthoc_ema_oracle.py)."""
import itertools

import numpy as np
import pytest
import torch

from osufusion_amd.ema import EMAConfig, ema_beta, sigma_rel_to_gamma
from osufusion_amd.posthoc_ema import SnapshotConfig, SnapshotStore, gram, profile_coeffs, solve_weights
from tests import posthoc_ema_oracle as O

GAMMAS = (0.0, 6.9372, 16.9722)
EPS = 2.0 ** -52


@pytest.mark.parametrize("gamma", GAMMAS)
@pytest.mark.parametrize("t", [1, 2, 7, 500])
def test_profile_coeffs_are_the_recurrence_weights(gamma, t):
    c = profile_coeffs(gamma, t)
    assert c.dtype == np.float64 and c.shape == (t,)
    assert abs(c.sum() - 1.0) <= 1e-12
    want = O.recurrence_weights(gamma, t)
    assert np.abs(c - want).max() <= 1e-12
    # the oracle's decay is the trainer's
    cfg = EMAConfig(kind="power", gamma=gamma)
    assert all(ema_beta(cfg, k) == O.beta(gamma, k) for k in (1, 2, 3, t))


def test_discrete_gram_is_the_inner_product_of_the_profiles():
    items = list(itertools.product((1, 3, 10, 250), GAMMAS))
    ts, gs = [t for t, _ in items], [g for _, g in items]
    A = gram(ts, gs, ts, gs)
    assert A.shape == (12, 12) and np.array_equal(A, A.T)
    worst = 0.0
    for (i, (ta, ga)), (j, (tb, gb)) in itertools.product(enumerate(items), repeat=2):
        want = O.brute_gram(ta, ga, tb, gb)
        worst = max(worst, abs(A[i, j] - want) / want)
    print(f"discrete gram vs brute force: worst relative error {worst:.3e}")
    assert worst < 1e-10
    # a rectangular call gives the same entries
    B = gram(ts[:5], gs[:5], ts[3:], gs[3:])
    assert np.abs(B - A[:5, 3:]).max() <= 1e-15 * np.abs(A).max()


def test_discrete_gram_does_not_overflow_at_long_runs():
    G = gram([1, 10 ** 7], [20.0, 20.0], [1, 10 ** 7], [20.0, 20.0])
    assert np.isfinite(G).all() and (G > 0).all(), G


def test_continuous_gram_approaches_the_discrete_one():
    gs = [6.9372, 16.9722]
    gaps = []
    for t in (10 ** 2, 10 ** 5):
        ts = [t, t]
        d, c = gram(ts, gs, ts, gs), gram(ts, gs, ts, gs, profile="continuous")
        gaps.append(np.abs(c / d - 1.0).max())
    print(f"continuous vs discrete gram, relative gap: t = 1e2 {gaps[0]:.3e}, t = 1e5 {gaps[1]:.3e}")
    assert gaps[1] < gaps[0]
    with pytest.raises(ValueError):
        gram([1], [0.0], [1], [0.0], profile="other")


def _store_items():
    g = [sigma_rel_to_gamma(s) for s in O.SIGMA_STORED]
    steps = np.arange(O.EVERY, O.T + 1, O.EVERY)
    return np.repeat(steps, len(g)), np.tile(g, len(steps))


def test_a_stored_profile_as_target_gives_its_unit_vector():
    ts, gs = _store_items()
    bound = np.linalg.cond(gram(ts, gs, ts, gs)) * EPS * 8
    for i in (0, 1, 17, len(ts) - 1):
        x = solve_weights(ts, gs, int(ts[i]), float(gs[i]))
        e = np.zeros(len(ts))
        e[i] = 1.0
        err = np.abs(x - e).max()
        print(f"unit vector {i}: error {err:.3e}, bound {bound:.3e}")
        assert err <= bound


def test_off_grid_target_meets_the_optimum_condition():
    """At the least-squares optimum the residual profile sum_i x_i c_i - c_r is orthogonal to every stored profile: A x = b."""
    ts, gs = _store_items()
    t_r, g_r = 1950, sigma_rel_to_gamma(O.SIGMA_TARGET)
    x = solve_weights(ts, gs, t_r, g_r)
    A, b = gram(ts, gs, ts, gs), gram(ts, gs, [t_r], [g_r])[:, 0]
    # |A x - b| of a backward-stable solve is eps-small against |A| |x|; the cond-scaled bound of the issue is taken relative to it
    resid, scale = np.abs(A @ x - b).max(), np.abs(A).max() * np.abs(x).max()
    bound = np.linalg.cond(A) * EPS * 8
    print(f"optimum condition: |Ax - b| = {resid:.3e} (relative {resid / scale:.3e}), bound {bound:.3e}")
    assert resid <= bound and resid / scale <= bound
    # explicitly: the residual profile against each stored one, from the profiles themselves
    r = -np.pad(profile_coeffs(g_r, t_r), (0, O.T - t_r))
    for xi, t, g in zip(x, ts, gs):
        r[:t] += xi * profile_coeffs(g, int(t))
    dots = [abs(np.dot(r[:t], profile_coeffs(g, int(t)))) for t, g in zip(ts, gs)]
    assert max(dots) <= bound


def test_duplicate_profiles_are_refused():
    ts, gs = _store_items()
    with pytest.raises(ValueError, match="linearly dependent"):
        solve_weights(np.append(ts, ts[3]), np.append(gs, gs[3]), O.T, 10.0)


def test_oracle_end_to_end_reconstruction_beats_both_stored_tracks():
    g_stored = [sigma_rel_to_gamma(s) for s in O.SIGMA_STORED]
    g_target = sigma_rel_to_gamma(O.SIGMA_TARGET)
    _, snaps, target = O.end_to_end(g_stored, g_target)
    steps = sorted(snaps)
    assert steps == list(range(O.EVERY, O.T + 1, O.EVERY))
    ts, gs = np.repeat(steps, 2), np.tile(g_stored, len(steps))
    x = solve_weights(ts, gs, O.T, g_target)
    rows = np.concatenate([snaps[s] for s in steps])          # snapshot-major, as the weights
    recon = x @ rows
    d_recon = np.linalg.norm(recon - target)
    d_tracks = [np.linalg.norm(snaps[O.T][g] - target) for g in range(2)]
    print(f"post-hoc reconstruction: distance {d_recon:.4e}; stored tracks {d_tracks[0]:.4e}, {d_tracks[1]:.4e}; "
          f"ratio to the nearer track {d_recon / min(d_tracks):.4e}")
    assert d_recon < min(d_tracks)


def _example(G=2, seed=0):
    names, shapes = ["a.weight", "a.bias", "b.weight"], [[3, 5], [3], [2, 2, 2]]
    g = torch.Generator().manual_seed(seed)
    return [6.94, 16.97][:G], names, shapes, torch.randn(G, 26, generator=g)


def test_snapshot_store_round_trip_is_bit_exact(tmp_path):
    store = SnapshotStore(tmp_path / "snaps")
    assert store.list() == []
    gammas, names, shapes, tracks = _example()
    tracks[0, 0], tracks[1, 3] = float("nan"), -0.0
    store.write(20, gammas, names, shapes, tracks, ema_step=20)
    store.write(10, gammas, names, shapes, tracks * 2, ema_step=10)
    assert store.list() == [10, 20]
    assert sorted(p.name for p in (tmp_path / "snaps").iterdir()) == ["snapshot_0000000010.pt", "snapshot_0000000020.pt"]
    d = store.load(20)
    assert d["step"] == 20 and d["ema_step"] == 20 and d["gammas"] == gammas and d["names"] == names and d["shapes"] == shapes
    assert d["tracks"].dtype == torch.float32 and torch.equal(d["tracks"].view(torch.int32), tracks.view(torch.int32))
    info = store.check()
    assert info["steps"] == [10, 20] and info["ema_steps"] == [10, 20] and info["names"] == names
    with pytest.raises(ValueError):
        store.write(30, gammas, names, shapes, tracks[:, :-1])
    with pytest.raises(ValueError):
        store.write(30, gammas, names, shapes, tracks.double())


@pytest.mark.parametrize("what", ["names", "shapes", "gammas", "restart"])
def test_snapshot_store_refuses_files_that_disagree(tmp_path, what):
    store = SnapshotStore(tmp_path)
    gammas, names, shapes, tracks = _example()
    store.write(10, gammas, names, shapes, tracks)
    if what == "names":
        store.write(20, gammas, ["x.weight"] + names[1:], shapes, tracks)
    elif what == "shapes":
        store.write(20, gammas, names, [[5, 3]] + shapes[1:], tracks)
    elif what == "gammas":
        store.write(20, [gammas[0], 3.0], names, shapes, tracks)
    else:
        store.write(20, gammas, names, shapes, tracks, ema_step=5)          # the tracks were restarted at step 15
    with pytest.raises(ValueError):
        store.check()
    with pytest.raises(ValueError):
        SnapshotStore(tmp_path / "empty").check()


def test_snapshot_config():
    assert SnapshotConfig("d", 3).every == 3
    with pytest.raises(ValueError):
        SnapshotConfig("d", 0)
