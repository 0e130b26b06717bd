"""fp64 numpy oracle for post-hoc EMA (osufusion_amd/posthoc_ema.py), written from the recurrence alone: nothing here imports the module.

A power track of exponent gamma runs  e_k = e_{k-1} + (1 - beta_k)(theta_k - e_{k-1}),  beta_k = (1 - 1/k)^(gamma+1)  (beta_1 = 0: the track
starts as theta_1).  Everything below is that loop, in the literal form, on whatever theta it is given.
"""
import numpy as np

SEED, DIM, T, EVERY = 20240612, 64, 2000, 100
SIGMA_STORED, SIGMA_TARGET = (0.05, 0.10), 0.075


def beta(gamma, k):
    return (1.0 - 1.0 / k) ** (gamma + 1.0)


def run_track(theta, gamma, keep=None):
    """theta: (T, ...) fp64, step k = row k-1.  Returns the track after the last step, or {k: track after step k} for k in `keep`."""
    e = np.zeros_like(theta[0])
    kept = {}
    for k in range(1, len(theta) + 1):
        e = e + (1.0 - beta(gamma, k)) * (theta[k - 1] - e)
        if keep is not None and k in keep:
            kept[k] = e.copy()
    return e if keep is None else kept


def recurrence_weights(gamma, t):
    """The weight the track puts on each of steps 1..t, read off the recurrence run on one-hot theta (theta_k = unit vector k)."""
    return run_track(np.eye(t), gamma)


def brute_gram(ta, ga, tb, gb):
    ca, cb = recurrence_weights(ga, ta), recurrence_weights(gb, tb)
    m = min(ta, tb)
    return float(np.dot(ca[:m], cb[:m]))


def random_walk(seed=SEED, dim=DIM, steps=T):
    rng = np.random.default_rng(seed)
    return np.cumsum(rng.standard_normal((steps, dim)), axis=0)


def end_to_end(gammas_stored, gamma_target, seed=SEED):
    """(theta, snapshots, target): snapshots[s] = (G, DIM) the stored tracks after step s (every EVERY steps), target = the track of
    gamma_target after step T, computed directly."""
    theta = random_walk(seed)
    keep = set(range(EVERY, T + 1, EVERY))
    per_gamma = [run_track(theta, g, keep) for g in gammas_stored]
    snapshots = {s: np.stack([pg[s] for pg in per_gamma]) for s in sorted(keep)}
    return theta, snapshots, run_track(theta, gamma_target)
