"""Post-hoc EMA (EDM2, Karras et al. 2024, section 3.2): any power-function averaging profile rebuilt from stored snapshots of a few.

Train with two or more `EMAConfig(kind="power", ...)` tracks, let `Trainer(..., ema_snapshots=SnapshotConfig(dir, every))` store them every
so often, and afterwards obtain the average for another sigma_rel, or for an earlier end point, as the linear combination of the stored
snapshots whose averaging profile is closest (least squares) to the wanted one.

Host side, all fp64 numpy: `profile_coeffs` (the weights a track puts on the optimizer steps), `gram` (inner products of profiles),
`solve_weights` (the least-squares weights), `SnapshotStore` (the files).  Device side: `reconstruct` streams the snapshots through
ops.lincomb (osuf_lincomb), at most eight sources per launch, one fp64 accumulator carried between launches -- the weights alternate in
sign and exceed 1 in magnitude, so an fp32 running sum would lose the result to cancellation.

Times.  A profile's length t is the number of optimizer steps its track has seen (FusedAdamW.ema_step), not the optimizer's step count: a
run resumed from a checkpoint without EMA state restarts its tracks as copies of the loaded weights, and snapshots from before and after
such a restart do not belong to one profile.  Every file records both numbers; a store whose files disagree on step - ema_step is refused.
"""
from __future__ import annotations

import re
from dataclasses import dataclass
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from .ema import sigma_rel_to_gamma

_CHUNK = 1 << 20


def _one_minus_beta(gamma: float, j: np.ndarray) -> np.ndarray:
    """1 - beta_j = 1 - (1 - 1/j)^(gamma+1) without the cancellation of the literal form at large j; exactly 1 at j = 1."""
    j = np.asarray(j, dtype=np.float64)
    out = np.ones_like(j)
    later = j > 1.0
    out[later] = -np.expm1((gamma + 1.0) * np.log1p(-1.0 / j[later]))
    return out


def profile_coeffs(gamma: float, t: int) -> np.ndarray:
    """c[j-1], j = 1..t: the weight that the power track of exponent `gamma` (ema.ema_beta: beta_1 = 0, beta_k = (1 - 1/k)^(gamma+1)),
    after optimizer step t, puts on the weights of optimizer step j:  c_t(j) = (1 - beta_j) (j/t)^(gamma+1).  They sum to 1."""
    if t < 1:
        raise ValueError(f"a profile spans at least one optimizer step, got t = {t}")
    j = np.arange(1, int(t) + 1, dtype=np.float64)
    return _one_minus_beta(float(gamma), j) * (j / float(t)) ** (float(gamma) + 1.0)


def _prefix_inner(ga: float, gb: float, ms: np.ndarray) -> np.ndarray:
    """S(m) = sum_{j <= m} (1 - beta^a_j)(1 - beta^b_j) (j/m)^(ga+gb+2) at the ascending step counts `ms`: one running sum over j,
    re-normalised to the current m at every requested point, so no term exceeds 1 and the sum is never below its last term."""
    p = ga + gb + 2.0
    out = np.empty(len(ms), dtype=np.float64)
    run, prev = 0.0, 0
    for i, m in enumerate(ms):
        m = int(m)
        run *= (prev / m) ** p if prev else 0.0
        for lo in range(prev + 1, m + 1, _CHUNK):
            j = np.arange(lo, min(lo + _CHUNK, m + 1), dtype=np.float64)
            run += float(np.sum(_one_minus_beta(ga, j) * _one_minus_beta(gb, j) * (j / m) ** p))
        out[i], prev = run, m
    return out


def _items(ts, gammas) -> Tuple[np.ndarray, np.ndarray]:
    ts, gammas = np.atleast_1d(np.asarray(ts)), np.atleast_1d(np.asarray(gammas, dtype=np.float64))
    if ts.shape != gammas.shape or ts.ndim != 1:
        raise ValueError("ts and gammas are two 1-D sequences of one length: one (t, gamma) per profile")
    if not (np.all(ts >= 1) and np.all(ts == np.floor(ts))):
        raise ValueError("profile lengths are whole numbers of optimizer steps >= 1")
    if not np.all(gammas >= 0):
        raise ValueError("power exponents must be >= 0")
    return ts.astype(np.int64), gammas


def gram(ts_a, gammas_a, ts_b, gammas_b, profile: str = "discrete") -> np.ndarray:
    """(len(a), len(b)) inner products of the averaging profiles (t_a[i], gamma_a[i]) and (t_b[j], gamma_b[j]).

    "discrete":   sum_j c_a(j) c_b(j) of the exact profiles `profile_coeffs` (the shorter one zero-padded).  With m = min(t_a, t_b) this
                  is S(m) (m/t_a)^(ga+1) (m/t_b)^(gb+1) with S of `_prefix_inner`: O(T) per pair of exponents, every factor in (0, 1].
    "continuous": EDM2 algorithm 3's closed form for the continuous-time profiles (the limit of large t): a cross-check, and the right
                  choice for stores written by trainers that run the continuous schedule."""
    ta, ga = _items(ts_a, gammas_a)
    tb, gb = _items(ts_b, gammas_b)
    if profile == "continuous":
        TA, TB = ta[:, None].astype(np.float64), tb[None, :].astype(np.float64)
        GA, GB = ga[:, None], gb[None, :]
        e = np.where(TA < TB, GB, -GA)
        return (GA + 1.0) * (GB + 1.0) * (TA / TB) ** e / ((GA + GB + 1.0) * np.maximum(TA, TB))
    if profile != "discrete":
        raise ValueError(f"profile is 'discrete' or 'continuous', got {profile!r}")
    out = np.empty((len(ta), len(tb)), dtype=np.float64)
    M = np.minimum(ta[:, None], tb[None, :])
    # one prefix sum per unordered pair of exponents, shared by (ga, gb) and (gb, ga): the entry does not depend on which side it is on
    lo, hi = np.minimum(ga[:, None], gb[None, :]), np.maximum(ga[:, None], gb[None, :])
    for g0, g1 in sorted({(float(a), float(b)) for a, b in zip(lo.ravel(), hi.ravel())}):
        sel = (lo == g0) & (hi == g1)
        ms = np.unique(M[sel])
        S = dict(zip(ms.tolist(), _prefix_inner(g0, g1, ms)))
        for i, j in zip(*np.nonzero(sel)):
            m = int(M[i, j])
            fa, fb = (m / float(ta[i])) ** (ga[i] + 1.0), (m / float(tb[j])) ** (gb[j] + 1.0)
            out[i, j] = S[m] * (fa * fb)
    return out


def solve_weights(ts, gammas, t_r: int, gamma_r: float, profile: str = "discrete") -> np.ndarray:
    """x minimising || sum_i x_i profile(t_i, gamma_i) - profile(t_r, gamma_r) ||: solve(A, b), A the Gram matrix of the stored profiles,
    b their inner products with the target.  ValueError when A is singular to working precision (cond(A) > 1 / eps: duplicate profiles)."""
    ts, gammas = _items(ts, gammas)
    tr, gr = _items([t_r], [gamma_r])
    # one call over the stored profiles and the target: a target equal to a stored profile then gives that column of A bit for bit
    G = gram(np.concatenate([ts, tr]), np.concatenate([gammas, gr]), np.concatenate([ts, tr]), np.concatenate([gammas, gr]), profile)
    A, b = G[:-1, :-1], G[:-1, -1]
    cond = np.linalg.cond(A)
    if not np.isfinite(cond) or cond > 1.0 / np.finfo(np.float64).eps:
        raise ValueError(f"the stored profiles are linearly dependent to working precision (cond = {cond:.3e}): duplicate snapshots or exponents")
    return np.linalg.solve(A, b)


# ---- the files ------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class SnapshotConfig:
    """Trainer's `ema_snapshots` argument: store every power track after each optimizer step k with k % every == 0."""
    dir: Union[str, Path]
    every: int

    def __post_init__(self) -> None:
        if int(self.every) < 1:
            raise ValueError(f"ema_snapshots.every must be >= 1, got {self.every}")


class SnapshotStore:
    """One file per snapshot step, `snapshot_<step, 10 digits>.pt` (torch.save of plain containers and one tensor):
        step, ema_step   the optimizer's step count and the number of steps the tracks had seen (the profile length)
        gammas           the power exponents of the stored tracks
        names, shapes    the trainable parameters in model.named_parameters() order
        tracks           (G, n) fp32: row g = track g, the parameters flattened and concatenated in that order (no padding)
    That order is not the trainer's flat buffer order, which follows the observed gradient-completion order and may change."""

    _NAME = re.compile(r"^snapshot_(\d{10})\.pt$")

    def __init__(self, dir: Union[str, Path]) -> None:
        self.dir = Path(dir)

    def path(self, step: int) -> Path:
        return self.dir / f"snapshot_{int(step):010d}.pt"

    def write(self, step: int, gammas: Sequence[float], names: Sequence[str], shapes: Sequence[Sequence[int]], tracks: torch.Tensor,
              ema_step: Optional[int] = None) -> Path:
        gammas, names, shapes = [float(g) for g in gammas], [str(k) for k in names], [[int(d) for d in s] for s in shapes]
        n = sum(int(np.prod(s, dtype=np.int64)) for s in shapes)
        if tracks.dtype != torch.float32 or tuple(tracks.shape) != (len(gammas), n) or len(names) != len(shapes):
            raise ValueError(f"tracks must be fp32 of shape ({len(gammas)}, {n}) for these gammas and shapes, got {tracks.dtype} {tuple(tracks.shape)}")
        if step < 1:
            raise ValueError(f"snapshots are taken after an optimizer step (step >= 1), got {step}")
        self.dir.mkdir(parents=True, exist_ok=True)
        path = self.path(step)
        tmp = path.with_suffix(".tmp")
        torch.save({"step": int(step), "ema_step": int(step if ema_step is None else ema_step), "gammas": gammas, "names": names,
                    "shapes": shapes, "tracks": tracks.detach().contiguous().cpu()}, tmp)
        tmp.replace(path)                                   # a reader never sees half a file
        return path

    def list(self) -> List[int]:
        """The stored steps, ascending."""
        if not self.dir.is_dir():
            return []
        return sorted(int(m.group(1)) for m in (self._NAME.match(p.name) for p in self.dir.iterdir()) if m)

    def load(self, step: int, device: Union[str, torch.device] = "cpu") -> dict:
        d = torch.load(self.path(step), map_location="cpu", weights_only=True)
        if d["step"] != int(step):
            raise ValueError(f"{self.path(step).name} says it holds step {d['step']}")
        d["tracks"] = d["tracks"].to(device)
        return d

    def check(self) -> dict:
        """ValueError unless every file names the same parameters, shapes and exponents and all come from one run of the tracks (one
        value of step - ema_step).  Returns {"steps", "ema_steps", "gammas", "names", "shapes"}."""
        steps = self.list()
        if not steps:
            raise ValueError(f"no snapshots in {self.dir}")
        first, ema_steps = None, []
        for s in steps:
            d = self.load(s)
            if first is None:
                first = d
            for key in ("names", "shapes", "gammas"):
                if d[key] != first[key]:
                    raise ValueError(f"{self.path(s).name} and {self.path(steps[0]).name} disagree on {key}")
            if d["step"] - d["ema_step"] != first["step"] - first["ema_step"] or d["ema_step"] < 1:
                raise ValueError(f"{self.path(s).name}: the tracks had seen {d['ema_step']} steps at step {d['step']}, "
                                 f"{first['ema_step']} at step {first['step']}: they were restarted in between, the snapshots are not one profile")
            ema_steps.append(d["ema_step"])
            del d
        return {"steps": steps, "ema_steps": ema_steps, "gammas": first["gammas"], "names": first["names"], "shapes": first["shapes"]}


def _as_store(store) -> SnapshotStore:
    return store if isinstance(store, SnapshotStore) else SnapshotStore(store)


def reconstruct(store, sigma_rel: Optional[float] = None, gamma: Optional[float] = None, at_step: Optional[int] = None,
                device: Union[str, torch.device] = "cuda", profile: str = "discrete", max_resident: int = 8
                ) -> Tuple[Dict[str, torch.Tensor], np.ndarray]:
    """The power-function average of exponent `gamma` (or of relative width `sigma_rel`) as it would stand after optimizer step `at_step`
    (default: the last snapshot), as the least-squares combination of every stored track at every snapshot step <= at_step.

    Returns ({name: tensor}, weights): views of one fp32 (n,) device buffer in the store's parameter order, and the fp64 weight vector,
    snapshot-major (weights[s * G + g] multiplies track g of the s-th snapshot used).  At most min(max_resident, 8) snapshot rows are on
    the device at a time."""
    from . import ops
    if (sigma_rel is None) == (gamma is None):
        raise ValueError("reconstruct takes exactly one of sigma_rel and gamma")
    gamma_r = float(gamma) if gamma is not None else sigma_rel_to_gamma(sigma_rel)
    store = _as_store(store)
    info = store.check()
    at_step = info["steps"][-1] if at_step is None else int(at_step)
    used = [(s, e) for s, e in zip(info["steps"], info["ema_steps"]) if s <= at_step]
    offset = info["steps"][0] - info["ema_steps"][0]
    if not used or at_step - offset < 1:
        raise ValueError(f"no snapshot at or before step {at_step} (the store holds steps {info['steps'][0]} .. {info['steps'][-1]})")
    G = len(info["gammas"])
    ts = np.repeat([e for _, e in used], G)
    gs = np.tile(info["gammas"], len(used))
    weights = solve_weights(ts, gs, at_step - offset, gamma_r, profile)

    group = max(1, min(int(max_resident), ops.LINCOMB_MAX))
    n = sum(int(np.prod(s, dtype=np.int64)) for s in info["shapes"])
    dev = torch.device(device)
    out = torch.empty(n, dtype=torch.float32, device=dev)
    launches = -(-len(weights) // group)
    acc = torch.empty(n, dtype=torch.float64, device=dev) if launches > 1 else None
    pending, done = [], 0

    def flush(last: bool) -> None:
        nonlocal pending, done
        ops.lincomb([r for r, _ in pending], [w for _, w in pending], acc=acc, out=out if last else None, cont=done > 0)
        done += 1
        pending = []

    k = 0
    for s, _ in used:
        host = store.load(s)["tracks"]
        for g in range(G):
            pending.append((host[g].to(dev), weights[k]))  # a row of its own on the device: aligned, whatever n is
            k += 1
            if len(pending) == group:
                flush(last=k == len(weights))
    if pending:
        flush(last=True)
    named, o = {}, 0
    for name, shape in zip(info["names"], info["shapes"]):
        cnt = int(np.prod(shape, dtype=np.int64))
        named[name] = out[o:o + cnt].view(*shape)
        o += cnt
    return named, weights
