#!/usr/bin/env python3
"""Golden signals of the beatmap encoder.  Runs ONLY in the build container, next to the reference:

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=/path/to/reference:. python3 tests/golden/make_encode_golden.py

It imports the reference's osu_fusion.library.osu (nothing is copied) and records, for every fixture under tests/golden/encode/,
encode_beatmap(Beatmap(file), frame_times) in fp64 with frame_times = arange(n) * 176 / 22050 * 1000 and n = the frames up to 600 ms
past the last object, into tests/golden/encode_cases.npz (key = the fixture's stem; `<stem>/uses_stand_in` = 0 or 1).

The reference's sliders.py imports the `bezier` package, which is not installed.  A small stand-in `Curve` is put into sys.modules
before the import, written from the package's documented behaviour: `Curve.from_nodes(nodes)` (nodes: 2 x (degree + 1), one column per
control point), `.nodes`, `.length` (scipy.integrate.quad of the norm of the hodograph over [0, 1], as the package's
compute_length does), `.evaluate(s)` -> 2 x 1 and `.evaluate_hodograph(s)` -> 2 x 1.  The stand-in counts how often it is constructed:

    PINNED TO THE REFERENCE ITSELF (the stand-in is never constructed):  circles, basic, edge
    PINNED ONLY UP TO THE STAND-IN (Bezier sliders):                     sliders

The script asserts that list.
"""
from __future__ import annotations

import sys
import types
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
NEVER_TOUCH_STAND_IN = ("basic", "circles", "edge")


class Curve:
    constructed = 0

    def __init__(self, nodes: np.ndarray) -> None:
        Curve.constructed += 1
        self.nodes = np.asarray(nodes, dtype=np.float64)
        self.degree = self.nodes.shape[1] - 1
        self._length = None

    @classmethod
    def from_nodes(cls, nodes) -> "Curve":
        return cls(nodes)

    def evaluate(self, s: float) -> np.ndarray:
        return _evaluate(self.nodes, float(s))

    def evaluate_hodograph(self, s: float) -> np.ndarray:
        first_deriv = self.nodes[:, 1:] - self.nodes[:, :-1]
        return self.degree * _evaluate(first_deriv, float(s))

    @property
    def length(self) -> float:
        if self._length is None:
            from scipy.integrate import quad
            if self.degree == 1:
                self._length = float(np.linalg.norm(self.nodes[:, 1] - self.nodes[:, 0]))
            else:
                first_deriv = self.degree * (self.nodes[:, 1:] - self.nodes[:, :-1])
                self._length = quad(lambda s: float(np.linalg.norm(_evaluate(first_deriv, s))), 0.0, 1.0)[0]
        return self._length


def _evaluate(nodes: np.ndarray, s: float) -> np.ndarray:
    """Barycentric evaluation with weights (1 - s, s): a Horner-like pass that carries the binomial coefficient and the power of s."""
    degree = nodes.shape[1] - 1
    lambda1, lambda2 = 1.0 - s, s
    result = lambda1 * nodes[:, [0]]
    if degree == 0:
        return nodes[:, [0]].copy()
    binom_val, lambda2_pow = 1.0, 1.0
    for index in range(1, degree):
        lambda2_pow *= lambda2
        binom_val = (binom_val * (degree - index + 1)) / index
        result = result + binom_val * lambda2_pow * nodes[:, [index]]
        result = result * lambda1
    return result + lambda2 * lambda2_pow * nodes[:, [degree]]


def main() -> None:
    stand_in = types.ModuleType("bezier")
    stand_in.Curve = Curve
    sys.modules["bezier"] = stand_in
    from osu_fusion.library.osu.beatmap import Beatmap               # reference, PYTHONPATH
    from osu_fusion.library.osu.data.encode import encode_beatmap

    arrays = {}
    for path in sorted((HERE / "encode").glob("*.osu")):
        before = Curve.constructed
        beatmap = Beatmap(path)
        last = max(ho.end_time() for ho in beatmap.hit_objects)
        n = int((last + 600) * 22050 / 176 / 1000) + 1
        frame_times = np.arange(n, dtype=np.float64) * 176 / 22050 * 1000
        x = encode_beatmap(beatmap, frame_times)
        assert x.shape == (6, n) and np.isfinite(x).all(), path.name
        used = Curve.constructed > before
        assert used == (path.stem not in NEVER_TOUCH_STAND_IN), (path.name, used)
        arrays[path.stem] = x
        arrays[f"{path.stem}/uses_stand_in"] = np.array(int(used))
        print(f"{path.name}: {n} frames, stand-in {'used' if used else 'never constructed'}")
    fn = HERE / "encode_cases.npz"
    np.savez_compressed(fn, **arrays)
    print(f"wrote {fn.name} ({fn.stat().st_size / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
