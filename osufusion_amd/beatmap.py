"""``.osu`` text -> hit objects: host-side restatement of ``osu_fusion/library/osu/beatmap.py`` (section parser, timing points, hit
objects), ``hit_objects.py`` (Circle / Spinner / Slider) and ``sliders.py`` (Line / Perfect / Bezier and the decision tree that picks
one from the control points), numpy only.  The objects are what tests/encode_oracle.py walks and what osufusion_amd/encode.py packs into
the device tables of osuf_encode_signals.

The reference's quirks are kept: inherited timing points in front of the first uninherited one are dropped, a slider's timing point is
looked up at t, t - 1 and t + 1, a three-point slider becomes a Line, a Bezier or a Perfect arc by the reference's tests (circumradius
above 320 and forward-going -> Bezier), every slider position is rounded half-to-even to whole osu!pixels, ``end_time`` truncates.
One thing is wider than the reference: an integer field written with a decimal point ("96.0", "1234.56") is accepted and truncated
towards zero, because that is how ``decode.decode_beatmap`` writes times and control points (the reference's ``int(str)`` raises there).

The reference measures Bezier segments with the ``bezier`` package (``Curve.length``: QUADPACK on ||B'(s)|| over [0, 1]) and evaluates
them with the same package; neither is available here, so both are restated from their definitions (`bezier_length`, `bezier_point`):
**restated and unpinned**, DESIGN section 6e.
"""
from __future__ import annotations

import bisect
import re
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

CX, CY = 256, 192                                                   # spinner centre / empty-map cursor
CIRCLE, SPINNER, LINE, PERFECT, BEZIER = range(5)                   # `kind` of a hit object, as the device table stores it


def _int(s: str) -> int:
    try:
        return int(s)
    except ValueError:
        return int(float(s))


class TimingPoint:
    def __init__(self, t: int, beat_length: Optional[float], slider_multiplier: Optional[float], meter: Optional[float], kiai: Optional[bool]):
        self.t, self.beat_length, self.slider_multiplier, self.meter, self.kiai = t, beat_length, slider_multiplier, meter, kiai

    def _key(self):
        return (self.t, self.beat_length, self.slider_multiplier, self.meter, self.kiai)

    def __eq__(self, other) -> bool:
        return self._key() == other._key()

    def __repr__(self) -> str:
        return f"TimingPoint{self._key()}"


class HitObject:
    kind = -1

    def __init__(self, t: int, new_combo: bool) -> None:
        self.t, self.new_combo = t, new_combo

    def end_time(self) -> int:
        return self.t

    def start_pos(self, rounded: bool = True) -> np.ndarray:
        raise NotImplementedError

    def end_pos(self, rounded: bool = True) -> np.ndarray:
        return self.start_pos(rounded)


class Circle(HitObject):
    kind = CIRCLE

    def __init__(self, t: int, new_combo: bool, x: int, y: int) -> None:
        super().__init__(t, new_combo)
        self.x, self.y = x, y

    def start_pos(self, rounded: bool = True) -> np.ndarray:
        return np.array([self.x, self.y], dtype=np.float64)


class Spinner(HitObject):
    kind = SPINNER

    def __init__(self, t: int, new_combo: bool, u: int) -> None:
        super().__init__(t, new_combo)
        self.u = u

    def end_time(self) -> int:
        return self.u

    def start_pos(self, rounded: bool = True) -> np.ndarray:
        return np.array([CX, CY], dtype=np.float64)


class Slider(HitObject):
    """slide_duration: milliseconds of ONE slide; lerp(ts): position at the fraction ts of a slide, rounded half-to-even to whole
    pixels unless rounded=False (which only tests/encode_oracle.py's round_positions=False and the kernel's round_pos = 0 ask for)."""

    def __init__(self, t: int, beat_length: float, slider_multiplier: float, new_combo: bool, slides: int, length: float) -> None:
        super().__init__(t, new_combo)
        self.slides, self.length, self.slider_multiplier = slides, length, slider_multiplier
        self.slide_duration = length / (slider_multiplier * 100) * beat_length

    def end_time(self) -> int:
        return int(self.t + self.slide_duration * self.slides)

    def point(self, ts: float) -> np.ndarray:
        raise NotImplementedError

    def lerp(self, ts: float, rounded: bool = True) -> np.ndarray:
        p = self.point(float(ts))
        return p.round(0) if rounded else p

    def start_pos(self, rounded: bool = True) -> np.ndarray:
        return self.lerp(0.0, rounded)

    def end_pos(self, rounded: bool = True) -> np.ndarray:
        return self.lerp(float(self.slides % 2), rounded)


class Line(Slider):
    kind = LINE

    def __init__(self, t, beat_length, slider_multiplier, new_combo, slides, length, start, end) -> None:
        super().__init__(t, beat_length, slider_multiplier, new_combo, slides, length)
        self.start = np.asarray(start, dtype=np.float64)
        vec = np.asarray(end, dtype=np.float64) - self.start
        self.end = self.start + vec / np.linalg.norm(vec) * length       # the path is `length` long whatever the second point says

    def point(self, ts: float) -> np.ndarray:
        return (1 - ts) * self.start + ts * self.end


class Perfect(Slider):
    kind = PERFECT

    def __init__(self, t, beat_length, slider_multiplier, new_combo, slides, length, center, radius, start, end) -> None:
        super().__init__(t, beat_length, slider_multiplier, new_combo, slides, length)
        self.center, self.radius, self.start = np.asarray(center, dtype=np.float64), float(radius), float(start)
        self.end = self.start + length / self.radius * float(np.sign(end - start))    # the arc is `length` long, in the given direction

    def point(self, ts: float) -> np.ndarray:
        theta = (1 - ts) * self.start + ts * self.end
        return self.center + self.radius * np.array([np.cos(theta), np.sin(theta)])


# ---- Bezier pieces (the `bezier` package's Curve.length / Curve.evaluate, restated) ----------------------------------------------------------
_GL_X, _GL_W = np.polynomial.legendre.leggauss(16)


def bezier_point(nodes: np.ndarray, s: float) -> np.ndarray:
    """Point at parameter s of the Bezier curve with control points nodes (n + 1, 2), by the streaming Bernstein recurrence (a Horner
    form in s / (1 - s) that needs no array): the operations and their order are what osuf_encode_signals runs per frame."""
    deg = nodes.shape[0] - 1
    l1, l2 = 1.0 - s, s
    res = nodes[0] * l1
    pw, binom = 1.0, 1.0
    for i in range(1, deg):
        pw = pw * l2
        binom = (binom * (deg - i + 1)) / i
        res = res + (binom * pw) * nodes[i]
        res = res * l1
    return res + (l2 * pw) * nodes[deg]


def _casteljau(ctrl: np.ndarray, s: np.ndarray) -> np.ndarray:
    s = s[:, None, None]
    pts = np.broadcast_to(ctrl[None], (s.shape[0],) + ctrl.shape).copy()
    while pts.shape[1] > 1:
        pts = (1.0 - s) * pts[:, :-1] + s * pts[:, 1:]
    return pts[:, 0]


def bezier_length(nodes: np.ndarray) -> float:
    """Arc length: the integral of ||B'(s)|| over [0, 1].  Degree 1: the norm.  Else composite 16-point Gauss-Legendre, the panel count
    doubled until two successive values agree to 1e-14 relative (QUADPACK's adaptive rule converges to the same integral)."""
    nodes = np.asarray(nodes, dtype=np.float64)
    deg = nodes.shape[0] - 1
    if deg == 1:
        return float(np.linalg.norm(nodes[1] - nodes[0]))
    hodo = deg * (nodes[1:] - nodes[:-1])
    prev, pieces = None, 4
    while True:
        edges = np.linspace(0.0, 1.0, pieces + 1)
        half = 0.5 * (edges[1:] - edges[:-1])
        s = (half[:, None] * _GL_X[None] + 0.5 * (edges[1:] + edges[:-1])[:, None]).reshape(-1)
        speed = np.linalg.norm(_casteljau(hodo, s), axis=1).reshape(pieces, -1)
        total = float((half * (speed @ _GL_W)).sum())
        if prev is not None and abs(total - prev) <= 1e-14 * abs(total) or pieces >= 4096:
            return total
        prev, pieces = total, pieces * 2


class Bezier(Slider):
    """segments: control-point arrays (n_i + 1, 2), the control polygon split at repeated points, plus a straight tail when the path
    is shorter than `length`; cum_t[i]: the fraction of `length` at which segment i ends (the last one forced to 1)."""
    kind = BEZIER

    def __init__(self, t, beat_length, slider_multiplier, new_combo, slides, length, control_points: Sequence[np.ndarray]) -> None:
        super().__init__(t, beat_length, slider_multiplier, new_combo, slides, length)
        pts = [np.asarray(p, dtype=np.float64) for p in control_points]
        self.control_points = pts
        pieces, first = [], 0
        for i in range(1, len(pts)):
            if (pts[i - 1] == pts[i]).all():
                pieces.append(pts[first:i])
                first = i
        pieces.append(pts[first:])
        self.segments = [np.array(p) for p in pieces if len(p) >= 2]
        lengths = [bezier_length(seg) for seg in self.segments]
        tail = self.length - sum(lengths)
        if tail > 0:
            last = self.segments[-1]
            vec = last[-1] - last[-2]
            self.segments.append(np.array([last[-1], last[-1] + vec / np.linalg.norm(vec) * tail]))
            lengths.append(bezier_length(self.segments[-1]))
        self.cum_t = np.cumsum(lengths) / self.length
        self.cum_t[-1] = 1.0

    def reparametrize(self, ts: float) -> Tuple[int, float]:
        idx = int(np.searchsorted(self.cum_t, min(1.0, max(0.0, ts))))
        lo = self.cum_t[idx - 1] if idx > 0 else 0.0
        return idx, (ts - lo) / (self.cum_t[idx] - lo)

    def point(self, ts: float) -> np.ndarray:
        idx, s = self.reparametrize(ts)
        return bezier_point(self.segments[idx], s)


def slider_from_control_points(t: int, beat_length: float, slider_multiplier: float, new_combo: bool, slides: int, length: float,
                               control_points: Sequence[Sequence[int]]) -> Slider:
    """sliders.py's from_control_points: the curve letter of the .osu line is not looked at, the point count and geometry decide."""
    pts = [np.asarray(p, dtype=np.int64) for p in control_points]
    if len(pts) < 2:
        raise ValueError(f"not enough control points: {len(pts)}")
    head = (t, beat_length, slider_multiplier, new_combo, slides, length)
    if len(pts) == 2:
        return Line(*head, pts[0], pts[1])
    if len(pts) != 3:
        return Bezier(*head, pts)
    p1, p2, p3 = pts
    if (p2 == p3).all():
        return Line(*head, p1, p3)
    u, v = p2 - p1, p3 - p1
    cross = int(u[0] * v[1] - u[1] * v[0])
    if cross == 0:                                                   # collinear: forward -> Line, doubling back -> a two-piece Bezier
        if int(u @ v) > 0:
            return Line(*head, p1, p3)
        return Bezier(*head, [p1, p2, p2, p3])
    a, b, c = (float(np.linalg.norm(d)) for d in (p3 - p2, p3 - p1, p2 - p1))
    s = (a + b + c) / 2
    r = a * b * c / 4 / np.sqrt(s * (s - a) * (s - b) * (s - c))
    if r > 320 and int((p3 - p2) @ (p2 - p1)) > 0:                   # nearly straight and forward-going
        return Bezier(*head, pts)
    b1 = a * a * (b * b + c * c - a * a)                             # barycentric weights of the circumcentre
    b2 = b * b * (a * a + c * c - b * b)
    b3 = c * c * (a * a + b * b - c * c)
    centre = np.column_stack((p1, p2, p3)).dot(np.array([b1, b2, b3]))
    centre = centre / (b1 + b2 + b3)
    start = float(np.arctan2(p1[1] - centre[1], p1[0] - centre[0]))
    end = float(np.arctan2(p3[1] - centre[1], p3[0] - centre[0]))
    if cross < 0:                                                    # clockwise: the end angle lies below the start angle
        while end > start:
            end -= 2 * np.pi
    else:
        while start > end:
            start -= 2 * np.pi
    return Perfect(*head, centre, r, start, end)


# ---- the file ---------------------------------------------------------------------------------------------------------------------------
_LIST_SECTIONS = ("Events", "TimingPoints", "HitObjects")


def parse_sections(lines: Sequence[str]) -> Dict[str, object]:
    """[Section] -> dict of `key: value` pairs, or the list of lines for Events / TimingPoints / HitObjects.  `//` lines are comments;
    an empty line ends the section (lines up to the next header are ignored)."""
    cfg: Dict[str, object] = {}
    section = None
    for line in lines:
        line = line.rstrip("\r\n")
        if line.startswith("//"):
            continue
        if line.strip() == "":
            section = None
            continue
        m = re.search(r"^\[(.*)\]$", line)
        if m is not None:
            section = m.group(1)
            cfg[section] = [] if section in _LIST_SECTIONS else {}
            continue
        if section is None:
            continue
        if section in _LIST_SECTIONS:
            cfg[section].append(line.strip())
        else:
            kv = re.search(r"^(\w*)\s?:\s?(.*)$", line)
            if kv is not None:
                cfg[section][kv.group(1)] = kv.group(2).strip()
    return cfg


class Beatmap:
    """One difficulty.  meta_only=True stops after the header fields (no timing points, no hit objects)."""

    def __init__(self, lines: Sequence[str], filename: Optional[Path] = None, meta_only: bool = False) -> None:
        self.filename = filename
        self.timing_points: List[TimingPoint] = []
        self.uninherited_timing_points: List[TimingPoint] = []
        self.hit_objects: List[HitObject] = []
        cfg = parse_sections(lines)
        general, meta, diff = cfg["General"], cfg["Metadata"], cfg["Difficulty"]
        name = general["AudioFilename"]
        self.audio_filename = (filename.parent / name) if filename is not None else Path(name)
        self.mode = int(general["Mode"])
        self.title, self.artist, self.creator, self.version = meta["Title"], meta["Artist"], meta["Creator"], meta["Version"]
        self.mapset_id = int(meta["BeatmapSetID"]) if "BeatmapSetID" in meta else None
        self.hp, self.cs, self.od = float(diff["HPDrainRate"]), float(diff["CircleSize"]), float(diff["OverallDifficulty"])
        self.ar = float(diff["ApproachRate"]) if "ApproachRate" in diff else 7
        self.slider_multiplier = float(diff["SliderMultiplier"])
        self.slider_tick_rate = float(diff["SliderTickRate"])
        self.beat_divisor = int(diff["BeatDivisor"]) if "BeatDivisor" in diff else 4
        if not meta_only:
            self._parse_timing_points(cfg["TimingPoints"])
            self._parse_hit_objects(cfg["HitObjects"])

    @classmethod
    def from_text(cls, text: str, meta_only: bool = False) -> "Beatmap":
        return cls(text.splitlines(), None, meta_only)

    @classmethod
    def from_file(cls, path, meta_only: bool = False) -> "Beatmap":
        path = Path(path)
        with open(path, "r", encoding="utf-8") as f:
            return cls(f.readlines(), path, meta_only)

    def _parse_timing_points(self, lines: Sequence[str]) -> None:
        beat_length, multiplier, meter = None, 1.0, None
        for line in lines:
            vals = [float(v) for v in line.split(",")]
            t, x, m = vals[:3]
            kiai = int(vals[7] if len(vals) >= 8 else 0) % 2 == 1
            if vals[6] == 0:                                         # inherited: a slider-velocity change
                if not self.timing_points:
                    continue
                if self.timing_points[-1].t == t:
                    self.timing_points.pop()
                multiplier = min(10.0, max(0.1, round(-100 / float(x), 3)))
            else:
                beat_length, multiplier, meter = x, 1.0, m
            tp = TimingPoint(int(t), beat_length, multiplier, meter, kiai)
            if not self.timing_points or tp != self.timing_points[-1]:
                self.timing_points.append(tp)
            utp = TimingPoint(int(t), beat_length, None, meter, None)
            if not self.uninherited_timing_points or utp != self.uninherited_timing_points[-1]:
                self.uninherited_timing_points.append(utp)
        if not self.timing_points:
            raise ValueError("no timing points found")

    def get_active_timing_point(self, t: int) -> TimingPoint:
        """The last point at or before t; when there is none, at or before t - 1, then t + 1 (a slider a millisecond ahead of its
        point); else the first point."""
        times = [tp.t for tp in self.timing_points]
        for off in (0, -1, 1):
            idx = bisect.bisect_right(times, t + off) - 1
            if idx >= 0:
                return self.timing_points[idx]
        return self.timing_points[0]

    def _parse_hit_objects(self, lines: Sequence[str]) -> None:
        for line in lines:
            vals = line.split(",")
            x, y, t, k = (_int(v) for v in vals[:4])
            new_combo = (k & 4) > 0
            if k & 1:
                ho: HitObject = Circle(t, new_combo, x, y)
            elif k & 2:
                curve, slides, length = vals[5:8]
                points = [(x, y)] + [tuple(_int(v) for v in p.split(":")) for p in curve.split("|")[1:]]
                tp = self.get_active_timing_point(t)
                ho = slider_from_control_points(t, tp.beat_length, self.slider_multiplier * tp.slider_multiplier, new_combo, int(slides),
                                                float(length), points)
            elif k & 8:
                ho = Spinner(t, new_combo, _int(vals[5]))
            else:
                raise ValueError(f"hit object of unknown type {k}")
            if self.hit_objects and ho.t < self.hit_objects[-1].end_time():
                raise ValueError(f"hit objects not in chronological order: {ho.t} < {self.hit_objects[-1].end_time()}")
            self.hit_objects.append(ho)
        if not self.hit_objects:
            raise ValueError("no hit objects found")
