"""The beatmap encoder on the host: parser and slider geometry of osufusion_amd/beatmap.py against hand-written answers and closed forms,
the fp64 oracle (tests/encode_oracle.py) against the reference's recorded output (tests/golden/encode_cases.npz), the device tables of
osufusion_amd/encode.py walked on the host, the C ABI of osuf_encode_signals, and the round trip through decode.decode_beatmap."""
import math
from ctypes import c_int, c_void_p
from pathlib import Path

import numpy as np
import pytest

from osufusion_amd import _lib, decode, encode
from osufusion_amd.beatmap import (Beatmap, Bezier, Circle, Line, Perfect, Slider, Spinner, bezier_length, bezier_point,
                                   slider_from_control_points)
from tests import encode_oracle as EO

ROOT = Path(__file__).resolve().parent.parent
FIX = ROOT / "tests" / "golden" / "encode"
NAMES = ["basic", "circles", "edge", "sliders"]
_CACHE = {}


def _map(name):
    if name not in _CACHE:
        _CACHE[name] = Beatmap.from_file(FIX / f"{name}.osu")
    return _CACHE[name]


def _golden():
    if "golden" not in _CACHE:
        _CACHE["golden"] = dict(np.load(ROOT / "tests" / "golden" / "encode_cases.npz"))
    return _CACHE["golden"]


def _oracle(name, rounded=True):
    key = ("oracle", name, rounded)
    if key not in _CACHE:
        n = _golden()[name].shape[1]
        _CACHE[key] = EO.encode_beatmap(_map(name), EO.frame_times(n), rounded)
        _CACHE[key].setflags(write=False)
    return _CACHE[key]


def _rows(bm):
    return [(type(o).__name__, o.t, o.end_time(), o.new_combo) for o in bm.hit_objects]


# ---- parser -------------------------------------------------------------------------------------------------------------------------------
def test_parser_known_answers_circles_and_basic():
    bm = _map("circles")
    assert (bm.mode, bm.title, bm.version, bm.mapset_id, bm.ar, bm.beat_divisor, bm.slider_multiplier) == (0, "circles", "circle only", 7, 8.0, 4, 1.4)
    assert bm.audio_filename == FIX / "audio.wav"
    assert _rows(bm) == [("Circle", 0, 0, True), ("Circle", 400, 400, False), ("Circle", 800, 800, False), ("Circle", 800, 800, False),
                         ("Circle", 1600, 1600, True), ("Circle", 2003, 2003, False), ("Circle", 3520, 3520, True), ("Circle", 3900, 3900, False)]
    assert [(o.x, o.y) for o in bm.hit_objects[:2]] == [(64, 64), (448, 64)]
    bm = _map("basic")
    assert bm.mapset_id is None and bm.ar == 9.0
    assert _rows(bm) == [("Circle", 1000, 1000, True), ("Circle", 1500, 1500, False), ("Line", 2000, 3000, False), ("Spinner", 4000, 5500, True),
                         ("Circle", 6500, 6500, False)]
    assert bm.hit_objects[2].slide_duration == 1000.0                # 200 / (1 * 100) * 500


def test_parser_known_answers_sliders():
    bm = _map("sliders")
    assert bm.ar == 7 and bm.beat_divisor == 4                       # the reference's defaults
    assert [(tp.t, tp.slider_multiplier) for tp in bm.timing_points] == [(0, 1.0), (4000, 2.0), (6000, 0.5), (8001, 1.0), (9000, 1.0)]
    assert bm.timing_points[2].kiai and not bm.timing_points[1].kiai
    assert _rows(bm) == [("Spinner", 500, 1500, True), ("Line", 2000, 2319, False), ("Perfect", 4000, 4428, False), ("Perfect", 6000, 7714, True),
                         ("Bezier", 8000, 9142, False), ("Bezier", 10000, 11257, False), ("Bezier", 12000, 13371, False),
                         ("Bezier", 14000, 14742, True), ("Line", 16000, 16171, False), ("Line", 18000, 18342, False), ("Bezier", 20000, 20428, False)]
    sl = [o for o in bm.hit_objects if isinstance(o, Slider)]
    assert [o.slides for o in sl] == [1, 2, 3, 1, 2, 1, 1, 1, 1, 1]
    # length / (1.4 * multiplier * 100) * 400; the slider at 8000 sits 1 ms before its point and keeps the 0.5 of the point at 6000
    want = [111.8 / 140 * 400, 150 / 280 * 400, 100 / 70 * 400, 200 / 70 * 400, 220 / 140 * 400, 480 / 140 * 400, 260 / 140 * 400, 60 / 140 * 400,
            120 / 140 * 400, 150 / 140 * 400]
    assert [o.slide_duration for o in sl] == pytest.approx(want, rel=1e-15)
    assert [[len(s) - 1 for s in o.segments] for o in sl if isinstance(o, Bezier)] == [[2], [3], [12], [1, 1, 1], [1, 1]]
    assert sl[1].end > sl[1].start and sl[2].end < sl[2].start       # counter-clockwise, then clockwise, in the angle's own sense


def test_parser_known_answers_edge():
    bm = _map("edge")
    assert bm.ar == 9.3 and bm.beat_divisor == 8
    # the inherited point at 0 comes before the first uninherited one: dropped; the second `1,500` line is a duplicate: dropped;
    # 300,-50 is replaced by 300,-100 (same t)
    assert [(tp.t, tp.beat_length, tp.slider_multiplier) for tp in bm.timing_points] == [(1, 500.0, 1.0), (300, 500.0, 1.0), (2000, 500.0, 0.8)]
    assert _rows(bm) == [("Line", 0, 192, True), ("Line", 414, 798, False), ("Circle", 798, 798, False), ("Perfect", 2000, 2865, True),
                         ("Circle", 3520, 3520, False), ("Spinner", 3600, 4400, False)]
    one = bm.hit_objects[1]
    assert one.slide_duration == 100 / 130 * 500 and one.t + one.slide_duration > one.end_time() == bm.hit_objects[2].t


def test_timing_point_probe():
    bm = _map("edge")                                                 # points at 1, 300, 2000
    first, second = bm.timing_points[0], bm.timing_points[1]
    assert bm.get_active_timing_point(0) is first                     # nothing at 0 or -1; found at t + 1
    assert bm.get_active_timing_point(-1) is first                    # nothing at -1, -2, 0: the fall-back to the first point
    assert bm.get_active_timing_point(1) is first and bm.get_active_timing_point(299) is first
    assert bm.get_active_timing_point(300) is second and bm.get_active_timing_point(5000) is bm.timing_points[2]


def _text(timing, objects):
    return ("[General]\nAudioFilename: a.wav\nMode: 0\n\n[Metadata]\nTitle:t\nArtist:a\nCreator:c\nVersion:v\n\n[Difficulty]\nHPDrainRate:5\n"
            "CircleSize:4\nOverallDifficulty:6\nSliderMultiplier:1\nSliderTickRate:1\n\n[Events]\n\n[TimingPoints]\n" + timing +
            "\n[HitObjects]\n" + objects)


def test_the_three_value_errors():
    with pytest.raises(ValueError, match="timing"):
        Beatmap.from_text(_text("0,-100,4,2,0,60,0,0\n", "1,1,0,1,0\n"))          # only an inherited point, which is dropped
    with pytest.raises(ValueError, match="no hit objects"):
        Beatmap.from_text(_text("0,500,4,2,0,60,1,0\n", ""))
    with pytest.raises(ValueError, match="chronological"):
        Beatmap.from_text(_text("0,500,4,2,0,60,1,0\n", "0,0,1000,2,0,L|100:0,1,100\n5,5,1499,1,0\n"))     # the slider ends at 1500
    ok = Beatmap.from_text(_text("0,500,4,2,0,60,1,0\n", "0,0,1000,2,0,L|100:0,1,100\n5,5,1500,1,0\n"))
    assert len(ok.hit_objects) == 2
    meta = Beatmap.from_text(_text("", ""), meta_only=True)
    assert meta.title == "t" and meta.hit_objects == []


# ---- sliders ------------------------------------------------------------------------------------------------------------------------------
def _slider(points, length=100.0, slides=1):
    return slider_from_control_points(0, 500.0, 1.0, False, slides, length, points)


def test_slider_classification():
    assert isinstance(_slider([(0, 0), (50, 0)]), Line)
    assert isinstance(_slider([(0, 0), (50, 10), (50, 10)]), Line)                       # p2 == p3
    assert isinstance(_slider([(0, 0), (50, 0), (120, 0)]), Line)                        # collinear, forward
    back = _slider([(0, 0), (100, 0), (-50, 0)])                                         # collinear, doubling back
    assert isinstance(back, Bezier) and [s.tolist() for s in back.segments[:2]] == [[[0, 0], [100, 0]], [[100, 0], [-50, 0]]]
    flat = _slider([(0, 0), (100, 2), (200, 0)])                                         # circumradius 2501 > 320, forward
    assert isinstance(flat, Bezier) and len(flat.segments[0]) == 3
    assert isinstance(_slider([(0, 0), (100, 2), (50, 0)]), Perfect)                     # large radius but not forward-going
    arc = _slider([(100, 200), (150, 150), (200, 200)])
    assert isinstance(arc, Perfect) and arc.center.tolist() == pytest.approx([150, 200]) and arc.radius == pytest.approx(50)
    assert isinstance(_slider([(0, 0), (10, 30), (40, 30), (50, 0)]), Bezier)
    with pytest.raises(ValueError):
        _slider([(0, 0)])


@pytest.mark.parametrize("points,length", [([(100, 200), (150, 150), (200, 200)], 150.0), ([(100, 100), (150, 150), (200, 100)], 100.0),
                                           ([(120, 80), (180, 140), (120, 200)], 90.0)])
def test_perfect_arc_length_is_the_length(points, length):
    arc = _slider(points, length)
    assert abs(abs(arc.end - arc.start) * arc.radius - length) <= 1e-9
    assert np.linalg.norm(arc.point(0.0) - np.array(points[0])) <= 1e-9                  # starts on the first control point
    (ux, uy), (vx, vy) = np.subtract(points[1], points[0]), np.subtract(points[2], points[0])
    cross = ux * vy - uy * vx
    assert np.sign(arc.end - arc.start) == np.sign(cross)


def test_bezier_length_closed_forms():
    assert bezier_length(np.array([[3.0, 4.0], [6.0, 8.0]])) == 5.0
    # y = x^2 over [0, 1] is the quadratic with control points (0, 0), (1/2, 0), (1, 1): sqrt(5) / 2 + asinh(2) / 4
    want = math.sqrt(5.0) / 2 + math.asinh(2.0) / 4
    assert bezier_length(np.array([[0.0, 0.0], [0.5, 0.0], [1.0, 1.0]])) == pytest.approx(want, rel=1e-9)
    assert bezier_length(300 * np.array([[0.0, 0.0], [0.5, 0.0], [1.0, 1.0]])) == pytest.approx(300 * want, rel=1e-9)
    # a cubic that is a straight line run at uneven speed
    assert bezier_length(np.array([[0.0, 0.0], [10.0, 0.0], [15.0, 0.0], [40.0, 0.0]])) == pytest.approx(40.0, rel=1e-9)


def test_bezier_point_is_the_bernstein_sum():
    rng = np.random.default_rng(5)
    for deg in (1, 2, 3, 12):
        nodes = rng.uniform(0, 512, (deg + 1, 2))
        for s in (0.0, 0.3, 0.5, 1.0):
            want = sum(math.comb(deg, i) * (1 - s) ** (deg - i) * s ** i * nodes[i] for i in range(deg + 1))
            assert bezier_point(nodes, s) == pytest.approx(want, rel=1e-12, abs=1e-9)


def test_cum_t_is_monotone_and_ends_at_one():
    seen = 0
    for name in NAMES:
        for o in _map(name).hit_objects:
            if isinstance(o, Bezier):
                seen += 1
                assert (np.diff(o.cum_t) > 0).all() and o.cum_t[0] > 0 and o.cum_t[-1] == 1.0 and len(o.cum_t) == len(o.segments)
    assert seen == 5
    tail = _map("sliders").hit_objects[7]                             # 100 + 100 of control polygon, length 260: a 60-pixel straight tail
    assert tail.cum_t.tolist() == pytest.approx([100 / 260, 200 / 260, 1.0]) and tail.segments[2].tolist() == [[200, 200], [200, 260]]
    assert tail.end_pos().tolist() == [200, 260]


def test_lerp_rounds_half_to_even():
    line = slider_from_control_points(0, 500.0, 1.0, False, 2, 5.0, [(0, 0), (5, 0)])
    assert [line.lerp(s).tolist() for s in (0.1, 0.3, 0.5, 0.7)] == [[0, 0], [2, 0], [2, 0], [4, 0]]        # 0.5, 1.5, 2.5, 3.5
    assert line.lerp(0.3, rounded=False).tolist() == [1.5, 0.0]
    assert line.start_pos().tolist() == [0, 0] and line.end_pos().tolist() == [0, 0]                       # slides = 2: back at the start
    assert slider_from_control_points(0, 500.0, 1.0, False, 3, 5.0, [(0, 0), (5, 0)]).end_pos().tolist() == [5, 0]


# ---- oracle -----------------------------------------------------------------------------------------------------------------------------
def test_frame_times_are_the_bits_of_inpaint_frame_times_ms():
    from osufusion_amd import inpaint
    assert np.array_equal(EO.frame_times(3000), inpaint.frame_times_ms(3000).numpy())
    assert np.array_equal(EO.frame_times(7, 441), inpaint.frame_times_ms(448).numpy()[441:])


@pytest.mark.parametrize("name", NAMES)
def test_oracle_against_the_reference(name):
    """Hit channels equal; the cursor within 1e-12 -- on basic, circles and edge that is the reference itself, on sliders the reference
    with the stand-in for the `bezier` package (tests/golden/make_encode_golden.py)."""
    want = _golden()[name]
    assert int(_golden()[f"{name}/uses_stand_in"]) == (1 if name == "sliders" else 0)
    got = _oracle(name)
    assert got.shape == want.shape and np.array_equal(got[:4], want[:4])
    assert np.abs(got[4:] - want[4:]).max() <= 1e-12
    assert set(np.unique(got[:4])) <= {-1.0, 1.0}


def test_the_traps_are_in_the_fixtures():
    x, t = _oracle("edge"), EO.frame_times(_golden()["edge"].shape[1])
    f = 100                                                           # 798.19 ms: past the slider's end_time (798), inside t + slide_duration
    assert 798 <= t[f] < 414 + 100 / 130 * 500
    assert x[encode.SLIDER, f] == 1 and x[encode.SUSTAIN, f] == -1 and x[encode.HIT, f] != x[encode.HIT, f - 1]
    c = _oracle("circles")
    assert c[encode.HIT, 100] == c[encode.HIT, 101] == c[encode.HIT, 99]                 # two circles at t = 800 (frame 101): two flips
    assert c[encode.HIT, 0] == 1 and c[encode.COMBO, 0] == 1                              # an object at t = 0
    assert (c[encode.SUSTAIN] == -1).all() and (c[encode.SLIDER] == -1).all()


def test_no_slider_coordinate_sits_on_a_rounding_edge():
    """The screening condition of the GPU comparison: over every frame inside a slider no unrounded coordinate lies within 1e-6 px of a
    half-integer, so a last-bit difference in cos / sin cannot move a rounded position."""
    frames = 0
    for name in NAMES:
        pos, _ = EO.slider_positions(_map(name), EO.frame_times(_golden()[name].shape[1]), round_positions=False)
        frames += len(pos)
        if len(pos):
            margin = np.abs((pos - 0.5) - np.round(pos - 0.5)).min()
            assert margin > 1e-6, (name, margin)
    assert frames > 1000


# ---- tables -----------------------------------------------------------------------------------------------------------------------------
def _walk(tab, m, times, round_pos=True):
    """osuf_encode_signals's table walk, on the host in fp64 (before the rounding to fp32)."""
    n_obj, o0, n_sus, sus_off, n_sld, sld_off = tab["map_hdr"][m, :6]
    of, oi = tab["obj_f"][o0:o0 + n_obj], tab["obj_i"][o0:o0 + n_obj]
    out = np.zeros((6, len(times)))

    def inside(off, n, t):
        iv = tab["ivl"][off:off + n]
        k = int(np.searchsorted(iv[:, 0], t, side="right"))
        return float(k > 0 and t < iv[k - 1, 1])
    ps = 2 if round_pos else 6
    for j, t in enumerate(times):
        cnt = int(np.searchsorted(of[:, 0], t, side="right"))
        hit, combo = cnt & 1, (oi[cnt - 1, 1] & 1) if cnt else 0
        if cnt == 0:
            p = of[0, ps:ps + 2]
        else:
            f, i = of[cnt - 1], oi[cnt - 1]
            if t < f[1]:
                if i[0] < 2:
                    p = f[ps:ps + 2]
                else:
                    ts = math.fmod(t - f[0], f[10] * 2) / f[10]
                    ts = ts if ts < 1 else 2 - ts
                    if i[0] == 2:
                        p = (1 - ts) * f[11:13] + ts * f[13:15]
                    elif i[0] == 3:
                        th = (1 - ts) * f[14] + ts * f[15]
                        p = f[11:13] + f[13] * np.array([math.cos(th), math.sin(th)])
                    else:
                        cum = tab["seg_cum"][i[2]:i[2] + i[3]]
                        k = int(np.searchsorted(cum, min(1.0, max(0.0, ts))))
                        lo = cum[k - 1] if k else 0.0
                        off, deg = tab["seg_i"][i[2] + k]
                        p = bezier_point(tab["nodes"][off:off + deg + 1], (ts - lo) / (cum[k] - lo))
                    p = p.round(0) if round_pos else p
            elif cnt == n_obj:
                p = f[ps + 2:ps + 4]
            else:
                nf = of[cnt]
                w = (t - f[1]) / (nf[0] - f[1])
                p = (1 - w) * f[ps + 2:ps + 4] + w * nf[ps:ps + 2]
        out[:, j] = [hit, inside(sus_off, n_sus, t), inside(sld_off, n_sld, t), combo, p[0] / 512, p[1] / 384]
    return out * 2 - 1


@pytest.mark.parametrize("rounded", [True, False])
def test_packed_tables_walk_to_the_oracle(rounded):
    tab = encode.pack_tables([_map(n) for n in NAMES])
    assert all(len(tab[k]) > 0 for k in encode.TABLES) and tab["obj_f"].shape[1] == 16 and tab["map_hdr"].shape == (4, 8)
    assert tab["map_hdr"][1, 2] == 0 and tab["map_hdr"][1, 4] == 0                       # circles: both interval lists empty
    for m, name in enumerate(NAMES):
        want = _oracle(name, rounded)
        assert np.array_equal(_walk(tab, m, EO.frame_times(want.shape[1]), rounded), want), name


def test_merge_intervals():
    assert encode.merge_intervals([]).shape == (0, 2)
    assert encode.merge_intervals([(5, 7), (0, 2), (1, 3.5), (3.5, 4), (9, 9), (10, 8)]).tolist() == [[0, 4], [5, 7]]
    one = _map("edge").hit_objects[1]
    tab = encode.pack_tables([_map("edge")])
    hdr = tab["map_hdr"][0]
    assert tab["ivl"][hdr[5]:hdr[5] + hdr[4]][1].tolist() == [414.0, 414 + one.slide_duration]


# ---- C ABI --------------------------------------------------------------------------------------------------------------------------------
def test_capi_encode_signals_is_declared_bound_and_exported():
    decls = _lib.read_header()[0]
    assert "osuf_encode_signals" in decls, "osuf_encode_signals is not declared in include/osufusion_hip.h"
    ret, params = decls["osuf_encode_signals"]
    assert ret == "int" and [p.split()[-1].lstrip("*") for p in params] == ["map_hdr", "n_maps", "obj_f", "obj_i", "ivl", "seg_cum", "seg_i", "nodes", "map_idx", "start", "len", "flip", "round_pos", "out",
                     "pos_px", "B", "L", "stream"]
    P, I = c_void_p, c_int
    assert _lib.SIGNATURES["osuf_encode_signals"] == [P, I, P, P, P, P, P, P, P, P, P, P, I, P, P, I, I, P]
    assert hasattr(_lib.load(), "osuf_encode_signals")
    from osufusion_amd.csrc import build
    assert "encode.hip" in build.SOURCES


def test_capi_encode_signals_validates_on_the_host():
    """Every call returns -1 before a launch: the device "pointers" are never dereferenced."""
    fn = _lib.load().osuf_encode_signals
    good = dict(map_hdr=4096, n_maps=1, obj_f=4096, obj_i=4096, ivl=4096, seg_cum=4096, seg_i=4096, nodes=4096, map_idx=4096, start=4096, len=4096,
                flip=None, round_pos=1, out=4096, pos_px=None, B=2, L=8)
    bad = [{k: None} for k in ("map_hdr", "obj_f", "obj_i", "ivl", "seg_cum", "seg_i", "nodes", "map_idx", "start", "len", "out")]
    bad += [dict(n_maps=0), dict(B=0), dict(B=-1), dict(L=0), dict(L=-5), dict(B=65536)]
    for change in bad:
        assert fn(*{**good, **change}.values(), None) == -1, change


# ---- round trip ---------------------------------------------------------------------------------------------------------------------------
def test_round_trip_through_decode_beatmap():
    """oracle encode -> decode.decode_beatmap -> Beatmap.from_text keeps the objects of basic.osu.  Tolerance, read off decode.py: a flip
    (or the start of a positive run) between frames f - 1 and f makes a two-sample plateau in np.gradient whose middle, (i + j) // 2,
    is f - 1 (_peaks_above; decode_extents names the same frame, the last non-positive one), so an object at time t, whose first frame at
    or after t is f, is written at frame_times[f - 1], in [t - one frame, t); a run's end is its last positive frame, in [end - one
    frame, end).  The parser then truncates the written float to an integer: up to 1 ms more.  So written - true lies in
    (-(one frame + 1 ms), 0] for starts and spinner ends; nothing is later than the truth.  Beat snapping is off."""
    bm = _map("basic")
    n = _golden()["basic"].shape[1]
    times = EO.frame_times(n)
    meta = decode.Metadata("audio.wav", bm.title, bm.artist, bm.version, bm.cs, bm.ar, bm.od, bm.hp)
    text = decode.decode_beatmap(meta, _oracle("basic"), times, None, allow_beat_snap=False, verbose=False)
    back = Beatmap.from_text(text)
    base = lambda o: Slider if isinstance(o, Slider) else type(o)                        # the decoder refits the path: any slider kind
    assert len(back.hit_objects) == len(bm.hit_objects)
    assert [base(o) for o in back.hit_objects] == [base(o) for o in bm.hit_objects] == [Circle, Circle, Slider, Spinner, Circle]
    assert [o.new_combo for o in back.hit_objects] == [o.new_combo for o in bm.hit_objects]
    frame = times[1]
    for got, want in zip(back.hit_objects, bm.hit_objects):
        assert -(frame + 1) < got.t - want.t <= 0, (got.t, want.t)
        if isinstance(want, Spinner):
            assert -(frame + 1) < got.end_time() - want.end_time() <= 0
    assert (back.title, back.version, back.ar, back.mode) == (bm.title, bm.version, bm.ar, 0)
