"""fp64 yardstick of osuf_encode_signals: the reference's library/osu/data/hit.py (flips, extents, hit_signals), cursor.py
(cursor_signal) and encode.py (encode_beatmap) restated as plain loops over the hit objects of osufusion_amd/beatmap.py and any
frame_times array.  Written for clarity, not speed.  round_positions=False skips the integer rounding inside slider lerp only (and so
in a slider's start_pos / end_pos, which are lerp values); everything else is the same arithmetic."""
from __future__ import annotations

import numpy as np

from osufusion_amd.beatmap import CX, CY, Beatmap, Slider, Spinner

HOP_LENGTH, SR = 176, 22050


def frame_times(n: int, start: int = 0) -> np.ndarray:
    """inpaint.frame_times_ms in numpy: frame g sits at g * 176 / 22050 * 1000 ms, evaluated in that order."""
    return np.arange(start, start + int(n), dtype=np.float64) * HOP_LENGTH / SR * 1000.0


def flips(beatmap: Beatmap, times: np.ndarray, combo: bool = False) -> np.ndarray:
    """0/1 signal that changes state at the first frame at or after every (new-combo) object's time."""
    out = np.zeros(len(times))
    state = 0.0
    for ho in beatmap.hit_objects:
        if combo and not ho.new_combo:
            continue
        first = 0
        while first < len(times) and times[first] < ho.t:            # searchsorted(times, ho.t), from the left
            first += 1
        if first < len(times):
            state = 1.0 - state
            out[first:] = state
    return out


def extents(regions, times: np.ndarray) -> np.ndarray:
    out = np.zeros(len(times))
    for s, e in regions:
        for i, t in enumerate(times):
            if s <= t < e:
                out[i] = 1.0
    return out


def hit_signals(beatmap: Beatmap, times: np.ndarray) -> np.ndarray:
    sustain = [(ho.t, ho.end_time()) for ho in beatmap.hit_objects if isinstance(ho, (Slider, Spinner))]
    slider = [(ho.t, ho.t + ho.slide_duration) for ho in beatmap.hit_objects if isinstance(ho, Slider)]
    return np.stack([flips(beatmap, times), extents(sustain, times), extents(slider, times), flips(beatmap, times, combo=True)])


def cursor_signal(beatmap: Beatmap, times: np.ndarray, round_positions: bool = True) -> np.ndarray:
    objs = beatmap.hit_objects
    rp = round_positions
    nxt = 0                                                          # index of the next object; nxt - 1 is the current one
    out = []
    for t in times:
        while nxt < len(objs) and objs[nxt].t <= t:
            nxt += 1
        cur = objs[nxt - 1] if nxt > 0 else None
        following = objs[nxt] if nxt < len(objs) else None
        if cur is None:
            pos = np.array([CX, CY], dtype=np.float64) if following is None else following.start_pos(rp)
        elif t < cur.end_time():
            if isinstance(cur, Spinner):
                pos = cur.start_pos(rp)
            else:
                ts = (t - cur.t) % (cur.slide_duration * 2) / cur.slide_duration
                pos = cur.lerp(ts, rp) if ts < 1 else cur.lerp(2 - ts, rp)
        elif following is None:
            pos = cur.end_pos(rp)
        else:
            f = (t - cur.end_time()) / (following.t - cur.end_time())
            pos = (1 - f) * cur.end_pos(rp) + f * following.start_pos(rp)
        out.append(pos)
    return (np.array(out, dtype=np.float64).reshape(-1, 2) / np.array([512, 384])).T


def encode_beatmap(beatmap: Beatmap, times: np.ndarray, round_positions: bool = True) -> np.ndarray:
    """(6, n) fp64 in [-1, 1]: HIT, SUSTAIN, SLIDER, COMBO, CURSOR_X, CURSOR_Y."""
    times = np.asarray(times, dtype=np.float64)
    return np.concatenate([hit_signals(beatmap, times), cursor_signal(beatmap, times, round_positions)], axis=0) * 2 - 1


def slider_positions(beatmap: Beatmap, times: np.ndarray, round_positions: bool = True):
    """Pixel positions (k, 2) of every frame that lies inside a slider (the frames whose cursor goes through lerp), and their indices."""
    times = np.asarray(times, dtype=np.float64)
    cur = cursor_signal(beatmap, times, round_positions).T * np.array([512, 384])
    inside = np.zeros(len(times), dtype=bool)
    for ho in beatmap.hit_objects:
        if isinstance(ho, Slider):
            nxt = min((o.t for o in beatmap.hit_objects if o.t > ho.t), default=np.inf)
            inside |= (times >= ho.t) & (times < ho.end_time()) & (times < nxt)
    return cur[inside], np.flatnonzero(inside)
