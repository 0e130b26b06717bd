"""The host side of the batched decode (osufusion_amd/decode_gpu.py, csrc/decode.hip): the ABI surface, numpy's uniform-bin rule as the
tempo-scan kernel restates it, and the table -> text helper that both decode paths share.  The kernels themselves are compared with the
host functions in tests/test_decode_gpu.py."""
from pathlib import Path

import numpy as np
import pytest

from osufusion_amd import _lib
from osufusion_amd import decode as D
from osufusion_amd.beatmap import Beatmap
from osufusion_amd.csrc import build
from tests import encode_oracle as EO

ROOT = Path(__file__).resolve().parent.parent
FIX = ROOT / "tests" / "golden" / "encode"
NAMES = ["basic", "circles", "edge", "sliders"]
FRAMES = {"basic": 890, "circles": 564, "edge": 627, "sliders": 2635}        # the lengths recorded in tests/golden/encode_cases.npz
META = D.Metadata("audio.mp3", "Song", "Artist", "Version", cs=4.0, ar=9.0, od=8.0, hp=5.0)


def test_abi_surface():
    P, I = _lib.P, _lib.I
    decls = _lib.read_header()[0]
    for name, n_args in (("osuf_decode_objects", 13), ("osuf_tempo_scan", 11)):
        assert name in decls and decls[name][0] == "int", f"{name} is not declared in include/osufusion_hip.h"
        assert len(decls[name][1]) == n_args == len(_lib.SIGNATURES[name])
    assert _lib.SIGNATURES["osuf_decode_objects"] == [P, P, I, I, I, P, P, P, P, P, P, P, P]
    assert _lib.SIGNATURES["osuf_tempo_scan"] == [P, P, I, P, I, P, I, I, P, P, P]
    assert "decode.hip" in build.SOURCES
    assert "osuf_decode_objects" in (ROOT / "INTEGRATION.md").read_text() and "osuf_tempo_scan" in (ROOT / "INTEGRATION.md").read_text()


def uniform_bins(phase: np.ndarray, bl: float) -> np.ndarray:
    """numpy/lib/_histograms_impl.py's equal-bin path for bins=100, range=(0, bl), as osuf_tempo_scan restates it."""
    phase = phase[(phase >= 0) & (phase <= bl)]
    width = bl / 100
    idx = (phase / bl * 100).astype(np.intp)
    idx[idx == 100] = 99
    idx[phase < idx * width] -= 1
    upper = np.where(idx + 1 == 100, bl, (idx + 1) * width)
    idx[(phase >= upper) & (idx != 99)] += 1
    return np.bincount(idx, minlength=100)


@pytest.mark.parametrize("bl", [60000 / 173, 300.0, 60000 / 187.5, 1 / 3, 1e-3 * np.pi, 59999.99999, 60000 / 299.7])
def test_binning_rule_equals_np_histogram_on_every_edge(bl):
    bl = float(bl)
    edges = np.arange(101) * (bl / 100)
    edges[100] = bl
    assert np.array_equal(edges, np.linspace(0, bl, 101))                 # what np.histogram compares against
    on = np.arange(100) * (bl / 100)
    pts = np.concatenate([on, np.nextafter(on, -np.inf), np.nextafter(on, np.inf), [0.0, np.nextafter(bl, 0), bl],
                          np.nextafter(bl, np.inf, dtype=np.float64)[None], [-1.0]])
    want = np.histogram(pts, bins=100, range=(0, bl))[0]
    assert np.array_equal(uniform_bins(pts, bl), want)
    assert want.sum() == len(pts) - 3                                      # below 0 (twice) and above bl: not counted
    for p in pts:                                                          # one at a time: no cancelling errors
        assert np.array_equal(uniform_bins(np.array([p]), bl), np.histogram([p], bins=100, range=(0, bl))[0]), p
    rng = np.random.default_rng(5)
    t = rng.uniform(-50.0, 200000.0, 4000)
    assert np.array_equal(uniform_bins(t % bl, bl), np.histogram(t % bl, bins=100, range=(0, bl))[0])


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("bpm, snap", [(None, True), (None, False), (187.5, True)])
def test_table_to_text_reproduces_decode_beatmap(name, bpm, snap):
    """A host-built table through the shared helper, with the timing computed as decode_beatmaps computes it (candidates on the host,
    fullest bin per candidate, first argmax), gives decode_beatmap's text."""
    n = FRAMES[name]
    ft = EO.frame_times(n)
    enc = EO.encode_beatmap(Beatmap.from_file(FIX / f"{name}.osu"), ft, True).astype(np.float32).astype(np.float64)
    want = D.decode_beatmap(META, enc, ft, bpm, snap, verbose=False)
    table = D.object_table(enc)
    assert len(table.frame) > 3 and table.frame == sorted(table.frame)
    hit_times = ft[table.frame]
    scan = D.tempo_candidates(hit_times, verbose=False) if bpm is None and snap else None
    if bpm is not None:
        bls = [60000 / bpm]
    elif scan is not None:
        bls = list(60000.0 / scan)
    else:
        bls = None
    if bls is None:
        ok, tp = D.TIMING_FALLBACK
    else:
        hists = [uniform_bins(hit_times % bl, bl) for bl in bls]
        c = int(np.argmax([h.max() for h in hists]))
        ok, tp = True, D.TimingPoint(float(np.linspace(0, bls[c], 101)[int(np.argmax(hists[c]))]), bls[c], 4)
    cursor = (enc[[D.CURSOR_X, D.CURSOR_Y]] + 1.0) / 2.0 * np.array([[512.0], [384.0]])
    assert D.table_to_text(META, table, cursor, ft, ok, tp, verbose=False) == want
    assert want.count("\n") > 30


def test_table_of_a_hand_made_row():
    """object_table's fields on a signal small enough to read: an onset at a two-frame plateau, a sustain run that starts at the onset, one
    that starts a frame late, a run open at the end, and a combo flip away from any onset."""
    enc = -np.ones((6, 40))
    enc[D.HIT, 10:20] = 1.0                                                 # flips 9|10 and 19|20: onsets 9 and 19
    enc[D.HIT, 30:] = 1.0                                                   # 29|30: onset 29
    enc[D.SUSTAIN, 10:16] = 1.0                                             # starts at onset 9, ends at 15
    enc[D.SUSTAIN, 21:25] = 1.0                                             # starts at 20: one frame off onset 19
    enc[D.SUSTAIN, 30:] = 1.0                                               # starts at onset 29, never ends
    enc[D.SLIDER, 10:13] = 1.0
    enc[D.COMBO, 10:] = 1.0                                                 # at onset 9
    enc[D.COMBO, 25:] = -1.0                                                # flip 24|25: no onset there -> the last object
    enc[D.CURSOR_X] = -1 + 2 * (np.arange(40) + 0.5) / 512                  # pixel k + 0.5: ties go to even
    t = D.object_table(enc)
    assert t.frame == [9, 19, 29] and t.sustain_end == [15, -1, -1] and t.slider_end == [12, -1, -1]
    assert t.new_combo == [True, False, True]
    assert t.px.tolist() == [10, 20, 30] and t.py.tolist() == [0, 0, 0]
