"""osuf_decode_objects / osuf_tempo_scan / decode_gpu.decode_beatmaps on the GPU against the host code they restate
(osufusion_amd/decode.py: decode_flips, decode_extents, the loop of decode_beatmap; np.histogram + argmax), with every buffer in
poisoned, canary-guarded allocations (tests/memguard.py).  Everything compared is an integer or a string: equality, no tolerance."""
from pathlib import Path

import numpy as np
import pytest
import torch

from osufusion_amd import _lib, decode_gpu, encode, inpaint, ops
from osufusion_amd import decode as D
from osufusion_amd.beatmap import Beatmap
from osufusion_amd.pattern import onset_train
from tests.memguard import guard

pytestmark = pytest.mark.gpu
DEV = "cuda"
EINVAL = -1
FIX = Path(__file__).resolve().parent / "golden" / "encode"
NAMES = ["basic", "circles", "edge", "sliders"]
FRAMES = {"basic": 890, "circles": 564, "edge": 627, "sliders": 2635}
LENGTHS = [2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 257]
META = D.Metadata("audio.mp3", "Song", "Artist", "Version", cs=4.0, ar=9.0, od=8.0, hp=5.0)
_CACHE = {}


# ---- signals ------------------------------------------------------------------------------------------------------------------------------
def _sign_rows(n):
    """The +-1 rows the issue lists, each of n frames (bool: positive)."""
    i = np.arange(n)
    rows = [np.ones(n, bool), np.zeros(n, bool), i % 2 == 0, i % 2 == 1]
    for k in (0, 1, n - 3, n - 2):                                           # one flip between frames k | k + 1, both directions
        if 0 <= k < n - 1:
            rows += [i > k, i <= k]
    edges = [e for e in (32, 64, 128, 192, 256) if e < n]
    if edges:
        flips = np.zeros(n, int)
        flips[edges] = 1                                                     # a flip between frames e - 1 | e at every word boundary
        rows += [np.cumsum(flips) % 2 == 1, np.cumsum(flips) % 2 == 0]
        for e in edges:                                                      # two-frame pulses straddling a boundary, one frame either side
            rows += [(i >= e - 1) & (i <= e), (i >= e - 2) & (i < e), (i >= e) & (i <= e + 1), ~((i >= e - 1) & (i <= e))]
    rows += [(i // 3) % 2 == 0, (i // 2) % 2 == 1, i >= n // 2]              # starts positive; two-frame runs; positive to the end
    return rows


def _as_signal(sig, rng, cursor=None):
    """(4, n) bool -> (6, n) fp32: magnitudes in (0.1, 1.5) under the given signs, a random cursor in [-1.2, 1.2] unless one is given."""
    n = sig.shape[1]
    x = np.empty((6, n), dtype=np.float32)
    x[:4] = np.where(sig, 1.0, -1.0) * rng.uniform(0.1, 1.5, (4, n))
    x[4:] = rng.uniform(-1.2, 1.2, (2, n)) if cursor is None else cursor
    return x


def _cases():
    """[(6, n) fp32]: every row of _sign_rows as the HIT row of some sample of every length, the other three rows rotating through the
    same list; then the hand-made ones."""
    if "cases" in _CACHE:
        return _CACHE["cases"]
    rng = np.random.default_rng(11)
    cases = []
    for n in LENGTHS:
        rows = _sign_rows(n)
        for k in range(len(rows)):
            sig = np.stack([rows[k], rows[(k + 1) % len(rows)], rows[(k + 5) % len(rows)], rows[(k + 2) % len(rows)]])
            cases.append(_as_signal(sig, rng))
    n = 65
    i = np.arange(n)
    hit = (i >= 10) & (i < 20) | (i >= 30) & (i < 45) | (i >= 63)             # onsets 9, 19, 29, 44, 62
    # a sustain run from its onset; one a frame late; one a frame early; one open at the end; sliders inside the first and the last
    sustain = (i >= 10) & (i < 16) | (i >= 21) & (i < 27) | (i >= 29) & (i < 40) | (i >= 63)
    slider = (i >= 10) & (i < 13) | (i >= 45) & (i < 50) | (i >= 63)
    combo = (i >= 10) & (i < 25) | (i >= 45)                                  # flips at onsets 9 and 44, and at 24: no onset there
    ties = -1 + 2 * (i + 0.5) / 512                                           # pixel k + 0.5 on x: ties to even
    cursor = np.stack([ties, np.where(i % 2 == 0, 1.0, -1.0)])                # y at +-1: pixels 384 and 0
    cases.append(_as_signal(np.stack([hit, sustain, slider, combo]), rng, cursor))
    cursor = np.stack([np.where(i % 3 == 0, -1.0, 1.0), -1 + 2 * (2 * i + 0.5) / 384])
    cases.append(_as_signal(np.stack([hit, slider, sustain, ~combo]), rng, cursor))
    cases.append(_as_signal(np.stack([np.zeros(n, bool), sustain, slider, combo]), rng))      # combo flips and no onset at all
    cases.append(_as_signal(np.stack([np.ones(n, bool), sustain, slider, combo]), rng))
    special = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1e-45, -1e-45, 1.0, -1.0, np.nan, -np.nan, 0.0, 3e38, -3e38], dtype=np.float32)
    for shift in range(4):                                                    # 0.0, -0.0, NaN, +-inf and the smallest denormals in the hit channels
        x = _as_signal(np.stack([hit, sustain, slider, combo]), rng)
        for r in range(4):
            x[r] = np.resize(np.roll(special, shift + 3 * r), n)
        cases.append(x)
    for dens in (0.02, 0.15, 0.5):                                            # seeded random signs at three densities
        for n in (257, 64, 33):
            sig = (np.cumsum(rng.random((4, n)) < dens, axis=1) + rng.integers(0, 2, (4, 1))) % 2 == 1
            cases.append(_as_signal(sig, rng))
    _CACHE["cases"] = cases
    return cases


def _host_table(x):
    """The host's table of one (6, n) sample; no onset but a combo flip (IndexError on the host): the empty table."""
    if "host" not in _CACHE:
        _CACHE["host"] = {}
    key = x.tobytes() + bytes(x.shape[1].to_bytes(4, "little"))
    if key not in _CACHE["host"]:
        enc = np.asarray(x, dtype=np.float64)
        try:
            t = D.object_table(enc)
        except IndexError:
            assert D.decode_flips(np.where(enc[D.HIT] > 0, 1.0, -1.0)) == []
            t = D.HostTable([], [], [], [], np.zeros(0, int), np.zeros(0, int))
        _CACHE["host"][key] = t
    return _CACHE["host"][key]


def _batch(cases, L=None):
    L = max(c.shape[1] for c in cases) if L is None else L
    x = np.full((len(cases), 6, L), 0.75, dtype=np.float32)                   # behind a sample's end: positive, so a leak would show
    for b, c in enumerate(cases):
        x[b, :, :c.shape[1]] = c
    return torch.from_numpy(x), torch.tensor([c.shape[1] for c in cases], dtype=torch.int32)


def _assert_table(got: D.HostTable, want: D.HostTable, what):
    assert got.frame == want.frame, (what, "frame")
    assert got.sustain_end == want.sustain_end, (what, "sustain_end")
    assert got.slider_end == want.slider_end, (what, "slider_end")
    assert got.new_combo == [bool(v) for v in want.new_combo], (what, "new_combo")
    assert got.px.tolist() == want.px.tolist() and got.py.tolist() == want.py.tolist(), (what, "px / py")


def _decode_objects(g, x, lengths=None, cap=None):
    table = decode_gpu.decode_objects(g.place(x.to(DEV)), None if lengths is None else g.place(lengths.to(DEV)), cap)
    g.check()
    return table


# ---- the table ------------------------------------------------------------------------------------------------------------------------------
def test_ragged_batch_equals_the_host_tables():
    cases = _cases()
    x, lengths = _batch(cases)
    with guard(0xFF) as g:
        tables = _decode_objects(g, x, lengths).host()
    assert len(tables) == len(cases)
    objects = 0
    for b, c in enumerate(cases):
        _assert_table(tables[b], _host_table(c), (b, c.shape[1]))
        objects += len(tables[b].frame)
    assert objects > 300 and any(t.frame == [] for t in tables)
    assert any(-1 < e for t in tables for e in t.sustain_end) and any(-1 < e for t in tables for e in t.slider_end)


def test_without_lengths_every_sample_is_full_length():
    for n in LENGTHS:
        cases = [c for c in _cases() if c.shape[1] == n][:6]
        for c in cases[:2]:                                                   # B = 1
            with guard(0xFF) as g:
                (t,) = _decode_objects(g, torch.from_numpy(c[None])).host()
            _assert_table(t, _host_table(c), n)
        with guard(0x7F) as g:
            tables = _decode_objects(g, torch.from_numpy(np.stack(cases))).host()
        for t, c in zip(tables, cases):
            _assert_table(t, _host_table(c), n)


def test_lengths_outside_the_signal_give_no_objects():
    c = [c for c in _cases() if c.shape[1] == 65][0]
    x, _ = _batch([c] * 5)
    with guard(0xFF) as g:
        table = _decode_objects(g, x, torch.tensor([65, 1, 0, 66, -3], dtype=torch.int32))
        assert table.count.tolist() == [len(_host_table(c).frame), 0, 0, 0, 0]
        _assert_table(table.host()[0], _host_table(c), "the valid one")


def test_the_longest_sequence():
    """L = 65 536: all 1024 lanes own a word; realistic and dense rows; a sustain run over hundreds of words."""
    rng = np.random.default_rng(3)
    L = 65536
    cases = []
    for dens in (0.01, 0.3):
        sig = (np.cumsum(rng.random((4, L)) < dens, axis=1) + rng.integers(0, 2, (4, 1))) % 2 == 1
        cases.append(_as_signal(sig, rng))
    i = np.arange(L)
    sig = np.stack([i >= 100, (i > 99) & (i < 60000), (i > 99) & (i < L - 1), i >= 100])
    cases.append(_as_signal(sig, rng))
    with guard(0xFF) as g:
        tables = _decode_objects(g, torch.from_numpy(np.stack(cases))).host()
    for t, c in zip(tables, cases):
        _assert_table(t, _host_table(c), "L = 65536")
    assert tables[2].frame == [99] and tables[2].sustain_end == [59999] and tables[2].slider_end == [L - 2]
    assert len(tables[1].frame) > 5000


def test_rows_do_not_depend_on_the_batch_and_runs_repeat():
    cases = _cases()
    pick = [len(cases) - 1, len(cases) - 9, 40]
    x, lengths = _batch(cases)
    with guard(0xFF) as g:
        first = _decode_objects(g, x, lengths)
        second = _decode_objects(g, x, lengths)
        fields = ("count", "frame", "sustain_end", "slider_end", "new_combo")
        counts = first.count.tolist()
        for f in fields:
            assert torch.equal(getattr(first, f), getattr(second, f)), f        # (unwritten rows hold the guard's zero fill in both)
        for f in ("px", "py"):
            a, b = getattr(first, f).cpu().numpy(), getattr(second, f).cpu().numpy()
            for r, n in enumerate(counts):
                assert np.array_equal(a[r, :n].view(np.int64), b[r, :n].view(np.int64)), f
        whole = first.host()
        for b in pick:
            xb, lb = _batch([cases[b]], L=x.shape[2])
            (alone,) = _decode_objects(g, xb, lb).host()
            _assert_table(alone, whole[b], b)
            (short,) = _decode_objects(g, torch.from_numpy(cases[b][None])).host()
            _assert_table(short, whole[b], b)


def test_cap_overflow_writes_the_count_and_nothing_past_cap():
    c = [c for c in _cases() if c.shape[1] == 257 and len(_host_table(c).frame) > 12][0]
    want = _host_table(c)
    with guard(0xFF) as g:
        table = _decode_objects(g, torch.from_numpy(c[None]), cap=4)            # g.check() inside: the slack behind (1, 4) rows is intact
        assert table.cap == 4 and table.count.tolist() == [len(want.frame)]
        assert table.frame[0].tolist() == want.frame[:4] and table.sustain_end[0].tolist() == want.sustain_end[:4]
        assert table.px[0].tolist() == want.px[:4].tolist() and table.new_combo[0].tolist() == [int(v) for v in want.new_combo[:4]]
        with pytest.raises(ValueError, match="objects"):
            table.host()
        exact = _decode_objects(g, torch.from_numpy(c[None]), cap=len(want.frame))
        _assert_table(exact.host()[0], want, "cap == count")


def test_argument_errors_launch_nothing():
    lib = _lib.load()
    B, L, cap = 2, 64, 8
    x = torch.ones((B, 6, L), device=DEV)
    ln = torch.full((B,), L, dtype=torch.int32, device=DEV)
    count = torch.full((B,), 7, dtype=torch.int32, device=DEV)
    ints = [torch.full((B, cap), 7, dtype=torch.int32, device=DEV) for _ in range(4)]
    px, py = (torch.full((B, cap), 7.0, dtype=torch.float64, device=DEV) for _ in range(2))
    good = dict(x=x.data_ptr(), lengths=ln.data_ptr(), B=B, L=L, cap=cap, count=count.data_ptr(), frame=ints[0].data_ptr(),
                sustain_end=ints[1].data_ptr(), slider_end=ints[2].data_ptr(), new_combo=ints[3].data_ptr(), px=px.data_ptr(), py=py.data_ptr())
    bad = [{k: None} for k in ("x", "count", "frame", "sustain_end", "slider_end", "new_combo", "px", "py")]
    bad += [dict(B=0), dict(B=-1), dict(L=1), dict(L=0), dict(L=65537), dict(cap=0), dict(cap=-1)]
    for change in bad:
        assert lib.osuf_decode_objects(*{**good, **change}.values(), ops._stream()) == EINVAL, change
    torch.cuda.synchronize()
    assert (count == 7).all() and all((t == 7).all() for t in ints) and (px == 7).all() and (py == 7).all()
    assert lib.osuf_decode_objects(*{**good, "lengths": None}.values(), ops._stream()) == 0
    torch.cuda.synchronize()
    assert count.tolist() == [0, 0]                                            # all positive: no flip
    bl = torch.full((B, 3), 300.0, dtype=torch.float64, device=DEV)
    ft = torch.zeros(L, dtype=torch.float64, device=DEV)
    best = [torch.full((B, 3), 7, dtype=torch.int32, device=DEV) for _ in range(2)]
    good = dict(frame=ints[0].data_ptr(), count=count.data_ptr(), cap=cap, frame_times=ft.data_ptr(), L=L, beat_len=bl.data_ptr(), B=B, C=3,
                best_count=best[0].data_ptr(), best_bin=best[1].data_ptr())
    bad = [{k: None} for k in ("frame", "count", "frame_times", "beat_len", "best_count", "best_bin")]
    bad += [dict(B=0), dict(B=65536), dict(C=0), dict(L=0), dict(cap=0)]
    for change in bad:
        assert lib.osuf_tempo_scan(*{**good, **change}.values(), ops._stream()) == EINVAL, change
    torch.cuda.synchronize()
    assert all((t == 7).all() for t in best)
    with pytest.raises(ValueError):
        decode_gpu.decode_objects(torch.zeros((1, 6, 65537), device=DEV))
    with pytest.raises(ValueError):
        decode_gpu.decode_objects(torch.zeros((1, 6, 1), device=DEV))
    with pytest.raises(ValueError):
        decode_gpu.decode_objects(torch.zeros((1, 6, 8), device=DEV), cap=0)
    with pytest.raises(ValueError):
        decode_gpu.decode_objects(torch.zeros((1, 5, 8), device=DEV))


# ---- the tempo scan -------------------------------------------------------------------------------------------------------------------------
def _scan_inputs():
    """Five samples over one frame_times: no hit, one, two, 300 irregular ones (the first at a negative time), 200 on exact multiples
    of 300 ms."""
    rng = np.random.default_rng(8)
    L = 4096
    ft = np.arange(L) * 176 / 22050 * 1000.0
    ft[0] = -37.25                                                             # a negative time
    ft[2048:2048 + 512] = np.arange(512) * 300.0                               # exact multiples of the 300 ms beat
    frames = [[], [77], [0, 1500], [0] + sorted(rng.choice(np.arange(1, 2048), 299, replace=False).tolist()),
              sorted(rng.choice(np.arange(2048, 2048 + 512), 200, replace=False).tolist())]
    return L, ft, frames


def _table_of(g, frames, cap):
    count = g.place(torch.tensor([len(f) for f in frames], dtype=torch.int32, device=DEV))
    fr = torch.full((len(frames), cap), 1 << 20, dtype=torch.int32)            # behind a row's end: a frame far outside frame_times
    for b, f in enumerate(frames):
        fr[b, :len(f)] = torch.tensor(f, dtype=torch.int32)
    fr = g.place(fr.to(DEV))
    return decode_gpu.ObjectTable(count, fr, fr, fr, fr, None, None)


def _host_scan(ft, frames, beat_len):
    out_c, out_b = np.zeros(beat_len.shape, int), np.zeros(beat_len.shape, int)
    for b, f in enumerate(frames):
        t = ft[f] if len(f) else np.zeros(0)
        for c, bl in enumerate(beat_len[b]):
            hist = np.histogram(t % bl, bins=100, range=(0, bl))[0]
            out_c[b, c], out_b[b, c] = hist.max(), hist.argmax()
    return out_c, out_b


@pytest.mark.parametrize("C", [1, 1000])
def test_tempo_scan_equals_np_histogram(C):
    L, ft, frames = _scan_inputs()
    if C == 1:
        beat_len = np.array([[300.0], [60000 / 173], [300.0], [60000 / 187.5], [300.0]])
    else:
        beat_len = np.stack([60000.0 / np.linspace(bpm * 0.95, bpm * 1.05, C) for bpm in (200.0, 173.0, 120.0, 187.5, 200.0)])
        beat_len[4, 500] = 300.0
    with guard(0xFF) as g:
        table = _table_of(g, frames, 320)
        got_c, got_b = decode_gpu.tempo_scan(table, g.place(torch.from_numpy(ft).to(DEV)), g.place(torch.from_numpy(beat_len).to(DEV)))
        g.check()
        got_c, got_b = got_c.cpu().numpy(), got_b.cpu().numpy()
    want_c, want_b = _host_scan(ft, frames, beat_len)
    assert np.array_equal(got_c, want_c) and np.array_equal(got_b, want_b)
    assert (got_c[0] == 0).all() and (got_b[0] == 0).all() and (got_c[1] == 1).all() and got_c[2].max() <= 2
    assert got_c[4, 0 if C == 1 else 500] == 200 and got_b[4, 0 if C == 1 else 500] == 0   # every hit at phase 0 of the 300 ms beat
    assert got_c[3].max() > 5


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------
def _fixture_batch():
    """The four fixtures encoded on the GPU as one ragged batch (padding: -1.0), once."""
    if "fixtures" not in _CACHE:
        maps = [Beatmap.from_file(FIX / f"{n}.osu") for n in NAMES]
        n = [FRAMES[k] for k in NAMES]
        x, ln = encode.BeatmapTable(maps, DEV).encode([0, 1, 2, 3], [0, 0, 0, 0], n)
        _CACHE["fixtures"] = (x, ln, n, x.cpu().numpy(), inpaint.frame_times_ms(max(n)).numpy())
    return _CACHE["fixtures"]


def _host_text(b, bpm, snap):
    key = ("text", b, bpm, snap)
    if key not in _CACHE:
        _, _, n, x_host, ft = _fixture_batch()
        _CACHE[key] = D.decode_beatmap(META, x_host[b, :, :n[b]], ft[:n[b]], bpm, snap, verbose=False)
    return _CACHE[key]


@pytest.mark.parametrize("bpm, snap", [(None, True), (None, False), (187.5, True)])
def test_decode_beatmaps_equals_decode_beatmap(bpm, snap):
    x, ln, n, _, ft = _fixture_batch()
    with guard(0xFF) as g:
        texts = decode_gpu.decode_beatmaps([META] * 4, g.place(x), ft, bpm=bpm, allow_beat_snap=snap, lengths=g.place(ln))
        g.check()
    for b, name in enumerate(NAMES):
        assert texts[b] == _host_text(b, bpm, snap), name
        assert texts[b].count("\n") > 30


def test_dense_samples_take_the_tempo_scan():
    """The fixtures hold too few onsets for the estimator (its smallest lag is 190 onsets) and end on the fallback timing; a synthetic
    onset train of about 240 onsets does not: the autocorrelation finds a lag, the 1000-candidate scan runs, and both paths must
    choose the same candidate and the same offset."""
    L = 4096
    xh = np.stack([onset_train(L, 1), onset_train(L, 2, keep=0.8, bpm=173.0)])
    ft = inpaint.frame_times_ms(L).numpy()
    lengths = [L, L - 5]
    with guard(0xFF) as g:
        texts = decode_gpu.decode_beatmaps([META] * 2, g.place(torch.from_numpy(xh).to(DEV)), ft, lengths=lengths)
        g.check()
    for b in range(2):
        want = D.decode_beatmap(META, xh[b, :, :lengths[b]], ft[:lengths[b]], None, True, verbose=False)
        assert texts[b] == want, b
        assert not want.split("[TimingPoints]\n")[1].startswith("0,300.0,")                         # the scan chose a tempo


def test_a_text_does_not_depend_on_the_batch():
    x, ln, n, _, ft = _fixture_batch()
    b = 3
    alone = decode_gpu.decode_beatmaps([META], x[b:b + 1, :, :n[b]].contiguous(), ft[:n[b]], bpm=None)
    assert alone[0] == _host_text(b, None, True)
    pair = decode_gpu.decode_beatmaps([META] * 2, x[[3, 0]].contiguous(), ft, lengths=[n[3], n[0]])
    assert pair == [_host_text(3, None, True), _host_text(0, None, True)]
    timings = {}
    again = decode_gpu.decode_beatmaps([META] * 2, x[[3, 0]].contiguous(), ft, lengths=[n[3], n[0]], timings=timings)
    assert again == pair and set(timings) == {"table", "scan", "fits", "host"}


def test_no_onset_but_a_combo_flip_gives_the_empty_map():
    """The one deliberate difference: the host raises IndexError there."""
    x = -np.ones((1, 6, 64), dtype=np.float32)
    x[0, D.COMBO, 30:] = 1.0
    with pytest.raises(IndexError):
        D.decode_beatmap(META, x[0], np.arange(64) * 8.0, None, verbose=False)
    flat = -np.ones((6, 64), dtype=np.float32)
    want = D.decode_beatmap(META, flat, np.arange(64) * 8.0, None, verbose=False)
    assert decode_gpu.decode_beatmaps([META], torch.from_numpy(x).to(DEV), np.arange(64) * 8.0) == [want]
