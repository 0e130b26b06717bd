"""osuf_encode_signals on the GPU against the fp64 yardstick (tests/encode_oracle.py) on every fixture of tests/golden/encode, with the
tables, the per-row arrays and the output in poisoned, canary-guarded allocations (tests/memguard.py): hit channels bit for bit, cursor
channels within one fp32 ulp on every frame (tests/test_encode_cpu.py asserts the screening condition that makes this fair)."""
from pathlib import Path

import numpy as np
import pytest
import torch

from osufusion_amd import _lib, encode, inpaint, ops
from osufusion_amd.beatmap import Beatmap
from osufusion_amd.models import DiffusionOsuFusionDiT
from osufusion_amd.pattern import param_pattern, synth_inputs
from tests import encode_oracle as EO
from tests.memguard import guard

pytestmark = pytest.mark.gpu
DEV = "cuda"
EINVAL = -1
FIX = Path(__file__).resolve().parent / "golden" / "encode"
NAMES = ["basic", "circles", "edge", "sliders"]
FRAMES = {"basic": 890, "circles": 564, "edge": 627, "sliders": 2635}        # the lengths recorded in tests/golden/encode_cases.npz
SCREENING_MARGIN_PX = 1e-6                                                    # tests/test_encode_cpu.py's screening condition
_CACHE = {}


def _maps():
    if "maps" not in _CACHE:
        _CACHE["maps"] = [Beatmap.from_file(FIX / f"{n}.osu") for n in NAMES]
    return _CACHE["maps"]


def _oracle(name, rounded=True):
    """(6, n) fp64, computed once and shared read-only."""
    key = (name, rounded)
    if key not in _CACHE:
        _CACHE[key] = EO.encode_beatmap(_maps()[NAMES.index(name)], EO.frame_times(FRAMES[name]), rounded)
        _CACHE[key].setflags(write=False)
    return _CACHE[key]


def _table(g=None):
    """All four fixtures in one table; with a guard, every table moved into a guarded allocation."""
    table = encode.BeatmapTable(_maps(), DEV)
    if g is not None:
        table.tables = {k: g.place(v) for k, v in table.tables.items()}
    return table


def _dev(g, values, dtype):
    return g.place(torch.tensor(values, dtype=dtype, device=DEV))


def _encode(g, table, idx, start, length, flip=None, L=None, **kw):
    L = max(length) if L is None else L
    x, ln = table.encode(_dev(g, idx, torch.int32), _dev(g, start, torch.int64), _dev(g, length, torch.int32),
                         None if flip is None else _dev(g, flip, torch.int32), L=L, **kw)
    g.check()
    assert x.shape == (len(idx), 6, L) and x.dtype == torch.float32 and ln.tolist() == list(length)
    return x.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _ulps(a, b):
    """Distance in fp32 steps between two float32 arrays (finite values)."""
    def ordered(v):
        i = _bits(v).astype(np.int64)
        return np.where(i & 0x80000000, -(i & 0x7FFFFFFF), i)
    return np.abs(ordered(a) - ordered(b))


def _assert_matches(got, want64, what):
    want = want64.astype(np.float32)
    assert np.array_equal(_bits(got[:4]), _bits(want[:4])), (what, "hit channels")
    worst = int(_ulps(got[4:], want[4:]).max())
    assert worst <= 1, (what, "cursor", worst)


# ---- the kernel against the oracle -----------------------------------------------------------------------------------------------------------
def test_every_fixture_matches_the_oracle():
    """One launch over the four fixtures, full length each (ragged: the longest sets L); padding is bitwise -1.0f."""
    n = [FRAMES[k] for k in NAMES]
    with guard(0xFF) as g:
        x = _encode(g, _table(g), [0, 1, 2, 3], [0, 0, 0, 0], n)
    for b, name in enumerate(NAMES):
        _assert_matches(x[b, :, :n[b]], _oracle(name), name)
        assert np.array_equal(_bits(x[b, :, n[b]:]), _bits(np.full((6, max(n) - n[b]), -1.0)))
    exact = sum(int((_ulps(x[b, 4:, :n[b]], _oracle(k)[4:].astype(np.float32)) == 0).sum()) for b, k in enumerate(NAMES))
    print(f"cursor values bit-equal to the oracle: {exact} of {2 * sum(n)}")


def test_unrounded_positions_are_far_inside_the_screening_margin():
    """round_pos = 0: the kernel's fp64 pixel positions (pos_px) against the oracle's unrounded ones over all fixtures.  The largest
    deviation must be at least 100 times smaller than the 1e-6 px screening margin; the figure goes to profiles/encode.md."""
    n = [FRAMES[k] for k in NAMES]
    with guard(0xFF) as g:
        pos = torch.empty((4, 2, max(n)), dtype=torch.float64, device=DEV)
        x = _encode(g, _table(g), [0, 1, 2, 3], [0, 0, 0, 0], n, round_pos=0, pos_px=pos)
        pos = pos.cpu().numpy()
    worst = 0.0
    for b, name in enumerate(NAMES):
        want = (_oracle(name, False)[4:] + 1) / 2 * np.array([[512.0], [384.0]])           # back to pixels (exact to an ulp of fp64)
        dev = float(np.abs(pos[b, :, :n[b]] - want).max())
        print(f"{name}: largest deviation of the unrounded cursor {dev:.3e} px")
        worst = max(worst, dev)
        _assert_matches(x[b, :, :n[b]], _oracle(name, False), name)
        assert (pos[b, :, n[b]:] == 0).all()
    print(f"largest deviation over all fixtures: {worst:.3e} px")
    assert worst * 100 <= SCREENING_MARGIN_PX


@pytest.mark.parametrize("n", [1, 257])
def test_short_rows(n):
    """n = 1: one live lane; n = 257: two workgroups, the second with one live lane."""
    with guard(0xFF) as g:
        x = _encode(g, _table(g), [3], [0], [n])
    _assert_matches(x[0], _oracle("sliders")[:, :n], n)


def test_ragged_batch_pads_with_minus_one():
    lens = (5, 257, 300)
    with guard(0xFF) as g:
        x = _encode(g, _table(g), [3, 0, 2], [0, 0, 0], lens, L=300)
    for b, (name, n) in enumerate(zip(("sliders", "basic", "edge"), lens)):
        _assert_matches(x[b, :, :n], _oracle(name)[:, :n], name)
        assert np.array_equal(_bits(x[b, :, n:]), _bits(np.full((6, 300 - n), -1.0)))


def test_crops_equal_slices_of_the_full_encode():
    """start > 0 bit for bit; a window wholly before the first object (basic: first object at 1000 ms = frame 125.3) and one wholly after
    the last (basic: 6500 ms = frame 814.3; sliders ends at 20428 ms, frames from 2560 on); the same map named twice."""
    with guard(0xFF) as g:
        table = _table(g)
        full = _encode(g, table, [0, 3], [0, 0], [FRAMES["basic"], FRAMES["sliders"]])
        crops = _encode(g, table, [3, 0, 0, 3, 3], [1000, 10, 820, 2570, 1000], [300, 100, 60, 60, 300])
    for b, (m, s, n) in enumerate([(1, 1000, 300), (0, 10, 100), (0, 820, 60), (1, 2570, 60), (1, 1000, 300)]):
        assert np.array_equal(_bits(crops[b, :, :n]), _bits(full[m, :, s:s + n])), b
    before, after = crops[1, :, :100], crops[2, :, :60]
    first, last = _maps()[0].hit_objects[0], _maps()[0].hit_objects[-1]
    assert (before[:4] == -1).all() and (before[4] == np.float32(first.x / 512 * 2 - 1)).all()          # waits on the first object
    assert (after[4] == np.float32(last.x / 512 * 2 - 1)).all() and (after[5] == np.float32(last.y / 384 * 2 - 1)).all()
    assert (after[0] == after[0, 0]).all() and (after[1:3] == -1).all()
    _assert_matches(crops[3, :, :60], EO.encode_beatmap(_maps()[3], EO.frame_times(60, 2570)), "after the last slider")
    far = 1 << 33                                                    # a global frame index past 2^31: times stay exact in fp64
    with guard(0xFF) as g:
        x = _encode(g, _table(g), [0], [far], [40])
    _assert_matches(x[0], EO.encode_beatmap(_maps()[0], EO.frame_times(40, far)), "far")


def test_a_map_without_sliders_and_a_bad_map_index():
    with guard(0xFF) as g:
        table = _table(g)
        hdr = table.host["map_hdr"][1]
        assert hdr[2] == 0 and hdr[4] == 0                              # circles: both interval lists empty
        x = _encode(g, table, [1, 4, -1], [0, 0, 0], [FRAMES["circles"]] * 3)
    _assert_matches(x[0], _oracle("circles"), "circles")
    assert (x[0, 1:3] == -1).all() and np.array_equal(_bits(x[1:]), _bits(np.full((2, 6, FRAMES["circles"]), -1.0)))
    with guard(0xFF) as g:                                               # a table of that one map: the padded one-entry tables are never read
        alone = encode.BeatmapTable([_maps()[1]], DEV)
        alone.tables = {k: g.place(v) for k, v in alone.tables.items()}
        y = _encode(g, alone, [0], [0], [FRAMES["circles"]])
    assert np.array_equal(_bits(y[0]), _bits(x[0]))


@pytest.mark.parametrize("flip", [0, 1, 2, 3])
def test_flips_negate_the_stored_value(flip):
    """Against the oracle with the channel negated (numpy's unary minus: -0.0 where the value is +0.0), bits compared.  edge.osu rests
    at (256, 192) inside its spinner (about 100 frames): both cursor channels are exactly 0 there."""
    n = FRAMES["edge"]
    with guard(0xFF) as g:
        table = _table(g)
        plain = _encode(g, table, [2], [0], [n])
        x = _encode(g, table, [2, 2], [0, 0], [n, n], flip=[flip, 0])
    want = plain[0].copy()
    if flip & 1:
        want[4] = -want[4]
    if flip & 2:
        want[5] = -want[5]
    assert np.array_equal(_bits(x[0]), _bits(want)) and np.array_equal(_bits(x[1]), _bits(plain[0]))
    zeros = plain[0, 4] == 0
    assert zeros.sum() > 50 and np.signbit(x[0, 4][zeros]).all() == bool(flip & 1) and not np.signbit(plain[0, 4][zeros]).any()
    oracle = _oracle("edge").copy()
    oracle[4] = -oracle[4] if flip & 1 else oracle[4]
    oracle[5] = -oracle[5] if flip & 2 else oracle[5]
    _assert_matches(x[0], oracle, flip)


def test_rows_do_not_depend_on_the_rest_of_the_batch():
    with guard(0xFF) as g:
        table = _table(g)
        alone = _encode(g, table, [3], [700], [300], flip=[1])
        mixed = _encode(g, table, [0, 3, 2, 1], [5, 700, 0, 40], [64, 300, 7, 512], flip=[3, 1, 0, 2], L=640)
    assert np.array_equal(_bits(mixed[1, :, :300]), _bits(alone[0]))


def test_argument_errors_leave_the_output_untouched():
    lib = _lib.load()
    table = _table()
    B, L = 2, 8
    idx, st, ln = (torch.zeros(B, dtype=d, device=DEV) for d in (torch.int32, torch.int64, torch.int32))
    ln += L
    out = torch.full((B, 6, L), 7.0, device=DEV)
    t = table.tables
    good = dict(map_hdr=t["map_hdr"].data_ptr(), n_maps=4, obj_f=t["obj_f"].data_ptr(), obj_i=t["obj_i"].data_ptr(), ivl=t["ivl"].data_ptr(),
                seg_cum=t["seg_cum"].data_ptr(), seg_i=t["seg_i"].data_ptr(), nodes=t["nodes"].data_ptr(), map_idx=idx.data_ptr(), start=st.data_ptr(),
                len=ln.data_ptr(), flip=None, round_pos=1, out=out.data_ptr(), pos_px=None, B=B, L=L)
    bad = [{k: None} for k in ("map_hdr", "obj_f", "obj_i", "ivl", "seg_cum", "seg_i", "nodes", "map_idx", "start", "len", "out")]
    bad += [dict(n_maps=0), dict(B=0), dict(B=-1), dict(L=0), dict(L=-1)]
    for change in bad:
        assert lib.osuf_encode_signals(*{**good, **change}.values(), ops._stream()) == EINVAL, change
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    assert lib.osuf_encode_signals(*good.values(), ops._stream()) == 0
    torch.cuda.synchronize()
    _assert_matches(out[0].cpu().numpy(), _oracle("basic")[:, :L], "good call")


def test_encode_beatmap_is_the_one_map_call():
    x = encode.encode_beatmap(_maps()[2], FRAMES["edge"], DEV)
    assert x.shape == (6, FRAMES["edge"])
    _assert_matches(x.cpu().numpy(), _oracle("edge"), "edge")
    with pytest.raises(ValueError):
        encode.BeatmapTable([], DEV)
    with pytest.raises(ValueError):
        _table().encode([0], [0], torch.tensor([5], device=DEV))      # a device `length` needs L


# ---- into the sampler ---------------------------------------------------------------------------------------------------------------------
def test_known_from_beatmap_feeds_the_masked_sampler():
    """The smallest DiT of tests/test_inpaint_gpu.py: with a hard mask the kept frames of the sample equal `known` bit for bit."""
    n = 96
    known, mask = encode.known_from_beatmap(_maps()[2], n, [(0.0, 300.0), (500.0, 600.0)], device=DEV)
    assert known.shape == (1, 6, n) and mask.shape == (n,) and mask.device.type == "cuda"
    assert torch.equal(mask.cpu(), inpaint.frame_mask(n, [(0.0, 300.0), (500.0, 600.0)]))
    _assert_matches(known[0].cpu().numpy(), _oracle("edge")[:, :n], "known")
    model = DiffusionOsuFusionDiT(sampling_timesteps=4, backbone="mmdit", dim_h=64, depth=2, attn_heads=4, attn_kv_heads=2, attn_dim_head=16)
    model.load_state_dict({k: torch.from_numpy(param_pattern(k[len("unet."):], tuple(v.shape)).copy()) for k, v in model.state_dict().items()})
    model = model.to(DEV)
    _, a, c, _, noise = (torch.from_numpy(v).to(DEV) for v in synth_inputs("encode", 1, n))
    torch.manual_seed(7)
    got = model.sample(a, c, noise.float().contiguous(), cond_scale=2.0, known=known, known_mask=mask)
    keep = (mask > 0)[None, None, :].expand_as(got)
    assert 0 < int(keep.sum()) < keep.numel() and torch.isfinite(got).all()
    assert torch.equal(got[keep].view(torch.int32), known[keep].view(torch.int32))
    assert not torch.equal(got[~keep], known[~keep])
