"""Windowed sampling without a GPU: the window layout and the taper of osufusion_amd/windowed.py, the partition of unity of the fuse rule as
tests/windowed_oracle.py restates it, and the argument validation of every transformer sample()."""
import numpy as np
import pytest
import torch

from osufusion_amd import windowed
from osufusion_amd.models import ContinuousDiffusionOsuFusionDiT, DiffusionOsuFusionDiT, RectifiedFlowOsuFusionDiT
from tests import windowed_oracle as WO

LAYOUTS = [(5, 4, 4), (9, 4, 3), (11, 4, 1), (24, 8, 4), (28, 8, 8), (1027, 256, 192), (4100, 1024, 768), (336, 96, 72), (32768, 4096, 3072)]
IDS = lambda s: "x".join(map(str, s))  # noqa: E731


# ---- window_starts -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS, ids=IDS)
def test_starts_cover_every_frame_and_only_the_last_is_clamped(layout):
    n, window, stride = layout
    s = windowed.window_starts(n, window, stride)
    assert s == WO.starts(n, window, stride) and all(isinstance(v, int) for v in s)
    W = -(-(n - window) // stride) + 1
    assert len(s) == W and s[0] == 0 and s[-1] == n - window
    assert all(0 <= v <= n - window for v in s)                       # every window of exactly `window` frames lies inside the sequence
    assert s[:-1] == [j * stride for j in range(W - 1)]                # only the last start is clamped ...
    assert (W - 1) * stride >= s[-1] > (W - 2) * stride                # ... and it stays behind its predecessor
    covered = np.zeros(n, np.int64)
    for v in s:
        covered[v:v + window] += 1
    assert covered.min() >= 1 and covered[0] == 1 and covered[-1] == 1


def test_known_layouts():
    assert windowed.window_starts(336, 96, 72) == [0, 72, 144, 216, 240]
    assert windowed.window_starts(5, 4, 4) == [0, 1]
    assert windowed.window_starts(24, 8, 4) == [0, 4, 8, 12, 16]      # an exact fit: nothing is clamped
    assert windowed.window_starts(28, 8, 8) == [0, 8, 16, 20]
    assert len(windowed.window_starts(32768, 4096, 3072)) == 11


@pytest.mark.parametrize("n", [1, 7, 8])
def test_one_window_when_the_sequence_fits(n):
    assert windowed.window_starts(n, 8, 6) == [0]


@pytest.mark.parametrize("bad", [(10, 0, 1), (10, 4, 0), (10, 4, 5), (0, 4, 2), (10, -1, -1)])
def test_starts_reject_bad_layouts(bad):
    with pytest.raises(ValueError):
        windowed.window_starts(*bad)


# ---- window_weight -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS, ids=IDS)
def test_weights_are_positive_symmetric_and_flat_in_the_middle(layout):
    _, window, stride = layout
    r = window - stride
    for taper in ("trapezoid", "flat"):
        w = windowed.window_weight(window, stride, taper)
        assert w.dtype == torch.float32 and tuple(w.shape) == (window,) and w.device.type == "cpu"
        assert np.array_equal(w.numpy().view(np.uint32), WO.weight(window, stride, taper).view(np.uint32))
        assert (w > 0).all() and (w <= 1).all() and torch.equal(w, w.flip(0))
    assert torch.equal(windowed.window_weight(window, stride, "flat"), torch.ones(window))
    w = windowed.window_weight(window, stride)                        # the trapezoid is the default
    assert w.min().item() == np.float32(1.0 / (r + 1))
    if r <= window - 1 - r:
        assert (w[r:window - r] == 1.0).all()
    if r > 0:
        assert (w[:min(r, window // 2)] < 1.0).all()


def test_weight_rejects_bad_arguments():
    with pytest.raises(ValueError, match="taper"):
        windowed.window_weight(8, 6, "hann")
    for window, stride in ((0, 1), (8, 0), (8, 9)):
        with pytest.raises(ValueError):
            windowed.window_weight(window, stride)


# ---- the fuse rule -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS[:-1], ids=IDS)
@pytest.mark.parametrize("taper", ["trapezoid", "flat"])
def test_partition_of_unity(layout, taper):
    """Fusing the windows of y returns y: bit for bit where one window covers the frame (a select), elsewhere within 2 ulp, the error of an
    fp32 weighted mean of equal values.  The margin is measured against the same mean evaluated in fp64, which returns y to fp64's own
    rounding."""
    n, window, stride = layout
    rng = np.random.default_rng(n + window)
    y = rng.standard_normal((2, 3, n)).astype(np.float32)
    y[0, 0, 0], y[0, 0, -1] = -0.0, -0.0
    w = WO.weight(window, stride, taper)
    got = WO.fuse32(WO.gather(y, window, stride), w, n, stride)
    J = WO.cover(n, window, stride)
    s = WO.starts(n, window, stride)
    single = np.array([len(c) == 1 for c in J])
    assert single[0] and single[-1]
    assert np.array_equal(got[:, :, single].view(np.uint32), y[:, :, single].view(np.uint32))
    multi = np.flatnonzero(~single)
    if len(multi) == 0:
        assert stride == window and n % window == 0 or n <= window
        return
    y64, w64 = y.astype(np.float64), w.astype(np.float64)
    mean64 = np.stack([sum(w64[l - s[j]] * y64[:, :, l] for j in J[l]) / sum(w64[l - s[j]] for j in J[l]) for l in multi], -1)
    assert np.abs(mean64 - y64[:, :, multi]).max() <= 4 * np.finfo(np.float64).eps * np.abs(y64).max()
    ulp = np.spacing(np.abs(y[:, :, multi])).astype(np.float64)
    err = np.abs(got[:, :, multi].astype(np.float64) - mean64) / ulp
    print(f"partition of unity {layout} {taper}: worst error {err.max():.3f} ulp over {err.size} multiply covered elements")
    assert err.max() <= 2.0


def test_oracle_cover_matches_the_closed_form():
    """The window range of a frame from l, stride and window alone (what the kernel computes) against the search over the starts."""
    for n, window, stride in LAYOUTS[:-1]:
        W = len(WO.starts(n, window, stride))
        for l, J in enumerate(WO.cover(n, window, stride)):
            j_lo = (l - window) // stride + 1 if l >= window else 0
            j_hi = min(l // stride, W - 2)
            closed = list(range(j_lo, j_hi + 1)) + ([W - 1] if l >= n - window else [])
            assert closed == J, (n, window, stride, l)


# ---- the arguments of sample() --------------------------------------------------------------------------------------------------------------
BACKBONE_KW = {"dit": dict(backbone="dit", dim_h=96, depth=2, attn_heads=6, attn_dim_head=16),
               "mmdit": dict(backbone="mmdit", dim_h=32, depth=2, attn_heads=2, attn_kv_heads=1, attn_dim_head=16)}
MODELS = {"dit_ddim": lambda bb: DiffusionOsuFusionDiT(**BACKBONE_KW[bb]), "dit_flow": lambda bb: RectifiedFlowOsuFusionDiT(**BACKBONE_KW[bb]),
          "ct_ddpm": lambda bb: ContinuousDiffusionOsuFusionDiT(**BACKBONE_KW[bb]),
          "ct_2m": lambda bb: ContinuousDiffusionOsuFusionDiT(sampler="dpmpp_2m", **BACKBONE_KW[bb])}


def test_plan_defaults():
    assert windowed.plan(None, None, "trapezoid", None) is None
    assert windowed.plan(4096, None, "trapezoid", None, 4) == (4096, 3072, "trapezoid", None)
    assert windowed.plan(96, None, "flat", 4, 1) == (96, 72, "flat", 4)
    assert windowed.plan(10, None, "trapezoid", None, 1).stride == 7
    assert windowed.plan(12, None, "trapezoid", None, 4).stride == 8   # 9 rounded down to a multiple of the patch size
    assert windowed.plan(96, 96, "trapezoid", None, 4).stride == 96


@pytest.mark.parametrize("kind", list(MODELS))
@pytest.mark.parametrize("backbone", ["dit", "mmdit"])
def test_sample_rejects_bad_window_arguments(kind, backbone):
    model = MODELS[kind](backbone)
    a, c = torch.zeros(2, 96, 64), torch.zeros(2, 5)
    bad = [dict(window=0), dict(window=-4), dict(window=16, window_stride=0), dict(window=16, window_stride=20), dict(window=16, window_stride=-4),
           dict(window=16, window_taper="hann"), dict(window=16, window_batch=0), dict(window=16, window_batch=-1),
           dict(window_stride=12), dict(window_taper="flat"), dict(window_batch=2), dict(window_stride=12, window_batch=2)]
    for kw in bad:
        with pytest.raises(ValueError, match="window"):
            model.sample(a, c, **kw)
    if backbone == "mmdit":                                            # patch size 4: window, the stride and a windowed n are multiples of it
        assert model.unet.patch_size == 4
        for kw in (dict(window=18), dict(window=16, window_stride=10)):
            with pytest.raises(ValueError, match="patch size"):
                model.sample(a, c, **kw)
        with pytest.raises(ValueError, match="patch size"):
            model.sample(torch.zeros(2, 96, 66), c, window=16)
        with pytest.raises(ValueError, match="window"):               # the default stride of window 4 would be 3 -> 0
            model.sample(a, c, window=4)
    for kw in (dict(window=16), dict(window=16, window_stride=12, window_taper="flat", window_batch=3), dict(window=64), dict(window=128)):
        with pytest.raises(RuntimeError, match="MI355X"):              # past the checks, at the GPU-only guard
            model.sample(a, c, **kw)


def test_module_imports_without_a_gpu():
    assert windowed.TAPERS == ("trapezoid", "flat")
    assert callable(windowed.window_gather) and callable(windowed.window_fuse)
