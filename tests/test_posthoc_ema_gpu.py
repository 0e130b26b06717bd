"""Post-hoc EMA on the GPU: osuf_lincomb at the kernel level (through tests/memguard.py's poisoned, canary-guarded allocations), and the
Trainer that writes the snapshots, reconstructs from them and swaps the reconstruction in (osufusion_amd/posthoc_ema.py, train.py).

Bounds are computed per element from the inputs.  osuf_lincomb runs a = fma(w_k, x_k, a) in fp64, k ascending from a = 0: each step rounds
once, by at most 2^-53 |a_k|, and |a_k| <= S = sum_k |w_k x_k|, so the accumulator lies within K 2^-53 S of the exact sum (the reference
is summed exactly: _exact_error).  The fp32 output is the rounding of the accumulator: its bits must be
float32(acc)'s; against an fp64 reference it may be off by the accumulator bound plus half an fp32 spacing, 2^-24 |ref|."""
import ctypes
import gc
import math

import numpy as np
import pytest
import torch

from osufusion_amd import _lib, forced_compute_dtype, ops
from osufusion_amd import functional as Fn
from osufusion_amd.ema import EMAConfig, sigma_rel_to_gamma
from osufusion_amd.posthoc_ema import SnapshotConfig, SnapshotStore, reconstruct
from tests.memguard import guard

pytestmark = pytest.mark.gpu
DEV = "cuda"
EINVAL = -1
NS = [1, 3, 4, 5, 4099, 65537]
KS = [1, 2, 8]


def _bits32(t):
    return t.contiguous().view(torch.int32)


def _bits64(t):
    return t.contiguous().view(torch.int64)


def _same(a, b):
    view = _bits64 if a.dtype == torch.float64 else _bits32
    return a.dtype == b.dtype and torch.equal(view(a), view(b))


def _case(n, K, seed=0):
    """K fp32 sources of mixed magnitude and K fp64 weights of mixed sign, up to 50 in magnitude."""
    rng = np.random.default_rng(1000 * n + 10 * K + seed)
    xs = (rng.standard_normal((K, n)) * 10.0 ** rng.integers(-3, 3, size=(K, 1))).astype(np.float32)
    w = rng.uniform(-50.0, 50.0, size=K)
    w[0] = 50.0 if K > 1 else -37.25
    return xs, w


def _split(w):
    """Veltkamp: w = hi + lo with at most 26 significant bits each, so that hi * x and lo * x are exact in fp64 for an fp32 x."""
    c = w * (2.0 ** 27 + 1.0)
    hi = c - (c - w)
    return hi, w - hi


def _exact_error(acc, xs, w):
    """(|acc - sum_k w_k x_k| with the sum taken exactly, S = sum_k |w_k x_k|), per element.  The 2K partial products are exact fp64
    numbers; math.fsum adds them and -acc without error and rounds once, so the error itself is known to 2^-53 of its own size."""
    hi, lo = _split(np.asarray(w, dtype=np.float64))
    x64 = xs.astype(np.float64)
    terms = np.concatenate([hi[:, None] * x64, lo[:, None] * x64, -np.asarray(acc, dtype=np.float64)[None]])
    err = np.abs(np.array([math.fsum(col) for col in terms.T]))
    return err, np.abs(np.asarray(w)[:, None] * x64).sum(axis=0)


def _poisoned(t):
    return bool((t.contiguous().view(torch.uint8) == 0xFF).all())


def _raw(ptrs, ws, K, acc, out, n, flags):
    p = (ctypes.c_void_p * 8)(*ptrs)
    w = (ctypes.c_double * 8)(*ws)
    return _lib.load().osuf_lincomb(ctypes.cast(p, ctypes.c_void_p), ctypes.cast(w, ctypes.c_void_p), K, acc, out, n, flags,
                                    torch.cuda.current_stream().cuda_stream)


# ---- the kernel ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("n", NS)
def test_lincomb_against_fp64(n, K):
    xs, w = _case(n, K)
    with guard(0xFF) as gd:
        srcs = [gd.place(torch.from_numpy(x)) for x in xs]
        acc, out = torch.empty(n, dtype=torch.float64, device=DEV), torch.empty(n, device=DEV)
        ops.lincomb(srcs, w, acc=acc, out=out)
        gd.check()
        err, S = _exact_error(acc.cpu().numpy(), xs, w)
        bound = K * 2.0 ** -53 * S
        print(f"lincomb n={n} K={K}: worst acc error / bound = {(err / np.maximum(bound, 1e-300)).max():.3f}")
        assert (err <= bound).all()
        assert _same(out, acc.float())
        # either output alone: the same bits
        acc2, out2 = torch.empty(n, dtype=torch.float64, device=DEV), torch.empty(n, device=DEV)
        ops.lincomb(srcs, w, acc=acc2)
        ops.lincomb(srcs, w, out=out2)
        gd.check()
        assert _same(acc2, acc) and _same(out2, out)
        for s, x in zip(srcs, xs):
            assert _same(s, torch.from_numpy(x).to(DEV))                     # the sources are read only
        gd.release()


@pytest.mark.parametrize("n", [5, 4099, 65537])
def test_grouping_does_not_change_a_bit(n):
    xs, w = _case(n, 8, seed=1)
    with guard(0xFF) as gd:
        srcs = [gd.place(torch.from_numpy(x)) for x in xs]
        results = []
        for cuts in ([8], [4, 4], [3, 3, 2], [1, 7], [1] * 8):
            acc, out = torch.empty(n, dtype=torch.float64, device=DEV), torch.empty(n, device=DEV)
            k = 0
            for g, size in enumerate(cuts):
                last = g == len(cuts) - 1
                ops.lincomb(srcs[k:k + size], w[k:k + size], acc=acc, out=out if last else None, cont=g > 0)
                k += size
            results.append((acc, out))
        gd.check()
        for acc, out in results[1:]:
            assert _same(acc, results[0][0]) and _same(out, results[0][1])
        gd.release()


@pytest.mark.parametrize("n", [3, 4099])
def test_zero_weight_is_a_select(n):
    xs, w = _case(n, 4, seed=2)
    with guard(0xFF) as gd:
        srcs = [gd.place(torch.from_numpy(x)) for x in xs]
        nan = torch.empty(n, device=DEV)                                       # poison: every element NaN
        assert torch.isnan(nan).all()
        acc, out = torch.empty(n, dtype=torch.float64, device=DEV), torch.empty(n, device=DEV)
        ops.lincomb(srcs, w, acc=acc, out=out)
        acc2, out2 = torch.empty(n, dtype=torch.float64, device=DEV), torch.empty(n, device=DEV)
        ops.lincomb([srcs[0], nan, srcs[1], srcs[2], nan, srcs[3]], [w[0], 0.0, w[1], w[2], -0.0, w[3]], acc=acc2, out=out2)
        gd.check()
        assert torch.isfinite(acc2).all() and _same(acc2, acc) and _same(out2, out)
        # every weight zero: the accumulator as it stands (continue) or zero
        acc3, out3 = acc.clone(), torch.empty(n, device=DEV)
        ops.lincomb([nan], [0.0], acc=acc3, out=out3, cont=True)
        assert _same(acc3, acc) and _same(out3, out)
        ops.lincomb([nan, nan], [0.0, 0.0], out=out3)
        assert torch.equal(out3, torch.zeros(n, device=DEV))
        # a source under a zero weight need not exist
        stream_ok = _raw([srcs[0].data_ptr(), None], [w[0], 0.0], 2, acc3.data_ptr(), None, n, 0)
        assert stream_ok == 0
        gd.check()
        gd.release()


def test_bad_arguments_return_a_code_and_launch_nothing():
    n = 4099
    xs, w = _case(n, 8, seed=3)
    with guard(0xFF) as gd:
        srcs = [gd.place(torch.from_numpy(x)) for x in xs]
        acc, out = torch.empty(n, dtype=torch.float64, device=DEV), torch.empty(n, device=DEV)
        ptrs, ws = [s.data_ptr() for s in srcs], list(w)
        a, o = acc.data_ptr(), out.data_ptr()
        assert _raw(ptrs, ws, 0, a, o, n, 0) == EINVAL
        assert _raw(ptrs, ws, 9, a, o, n, 0) == EINVAL
        assert _raw(ptrs, ws, -1, a, o, n, 0) == EINVAL
        assert _raw(ptrs, ws, 8, a, o, -1, 0) == EINVAL
        assert _raw(ptrs, ws, 8, None, None, n, 0) == EINVAL                   # nowhere to write
        assert _raw(ptrs, ws, 8, None, o, n, 1) == EINVAL                      # continue without an accumulator
        assert _raw(ptrs, [float("nan")] + ws[1:], 8, a, o, n, 0) == EINVAL
        assert _raw(ptrs, ws[:7] + [float("nan")], 8, a, o, n, 0) == EINVAL
        assert _raw(ptrs[:3] + [None] + ptrs[4:], ws, 8, a, o, n, 0) == EINVAL  # a NULL source under a non-zero weight
        assert _lib.load().osuf_lincomb(None, None, 1, a, o, n, 0, torch.cuda.current_stream().cuda_stream) == EINVAL
        assert _raw(ptrs, ws, 8, a, o, 0, 0) == 0                              # nothing to do is not an error
        gd.check()
        assert _poisoned(acc) and _poisoned(out)
        with pytest.raises(RuntimeError, match="invalid argument"):
            ops.lincomb(srcs + [srcs[0]], list(w) + [1.0], acc=acc)
        assert _poisoned(acc)
        gd.release()


@pytest.mark.parametrize("n", [1, 5, 4099, 65537])
def test_misaligned_pointers_give_the_same_bits(n):
    """Every buffer 4 bytes (fp32) or 8 bytes (the fp64 accumulator: its own alignment) past its allocation, singly and together: the
    one-element-per-lane path, the bits of the four-wide one."""
    K = 3
    xs, w = _case(n, K, seed=4)
    with guard(0xFF) as gd:
        srcs = [gd.place(torch.from_numpy(x)) for x in xs]
        acc, out = torch.empty(n, dtype=torch.float64, device=DEV), torch.empty(n, device=DEV)
        ops.lincomb(srcs, w, acc=acc, out=out)
        shifted = []
        for x in xs:
            buf = torch.empty(n + 1, device=DEV)
            buf[1:] = torch.from_numpy(x).to(DEV)
            shifted.append(buf[1:])
            assert buf[1:].data_ptr() % 16 == 4
        acc_s, out_s = torch.empty(n + 1, dtype=torch.float64, device=DEV), torch.empty(n + 1, device=DEV)
        for which in ("src0", "acc", "out", "all"):
            use = [shifted[0] if which in ("src0", "all") else srcs[0], *(shifted[1:] if which == "all" else srcs[1:])]
            a = acc_s[1:] if which in ("acc", "all") else torch.empty(n, dtype=torch.float64, device=DEV)
            o = out_s[1:] if which in ("out", "all") else torch.empty(n, device=DEV)
            ops.lincomb(use, w, acc=a, out=o)
            gd.check()
            assert _same(a, acc) and _same(o, out), which
            a2 = acc_s[1:] if which in ("acc", "all") else a
            ops.lincomb(use[:1], w[:1], acc=a2)
            ops.lincomb(use[1:], w[1:], acc=a2, out=o, cont=True)
            assert _same(a2, acc) and _same(o, out), which
        # the element in front of every shifted view was not written
        assert _poisoned(acc_s[:1]) and _poisoned(out_s[:1])
        gd.check()
        gd.release()


# ---- Trainer ------------------------------------------------------------------------------------------------------------------------------------
NAME = "dit_h96"                                                               # the smallest DiT of the existing GPU tests
TRACKS = (EMAConfig(kind="power", sigma_rel=0.05), EMAConfig(kind="power", sigma_rel=0.10))
STEPS, EVERY = 12, 3


def _trainer(**kw):
    from osufusion_amd.models import DiffusionOsuFusionDiT
    from osufusion_amd.train import Trainer
    from tests.test_transformer_sampling_gpu import _inputs, _model
    model = _model(DiffusionOsuFusionDiT, NAME, sampling_timesteps=2)
    model.cond_drop_prob = 0.0
    x, a, c, t, noise = _inputs(NAME)
    return Trainer(model, lr=1e-3, compute_dtype=torch.float32, **kw), (x, a, c, noise, t)


@pytest.fixture(autouse=True)
def _leave_no_hooks_behind():
    yield
    Fn.enable_direct_grads(False)
    gc.collect()


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """One trainer with two power tracks after STEPS optimizer steps with a snapshot every EVERY: (trainer, batch, store).  Read only."""
    d = tmp_path_factory.mktemp("snapshots")
    tr, batch = _trainer(ema=TRACKS, ema_snapshots=SnapshotConfig(d, EVERY))
    for _ in range(STEPS):
        tr.step(*batch)
    yield tr, batch, SnapshotStore(d)
    Fn.enable_direct_grads(False)
    del tr
    gc.collect()


def _rows(store, info):
    """Every stored row, snapshot-major as reconstruct's weights, fp64 on the host: (K, n)."""
    return np.concatenate([store.load(s)["tracks"].double().numpy() for s in info["steps"]])


def _flat(named, info):
    return torch.cat([named[k].reshape(-1) for k in info["names"]])


def test_trainer_writes_snapshots_and_reconstruction_matches(trained):
    tr, _, store = trained
    assert store.list() == [3, 6, 9, 12]
    info = store.check()
    names = [k for k, p in tr.model.named_parameters() if p.requires_grad]
    assert info["names"] == names and info["ema_steps"] == [3, 6, 9, 12]
    assert info["gammas"] == [c.power_gamma() for c in TRACKS]
    last = store.load(12)["tracks"]
    for g in range(2):                                                         # the last file holds the tracks as they stand
        assert _same(last[g], torch.cat([v.reshape(-1) for v in tr.opt.ema_state_dict(tr.model)[g].values()]).cpu())
    rows = _rows(store, info)
    K = rows.shape[0]
    assert K == 8

    # the target is a stored profile: the weights are its unit vector up to rounding, the result the track itself
    named, w = reconstruct(store, gamma=info["gammas"][0], at_step=12, device=DEV)
    assert list(named) == names and w.shape == (K,) and w.dtype == np.float64
    delta = np.zeros(K)
    delta[6] = 1.0                                                             # snapshot 12 (index 3), track 0
    want = torch.cat([tr.ema_state_dict(0)[k].reshape(-1) for k in names]).double().cpu().numpy()
    bound = (np.abs(w - delta)[:, None] * np.abs(rows)).sum(axis=0) + 2.0 ** -24 * np.abs(want)
    err = np.abs(_flat(named, info).double().cpu().numpy() - want)
    print(f"reconstruct(track 0's gamma): |w - delta| max {np.abs(w - delta).max():.3e}; worst error {err.max():.3e}")
    assert (err <= bound).all()
    for k, p in tr.model.named_parameters():
        assert named[k].shape == p.shape

    # off the grid: the fp64 combination of the same files with the same weights; three launches (3 + 3 + 2) and one give the same bits
    named3, w3 = reconstruct(store, sigma_rel=0.075, device=DEV, max_resident=3)
    named8, w8 = reconstruct(store, sigma_rel=0.075, device=DEV, max_resident=64)
    assert np.array_equal(w3, w8) and np.abs(w3).max() > 1e-3
    got3, got8 = _flat(named3, info), _flat(named8, info)
    assert _same(got3, got8)
    wl, xl = w3.astype(np.longdouble)[:, None], rows.astype(np.longdouble)
    ref, S = (wl * xl).sum(axis=0), np.abs(wl * xl).sum(axis=0)             # extended precision: 2^-64, far below either term
    err = np.abs(got3.double().cpu().numpy().astype(np.longdouble) - ref)
    bound = K * 2.0 ** -53 * S + 2.0 ** -24 * np.abs(ref)
    print(f"reconstruct(sigma_rel 0.075): weights {np.array2string(w3, precision=4)}; worst error / bound {(err / np.maximum(bound, 1e-300)).max():.3f}")
    assert (err <= bound).all()
    assert not torch.equal(got3, torch.from_numpy(rows[6]).float().to(DEV))    # not simply a stored track

    # an earlier end point uses the earlier files only
    _, w6 = reconstruct(store, sigma_rel=0.075, at_step=6, device=DEV)
    assert w6.shape == (4,)
    with pytest.raises(ValueError):
        reconstruct(store, device=DEV)
    with pytest.raises(ValueError):
        reconstruct(store, sigma_rel=0.075, gamma=5.0, device=DEV)
    with pytest.raises(ValueError):
        reconstruct(store, sigma_rel=0.075, at_step=2, device=DEV)


def test_posthoc_weights_context(trained):
    tr, batch, store = trained
    x, a, c, _, _ = batch
    named, _ = reconstruct(store, sigma_rel=0.075, device=DEV)
    live, tracks = tr.flat.data.clone(), tr.opt.ema.clone()
    for source, kw in ((store, dict(sigma_rel=0.075)), (store.dir, dict(gamma=sigma_rel_to_gamma(0.075), at_step=12)), (named, {})):
        with tr.posthoc_weights(source, **kw) as m:
            assert m is tr.model
            sd = tr.model.state_dict()
            for k, v in named.items():
                assert _same(sd[k], v), k
            assert not torch.equal(tr.flat.data, live)
            with forced_compute_dtype(torch.float32):
                y = tr.model.sample(a, c, x, cond_scale=2.0)
            assert torch.isfinite(y).all()
            with pytest.raises(RuntimeError):
                tr.step(*batch)
            with pytest.raises(RuntimeError):
                with tr.posthoc_weights(named):
                    pass
            with pytest.raises(RuntimeError):
                with tr.ema_weights(0):
                    pass
            with pytest.raises(RuntimeError):
                tr.state_dict()
            assert _same(tr.opt.ema, tracks)
        assert _same(tr.flat.data, live) and _same(tr.opt.ema, tracks)
    with pytest.raises(ValueError):
        with tr.posthoc_weights(named, sigma_rel=0.075):
            pass
    with pytest.raises(ValueError):
        with tr.posthoc_weights({k: v for k, v in list(named.items())[1:]}):
            pass
    assert _same(tr.flat.data, live) and tr._ema_swapped is None


def test_command_line_tool_writes_a_loadable_model_file(trained, tmp_path, capsys):
    import importlib.util
    from pathlib import Path
    from osufusion_amd import data as D
    from osufusion_amd.models import DiffusionOsuFusionDiT
    from tests.test_transformer_sampling_gpu import _model
    tr, _, store = trained
    spec = importlib.util.spec_from_file_location("posthoc_ema_tool", Path(__file__).resolve().parent.parent / "tools" / "posthoc_ema.py")
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    named, _ = reconstruct(store, sigma_rel=0.075, at_step=9, device=DEV)
    for suffix in (".safetensors", ".pt"):
        out = tmp_path / ("posthoc" + suffix)
        assert tool.main(["--dir", str(store.dir), "--sigma-rel", "0.075", "--at-step", "9", "--out", str(out)]) == 0
        assert "6 stored tracks" in capsys.readouterr().out
        other = _model(DiffusionOsuFusionDiT, NAME)
        res = D.load_model_sd(other, out, strict=False)
        assert res["unexpected"] == [] and not set(res["missing"]) & set(named)
        sd = other.state_dict()
        for k, v in named.items():
            assert _same(sd[k], v), k


def test_no_change_when_off(tmp_path, monkeypatch):
    from tests.test_ema_gpu import _twin_step
    calls = []
    orig = ops.call
    monkeypatch.setattr(ops, "call", lambda name, *args, **kw: (calls.append(name), orig(name, *args, **kw))[1])
    monkeypatch.setattr(SnapshotStore, "write", lambda *a, **k: pytest.fail("a snapshot was written"))
    monkeypatch.chdir(tmp_path)
    plain, batch = _trainer(ema=TRACKS)
    off, _ = _trainer(ema=TRACKS, ema_snapshots=None)
    assert off.snapshots is None
    for _ in range(3):
        del calls[:]
        plain.step(*batch)
        mine = list(calls)
        del calls[:]
        off.step(*batch)
        assert not set(calls) - set(mine) and "osuf_lincomb" not in calls       # no kernel the plain trainer does not launch
        assert calls.count("osuf_adamw_ema") == mine.count("osuf_adamw_ema") == 1
    plain, _ = _trainer(ema=TRACKS)
    off, _ = _trainer(ema=TRACKS, ema_snapshots=None)
    for _ in range(3):
        _twin_step(plain, off, batch)                                          # one gradient for both: two backwards never agree to the bit
    for (k, p), (k2, q) in zip(plain.model.named_parameters(), off.model.named_parameters()):
        assert k == k2 and _same(p.detach(), q.detach()), k
    for j in range(2):
        for (k, e), (k2, f) in zip(plain.ema_state_dict(j).items(), off.ema_state_dict(j).items()):
            assert k == k2 and _same(e, f), k
    assert list(tmp_path.iterdir()) == []


def test_snapshots_need_a_power_track_and_follow_optimizer_steps(tmp_path):
    with pytest.raises(ValueError, match="power"):
        _trainer(ema=EMAConfig(kind="constant", beta=0.9), ema_snapshots=SnapshotConfig(tmp_path / "a", 1))
    with pytest.raises(ValueError, match="power"):
        _trainer(ema_snapshots=SnapshotConfig(tmp_path / "a", 1))
    Fn.enable_direct_grads(False)
    # two micro-batches per optimizer step; a constant track next to the power one is not stored
    cfg = (EMAConfig(kind="constant", beta=0.9), TRACKS[1])
    tr, batch = _trainer(ema=cfg, ema_snapshots=SnapshotConfig(tmp_path / "b", 1), gradient_accumulation_steps=2)
    for micro in range(4):
        tr.step(*batch)
        assert SnapshotStore(tmp_path / "b").list() == list(range(1, micro // 2 + 1 + (micro % 2)))
    info = SnapshotStore(tmp_path / "b").check()
    assert info["steps"] == [1, 2] and info["gammas"] == [TRACKS[1].power_gamma()]
    d = SnapshotStore(tmp_path / "b").load(2)
    assert _same(d["tracks"][0], torch.cat([v.reshape(-1) for v in tr.opt.ema_state_dict(tr.model)[1].values()]).cpu())
