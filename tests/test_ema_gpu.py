"""EMA tracks of the weights on the GPU: osuf_adamw_ema / osuf_ema_update / osuf_swap at the kernel level, and the Trainer that keeps,
re-lays, swaps in and checkpoints the tracks (osufusion_amd/train.py, osufusion_amd/ema.py).

The one tolerance here is derived, not measured.  A blending step computes e' = fma(d, p - e, e) in fp32: one rounding of the difference
(a quantity of at most 2M, so at most 2^-24 * 2M of error, scaled by d <= 1) and one of the result (at most 2^-24 * M); the issue's budget
allows a third for an unfused multiply.  The recurrence multiplies the error already in e by 1 - d <= 1, so K steps stay within
5 * K * 2^-24 * M of the fp64 recurrence over the same fp32 parameters with the same fp32 d, M = the largest magnitude seen in p and e."""
import gc
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from osufusion_amd import _lib, forced_compute_dtype, ops
from osufusion_amd import functional as Fn
from osufusion_amd.ema import EMAConfig, ema_d
from osufusion_amd.pattern import synth_inputs
from tests.memguard import guard

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = Path(__file__).resolve().parent.parent

# ew_grid caps the grid; beyond cap * 256 lanes * 4 elements the grid-stride loop of the four-wide body wraps
_CAP = int(re.search(r"if \(blocks > (\d+)\) blocks = \1;", (ROOT / "osufusion_amd" / "csrc" / "common.hpp").read_text()).group(1))
NS = [1, 3, 4, 5, 1023, 1024, 4099, _CAP * 256 * 4 + 5]
DS = [float(np.float32(v)) for v in (0.1, 0.003, 0.25, 0.6)]
HYPER = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8)
EINVAL = -1


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _state(n, tracks, ld=None):
    ld = (n + 3) // 4 * 4 if ld is None else ld
    p, g = torch.randn(n, device=DEV), torch.randn(n, device=DEV)
    m, v = 0.1 * torch.randn(n, device=DEV), 0.01 * torch.rand(n, device=DEV)
    return p, g, m, v, torch.randn(tracks, ld, device=DEV)


def _raw_adamw_ema(p, g, m, v, n, ema, ld, tracks, d=(0.5, 0.5, 0.5, 0.5), step=1, ema_ptr=None):
    return _lib.load().osuf_adamw_ema(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, 1e-2, 0.9, 0.999, 1e-8, 1e-2, step, None,
                                      ema.data_ptr() if ema_ptr is None else ema_ptr, ld, tracks, *d, torch.cuda.current_stream().cuda_stream)


def _raw_ema_update(p, n, ema, ld, tracks, d=(0.5, 0.5, 0.5, 0.5), ema_ptr=None):
    return _lib.load().osuf_ema_update(p.data_ptr(), ema.data_ptr() if ema_ptr is None else ema_ptr, ld, n, tracks, *d,
                                       torch.cuda.current_stream().cuda_stream)


# ---- kernels --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tracks", [1, 2, 4])
@pytest.mark.parametrize("n", NS)
def test_fused_pass_is_adamw_plus_the_standalone_track_update(n, tracks):
    """p, m, v after osuf_adamw_ema == after osuf_adamw on clones, bitwise; the tracks == osuf_ema_update applied to the fused call's p."""
    for step, (with_scale, wd) in enumerate([(False, 0.0), (True, 1e-2), (False, 1e-2), (True, 0.0)], start=1):
        p, g, m, v, ema = _state(n, tracks)
        gscale = torch.tensor([0.37], device=DEV) if with_scale else None
        p0, m0, v0, ema0 = p.clone(), m.clone(), v.clone(), ema.clone()
        ops.adamw(p0, g, m0, v0, wd=wd, step=step, gscale=gscale, **HYPER)
        ops.adamw_ema(p, g, m, v, wd=wd, step=step, gscale=gscale, ema=ema, d=DS[:tracks], **HYPER)
        assert _same(p, p0) and _same(m, m0) and _same(v, v0), (n, tracks, with_scale, wd)
        assert not torch.equal(ema[:, :n], ema0[:, :n])
        ops.ema_update(p, ema0, DS[:tracks])
        assert _same(ema, ema0), (n, tracks, with_scale, wd)


def test_tracks_follow_the_fp64_recurrence_over_twenty_steps():
    K, n, tracks = 20, 4099, 4
    p, g, m, v, ema = _state(n, tracks)
    ema[:, :n] = p                                                            # tracks start as copies of the weights
    e64 = ema[:, :n].double()
    big = max(p.abs().max().item(), e64.abs().max().item())
    d64 = torch.tensor(DS, dtype=torch.float64, device=DEV)[:, None]          # the fp32 values, widened exactly
    for k in range(1, K + 1):
        g.normal_()
        ops.adamw_ema(p, g, m, v, wd=1e-2, step=k, gscale=None, ema=ema, d=DS, **HYPER)
        e64 += d64 * (p.double()[None] - e64)
        big = max(big, p.abs().max().item(), e64.abs().max().item())
    err = (ema[:, :n].double() - e64).abs().max().item()
    bound = 5 * K * 2.0 ** -24 * big
    print(f"ema vs fp64 recurrence after {K} steps: max abs err {err:.3e}, bound {bound:.3e} (M = {big:.3f})")
    assert err <= bound
    assert (ema[:, :n].double() - p.double()[None]).abs().max().item() > 100 * bound        # the tracks did lag behind the weights


@pytest.mark.parametrize("n", [3, 5, 4099])
@pytest.mark.parametrize("d", [(0.0, DS[0], 1.0), (DS[0], 0.0, 1.0), (1.0, DS[1], 0.0), (2.0, 0.0, DS[2])], ids=lambda d: "-".join(f"{x:g}" for x in d))
def test_d_of_zero_and_one_are_selects(n, d):
    """d == 0: the track's bits stay (also bits no arithmetic would return: NaN payloads, -0.0); d >= 1: the new p itself, whatever the
    track held (NaN, inf); the neighbouring track blends as usual.  Fused and standalone."""
    for fused in (True, False):
        p, g, m, v, ema = _state(n, 3)
        odd = torch.tensor([0x7FC01234, -0x00400000 + 0x1ABC, -0x80000000, 0x7F800000, 0x00000001], dtype=torch.int32, device=DEV).view(torch.float32)
        for j, dj in enumerate(d):
            if dj == 0.0 or dj >= 1.0:
                ema[j, :n] = odd.repeat(n // 5 + 1)[:n]
        ema0 = ema.clone()
        if fused:
            ops.adamw_ema(p, g, m, v, wd=1e-2, step=2, gscale=None, ema=ema, d=d, **HYPER)
        else:
            ops.ema_update(p, ema, d)
        for j, dj in enumerate(d):
            if dj == 0.0:
                assert _same(ema[j], ema0[j]), (fused, j)
            elif dj >= 1.0:
                assert _same(ema[j, :n], p), (fused, j)
            else:
                want = ema0[j, :n].double() + float(dj) * (p.double() - ema0[j, :n].double())
                assert (ema[j, :n].double() - want).abs().max().item() <= 5 * 2.0 ** -24 * max(p.abs().max().item(), ema0[j, :n].abs().max().item())
                assert not torch.equal(ema[j, :n], ema0[j, :n])


@pytest.mark.parametrize("n,ld", [(1, 4), (5, 8), (1023, 1028), (1024, 1024), (4099, 4104)])
@pytest.mark.parametrize("tracks", [1, 2])
def test_nothing_is_written_outside_the_tracks(n, ld, tracks):
    """Canary-guarded buffers: rows at or beyond `tracks`, the padding n..ema_ld of every row and the slack behind every buffer keep
    their bits; so do g and the unused rows under the standalone entry point."""
    with guard(0xFF) as gd:
        bufs = [torch.empty(n, device=DEV) for _ in range(4)]
        ema = torch.empty(4, ld, device=DEV)
        for b in (*bufs, ema):
            b.normal_()
        p, g, m, v = bufs
        v.abs_()
        ema0, g0 = ema.clone(), g.clone()
        ops.adamw_ema(p, g, m, v, wd=1e-2, step=1, gscale=None, ema=ema[:tracks], d=DS[:tracks], **HYPER)
        gd.check()
        assert _same(ema[tracks:], ema0[tracks:]) and _same(ema[:, n:], ema0[:, n:]) and _same(g, g0)
        assert not torch.equal(ema[:tracks, :n], ema0[:tracks, :n])
        ema1, p1 = ema.clone(), p.clone()
        ops.ema_update(p, ema[:tracks], DS[:tracks])
        gd.check()
        assert _same(ema[tracks:], ema1[tracks:]) and _same(ema[:, n:], ema1[:, n:]) and _same(p, p1)
        gd.release()


def test_bad_arguments_return_a_code_and_launch_nothing():
    n, ld = 1024, 1028
    p, g, m, v, ema = _state(n, 4, ld)
    keep = [t.clone() for t in (p, g, m, v, ema)]
    assert _raw_adamw_ema(p, g, m, v, n, ema, ld, 0) == EINVAL
    assert _raw_adamw_ema(p, g, m, v, n, ema, ld, 5) == EINVAL
    assert _raw_adamw_ema(p, g, m, v, n, ema, n - 1, 1) == EINVAL                      # ema_ld < n
    assert _raw_adamw_ema(p, g, m, v, n, ema, n + 1, 2) == EINVAL                      # ema_ld not a multiple of 4 floats, four-wide path
    assert _raw_adamw_ema(p, g, m, v, n - 4, ema, ld, 1, ema_ptr=ema.data_ptr() + 4) == EINVAL       # ema itself off a 16-byte boundary
    assert _raw_adamw_ema(p, g, m, v, n, ema, ld, 2, d=(0.5, -0.1, 0.5, 0.5)) == EINVAL
    assert _raw_adamw_ema(p, g, m, v, n, ema, ld, 2, d=(0.5, float("nan"), 0.5, 0.5)) == EINVAL
    assert _raw_adamw_ema(p, g, m, v, n, ema, ld, 1, ema_ptr=0) == EINVAL
    assert _raw_ema_update(p, n, ema, ld, 0) == EINVAL and _raw_ema_update(p, n, ema, ld, 5) == EINVAL
    assert _raw_ema_update(p, n, ema, n - 1, 1) == EINVAL and _raw_ema_update(p, n, ema, n + 1, 2) == EINVAL
    assert _raw_ema_update(p, n - 4, ema, ld, 1, ema_ptr=ema.data_ptr() + 4) == EINVAL
    torch.cuda.synchronize()
    for t, k in zip((p, g, m, v, ema), keep):
        assert _same(t, k)
    with pytest.raises(RuntimeError, match="invalid argument"):
        ops.adamw_ema(p, g, m, v, wd=0.0, step=0, gscale=None, ema=ema, d=DS, **HYPER)   # what osuf_adamw rejects
    # the scalar tail alone (n < 4) needs no alignment of the tracks: an odd ema_ld and an ema off the boundary are served
    q, gq, mq, vq, e = _state(3, 2, 7)
    e0, q0, m0, v0 = e.clone(), q.clone(), mq.clone(), vq.clone()
    assert _raw_adamw_ema(q, gq, mq, vq, 3, e, 7, 1, d=(1.0, 0.0, 0.0, 0.0), ema_ptr=e.data_ptr() + 4) == 0
    ops.adamw(q0, gq, m0, v0, wd=1e-2, step=1, gscale=None, **HYPER)
    assert _same(q, q0) and _same(e[0, 1:4], q) and _same(e[0, :1], e0[0, :1]) and _same(e[0, 4:], e0[0, 4:]) and _same(e[1], e0[1])


@pytest.mark.parametrize("n", NS)
def test_swap_exchanges_two_buffers(n):
    with guard(0xFF) as gd:
        a, b = torch.empty(n, device=DEV).normal_(), torch.empty(n, device=DEV).normal_()
        a0, b0 = a.clone(), b.clone()
        ops.swap(a, b)
        gd.check()
        assert _same(a, b0) and _same(b, a0)
        stream = torch.cuda.current_stream().cuda_stream
        assert _lib.load().osuf_swap(a.data_ptr(), a.data_ptr(), n, stream) == EINVAL
        if n > 8:
            assert _lib.load().osuf_swap(a.data_ptr(), a.data_ptr() + 16, n - 4, stream) == EINVAL      # overlapping ranges
        assert _same(a, b0) and _same(b, a0)
        ops.swap(b, a)
        assert _same(a, a0) and _same(b, b0)
        gd.release()


# ---- Trainer ----------------------------------------------------------------------------------------------------------------------------
MODELS = ["dit_h96", "mmdit_h96", "unet_tiny"]
TWO_TRACKS = (EMAConfig(kind="constant", beta=0.9), EMAConfig(kind="power", gamma=6.94))


@pytest.fixture(autouse=True)
def _leave_no_model_behind():
    """functional._PACK_JOBS is process-wide and other tests read all of it: a model of this file that only the cycle collector can free
    (parameter -> completion hook -> reducer -> flat buffers -> parameter) must be gone before the next test starts."""
    yield
    Fn.enable_direct_grads(False)
    gc.collect()


def _make(name, golden_dir):
    """The smallest configurations of the existing GPU tests, at their own B and L: (model, (x, a, c, noise, t))."""
    if name == "unet_tiny":
        from tests.test_hip_parity import _build_model
        meta, _, model = _build_model("unet_tiny", golden_dir)
        x, a, c, t, noise = (torch.from_numpy(v).to(DEV) for v in synth_inputs("unet_tiny", meta["B"], meta["L"]))
    else:
        from osufusion_amd.models import DiffusionOsuFusionDiT
        from tests.test_transformer_sampling_gpu import _inputs, _model
        model = _model(DiffusionOsuFusionDiT, name)
        x, a, c, t, noise = _inputs(name)
    model.cond_drop_prob = 0.0                                                # no draw from the generator inside a step
    return model, (x, a, c, noise, t)


def _trainer(name, golden_dir, **kw):
    from osufusion_amd.train import Trainer
    model, batch = _make(name, golden_dir)
    return Trainer(model, lr=1e-3, compute_dtype=torch.float32, **kw), batch


def _params(tr):
    return {k: p.detach().clone() for k, p in tr.model.named_parameters()}


def _twin_step(leader, follower, batch):
    """leader.step(batch), then follower.step(batch) with the follower's optimizer fed the LEADER's gradient, copied by parameter name
    just before its launch.  Two identically seeded trainers do not stay bitwise equal on their own: the backward kernels sum with float
    atomics, so two runs of one step differ in the last bits (measured on plain trainers without any EMA: 24 of 42 DiT tensors, 17 of 75
    MMDiT tensors and 427 of 495 UNet tensors differ after ONE step, by up to 3e-7, 7e-9 and 2e-3).  Given the same gradient bits the
    whole optimizer side -- norm, clip coefficient, AdamW with or without tracks, re-layout -- is deterministic, and that is what the twin
    comparisons below hold to bitwise equality.  The follower still runs its own forward and backward."""
    leader.step(*batch)
    grads = {leader.reducer.names[id(p)]: leader.flat.grad[o:o + p.numel()] for p, o in zip(leader.flat.params, leader.flat.offsets)}
    opt_step = follower.opt.step

    def step_on_leaders_gradient(*args, **kw):
        for p, o in zip(follower.flat.params, follower.flat.offsets):
            follower.flat.grad[o:o + p.numel()].copy_(grads[follower.reducer.names[id(p)]])
        return opt_step(*args, **kw)

    follower.opt.step = step_on_leaders_gradient
    try:
        follower.step(*batch)
    finally:
        del follower.opt.step


def _assert_same_dicts(a, b):
    assert list(a) == list(b)
    for k in a:
        assert _same(a[k], b[k]), k


class _Recurrence:
    """fp64 e += d (p - e) per parameter name, from the weights a trainer starts with; d is the fp32 value the kernel receives."""

    def __init__(self, tr, cfgs):
        self.cfgs, self.k = cfgs, 0
        start = _params(tr)
        self.e = [{k: v.double() for k, v in start.items()} for _ in cfgs]
        self.big = {k: v.abs().max().item() for k, v in start.items()}

    def advance(self, tr):
        self.k += 1
        for k, p in _params(tr).items():
            for j, cfg in enumerate(self.cfgs):
                self.e[j][k] += ema_d(cfg, self.k) * (p.double() - self.e[j][k])
                self.big[k] = max(self.big[k], p.abs().max().item(), self.e[j][k].abs().max().item())

    def check(self, tr):
        worst = 0.0
        for j in range(len(self.cfgs)):
            got = tr.ema_state_dict(j)
            for k, want in self.e[j].items():
                err, bound = (got[k].double() - want).abs().max().item(), 5 * self.k * 2.0 ** -24 * self.big[k]
                worst = max(worst, err / bound)
                assert err <= bound, (j, k, err, bound)
        return worst


@pytest.mark.parametrize("name", MODELS)
def test_tracks_do_not_disturb_training(name, golden_dir):
    """Twin trainers, one with two tracks: bitwise equal parameters after each of three steps (the first ends with the re-layout of the
    flat buffers), and each track within the derived bound of the fp64 recurrence over the per-step parameters, read by name.  The twin
    without tracks is stepped on the gradient bits of the one with tracks (see _twin_step: two backwards never agree to the bit)."""
    try:
        plain, batch = _trainer(name, golden_dir, reorder_buckets=True)
        with_ema, _ = _trainer(name, golden_dir, reorder_buckets=True, ema=TWO_TRACKS)
        _assert_same_dicts(_params(plain), _params(with_ema))
        ref = _Recurrence(with_ema, TWO_TRACKS)
        first_layout = [id(p) for p in with_ema.flat.params]
        for step in range(3):
            _twin_step(with_ema, plain, batch)
            _assert_same_dicts(_params(plain), _params(with_ema))
            ref.advance(with_ema)
            worst = ref.check(with_ema)
            print(f"{name} step {step + 1}: worst track error / bound = {worst:.3f}")
        relaid = [id(p) for p in with_ema.flat.params] != first_layout
        print(f"{name}: flat buffers re-laid out after step 1: {relaid}")
        assert relaid or name != "unet_tiny", "the UNet's completion order differs from the first guess (test_trainer_gradient_accumulation_and_relayout)"
        assert with_ema.opt.ema_step == 3 and with_ema.opt.ema.shape == (2, (with_ema.flat.numel + 3) // 4 * 4)
        moved = max((a - b).abs().max().item() for a, b in zip(with_ema.ema_state_dict(0).values(), with_ema.model.state_dict().values()))
        assert moved > 0.0                                                    # the constant-0.9 track lags behind the weights
        # a re-layout whatever order the backward completed in: reversed; every track still reads the same by name, and trains on
        by_name = [with_ema.ema_state_dict(j) for j in range(2)]
        backwards = list(reversed(range(len(with_ema.flat.params))))
        with_ema.reducer.observed_order = lambda: backwards
        with_ema.apply_observed_order()
        for j in range(2):
            _assert_same_dicts(by_name[j], with_ema.ema_state_dict(j))
        _twin_step(with_ema, plain, batch)
        _assert_same_dicts(_params(plain), _params(with_ema))
        ref.advance(with_ema)
        ref.check(with_ema)
    finally:
        Fn.enable_direct_grads(False)


def test_gradient_accumulation_moves_the_tracks_once_per_optimizer_step(golden_dir):
    cfg = (EMAConfig(kind="constant", beta=0.9),)
    try:
        tr, batch = _trainer("dit_h96", golden_dir, gradient_accumulation_steps=2, ema=cfg)
        ref = _Recurrence(tr, cfg)
        for micro in range(4):
            before = tr.opt.ema.clone()
            _, norm = tr.step(*batch)
            if micro % 2 == 0:
                assert norm is None and _same(tr.opt.ema, before)            # accumulation only: nothing moved
            else:
                ref.advance(tr)
                ref.check(tr)
        assert tr.opt.ema_step == 2 == tr.opt.step_count and ref.k == 2
    finally:
        Fn.enable_direct_grads(False)


def _eval_forward(model, batch):
    x, a, c, noise, t = batch
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad(), forced_compute_dtype(torch.float32), ops.reproducible_mode(True):
            return model.unet(x, a, t, c, cond_drop_prob=0.0).clone()
    finally:
        model.train(was_training)


@pytest.mark.parametrize("name", MODELS)
def test_ema_weights_context(name, golden_dir):
    cfg = (EMAConfig(kind="constant", beta=0.9), EMAConfig(kind="constant", beta=0.5))
    try:
        tr, batch = _trainer(name, golden_dir, ema=cfg)
        twin, _ = _trainer(name, golden_dir, ema=cfg)
        for _ in range(2):
            _twin_step(tr, twin, batch)
        live, tracks = tr.flat.data.clone(), tr.opt.ema.clone()
        y_live = _eval_forward(tr.model, batch)
        for track in (0, 1):
            averaged = tr.ema_state_dict(track)
            fresh, _ = _make(name, golden_dir)
            fresh.load_state_dict(averaged)
            want = _eval_forward(fresh, batch)
            with tr.ema_weights(track) as m:
                assert m is tr.model
                got = _eval_forward(tr.model, batch)
                _assert_same_dicts({k: v for k, v in tr.model.state_dict().items()}, averaged)
                _assert_same_dicts(tr.ema_state_dict(track), averaged)
                with pytest.raises(RuntimeError):
                    with tr.ema_weights(1 - track):
                        pass
                with pytest.raises(RuntimeError):
                    tr.step(*batch)
                with pytest.raises(RuntimeError):
                    tr.state_dict()
            assert _same(got, want) and torch.isfinite(got).all()
            assert not torch.equal(got, y_live)                               # the averaged weights are not the live ones
            assert _same(tr.flat.data, live) and _same(tr.opt.ema, tracks)
        assert _same(_eval_forward(tr.model, batch), y_live)                  # the packed operands are the live weights' again
        with pytest.raises(IndexError):
            with tr.ema_weights(2):
                pass
        _twin_step(tr, twin, batch)
        _assert_same_dicts(_params(tr), _params(twin))
        for track in (0, 1):                                                  # by name: the twins' flat layouts need not agree
            _assert_same_dicts(tr.ema_state_dict(track), twin.ema_state_dict(track))
    finally:
        Fn.enable_direct_grads(False)


def test_checkpoint_round_trip(golden_dir, capsys, tmp_path):
    name = "mmdit_h96"
    try:
        tr, batch = _trainer(name, golden_dir, ema=TWO_TRACKS)
        for _ in range(2):
            tr.step(*batch)
        ck = tr.state_dict()
        assert list(ck) == ["model_state_dict", "optimizer_state_dict", "scheduler_state_dict", "rng_state", "ema_state_dict", "ema_config", "ema_step"]
        assert ck["ema_step"] == 2 and ck["ema_config"] == [c.as_dict() for c in TWO_TRACKS]
        names = [k for k, p in tr.model.named_parameters() if p.requires_grad]
        assert len(ck["ema_state_dict"]) == 2 and all(list(t) == names for t in ck["ema_state_dict"])
        torch.save(ck, tmp_path / "checkpoint.pt")
        ck = torch.load(tmp_path / "checkpoint.pt", weights_only=False)
        # the averaged model file: data.save_model_sd's format, loaded by the usual loader
        from osufusion_amd import data as D
        with tr.ema_weights(0):
            D.save_model_sd(tr.model, tmp_path / "ema.safetensors")
        other, _ = _make(name, golden_dir)
        assert D.load_model_sd(other, tmp_path / "ema.safetensors") == {"missing": [], "unexpected": []}
        _assert_same_dicts(dict(other.state_dict()), tr.ema_state_dict(0))

        tr2, _ = _trainer(name, golden_dir, ema=TWO_TRACKS)
        tr2.load_state_dict(ck)
        assert tr2.opt.ema_step == 2 and "EMA" not in capsys.readouterr().out
        for j in range(2):
            _assert_same_dicts(tr.ema_state_dict(j), tr2.ema_state_dict(j))
        _twin_step(tr, tr2, batch)
        _assert_same_dicts(_params(tr), _params(tr2))
        for j in range(2):
            _assert_same_dicts(tr.ema_state_dict(j), tr2.ema_state_dict(j))

        # a checkpoint without the keys (a trainer without tracks, the reference trainer): every track restarts as the loaded weights
        plain_ck = {k: v for k, v in ck.items() if not k.startswith("ema_")}
        tr3, _ = _trainer(name, golden_dir, ema=TWO_TRACKS)
        tr3.step(*batch)
        capsys.readouterr()
        tr3.load_state_dict(plain_ck)
        out = capsys.readouterr().out
        assert out.count("\n") == 1 and "EMA" in out
        assert tr3.opt.ema_step == 0
        for j in range(2):
            _assert_same_dicts(tr3.ema_state_dict(j), {k: v for k, v in tr3.model.state_dict().items()})
            _assert_same_dicts(tr3.ema_state_dict(j), ck["model_state_dict"])

        # mismatches: nothing is loaded
        one, _ = _trainer(name, golden_dir, ema=TWO_TRACKS[:1])
        before = _params(one)
        with pytest.raises(ValueError, match="EMA tracks"):
            one.load_state_dict(ck)
        _assert_same_dicts(_params(one), before)
        bad = dict(ck, ema_state_dict=[dict(t) for t in ck["ema_state_dict"]])
        bad["ema_state_dict"][1][names[0]] = torch.zeros(3, device=DEV)
        with pytest.raises(ValueError, match="shape"):
            tr3.load_state_dict(bad)
    finally:
        Fn.enable_direct_grads(False)


def test_without_ema_the_trainer_is_todays_trainer(golden_dir, monkeypatch):
    calls = []
    orig = ops.call
    monkeypatch.setattr(ops, "call", lambda name, *args, **kw: (calls.append(name), orig(name, *args, **kw))[1])
    try:
        tr, batch = _trainer("dit_h96", golden_dir)
        tr.step(*batch)
        assert calls.count("osuf_adamw") == 1 and not {"osuf_adamw_ema", "osuf_ema_update", "osuf_swap"} & set(calls)
        assert tr.opt.ema is None and tr.opt.ema_cfgs == ()
        assert list(tr.state_dict()) == ["model_state_dict", "optimizer_state_dict", "scheduler_state_dict", "rng_state"]
        with pytest.raises(IndexError):
            tr.ema_state_dict(0)
        Fn.enable_direct_grads(False)
        del calls[:]
        tr, batch = _trainer("dit_h96", golden_dir, ema=EMAConfig())
        tr.step(*batch)
        assert calls.count("osuf_adamw_ema") == 1 and "osuf_adamw" not in calls          # one fused launch, not two passes
    finally:
        Fn.enable_direct_grads(False)
