"""Host side of the EMA tracks (osufusion_amd/ema.py): the decay schedules against their closed forms, sigma_rel -> gamma against the
check values of the EDM2 cubic, and every argument error.  No GPU."""
import numpy as np
import pytest

from osufusion_amd.ema import EMAConfig, as_tracks, ema_beta, ema_d, sigma_rel_to_gamma

KS = (1, 2, 10, 10 ** 6)


def test_constant_schedule():
    cfg = EMAConfig(kind="constant", beta=0.999)
    for k in KS:
        assert ema_beta(cfg, k) == 0.999
    assert EMAConfig().kind == "constant" and ema_beta(EMAConfig(), 7) == 0.9999


def test_warmup_schedule_closed_form_and_defaults():
    cfg = EMAConfig(kind="warmup")
    assert (cfg.beta, cfg.inv_gamma, cfg.power, cfg.min_beta, cfg.update_after_step) == (0.9999, 1.0, 2.0 / 3.0, 0.0, 0)
    assert ema_beta(cfg, 1) == 0.0                                            # j = 0: the track is a copy
    for k in KS[1:]:
        j = k - 1
        want = min(max(1.0 - (1.0 + j) ** (-2.0 / 3.0), 0.0), 0.9999)
        assert ema_beta(cfg, k) == pytest.approx(want, rel=0, abs=1e-15)
    assert ema_beta(cfg, 2) == pytest.approx(1.0 - 2.0 ** (-2.0 / 3.0), abs=1e-15)
    assert ema_beta(cfg, 10 ** 7) == 0.9999                                  # 1 - (10^7)^(-2/3) = 0.99998: cut at beta
    cfg = EMAConfig(kind="warmup", inv_gamma=5.0, power=0.75)
    for k in KS[1:]:
        assert ema_beta(cfg, k) == pytest.approx(min(1.0 - (1.0 + (k - 1) / 5.0) ** -0.75, 0.9999), abs=1e-15)


def test_warmup_update_after_step_delays_the_first_nonzero_beta():
    cfg = EMAConfig(kind="warmup", update_after_step=5)
    assert [ema_beta(cfg, k) for k in range(1, 7)] == [0.0] * 6                # j = k - 6 <= 0
    assert ema_beta(cfg, 7) == pytest.approx(1.0 - 2.0 ** (-2.0 / 3.0), abs=1e-15)   # j = 1
    assert ema_beta(cfg, 7) == ema_beta(EMAConfig(kind="warmup"), 2)
    assert ema_d(cfg, 6) == 1.0 and 0.0 < ema_d(cfg, 7) < 1.0


def test_warmup_clamp_takes_effect_at_both_ends():
    cfg = EMAConfig(kind="warmup", beta=0.9, min_beta=0.5)
    assert ema_beta(cfg, 1) == 0.0                                            # before the first update the clamp does not apply
    assert 1.0 - 2.0 ** (-2.0 / 3.0) < 0.5 and ema_beta(cfg, 2) == 0.5       # raised to min_beta
    assert ema_beta(cfg, 10) == pytest.approx(1.0 - 10.0 ** (-2.0 / 3.0), abs=1e-15)          # 0.7846: between the clamps
    assert ema_beta(cfg, 10 ** 6) == 0.9                                      # cut at beta


def test_power_schedule_closed_form():
    for gamma in (6.94, 16.97, 0.0):
        cfg = EMAConfig(kind="power", gamma=gamma)
        assert ema_beta(cfg, 1) == 0.0
        for k in KS[1:]:
            assert ema_beta(cfg, k) == pytest.approx((1.0 - 1.0 / k) ** (gamma + 1.0), rel=1e-15)
    assert ema_beta(EMAConfig(kind="power", gamma=1.0), 2) == 0.25
    by_sigma = EMAConfig(kind="power", sigma_rel=0.10)
    assert ema_beta(by_sigma, 10) == pytest.approx(0.9 ** (sigma_rel_to_gamma(0.10) + 1.0), rel=1e-15)


def test_sigma_rel_to_gamma_check_values():
    assert abs(sigma_rel_to_gamma(0.05) - 16.9722) < 1e-3
    assert abs(sigma_rel_to_gamma(0.10) - 6.9372) < 1e-3
    for s in (0.05, 0.10, 0.2):                                                # a root of the cubic, and the largest one
        g, t = sigma_rel_to_gamma(s), s ** -2
        scale = abs(g) ** 3 + 7 * g * g + abs(16 - t) * abs(g) + abs(12 - t)
        assert abs(g ** 3 + 7 * g ** 2 + (16 - t) * g + (12 - t)) < 1e-9 * scale
        roots = np.roots([1.0, 7.0, 16.0 - t, 12.0 - t])
        assert g >= roots[np.abs(roots.imag) < 1e-9].real.max() - 1e-9


def test_ema_d_is_the_fp32_complement():
    cfg = EMAConfig(kind="constant", beta=0.9)
    assert ema_d(cfg, 3) == float(np.float32(1.0 - 0.9))
    assert ema_d(EMAConfig(kind="constant", beta=0.0), 1) == 1.0 and ema_d(EMAConfig(kind="constant", beta=1.0), 1) == 0.0
    assert ema_d(EMAConfig(kind="power", gamma=3.0), 1) == 1.0


@pytest.mark.parametrize("kw", [dict(kind="linear"), dict(beta=-0.1), dict(beta=1.5), dict(kind="warmup", beta=2.0), dict(kind="warmup", min_beta=-1.0),
                                dict(kind="power"), dict(kind="power", gamma=1.0, sigma_rel=0.1), dict(kind="power", sigma_rel=0.0),
                                dict(kind="power", gamma=-2.0), dict(kind="warmup", inv_gamma=0.0), dict(kind="warmup", update_after_step=-1)])
def test_bad_configs_raise(kw):
    with pytest.raises(ValueError):
        EMAConfig(**kw)


def test_track_lists():
    c = EMAConfig()
    assert as_tracks(None) == () and as_tracks(c) == (c,) and as_tracks([c, c, c, c]) == (c, c, c, c)
    with pytest.raises(ValueError):
        as_tracks([c] * 5)
    with pytest.raises(ValueError):
        as_tracks([c, 0.999])
    with pytest.raises(ValueError):
        ema_beta(c, 0)


def test_trainer_rejects_bad_tracks_before_it_touches_the_model():
    """More than four tracks: ValueError from Trainer itself, with the model's parameters left where they were."""
    torch = pytest.importorskip("torch")
    from osufusion_amd.train import Trainer
    model = torch.nn.Linear(4, 4)
    ptr = model.weight.data_ptr()
    with pytest.raises(ValueError):
        Trainer(model, ema=[EMAConfig()] * 5)
    with pytest.raises(ValueError):
        Trainer(model, ema="constant")
    assert model.weight.data_ptr() == ptr


def test_config_round_trips_through_a_plain_dict():
    c = EMAConfig(kind="power", sigma_rel=0.05)
    assert EMAConfig(**c.as_dict()) == c and isinstance(c.as_dict(), dict)
