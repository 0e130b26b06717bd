"""osuf_resample on the GPU against the fp64 restatement of resampy (tests/resample_oracle.py), through poisoned, canary-guarded
allocations (tests/memguard.py): the padded input and the table are placed exactly sized, so a read outside either meets NaN.

The bound is derived, not measured: for every output |y - y64| <= (T + 2) * 2**-24 * sum_j |w_j| |x_j| -- an fp32 dot product of T
terms (T * 2**-24, first order), one rounding of each table entry to fp32 and one of the stored result.  The oracle supplies
sum|w||x| per output; where it is 0 (an impulse out of an output's reach) the output must be exactly 0.

Shapes: kRun = 256 outputs per workgroup.  Ratios 1/2 (one table row, staged in LDS), 147/320, 441/160 (upsampling), 22050/44101
(a row per output); lengths of 1, 2, T - 1, T + 1 samples (shorter than one wing) and lengths that give 255, 256, 257 and 3 * 256 + 5
outputs; and two ratios below 1/40 (kaiser_fast, 96 000 -> 1 000 and -> 1 001) at which the span of one run no longer fits the LDS
budget and the kernel reads the input in place, with the row in LDS and through L2."""
import math

import numpy as np
import pytest
import torch

from osufusion_amd import audio as A
from tests import resample_oracle as RO
from tests.memguard import guard

RUN = 256
RATIOS = [(44100, 22050), (48000, 22050), (8000, 22050), (44101, 22050)]
_REF = {}


def _length_for(n_out, sr_orig, sr_new):
    """The shortest input with int(n * ratio) >= n_out: equal to it when downsampling; when upsampling (441/160 gives 253, 256, 259
    outputs) the nearest count on that side, and for a count below a run the longest input that stays below."""
    n = max(1, int(n_out * sr_orig / sr_new) - 1)
    while A.resample_length(n, sr_orig, sr_new) < n_out:
        n += 1
    if n_out % RUN == RUN - 1 and A.resample_length(n, sr_orig, sr_new) > n_out:
        n -= 1
    assert sr_new > sr_orig or A.resample_length(n, sr_orig, sr_new) == n_out
    return n


def _signal(kind, n, seed):
    if kind == "noise":
        return np.random.default_rng(seed).standard_normal(n).astype(np.float32)
    if kind == "impulses":
        x = np.zeros(n, np.float32)
        x[0] += 1.0
        x[n - 1] += 1.0 if n > 1 else 0.0
        return x
    return np.full(n, 0.75, np.float32)


def _oracle(kind, n, sr_orig, sr_new, res_type):
    """Computed once per case and shared; never modified."""
    key = (kind, n, sr_orig, sr_new, res_type)
    if key not in _REF:
        x = _signal(kind, n, n * 7 + sr_orig)
        y, mass, _ = RO.resample_direct(x.astype(np.float64), sr_orig, sr_new, res_type, exact=True)
        for a in (x, y, mass):
            a.setflags(write=False)
        _REF[key] = (x, y, mass)
    return _REF[key]


def _padded(x, plan, n_out):
    front = plan.t_left - 1
    last = ((n_out - 1) * plan.M) // plan.L
    xp = np.zeros(max(front + len(x), last + plan.T), np.float32)
    xp[front:front + len(x)] = x
    return xp


def _launch(g, x, sr_orig, sr_new, res_type="kaiser_best"):
    from osufusion_amd import ops
    plan = A.resample_plan(sr_orig, sr_new, res_type)
    n_out = A.resample_length(len(x), sr_orig, sr_new)
    x_pad = g.place(torch.from_numpy(_padded(x, plan, n_out)))
    table = g.place(torch.from_numpy(plan.table))
    y = torch.empty(n_out, dtype=torch.float32, device="cuda")
    ops.resample(x_pad, table, plan.L, plan.M, 0, y)
    g.check()
    return y.cpu().numpy()


def _assert_parity(got, want, mass, T, what):
    bound = (T + 2) * 2.0 ** -24 * mass
    err = np.abs(got.astype(np.float64) - want)
    assert np.isfinite(got).all(), what
    live = mass > 0
    if live.any():
        print(f"{what}: max err / bound = {(err[live] / bound[live]).max():.3f} over {int(live.sum())} outputs")
    assert np.all(err <= bound), (what, float(err.max()))


def _cases():
    out = []
    for sr_orig, sr_new in RATIOS:
        T = A.resample_plan(sr_orig, sr_new).T
        lengths = [1, 2, T - 1, T + 1] + [_length_for(k, sr_orig, sr_new) for k in (RUN - 1, RUN, RUN + 1, 3 * RUN + 5)]
        out += [(sr_orig, sr_new, n) for n in lengths]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("sr_orig,sr_new,n", _cases())
def test_parity_with_the_fp64_oracle(sr_orig, sr_new, n):
    plan = A.resample_plan(sr_orig, sr_new)
    n_out = A.resample_length(n, sr_orig, sr_new)
    if n_out == 0:                                                   # nothing to launch: the public entry point pads to ceil(n * ratio)
        y = A.resample(_signal("noise", n, 1), sr_orig, sr_new)
        assert y.shape == (math.ceil(n * (sr_new / sr_orig)),) and not bool(y.any())
        assert A.resample(_signal("noise", n, 1), sr_orig, sr_new, fix=False).numel() == 0
        return
    with guard(0xFF) as g:
        for kind in ("noise", "impulses", "constant"):
            x, want, mass = _oracle(kind, n, sr_orig, sr_new, "kaiser_best")
            got = _launch(g, x, sr_orig, sr_new)
            assert got.shape == want.shape == (n_out,)
            _assert_parity(got, want, mass, plan.T, f"{sr_orig}->{sr_new} n={n} {kind}")
            if kind == "constant":                                   # interior outputs: the row sums (the DC gain of each phase)
                W, t_left = A.resample_table(sr_orig, sr_new)
                t = np.arange(n_out)
                pos, ph = (t * plan.M) // plan.L, (t * plan.M) % plan.L
                inner = (pos - (t_left - 1) >= 0) & (pos - (t_left - 1) + plan.T <= n)
                bound = (plan.T + 2) * 2.0 ** -24 * 0.75 * np.abs(W).sum(axis=1)[ph]
                assert np.all(np.abs(got - 0.75 * W.sum(axis=1)[ph])[inner] <= bound[inner])
        g.release()
    # the public entry point: the same numbers, the length fixed to ceil(n * ratio)
    x, want, mass = _oracle("noise", n, sr_orig, sr_new, "kaiser_best")
    y = A.resample(x.copy(), sr_orig, sr_new).cpu().numpy()
    assert y.shape == (RO.fixed_length(n, sr_orig, sr_new),) and not y[n_out:].any()
    _assert_parity(y[:n_out], want, mass, plan.T, "audio.resample")


@pytest.mark.gpu
@pytest.mark.parametrize("sr_new", [1000, 1001])
def test_parity_where_the_span_is_read_in_place(sr_new):
    """96 000 -> 1 000 / 1 001, kaiser_fast: T = 3 072, one run covers 255 * 96 + T floats = 108 KiB, more than the kernel stages."""
    sr_orig, n = 96000, 60000
    plan = A.resample_plan(sr_orig, sr_new, "kaiser_fast")
    assert (255 * plan.M) // plan.L + plan.T > 16384 and (plan.L == 1) == (sr_new == 1000)
    x, want, mass = _oracle("noise", n, sr_orig, sr_new, "kaiser_fast")
    assert len(want) > 2 * RUN
    with guard(0xFF) as g:
        got = _launch(g, x, sr_orig, sr_new, "kaiser_fast")
        g.release()
    _assert_parity(got, want, mass, plan.T, f"{sr_orig}->{sr_new} in place")


@pytest.mark.gpu
@pytest.mark.parametrize("sr_orig,sr_new", RATIOS)
def test_bits_do_not_depend_on_the_launch(sr_orig, sr_new):
    plan = A.resample_plan(sr_orig, sr_new)
    n = _length_for(3 * RUN + 5, sr_orig, sr_new)
    x = _signal("noise", n, 3)
    n_cut = n - n // 3
    reach = (np.arange(A.resample_length(n_cut, sr_orig, sr_new)) * plan.M) // plan.L - (plan.t_left - 1) + plan.T
    k = int((reach <= n_cut).sum())                                  # outputs whose taps all lie inside the cut signal
    assert RUN < k < A.resample_length(n_cut, sr_orig, sr_new)
    with guard(0xFF) as g:
        a = _launch(g, x, sr_orig, sr_new)
        b = _launch(g, x, sr_orig, sr_new)
        c = _launch(g, x[:n_cut], sr_orig, sr_new)
        g.release()
    assert a.tobytes() == b.tobytes()
    assert a[:k].tobytes() == c[:k].tobytes()


@pytest.mark.gpu
def test_invalid_arguments_through_the_c_abi():
    from osufusion_amd import _lib
    lib = _lib.load()
    plan = A.resample_plan(44100, 22050)
    n_out = 300
    with guard(0xFF) as g:
        x_pad = g.place(torch.zeros(2 * (n_out - 1) + plan.T))
        table = g.place(torch.from_numpy(plan.table))
        y = torch.empty(n_out, dtype=torch.float32, device="cuda")
        before = y.clone()

        def call(x=x_pad.data_ptr(), n_pad=x_pad.numel(), tab=table.data_ptr(), L=1, M=2, T=plan.T, base0=0, out=y.data_ptr(), n=n_out):
            return lib.osuf_resample(x, n_pad, tab, L, M, T, base0, out, n, None)

        assert call(out=None) == -1 and call(x=None) == -1 and call(tab=None) == -1      # null pointers
        assert call(n=0) == -1 and call(n=-5) == -1 and call(n_pad=0) == -1 and call(L=0) == -1 and call(M=0) == -1 and call(T=0) == -1
        assert call(base0=-1) == -1                                                        # reads in front of the buffer
        assert call(base0=1) == -1 and call(n=n_out + 1) == -1 and call(n_pad=x_pad.numel() - 1) == -1      # ... and behind it
        assert call(n=1 << 62) == -1
        torch.cuda.synchronize()
        assert torch.equal(y.view(torch.int32), before.view(torch.int32))                  # nothing was launched
        assert call() == 0
        g.check()
        g.release()
    assert not bool(y.any())


# -------------------------------------------------------------------------------------------------------------- load_audio
@pytest.mark.gpu
def test_load_audio_resamples_as_the_oracle_does(tmp_path):
    """0.5 s at 44.1 kHz, one tone below the new Nyquist (11 025 Hz) and one above it, as a float32 .wav (16-bit samples would put
    their own quantisation noise, -98 dB, on top of a 133 dB measurement).  load_audio against the fp64 chain oracle-resample ->
    oracle VQT within the bounds of tests/test_audio_frontend.py (linear magnitudes 2e-5 of the peak, log features 1e-3 above 1e-3 of
    the peak); the 13 kHz tone, in the stop band (above (rolloff + transition) x 11 025 = 11 256 Hz), folds to 9 050 Hz and must lie
    A - 10 dB = 132.7 dB below its input level, A from Kaiser's formula."""
    from oracle import vqt_oracle as VO
    from tests.test_resample_cpu import _write_riff
    sr, f_lo, f_hi, a_lo, a_hi = 44100, 3000.0, 13000.0, 0.4, 0.3
    assert f_hi > (RO.FILTERS["kaiser_best"][2] + RO.kaiser_transition()) * A.SR / 2
    t = np.arange(sr // 2) / sr
    x = (a_lo * np.cos(2 * np.pi * f_lo * t) + a_hi * np.cos(2 * np.pi * f_hi * t + 0.3)).astype("<f4")
    _write_riff(tmp_path / "two_tones.wav", 3, 1, sr, 32, x.tobytes())
    got = A.load_audio(tmp_path / "two_tones.wav").cpu().numpy().astype(np.float64)
    y64 = RO.resample(x.astype(np.float64), sr, A.SR)
    v = np.abs(VO.vqt_recursive(y64))
    assert got.shape == v.shape == (96, 1 + len(y64) // 176)
    peak = v.max()
    assert np.abs(np.exp(got) - 1e-10 - v).max() <= 2e-5 * peak
    big = v > 1e-3 * peak
    assert np.abs(got[big] - np.log(v[big] + 1e-10)).max() < 1e-3

    wave, rate = A.read_wave(tmp_path / "two_tones.wav", resample=False)
    assert rate == sr
    y = A.resample(wave, rate).cpu().numpy().astype(np.float64)
    assert y.shape == y64.shape
    T = A.resample_plan(sr, A.SR).T
    seg = np.arange(T, len(y) - T)                                   # outputs whose wings lie inside the signal
    ts = seg / A.SR
    f_alias = A.SR - f_hi
    basis = np.stack([np.cos(2 * np.pi * f_lo * ts), np.sin(2 * np.pi * f_lo * ts),
                      np.cos(2 * np.pi * f_alias * ts), np.sin(2 * np.pi * f_alias * ts)], axis=1)
    coef = np.linalg.lstsq(basis, y[seg], rcond=None)[0]
    kept, folded = math.hypot(coef[0], coef[1]), math.hypot(coef[2], coef[3])
    floor_db = RO.kaiser_attenuation_db() - 10.0
    print(f"pass tone {kept / a_lo:.8f} of its input level; folded tone {20 * math.log10(max(folded, 1e-300) / a_hi):.1f} dB (bound -{floor_db:.1f})")
    assert folded <= a_hi * 10.0 ** (-floor_db / 20.0)
    assert abs(kept / a_lo - 1.0) <= 10.0 ** (-floor_db / 20.0) + 4 * 2.0 ** -24           # pass-band ripple + fp32 input and output
