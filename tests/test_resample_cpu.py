"""Host side of the resampler (no GPU): the per-phase weight table of osufusion_amd.audio.resample_plan against the two-wing loop of
tests/resample_oracle.py (resampy's algorithm restated in fp64), integer phase arithmetic, output lengths, known-answer filter properties
read from the table itself, and the .wav reader.

Bounds.  Table vs loop: 1e-12 of sum|w||x| per output (both are fp64 sums of the same products; what differs is the order of the sum and
the rounding of the output time t / ratio, half an ulp of a number below 2**13 = 4.5e-13 samples, times a filter slope below 1.3 per
sample).  Filter properties: Kaiser's design formula A = beta / 0.1102 + 8.7 dB (142.7 dB for kaiser_best) with a 10 dB margin, i.e.
ripple 10**(-(A - 10) / 20) = 2.3e-7, outside the transition band that the same design formulas give (resample_oracle.kaiser_transition).

DC gain.  A row's sum is the filter sampled every index_step table points, and its integral is 1.  Where scale * 2**precision is an
integer (44 100 -> 22 050: step 256; 88 200 -> 22 050: 128) both wings lie on one uniform grid and every row sums to 1 up to the ripple.
Otherwise resampy truncates index_step = int(scale * 2**precision) (48 000 -> 22 050: 235.2 -> 235): the taps of each wing are
step / 2**precision apart, but the two wings' first taps are scale apart, one wider gap at the filter's centre.  The Riemann sum with
the true gaps is 1 up to the ripple; counting every gap as the narrower one leaves out (scale 2**precision - step) h(centre) / 2**precision
with 0 < h(centre) < 1, so 1 <= row sum <= scale * 2**precision / index_step (measured for 48 000: 1.00047..1.00050 under 1.00085).
That gain belongs to the definition (resampy has it); it is not the stop-band ripple, and the rows are held to the interval."""
import math
import struct
import wave

import numpy as np
import pytest

from osufusion_amd import audio as A
from tests import resample_oracle as RO

RATES = [44100, 48000, 32000, 8000, 11025, 44101]


def _ripple(res_type="kaiser_best"):
    return 10.0 ** (-(RO.kaiser_attenuation_db(res_type) - 10.0) / 20.0)


def _apply_table(x, sr_orig, sr_new, res_type="kaiser_best"):
    """The plan's arithmetic in fp64 numpy: zero padding, integer positions, one dot product per output."""
    W, t_left = A.resample_table(sr_orig, sr_new, res_type)
    g = math.gcd(sr_orig, sr_new)
    L, M = sr_new // g, sr_orig // g
    T = W.shape[1]
    n_out = A.resample_length(len(x), sr_orig, sr_new)
    xp = np.concatenate([np.zeros(t_left - 1), np.asarray(x, np.float64), np.zeros(T + 1)])
    y = np.zeros(n_out)
    for t in range(n_out):
        n, p = A.resample_phase(t, L, M)
        y[t] = np.dot(W[p], xp[n:n + T])
    return y


def test_plan_shapes_named_in_the_design():
    p = A.resample_plan(44100, 22050)
    assert (p.L, p.M, p.T, p.t_left) == (1, 2, 256, 128) and p.table.shape == (1, 256) and p.table.dtype == np.float32
    p = A.resample_plan(48000, 22050)
    assert (p.L, p.M) == (147, 320) and p.table.shape == (147, p.T) and p.T % 4 == 0
    p = A.resample_plan(8000, 22050)
    assert (p.L, p.M, p.T) == (441, 160, 128)
    assert A.resample_plan(44101, 22050).L == 22050
    assert A.resample_plan(44100, 22050) is A.resample_plan(44100, 22050)                     # cached per triple
    assert A.resample_plan(44100, 22050, "kaiser_fast").T == 64
    with pytest.raises(ValueError, match="res_type"):
        A.resample_plan(44100, 22050, "soxr_hq")
    with pytest.raises(ValueError, match="positive integers"):
        A.resample_plan(0, 22050)


@pytest.mark.parametrize("rate", RATES)
def test_table_form_equals_the_two_wing_loop(rate):
    """The loop takes the integer and fractional parts of the output time t*M/L exactly (exact=True): those are the positions the
    definition names.  resampy's own fp64 `t / ratio` carries two roundings (of ratio and of the quotient, 2**-53 relative each), which
    move every weight by at most slope * scale * 2**-52 * time; at time ~ 5000 that alone reaches 1.5e-12 of sum|w||x| (measured,
    8 000 -> 22 050), so that loop is held to 1e-12 sum|w||x| plus this term, the table being the exact one of the two."""
    T = A.resample_plan(rate, A.SR).T
    win, delta, num_table, scale, _, _ = RO.setup(rate, A.SR)
    slope = np.abs(delta).max() * num_table * scale                                           # |d weight / d time|, per input sample
    rng = np.random.default_rng(rate)
    worst = worst_f = 0.0
    for n in (1, 2, 3, T - 1, T, T + 1, 5000):
        x = rng.standard_normal(n)
        want, mass, reach = RO.resample_direct(x, rate, A.SR, exact=True)
        got = _apply_table(x, rate, A.SR)
        assert got.shape == want.shape == (int(n * (A.SR / rate)),)
        floated = RO.resample_direct(x, rate, A.SR)[0]
        if len(want):
            worst = max(worst, float((np.abs(got - want) / mass).max()))
            worst_f = max(worst_f, float((np.abs(got - floated) / mass).max()))
        assert np.all(np.abs(got - want) <= 1e-12 * mass), (rate, n, worst)
        assert np.all(np.abs(got - floated) <= 1e-12 * mass + slope * 2.0 ** -52 * n * reach), (rate, n, worst_f)
    print(f"{rate} -> {A.SR}: max |table - loop| / sum|w||x| = {worst:.3e} (exact times), {worst_f:.3e} (fp64 t / ratio)")


def test_kaiser_fast_table_equals_the_loop():
    rng = np.random.default_rng(5)
    x = rng.standard_normal(700)
    for rate in (44100, 48000, 8000):
        want, mass, _ = RO.resample_direct(x, rate, A.SR, "kaiser_fast", exact=True)
        assert np.all(np.abs(_apply_table(x, rate, A.SR, "kaiser_fast") - want) <= 1e-12 * mass)


def test_integer_phases():
    """Integer positions equal the fp64 evaluation of t / ratio where that is still accurate, and stay exactly periodic where it is not."""
    for rate in (48000, 8000, 44101):
        g = math.gcd(rate, A.SR)
        L, M = A.SR // g, rate // g
        ratio = A.SR / rate
        t = np.arange(0, 2 ** 20, 997)
        time = t / ratio
        n = np.array([A.resample_phase(int(v), L, M)[0] for v in t])
        p = np.array([A.resample_phase(int(v), L, M)[1] for v in t])
        # fp64 t / ratio: two roundings (ratio, the quotient), each 2**-53 relative
        assert np.all(np.abs((n + p / L) - time) <= 4 * 2.0 ** -53 * np.maximum(time, 1.0))
        t9 = 10 ** 9
        for k in (0, 1, 7):
            n0, p0 = A.resample_phase(t9 + k, L, M)
            n1, p1 = A.resample_phase(t9 + k + L, L, M)
            assert p1 == p0 and n1 - n0 == M                                                  # one period later: same row, M samples on
            assert n0 * L + p0 == (t9 + k) * M
    # at t = 1e9 the fp64 product has lost the low bits of the phase: spacing of doubles near 2e9 is 2.4e-7 samples
    L, M = 147, 320
    n0, p0 = A.resample_phase(10 ** 9, L, M)
    assert abs(math.fmod(10 ** 9 / (22050 / 48000), 1.0) - p0 / L) < 2.0 ** -21


def test_output_lengths():
    for rate in (44100, 48000, 8000, 44101):
        g = math.gcd(rate, A.SR)
        M = rate // g
        for n in (1, M - 1, M, M + 1, 3 * M - 1, 3 * M, 3 * M + 1, 5000):
            ratio = A.SR / rate
            assert A.resample_length(n, rate, A.SR) == int(n * ratio) == RO.output_length(n, rate, A.SR)
            assert A.resample_length(n, rate, A.SR, fix=True) == int(math.ceil(n * ratio)) == RO.fixed_length(n, rate, A.SR)
            assert 0 <= A.resample_length(n, rate, A.SR, fix=True) - A.resample_length(n, rate, A.SR) <= 1
            if n <= 1000:
                assert len(RO.resample(np.ones(n), rate, A.SR)) == int(math.ceil(n * ratio))
            # the last output reads no sample behind the signal's end: its integer position is inside it
            n_out = A.resample_length(n, rate, A.SR)
            if n_out:
                assert A.resample_phase(n_out - 1, A.SR // g, M)[0] <= n - 1


@pytest.mark.parametrize("rate", [44100, 88200, 48000, 32000, 44101])
def test_dc_gain_of_every_phase(rate):
    """A row's sum is the DC gain of its phase: 1 up to the Kaiser ripple where the taps sit on a uniform grid (see the module
    docstring), between 1 and scale * 2**precision / index_step where the truncated step leaves one wider gap at the centre."""
    W, _ = A.resample_table(rate, A.SR)
    _, _, num_table, scale, step, _ = RO.setup(rate, A.SR)
    over = scale * num_table / step
    assert 1.0 <= over < 1.0 + 1.0 / step
    if rate in (44100, 88200):
        assert over == 1.0
    sums = W.sum(axis=1)
    print(f"{rate}: row sums in [{sums.min():.8f}, {sums.max():.8f}], scale * 2**precision / index_step = {over:.8f}")
    assert sums.min() >= 1.0 - _ripple() and sums.max() <= over + _ripple()


@pytest.mark.parametrize("res_type", ["kaiser_best", "kaiser_fast"])
def test_frequency_response_of_the_half_rate_row(res_type):
    """44 100 -> 22 050 (L = 1): the one row IS the decimation filter at the input rate.  With f in units of the new Nyquist frequency:
    flat to the Kaiser ripple below rolloff - w, down by A - 10 dB above rolloff + w, half amplitude at the cutoff rolloff itself, and
    falling through the new Nyquist."""
    W, _ = A.resample_table(44100, 22050, res_type)
    rolloff = RO.FILTERS[res_type][2]
    w = RO.kaiser_transition(res_type)
    nfft = 1 << 16
    H = np.abs(np.fft.rfft(W[0], nfft))
    f = np.arange(len(H)) / (nfft / 2) * 2.0                                                   # input Nyquist = 2 new Nyquists
    tol = _ripple(res_type)
    print(f"{res_type}: passband dev {np.abs(H[f <= rolloff - w] - 1).max():.2e}, stopband {H[f >= rolloff + w].max():.2e}, bound {tol:.2e}")
    assert np.abs(H[f <= rolloff - w] - 1.0).max() <= tol
    assert H[f >= rolloff + w].max() <= tol
    assert abs(np.interp(rolloff, f, H) - 0.5) < 0.01
    band = (f >= rolloff - w) & (f <= 1.0)
    assert np.all(np.diff(H[band]) < 0) and np.interp(1.0, f, H) < 0.05


# ------------------------------------------------------------------------------------------------------------------ .wav reader
def _write_riff(path, tag, ch, rate, bits, payload, extensible=False):
    align = ch * bits // 8
    if extensible:
        guid_tail = bytes.fromhex("000000001000800000aa00389b71")
        fmt = struct.pack("<HHIIHHHHI", 0xFFFE, ch, rate, rate * align, align, bits, 22, bits, 0) + struct.pack("<H", tag) + guid_tail
    else:
        fmt = struct.pack("<HHIIHH", tag, ch, rate, rate * align, align, bits)
    chunks = b"fmt " + struct.pack("<I", len(fmt)) + fmt
    chunks += b"LIST" + struct.pack("<I", 5) + b"abcde" + b"\0"                                # an odd-sized chunk to step over
    chunks += b"data" + struct.pack("<I", len(payload)) + payload + (b"\0" if len(payload) & 1 else b"")
    path.write_bytes(b"RIFF" + struct.pack("<I", 4 + len(chunks)) + b"WAVE" + chunks)


def test_wave_reader_formats(tmp_path):
    rng = np.random.default_rng(11)
    x = rng.uniform(-0.9, 0.9, 1001)
    i16 = np.round(x * 32767).astype("<i2")
    _write_riff(tmp_path / "i16.wav", 1, 1, 48000, 16, i16.tobytes())
    y, rate = A.read_wave(tmp_path / "i16.wav", resample=False)
    assert rate == 48000 and y.dtype == np.float32
    np.testing.assert_array_equal(y, i16.astype(np.float32) / 32768.0)

    i24 = np.round(x * 8388607).astype(np.int32)
    b = (i24 & 0xFFFFFF).astype("<u4").view(np.uint8).reshape(-1, 4)[:, :3]
    _write_riff(tmp_path / "i24.wav", 1, 1, 44100, 24, b.tobytes())
    y, rate = A.read_wave(tmp_path / "i24.wav", resample=False)
    assert rate == 44100
    np.testing.assert_array_equal(y, i24.astype(np.float32) / 8388608.0)

    f32 = x.astype("<f4")
    _write_riff(tmp_path / "f32.wav", 3, 1, 32000, 32, f32.tobytes())
    y, rate = A.read_wave(tmp_path / "f32.wav", resample=False)
    assert rate == 32000
    np.testing.assert_array_equal(y, f32)

    st = rng.uniform(-0.9, 0.9, (500, 2)).astype("<f4")
    _write_riff(tmp_path / "ext_f32.wav", 3, 2, 96000, 32, st.tobytes(), extensible=True)
    y, rate = A.read_wave(tmp_path / "ext_f32.wav", resample=False)
    assert rate == 96000
    np.testing.assert_array_equal(y, st.mean(axis=1))                                          # mono = the mean over channels
    _write_riff(tmp_path / "ext_i16.wav", 1, 1, 22050, 16, i16.tobytes(), extensible=True)
    np.testing.assert_array_equal(A.read_wave(tmp_path / "ext_i16.wav"), i16.astype(np.float32) / 32768.0)

    np.save(tmp_path / "w.npy", f32)
    y, rate = A.read_wave(tmp_path / "w.npy", resample=False)
    assert rate == A.SR
    np.testing.assert_array_equal(y, f32)
    with pytest.raises(ValueError, match="format tag"):
        _write_riff(tmp_path / "alaw.wav", 6, 1, 8000, 8, b"\0" * 16)
        A.read_wave(tmp_path / "alaw.wav")
    with pytest.raises(ValueError, match="RIFF"):
        (tmp_path / "junk.wav").write_bytes(b"not a wave file at all")
        A.read_wave(tmp_path / "junk.wav")


def test_wave_reader_default_call_keeps_the_host_path(tmp_path):
    """A 44.1 kHz stereo file through the default call: the bits of mean-over-channels + scipy.signal.resample_poly, as before."""
    from scipy.signal import resample_poly
    rng = np.random.default_rng(1)
    pcm = (rng.uniform(-0.5, 0.5, (4410, 2)) * 32767).astype("<i2")
    with wave.open(str(tmp_path / "s.wav"), "wb") as f:
        f.setnchannels(2)
        f.setsampwidth(2)
        f.setframerate(44100)
        f.writeframes(pcm.tobytes())
    mono = (pcm.astype(np.float32) / 32768.0).mean(axis=1)
    want = resample_poly(mono.astype(np.float64), 1, 2).astype(np.float32)
    got = A.read_wave(tmp_path / "s.wav")
    assert got.dtype == np.float32 and got.flags["C_CONTIGUOUS"]
    np.testing.assert_array_equal(got, want)
    raw, rate = A.read_wave(tmp_path / "s.wav", resample=False)
    assert rate == 44100
    np.testing.assert_array_equal(raw, mono)


def test_resample_errors_without_gpu_work():
    with pytest.raises(ValueError, match="mono"):
        A.resample(np.zeros((2, 10), np.float32), 44100)
    with pytest.raises(ValueError, match="res_type"):
        A.resample(np.zeros(10, np.float32), 44100, res_type="sinc_best")
    with pytest.raises(RuntimeError, match="GPU only"):
        A.resample(np.zeros(10, np.float32), 44100, device="cpu")
    x = np.arange(5, dtype=np.float32)
    assert A.resample(x, 22050, 22050, device="cpu") is x                                      # equal rates: the input, untouched
