"""fp64 restatement of resampy's band-limited sinc interpolation (the resampler behind the reference's
``librosa.load(file, sr=22050, res_type="kaiser_best")``, scripts/dataset_creator.py:36-38), written from its published algorithm
(J. O. Smith, "Digital Audio Resampling"; resampy's ``sinc_window`` / ``resample_f``).  resampy is not installed and is not part of the
reference tree: the filter constants below are quoted from its documentation and the result is **unpinned** against resampy itself
(DESIGN.md section 6d).  A plain helper module (no tests in it); everything is numpy fp64.

``resample_direct`` is the two-wing loop exactly as resampy runs it, one output at a time, with the output's time ``t / ratio``
evaluated in fp64 as resampy evaluates it; ``exact=True`` takes the integer and fractional parts of that time from integer arithmetic
instead (what the host plan of osufusion_amd.audio does)."""
from __future__ import annotations

import math

import numpy as np

#              num_zeros, precision, rolloff, Kaiser beta
FILTERS = {
    "kaiser_best": (64, 9, 0.9475937167399596, 14.769656459379492),
    "kaiser_fast": (16, 9, 0.85, 8.555504641634386),
}


def kaiser_attenuation_db(res_type: str = "kaiser_best") -> float:
    """Kaiser's design formula: stop-band attenuation of a Kaiser(beta) windowed sinc, A = beta / 0.1102 + 8.7 dB."""
    return FILTERS[res_type][3] / 0.1102 + 8.7


def kaiser_transition(res_type: str = "kaiser_best") -> float:
    """Half width of the transition band around rolloff x Nyquist, as a fraction of the Nyquist frequency.  Kaiser: a window that
    spans D periods of the Nyquist-rate grid has a transition band (A - 7.95) / (14.36 D) of the sample rate wide; here D = 2 num_zeros,
    so the full width is (A - 7.95) / (14.36 * 2 num_zeros) cycles per sample = twice that in Nyquist units, and half of it lies on
    either side of the cutoff."""
    return (kaiser_attenuation_db(res_type) - 7.95) / (14.36 * 2 * FILTERS[res_type][0])


def sinc_window(num_zeros: int, precision: int, rolloff: float, beta: float) -> np.ndarray:
    """Right half (centre included) of the Kaiser-windowed sinc, 2**precision samples per zero crossing."""
    n = num_zeros * 2 ** precision
    i = np.arange(n + 1, dtype=np.float64)
    return rolloff * np.sinc(rolloff * i / 2 ** precision) * np.kaiser(2 * n + 1, beta)[n:]


def setup(sr_orig: int, sr_new: int, res_type: str = "kaiser_best"):
    """(win, delta, num_table, scale, index_step, ratio) as resample_f receives them."""
    num_zeros, precision, rolloff, beta = FILTERS[res_type]
    ratio = float(sr_new) / float(sr_orig)
    win = sinc_window(num_zeros, precision, rolloff, beta)
    scale = min(1.0, ratio)
    if ratio < 1:
        win = win * ratio
    delta = np.diff(win, append=0.0)
    num_table = 2 ** precision
    return win, delta, num_table, scale, int(scale * num_table), ratio


def output_length(n_orig: int, sr_orig: int, sr_new: int) -> int:
    return int(n_orig * (float(sr_new) / float(sr_orig)))


def fixed_length(n_orig: int, sr_orig: int, sr_new: int) -> int:
    """librosa.resample's fix=True target."""
    return int(math.ceil(n_orig * (float(sr_new) / float(sr_orig))))


def resample_direct(x, sr_orig: int, sr_new: int, res_type: str = "kaiser_best", exact: bool = False):
    """-> (y, mass, reach): y[t] the two-wing sums, mass[t] = sum_j |w_j| |x_j| over the same taps (the scale of a dot product's rounding
    error), reach[t] = sum_j |x_j| over them (the scale of an error in the weights)."""
    x = np.asarray(x, dtype=np.float64)
    assert x.ndim == 1
    win, delta, num_table, scale, step, ratio = setup(sr_orig, sr_new, res_type)
    nwin, n_orig = len(win), len(x)
    n_out = output_length(n_orig, sr_orig, sr_new)
    g = math.gcd(sr_orig, sr_new)
    L, M = sr_new // g, sr_orig // g
    y, mass, reach = np.zeros(n_out), np.zeros(n_out), np.zeros(n_out)
    ax = np.abs(x)
    for t in range(n_out):
        if exact:
            n, rem = divmod(t * M, L)
            part = rem / L
        else:
            time = t / ratio
            n = int(time)
            part = time - n
        frac = scale * part
        index_frac = frac * num_table
        offset = int(index_frac)
        eta = index_frac - offset
        i_max = min(n + 1, (nwin - offset) // step)
        idx = offset + step * np.arange(i_max)
        w = win[idx] + eta * delta[idx]
        seg = slice(n - i_max + 1, n + 1)
        y[t] += np.dot(w[::-1], x[seg])
        mass[t] += np.dot(np.abs(w[::-1]), ax[seg])
        reach[t] += ax[seg].sum()
        frac = scale - frac
        index_frac = frac * num_table
        offset = int(index_frac)
        eta = index_frac - offset
        k_max = max(0, min(n_orig - n - 1, (nwin - offset) // step))
        idx = offset + step * np.arange(k_max)
        w = win[idx] + eta * delta[idx]
        seg = slice(n + 1, n + 1 + k_max)
        y[t] += np.dot(w, x[seg])
        mass[t] += np.dot(np.abs(w), ax[seg])
        reach[t] += ax[seg].sum()
    return y, mass, reach


def resample(x, sr_orig: int, sr_new: int, res_type: str = "kaiser_best", fix: bool = True) -> np.ndarray:
    """librosa.resample(x, orig_sr, target_sr, res_type, fix, scale=False) for mono x: resampy, then the length fixed to
    ceil(n * ratio) by zero padding (at most one sample)."""
    x = np.asarray(x, dtype=np.float64)
    if sr_orig == sr_new:
        return x
    y = resample_direct(x, sr_orig, sr_new, res_type, exact=True)[0]
    if fix:
        n = fixed_length(len(x), sr_orig, sr_new)
        y = np.concatenate([y, np.zeros(n - len(y))]) if n > len(y) else y[:n]
    return y
