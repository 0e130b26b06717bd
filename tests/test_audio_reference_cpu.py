"""The hand-written references of tests/audio_reference.py against independent formulations and against the slips they must tell apart,
its restated launcher arithmetic against the branch each table entry names, the caps written next to the tables, and the inventory of
csrc/audio.hip's entry points (CPU only).

tests/test_audio_rows_gpu.py measures the audio front end's kernels against these functions, so a slip in one of them would either hide a
kernel bug or report one that is not there."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import vqt_oracle as VO
from tests import audio_reference as R
from tests.bound_check import FLOOR
from tests.test_poisoned_memory import relmax

TOL = 1e-12                                                # fp64 against fp64
F32, F64 = torch.float32, torch.float64
ROOT = Path(__file__).resolve().parent.parent
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))


def convolve_decimate(x, taps, n_out, centre=None):
    """np.convolve on an explicitly padded signal, then every other sample: out[m] = sum_j taps[j] xpad[2m + j], xpad[i] = x[i - centre]."""
    c = (len(taps) - 1) // 2 if centre is None else centre
    xp = np.concatenate([np.zeros(c), x, np.zeros(2 * n_out + len(taps))])
    return np.convolve(xp, taps[::-1], mode="valid")[::2][:n_out]


# ---------------------------------------------------------------------------------------------------------------------------------
# references against independent formulations
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_in,ntaps,n_out", [(1, 1, 1), (2, 3, 1), (3, 257, 2), (513, 375, 257), (1000, 8191, 500), (3, 3, 7), (40, 9, 31)])
def test_fir_reference_equals_convolve_then_stride(n_in, ntaps, n_out):
    x, taps = R.uni("cx", (n_in,)).double(), R.uni("ct", (ntaps,)).double()
    want = convolve_decimate(x.numpy(), taps.numpy(), n_out)
    assert relmax(R.fir_decimate2(x, taps, n_out), T(want)) < TOL
    if n_in > 2:                                                                         # and the oracle's own decimator, at its n_out
        assert relmax(R.fir_decimate2(x, taps, (n_in + 1) // 2), T(VO.decimate2(x.numpy(), taps.numpy()))) < TOL


def test_fir_reference_rejects_the_obvious_slips():
    n_in, ntaps = 41, 9
    x, taps = R.uni("sx", (n_in,)).double(), R.uni("st", (ntaps,)).double()
    ref = R.fir_decimate2(x, taps, 21)
    for centre in (3, 5):                                                                # centre off by one, either way
        assert relmax(T(convolve_decimate(x.numpy(), taps.numpy(), 21, centre)), ref) > 1e-2
    # floor against ceil of n_in / 2: the 21st output of an odd-length signal exists and is not zero
    assert (n_in + 1) // 2 == 21 and n_in // 2 == 20 and abs(ref[20].item()) > 1e-3
    assert torch.equal(R.fir_decimate2(x, taps, 20), ref[:20])
    assert relmax(R.fir_decimate2(x, taps.flip(0), 21), ref) > 1e-2                      # convolution instead of correlation
    tail = R.fir_decimate2(x, taps, 30)                                                  # outputs past the signal and its filter tail: zero
    assert torch.equal(tail[:21], ref) and (tail[23:] == 0).all() and tail[22].abs() > 0


@pytest.mark.parametrize("cid,n_in,hop,K,frames,branch", [e for e in R.FRAME if e[4] * e[3] < 1 << 18], ids=lambda v: v if isinstance(v, str) else None)
def test_frame_reference_equals_strided_view(cid, n_in, hop, K, frames, branch):
    x = R.frame_signal(cid, n_in).double()
    xp = np.concatenate([x.numpy(), np.zeros(max(0, (frames - 1) * hop + K - n_in))])
    want = np.lib.stride_tricks.as_strided(xp, shape=(frames, K), strides=(8 * hop, 8))
    assert torch.equal(R.frame_rows(x, hop, K, frames), T(want))


def test_frame_reference_rejects_the_obvious_slips():
    x = R.frame_signal("s", 100).double()
    ref = R.frame_rows(x, 11, 32, 11)
    assert not torch.equal(R.frame_rows(x, 32, 32, 11)[1], ref[1])                       # rows K apart instead of hop apart
    assert torch.equal(ref[3], x[33:65]) and torch.equal(ref[9], torch.cat([x[99:], torch.zeros(31, dtype=F64)])) and (ref[10] == 0).all()
    assert not torch.equal(R.frame_rows(x[:99], 11, 32, 11), ref)                        # one sample fewer changes exactly the cut frames
    # the signal names its indices and holds no zero: a zero in a row is the fill, never a sample
    assert (x != 0).all()


def test_logmag_reference_equals_hypot():
    bins, frames = 5, 7
    spec, scale = R.logmag_real("h", bins, frames).double(), R.bin_scales(bins).double()
    want = np.log(scale.numpy()[:, None] * np.hypot(spec.numpy()[:, :bins], spec.numpy()[:, bins:]).T + R.EPS32)
    assert relmax(R.logmag(spec, scale), T(want)) < TOL
    assert torch.equal(R.logmag(torch.zeros(3, 4, dtype=F64), torch.ones(2, dtype=F64)), torch.full((2, 3), np.log(R.EPS32), dtype=F64))
    assert abs(R.EPS32 - 1e-10) < 1e-17 and R.EPS32 != 1e-10                             # the float the kernel is handed, not the decimal


def test_logmag_reference_rejects_the_obvious_slips():
    bins, frames = 6, 9
    spec, scale = R.logmag_real("s", bins, frames).double(), R.bin_scales(bins).double()
    ref = R.logmag(spec, scale)
    inter = torch.stack([spec[:, 0::2], spec[:, 1::2]], 0)                               # (re, im) interleaved instead of two halves
    slip = torch.log(scale[:, None] * torch.sqrt(inter[0] ** 2 + inter[1] ** 2).T + R.EPS32)
    assert (slip - ref).abs().max() > 1e-2
    assert (R.logmag(spec, scale.roll(1)) - ref).abs().max() > 0.5                       # the neighbouring bin's scale: a factor of two
    assert (torch.log(scale[:, None] * (spec[:, :bins] ** 2 + spec[:, bins:] ** 2).T + R.EPS32) - ref).abs().max() > 1e-2   # no root
    # |.| cannot see the two halves swapped; the spectrum can, and the exact log_vqt case compares the spectrum
    assert torch.equal(R.logmag(torch.cat([spec[:, bins:], spec[:, :bins]], 1), scale), ref)
    x, bank = R.logvqt_exact("s", 4, 32, 5, 3)
    s = R.spectrum(x.double(), bank.double(), 4, 5)
    assert not torch.equal(R.spectrum(x.double(), torch.cat([bank[3:], bank[:3]]).double(), 4, 5), s)
    assert not torch.equal(R.spectrum(x.double(), bank.double(), 8, 5)[1], s[1])         # a frame read at the wrong offset


def test_log_vqt_reference_equals_the_oracle_on_a_product_group():
    """The top octave of the product's plan (hop 176, 256-sample kernels, 12 bins, no decimation in front of it) through the reference
    equals the recursive oracle's rows for those bins."""
    from osufusion_amd import audio as A
    g = A.librosa_plan().groups[0]
    assert (g.decimations, g.hop, g.n_fft, g.bank.shape[0]) == (0, 176, 256, 24)
    n = 4000
    y = np.random.default_rng(11).standard_normal(n) * 0.2 + np.sin(2 * np.pi * 5000 * np.arange(n) / VO.SR)
    frames = 1 + n // 176
    pad = np.zeros(max((frames - 1) * g.hop + g.n_fft, g.n_fft // 2 + n))
    pad[g.n_fft // 2:g.n_fft // 2 + n] = y
    got = R.log_vqt(T(pad), T(g.bank).double(), torch.ones(12, dtype=F64), g.hop, frames)
    want = np.abs(VO.vqt_recursive(y))[g.bin0:g.bin0 + 12]
    assert got.shape == want.shape
    assert (R.magnitude(got) - T(want)).abs().max() < 1e-6 * want.max()                  # the bank is stored in fp32


def test_ulp32():
    v = torch.tensor([1.0, 1.5, 2.0, 0.75, -23.02585, 0.0606], dtype=F64)
    want = [np.spacing(np.float32(abs(x))) for x in v.tolist()]
    assert R.ulp32(v).tolist() == [float(w) for w in want]


# ---------------------------------------------------------------------------------------------------------------------------------
# branches
# ---------------------------------------------------------------------------------------------------------------------------------
def test_every_table_entry_reaches_the_branch_it_names():
    fir = {e[0]: e for e in R.FIR}
    assert len(fir) == len(R.FIR) == len(R.FIR_N) * len(R.FIR_TAPS) + 2
    for cid, n_in, ntaps, n_out, br in R.FIR:
        assert ntaps % 2 == 1 and 0 < ntaps <= 8192 and n_out >= (n_in + 1) // 2 and br == R.fir_branch(n_in, ntaps, n_out), cid
    # hand-stated: staging trips (ntaps > 256: a second trip), blocks (n_out > 256), taps wider than the signal on both sides, an all-zero tail
    assert fir["n513_t257"][4] == (2, 2, False, False) and fir["n512_t255"][4] == (1, 1, False, False) and fir["n511_t1"][4] == (1, 1, False, False)
    assert fir["n1000_t8191"][4] == (32, 2, True, False) and fir["n1_t3"][4] == (1, 1, True, False) and fir["n2_t3"][4] == (1, 1, False, False)
    assert fir[f"n1000_t{R.HALFBAND}"][4] == (2, 2, False, False) and fir["n3_t3_tail"][4] == (1, 1, False, True)
    assert fir["n1000_t255_tail"][4] == (1, 4, False, True)
    from osufusion_amd import audio as A
    assert len(A.halfband_taps()) == R.HALFBAND
    assert {(n + 1) // 2 for n in R.FIR_N} >= {256, 257}                                  # n_out crosses the 256-lane block

    for cid, n_in, hop, K, frames, br in R.FRAME:
        assert br == R.frame_branch(n_in, hop, K, frames), (cid, R.frame_branch(n_in, hop, K, frames))
    assert {e[2] for e in R.FRAME} == {1, 11, 22, 64} and {e[3] for e in R.FRAME} == {1, 32, 257, 1024}
    capped = [e for e in R.FRAME if e[5][1] > 1]
    assert len(capped) == 1 and capped[0][4] * capped[0][3] > R.FRAME_BLOCK_CAP * 256 and capped[0][5][0] == R.FRAME_BLOCK_CAP
    assert capped[0][4] * capped[0][3] * 4 <= 8.5e6                                       # the largest case of the file: about 8 MB
    assert any(e[5][2] for e in R.FRAME) and any(e[5][3] for e in R.FRAME)

    for cid, bins, frames, dld, dldo, br in R.LOGMAG:
        assert br == R.logmag_branch(bins, frames), (cid, R.logmag_branch(bins, frames))
    assert {e[1] for e in R.LOGMAG} == {1, 12, 96, 127, 128, 319} and {e[2] for e in R.LOGMAG} == {1, 63, 64, 65, 130}
    assert {e[3] for e in R.LOGMAG} == {0, 4} and {e[4] for e in R.LOGMAG} == {0, 3}
    assert R.logmag_lds(127) <= 64 * 1024 < R.logmag_lds(128) and R.logmag_lds(319) <= 160 * 1024 < R.logmag_lds(R.LOGMAG_UNSUPPORTED)
    assert R.logmag_branch(R.LOGMAG_UNSUPPORTED, 1)[0] == "unsupported"

    for cid, hop, K, frames, bins, br in R.LOGVQT:
        assert hop % 4 == 0 and K % 4 == 0 and (2 * bins) % 4 == 0 and br == R.logvqt_branch(hop, K, frames, bins), cid
    assert {e[1] for e in R.LOGVQT} >= {4, 8, 44, 176} and {e[2] for e in R.LOGVQT} >= {32, 36, 64, 1024}
    assert {e[3] for e in R.LOGVQT} == {1, 127, 128, 129} and {2 * e[4] for e in R.LOGVQT} == {4, 24, 132, 192}
    assert {e[5][0] for e in R.LOGVQT} == {"<", "==", ">"}


def test_exact_cases_stay_exact_in_fp32():
    assert max(R.FIR_TAPS) * 3 * 4 < 2 ** 24 and max(e[2] for e in R.LOGVQT) * 3 < 2 ** 24       # in units of 1/8
    assert max(e[1] for e in R.FRAME) < 2 ** 24                                                   # frame_signal names indices exactly
    for a, b in R.PYTHAGOREAN:
        assert int(np.sqrt(a * a + b * b)) ** 2 == a * a + b * b
    spec = R.logmag_pythagorean("x", 12, 63)
    re, im = spec[:, :12].double(), spec[:, 12:].double()
    h = torch.sqrt(re * re + im * im)
    assert torch.equal(h.float().double(), h) and torch.equal((re * re + im * im).float().double(), re * re + im * im)


# ---------------------------------------------------------------------------------------------------------------------------------
# caps: 16 x the fp32 CPU evaluation's own distance to fp64, over every case, lies under the cap written next to the table, and that cap
# is the smallest of CAP_SET that does
# ---------------------------------------------------------------------------------------------------------------------------------
def test_caps_fir():
    worst = 0.0
    for cid, n_in, ntaps, n_out, _ in R.FIR:
        x, taps = R.fir_real(cid, n_in, ntaps)
        worst = max(worst, 16 * relmax(R.fir_decimate2(x, taps, n_out), R.fir_decimate2(x.double(), taps.double(), n_out)))
    assert FLOOR < R.FIR_CAP == R.smallest_cap(worst), worst


def test_caps_logmag():
    worst_mag = worst_log = 0.0
    for cid, bins, frames, *_ in R.LOGMAG:
        spec, scale = R.logmag_real(cid, bins, frames), R.bin_scales(bins)
        r64, r32 = R.logmag(spec.double(), scale.double()), R.logmag(spec, scale)
        worst_mag = max(worst_mag, 16 * R.rowrel(R.magnitude(r32), R.magnitude(r64)))
        worst_log = max(worst_log, 16 * R.logdiff(r32, r64, R.loud(R.magnitude(r64))))
    assert FLOOR < R.MAG_CAP == R.smallest_cap(worst_mag), worst_mag
    assert FLOOR < R.LOG_CAP == R.smallest_cap(worst_log), worst_log


def test_caps_log_vqt():
    worst_spec = worst_mag = 0.0
    for cid, hop, K, frames, bins, _ in R.LOGVQT:
        x, bank = R.logvqt_real(cid, hop, K, frames, bins)
        scale = R.bin_scales(bins)
        s64, s32 = R.spectrum(x.double(), bank.double(), hop, frames), R.spectrum(x, bank, hop, frames)
        r64, r32 = R.logmag(s64, scale.double()), R.logmag(s32, scale)
        worst_spec = max(worst_spec, 16 * relmax(s32, s64))
        worst_mag = max(worst_mag, 16 * R.rowrel(R.magnitude(r32), R.magnitude(r64)))
    assert FLOOR < R.SPEC_CAP == R.smallest_cap(worst_spec), worst_spec
    assert FLOOR < R.VQT_MAG_CAP == R.smallest_cap(worst_mag), worst_mag


# ---------------------------------------------------------------------------------------------------------------------------------
# inventory
# ---------------------------------------------------------------------------------------------------------------------------------
def test_every_entry_point_of_audio_hip_has_a_case_table():
    src = (ROOT / "osufusion_amd" / "csrc" / "audio.hip").read_text()
    defined = set(re.findall(r'extern "C"\s+\w+\s+(osuf_\w+)\s*\([^)]*\)\s*\{', src))
    assert defined and defined == set(R.KERNELS) | R.ELSEWHERE, defined ^ (set(R.KERNELS) | R.ELSEWHERE)
    gpu = (ROOT / "tests" / "test_audio_rows_gpu.py").read_text()
    for name, tables in R.KERNELS.items():
        assert all(len(R.TABLES[t]) > 0 for t in tables) and f'"{name}"' in gpu, name
        assert all(f"R.{t}" in gpu for t in tables), name
