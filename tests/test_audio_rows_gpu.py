"""The audio front end's kernels (csrc/audio.hip: osuf_fir_decimate2, osuf_frame_rows, osuf_vqt_logmag, osuf_log_vqt) against plain fp64
references, on every branch their launchers pick from size and stride.  Launches go through ops.call on the raw entry points, so that
strides, NULL arguments and alignment are the test's to choose; no launch consumes another kernel's output.

References, generators and case tables: tests/audio_reference.py (checked on the CPU by tests/test_audio_reference_cpu.py, which also holds
every cap used here at the smallest step above 16 x the fp32 evaluation's own noise).  The branch each case reaches is named in its table
entry and goes to the parity metrics file with the achieved figures (audio_rows::*).

A. Exact: integer signals, taps and banks that are small multiples of a power of two (every partial sum exact in fp32 in any order), and
   the copy kernel: torch.equal against the fp64 result.  osuf_log_vqt's exact statement is about its spectrum workspace: a frame read
   at the wrong offset, or the wrong half of the bank, is an O(1) error there.
B. Real-valued, bounded (tests/bound_check.py): within 16 x e32 of the fp64 reference, e32 being the fp32 CPU evaluation's own distance,
   floored at 1e-6 and capped as the tables say.  Log features are judged as linear magnitudes exp(out) - eps against each bin's own peak,
   and, for osuf_vqt_logmag, as logs where the magnitude is at least 1e-3 of its bin's peak.
C. Exact-argument logs: Pythagorean (re, im) and power-of-two scales make the argument of the log exact up to the rounding of + eps:
   |got - ref| <= 2 ulp32(ref) + 2^-22 (one correctly rounded sqrtf, one product and one sum: 1.5 ulp on the argument; then a 1-ulp logf).
D. Every output sits in a sentinel frame that stays intact, and every refused launch returns its code and writes nothing.
"""
import functools

import pytest
import torch

from osufusion_amd import _lib, ops
from tests import audio_reference as R
from tests import bound_check
from tests.test_poisoned_memory import relmax

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = torch.float32, torch.float64
SENT = 777.0
GUARD = 8                                                   # floats of sentinel on either side of a flat output (keeps 16-byte alignment)
EINVAL, EUNSUPPORTED = _lib.CONSTS["OSUF_EINVAL"], _lib.CONSTS["OSUF_EUNSUPPORTED"]
ID0 = lambda v: v[0] if isinstance(v, tuple) else None


class Check(bound_check.Check):
    prefix = "audio_rows"


def stream():
    return torch.cuda.current_stream().cuda_stream


def p(t):
    return None if t is None else t.data_ptr()


def flat(n):
    """(buffer, the n floats the kernel is given) with GUARD sentinels on either side."""
    buf = torch.full((n + 2 * GUARD,), SENT, dtype=F32, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def flat_intact(buf, n):
    b = buf.cpu()
    assert (b[:GUARD] == SENT).all() and (b[GUARD + n:] == SENT).all(), "written outside the output"


def rows(nrows, width, ld):
    """(buffer, view): `nrows` rows of `width` at row stride ld inside a sentinel-filled (nrows + 2, ld), one spare row above and below."""
    buf = torch.full((nrows + 2, ld), SENT, dtype=F32, device=DEV)
    return buf, buf[1:1 + nrows, :width]


def rows_intact(buf, nrows, width):
    keep = torch.ones(buf.shape, dtype=torch.bool)
    keep[1:1 + nrows, :width] = False
    bad = (keep & (buf.cpu() != SENT)).nonzero()
    assert len(bad) == 0, (len(bad), "cells outside the output were written, first (row, col):", bad[:8].tolist())


def untouched(*ts):
    return all((t.cpu() == SENT).all() for t in ts)


def same(ck, key, got, want64):
    """Exact: the count of differing elements goes to the metrics (bound 0); the assertion names the first of them."""
    got, want = got.cpu(), want64.to(F32)
    assert got.shape == want.shape
    bad = (got != want).nonzero()
    ck.fixed(key + "_mismatches", len(bad), 0)
    ck.done()
    assert torch.equal(got, want), (key, len(bad), "first bad indices:", bad[:8].tolist())


# ---------------------------------------------------------------------------------------------------------------------------------
# osuf_fir_decimate2
# ---------------------------------------------------------------------------------------------------------------------------------
def k_fir(x, taps, out, n_out):
    ops.call("osuf_fir_decimate2", p(x), x.numel(), p(taps), taps.numel(), p(out), n_out, stream())


def fir_where(e):
    st, bl, wide, tail = e[4]
    return dict(case=e[0], branch=f"stage_trips={st},blocks={bl},wide={int(wide)},tail={int(tail)}")


@pytest.mark.parametrize("e", R.FIR, ids=ID0)
def test_fir_exact(e):
    cid, n_in, ntaps, n_out, _ = e
    x, taps = R.fir_exact(cid, n_in, ntaps)
    buf, out = flat(n_out)
    k_fir(x.to(DEV), taps.to(DEV), out, n_out)
    flat_intact(buf, n_out)
    same(Check("fir_exact", F32, **fir_where(e)), "out", out, R.fir_decimate2(x.double(), taps.double(), n_out))


@functools.lru_cache(maxsize=None)
def fir_real(cid, n_in, ntaps, n_out):
    x, taps = R.fir_real(cid, n_in, ntaps)
    return x, taps, R.fir_decimate2(x.double(), taps.double(), n_out), R.fir_decimate2(x, taps, n_out)


@pytest.mark.parametrize("e", R.FIR, ids=ID0)
def test_fir_bounded(e):
    cid, n_in, ntaps, n_out, _ = e
    x, taps, r64, r32 = fir_real(cid, n_in, ntaps, n_out)
    buf, out = flat(n_out)
    k_fir(x.to(DEV), taps.to(DEV), out, n_out)
    flat_intact(buf, n_out)
    ck = Check("fir", F32, **fir_where(e))
    ck.f32("out", out, r64, r32, relmax, R.FIR_CAP)
    ck.done()


def test_fir_bad_arguments_are_refused():
    """Even ntaps, ntaps > 8192, n_out <= 0, n_in <= 0 and NULL pointers: OSUF_EINVAL, and the output keeps its sentinels."""
    lib = _lib.load()
    x, taps = torch.ones(64, device=DEV), torch.ones(8200, device=DEV)
    buf, out = flat(32)
    good = (p(x), 64, p(taps), 3, p(out), 32)
    assert lib.osuf_fir_decimate2(*good, stream()) == 0
    torch.cuda.synchronize()
    out.fill_(SENT)
    for i, v in [(3, 4), (3, 2), (3, 0), (3, 8193), (3, 8194), (3, -1), (5, 0), (5, -1), (1, 0), (1, -1), (0, None), (2, None), (4, None)]:
        a = list(good)
        a[i] = v
        assert lib.osuf_fir_decimate2(*a, stream()) == EINVAL, (i, v)
    assert untouched(buf)


# ---------------------------------------------------------------------------------------------------------------------------------
# osuf_frame_rows
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("e", R.FRAME, ids=ID0)
def test_frame_rows_exact(e):
    """A copy: every row equals the reference bit for bit, cut frames end in zeros and frames wholly past the signal are zeros."""
    cid, n_in, hop, K, frames, (blocks, trips, cut, past) = e
    x = R.frame_signal(cid, n_in)
    buf, out = flat(frames * K)
    xd = x.to(DEV)                                                                       # held until the launch is queued
    ops.call("osuf_frame_rows", p(xd), n_in, hop, K, p(out), frames, stream())
    flat_intact(buf, frames * K)
    got = out.view(frames, K)
    if past:
        assert (got[frames - past:].cpu() == 0).all()
    same(Check("frame_rows", F32, case=cid, branch=f"blocks={blocks},trips={trips},cut={cut},past={past}"), "rows", got,
         R.frame_rows(x.double(), hop, K, frames))


def test_frame_rows_bad_arguments_are_refused():
    lib = _lib.load()
    x = torch.ones(64, device=DEV)
    buf, out = flat(64)
    good = (p(x), 64, 4, 8, p(out), 8)
    for i, v in [(0, None), (4, None), (1, 0), (1, -1), (2, 0), (2, -4), (3, 0), (3, -8), (5, 0), (5, -1)]:
        a = list(good)
        a[i] = v
        assert lib.osuf_frame_rows(*a, stream()) == EINVAL, (i, v)
    assert untouched(buf)


# ---------------------------------------------------------------------------------------------------------------------------------
# osuf_vqt_logmag
# ---------------------------------------------------------------------------------------------------------------------------------
def logmag_where(e):
    kind, blocks, last = e[5]
    return dict(case=e[0], branch=f"{kind},blocks={blocks},last={last},ld=2b+{e[3]},ldo=f+{e[4]}")


def k_logmag(spec, bins, frames, dld, dldo, scale):
    """spec (frames, 2 bins) CPU -> (out buffer, out view) after one launch at ld = 2 bins + dld (sentinels in the padding), ldo = frames + dldo."""
    ld = 2 * bins + dld
    sp = torch.full((frames, ld), SENT, dtype=F32, device=DEV)
    sp[:, :2 * bins] = spec.to(DEV)
    buf, out = rows(bins, frames, frames + dldo)
    sc = scale.to(DEV)
    ops.call("osuf_vqt_logmag", p(sp), ld, p(out), frames + dldo, p(sc), bins, frames, R.EPS, stream())
    rows_intact(buf, bins, frames)
    return out


@pytest.mark.parametrize("e", R.LOGMAG, ids=ID0)
def test_logmag_exact_argument(e):
    cid, bins, frames, dld, dldo, _ = e
    spec, scale = R.logmag_pythagorean(cid, bins, frames), R.bin_scales(bins)
    out = k_logmag(spec, bins, frames, dld, dldo, scale)
    ref = R.logmag(spec.double(), scale.double())
    allow = 2 * R.ulp32(ref) + 2.0 ** -22
    ck = Check("logmag_exact_argument", F32, **logmag_where(e))
    ck.fixed("out_over_allowance", ((out.cpu().double() - ref).abs() / allow).max().item(), 1.0)
    ck.fixed("out_abs", (out.cpu().double() - ref).abs().max().item(), allow.max().item())
    ck.done()


@pytest.mark.parametrize("e", R.LOGMAG, ids=ID0)
def test_logmag_silence_is_log_eps(e):
    cid, bins, frames, dld, dldo, _ = e
    out = k_logmag(torch.zeros(frames, 2 * bins), bins, frames, dld, dldo, R.bin_scales(bins))
    ref = torch.full((bins, frames), R.EPS32, dtype=F64).log()
    ck = Check("logmag_silence", F32, **logmag_where(e))
    ck.fixed("out_abs", (out.cpu().double() - ref).abs().max().item(), (2 * R.ulp32(ref) + 2.0 ** -22).max().item())
    ck.done()


@functools.lru_cache(maxsize=None)
def logmag_real(cid, bins, frames):
    spec, scale = R.logmag_real(cid, bins, frames), R.bin_scales(bins)
    return spec, scale, R.logmag(spec.double(), scale.double()), R.logmag(spec, scale)


def features(ck, out, r64, r32, mag_cap, log_cap=None):
    """Section B's statements about a (bins, frames) block of log features."""
    m64 = R.magnitude(r64)
    ck.f32("mag", R.magnitude(out).float(), m64, R.magnitude(r32), R.rowrel, mag_cap)
    if log_cap is not None:
        mask = R.loud(m64)
        ck.f32("log", out, r64, r32, lambda a, b: R.logdiff(a, b, mask), log_cap)


@pytest.mark.parametrize("e", R.LOGMAG, ids=ID0)
def test_logmag_bounded(e):
    cid, bins, frames, dld, dldo, _ = e
    spec, scale, r64, r32 = logmag_real(cid, bins, frames)
    out = k_logmag(spec, bins, frames, dld, dldo, scale)
    ck = Check("logmag", F32, **logmag_where(e))
    features(ck, out, r64, r32, R.MAG_CAP, R.LOG_CAP)
    ck.done()


def test_logmag_refusals_write_nothing():
    """bins = 320 needs 164,096 B of LDS: OSUF_EUNSUPPORTED.  ld < 2 bins, ldo < frames, NULL pointers and empty shapes: OSUF_EINVAL."""
    lib = _lib.load()
    bins, frames = R.LOGMAG_UNSUPPORTED, 3
    assert R.logmag_branch(bins, frames)[0] == "unsupported"
    sp, sc = torch.ones(frames, 2 * bins, device=DEV), torch.ones(bins, device=DEV)
    buf, out = rows(bins, frames, frames)
    assert lib.osuf_vqt_logmag(p(sp), 2 * bins, p(out), frames, p(sc), bins, frames, R.EPS, stream()) == EUNSUPPORTED
    good = [p(sp), 24, p(out), frames, p(sc), 12, frames, R.EPS]
    for i, v in [(1, 23), (1, 0), (3, frames - 1), (3, 0), (0, None), (2, None), (4, None), (5, 0), (5, -1), (6, 0), (6, -1)]:
        a = list(good)
        a[i] = v
        assert lib.osuf_vqt_logmag(*a, stream()) == EINVAL, (i, v)
    assert untouched(buf)


# ---------------------------------------------------------------------------------------------------------------------------------
# osuf_log_vqt: the fp32 NT GEMM on overlapping rows (lda = hop), then the log-magnitude transpose
# ---------------------------------------------------------------------------------------------------------------------------------
def logvqt_where(e):
    rel, tiles, last, ksteps, klast = e[5]
    return dict(case=e[0], branch=f"hop{rel}K,m_tiles={tiles},last_rows={last},k_steps={ksteps},k_last={klast},N={2 * e[4]}")


def k_logvqt(x, bank, scale, hop, frames):
    """-> (spectrum workspace, out view): out is rows [2, 2 + bins) of a sentinel-filled (bins + 5, frames + 3), as audio.py slices its result."""
    bins, K = bank.shape[0] // 2, bank.shape[1]
    wbuf, ws = flat(frames * 2 * bins)
    total = torch.full((bins + 5, frames + R.OUT_PAD), SENT, dtype=F32, device=DEV)
    out = total[2:2 + bins, :frames]
    xd, bd, sd = x.to(DEV), bank.to(DEV), scale.to(DEV)                                  # held until the launch is queued
    ops.call("osuf_log_vqt", p(xd), x.numel(), p(bd), K, bins, hop, p(sd), R.EPS, p(ws), p(out), total.stride(0), frames, stream())
    flat_intact(wbuf, frames * 2 * bins)
    keep = torch.ones(total.shape, dtype=torch.bool)
    keep[2:2 + bins, :frames] = False
    bad = (keep & (total.cpu() != SENT)).nonzero()
    assert len(bad) == 0, (len(bad), "cells outside the row slice were written, first (row, col):", bad[:8].tolist())
    return ws.view(frames, 2 * bins), out


@pytest.mark.parametrize("e", R.LOGVQT, ids=ID0)
def test_log_vqt_exact_spectrum(e):
    cid, hop, K, frames, bins, _ = e
    x, bank = R.logvqt_exact(cid, hop, K, frames, bins)
    scale = R.bin_scales(bins)
    ws, out = k_logvqt(x, bank, scale, hop, frames)
    s64 = R.spectrum(x.double(), bank.double(), hop, frames)
    r64, r32 = R.logmag(s64, scale.double()), R.logmag(s64.float(), scale)
    ck = Check("log_vqt_exact", F32, **logvqt_where(e))
    features(ck, out, r64, r32, R.VQT_MAG_CAP)
    same(ck, "spectrum", ws, s64)


@functools.lru_cache(maxsize=None)
def logvqt_real(cid, hop, K, frames, bins):
    x, bank = R.logvqt_real(cid, hop, K, frames, bins)
    scale = R.bin_scales(bins)
    s64, s32 = R.spectrum(x.double(), bank.double(), hop, frames), R.spectrum(x, bank, hop, frames)
    return x, bank, scale, s64, s32, R.logmag(s64, scale.double()), R.logmag(s32, scale)


@pytest.mark.parametrize("e", R.LOGVQT, ids=ID0)
def test_log_vqt_bounded(e):
    cid, hop, K, frames, bins, _ = e
    x, bank, scale, s64, s32, r64, r32 = logvqt_real(cid, hop, K, frames, bins)
    ws, out = k_logvqt(x, bank, scale, hop, frames)
    ck = Check("log_vqt", F32, **logvqt_where(e))
    ck.f32("spectrum", ws, s64, s32, relmax, R.SPEC_CAP)
    features(ck, out, r64, r32, R.VQT_MAG_CAP)
    ck.done()


def test_log_vqt_refusals_write_nothing():
    """A last frame past n_pad, hop % 4 != 0, K % 4 != 0, NULL pointers and empty shapes: OSUF_EINVAL, and neither the workspace nor the
    output is written."""
    lib = _lib.load()
    hop, K, frames, bins = 8, 32, 5, 6
    n_pad = R.logvqt_n_pad(hop, K, frames)
    x, bank, sc = torch.ones(n_pad + 64, device=DEV), torch.ones(2 * bins, 40, device=DEV), torch.ones(bins, device=DEV)
    wbuf, ws = flat(frames * 2 * bins)
    buf, out = rows(bins, frames, frames + R.OUT_PAD)
    # (wave_pad, n_pad, bank, K, bins, hop, scale, eps, spec_ws, out, ldo, frames)
    good = [p(x), n_pad, p(bank), K, bins, hop, p(sc), R.EPS, p(ws), p(out), frames + R.OUT_PAD, frames]
    bad = [(1, n_pad - 1), (11, frames + 1), (5, 6), (5, 10), (3, 34), (3, 30), (0, None), (2, None), (8, None), (9, None), (6, None),
           (11, 0), (11, -1), (5, 0), (3, 0), (4, 0), (10, frames - 1)]
    for i, v in bad:
        a = list(good)
        a[i] = v
        assert lib.osuf_log_vqt(*a, stream()) == EINVAL, (i, v)
    assert untouched(wbuf, buf)
