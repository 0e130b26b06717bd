"""Plain torch references of the audio front end's kernels (csrc/audio.hip: fir_decimate2, frame_rows, vqt_logmag, log_vqt), written from
the comments above each kernel and from include/osufusion_hip.h alone, the launchers' branch arithmetic restated, and the case tables and
seeded generators of tests/test_audio_rows_gpu.py.

    fir_decimate2 : out[m] = sum_j taps[j] * x[2m + j - (ntaps-1)/2], x zero outside [0, n_in), m < n_out
    frame_rows    : rows[t][i] = x[t*hop + i], zero past n_in
    logmag        : out[k][t] = log(scale[k] * |spec[t][k] + i spec[t][bins + k]| + eps)
    log_vqt       : logmag(frame_rows(wave_pad, hop, K, frames) @ bank^T, scale, eps)

Every function computes in the dtype of its inputs: fp64 for the reference, fp32 for the "same formula in single precision" whose
distance to the fp64 result scales the tests' bounds (tests/bound_check.py).  Nothing here needs a GPU; tests/test_audio_reference_cpu.py
checks these functions against independent formulations and against the slips they must tell apart, the branch each table entry names,
and the caps written next to the tables.
"""
from __future__ import annotations

import math

import torch

from tests.gemm_reference import _gen, ints  # noqa: F401  (ints: the exact cases' operands)

F32, F64 = torch.float32, torch.float64
EPS = 1e-10                                                 # the product's LOG_EPS; the kernels take it as a float
EPS32 = torch.tensor(EPS, dtype=F32).item()                 # what the kernel adds
CAP_SET = (1e-5, 2e-5, 5e-5, 1e-4)

# every extern "C" entry point of csrc/audio.hip but osuf_resample (tests/test_resample_gpu.py) -> the tables below that launch it
KERNELS = {"osuf_fir_decimate2": ("FIR",), "osuf_frame_rows": ("FRAME",), "osuf_vqt_logmag": ("LOGMAG",), "osuf_log_vqt": ("LOGVQT",)}
ELSEWHERE = {"osuf_resample"}


# ---------------------------------------------------------------------------------------------------------------------------------
# formulas
# ---------------------------------------------------------------------------------------------------------------------------------
def fir_decimate2(x, taps, n_out):
    """The zero-extended correlation, accumulated tap by tap (j ascending) in the dtype of x."""
    n_in, ntaps = x.numel(), taps.numel()
    c = (ntaps - 1) // 2
    xp = torch.zeros(c + max(n_in, 2 * n_out) + ntaps, dtype=x.dtype)
    xp[c:c + n_in] = x
    out = torch.zeros(n_out, dtype=x.dtype)
    for j in range(ntaps):
        out += taps[j] * xp[j:j + 2 * n_out:2]              # xp[2m + j] = x[2m + j - c]
    return out


def frame_rows(x, hop, K, frames):
    idx = torch.arange(frames)[:, None] * hop + torch.arange(K)[None, :]
    return torch.where(idx < x.numel(), x[idx.clamp_max(x.numel() - 1)], torch.zeros((), dtype=x.dtype))


def logmag(spec, scale, eps=EPS32):
    """spec (frames, 2*bins) -> (bins, frames)."""
    bins = spec.shape[1] // 2
    re, im = spec[:, :bins], spec[:, bins:]
    return torch.log(scale[:, None] * torch.sqrt(re * re + im * im).T + eps)


def spectrum(wave_pad, bank, hop, frames):
    return frame_rows(wave_pad, hop, bank.shape[1], frames) @ bank.T


def log_vqt(wave_pad, bank, scale, hop, frames, eps=EPS32):
    return logmag(spectrum(wave_pad, bank, hop, frames), scale, eps)


def magnitude(out, eps=EPS32):
    """The linear magnitude behind a log feature, in fp64."""
    return torch.exp(out.double()) - eps


# ---------------------------------------------------------------------------------------------------------------------------------
# metrics and bounds
# ---------------------------------------------------------------------------------------------------------------------------------
def rowrel(a, b):
    """max over the rows (bins) of max|a - b| / max|b|: each bin is judged against its own peak."""
    a, b = a.double().cpu(), b.double()
    return ((a - b).abs().amax(1) / b.abs().amax(1).clamp_min(1e-300)).max().item()


def loud(mag64):
    """Where a row's magnitude is at least 1e-3 of that row's maximum."""
    return mag64 >= 1e-3 * mag64.amax(1, keepdim=True)


def logdiff(a, b, mask):
    """max |a - b| over mask (0 when the mask is empty)."""
    d = (a.double().cpu() - b.double()).abs()[mask]
    return d.max().item() if d.numel() else 0.0


def ulp32(v):
    """Spacing of fp32 at |v| (fp64 tensor in, fp64 out)."""
    _, e = torch.frexp(v.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(v), e - 24)


def smallest_cap(worst):
    """The smallest of CAP_SET above `worst` (16 x the fp32 CPU evaluation's distance, over every case of a kernel)."""
    return next(c for c in CAP_SET if worst < c)


# ---------------------------------------------------------------------------------------------------------------------------------
# which branch the launchers take (osuf_fir_decimate2 / osuf_frame_rows / osuf_vqt_logmag / osuf_log_vqt restated)
# ---------------------------------------------------------------------------------------------------------------------------------
def fir_branch(n_in, ntaps, n_out):
    """(trips of the 256-lane tap staging loop, blocks, every output loses taps on both sides, outputs past ceil(n_in / 2))."""
    return -(-ntaps // 256), -(-n_out // 256), ntaps > 2 * n_in, n_out > (n_in + 1) // 2


FRAME_BLOCK_CAP = 8192


def frame_branch(n_in, hop, K, frames):
    """(blocks, grid-stride trips, frames cut by n_in, frames wholly past n_in)."""
    blocks = min(-(-frames * K // 256), FRAME_BLOCK_CAP)
    starts = [t * hop for t in range(frames)]
    return blocks, -(-frames * K // (blocks * 256)), sum(s < n_in < s + K for s in starts), sum(s >= n_in for s in starts)


def logmag_lds(bins):
    return 64 * (2 * bins + 1) * 4


def logmag_branch(bins, frames):
    """("plain" | "attr" | "unsupported", blocks, frames of the last block)."""
    lds = logmag_lds(bins)
    kind = "unsupported" if lds > 160 * 1024 else "attr" if lds > 64 * 1024 else "plain"
    return kind, -(-frames // 64), frames - 64 * ((frames - 1) // 64)


def logvqt_branch(hop, K, frames, bins):
    """(hop against K, 128-row tiles, rows of the last tile, 32-float k steps, floats of the last k step)."""
    rel = "<" if hop < K else "==" if hop == K else ">"
    return rel, -(-frames // 128), frames - 128 * ((frames - 1) // 128), -(-K // 32), K - 32 * ((K - 1) // 32)


# ---------------------------------------------------------------------------------------------------------------------------------
# case tables.  Caps (relmax for fir and the spectrum, rowrel for magnitudes, absolute for logs): the smallest of CAP_SET above 16 x the
# fp32 CPU evaluation's own distance to fp64 over every case of the table, held there by test_caps_* of the CPU file.
# ---------------------------------------------------------------------------------------------------------------------------------
HALFBAND = 375                                              # len(audio.halfband_taps())
FIR_N = (1, 2, 3, 511, 512, 513, 1000)
FIR_TAPS = (1, 3, 255, 257, HALFBAND, 8191)
# (id, n_in, ntaps, n_out, branch): every n_in x ntaps at n_out = ceil(n_in / 2), and two cases whose tail is all zero-extension
FIR = [(f"n{n}_t{t}", n, t, (n + 1) // 2, fir_branch(n, t, (n + 1) // 2)) for n in FIR_N for t in FIR_TAPS] + \
      [("n3_t3_tail", 3, 3, 7, fir_branch(3, 3, 7)), ("n1000_t255_tail", 1000, 255, 800, fir_branch(1000, 255, 800))]
FIR_CAP = 2e-5

# (id, n_in, hop, K, frames, (blocks, trips, cut frames, frames wholly past))
FRAME = [
    ("h1_k1", 5, 1, 1, 7, (1, 1, 0, 2)),                    # K = 1: a frame is in or out
    ("h11_k32", 100, 11, 32, 11, (2, 1, 3, 1)),
    ("h22_k257", 700, 22, 257, 33, (34, 1, 11, 1)),         # odd K: rows start at every alignment
    ("h64_k1024", 3000, 64, 1024, 48, (192, 1, 16, 1)),
    ("h64_k32", 1000, 64, 32, 16, (2, 1, 0, 0)),            # hop > K, nothing cut
    ("h11_k1", 30, 11, 1, 4, (1, 1, 0, 1)),
    ("h1_k1024_cap", 2100, 1, 1024, 2049, (8192, 2, 972, 0)),   # frames K = 2,098,176 > 8192 x 256: the grid-stride second trip (8 MB of rows)
]

# (id, bins, frames, ld - 2 bins, ldo - frames, (kind, blocks, frames of the last block))
LOGMAG = [
    ("b1_f1", 1, 1, 0, 0, ("plain", 1, 1)),
    ("b12_f63", 12, 63, 4, 3, ("plain", 1, 63)),
    ("b96_f64", 96, 64, 0, 3, ("plain", 1, 64)),            # the product's width
    ("b127_f65", 127, 65, 4, 0, ("plain", 2, 1)),           # 65,280 B: the last size without the attribute
    ("b128_f130", 128, 130, 4, 3, ("attr", 3, 2)),          # 65,792 B
    ("b128_f1", 128, 1, 0, 0, ("attr", 1, 1)),
    ("b319_f65", 319, 65, 0, 0, ("attr", 2, 1)),            # 163,584 B of the 163,840 a workgroup can have
    ("b319_f130", 319, 130, 4, 3, ("attr", 3, 2)),
    ("b12_f130", 12, 130, 0, 0, ("plain", 3, 2)),
]
LOGMAG_UNSUPPORTED = 320                                    # 164,096 B
MAG_CAP, LOG_CAP = 1e-5, 1e-5

# (id, hop, K, frames, bins, (hop against K, m tiles, rows of the last tile, k steps, floats of the last k step))
LOGVQT = [
    ("h4_k32_f129_n4", 4, 32, 129, 2, ("<", 2, 1, 1, 32)),
    ("h8_k36_f127_n24", 8, 36, 127, 12, ("<", 1, 127, 2, 4)),
    ("h44_k64_f128_n132", 44, 64, 128, 66, ("<", 1, 128, 2, 32)),       # two n tiles (132 = 128 + 4)
    ("h176_k1024_f129_n192", 176, 1024, 129, 96, ("<", 2, 1, 32, 32)),  # the product's hop and width
    ("h36_k36_f1_n24", 36, 36, 1, 12, ("==", 1, 1, 2, 4)),              # hop == K: dense rows, what the framed low octaves hand over
    ("h176_k32_f127_n4", 176, 32, 127, 2, (">", 1, 127, 1, 32)),        # hop > K: rows with gaps between them
    ("h8_k64_f1_n132", 8, 64, 1, 66, ("<", 1, 1, 2, 32)),
]
# the spectrum (relmax) and the linear magnitude (rowrel).  The log of a magnitude at 1e-3 of its row's peak carries the spectrum's error a
# thousandfold (1.6e-4 .. 2.6e-4 in the fp32 CPU evaluation, above every cap of CAP_SET), so log_vqt's features are judged as magnitudes;
# the log itself is osuf_vqt_logmag's, checked on spectra it is handed exactly.
SPEC_CAP, VQT_MAG_CAP = 1e-5, 1e-5
OUT_PAD = 3                                                 # out is a row slice of a (bins_total, frames + 3) buffer
TABLES = {"FIR": FIR, "FRAME": FRAME, "LOGMAG": LOGMAG, "LOGVQT": LOGVQT}


# ---------------------------------------------------------------------------------------------------------------------------------
# seeded inputs
# ---------------------------------------------------------------------------------------------------------------------------------
def uni(tag, shape, scale=1.0):
    """fp32 U(-scale, scale), deterministic in (tag, shape)."""
    return ((2 * torch.rand(*shape, generator=_gen(tag, shape), dtype=F64) - 1) * scale).to(F32)


def halfband():
    from osufusion_amd import audio
    return torch.from_numpy(audio.halfband_taps()).to(F32)


def fir_exact(cid, n_in, ntaps):
    """Integer signal |x| <= 3, taps = integers of [-4, 4] / 8: every partial sum is a multiple of 1/8 below 2^24 / 8, exact in fp32."""
    return ints(f"au.fx.{cid}", (n_in,), 3), ints(f"au.ft.{cid}", (ntaps,), 4) / 8


def fir_real(cid, n_in, ntaps):
    """|x| <= 1; the product's half-band filter where the length is its length, else U(-1, 1) / sqrt(ntaps)."""
    taps = halfband() if ntaps == HALFBAND else uni(f"au.frt.{cid}", (ntaps,), 1 / math.sqrt(ntaps))
    return uni(f"au.frx.{cid}", (n_in,)), taps


def frame_signal(cid, n_in):
    """Values that name their index (exact in fp32, none of them zero)."""
    return torch.arange(1, n_in + 1, dtype=F32)


def bin_scales(bins):
    """A distinct power of two per bin, 2^-3 .. 2^3."""
    return torch.ldexp(torch.ones(bins, dtype=F32), torch.arange(bins) % 7 - 3)


PYTHAGOREAN = ((3, 4), (5, 12), (8, 15), (7, 24), (20, 21), (12, 35), (9, 40))


def logmag_pythagorean(cid, bins, frames):
    """(re, im) = +-(a, b) or +-(b, a) of a Pythagorean pair times 2^(-2..2): the root is exact, and so is the product with a power of two."""
    g = _gen(f"au.py.{cid}", (frames, bins))
    pick = torch.randint(0, len(PYTHAGOREAN), (frames, bins), generator=g)
    pairs = torch.tensor(PYTHAGOREAN, dtype=F32)[pick]                                   # (frames, bins, 2)
    swap = torch.randint(0, 2, (frames, bins), generator=g).bool()
    re, im = torch.where(swap, pairs[..., 1], pairs[..., 0]), torch.where(swap, pairs[..., 0], pairs[..., 1])
    sign = lambda: (2 * torch.randint(0, 2, (frames, bins), generator=g) - 1).float()
    mul = torch.ldexp(torch.ones(frames, bins), torch.randint(-2, 3, (frames, bins), generator=g))
    return torch.cat([re * sign() * mul, im * sign() * mul], 1)


def logmag_real(cid, bins, frames):
    """A spectrum whose rows span three decades, so that every bin has loud and quiet frames."""
    amp = torch.pow(10.0, uni(f"au.la.{cid}", (frames, 1), 1.5).double()).to(F32)
    return uni(f"au.ls.{cid}", (frames, 2 * bins)) * amp


def logvqt_n_pad(hop, K, frames):
    return (frames - 1) * hop + K


def logvqt_exact(cid, hop, K, frames, bins):
    """Integer waveform |x| <= 3 and bank entries of {-1, 0, 1} / 8: the spectrum is a multiple of 1/8 below 2^24 / 8."""
    return ints(f"au.vx.{cid}", (logvqt_n_pad(hop, K, frames),), 3), ints(f"au.vb.{cid}", (2 * bins, K), 1) / 8


def logvqt_real(cid, hop, K, frames, bins):
    return uni(f"au.vrx.{cid}", (logvqt_n_pad(hop, K, frames),)), uni(f"au.vrb.{cid}", (2 * bins, K), 1 / math.sqrt(K))
