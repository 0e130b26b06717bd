"""Plain references of the layout, loss, optimizer and DDPM / DDIM kernels (the head of csrc/elementwise.hip, the two kernels at the top of
csrc/sampling.hip), written from the formulas in the kernels' comments and include/osufusion_hip.h, with the input generators, the case
tables and the contract table of tests/test_elementwise_rows_gpu.py.  Nothing here needs a GPU; tests/test_elementwise_reference_cpu.py
checks every function against an independent restatement, the branch each table entry names, and the caps.

    moves      : index arithmetic on fp32 values; a bf16 result is the fp32 value rounded once by rne_bf16 (integer arithmetic on the bits)
    arithmetic : every function computes in the dtype of its tensor inputs: fp64 is the reference, fp32 the "same formula in single
                 precision" whose distance to the fp64 result (e32) scales the bounds of tests/bound_check.py

The grid of every kernel here is capped at GRID_CAP threads (ew_grid: 2048 blocks of 256); above it a thread takes a second trip of its
grid-stride loop, and the kernels with a scalar tail leave it to block 0.  "second_pass" cases sit just above the cap and are no multiple
of it.  A chunk kernel (ncl_to_rows, copy2d, add2d) spends a thread on 8 elements, so its case above the cap has 4.2 M of them.
"""
from __future__ import annotations

import numpy as np
import torch

from tests.gemm_reference import _gen, ints  # noqa: F401  (ints: the exact cases' operands)

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
GRID_CAP = 2048 * 256
EINVAL, EUNSUPPORTED = -1, -2


# ---------------------------------------------------------------------------------------------------------------------------------
# bits
# ---------------------------------------------------------------------------------------------------------------------------------
def rne_bf16(bits):
    """fp32 bit patterns (uint32) -> bf16 bit patterns (uint16), round to nearest, ties to even, in integer arithmetic: the half-word that
    is dropped is compared with 0x8000 by adding 0x7FFF plus the last kept bit.  The carry walks into the exponent, so the largest finite
    values round to +-inf, subnormals round like every other value and +-0 keep their sign.  A NaN stays a NaN (quiet bit set: its payload
    could otherwise be rounded away); a kernel may return any NaN for it."""
    b = np.asarray(bits, dtype=np.uint32).astype(np.uint64)
    nan = ((b & 0x7F800000) == 0x7F800000) & ((b & 0x007FFFFF) != 0)
    r = (b + 0x7FFF + ((b >> 16) & 1)) >> 16
    return np.where(nan, (b >> 16) | 0x0040, r).astype(np.uint16)


def bf16_is_nan(h):
    h = np.asarray(h, dtype=np.uint16)
    return ((h & 0x7F80) == 0x7F80) & ((h & 0x007F) != 0)


def f32_bits(t):
    """fp32 tensor -> uint32 array of its bits (same shape)."""
    return t.detach().cpu().contiguous().view(torch.int32).numpy().view(np.uint32)


def f32_from_bits(bits):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(bits, dtype=np.uint32)).view(np.int32)).view(F32)


def bf16_bits(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def bf16_from_bits(h):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(h, dtype=np.uint16)).view(np.int16)).view(BF16)


def round_bf16(t):
    """fp32 tensor -> bf16 tensor, through rne_bf16."""
    return bf16_from_bits(rne_bf16(f32_bits(t)))


def stored_bits(t):
    """What a tensor of either storage dtype holds, as an unsigned integer array."""
    return f32_bits(t) if t.dtype == F32 else bf16_bits(t)


def expect_bits(v32, dtype):
    """The bits a kernel must store for the fp32 values v32 in `dtype`."""
    return f32_bits(v32) if dtype == F32 else rne_bf16(f32_bits(v32))


def bits_differ(got, want, dtype):
    """Boolean array: where the stored bits differ from the expected ones; where a NaN is expected, any NaN is equal."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    if dtype == F32:
        gn = ((got & 0x7F800000) == 0x7F800000) & ((got & 0x007FFFFF) != 0)
        wn = ((want & 0x7F800000) == 0x7F800000) & ((want & 0x007FFFFF) != 0)
    else:
        gn, wn = bf16_is_nan(got), bf16_is_nan(want)
    return np.where(wn, ~gn, got != want)


LOW_HALVES = (0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF)


def pattern_table():
    """Every upper half-word crossed with LOW_HALVES: 393 216 fp32 bit patterns (ties to even in both directions, the largest finite
    values, subnormals, +-0, +-inf and NaNs of every upper payload)."""
    hi = np.arange(0x10000, dtype=np.uint32)[:, None] << 16
    return (hi | np.array(LOW_HALVES, dtype=np.uint32)[None, :]).reshape(-1)


SPECIAL_EXPONENTS = (0, 1, 2, 64, 100, 126, 127, 128, 200, 253, 254, 255)


def special_patterns():
    """About 200 patterns for the scalar conversion: for a dozen exponents (0: subnormals, 255: inf / NaN, 254: rounds to inf), both
    signs, an even and an odd last kept bit, the dropped half just below, at and just above the tie and at its maximum; then +-0, +-inf,
    the smallest subnormal, the largest finite value, a quiet and a signalling NaN."""
    out = []
    for e in SPECIAL_EXPONENTS:
        for s in (0, 1):
            for m7 in (0x00, 0x7F):
                for lo in (0x7FFF, 0x8000, 0x8001, 0xFFFF):
                    out.append((s << 31) | (e << 23) | (m7 << 16) | lo)
    out += [0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x7F7FFFFF, 0x7FC00000, 0x7F800001, 0x00008000, 0x00018000, 0x3F808000]
    return np.array(out, dtype=np.uint32)


# ---------------------------------------------------------------------------------------------------------------------------------
# moves (fp32 values; the storage rounding is expect_bits')
# ---------------------------------------------------------------------------------------------------------------------------------
def ncl_to_rows(x, C, L, KT, width):
    """x (B, C, L) -> (B * L, width):  out[b*L + n][t*C + ci] = x[b][ci][n + t - KT/2], zero outside [0, L), zero in columns [C*KT, width)."""
    B = x.shape[0]
    assert tuple(x.shape) == (B, C, L) and width >= C * KT
    row, col = np.indices((B * L, width))
    b, n = row // L, row % L
    t, ci = col // C, col % C
    src = n + t - KT // 2
    ok = (t < KT) & (src >= 0) & (src < L)
    flat = x.reshape(-1)[torch.from_numpy((b * C + ci) * L + np.clip(src, 0, L - 1))]
    return torch.where(torch.from_numpy(ok), flat, torch.zeros((), dtype=x.dtype))


def rows_to_ncl(rows, B, C, L):
    """rows (B * L, ld >= C) -> (B, C, L):  out[b][ci][n] = rows[b*L + n][ci]."""
    assert rows.shape[0] == B * L and rows.shape[1] >= C
    b, ci, n = np.indices((B, C, L))
    return rows[torch.from_numpy(b * L + n), torch.from_numpy(ci)]


def copy2d(src, cols):
    """dst[m][c] = src[m][c] for c < cols."""
    m, c = np.indices((src.shape[0], cols))
    return src[torch.from_numpy(m), torch.from_numpy(c)]


def add2d(a, b, cols):
    """dst[m][c] = a[m][c] + b[m][c] for c < cols, in the dtype of a and b."""
    return copy2d(a, cols) + copy2d(b, cols)


# ---------------------------------------------------------------------------------------------------------------------------------
# arithmetic (in the dtype of the tensor arguments)
# ---------------------------------------------------------------------------------------------------------------------------------
def mse_weight(orig_len, wt, B, L, dtype):
    """w[b][n] = [n < len[b]] * wt[b]; a missing len is L, a missing wt one."""
    w = torch.ones(B, L, dtype=dtype)
    if orig_len is not None:
        w = (torch.arange(L)[None, :] < orig_len.long()[:, None]).to(dtype)
    if wt is not None:
        w = w * wt.to(dtype)[:, None]
    return w


def mse(pred, target, orig_len=None, wt=None):
    """-> (sum w (p - t)^2, grad = (2 w) (p - t)) for (B, Dch, L) tensors."""
    B, _, L = pred.shape
    w = mse_weight(orig_len, wt, B, L, pred.dtype)[:, None, :]
    d = pred - target
    return (w * d * d).sum(), (2 * w) * d


def sqnorm(g):
    return (g * g).sum()


def f32v(x):
    """A hyper-parameter as the entry point receives it: the fp32 value nearest to x, as a Python float."""
    return float(np.float32(x))


# (lr, beta1, beta2, eps); the kernels take floats, so the references start from the same fp32 values (1 - float(0.999) is not 0.001)
HYPER = tuple(f32v(x) for x in (1e-3, 0.9, 0.999, 1e-8))


def adamw_step(p, g, m, v, hyper, step, gs=1.0):
    """torch.optim.AdamW (decoupled decay, no amsgrad), one step from the state (m, v):  hyper = (lr, beta1, beta2, eps, wd); the gradient
    is g * gs.  -> (p', m', v')"""
    lr, b1, b2, eps, wd = hyper
    ge = g * gs
    m2 = b1 * m + (1 - b1) * ge
    v2 = b2 * v + (1 - b2) * ge * ge
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    denom = v2.sqrt() / bc2 ** 0.5 + eps
    return p * (1 - lr * wd) - (lr / bc1) * m2 / denom, m2, v2


def clip_coef(sumsq, max_norm, base):
    """coef = min(1, max_norm / (sqrt(sumsq) + 1e-6)) * base, or base when max_norm <= 0; in fp64 (Python floats)."""
    if not max_norm > 0:
        return base
    return min(1.0, max_norm / (sumsq ** 0.5 + 1e-6)) * base


def _per_sample(c, x):
    return c.to(x.dtype).view(-1, *([1] * (x.dim() - 1)))


def axpby(x, y, ca, cb):
    """out[b] = ca[b] x[b] + cb[b] y[b]"""
    return _per_sample(ca, x) * x + _per_sample(cb, x) * y


def ddim_step(x, cond, null, cond_scale, coef):
    """eps = null + (cond - null) cond_scale (cond without null); x0 = clamp((x - c0 eps) / c1, -1, 1); out = c2 x0 + c3 eps, c = coef[b]."""
    eps = cond if null is None else null + (cond - null) * cond_scale
    c = [_per_sample(coef[:, j], x) for j in range(4)]
    x0 = ((x - c[0] * eps) / c[1]).clamp(-1.0, 1.0)
    return c[2] * x0 + c[3] * eps


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------
def uni(tag, shape, scale=1.0):
    """fp32 U(-scale, scale), deterministic in (tag, shape)."""
    return ((2 * torch.rand(*shape, generator=_gen(tag, shape), dtype=F64) - 1) * scale).to(F32)


def ncl_input(tag, B, C, L):
    """|noise| < 1 around 8 (b + 1): a tap that reads its neighbour's sample returns a value 8 off, not a zero."""
    return uni(tag, (B, C, L)) + 8.0 * torch.arange(1, B + 1, dtype=F32).view(B, 1, 1)


def rows_input(tag, M, ld, dtype):
    """(M, ld) values that `dtype` holds exactly, as fp32."""
    v = uni(tag, (M, ld), 4.0)
    return v if dtype == F32 else round_bf16(v).to(F32)


MSE_WT = (1.0, 0.0, -0.5, 1000.0)                          # one, zero, a negative and a large weight; a sample's share never cancels another's


def mse_inputs(cid, B, Dch, L, has_len, has_wt):
    pred, target = uni(f"mse.p.{cid}", (B, Dch, L), 2.0), uni(f"mse.t.{cid}", (B, Dch, L), 2.0)
    lens = ([max(L // 3, 1), 0, L + 5, L] * B)[:B]                                      # interior, empty, past the end, exactly L
    wts = [MSE_WT[(b + 3) % 4] for b in range(B)]                                       # the large weight first: it owns a non-empty sample
    return dict(pred=pred, target=target, orig_len=torch.tensor(lens, dtype=torch.int32) if has_len else None,
                wt=torch.tensor(wts, dtype=F32) if has_wt else None)


ZERO_BLOCK = 5                                             # adamw: elements [1, 1 + ZERO_BLOCK) (as far as n goes) have g = 0 and v = 0


def adamw_inputs(n):
    """p, g of order one, m of order 0.1, v >= 0; in the zero block the denominator is eps alone, and m is of order eps so that the
    update there is of the order of the others (a wrong eps shows, and does not drown the rest in max|update|)."""
    p, g = uni("aw.p", (n,), 2.0), uni("aw.g", (n,), 1.0)
    m, v = uni("aw.m", (n,), 0.1), uni("aw.v", (n,), 0.5).abs() * 0.02
    z = slice(1, 1 + ZERO_BLOCK)
    g[z], v[z] = 0.0, 0.0
    m[z] = m[z] * 1e-7
    return p, g, m, v


def ddim_coef(ts=(980, 500, 20, 0), steps=50, dtype=F64):
    """coef[b] = {sqrt(1 - a_t), sqrt(a_t), sqrt(a_prev), sqrt(1 - a_prev)} of the DDIM schedule (1000 linear betas, `steps` sampling
    steps, alpha_prev = 1 past the end) at four different t."""
    betas = torch.linspace(1e-4, 0.02, 1000, dtype=F64)
    acp = torch.cumprod(1 - betas, 0)
    rows = []
    for t in ts:
        prev = t - 1000 // steps
        a_t, a_p = acp[t], acp[prev] if prev >= 0 else torch.tensor(1.0, dtype=F64)
        rows.append(torch.stack([(1 - a_t).sqrt(), a_t.sqrt(), a_p.sqrt(), (1 - a_p).sqrt()]))
    return torch.stack(rows).to(dtype)


def ddim_inputs(cid, B, per, has_null, cond_scale, span):
    """x is built from the start prediction it should give: |x0| <= span (0.8: the clamp is inactive everywhere; 3: it saturates on both
    sides in every sample).  All fp32."""
    coef = ddim_coef()[:B].to(F32)
    cond = uni(f"dd.c.{cid}", (B, per))
    null = uni(f"dd.n.{cid}", (B, per)) if has_null else None
    x0 = uni(f"dd.x0.{cid}", (B, per), span)
    if per >= 2:
        x0[:, 0], x0[:, 1] = span, -span
    eps = cond.double() if null is None else null.double() + (cond.double() - null.double()) * cond_scale
    c = coef.double()
    x = (c[:, 1:2] * x0.double() + c[:, 0:1] * eps).to(F32)
    return dict(x=x, cond=cond, null=null, cond_scale=float(cond_scale), coef=coef)


# ---------------------------------------------------------------------------------------------------------------------------------
# case tables: (id, shape..., the branch the case is there for).  branches_* restate which branches a shape reaches.
# ---------------------------------------------------------------------------------------------------------------------------------
def passes(threads):
    return "second_pass" if threads > GRID_CAP and threads % GRID_CAP else "one_pass"


# (id, B, C, L, KT, width, ld, branch)
NCL = [
    ("plain", 2, 72, 200, 1, 80, 80, "plain"),
    ("stem", 3, 6, 40, 15, 96, 96, "straddle"),            # the model's x stem: 8-wide chunks straddle taps; padding columns 90..95
    ("short", 2, 6, 5, 15, 96, 104, "L<KT/2"),             # every tap but the middle ones falls off one end; ld > width
    ("l1", 2, 8, 1, 3, 24, 24, "L=1"),
    ("even_kt", 2, 5, 33, 2, 16, 16, "even_KT"),
    ("c1", 1, 1, 7, 1, 8, 8, "C=1"),
    ("above_cap", 2, 5, 262200, 1, 8, 8, "second_pass"),   # B L (width / 8) = 524 400 threads
]
NCL_BRANCHES = {"plain", "straddle", "L<KT/2", "L=1", "even_KT", "C=1", "second_pass", "padding", "ld>width"}


def branches_ncl(B, C, L, KT, width, ld):
    out = {passes(B * L * (width // 8))}
    if KT == 1 and C > 1 and L > 1:
        out.add("plain")
    if any((c // C) != ((c + 7) // C) and (c + 7) // C < KT for c in range(0, width, 8)) and KT > 1:
        out.add("straddle")
    if L < KT // 2:
        out.add("L<KT/2")
    if L == 1:
        out.add("L=1")
    if KT % 2 == 0:
        out.add("even_KT")
    if C == 1:
        out.add("C=1")
    if width > C * KT:
        out.add("padding")
    if ld > width:
        out.add("ld>width")
    return out


# (id, B, C, L, ld, branch)
R2N = [
    ("ld_c", 2, 72, 50, 72, "ld=C"),
    ("ld_c3", 2, 14, 21, 17, "ld=C+3"),                    # an odd ld: rows start at 2-byte boundaries, scalar loads in bf16
    ("c1", 3, 1, 9, 1, "C=1"),
    ("l1", 3, 5, 1, 8, "L=1"),
    ("above_cap", 2, 9, 29130, 9, "second_pass"),          # B C L = 524 340 threads
]
R2N_BRANCHES = {"ld=C", "ld=C+3", "C=1", "L=1", "second_pass"}


def branches_r2n(B, C, L, ld):
    out = {passes(B * C * L), "ld=C" if ld == C else f"ld=C+{ld - C}"}
    if C == 1:
        out.add("C=1")
    if L == 1:
        out.add("L=1")
    return out


DT_PAIRS = [("f32", "f32"), ("f32", "bf16"), ("bf16", "f32"), ("bf16", "bf16")]
# (id, M, cols, lds, ldd, branch)
COPY = [
    ("strides", 5, 24, 40, 32, "lds!=ldd"),
    ("cols8", 3, 8, 8, 8, "cols=8"),
    ("m1", 1, 16, 16, 24, "M=1"),
    ("above_cap", 4104, 1032, 1032, 1032, "second_pass"),  # M (cols / 8) = 529 416 threads
]
COPY_BRANCHES = {"lds!=ldd", "cols=8", "M=1", "second_pass"}


def branches_copy(M, cols, lds, ldd):
    out = {passes(M * (cols // 8))}
    if lds != ldd and lds > cols and ldd > cols:
        out.add("lds!=ldd")
    if cols == 8:
        out.add("cols=8")
    if M == 1:
        out.add("M=1")
    return out


# (id, M, cols, lda, ldb, ldd, branch)
ADD = [
    ("three_lds", 5, 24, 32, 40, 48, "three_lds"),
    ("m1_cols8", 1, 8, 8, 16, 24, "M=1"),
    ("dense", 33, 40, 40, 40, 40, "dense"),
]
ADD_BRANCHES = {"three_lds", "M=1", "dense"}

# (id, B, Dch, L, branch)
MSE = [
    ("b3_l50", 3, 6, 50, "one_block"),
    ("b4_l1", 4, 1, 1, "L=1"),
    ("b2_l257", 2, 6, 257, "several_blocks"),
    ("above_cap", 4, 6, 22000, "second_pass"),             # 528 000 threads
]
MSE_BRANCHES = {"one_block", "L=1", "several_blocks", "second_pass"}
MSE_OPTS = [(has_len, has_wt, has_grad) for has_len in (False, True) for has_wt in (False, True) for has_grad in (False, True)]


def branches_mse(B, Dch, L):
    n = B * Dch * L
    out = {passes(n), "one_block" if n <= 1024 and L > 1 else "several_blocks" if n > 1024 else "tiny"}
    if L == 1:
        out.add("L=1")
    return out


# sqnorm and adamw: n; 1..3 are the tail alone, 4 the body alone, 5 and 1027 both, the last one two trips of the body and a tail
FLAT_N = [1, 2, 3, 4, 5, 1027, 2097152 + 1203]
FLAT_BRANCHES = {"tail_only", "body_only", "body+tail", "second_pass"}


def branches_flat(n):
    out = {"tail_only" if n < 4 else "body_only" if n % 4 == 0 else "body+tail"}
    if passes(n // 4) == "second_pass":
        out.add("second_pass")
    return out


ADAMW_STEPS = [1, 2, 1000, 100000]
ADAMW_GSCALE = [None, 0.25, 1.0, 0.0]
ADAMW_WD = [0.0, f32v(1e-2)]

# (sumsq, max_norm, base, branch)
CLIP = [
    (4.0, 0.0, 0.5, "off"),                                # max_norm = 0: base
    (4.0, -1.0, 0.25, "off"),
    (0.25, 1.0, 0.5, "below"),                             # norm 0.5 < 1
    (0.0, 1.0, 0.125, "zero"),
    (123.456, 1.0, 0.5, "active"),
    (1e6, 0.5, 1.0 / 8, "active"),
    (3.0, 1.0, 1.0, "active"),
    (1.0000001, 1.0, 1.0, "active"),                       # just above the threshold
]
CLIP_BRANCHES = {"off", "below", "zero", "active"}
CLIP_TOL = 4 * 2.0 ** -24                                  # the cast of the square root, the add, the divide, the multiply

PER_SAMPLE = [1, 257, 600]
GUIDE = [(False, 1.0), (True, 1.0), (True, 2.0), (True, 7.0)]
SPANS = [("inactive", 0.8), ("saturating", 3.0)]
STEP_B = 4
STEP_BIG = 131100                                          # B * per_sample = 524 400 threads
# (id, per_sample, has_null, cond_scale, span name, span)
DDIM = [(f"p{per}_n{int(hn)}_s{cs:g}_{sn}", per, hn, cs, sn, sp) for per in PER_SAMPLE for hn, cs in GUIDE for sn, sp in SPANS]
DDIM.append((f"p{STEP_BIG}_n1_s2_saturating", STEP_BIG, True, 2.0, "saturating", 3.0))
AXPBY = PER_SAMPLE + [STEP_BIG]

# caps of section C.  Each is what the suite already asks of the quantity; tests/test_elementwise_reference_cpu.py asserts that the fp32
# evaluation alone keeps every one of them, case by case.
SUM_CAP = 1e-6                                             # mse and sqnorm sums, relative (scheduler_and_loss in the poisoned-memory suite)
MOMENT_CAP = 2e-6                                          # adamw m', v', relmax
UPDATE_CAP = 2e-6                                          # adamw p' - p, relative to max|update|, beside p's own spacing
STEP_CAP = 2e-6                                            # axpby_rows, ddim_step, relmax (test_scheduler_and_optimizer_kernels: atol 2e-6 at order one)


def rel1(got, ref):
    """|got - ref| / |ref| of two scalars."""
    got, ref = float(got), float(ref)
    return abs(got - ref) / max(abs(ref), 1e-300)


def update_metric(p):
    """metric(p', p'_ref) for bound_check: the worst excess of |(p' - p) - (p'_ref - p)| over 2^-23 |p| (p's own spacing: the rounding of
    p' and of the decay factor), relative to max|p'_ref - p|."""
    p64 = p.double()

    def metric(got, ref):
        dg, dr = got.double().cpu() - p64, ref.double() - p64
        return (((dg - dr).abs() - 2.0 ** -23 * p64.abs()).clamp_min(0).max() / dr.abs().max().clamp_min(1e-300)).item()
    return metric


# ---------------------------------------------------------------------------------------------------------------------------------
# contract: (entry point, what is wrong, {argument: value}) over the good call of that entry point (tests/test_elementwise_rows_gpu.py:
# GOOD).  A pointer argument takes "null" or "off4" (the good pointer plus 4 bytes); every line must return `status` and write nothing.
# ---------------------------------------------------------------------------------------------------------------------------------
EW_BAD = [
    ("osuf_ncl_to_rows", "width % 8", dict(width=92, ld=96)),
    ("osuf_ncl_to_rows", "width < C*KT", dict(width=88)),
    ("osuf_ncl_to_rows", "width > ld", dict(ld=88)),
    ("osuf_ncl_to_rows", "ld % 8", dict(ld=100)),
    ("osuf_ncl_to_rows", "n <= 0", dict(B=0)),
    ("osuf_ncl_to_rows", "n <= 0", dict(L=0)),
    ("osuf_ncl_to_rows", "n <= 0", dict(KT=0)),
    ("osuf_ncl_to_rows", "n <= 0", dict(C=-6)),
    ("osuf_ncl_to_rows", "al16", dict(out="off4")),
    ("osuf_ncl_to_rows", "null", dict(inp="null")),
    ("osuf_ncl_to_rows", "null", dict(out="null")),
    ("osuf_ncl_to_rows", "dtype", dict(dtype=7)),
    ("osuf_rows_to_ncl", "ld < C", dict(ld=5)),
    ("osuf_rows_to_ncl", "n <= 0", dict(B=0)),
    ("osuf_rows_to_ncl", "n <= 0", dict(C=0)),
    ("osuf_rows_to_ncl", "n <= 0", dict(L=-1)),
    ("osuf_rows_to_ncl", "null", dict(inp="null")),
    ("osuf_rows_to_ncl", "null", dict(out="null")),
    ("osuf_rows_to_ncl", "dtype", dict(dtype=7)),
    ("osuf_copy2d", "cols % 8", dict(cols=12)),
    ("osuf_copy2d", "ld % 8", dict(lds=28)),
    ("osuf_copy2d", "ld % 8", dict(ldd=36)),
    ("osuf_copy2d", "n <= 0", dict(M=0)),
    ("osuf_copy2d", "n <= 0", dict(cols=0)),
    ("osuf_copy2d", "al16", dict(src="off4")),
    ("osuf_copy2d", "al16", dict(dst="off4")),
    ("osuf_copy2d", "null", dict(src="null")),
    ("osuf_copy2d", "null", dict(dst="null")),
    ("osuf_copy2d", "dtype", dict(sdt=7)),
    ("osuf_copy2d", "dtype", dict(ddt=2)),
    ("osuf_add2d", "cols % 8", dict(cols=12)),
    ("osuf_add2d", "ld % 8", dict(lda=28)),
    ("osuf_add2d", "ld % 8", dict(ldb=36)),
    ("osuf_add2d", "ld % 8", dict(ldd=44)),
    ("osuf_add2d", "n <= 0", dict(M=0)),
    ("osuf_add2d", "n <= 0", dict(cols=-8)),
    ("osuf_add2d", "al16", dict(a="off4")),
    ("osuf_add2d", "al16", dict(b="off4")),
    ("osuf_add2d", "al16", dict(dst="off4")),
    ("osuf_add2d", "null", dict(a="null")),
    ("osuf_add2d", "null", dict(b="null")),
    ("osuf_add2d", "null", dict(dst="null")),
    ("osuf_add2d", "dtype", dict(dtype=7)),
    ("osuf_mse", "n <= 0", dict(B=0)),
    ("osuf_mse", "n <= 0", dict(Dch=0)),
    ("osuf_mse", "n <= 0", dict(L=-3)),
    ("osuf_mse", "null", dict(pred="null")),
    ("osuf_mse", "null", dict(target="null")),
    ("osuf_mse", "null", dict(loss_sum="null")),
    ("osuf_mse_w", "n <= 0", dict(B=0)),
    ("osuf_mse_w", "null", dict(pred="null")),
    ("osuf_mse_w", "null", dict(target="null")),
    ("osuf_mse_w", "null", dict(loss_sum="null")),
    ("osuf_mse_w", "null", dict(w="null")),
    ("osuf_sqnorm", "n <= 0", dict(n=0)),
    ("osuf_sqnorm", "n <= 0", dict(n=-4)),
    ("osuf_sqnorm", "al16", dict(g="off4")),
    ("osuf_sqnorm", "null", dict(g="null")),
    ("osuf_sqnorm", "null", dict(out="null")),
    ("osuf_adamw", "n <= 0", dict(n=0)),
    ("osuf_adamw", "step <= 0", dict(step=0)),
    ("osuf_adamw", "step <= 0", dict(step=-1)),
    ("osuf_adamw", "al16", dict(p="off4")),
    ("osuf_adamw", "al16", dict(g="off4")),
    ("osuf_adamw", "al16", dict(m="off4")),
    ("osuf_adamw", "al16", dict(v="off4")),
    ("osuf_clip_coef", "null", dict(sumsq="null")),
    ("osuf_clip_coef", "null", dict(coef="null")),
    ("osuf_cast_f32_bf16", "n <= 0", dict(n=0)),
    ("osuf_cast_f32_bf16", "al16", dict(src="off4")),
    ("osuf_cast_f32_bf16", "al16", dict(dst="off4")),
    ("osuf_axpby_rows", "n <= 0", dict(B=0)),
    ("osuf_axpby_rows", "n <= 0", dict(per=0)),
    ("osuf_ddim_step", "n <= 0", dict(B=-1)),
    ("osuf_ddim_step", "n <= 0", dict(per=0)),
]
EW_BAD_KINDS = {"width % 8", "width < C*KT", "width > ld", "ld < C", "cols % 8", "ld % 8", "n <= 0", "step <= 0", "al16", "null", "dtype"}
# entry points whose source checks the named pointers for NULL (csrc/elementwise.hip): a "null" line may only name one of these
NULL_GUARDED = {"osuf_ncl_to_rows": {"inp", "out"}, "osuf_rows_to_ncl": {"inp", "out"}, "osuf_copy2d": {"src", "dst"},
                "osuf_add2d": {"a", "b", "dst"}, "osuf_mse": {"pred", "target", "loss_sum"}, "osuf_mse_w": {"pred", "target", "loss_sum", "w"},
                "osuf_sqnorm": {"g", "out"}, "osuf_clip_coef": {"sumsq", "coef"}}
AL16_GUARDED = {"osuf_ncl_to_rows": {"out"}, "osuf_copy2d": {"src", "dst"}, "osuf_add2d": {"a", "b", "dst"}, "osuf_sqnorm": {"g"},
                "osuf_adamw": {"p", "g", "m", "v"}, "osuf_cast_f32_bf16": {"src", "dst"}}


def bad_status(kind):
    return EUNSUPPORTED if kind == "dtype" else EINVAL
