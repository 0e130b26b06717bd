"""Plain references of the DiT row kernels (csrc/dit.hip: adaLN forward / backward, the joint QK RMS-norm forward / backward, pack / unpack,
rowpart_finish_kernel behind both backwards, stat_pool), written out by hand from the formulas in the kernels' comments and
include/osufusion_hip.h (no autograd), with the input generators, the case tables and the contract table of tests/test_dit_rows_gpu.py.
Nothing here needs a GPU; tests/test_dit_rows_reference_cpu.py checks every backward against fp64 autograd of its forward, the branch each
table entry names (from the launcher arithmetic restated below) and the caps.

Every function computes in the dtype of its tensor inputs: fp64 is the reference, fp32 the "same formula in single precision" whose
distance to the fp64 result (e32) scales the bounds of tests/bound_check.py.  The backwards take mean | rstd and the inverse norms as
inputs, as the kernels do: the GPU file hands both evaluations and the kernel the fp64 forward's values rounded to fp32.
"""
from __future__ import annotations

import functools

import torch

from tests.elementwise_reference import EINVAL, EUNSUPPORTED, GRID_CAP, _gen, f32v, round_bf16  # noqa: F401

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
LN_EPS = f32v(1e-6)                                        # what the entry point receives
NORM_EPS = 1e-12                                           # kNormEps


def stored(t, dtype):
    """fp32 values that `dtype` holds exactly."""
    return t.to(F32) if dtype == F32 else round_bf16(t.to(F32)).to(F32)


def rnd(tag, shape, scale=1.0):
    return (torch.randn(*shape, generator=_gen(tag, shape), dtype=F64) * scale).to(F32)


# ---------------------------------------------------------------------------------------------------------------------------------
# launcher arithmetic, restated from csrc/dit.hip and csrc/common.hpp
# ---------------------------------------------------------------------------------------------------------------------------------
FWD_GRID_CAP = 4096                                        # workgroups of 4 waves: one row per wave, grid-stride above 16384 rows
QKNORM_BWD_CAP = 1024
FIN_SLICES = 16                                            # rowpart_finish_kernel: slice y adds k = y, y + 16, ...


def chunk_iters(chunks):
    j = (chunks + 63) // 64
    return 1 if j <= 1 else 2 if j <= 2 else 4 if j <= 4 else 8 if j <= 8 else 0


def last_pass_lanes(chunks):
    """Live lanes of the last pass that has any."""
    return chunks - 64 * ((chunks + 63) // 64 - 1)


def fwd_blocks(M):
    return min((M + 3) // 4, FWD_GRID_CAP)


def fwd_trips(M):
    """Rows of the busiest wave of the forward kernels."""
    waves = 4 * fwd_blocks(M)
    return (M + waves - 1) // waves


def adaln_bwd_blocks(B, L):
    return min((L + 15) // 16, max(2048 // B, 1))


def adaln_bwd_trips(B, L):
    """Rows of the busiest wave of adaln_bwd_kernel: n = 4 k + wave, stepping by 4 nblk."""
    step = 4 * adaln_bwd_blocks(B, L)
    return (L + step - 1) // step


def adaln_bwd_cap_binds(B, L):
    return (L + 15) // 16 > max(2048 // B, 1)


def qknorm_bwd_blocks(M):
    return min((M + 15) // 16, QKNORM_BWD_CAP)


def ew_grid(threads):
    return max(min((threads + 255) // 256, GRID_CAP // 256), 1)


def finish_kind(nblk):
    """How rowpart_finish_kernel's 16 slices are filled."""
    if nblk < FIN_SLICES:
        return "nblk<16"
    return f"nblk={nblk}" if nblk == QKNORM_BWD_CAP else "nblk%16!=0" if nblk % FIN_SLICES else "nblk%16==0"


def adaln_branches(B, L, C, strides=None, dirs="both"):
    ch = C // 8
    out = {f"J={chunk_iters(ch)}", "last_pass=full" if last_pass_lanes(ch) == 64 else f"last_pass={last_pass_lanes(ch)}"}
    if dirs != "bwd" and (B * L + 3) // 4 > FWD_GRID_CAP:
        out.add("fwd_grid_cap")
    if dirs != "fwd":
        out.add("finish:" + finish_kind(adaln_bwd_blocks(B, L)))
        if adaln_bwd_cap_binds(B, L):
            out.add("bwd_cap")
        if adaln_bwd_trips(B, L) > 1:
            out.add(f"bwd_trips={adaln_bwd_trips(B, L)}")
        if B == 65535:
            out.add("grid.y=65535")
    if strides:
        out.add("strided")
        if strides["off2"] < 0:
            out.add("off2<0")
    return out


def joint_branches(B, Ns, Nj, off, H, G, D, strided=False, dirs="both"):
    ch, M = (H + 2 * G) * D // 8, B * Ns
    identity = Ns == Nj and off == 0 and G == H
    out = {f"J={chunk_iters(ch)}", "identity" if identity else "joint", "last_pass=full" if last_pass_lanes(ch) == 64 else f"last_pass={last_pass_lanes(ch)}"}
    if (H + 2 * G) * D == 4096:
        out.add("width=4096")
    if dirs != "bwd" and (M + 3) // 4 > FWD_GRID_CAP:
        out.add("fwd_grid_cap")
    if dirs != "fwd":
        out.add("finish:" + finish_kind(qknorm_bwd_blocks(M)))
        if (M + 15) // 16 > QKNORM_BWD_CAP:
            out.add("bwd_cap")
    if strided:
        out.add("strided")
    return out


def perm_branches(B, Ns, H, D):
    return {"ew_grid_cap" if (B * Ns * (H * D // 8) + 255) // 256 > GRID_CAP // 256 else "one_pass"}


# ---------------------------------------------------------------------------------------------------------------------------------
# adaLN:  out = LN(x) (1 + scale[b]) + shift[b], rows [M][C], sample of row m = m / L
# ---------------------------------------------------------------------------------------------------------------------------------
def adaln_fwd(x, shift, scale, L, eps=LN_EPS):
    """x (M, C), shift / scale (B, C) in the dtype of x -> (out (M, C), mean (M), rstd (M))."""
    M, C = x.shape
    b = torch.arange(M) // L
    mean = x.sum(-1, keepdim=True) / C
    d = x - mean
    var = (d * d).sum(-1, keepdim=True) / C
    rstd = 1 / torch.sqrt(var + eps)
    return d * rstd * (1 + scale[b]) + shift[b], mean[:, 0], rstd[:, 0]


def adaln_bwd(dy, x, mean, rstd, scale, L, dres=None):
    """-> (dx (M, C), dshift (B, C), dscale (B, C)):  g = dy (1 + scale[b]);  dx = rstd (g - mean_c g - xhat mean_c(g xhat)) (+ dres);
    dshift[b] = sum_n dy, dscale[b] = sum_n dy xhat."""
    M, C = x.shape
    B = M // L
    b = torch.arange(M) // L
    xh = (x - mean[:, None]) * rstd[:, None]
    g = dy * (1 + scale[b])
    s1 = g.sum(-1, keepdim=True) / C
    s2 = (g * xh).sum(-1, keepdim=True) / C
    dx = rstd[:, None] * (g - s1 - xh * s2)
    if dres is not None:
        dx = dx + dres
    return dx, dy.view(B, L, C).sum(1), (dy * xh).view(B, L, C).sum(1)


# ---------------------------------------------------------------------------------------------------------------------------------
# joint QK-norm: a stream's raw rows [M][(H + 2G) D] = [q (h d) | k (g d) | v (g d)] -> its rows of the joint buffer
# ---------------------------------------------------------------------------------------------------------------------------------
def joint_rows(B, Ns, Nj, off):
    """The joint row of the stream's row m = b Ns + n: b Nj + off + n."""
    m = torch.arange(B * Ns)
    return (m // Ns) * Nj + off + m % Ns


def joint_cols(H, G, D, heads):
    """Column in the joint row of each of the first `heads` D natural columns: natural query head j goes to block (j % G) (H / G) + j / G;
    the k and v heads keep their place."""
    c = torch.arange(heads * D)
    head, e = c // D, c % D
    blk = torch.where(head < H, (head % G) * (H // G) + head // G, head)
    return blk * D + e


def pack(rows, H, G, D):
    """rows (M, H D), natural head order -> the values of their joint rows (M, H D), group-major."""
    out = torch.empty_like(rows)
    out[:, joint_cols(H, G, D, H)] = rows
    return out


def unpack(joint, H, G, D):
    return joint[:, joint_cols(H, G, D, H)]


def _gammas(gq, gk, H, G, D):
    return torch.cat([gq.reshape(H, D), gk.reshape(G, D)], 0)                          # (H + G, D): q heads, then k heads


def qknorm_fwd(x, gq, gk, H, G, D):
    """x (M, (H + 2G) D) -> (the stream's joint rows (M, W), inv (M, H + G) or None).  y = x / max(||x||, 1e-12) gamma sqrt(D) per q / k
    head, v unchanged; gq None: no norm."""
    M = x.shape[0]
    W, QK = (H + 2 * G) * D, (H + G) * D
    y, inv = x.clone(), None
    if gq is not None:
        h = x[:, :QK].reshape(M, H + G, D)
        n = (h * h).sum(-1).sqrt()
        inv = 1 / n.clamp_min(NORM_EPS)
        sD = torch.tensor(float(D), dtype=x.dtype).sqrt()
        y[:, :QK] = (h * inv[..., None] * _gammas(gq, gk, H, G, D) * sD).reshape(M, QK)
    out = torch.empty_like(y)
    out[:, joint_cols(H, G, D, H + 2 * G)] = y
    assert out.shape == (M, W)
    return out, inv


def qknorm_bwd(g, x, inv, gq, gk, H, G, D):
    """g (M, W): the stream's joint rows of dq|dk|dv -> (dx (M, W) natural order, dgamma (H + G, D) or None).  Per q / k head, with
    u = x inv, gu = g gamma sqrt(D):  n >= 1e-12: dx = (gu - u (u . gu)) inv;  n < 1e-12 (the clamp holds the norm constant): dx = gu inv.
    dgamma = sum_m g u sqrt(D).  gq None: the permutation alone."""
    M = g.shape[0]
    QK = (H + G) * D
    gn = g[:, joint_cols(H, G, D, H + 2 * G)]                                          # natural order
    if gq is None:
        return gn, None
    sD = torch.tensor(float(D), dtype=g.dtype).sqrt()
    h = x[:, :QK].reshape(M, H + G, D)
    gh = gn[:, :QK].reshape(M, H + G, D)
    clamped = (h * h).sum(-1).sqrt() < NORM_EPS
    u = h * inv[..., None]
    dgamma = (gh * u * sD).sum(0)
    gu = gh * _gammas(gq, gk, H, G, D) * sD
    d = torch.where(clamped, torch.zeros((), dtype=g.dtype), (u * gu).sum(-1))
    dx = gn.clone()
    dx[:, :QK] = ((gu - u * d[..., None]) * inv[..., None]).reshape(M, QK)
    return dx, dgamma


# ---------------------------------------------------------------------------------------------------------------------------------
# stat_pool: a (B, C, L) -> (B, 2C) = [mean_l | unbiased std_l], two passes
# ---------------------------------------------------------------------------------------------------------------------------------
def stat_pool(a):
    L = a.shape[-1]
    mean = a.sum(-1) / L
    d = a - mean[..., None]
    return torch.cat([mean, ((d * d).sum(-1) / (L - 1)).sqrt()], 1)


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------
ADALN_KINDS = ("a", "b", "c", "d")                         # c: fp32 only (1 +- 2^-10 needs 11 significand bits)
OFFSET = {"c": 1.0, "d": 3.0}


def adaln_x(kind, cid, M, C, dtype):
    """a: 2 randn + 0.5 (var ~ 4: eps invisible);  b: half the cells +2^-10, half -2^-10 in a per-row random order: mean exactly 0,
    var = 2^-20 ~ eps = 1e-6, exact in bf16 and fp32, every partial sum exact;  c: the rows of b plus 1.0 (fp32 only; sums still exact);
    d: the constant 3.0 (out = shift)."""
    if kind == "a":
        return stored(rnd(f"ad.x.{cid}", (M, C)) * 2 + 0.5, dtype)
    if kind == "d":
        return torch.full((M, C), OFFSET["d"], dtype=F32)
    order = torch.rand(M, C, generator=_gen(f"ad.o.{cid}", (M, C))).argsort(-1)
    x = torch.where(order < C // 2, 2.0 ** -10, -(2.0 ** -10)).to(F32)
    return x + OFFSET["c"] if kind == "c" else x


@functools.lru_cache(maxsize=None)
def adaln_inputs(cid, B, L, C, dt, kind="a"):
    """fp32 tensors of values the storage dtype holds: x, dy, dres (M, C); shift, scale (B, C) fp32."""
    dtype = F32 if dt == "f32" else BF16
    M = B * L
    return dict(x=adaln_x(kind, cid, M, C, dtype), shift=rnd(f"ad.sh.{cid}", (B, C), 0.3), scale=rnd(f"ad.sc.{cid}", (B, C), 0.3),
                dy=stored(rnd(f"ad.dy.{cid}", (M, C)), dtype), dres=stored(rnd(f"ad.dr.{cid}", (M, C)), dtype))


def adaln_extra(kind, scale, ref_out, eps=LN_EPS):
    """Kinds c and d: the kernel forms the mean as sum * (1 / C); when C is no power of two the rounded reciprocal costs the mean up to
    2^-23 |offset| (the row sums themselves are exact), and out = (x - mean) rstd (1 + scale) + shift carries that times
    rstd (1 + max|scale|), rstd <= 1 / sqrt(eps).  Relative to max|ref|, as relmax is."""
    if kind not in OFFSET:
        return 0.0
    var = 2.0 ** -20 if kind == "c" else 0.0
    rstd = 1 / (var + eps) ** 0.5
    return 2.0 ** -23 * OFFSET[kind] * rstd * (1 + scale.abs().max().item()) / ref_out.abs().max().item()


SPECIAL_KINDS = {"zero": 0.0, "tiny": 2.0 ** -50, "near": 2.0 ** -39}                 # norm 0; below 1e-12 but u != 0; just above the clamp


def specials(Ns, H, G):
    """(b, n, head in 0 .. H + G - 1, kind): a q head and a k head of each kind, in rows of their own."""
    hq, hk = min(1, H - 1), H + G - 1
    rows = [(0, 1 % Ns), (1, 2 % Ns), (0, 3 % Ns), (1, 4 % Ns), (0, 5 % Ns), (1, 6 % Ns)]
    kinds = ("zero", "zero", "tiny", "tiny", "near", "near")
    return [(b, n, hq if i % 2 == 0 else hk, kinds[i]) for i, (b, n) in enumerate(rows)]


def special_mask(B, Ns, H, G, D, sp):
    """kind -> boolean (M, W) mask of the cells of the heads of that kind."""
    W = (H + 2 * G) * D
    out = {k: torch.zeros(B * Ns, W, dtype=torch.bool) for k in SPECIAL_KINDS}
    for b, n, head, kind in sp:
        out[kind][b * Ns + n, head * D:(head + 1) * D] = True
    return out


@functools.lru_cache(maxsize=None)
def joint_inputs(cid, B, Ns, Nj, H, G, D, dt, with_specials):
    """fp32 tensors: x (M, W) of values the storage dtype holds, g (B Nj, W) fp32 joint gradient rows, gq (H, D), gk (G, D)."""
    dtype = F32 if dt == "f32" else BF16
    W, M = (H + 2 * G) * D, B * Ns
    x = stored(rnd(f"qk.x.{cid}", (M, W)), dtype)
    sp = specials(Ns, H, G) if with_specials else []
    for b, n, head, kind in sp:
        x[b * Ns + n, head * D:(head + 1) * D] = SPECIAL_KINDS[kind]
    return dict(x=x, g=rnd(f"qk.g.{cid}", (B * Nj, W)), gq=1 + 0.2 * rnd(f"qk.gq.{cid}", (H, D)), gk=1 + 0.2 * rnd(f"qk.gk.{cid}", (G, D)), specials=sp)


def stat_input(kind, B, C, L):
    """plain: 5 randn - 10 (what tests/test_dit_gpu.py uses);  offset: 1000 + 0.01 randn: a one-pass variance loses every digit here."""
    r = rnd(f"sp.{kind}", (B, C, L))
    return r * 5 - 10 if kind == "plain" else 1000 + 0.01 * r


# ---------------------------------------------------------------------------------------------------------------------------------
# case tables.  The branch(es) a case exists for are named last; *_branches() derive what a shape reaches from the launcher arithmetic.
# ---------------------------------------------------------------------------------------------------------------------------------
def _strides(C, B_cols=0):
    """Five different row strides above C (multiples of 8), a modulation stride and a gradient stride of their own."""
    return dict(ldx=C + 8, ldo=C + 16, lddy=C + 24, ldr=C + 32, lddx=C + 40, ldm=3 * C + 12, ldd=2 * C + 20, off2=C + 12)


# (id, B, L, C, strides or None, which launches: "fwd" | "bwd" | "both", branches named)
ADALN = [(f"C{C}_L{L}", 2, L, C, None, "both", ()) for C in (8, 504, 512, 520, 1024, 1032, 2048) for L in (1, 5, 67)]
ADALN += [
    ("L300", 2, 300, 520, None, "both", ("finish:nblk%16!=0",)),                       # 19 workgroups per sample: slices 0..2 add two terms
    ("fwd_stride", 4, 4100, 8, None, "fwd", ("fwd_grid_cap",)),                        # M = 16400 rows over 16384 waves
    ("bwd_cap", 256, 200, 8, None, "bwd", ("bwd_cap", "bwd_trips=7")),                 # 8 workgroups per sample, rows n, n + 32, ...
    ("grid_y", 65535, 1, 8, None, "bwd", ("grid.y=65535",)),
    ("strided_520", 2, 67, 520, _strides(520), "both", ("strided", "J=2")),
    ("strided_1032", 3, 5, 1032, _strides(1032), "both", ("strided", "J=4")),
    ("off2_neg", 2, 5, 520, dict(_strides(520), off2=-(520 + 4)), "bwd", ("off2<0",)),   # the dscale block 524 cells before dshift
]
ADALN_NAMED = {"J=1", "J=2", "J=4", "last_pass=full", "last_pass=1", "last_pass=63", "fwd_grid_cap", "bwd_cap", "bwd_trips=7", "grid.y=65535",
               "strided", "off2<0", "finish:nblk<16", "finish:nblk%16!=0"}

# (id, B, Ns, Nj, off, H, G, D, strided, with special heads, which launches, branches named).  Two streams (Na, Nx) = (5, 12): _a and _x.
# j2's 64 query chunks fill pass 0 exactly; j2c has 96, so that a permuted query chunk lands in another 64-chunk pass than its source.
_SHAPES = [("j1", 6, 2, 16, ("J=1",)), ("j2", 8, 4, 64, ("J=2",)), ("j2c", 12, 2, 64, ("J=2", "last_pass=full")), ("j4", 8, 2, 128, ("J=4",)), ("j8p", 16, 4, 128, ("J=8",)),
           ("j8f", 16, 8, 128, ("J=8", "width=4096", "last_pass=full"))]
JOINT = [(f"{n}_{s}", 2, Ns, 17, off, H, G, D, False, s == "x", "both", br + ("joint",))
         for n, H, G, D, br in _SHAPES for s, Ns, off in (("a", 5, 0), ("x", 12, 5))]
JOINT += [
    ("id_j2", 2, 12, 12, 0, 4, 4, 64, False, True, "both", ("identity", "J=2")),
    ("id_j8", 2, 12, 12, 0, 85, 85, 16, False, True, "both", ("identity", "J=8")),     # 4080 wide: 3 H D = 4096 has no solution with G = H
    ("big", 4, 4100, 4101, 1, 1, 1, 16, False, False, "both", ("fwd_grid_cap", "bwd_cap", "finish:nblk=1024")),
    ("strided_j2", 2, 12, 17, 5, 8, 4, 64, True, True, "both", ("strided", "J=2")),
    ("strided_j1", 3, 5, 9, 2, 6, 2, 16, True, False, "both", ("strided", "J=1")),
]
JOINT_NAMED = {"J=1", "J=2", "J=4", "J=8", "joint", "identity", "width=4096", "last_pass=full", "fwd_grid_cap", "bwd_cap", "strided",
               "finish:nblk<16", "finish:nblk=1024"}


def joint_strides(W, strided):
    return dict(ldx=W + 8, ldy=W + 16, ldg=W + 24, lddx=W + 40) if strided else dict(ldx=W, ldy=W, ldg=W, lddx=W)


# (id, B, Ns, Nj, off, H, G, D, lds, ldj, branch)
PERM = [
    ("h6g2", 2, 12, 17, 5, 6, 2, 16, 96, 96, "one_pass"),
    ("h8g4", 2, 5, 17, 0, 8, 4, 64, 512 + 8, 512 + 24, "one_pass"),                  # both strides above the width
    ("h16g8", 2, 12, 17, 5, 16, 8, 128, 2048, 2048, "one_pass"),
    ("big", 4, 4100, 4101, 1, 2, 1, 128, 256, 256, "ew_grid_cap"),                    # 16400 x 32 = 524 800 chunks
]

STAT_L = [2, 255, 256, 257, 1000]
STAT_C = [1, 96]
STAT_B = 3
STAT_KINDS = ["plain", "offset"]

# caps: what tests/test_dit_gpu.py and tests/test_mmdit_gpu.py already ask of the same quantity
OUT_CAP = 2e-6                                             # adaLN out (and mean | rstd, the same arithmetic)
Y_CAP = 1e-5                                               # the fp32 term of the normed joint rows: x inv gamma sqrt(D), held to what inv is
GRAD_CAP = 1e-5                                            # dx, dshift | dscale, dgamma
INV_CAP = 1e-5
STAT_CAP = 1e-5

# ---------------------------------------------------------------------------------------------------------------------------------
# contract: (entry point, what is wrong, {argument: value}) over the good call of that entry point (tests/test_dit_rows_gpu.py:
# good_calls).  A pointer argument takes "null" or "off4" (the good pointer plus 4 bytes).  Every line is stopped by the host-side check
# with `status` (the workspace functions: 0 bytes) before any launch, and nothing is written.
# ---------------------------------------------------------------------------------------------------------------------------------
_JOINT_SHAPE_BAD = [("n <= 0", dict(M=0)), ("n <= 0", dict(Ns=0)), ("n <= 0", dict(Nj=0)), ("off", dict(off=-1)), ("off", dict(off=6)),
                    ("M % Ns", dict(M=11)), ("n <= 0", dict(H=0)), ("n <= 0", dict(G=0)), ("H % G", dict(G=4)), ("D", dict(D=24)),
                    ("width > 4096", dict(H=32, G=16, D=128))]
DIT_BAD = [
    ("osuf_adaln_fwd", "C", dict(C=0)), ("osuf_adaln_fwd", "C", dict(C=60)), ("osuf_adaln_fwd", "C", dict(C=2056)),
    ("osuf_adaln_fwd", "n <= 0", dict(M=0)), ("osuf_adaln_fwd", "n <= 0", dict(L=0)), ("osuf_adaln_fwd", "M % L", dict(L=4)),
    ("osuf_adaln_fwd", "ld % 8", dict(ldx=76)), ("osuf_adaln_fwd", "ld % 8", dict(ldo=76)), ("osuf_adaln_fwd", "ld % 4", dict(ldm=66)),
    ("osuf_adaln_fwd", "ld < C", dict(ldx=56)), ("osuf_adaln_fwd", "ld < C", dict(ldo=56)), ("osuf_adaln_fwd", "ld < C", dict(ldm=60)),
    ("osuf_adaln_fwd", "al16", dict(x="off4")), ("osuf_adaln_fwd", "al16", dict(out="off4")), ("osuf_adaln_fwd", "al16", dict(shift="off4")),
    ("osuf_adaln_fwd", "al16", dict(scale="off4")),
    ("osuf_adaln_fwd", "null", dict(x="null")), ("osuf_adaln_fwd", "null", dict(out="null")), ("osuf_adaln_fwd", "null", dict(shift="null")),
    ("osuf_adaln_fwd", "null", dict(scale="null")), ("osuf_adaln_fwd", "dtype", dict(dtype=7)),
    ("osuf_adaln_bwd_workspace_bytes", "C", dict(C=60)), ("osuf_adaln_bwd_workspace_bytes", "C", dict(C=2056)),
    ("osuf_adaln_bwd_workspace_bytes", "n <= 0", dict(M=0)), ("osuf_adaln_bwd_workspace_bytes", "n <= 0", dict(L=0)),
    ("osuf_adaln_bwd_workspace_bytes", "M % L", dict(L=4)), ("osuf_adaln_bwd_workspace_bytes", "B > 65535", dict(M=65536, L=1)),
    ("osuf_adaln_bwd", "C", dict(C=60)), ("osuf_adaln_bwd", "C", dict(C=2056)), ("osuf_adaln_bwd", "n <= 0", dict(M=0)),
    ("osuf_adaln_bwd", "n <= 0", dict(L=-5)), ("osuf_adaln_bwd", "M % L", dict(L=4)), ("osuf_adaln_bwd", "B > 65535", dict(M=65536, L=1)),
    ("osuf_adaln_bwd", "ld % 8", dict(lddy=76)), ("osuf_adaln_bwd", "ld % 8", dict(ldx=76)), ("osuf_adaln_bwd", "ld % 8", dict(lddx=76)),
    ("osuf_adaln_bwd", "ld % 8", dict(ldr=76)), ("osuf_adaln_bwd", "ld % 4", dict(ldm=66)),
    ("osuf_adaln_bwd", "ld < C", dict(lddy=56)), ("osuf_adaln_bwd", "ld < C", dict(ldx=56)), ("osuf_adaln_bwd", "ld < C", dict(ldr=56)),
    ("osuf_adaln_bwd", "ld < C", dict(lddx=56)), ("osuf_adaln_bwd", "ld < C", dict(ldm=60)), ("osuf_adaln_bwd", "ld < C", dict(ldd=63)),
    ("osuf_adaln_bwd", "null", dict(dy="null")), ("osuf_adaln_bwd", "null", dict(x="null")), ("osuf_adaln_bwd", "null", dict(dx="null")),
    ("osuf_adaln_bwd", "null", dict(scale="null")), ("osuf_adaln_bwd", "null", dict(mr="null")), ("osuf_adaln_bwd", "null", dict(dmod="null")),
    ("osuf_adaln_bwd", "null", dict(workspace="null")),
    ("osuf_adaln_bwd", "al16", dict(dy="off4")), ("osuf_adaln_bwd", "al16", dict(x="off4")), ("osuf_adaln_bwd", "al16", dict(dres="off4")),
    ("osuf_adaln_bwd", "al16", dict(dx="off4")), ("osuf_adaln_bwd", "al16", dict(scale="off4")),
    ("osuf_adaln_bwd", "workspace", dict(workspace_bytes=2 * 2 * 64 * 4 - 1)), ("osuf_adaln_bwd", "dtype", dict(dtype=7)),
    ("osuf_stat_pool", "null", dict(a="null")), ("osuf_stat_pool", "null", dict(out="null")), ("osuf_stat_pool", "n <= 0", dict(B=0)),
    ("osuf_stat_pool", "n <= 0", dict(C=0)), ("osuf_stat_pool", "n <= 0", dict(L=0)), ("osuf_stat_pool", "B > 65535", dict(B=65536)),
]
DIT_BAD += [("osuf_joint_qknorm_fwd", k, o) for k, o in _JOINT_SHAPE_BAD] + [
    ("osuf_joint_qknorm_fwd", "ld % 8", dict(ldx=196)), ("osuf_joint_qknorm_fwd", "ld % 8", dict(ldy=196)),
    ("osuf_joint_qknorm_fwd", "ld < W", dict(ldx=152)), ("osuf_joint_qknorm_fwd", "ld < W", dict(ldy=152)),
    ("osuf_joint_qknorm_fwd", "al16", dict(x="off4")), ("osuf_joint_qknorm_fwd", "al16", dict(y="off4")),
    ("osuf_joint_qknorm_fwd", "al16", dict(gamma_q="off4")), ("osuf_joint_qknorm_fwd", "al16", dict(gamma_k="off4")),
    ("osuf_joint_qknorm_fwd", "null", dict(x="null")), ("osuf_joint_qknorm_fwd", "null", dict(y="null")),
    ("osuf_joint_qknorm_fwd", "one gamma", dict(gamma_q="null")), ("osuf_joint_qknorm_fwd", "one gamma", dict(gamma_k="null")),
    ("osuf_joint_qknorm_fwd", "null", dict(inv="null")), ("osuf_joint_qknorm_fwd", "dtype", dict(dtype=7)),
]
for _e in ("osuf_joint_pack", "osuf_joint_unpack"):
    DIT_BAD += [(_e, k, o) for k, o in _JOINT_SHAPE_BAD] + [
        (_e, "ld % 8", dict(lds=100)), (_e, "ld % 8", dict(ldj=100)), (_e, "ld < W", dict(lds=88)), (_e, "ld < W", dict(ldj=88)),
        (_e, "al16", dict(s="off4")), (_e, "al16", dict(joint="off4")), (_e, "null", dict(s="null")), (_e, "null", dict(joint="null")),
        (_e, "dtype", dict(dtype=7))]
DIT_BAD += [("osuf_joint_qknorm_bwd_workspace_bytes", k, o) for k, o in _JOINT_SHAPE_BAD if not set(o) & {"Ns", "Nj", "off"} and o != dict(M=11)]
DIT_BAD += [("osuf_joint_qknorm_bwd", k, o) for k, o in _JOINT_SHAPE_BAD] + [
    ("osuf_joint_qknorm_bwd", "ld % 4", dict(ldg=194)), ("osuf_joint_qknorm_bwd", "ld % 8", dict(ldx=196)), ("osuf_joint_qknorm_bwd", "ld % 8", dict(lddx=196)),
    ("osuf_joint_qknorm_bwd", "ld < W", dict(ldg=156)), ("osuf_joint_qknorm_bwd", "ld < W", dict(ldx=152)), ("osuf_joint_qknorm_bwd", "ld < W", dict(lddx=152)),
    ("osuf_joint_qknorm_bwd", "null", dict(g="null")), ("osuf_joint_qknorm_bwd", "null", dict(dx="null")), ("osuf_joint_qknorm_bwd", "null", dict(x="null")),
    ("osuf_joint_qknorm_bwd", "null", dict(inv="null")), ("osuf_joint_qknorm_bwd", "null", dict(dgamma="null")),
    ("osuf_joint_qknorm_bwd", "null", dict(workspace="null")),
    ("osuf_joint_qknorm_bwd", "al16", dict(g="off4")), ("osuf_joint_qknorm_bwd", "al16", dict(dx="off4")), ("osuf_joint_qknorm_bwd", "al16", dict(x="off4")),
    ("osuf_joint_qknorm_bwd", "al16", dict(gamma_q="off4")), ("osuf_joint_qknorm_bwd", "al16", dict(gamma_k="off4")),
    ("osuf_joint_qknorm_bwd", "one gamma", dict(gamma_q="null")), ("osuf_joint_qknorm_bwd", "one gamma", dict(gamma_k="null")),
    ("osuf_joint_qknorm_bwd", "workspace", dict(workspace_bytes=8 * 16 * 4 - 1)), ("osuf_joint_qknorm_bwd", "dtype", dict(dtype=7)),
]
DIT_ENTRIES = ["osuf_adaln_fwd", "osuf_adaln_bwd_workspace_bytes", "osuf_adaln_bwd", "osuf_stat_pool", "osuf_joint_qknorm_fwd", "osuf_joint_pack",
               "osuf_joint_unpack", "osuf_joint_qknorm_bwd_workspace_bytes", "osuf_joint_qknorm_bwd"]
# the good calls' shapes (tests/test_dit_rows_gpu.py builds the tensors): adaLN B = 2, L = 5, C = 64 with row strides 72 and ldm = ldd = 136;
# joint B = 2, Ns = 5, Nj = 9, off = 3, H = 6, G = 2, D = 16 (W = 160, strides 192; pack width 96, strides 104)
GOOD_ADALN = dict(B=2, L=5, C=64, ld=72, ldm=136)
GOOD_JOINT = dict(B=2, Ns=5, Nj=9, off=3, H=6, G=2, D=16, ld=192, ldp=104)
# the clauses of the checks in csrc/dit.hip, as the source spells them: tests/test_dit_rows_reference_cpu.py looks each one up
DIT_CLAUSES = [
    "bad_c(C) || M <= 0 || L <= 0 || M % L || ldx % 8 || ldo % 8 || ldm % 4 || !al16(x) || !al16(out) || !al16(shift) || !al16(scale)",
    "!x || !out || !shift || !scale || ldx < C || ldo < C || ldm < C",
    "bad_c(C) || M <= 0 || L <= 0 || M % L || M / L > 65535) return 0",
    "bad_c(C) || M <= 0 || L <= 0 || M % L || M / L > 65535 || lddy % 8 || ldx % 8 || lddx % 8 || (dres && ldr % 8) || ldm % 4 || !mr || !dmod || !workspace",
    "!al16(dy) || !al16(x) || !al16(dx) || (dres && !al16(dres)) || !al16(scale)",
    "!dy || !x || !dx || !scale || lddy < C || ldx < C || lddx < C || (dres && ldr < C) || ldm < C || ldd < C",
    "workspace_bytes < osuf_adaln_bwd_workspace_bytes(M, C, L)",
    "M <= 0 || Ns <= 0 || Nj <= 0 || off < 0 || (long)off + Ns > Nj || M % Ns || H <= 0 || G <= 0 || H % G ||",
    "!(D == 16 || D == 32 || D == 64 || D == 128) || ((long)H + 2L * G) * D > 4096",
    "ldx % 8 || ldy % 8 || ldx < (long)(H + 2 * G) * D || ldy < (long)(H + 2 * G) * D || !al16(x) || !x || !y || !al16(y)",
    "(gamma_q == nullptr) != (gamma_k == nullptr) || (gamma_q && !inv) || !al16(gamma_q) || !al16(gamma_k)",
    "lds % 8 || ldj % 8 || lds < (long)H * D || ldj < (long)H * D || !s || !joint || !al16(s) || !al16(joint)",
    "ldg % 4 || ldx % 8 || lddx % 8 || ldg < (long)(H + 2 * G) * D || lddx < (long)(H + 2 * G) * D || !g || !dx ||",
    "!al16(g) || !al16(dx)",
    "(gamma_q == nullptr) != (gamma_k == nullptr) || !al16(gamma_q) || !al16(gamma_k)",
    "norm && (!x || !al16(x) || ldx < (long)(H + 2 * G) * D || !inv || !dgamma || !workspace ||",
    "workspace_bytes < osuf_joint_qknorm_bwd_workspace_bytes(M, H, G, D)",
    "!a || !out || B <= 0 || C <= 0 || L <= 0 || B > 65535",
]
DIT_BAD_KINDS = {k for _, k, _ in DIT_BAD}


def bad_status(entry, kind):
    return 0 if entry.endswith("_workspace_bytes") else EUNSUPPORTED if kind == "dtype" else EINVAL
