"""Plain torch references of the embedding-sized linears (csrc/skinny.hip), written from the formulas of include/osufusion_hip.h alone,
the restated slice plan of osuf_skinny_bwd, and the case tables of tests/test_skinny_rows_gpu.py.

    fwd : y = out_act( in_act(x) W^T + b )
    bwd : dz = dy * out_act'(y);  dx = (dz W) * in_act'(x);  dW (+)= dz^T in_act(x);  db += colsum(dz)

Every function computes in the dtype of its inputs (fp64 for the reference, fp32 for the "same formula in single precision" whose distance
to the fp64 result scales the tests' bounds) and models the kernels' roundings: in mode "bf16" both MFMA operands are rounded to bf16 after
the steps that produce them -- bf16(in_act(x)), bf16(W), bf16(dy * y(1-y)) -- the accumulation is unrounded, silu'(x) multiplies the finished
sum, db sums the UNROUNDED dz, and the sigmoid derivative is taken from the stored y.  Mode "f32" rounds nothing.

A reference that rounds an operand to bf16 would depend on the last bit of the activation behind it (the kernels use a fast exp and a
reciprocal, FAST = 2^-21 relative), so the input generators keep every such operand out of a band of 4 * FAST (relative) around each bf16
rounding boundary: a value inside is replaced by the next generated one that is not.  Nothing here needs a GPU;
tests/test_skinny_reference_cpu.py checks these functions against autograd, the slice plan against the branch each table entry names,
the band, and that no cap of the GPU file binds below fp32's own noise.
"""
from __future__ import annotations

import torch

from tests.gemm_reference import FAST, _gen, ints, sigmoid, silu_grad  # noqa: F401  (ints: the exact cases' operands)

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
MODES = ("f32", "bf16")
ACTS = [(0, 0), (1, 0), (0, 2), (1, 2)]                     # (in_act, out_act) pairs the kernels accept: 1 SiLU on x, 2 sigmoid on y
BAND = 4 * FAST
OUT_CAP, DB_CAP = 2e-5, 1e-5                                # the suite's own f32 figures for y / dx / dW and for db (test_skinny_linear_kernels)
ELEM_REL = 2.0 ** -20                                       # per-element term of the element-by-element check


# ---------------------------------------------------------------------------------------------------------------------------------
# formulas
# ---------------------------------------------------------------------------------------------------------------------------------
def rb(t, mode):
    """What an MFMA operand keeps of t: bf16 in mode "bf16", everything otherwise; returned in t's dtype."""
    return t.to(F32).to(BF16).to(t.dtype) if mode == "bf16" else t


def silu(x):
    return x * sigmoid(x)


def fwd(x, W, b, in_act, out_act, mode="f32"):
    z = rb(silu(x) if in_act else x, mode) @ rb(W, mode).T
    if b is not None:
        z = z + b
    return sigmoid(z) if out_act == 2 else z


def dz_of(dy, y, out_act):
    """dz = dy * out_act'(y), unrounded; the sigmoid derivative through the output."""
    return dy * (y * (1 - y)) if out_act == 2 else dy


def dx(dy, y, x, W, in_act, out_act, mode="f32"):
    g = rb(dz_of(dy, y, out_act), mode) @ rb(W, mode)
    return g * silu_grad(x) if in_act else g


def dw(dy, y, x, in_act, out_act, base_dW=None, base_db=None, accumulate=False, mode="f32"):
    """-> (dW, db): dW = dz^T in_act(x) (+ base_dW when accumulate); db = base_db + colsum(dz), None without base_db."""
    d = dz_of(dy, y, out_act)
    g = rb(d, mode).T @ rb(silu(x) if in_act else x, mode)
    if accumulate:
        g = g + base_dW
    return g, (None if base_db is None else base_db + d.sum(0))


def fwd_group(x, Ws, bs, in_act, mode="f32"):
    return [fwd(x, W, b, in_act, 0, mode) for W, b in zip(Ws, bs)]


def dx_group(dys, Ws, x, in_act, mode="f32"):
    """in_act'(x) * sum_i dy_i W_i over the linears whose dy is present."""
    g = sum(rb(d, mode) @ rb(W, mode) for d, W in zip(dys, Ws) if d is not None)
    return g * silu_grad(x) if in_act else g


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------
def uni(tag, shape, scale=1.0):
    """fp32 U(-scale, scale), deterministic in (tag, shape)."""
    return ((2 * torch.rand(*shape, generator=_gen(tag, shape), dtype=F64) - 1) * scale).to(F32)


def near_boundary(v, band=BAND):
    """True where |v| lies within band * |v| of the midpoint of two adjacent bf16 numbers (where bf16 rounding changes direction)."""
    a = v.double().abs()
    m, _ = torch.frexp(a)                                    # a = m * 2^e, m in [0.5, 1): bf16 numbers sit at the integers of t = 256 m
    t = m * 256
    return ((t - torch.floor(t) - 0.5).abs() <= band * t) & (a > 0)


def nudged(tag, shape, scale, operands):
    """uni(tag, shape, scale) with every element replaced, until none of operands(v) (fp64 tensors of v's shape) is near a boundary, by
    the element at the same place of the next draw."""
    v = uni(tag, shape, scale)
    for r in range(1, 16):
        bad = torch.zeros(shape, dtype=torch.bool)
        for o in operands(v.double()):
            bad |= near_boundary(o)
        if not bad.any():
            return v
        v = torch.where(bad, uni(f"{tag}#{r}", shape, scale), v)
    raise AssertionError(f"{tag}: still inside the band after 15 draws")


def make_x(tag, M, K):
    """|x| <= 1.5; neither x nor silu(x) near a boundary (the operand in either activation setting)."""
    return nudged(tag, (M, K), 1.5, lambda v: (v, silu(v)))


def make_w(tag, N, K):
    return nudged(tag, (N, K), 1.0 / K ** 0.5, lambda v: (v,))


def make_b(tag, N):
    return uni(tag, (N,), 0.2)


def make_y(x, W, b, in_act, out_act, mode):
    """The y a backward launch is given: the fp64 forward rounded once to fp32 (not a kernel's output)."""
    return fwd(x.double(), W.double(), None if b is None else b.double(), in_act, out_act, mode).to(F32)


def make_dy(tag, y, out_act):
    """|dy| <= 1; neither dy nor dy * y(1-y) near a boundary."""
    yd = y.double()
    return nudged(tag, tuple(y.shape), 1.0, lambda v: (v, dz_of(v, yd, out_act)))


# ---------------------------------------------------------------------------------------------------------------------------------
# which branch the host picks (osuf_skinny_fwd / osuf_skinny_bwd restated)
# ---------------------------------------------------------------------------------------------------------------------------------
def fwd_vec(K, ldx, x_off=0):
    """x_off: offset of x from a 16-byte boundary in floats (W is always aligned here)."""
    return K % 8 == 0 and ldx % 4 == 0 and x_off % 4 == 0


def dx_vec(N, lddy, dy_off=0):
    return N % 8 == 0 and lddy % 4 == 0 and dy_off % 4 == 0


def bwd_split(N, K):
    """-> (nsplit, rows per slice) of the dx launch: one slice stores, more than one add into a zeroed dx with atomics."""
    ktiles = -(-K // 32)
    nsplit = min(-(-256 // ktiles), -(-N // 128))
    if N * K <= 64 * 1024:
        nsplit = 1
    nsplit = max(nsplit, 1)
    nps = -(-(-(-N // nsplit)) // 64) * 64
    return -(-N // nps), nps


def dx_branch(N, K, dy_off=0):
    """(vec, slices, rows of the last slice)."""
    ns, nps = bwd_split(N, K)
    return dx_vec(N, N, dy_off), ns, N - (ns - 1) * nps


def dw_tiles(N, K):
    return -(-K // 32) * -(-N // 32)


# ---------------------------------------------------------------------------------------------------------------------------------
# case tables: the smallest shapes that still reach each branch.  Every shape runs at M = 33 (two trips of the m0 loop, a ragged second)
# and at one other M of {1, 5, 32, 65}; each M appears at least twice per table.
# ---------------------------------------------------------------------------------------------------------------------------------
# forward: (id, N, K, (M, M), x offset in floats, ldx - K, pure geometry, vec)
FWD = [
    ("n33_k5", 33, 5, (33, 5), 0, 0, False, False),          # K < 8: non-vec, zero fill past K
    ("n8_k8", 8, 8, (33, 1), 0, 0, False, True),             # vec, one k-step: only the lh = 0 lane half of wave 0 has work
    ("n40_k72", 40, 72, (33, 65), 0, 0, False, True),        # N tail in the second block, k-steps in five of the eight (wave, half) slots
    ("n31_k264", 31, 264, (33, 32), 0, 0, False, True),      # second trip of the 256-wide k loop
    ("n72_k520", 72, 520, (33, 65), 0, 0, False, True),      # third trip
    ("n64_k1", 64, 1, (33, 1), 0, 0, False, False),          # K = 1
    ("n1_k64", 1, 64, (33, 5), 0, 0, False, True),           # N = 1: every W row but one is the clamped row
    ("n40_k72_xoff1", 40, 72, (33, 32), 1, 0, True, False),  # K % 8 == 0 but x one float off: non-vec, sk_load8's fallback on every x load
    ("n40_k72_ldx4", 40, 72, (33, 5), 0, 4, True, True),     # vec with a row stride of its own
    ("n40_k72_ldx1", 40, 72, (33, 65), 0, 1, True, False),   # ldx % 4 != 0: non-vec, aligned and misaligned rows alternate load by load
]
# input gradient: (id, N, K, (M, M), dy offset in floats, pure geometry, vec, slices, rows of the last slice)
DX = [
    ("n256_k256", 256, 256, (33, 65), 0, False, True, 1, 256),       # N K = 65536 exactly: one slice, plain stores
    ("n264_k256", 264, 256, (33, 5), 0, False, True, 3, 8),          # memset + atomics; the last slice is one 8-row group
    ("n257_k256", 257, 256, (33, 1), 0, False, False, 3, 1),         # non-vec, last slice of one row
    ("n136_k488", 136, 488, (33, 32), 0, False, True, 2, 8),         # ragged last k tile (488 = 15 * 32 + 8)
    ("n2048_k40", 2048, 40, (33, 65), 0, False, True, 16, 128),      # 16 slices
    ("n33_k17", 33, 17, (33, 5), 0, False, False, 1, 33),
    ("n8_k8", 8, 8, (33, 1), 0, False, True, 1, 8),
    ("n264_k256_dyoff1", 264, 256, (33, 32), 1, True, False, 3, 8),  # N % 8 == 0 but dy one float off: non-vec through sk_load8's fallback
]
# weight gradient: (id, N, K, (M, M), accumulate, db given); bases are non-zero in every case
DW = [
    ("n33_k5", 33, 5, (33, 5), 1, True),
    ("n8_k8", 8, 8, (33, 1), 0, True),
    ("n40_k72_a0_db", 40, 72, (33, 65), 0, True),            # 6 tiles: the second workgroup has two idle waves
    ("n40_k72_a1_db", 40, 72, (33, 65), 1, True),
    ("n40_k72_a0", 40, 72, (33, 32), 0, False),
    ("n40_k72_a1", 40, 72, (33, 32), 1, False),
    ("n31_k264", 31, 264, (33, 32), 1, True),
    ("n72_k520", 72, 520, (33, 65), 0, False),
    ("n64_k1", 64, 1, (33, 1), 1, False),
    ("n1_k64", 1, 64, (33, 5), 0, True),
]
# group: (id, M, K, N_i, index of the linear without bias, index of the linear whose dy is absent)
GROUP_N = (8, 40, 520, 1032, 64)                             # 520 and 1032: dx slices of 512 + 8 rows; 8 and 40: no multiple of 32
GROUP = [(f"m{M}_k{K}", M, K, GROUP_N, 2, 1) for M in (5, 33) for K in (96, 264)] + [("single_m33_k96", 33, 96, (40,), None, None)]
GROUP_ACTS = [0, 1]                                          # the group forms have no output activation

# strided outputs (section C): M, and the shapes whose dx takes one slice and atomics
STRIDED_M, PAD_L, PAD_R = 33, 8, 16                          # the output is columns [8, 8 + width) of a buffer 24 wider, with a spare last row
STRIDED_FWD = ("n40_k72", 40, 72)
STRIDED_DX = [("n256_k256", 256, 256), ("n264_k256", 264, 256)]
STRIDED_GROUP = ("m33_k96", 33, 96, GROUP_N, 2, 1)


def cases(table):
    """(entry, M) for every entry of FWD / DX / DW."""
    for e in table:
        for M in e[3]:
            yield e, M


# ---------------------------------------------------------------------------------------------------------------------------------
# real-valued cases: inputs and references (shared by the GPU file and the CPU guard of its caps)
# ---------------------------------------------------------------------------------------------------------------------------------
def linear_inputs(cid, M, N, K, in_act, out_act, mode, bias=True):
    """x, W, b for a forward launch; y and dy for the backward launches of the same linear (y from the fp64 forward, never from a kernel)."""
    x, W = make_x(f"sk.x.{cid}", M, K), make_w(f"sk.w.{cid}", N, K)
    b = make_b(f"sk.b.{cid}", N) if bias else None
    y = make_y(x, W, b, in_act, out_act, mode)
    return dict(x=x, W=W, b=b, y=y, dy=make_dy(f"sk.dy.{cid}.{in_act}{out_act}{mode}", y, out_act), in_act=in_act, out_act=out_act, mode=mode)


def dw_bases(cid, N, K):
    return uni(f"sk.dW0.{cid}", (N, K), 0.5), uni(f"sk.db0.{cid}", (N,), 0.5)


def group_inputs(cid, M, K, Ns, nobias, nody):
    x = make_x(f"sk.gx.{cid}", M, K)
    Ws = [make_w(f"sk.gw{i}.{cid}", N, K) for i, N in enumerate(Ns)]
    bs = [None if i == nobias else make_b(f"sk.gb{i}.{cid}", N) for i, N in enumerate(Ns)]
    dys = [None if i == nody else nudged(f"sk.gdy{i}.{cid}", (M, N), 1.0, lambda v: (v,)) for i, N in enumerate(Ns)]
    return dict(x=x, Ws=Ws, bs=bs, dys=dys)


def cast(t, dtype):
    if isinstance(t, (list, tuple)):
        return [cast(u, dtype) for u in t]
    return None if t is None else t.to(dtype)


def linear_refs(inp, dtype, base_dW=None, base_db=None, accumulate=False):
    """(y, dx, dW, db) of one linear in `dtype`."""
    c = lambda k: cast(inp[k], dtype)
    ia, oa, mode = inp["in_act"], inp["out_act"], inp["mode"]
    gw, gb = dw(c("dy"), c("y"), c("x"), ia, oa, cast(base_dW, dtype), cast(base_db, dtype), accumulate, mode)
    return fwd(c("x"), c("W"), c("b"), ia, oa, mode), dx(c("dy"), c("y"), c("x"), c("W"), ia, oa, mode), gw, gb


def group_refs(inp, dtype, in_act, mode):
    """([y_i], dx) of a group in `dtype`."""
    c = lambda k: cast(inp[k], dtype)
    return fwd_group(c("x"), c("Ws"), c("bs"), in_act, mode), dx_group(c("dys"), c("Ws"), c("x"), in_act, mode)


def extra_y(out_act):
    """The fast-math allowance of an output: FAST for an output sigmoid."""
    return FAST if out_act == 2 else 0.0


def extra_dx(in_act, x):
    """FAST * (1 + max|x|) for silu'(x) (its 1 - s carries an ulp of 1, times x)."""
    return FAST * (1 + x.abs().max().item()) if in_act else 0.0


def elementwise_excess(got, ref64, b):
    """max over the elements of |got - ref| / (b * max|ref| + 2^-20 |ref|): at most 1 when no single element is off by more."""
    r = ref64.double()
    return ((got.double().cpu() - r).abs() / (b * r.abs().max() + ELEM_REL * r.abs()).clamp_min(1e-300)).max().item()
