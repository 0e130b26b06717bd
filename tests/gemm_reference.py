"""Plain torch references of the tap-GEMMs (csrc/gemm.hip), written from the formulas of include/osufusion_hip.h alone, and the case
tables of tests/test_gemm_rows_gpu.py.

    gemm_nt : C[m][n] = act( sum_t sum_k A[rowmap(m,t)][k] * W[t][n][k] + bias[n] ) * silu'(U[m][n]) + R[m][n] * rscale[b][n]
    gemm_tn : dW[t][n1][n2] (+)= sum_m dY[m][n1] * X[rowmap(m,t)][n2]

Every function computes in the dtype of its inputs: the tests call them with fp64 tensors for the reference and with fp32 tensors for
the "same formula in single precision" whose distance to the fp64 result scales the tests' bounds.  The tap sum is one gather and one
matrix product per tap (no per-row loop: tests/test_host_logic.py has that form, and the two are compared on the CPU).  Nothing here
needs a GPU; tests/test_gemm_reference_cpu.py checks these functions against torch.nn.functional and autograd, and that no cap of the
GPU file binds below fp32's own noise on any of the cases listed here.
"""
from __future__ import annotations

import zlib

import torch

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16


# ---------------------------------------------------------------------------------------------------------------------------------
# formulas
# ---------------------------------------------------------------------------------------------------------------------------------
def rowmap(Lin, Lout, stride, pad, mode, taps):
    """[taps][Lout] source row of output row i under tap t, -1 for a zero row.
    mode 0: i*stride + t - pad inside [0, Lin).  mode 1: the same, with row Lin reflected to Lin-2 (right reflect pad of one).
    mode 2: u = i*stride + t - pad indexes the nearest-x2 upsampled input, u // 2 inside [0, 2 Lin).
    mode 3: input gradient of mode 1 (stride 2, three taps): taps 0..2 take e = i - t where e is even and e/2 < Lin; tap 3 is the
    reflected column: only row Lout-2, from Lin-1."""
    i = torch.arange(Lout)[None, :]
    t = torch.arange(taps)[:, None]
    if mode == 3:
        e = i - t
        src = torch.where((e >= 0) & (e % 2 == 0) & (e // 2 < Lin), e // 2, torch.full_like(e, -1))
        if taps > 3:
            src[3] = torch.where(torch.arange(Lout) == Lout - 2, Lin - 1, -1)
        return src
    s = i * stride + t - pad
    if mode == 2:
        return torch.where((s >= 0) & (s < 2 * Lin), s // 2, torch.full_like(s, -1))
    if mode == 1:
        s = torch.where(s == Lin, torch.full_like(s, Lin - 2), s)
    return torch.where((s >= 0) & (s < Lin), s, torch.full_like(s, -1))


def gather_rows(X, idx, Lin):
    """X rows [B*Lin][K] -> [taps][B][Lout][K]: X[b*Lin + idx[t][i]], zeros where idx is -1."""
    Xb = X.reshape(-1, Lin, X.shape[-1])
    Xz = torch.cat([Xb, torch.zeros_like(Xb[:, :1])], 1)                      # row Lin of every sample is the zero row
    return torch.stack([Xz[:, torch.where(ix >= 0, ix, torch.full_like(ix, Lin))] for ix in idx])


def gemm_nt(A, W, *, taps=1, lin=None, lout=None, stride=1, pad=0, mode=0, n_out=None):
    """The accumulator of osuf_gemm_nt: [B*Lout][N] = sum_t gather_t(A) @ W[t]^T.  A rows [B*Lin][K], W [taps][N][K]."""
    W = W if W.dim() == 3 else W[None]
    if lin is None:
        lin = lout = A.shape[0]
    G = gather_rows(A, rowmap(lin, lout, stride, pad, mode, taps), lin)       # [taps][B][Lout][K]
    acc = sum(G[t] @ W[t].T for t in range(taps)).reshape(-1, W.shape[1])
    return acc if n_out is None else acc[:, :n_out]


def sigmoid(x):
    return 1 / (1 + torch.exp(-x))


def silu_grad(u):
    s = sigmoid(u)
    return s * (1 + u * (1 - s))


def epilogue(acc, bias=None, act=0, U=None, R=None, rscale=None, Lout=None):
    """-> (out, pre): pre = acc + bias; out = act(pre) * silu'(U) + R * rscale[b]  (act 1: silu, 2: sigmoid; rscale [B][N])."""
    pre = acc if bias is None else acc + bias[: acc.shape[1]]
    out = pre
    if act == 1:
        out = pre * sigmoid(pre)
    elif act == 2:
        out = sigmoid(pre)
    if U is not None:
        out = out * silu_grad(U)
    if R is not None:
        out = out + (R if rscale is None else R * rscale.repeat_interleave(Lout, 0))
    return out, pre


def gemm_tn(dY, X, *, taps=1, lin=None, lout=None, stride=1, pad=0, mode=0, conv_layout=False, out=None, accumulate=False):
    """[taps][N1][N2], or (N1, N2, taps) with conv_layout; accumulate adds the result to `out`."""
    if lin is None:
        lin = lout = dY.shape[0]
    G = gather_rows(X, rowmap(lin, lout, stride, pad, mode, taps), lin).reshape(taps, -1, X.shape[-1])
    dW = torch.stack([dY.T @ G[t] for t in range(taps)])
    if conv_layout:
        dW = dW.permute(1, 2, 0)
    return dW + out.reshape(dW.shape) if accumulate else dW


def colsum(Y, out=None):
    s = Y.sum(0)
    return s if out is None else s + out


def rowdot_delta(C_stored, O, L, heads):
    """delta[b][h][l] = sum over the head's 64 columns of bf16(C as stored) * O."""
    c = C_stored.to(BF16).to(O.dtype)
    return (c * O).reshape(-1, L, heads, 64).sum(-1).permute(0, 2, 1)


def split_x3(t):
    """(hi, lo) with hi = bf16(t), lo = bf16(t - hi), both returned in t's dtype."""
    f = t.to(F32)
    hi = f.to(BF16).to(F32)
    lo = (f - hi).to(BF16).to(F32)
    return hi.to(t.dtype), lo.to(t.dtype)


def x3_product(mul, a, b):
    """The three products mfma_x3 issues, for any bilinear mul: a_lo b_hi + a_hi b_lo + a_hi b_hi (a_lo b_lo is dropped)."""
    ah, al = split_x3(a)
    bh, bl = split_x3(b)
    return mul(al, bh) + mul(ah, bl) + mul(ah, bh)


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------
def _gen(tag, shape):
    return torch.Generator().manual_seed(zlib.crc32(f"{tag}{tuple(shape)}".encode()))


def rnd(tag, shape, scale=1.0):
    return torch.randn(*shape, generator=_gen(tag, shape)) * scale


def ints(tag, shape, lim):
    """fp32 tensor of integers in [-lim, lim]."""
    return torch.randint(-lim, lim + 1, shape, generator=_gen(tag, shape)).float()


def stored(t, mode):
    """fp32 tensor holding what the storage dtype of `mode` ("bf16" | "f32" | "x3") keeps of t."""
    return t.to(BF16).to(F32) if mode == "bf16" else t.to(F32)


def geom(kind, k, L):
    """-> (forward geometry, input-gradient geometry) as keyword dicts of gemm_nt."""
    if kind == "same":
        return dict(taps=k, lin=L, lout=L, stride=1, pad=k // 2, mode=0), dict(taps=k, lin=L, lout=L, stride=1, pad=k - 1 - k // 2, mode=0)
    if kind == "down":
        return dict(taps=3, lin=L, lout=L // 2, stride=2, pad=0, mode=1), dict(taps=4, lin=L // 2, lout=L, stride=1, pad=0, mode=3)
    assert kind == "up"
    return dict(taps=3, lin=L, lout=2 * L, stride=1, pad=1, mode=2), dict(taps=4, lin=2 * L, lout=L, stride=2, pad=1, mode=0)


# ---------------------------------------------------------------------------------------------------------------------------------
# which kernel the launchers pick (gemm_nt_launch / gemm_tn_launch restated; the kernel trace of the GPU file is the proof)
# ---------------------------------------------------------------------------------------------------------------------------------
def nt_kernel(mode, M, N, K, g, big, no8p=False, nohalo=False, plain=True):
    """mode "bf16" | "f32" | "x3"; g: geometry dict; big: ops.force(gemm_big=1); plain: no epilogue operand at all."""
    if mode == "bf16" and N <= 32 and M >= 4096 and plain:
        return "gemm_nt_skinny_kernel"
    if not big or mode == "f32":
        return {"bf16": "gemm_nt_glds_kernel<bf16>", "f32": "gemm_nt_glds_kernel<float>", "x3": "gemm_nt_glds_kernel<float, true>"}[mode]
    bk = 64 if mode == "bf16" else 32
    halo = (g["taps"] == 3 and g["mode"] == 0 and g["stride"] == 1 and g["pad"] == 1 and g["lin"] == g["lout"] and g["lout"] % 256 == 0
            and K % bk == 0 and not nohalo)
    if halo:
        if mode == "bf16":
            return "gemm_nt_big8_halo3_kernel" if (not no8p and K <= 8192) else "gemm_nt_big_halo3_kernel<bf16>"
        return "gemm_nt_big_halo3_kernel<float>"
    if mode == "bf16" and not no8p and g["taps"] <= 16 and K <= 8192 and K % 64 == 0:
        return "gemm_nt_big8_kernel"
    return "gemm_nt_big_kernel<bf16>" if mode == "bf16" else "gemm_nt_big_kernel<float, true>"


# ---------------------------------------------------------------------------------------------------------------------------------
# case tables
# ---------------------------------------------------------------------------------------------------------------------------------
GEO_N, GEO_B = 328, 3            # N tails at both tile sizes (328 = 2 * 128 + 72 = 256 + 72), and M = 3 L is no multiple of a tile

# A. geometry, exact: (id, kind, k, L, K, use the input-gradient geometry)
GEOMETRIES = [
    ("same1_L520_K64", "same", 1, 520, 64, False),            # one K-step
    ("same1_L200_K128", "same", 1, 200, 128, False),          # two
    ("same1_L264_K192", "same", 1, 264, 192, False),          # odd K-step count
    ("same1_L200_K72", "same", 1, 200, 72, False),            # K % 64 != 0: the one-barrier loop, with a K tail
    ("same1_L40_K40", "same", 1, 40, 40, False),              # K smaller than a K-step
    ("same3_L200_K64", "same", 3, 200, 64, False),            # zero rows at sample edges
    ("same7_L40_K72", "same", 7, 40, 72, False),
    ("same15_L64_K64", "same", 15, 64, 64, False),            # near the 16-tap limit of the 8-phase table
    ("down3_L96_K128", "down", 3, 96, 128, False),            # mode 1
    ("down3_L96_K128_dgrad", "down", 3, 96, 128, True),       # mode 3, four taps
    ("up3_L56_K64", "up", 3, 56, 64, False),                  # mode 2
    ("up3_L56_K64_dgrad", "up", 3, 56, 64, True),             # stride 2
]
# (mode, forced 256^2) crossed with every geometry; exact f32 has no 256^2 kernel
GEO_MODES = [("bf16", False), ("bf16", True), ("f32", False), ("x3", False), ("x3", True)]
# shared-panel k = 3 kernels (forced 256^2, L % 256 == 0): (mode, L, K, ops.force(no8p=True))
HALO = ([("bf16", L, K, no8p) for L in (256, 512) for K in (64, 128, 192) for no8p in (False, True)] +
        [("x3", L, K, False) for L in (256, 512) for K in (32, 96)])
# K > 8192: both 8-phase kernels fall back to the one-barrier loops -- (k, B, L): M = 264 for k = 1; the k = 3 panel needs L = 256
K8256 = [(1, 1, 264), (3, 1, 256)]
# skinny-N (bf16, N <= 32, M >= 4096, no epilogue operand): (N, K, k, B, L)
SKINNY_NT = [(8, 64, 3, 3, 1500), (32, 328, 1, 1, 4100)]

# B. epilogue, real-valued: option sets, each alone and then the combinations the model issues
EPI = {
    "plain": dict(),
    # A and W hold bf16-representable values in every mode: each product is exact in fp32 and only the accumulation rounds, which keeps
    # 16 x the fp32 evaluation's own rel-L2 noise (5e-8 here; 1.5e-7 with 24-bit operands, at any depth from 64 up) under PROD_CAP_L2
    "product": dict(coarse=True),
    "bias": dict(bias=True),
    "silu": dict(bias=True, act=1),
    "sigmoid": dict(bias=True, act=2),
    "pre": dict(bias=True, act=1, want_pre=True),                                  # C2
    "dact": dict(U=True),                                                          # FeedForward backward: (dout W2) * silu'(pre), MODE 2
    "res": dict(R=True),                                                           # MODE 1
    "res_rscale": dict(R=True, rscale=True),
    "res_dact": dict(R=True, U=True),                                              # MODE 3
    "stats": dict(bias=True, stats=True),
    "block": dict(bias=True, stats=True, want_pre=True),                           # Block.proj: conv + bias, GroupNorm sums
    "resblock_out": dict(bias=True, act=1, R=True, rscale=True, stats=True, want_pre=True),   # every operand the forward can carry
    "dgrad_res": dict(R=True, rscale=True, U=True),
}
EPI_SHAPE = dict(B=2, L=200, K=64, N=328, k=3)
# sample boundaries inside a tile (B = 5, L = 40) and inside an 8-row pass (B = 20, L = 12), for the per-sample operands
BOUNDARY = [(5, 40), (20, 12)]
BOUNDARY_EPI = ["stats", "res_rscale", "resblock_out"]
EPI_MODES = [("bf16", False), ("bf16", True), ("f32", False), ("x3", False), ("x3", True)]
ROWDOT = dict(B=3, L=43, K=64, heads=5)                                            # N = 320: a 64-column tail at both tile sizes
# strided operands, one per epilogue implementation: (options, forced 256^2)
STRIDED = [("plain", False), ("res_dact", False), ("plain", True), ("res_dact", True)]

OUT_CAP, PROD_CAP_L2, X3_L2, PK_L2 = 2e-5, 2e-6, 3e-5, 3e-3
FAST = 2.0 ** -21

COLSUM_M, COLSUM_N = [1, 256, 257, 700], [8, 264, 520]

# Weight gradients, exact: (id, mode, B, L, N1, N2, kind, k, conv_layout, accumulate, ops.force keywords, kernel, reduce kernel or None)
_F32P = {"wgrad_f32_partials": True}
_OFF = {"gemm_big": 0}
_BIG = {"gemm_big": 1}
WGRAD_EXACT = [
    ("tn128_bf16_t3", "bf16", 3, 200, 328, 128, "same", 3, True, False, _OFF, "gemm_tn_kernel<bf16>", None),
    ("tn128_f32_t3", "f32", 3, 200, 328, 128, "same", 3, True, True, {}, "gemm_tn_kernel<float>", None),
    ("tn128_x3_t3", "x3", 3, 200, 328, 128, "same", 3, True, False, _OFF, "gemm_tn_kernel<float, true>", None),
    ("tn128_bf16_t1", "bf16", 3, 200, 328, 128, "same", 1, False, True, _OFF, "gemm_tn_kernel<bf16>", None),
    ("tn128_f32_t1", "f32", 3, 200, 328, 128, "same", 1, False, False, {}, "gemm_tn_kernel<float>", None),
    ("tn128_x3_t1", "x3", 3, 200, 328, 128, "same", 1, False, True, _OFF, "gemm_tn_kernel<float, true>", None),
    # 256^2 kernel, fp32 partial tiles.  (M, N1, N2, taps) = (1024, 328, 128, 3): 16 splits; L = 64 keeps it off the merged-taps kernel
    ("big_bf16_t3_conv", "bf16", 16, 64, 328, 128, "same", 3, True, False, _F32P, "gemm_tn_big_kernel", "wgrad_reduce4_kernel<1>"),
    ("big_x3_t3_conv", "x3", 16, 64, 328, 128, "same", 3, True, True, {}, "gemm_tn_big_x3_kernel", "wgrad_reduce4_kernel<1>"),
    ("big_bf16_t3_few", "bf16", 7, 64, 328, 128, "same", 3, False, True, _F32P, "gemm_tn_big_kernel", "wgrad_reduce_kernel<0>"),     # 7 splits
    ("big_x3_t3_few", "x3", 7, 64, 328, 128, "same", 3, True, False, {}, "gemm_tn_big_x3_kernel", "wgrad_reduce_kernel<1>"),
    # (2048, 256, 64, 1): 32 splits; the conv layout with one tap has no four-lane reduce
    ("big_bf16_t1", "bf16", 2, 1024, 256, 64, "same", 1, False, False, _F32P, "gemm_tn_big_kernel", "wgrad_reduce4_kernel<0>"),
    ("big_bf16_t1_conv", "bf16", 2, 1024, 256, 64, "same", 1, True, True, _F32P, "gemm_tn_big_kernel", "wgrad_reduce_kernel<1>"),
    ("big_x3_t1", "x3", 2, 1024, 256, 64, "same", 1, False, True, {}, "gemm_tn_big_x3_kernel", "wgrad_reduce4_kernel<0>"),
    # merged taps (L % 128 == 0): (2 * 256, 256, 256, 3) is four splits, (4 * 256, ...) eight
    ("taps3_bf16_conv", "bf16", 2, 256, 256, 256, "same", 3, True, False, _F32P, "gemm_tn_taps3_kernel", "wgrad_reduce_kernel<1>"),
    ("taps3_bf16", "bf16", 2, 256, 256, 256, "same", 3, False, True, _F32P, "gemm_tn_taps3_kernel", "wgrad_reduce_kernel<0>"),
    ("taps3_x3_conv", "x3", 2, 256, 256, 256, "same", 3, True, True, {}, "gemm_tn_taps3_x3_kernel", "wgrad_reduce_kernel<1>"),
    ("taps3_bf16_many", "bf16", 4, 256, 256, 256, "same", 3, True, False, _F32P, "gemm_tn_taps3_kernel", "wgrad_reduce4_kernel<1>"),
    ("taps3_x3_many", "x3", 4, 256, 256, 256, "same", 3, False, False, {}, "gemm_tn_taps3_x3_kernel", "wgrad_reduce4_kernel<0>"),
    # skinny (bf16, N2 <= 32, M >= 4096): atomics
    ("skinny_t3", "bf16", 2, 2100, 328, 32, "same", 3, True, False, {}, "gemm_tn_skinny_kernel", None),
    ("skinny_t1", "bf16", 1, 4100, 328, 8, "same", 1, False, True, {}, "gemm_tn_skinny_kernel", None),
    # down and up geometries on the 256^2 kernel
    ("big_bf16_down", "bf16", 4, 192, 328, 128, "down", 3, True, False, {**_F32P, **_BIG}, "gemm_tn_big_kernel", "wgrad_reduce_kernel<1>"),
    ("big_bf16_up", "bf16", 3, 56, 328, 128, "up", 3, True, True, {**_F32P, **_BIG}, "gemm_tn_big_kernel", "wgrad_reduce_kernel<1>"),
    ("big_x3_down", "x3", 4, 192, 328, 128, "down", 3, False, False, _BIG, "gemm_tn_big_x3_kernel", "wgrad_reduce_kernel<0>"),
]
# bf16-pair partial tiles (they round: real-valued operands, rel-L2 against fp64): (id, B, L, N1, N2, k, conv_layout, accumulate, kernel, reduce)
WGRAD_PK = [
    ("big_t3_conv", 16, 64, 328, 128, 3, True, False, "gemm_tn_big_kernel", "wgrad_reduce_pk_kernel<1, 3>"),
    ("big_t1_conv", 2, 1024, 256, 64, 1, True, True, "gemm_tn_big_kernel", "wgrad_reduce_pk_kernel<1, 1>"),
    ("big_t1", 2, 1024, 256, 64, 1, False, False, "gemm_tn_big_kernel", "wgrad_reduce_pk_kernel<0, 1>"),
    ("taps3_conv", 2, 256, 256, 256, 3, True, True, "gemm_tn_taps3_kernel", "wgrad_reduce_pk_kernel<1, 3>"),
    ("taps3", 2, 256, 256, 256, 3, False, False, "gemm_tn_taps3_kernel", "wgrad_reduce_pk_kernel<0, 1>"),
]


def tn_splits(kernel, M, N1, N2, taps):
    """Splits of the 256^2 and merged-taps weight-gradient plans (tn_big_plan and the merged-taps branch of gemm_tn_launch)."""
    if "taps3" in kernel:
        bt = -(-N1 // 128) * -(-N2 // 128)
        sp = max(256 // bt, 1)
        rows = -(-(-(-M // sp)) // 128) * 128
        return -(-M // rows)
    bt = -(-N1 // 256) * -(-N2 // 256)
    sp = max((256 + bt * taps // 2) // (bt * taps), 1)
    while sp > 1 and -(-sp * bt // 8) * 8 * taps > 256:
        sp -= 1
    rows = -(-(-(-M // sp)) // 64) * 64
    return -(-M // rows)


def reduce_kernel(kernel, M, N1, N2, taps, conv_layout, pk):
    """launch_wgrad_reduce restated."""
    sp = tn_splits(kernel, M, N1, N2, taps)
    lay = 1 if conv_layout else 0
    if pk:
        return f"wgrad_reduce_pk_kernel<{lay}, {3 if (lay == 1 and taps == 3) else 1}>"
    groups = N1 * N2 // 4 if conv_layout else N1 * N2 * taps // 4
    blocks = min(-(-groups // 256), 2048)
    many_ok = True if "taps3" in kernel else (lay == 0 or taps == 3)
    return f"wgrad_reduce4_kernel<{lay}>" if (sp >= 8 and blocks < 512 and many_ok) else f"wgrad_reduce_kernel<{lay}>"


# ---------------------------------------------------------------------------------------------------------------------------------
# real-valued cases: inputs and references (shared by the GPU file and the CPU guard of its caps)
# ---------------------------------------------------------------------------------------------------------------------------------
def epi_inputs(name, mode, B, L, K, N, k):
    """CPU fp32 tensors holding what the storage dtype of `mode` keeps; bias and rscale are fp32 in every mode."""
    o = EPI[name]
    g = geom("same", k, L)[0]
    M = B * L
    ab = "bf16" if o.get("coarse") else mode
    inp = dict(A=stored(rnd("A", (M, K)), ab), W=stored(rnd("W", (k, N, K)) / (K * k) ** 0.5, ab), g=g, act=o.get("act", 0),
               bias=0.5 * rnd("bias", (N,)) if o.get("bias") else None,
               U=stored(1.5 * rnd("U", (M, N)), mode) if o.get("U") else None,
               R=stored(rnd("R", (M, N)), mode) if o.get("R") else None,
               rscale=1 + 0.3 * rnd("rscale", (B, N)) if o.get("rscale") else None)
    return inp


def epi_refs(inp, dtype, x3):
    """(out, pre) of the header's formula in `dtype`; x3: the product as the three split products."""
    c = lambda t: None if t is None else t.to(dtype)
    mul = lambda a, w: gemm_nt(a, w, **inp["g"])
    A, W = c(inp["A"]), c(inp["W"])
    acc = x3_product(mul, A, W) if x3 else mul(A, W)
    return epilogue(acc, c(inp["bias"]), inp["act"], c(inp["U"]), c(inp["R"]), c(inp["rscale"]), inp["g"]["lout"])


def epi_extra(inp):
    """The fast-math allowance of a case: FAST for silu / sigmoid, FAST * (1 + max|U|) for silu' (its 1 - s carries an ulp of 1, times u)."""
    e = FAST if inp["act"] else 0.0
    if inp["U"] is not None:
        e += FAST * (1 + inp["U"].abs().max().item())
    return e


def epi_cases():
    """Every (name, mode, shape) of section B, for the CPU guard."""
    for name in EPI:
        for mode in ("bf16", "f32", "x3"):
            yield name, mode, EPI_SHAPE
    for B, L in BOUNDARY:
        for name in BOUNDARY_EPI:
            for mode in ("bf16", "f32", "x3"):
                yield name, mode, dict(EPI_SHAPE, B=B, L=L)


def rowdot_inputs(mode):
    B, L, K, heads = ROWDOT["B"], ROWDOT["L"], ROWDOT["K"], ROWDOT["heads"]
    return dict(A=stored(rnd("rdA", (B * L, K)), mode), W=stored(rnd("rdW", (1, heads * 64, K)) / K ** 0.5, mode),
                O=stored(rnd("rdO", (B * L, heads * 64)), mode))


def colsum_inputs(M, N, mode):
    return stored(rnd("cs", (M, N + 8)) + 0.25, mode), rnd("cs_out", (N,))


def wgrad_pk_inputs(B, L, N1, N2):
    return stored(0.5 * rnd("pk_dy", (B * L, N1)), "bf16"), stored(rnd("pk_x", (B * L, N2)), "bf16")
