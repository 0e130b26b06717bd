"""Plain torch references of the LoRA / DoRA adapter kernels of csrc/elementwise.hip (osuf_dora_effective, osuf_dora_gain,
osuf_pack_weight_adapted, osuf_adapter_finish), written from the comment blocks above the kernels and from include/osufusion_hip.h alone,
the launchers' branch arithmetic restated, and the case tables and seeded generators of tests/test_adapter_rows_gpu.py.

    V[o]  = W[o] + s * sum_q B[o][q] A[q]          W (O, I, k), A (r, I, k), B (O, r)
    g[o]  = m[o] / ||V[o]||_2                       (1 without a magnitude)
    Weff  = g[o] * V[o]
    fwd   F[t][o][i]  = Weff[o][i][t]
    dgrad D[t'][i][o] : same  t' < k : Weff[o][i][k-1-t']
                        down  4 taps : w0, w1, w2, w2
                        up    4 taps : w2, w1 + w2, w0 + w1, w0
    sgbt  = (s g B)^T                               [r][O]
    finish: dB[o][q] (+)= sg[o] tb[o][q];  dA[q][i][t] (+)= gt[k-1-t][i][q];  dm[o] (+)= (s0[o] - bias[o] s1[o]) / m[o]

Every function computes in the dtype of its inputs: fp64 for the reference, fp32 for the "same formula in single precision" whose
distance to the fp64 result scales the tests' bounds (tests/bound_check.py).  In every generated case the rows differ in magnitude by
factors of two, so a gain, a norm or a partial sum taken from the wrong row is an O(1) error.  Nothing here needs a GPU;
tests/test_adapter_reference_cpu.py checks these functions against oracle/lora_oracle.py and fp64 autograd, the branch each table entry
names, and the caps written next to the tables.
"""
from __future__ import annotations

import torch

from tests.audio_reference import CAP_SET, smallest_cap, uni  # noqa: F401
from tests.gemm_reference import _gen, ints  # noqa: F401

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
KINDS = ("same", "down", "up")

# the four adapter entry points -> the tables below that launch them
KERNELS = {"osuf_dora_effective": ("EFFECTIVE",), "osuf_dora_gain": ("GAIN",), "osuf_pack_weight_adapted": ("PACK",),
           "osuf_adapter_finish": ("FINISH",)}


# ---------------------------------------------------------------------------------------------------------------------------------
# formulas
# ---------------------------------------------------------------------------------------------------------------------------------
def adapted(W, A, B, s):
    """V = W + s B A, shaped like W."""
    return W + s * (B @ A.flatten(1)).reshape(W.shape)


def gain(V, mag):
    return mag / torch.sqrt((V.flatten(1) ** 2).sum(1))


def scale_rows(V, g):
    return V if g is None else g.reshape(-1, *([1] * (V.dim() - 1))) * V


def effective(W, A, B, mag, s):
    """-> (Weff, g); g is None without a magnitude."""
    V = adapted(W, A, B, s)
    g = None if mag is None else gain(V, mag)
    return scale_rows(V, g), g


def fwd_layout(We):
    return We.permute(2, 0, 1)


def dgrad_layout(We, kind):
    w = We.permute(2, 1, 0)                                  # [t][i][o]
    if kind == "same":
        return w.flip(0)
    w0, w1, w2 = w
    return torch.stack([w0, w1, w2, w2] if kind == "down" else [w2, w1 + w2, w0 + w1, w0])


def sgbt(B, g, s):
    return (s * B if g is None else s * g[:, None] * B).T


def finish(tb, sg, gt, s0=None, s1=None, bias=None, m=None, bases=None):
    """-> (dB (O, r), dA (r, I, k), dm (O) or None); bases = (dB0, dA0, dm0) are added when given (accumulate = 1)."""
    dB, dA = sg[:, None] * tb, gt.flip(0).permute(2, 1, 0)
    dm = None if m is None else (s0 - (bias * s1 if bias is not None else 0)) / m
    if bases is not None:
        dB, dA = dB + bases[0], dA + bases[1]
        dm = None if dm is None else dm + bases[2]
    return dB, dA, dm


# ---------------------------------------------------------------------------------------------------------------------------------
# which branch the launchers take
# ---------------------------------------------------------------------------------------------------------------------------------
EFFECTIVE_IK_MAX = 150 * 1024 // 4                          # 38400


def effective_branch(O, IK):
    """(channels per block, bytes of LDS above the 48 KiB that need the attribute, blocks, channels of the last block) or "einval"."""
    if IK * 4 > 150 * 1024:
        return "einval"
    oc = 8 if IK * 32 <= 96 * 1024 else 4 if IK * 16 <= 96 * 1024 else 2 if IK * 8 <= 96 * 1024 else 1
    return oc, IK * 4 * oc > 48 * 1024, -(-O // oc), O - oc * ((O - 1) // oc)


def adapt_lds(r, k):
    return (r * 32 * k + 32 * r + 32) * 4


def adapt_branch(O, I, k, r):
    """("plain" | "attr" | "unsupported", i tiles, o tiles, tap chunks)."""
    lds = adapt_lds(r, k)
    kind = "unsupported" if lds > 96 * 1024 else "attr" if lds > 32 * 1024 else "plain"
    return kind, -(-I // 32), -(-O // 32), -(-k // 4)


def finish_branch(O, I, k, r):
    """(the index range that sizes the grid, blocks)."""
    n = max(O * r, r * I * k)
    return ("O*r" if O * r >= r * I * k else "r*I*k"), -(-n // 256)


# ---------------------------------------------------------------------------------------------------------------------------------
# case tables.  Caps (relmax): the smallest of CAP_SET above 16 x the fp32 CPU evaluation's own distance to fp64 over every case of the
# table, held there by test_caps_* of the CPU file.
# ---------------------------------------------------------------------------------------------------------------------------------
S = 0.5                                                     # the adapters' scaling, a power of two for the exact cases
# (id, O, IK, r, mag given, g given, (OC, attribute, blocks, channels of the last block))
EFFECTIVE = [
    ("o1_ik1", 1, 1, 1, True, True, (8, False, 1, 1)),                  # a single element: g = m / |v|
    ("o3_ik200", 3, 200, 8, True, True, (8, False, 1, 3)),              # O < OC: five clamped duplicates of row 2
    ("o9_ik3072", 9, 3072, 17, True, True, (8, True, 2, 1)),            # 96 KiB of LDS
    ("o5_ik3073", 5, 3073, 8, True, True, (4, True, 2, 1)),             # OC 4, O % OC != 0
    ("o3_ik6145", 3, 6145, 8, True, True, (2, True, 2, 1)),             # OC 2, O % OC != 0: the reference trainer's width
    ("o3_ik6145_lora", 3, 6145, 17, False, True, (2, True, 2, 1)),      # mag NULL: g == 1
    ("o2_ik12289", 2, 12289, 1, True, True, (1, True, 2, 1)),           # OC 1
    ("o2_ik38400", 2, 38400, 8, True, False, (1, True, 2, 1)),          # OC 1 at the widest row (150 KiB), g NULL
]
EFFECTIVE_EINVAL = (2, EFFECTIVE_IK_MAX + 1)
EFFECTIVE_CAP, G_CAP = 1e-5, 1e-5

# (id, O, I, k, r, mag given, outputs "32" | "16" | "both", (lds kind, i tiles, o tiles, tap chunks))
GAIN = [
    ("o1_i1_k1", 1, 1, 1, 1, True, "both", ("plain", 1, 1, 1)),
    ("o33_i31_k3", 33, 31, 3, 8, True, "32", ("plain", 1, 2, 1)),
    ("o255_i32_k7", 255, 32, 7, 4, True, "16", ("plain", 1, 8, 2)),
    ("o256_i33_k1", 256, 33, 1, 17, True, "both", ("plain", 2, 8, 1)),
    ("o257_i70_k3", 257, 70, 3, 8, True, "both", ("plain", 3, 9, 1)),   # three partial tiles; the gain kernel's second block
    ("o33_i70_k7_r32", 33, 70, 7, 32, True, "both", ("attr", 3, 2, 2)), # 32,896 B of LDS
    ("o257_i33_k3_lora", 257, 33, 3, 8, False, "both", ("plain", 2, 9, 1)),   # mag NULL: g == 1, partial NULL
]
ADAPT_UNSUPPORTED = (96, 7)                                 # (r, k): 98,432 B
SGBT_CAP = 1e-5

# (id, O, I, k, r, kind, g given, outputs "FD" | "F" | "D", (lds kind, i tiles, o tiles, tap chunks))
PACK = [
    ("o1_i1_k1", 1, 1, 1, 1, "same", True, "FD", ("plain", 1, 1, 1)),
    ("o31_i33_k3_same", 31, 33, 3, 8, "same", True, "FD", ("plain", 2, 1, 1)),
    ("o33_i31_k3_down", 33, 31, 3, 8, "down", True, "FD", ("plain", 1, 2, 1)),
    ("o70_i32_k3_up", 70, 32, 3, 17, "up", True, "FD", ("plain", 1, 3, 1)),
    ("o32_i70_k4", 32, 70, 4, 8, "same", False, "FD", ("plain", 3, 1, 1)),
    ("o33_i33_k5", 33, 33, 5, 8, "same", True, "FD", ("plain", 2, 2, 2)),         # 4 + 1 taps
    ("o70_i70_k7", 70, 70, 7, 8, "same", True, "FD", ("plain", 3, 3, 2)),         # 4 + 3 taps, with a gain
    ("o33_i31_k7_f", 33, 31, 7, 4, "same", True, "F", ("plain", 1, 2, 2)),        # F only
    ("o31_i33_k3_up_d", 31, 33, 3, 8, "up", False, "D", ("plain", 2, 1, 1)),      # D only
    ("o33_i70_k3_down_r64", 33, 70, 3, 64, "down", True, "FD", ("attr", 3, 2, 1)),    # 32,896 B of LDS
    ("o32_i32_k7_r32", 32, 32, 7, 32, "same", False, "FD", ("attr", 1, 1, 2)),
]
PACK_CAP = 1e-5
STACKED = ("o33_i31_k3_stacked", 33, 31, 3, 8, 40, 5)       # ..., rows of the stacked operand, row_offset

# (id, O, I, k, r, accumulate, dm given, bias given, (largest range, blocks))
FINISH = [
    ("o300_i2_k1_r3", 300, 2, 1, 3, 0, True, True, ("O*r", 4)),         # O r = 900 > r I k = 6
    ("o5_i40_k7_r3", 5, 40, 7, 3, 1, True, True, ("r*I*k", 4)),         # r I k = 840 > O r = 15
    ("o33_i31_k3_r8", 33, 31, 3, 8, 0, True, False, ("r*I*k", 3)),      # bias NULL with dm
    ("o33_i31_k3_r8_nodm", 33, 31, 3, 8, 1, False, False, ("r*I*k", 3)),
    ("o1_i1_k1_r1", 1, 1, 1, 1, 0, True, True, ("O*r", 1)),
    ("o257_i3_k3_r1", 257, 3, 3, 1, 1, True, True, ("O*r", 2)),         # r = 1: the dm range is as long as the dB range
    ("o40_i5_k7_r17", 40, 5, 7, 17, 0, True, True, ("O*r", 3)),
]
DM_CAP = 1e-5
TABLES = {"EFFECTIVE": EFFECTIVE, "GAIN": GAIN, "PACK": PACK, "FINISH": FINISH}


# ---------------------------------------------------------------------------------------------------------------------------------
# seeded inputs
# ---------------------------------------------------------------------------------------------------------------------------------
def row_pow2(O, lo=-2, span=5):
    """2^(lo + o % span): neighbouring rows differ by factors of two."""
    return torch.ldexp(torch.ones(O, dtype=F32), torch.arange(O) % span + lo)


def real_factors(cid, O, I, k, r, mag=True):
    """W, A, B (fp32) with rows of W and B scaled by row_pow2, and m = 2^(o % 3) * (1 + U(-0.2, 0.2)), or None."""
    sc = row_pow2(O)
    W = uni(f"ad.w.{cid}", (O, I, k), 0.3) * sc[:, None, None]
    A = uni(f"ad.a.{cid}", (r, I, k), 1.0 / (I * k) ** 0.5)
    B = uni(f"ad.b.{cid}", (O, r), 1.0 / r ** 0.5) * sc[:, None]
    m = (row_pow2(O, 0, 3) * (1 + uni(f"ad.m.{cid}", (O,), 0.2))) if mag else None
    return W, A, B, m


def real_gain(cid, O):
    """A gain handed to the pack kernel: row_pow2 * (1 + U(-0.3, 0.3)), fp32 (not a kernel's output)."""
    return row_pow2(O, -1, 4) * (1 + uni(f"ad.g.{cid}", (O,), 0.3))


def exact_factors(cid, O, I, k, r):
    """w[o][i][t] = (o I + i) k + t (names its place, < 2^16), A and B integers of [-2, 2]; with s = 1/2 and g = 2^(-2..2) every value of
    g (w + s B A) and every sum of two of them is a multiple of 1/8 below 2^21: exact in fp32 in any order."""
    W = torch.arange(O * I * k, dtype=F32).reshape(O, I, k)
    return W, ints(f"ad.xa.{cid}", (r, I, k), 2), ints(f"ad.xb.{cid}", (O, r), 2)


def finish_inputs(cid, O, I, k, r, exact):
    """tb, sg, gt and (dB0, dA0, dm0) bases as integers / powers of two when exact; s0, s1, bias, m real-valued always."""
    if exact:
        tb, gt, sg = ints(f"ad.tb.{cid}", (O, r), 9), ints(f"ad.gt.{cid}", (k, I, r), 9), row_pow2(O)
        bases = [ints(f"ad.b0.{cid}", (O, r), 9), ints(f"ad.a0.{cid}", (r, I, k), 9)]
    else:
        tb, gt, sg = uni(f"ad.tb.{cid}", (O, r)), uni(f"ad.gt.{cid}", (k, I, r)), row_pow2(O) * (1 + uni(f"ad.sg.{cid}", (O,), 0.3))
        bases = [uni(f"ad.b0.{cid}", (O, r)), uni(f"ad.a0.{cid}", (r, I, k))]
    s0, s1, bias = uni(f"ad.s0.{cid}", (O,), 4.0), uni(f"ad.s1.{cid}", (O,), 4.0), uni(f"ad.bias.{cid}", (O,), 0.5)
    m = row_pow2(O, 0, 3) * (1 + uni(f"ad.fm.{cid}", (O,), 0.2))
    return dict(tb=tb, sg=sg, gt=gt, s0=s0, s1=s1, bias=bias, m=m, bases=bases + [uni(f"ad.m0.{cid}", (O,))])


def cast(t, dtype):
    if isinstance(t, (list, tuple)):
        return [cast(u, dtype) for u in t]
    return None if t is None else t.to(dtype)
