"""Exact attention cases and an fp64 reference for the attention sweeps (tests/test_attn_reference_cpu.py, tests/test_attn_exact_gpu.py).

Plain torch on the CPU; nothing here imports the kernels' Python wrappers.

attention_fp64 is the general reference of softmax(q k^T * scale + bias) v with dq, dk, dv, dbias, delta and lse2 (the log-sum-exp in
the log2 domain, as the kernels store it).  It does not know the closed forms below.

The cases make every intermediate the kernels round to bf16 exactly representable, so one mis-addressed key, query, row constant or
table entry is an O(1) error instead of O(1/N):
  * keys are binary codes: code bit t of key j sits in column col[t] with sign sgn[t] (both differ per (batch, K/V head), so a K row of
    the wrong group or sample is a different code), +1 in every other column;
  * selector: q = s * k[pi(i)] on the code columns, 0 elsewhere, s the power of two with s * scale >= 20: 40 nats separate two distinct
    scores, P[i, pi(i)] = 1, O[i] = v[pi(i)], dV = sums of integer dO rows, dQ = dK = dbias = 0;
  * tie: q = s/2 * (k[a] + k[b]), b = a with one code bit flipped: P = 1/2, 1/2 exactly, dS = +-(dP_a - dP_b)/4 a multiple of 1/2;
  * shift: k[:, D-1] = 1 and q[:, D-1] = -+16 s move every score of a row alike: nothing changes but lse2, which leaves +-128;
  * bias cases: q = 0 and an additive bf16 bias selects one key or ties two;
  * RoPE tables of exact quarter turns, (cos, sin) in {(1, 0), (0, 1), (-1, 0), (0, -1)} by a hash of (position, frequency).
"""
import math

import torch

F64 = torch.float64
BF16 = torch.bfloat16
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
KEY_TILE, Q_BLOCK = 64, 32
# the variants of ops.mqa_bwd at head dim 64: (name, variant name in ops, qsplit).  tests/test_round2_gpu.py takes its list from here.
BWD_CASES = [("auto", "ATTN_AUTO", 0), ("plain", "ATTN_PLAIN", 0), ("pipe-unsplit", "ATTN_PIPE", 1), ("pipe-split2", "ATTN_PIPE", 2),
             ("pipe-split4", "ATTN_PIPE", 4), ("fused", "ATTN_FUSED", 0), ("fused-split2", "ATTN_FUSED", 2),
             ("fused-slabs", "ATTN_FUSED_SLABS", 0), ("fused256", "ATTN_FUSED256", 0)]
BWD_CASES_512 = [("fused512", "ATTN_FUSED512", 1), ("fused512-split2", "ATTN_FUSED512", 2), ("fused512-auto", "ATTN_FUSED512", 0)]
# the shapes of the GPU sweep (tests/test_attn_reference_cpu.py checks every construction at every one of them)
HEAD_DIMS = [16, 32, 64, 128]
LENGTHS = [1, 31, 32, 33, 63, 64, 65, 200, 255, 256, 257, 512, 513, 1024]        # the kernels that take any N
LENGTHS_512 = [512, 1024, 2048]                                                     # the 512-key sweeps; 2048 also the AUTO pipelined dQ
CROSS_LENGTHS = [(40, 5), (33, 257), (64, 1000), (1, 64), (65, 1)]
SHIFT_FWD, SHIFT_BWD = [65, 200], [33, 200, 257]
BIAS_FORMS = ["bhqk", "hqk", "bqk", "bhk", "qk"]
BWD_CASES_512A = [("fused512a", "ATTN_FUSED512A", 1), ("fused512a-split2", "ATTN_FUSED512A", 2), ("fused512a-auto", "ATTN_FUSED512A", 0)]


def bwd_cases(ops, N, ragged512_ok=True):
    """[(name, variant, qsplit)] of every head-dim-64 backward kernel that takes N keys (the 512-key sweeps: whole 32-query blocks /
    whole 512-key blocks, as test_every_attention_backward_kernel_vs_fp32_autograd has always chosen them)."""
    cases = list(BWD_CASES)
    if N % 32 == 0 and (ragged512_ok or N % 512 == 0):
        cases += BWD_CASES_512
    if N % 512 == 0:
        cases += BWD_CASES_512A
    return [(n, getattr(ops, v), s) for n, v, s in cases]


# ---------------------------------------------------------------------------------------------------------
# the general fp64 reference
# ---------------------------------------------------------------------------------------------------------
def attention_fp64(q, k, v, do=None, scale=None, bias=None):
    """q, do (B, H, Nq, D); k, v (B, G, Nk, D) with H % G == 0 (query heads group-major: head h reads K/V head h // (H / G));
    bias broadcastable to (B, H, Nq, Nk).  -> dict(o, lse2[, delta, dq, dk, dv, dbias]) in fp64; dbias dense (B, H, Nq, Nk)."""
    q, k, v = q.to(F64), k.to(F64), v.to(F64)
    B, H, Nq, D = q.shape
    G, Nk = k.shape[1], k.shape[2]
    r = H // G
    scale = D ** -0.5 if scale is None else scale
    ke, ve = k.repeat_interleave(r, dim=1), v.repeat_interleave(r, dim=1)
    s = (q @ ke.transpose(-1, -2)) * scale
    if bias is not None:
        s = s + bias.to(F64)
    m = s.amax(-1, keepdim=True)
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    p = e / l
    out = {"o": p @ ve, "lse2": ((m + l.log()) * LOG2E).squeeze(-1)}
    if do is None:
        return out
    do = do.to(F64)
    dp = do @ ve.transpose(-1, -2)
    delta = (do * out["o"]).sum(-1, keepdim=True)
    ds = p * (dp - delta)
    out["delta"] = delta.squeeze(-1)
    out["dq"] = (ds @ ke) * scale
    out["dk"] = ((ds.transpose(-1, -2) @ q) * scale).view(B, G, r, Nk, D).sum(2)
    out["dv"] = (p.transpose(-1, -2) @ do).view(B, G, r, Nk, D).sum(2)
    out["dbias"] = ds
    return out


def rows(x):
    """(B, h, N, D) -> rows (B, N, h * D)"""
    return x.permute(0, 2, 1, 3).reshape(x.shape[0], x.shape[2], -1)


def heads(x, D):
    """rows (B, N, h * D) -> (B, h, N, D)"""
    return x.reshape(x.shape[0], x.shape[1], -1, D).permute(0, 2, 1, 3)


def is_bf16(x):
    return bool((x.to(BF16).to(x.dtype) == x).all())


# ---------------------------------------------------------------------------------------------------------
# RoPE by quarter turns
# ---------------------------------------------------------------------------------------------------------
def quarter_tables(N, D):
    """(cos, sin) fp32 [N][D/2] with entries in {(1, 0), (0, 1), (-1, 0), (0, -1)}, the turn a hash of (position, frequency index)."""
    n = torch.arange(N, dtype=torch.int64)[:, None]
    f = torch.arange(D // 2, dtype=torch.int64)[None, :]
    t = ((n * 2654435761 + f * 40503 + (n ^ f) * 97 + 12345) >> 7) & 3
    cos = torch.tensor([1.0, 0.0, -1.0, 0.0])[t]
    sin = torch.tensor([0.0, 1.0, 0.0, -1.0])[t]
    return cos.float().contiguous(), sin.float().contiguous()


def rope(x, cos, sin, inverse=False):
    """Half-split RoPE of (..., N, D) by tables [N][D/2]: y1 = x1 c - x2 s, y2 = x2 c + x1 s; inverse: the transpose (which is also what
    the gradient of the un-rotated operand is to the gradient of the rotated one)."""
    h = x.shape[-1] // 2
    c, s = cos.to(x.dtype), sin.to(x.dtype)
    if inverse:
        s = -s
    x1, x2 = x[..., :h], x[..., h:]
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1)


# ---------------------------------------------------------------------------------------------------------
# the constructions
# ---------------------------------------------------------------------------------------------------------
def code_bits(N):
    return max(1, math.ceil(math.log2(N))) if N > 1 else 1


def score_unit(D):
    """the power of two s with s * D^-1/2 >= 20"""
    return 2 ** math.ceil(math.log2(20 * D ** 0.5))


def block_targets(Nk):
    """what every 32-query block must reach: the last valid key, a key of the first key tile, a key of the last key tile"""
    last_tile = ((Nk - 1) // KEY_TILE) * KEY_TILE
    return Nk - 1, range(0, min(KEY_TILE, Nk)), range(last_tile, Nk)


def make_map(Nq, Nk, gen, rot=0):
    """pi: a random permutation (Nq == Nk) or map, patched so that every 32-query block sends one query to the last valid key (which lies
    in the last key tile), one to the first key tile and one more into the last tile.  A block with fewer queries than that (the tail
    block of N = 33 or 65) takes the targets in an order that `rot` rotates, so the heads of a case cover all of them between them."""
    pi = torch.randperm(Nk, generator=gen)[:Nq] if Nq <= Nk else torch.randint(0, Nk, (Nq,), generator=gen)
    last, first_tile, last_tile = block_targets(Nk)
    for q0 in range(0, Nq, Q_BLOCK):
        n = min(Q_BLOCK, Nq - q0)
        want = [last, first_tile[int(torch.randint(0, len(first_tile), (1,), generator=gen))],
                last_tile[int(torch.randint(0, len(last_tile), (1,), generator=gen))]]
        want = want[rot % 3:] + want[:rot % 3]
        slots = torch.randperm(n, generator=gen)[:3].tolist()
        for slot, key in zip(slots, want):
            pi[q0 + slot] = key
    return pi


def map_conditions(pi, Nk):
    """-> the 32-query blocks of pi that miss a condition, as (first query, [last valid key, first tile, last tile] reached).  A block of
    three or more queries must reach all three; a shorter one (it cannot always) as many as it has queries."""
    return [(q0, got) for q0, got in _block_reach(pi, Nk) if sum(got) < min(3, min(Q_BLOCK, pi.numel() - q0))]


def _block_reach(pi, Nk):
    """[(first query of the block, [last valid key, first tile, last tile] reached)]"""
    last, first_tile, last_tile = block_targets(Nk)
    out = []
    for q0 in range(0, pi.numel(), Q_BLOCK):
        blk = pi[q0:q0 + Q_BLOCK].tolist()
        out.append((q0, [last in blk, any(j in first_tile for j in blk), any(j in last_tile for j in blk)]))
    return out


def map_coverage(maps, Nk):
    """-> the 32-query blocks whose targets the maps of one case (all its batch elements and heads) do not cover BETWEEN them: what a
    tail block of one or two queries, which no single map can send to all three targets, still has to meet."""
    per_map = [{q0: got for q0, got in _block_reach(pi, Nk)} for pi in maps]
    return [q0 for q0 in per_map[0] if not all(any(m[q0][t] for m in per_map) for t in range(3))]


class Case:
    """One exact case.  Operands (fp64, all bf16-representable): q, do (B, H, Nq, D); k, v (B, G, Nk, D); closed: the closed-form
    o, lse2, dq, dk, dv and (sparse, as dense) ds."""

    def rows_qkv(self):
        """the kernels' self-attention row image [B][N][(H + 2G) D]: q heads group-major | G k heads | G v heads"""
        return torch.cat([rows(self.q), rows(self.k), rows(self.v)], dim=-1)


def make_case(kind, B, Nq, Nk, H, G, D, shift=0, seed=0, keep_ds=False):
    """kind: "selector" | "tie".  shift: 0, or -1 / +1 for q[:, D-1] = -+16 s against k[:, D-1] = 1."""
    assert kind in ("selector", "tie") and H % G == 0 and (kind == "selector" or Nk >= 2)
    gen = torch.Generator().manual_seed(1000003 * seed + 7919 * Nq + 31 * Nk + D + (0 if kind == "selector" else 1 << 20))
    nb, s, scale, r = code_bits(Nk), score_unit(D), D ** -0.5, H // G
    assert nb <= D - 1
    c = Case()
    c.kind, c.B, c.Nq, c.Nk, c.H, c.G, c.D, c.shift, c.scale, c.s, c.nb = kind, B, Nq, Nk, H, G, D, shift, scale, s, nb
    j = torch.arange(Nk)
    code = torch.stack([1.0 - 2.0 * ((j >> t) & 1) for t in range(nb)], dim=-1).to(F64)            # (Nk, nb)
    k = torch.ones(B, G, Nk, D, dtype=F64)
    col = torch.empty(B, G, nb, dtype=torch.int64)
    for b in range(B):
        for g in range(G):
            col[b, g] = torch.randperm(D - 1, generator=gen)[:nb]
            sgn = (torch.randint(0, 2, (nb,), generator=gen) * 2 - 1).to(F64)
            k[b, g][:, col[b, g]] = code * sgn
    vmax = 7 if kind == "selector" else 1
    v = torch.randint(1, vmax + 1, (B, G, Nk, D), generator=gen).to(F64) * (torch.randint(0, 2, (B, G, Nk, D), generator=gen) * 2 - 1)
    if kind == "selector":
        do = torch.randint(-3, 4, (B, H, Nq, D), generator=gen).to(F64)
    else:                                                          # at most four nonzeros of +-1 per (row, head)
        do = torch.zeros(B, H, Nq, D, dtype=F64)
        where = torch.randint(0, D, (B, H, Nq, 4), generator=gen)
        do.scatter_(-1, where, (torch.randint(0, 2, (B, H, Nq, 4), generator=gen) * 2 - 1).to(F64))
    q = torch.zeros(B, H, Nq, D, dtype=F64)
    pa = torch.empty(B, H, Nq, dtype=torch.int64)
    pb = torch.empty(B, H, Nq, dtype=torch.int64)
    for b in range(B):
        for h in range(H):
            g = h // r
            a = make_map(Nq, Nk, gen, rot=b * H + h)
            pa[b, h] = a
            cols = col[b, g]
            if kind == "selector":
                pb[b, h] = a
                q[b, h][:, cols] = s * k[b, g][a][:, cols]
            else:
                i = torch.arange(Nq)
                other = torch.full((Nq,), -1, dtype=torch.int64)
                for t in range(nb):                                # the first bit from (i + h) on whose flip stays below Nk
                    cand = a ^ torch.bitwise_left_shift(torch.ones_like(i), (i + h + t) % nb)
                    other = torch.where((other < 0) & (cand < Nk), cand, other)
                assert (other >= 0).all() and (other != a).all()
                pb[b, h] = other
                q[b, h][:, cols] = (s / 2) * (k[b, g][a][:, cols] + k[b, g][other][:, cols])
    if shift:
        k[..., D - 1] = 1.0
        q[..., D - 1] = -16.0 * s * (1 if shift < 0 else -1)
    c.q, c.k, c.v, c.do, c.pa, c.pb, c.col = q, k, v, do, pa, pb, col
    # ---- closed forms, from the maps alone ----
    ke, ve = k.repeat_interleave(r, dim=1), v.repeat_interleave(r, dim=1)
    ix = lambda t, idx: torch.gather(t, 2, idx[..., None].expand(-1, -1, -1, D))
    va, vb, ka, kb = ix(ve, pa), ix(ve, pb), ix(ke, pa), ix(ke, pb)
    top = s * (nb if kind == "selector" else nb - 1) * scale + (16.0 * s * scale * (-1 if shift < 0 else 1) if shift else 0.0)
    closed = {"o": (va + vb) / 2, "lse2": torch.full((B, H, Nq), top * LOG2E + (0.0 if kind == "selector" else 1.0), dtype=F64)}
    dsa = ((do * va).sum(-1) - (do * vb).sum(-1)) / 4              # tie: dS at a (= -dS at b); selector: va == vb -> 0
    closed["dq"] = scale * dsa[..., None] * (ka - kb)
    dk = torch.zeros(B, H, Nk, D, dtype=F64)
    dv = torch.zeros(B, H, Nk, D, dtype=F64)
    e = lambda idx: idx[..., None].expand(-1, -1, -1, D)
    dk.scatter_add_(2, e(pa), scale * dsa[..., None] * q)
    dk.scatter_add_(2, e(pb), -scale * dsa[..., None] * q)
    dv.scatter_add_(2, e(pa), do / 2)
    dv.scatter_add_(2, e(pb), do / 2)
    closed["dk"] = dk.view(B, G, r, Nk, D).sum(2)
    closed["dv"] = dv.view(B, G, r, Nk, D).sum(2)
    closed["dsa"] = dsa
    c.closed = closed
    # the cancellation scales of the quantities that are exactly zero (the bounds of the sweep are relative to these)
    c.zero_scale = float(do.abs().max() * v.abs().max() * D)
    return c


def make_bias_case(kind, B, Nq, Nk, H, D, form, seed=0):
    """q = 0 and an additive bf16 bias does the selecting.  kind: "selector" (+64 on one key per query), "tie" (+64 on two), "bool" (the
    lowest finite bf16 on all keys but two).  form: which dimensions the bias has -- "bhqk", "hqk" (broadcast over b), "bqk" (over h),
    "bhk" (over q: key padding), "qk" (over b and h).  -> Case with .bias (its own shape, size-1 broadcast dims) and closed o / lse2 / dsa."""
    assert kind in ("selector", "tie", "bool") and (kind == "selector" or Nk >= 2)
    gen = torch.Generator().manual_seed(424243 * seed + 7919 * Nq + 31 * Nk + D + len(form) * 1009 + {"selector": 0, "tie": 1, "bool": 2}[kind])
    c = Case()
    c.kind, c.B, c.Nq, c.Nk, c.H, c.G, c.D, c.shift, c.scale, c.form = kind, B, Nq, Nk, H, 1, D, 0, D ** -0.5, form
    shape = (B if "b" in form else 1, H if "h" in form else 1, Nq if "q" in form else 1, Nk)
    sel = kind == "selector"
    vmax = 7 if sel else 1
    c.q = torch.zeros(B, H, Nq, D, dtype=F64)
    c.k = torch.randint(-2, 3, (B, 1, Nk, D), generator=gen).to(F64)             # any keys: the queries are zero
    c.v = torch.randint(1, vmax + 1, (B, 1, Nk, D), generator=gen).to(F64) * (torch.randint(0, 2, (B, 1, Nk, D), generator=gen) * 2 - 1)
    if sel:
        c.do = torch.randint(-3, 4, (B, H, Nq, D), generator=gen).to(F64)
    else:
        c.do = torch.zeros(B, H, Nq, D, dtype=F64)
        c.do.scatter_(-1, torch.randint(0, D, (B, H, Nq, 4), generator=gen), (torch.randint(0, 2, (B, H, Nq, 4), generator=gen) * 2 - 1).to(F64))
    pa = torch.empty(shape[:3], dtype=torch.int64)
    for b in range(shape[0]):
        for h in range(shape[1]):
            pa[b, h] = make_map(shape[2], Nk, gen, rot=b * H + h) if shape[2] > 1 else torch.tensor([Nk - 1 if (b + h) % 2 == 0 else 0])
    pb = pa if sel else (pa + 1 + torch.randint(0, Nk - 1, pa.shape, generator=gen)) % Nk
    low = float(torch.finfo(BF16).min)
    bias = torch.full(shape, low if kind == "bool" else 0.0, dtype=F64)
    hi = 0.0 if kind == "bool" else 64.0
    bias.scatter_(-1, pa[..., None], hi)
    bias.scatter_(-1, pb[..., None], hi)
    c.bias = bias
    c.pa, c.pb = pa.expand(B, H, Nq).contiguous(), pb.expand(B, H, Nq).contiguous()
    ve = c.v.expand(B, H, Nk, D)
    ix = lambda idx: torch.gather(ve, 2, idx[..., None].expand(-1, -1, -1, D))
    va, vb = ix(c.pa), ix(c.pb)
    c.closed = {"o": (va + vb) / 2, "lse2": torch.full((B, H, Nq), hi * LOG2E + (0.0 if sel else 1.0), dtype=F64),
                "dsa": ((c.do * va).sum(-1) - (c.do * vb).sum(-1)) / 4}
    c.zero_scale = float(c.do.abs().max() * c.v.abs().max() * D)
    c.s = 1.0
    return c


def closed_dbias(c):
    """dense (B, H, Nq, Nk) dS of a case from its maps: +dsa at a, -dsa at b (selector: zero)"""
    ds = torch.zeros(c.B, c.H, c.Nq, c.Nk, dtype=F64)
    ds.scatter_add_(-1, c.pa[..., None], c.closed["dsa"][..., None])
    ds.scatter_add_(-1, c.pb[..., None], -c.closed["dsa"][..., None])
    return ds


def ulp32(x):
    """spacing of fp32 at |x| (fp64 tensor in, fp64 out)"""
    return torch.exp2(torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126))) - 23)
