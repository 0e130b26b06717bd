"""HIP-backed mirror of osu_fusion/modules/mmdit.py (the two-stream MMDiT): same classes, constructor arguments, attribute names and
state_dict keys.  Both streams are rows (B, N, dim_h) in the compute dtype; a block runs the DiT's kernels once per stream (adaLN,
gated residual, feed-forward: osufusion_amd/dit.py) around one joint attention over [audio; map] (osufusion_amd/mmdit.py).  The tiny
embedding MLPs run on the skinny-linear kernels and all 2 depth + 1 adaLN modulation projections of a forward in one grouped launch."""
from typing import Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F  # noqa: N812
from torch.utils.checkpoint import checkpoint

from .. import dit as Dt
from .. import functional as Fn
from .. import mmdit as Mm
from .. import ops
from .. import runtime as rt
from .dit import FeedForward, MultiHeadRMSNorm, _TransformerBackbone
from .unet import SinusoidalPositionEmbedding

__all__ = ["modulate", "SinusoidalPositionEmbedding", "FeedForward", "PatchEmbedding", "MultiHeadRMSNorm", "JointAttention", "MMDiTBlock",
           "FinalLayer", "MMDiT"]


def modulate(x: torch.Tensor, shift: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """mmdit.py:13-15, for code written against the reference (the blocks run it inside osuf_adaln_fwd)."""
    return x * (1 + scale.unsqueeze(1)) + shift.unsqueeze(1)


def _head_guard(dim_head: int, heads: int, kv_heads: int) -> None:
    if kv_heads <= 0 or heads % kv_heads != 0:
        raise ValueError(f"attn_heads must be a multiple of attn_kv_heads (got {heads} and {kv_heads})")
    if dim_head not in (16, 32, 64, 128):
        raise NotImplementedError(f"the HIP attention kernels cover head dims 16, 32, 64 and 128 (got attn_dim_head={dim_head})")
    if (heads + 2 * kv_heads) * dim_head > 4096:
        raise NotImplementedError(f"the joint q|k|v rows are at most 4096 wide (got {(heads + 2 * kv_heads) * dim_head})")


def _pad8(n: int) -> int:
    return (n + 7) // 8 * 8


class PatchEmbedding(nn.Module):
    """mmdit.py:44-52: Conv1d with kernel = stride = patch_size.  (B, C, L) is regrouped to (B, C p, L / p) -- channel c p + t holds tap
    t of channel c, the order of proj.weight.reshape(O, C p) -- and runs as rows (B, L / p, C p) through one GEMM; C p is zero-padded
    to a multiple of 8 (the GEMM's K), which adds exact zeros."""

    def __init__(self, dim_in: int, dim_emb: int, patch_size: int) -> None:
        super().__init__()
        self.patch_size = patch_size
        self.proj = nn.Conv1d(dim_in, dim_emb, patch_size, stride=patch_size)
        self._cache = Fn.PackCache()

    def forward_rows(self, x: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
        B, C, L = x.shape
        p = self.patch_size
        assert L % p == 0, "Input sequence length must be divisible by the patch size"
        xr = x.float().reshape(B, C, L // p, p).permute(0, 1, 3, 2).reshape(B, C * p, L // p)
        w = self.proj.weight.reshape(self.proj.weight.shape[0], C * p)
        cpad = _pad8(C * p)
        if cpad != C * p:
            xr = F.pad(xr, (0, 0, 0, cpad - C * p))
            w = F.pad(w, (0, cpad - C * p))
        rows = Fn.RowsFromNCLFn.apply(xr.contiguous(), dtype, cpad, 1)
        return Fn.ConvFn.apply(rows, w, self.proj.bias, self._cache, "same", ("patch", self.proj.weight))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """(B, dim_in, L) -> (B, L / patch_size, dim_emb)."""
        rt.require_gpu(x)
        return self.forward_rows(x, rt.compute_dtype(self.proj.weight.dtype))


class JointAttention(nn.Module):
    """mmdit.py:65-127.  forward(x: (B, Nx, dim), a: (B, Na, dim)) -> (out_x (B, Nx, heads * dim_head), out_a (B, Na, ...)); the two
    lengths may differ."""

    def __init__(self, dim: int, dim_head: int, heads: int, kv_heads: int, qk_norm: bool = True, context_len: int = 4096) -> None:
        super().__init__()
        _head_guard(dim_head, heads, kv_heads)
        self.heads, self.kv_heads, self.qk_norm, self.dim_head = heads, kv_heads, qk_norm, dim_head
        self.to_q_x = nn.Linear(dim, dim_head * heads, bias=False)
        self.to_k_x = nn.Linear(dim, dim_head * kv_heads, bias=False)
        self.to_v_x = nn.Linear(dim, dim_head * kv_heads, bias=False)
        self.q_x_norm = MultiHeadRMSNorm(dim_head, heads) if qk_norm else nn.Identity()
        self.k_x_norm = MultiHeadRMSNorm(dim_head, kv_heads) if qk_norm else nn.Identity()
        self.to_q_a = nn.Linear(dim, dim_head * heads, bias=False)
        self.to_k_a = nn.Linear(dim, dim_head * kv_heads, bias=False)
        self.to_v_a = nn.Linear(dim, dim_head * kv_heads, bias=False)
        self.q_a_norm = MultiHeadRMSNorm(dim_head, heads) if qk_norm else nn.Identity()
        self.k_a_norm = MultiHeadRMSNorm(dim_head, kv_heads) if qk_norm else nn.Identity()
        self._cache = Fn.PackCache()

    def forward_rows(self, x: torch.Tensor, a: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        gx = (self.q_x_norm.gamma, self.k_x_norm.gamma) if self.qk_norm else (None, None)
        ga = (self.q_a_norm.gamma, self.k_a_norm.gamma) if self.qk_norm else (None, None)
        return Mm.joint_attention(x, a, (self.to_q_x.weight, self.to_k_x.weight, self.to_v_x.weight),
                                  (self.to_q_a.weight, self.to_k_a.weight, self.to_v_a.weight), gx, ga, self._cache,
                                  self.heads, self.kv_heads, self.dim_head)

    def forward(self, x: torch.Tensor, a: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        rt.require_gpu(x)
        dt = rt.compute_dtype(self.to_q_x.weight.dtype)
        return self.forward_rows(rt.cast_rows(x.contiguous(), dt), rt.cast_rows(a.contiguous(), dt))


class MMDiTBlock(nn.Module):
    """mmdit.py:130-222: per stream s in (x, a), s + gate_attn_s * attn_out_s(attn(modulate(norm1_s(s)))), then
    s + gate_mlp_s * mlp_s(modulate(norm2_s(s))), with one JointAttention over both.  The LayerNorms have no parameters; norm1_* /
    norm2_* are kept for the module tree (their eps, 1e-6, is the kernels')."""

    def __init__(self, dim_h: int, dim_h_mult: int = 4, attn_dim_head: int = 64, attn_heads: int = 8, attn_kv_heads: int = 2,
                 attn_qk_norm: bool = True, attn_context_len: int = 4096) -> None:
        super().__init__()
        if attn_heads * attn_dim_head != dim_h:
            raise ValueError(f"MMDiT attention needs attn_heads * attn_dim_head == dim_h (attn_out_* is Linear(dim_h, dim_h)): "
                             f"{attn_heads} * {attn_dim_head} != {dim_h}")
        self.modulation_x = nn.Sequential(nn.SiLU(), nn.Linear(dim_h, dim_h * 6, bias=True))
        self.modulation_a = nn.Sequential(nn.SiLU(), nn.Linear(dim_h, dim_h * 6, bias=True))
        self.norm1_x = nn.LayerNorm(dim_h, elementwise_affine=False, eps=1e-6)
        self.attn_out_x = nn.Linear(dim_h, dim_h, bias=False)
        self.norm2_x = nn.LayerNorm(dim_h, elementwise_affine=False, eps=1e-6)
        self.mlp_x = FeedForward(dim_h, dim_mult=dim_h_mult)
        self.norm1_a = nn.LayerNorm(dim_h, elementwise_affine=False, eps=1e-6)
        self.attn_out_a = nn.Linear(dim_h, dim_h, bias=False)
        self.norm2_a = nn.LayerNorm(dim_h, elementwise_affine=False, eps=1e-6)
        self.mlp_a = FeedForward(dim_h, dim_mult=dim_h_mult)
        self.attn = JointAttention(dim_h, attn_dim_head, attn_heads, attn_kv_heads, qk_norm=attn_qk_norm, context_len=attn_context_len)
        self.gradient_checkpointing = False
        self._caches = {k: Fn.PackCache() for k in ("out_x", "out_a", "mlp_x", "mlp_a")}

    def modulate_input(self, c: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """(modulation_x(c), modulation_a(c)) -> fp32 (B, 6 dim_h) each, on the skinny-linear kernels (MMDiT.forward runs all blocks' at once)."""
        lx, la = self.modulation_x[1], self.modulation_a[1]
        return (rt.small_linear(c.float(), lx.weight, lx.bias, in_act=ops.ACT_SILU),
                rt.small_linear(c.float(), la.weight, la.bias, in_act=ops.ACT_SILU))

    def forward_body(self, x: torch.Tensor, a: torch.Tensor, mod_x: torch.Tensor, mod_a: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """rows (B, Nx, dim_h), (B, Na, dim_h) and the two modulation outputs (B, 6 dim_h) fp32 -> rows.  Column blocks of a modulation
        output: shift_attn, scale_attn, gate_attn, shift_mlp, scale_mlp, gate_mlp."""
        C = x.shape[-1]
        link_x, link_a = Fn.ResLink(), Fn.ResLink()
        h_x = Dt.adaln(x, mod_x, 0, 1, link_x)
        h_a = Dt.adaln(a, mod_a, 0, 1, link_a)
        o_x, o_a = self.attn.forward_rows(h_x, h_a)
        streams = []
        for s, o, mod, link, out, mlp, tag in ((x, o_x, mod_x, link_x, self.attn_out_x, self.mlp_x, "x"),
                                               (a, o_a, mod_a, link_a, self.attn_out_a, self.mlp_a, "a")):
            h = Fn.ConvFn.apply(o, out.weight, None, self._caches["out_" + tag], "same")
            s = Fn.GateResFn.apply(h, mod[:, 2 * C:3 * C], s, None, link)
            link = Fn.ResLink()
            h = Dt.adaln(s, mod, 3, 4, link)
            h = Dt.DiTFeedForwardFn.apply(h, mlp[0].weight, mlp[0].bias, mlp[2].weight, mlp[2].bias, self._caches["mlp_" + tag])
            streams.append(Fn.GateResFn.apply(h, mod[:, 5 * C:6 * C], s, None, link))
        return streams[0], streams[1]

    def forward_rows(self, x: torch.Tensor, a: torch.Tensor, mod_x: torch.Tensor, mod_a: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        if self.training and self.gradient_checkpointing:
            return checkpoint(self.forward_body, x, a, mod_x, mod_a, use_reentrant=False)
        return self.forward_body(x, a, mod_x, mod_a)

    def forward(self, x: torch.Tensor, a: torch.Tensor, c: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """x: (B, Nx, dim_h), a: (B, Na, dim_h), c: (B, dim_h) -> (x, a) (the reference's API)."""
        rt.require_gpu(x)
        dt = rt.compute_dtype(self.mlp_x[0].weight.dtype)
        x, a = rt.cast_rows(x.contiguous(), dt), rt.cast_rows(a.contiguous(), dt)
        return self.forward_rows(x, a, *self.modulate_input(c))


class FinalLayer(nn.Module):
    """mmdit.py:225-238."""

    def __init__(self, dim_h: int, patch_size: int, dim_out: int) -> None:
        super().__init__()
        self.norm = nn.LayerNorm(dim_h, elementwise_affine=False, eps=1e-6)
        self.modulation = nn.Sequential(nn.SiLU(), nn.Linear(dim_h, dim_h * 2, bias=True))
        self.linear = nn.Linear(dim_h, patch_size * dim_out)
        self._cache = Fn.PackCache()

    def forward_rows(self, x: torch.Tensor, mod: torch.Tensor) -> torch.Tensor:
        h = Dt.adaln(x, mod, 0, 1)
        return Fn.ConvFn.apply(h, self.linear.weight, self.linear.bias, self._cache, "same")

    def forward(self, x: torch.Tensor, c: torch.Tensor) -> torch.Tensor:
        rt.require_gpu(x)
        x = rt.cast_rows(x.contiguous(), rt.compute_dtype(self.linear.weight.dtype))
        lin = self.modulation[1]
        return self.forward_rows(x, rt.small_linear(c.float(), lin.weight, lin.bias, in_act=ops.ACT_SILU))


class MMDiT(_TransformerBackbone, nn.Module):
    """mmdit.py:241-389."""

    def __init__(self, dim_in_x: int, dim_in_a: int, dim_in_c: int, dim_h: int, dim_h_mult: int = 4, patch_size: int = 4, depth: int = 12,
                 attn_dim_head: int = 64, attn_heads: int = 8, attn_kv_heads: int = 2, attn_qk_norm: bool = True,
                 attn_context_len: int = 4096) -> None:
        super().__init__()
        self.dim_h = dim_h
        self.dim_in_x = dim_in_x
        self.patch_size = patch_size
        self.attn_context_len = (attn_context_len // patch_size) * 2          # two modalities
        self.emb_x = PatchEmbedding(dim_in_x, dim_h, patch_size)
        self.emb_a = PatchEmbedding(dim_in_a, dim_h, patch_size)
        self.feature_extractor_a = nn.Linear(dim_in_a * 2, dim_h)
        self.mlp_a = FeedForward(dim_h, dim_mult=dim_h_mult)
        self.mlp_time = nn.Sequential(SinusoidalPositionEmbedding(dim_h), FeedForward(dim_h, dim_mult=dim_h_mult))
        self.mlp_cond = nn.Sequential(nn.Linear(dim_in_c, dim_h), FeedForward(dim_h, dim_mult=dim_h_mult))
        self.null_cond = nn.Parameter(torch.randn(dim_h))
        self.blocks = nn.ModuleList([
            MMDiTBlock(dim_h, dim_h_mult=dim_h_mult, attn_dim_head=attn_dim_head, attn_heads=attn_heads, attn_kv_heads=attn_kv_heads,
                       attn_qk_norm=attn_qk_norm, attn_context_len=self.attn_context_len) for _ in range(depth)])
        self.final_layer = FinalLayer(dim_h, self.patch_size, dim_h)
        self.out = nn.Conv1d(dim_h, dim_in_x, 1)
        self._out_cache = Fn.PackCache()
        self.initialize_weights()

    def initialize_weights(self) -> None:
        """mmdit.py:298-329: xavier-uniform Linear / Conv1d weights and zero biases, N(0, 0.02) embedders, zeroed adaLN modulations,
        final layer and output convolution."""
        self.apply(self._basic_init)
        for m in (self.mlp_a[0], self.mlp_a[2], self.mlp_time[1][0], self.mlp_time[1][2], self.mlp_cond[1][0], self.mlp_cond[1][2]):
            nn.init.normal_(m.weight, std=0.02)
        for block in self.blocks:
            for lin in (block.modulation_x[1], block.modulation_a[1]):
                nn.init.zeros_(lin.weight)
                nn.init.zeros_(lin.bias)
        for m in (self.final_layer.modulation[1], self.final_layer.linear, self.out):
            nn.init.zeros_(m.weight)
            nn.init.zeros_(m.bias)

    # -- pieces ---------------------------------------------------------------------------------------------------
    def _embed_cond(self, c: torch.Tensor) -> torch.Tensor:
        """mlp_cond(c)."""
        return self._ff(rt.small_linear(c.float(), self.mlp_cond[0].weight, self.mlp_cond[0].bias), self.mlp_cond[1])

    def _embed_audio(self, a: torch.Tensor) -> torch.Tensor:
        """mlp_a(feature_extractor_a(stat_pool(a))) (mmdit.py:355-359)."""
        fe = self.feature_extractor_a
        return self._ff(rt.small_linear(Dt.stat_pool(a), fe.weight, fe.bias), self.mlp_a)

    def embed_time(self, t: torch.Tensor) -> torch.Tensor:
        """mlp_time(t), fp32 (B, dim_h)."""
        return self._ff(self.mlp_time[0](t).float(), self.mlp_time[1])

    def pad_len(self, n: int) -> int:
        p = self.patch_size
        return (p - n % p) % p

    def encode_audio(self, a: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
        """The audio stream's patch-embedding rows (B, ceil(L / p), dim_h): independent of t and x."""
        return self.emb_a.forward_rows(F.pad(a.float(), (0, self.pad_len(a.shape[-1])), value=-23.0), dtype)

    def encode_x(self, x: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
        return self.emb_x.forward_rows(F.pad(x.float(), (0, self.pad_len(x.shape[-1])), value=-1.0), dtype)

    def denoise_rows(self, h_x: torch.Tensor, h_a: torch.Tensor, cvec: torch.Tensor, n: int) -> torch.Tensor:
        """The two streams' patch rows and the conditioning vector (fp32 (B, dim_h), contiguous) -> the prediction (B, dim_in_x, n)."""
        p = self.patch_size
        lins = [m for b in self.blocks for m in (b.modulation_x[1], b.modulation_a[1])] + [self.final_layer.modulation[1]]
        mods = self._modulations(cvec, lins)                                    # 2 depth + 1
        for i, block in enumerate(self.blocks):
            h_x, h_a = block.forward_rows(h_x, h_a, mods[2 * i], mods[2 * i + 1])
        h = self.final_layer.forward_rows(h_x, mods[-1])                        # (B, N, p dim_h)
        B, N, _ = h.shape
        h = h.view(B, N * p, self.dim_h)                                        # "b n (p d) -> b (n p) d": a view of the rows
        nx = self.dim_in_x
        npad = _pad8(nx)
        w = F.pad(self.out.weight[:, :, 0], (0, 0, 0, npad - nx))
        b = F.pad(self.out.bias, (0, npad - nx))
        y = Fn.ConvFn.apply(h, w, b, self._out_cache, "same", ("out", self.out.weight))
        return Fn.NCLFromRowsFn.apply(y, nx)[:, :, :n]

    def sample_rows(self, x: torch.Tensor, a_rows: torch.Tensor, cvec: torch.Tensor, n: int, dtype: torch.dtype) -> torch.Tensor:
        """A sampler's step: the iterate x (B, dim_in_x, n), encode_audio's rows and the conditioning vector -> the prediction."""
        return self.denoise_rows(self.encode_x(x, dtype), a_rows, cvec, n)

    def forward(self, x: torch.Tensor, a: torch.Tensor, t: torch.Tensor, c: torch.Tensor, cond_drop_prob: float = 0.0) -> torch.Tensor:
        rt.require_gpu(x)
        n = x.shape[-1]
        p = self.patch_size
        dtype = rt.compute_dtype(self.out.weight.dtype)
        cvec = self.embed(a, t, c, cond_drop_prob).contiguous()               # statistics of the unpadded audio
        pad_len = (p - n % p) % p
        h_x = self.emb_x.forward_rows(F.pad(x.float(), (0, pad_len), value=-1.0), dtype)
        h_a = self.emb_a.forward_rows(F.pad(a.float(), (0, pad_len), value=-23.0), dtype)
        return self.denoise_rows(h_x, h_a, cvec, n)
