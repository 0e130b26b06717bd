"""HIP-backed mirror of osu_fusion/modules/dit.py (the adaLN-Zero DiT): same classes, constructor arguments, attribute names and
state_dict keys.  The hot path is rows (B, L, dim_h) in the compute dtype through the kernels of osufusion_amd/dit.py; the tiny
embedding MLPs run on the skinny-linear kernels and every adaLN modulation projection of a forward in one grouped launch."""
import math
from typing import Dict, List, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F  # noqa: N812
from torch.utils.checkpoint import checkpoint

from .. import dit as Dt
from .. import functional as Fn
from .. import ops
from .. import runtime as rt
from .unet import CrossEmbedLayer, SinusoidalPositionEmbedding
from .utils import prob_mask_like


class FeedForward(nn.Sequential):
    """dit.py:53-60 (parameter container; DiTBlock runs it as DiTFeedForwardFn)."""

    def __init__(self, dim: int, dim_mult: int = 4) -> None:
        inner_dim = dim * dim_mult
        super().__init__(nn.Linear(dim, inner_dim), nn.SiLU(), nn.Linear(inner_dim, dim))


class MultiHeadRMSNorm(nn.Module):
    """dit.py:63-70: F.normalize(x, dim=-1) * gamma[h] * sqrt(dim) on (B, H, N, dim).  Inside DiTAttention and JointAttention it is
    osuf_joint_qknorm_fwd; the stand-alone forward (plain torch on whatever device) exists for code written against the reference class."""

    def __init__(self, dim: int, heads: int) -> None:
        super().__init__()
        self.scale = dim ** 0.5
        self.gamma = nn.Parameter(torch.ones(heads, 1, dim))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return F.normalize(x, dim=-1) * self.gamma * self.scale


def _head_guard(dim: int, heads: int, dim_head: int) -> None:
    if heads * dim_head != dim:
        raise ValueError(f"DiT attention needs attn_heads * attn_dim_head == dim_h (it has no output projection): {heads} * {dim_head} != {dim}")
    if dim_head not in (16, 32, 64, 128):
        raise NotImplementedError(f"the HIP attention kernels cover head dims 16, 32, 64 and 128 (got attn_dim_head={dim_head})")


class DiTAttention(nn.Module):
    """dit.py:89-116.  forward(x: (B, N, dim)) -> (B, N, heads * dim_head)."""

    def __init__(self, dim: int, heads: int, dim_head: int, qk_norm: bool = True, context_len: int = 4096) -> None:
        super().__init__()
        self.heads, self.dim_head = heads, dim_head
        inner_dim = dim_head * heads
        self.to_qkv = nn.Linear(dim, inner_dim * 3, bias=False)
        self.q_norm = MultiHeadRMSNorm(dim_head, heads=heads) if qk_norm else nn.Identity()
        self.k_norm = MultiHeadRMSNorm(dim_head, heads=heads) if qk_norm else nn.Identity()
        self._cache = Fn.PackCache()

    def forward_rows(self, x: torch.Tensor) -> torch.Tensor:
        gq = self.q_norm.gamma if isinstance(self.q_norm, MultiHeadRMSNorm) else None
        gk = self.k_norm.gamma if isinstance(self.k_norm, MultiHeadRMSNorm) else None
        return Dt.dit_attention(x, self.to_qkv.weight, gq, gk, self._cache, self.heads, self.dim_head)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        rt.require_gpu(x)
        _head_guard(self.heads * self.dim_head, self.heads, self.dim_head)
        return self.forward_rows(rt.cast_rows(x.contiguous(), rt.compute_dtype(self.to_qkv.weight.dtype)))


class DiTBlock(nn.Module):
    """dit.py:119-159: x + gate_msa * attn(modulate(norm1(x))), then x + gate_ff * ff(modulate(norm2(x))).  The LayerNorms have no
    parameters; norm1 / norm2 are kept for the module tree (their eps, 1e-6, is the kernels')."""

    def __init__(self, dim_h: int, dim_h_mult: int = 4, attn_heads: int = 8, attn_dim_head: int = 64, attn_qk_norm: bool = True,
                 attn_context_len: int = 4096) -> None:
        super().__init__()
        self.modulation = nn.Sequential(nn.SiLU(), nn.Linear(dim_h, dim_h * 6, bias=True))
        self.norm1 = nn.LayerNorm(dim_h, elementwise_affine=False, eps=1e-6)
        self.attn = DiTAttention(dim_h, heads=attn_heads, dim_head=attn_dim_head, qk_norm=attn_qk_norm, context_len=attn_context_len)
        self.norm2 = nn.LayerNorm(dim_h, elementwise_affine=False, eps=1e-6)
        self.ff = FeedForward(dim_h, dim_h_mult)
        self.gradient_checkpointing = False
        self._cache = Fn.PackCache()

    def modulate_input(self, c: torch.Tensor) -> torch.Tensor:
        """Sequential(SiLU, Linear)(c) -> fp32 (B, 6 dim_h) on the skinny-linear kernels (DiT.forward runs all blocks' at once)."""
        lin = self.modulation[1]
        return rt.small_linear(c.float(), lin.weight, lin.bias, in_act=ops.ACT_SILU)

    def forward_body(self, x: torch.Tensor, mod: torch.Tensor) -> torch.Tensor:
        """rows (B, L, dim_h) and the modulation output (B, 6 dim_h) fp32 -> rows."""
        C = x.shape[-1]
        gate_msa, gate_ff = mod[:, 2 * C:3 * C], mod[:, 5 * C:6 * C]       # blocks: shift_msa, scale_msa, gate_msa, shift_ff, scale_ff, gate_ff
        link = Fn.ResLink()
        h = Dt.adaln(x, mod, 0, 1, link)
        h = self.attn.forward_rows(h)
        x = Fn.GateResFn.apply(h, gate_msa, x, None, link)
        link = Fn.ResLink()
        h = Dt.adaln(x, mod, 3, 4, link)
        h = Dt.DiTFeedForwardFn.apply(h, self.ff[0].weight, self.ff[0].bias, self.ff[2].weight, self.ff[2].bias, self._cache)
        return Fn.GateResFn.apply(h, gate_ff, x, None, link)

    def forward_rows(self, x: torch.Tensor, mod: torch.Tensor) -> torch.Tensor:
        if self.training and self.gradient_checkpointing:
            return checkpoint(self.forward_body, x, mod, use_reentrant=False)
        return self.forward_body(x, mod)

    def forward(self, x: torch.Tensor, c: torch.Tensor) -> torch.Tensor:
        """x: (B, N, dim_h), c: (B, dim_h) -> (B, N, dim_h) (the reference's API)."""
        rt.require_gpu(x)
        _head_guard(x.shape[-1], self.attn.heads, self.attn.dim_head)
        x = rt.cast_rows(x.contiguous(), rt.compute_dtype(self.ff[0].weight.dtype))
        return self.forward_rows(x, self.modulate_input(c))


class FinalLayer(nn.Module):
    """dit.py:73-86."""

    def __init__(self, dim_h: int) -> None:
        super().__init__()
        self.norm = nn.LayerNorm(dim_h, elementwise_affine=False, eps=1e-6)
        self.modulation = nn.Sequential(nn.SiLU(), nn.Linear(dim_h, dim_h * 2, bias=True))
        self.linear = nn.Linear(dim_h, dim_h)
        self._cache = Fn.PackCache()

    def forward_rows(self, x: torch.Tensor, mod: torch.Tensor) -> torch.Tensor:
        h = Dt.adaln(x, mod, 0, 1)
        return Fn.ConvFn.apply(h, self.linear.weight, self.linear.bias, self._cache, "same")

    def forward(self, x: torch.Tensor, c: torch.Tensor) -> torch.Tensor:
        rt.require_gpu(x)
        x = rt.cast_rows(x.contiguous(), rt.compute_dtype(self.linear.weight.dtype))
        lin = self.modulation[1]
        return self.forward_rows(x, rt.small_linear(c.float(), lin.weight, lin.bias, in_act=ops.ACT_SILU))


class _TransformerBackbone:
    """What DiT and MMDiT share; no module, parameter or buffer of its own.  A backbone brings null_cond, embed_time(t) and the hooks
    _embed_cond(c) (its conditioning MLP) and _embed_audio(a) (its MLP of the audio statistics): fp32 (B, dim_h) each."""

    @staticmethod
    def _basic_init(module: nn.Module) -> None:
        if isinstance(module, (nn.Linear, nn.Conv1d)):
            nn.init.xavier_uniform_(module.weight)
            if module.bias is not None:
                nn.init.zeros_(module.bias)

    def set_gradient_checkpointing(self, value: bool) -> None:
        """dit.py:247-251, mmdit.py:331-335 (same log line per module)."""
        for name, module in self.named_modules():
            if hasattr(module, "gradient_checkpointing"):
                module.gradient_checkpointing = value
                print(f"Set gradient checkpointing to {value} for {name}")

    def forward_with_cond_scale(self, *args: List, cond_scale: float = 1.0, **kwargs: Dict) -> torch.Tensor:
        """dit.py:253-260, mmdit.py:337-344."""
        logits = self(*args, **kwargs)
        if cond_scale == 1.0:
            return logits
        null_logits = self(*args, **kwargs, cond_drop_prob=1.0)
        return null_logits + (logits - null_logits) * cond_scale

    @staticmethod
    def _ff(x: torch.Tensor, ff: nn.Sequential) -> torch.Tensor:
        """Sequential(Linear, SiLU, Linear) on the skinny-linear kernels."""
        h = rt.small_linear(x, ff[0].weight, ff[0].bias)
        return rt.small_linear(h, ff[2].weight, ff[2].bias, in_act=ops.ACT_SILU)

    def _cond(self, c: torch.Tensor, keep: torch.Tensor) -> torch.Tensor:
        return torch.where(keep[:, None], self._embed_cond(c), self.null_cond.float()[None, :].expand(keep.shape[0], -1))

    def embed(self, a: torch.Tensor, t: torch.Tensor, c: torch.Tensor, cond_drop_prob: float) -> torch.Tensor:
        """The conditioning vector where(keep, mlp_cond(c), null_cond) + mlp_time(t) + the audio statistics' MLP (dit.py:274-285,
        mmdit.py:355-378), fp32 (B, dim_h); keep is drawn here.  a: the audio before any padding."""
        keep = prob_mask_like((a.shape[0],), 1.0 - cond_drop_prob, device=a.device)
        return self._cond(c, keep) + self.embed_time(t) + self._embed_audio(a)

    def embed_static(self, a: torch.Tensor, c: torch.Tensor, keep: torch.Tensor) -> torch.Tensor:
        """The part of embed() that does not depend on t, fp32 (B, dim_h).  keep: bool (B,).  A sampler computes it once per call and adds
        embed_time(t) per step."""
        return self._cond(c, keep) + self._embed_audio(a)

    @staticmethod
    def _modulations(cvec: torch.Tensor, lins: List[nn.Linear]) -> List[torch.Tensor]:
        """The backbone's Sequential(SiLU, Linear) projections of c: one grouped launch (runtime.film_prepare), else one each."""
        grouped = rt.film_prepare(cvec, lins)
        outs = []
        for lin in lins:
            m = rt.film_take(cvec, lin) if grouped else None
            outs.append(m if m is not None else rt.small_linear(cvec, lin.weight, lin.bias, in_act=ops.ACT_SILU))
        rt.film_clear()
        return outs


class DiT(_TransformerBackbone, nn.Module):
    """dit.py:162-292."""

    def __init__(self, dim_in_x: int, dim_in_a: int, dim_in_c: int, dim_h: int, dim_h_mult: int = 4, depth: int = 12,
                 cross_embed_kernel_sizes: Tuple[int] = (3, 7, 15), attn_heads: int = 8, attn_dim_head: int = 64, attn_qk_norm: bool = True,
                 attn_context_len: int = 4096) -> None:
        super().__init__()
        _head_guard(dim_h, attn_heads, attn_dim_head)
        self.dim_in_x = dim_in_x
        self.preprocess = CrossEmbedLayer(dim_in_x + dim_in_a, dim_h, cross_embed_kernel_sizes)
        self.postprocess = nn.Conv1d(dim_h, dim_in_x, 1, bias=False)
        self.mlp_time = nn.Sequential(SinusoidalPositionEmbedding(dim_h), nn.Linear(dim_h, dim_h, bias=False), nn.SiLU(),
                                      nn.Linear(dim_h, dim_h, bias=False))
        self.mlp_cond = nn.Sequential(nn.Linear(dim_in_c, dim_h), nn.SiLU(), nn.Linear(dim_h, dim_h))
        self.null_cond = nn.Parameter(torch.randn(dim_h))
        self.feature_extractor_a = nn.Linear(dim_in_a * 2, dim_h)
        self.mlp_audio = nn.Sequential(nn.Linear(dim_h, dim_h), nn.SiLU(), nn.Linear(dim_h, dim_h))
        self.blocks = nn.ModuleList([
            DiTBlock(dim_h, dim_h_mult=dim_h_mult, attn_heads=attn_heads, attn_dim_head=attn_dim_head, attn_qk_norm=attn_qk_norm,
                     attn_context_len=attn_context_len) for _ in range(depth)])
        self.final = FinalLayer(dim_h)
        self._stem_cache = Fn.PackCache()
        self._post_cache = Fn.PackCache()
        self.initialize_weights()

    def initialize_weights(self) -> None:
        """dit.py:218-245: xavier-uniform Linear / Conv1d weights and zero biases, N(0, 0.02) embedders, zeroed adaLN / final modulation
        and postprocess."""
        self.apply(self._basic_init)
        for m in (self.mlp_time[1], self.mlp_time[3], self.mlp_cond[0], self.mlp_cond[2], self.mlp_audio[0], self.mlp_audio[2]):
            nn.init.normal_(m.weight, std=0.02)
        for block in self.blocks:
            nn.init.zeros_(block.modulation[1].weight)
            nn.init.zeros_(block.modulation[1].bias)
        nn.init.zeros_(self.final.modulation[1].weight)
        nn.init.zeros_(self.final.modulation[1].bias)
        nn.init.zeros_(self.postprocess.weight)

    # -- pieces ---------------------------------------------------------------------------------------------------
    def _stem(self, x: torch.Tensor, a: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
        """preprocess(cat(x, a)) -> rows (B, L, dim_h).  dim_in_x + dim_in_a = 102 input channels: the input and the merged stem weight
        are zero-padded to the next multiple of 8 (the tap-GEMM's K), which adds exact zeros."""
        pre = self.preprocess
        xa = torch.cat([x.float(), a.float()], dim=1)
        cin = xa.shape[1]
        cpad = (cin + 7) // 8 * 8
        w, b = pre._merged()
        if cpad != cin:
            xa = F.pad(xa, (0, 0, 0, cpad - cin))
            w = F.pad(w, (0, 0, 0, cpad - cin))
        rows = Fn.RowsFromNCLFn.apply(xa.contiguous(), dtype, cpad, 1)
        return Fn.ConvFn.apply(rows, w, b, self._stem_cache, "same", ("dit_stem", *[c.weight for c in pre.convs]))

    def _embed_cond(self, c: torch.Tensor) -> torch.Tensor:
        """mlp_cond(c)."""
        return self._ff(c.float(), self.mlp_cond)

    def _embed_audio(self, a: torch.Tensor) -> torch.Tensor:
        """mlp_audio(feature_extractor_a(stat_pool(a))) (dit.py:275-279)."""
        fe = self.feature_extractor_a
        return self._ff(rt.small_linear(Dt.stat_pool(a), fe.weight, fe.bias), self.mlp_audio)

    def embed_time(self, t: torch.Tensor) -> torch.Tensor:
        """mlp_time(t), fp32 (B, dim_h)."""
        te = rt.small_linear(self.mlp_time[0](t), self.mlp_time[1].weight, None)
        return rt.small_linear(te, self.mlp_time[3].weight, None, in_act=ops.ACT_SILU)

    def encode_audio(self, a: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
        """The audio's share of the stem, rows (B, L, dim_h): preprocess is linear in cat(x, a), so its audio input channels (and the bias)
        are applied once per sample call; encode_x adds the map channels' share per step.  Differs from _stem by one rounding of this
        partial sum to the compute dtype and the order of the sum."""
        pre = self.preprocess
        w, b = pre._merged()
        nx = self.dim_in_x
        rows = Fn.RowsFromNCLFn.apply(a.float().contiguous(), dtype, a.shape[1], 1)
        return Fn.ConvFn.apply(rows, w[:, nx:].contiguous(), b, self._stem_cache, "same", ("dit_stem_a", *[c.weight for c in pre.convs]))

    def encode_x(self, x: torch.Tensor, a_rows: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
        """preprocess(cat(x, a)) as rows from the audio's share (encode_audio): the map channels' tap GEMM with a_rows added in its epilogue."""
        pre = self.preprocess
        nx = self.dim_in_x
        npad = (nx + 7) // 8 * 8
        w = F.pad(pre._merged()[0][:, :nx], (0, 0, 0, npad - nx))
        rows = Fn.RowsFromNCLFn.apply(F.pad(x.float(), (0, 0, 0, npad - nx)).contiguous(), dtype, npad, 1)
        return Fn.conv_forward(rows, w, None, self._stem_cache, "same", ("dit_stem_x", *[c.weight for c in pre.convs]), residual=a_rows)

    def denoise_rows(self, h: torch.Tensor, cvec: torch.Tensor, n: int) -> torch.Tensor:
        """The stem's rows (B, L, dim_h) and the conditioning vector (fp32 (B, dim_h), contiguous) -> the prediction (B, dim_in_x, n)."""
        mods = self._modulations(cvec, [b.modulation[1] for b in self.blocks] + [self.final.modulation[1]])      # depth + 1
        for block, mod in zip(self.blocks, mods[:-1]):
            h = block.forward_rows(h, mod)
        h = self.final.forward_rows(h, mods[-1])
        nx = self.dim_in_x
        npad = (nx + 7) // 8 * 8
        w = F.pad(self.postprocess.weight[:, :, 0], (0, 0, 0, npad - nx))
        y = Fn.ConvFn.apply(h, w, None, self._post_cache, "same", ("post", self.postprocess.weight))
        return Fn.NCLFromRowsFn.apply(y, nx)[:, :, :n]

    def sample_rows(self, x: torch.Tensor, a_rows: torch.Tensor, cvec: torch.Tensor, n: int, dtype: torch.dtype) -> torch.Tensor:
        """A sampler's step: the iterate x (B, dim_in_x, n), encode_audio's rows and the conditioning vector -> the prediction."""
        return self.denoise_rows(self.encode_x(x, a_rows, dtype), cvec, n)

    def forward(self, x: torch.Tensor, a: torch.Tensor, t: torch.Tensor, c: torch.Tensor, cond_drop_prob: float = 0.0) -> torch.Tensor:
        rt.require_gpu(x)
        n = x.shape[-1]
        dtype = rt.compute_dtype(self.postprocess.weight.dtype)
        h = self._stem(x, a, dtype)
        cvec = self.embed(a, t, c, cond_drop_prob).contiguous()
        return self.denoise_rows(h, cvec, n)
