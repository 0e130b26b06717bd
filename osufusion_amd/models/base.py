"""What the models share.  ``_OsuFusion`` is the base of both backbone families: the compute-dtype switch, the start iterate and ``_run``, the
one loop of the diffusion samplers, over the family's one hook ``_denoiser(a, c, cfg) -> f(x, t)``.  ``_UNetOsuFusion`` is the UNet family:
the backbone built once and its denoiser closure (transformer_diffusion._TransformerOsuFusion is the other family).  The objectives are
written once each and mixed into either family: diffusion._DDIM and rectified_flow._Flow."""
from dataclasses import dataclass
from typing import Callable, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F  # noqa: N812

from .. import guidance, inpaint, ops
from .. import runtime as rt
from ..modules.unet import UNet

TOTAL_DIM = 6        # library/osu/data/encode.py:10-26
AUDIO_DIM = 96       # scripts/dataset_creator.py:22-24
CONTEXT_DIM = 5      # scripts/dataset_creator.py:25


@dataclass
class _Steps:
    """What a sampler tells _OsuFusion._run.  S = the steps of a full run."""
    coef: torch.Tensor                  # (S, b, cols): step i's coefficient rows, also the levels of the blends
    t_in: torch.Tensor                  # (S, nb): step i's time input of the denoiser
    step: Callable                      # step(i, row, x, cond, null, noise, state) -> (x, state); row = coef[i]; state is None on the first call
    draw_steps: int                     # steps i < draw_steps draw a torch.randn of the iterate's shape for `noise`, the others get None
    fresh: bool                         # the level blends draw fresh noise (else: one fixed tensor, a clone of the start iterate)
    start_cols: Tuple[int, int]         # columns (a, s) of coef[0] for the level blend of the start iterate
    step_cols: Tuple[int, int]          # columns (a, s) of coef[i] for the level blend after step i
    last: int                           # the step that ends a full run: the exact blend instead of a level blend, and no resampling
    resample: int = 1                   # the ancestral sampler's RePaint passes per step, with the factors of the way back one level:
    k_r: Optional[torch.Tensor] = None  # (S, b) x = k_r x + k_g z
    k_g: Optional[torch.Tensor] = None
    log_snr: Optional[Callable] = None  # log_snr() -> S host floats, step i's log-SNR for a guidance interval; called at most once per run


class _OsuFusion(nn.Module):
    """A backbone as `unet`, the compute-dtype switch and the sampling loop.  A family gives `_denoiser`."""

    def __init__(self, cond_drop_prob: float) -> None:
        super().__init__()
        self.cond_drop_prob = cond_drop_prob
        self._full_bf16 = False

    def set_full_bf16(self) -> None:
        """diffusion.py:56-57 casts the UNet weights to bf16; here the fp32 masters are kept and every kernel computes in
        bf16 (bf16 MFMA operands and activations) -- the same arithmetic, without losing the master weights."""
        self._full_bf16 = True

    def _dtype_ctx(self):
        return rt.forced_compute_dtype(torch.bfloat16 if self._full_bf16 else None)

    def _denoiser(self, a: torch.Tensor, c: torch.Tensor, cfg: bool):
        """-> f(x (b, 6, n) fp32, t (nb,)) = the prediction (nb, 6, n), nb = 2b with guidance (conditional rows first), else b.  Everything
        that does not depend on the step is computed here, once per sample call."""
        raise NotImplementedError

    def _make_denoiser(self, a: torch.Tensor, c: torch.Tensor, cfg: bool, wp=None):
        """The closure every sampling loop calls.  Windows (wp) are the transformer family's."""
        assert wp is None
        return self._denoiser(a, c, cfg)

    def _start(self, a: torch.Tensor, x: Optional[torch.Tensor]) -> torch.Tensor:
        rt.require_gpu(a)
        if x is None:
            x = torch.randn((a.shape[0], TOTAL_DIM, a.shape[-1]), device=a.device)
        rt.require_gpu(x)
        return x.float().contiguous()

    def _run(self, describe, a, c, x, cond_scale, stop_after, keep_region=None, wp=None, gd: Optional[guidance.Guidance] = None, wrap=None):
        """The sampling loop of the diffusion samplers; describe(b, cfg, cond_scale, device) -> the sampler's _Steps.  Draws, in this order:
        the start iterate (x None), the start blend's noise; then per pass of a step its own noise, its level blend's noise, the resample
        draw -- each only where the sampler has one.  Per pass: the denoiser, the step, the blend of the known region, the resample.
        gd (guidance.plan; None: the loop as it was before it): with an interval, which steps are guided is decided here, before the loop,
        from the sampler's per-step log-SNR -- the one host read; the passes of a step share its decision.  An unguided step calls the
        denoiser on the conditional b rows and hands (pred, None) to the step; with gd.phi > 0 a guided step hands it
        (ops.cfg_rescale(cond, null), None).
        wrap(one_pass, steps) -> a callable that stands in for one_pass(i, t, row, x, state) -> (x, state), the denoiser call and the step of
        one pass (models/diffusion.OsuFusion replays it from a hipGraph); the blends and the resample stay in this loop."""
        x = self._start(a, x)
        b, device = a.shape[0], a.device
        cfg = cond_scale != 1.0
        sp = describe(b, cfg, cond_scale, device)
        total = sp.coef.shape[0]
        steps = total if stop_after is None else min(stop_after, total)
        gd = gd if cfg else None                           # cond_scale == 1: nothing to control
        guided = guidance.guided_calls(sp.log_snr(), gd, cond_scale) if gd is not None and gd.bounded else None
        blender = inpaint.Blender(*keep_region, x, fresh=sp.fresh) if keep_region is not None else None
        if blender is not None and steps > 0:
            x = blender.level(x, sp.coef[0], *sp.start_cols)
        state = None
        with self._dtype_ctx():
            f = self._make_denoiser(a, c, cfg, wp)

            def one_pass(i, t, row, x, state):
                if guided is not None and not guided[i]:
                    cond, null = f(x, t, False), None
                else:
                    pred = f(x, t)
                    cond, null = pred[:b], pred[b:] if cfg else None
                    if gd is not None and gd.phi > 0.0:
                        cond, null = ops.cfg_rescale(cond, null, cond_scale, gd.phi)[0], None
                noise = torch.randn(x.shape, device=device) if i < sp.draw_steps else None
                return sp.step(i, row, x, cond, null, noise, state)
            run_pass = one_pass if wrap is None else wrap(one_pass, steps)
            for i in range(steps):
                passes = sp.resample if i < sp.last else 1
                for u in range(passes):
                    x, state = run_pass(i, sp.t_in[i], sp.coef[i], x, state)
                    if blender is not None:
                        x = blender.exact(x) if i == sp.last else blender.level(x, sp.coef[i], *sp.step_cols)
                    if u < passes - 1:
                        x = ops.axpby_rows(x, torch.randn(x.shape, device=device), sp.k_r[i], sp.k_g[i])
        return x


class _UNetOsuFusion(_OsuFusion):
    """The UNet family: the reference's backbone and constructor keywords."""

    def __init__(self, dim_h, dim_h_mult, num_layer_blocks, num_middle_transformers, cross_embed_kernel_sizes, attn_dim_head, attn_heads,
                 attn_kv_heads, attn_context_len, cond_drop_prob) -> None:
        super().__init__(cond_drop_prob)
        self.unet = UNet(dim_in_x=TOTAL_DIM, dim_in_a=AUDIO_DIM, dim_in_c=CONTEXT_DIM, dim_h=dim_h, dim_h_mult=dim_h_mult,
                         num_layer_blocks=num_layer_blocks, num_middle_transformers=num_middle_transformers,
                         cross_embed_kernel_sizes=cross_embed_kernel_sizes, attn_dim_head=attn_dim_head, attn_heads=attn_heads,
                         attn_kv_heads=attn_kv_heads, attn_context_len=attn_context_len)

    def _denoiser(self, a: torch.Tensor, c: torch.Tensor, cfg: bool):
        """Once, here: the padding to the UNet's stride, the audio code (it does not depend on t or x) and embed_cond on [keep; ~keep], the
        conditional and null branches of classifier-free guidance as one batch of 2b.  Per call of f: the iterate doubled and padded
        with -1, its stem, and the UNet body cut back to n frames."""
        unet = self.unet
        b, n = a.shape[0], a.shape[-1]
        depth = len(unet.down_layers)
        pad_len = (2 ** depth - (n % (2 ** depth))) % (2 ** depth)
        dtype = rt.compute_dtype(unet.final_conv.weight.dtype)
        a_rows = unet.encode_audio(a, pad_len, dtype)
        keep = torch.ones(b, dtype=torch.bool, device=a.device)
        if cfg:
            a_rows = torch.cat([a_rows, a_rows], 0)
            ce = unet.embed_cond(torch.cat([c, c], 0), torch.cat([keep, ~keep], 0))
        else:
            ce = unet.embed_cond(c, keep)

        def f(x: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
            xin = torch.cat([x, x], 0) if cfg else x
            x_rows = unet.init_x.forward_rows(F.pad(xin, (0, pad_len), value=-1.0), dtype)
            return unet.denoise_rows(x_rows, a_rows, unet.embed_time(t), ce)[:, :, :n].contiguous()
        return f
