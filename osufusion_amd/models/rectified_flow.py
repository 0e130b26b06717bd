"""HIP-backed mirror of osu_fusion/models/rectified_flow.py: ``OsuFusion`` (flow-matching variant) with the same ctor,
``forward`` (training loss), ``sample`` (fixed-grid midpoint ODE + classifier-free guidance), ``set_full_bf16`` and the
``unet`` / ``sample_timesteps`` attributes.

``_Flow`` is the objective, written once for both backbone families (models/base.py): ``forward`` / ``loss_with`` and the sampler, the
guided flow f(t, y) over the family's denoiser closure handed to osufusion_amd/ode.ode_loop (the reference's midpoint loop by default).
``OsuFusion`` is that objective on the UNet family.
"""
import math
from typing import Optional, Tuple

import torch

from .. import guidance, inpaint, ode, ops
from .. import runtime as rt
from .base import _UNetOsuFusion
from .diffusion import _MSEFn


def cosmap(t: torch.Tensor) -> torch.Tensor:
    """rectified_flow.py:15-16."""
    return 1.0 - (1.0 / (torch.tan(math.pi / 2 * t) + 1))


class _Flow:
    """The rectified-flow objective of a base._OsuFusion family: the training loss and the ODE sampler.  The family's constructor sets
    `sample_timesteps`."""
    last_ode_stats = None

    def _sample(self, a, c, x, cond_scale, keep_region=None, wp=None, gd: Optional[guidance.Guidance] = None, solver: Optional[dict] = None):
        x = self._start(a, x)
        b, device = a.shape[0], a.device
        cfg = cond_scale != 1.0
        gd = gd if cfg else None                           # cond_scale == 1: nothing to control
        ones = torch.ones(b, dtype=torch.float32, device=device)
        with self._dtype_ctx():
            den = self._make_denoiser(a, c, cfg, wp)

            def f(t: float, y: torch.Tensor) -> torch.Tensor:
                tt = torch.full((2 * b if cfg else b,), t, dtype=torch.float32, device=device)
                if gd is not None and gd.bounded and not gd.contains(guidance.flow_log_snr(t)):
                    return den(y, tt, False)               # outside the interval: the conditional b rows are the flow
                out = den(y, tt)
                if gd is not None and gd.phi > 0.0:
                    out = ops.cfg_rescale(out[:b], out[b:], cond_scale, gd.phi)[0]
                elif cfg:                                  # null + (cond - null) * s  ==  (1 - s) * null + s * cond
                    out = ops.axpby_rows(out[b:].contiguous(), out[:b].contiguous(), ones * (1.0 - cond_scale), ones * cond_scale)
                return out

            times = torch.linspace(0.0, 1.0, self.sample_timesteps).tolist()
            x, self.last_ode_stats = ode.ode_loop(f, x, times, ones, keep_region=keep_region, **(solver or {}))
        return x

    def forward(self, x: torch.Tensor, a: torch.Tensor, c: torch.Tensor, orig_len: Optional[torch.Tensor] = None) -> torch.Tensor:
        assert x.shape[-1] == a.shape[-1], "x and a must have the same number of sequence length"
        rt.require_gpu(x)
        noise = torch.randn_like(x, device=x.device)
        times = torch.rand(x.shape[0], device=x.device)
        return self.loss_with(x, a, c, noise, times, orig_len)

    def loss_with(self, x, a, c, noise, times, orig_len=None, cond_drop_prob: Optional[float] = None) -> torch.Tensor:
        """forward() with the RNG draws passed in (parity tests, benchmarks)."""
        p = self.cond_drop_prob if cond_drop_prob is None else cond_drop_prob
        x, noise = x.float().contiguous(), noise.float().contiguous()
        t = cosmap(times.float())
        ones = torch.ones_like(t)
        with self._dtype_ctx():
            x_noisy = ops.axpby_rows(x, noise, t.contiguous(), (1 - t).contiguous())
            flow = ops.axpby_rows(x, noise, ones, -ones)
            pred = self.unet(x_noisy, a, times.float(), c, cond_drop_prob=p)
        return _MSEFn.apply(pred, flow, orig_len)


class OsuFusion(_Flow, _UNetOsuFusion):
    def __init__(self, dim_h: int, dim_h_mult: Tuple[int] = (1, 2, 3, 4), num_layer_blocks: Tuple[int] = (3, 3, 3, 3),
                 num_middle_transformers: int = 3, cross_embed_kernel_sizes: Tuple[int] = (3, 7, 15), attn_dim_head: int = 64,
                 attn_heads: int = 16, attn_kv_heads: int = 1, attn_context_len: int = 4096, cond_drop_prob: float = 0.5,
                 sampling_timesteps: int = 16) -> None:
        super().__init__(dim_h, dim_h_mult, num_layer_blocks, num_middle_transformers, cross_embed_kernel_sizes, attn_dim_head, attn_heads,
                         attn_kv_heads, attn_context_len, cond_drop_prob)
        self.sample_timesteps = sampling_timesteps

    @torch.inference_mode()
    def sample(self, a: torch.Tensor, c: torch.Tensor, x: Optional[torch.Tensor] = None, cond_scale: float = 2.0) -> torch.Tensor:
        """rectified_flow.py:57-79.  Same restructuring as the DDIM sampler: audio code computed once, conditional + null
        branches as one batch of 2B; 2 * (S - 1) UNet evaluations.  Bit-reproducible (ops.reproducible_mode), as the DDIM sampler.  The
        signature is the reference's (tests/test_host_logic.py holds it there); masked generation is `sample_masked`."""
        with ops.reproducible_mode(True):
            return self._sample(a, c, x, cond_scale)

    @torch.inference_mode()
    def sample_masked(self, a: torch.Tensor, c: torch.Tensor, x: Optional[torch.Tensor] = None, cond_scale: float = 2.0,
                      known: Optional[torch.Tensor] = None, known_mask: Optional[torch.Tensor] = None, method: str = "midpoint",
                      rtol: float = 1e-5, atol: float = 1e-5, first_step: Optional[float] = None, max_steps: int = 1000) -> torch.Tensor:
        """sample() with the keywords the transformer models' sample() takes (the reference's signature of sample() is kept as it is).
        known (B, 6, n) and known_mask ((n,), (B, n) or (B, 1, n); 1 / True = keep), both or neither: masked generation (ode.flow_levels,
        osufusion_amd/inpaint.py).  The iterate at ODE time t is t x_0 + (1 - t) noise -- the sampler's own state, not the cosmap position of
        training -- so every state handed to the UNet is blended at (t, 1 - t): the start iterate at (0, 1), the midpoint state at
        t0 + dt / 2, the end of an interval at t1, and the end of the last interval by the exact blend (`known` bit for bit where the mask is
        1).  The noise is one fixed tensor, a clone of the start iterate: nothing new is drawn.  With both None: the unmasked sampler's bits.
        method, rtol, atol, first_step, max_steps: the ODE solver (osufusion_amd/ode.py): "euler", "midpoint" (the default: sample()'s launches
        and bits) and "rk4" on the sampler's grid, "bosh3" and "dopri5" adaptive from rtol / atol; an adaptive method with known / known_mask
        raises ValueError.  The call's evaluations and accepted / rejected steps are left in self.last_ode_stats."""
        masked = inpaint.check_pair(known, known_mask)
        solver = dict(method=method, rtol=rtol, atol=atol, first_step=first_step, max_steps=max_steps)
        ode.check_options(**solver)
        with ops.reproducible_mode(True):
            return self._sample(a, c, x, cond_scale, (known, known_mask) if masked else None, solver=solver)
