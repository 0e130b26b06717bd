"""HIP-backed mirror of osu_fusion/models/diffusion.py: ``OsuFusion`` with the same ctor, ``forward`` (training loss),
``sample`` (DDIM + classifier-free guidance), ``set_full_bf16`` and the ``unet`` / ``sampling_timesteps`` attributes.

The DDIM arithmetic of diffusers==0.29.2's ``DDIMScheduler`` (absent from this image) is restated in ``DDIMSchedule``
(linear betas 1e-4..0.02, 1000 train steps, "leading" spacing, eta=0, epsilon prediction, clip_sample=True,
set_alpha_to_one=True) and executed by the osuf_axpby_rows / osuf_ddim_step kernels.

``_DDIM`` is the objective, written once for both backbone families (models/base.py): ``forward`` / ``loss_with`` and the description of the
DDIM sampler that base._OsuFusion._run loops over.  ``OsuFusion`` is that objective on the UNet family; its sampler is _run over the UNet's
denoiser closure, and ``use_hip_graph`` wraps the pass of that loop in a captured hipGraph (``_graph_pass``).
"""
from typing import Optional, Tuple

import torch

from .. import guidance, inpaint, ops
from .. import runtime as rt
from .base import AUDIO_DIM, CONTEXT_DIM, TOTAL_DIM, _Steps, _UNetOsuFusion  # noqa: F401  (the dims are imported from here)


class DDIMSchedule:
    """Restatement of the DDIMScheduler calls made at diffusion.py:48-51,71,75,96."""

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 1e-4, beta_end: float = 0.02) -> None:
        self.num_train_timesteps = num_train_timesteps
        betas = torch.linspace(beta_start, beta_end, num_train_timesteps, dtype=torch.float32)
        self.alphas_cumprod = torch.cumprod(1.0 - betas, dim=0)
        self.final_alpha_cumprod = torch.tensor(1.0)
        self.timesteps = torch.arange(num_train_timesteps).flip(0)
        self.num_inference_steps: Optional[int] = None
        self._dev = {}

    def _acp(self, device) -> torch.Tensor:
        key = str(device)
        if key not in self._dev:
            self._dev[key] = self.alphas_cumprod.to(device)
        return self._dev[key]

    def set_timesteps(self, num_inference_steps: int) -> None:
        self.num_inference_steps = num_inference_steps
        ratio = self.num_train_timesteps // num_inference_steps
        self.timesteps = (torch.arange(num_inference_steps) * ratio).flip(0).to(torch.int64)

    def add_noise(self, x: torch.Tensor, noise: torch.Tensor, timesteps: torch.Tensor) -> torch.Tensor:
        acp = self._acp(x.device)[timesteps]
        return ops.axpby_rows(x.contiguous().float(), noise.contiguous().float(), (acp ** 0.5).contiguous(), ((1 - acp) ** 0.5).contiguous())

    def step_coefficients(self, t: int) -> Tuple[float, float, float, float]:
        prev_t = t - self.num_train_timesteps // self.num_inference_steps
        a_t = self.alphas_cumprod[t]
        a_prev = self.alphas_cumprod[prev_t] if prev_t >= 0 else self.final_alpha_cumprod
        return (float((1 - a_t) ** 0.5), float(a_t ** 0.5), float(a_prev ** 0.5), float((1 - a_prev) ** 0.5))


class _MSEFn(torch.autograd.Function):
    """F.mse_loss(pred, target, 'none') (* length mask).sum() / count   (diffusion.py:101-111) in one pass.  weight (optional, per-sample
    fp32 (B,), min-SNR-gamma): sum_b w_b sum_{d, l < len_b} (pred - target)^2 over the same count (osuf_mse_w); None is the unweighted loss."""

    @staticmethod
    def forward(ctx, pred, target, orig_len, weight=None):
        acc, grad = ops.mse(pred.contiguous(), target.contiguous(), orig_len, pred.requires_grad, weight)
        B, Dc, L = pred.shape
        if orig_len is not None:
            count = orig_len.to(pred.device).clamp(max=L).sum().double() * Dc
        else:
            count = torch.tensor(float(B * Dc * L), dtype=torch.float64, device=pred.device)
        ctx.save_for_backward(grad if grad is not None else acc, count)
        return (acc / count).float().reshape(())

    @staticmethod
    def backward(ctx, g):
        grad, count = ctx.saved_tensors
        return grad * (g / count.float()), None, None, None      # (a trailing None for an omitted weight is dropped by autograd)


class _DDIM:
    """The discrete DDIM objective of a base._OsuFusion family: the training loss and the sampler's description."""

    def _init_ddim(self, train_timesteps: int, sampling_timesteps: int) -> None:
        self.scheduler = DDIMSchedule(num_train_timesteps=train_timesteps)
        self.train_timesteps = train_timesteps
        self.sampling_timesteps = sampling_timesteps
        self.stop_after: Optional[int] = None

    def _ddim(self, b, cfg, cond_scale, device) -> _Steps:
        self.scheduler.set_timesteps(self.sampling_timesteps)
        steps = self.scheduler.timesteps.tolist()
        coef = torch.tensor([[self.scheduler.step_coefficients(t)] * b for t in steps], dtype=torch.float32, device=device)
        t_in = torch.tensor([[t] * (2 * b if cfg else b) for t in steps], dtype=torch.int64, device=device)

        def step(i, row, x, cond, null, noise, state):
            return ops.ddim_step(x, cond, null, cond_scale, row), None
        return _Steps(coef, t_in, step, draw_steps=0, fresh=False, start_cols=(1, 0), step_cols=(2, 3), last=self.sampling_timesteps - 1,
                      log_snr=lambda: guidance.ddim_log_snr(self.scheduler.alphas_cumprod, steps))

    def forward(self, x: torch.Tensor, a: torch.Tensor, c: torch.Tensor, orig_len: Optional[torch.Tensor] = None) -> torch.Tensor:
        assert x.shape[-1] == a.shape[-1], "x and a must have the same number of sequence length"
        rt.require_gpu(x)
        noise = torch.randn_like(x, device=x.device)
        timesteps = torch.randint(0, self.scheduler.num_train_timesteps, (x.shape[0],), dtype=torch.int64, device=x.device)
        return self.loss_with(x, a, c, noise, timesteps, orig_len)

    def loss_with(self, x, a, c, noise, timesteps, orig_len=None, cond_drop_prob: Optional[float] = None) -> torch.Tensor:
        """forward() with the RNG draws passed in (parity tests, benchmarks)."""
        p = self.cond_drop_prob if cond_drop_prob is None else cond_drop_prob
        with self._dtype_ctx():
            x_noisy = self.scheduler.add_noise(x, noise, timesteps)
            pred = self.unet(x_noisy, a, timesteps, c, cond_drop_prob=p)
        return _MSEFn.apply(pred, noise.float(), orig_len)


class OsuFusion(_DDIM, _UNetOsuFusion):
    def __init__(self, dim_h: int, dim_h_mult: Tuple[int] = (1, 2, 3, 4), num_layer_blocks: Tuple[int] = (3, 3, 3, 3),
                 num_middle_transformers: int = 3, cross_embed_kernel_sizes: Tuple[int] = (3, 7, 15), attn_dim_head: int = 64,
                 attn_heads: int = 16, attn_kv_heads: int = 1, attn_context_len: int = 4096, cond_drop_prob: float = 0.5,
                 train_timesteps: int = 1000, sampling_timesteps: int = 35) -> None:
        super().__init__(dim_h, dim_h_mult, num_layer_blocks, num_middle_transformers, cross_embed_kernel_sizes, attn_dim_head, attn_heads,
                         attn_kv_heads, attn_context_len, cond_drop_prob)
        self._init_ddim(train_timesteps, sampling_timesteps)
        self.use_hip_graph = False       # capture one DDIM step (2B-batched CFG forward + fused step kernel) in a hipGraph
        # GroupNorm statistics / GlobalContext pooling by fixed-order reductions while sampling: the same (a, c, x) gives the same
        # beatmap bit for bit, eager or graph-replayed (costs one extra read of each conv output; False = the training kernels)
        self.reproducible_sampling = True

    @torch.inference_mode()
    def sample(self, a: torch.Tensor, c: torch.Tensor, x: Optional[torch.Tensor] = None, cond_scale: float = 7.0) -> torch.Tensor:
        """diffusion.py:59-77.  Same outputs, restructured: the audio code is computed once (it does not depend on t or x),
        the conditional and null branches of classifier-free guidance run as one batch of 2B, and the guidance combine is
        fused into the DDIM-step kernel.  (Attribute `stop_after`, None by default and absent from the reference: return the
        iterate after that many of the sampling_timesteps steps -- lets tests check single steps of a long schedule.)  The signature is
        the reference's (tests/test_host_logic.py holds it there); masked generation is `sample_masked`."""
        with ops.reproducible_mode(self.reproducible_sampling):
            return self._sample(a, c, x, cond_scale)

    @torch.inference_mode()
    def sample_masked(self, a: torch.Tensor, c: torch.Tensor, x: Optional[torch.Tensor] = None, cond_scale: float = 7.0,
                      known: Optional[torch.Tensor] = None, known_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """sample() with the keywords the transformer models' sample() takes (the reference's signature of sample() is kept as it is).
        known (B, 6, n) and known_mask ((n,), (B, n) or (B, 1, n); 1 / True = keep), both or neither: masked generation by replacement
        conditioning (osufusion_amd/inpaint.py).  The iterate handed to the UNet has its known region at its own level: one
        ops.inpaint_blend of the start iterate at columns (1, 0) of the first coefficient row, one after every step at columns (2, 3) of the
        step's row, and after the final step of a full run the exact blend, so that the result holds `known` bit for bit where the mask is
        1.  The noise is one fixed tensor, a clone of the start iterate: nothing new is drawn.  Under use_hip_graph the blend is launched
        eagerly after each replay.  With both None: no extra launch, the bits of the unmasked sampler."""
        masked = inpaint.check_pair(known, known_mask)
        with ops.reproducible_mode(self.reproducible_sampling):
            return self._sample(a, c, x, cond_scale, (known, known_mask) if masked else None)

    def _sample(self, a, c, x, cond_scale, keep_region=None):
        return self._run(self._ddim, a, c, x, cond_scale, self.stop_after, keep_region, wrap=self._graph_pass if self.use_hip_graph else None)

    def _graph_pass(self, one_pass, steps):
        """use_hip_graph: the pass of _run (the 2B-batched UNet call and ops.ddim_step) replayed from a hipGraph.  Step 0 runs eagerly (it
        also warms pack caches / RoPE tables); then one synchronise and one capture of the pass and the copy of its result into the static
        iterate, reading static x / t / coef buffers; the iterate is restored and every later step is a replay after its t and coef rows are
        copied in.  _run's blends stay outside the graph: eager and replay issue the same sequence."""
        if steps < 2:
            return one_pass
        graph = x_buf = t_buf = coef_buf = None

        def run(i, t, row, x, state):
            nonlocal graph, x_buf, t_buf, coef_buf
            if graph is None:
                x_buf, t_buf, coef_buf = one_pass(i, t, row, x, state)[0], t.clone(), row.clone()
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()
                keep_x = x_buf.clone()
                with torch.cuda.graph(graph):            # capture records the launches only; x_buf is restored below
                    x_buf.copy_(one_pass(i, t_buf, coef_buf, x_buf, None)[0])
                x_buf.copy_(keep_x)
                return x_buf, None
            if x is not x_buf:                           # a blend wrote the iterate to a new tensor
                x_buf.copy_(x)
            t_buf.copy_(t)
            coef_buf.copy_(row)
            graph.replay()
            return x_buf, None
        return run

