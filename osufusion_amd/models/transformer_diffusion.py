"""The DiT / MMDiT backbones behind the reference's ``OsuFusion`` interface: ``DiffusionOsuFusionDiT`` mirrors models/diffusion.OsuFusion and
``RectifiedFlowOsuFusionDiT`` models/rectified_flow.OsuFusion method for method (``forward`` = training loss, ``loss_with``, ``sample``,
``set_full_bf16``).  ``ContinuousDiffusionOsuFusionDiT`` is the same interface on modules/scheduler.GaussianDiffusionContinuousTimes: the
backbone's time input is the log-SNR, sampling is ancestral (DDPM, the default), one osuf_ct_step per step, or DDIM / DPM-Solver++(2M) on a
log-SNR grid, one osuf_ct_solver_step per step.  The backbone is stored as ``self.unet``: the reference trainers call ``model.unet.set_gradient_checkpointing`` and write
checkpoints with ``unet.``-prefixed keys, so train.py / data.py take these models as they are.

``sample`` is restructured like the UNet samplers: everything that does not depend on the step -- the audio's embedding rows and
where(keep, mlp_cond(c), null_cond) + mlp_a(feature_extractor_a(stat_pool(a))) -- is computed once per call, the conditional and null
branches of classifier-free guidance run as one batch of 2B, the guidance combine rides the DDIM-step kernel, and the attention forward of
every block is one launch over all K/V groups (ops.one_launch_attention -> osuf_gqa_fwd).  Every ``sample`` takes ``known`` / ``known_mask``:
masked generation by replacement conditioning, one ops.inpaint_blend per iterate handed to the denoiser (osufusion_amd/inpaint.py), with
RePaint resampling on the ancestral sampler, and ``window`` / ``window_stride`` / ``window_taper`` / ``window_batch``: songs longer than the
trained context by fused-window denoising (osufusion_amd/windowed.py), one gather and one fuse around a batched backbone call per step,
and ``guidance_rescale`` / ``guidance_interval``: the CFG rescale (one ops.cfg_rescale before a guided step) and guidance only inside a band
of log-SNR, the conditional B rows alone outside it (osufusion_amd/guidance.py).
The three diffusion samplers (discrete DDIM, ancestral, DDIM / 2M solver) share one loop with the UNet's DDIM sampler, base._OsuFusion._run;
each describes its steps to it with a _Steps record.  The flow sampler's loop is osufusion_amd/ode.ode_loop: ode.midpoint_loop by default,
fixed-grid Euler / RK4 or an adaptive embedded pair by ``method``.  The DDIM and flow objectives (``forward``, ``loss_with``, the sampler)
are the UNet models' own, diffusion._DDIM and rectified_flow._Flow; this module adds the transformer family under them --
``_TransformerOsuFusion``: the backbone, its denoiser closures and the window plan -- and each model's ``sample`` keywords.
Not here: hipGraph capture of the step, LoRA on these backbones.
"""
from typing import Optional, Tuple

import torch

from .. import ct, guidance, inpaint, ode, ops, windowed
from .. import runtime as rt
from ..modules.dit import DiT
from ..modules.mmdit import MMDiT
from ..modules.scheduler import GaussianDiffusionContinuousTimes
from .base import AUDIO_DIM, CONTEXT_DIM, TOTAL_DIM, _OsuFusion, _Steps
from .diffusion import _DDIM, _MSEFn
from .rectified_flow import _Flow

BACKBONES = {"mmdit": MMDiT, "dit": DiT}
SAMPLERS = ("ddpm", "ddim", "dpmpp_2m")                      # of ContinuousDiffusionOsuFusionDiT


class _TransformerOsuFusion(_OsuFusion):
    """The transformer family: a DiT or MMDiT as `unet` and the step-independent part of a sample call, whole or in windows."""

    WINDOW_DOC = """The window keywords of every sample() here: windowed sampling (fused-window denoising, MultiDiffusion), for songs longer than the
    trained context.
      window: the window length in frames, usually the trained attn_context_len.  None (the default): the whole sequence goes to the
        backbone at once, with the launches and the bits sample() had before these keywords.  A sequence of n <= window frames is
        sampled that way too.  For n > window every denoiser call becomes: ops.window_gather of the iterate into W windows of exactly
        `window` frames (windowed.window_starts; only the last start is clamped), the backbone on the b W windows as one batch, and
        ops.window_fuse of the window predictions into one full-length prediction.  The step kernels, thresholding and the
        known / known_mask blends work on the full-length tensors as before; the draws keep their shapes and their order.
      window_stride: frames between window starts, in [1, window]; default window * 3 // 4 rounded down to a multiple of the backbone's
        patch size (MMDiT's patch_size; a DiT counts as 1).
      window_taper: "trapezoid" (the default; linear ramps over the window - window_stride overlapping frames) or "flat" (a plain mean).
      window_batch: at most this many window rows per backbone call (None: all b W at once); bounds the activation memory.  Results under
        different window_batch values are not promised to be bit-equal: the GEMM dispatch may depend on the row count.
    ValueError: window < 1; a stride outside [1, window]; an unknown taper; window_batch < 1; window, the stride or (when n > window) n not
    a multiple of the patch size; any of the other three given while window is None.
    Out of scope: the two UNet models (the same loops over a closure of the same contract, but not wired to windows yet), hipGraph
    capture of a windowed step, and any claim about map quality (no trained weights were at hand)."""

    GUIDANCE_DOC = """The guidance keywords of every sample() here (osufusion_amd/guidance.py).  A denoiser call is guided iff cond_scale != 1 and its
    log-SNR lies in the interval; all log-SNR values are host floats, fixed before the loop.
      guidance_interval: (lo, hi) in log-SNR, both ends inclusive, None at an end = unbounded; None (the default): every call is guided.
        A guided call runs 2B rows, as before.  An unguided call runs the conditional B rows only -- the first B rows of the
        step-independent audio rows and conditioning vector, the first B entries of the step's time input -- and the step takes
        (cond, None), the unguided path of every step kernel and of ops.ct_x0_quantile.  window_batch chunks both forms.
      guidance_rescale: phi in [0, 1] (Lin et al. 2024, sec. 3.4).  With phi > 0 one ops.cfg_rescale goes before the step of every guided
        call: the guided prediction scaled per sample by phi std(cond) / std(guided) + (1 - phi); the step, and ops.ct_x0_quantile under
        dynamic thresholding, take (that, None).  With windows it sees the fused full-length prediction.  The 2M state, the draws and
        their order, known / known_mask, resample and stop_after are unchanged.
    At the defaults, with (None, None), and with an interval that contains every call at phi = 0: the launches and the bits sample() had
    before these keywords (a bounded interval on the continuous-time model reads the grid's log-SNR back once).  With cond_scale == 1 both
    are accepted and change nothing.
    ValueError: phi outside [0, 1]; an interval that is not a pair; lo > hi; a NaN end.
    Not promised: that a B-row call equals the first B rows of a 2B-row call bit for bit -- the GEMM dispatch may depend on the row count --
    so results across different intervals are comparable to fp noise, not bit for bit.
    Out of scope: the two UNet models (not wired to these keywords yet: their closure has no unguided call), a schedule of cond_scale, and any claim
    about map quality (no trained weights were at hand)."""

    def __init__(self, dim_h: int, backbone: str, cond_drop_prob: float, **backbone_kwargs) -> None:
        super().__init__(cond_drop_prob)
        if backbone not in BACKBONES:
            raise ValueError(f"backbone must be one of {sorted(BACKBONES)} (got {backbone!r})")
        self.backbone = backbone
        self.unet = BACKBONES[backbone](dim_in_x=TOTAL_DIM, dim_in_a=AUDIO_DIM, dim_in_c=CONTEXT_DIM, dim_h=dim_h, **backbone_kwargs)

    def _denoiser(self, a: torch.Tensor, c: torch.Tensor, cfg: bool):
        """-> f(x (b, 6, n) fp32, t (nb,), guided=cfg) = the prediction (nb, 6, n), nb = 2b with guidance (conditional rows first), else b.
        The audio rows and the step-independent conditioning vector are computed here, once.  A denoiser built with cfg also serves the
        unguided call of a guidance interval, f(x, t, False): the conditional b rows alone, from the first b rows of the same audio rows
        and conditioning vector and the first b entries of t."""
        net = self.unet
        b, n = a.shape[0], a.shape[-1]
        dtype = rt.compute_dtype(next(net.parameters()).dtype)
        keep = torch.ones(b, dtype=torch.bool, device=a.device)
        a_rows = net.encode_audio(a, dtype)
        if cfg:
            a_rows = torch.cat([a_rows, a_rows], 0)
            static = net.embed_static(torch.cat([a, a], 0), torch.cat([c, c], 0), torch.cat([keep, ~keep], 0))
        else:
            static = net.embed_static(a, c, keep)

        def f(x: torch.Tensor, t: torch.Tensor, guided: bool = cfg) -> torch.Tensor:
            rows, st = a_rows, static
            if cfg and not guided:
                rows, st, t = a_rows[:b], static[:b], t[:b]
            xin = torch.cat([x, x], 0) if cfg and guided else x
            cvec = (st + net.embed_time(t)).contiguous()
            return net.sample_rows(xin, rows, cvec, n, dtype).contiguous()
        return f

    def _windowed_denoiser(self, a: torch.Tensor, c: torch.Tensor, cfg: bool, window: int, stride: int, taper: str = "trapezoid",
                           window_batch: Optional[int] = None):
        """-> f(x (b, 6, n) fp32, t (nb,)) = the prediction (nb, 6, n) with _denoiser's contract (conditional rows first), by fused-window
        denoising (osufusion_amd/windowed.py), n >= window.  Once, here: the audio cut into its W windows, a_w (b W, 96, window), the
        conditioning repeated per window, and one inner _denoiser per chunk of at most window_batch of the b W window rows (None: one
        chunk), so the audio rows and the static conditioning vector are still computed once per call; the statistics pooling sees the
        window, as it does in training on sub-sequences.  Per step: one ops.window_gather of the iterate, one inner call per chunk with the
        step's t repeated per window, the halves of its [cond; null] result written into one (2, b W, 6, window) buffer (a single chunk's
        result is that buffer already), one ops.window_fuse over R = nb rows.  f(x, t, False) on a denoiser built with cfg: the
        unguided call of a guidance interval, every chunk's inner denoiser on its conditional rows alone, nb = b."""
        b, n = a.shape[0], a.shape[-1]
        W = len(windowed.window_starts(n, window, stride))
        rows = b * W
        a_w = ops.window_gather(a.float().contiguous(), window, stride)
        c_w = c.repeat_interleave(W, 0)
        step = rows if window_batch is None else min(int(window_batch), rows)
        chunks = [(lo, min(lo + step, rows)) for lo in range(0, rows, step)]
        inner = [self._denoiser(a_w[lo:hi], c_w[lo:hi], cfg) for lo, hi in chunks]
        weight = windowed.window_weight(window, stride, taper).to(a.device)

        def f(x: torch.Tensor, t: torch.Tensor, guided: bool = cfg) -> torch.Tensor:
            g = 2 if cfg and guided else 1
            how = (False,) if cfg and not guided else ()     # the inner denoisers' own default otherwise
            x_w = ops.window_gather(x, window, stride)
            t_w = t[:g * b].view(g, b).repeat_interleave(W, 1)
            if len(chunks) == 1:
                pred = inner[0](x_w, t_w.reshape(-1), *how)
            else:
                pred = torch.empty((g, rows, x.shape[1], window), dtype=torch.float32, device=x.device)
                for (lo, hi), den in zip(chunks, inner):
                    pred[:, lo:hi] = den(x_w[lo:hi], t_w[:, lo:hi].reshape(-1), *how).view(g, hi - lo, x.shape[1], window)
            return ops.window_fuse(pred.view(g * rows, x.shape[1], window), weight, n, stride)
        return f

    def _make_denoiser(self, a: torch.Tensor, c: torch.Tensor, cfg: bool, wp: Optional[windowed.WindowPlan] = None):
        """The closure every sampling loop calls: _denoiser over the whole sequence when no window is asked for or the sequence fits into
        one, else _windowed_denoiser."""
        if wp is None or a.shape[-1] <= wp.window:
            return self._denoiser(a, c, cfg)
        return self._windowed_denoiser(a, c, cfg, wp.window, wp.stride, wp.taper, wp.batch)

    def _window_plan(self, a: torch.Tensor, window, window_stride, window_taper, window_batch) -> Optional[windowed.WindowPlan]:
        """The window keywords of sample() checked against the backbone's patch size (a DiT counts as 1) and the length of `a`."""
        p = getattr(self.unet, "patch_size", 1)
        wp = windowed.plan(window, window_stride, window_taper, window_batch, p)
        if wp is not None:
            windowed.check_length(a.shape[-1], wp, p)
        return wp


class DiffusionOsuFusionDiT(_DDIM, _TransformerOsuFusion):
    def __init__(self, dim_h: int, backbone: str = "mmdit", cond_drop_prob: float = 0.5, train_timesteps: int = 1000,
                 sampling_timesteps: int = 35, **backbone_kwargs) -> None:
        super().__init__(dim_h, backbone, cond_drop_prob, **backbone_kwargs)
        self._init_ddim(train_timesteps, sampling_timesteps)

    @torch.inference_mode()
    def sample(self, a: torch.Tensor, c: torch.Tensor, x: Optional[torch.Tensor] = None, cond_scale: float = 7.0,
               known: Optional[torch.Tensor] = None, known_mask: Optional[torch.Tensor] = None,
               window: Optional[int] = None, window_stride: Optional[int] = None, window_taper: str = "trapezoid",
               window_batch: Optional[int] = None, guidance_rescale: float = 0.0,
               guidance_interval: Optional[Tuple[Optional[float], Optional[float]]] = None) -> torch.Tensor:
        """diffusion.py:59-77 on the transformer backbones.  Bit-reproducible.  (Attribute `stop_after`, None by default: return the iterate
        after that many of the sampling_timesteps steps, as models/diffusion.OsuFusion.)

        known (B, 6, n) and known_mask ((n,), (B, n) or (B, 1, n); 1 / True = keep), both or neither: masked generation as in
        models/diffusion.OsuFusion.sample_masked -- the start iterate blended at columns (1, 0) of the first coefficient row, every step's result at
        columns (2, 3) of its row, the final step of a full run exactly; one fixed noise tensor (a clone of the start iterate), no new draw.
        With both None: no extra launch, the unmasked sampler's bits.

        window, window_stride, window_taper, window_batch: windowed sampling, see _TransformerOsuFusion.WINDOW_DOC.

        guidance_rescale, guidance_interval: see _TransformerOsuFusion.GUIDANCE_DOC; a step's log-SNR is log(abar_t / (1 - abar_t)) of the
        scheduler's cumulative alphas, in fp64."""
        masked = inpaint.check_pair(known, known_mask)
        wp = self._window_plan(a, window, window_stride, window_taper, window_batch)
        gd = guidance.plan(guidance_rescale, guidance_interval)
        with ops.reproducible_mode(True), ops.one_launch_attention(True):
            return self._run(self._ddim, a, c, x, cond_scale, self.stop_after, (known, known_mask) if masked else None, wp, gd)


class ContinuousDiffusionOsuFusionDiT(_TransformerOsuFusion):
    """Continuous-time Gaussian diffusion: a noise (default), x_start or v prediction conditioned on log_snr(t) (scheduler.get_condition), t
    uniform in [0, 1]."""

    def __init__(self, dim_h: int, backbone: str = "mmdit", cond_drop_prob: float = 0.5, noise_schedule: str = "cosine",
                 sampling_timesteps: int = 35, pred_objective: str = "noise", dynamic_thresholding: bool = False,
                 dynamic_thresholding_percentile: float = 0.95, min_snr_gamma: Optional[float] = None, sampler: str = "ddpm",
                 ddim_eta: float = 0.0, solver_spacing: str = "logsnr", solver_logsnr_min: float = -15.0, **backbone_kwargs) -> None:
        """pred_objective: what the backbone predicts, "noise" (the default), "x_start" or "v" = alpha noise - sigma x_0.
        dynamic_thresholding: sample() clamps the start prediction to its per-sample `dynamic_thresholding_percentile` quantile of |x_0|
        (at least 1) and rescales, instead of the static clamp to [-1, 1].  min_snr_gamma: min-SNR-gamma weighting of the training loss.
        sampler: "ddpm" (the default: ancestral, over the time grid), "ddim" (deterministic at ddim_eta = 0, the ancestral variance at 1) or
        "dpmpp_2m" (DPM-Solver++(2M), second order, deterministic); the last two run sampling_timesteps steps over
        scheduler.solver_log_snr_grid(sampling_timesteps, solver_spacing, solver_logsnr_min).  Training does not depend on any of the four."""
        if sampler not in SAMPLERS:
            raise ValueError(f"Unknown sampler: {sampler!r} (one of {list(SAMPLERS)})")
        if not 0.0 <= ddim_eta <= 1.0:
            raise ValueError(f"ddim_eta must be in [0, 1] (got {ddim_eta})")
        if solver_spacing not in ("logsnr", "time"):
            raise ValueError(f"Unknown solver spacing: {solver_spacing!r} (one of ['logsnr', 'time'])")
        if pred_objective not in ct.OBJECTIVES:
            raise ValueError(f"Unknown prediction objective: {pred_objective!r} (one of {sorted(ct.OBJECTIVES)})")
        if not 0.0 < dynamic_thresholding_percentile <= 1.0:
            raise ValueError(f"dynamic_thresholding_percentile must be in (0, 1] (got {dynamic_thresholding_percentile})")
        super().__init__(dim_h, backbone, cond_drop_prob, **backbone_kwargs)
        self.scheduler = GaussianDiffusionContinuousTimes(noise_schedule=noise_schedule, timesteps=sampling_timesteps)
        self.sampling_timesteps = sampling_timesteps
        self.stop_after: Optional[int] = None
        self.pred_objective = pred_objective
        self.dynamic_thresholding = bool(dynamic_thresholding)
        self.dynamic_thresholding_percentile = float(dynamic_thresholding_percentile)
        self.min_snr_gamma = min_snr_gamma
        self.sampler = sampler
        self.ddim_eta = float(ddim_eta)
        self.solver_spacing = solver_spacing
        self.solver_logsnr_min = float(solver_logsnr_min)

    @torch.inference_mode()
    def sample(self, a: torch.Tensor, c: torch.Tensor, x: Optional[torch.Tensor] = None, cond_scale: float = 7.0,
               known: Optional[torch.Tensor] = None, known_mask: Optional[torch.Tensor] = None, resample: int = 1,
               window: Optional[int] = None, window_stride: Optional[int] = None, window_taper: str = "trapezoid",
               window_batch: Optional[int] = None, guidance_rescale: float = 0.0,
               guidance_interval: Optional[Tuple[Optional[float], Optional[float]]] = None) -> torch.Tensor:
        """sampler = "ddpm": ancestral sampling over scheduler.get_sampling_timesteps: per step one denoiser call at log_snr(t) (2B rows with guidance) and one
        ops.ct_step (guidance, start prediction clamped to [-1, 1], posterior mean, noise).  Draws from the global generator, in this order:
        the start iterate torch.randn((B, 6, n)) when x is None, then one torch.randn of the iterate's shape per step, in step order; the
        last step (t_next == 0) adds no noise and draws none.  A plain loop that draws the same way from the same seed sees the same
        noise.  Bit-reproducible for a given seed.  (Attribute `stop_after` as in DiffusionOsuFusionDiT.)  With another pred_objective the
        step is ops.ct_step_ex; with dynamic_thresholding one ops.ct_x0_quantile goes before it (two launches per step, no extra draw).

        sampler = "ddim" / "dpmpp_2m": one ops.ct_solver_schedule per call, then per step one denoiser call at the grid's log_snr, one
        ops.ct_x0_quantile only with dynamic_thresholding, and one ops.ct_solver_step, which also returns the clamped start prediction that
        the next 2M step takes as x0_prev.  Draws from the global generator, in this order: the start iterate torch.randn((B, 6, n)) when x is
        None; then, for "ddim" with ddim_eta > 0 only, one torch.randn of the iterate's shape per step, in step order, the last step
        included (its gain is eta times the ancestral one, not zero: the grid ends at log_snr(0), not at infinity).  "dpmpp_2m" and "ddim" at
        ddim_eta = 0 draw nothing after the start iterate.  Bit-reproducible; `stop_after` as above.

        known (B, 6, n) and known_mask ((n,), (B, n) or (B, 1, n); 1 / True = keep), both or neither: masked generation by replacement
        conditioning (osufusion_amd/inpaint.py).  Every iterate handed to the denoiser has its known region at its own level,
        alpha known + sigma noise: one ops.inpaint_blend of the start iterate at columns (1, 2) of the first schedule row, one after every step
        at columns (4, 5) of the step's row, and after the final step of a full run the exact blend (`known` bit for bit where the mask is 1;
        a run cut short by `stop_after` ends on a level blend).  "dpmpp_2m" and "ddim" at ddim_eta = 0 take one fixed noise tensor, a clone of
        the start iterate, and draw nothing new; the x0_prev of a 2M step stays as the step kernel wrote it.  "ddpm" and "ddim" with
        ddim_eta > 0 draw a fresh torch.randn of the iterate's shape per level blend, which extends the order above: the start iterate, then
        the start blend's noise; then per step the step's own noise (where it draws one) and after it the noise of that step's level blend.
        The exact blend draws nothing.  With both None: no extra launch, no extra draw, the bits of the unmasked sampler.

        resample = r > 1 (RePaint's resampling; "ddpm" with a known region only): every step but the final one of a full run is taken r
        times.  After pass u < r - 1 (the step, then its level blend) the whole iterate goes back one level by the exact forward transition
        x = k_r x + k_g z through ops.axpby_rows, z a fresh torch.randn, the last draw of that pass, with per sample
        k_r = alpha / alpha_next and k_g = sigma sqrt(c) (columns 1, 4 and 2, 6 of the step's row; sigma^2 - k_r^2 sigma_next^2 = sigma^2 c, so
        nothing cancels), computed in fp32 torch once per call.  r (S - 1) + 1 denoiser calls for S steps.

        window, window_stride, window_taper, window_batch: windowed sampling, see _TransformerOsuFusion.WINDOW_DOC; the draws above are of
        the full-length iterate's shape and keep their order.

        guidance_rescale, guidance_interval: see _TransformerOsuFusion.GUIDANCE_DOC; a step's log-SNR is the fp32 value the denoiser is
        given for it, under every sampler, read back once per call when an interval is given.  The RePaint passes of a step share its
        decision; with dynamic_thresholding the quantile of a rescaled step is taken of the rescaled prediction."""
        masked = inpaint.check_pair(known, known_mask)
        gd = guidance.plan(guidance_rescale, guidance_interval)
        resample = int(resample)
        if resample < 1:
            raise ValueError(f"resample must be >= 1 (got {resample})")
        if resample > 1 and (self.sampler != "ddpm" or not masked):
            raise ValueError('resample > 1 needs sampler == "ddpm" and a known region (known, known_mask)')
        keep_region = (known, known_mask) if masked else None
        wp = self._window_plan(a, window, window_stride, window_taper, window_batch)
        with ops.reproducible_mode(True), ops.one_launch_attention(True):
            describe = self._solver if self.sampler != "ddpm" else lambda *args: self._ancestral(*args, resample)
            return self._run(describe, a, c, x, cond_scale, self.stop_after, keep_region, wp, gd)

    def _threshold(self, x, cond, null, cond_scale, row) -> Optional[torch.Tensor]:
        """The per-sample dynamic threshold of a step, one ops.ct_x0_quantile; None (the static clamp) without dynamic_thresholding."""
        if not self.dynamic_thresholding:
            return None
        return ops.ct_x0_quantile(x, cond, null, cond_scale, row, self.pred_objective, self.dynamic_thresholding_percentile)[:, 2]

    def _solver(self, b, cfg, cond_scale, device) -> _Steps:
        total = self.scheduler.timesteps
        grid = self.scheduler.solver_log_snr_grid(total, self.solver_spacing, self.solver_logsnr_min, device=device)
        coef, fac = self.scheduler.solver_coefficients(grid, self.sampler, self.ddim_eta, batch=b)
        log_snr = grid[:-1, None].repeat(1, 2 * b if cfg else b)
        draws = self.sampler == "ddim" and self.ddim_eta > 0.0

        def step(i, row, x, cond, null, noise, x0_prev):   # the state: the clamped start prediction, the next 2M step's x0_prev
            s = self._threshold(x, cond, null, cond_scale, row)
            return ops.ct_solver_step(x, cond, null, cond_scale, row, fac[i], x0_prev, noise, self.pred_objective, s)
        return _Steps(coef, log_snr, step, draw_steps=total if draws else 0, fresh=draws, start_cols=(ct.ALPHA, ct.SIGMA),
                      step_cols=(ct.ALPHA_NEXT, ct.SIGMA_NEXT), last=total - 1, log_snr=lambda: grid[:-1].tolist())

    def _ancestral(self, b, cfg, cond_scale, device, resample=1) -> _Steps:
        total = self.scheduler.timesteps
        times = torch.linspace(1.0, 0.0, total + 1, device=device, dtype=torch.float32)        # get_sampling_timesteps' grid, every pair at once
        coef = self.scheduler.coefficients(times[:-1].repeat_interleave(b), times[1:].repeat_interleave(b)).view(total, b, -1)
        log_snr = coef[:, :, 0].repeat(1, 2 if cfg else 1).contiguous()
        plain = self.pred_objective == "noise" and not self.dynamic_thresholding
        k_r = k_g = None
        if resample > 1:                                    # the forward transition from a step's level back to the level it left
            k_r = (coef[:, :, ct.ALPHA] / coef[:, :, ct.ALPHA_NEXT]).contiguous()
            k_g = (coef[:, :, ct.SIGMA] * torch.sqrt(coef[:, :, ct.C])).contiguous()

        def step(i, row, x, cond, null, noise, state):
            if plain:
                return ops.ct_step(x, cond, null, cond_scale, row, noise), None
            s = self._threshold(x, cond, null, cond_scale, row)
            return ops.ct_step_ex(x, cond, null, cond_scale, row, noise, self.pred_objective, s), None
        return _Steps(coef, log_snr, step, draw_steps=total - 1, fresh=True, start_cols=(ct.ALPHA, ct.SIGMA),
                      step_cols=(ct.ALPHA_NEXT, ct.SIGMA_NEXT), last=total - 1, resample=resample, k_r=k_r, k_g=k_g,
                      log_snr=lambda: coef[:, 0, ct.LOG_SNR].tolist())

    def forward(self, x: torch.Tensor, a: torch.Tensor, c: torch.Tensor, orig_len: Optional[torch.Tensor] = None) -> torch.Tensor:
        assert x.shape[-1] == a.shape[-1], "x and a must have the same number of sequence length"
        rt.require_gpu(x)
        noise = torch.randn_like(x, device=x.device)
        times = self.scheduler.sample_random_times(x.shape[0], x.device)
        return self.loss_with(x, a, c, noise, times, orig_len)

    def loss_with(self, x, a, c, noise, times, orig_len=None, cond_drop_prob: Optional[float] = None) -> torch.Tensor:
        """forward() with the RNG draws passed in (parity tests, benchmarks)."""
        p = self.cond_drop_prob if cond_drop_prob is None else cond_drop_prob
        with self._dtype_ctx():
            if self.pred_objective == "noise":
                x_noisy, log_snr, _, _ = self.scheduler.q_sample(x, times.float(), noise)
                target = noise.float()
            else:                                           # x_noisy and the x_start / v target in one pass
                sched = self.scheduler.coefficients(times.float())
                x_noisy, target = ops.ct_qsample(x.float().contiguous(), noise.float().contiguous(), sched, self.pred_objective)
                log_snr = sched[:, ct.LOG_SNR]
            pred = self.unet(x_noisy, a, log_snr.contiguous(), c, cond_drop_prob=p)
        weight = self.scheduler.loss_weight(log_snr, self.pred_objective, self.min_snr_gamma)
        if weight is None:
            return _MSEFn.apply(pred, target, orig_len)
        return _MSEFn.apply(pred, target, orig_len, weight.float().contiguous())


class RectifiedFlowOsuFusionDiT(_Flow, _TransformerOsuFusion):
    def __init__(self, dim_h: int, backbone: str = "mmdit", cond_drop_prob: float = 0.5, sampling_timesteps: int = 16,
                 **backbone_kwargs) -> None:
        super().__init__(dim_h, backbone, cond_drop_prob, **backbone_kwargs)
        self.sample_timesteps = sampling_timesteps

    @torch.inference_mode()
    def sample(self, a: torch.Tensor, c: torch.Tensor, x: Optional[torch.Tensor] = None, cond_scale: float = 2.0,
               known: Optional[torch.Tensor] = None, known_mask: Optional[torch.Tensor] = None,
               window: Optional[int] = None, window_stride: Optional[int] = None, window_taper: str = "trapezoid",
               window_batch: Optional[int] = None, guidance_rescale: float = 0.0,
               guidance_interval: Optional[Tuple[Optional[float], Optional[float]]] = None, method: str = "midpoint",
               rtol: float = 1e-5, atol: float = 1e-5, first_step: Optional[float] = None, max_steps: int = 1000) -> torch.Tensor:
        """rectified_flow.py:57-79 on the transformer backbones: the fixed-grid midpoint loop, 2 * (S - 1) evaluations.  Bit-reproducible.
        known / known_mask (both or neither): masked generation as in models/rectified_flow.OsuFusion.sample_masked -- every state handed to the
        backbone blended at (t, 1 - t), the end of the last interval exactly, one fixed noise tensor, no new draw.

        window, window_stride, window_taper, window_batch: windowed sampling, see _TransformerOsuFusion.WINDOW_DOC.

        guidance_rescale, guidance_interval: see _TransformerOsuFusion.GUIDANCE_DOC; an evaluation's log-SNR is 2 log(t / (1 - t)) of its
        time, in fp64, -inf at t = 0, and every evaluation of a step decides for itself.  On a rescaled evaluation
        ops.cfg_rescale replaces the ops.axpby_rows combine.

        method, rtol, atol, first_step, max_steps: the ODE solver, as the reference's odeint call takes them (osufusion_amd/ode.py).
        "euler", "midpoint" (the default: this loop's launches and bits as they were) and "rk4" step over the sampler's grid, S - 1,
        2 (S - 1) and 4 (S - 1) evaluations, and ignore the tolerances; "bosh3" and "dopri5" choose their steps from rtol / atol (one step
        size for the batch, B doubles read back per attempted step), start at first_step (None: the grid's 1 / (S - 1)) and raise
        RuntimeError after max_steps attempted steps; with known / known_mask they raise ValueError.  The call's evaluations, accepted and
        rejected steps and accepted step ends are left in self.last_ode_stats."""
        masked = inpaint.check_pair(known, known_mask)
        wp = self._window_plan(a, window, window_stride, window_taper, window_batch)
        gd = guidance.plan(guidance_rescale, guidance_interval)
        solver = dict(method=method, rtol=rtol, atol=atol, first_step=first_step, max_steps=max_steps)
        ode.check_options(**solver)
        with ops.reproducible_mode(True), ops.one_launch_attention(True):
            return self._sample(a, c, x, cond_scale, (known, known_mask) if masked else None, wp, gd, solver)
