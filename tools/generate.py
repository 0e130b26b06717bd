#!/usr/bin/env python3
"""The way out: an audio file -> ``.osu`` files, every stage on the GPU but the slider fits and the text.

    python tools/generate.py SONG.wav --out DIR [--backbone mmdit|dit] [--objective ddim|ct-noise|ct-x_start|ct-v|flow]
        [--checkpoint model.safetensors | --seed 0] [--model-kw '{"dim_h": 512, "depth": 12}']
        [--cs 4 --ar 9 --od 8 --hp 5 --sr 5.5] [--steps 16 --cond-scale 2 --window 4096 --window-stride 3072] [--n 4] [--bpm 180]
        [--dump-signals]

audio.load_audio computes the log-VQT `a` (96, frames); it is padded with -23 (data.collate_fn's audio padding) to the multiple of the
backbone's patch size; the model's sample() draws --n candidates in one batch; decode_gpu.decode_beatmaps decodes them in one batch,
cut back to the song's own frames through `lengths=`; DIR receives NAME_k.osu (NAME = the audio file's stem) and, with --dump-signals,
NAME_k.npz holding `x` (6, frames) -- the sample cut to the song's frames -- and `frame_times`.

Without --checkpoint the weights are random (torch.manual_seed(--seed) before the model is built): that exercises the pipeline, it makes no
map worth playing -- no trained weights were at hand, so nothing here says anything about map quality.  The models are the transformer
family (DiffusionOsuFusionDiT, ContinuousDiffusionOsuFusionDiT, RectifiedFlowOsuFusionDiT); the two UNet models are not wired to this tool.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

AUDIO_PAD = -23.0                                                    # data.collate_fn


def build_model(backbone: str, objective: str, steps: int, model_kw: dict):
    from osufusion_amd.models import ContinuousDiffusionOsuFusionDiT, DiffusionOsuFusionDiT, RectifiedFlowOsuFusionDiT
    model_kw = {"dim_h": 512, **model_kw}
    if objective == "ddim":
        return DiffusionOsuFusionDiT(backbone=backbone, sampling_timesteps=steps, **model_kw)
    if objective == "flow":
        return RectifiedFlowOsuFusionDiT(backbone=backbone, sampling_timesteps=steps, **model_kw)
    if objective.startswith("ct-"):
        kw = {"sampler": "dpmpp_2m", **model_kw}
        return ContinuousDiffusionOsuFusionDiT(backbone=backbone, sampling_timesteps=steps, pred_objective=objective[3:], **kw)
    raise ValueError(f"unknown objective {objective!r}")


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("audio", type=Path)
    ap.add_argument("--out", type=Path, required=True)
    ap.add_argument("--backbone", choices=("mmdit", "dit"), default="mmdit")
    ap.add_argument("--objective", choices=("ddim", "ct-noise", "ct-x_start", "ct-v", "flow"), default="ct-v")
    ap.add_argument("--model-kw", type=json.loads, default={}, help="JSON: the model's constructor keywords (dim_h, depth, attn_heads, ...)")
    ap.add_argument("--checkpoint", type=Path, default=None, help="model.safetensors or checkpoint.pt (data.load_model_sd); random weights without")
    ap.add_argument("--seed", type=int, default=0, help="seeds the random weights (no --checkpoint) and the sampler's draws")
    for name, default in (("cs", 4.0), ("ar", 9.0), ("od", 8.0), ("hp", 5.0), ("sr", 5.0)):
        ap.add_argument(f"--{name}", type=float, default=default)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--cond-scale", type=float, default=2.0)
    ap.add_argument("--window", type=int, default=None)
    ap.add_argument("--window-stride", type=int, default=None)
    ap.add_argument("--n", type=int, default=1, help="candidates, drawn and decoded as one batch")
    ap.add_argument("--bpm", type=float, default=None, help="the song's tempo, if known (else it is estimated from the onsets)")
    ap.add_argument("--no-beat-snap", action="store_true")
    ap.add_argument("--title", default=None)
    ap.add_argument("--artist", default="Unknown")
    ap.add_argument("--dump-signals", action="store_true")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    if args.n < 1:
        ap.error("--n must be at least 1")

    import torch

    from osufusion_amd import audio, data, decode, decode_gpu, inpaint

    torch.manual_seed(args.seed)
    model = build_model(args.backbone, args.objective, args.steps, dict(args.model_kw))
    if args.checkpoint is not None:
        data.load_model_sd(model, args.checkpoint)
    model = model.to(args.device).eval()

    a = audio.load_audio(args.audio, args.device)                    # (96, frames)
    frames = int(a.shape[1])
    p = int(getattr(model.unet, "patch_size", 1))
    padded = -(-frames // p) * p
    if padded > decode_gpu.MAX_LENGTH:
        raise ValueError(f"{frames} frames: longer than the {decode_gpu.MAX_LENGTH} frames a map is decoded over")
    a_pad = torch.full((a.shape[0], padded), AUDIO_PAD, dtype=a.dtype, device=a.device)
    a_pad[:, :frames] = a
    a_b = a_pad[None].repeat(args.n, 1, 1).contiguous()
    c = data.normalize_context(np.array([args.cs, args.ar, args.od, args.hp, min(20.0, max(0.0, args.sr))], dtype=np.float32))
    c_b = torch.from_numpy(c).to(args.device)[None].repeat(args.n, 1).contiguous()

    kw = dict(cond_scale=args.cond_scale)
    if args.window is not None:
        kw.update(window=args.window, window_stride=args.window_stride)
    x = model.sample(a_b, c_b, **kw).float().contiguous()            # (n, 6, padded)

    stem = args.audio.stem
    metas = [decode.Metadata(args.audio.name, args.title or stem, args.artist, f"OsuFusion {k}", args.cs, args.ar, args.od, args.hp)
             for k in range(args.n)]
    frame_times = inpaint.frame_times_ms(padded).numpy()
    lengths = torch.full((args.n,), frames, dtype=torch.int32, device=x.device)
    texts = decode_gpu.decode_beatmaps(metas, x, frame_times, bpm=args.bpm, allow_beat_snap=not args.no_beat_snap, lengths=lengths)
    args.out.mkdir(parents=True, exist_ok=True)
    signals = x[:, :, :frames].cpu().numpy() if args.dump_signals else None
    for k, text in enumerate(texts):
        (args.out / f"{stem}_{k}.osu").write_text(text, encoding="utf-8")
        if signals is not None:
            np.savez_compressed(args.out / f"{stem}_{k}.npz", x=signals[k], frame_times=frame_times[:frames])
    print(f"wrote {len(texts)} maps of {frames} frames ({padded} sampled) to {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
