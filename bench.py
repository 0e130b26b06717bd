#!/usr/bin/env python3
"""Headline benchmark: denoise-steps/sec of one full train step (forward + backward + gradient all-reduce + clip + AdamW)
of the full OsuFusion UNet (dim_h=256, 343.5 M parameters) at per-GPU batch 32, L=4096, bf16 compute -- BASELINE.json
configs[1] (N=1) / configs[2] (N>1, weak scaling: global batch 32*N, one process per GPU, RCCL over xGMI).

    python bench.py --gpus 1 --steps K --warmup W [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

A plain run sets up, warms up, times K steps and prints the result line.  --full adds everything else the benchmark measures: the
HIP-event roofline of the timed steps' attention kernels, and on one GPU the CPU baseline and, at the full size, the fp32 compute modes,
the config-4 sampler and the DoRA config-5 shard (each can still be left out with its --no-* switch).  --dump-outputs DIR writes what the
last timed step computed as DIR/<name>.npy (see dump_outputs).  Every step starts from the same seeded parameters (restored between
steps, outside the timed spans), so that with the same arguments a run's outputs are the same, to rounding, in every run.

Shape-mapping note printed with every result: the reference UNet takes audio as (B, 96, L) with the
same L as the map sequence (models/diffusion.py:86); BASELINE's "C=256" is dim_h=256 and "audio-ctx=1024x128" has no literal
counterpart (no cross-attention: the audio is encoded to (B, 1024, L/8) and concatenated at the bottleneck, unet.py:483,500).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

MFMA_BF16_PEAK_TFLOPS = 2500.0          # dense bf16, /opt/skills/guides/MI355X_MICROARCH.md "Chip-level parameters"
DIM_H, BATCH, LENGTH, HEADS, HEAD_DIM = 256, 32, 4096, 16, 64
STEP_TFLOP = 125.1                      # 3 x 1,303 GFLOP/sample x 32 (recompute not counted)
# C-ABI entry point -> (algorithmic, executed) attention FLOPs per launch in units of B*H*N^2*D.  SURVEY.md section 8d counts the
# backward as 2x the forward (recompute is not work): forward 4; the dQ kernel and the dK/dV kernel 4 + 4 (they EXECUTE 6 + 8: S
# and dP are recomputed in both); the fused backward sweep is the whole backward, 8 (it executes 10: five products).
ATTN_UNITS = {"osuf_mqa_fwd": (4.0, 4.0), "osuf_mqa_bwd_dq": (4.0, 6.0), "osuf_mqa_bwd_dkv": (4.0, 8.0), "osuf_mqa_bwd_fused": (8.0, 10.0)}
PMC_MANIFEST = ROOT / "profiles" / "pmc_manifest.json"    # which committed counter summaries to quote + the kernel-source hash they were taken on


def pmc_manifest():
    """The committed counter summaries (tools/pmc_manifest.py) -- or (None, why) when the attention kernel sources of this tree are not
    the ones those counters were collected on: bench.py cannot run the profiler on itself, so it must not quote stale counters."""
    try:
        man = json.loads(PMC_MANIFEST.read_text())
        from osufusion_amd.csrc.build import source_hash
        now = source_hash(man["attn_sources"])
    except (OSError, ValueError, KeyError) as e:
        return None, f"no usable profiles/pmc_manifest.json ({type(e).__name__})"
    if now != man["attn_source_sha256"]:
        return None, f"stale: attention kernel sources changed since the counter passes of tree {man.get('tree')} (no new PMC pass committed)"
    return man, None


def pmc_traffic(kernel: str):
    """(HBM bytes per launch of `kernel`, source tag): mean over one step's launches at the headline shape, separate FETCH_SIZE /
    WRITE_SIZE passes, FETCH_SIZE doubled as MI355X_MICROARCH.md 'HBM' prescribes.  (None, reason) when stale or absent."""
    man, why = pmc_manifest()
    if man is None:
        return None, why
    try:
        row = json.loads((ROOT / man["traffic"]).read_text()).get(kernel)
    except (OSError, ValueError):
        return None, f"{man['traffic']} unreadable"
    return (row["bytes_per_launch"], f"{row.get('source')} [tree {man.get('tree')}]") if row else (None, f"no row for {kernel} in {man['traffic']}")


def pmc_mfma_busy():
    """(MFMA-busy share of the attention-backward sweep over a train step, source): SQ_VALU_MFMA_BUSY_CYCLES / (GRBM_GUI_ACTIVE / 8 x 1,024
    SIMDs) from the committed counter pass (tools/pmc_mfma.py).  (None, reason) when stale or absent."""
    man, why = pmc_manifest()
    if man is None:
        return None, why
    try:
        for line in (ROOT / man["mfma_busy"]).read_text().splitlines():
            if line.startswith("mqa_bwd_fused512a_kernel"):
                return round(float(line.split("%")[0].split()[-1]) / 100.0, 4), f"{man['mfma_busy']} [tree {man.get('tree')}]"
    except (OSError, ValueError, IndexError):
        pass
    return None, f"no mqa_bwd_fused512a_kernel row in {man['mfma_busy']}"


def synth_batch(rank: int, device, batch: int, length: int):
    """SURVEY section 8d synthetic inputs, generated once and resident in HBM before the timed region."""
    g = torch.Generator(device="cpu").manual_seed(1234 + rank)
    x = (torch.randn(batch, 6, length, generator=g) * 0.5).clamp_(-1, 1)
    a = torch.randn(batch, 96, length, generator=g) * 3 - 10
    c = torch.rand(batch, 5, generator=g) * 2 - 1
    t = torch.randint(0, 1000, (batch,), generator=g)
    noise = torch.randn(batch, 6, length, generator=g)
    return tuple(v.to(device) for v in (x, a, c, noise, t))


def build_model(device, dim_h: int):
    from osufusion_amd.models.diffusion import OsuFusion
    torch.manual_seed(0)                                   # identical replicas on every rank
    model = OsuFusion(dim_h)
    with torch.no_grad():                                  # the reference zero-inits final_conv (unet.py:354): every other
        model.unet.final_conv.weight.normal_(0.0, 0.02)    # gradient would be exactly zero -- use a live head instead
    return model.to(device)


DUMP_SAMPLE = 1 << 22                   # elements per sampled array of --dump-outputs: 16 MiB of float32 each


def dump_outputs(out_dir, model, loss, grad_norm) -> list:
    """--dump-outputs: what a caller of the timed train step holds after its last step, as float32 .npy files in out_dir -- the loss and the
    clipped step's gradient norm, and the trainable parameters as AdamW left them and their gradients, at a fixed seeded sample of
    DUMP_SAMPLE positions of the named_parameters() order (every position when there are fewer).  Indexed by parameter name, not by the
    flat buffer, whose layout follows the first backward's completion order."""
    import numpy as np
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    sizes = torch.tensor([p.numel() for _, p in named], dtype=torch.int64)
    ends = sizes.cumsum(0)
    total = int(ends[-1])
    if total <= DUMP_SAMPLE:
        idx = torch.arange(total)
    else:
        idx = torch.randint(0, total, (DUMP_SAMPLE,), generator=torch.Generator().manual_seed(4096)).sort().values
    cut = torch.searchsorted(idx, ends).tolist()       # idx[cut[i-1]:cut[i]] lie in parameter i
    params, grads, lo = [], [], 0
    for (name, p), hi, end in zip(named, cut, ends.tolist()):
        if hi > lo:
            assert p.grad is not None, f"{name} has no gradient after the timed step"
            local = (idx[lo:hi] - (end - p.numel())).to(p.device)
            params.append(p.detach().reshape(-1)[local].float())
            grads.append(p.grad.detach().reshape(-1)[local].float())
        lo = hi
    arrays = {"loss": loss.detach().float().reshape(1), "grad_norm": grad_norm.detach().float().reshape(1),
              "params": torch.cat(params), "grads": torch.cat(grads)}
    out_dir = Path(out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    for name, v in arrays.items():
        np.save(out_dir / f"{name}.npy", v.cpu().numpy().astype(np.float32))
    return sorted(arrays)


def cpu_baseline(model, length: int, thread_counts):
    """The oracle (CPU restatement of the reference, pinned to its golden vectors) on this box's host cores: one fwd+bwd
    of the same full-size model at B=1, L=length, fp32 params + bf16 SDPA exactly as the reference computes on CPU.  Timed at
    every thread count given, smallest first (BASELINE.md section 3's 3 warm-ups + 5 timed iterations); a larger count that is already
    slower on its first iteration (a 1-GPU box of the pool grants ~16 CPUs: more threads than that only oversubscribe them) is
    recorded from that one iteration and not pursued.  `value` is the FASTEST count (the CPU's best); the others are listed."""
    runs = []
    for n in sorted(thread_counts):
        limit = 1.25 * runs[0]["seconds_per_sample"] if runs else None
        runs.append(_cpu_baseline_at(model, length, n, give_up_above=limit))
    best = max(runs, key=lambda r: r["value"])
    best["other_thread_counts"] = [dict(cores=r["cores"], value=r["value"], sample=r["sample"]) for r in runs if r is not best]
    return best


def _cpu_baseline_at(model, length: int, threads: int, warm: int = 3, timed: int = 5, give_up_above=None):
    from oracle import diffusion_oracle as DO
    from oracle import unet_oracle as O
    torch.set_num_threads(threads)
    print(f"[bench] cpu_baseline: oracle fwd+bwd at B=1, L={length} on {threads} host threads ...", file=sys.stderr, flush=True)
    cfg = O.UNetConfig(dim_h=DIM_H)
    p = {k: v.detach().float().cpu().clone().requires_grad_() for k, v in model.state_dict().items()}
    x, a, c, noise, t = synth_batch(0, "cpu", 1, length)
    times = []
    gave_up = False
    for it in range(warm + timed):
        for v in p.values():
            v.grad = None
        t0 = time.perf_counter()
        loss = DO.training_loss(p, cfg, x, a, c, noise, t, cond_drop_prob=0.0)
        loss.backward()
        times.append(time.perf_counter() - t0)
        print(f"[bench] cpu_baseline: iteration {it} fwd+bwd {times[-1]:.1f} s", file=sys.stderr, flush=True)
        if give_up_above is not None and ((it == 0 and times[0] > 3.0 * give_up_above) or (it == 1 and min(times) > give_up_above)):
            gave_up = True                                 # the first iteration pays one-time allocations: give up on it alone only when it is several times
            break                                          # slower (128 threads on a 16-CPU share: 20 s against 2.9), else after the second: oversubscribed
    if gave_up:
        dt, how = min(times), f"best of {len(times)} iterations, not pursued: slower than the smaller thread count"
    else:
        dt, how = sorted(times[warm:])[timed // 2], f"median of {timed} after {warm} warm-ups"
    return dict(value=1.0 / (BATCH * dt), unit="denoise-steps/sec (B=32, linear extrapolation from B=1)", cores=threads, cpu=cpu_model(), kind="port",
                seconds_per_sample=round(dt, 3),
                sample=f"fwd+bwd of the full UNet at B=1, L={length}: {dt:.2f} s/sample ({how}; oracle/, "
                       f"fp32 + bf16 SDPA as the reference computes on CPU)")


SAMPLER_B, SAMPLER_L, SAMPLER_S, SAMPLER_CFG = 16, 8192, 50, 2.0
SAMPLER_PFLOP = 2 * (4256.0 - 1317.5) * SAMPLER_B * SAMPLER_S / 1e6 + 1317.5 * SAMPLER_B / 1e6   # = 4.72; SURVEY 8d: 4,256 GF per eval and
# sample at L=8192, two evals per step (CFG); the audio encoder's 1,317.5 GF of an eval is computed ONCE per sample (cached code)


def sampler_secondary(model, device):
    """BASELINE config 4 on the driver's clock: one 50-step DDIM sample at B=16, L=8192, cond_scale 2 (inference_gradio.py:105,128 ->
    models/diffusion.py:59-77) of the same full-size model, bf16, after a 2-step warm-up; then the same sample again, which must
    be bit-identical (fixed-order reductions while sampling)."""
    g = torch.Generator().manual_seed(7)
    a = (torch.randn(SAMPLER_B, 96, SAMPLER_L, generator=g) * 3 - 10).to(device)
    c = (torch.rand(SAMPLER_B, 5, generator=g) * 2 - 1).to(device)
    x0 = torch.randn(SAMPLER_B, 6, SAMPLER_L, generator=g).to(device)
    model.eval()
    was = model.sampling_timesteps
    from osufusion_amd import forced_compute_dtype, ops
    try:
        with forced_compute_dtype(torch.bfloat16):
            model.sampling_timesteps = 2
            model.sample(a, c, x0.clone(), cond_scale=SAMPLER_CFG)
            model.sampling_timesteps = SAMPLER_S
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            y = model.sample(a, c, x0.clone(), cond_scale=SAMPLER_CFG)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            prof = ops.KernelTimer(["osuf_mqa_fwd"])        # the repeat (bit-identity check) carries the HIP-event timing of the sampler's
            ops.set_kernel_timer(prof)                      # dominant kernel, so that the events do not sit in the timed sample
            y2 = model.sample(a, c, x0.clone(), cond_scale=SAMPLER_CFG)
            torch.cuda.synchronize()
            ops.set_kernel_timer(None)
    finally:
        model.sampling_timesteps = was
        model.train()
    roof = None
    st = prof.summary().get("osuf_mqa_fwd")
    if st:
        tfl = sum(4.0 * n.b * HEADS * int(n) * int(n) * HEAD_DIM for n in st["sizes"]) / 1e12
        ach = tfl / (st["total_ms"] / 1e3)
        pmc, (man, why) = {}, pmc_manifest()
        if man is not None:
            try:
                kern = json.loads((ROOT / man["sampler"]).read_text())["kernels"]
                pmc = next((v for k, v in kern.items() if k.startswith("mqa_fwd_kernel<8")), {})      # <8> or <8, true> (pre-scaled queries)
                why = f"{man['sampler']} [tree {man.get('tree')}] (rocprofv3 --pmc passes over tools/sampler_short.py, S = 3)"
            except (OSError, ValueError, KeyError):
                why = f"{man['sampler']} unreadable"
        traffic = (pmc.get("fetch_bytes_x2_per_launch", 0) + pmc.get("write_bytes_per_launch", 0)) or None
        roof = dict(bound="mfma", kernel="osuf_mqa_fwd", achieved=round(ach, 1), peak=MFMA_BF16_PEAK_TFLOPS, unit="TFLOP/s", frac=round(ach / MFMA_BF16_PEAK_TFLOPS, 4),
                    launches=st["launches"], mean_launch_ms=round(st["total_ms"] / st["launches"], 3), share_of_sample=round(st["total_ms"] / 1e3 / dt, 3),
                    traffic=traffic, traffic_unit="HBM-side bytes per launch (mean over the sampler's launches, N = 8192 .. 1024)",
                    mfma_busy=pmc.get("mfma_busy"), scratch_bytes_per_lane=pmc.get("scratch_bytes_per_lane"),
                    traffic_source=why)
    return dict(metric=f"DDIM sampling steps/sec at B={SAMPLER_B} L={SAMPLER_L} S={SAMPLER_S} cond_scale={SAMPLER_CFG} (BASELINE config 4), 1 MI355X",
                sampling_steps_per_s=round(SAMPLER_S / dt, 3), seconds=round(dt, 3), samples_per_s=round(SAMPLER_B / dt, 3), dtype="bf16",
                pflop=round(SAMPLER_PFLOP, 3), frac_of_peak=round(SAMPLER_PFLOP * 1e3 / dt / MFMA_BF16_PEAK_TFLOPS, 4),
                bit_identical=bool(torch.equal(y, y2)), finite=bool(torch.isfinite(y).all().item()), roofline=roof,
                note="eager launches (hipGraph replay of the step is bit-identical and no faster: GPU-bound); audio code cached, CFG as one 2B batch")


CONFIG5_B, CONFIG5_R = 64, 16


def config5_secondary(model, rank: int, device):
    """BASELINE config 5's per-GPU shard on the driver's clock (global batch 512 on 8 GPUs = 64 per GPU; trainer_peft.py:236-244 with
    r = 16 as config 5 says): the SAME weights, frozen, DoRA adapters on attn.to_q / to_kv / block1.proj / block2.proj, one warm-up
    and two timed train steps (fwd + bwd of the adapters + clip + AdamW) at B=64, L=4096, bf16."""
    from osufusion_amd.modules import lora_layers as LL
    from osufusion_amd.train import Trainer
    LL.get_peft_model(model, LL.LoraConfig(r=CONFIG5_R, lora_alpha=CONFIG5_R, use_dora=True))
    with torch.no_grad():                                  # peft zero-inits lora_B: give it life so every adapter gradient is exercised
        for m in LL.lora_modules(model):
            m.lora_B["default"].weight.normal_(0.0, 0.02)
    n_train, n_all = LL.trainable_parameter_counts(model)
    trainer = Trainer(model, lr=1e-4, weight_decay=1e-2, clip_grad_norm=1.0, compute_dtype=torch.bfloat16)
    x, a, c, noise, t = synth_batch(rank, device, CONFIG5_B, LENGTH)
    trainer.step(x, a, c, noise, t)
    torch.cuda.synchronize()
    steps = 2
    t0 = time.perf_counter()
    for _ in range(steps):
        loss, gnorm = trainer.step(x, a, c, noise, t)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    return dict(metric=f"DoRA r={CONFIG5_R} fine-tune step at per-GPU B={CONFIG5_B} L={LENGTH} (BASELINE config 5's shard of global batch 512), 1 MI355X",
                ms_per_step=round(1e3 * dt, 1), steps_per_s=round(1.0 / dt, 3), samples_per_s=round(CONFIG5_B / dt, 1), dtype="bf16",
                trainable_params=int(n_train), total_params=int(n_all), loss=round(loss.item(), 5), grad_norm=round(gnorm.item(), 4),
                finite=bool(torch.isfinite(loss).item() and torch.isfinite(gnorm).item()), timed_steps=steps, warmup=1)


def cpu_model() -> str:
    try:
        for line in Path("/proc/cpuinfo").read_text().splitlines():
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def physical_cores_in_affinity() -> int:
    """Physical cores this process may run on (`torch.set_num_threads(<physical cores>)`): distinct
    (package, core) pairs of the CPUs in the affinity mask; the mask size itself when sysfs has no topology."""
    try:
        cpus = sorted(os.sched_getaffinity(0))
    except AttributeError:
        return os.cpu_count() or 1
    cores = set()
    for c in cpus:
        try:
            base = Path(f"/sys/devices/system/cpu/cpu{c}/topology")
            cores.add(((base / "physical_package_id").read_text().strip(), (base / "core_id").read_text().strip()))
        except OSError:
            return len(cpus)
    return max(1, len(cores))


def host_thread_counts():
    """Thread counts the CPU baseline is timed at: every physical core of the affinity mask, and the
    16-thread share a 1-GPU box of the pool is entitled to (a cgroup quota, where there is one, makes the smaller count the faster)."""
    n = physical_cores_in_affinity()
    return sorted({n, min(n, 16)})


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=BATCH, help="per-GPU batch (the metric is defined at 32)")
    ap.add_argument("--length", type=int, default=LENGTH)
    ap.add_argument("--dim-h", type=int, default=DIM_H)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--lora", type=int, default=0, metavar="R",
                    help="BASELINE config 5 instead of the headline metric: DoRA rank-R adapters on attn.to_q/to_kv and "
                         "block{1,2}.proj (trainer_peft.py:236-244), base frozen; the reference runs R=32, config 5 says 16")
    ap.add_argument("--cpu-threads", type=int, default=0)
    ap.add_argument("--no-sampler", action="store_true", help="skip the secondary metric (one 50-step DDIM sample at BASELINE config 4's size)")
    ap.add_argument("--no-config5", action="store_true", help="skip the DoRA r=16, B=64 secondary (BASELINE config 5's per-GPU shard)")
    ap.add_argument("--no-fp32-mode", action="store_true", help="skip the extra fp32-compute-mode step (the mode in which the 1e-3 parity bound holds)")
    ap.add_argument("--attn-bwd", choices=["auto", "pair", "fused", "fused256", "fused512", "slabs"], default="auto",
                    help="attention backward: auto = the library default (fused sweep, atomic dQ, 256 or 512 keys per workgroup by shape); "
                         "fused256 / fused512 = force that sweep (A/B); pair = dQ + dK/dV kernels; slabs = fused, fixed-order dQ")
    ap.add_argument("--timed-mode", choices=["bf16", "fp32x3", "fp32"], default="bf16",
                    help="profiling only: run the TIMED region in an fp32 compute mode (the headline metric is bf16; such a line is labelled)")
    ap.add_argument("--grad-comm", choices=["fp32", "bf16"], default="fp32",
                    help="N > 1: element type of the gradient all-reduce (bf16 halves the xGMI bytes at one bf16 rounding per rank contribution; default fp32)")
    ap.add_argument("--no-fuse-rowdot", action="store_true", help="A/B: sum(dO*O) by the stand-alone pass instead of the to_out dgrad epilogue")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline figure does not need: the attention kernels' HIP-event roofline of the timed steps "
                         "and, on one GPU, the fp32 modes, the config-4 sampler, the CPU baseline and config 5 (subject to the --no-* switches)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed steps write what the last one computed (loss, grad norm, a seeded sample of the parameters and their "
                         "gradients) as DIR/<name>.npy, float32")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    # stdout carries the ONE JSON line and nothing else: RCCL prints a five-line version banner to fd 1 at communicator set-up (seen in the
    # one-rank rehearsal, profiles/r05_rccl_one_rank/), so fd 1 is pointed at stderr for the run and the line goes to the saved descriptor
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world} (launch N>1 with torch.distributed.run)"
    # rehearsal knobs (CPU-side testing of the N>1 path on a 1-GPU box): OSUF_DIST_BACKEND=gloo, OSUF_SINGLE_DEVICE=1
    backend = os.environ.get("OSUF_DIST_BACKEND", "nccl")
    if os.environ.get("OSUF_SINGLE_DEVICE"):
        local_rank = 0
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    # OSUF_DIST_REHEARSE=1 at N = 1: a ONE-rank process group, so that communicator set-up, the bucketed async all-reduces beside the backward and
    # the comm diagnostics below run through RCCL on a 1-GPU box (no bytes cross a link; everything else is the N > 1 code path)
    rehearse = world == 1 and os.environ.get("OSUF_DIST_REHEARSE") == "1"
    if rehearse:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
    dist_on = world > 1 or rehearse
    if dist_on:
        if backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=device)  # "nccl" is RCCL on ROCm
        else:
            dist.init_process_group(backend=backend)

    from osufusion_amd import ops
    from osufusion_amd.train import Trainer

    model = build_model(device, args.dim_h)
    if args.lora:
        from osufusion_amd.modules import lora_layers as LL
        LL.get_peft_model(model, LL.LoraConfig(r=args.lora, lora_alpha=args.lora, use_dora=True))
        with torch.no_grad():                              # peft zero-inits lora_B: give it life so every adapter gradient is exercised
            for m in LL.lora_modules(model):
                m.lora_B["default"].weight.normal_(0.0, 0.02)
    if args.no_fuse_rowdot:
        ops.FUSE_ROWDOT = False
    if args.attn_bwd != "auto":
        ops.ATTN_BWD_DEFAULT = {"fused": ops.ATTN_FUSED, "slabs": ops.ATTN_FUSED_SLABS, "pair": ops.ATTN_AUTO, "fused256": ops.ATTN_FUSED256,
                                "fused512": ops.ATTN_FUSED512}[args.attn_bwd]
    trainer = Trainer(model, lr=1e-4, weight_decay=1e-2, clip_grad_norm=1.0,
                      compute_dtype=torch.bfloat16 if args.timed_mode == "bf16" else torch.float32,
                      comm_dtype=torch.bfloat16 if args.grad_comm == "bf16" else None)
    if args.timed_mode == "fp32x3":
        ops.set_f32_matmul("x3")
    x, a, c, noise, t = synth_batch(rank, device, args.batch, args.length)

    def sync():
        torch.cuda.synchronize()
        if dist_on:
            dist.barrier()
        torch.cuda.synchronize()

    # Every step, warm-up and timed, starts from the same seeded parameters, restored between the steps and outside the timed spans.
    # The float-atomic reductions of a step (dQ, weight and bias gradients, GroupNorm statistics) round differently from run to run, and
    # along an evolving trajectory those differences compound step by step; from a fixed start a step's outputs are a function of its
    # inputs, equal to rounding in every run.  The AdamW moments still accumulate over the steps, as in training.
    from osufusion_amd import functional as Fn
    start = [(p, p.detach().clone()) for p in trainer.flat.params]

    def restore():
        with torch.no_grad():
            torch._foreach_copy_([p.data for p, _ in start], [v for _, v in start])
        Fn.bump_weight_epoch()                             # written behind autograd's back, as the fused optimizer does; then the
        for job in Fn._PACK_JOBS.values():                 # grouped re-pack of the step's end again (it only takes the packs used
            job.used = True                                # since its last call), so the next step finds its GEMM operands current
        Fn.refresh_packs()

    if rank == 0:
        print(f"[bench] model + data resident; {args.warmup} warmup + {args.steps} timed steps ...", file=sys.stderr, flush=True)
    for _ in range(args.warmup):
        restore()
        trainer.step(x, a, c, noise, t)
    sync()
    prof = ops.KernelTimer(list(ATTN_UNITS)) if args.full else None
    ops.set_kernel_timer(prof)
    spans = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
    for t_start, t_end in spans:                           # timed by events on the stream: the restore in between is not counted,
        restore()                                          # and the host runs ahead of the GPU as in back-to-back steps
        t_start.record()
        loss, gnorm = trainer.step(x, a, c, noise, t)
        t_end.record()
    sync()
    elapsed = sum(s.elapsed_time(e) for s, e in spans) / 1e3
    ops.set_kernel_timer(None)
    start.clear()
    if args.dump_outputs and rank == 0:                    # before anything below touches the parameters or gradients
        names = dump_outputs(args.dump_outputs, model, loss, gnorm)
        print(f"[bench] outputs of the last timed step written to {args.dump_outputs}: {', '.join(names)}", file=sys.stderr, flush=True)
    if dist_on:
        tmax = torch.tensor([elapsed], dtype=torch.float64, device=device)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        elapsed = tmax.item()

    comm = None
    if dist_on:
        # what a first multi-GPU run needs to diagnose itself: what the reducer did in the last timed step on this rank, the same over
        # all ranks, and the gradient all-reduce ALONE (all buckets back to back on an idle GPU: the xGMI-bound part of a step)
        comm = trainer.comm_stats()
        per_rank = [None] * world
        dist.all_gather_object(per_rank, {k: comm[k] for k in ("buckets_fired_before_finish", "out_of_order_completions", "finish_wait_ms",
                                                                "order_disagreements", "layout_fingerprint", "allreduce_bytes")})
        red = trainer.reducer
        alone = []
        for _ in range(3):
            sync()
            t1 = time.perf_counter()
            hs = [dist.all_reduce(trainer.flat.grad[s0:e0], op=dist.ReduceOp.SUM, async_op=True) for s0, e0 in red.bounds]
            for h in hs:
                h.wait()
            torch.cuda.synchronize()
            alone.append(time.perf_counter() - t1)
        alone_t = torch.tensor([min(alone)], dtype=torch.float64, device=device)
        dist.all_reduce(alone_t, op=dist.ReduceOp.MAX)
        nbytes = trainer.flat.grad.numel() * trainer.flat.grad.element_size()
        comm.update(per_rank=per_rank, devices_visible=torch.cuda.device_count(), device=torch.cuda.get_device_name(device),
                    allreduce_alone_ms=round(1e3 * alone_t.item(), 3),
                    allreduce_alone_busbw_gbs=round(2 * (world - 1) / world * nbytes / alone_t.item() / 1e9, 1), rehearsal=rehearse,
                    fingerprints_agree=len({r["layout_fingerprint"] for r in per_rank}) == 1)
    if rank == 0:
        print(f"[bench] timed region done: {1e3 * elapsed / args.steps:.1f} ms/step", file=sys.stderr, flush=True)
        ms = 1e3 * elapsed / args.steps
        full = (args.batch, args.length, args.dim_h) == (BATCH, LENGTH, DIM_H)
        value = world * args.steps / elapsed * (args.batch / BATCH)
        # roofline of the dominant kernel: algorithmic FLOPs per launch / mean launch duration (HIP events, timed region; --full only)
        stats = prof.summary() if prof is not None else {}
        dom = max(stats, key=lambda k: stats[k]["total_ms"]) if stats else None
        roof = None
        if dom is not None:
            def tflop(name, which):                        # FLOPs of all timed launches of one entry point
                return sum(ATTN_UNITS[name][which] * args.batch * HEADS * n * n * HEAD_DIM for n in stats[name]["sizes"]) / 1e12
            sec = stats[dom]["total_ms"] / 1e3
            ach, exe = tflop(dom, 0) / sec, tflop(dom, 1) / sec
            traffic, tsrc = pmc_traffic(dom) if full else (None, None)
            bwd = [k for k in stats if k != "osuf_mqa_fwd"]
            bwd_ms = sum(stats[k]["total_ms"] for k in bwd)
            busy, bsrc = pmc_mfma_busy() if (full and dom == "osuf_mqa_bwd_fused") else (None, None)
            roof = dict(bound="mfma", kernel=dom, achieved=round(ach, 1), peak=MFMA_BF16_PEAK_TFLOPS, unit="TFLOP/s",
                        frac=round(ach / MFMA_BF16_PEAK_TFLOPS, 4), traffic=traffic, traffic_unit="HBM-side bytes per launch", traffic_source=tsrc,
                        flops="algorithmic (SURVEY 8d: attention backward = 2 x forward, recomputed products not counted)",
                        executed=round(exe, 1), executed_frac=round(exe / MFMA_BF16_PEAK_TFLOPS, 4), launches=stats[dom]["launches"],
                        mfma_busy=busy, mfma_busy_source=bsrc,
                        mean_launch_ms=round(stats[dom]["total_ms"] / stats[dom]["launches"], 3),
                        attention_backward=dict(kernels=bwd, ms_per_step=round(bwd_ms / args.steps, 2),
                                                achieved=round(sum(tflop(k, 0) for k in bwd) / (bwd_ms / 1e3), 1) if bwd_ms else None),
                        step_frac_of_peak=round(STEP_TFLOP / (ms / 1e3) / MFMA_BF16_PEAK_TFLOPS, 4) if full else None,
                        all_kernels_ms_per_step={k: round(v["total_ms"] / args.steps, 2) for k, v in stats.items()})
        metric = "denoise-steps/sec (train fwd+bwd) at B=32 L=4096"
        if args.lora:
            metric = f"DoRA r={args.lora} fine-tune steps/sec at B={args.batch} L={args.length} (BASELINE config 5, per-GPU shard)"
            value = world * args.steps / elapsed
        out = {
            "metric": metric, "value": round(value, 4), "unit": "steps/s", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms, 2), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "bf16", "data": "synthetic (SURVEY 8d shapes; random-init weights, live final_conv)",
            "config": {"workload": (f"trainer_peft path: frozen base + DoRA r={args.lora} on attn.to_q/to_kv/block1.proj/block2.proj "
                                    f"({trainer.flat.numel / 1e6:.1f}M trainable); " if args.lora else "") +
                                   f"full OsuFusion UNet dim_h={args.dim_h} (343.5M params) train step: fwd+bwd+grad-norm+clip+AdamW"
                                   f"{'+RCCL all-reduce' if world > 1 else '+one-rank RCCL all-reduce (rehearsal)' if rehearse else ''}, per-GPU batch {args.batch}, L={args.length}, x (B,6,L), "
                                   f"audio (B,96,L) [BASELINE 'audio-ctx=1024x128' maps to the (B,1024,L/8) bottleneck code]",
                       "global_batch": args.batch * world, "seq_len": args.length, "parallelism": f"dp{world}"},
            "loss": round(loss.item(), 5), "grad_norm": round(gnorm.item(), 4),
        }
        if args.full:
            out["roofline"] = roof
        if comm is not None:
            out["comm"] = comm

        def guarded(key, fn):
            """A failing secondary must not lose the primary line: record the error under its key and go on."""
            try:
                out[key] = fn()
            except Exception as e:                         # noqa: BLE001
                out[key] = {"error": f"{type(e).__name__}: {e}"[:400]}
                print(f"[bench] secondary '{key}' failed: {out[key]['error']}", file=sys.stderr, flush=True)
        if args.timed_mode != "bf16":
            out["metric"] += f" [PROFILING RUN in the {args.timed_mode} compute mode -- not the headline number]"
            out["dtype"] = args.timed_mode
        more = world == 1 and args.full                    # the single-GPU legs beyond the headline figure
        if more and not args.no_fp32_mode and not args.lora and full and args.timed_mode == "bf16":
            # the compute mode in which north_star's 1e-3 bound holds (exact-f32 MFMA everywhere, bf16 only where the reference casts):
            # one warm-up + two timed steps (the faster is reported), after the timed region; bf16 (timed above) sits at the reference's own autocast distance
            def fp32_modes():
                trainer.compute_dtype = torch.float32
                res = {}
                for key, mm in (("fp32x3_mode_ms_per_step", "x3"), ("fp32_mode_ms_per_step", "exact")):
                    prev = ops.set_f32_matmul(mm)          # x3: fp32 storage, GEMM products as three bf16 MFMAs on split operands (~17 bits);
                    try:                                   # exact: v_mfma_f32_32x32x2_f32, the reference's fp32 arithmetic bit for bit
                        trainer.step(x, a, c, noise, t)
                        torch.cuda.synchronize()
                        best = None                        # two timed steps, the faster one: a single step after a mode switch still saw allocator
                        for _ in range(2):                 # growth on some boxes (x3: 294.5 and 332.7 ms on two boxes of the same tree)
                            t1 = time.perf_counter()
                            trainer.step(x, a, c, noise, t)
                            torch.cuda.synchronize()
                            dt1 = time.perf_counter() - t1
                            best = dt1 if best is None else min(best, dt1)
                        res[key] = round(1e3 * best, 1)
                    finally:
                        ops.set_f32_matmul(prev)
                return res
            # (key names: fp32_mode_ms_per_step is the EXACT-f32 mode in every round's record but round 3's, which printed the x3 mode
            #  under that key and the exact one under fp32_exact_mode_ms_per_step -- kept as an alias)
            guarded("fp32_modes", fp32_modes)
            if "error" not in out["fp32_modes"]:
                out.update(out.pop("fp32_modes"))
                out["fp32_exact_mode_ms_per_step"] = out["fp32_mode_ms_per_step"]
            out["parity_note"] = ("bf16 (timed) vs the fp32 golden of the imported reference (unet_mid): output 8.5e-3, flat gradient 6.6e-3 -- the reference's OWN "
                                  "bf16 autocast (trainer.py:295,374; tests/golden/unet_mid_autocast.npz) sits at 1.08e-2 / 8.0e-3 from its fp32 run, per-parameter "
                                  "HIP / reference ratio max 1.16, median 0.82 (tests/test_hip_parity.py::test_unet_bf16_vs_reference_autocast); both fp32 modes are "
                                  "held to 1e-3 at full size by tests/test_full_size.py (forward of two samples and all 1,239 gradients of one sample, each with "
                                  "set_f32_matmul('exact') and ('x3')): fp32x3_mode = split-bf16 GEMMs, fp32_mode = f32 MFMA")
        if more and not args.no_sampler and not args.lora and full:
            print("[bench] secondary: DDIM sample at config 4's size ...", file=sys.stderr, flush=True)
            guarded("secondary", lambda: sampler_secondary(model, device))
        if more and not args.no_cpu_baseline and not args.lora:
            guarded("cpu_baseline", lambda: cpu_baseline(model, args.length, [args.cpu_threads] if args.cpu_threads else host_thread_counts()))
            if "value" in out["cpu_baseline"]:
                out["gpu_over_cpu"] = round(out["value"] / out["cpu_baseline"]["value"], 1)
        if more and not args.no_config5 and not args.lora and full:
            print("[bench] config 5: DoRA r=16 steps at the per-GPU shard B=64 ...", file=sys.stderr, flush=True)
            del trainer
            guarded("config5", lambda: config5_secondary(model, rank, device))      # LAST: wraps the model's layers in place
        sys.stdout.flush()
        os.write(json_fd, (json.dumps(out) + "\n").encode())
    if dist_on:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
