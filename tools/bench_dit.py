"""Timing of the DiT backbone (osufusion_amd/modules/dit.py) at the reference's defaults against torch eager + SDPA in the same process.

    python tools/bench_dit.py [--out profiles/dit_step.json] [--B 32] [--L 4096] [--steps 5] [--no-eager] [--rows-only]

Model: DiT(6, 96, 5, 512) = depth 12, 8 x 64 heads, FF x4, bf16 compute.  Rows:
  * hip: the HIP module (forced bf16 compute), train step = forward + MSE + backward (no optimizer), forward-only under no_grad;
  * eager: the same parameters through the plain-torch restatement (tests/dit_oracle.py) under torch.autocast("cuda", bfloat16) with
    F.scaled_dot_product_attention on bf16 q / k / v -- what the reference runs on a GPU;
  * row kernels alone at M = B * L, C = 512 bf16: adaLN forward / backward and QK-norm forward / backward, effective TB/s over the
    bytes each must move (read + write once).
A timing tool, not a gate: medians of event-timed repetitions after warm-up; peak memory from torch's allocator per row."""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from osufusion_amd import dit as Dt  # noqa: E402
from osufusion_amd import forced_compute_dtype  # noqa: E402
from osufusion_amd.modules.dit import DiT  # noqa: E402
from tests import dit_oracle as O  # noqa: E402

DEV = "cuda"


def timeit(fn, warmup=2, reps=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e))
    return statistics.median(ts)


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 30, 2)


def sdpa_bf16(q, k, v):
    dt = v.dtype
    q, k, v = (z.to(torch.bfloat16) for z in (q, k, v))
    return F.scaled_dot_product_attention(q, k, v).to(dt)


def row_kernels(B, L, C=512, H=8, D=64):
    M = B * L
    x = torch.randn(B, L, C, device=DEV).bfloat16()
    mod = torch.randn(B, 6 * C, device=DEV) * 0.1
    dy = torch.randn(B, L, C, device=DEV).bfloat16()
    raw = torch.randn(B, L, 3 * C, device=DEV).bfloat16()
    g = torch.randn(B, L, 3 * C, device=DEV)
    gq = torch.ones(H, 1, D, device=DEV)
    out, mr = Dt.adaln_fwd(x, mod[:, :C], mod[:, C:2 * C])
    _, inv = Dt.qknorm_fwd(raw, gq, gq, H, D)
    rows = []
    cases = (("adaln_fwd", lambda: Dt.adaln_fwd(x, mod[:, :C], mod[:, C:2 * C]), M * C * 2 * 2 + M * 8),
             ("adaln_bwd", lambda: Dt.adaln_bwd(dy, x, mr, mod[:, C:2 * C], None), M * C * 2 * 3 + M * 8),
             ("adaln_bwd+dres", lambda: Dt.adaln_bwd(dy, x, mr, mod[:, C:2 * C], out), M * C * 2 * 4 + M * 8),
             ("qknorm_fwd", lambda: Dt.qknorm_fwd(raw, gq, gq, H, D), M * 3 * C * 2 * 2 + M * 2 * H * 4),
             ("qknorm_bwd", lambda: Dt.qknorm_bwd(g, raw, inv, gq, gq, H, D), M * 3 * C * (4 + 2 + 2) + M * 2 * H * 4))
    for name, fn, nbytes in cases:
        ms = timeit(fn, 3, 20)
        rows.append({"kernel": name, "M": M, "C": C, "ms": round(ms, 4), "TB_s": round(nbytes / (ms / 1e3) / 1e12, 2)})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--L", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--no-eager", action="store_true")
    ap.add_argument("--rows-only", action="store_true")
    args = ap.parse_args()
    B, L = args.B, args.L
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "B": B, "L": L,
           "model": "DiT(6, 96, 5, 512): depth 12, 8 x 64 heads, FF x4", "dtype": "bf16"}
    res["row_kernels"] = row_kernels(B, L)
    if not args.rows_only:
        torch.manual_seed(0)
        net = DiT(6, 96, 5, 512).to(DEV)
        with torch.no_grad():                                # the reference zero-inits adaLN / postprocess: use live weights instead
            for p in net.parameters():
                if not p.any():
                    p.normal_(0, 0.02)
        x = torch.rand(B, 6, L, device=DEV) * 2 - 1
        a = torch.rand(B, 96, L, device=DEV) * 10 - 15
        c = torch.rand(B, 5, device=DEV) * 2 - 1
        t = torch.randint(0, 1000, (B,), device=DEV)
        noise = torch.randn(B, 6, L, device=DEV)

        def hip_step():
            net.zero_grad(set_to_none=True)
            with forced_compute_dtype(torch.bfloat16):
                F.mse_loss(net(x, a, t, c), noise).backward()

        def hip_fwd():
            with torch.no_grad(), forced_compute_dtype(torch.bfloat16):
                net(x, a, t, c)

        hip = {"step_ms": round(timeit(hip_step, 2, args.steps), 2), "fwd_ms": round(timeit(hip_fwd, 2, args.steps), 2),
               "step_peak_GiB": peak(hip_step), "fwd_peak_GiB": peak(hip_fwd)}
        res["hip"] = hip
        print(json.dumps({"hip": hip}), flush=True)
        net.zero_grad(set_to_none=True)
        if not args.no_eager:
            p = {k: v.detach().clone().requires_grad_() for k, v in net.state_dict().items()}
            cfg = O.DiTConfig()

            def eager_step():
                for v in p.values():
                    v.grad = None
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    y = O.dit_forward(p, cfg, x, a, t, c, attend=sdpa_bf16)
                F.mse_loss(y.float(), noise).backward()

            def eager_fwd():
                with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                    O.dit_forward(p, cfg, x, a, t, c, attend=sdpa_bf16)

            try:
                eager = {"step_ms": round(timeit(eager_step, 2, args.steps), 2), "fwd_ms": round(timeit(eager_fwd, 2, args.steps), 2),
                         "step_peak_GiB": peak(eager_step), "fwd_peak_GiB": peak(eager_fwd)}
            except RuntimeError as e:                        # out of memory or no SDPA backend
                eager = {"error": str(e).split("\n")[0][:200]}
            res["eager_sdpa"] = eager
            print(json.dumps({"eager_sdpa": eager}), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
