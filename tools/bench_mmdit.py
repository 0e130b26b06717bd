"""Timing of the MMDiT backbone (osufusion_amd/modules/mmdit.py) against torch eager + SDPA in the same process.

    python tools/bench_mmdit.py [--out profiles/mmdit_step.json] [--B 32] [--L 4096] [--dim 512] [--heads 8] [--kv-heads 2] [--depth 12]
                                [--patch 4] [--steps 5] [--no-eager] [--rows-only]

Model: MMDiT(6, 96, 5, dim) with heads x (dim / heads) attention on kv-heads K/V heads, FF x4, bf16 compute; each stream has L / patch rows
and the joint attention runs over 2 L / patch.  Rows:
  * hip: the HIP module (forced bf16 compute), train step = forward + MSE + backward (no optimizer), forward-only under no_grad;
  * eager: the same parameters through the plain-torch restatement (tests/mmdit_oracle.py) under torch.autocast("cuda", bfloat16) with
    F.scaled_dot_product_attention on bf16 q / k / v -- what the reference runs on a GPU;
  * the joint-attention row kernels alone on one stream of M = B * L / patch rows (bf16 raw rows): effective TB/s over the bytes each
    must move (read + write once).
A timing tool, not a gate: medians of event-timed repetitions after warm-up; peak memory from torch's allocator per row."""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from osufusion_amd import forced_compute_dtype  # noqa: E402
from osufusion_amd import mmdit as Mm  # noqa: E402
from osufusion_amd.modules.mmdit import MMDiT  # noqa: E402
from tests import mmdit_oracle as O  # noqa: E402
from tools.bench_dit import peak, sdpa_bf16, timeit  # noqa: E402

DEV = "cuda"


def row_kernels(B, N, H, G, D):
    """One stream (the second half of a joint buffer of 2 N rows per sample)."""
    M, W, HD = B * N, (H + 2 * G) * D, H * D
    raw = torch.randn(B, N, W, device=DEV).bfloat16()
    g = torch.randn(B, 2 * N, W, device=DEV)
    o = torch.randn(B, N, HD, device=DEV).bfloat16()
    gq, gk = torch.ones(H, 1, D, device=DEV), torch.ones(G, 1, D, device=DEV)
    joint, jo = Mm.joint_buffer(B, 2 * N, W, DEV), Mm.joint_buffer(B, 2 * N, HD, DEV)
    inv = Mm.joint_qknorm_fwd(raw, joint, N, gq, gk, H, G, D)
    rows = []
    cases = (("joint_qknorm_fwd", lambda: Mm.joint_qknorm_fwd(raw, joint, N, gq, gk, H, G, D), M * W * 2 * 2 + M * (H + G) * 4),
             ("joint_qknorm_bwd", lambda: Mm.joint_qknorm_bwd(g, raw, N, inv, gq, gk, H, G, D), M * W * (4 + 2 + 2) + M * (H + G) * 4),
             ("joint_pack", lambda: Mm.joint_pack(o, jo, N, H, G, D), M * HD * 2 * 2),
             ("joint_unpack", lambda: Mm.joint_unpack(jo, N, N, torch.bfloat16, H, G, D), M * HD * 2 * 2))
    for name, fn, nbytes in cases:
        ms = timeit(fn, 3, 20)
        rows.append({"kernel": name, "M": M, "H": H, "G": G, "D": D, "ms": round(ms, 4), "TB_s": round(nbytes / (ms / 1e3) / 1e12, 2)})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--L", type=int, default=4096)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--heads", type=int, default=8)
    ap.add_argument("--kv-heads", type=int, default=2)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--patch", type=int, default=4)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--no-eager", action="store_true")
    ap.add_argument("--rows-only", action="store_true")
    args = ap.parse_args()
    B, L, H, G, D = args.B, args.L, args.heads, args.kv_heads, args.dim // args.heads
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "B": B, "L": L, "dtype": "bf16",
           "model": f"MMDiT(6, 96, 5, {args.dim}): depth {args.depth}, {H} x {D} heads on {G} K/V heads, patch {args.patch}, FF x4"}
    res["row_kernels"] = row_kernels(B, -(-L // args.patch), H, G, D)
    if not args.rows_only:
        torch.manual_seed(0)
        net = MMDiT(6, 96, 5, args.dim, depth=args.depth, patch_size=args.patch, attn_dim_head=D, attn_heads=H, attn_kv_heads=G).to(DEV)
        with torch.no_grad():                                # the reference zero-inits adaLN / final layer / out: use live weights instead
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
            cfg = O.MMDiTConfig(dim_h=args.dim, depth=args.depth, patch_size=args.patch, heads=H, kv_heads=G, dim_head=D)

            def eager_step():
                for v in p.values():
                    v.grad = None
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    y = O.mmdit_forward(p, cfg, x, a, t, c, attend=sdpa_bf16)
                F.mse_loss(y.float(), noise).backward()

            def eager_fwd():
                with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                    O.mmdit_forward(p, cfg, x, a, t, c, attend=sdpa_bf16)

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
