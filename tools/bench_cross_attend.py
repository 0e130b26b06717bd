"""Timing of the stand-alone Attend module with k / v of another length than q (osufusion_amd/cross_attend.py), forward and forward +
backward, against torch's own SDPA on the same tensors and the same GPU.

    python tools/bench_cross_attend.py [--out profiles/cross_attend.json] [--reps 20]

B = 32, H = 8, D = 64, k / v with one head (the dK/dV kernel sums the query heads), fp32 leaves as a model would hand them over;
(Nq, Nk) in {(4096, 256), (4096, 1024), (1024, 4096)}, unmasked and with a dense (B, H, Nq, Nk) bf16 mask (no grad on it).  The last
column per row is the backward launch pair alone with its dK/dV workgroup count ceil(Nk / 128) * B: the baseline for a later query split.
A timing tool, not a gate: medians of event-timed repetitions after warm-up."""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from osufusion_amd import cross_attend as Xa  # noqa: E402
from osufusion_amd.modules.attention import Attend  # noqa: E402

B, H, D = 32, 8, 64
SHAPES = ((4096, 256), (4096, 1024), (1024, 4096))
DEV = "cuda"


def timeit(fn, warmup, reps):
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


def fwd_bwd(fn, q, k, v, go, mask):
    def run():
        for t in (q, k, v):
            t.grad = None
        fn(q, k, v, mask).backward(go)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_cross_attend.py needs a GPU: nothing is measured without one")
    att = Attend()
    ours = lambda q, k, v, m: att(q, k, v, attn_mask=m)

    def sdpa(q, k, v, m):
        qb, kb, vb = (t.to(torch.bfloat16) for t in (q, k, v))
        return F.scaled_dot_product_attention(qb, kb.expand(-1, H, -1, -1), vb.expand(-1, H, -1, -1), attn_mask=m).to(v.dtype)

    tm = lambda fn: timeit(fn, args.warmup, args.reps)
    rows = []
    for Nq, Nk in SHAPES:
        torch.manual_seed(0)
        q = torch.randn(B, H, Nq, D, device=DEV).requires_grad_()
        k, v = (torch.randn(B, 1, Nk, D, device=DEV).requires_grad_() for _ in range(2))
        go = torch.randn(B, H, Nq, D, device=DEV)
        dense = torch.randn(B, H, Nq, Nk, device=DEV).to(torch.bfloat16)
        flops_fwd = 4.0 * B * H * Nq * Nk * D                  # algorithmic: forward 4 B H Nq Nk D, backward twice that
        for name, mask in (("unmasked", None), ("dense mask", dense)):
            rec = {"Nq": Nq, "Nk": Nk, "case": name, "dkv_workgroups": -(-Nk // 128) * B}
            with torch.no_grad():
                rec["ours_fwd_ms"] = tm(lambda: ours(q, k, v, mask))
            rec["ours_fwd_bwd_ms"] = tm(fwd_bwd(ours, q, k, v, go, mask))
            try:
                with torch.no_grad():
                    rec["sdpa_fwd_ms"] = tm(lambda: sdpa(q, k, v, mask))
                rec["sdpa_fwd_bwd_ms"] = tm(fwd_bwd(sdpa, q, k, v, go, mask))
            except RuntimeError as e:                          # no SDPA backend for this case on this build
                rec["sdpa_error"] = str(e).split("\n")[0][:200]
            # the backward launch pair alone (osuf_attn_delta + dQ + dK/dV), on the rows the module would keep
            rq, rk, rv = (Xa._rows(t.detach(), torch.bfloat16) for t in (q, k, v))
            o, lse = Xa.xattn_fwd(rq, rk, rv, mask, B, Nq, Nk, H, D, torch.bfloat16, D ** -0.5)
            do = Xa._rows(go, torch.bfloat16)
            rec["ours_bwd_kernels_ms"] = tm(lambda: Xa.xattn_bwd(rq, rk, rv, mask, o, do, lse, B, Nq, Nk, H, D, D ** -0.5, False))
            rec["ours_fwd_tflops_alg"] = round(flops_fwd / (rec["ours_fwd_ms"] / 1e3) / 1e12, 2)
            rec["ours_bwd_kernels_tflops_alg"] = round(2.0 * flops_fwd / (rec["ours_bwd_kernels_ms"] / 1e3) / 1e12, 2)
            rows.append(rec)
            print(json.dumps(rec), flush=True)
            del o, lse, do, rq, rk, rv
        del dense
    if args.out:
        out = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "B": B, "H": H, "D": D, "kv_heads": 1,
               "warmup": args.warmup, "reps": args.reps, "rows": rows}
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
