"""Timing of the stand-alone Attend module, forward + backward (osufusion_amd/attend.py, cross_attend.py), against torch's own SDPA on the same GPU.

    python tools/bench_attend.py [--out profiles/attend_fwd_bwd.json] [N ...]

B = 2, H = 8, D = 64, one K/V head per query head, fp32 leaves as a model would hand them over.  Rows:
  * unmasked: ops.mqa_fwd + the tuned fused backward sweep;
  * causal (N, N) float mask, no grad on it: the generic kernels (cross_attend.py: osuf_xattn_fwd / osuf_xattn_bwd with Nk = N), one launch set per head;
  * the same with the mask requiring grad (dense fp32 dbias [B][H][N][N] stored, then summed to (N, N));
  * the masked backward kernels alone with a broadcast (1, 1, N, N) and a dense (B, H, N, N) bias: how much the per-lane bias gather costs.
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

B, H, D = 2, 8, 64
DEV = "cuda"


def timeit(fn, warmup=3, reps=10):
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
        if mask is not None and mask.requires_grad:
            mask.grad = None
        fn(q, k, v, mask).backward(go)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("sizes", nargs="*", type=int)
    args = ap.parse_args()
    att = Attend()
    ours = lambda q, k, v, m: att(q, k, v, attn_mask=m)

    def sdpa(q, k, v, m):
        qb, kb, vb = (t.to(torch.bfloat16) for t in (q, k, v))
        return F.scaled_dot_product_attention(qb, kb, vb, attn_mask=None if m is None else m.to(torch.bfloat16)).to(v.dtype)

    rows = []
    for N in args.sizes or [1024, 4096]:
        torch.manual_seed(0)
        q, k, v = (torch.randn(B, H, N, D, device=DEV).requires_grad_() for _ in range(3))
        go = torch.randn(B, H, N, D, device=DEV)
        causal = torch.zeros(N, N, device=DEV).masked_fill(torch.ones(N, N, device=DEV, dtype=torch.bool).triu(1), float("-inf"))
        causal_g = causal.clone().requires_grad_()
        flops = 4.0 * B * H * N * N * D * 3.0              # algorithmic: forward 4 B H N^2 D, backward twice that
        for name, mask in (("unmasked", None), ("causal", causal), ("causal+dmask", causal_g)):
            rec = {"N": N, "case": name}
            rec["ours_fwd_ms"] = timeit(lambda: ours(q.detach(), k.detach(), v.detach(), None if mask is None else mask.detach()))
            rec["ours_fwd_bwd_ms"] = timeit(fwd_bwd(ours, q, k, v, go, mask))
            try:
                rec["sdpa_fwd_ms"] = timeit(lambda: sdpa(q.detach(), k.detach(), v.detach(), None if mask is None else mask.detach()))
                rec["sdpa_fwd_bwd_ms"] = timeit(fwd_bwd(sdpa, q, k, v, go, mask))
            except RuntimeError as e:                      # no SDPA backend for this case on this build
                rec["sdpa_error"] = str(e).split("\n")[0][:200]
            rec["ours_fwd_bwd_tflops_alg"] = round(flops / (rec["ours_fwd_bwd_ms"] / 1e3) / 1e12, 2)
            rows.append(rec)
            print(json.dumps(rec), flush=True)
        # the masked backward kernels alone (one launch set over all H heads, one K/V head): broadcast vs dense bias
        qkv = torch.randn(B, N, (H + 2) * D, device=DEV).to(torch.bfloat16)
        qc, kc, vc = qkv[..., :H * D], qkv[..., H * D:(H + 1) * D], qkv[..., (H + 1) * D:]      # column views of the q|k|v image
        do = torch.randn(B, N, H * D, device=DEV).to(torch.bfloat16)
        for name, m4 in (("bwd_kernels/bias(1,1,N,N)", causal.to(torch.bfloat16).expand(B, H, N, N)),
                         ("bwd_kernels/bias(B,H,N,N)", causal.to(torch.bfloat16).expand(B, H, N, N).contiguous())):
            o, lse = Xa.xattn_fwd(qc, kc, vc, m4, B, N, N, H, D, torch.bfloat16, D ** -0.5)
            rec = {"N": N, "case": name, "kv_heads": 1}
            rec["ms"] = timeit(lambda: Xa.xattn_bwd(qc, kc, vc, m4, o, do, lse, B, N, N, H, D, D ** -0.5, False))
            rec["ms_with_dbias"] = timeit(lambda: Xa.xattn_bwd(qc, kc, vc, m4, o, do, lse, B, N, N, H, D, D ** -0.5, True))
            rec["tflops_alg"] = round(4.0 * B * H * N * N * D * 2.0 / (rec["ms"] / 1e3) / 1e12, 2)
            rows.append(rec)
            print(json.dumps(rec), flush=True)
    if args.out:
        out = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "B": B, "H": H, "D": D, "rows": rows}
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
