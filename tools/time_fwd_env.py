"""Forward attention (pre-scaled queries) A/B on one ops.force switch, interleaved in one process: attn_fwd_nowhole (the default: the kernel without /
with the bounds checks of its K / V loads, bit-identical) or attn_fwd_noqsk (the QS kernel -- running maximum as the S chain's C operand -- against
the plain kernel fed the same queries: equal to rounding).   python tools/time_fwd_env.py [SWITCH]"""
import contextlib, sys
sys.path.insert(0, "/root/repo")
import torch
from osufusion_amd import ops
VAR = sys.argv[1] if len(sys.argv) > 1 else "attn_fwd_nowhole"
ops.force(**{VAR: True})                                      # an unknown name stops here
D = 64
for B, N, H in ((32, 4096, 16), (32, 2048, 16), (32, 1024, 16), (32, 512, 16), (32, 8192, 16)):
    qkv = torch.randn(B, N, (H + 2) * D, device="cuda").to(torch.bfloat16)
    qkv[..., : H * D] = (qkv[..., : H * D].float() * (D ** -0.5 * ops.LOG2E)).to(torch.bfloat16)
    outs, ts = {}, {False: [], True: []}
    for rnd in range(3):
        for old in (False, True):
            fn = lambda: ops.mqa_fwd(qkv, B, N, H, D, torch.bfloat16, D ** -0.5, qs=True)
            with ops.force(**{VAR: True}) if old else contextlib.nullcontext():
                outs[old] = fn()
                for _ in range(2): fn()
                torch.cuda.synchronize()
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for _ in range(8): fn()
                e.record(); torch.cuda.synchronize()
            ts[old].append(s.elapsed_time(e) / 8)
    f = 4.0 * B * H * N * N * D
    same = torch.equal(outs[False][0], outs[True][0]) and torch.equal(outs[False][1], outs[True][1])
    eo = ((outs[False][0].float() - outs[True][0].float()).norm() / outs[True][0].float().norm()).item()
    el = (outs[False][1] - outs[True][1]).abs().max().item()
    print(f"B={B} N={N}: {VAR} {min(ts[True]):.3f} ms ({f / min(ts[True]) / 1e9:5.0f} TF/s)   default {min(ts[False]):.3f} ms ({f / min(ts[False]) / 1e9:5.0f} TF/s)   "
          f"bit-identical {same}  o rel diff {eo:.2e}  lse max diff {el:.2e}", flush=True)
