"""osuf_gqa_fwd (ops.gqa_fwd): the grouped-query attention forward with the K/V group as a grid dimension, against the launch-per-group
loop of ops.mqa_fwd(kv_heads=G) bit for bit, against fp64 softmax(q k^T scale) v, through its argument checks, and on poisoned memory."""
import numpy as np
import pytest
import torch

from osufusion_amd import _lib, ops
from tests.test_poisoned_memory import relmax, rell2, rnd, run_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
B = 2
# (H, G, D): r = 3 (a workgroup's waves straddle query blocks unevenly), r = 1 (the DiT), G = 1 (osuf_mqa_fwd itself), tuned (64) and generic kernels
HGD = [(6, 2, 16), (4, 4, 32), (8, 2, 64), (2, 1, 64), (6, 3, 64), (4, 2, 128), (3, 3, 64)]
# shorter than a key tile; the WHOLE path; ragged last tile and query block; three whole tiles
LENGTHS = [40, 64, 100, 192]
# tests/test_hip_parity.py::test_mqa_flash_vs_sdpa's bounds (bf16 P and bf16 output rounding)
O_RELMAX, O_RELL2, LSE_ABS = 1.5e-2, 5e-3, 2e-3


def _qkv(H, G, D, N):
    return rnd("qkv", (B, N, (H + 2 * G) * D)).to(torch.bfloat16).to(DEV)


@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("N", LENGTHS)
@pytest.mark.parametrize("H,G,D", HGD, ids=lambda v: str(v))
def test_one_launch_equals_the_launch_per_group_bit_for_bit(H, G, D, N, out_dtype):
    qkv = _qkv(H, G, D, N)
    o_ref, lse_ref = ops.mqa_fwd(qkv, B, N, H, D, out_dtype, D ** -0.5, kv_heads=G)
    o, lse = ops.gqa_fwd(qkv, B, N, H, D, out_dtype, D ** -0.5, kv_heads=G)
    assert o.dtype == out_dtype and o.shape == o_ref.shape and lse.shape == lse_ref.shape
    assert lse.shape == ((B, H, N) if G == 1 else (G, B, H // G, N))
    assert torch.isfinite(o.float()).all() and torch.isfinite(lse).all()
    assert torch.equal(o, o_ref)
    assert torch.equal(lse, lse_ref)


@pytest.mark.parametrize("H,G,D", [(6, 2, 16), (4, 4, 32), (6, 3, 64), (4, 2, 128)], ids=lambda v: str(v))
def test_vs_fp64_softmax(H, G, D):
    """Independent of the per-group loop: fp64 softmax(q k^T scale) v on the bf16-rounded inputs, query head j of the group-major layout
    reading K/V head j // r."""
    N, r = 100, H // G
    qkv = _qkv(H, G, D, N)
    o, lse = ops.gqa_fwd(qkv, B, N, H, D, torch.float32, D ** -0.5, kv_heads=G)
    x = qkv.double().cpu()
    q = x[..., :H * D].view(B, N, H, D).permute(0, 2, 1, 3)
    k = x[..., H * D:(H + G) * D].view(B, N, G, D).permute(0, 2, 1, 3).repeat_interleave(r, dim=1)
    v = x[..., (H + G) * D:].view(B, N, G, D).permute(0, 2, 1, 3).repeat_interleave(r, dim=1)
    s = (q @ k.transpose(-1, -2)) * D ** -0.5
    ref = (s.softmax(-1) @ v).permute(0, 2, 1, 3).reshape(B, N, H * D)
    ref_lse2 = (torch.logsumexp(s, -1) / np.log(2.0)).view(B, G, r, N).permute(1, 0, 2, 3)
    e_max, e_l2, e_lse = relmax(o, ref), rell2(o, ref), (lse.double().cpu() - ref_lse2).abs().max().item()
    print(f"gqa_fwd vs fp64 H{H} G{G} D{D}: relmax={e_max:.3e} rel_l2={e_l2:.3e} lse={e_lse:.3e}")
    assert e_max < O_RELMAX and e_l2 < O_RELL2 and e_lse < LSE_ABS


def test_argument_checks_return_error_codes_without_launching():
    """Valid device buffers, invalid arguments: the library's codes (-1 invalid argument, -2 unsupported), and the outputs stay untouched."""
    H, G, D, N = 4, 2, 64, 40
    W = (H + 2 * G) * D
    qkv = _qkv(H, G, D, N)
    o = torch.full((B, N, H * D), -7.0, dtype=torch.bfloat16, device=DEV)
    lse = torch.full((G, B, H // G, N), -7.0, dtype=torch.float32, device=DEV)
    lib = _lib.load()
    base = qkv.data_ptr()

    def call(q=base, H_=H, G_=G, D_=D):
        return lib.osuf_gqa_fwd(q, W, base + 2 * H * D, W, base + 2 * (H + G) * D, W, o.data_ptr(), H * D, ops.BF16, lse.data_ptr(), B, H_, G_, N, D_,
                                D ** -0.5, torch.cuda.current_stream().cuda_stream)
    assert call(G_=3) == -1                                # H % G
    assert call(G_=0) == -1
    assert call(q=base + 2) == -1                          # a misaligned pointer
    assert call(q=base + 2, G_=1) == -1
    assert call(D_=48) == -2
    torch.cuda.synchronize()
    assert (o == -7.0).all() and (lse == -7.0).all()
    assert call() == 0
    torch.cuda.synchronize()
    ref = ops.mqa_fwd(qkv, B, N, H, D, torch.bfloat16, D ** -0.5, kv_heads=G)
    assert torch.equal(o, ref[0]) and torch.equal(lse, ref[1])


def _guarded(H, G, D, N, out_dtype):
    def run(c):
        qkv = c.inp(rnd("qkv", (B, N, (H + 2 * G) * D)), torch.bfloat16)
        o, lse = ops.gqa_fwd(qkv, B, N, H, D, out_dtype, D ** -0.5, kv_heads=G)
        c.eq("o", o), c.eq("lse", lse)
    return run


@pytest.mark.parametrize("H,G,D,N,out_dtype", [(6, 3, 64, 100, torch.bfloat16), (6, 2, 16, 100, torch.float32)], ids=["tuned", "generic"])
def test_on_poisoned_canary_guarded_memory(H, G, D, N, out_dtype):
    """Inside tests/memguard.py's allocations: no write outside o / lse (canaries), nothing unwritten read (finite under every poison pattern, the
    same bits under all of them)."""
    run_case(_guarded(H, G, D, N, out_dtype))
