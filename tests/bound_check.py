"""Check: the bound rule shared by the kernel-against-fp64 sweeps (tests/test_norm_rows_gpu.py, tests/test_gemm_rows_gpu.py).

Bounds are not taken from the kernels: for an output of fp32 arithmetic the same reference is also evaluated in fp32 torch on the CPU,
e32 is its distance to the fp64 result in the same metric and the bound is 16 * e32 (a different summation order, atomics), at least
FLOOR and never above the cap the caller names (what the suite already asks of the quantity).  A bf16-stored output must lie within one
bf16 spacing of the reference plus that fp32 term: |got - ref| <= 2^-7 |ref| + bound * max|ref|.  Every achieved figure goes to the
suite's parity metrics file (report()).
"""
import torch

from tests.test_hip_parity import report
from tests.test_poisoned_memory import relmax

F32 = torch.float32
FLOOR = 1e-6


def tag(dtype):
    return dtype if isinstance(dtype, str) else ("f32" if dtype == F32 else "bf16")


def bound(ref32, ref64, metric, cap, extra=0.0):
    return min(max(16 * metric(ref32, ref64), FLOOR) + extra, cap)


class Check:
    """Collects (quantity, achieved error, bound) of one case; done() reports all of them, then asserts."""

    prefix = "rows"

    def __init__(self, kernel, dtype, **where):
        self.kernel, self.dtype, self.where, self.rows = kernel, dtype, where, []

    def bound(self, ref32, ref64, metric, cap, extra=0.0):
        return bound(ref32, ref64, metric, cap, extra)

    def f32(self, key, got, ref64, ref32, metric, cap, extra=0.0):
        """An output of fp32 arithmetic (in either storage mode)."""
        assert got.dtype == F32, (key, got.dtype)
        self.rows.append((key, metric(got.cpu(), ref64), self.bound(ref32, ref64, metric, cap, extra)))

    def out(self, key, got, ref64, ref32, cap, extra=0.0):
        """An elementwise output in the storage dtype."""
        if got.dtype == F32:
            return self.f32(key, got, ref64, ref32, relmax, cap, extra)
        assert got.dtype == torch.bfloat16, (key, got.dtype)
        b = self.bound(ref32, ref64, relmax, cap, extra)
        allow = 2.0 ** -7 * ref64.abs() + b * ref64.abs().max()
        self.rows.append((key + "_bf16", ((got.cpu().double() - ref64).abs() / allow).max().item(), 1.0))

    def fixed(self, key, err, limit):
        """A figure with a limit that the suite states as a number (no fp32 evaluation behind it)."""
        self.rows.append((key, float(err), float(limit)))

    def done(self):
        report(f"{self.prefix}::{self.kernel}", dtype=tag(self.dtype), **self.where,
               **{k: e for k, e, _ in self.rows}, **{k + "_bound": b for k, _, b in self.rows})
        print(self.kernel, tag(self.dtype), self.where, [(k, f"{e:.3g}", f"{b:.3g}") for k, e, b in self.rows])
        bad = [(k, e, b) for k, e, b in self.rows if not e <= b]
        assert not bad, bad
