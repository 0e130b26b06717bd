"""Poisoned, canary-guarded allocations for the kernel tests (a plain helper module, imported by the tests that use it).

    with guard(0xFF) as g:          # every CUDA torch.empty / torch.empty_like in the block
        y = ops.gn_apply(...)       #   - floating dtypes: every byte = 0xFF (NaN in f64 / f32 / bf16); 0x7F: ~3.4e38 (f32, bf16), finite
        g.check()                   #   - integer / bool dtypes: zeros (an index read before it is written points at row 0)
                                    #   - max(4 KiB, n / 4) bytes of slack behind the tensor, filled like it; check() names the
                                    #     allocating line of every tensor whose slack a kernel wrote

Both poison bytes are needed: fmaxf drops a NaN operand, so a NaN read into a running maximum (softmax row max, pooling) vanishes where
a huge finite value does not.  On entry the module caches that hold device buffers are invalidated so that they are re-allocated
poisoned: the shared split-wgrad workspace (ops._WS), every PackCache entry (functional._WEIGHT_EPOCH) and the shared concatenations of
the runtime.  CPU (unless device="cpu"), pinned and out= allocations pass through untouched.
"""
from __future__ import annotations

import sys
from typing import List, Optional, Tuple

import torch

_orig_empty = torch.empty
_orig_empty_like = torch.empty_like

SLACK_MIN_BYTES = 4096


class CanaryError(AssertionError):
    pass


class guard:
    """Context manager; `byte` = 0x00 (zero fill: the clean run), 0xFF or 0x7F.  canaries=False: poison only, nothing is retained
    (full-size runs)."""

    def __init__(self, byte: int = 0xFF, device: str = "cuda", canaries: bool = True) -> None:
        assert 0 <= byte <= 0xFF
        self.byte = byte
        self.device = torch.device(device).type
        self.canaries = canaries
        self.records: List[Tuple[torch.Tensor, int, int, str]] = []     # (flat uint8 view of the buffer, tensor bytes, tail byte, site)
        self.allocations = 0
        self._saved = None

    # -- allocation -----------------------------------------------------------------------------------------------
    def _guarded(self, meta: torch.Tensor, dev: torch.device, requires_grad: bool) -> torch.Tensor:
        n, es = meta.numel(), meta.element_size()
        slack = max(-(-SLACK_MIN_BYTES // es), n // 4)
        buf = _orig_empty(n + slack, dtype=meta.dtype, device=dev)
        poison = meta.dtype.is_floating_point or meta.dtype.is_complex
        fill = self.byte if poison else 0
        buf.view(torch.uint8).fill_(fill)
        t = buf.as_strided(meta.shape, meta.stride(), 0)
        self.allocations += 1
        if self.canaries:
            f = sys._getframe(2)
            site = f"{f.f_code.co_name} ({f.f_code.co_filename.rsplit('/', 1)[-1]}:{f.f_lineno})"
            self.records.append((buf.view(torch.uint8), n * es, fill, site))
        if requires_grad:
            t.requires_grad_(True)
        return t

    def _wants(self, dev: torch.device) -> bool:
        return dev.type == self.device

    def _empty(self, *size, out=None, device=None, pin_memory=False, requires_grad=False, **kw):
        dev = torch.device(device) if device is not None else torch.get_default_device()
        if out is not None or pin_memory or not self._wants(dev) or kw.get("layout", torch.strided) != torch.strided:
            return _orig_empty(*size, out=out, device=device, pin_memory=pin_memory, requires_grad=requires_grad, **kw)
        meta = _orig_empty(*size, device="meta", **kw)
        return self._guarded(meta, dev, requires_grad)

    def _empty_like(self, x, *, device=None, pin_memory=False, requires_grad=False, **kw):
        dev = torch.device(device) if device is not None else x.device
        if pin_memory or not self._wants(dev) or x.layout != torch.strided or kw.get("layout", torch.strided) != torch.strided:
            return _orig_empty_like(x, device=device, pin_memory=pin_memory, requires_grad=requires_grad, **kw)
        meta = _orig_empty_like(x, device="meta", **kw)            # torch's own stride rule (preserve_format: dense inputs keep theirs)
        return self._guarded(meta, dev, requires_grad)

    def place(self, t: torch.Tensor) -> torch.Tensor:
        """A test input copied to the front of a guarded allocation: a kernel reading past its end meets poison."""
        dst = self._empty(t.shape, dtype=t.dtype, device=t.device if t.device.type == self.device else self.device)
        return dst.copy_(t)

    # -- checks -----------------------------------------------------------------------------------------------------
    def check(self) -> None:
        """Sync, then assert that every retained tensor's slack still holds its fill byte; names the allocating line of each one that does not."""
        if self.device == "cuda":
            torch.cuda.synchronize()
        bad = []
        for i in range(0, len(self.records), 256):
            chunk = self.records[i:i + 256]
            flags = torch.stack([(u[nb:] != fill).any() for u, nb, fill, _ in chunk]).cpu()
            bad += [(site, u.numel() - nb, int((u[nb:] != fill).nonzero()[0].item())) for (u, nb, fill, site), f in zip(chunk, flags.tolist()) if f]
        if bad:
            raise CanaryError("written past the end of an allocation: " +
                              "; ".join(f"{site} (first overwritten slack byte {off} of {slack})" for site, slack, off in bad[:8]) +
                              (f" ... and {len(bad) - 8} more" if len(bad) > 8 else ""))

    def release(self) -> None:
        self.records.clear()

    # -- the patch ----------------------------------------------------------------------------------------------------
    def __enter__(self) -> "guard":
        assert self._saved is None, "guard is not re-entrant"
        saved = {"empty": torch.empty, "empty_like": torch.empty_like}
        caches = _device_caches()
        if caches is not None:
            ops, Fn, rt = caches
            saved["ws"] = dict(ops._WS)
            ops._WS.clear()
            Fn.bump_weight_epoch()                                   # every PackCache entry fails its version check and is rebuilt
            rt.clear_shared_cat()
        self._saved = saved
        torch.empty = self._empty
        torch.empty_like = self._empty_like
        return self

    def __exit__(self, *exc) -> bool:
        saved, self._saved = self._saved, None
        torch.empty, torch.empty_like = saved["empty"], saved["empty_like"]
        if "ws" in saved:
            ops, Fn, rt = _device_caches()
            ops._WS.clear()
            ops._WS.update(saved["ws"])
            rt.clear_shared_cat()                                    # (the weight epoch only ever grows: see functional.PackCache)
        return False


def _device_caches() -> Optional[tuple]:
    """(ops, functional, runtime) when the package is importable (it needs its built library), else None (the CPU self-test)."""
    try:
        from osufusion_amd import functional as Fn
        from osufusion_amd import ops
        from osufusion_amd import runtime as rt
    except Exception:                                                # noqa: BLE001 -- no library on a CPU-only checkout is fine here
        return None
    return ops, Fn, rt
