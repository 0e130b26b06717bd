"""Sampled signals -> ``.osu`` texts, a batch at a time: the object tables (onsets, run ends, new combos, cursor pixels) and the tempo
scan on the GPU (osuf_decode_objects / osuf_tempo_scan, csrc/decode.hip), the rest -- autocorrelation, slider fits, snapping, text --
through the same host functions that ``decode.decode_beatmap`` runs, so that ``decode_beatmaps(...)[b]`` is ``decode_beatmap`` of sample b
as a string (tests/test_decode_gpu.py).  The allocating wrappers live here, as encode.py's do; ``ops.decode_objects`` and
``ops.tempo_scan`` are these.

One deliberate difference: a sample with no onset but a combo flip makes the host index an empty list (IndexError); here it gives the
empty map the host returns when that COMBO row holds no flip.  And one condition: frame_times is taken as fp64 (the host path computes
in whatever dtype it is handed).
"""
from __future__ import annotations

import time
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import decode, ops
from .decode import HostTable, Metadata, TimingPoint

MAX_LENGTH = 65536                                                   # osuf_decode_objects' limit: FullSequenceDataset.MAX_LENGTH frames
SCAN_POINTS = 1000                                                   # candidates of decode.tempo_candidates
BINS = 100


@dataclass
class ObjectTable:
    """The objects of B samples on the device: count int32 (B,), the true number of onsets; frame, sustain_end, slider_end, new_combo
    int32 (B, cap) and px, py fp64 (B, cap), of which row b holds count[b] entries in ascending frame order (the rest is unwritten)."""
    count: torch.Tensor
    frame: torch.Tensor
    sustain_end: torch.Tensor
    slider_end: torch.Tensor
    new_combo: torch.Tensor
    px: torch.Tensor
    py: torch.Tensor

    @property
    def cap(self) -> int:
        return int(self.frame.shape[1])

    def host(self) -> List[HostTable]:
        """One device-to-host copy per field, cut to the longest row; raises if a sample overflowed the capacity."""
        count = self.count.cpu().numpy()
        if len(count) and int(count.max()) > self.cap:
            raise ValueError(f"sample {int(count.argmax())} has {int(count.max())} objects, the table holds {self.cap} per sample")
        m = int(count.max()) if len(count) else 0
        fr, se, le, nc = (t[:, :m].cpu().numpy() for t in (self.frame, self.sustain_end, self.slider_end, self.new_combo))
        px, py = (t[:, :m].cpu().numpy() for t in (self.px, self.py))        # (cast per row: what lies behind a row's end is unwritten)
        return [HostTable(fr[b, :n].tolist(), se[b, :n].tolist(), le[b, :n].tolist(), [bool(v) for v in nc[b, :n]],
                          px[b, :n].astype(int), py[b, :n].astype(int)) for b, n in enumerate(count.tolist())]


def decode_objects(x: torch.Tensor, lengths: Optional[torch.Tensor] = None, cap: Optional[int] = None) -> ObjectTable:
    """x fp32 (B, 6, L) on the device, lengths int32 (B,) on the device or None -> ObjectTable.  One launch, no host sync; cap (default L,
    which always suffices) is the number of rows kept per sample: `ObjectTable.host` raises when a sample has more."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and x.shape[1] == decode.TOTAL_DIM):
        raise ValueError(f"x must be an fp32 (B, 6, L) tensor on the device (got {tuple(x.shape)} {x.dtype} on {x.device})")
    B, _, L = x.shape
    cap = L if cap is None else int(cap)
    if B < 1 or L < 2 or L > MAX_LENGTH or cap < 1:
        raise ValueError(f"B = {B}, L = {L}, cap = {cap}: need B >= 1, 2 <= L <= {MAX_LENGTH}, cap >= 1")
    if lengths is not None and not (lengths.is_cuda and lengths.dtype == torch.int32 and lengths.shape == (B,) and lengths.is_contiguous()):
        raise ValueError("lengths must be a contiguous int32 (B,) tensor on the device")
    x = x.contiguous()
    count = torch.empty(B, dtype=torch.int32, device=x.device)
    ints = [torch.empty((B, cap), dtype=torch.int32, device=x.device) for _ in range(4)]
    px, py = (torch.empty((B, cap), dtype=torch.float64, device=x.device) for _ in range(2))
    ops.call("osuf_decode_objects", x.data_ptr(), None if lengths is None else lengths.data_ptr(), B, L, cap, count.data_ptr(),
          *(t.data_ptr() for t in ints), px.data_ptr(), py.data_ptr(), ops._stream())
    return ObjectTable(count, *ints, px, py)


def tempo_scan(table: ObjectTable, frame_times: torch.Tensor, beat_len: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """frame_times fp64 (L,) ms and beat_len fp64 (B, C) on the device -> (best_count, best_bin) int32 (B, C): the largest count of the
    100-bin histogram of the onset times modulo beat_len[b, c] and its first fullest bin.  One launch, no host sync."""
    B = int(table.count.shape[0])
    for t, what in ((frame_times, "frame_times"), (beat_len, "beat_len")):
        if not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()):
            raise ValueError(f"{what} must be a contiguous fp64 tensor on the device")
    if frame_times.dim() != 1 or beat_len.dim() != 2 or beat_len.shape[0] != B or beat_len.shape[1] < 1 or frame_times.numel() < 1:
        raise ValueError(f"frame_times (L,) and beat_len ({B}, C) expected, got {tuple(frame_times.shape)} and {tuple(beat_len.shape)}")
    C = int(beat_len.shape[1])
    best_count = torch.empty((B, C), dtype=torch.int32, device=beat_len.device)
    best_bin = torch.empty((B, C), dtype=torch.int32, device=beat_len.device)
    ops.call("osuf_tempo_scan", table.frame.data_ptr(), table.count.data_ptr(), table.cap, frame_times.data_ptr(), frame_times.numel(),
          beat_len.data_ptr(), B, C, best_count.data_ptr(), best_bin.data_ptr(), ops._stream())
    return best_count, best_bin


def _bin_edge(beat_length: float, k: int) -> float:
    """The left edge of bin k as np.histogram returns it (get_timings' offset)."""
    return float(np.linspace(0, beat_length, BINS + 1)[k])


def decode_beatmaps(metadatas: Sequence[Metadata], x: torch.Tensor, frame_times, bpm: Optional[float] = None, allow_beat_snap: bool = True,
                    lengths=None, verbose: bool = False, timings: Optional[dict] = None) -> List[str]:
    """x fp32 (B, 6, L) on the device, frame_times (L,) ms, lengths (None, a host sequence or an int32 device tensor): only the first
    lengths[b] frames of sample b are decoded -> B ``.osu`` texts, text b = decode.decode_beatmap(metadatas[b], x[b, :, :lengths[b]],
    frame_times[:lengths[b]], bpm, allow_beat_snap).  Two launches for the batch (tables; tempo scan, unless snapping is off), the
    tables, the scan results and the two cursor rows copied back once each.  timings: a dict that receives the seconds spent in
    "table", "scan" (launch to results on the host), "fits" (slider_decoder) and "host" (everything else)."""
    B, _, L = x.shape
    if len(metadatas) != B:
        raise ValueError(f"{len(metadatas)} metadatas for a batch of {B}")
    ft = np.ascontiguousarray(np.asarray(frame_times.cpu() if isinstance(frame_times, torch.Tensor) else frame_times, dtype=np.float64))
    if ft.shape != (L,):
        raise ValueError(f"frame_times must have {L} entries (got {ft.shape})")
    if lengths is not None and not (isinstance(lengths, torch.Tensor) and lengths.is_cuda):
        lengths = torch.as_tensor(np.asarray(lengths.cpu() if isinstance(lengths, torch.Tensor) else lengths)).to(torch.int32).to(x.device)
    clock = {"table": 0.0, "scan": 0.0, "fits": 0.0, "host": 0.0}
    t_all = t0 = time.perf_counter()
    table = decode_objects(x, lengths)
    tables = table.host()
    clock["table"] = time.perf_counter() - t0
    n_frames = [L] * B if lengths is None else [int(v) for v in lengths.cpu().tolist()]
    cursor_f32 = x[:, decode.CURSOR_X:decode.CURSOR_Y + 1, :].cpu().numpy()

    # the timing of every sample: the candidates on the host, one scan launch, the first fullest candidate
    timing: List[Optional[Tuple[bool, TimingPoint]]] = [None] * B
    beat_len = np.full((B, 1 if bpm is not None else SCAN_POINTS), 60000 / 200, dtype=np.float64)
    for b, tab in enumerate(tables):
        if bpm is not None:
            beat_len[b, 0] = 60000 / bpm
            continue
        scan = decode.tempo_candidates(ft[tab.frame], verbose) if allow_beat_snap else None
        if scan is None:
            timing[b] = decode.TIMING_FALLBACK
        else:
            beat_len[b] = 60000.0 / scan
    if any(t is None for t in timing):
        t0 = time.perf_counter()
        best_count, best_bin = tempo_scan(table, torch.from_numpy(ft).to(x.device), torch.from_numpy(beat_len).to(x.device))
        best_count, best_bin = best_count.cpu().numpy(), best_bin.cpu().numpy()
        clock["scan"] = time.perf_counter() - t0
        for b in range(B):
            if timing[b] is None:
                c = int(np.argmax(best_count[b]))
                bl = beat_len[b, c] if bpm is None else 60000 / bpm      # (the types decode_beatmap hands to its f-strings)
                timing[b] = (True, TimingPoint(_bin_edge(bl, int(best_bin[b, c])), bl, 4))

    out = []
    fits = [0.0]
    inner = decode.slider_decoder

    def timed_fit(*args):
        t1 = time.perf_counter()
        try:
            return inner(*args)
        finally:
            fits[0] += time.perf_counter() - t1

    for b, tab in enumerate(tables):
        n = n_frames[b]
        if not 2 <= n <= L:
            n = 0                                                        # (the kernel reports no objects for such a sample)
        cursor = (cursor_f32[b, :, :n].astype(np.float64) + 1.0) / 2.0 * np.array([[decode.PLAYFIELD[0]], [decode.PLAYFIELD[1]]])
        snap, tp = timing[b]
        out.append(decode.table_to_text(metadatas[b], tab, cursor, ft[:n], snap, tp, verbose, slider_fit=timed_fit))
    clock["fits"] = fits[0]
    clock["host"] = time.perf_counter() - t_all - clock["table"] - clock["scan"] - clock["fits"]
    if timings is not None:
        timings.update(clock)
    return out
