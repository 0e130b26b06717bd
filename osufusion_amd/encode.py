"""``.osu`` beatmaps -> the six training signals on the GPU (osuf_encode_signals, csrc/encode.hip): the `prepare_map` stage of the
pipeline, and the source of `known` for ``sample(known=, known_mask=)``.  The host parses (osufusion_amd/beatmap.py) and packs every
map's hit objects into flat device tables once (`BeatmapTable`); after that a whole song, or a training batch of random crops with the
reference's cursor flips and collate_fn's -1 padding, is ONE launch with one thread per (sample, frame).  The fp64 yardstick is
tests/encode_oracle.py; the guarded-memory cases are in tests/test_encode_gpu.py.  The allocating wrapper lives here, as inpaint.py's
and windowed.py's do.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import inpaint, ops
from .beatmap import BEZIER, LINE, PERFECT, Beatmap, Bezier, Line, Perfect, Slider, Spinner

HIT, SUSTAIN, SLIDER, COMBO, CURSOR_X, CURSOR_Y = range(6)
TOTAL_DIM = 6
OBJ_F, OBJ_I, HDR = 16, 4, 8                                         # row widths of obj_f, obj_i and map_hdr (include/osufusion_hip.h)
FLIP_X, FLIP_Y = 1, 2                                                # library/augment.py: flip_cursor_horizontal / _vertical
TABLES = ("map_hdr", "obj_f", "obj_i", "ivl", "seg_cum", "seg_i", "nodes")


def merge_intervals(regions: Sequence[Tuple[float, float]]) -> np.ndarray:
    """[s, e) regions -> their union as disjoint intervals sorted by s, fp64 (k, 2); empty regions (e <= s) are dropped.  A frame lies
    in some region exactly when it lies in the one merged interval that starts last at or before it."""
    out = []
    for s, e in sorted((float(s), float(e)) for s, e in regions if e > s):
        if out and s <= out[-1][1]:
            out[-1][1] = max(out[-1][1], e)
        else:
            out.append([s, e])
    return np.array(out, dtype=np.float64).reshape(-1, 2)


def pack_tables(beatmaps: Sequence[Beatmap]) -> Dict[str, np.ndarray]:
    """The flat tables of osuf_encode_signals for N maps, on the host (layout: include/osufusion_hip.h).  No table is empty: one unused
    zero entry is appended where a map set has no intervals, segments or control points."""
    hdr = np.zeros((len(beatmaps), HDR), dtype=np.int32)
    obj_f, obj_i, ivl, seg_cum, seg_i, nodes = [], [], [], [], [], []
    n_ivl = n_nodes = 0
    for m, bm in enumerate(beatmaps):
        objs = bm.hit_objects
        assert all(a.t <= b.t for a, b in zip(objs, objs[1:])), "hit objects must be sorted by time"
        sustain = merge_intervals([(o.t, o.end_time()) for o in objs if isinstance(o, (Slider, Spinner))])
        slider = merge_intervals([(o.t, o.t + o.slide_duration) for o in objs if isinstance(o, Slider)])
        hdr[m, :6] = (len(objs), len(obj_f), len(sustain), n_ivl, len(slider), n_ivl + len(sustain))
        ivl += [sustain, slider]
        n_ivl += len(sustain) + len(slider)
        combos = 0
        for o in objs:
            combos += int(o.new_combo)
            f = np.zeros(OBJ_F)
            f[0], f[1] = o.t, o.end_time()
            f[2:4], f[4:6], f[6:8], f[8:10] = o.start_pos(True), o.end_pos(True), o.start_pos(False), o.end_pos(False)
            i = [o.kind, combos, 0, 0]
            if isinstance(o, Slider):
                f[10] = o.slide_duration
            if isinstance(o, Line):
                f[11:15] = (*o.start, *o.end)
            elif isinstance(o, Perfect):
                f[11:16] = (*o.center, o.radius, o.start, o.end)
            elif isinstance(o, Bezier):
                i[2], i[3] = len(seg_cum), len(o.segments)
                for seg, cum in zip(o.segments, o.cum_t):
                    seg_cum.append(cum)
                    seg_i.append((n_nodes, len(seg) - 1))
                    nodes.append(seg)
                    n_nodes += len(seg)
            assert i[0] in (0, 1, LINE, PERFECT, BEZIER)
            obj_f.append(f)
            obj_i.append(i)

    def table(rows, width, dtype):
        a = np.concatenate([np.asarray(r, dtype=dtype).reshape(-1, width) for r in rows] + [np.zeros((0, width), dtype)], axis=0)
        return np.ascontiguousarray(a if len(a) else np.zeros((1, width), dtype))
    return {"map_hdr": hdr, "obj_f": table(obj_f, OBJ_F, np.float64), "obj_i": table(obj_i, OBJ_I, np.int32), "ivl": table(ivl, 2, np.float64),
            "seg_cum": table(seg_cum, 1, np.float64).reshape(-1), "seg_i": table(seg_i, 2, np.int32), "nodes": table(nodes, 2, np.float64)}


def _staged(values, dtype: torch.dtype, device) -> torch.Tensor:
    """A host sequence (or array, or CPU tensor) -> device tensor through pinned staging, one asynchronous copy; a tensor already on the
    device passes through (converted there)."""
    if isinstance(values, torch.Tensor) and values.device.type != "cpu":
        return values.to(device=device, dtype=dtype).contiguous()
    host = torch.as_tensor(np.asarray(values.cpu() if isinstance(values, torch.Tensor) else values)).to(dtype).contiguous()
    if torch.device(device).type == "cuda":
        host = host.pin_memory()
    return host.to(device, non_blocking=True)


class BeatmapTable:
    """N parsed maps resident on the device: one H2D copy per table from pinned staging, then any number of `encode` launches."""

    def __init__(self, beatmaps: Sequence[Beatmap], device: Union[str, torch.device] = "cuda") -> None:
        if len(beatmaps) == 0:
            raise ValueError("a table of no beatmaps")
        self.device = torch.device(device)
        self.n_maps = len(beatmaps)
        self.host = pack_tables(beatmaps)
        self.tables = {k: _staged(v, torch.from_numpy(v).dtype, self.device) for k, v in self.host.items()}

    def encode(self, map_idx, start, length, flip=None, L: Optional[int] = None, round_pos: int = 1,
               pos_px: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (x fp32 (B, 6, L), orig_len int32 (B,) on the device): row b holds frames start[b] .. start[b] + length[b] - 1 of map
        map_idx[b] and -1.0 from length[b] on -- a collated batch and its orig_len.  flip[b]: FLIP_X | FLIP_Y bits.  map_idx, start,
        length, flip: host sequences (staged through pinned memory) or device tensors; L (default max(length)) must be given when
        `length` is a device tensor, so that nothing here waits for the device.  round_pos = 0 leaves slider positions unrounded and
        pos_px, a caller's fp64 (B, 2, L) buffer, receives the cursor in pixels: both are for measuring the kernel, not for data.
        One launch, no host sync."""
        if L is None:
            if isinstance(length, torch.Tensor) and length.device.type != "cpu":
                raise ValueError("L must be given when length is a device tensor (reading it back would force a sync)")
            L = int(max(int(v) for v in length))
        idx = _staged(map_idx, torch.int32, self.device)
        B, L = int(idx.numel()), int(L)
        if B < 1 or L < 1:
            raise ValueError(f"an empty batch: B = {B}, L = {L}")
        st, ln = _staged(start, torch.int64, self.device), _staged(length, torch.int32, self.device)
        fl = None if flip is None else _staged(flip, torch.int32, self.device)
        for name, v in (("start", st), ("length", ln), ("flip", fl)):
            if v is not None and v.numel() != B:
                raise ValueError(f"{name} has {v.numel()} entries for a batch of {B}")
        if pos_px is not None:
            assert pos_px.dtype == torch.float64 and pos_px.is_contiguous() and tuple(pos_px.shape) == (B, 2, L) and pos_px.device == idx.device
        out = torch.empty((B, TOTAL_DIM, L), dtype=torch.float32, device=self.device)
        t = self.tables
        ops.call("osuf_encode_signals", ops._p(t["map_hdr"]), self.n_maps, ops._p(t["obj_f"]), ops._p(t["obj_i"]), ops._p(t["ivl"]),
                 ops._p(t["seg_cum"]), ops._p(t["seg_i"]), ops._p(t["nodes"]), ops._p(idx), ops._p(st), ops._p(ln), ops._p(fl), int(round_pos),
                 ops._p(out), ops._p(pos_px), B, L, ops._stream())
        return out, ln


def encode_beatmap(beatmap: Beatmap, n_frames: int, device: Union[str, torch.device] = "cuda") -> torch.Tensor:
    """The reference's encode_beatmap(beatmap, frame_times) at frame_times = inpaint.frame_times_ms(n_frames) -> fp32 (6, n_frames)."""
    x, _ = BeatmapTable([beatmap], device).encode([0], [0], [int(n_frames)])
    return x[0]


def known_from_beatmap(beatmap: Beatmap, n: int, spans_ms: Sequence[Tuple[float, float]], feather_ms: float = 0.0,
                       device: Union[str, torch.device] = "cuda") -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (known fp32 (1, 6, n), mask fp32 (n,)) for sample(known=, known_mask=): the map's own signal, kept over `spans_ms`
    (inpaint.frame_mask: [start, end] in milliseconds, feathered over feather_ms)."""
    known = encode_beatmap(beatmap, n, device)[None].contiguous()
    return known, inpaint.frame_mask(n, spans_ms, feather_ms).to(device)
