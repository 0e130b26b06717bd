#!/usr/bin/env python3
"""Timing of osuf_encode_signals (not a gate): one launch of B = 32 random crops of L = 4096 frames from a table of synthetic maps of
about 1 000 objects each, against (a) the fp64 host loop of tests/encode_oracle.py on the same crops (timed on --oracle-rows rows and
scaled to B) and (b) the H2D copy of the same batch of precomputed x from pinned memory.  Optionally folds in the figure that
tests/test_encode_gpu.py prints for round_pos = 0 (--deviation).  Writes profiles/encode.md.

    python tools/bench_encode.py [--maps 16] [--iters 200] [--oracle-rows 2] [--deviation 2.8e-14]
"""
from __future__ import annotations

import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

HEAD = ("[General]\nAudioFilename: a.wav\nMode: 0\n\n[Metadata]\nTitle:synthetic\nArtist:bench\nCreator:bench\nVersion:{v}\n\n[Difficulty]\n"
        "HPDrainRate:5\nCircleSize:4\nOverallDifficulty:8\nApproachRate:9\nSliderMultiplier:1.6\nSliderTickRate:1\n\n[Events]\n\n"
        "[TimingPoints]\n0,350,4,2,0,60,1,0\n\n[HitObjects]\n")


def synthetic_map(seed: int, n_objects: int = 1000) -> str:
    """About n_objects objects over ~3 minutes: circles, three-point arcs, four-point Beziers, straight sliders and the odd spinner."""
    rng = np.random.default_rng(seed)
    t, lines = 1000, []
    for _ in range(n_objects):
        x, y = int(rng.integers(40, 470)), int(rng.integers(40, 340))
        kind = rng.choice(5, p=[0.55, 0.15, 0.15, 0.13, 0.02])
        combo = 4 if rng.random() < 0.2 else 0
        if kind == 0:
            lines.append(f"{x},{y},{t},{1 + combo},0,0:0:0:0:")
            t += int(rng.integers(90, 260))
            continue
        if kind == 4:
            lines.append(f"256,192,{t},{8 + combo},0,{t + 700}")
            t += 900
            continue
        pts = [(x + int(rng.integers(-60, 61)), y + int(rng.integers(-60, 61))) for _ in range({1: 1, 2: 2, 3: 3}[int(kind)])]
        pts = [(px + (px == x), py) for px, py in pts]                 # never on top of the head
        length = int(rng.integers(40, 120))
        slides = int(rng.integers(1, 3))
        curve = "|".join(f"{px}:{py}" for px, py in pts)
        lines.append(f"{x},{y},{t},{2 + combo},0,B|{curve},{slides},{length}")
        t += int(length / 160 * 350 * slides) + int(rng.integers(120, 260))
    return HEAD.format(v=seed) + "\n".join(lines) + "\n"


def events_ms(fn, iters: int, rounds: int = 7) -> float:
    """Median over `rounds` of the mean device time of `iters` back-to-back calls."""
    out = []
    for _ in range(rounds):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            fn()
        e.record()
        torch.cuda.synchronize()
        out.append(s.elapsed_time(e) / iters)
    return statistics.median(out)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--maps", type=int, default=16)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--oracle-rows", type=int, default=2)
    ap.add_argument("--deviation", type=float, default=None, help="largest round_pos = 0 deviation in px, as tests/test_encode_gpu.py printed it")
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "encode.md")
    args = ap.parse_args(argv)

    from osufusion_amd import encode
    from osufusion_amd.beatmap import Beatmap
    from tests import encode_oracle as EO

    B, L = 32, 4096
    maps = [Beatmap.from_text(synthetic_map(s)) for s in range(args.maps)]
    n_obj = [len(m.hit_objects) for m in maps]
    frames = [int(max(o.end_time() for o in m.hit_objects) * 22050 / 176 / 1000) for m in maps]
    t0 = time.perf_counter()
    table = encode.BeatmapTable(maps, "cuda")
    torch.cuda.synchronize()
    t_table = (time.perf_counter() - t0) * 1e3
    rng = np.random.default_rng(0)
    idx = rng.integers(0, args.maps, B)
    start = np.array([rng.integers(0, max(1, frames[m] - L)) for m in idx])
    flip = rng.integers(0, 4, B)
    d_idx, d_start, d_len, d_flip = (torch.tensor(v, device="cuda", dtype=d) for v, d in
                                     ((idx, torch.int32), (start, torch.int64), (np.full(B, L), torch.int32), (flip, torch.int32)))
    launch = lambda: table.encode(d_idx, d_start, d_len, d_flip, L=L)
    for _ in range(10):
        x, _ = launch()
    torch.cuda.synchronize()
    t_kernel = events_ms(launch, args.iters)

    pinned = x.cpu().pin_memory()
    dst = torch.empty_like(x)
    copy = lambda: dst.copy_(pinned, non_blocking=True)
    for _ in range(10):
        copy()
    torch.cuda.synchronize()
    t_copy = events_ms(copy, args.iters)

    t0 = time.perf_counter()
    got = x.cpu().numpy()
    worst = 0
    for b in range(args.oracle_rows):
        want = EO.encode_beatmap(maps[idx[b]], EO.frame_times(L, int(start[b])))
        if flip[b] & 1:
            want[4] = -want[4]
        if flip[b] & 2:
            want[5] = -want[5]
        assert np.array_equal(got[b, :4], want[:4].astype(np.float32)), "the timed launch disagrees with the oracle"
        worst = max(worst, float(np.abs(got[b, 4:] - want[4:]).max()))
    t_oracle = (time.perf_counter() - t0) * 1e3 / max(1, args.oracle_rows) * B
    assert worst < 1e-6

    dev = torch.cuda.get_device_name(0)
    lines = [
        "# Beatmap encoding (osuf_encode_signals, osufusion_amd/encode.py)",
        "",
        f"Measured by `tools/bench_encode.py` on {dev}.  Not a gate.  One launch, B = {B} crops of L = {L} frames with flips, from a table of",
        f"{args.maps} synthetic maps ({min(n_obj)}-{max(n_obj)} objects each, {sum(table.host[k].nbytes for k in table.host) / 1024:.0f} KiB of tables).",
        f"Device times: median of 7 rounds of the mean over {args.iters} back-to-back calls between two events, so each includes the",
        "wrapper's host work per call (the kernel is short enough that the launch path is what is timed).",
        "",
        "| what | time |",
        "|---|---|",
        f"| `BeatmapTable` pack + upload ({args.maps} maps, parse excluded; the first device work of the process) | {t_table:.1f} ms |",
        f"| `table.encode`, one launch ({B} x 6 x {L}) | {t_kernel * 1e3:.1f} us |",
        f"| H2D copy of the same batch of precomputed x ({x.numel() * 4 / 2**20:.1f} MiB, pinned) | {t_copy * 1e3:.1f} us |",
        f"| fp64 host loop of tests/encode_oracle.py (timed on {args.oracle_rows} rows, scaled to {B}) | {t_oracle:.0f} ms |",
        "",
        f"The timed launch agrees with the host loop on the {args.oracle_rows} rows checked (hit channels equal, cursor within {worst:.1e}).",
        "",
        "## round_pos = 0: distance of the kernel's fp64 positions from the oracle's",
        "",
    ]
    if args.deviation is None:
        lines.append("not measured yet (tests/test_encode_gpu.py::test_unrounded_positions_are_far_inside_the_screening_margin prints it)")
    else:
        lines.append(f"Largest deviation over all fixtures of tests/golden/encode: {args.deviation:.3e} px (printed by "
                     "tests/test_encode_gpu.py::test_unrounded_positions_are_far_inside_the_screening_margin); the screening margin is 1e-6 px.")
    args.out.write_text("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
