#!/usr/bin/env python3
"""Timing of the last stage, sample -> ``.osu`` text (not a gate): the host loop `decode.decode_beatmap` per sample against
`decode_gpu.decode_beatmaps` on the same device-resident batch, at B = 16, L = 8192 and B = 1, L = 32 768.  Inputs: the four golden
fixtures of tests/golden/encode, encoded by BeatmapTable.encode and tiled along time to L (sample b starts fixture b % 4 at another
offset), so the object densities are those of real maps, not of noise.  The texts of the two paths are asserted equal before anything is
timed.  The fixtures hold 12-19 objects each, too few for the tempo estimator to find a lag (its smallest is 190 onsets), so on them
both paths end on the fallback timing and neither runs its scan; a third set, B = 16 synthetic onset trains (pattern.onset_train, about
470 circles per sample), is there so that the scan is timed at all.  Writes profiles/decode.md.

    python tools/bench_decode.py [--rounds 5] [--out profiles/decode.md]
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

NAMES = ["basic", "circles", "edge", "sliders"]
FRAMES = {"basic": 890, "circles": 564, "edge": 627, "sliders": 2635}
SHAPES = [(16, 8192, "fixtures"), (1, 32768, "fixtures"), (16, 8192, "onset trains")]


def tiled_batch(B: int, L: int) -> torch.Tensor:
    from osufusion_amd import encode
    from osufusion_amd.beatmap import Beatmap
    maps = [Beatmap.from_file(ROOT / "tests" / "golden" / "encode" / f"{n}.osu") for n in NAMES]
    n = [FRAMES[k] for k in NAMES]
    x, _ = encode.BeatmapTable(maps, "cuda").encode([0, 1, 2, 3], [0, 0, 0, 0], n)
    rows = []
    for b in range(B):
        m = b % 4 if B > 1 else 3
        one = x[m, :, :n[m]]
        reps = -(-(L + n[m]) // n[m])
        shift = (b // 4) * 97 % n[m]
        rows.append(one.repeat(1, reps)[:, shift:shift + L])
    return torch.stack(rows).contiguous()


def events_us(fn, iters: int = 50, rounds: int = 7) -> float:
    out = []
    for _ in range(rounds):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            fn()
        e.record()
        torch.cuda.synchronize()
        out.append(s.elapsed_time(e) / iters * 1e3)
    return statistics.median(out)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "decode.md")
    args = ap.parse_args(argv)

    from osufusion_amd import decode, decode_gpu, inpaint
    from osufusion_amd.pattern import onset_train

    meta = decode.Metadata("audio.mp3", "Song", "Artist", "Version", 4.0, 9.0, 8.0, 5.0)
    dev = torch.cuda.get_device_name(0)
    lines = [
        "# Decoding samples into maps (osufusion_amd/decode.py, decode_gpu.py; csrc/decode.hip)",
        "",
        f"Measured by `tools/bench_decode.py` on {dev}, clocks as the machine's power management left them (not pinned).  Not a gate.",
        "The sample is on the device when the clock starts, as it is when a sampler returns; both paths end with the texts on the host.",
        f"Wall-clock times are medians of {args.rounds} rounds after one warm-up round of each path; kernel times are medians of 7 rounds of the",
        "mean over 50 back-to-back launches between two events (so they include the wrapper's allocations and the launch path).  The two",
        "paths' texts are equal on every sample timed.  bpm = None with beat snapping: the path with the tempo scan.",
        "",
    ]
    for B, L, kind in SHAPES:
        if kind == "fixtures":
            x = tiled_batch(B, L)
        else:
            x = torch.from_numpy(np.stack([onset_train(L, b, keep=0.5 + 0.02 * b, bpm=150.0 + 5 * b) for b in range(B)])).cuda()
        ft = inpaint.frame_times_ms(L).numpy()
        metas = [meta] * B

        def host_loop():
            xh = x.cpu().numpy()
            return [decode.decode_beatmap(meta, xh[b], ft, None, True, verbose=False) for b in range(B)]

        def batch(timings=None):
            return decode_gpu.decode_beatmaps(metas, x, ft, bpm=None, allow_beat_snap=True, timings=timings)

        want, got = host_loop(), batch()                                  # warm-up of both, and the check
        assert want == got, "the two paths disagree"
        tables = decode_gpu.decode_objects(x).host()
        objects = [len(t.frame) for t in tables]
        sliders = sum(text.count(",B|") for text in got)

        # the host loop's own split: table, scan (the 1,001 np.histogram calls), fits, the rest
        host_total, host_parts = [], []
        for _ in range(args.rounds):
            parts = {"table": 0.0, "scan": 0.0, "fits": 0.0}
            scanned = 0
            t0 = time.perf_counter()
            xh = x.cpu().numpy()
            for b in range(B):
                t1 = time.perf_counter()
                enc = np.asarray(xh[b], dtype=np.float64)
                tab = decode.object_table(enc)
                parts["table"] += time.perf_counter() - t1
                hit_times = ft[tab.frame]
                scan = decode.tempo_candidates(hit_times, False)
                t1 = time.perf_counter()
                scanned += scan is not None
                if scan is not None:
                    score = [np.histogram(hit_times % (60000.0 / s), bins=100, range=(0, 60000.0 / s))[0].max() for s in scan]
                    snap, tp = decode.get_timings(hit_times, 60000.0 / scan[int(np.argmax(score))])
                else:
                    snap, tp = decode.TIMING_FALLBACK
                parts["scan"] += time.perf_counter() - t1
                cursor = (enc[[4, 5]] + 1.0) / 2.0 * np.array([[512.0], [384.0]])
                fit = [0.0]

                def timed(*a):
                    t2 = time.perf_counter()
                    try:
                        return decode.slider_decoder(*a)
                    finally:
                        fit[0] += time.perf_counter() - t2
                text = decode.table_to_text(meta, tab, cursor, ft, snap, tp, False, slider_fit=timed)
                assert text == want[b]
                parts["fits"] += fit[0]
            host_total.append(time.perf_counter() - t0)
            host_parts.append(parts)
        plain = []
        for _ in range(args.rounds):                                      # decode_beatmap itself, untouched: the figure to compare with
            t0 = time.perf_counter()
            host_loop()
            plain.append(time.perf_counter() - t0)

        gpu_total, gpu_parts = [], []
        for _ in range(args.rounds):
            tm = {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            batch(tm)
            gpu_total.append(time.perf_counter() - t0)
            gpu_parts.append(tm)

        table = decode_gpu.decode_objects(x)
        ft_d = torch.from_numpy(ft).cuda()
        bl = torch.from_numpy(np.stack([60000.0 / np.linspace(171.0, 189.0, 1000)] * B)).cuda()
        k_table = events_us(lambda: decode_gpu.decode_objects(x))
        k_scan = events_us(lambda: decode_gpu.tempo_scan(table, ft_d, bl))

        med = statistics.median
        hp = {k: med(p[k] for p in host_parts) * 1e3 for k in ("table", "scan", "fits")}
        gp = {k: med(p[k] for p in gpu_parts) * 1e3 for k in ("table", "scan", "fits", "host")}
        h_tot, h_plain, g_tot = med(host_total) * 1e3, med(plain) * 1e3, med(gpu_total) * 1e3
        lines += [
            f"## B = {B}, L = {L}, {kind}",
            "",
            f"{sum(objects)} objects in the batch ({min(objects)}-{max(objects)} per sample), {sliders} sliders fitted; the tempo estimator found a lag, and so",
            f"the 1000-candidate scan ran, on {scanned} of {B} samples.",
            "",
            "| part | host loop (`decode_beatmap` per sample) | batch (`decode_beatmaps`) |",
            "|---|---|---|",
            f"| object tables (host: `object_table`; batch: the launch + 7 copies back + lists) | {hp['table']:.1f} ms | {gp['table']:.2f} ms |",
            f"| tempo scan (host: 1,001 `np.histogram` per sample; batch: upload, one launch of {B} x 1000 candidates, results back) | {hp['scan']:.1f} ms | {gp['scan']:.2f} ms |",
            f"| slider fits (`slider_decoder`, the same host code in both) | {hp['fits']:.1f} ms | {gp['fits']:.1f} ms |",
            f"| the rest (D2H of x or of its cursor rows, autocorrelation, snapping, text) | {h_tot - hp['table'] - hp['scan'] - hp['fits']:.1f} ms | {gp['host']:.1f} ms |",
            f"| **total** | **{h_tot:.1f} ms** (`decode_beatmap` called as it stands: {h_plain:.1f} ms) | **{g_tot:.1f} ms** |",
            "",
            f"Kernels alone: `osuf_decode_objects` {k_table:.1f} us per launch of the batch, `osuf_tempo_scan` ({B} x 1000 candidates) {k_scan:.1f} us.",
            f"Batch against host loop: {h_plain / g_tot:.2f}x.",
            "",
        ]
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
