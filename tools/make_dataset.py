#!/usr/bin/env python3
"""The `prepare_map` stage: a folder of beatmap sets -> the dataset files osufusion_amd.data reads.

    python tools/make_dataset.py SONGS_DIR OUT_DIR [--stars 4.5 | --stars-csv stars.csv] [--device cuda]

For every `.osu` under SONGS_DIR (one folder per set): maps whose Mode is not 0 are skipped; the audio's log-VQT `a` is computed once
per audio file (audio.load_audio); the six-channel signal `x` comes from osuf_encode_signals over as many frames as `a` has; the pair is
written as OUT_DIR/<set folder>/<map file stem>.map.npz and OUT_DIR/<set folder>/spec.npz through data.save_tensor.

The context is (CS, AR, OD, HP, star rating), normalised by data.normalize_context.  The star rating CANNOT be computed here (the
reference asks rosu-pp for it, which is not available): it is taken from --stars (one value for every map) or from --stars-csv, a
`name,stars` file whose names are the .osu file names, and clipped to [0, 20].  A map with no rating given is skipped with a message.
"""
from __future__ import annotations

import argparse
import csv
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def read_stars(path: Path) -> dict:
    with open(path, newline="", encoding="utf-8") as f:
        return {row[0].strip(): float(row[1]) for row in csv.reader(f) if len(row) >= 2 and row[0].strip() and not row[0].startswith("#")}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("songs_dir", type=Path)
    ap.add_argument("out_dir", type=Path)
    ap.add_argument("--stars", type=float, default=None, help="star rating of every map (it cannot be computed here); clipped to [0, 20]")
    ap.add_argument("--stars-csv", type=Path, default=None, help="`name,stars` rows, name = the .osu file name; clipped to [0, 20]")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    if args.stars is None and args.stars_csv is None:
        ap.error("give --stars or --stars-csv: the star rating cannot be computed here")

    from osufusion_amd import audio, data, encode
    from osufusion_amd.beatmap import Beatmap

    stars = read_stars(args.stars_csv) if args.stars_csv is not None else {}
    specs = {}
    written = skipped = 0
    for path in sorted(args.songs_dir.glob("*/*.osu")):
        try:
            bm = Beatmap.from_file(path)
        except Exception as e:  # noqa: BLE001 -- one broken map does not stop the folder, as in the reference's all_maps
            print(f"skipped {path}: {e}")
            skipped += 1
            continue
        rating = stars.get(path.name, args.stars)
        if bm.mode != 0 or rating is None:
            print(f"skipped {path}: " + (f"mode {bm.mode}" if bm.mode != 0 else "no star rating given"))
            skipped += 1
            continue
        if bm.audio_filename not in specs:
            specs[bm.audio_filename] = audio.load_audio(bm.audio_filename, args.device).cpu().numpy()
        a = specs[bm.audio_filename]
        x = encode.encode_beatmap(bm, a.shape[1], args.device).cpu().numpy()
        c = data.normalize_context(np.array([bm.cs, bm.ar, bm.od, bm.hp, min(20.0, max(0.0, float(rating)))], dtype=np.float32))
        out = args.out_dir / path.parent.name
        out.mkdir(parents=True, exist_ok=True)
        data.save_tensor(out / f"{path.stem}.map.npz", x, c, a)
        written += 1
    print(f"wrote {written} maps, skipped {skipped}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
