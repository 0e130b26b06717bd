"""Time the resampling front end on a song-length signal and write profiles/resample.md.
usage: python tools/bench_resample.py [seconds_of_audio] [--out profiles/resample.md]

For 44 100 and 48 000 Hz input: osuf_resample alone (device events around repeated launches on a resident signal), host
scipy.signal.resample_poly (what read_wave's default call runs), and load_audio end to end from a float32 .wav on disk by the old path
(read_wave -> resample_poly -> log_vqt) and by the new one (read_wave(resample=False) -> resample -> log_vqt), host clock around work
that ends in a device synchronise, medians of alternating repeats.  Needs a GPU: there is no fallback."""
import math
import struct
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, ".")
from osufusion_amd import audio as A  # noqa: E402
from osufusion_amd import ops  # noqa: E402


def _write_f32_wav(path, x, rate):
    fmt = struct.pack("<HHIIHH", 3, 1, rate, rate * 4, 4, 32)
    body = x.astype("<f4").tobytes()
    chunks = b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", len(body)) + body
    path.write_bytes(b"RIFF" + struct.pack("<I", 4 + len(chunks)) + b"WAVE" + chunks)


def _median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    secs = float(args[0]) if args else 240.0
    out_path = Path(sys.argv[sys.argv.index("--out") + 1]) if "--out" in sys.argv else Path("profiles/resample.md")
    if not torch.cuda.is_available():
        raise SystemExit("bench_resample needs a GPU (no CPU fallback); profiles/resample.md is left as it is")
    from scipy.signal import resample_poly
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for rate in (44100, 48000):
            n = int(secs * rate)
            x = (np.random.default_rng(0).standard_normal(n) * 0.1).astype(np.float32)
            wav = Path(tmp) / f"song_{rate}.wav"
            _write_f32_wav(wav, x, rate)
            plan = A.resample_plan(rate, A.SR)
            n_out = A.resample_length(n, rate, A.SR)
            # ---- the kernel alone
            table = torch.from_numpy(plan.table).cuda()
            x_pad = torch.zeros(max(plan.t_left - 1 + n, ((n_out - 1) * plan.M) // plan.L + plan.T), dtype=torch.float32, device="cuda")
            x_pad[plan.t_left - 1:plan.t_left - 1 + n] = torch.from_numpy(x).cuda()
            y = torch.zeros(n_out, dtype=torch.float32, device="cuda")
            for _ in range(3):
                ops.resample(x_pad, table, plan.L, plan.M, 0, y)
            torch.cuda.synchronize()
            reps = 50
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            for _ in range(reps):
                ops.resample(x_pad, table, plan.L, plan.M, 0, y)
            ev[1].record()
            torch.cuda.synchronize()
            k_ms = ev[0].elapsed_time(ev[1]) / reps
            gfma = n_out * plan.T / 1e9
            # ---- host polyphase resampler
            g = math.gcd(A.SR, rate)
            host = []
            for _ in range(3):
                t0 = time.perf_counter()
                resample_poly(x.astype(np.float64), A.SR // g, rate // g).astype(np.float32)
                host.append((time.perf_counter() - t0) * 1e3)
            # ---- load_audio end to end, old and new path alternating
            old_fn = lambda: A.log_vqt(A.read_wave(wav))              # noqa: E731
            new_fn = lambda: A.load_audio(wav)                        # noqa: E731
            for fn in (old_fn, new_fn):
                fn()
            torch.cuda.synchronize()
            old, new = [], []
            for _ in range(5):
                old.append(_median_ms(old_fn, 1)[0])
                new.append(_median_ms(new_fn, 1)[0])
            rows.append((rate, n, n_out, plan.L, plan.T, k_ms, gfma, float(np.median(host)), min(host), max(host),
                         float(np.median(old)), min(old), max(old), float(np.median(new)), min(new), max(new)))
    lines = ["# Resampling front end: measured times", "",
             f"`python tools/bench_resample.py {secs:g}` on {torch.cuda.get_device_name(0)}; {secs:g} s of Gaussian noise per case, float32 .wav on a",
             "temporary directory.  Kernel: device events around 50 launches on a resident signal (3 warm-up launches).  Host and end-to-end:",
             "host clock, the end-to-end ones around work that ends in a device synchronise, old and new path alternating; median (min .. max).",
             "The end-to-end times include reading and decoding the file and the upload; the log-VQT is the same work in both.", "",
             "| input rate | samples in -> out | L | T | osuf_resample | GFMA/s | host resample_poly | load_audio, host resampler | load_audio, osuf_resample |",
             "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r[0]} Hz | {r[1]} -> {r[2]} | {r[3]} | {r[4]} | {r[5]:.3f} ms | {r[6] / (r[5] * 1e-3):.0f} | {r[7]:.0f} ms ({r[8]:.0f} .. {r[9]:.0f}) | "
                     f"{r[10]:.0f} ms ({r[11]:.0f} .. {r[12]:.0f}) | {r[13]:.0f} ms ({r[14]:.0f} .. {r[15]:.0f}) |")
    lines += ["", "GFMA/s = n_out * T multiply-adds over the kernel time (the table's zero padding included): a rate, not a share of peak.", ""]
    text = "\n".join(lines)
    print(text)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(text)


if __name__ == "__main__":
    main()
