"""tools/generate.py end to end, in-process: a 3 s sine -> log-VQT -> the smallest MMDiT the suites use (random weights) -> two samples
-> two ``.osu`` files, each the host decode_beatmap of its dumped signal."""
import importlib.util
import math
import struct
import wave
from pathlib import Path

import numpy as np
import pytest

from osufusion_amd import audio
from osufusion_amd import decode as D

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
MODEL_KW = '{"dim_h": 64, "depth": 2, "attn_heads": 4, "attn_kv_heads": 2, "attn_dim_head": 16}'     # tests/test_guidance_gpu.py BACKBONE_KW["mmdit"]


def _tool():
    spec = importlib.util.spec_from_file_location("generate_tool", ROOT / "tools" / "generate.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("extra", [0, 500])
def test_generate_writes_maps_that_equal_the_host_decode(tmp_path, extra):
    """3 s is 376 frames, a multiple of the patch size 4; 500 samples more are 379 frames, sampled as 380 and cut back."""
    sr, samples = 22050, 22050 * 3 + extra
    song = tmp_path / "sine.wav"
    with wave.open(str(song), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(b"".join(struct.pack("<h", int(12000 * math.sin(2 * math.pi * 440.0 * i / sr))) for i in range(samples)))
    out = tmp_path / "maps"
    rc = _tool().main([str(song), "--out", str(out), "--backbone", "mmdit", "--objective", "ddim", "--model-kw", MODEL_KW, "--seed", "3",
                       "--n", "2", "--steps", "4", "--dump-signals"])
    assert rc == 0
    frames = audio.n_frames(samples)
    assert frames == (379 if extra else 376)
    assert sorted(p.name for p in out.iterdir()) == ["sine_0.npz", "sine_0.osu", "sine_1.npz", "sine_1.osu"]
    signals = []
    for k in range(2):
        dump = np.load(out / f"sine_{k}.npz")
        x, ft = dump["x"], dump["frame_times"]
        assert x.shape == (6, frames) and x.dtype == np.float32 and ft.shape == (frames,) and np.isfinite(x).all()
        meta = D.Metadata("sine.wav", "sine", "Unknown", f"OsuFusion {k}", 4.0, 9.0, 8.0, 5.0)
        text = (out / f"sine_{k}.osu").read_text(encoding="utf-8")
        assert text == D.decode_beatmap(meta, x, ft, None, True, verbose=False)
        assert text.startswith("osu file format v14")
        signals.append(x)
    assert not np.array_equal(*signals)                                           # two draws
