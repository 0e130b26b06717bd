"""The samplers of all model kinds against the bits and the osuf_* call counts of the commit before the models layer was folded onto one
denoiser contract and one loop (tools/sampler_digests.py, recorded on an MI355X into tests/golden/sampler_parent_digests.json).  The one case
that commit could not run -- stop_after = 0 on the DDIM UNet, an IndexError in its static-buffer set-up -- is recorded there as an error; here
it is held to what the tool itself asserts of it: the result equals the start iterate."""
import importlib.util
import json
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
GOLDEN = json.loads((ROOT / "tests" / "golden" / "sampler_parent_digests.json").read_text())
KINDS = ["unet_ddim", "unet_flow", "dit_ddim", "dit_flow", "ct_ddpm", "ct_2m"]


def _tool():
    spec = importlib.util.spec_from_file_location("sampler_digests_tool", ROOT / "tools" / "sampler_digests.py")
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_the_golden_file_covers_the_case_list():
    tool = _tool()
    assert tool.KINDS == KINDS
    ids = [case[0] for kind in KINDS for case in tool.cases(kind)]
    assert sorted(ids) == sorted(GOLDEN) and len(ids) == 2 * 16 + 2 + 3 + 4
    failed = [k for k, v in GOLDEN.items() if "error" in v]
    assert failed == ["unet_ddim/n250/cs2.0/bf16/plain/stop0"]
    assert all(sum(v["calls"].values()) > 0 for k, v in GOLDEN.items() if k not in failed)


@pytest.mark.parametrize("kind", KINDS)
def test_bits_and_call_counts_are_the_parents(kind):
    got = _tool().run_kind(kind)
    assert got and not [k for k, v in got.items() if "error" in v]
    for case_id, rec in got.items():
        want = GOLDEN[case_id]
        if "error" not in want:
            assert rec["sha256"] == want["sha256"], case_id
            assert rec["calls"] == want["calls"], case_id
            assert rec.get("ode") == want.get("ode"), case_id
