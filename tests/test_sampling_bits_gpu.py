"""The sampling step kernels and the transformer diffusion samplers against the bits they produced before the two step kernels became one
template and the three sampling loops one loop (tests/golden/sampling_bits.npz, recorded on the MI355X by
tests/golden/make_sampling_bits_golden.py, whose docstring lists the cases).  Every output is compared on its integer view: no tolerance."""
import pytest
import torch

from tests.golden import make_sampling_bits_golden as G

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def recorded():
    return {name: torch.from_numpy(bits.copy()) for name, bits in G.load().items()}


def _assert_bits(cases, recorded, prefixes):
    """Every recomputed output equals its record, and every record under `prefixes` was recomputed."""
    seen, wrong = set(), []
    for name, out in cases:
        seen.add(name)
        if not torch.equal(G.bits(out), recorded[name]):
            wrong.append(name)
    assert not wrong, f"{len(wrong)} of {len(seen)} outputs differ from the record: {wrong[:8]}"
    assert seen == {n for n in recorded if n.startswith(prefixes)}


def test_ancestral_step_kernel_bits(recorded):
    _assert_bits(G.step_cases(DEV), recorded, ("schedule/", "step/"))


def test_solver_step_kernel_bits(recorded):
    _assert_bits(G.solver_cases(DEV), recorded, ("solver_schedule/", "solver/"))


@pytest.mark.parametrize("backbone", list(G.BACKBONE_KW))
def test_sampling_loop_bits(recorded, backbone):
    _assert_bits(G.loop_cases(DEV, backbone), recorded, (f"loop/{backbone}/",))
