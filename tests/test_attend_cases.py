"""CPU check: osufusion_amd/attend.py allocates nothing itself -- no unguarded torch.empty site, the rule tests/test_poisoned_memory.py keeps
for ops.py and functional.py.  Its launches are ops.mqa_fwd / ops.mqa_bwd (cases in tests/test_poisoned_memory.py) and cross_attend.py's
wrappers (cases in tests/test_cross_attend_gpu.py)."""
from pathlib import Path

from tests.test_poisoned_memory import allocating_functions

ROOT = Path(__file__).resolve().parent.parent


def test_every_allocating_function_of_attend_has_a_poisoned_memory_case():
    assert allocating_functions(ROOT / "osufusion_amd" / "attend.py") == set()
