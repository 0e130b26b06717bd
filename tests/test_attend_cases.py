"""CPU check: every allocating function of osufusion_amd/attend.py has a poisoned-memory case in tests/test_attend_autograd_gpu.py
(the same rule tests/test_poisoned_memory.py keeps for ops.py and functional.py)."""
import ast
from pathlib import Path

from tests.test_poisoned_memory import allocating_functions

ROOT = Path(__file__).resolve().parent.parent


def _case_keys():
    tree = ast.parse((ROOT / "tests" / "test_attend_autograd_gpu.py").read_text())
    for node in ast.walk(tree):
        if isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == "POISON_CASES" for t in node.targets):
            return {k.value: len(v.elts) for k, v in zip(node.value.keys, node.value.values)}
    raise AssertionError("tests/test_attend_autograd_gpu.py has no POISON_CASES table")


def test_every_allocating_function_of_attend_has_a_poisoned_memory_case():
    sites = allocating_functions(ROOT / "osufusion_amd" / "attend.py")
    assert {"mqa_fwd_masked", "mqa_bwd_masked"} <= sites            # the parser sees the module's wrappers
    keys = _case_keys()
    missing = sorted(s for s in sites if s not in keys)
    assert not missing, f"allocating functions of attend.py without a poisoned-memory case: {missing}"
    stale = sorted(k for k in keys if k not in sites)
    assert not stale, f"POISON_CASES names functions that do not allocate: {stale}"
    assert all(n > 0 for n in keys.values())
