"""CPU checks of the cross-attention path (osufusion_amd/cross_attend.py): the shape validation Attend.forward runs first, the two C-ABI
symbols in the header, the ctypes table and the built library, and a poisoned-memory case in tests/test_cross_attend_gpu.py for every
allocating function of the module (the rule tests/test_attend_cases.py keeps for attend.py)."""
import ast
import re
import subprocess
from pathlib import Path

import pytest
import torch

from tests.test_poisoned_memory import allocating_functions

ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = ("osuf_xattn_fwd", "osuf_xattn_bwd")


def _qkv(B=2, H=4, Nq=10, Nk=7, D=16, G=1):
    return torch.zeros(B, H, Nq, D), torch.zeros(B, G, Nk, D), torch.zeros(B, G, Nk, D)


def test_check_shapes_accepts():
    from osufusion_amd.cross_attend import check_shapes
    q, k, v = _qkv()
    assert check_shapes(q, k, v, None) == (2, 4, 10, 7, 16, 1)
    assert check_shapes(*_qkv(G=4), None) == (2, 4, 10, 7, 16, 4)
    assert check_shapes(*_qkv(Nq=7, Nk=7), None) == (2, 4, 7, 7, 16, 1)           # self-attention passes through the same check
    for shape in ((10, 7), (1, 7), (10, 1), (4, 10, 7), (1, 1, 10, 7), (2, 1, 10, 7), (1, 4, 1, 7), (2, 4, 10, 7), (1,)):
        assert check_shapes(q, k, v, torch.zeros(shape)) == (2, 4, 10, 7, 16, 1)
    assert check_shapes(q, k, v, torch.zeros(10, 7, dtype=torch.bool))[3] == 7


def test_check_shapes_rejects():
    from osufusion_amd.cross_attend import check_shapes
    q, k, v = _qkv()
    with pytest.raises(ValueError, match="same length"):
        check_shapes(q, k, v[:, :, :5], None)
    with pytest.raises(ValueError, match="1 or 4 heads"):
        check_shapes(q, *_qkv(G=2)[1:], None)
    with pytest.raises(ValueError, match="1 or 4 heads"):
        check_shapes(q, _qkv(G=4)[1], v, None)
    with pytest.raises(ValueError, match="at least one key"):
        check_shapes(q, k[:, :, :0], v[:, :, :0], None)
    for shape in ((10, 10), (7, 10), (3, 10, 7), (3, 4, 10, 7), (2, 4, 10, 7, 1), (2, 2, 10, 7), (5,)):
        with pytest.raises(ValueError, match="does not broadcast"):
            check_shapes(q, k, v, torch.zeros(shape))
    with pytest.raises(ValueError):
        check_shapes(q, k[:1], v[:1], None)
    with pytest.raises(ValueError):
        check_shapes(q, k[..., :8], v[..., :8], None)


def test_symbols_declared_bound_and_exported():
    from osufusion_amd import _lib
    header, decls = _lib.HEADER.read_text(), _lib.read_header()[0]
    lib_path = _lib.LIB_PATH
    if not lib_path.exists():
        from osufusion_amd.csrc import build
        build.build()
    syms = subprocess.run(["nm", "-D", "--defined-only", str(lib_path)], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (osuf_\w+)", syms))
    for name in SYMBOLS:
        assert name in decls and decls[name][0] == "int", f"{name} is not declared in include/osufusion_hip.h"
        assert name in _lib.SIGNATURES and name in exported
    # Nq and Nk are two ints where the self-attention entry points have one N
    assert len(_lib.SIGNATURES["osuf_xattn_fwd"]) == len(_lib.SIGNATURES["osuf_mqa_fwd_masked"]) + 1
    assert len(_lib.SIGNATURES["osuf_xattn_bwd"]) == len(_lib.SIGNATURES["osuf_mqa_bwd_masked"]) + 1
    for name in SYMBOLS:                                            # the comment in front of each says what it replaces in the reference
        before = header[:header.index("int " + name + "(")]
        comment = before[before.rindex("/*"):]
        assert comment.rstrip().endswith("*/") and re.search(r"replaces:.*attention\.py:94-99", comment, flags=re.S), name


def _case_keys():
    tree = ast.parse((ROOT / "tests" / "test_cross_attend_gpu.py").read_text())
    for node in ast.walk(tree):
        if isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == "POISON_CASES" for t in node.targets):
            return {k.value: len(v.elts) for k, v in zip(node.value.keys, node.value.values)}
    raise AssertionError("tests/test_cross_attend_gpu.py has no POISON_CASES table")


def test_every_allocating_function_of_cross_attend_has_a_poisoned_memory_case():
    sites = allocating_functions(ROOT / "osufusion_amd" / "cross_attend.py")
    assert {"xattn_fwd", "xattn_bwd"} <= sites                      # the parser sees the module's wrappers
    keys = _case_keys()
    missing = sorted(s for s in sites if s not in keys)
    assert not missing, f"allocating functions of cross_attend.py without a poisoned-memory case: {missing}"
    stale = sorted(k for k in keys if k not in sites)
    assert not stale, f"POISON_CASES names functions that do not allocate: {stale}"
    assert all(n > 0 for n in keys.values())


def test_attend_py_keeps_its_two_allocating_functions():
    assert allocating_functions(ROOT / "osufusion_amd" / "attend.py") == set()       # both moved here: the masked path is this module's
