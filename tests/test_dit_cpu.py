"""CPU checks of the DiT backbone (osufusion_amd/modules/dit.py): module layout against the reference, the head-count guard, the torch
restatement (tests/dit_oracle.py) against the reference's recorded fixtures, and the poisoned-memory table of osufusion_amd/dit.py."""
import ast
import json
from pathlib import Path

import numpy as np
import pytest
import torch

from osufusion_amd.modules.dit import DiT
from osufusion_amd.pattern import param_pattern, synth_inputs
from tests import dit_oracle as O
from tests.test_poisoned_memory import allocating_functions

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden"
CASES = json.loads((GOLD / "dit_cases.json").read_text())


def test_state_dict_matches_reference_defaults():
    want = json.loads((GOLD / "state_dict_dit.json").read_text())
    got = {k: list(v.shape) for k, v in DiT(6, 96, 5, 512).state_dict().items()}
    assert list(got) == list(want)
    assert got == want


def test_no_qk_norm_has_no_gamma_keys():
    sd = DiT(6, 96, 5, 256, depth=1, attn_heads=8, attn_dim_head=32, attn_qk_norm=False).state_dict()
    assert not any("q_norm" in k or "k_norm" in k for k in sd)


def test_head_count_guard():
    with pytest.raises(ValueError, match="attn_heads \\* attn_dim_head == dim_h"):
        DiT(6, 96, 5, 512, depth=1, attn_heads=4, attn_dim_head=64)


def test_initialize_weights_zeroes_adaln_and_postprocess():
    m = DiT(6, 96, 5, 128, depth=2, attn_heads=2, attn_dim_head=64)
    for b in m.blocks:
        assert not b.modulation[1].weight.any() and not b.modulation[1].bias.any()
    assert not m.final.modulation[1].weight.any() and not m.postprocess.weight.any()
    assert m.blocks[0].attn.to_qkv.weight.abs().sum() > 0


def _cfg(m):
    return O.DiTConfig(dim_h=m["dim_h"], depth=m["depth"], heads=m["attn_heads"], dim_head=m["attn_dim_head"], qk_norm=m["attn_qk_norm"])


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_matches_reference_fixtures(name):
    """fp32 restatement, with the reference's own Attend arithmetic (bf16 SDPA), against the imported reference's fixtures: output 1e-5
    rel-L2, loss 1e-5, per-parameter gradient norms 1e-4 (fp32 summation order over up to 2,000 rows)."""
    m = CASES[name]
    net = DiT(6, 96, 5, m["dim_h"], depth=m["depth"], attn_heads=m["attn_heads"], attn_dim_head=m["attn_dim_head"], attn_qk_norm=m["attn_qk_norm"])
    p = {k: torch.from_numpy(param_pattern(k, tuple(v.shape)).copy()).requires_grad_() for k, v in net.state_dict().items()}
    x, a, c, t, noise = (torch.from_numpy(v) for v in synth_inputs(name, m["B"], m["L"]))
    g = np.load(GOLD / f"{name}.npz")
    y = O.dit_forward(p, _cfg(m), x, a, t, c, attend=O.attend_sdpa_bf16)
    loss = torch.nn.functional.mse_loss(y, noise)
    loss.backward()
    with torch.no_grad():
        yn = O.dit_forward(p, _cfg(m), x, a, t, c, keep=torch.zeros(m["B"], dtype=torch.bool), attend=O.attend_sdpa_bf16)
    rel = lambda u, w: float(np.linalg.norm(u - w) / np.linalg.norm(w))
    assert rel(y.detach().numpy(), g["y_cond"]) < 1e-5
    assert rel(yn.numpy(), g["y_null"]) < 1e-5
    assert abs(loss.item() - float(g["loss"])) / float(g["loss"]) < 1e-5
    gn = np.array([p[k].grad.norm().item() for k in m["param_names"]])
    assert np.all(np.abs(gn - g["grad_norm"]) <= 1e-4 * np.maximum(g["grad_norm"], 1e-3 * g["grad_norm"].max()))
    head = np.stack([np.pad(p[k].grad.flatten()[:16].numpy(), (0, max(0, 16 - p[k].numel()))) for k in m["param_names"]])
    assert np.abs(head - g["grad_head"]).max() <= 1e-4 * np.abs(g["grad_head"]).max()


def _case_keys():
    tree = ast.parse((ROOT / "tests" / "test_dit_gpu.py").read_text())
    for node in ast.walk(tree):
        if isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == "POISON_CASES" for t in node.targets):
            return {k.value: len(v.elts) for k, v in zip(node.value.keys, node.value.values)}
    raise AssertionError("tests/test_dit_gpu.py has no POISON_CASES table")


def test_every_allocating_function_of_dit_has_a_poisoned_memory_case():
    sites = allocating_functions(ROOT / "osufusion_amd" / "dit.py")
    assert {"adaln_fwd", "adaln_bwd", "qknorm_fwd", "qknorm_bwd", "stat_pool"} <= sites
    keys = _case_keys()
    assert not sorted(s for s in sites if s not in keys)
    assert not sorted(k for k in keys if k not in sites)
    assert all(n > 0 for n in keys.values())
