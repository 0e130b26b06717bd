"""CPU checks of the MMDiT backbone (osufusion_amd/modules/mmdit.py): module layout against the reference, the constructor guards, the
torch restatement (tests/mmdit_oracle.py) against the reference's recorded fixtures, and the C ABI of the joint-attention row kernels."""
import json
from ctypes import c_float, c_int, c_long, c_void_p
from pathlib import Path

import numpy as np
import pytest
import torch

from osufusion_amd import _lib
from osufusion_amd.modules import mmdit as M
from osufusion_amd.pattern import param_pattern, synth_inputs, uniform_pm
from tests import mmdit_oracle as O

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden"
META = json.loads((GOLD / "mmdit_cases.json").read_text())
CASES = {k: v for k, v in META.items() if k.startswith("mmdit_")}
JOINT_ENTRY_POINTS = ("osuf_joint_qknorm_fwd", "osuf_joint_pack", "osuf_joint_unpack", "osuf_joint_qknorm_bwd_workspace_bytes",
                      "osuf_joint_qknorm_bwd")


def _net(m):
    return M.MMDiT(6, 96, 5, m["dim_h"], depth=m["depth"], patch_size=m["patch_size"], attn_dim_head=m["attn_dim_head"],
                   attn_heads=m["attn_heads"], attn_kv_heads=m["attn_kv_heads"], attn_qk_norm=m["attn_qk_norm"])


def _cfg(m):
    return O.MMDiTConfig(dim_h=m["dim_h"], depth=m["depth"], patch_size=m["patch_size"], heads=m["attn_heads"], kv_heads=m["attn_kv_heads"],
                         dim_head=m["attn_dim_head"], qk_norm=m["attn_qk_norm"])


def test_the_three_cases_of_the_fixture_table():
    got = {(m["dim_h"], m["attn_heads"], m["attn_kv_heads"], m["attn_dim_head"], m["depth"], m["patch_size"], m["L"], m["B"], m["attn_qk_norm"])
           for m in CASES.values()}
    assert got == {(96, 6, 2, 16, 2, 4, 203, 2, True), (128, 2, 1, 64, 2, 4, 512, 2, True), (128, 4, 4, 32, 1, 2, 96, 2, False)}


def test_state_dict_matches_reference_defaults():
    want = json.loads((GOLD / "state_dict_mmdit.json").read_text())
    got = {k: list(v.shape) for k, v in M.MMDiT(6, 96, 5, 512).state_dict().items()}
    assert list(got) == list(want)
    assert got == want


@pytest.mark.parametrize("name", sorted(CASES))
def test_parameter_order_matches_the_fixtures(name):
    assert [k for k, _ in _net(CASES[name]).named_parameters()] == CASES[name]["param_names"]


def test_no_qk_norm_has_no_gamma_keys():
    sd = M.MMDiT(6, 96, 5, 128, depth=1, attn_heads=4, attn_kv_heads=4, attn_dim_head=32, attn_qk_norm=False).state_dict()
    assert not any("norm.gamma" in k for k in sd)


def test_reference_names_are_exported():
    from osufusion_amd.modules import dit, unet
    for n in ("modulate", "SinusoidalPositionEmbedding", "FeedForward", "PatchEmbedding", "MultiHeadRMSNorm", "JointAttention", "MMDiTBlock",
              "FinalLayer", "MMDiT"):
        assert hasattr(M, n), n
    assert M.FeedForward is dit.FeedForward and M.MultiHeadRMSNorm is dit.MultiHeadRMSNorm
    assert M.SinusoidalPositionEmbedding is unet.SinusoidalPositionEmbedding
    x, sh, sc = torch.randn(2, 3, 4), torch.randn(2, 4), torch.randn(2, 4)
    assert torch.equal(M.modulate(x, sh, sc), x * (1 + sc[:, None]) + sh[:, None])


def test_constructor_guards():
    with pytest.raises(ValueError, match="multiple of attn_kv_heads"):
        M.MMDiT(6, 96, 5, 384, depth=1, attn_heads=6, attn_kv_heads=4, attn_dim_head=64)
    with pytest.raises(ValueError, match="multiple of attn_kv_heads"):
        M.JointAttention(128, 32, 4, 3)
    with pytest.raises(NotImplementedError, match="head dims 16, 32, 64 and 128"):
        M.MMDiT(6, 96, 5, 96, depth=1, attn_heads=4, attn_kv_heads=2, attn_dim_head=24)
    with pytest.raises(NotImplementedError, match="head dims 16, 32, 64 and 128"):
        M.JointAttention(96, 48, 2, 1)


def test_cpu_tensors_are_refused():
    net = M.MMDiT(6, 96, 5, 64, depth=1, attn_heads=2, attn_kv_heads=1, attn_dim_head=32)
    x, a, c, t, _ = (torch.from_numpy(v) for v in synth_inputs("cpu", 1, 16))
    with pytest.raises(RuntimeError, match="MI355X only"):
        net(x, a, t, c)
    with pytest.raises(RuntimeError, match="MI355X only"):
        net.blocks[0](torch.zeros(1, 4, 64), torch.zeros(1, 4, 64), torch.zeros(1, 64))
    with pytest.raises(RuntimeError, match="MI355X only"):
        net.blocks[0].attn(torch.zeros(1, 4, 64), torch.zeros(1, 6, 64))


def test_initialize_weights_zeroes_adaln_final_layer_and_out():
    m = M.MMDiT(6, 96, 5, 128, depth=2, attn_heads=2, attn_kv_heads=1, attn_dim_head=64)
    for b in m.blocks:
        for lin in (b.modulation_x[1], b.modulation_a[1]):
            assert not lin.weight.any() and not lin.bias.any()
    for lin in (m.final_layer.modulation[1], m.final_layer.linear, m.out):
        assert not lin.weight.any() and not lin.bias.any()
    assert m.blocks[0].attn.to_q_x.weight.abs().sum() > 0 and m.emb_a.proj.weight.abs().sum() > 0
    assert m.attn_context_len == 2048


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_matches_reference_fixtures(name):
    """fp32 restatement, with the reference's own Attend arithmetic (bf16 SDPA), against the imported reference's fixtures at the bounds of
    tests/test_dit_cpu.py: output 1e-5 rel-L2, loss 1e-5, per-parameter gradient norms and gradient heads 1e-4."""
    m = CASES[name]
    p = {k: torch.from_numpy(param_pattern(k, tuple(v.shape)).copy()).requires_grad_() for k, v in _net(m).state_dict().items()}
    x, a, c, t, noise = (torch.from_numpy(v) for v in synth_inputs(name, m["B"], m["L"]))
    g = np.load(GOLD / f"{name}.npz")
    y = O.mmdit_forward(p, _cfg(m), x, a, t, c, attend=O.attend_sdpa_bf16)
    loss = torch.nn.functional.mse_loss(y, noise)
    loss.backward()
    with torch.no_grad():
        yn = O.mmdit_forward(p, _cfg(m), x, a, t, c, keep=torch.zeros(m["B"], dtype=torch.bool), attend=O.attend_sdpa_bf16)
    rel = lambda u, w: float(np.linalg.norm(u - w) / np.linalg.norm(w))
    assert rel(y.detach().numpy(), g["y_cond"]) < 1e-5
    assert rel(yn.numpy(), g["y_null"]) < 1e-5
    assert abs(loss.item() - float(g["loss"])) / float(g["loss"]) < 1e-5
    grad = {k: (p[k].grad if p[k].grad is not None else torch.zeros_like(p[k])) for k in m["param_names"]}      # (the last block's audio tail)
    gn = np.array([grad[k].norm().item() for k in m["param_names"]])
    assert np.all(np.abs(gn - g["grad_norm"]) <= 1e-4 * np.maximum(g["grad_norm"], 1e-3 * g["grad_norm"].max()))
    head = np.stack([np.pad(grad[k].flatten()[:16].numpy(), (0, max(0, 16 - grad[k].numel()))) for k in m["param_names"]])
    assert np.abs(head - g["grad_head"]).max() <= 1e-4 * np.abs(g["grad_head"]).max()


def test_joint_attention_restatement_matches_reference_fixture():
    """The module-level fixture (Na != Nx): outputs 1e-5 rel-L2, every input and parameter gradient 1e-4 (the bounds above)."""
    j = META["joint_attention"]
    g = np.load(GOLD / "mod_joint_attention.npz")
    net = M.JointAttention(j["dim"], j["dim_head"], j["heads"], j["kv_heads"])
    p = {"attn." + k: torch.from_numpy(param_pattern(k, tuple(v.shape)).copy()).requires_grad_() for k, v in net.state_dict().items()}
    x = torch.from_numpy(uniform_pm("joint/x", (j["B"], j["Nx"], j["dim"]), 1.0)).requires_grad_()
    a = torch.from_numpy(uniform_pm("joint/a", (j["B"], j["Na"], j["dim"]), 1.0)).requires_grad_()
    gx = torch.from_numpy(uniform_pm("joint/gx", (j["B"], j["Nx"], j["dim_head"] * j["heads"]), 1.0))
    ga = torch.from_numpy(uniform_pm("joint/ga", (j["B"], j["Na"], j["dim_head"] * j["heads"]), 1.0))
    ox, oa = O.joint_attention(p, "attn.", x, a, j["heads"], j["kv_heads"], j["dim_head"], True, attend=O.attend_sdpa_bf16)
    ((ox * gx).sum() + (oa * ga).sum()).backward()
    rel = lambda u, w: float(np.linalg.norm(u - w) / np.linalg.norm(w))
    assert ox.shape == (j["B"], j["Nx"], j["dim_head"] * j["heads"]) and oa.shape[1] == j["Na"]
    assert rel(ox.detach().numpy(), g["out_x"]) < 1e-5 and rel(oa.detach().numpy(), g["out_a"]) < 1e-5
    assert rel(x.grad.numpy(), g["dx"]) < 1e-4 and rel(a.grad.numpy(), g["da"]) < 1e-4
    for k, v in p.items():
        assert rel(v.grad.numpy(), g["grad/" + k[len("attn."):]]) < 1e-4, k


# ---- C ABI of the joint-attention row kernels (what tests/test_host_logic.py::test_capi_* check for every symbol) -----------------
def test_capi_declares_and_binds_the_joint_entry_points():
    decls = _lib.read_header()[0]
    kinds = {"*": c_void_p, "hipStream_t": c_void_p, "long": c_long, "int": c_int, "float": c_float}
    for name in JOINT_ENTRY_POINTS:
        assert name in decls, f"{name} is not declared in include/osufusion_hip.h"
        assert name in _lib.SIGNATURES, f"{name} is not bound in osufusion_amd/_lib.py"
        want = []
        for prm in decls[name][1]:
            key = "*" if "*" in prm else prm.split()[0]
            want.append(kinds[key])
        assert _lib.SIGNATURES[name] == want, name


def test_capi_joint_entry_points_validate_their_arguments():
    """Host-side checks only (every call returns before a launch): -1 invalid argument."""
    lib = _lib.load()
    M_, Ns, Nj, H, G, D = 8, 4, 10, 4, 2, 32
    assert lib.osuf_joint_qknorm_bwd_workspace_bytes(33, 4, 2, 32) == 3 * (4 + 2) * 32 * 4       # ceil(33 / 16) workgroups of partials
    assert lib.osuf_joint_qknorm_bwd_workspace_bytes(33, 4, 3, 32) == 0                          # H % G
    assert lib.osuf_joint_qknorm_bwd_workspace_bytes(33, 4, 2, 48) == 0                          # head dim
    assert lib.osuf_joint_qknorm_bwd_workspace_bytes(33, 24, 8, 128) == 0                        # (H + 2G) D > 4096
    buf = 4096                                                                                   # a non-null, 16-B aligned "pointer": never dereferenced
    W = (H + 2 * G) * D
    bad = [dict(H=3), dict(D=24), dict(off=7), dict(off=-1), dict(M_=9), dict(Ns=0), dict(ld=W + 2), dict(ptr=buf + 2), dict(ptr=None)]
    for kw in bad:
        a = dict(M_=M_, Ns=Ns, Nj=Nj, off=2, H=H, G=G, D=D, ld=W, ptr=buf)
        a.update(kw)
        tail = (a["M_"], a["Ns"], a["Nj"], a["off"], a["H"], a["G"], a["D"], None)
        assert lib.osuf_joint_qknorm_fwd(1, a["ptr"], a["ld"], buf, W, None, None, None, *tail) == -1, kw
        assert lib.osuf_joint_pack(1, a["ptr"], a["ld"], buf, W, *tail) == -1, kw
        assert lib.osuf_joint_unpack(1, a["ptr"], a["ld"], buf, W, *tail) == -1, kw
        assert lib.osuf_joint_qknorm_bwd(1, a["ptr"], a["ld"], None, W, None, None, None, buf, W, None, None, 0, *tail) == -1, kw
    tail = (M_, Ns, Nj, 2, H, G, D, None)
    assert lib.osuf_joint_qknorm_fwd(1, buf, W, buf, W, None, buf, None, *tail) == -1            # one gamma only
    assert lib.osuf_joint_qknorm_fwd(1, buf, W, buf, W, None, buf, buf, *tail) == -1             # gammas without inv
    assert lib.osuf_joint_qknorm_bwd(1, buf, W, buf, W, buf, buf, buf, buf, W, buf, buf, 16, *tail) == -1    # workspace too small
