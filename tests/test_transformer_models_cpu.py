"""CPU checks of the DiT / MMDiT model wrappers (osufusion_amd/models/transformer_diffusion.py): state-dict layout, constructor, the DDIM
schedule against the oracle, gradient checkpointing, the GPU-only guard, and the C ABI of the one-launch grouped attention forward."""
import json
from ctypes import c_float, c_int, c_long, c_void_p
from pathlib import Path

import pytest
import torch

from oracle import diffusion_oracle as DO
from osufusion_amd import _lib
from osufusion_amd.models import DiffusionOsuFusionDiT, RectifiedFlowOsuFusionDiT
from osufusion_amd.models.diffusion import DDIMSchedule
from osufusion_amd.modules.dit import DiT, DiTBlock
from osufusion_amd.modules.mmdit import MMDiT, MMDiTBlock

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden"
CLASSES = (DiffusionOsuFusionDiT, RectifiedFlowOsuFusionDiT)
SMALL = {"mmdit": dict(dim_h=32, depth=2, attn_heads=2, attn_kv_heads=1, attn_dim_head=16), "dit": dict(dim_h=96, depth=2, attn_heads=6, attn_dim_head=16)}


@pytest.mark.parametrize("cls", CLASSES, ids=lambda c: c.__name__)
@pytest.mark.parametrize("backbone", ["dit", "mmdit"])
def test_state_dict_is_the_backbones_under_unet(cls, backbone):
    want = json.loads((GOLD / f"state_dict_{backbone}.json").read_text())
    model = cls(512, backbone=backbone)
    got = {k: list(v.shape) for k, v in model.state_dict().items()}
    assert list(got) == ["unet." + k for k in want]
    assert got == {"unet." + k: v for k, v in want.items()}
    other = cls(512, backbone=backbone)
    sd = {k: torch.full_like(v, 0.25) for k, v in model.state_dict().items()}
    assert other.load_state_dict(sd) == torch.nn.modules.module._IncompatibleKeys([], [])
    assert all(torch.equal(v, sd[k]) for k, v in other.state_dict().items())


def test_constructor_defaults_and_backbone_validation():
    d = DiffusionOsuFusionDiT(**SMALL["mmdit"])
    assert isinstance(d.unet, MMDiT) and d.backbone == "mmdit"
    assert (d.cond_drop_prob, d.train_timesteps, d.sampling_timesteps, d.stop_after) == (0.5, 1000, 35, None)
    assert d.scheduler.num_train_timesteps == 1000
    r = RectifiedFlowOsuFusionDiT(**SMALL["mmdit"])
    assert isinstance(r.unet, MMDiT) and (r.cond_drop_prob, r.sample_timesteps) == (0.5, 16)
    assert isinstance(DiffusionOsuFusionDiT(backbone="dit", **SMALL["dit"]).unet, DiT)
    assert isinstance(RectifiedFlowOsuFusionDiT(backbone="dit", sampling_timesteps=5, **SMALL["dit"]).unet, DiT)
    assert (d.unet.dim_in_x, d.unet.emb_a.proj.in_channels, d.unet.mlp_cond[0].in_features) == (6, 96, 5)
    for cls in CLASSES:
        with pytest.raises(ValueError, match="backbone"):
            cls(32, backbone="unet")
    with pytest.raises(ValueError):                       # the backbone's own guards still apply
        DiffusionOsuFusionDiT(48, backbone="dit", attn_heads=2, attn_dim_head=16)


def test_ddim_schedule_for_four_steps_equals_the_oracle():
    sch = DDIMSchedule()
    sch.set_timesteps(4)
    assert sch.timesteps.tolist() == DO.ddim_timesteps(4).tolist() == [750, 500, 250, 0]
    acp = DO.ddim_alphas_cumprod()
    for t in sch.timesteps.tolist():
        a_t = acp[t]
        a_prev = acp[t - 250] if t >= 250 else torch.tensor(1.0)
        want = (float((1 - a_t).sqrt()), float(a_t.sqrt()), float(a_prev.sqrt()), float((1 - a_prev).sqrt()))
        assert sch.step_coefficients(t) == want
        # and the oracle's step is the affine map those coefficients describe (no clamp active at |x0| <= 1)
        x, eps = torch.full((1, 1, 1), 0.1), torch.full((1, 1, 1), 0.05)
        s1, sa, pa, p1 = want
        x0 = (x - s1 * eps) / sa
        assert x0.abs().item() <= 1
        assert torch.allclose(DO.ddim_step(eps, t, x, acp, 4), pa * x0 + p1 * eps, rtol=1e-6, atol=0)


@pytest.mark.parametrize("backbone", ["dit", "mmdit"])
def test_set_gradient_checkpointing_reaches_every_block(backbone, capsys):
    model = DiffusionOsuFusionDiT(backbone=backbone, **SMALL[backbone])
    blocks = [m for m in model.unet.modules() if isinstance(m, (DiTBlock, MMDiTBlock))]
    assert len(blocks) == 2 and not any(b.gradient_checkpointing for b in blocks)
    model.unet.set_gradient_checkpointing(True)
    assert all(b.gradient_checkpointing for b in blocks)
    assert capsys.readouterr().out.count("Set gradient checkpointing to True") == 2
    model.unet.set_gradient_checkpointing(False)
    assert not any(b.gradient_checkpointing for b in blocks)


@pytest.mark.parametrize("cls", CLASSES, ids=lambda c: c.__name__)
@pytest.mark.parametrize("backbone", ["dit", "mmdit"])
def test_cpu_tensors_are_refused(cls, backbone):
    model = cls(backbone=backbone, **SMALL[backbone])
    x, a, c = torch.zeros(1, 6, 16), torch.zeros(1, 96, 16), torch.zeros(1, 5)
    with pytest.raises(RuntimeError, match="MI355X only"):
        model.sample(a, c, x)
    with pytest.raises(RuntimeError, match="MI355X only"):
        model.sample(a, c)
    with pytest.raises(RuntimeError, match="MI355X only"):
        model(x, a, c)


def test_one_launch_switch_is_off_by_default_and_restored():
    from osufusion_amd import ops
    assert not ops.one_launch_attention_on()
    with ops.one_launch_attention(True):
        assert ops.one_launch_attention_on()
        with ops.one_launch_attention(False):
            assert not ops.one_launch_attention_on()
        assert ops.one_launch_attention_on()
    assert not ops.one_launch_attention_on()


def test_capi_gqa_fwd_is_declared_bound_and_exported():
    decls = _lib.read_header()[0]
    assert "osuf_gqa_fwd" in decls, "osuf_gqa_fwd is not declared in include/osufusion_hip.h"
    ret, params = decls["osuf_gqa_fwd"]
    assert ret == "int" and [p.split()[-1].lstrip("*") for p in params] == ["q", "ldq", "k", "ldk", "v", "ldv", "o", "ldo", "o_dtype", "lse2", "B", "H", "G", "N", "head_dim", "scale", "stream"]
    P, L, I, F = c_void_p, c_long, c_int, c_float
    assert _lib.SIGNATURES["osuf_gqa_fwd"] == [P, L, P, L, P, L, P, L, I, P, I, I, I, I, I, F, P]
    mqa = _lib.SIGNATURES["osuf_mqa_fwd"]
    assert _lib.SIGNATURES["osuf_gqa_fwd"] == mqa[:12] + [I] + mqa[12:]         # osuf_mqa_fwd's operands plus G behind H
    assert hasattr(_lib.load(), "osuf_gqa_fwd")


def test_capi_gqa_fwd_validates_its_arguments_on_the_host():
    """Every call returns before a launch (the "pointers" are never dereferenced): -1 invalid argument, -2 unsupported."""
    lib = _lib.load()
    buf = 4096
    H, G, D, B, N = 4, 2, 64, 2, 40
    W = (H + 2 * G) * D

    def call(**kw):
        a = dict(q=buf, k=buf, v=buf, o=buf, ld=W, ldo=H * D, B=B, H=H, G=G, N=N, D=D)
        a.update(kw)
        return lib.osuf_gqa_fwd(a["q"], a["ld"], a["k"], a["ld"], a["v"], a["ld"], a["o"], a["ldo"], 1, buf, a["B"], a["H"], a["G"], a["N"], a["D"],
                                0.125, None)
    for kw in (dict(G=3), dict(G=0), dict(G=-1), dict(H=0), dict(q=buf + 2), dict(k=buf + 8), dict(v=buf + 6), dict(o=buf + 4), dict(ld=W + 4),
               dict(ldo=H * D + 2), dict(B=0), dict(N=0), dict(G=1, q=buf + 2)):
        assert call(**kw) == -1, kw
    assert call(D=48) == -2 and call(D=48, G=1) == -2
