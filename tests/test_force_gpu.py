"""The override table of the library (osuf_override_set / osuf_override_get) and its Python front, ops.force: every slot can be set and read
back, bad arguments are refused and change nothing, force() restores what it found, and a forced value does change what the launchers decide.
The decisions are read from host-only entry points (osuf_gemm_tn_workspace_bytes takes no device memory), so only the two tests that allocate a
workspace or look at a device tensor need the GPU; which kernel each forced path then reaches is the business of the path tests themselves
(tests/test_gemm_rows_gpu.py, tests/test_attn_exact_gpu.py and their kernel listings under profiles/)."""
import ctypes

import pytest
import torch

from osufusion_amd import _lib, ops

DEFAULT, EINVAL = -1, -1                                    # OSUF_KNOB_DEFAULT, OSUF_EINVAL
LIB_SWITCHES = list(ops._KNOBS)
ALL = LIB_SWITCHES + list(ops._SWITCHES)
# (M, N1, N2, taps) of the weight gradient: a split plan by default (the 256^2 kernel's case of gemm_reference.WGRAD_EXACT), and none (N2 < 64)
SPLIT, SMALL = (1024, 328, 128, 3), (520, 96, 40, 1)


def get(knob):
    v = ctypes.c_int(12345)
    rc = _lib.load().osuf_override_get(knob, ctypes.byref(v))
    return rc, v.value


def state():
    return [ops._forced(name) for name in ALL]


def ws_bytes(shape):
    return _lib.load().osuf_gemm_tn_workspace_bytes(ops.BF16, *shape)


@pytest.fixture(autouse=True)
def defaults_before_and_after():
    want = [DEFAULT] * len(LIB_SWITCHES) + [True, True]
    assert state() == want
    yield
    assert state() == want


def test_every_slot_sets_and_reads_back_and_bad_arguments_change_nothing():
    lib = _lib.load()
    assert len(LIB_SWITCHES) == 6 and sorted(ops._KNOBS.values()) == list(range(6))
    for knob in range(6):
        for value in (0, 1, 7, DEFAULT):
            assert lib.osuf_override_set(knob, value) == 0
            assert get(knob) == (0, value)
            assert [get(k)[1] for k in range(6) if k != knob] == [DEFAULT] * 5
    assert lib.osuf_override_set(2, 1) == 0
    before = [get(k)[1] for k in range(6)]
    for knob in (-1, 6, 1 << 20):
        assert lib.osuf_override_set(knob, 1) == EINVAL
        assert get(knob) == (EINVAL, 12345)                                    # the out value is left alone
    assert lib.osuf_override_set(0, -2) == EINVAL                              # below OSUF_KNOB_DEFAULT
    assert lib.osuf_override_get(0, None) == EINVAL
    assert [get(k)[1] for k in range(6)] == before
    assert lib.osuf_override_set(2, DEFAULT) == 0


def test_force_restores_on_exit_on_raise_and_in_nesting_order():
    every = dict(gemm_big=3, no8p=True, nohalo=True, wgrad_f32_partials=True, attn_fwd_nowhole=True, attn_fwd_noqsk=True, zdq=False, fwd_rope=False)
    assert sorted(every) == sorted(ALL)
    with ops.force(**every):
        assert state() == [3, 1, 1, 1, 1, 1, False, False]
    with pytest.raises(ZeroDivisionError):
        with ops.force(**every):
            1 / 0
    with ops.force(gemm_big=1, zdq=False):
        with ops.force(gemm_big=0, no8p=True):
            assert state()[:2] == [0, 1] and not ops._SWITCHES["zdq"]
            with pytest.raises(KeyError):
                with ops.force(gemm_big=None, zdq=True):                       # None: the default, inside an outer force
                    assert state()[:2] == [DEFAULT, 1] and ops._SWITCHES["zdq"]
                    raise KeyError
            assert state()[:2] == [0, 1] and not ops._SWITCHES["zdq"]
        assert state()[:2] == [1, DEFAULT] and not ops._SWITCHES["zdq"]


def test_force_refuses_unknown_keywords_and_values():
    with pytest.raises(TypeError):
        ops.force(gemm_bigg=1)
    with pytest.raises(TypeError):
        with ops.force(no8p=True, OSUF_GEMM_NO8P=1):
            pass
    with pytest.raises(RuntimeError):
        with ops.force(no8p=True, gemm_big=-5):                                 # refused by the library: no8p, set first, is put back
            pass


def test_gemm_big_changes_the_weight_gradient_plan():
    assert ws_bytes(SPLIT) > 0 and ws_bytes(SMALL) == 0
    with ops.force(gemm_big=0):
        assert ws_bytes(SPLIT) == 0 and ws_bytes(SMALL) == 0
    with ops.force(gemm_big=1):
        assert ws_bytes(SMALL) > 0 and ws_bytes(SPLIT) > 0
    assert ws_bytes(SPLIT) > 0 and ws_bytes(SMALL) == 0


@pytest.mark.gpu
def test_zdq_decides_the_private_backward_workspace():
    args = (2, 1024, 1, 64, torch.bfloat16, "cuda")
    assert isinstance(ops.fused_bwd_workspace(*args), torch.Tensor)
    with ops.force(zdq=False):
        assert ops.fused_bwd_workspace(*args) is None
    assert isinstance(ops.fused_bwd_workspace(*args), torch.Tensor)


@pytest.mark.gpu
def test_fwd_rope_decides_the_rotating_forward():
    qkv = torch.empty(2, 1024, 3 * 64, dtype=torch.bfloat16, device="cuda")
    assert ops.fwd_rope_ok(qkv, 64, 1, True)
    with ops.force(fwd_rope=False):
        assert not ops.fwd_rope_ok(qkv, 64, 1, True)
    assert ops.fwd_rope_ok(qkv, 64, 1, True)
