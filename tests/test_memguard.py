"""CPU self-test of tests/memguard.py (the poisoned, canary-guarded allocator the kernel sweep in test_poisoned_memory.py runs under),
on the call signatures osufusion_amd/ops.py and functional.py use."""
import pytest
import torch

from tests.memguard import CanaryError, guard


def _calls():
    """(name, thunk) for every allocation form of the package: (n,), a tuple shape, varargs, dtype= / device= keywords, empty_like."""
    base = torch.zeros(6, 10)
    return [
        ("n", lambda: torch.empty(37, dtype=torch.float32, device="cpu")),
        ("tuple", lambda: torch.empty((3, 5, 7), dtype=torch.bfloat16, device="cpu")),
        ("varargs", lambda: torch.empty(4, 9, dtype=torch.float64, device=torch.device("cpu"))),
        ("default dtype", lambda: torch.empty((2, 3), device="cpu")),
        ("int32", lambda: torch.empty((5, 3), dtype=torch.int32, device="cpu")),
        ("int64", lambda: torch.empty(11, dtype=torch.int64, device="cpu")),
        ("bool", lambda: torch.empty(13, dtype=torch.bool, device="cpu")),
        ("uint8", lambda: torch.empty(1000, dtype=torch.uint8, device="cpu")),
        ("empty_like", lambda: torch.empty_like(base)),
        ("empty_like dtype", lambda: torch.empty_like(base, dtype=torch.bfloat16)),
        ("empty_like view", lambda: torch.empty_like(base[1:4, 2:7])),            # a non-dense view: a dense (3, 5) result
        ("empty_like permuted", lambda: torch.empty_like(base.t())),              # dense: torch keeps the strides
        ("zero elements", lambda: torch.empty(0, dtype=torch.float32, device="cpu")),
    ]


@pytest.mark.parametrize("byte", [0xFF, 0x7F, 0x00])
def test_fills_shapes_and_slack(byte):
    ref = {name: f() for name, f in _calls()}                                     # unpatched: shapes / dtypes / strides to match
    with guard(byte, device="cpu") as g:
        got = {name: f() for name, f in _calls()}
        for name, t in got.items():
            r = ref[name]
            assert t.shape == r.shape and t.dtype == r.dtype and t.stride() == r.stride() and t.device.type == "cpu", name
            assert t.storage_offset() == 0 and t.untyped_storage().nbytes() >= t.numel() * t.element_size() + 4096, name
            if t.dtype.is_floating_point:
                if t.numel():
                    if byte == 0xFF:
                        assert torch.isnan(t).all(), name
                    else:                                                        # 0x7F: ~3.4e38 in f32 / bf16, ~1.4e306 in f64; 0x00: zeros
                        want = torch.full((t.element_size(),), byte, dtype=torch.uint8).view(t.dtype)[0]
                        assert torch.isfinite(t).all() and (t == want).all(), (name, t.flatten()[0].item())
                        assert byte == 0 or want.double().abs().item() > 1e38
            else:
                assert (t == 0).all(), name                                      # indices / flags: zeros, never a poison byte
        assert g.allocations == len(got)
        g.check()                                                                # nothing written: intact


def test_fill_byte_in_bf16_and_f32_is_the_documented_value():
    with guard(0x7F, device="cpu"):
        a = torch.empty(4, dtype=torch.float32, device="cpu")
        b = torch.empty(4, dtype=torch.bfloat16, device="cpu")
    assert a[0].item() > 3e38 and b[0].float().item() > 3e38


@pytest.mark.parametrize("form", ["n", "tuple", "varargs", "empty_like", "empty_like view", "int32"])
def test_a_write_one_element_past_the_end_is_reported(form):
    f = dict(_calls())[form]
    with guard(0xFF, device="cpu") as g:
        t = f()
        g.check()
        flat = t.as_strided((t.numel() + 1,), (1,), 0) if t.is_contiguous() else None
        assert flat is not None
        flat[-1] = 1                                                             # what an off-by-one kernel store does
        with pytest.raises(CanaryError, match="written past the end") as e:
            g.check()
        assert "test_memguard.py" in str(e.value)                               # the allocating line is named
    # a write INSIDE the tensor is not a finding
    with guard(0xFF, device="cpu") as g:
        t = f()
        t.view(-1)[-1] = 1
        g.check()


def test_place_puts_an_input_in_front_of_poison():
    src = torch.arange(10, dtype=torch.float32)
    with guard(0xFF, device="cpu") as g:
        x = g.place(src)
        assert torch.equal(x, src)
        past = x.as_strided((12,), (1,), 0)
        assert torch.isnan(past[10:]).all()


def test_passthrough_and_restore():
    e, el = torch.empty, torch.empty_like
    with guard(0xFF, device="cpu") as g:
        assert torch.empty is not e and torch.empty_like is not el
        out = torch.zeros(5)
        r = torch.empty(5, out=out)                                              # out=: untouched
        assert r is out and (out == 0).all()
        if torch.cuda.is_available():
            p = torch.empty(8, dtype=torch.uint8, pin_memory=True)               # pinned host staging (ops._upload_table): passes through
            assert p.is_pinned()
        assert g.allocations == 0
    assert torch.empty is e and torch.empty_like is el
    # a guard targeting the GPU leaves CPU allocations (ZeroArena.take's element-size probe) alone
    with guard(0xFF, device="cuda") as g:
        t = torch.empty(0, dtype=torch.bfloat16)
        u = torch.empty(16, dtype=torch.float32, device="cpu")
        assert t.numel() == 0 and g.allocations == 0 and u.untyped_storage().nbytes() == 64
    assert torch.empty is e and torch.empty_like is el


def test_restored_after_an_exception():
    e, el = torch.empty, torch.empty_like
    with pytest.raises(RuntimeError, match="boom"):
        with guard(0x7F, device="cpu"):
            raise RuntimeError("boom")
    assert torch.empty is e and torch.empty_like is el


def test_no_retention_mode():
    with guard(0xFF, device="cpu", canaries=False) as g:
        t = torch.empty(100)
        assert torch.isnan(t).all()
        assert g.records == []
        g.check()
