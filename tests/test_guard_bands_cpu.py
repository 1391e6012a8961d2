"""The guard-band harness (tests/guard_bands.py) on CPU tensors: it must catch a write one element in front of a payload, one behind it and
one in a row gap, with the right offsets; pass an untouched run; report an unwritten output; and make a module that allocates the way
painter_amd.ops does hand out exact-size arena tensors."""
import types

import pytest
import torch

from tests.guard_bands import GUARD_BYTES, Arena, GuardViolation, TorchProxy, guarded_ops, roundup


def raw(t, n_before, n_total):
    """The elements around t in its storage, as a kernel with a wrong index would reach them: a flat view from n_before elements in front
    of t's first element."""
    return t.as_strided((n_total,), (1,), t.storage_offset() - n_before)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.uint8, torch.int32])
def test_untouched_and_fully_written_runs_pass(dtype):
    a = Arena("cpu", guard_bytes=4096)
    t = a.empty((5, 24), dtype)
    s = a.empty((5, 24), dtype, ld=48, col_off=16)
    assert t.is_contiguous() and s.stride() == (48, 1) and s.data_ptr() % 16 == 0 and t.data_ptr() % 16 == 0
    a.check()
    assert a.unwritten(t) == t.numel() and a.unwritten(s) == s.numel()
    if dtype.is_floating_point:
        assert bool(torch.isnan(t.float()).all()) and bool(torch.isnan(s.float()).all())
    else:
        assert bool((t == (255 if dtype == torch.uint8 else -1)).all())
    t.fill_(1)
    s.fill_(2)
    a.check()
    assert a.unwritten(t) == 0 and a.unwritten(s) == 0


def test_default_guard_is_four_mib_on_each_side():
    a = Arena("cpu")
    t = a.empty((3, 8), torch.float32)
    al = a.allocs[0]
    assert GUARD_BYTES >= 4 << 20 and al.guard == GUARD_BYTES and al.buf.numel() >= 2 * GUARD_BYTES + t.numel() * 4
    assert t.data_ptr() - al.buf.data_ptr() == GUARD_BYTES
    a.check()


def test_write_one_element_before_the_payload_is_caught():
    a = Arena("cpu", guard_bytes=4096)
    a.empty((4, 8), torch.float32, name="ok")
    t = a.empty((4, 8), torch.float32, name="victim")
    raw(t, 1, 1)[0] = 3.0
    with pytest.raises(GuardViolation) as e:
        a.check()
    msg = str(e.value)
    assert msg.count("\n") == 1 and "victim: 4 byte(s)" in msg             # (the untouched allocation is not named)
    assert "first at payload offset -4, last at -1 " in msg          # (3.0f = 00 00 40 40: all four bytes differ from 0xFF)


def test_write_one_element_after_the_payload_is_caught():
    a = Arena("cpu", guard_bytes=4096)
    t = a.empty((4, 8), torch.bfloat16, name="victim")
    raw(t, 0, 33)[32] = 1.0                                          # bf16 1.0 = 0x3F80: both bytes differ from 0xFF
    with pytest.raises(GuardViolation) as e:
        a.check()
    assert "victim: 2 byte(s)" in str(e.value) and "first at payload offset 64, last at 65" in str(e.value)


def test_write_into_a_row_gap_is_caught_on_either_side_of_the_slice():
    for col, where in ((7, 1 * 160 + 28), (32, 1 * 160 + 128)):        # row 1 of a [4, 40] fp32 payload, slice [:, 8:32]: columns 7 and 32
        a = Arena("cpu", guard_bytes=4096)
        t = a.empty((4, 24), torch.float32, ld=40, col_off=8, name="slice")
        t.fill_(0.5)
        raw(t, 8, 4 * 40)[1 * 40 + col] = 0.0
        with pytest.raises(GuardViolation) as e:
            a.check()
        assert "slice: 4 byte(s)" in str(e.value) and "first at payload offset %d, last at %d" % (where, where + 3) in str(e.value)
        assert "rows of 96 bytes at pitch 160 from byte 32" in str(e.value)


def test_unwritten_output_is_reported():
    a = Arena("cpu", guard_bytes=4096)
    t = a.empty((6, 16), torch.bfloat16, ld=24, col_off=8)
    t[:, :15] = 1.0
    assert a.unwritten(t) == 6
    t[:5, 15] = float("nan")                                       # a computed NaN (0x7FC0) is not the poison
    assert a.unwritten(t) == 1
    a.check()


def test_place_surrounds_an_operand_with_nan():
    a = Arena("cpu", guard_bytes=4096)
    x = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    v = a.place(x, ld=12, col_off=4)
    assert torch.equal(v, x) and v.stride() == (12, 1)
    around = raw(v, 4, 36).reshape(3, 12)
    assert bool(torch.isnan(around[:, :4]).all()) and bool(torch.isnan(around[:, 8:]).all())
    a.check()


def test_alignment_of_ld_and_col_off_is_enforced():
    a = Arena("cpu", guard_bytes=4096)
    with pytest.raises(AssertionError):
        a.empty((4, 8), torch.bfloat16, ld=12)                     # 24-byte pitch
    with pytest.raises(AssertionError):
        a.empty((4, 8), torch.bfloat16, ld=16, col_off=4)          # 8-byte offset
    a.empty((4, 8), torch.bfloat16, ld=12, align=8)                # a test that wants the odd pitch says so


def fake_ops():
    """A module that allocates the way painter_amd.ops does: torch.empty / empty_like for results, workspace() for scratch."""
    m = types.ModuleType("fake_ops")
    m.torch = torch
    m.old_helper = lambda M, N, K: 2 * N * K * 4               # what pa_linear_wgrad_workspace_bytes returned for (512, 256, 256): the fast route's 2 slabs
    m.new_helper = lambda M, N, K: 8 * N * K * 4               # the maximum over both routes: the generic engine's 8 slabs

    def workspace(nbytes, device, slot=0):
        return torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
    m.workspace = workspace

    def wgrad(dy, x, helper, slabs):
        """The shape of ops.linear_wgrad: scratch sized by the helper, a 'kernel' that writes `slabs` slabs of N * K floats into it."""
        M, N = dy.shape
        K = x.shape[1]
        out = m.torch.empty((N, K), dtype=m.torch.float32, device=dy.device)
        like = m.torch.empty_like(out)
        ws = m.workspace(helper(M, N, K), dy.device)
        part = ws.view(m.torch.float32).as_strided((slabs, N * K), (N * K, 1))       # (the kernel trusts the caller's size)
        part[:] = (dy.float().t() @ x.float()).reshape(1, -1) / slabs
        out.copy_(part.sum(0).reshape(N, K))
        like.copy_(out)
        return out, like, m.torch.float32, m.torch.zeros(3)
    m.wgrad = wgrad
    return m


def test_guarded_ops_makes_outputs_and_workspace_exact_and_forwards_the_rest(monkeypatch):
    m = fake_ops()
    a = Arena("cpu")
    g = torch.Generator().manual_seed(0)
    dy, x = torch.randn(512, 256, generator=g), torch.randn(512, 256, generator=g)
    with guarded_ops(monkeypatch, a, ops=m) as calls:
        assert isinstance(m.torch, TorchProxy) and m.torch.float32 is torch.float32 and m.torch.nn is torch.nn
        out, like, f32, z = m.wgrad(dy, x, m.new_helper, 8)
        other = m.torch.empty((3,), dtype=torch.float32, device="meta")     # another device: torch's own
        assert m.workspace(0, "cpu").numel() == 16 and m.workspace(17, "cpu").numel() == 32
    assert m.torch is torch and m.workspace(16, "cpu").numel() == 1 << 20     # undone
    assert other.device.type == "meta" and f32 is torch.float32 and z.tolist() == [0, 0, 0]
    assert [n for n, _ in calls] == [8 * 256 * 256 * 4, 0, 17] and calls[0][1].numel() == 8 * 256 * 256 * 4
    owned = [al.tensor.data_ptr() for al in a.allocs]
    assert out.data_ptr() in owned and like.data_ptr() in owned and calls[0][1].data_ptr() in owned
    a.check()
    assert a.unwritten(out) == 0 and torch.allclose(out, dy.t() @ x, atol=1e-3)


def test_an_undersized_workspace_helper_gives_a_guard_report(monkeypatch):
    """The weight-gradient defect as the harness sees it: the helper sizes the scratch for the fast route's 2 slabs, the call takes the
    generic route and writes 8 -- 1.5 MiB past the end.  Unguarded, workspace()'s 1 MiB floor and the allocator's rounding swallow it."""
    m = fake_ops()
    a = Arena("cpu")
    g = torch.Generator().manual_seed(0)
    dy, x = torch.randn(512, 256, generator=g), torch.randn(512, 256, generator=g)
    with guarded_ops(monkeypatch, a, ops=m):
        m.wgrad(dy, x, m.old_helper, 8)
    with pytest.raises(GuardViolation) as e:
        a.check()
    n = 256 * 256 * 4
    assert "workspace #0 (%d bytes asked" % (2 * n) in str(e.value)
    assert "first at payload offset %d" % (2 * n) in str(e.value) and "last at %d" % (8 * n - 1) in str(e.value)
    assert roundup(6 * n, 16) < GUARD_BYTES                       # the overrun fits the guard: nothing else was hit
