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


# ------------------------------------------------------------------------------------------------ the harness of the engine modules
from tests.guard_bands import ALIGN, CountingLib, abi_symbols      # noqa: E402


def test_payloads_start_on_256_bytes():
    a = Arena("cpu", guard_bytes=4096)
    for shape, dtype in (((1,), torch.uint8), ((3, 5), torch.int32), ((7,), torch.float64)):
        assert ALIGN == 256 and a.empty(shape, dtype).data_ptr() % 256 == 0
    s = a.empty((4, 8), torch.float32, ld=16, col_off=4)
    assert (s.data_ptr() - 16) % 256 == 0                              # the payload's base; the slice starts col_off elements in
    with pytest.raises(AssertionError):
        Arena("cpu", guard_bytes=4096 + 16)                            # a guard that would move the payload off its alignment
    a.check()


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int32, torch.int64, torch.float32, torch.float64])
def test_zeros_zeros_like_and_full_come_from_the_arena_and_leave_the_guards_poisoned(dtype):
    a = Arena("cpu", guard_bytes=4096)
    tp = TorchProxy(torch, a)
    z = tp.zeros((3, 5), dtype=dtype, device="cpu")
    z2 = tp.zeros(2, 7, dtype=dtype, device="cpu")                     # the varargs form (painter_engine._forward)
    zl = tp.zeros_like(z)
    f = tp.full((4,), 3, dtype=dtype, device="cpu")
    owned = [al.tensor.data_ptr() for al in a.allocs]
    assert len(a.allocs) == 4 and all(t.data_ptr() in owned for t in (z, z2, zl, f))
    assert z.shape == (3, 5) and z2.shape == (2, 7) and zl.shape == (3, 5) and f.shape == (4,)
    assert all(t.dtype == dtype for t in (z, z2, zl, f))
    assert not z.any() and not z2.any() and not zl.any() and bool((f == 3).all())
    for al in a.allocs:                                                # the fill stayed inside the payload: every other byte is 0xFF
        assert int((al.buf != 0xFF).sum()) <= al.payload_bytes and bool((al.buf[:al.guard] == 0xFF).all()) and bool((al.buf[al.guard + al.payload_bytes:] == 0xFF).all())
    a.check()


def test_the_new_allocators_follow_torch_on_other_devices_and_in_their_defaults():
    a = Arena("cpu", guard_bytes=4096)
    tp = TorchProxy(torch, a)
    assert tp.zeros((3,), device="meta").device.type == "meta" and tp.full((3,), 1.5, device="meta").device.type == "meta"
    assert tp.zeros_like(torch.empty(3, device="meta")).device.type == "meta" and not a.allocs
    assert tp.full((2,), 7, device="cpu").dtype == torch.int64 and tp.full((2,), 1.5, device="cpu").dtype == torch.float32
    assert tp.full((2,), True, device="cpu").dtype == torch.bool and tp.zeros(3, device="cpu").dtype == torch.float32
    assert tp.zeros_like(torch.ones(3, dtype=torch.int32), dtype=torch.float64).dtype == torch.float64 and len(a.allocs) == 5
    other = Arena("cuda", guard_bytes=4096)                            # (no allocation is made: owns() is a comparison of device types)
    assert TorchProxy(torch, other).zeros(3, dtype=torch.uint8).device.type == "cpu"      # no device named: torch's own, as for empty


def test_guarded_ops_works_for_a_module_without_a_workspace(monkeypatch):
    m = types.ModuleType("fake_engine")
    m.torch = torch
    m.run = lambda n: (m.torch.zeros(n, dtype=m.torch.uint8, device="cpu"), m.torch.full((n,), 2, dtype=m.torch.int32, device="cpu"))
    a = Arena("cpu", guard_bytes=4096)
    with guarded_ops(monkeypatch, a, ops=m) as calls:
        z, f = m.run(5)
        assert not hasattr(m, "workspace")
    assert m.torch is torch and calls == [] and len(a.allocs) == 2 and z.tolist() == [0] * 5 and f.tolist() == [2] * 5
    a.check()


def test_exact_workspace_hands_out_the_requested_bytes_unrounded(monkeypatch):
    m = fake_ops()
    a = Arena("cpu", guard_bytes=4096)
    with guarded_ops(monkeypatch, a, ops=m, exact_workspace=True) as calls:
        assert m.workspace(8, "cpu").numel() == 8 and m.workspace(17, "cpu").numel() == 17
        like = m.torch.zeros_like(torch.ones(3, 4), memory_format=torch.preserve_format)      # painter_amd.optim's moments
    assert [n for n, _ in calls] == [8, 17] and a.allocs[0].payload_bytes == 8 and like.shape == (3, 4) and not like.any()
    raw(calls[0][1], 0, 9)[8] = 0                                      # the byte behind an 8-byte workspace is guard
    with pytest.raises(GuardViolation) as e:
        a.check()
    assert "workspace #0 (8 bytes asked" in str(e.value) and "first at payload offset 8, last at 8 (payload 8 bytes)" in str(e.value)


def test_counting_lib_counts_pa_symbols_and_forwards_everything():
    class Stand:
        other = 7

        def pa_twice(self, x, k=1):
            return 2 * x + k

        def pa_never(self):
            return 0

        def load(self):
            return "loaded"
    c = CountingLib(Stand())
    assert c.pa_twice(3) == 7 and c.pa_twice(1, k=0) == 2 and c.load() == "loaded" and c.other == 7
    f = c.pa_twice                                                     # a bound name counts when it is called, not when it is looked up
    assert c.calls == {"pa_twice": 2}
    f(0)
    assert c.calls == {"pa_twice": 3} and "pa_never" not in c.calls and "load" not in c.calls
    with pytest.raises(AttributeError):
        c.pa_missing


def test_abi_symbols_of_the_header():
    import os
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "painter_hip.h")).read()
    names = abi_symbols(text)
    assert len(names) == 134 and all(n.startswith("pa_") for n in names)
    assert {"pa_abi_version", "pa_inst_decode", "pa_restore_tile", "pa_kpt_evaluate", "pa_color_jitter_workspace_bytes"} <= names
    from painter_amd._lib import parse_header
    assert names == set(parse_header())                                # the binding resolves the same set
    extra = "/* int pa_in_a_comment(int a); */\n// int pa_in_a_line_comment(void);\nint64_t pa_new_one(const void* a,\n    int b);\nint pa_call_not_decl(3)\n"
    assert abi_symbols(extra) == {"pa_new_one"} and abi_symbols(text + extra) == names | {"pa_new_one"}


def test_a_kernel_write_one_element_past_its_workspace_names_that_allocation(monkeypatch):
    """The sensitivity of the engine cases, simulated on the CPU: a module that sizes its scratch with a helper (through torch.empty, as
    painter_engine._workspace does) and whose 'kernel' writes one 8-byte key more than the helper allowed for."""
    m = types.ModuleType("fake_engine")
    m.torch = torch
    keys = lambda n, k: 8 * n * k                                       # pa_pose_workspace_bytes: one 64-bit key per box and channel

    def decode(n, k, wrong):
        out = m.torch.zeros(3 * n * k, dtype=m.torch.float32, device="cpu")
        ws = m.torch.empty(keys(n, k), dtype=m.torch.uint8, device="cpu")
        raw(ws.view(m.torch.int64), 0, n * k + wrong)[:] = 5            # (the kernel trusts the caller's size)
        return out
    a = Arena("cpu", guard_bytes=4096)
    with guarded_ops(monkeypatch, a, ops=m):
        decode(3, 17, 0)
    a.check()
    a = Arena("cpu", guard_bytes=4096)
    with guarded_ops(monkeypatch, a, ops=m):
        decode(3, 17, 1)
    with pytest.raises(GuardViolation) as e:
        a.check()
    msg = str(e.value)
    assert msg.count("\n") == 1 and "#1 (408,) uint8: 8 byte(s)" in msg      # the workspace, not the zero-filled output before it
    assert "first at payload offset 408, last at 415 (payload 408 bytes)" in msg
