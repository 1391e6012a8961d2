"""The backward at a run-time input size other than the constructed one (include/painter_anysize_grad.h, painter_amd/ops_anysize.py,
model.grad_at_any_size).  Kernel level: the attention backward for any token grid against float64 autograd of the reference
attention, and the adjoint of the rel-pos table resize against float64 autograd of F.interpolate(mode="linear").  Model level: the
gradients of a model run at another size against the UNMODIFIED reference's (tests/golden/painter_any_size_grads_*.npz) and the oracle's."""
import dataclasses

import pytest
import torch

from oracle import painter_oracle as O
from tests import any_size_cases as C
from tests import golden_util as G
from tests.any_size_grad_cases import DYADIC_PAIRS, RESIZE_PAIRS, resize_adjoint_statement, torch_resize_grad
from tests.guard_bands import CountingLib

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from painter_amd import ops, ops_anysize
    from tests.test_kernels_gpu import attn_reference, gen, relerr
    from tests.test_model_gpu import build

F32, BF16 = torch.float32, torch.bfloat16
# the gates of tests/test_kernels_gpu.py::test_attn_bwd, whose arithmetic per element the any-grid kernels restate
BWD_GATE = {F32: 5e-5, BF16: 1.6e-2}


# ------------------------------------------------------------------------------------------------ attention backward, kernel level
def operands(T, B, H, Hp, Wp, hd, seed=1):
    """-> qkv, rcat, rcatT, dout, (out, lse) of attn_any_fwd."""
    L = Hp * Wp
    qkv = gen((B * L, 3 * H * hd), seed, 1.0, T)
    rel_h, rel_w = gen((2 * Hp - 1, hd), seed + 1, 0.2), gen((2 * Wp - 1, hd), seed + 2, 0.2)
    dout = gen((B * L, H * hd), seed + 3, 1.0, T)
    rcat, rcatT = ops.relpos_pack(rel_h, rel_w, Hp, Wp, T), ops.relpos_pack_t(rel_h, rel_w, Hp, Wp, T)
    out, lse = ops_anysize.attn_any_fwd(qkv, rcat, B, L, H, Hp, Wp, hd ** -0.5)
    return qkv, rcat, rcatT, dout, out, lse


# grid -> what it reaches; B = 2, H = 2 except 70 x 35 (B = 1: the float64 reference stays small)
GRIDS = [(2, 1, 1, 64),          # a single key: dS = 0
         (2, 2, 1, 64),          # L = 2
         (2, 7, 1, 64), (2, 5, 2, 64), (2, 4, 3, 64),      # Wp < 4
         (2, 6, 3, 64),          # L = 18 < 32
         (2, 3, 11, 64),         # L = 33: one row into a second tile
         (2, 9, 7, 64),          # L = 63: one short of a tile
         (2, 10, 5, 64),         # odd Wp, 18-key tail
         (2, 12, 6, 64),         # Wp % 4 != 0
         (2, 8, 4, 64),          # an aligned grid through the any-grid kernel
         (2, 35, 17, 64),        # many tiles
         (1, 70, 35, 64),        # the evaluation recipe's grid
         (2, 5, 2, 80), (2, 3, 11, 80), (2, 10, 5, 80),
         # every wave count of kernel A (dq_kernel_waves; thin tall grids, L <= 250): S = Hp + Wp
         (1, 108, 2, 64),        # S = 110: the last four-wave grid in fp32
         (1, 120, 2, 64),        # S = 122: fp32 takes three waves
         (1, 124, 2, 64),        # S = 126, the largest there is: four waves in bf16, three in fp32
         (1, 90, 2, 80),         # S = 92: the last four-wave grid in fp32 at head dim 80
         (1, 120, 2, 80),        # S = 122: fp32 takes three waves
         (1, 122, 2, 80),        # S = 124: the last four-wave grid in bf16 at head dim 80; fp32 is refused
         (1, 124, 2, 80),        # S = 126: bf16 takes three waves; fp32 is refused
         (1, 70, 35, 80)]        # the evaluation recipe's grid at head dim 80: three waves in fp32


def dq_kernel_waves(T, hd, Hp, Wp):
    """Waves per workgroup of the dQ kernel (kernel A), restated from include/painter_anysize_grad.h: the most of 4, 3 or -- head dim 64
    only -- 2 with 2 * stage + NW * max(128 * (TS + TG), 32 * hd * e) <= 160 KiB, TS = (Hp + Wp + 3) | 1, TG = (Hp + Wp) | 1 (the per-wave
    region rounded up to 16 bytes), stage = 96 * hd * e at head dim 64 and 32 * (2 * (80 * e + 16) + 96 * e) at 80; 0 where none fits
    or Hp + Wp > 126 (the dK / dV kernel's table tile): the grid is refused.  By S = Hp + Wp this gives
        bf16, head dim 64   S <= 126: 4
        fp32, head dim 64   S <= 110: 4   111 - 126: 3
        bf16, head dim 80   S <= 124: 4   125 - 126: 3
        fp32, head dim 80   S <=  92: 4    93 - 123: 3   124 - 126: refused
    (test_dq_kernel_wave_counts).  TWO WAVES ARE UNREACHABLE: at head dim 64 three waves fit up to the S = 126 that kernel B allows, in
    both builds, so the NW = 2 instantiation is never launched."""
    e, S = (2 if T == BF16 else 4), Hp + Wp
    per_wave = (max(128 * (((S + 3) | 1) + (S | 1)), 32 * hd * e) + 15) // 16 * 16
    stage = 96 * hd * e if hd == 64 else 32 * (2 * (80 * e + 16) + 96 * e)
    if S > 126:
        return 0
    return next((nw for nw in ((4, 3, 2) if hd == 64 else (4, 3)) if 2 * stage + nw * per_wave <= 160 * 1024), 0)


def test_dq_kernel_wave_counts():
    """The thresholds of dq_kernel_waves' docstring, the library's refusals at every S (it refuses exactly where no wave count fits), and
    what GRIDS reaches: per (dtype, head dim) the largest four-wave S and, where there is one, a three-wave launch."""
    runs = {}
    for T in (BF16, F32):
        for hd in (64, 80):
            for S in range(3, 130):
                w = dq_kernel_waves(T, hd, S - 2, 2)
                assert dq_kernel_waves(T, hd, 2, S - 2) == w and dq_kernel_waves(T, hd, S // 2, S - S // 2) == w
                assert (ops_anysize.lib.pa_attn_any_bwd_workspace_bytes(ops.code(T), 1, (S - 2) * 2, 2, S - 2, 2, hd) > 0) == (w > 0), (T, hd, S)
                runs.setdefault((T, hd, w), []).append(S)
    span = {k: (min(v), max(v)) for k, v in runs.items()}
    assert span == {(BF16, 64, 4): (3, 126), (BF16, 64, 0): (127, 129),
                    (F32, 64, 4): (3, 110), (F32, 64, 3): (111, 126), (F32, 64, 0): (127, 129),
                    (BF16, 80, 4): (3, 124), (BF16, 80, 3): (125, 126), (BF16, 80, 0): (127, 129),
                    (F32, 80, 4): (3, 92), (F32, 80, 3): (93, 123), (F32, 80, 0): (124, 129)}, span
    assert not any(k[2] == 2 for k in span)                                # two waves: unreachable
    reached = {(T, hd, dq_kernel_waves(T, hd, Hp, Wp), Hp + Wp) for _, Hp, Wp, hd in GRIDS for T in (BF16, F32)}
    for (T, hd, w), (lo, hi) in span.items():
        if w == 4:
            assert (T, hd, 4, hi) in reached, (T, hd, hi)                  # the largest four-wave S
        elif w == 3:
            assert any(r[:3] == (T, hd, 3) for r in reached), (T, hd)      # a three-wave launch
    assert dq_kernel_waves(F32, 80, 70, 35) == 3 and dq_kernel_waves(F32, 64, 70, 35) == 4 and dq_kernel_waves(F32, 80, 124, 2) == 0


@pytest.mark.parametrize("T", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,Hp,Wp,hd", GRIDS, ids=["%dx%d-hd%d" % g[1:] for g in GRIDS])
def test_attn_any_bwd_vs_float64_autograd(T, B, Hp, Wp, hd):
    H, L = 2, Hp * Wp
    nh, nw = 2 * Hp - 1, 2 * Wp - 1
    scale = hd ** -0.5
    if dq_kernel_waves(T, hd, Hp, Wp) == 0:
        # a grid whose tables fit LDS in the other build only: refused before any launch, workspace bytes 0
        assert ops_anysize.lib.pa_attn_any_bwd_workspace_bytes(ops.code(T), B, L, H, Hp, Wp, hd) == 0
        assert ops_anysize.lib.pa_attn_any_bwd_workspace_bytes(ops.code(BF16), B, L, H, Hp, Wp, hd) > 0
        qkv, rcat, rcatT, dout, out, lse = operands(T, B, H, Hp, Wp, hd)     # (the forward takes the grid)
        n0 = ops_anysize.attn_any_bwd_launches()
        with pytest.raises(RuntimeError, match="do not fit LDS"):
            ops_anysize.attn_any_bwd(qkv, rcat, rcatT, out, dout, lse, B, L, H, Hp, Wp, scale)
        dq = torch.full_like(qkv, 7.0)
        ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
        err = ops_anysize.lib.pa_attn_any_bwd(ops.code(T), qkv.data_ptr(), qkv.stride(0), rcat.data_ptr(), rcatT.data_ptr(), out.data_ptr(),
                                              out.stride(0), dout.data_ptr(), dout.stride(0), lse.data_ptr(), dq.data_ptr(), 0, ws.data_ptr(), B, L,
                                              H, Hp, Wp, hd, scale, ops.stream())
        torch.cuda.synchronize()
        assert err == 1 and ops_anysize.attn_any_bwd_launches() == n0 and bool((dq == 7.0).all())
        return
    qkv, rcat, rcatT, dout, out, lse = operands(T, B, H, Hp, Wp, hd)
    n0, f0, c0 = ops_anysize.attn_any_bwd_launches(), ops_anysize.attn_any_launches(), ops.attn_launch_counts()
    dqkv, drcat = ops_anysize.attn_any_bwd(qkv, rcat, rcatT, out, dout, lse, B, L, H, Hp, Wp, scale)
    # its own counter; neither the forward's nor the old slots move
    assert ops_anysize.attn_any_bwd_launches() == n0 + 1 and ops_anysize.attn_any_launches() == f0 and ops.attn_launch_counts() == c0
    assert dqkv.shape == qkv.shape and dqkv.dtype == T and drcat.shape == rcat.shape and drcat.dtype == F32
    q64 = qkv.double().clone().requires_grad_(True)
    rh64 = rcat[:nh].double().clone().requires_grad_(True)
    rw64 = rcat[nh:nh + nw].double().clone().requires_grad_(True)
    ref, _ = attn_reference(q64, rh64, rw64, B, L, H, Hp, Wp, scale)
    ref.backward(dout.double())
    D = H * hd
    # Gate: of the largest entry of the tensor's float64 gradient.  A gradient that is ZERO by the mathematics has no such scale: dq, dk and
    # both table gradients with a single key (P = 1, dS = 0), the gradient of a table of one row (Hp = 1 / Wp = 1: its bias is the same for
    # every key, and sum_k dS = 0).  Such a field is held against the largest entry of the kernel result it is a part of (dqkv; drcat), and
    # with L = 1, where all of drcat is zero, against max|dqkv| * max|q| * B * H: the table gradient a dS of the size of dqkv's entries,
    # summed over the B * H queries, would give.
    gq, gr = q64.grad, torch.cat([rh64.grad, rw64.grad])
    whole_q = float(gq.abs().max())
    whole_r = float(gr.abs().max()) if L > 1 else whole_q * float(qkv.float().abs().max()) * B * H

    def err(got, ref, zero, whole):
        assert not zero or float(ref.abs().max()) < 1e-12 * whole, "the reference gradient is not zero where the mathematics says so"
        return float((got.double() - ref).abs().max()) / (whole if zero else float(ref.abs().max()))
    errs = dict(dq=err(dqkv[:, :D], gq[:, :D], L == 1, whole_q), dk=err(dqkv[:, D:2 * D], gq[:, D:2 * D], L == 1, whole_q),
                dv=err(dqkv[:, 2 * D:], gq[:, 2 * D:], False, whole_q), drh=err(drcat[:nh], rh64.grad, Hp == 1 or L == 1, whole_r),
                drw=err(drcat[nh:nh + nw], rw64.grad, Wp == 1, whole_r))
    print("attn_any_bwd %s B=%d %dx%d hd=%d (%d waves in the dQ kernel): %s"
          % (str(T)[6:], B, Hp, Wp, hd, dq_kernel_waves(T, hd, Hp, Wp), " ".join("%s %.2e" % kv for kv in errs.items())))
    assert max(errs.values()) < BWD_GATE[T], errs
    assert torch.isfinite(dqkv.float()).all() and torch.isfinite(drcat).all()
    assert not drcat[nh + nw:].any()                                      # the pad rows are exact zeros
    # no floating-point atomics: the same input gives the same bits
    dqkv2, drcat2 = ops_anysize.attn_any_bwd(qkv, rcat, rcatT, out, dout, lse, B, L, H, Hp, Wp, scale)
    assert torch.equal(dqkv2, dqkv) and torch.equal(drcat2, drcat)
    # frozen tables: the same data gradient, no table gradient
    dqkv3, none = ops_anysize.attn_any_bwd(qkv, rcat, rcatT, out, dout, lse, B, L, H, Hp, Wp, scale, need_drcat=False)
    assert none is None and torch.equal(dqkv3, dqkv)
    if not ops_anysize.attn_fwd_takes(L, Hp, Wp):
        with pytest.raises(RuntimeError):                                 # pa_attn_bwd keeps its refusal
            ops.attn_bwd(qkv, rcat, rcatT, out, dout, lse, B, L, H, Hp, Wp, scale)


@pytest.mark.parametrize("T", [F32, BF16], ids=["fp32", "bf16"])
def test_attn_any_bwd_row_pitches_are_free(T):
    """qkv, out and dout as column windows of wider buffers: dqkv comes back at qkv's pitch convention with the same bits."""
    B, H, Hp, Wp, hd = 2, 2, 10, 5, 64
    L = Hp * Wp
    qkv, rcat, rcatT, dout, out, lse = operands(T, B, H, Hp, Wp, hd)
    want = ops_anysize.attn_any_bwd(qkv, rcat, rcatT, out, dout, lse, B, L, H, Hp, Wp, hd ** -0.5)

    def wide(t, pad):
        w = torch.full((t.shape[0], t.shape[1] + pad), float("nan"), dtype=T, device=t.device)
        w[:, :t.shape[1]] = t
        return w[:, :t.shape[1]]
    got = ops_anysize.attn_any_bwd(wide(qkv, 64), rcat, rcatT, wide(out, 8), wide(dout, 24), lse, B, L, H, Hp, Wp, hd ** -0.5)
    assert got[0].stride(0) == qkv.shape[1] + 64 and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


@pytest.mark.parametrize("T", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("Hp,Wp", [(10, 5), (3, 11)])
@pytest.mark.parametrize("hd", [64, 80])
def test_attn_any_bwd_poisoned_neighbour(T, Hp, Wp, hd):
    """B = 2 with sample 1's qkv, out, dout and lse all NaN: the keys and query rows behind sample 0's last token are sample 1's first,
    physically.  Sample 0's dqkv rows must be finite and bit-equal to its B = 1 run (where those rows are not the caller's memory at all)."""
    H, L = 2, Hp * Wp
    scale = hd ** -0.5
    qkv, rcat, rcatT, dout, out, lse = operands(T, 1, H, Hp, Wp, hd, seed=21)
    one, _ = ops_anysize.attn_any_bwd(qkv, rcat, rcatT, out, dout, lse, 1, L, H, Hp, Wp, scale)

    def nan2(t):
        return torch.cat([t, torch.full_like(t, float("nan"))])
    two, _ = ops_anysize.attn_any_bwd(nan2(qkv), rcat, rcatT, nan2(out), nan2(dout), nan2(lse), 2, L, H, Hp, Wp, scale)
    assert torch.isfinite(one.float()).all() and torch.isfinite(two[:L].float()).all()
    assert torch.equal(two[:L], one)
    assert torch.isnan(two[L:].float()).all()                  # (and sample 1 is what it was given)


def test_attn_any_bwd_refuses_before_any_launch(monkeypatch):
    """A grid whose tables do not fit LDS, and a grid that is not Hp x Wp: an error, nothing launched, nothing counted."""
    T, B, H, hd = BF16, 1, 1, 64
    Hp, Wp = 100, 40                                           # Hp + Wp = 140 > 126
    L = Hp * Wp
    assert ops_anysize.lib.pa_attn_any_bwd_workspace_bytes(ops.code(T), B, L, H, Hp, Wp, hd) == 0
    assert ops_anysize.lib.pa_attn_any_bwd_workspace_bytes(ops.code(T), 8, 2450, 16, 70, 35, 64) > 0      # the recipe's grid is accepted
    assert ops_anysize.lib.pa_attn_any_bwd_workspace_bytes(ops.code(F32), 8, 2450, 16, 70, 35, 80) > 0
    qkv = torch.zeros((B * L, 3 * H * hd), dtype=T, device="cuda")
    rcat = torch.zeros((ops_anysize.lib.pa_relpos_rows_padded(Hp, Wp), hd), dtype=T, device="cuda")
    o = torch.zeros((B * L, H * hd), dtype=T, device="cuda")
    lse = torch.zeros((B * H, L), dtype=F32, device="cuda")
    n0 = ops_anysize.attn_any_bwd_launches()
    with pytest.raises(RuntimeError):
        ops_anysize.attn_any_bwd(qkv, rcat, rcat.t().contiguous(), o, o, lse, B, L, H, Hp, Wp, 0.125)
    dq = torch.full_like(qkv, 7.0)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    for hp, wp in ((Hp, Wp), (10, 5)):                         # the second: L != Hp * Wp
        err = ops_anysize.lib.pa_attn_any_bwd(ops.code(T), qkv.data_ptr(), qkv.stride(0), rcat.data_ptr(), rcat.data_ptr(), o.data_ptr(), o.stride(0),
                                              o.data_ptr(), o.stride(0), lse.data_ptr(), dq.data_ptr(), 0, ws.data_ptr(), B, L, H, hp, wp, hd, 0.125,
                                              ops.stream())
        assert err == 1                                        # hipErrorInvalidValue
    torch.cuda.synchronize()
    assert ops_anysize.attn_any_bwd_launches() == n0 and bool((dq == 7.0).all())


# ------------------------------------------------------------------------------------------------ adjoint of the rel-pos table resize
@pytest.mark.parametrize("hd", [64, 80])
@pytest.mark.parametrize("sh,sw,dh,dw", RESIZE_PAIRS)
def test_relpos_resize_bwd_vs_float64(sh, sw, dh, dw, hd):
    """The forward test's length pairs.  Gate: 2 x the deviation of CPU torch's own float32 autograd from the float64 statement on the same
    input -- both round a float32 coordinate, as in the forward's test."""
    rows = ops_anysize.lib.pa_relpos_rows_padded((dh + 1) // 2, (dw + 1) // 2)
    drcat = gen((rows, hd), 50, 1.0)                                        # rows behind dh + dw: not the adjoint's business
    out_rows = ops_anysize.lib.pa_relpos_rows_padded((sh + 1) // 2, (sw + 1) // 2)
    got = ops_anysize.relpos_resize_bwd(drcat, sh, sw, dh, dw, out=torch.full((out_rows, hd), float("nan"), device="cuda"))
    assert got.shape == (out_rows, hd) and not got[sh + sw:].any()          # written completely: zero rows behind the two tables
    worst = yard = 0.0
    g_cpu = drcat.cpu()
    for g, res, n in ((g_cpu[:dh], got[:sh], sh), (g_cpu[dh:dh + dw], got[sh:sh + sw], sw)):
        want = resize_adjoint_statement(g, n)
        scale = float(want.abs().max())
        worst = max(worst, float((res.cpu().double() - want).abs().max()) / scale)
        yard = max(yard, float((torch_resize_grad(g, n, torch.float32).double() - want).abs().max()) / scale)
    print("relpos_resize_bwd %d<-%d, %d<-%d hd %d: deviation %.2e of max|dt|, CPU autograd's own %.2e" % (sh, dh, sw, dw, hd, worst, yard))
    assert worst <= 2 * yard, (worst, yard)
    again = ops_anysize.relpos_resize_bwd(drcat, sh, sw, dh, dw, out=torch.empty((out_rows, hd), device="cuda"))
    assert torch.equal(again, got)


@pytest.mark.parametrize("hd", [64, 80])
@pytest.mark.parametrize("role", ["h", "w"])
@pytest.mark.parametrize("src,dst", DYADIC_PAIRS, ids=["%dto%d" % p for p in DYADIC_PAIRS])
def test_relpos_resize_bwd_dyadic_cases_are_exact(src, dst, role, hd):
    """The forward's exact length pairs with integer d out in [-64, 64]: every weight is a dyadic rational of a few bits and every partial
    sum an integer multiple of it far below 2^24, so float32 adds without a rounding in any order -- CPU torch's float32 autograd equals its
    float64 autograd bit for bit (asserted here; tests/test_any_size_grad_cpu.py asserts it without a GPU), and the kernel must too."""
    other = (15, 5)
    (sh, dh), (sw, dw) = ((src, dst), other) if role == "h" else (other, (src, dst))
    g = torch.Generator().manual_seed(100 * src + dst)
    d_out = torch.randint(-64, 65, (dh + dw, hd), generator=g).float()
    got = ops_anysize.relpos_resize_bwd(d_out.cuda(), sh, sw, dh, dw).cpu()
    assert got.shape == (sh + sw, hd)
    for name, gg, res, n in (("rel_pos_h", d_out[:dh], got[:sh], sh), ("rel_pos_w", d_out[dh:], got[sh:], sw)):
        want = resize_adjoint_statement(gg, n)
        assert torch.equal(torch_resize_grad(gg, n, torch.float64), want)
        assert torch.equal(torch_resize_grad(gg, n, torch.float32).double(), want)           # (the case is exact)
        bad = (res.double() != want).nonzero()
        assert not len(bad), ("%s %d <- %d: %d of %d entries differ from the float64 statement; first: row %d channel %d, got %r, expected %r"
                              % (name, n, gg.shape[0], len(bad), res.numel(), int(bad[0][0]), int(bad[0][1]), float(res[tuple(bad[0])]),
                                 float(want[tuple(bad[0])])))


def test_relpos_resize_bwd_of_equal_lengths_copies(monkeypatch):
    counting = CountingLib(ops_anysize.lib)
    monkeypatch.setattr(ops_anysize, "lib", counting)
    g = gen((32, 64), 3, 1.0)
    got = ops_anysize.relpos_resize_bwd(g, 15, 7, 15, 7)
    assert counting.calls == {"pa_relpos_resize_bwd": 1} and torch.equal(got, g[:22])
    got = ops_anysize.relpos_resize_bwd(g, 15, 7, 15, 9)                   # one length stays: copied bit for bit
    assert torch.equal(got[:15], g[:15]) and not torch.equal(got[15:], g[15:22])


# ------------------------------------------------------------------------------------------------ the model
GRADS, GRADS_DIMGS = "painter_any_size_grads_%s.npz", "painter_any_size_grads_%s_dimgs.npz"


def _routes():
    """(any-grid forwards, any-grid backwards, existing forwards, existing backwards) so far."""
    c = ops.attn_launch_counts()
    return ops_anysize.attn_any_launches(), ops_anysize.attn_any_bwd_launches(), sum(c["fwd"]), sum(c["bwd"])


def _step(m, name, leaves=True):
    """One forward + backward of case `name` -> (loss, imgs leaf, tgts leaf)."""
    imgs, tgts, mask, valid = C.inputs(name)
    xi, xt = imgs.cuda().requires_grad_(leaves), tgts.cuda().requires_grad_(leaves)
    loss = m(xi, xt, bool_masked_pos=mask.reshape(C.BATCH, *C.run_config(name).grid).cuda(), valid=valid.cuda())[0]
    loss.backward()
    return loss, xi, xt


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_fp32_build_gradients_at_another_size_vs_reference_golden(name):
    """The fp32 build with the switch on against the UNMODIFIED reference's loss.backward() at that size: every parameter gradient (pos_embed
    through the bicubic resize, every rel-pos table through the linear one), d imgs and d tgts."""
    fx, fxi = G.load(GRADS % name), G.load(GRADS_DIMGS % name)
    cfg = C.config(name)
    m, _ = build(cfg, C.CASES[name][1], "fp32")
    assert m.grad_at_any_size(True) is m
    r0 = _routes()
    loss, xi, xt = _step(m, name)
    r1 = _routes()
    d = tuple(b - a for a, b in zip(r0, r1))
    # every block's attention forward and backward on the any-grid kernels, or (D: 16 x 8) on the existing ones with resized tables
    assert d == ((cfg.depth, cfg.depth, 0, 0) if name != "D" else (0, 0, cfg.depth, cfg.depth)), d
    ref = float(fx["loss"])
    e_l = abs(loss.item() - ref) / abs(ref)
    rep = []
    G.check_grad_digests(fx, "", [(n, p.grad) for n, p in m.named_parameters()], 1e-3, 1e-3, 1e-3, sample_rtol=1e-3, report=rep)
    full = lambda n: fx["grad_full/" + n] if "grad_full/" + n in fx.files else fx["grad/" + n]
    tabs = max((G.rel_fro(p.grad.cpu().reshape(-1), full(n).reshape(-1)), n) for n, p in m.named_parameters() if "rel_pos" in n)
    e_i, e_t = G.rel_err(xi.grad.cpu(), fxi["dimgs"]), G.rel_err(xt.grad.cpu(), fx["dtgts"])
    print("case %s fp32 build, gradients at %s: loss %.2e, worst sampled gradient %.2e (%s), worst rel-pos table (full, rel. Frobenius) %.2e (%s), "
          "d imgs %.2e, d tgts %.2e" % ((name, C.CASES[name][3], e_l) + max(rep) + tabs + (e_i, e_t)))
    assert e_l < C.FP32_GATE and tabs[0] < C.FP32_GATE and e_i < C.FP32_GATE and e_t < C.FP32_GATE, (e_l, tabs, e_i, e_t)
    assert float(m.pos_embed.grad.abs().max()) > 0


def test_switch_off_refuses_and_switch_on_leaves_the_constructed_size_alone(monkeypatch):
    cfg = O.small_config()
    m, _ = build(cfg, 51, "fp32")
    counting = {mod: CountingLib(mod.lib) for mod in (ops, ops_anysize)}
    for mod, c in counting.items():
        monkeypatch.setattr(mod, "lib", c)
    calls = lambda: {k: v for c in counting.values() for k, v in c.calls.items()}
    x = lambda H, W: torch.zeros(1, 3, H, W, device="cuda")
    assert m._hot.grad_any_size is False
    with pytest.raises(NotImplementedError, match="forward only.*grad_at_any_size"):           # the default: today's refusal, nothing launched
        m(x(160, 80), x(160, 80))
    assert calls() == {}
    m.grad_at_any_size(True)
    for bad, what in (((168, 84), "whole numbers of 16-pixel patches"), ((160, 96), r"\(2W, W\)")):   # refused either way
        with pytest.raises(NotImplementedError, match=what):
            m(x(*bad), x(*bad))
    assert calls() == {}
    # the constructed size: the same entry points as often, and the same bits, with the switch on or off
    g = torch.Generator().manual_seed(3)
    H, W = cfg.img_size
    a, b = torch.randn(2, 3, H, W, generator=g).cuda(), torch.randn(2, 3, H, W, generator=g).cuda()
    res = {}
    for on in (None, False, True, False):                      # (None: a first call, which packs the tables once)
        m.grad_at_any_size(bool(on))
        for c in counting.values():
            c.calls.clear()
        m.zero_grad(set_to_none=True)
        xi = a.clone().requires_grad_(True)
        loss = m(xi, b)[0]
        loss.backward()
        torch.cuda.synchronize()
        cur = (calls(), loss.detach().clone(), xi.grad.clone(), {n: p.grad.clone() for n, p in m.named_parameters()})
        if on is None:
            continue
        if not res:
            res["first"] = cur
            continue
        first = res["first"]
        assert cur[0] == first[0] and "pa_attn_any_bwd" not in cur[0] and "pa_relpos_resize_bwd" not in cur[0]
        assert torch.equal(cur[1], first[1]) and torch.equal(cur[2], first[2])
        for n in first[3]:
            assert torch.equal(cur[3][n], first[3][n]), n


def test_frozen_model_prompt_tuning_at_160x80(monkeypatch):
    """imgs / tgts require grad, every parameter is frozen: d tgts against the reference, and none of the parameters' separable work runs."""
    name = "A"
    fx, fxi = G.load(GRADS % name), G.load(GRADS_DIMGS % name)
    m, _ = build(C.config(name), C.CASES[name][1], "fp32")
    m.grad_at_any_size(True)
    for p in m.parameters():
        p.requires_grad_(False)
    counting = {mod: CountingLib(mod.lib) for mod in (ops, ops_anysize)}
    for mod, c in counting.items():
        monkeypatch.setattr(mod, "lib", c)
    loss, xi, xt = _step(m, name)
    e_i, e_t = G.rel_err(xi.grad.cpu(), fxi["dimgs"]), G.rel_err(xt.grad.cpu(), fx["dtgts"])
    print("frozen model at 160 x 80: d imgs %.2e, d tgts %.2e" % (e_i, e_t))
    assert e_i < C.FP32_GATE and e_t < C.FP32_GATE
    launched = {k for c in counting.values() for k in c.calls}
    assert "pa_attn_any_bwd" in launched
    for sym in ("pa_linear_wgrad", "pa_relpos_resize_bwd", "pa_attn_bwd_relpos", "pa_layernorm_bwd_finish", "pa_conv3x3_wgrad", "pa_patch_embed_wgrad",
                "pa_pos_bwd"):
        assert sym not in launched, sym
    assert all(p.grad is None for p in m.parameters())


def test_sizes_used_alternately_with_backward_keep_their_bits():
    cfg = O.small_config()
    m, _ = build(cfg, 52, "bf16")
    m.grad_at_any_size(True)
    g = torch.Generator().manual_seed(5)
    xs = {s: (torch.randn(1, 3, 2 * s, s, generator=g).cuda(), torch.randn(1, 3, 2 * s, s, generator=g).cuda()) for s in (80, 48, cfg.img_size[1])}
    first = {}
    for rnd in range(3):
        for s, (a, b) in xs.items():
            m.zero_grad(set_to_none=True)
            xi = a.clone().requires_grad_(True)
            loss = m(xi, b)[0]
            loss.backward()
            cur = [loss.detach().clone(), xi.grad.clone()] + [p.grad.clone() for p in m.parameters()]
            ref = first.setdefault(s, cur)
            for k, (u, v) in enumerate(zip(ref, cur)):
                assert torch.equal(u, v), (rnd, s, k)


def test_one_adamw_step_at_160x80_moves_the_stored_tables(monkeypatch):
    from painter_amd import optim as PO
    cfg = O.small_config()
    m, _ = build(cfg, 54, "bf16")
    m.grad_at_any_size(True)
    counting = CountingLib(ops_anysize.lib)
    monkeypatch.setattr(ops_anysize, "lib", counting)
    opt = PO.AdamW([{"params": list(m.parameters()), "weight_decay": 0.0}], lr=1e-2).bind_model(m)
    g = torch.Generator().manual_seed(6)
    a, b = torch.randn(1, 3, 160, 80, generator=g).cuda(), torch.randn(1, 3, 160, 80, generator=g).cuda()
    mask = torch.zeros(1, 50, dtype=torch.bool)
    mask[:, 25:] = True
    before = {n: p.detach().clone() for n, p in m.named_parameters() if "rel_pos" in n or n == "pos_embed"}
    loss0 = m(a, b, bool_masked_pos=mask.cuda())[0]
    loss0.backward()
    assert counting.calls.get("pa_relpos_resize") == 1
    opt.step()
    for n, p in m.named_parameters():
        if n in before:
            assert p.shape == before[n].shape and not torch.equal(p.detach(), before[n]), n          # the STORED tables moved
    with torch.no_grad():
        loss1 = m(a, b, bool_masked_pos=mask.cuda())[0]
    assert counting.calls.get("pa_relpos_resize") == 2 and torch.isfinite(loss1) and float(loss1) != float(loss0)


def _oracle_on_device(cfg, P, imgs, tgts, mask, valid, dtype, autocast=False):
    """tests/test_model_gpu.py's: the oracle's loss, pred and parameter gradients on the GPU in `dtype` (optionally under bf16 autocast)."""
    Pd = {k: v.to("cuda", dtype).requires_grad_(True) for k, v in P.items()}
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        lo, po, _ = O.forward(Pd, cfg, imgs.to("cuda", dtype), tgts.to("cuda", dtype), mask.to("cuda"), valid.to("cuda", dtype))
    lo.backward()
    return lo.item(), po.detach().double(), {k: v.grad.double() for k, v in Pd.items()}


@pytest.mark.parametrize("name", ["A", "F"])
def test_bf16_build_gradients_at_another_size_vs_oracle_in_fp64(name):
    """Modelled on tests/test_model_gpu.py::test_vit_huge_full_width_vs_oracle_in_fp64: the loss, the pred and every weight matrix's gradient
    within 1.25 x the oracle's own CUDA bf16-autocast deviation from float64 on the same case."""
    cfg = C.config(name)
    m, P = build(cfg, C.CASES[name][1], "bf16")
    m.grad_at_any_size(True)
    imgs, tgts, mask, valid = C.inputs(name)
    r0 = _routes()
    loss, pred, _ = m(imgs.cuda(), tgts.cuda(), bool_masked_pos=mask.reshape(C.BATCH, *C.run_config(name).grid).cuda(), valid=valid.clone().cuda())
    loss.backward()
    d = tuple(b - a for a, b in zip(r0, _routes()))
    assert d == (cfg.depth, cfg.depth, 0, 0), d
    loss, pred = loss.item(), pred.detach().double()
    grads = {n: p.grad.double() for n, p in m.named_parameters()}
    lo, po, go = _oracle_on_device(cfg, P, imgs, tgts, mask, valid, torch.float64)
    la, pa, ga = _oracle_on_device(cfg, P, imgs, tgts, mask, valid, torch.float32, autocast=True)
    rf = lambda a, b: float((a - b).norm() / b.norm().clamp_min(1e-30))
    e_loss, e_pred, y_loss, y_pred = abs(loss - lo) / abs(lo), rf(pred, po), abs(la - lo) / abs(lo), rf(pa, po)
    mats = [n for n in grads if n.endswith("weight") and grads[n].dim() >= 2]
    ratio = {n: rf(grads[n].reshape(go[n].shape), go[n]) / rf(ga[n], go[n]) for n in mats}
    worst = max((v, n) for n, v in ratio.items())
    tabs = max((rf(grads[n].reshape(go[n].shape), go[n]) / rf(ga[n], go[n]), n) for n in grads if "rel_pos" in n)
    print("case %s bf16 build vs fp64 oracle (oracle's own bf16 autocast): loss %.2e (%.2e), pred %.2e (%.2e); %d weight matrices, worst gradient "
          "ratio %.2f (%s); rel-pos tables (reported, not gated), worst ratio %.2f (%s)" % ((name, e_loss, y_loss, e_pred, y_pred, len(mats)) + worst + tabs))
    assert e_loss <= 1.25 * y_loss and e_pred <= 1.25 * y_pred, (e_loss, y_loss, e_pred, y_pred)
    assert worst[0] <= 1.25, worst


def _worst_gradient(m, Po):
    worst = ("", 0.0)
    for name, p in m.named_parameters():
        go = Po[name].grad
        if p.grad is None or go is None:              # an unused parameter: None here, None or zeros there
            assert (go is None or float(go.abs().max()) == 0.0) and (p.grad is None or float(p.grad.abs().max()) == 0.0), name
            continue
        den = float(go.abs().max())
        if den == 0.0:
            assert float(p.grad.abs().max()) == 0.0, name
            continue
        e = float((p.grad.cpu().reshape(go.shape) - go).abs().max()) / den
        if e > worst[1]:
            worst = (name, e)
    return worst


def test_seggpt_gradients_at_10x5_vs_oracle():
    """Both type tokens and the feature ensemble at 160 x 80, fp32 build against the oracle's autograd: the fp32 gates of
    tests/test_model_gpu.py::test_small_seggpt_feature_ensemble_under_autograd_vs_oracle (loss 1e-4, every gradient 2e-3 of its largest entry)."""
    cfg = O.small_config(seggpt=True)
    run = dataclasses.replace(cfg, img_size=(160, 80))
    n, merge = 3, 0
    m, P = build(cfg, 71, "fp32")
    m.grad_at_any_size(True)
    imgs, tgts, _, valid = O.synthetic_batch(run, n, 72, "half")
    L = run.grid[0] * run.grid[1]
    mask = torch.zeros(1, L)
    mask[:, L // 2:] = 1
    seg_type = torch.tensor([[1.0], [0.0], [1.0]])             # both type tokens
    r0 = _routes()
    loss, _, _ = m(imgs.cuda(), tgts.cuda(), mask.cuda(), valid.clone().cuda(), seg_type.cuda(), merge)
    loss.backward()
    d = tuple(b - a for a, b in zip(r0, _routes()))
    assert d == (cfg.depth, cfg.depth, 0, 0), d
    Po = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    lo, _, _ = O.forward(Po, cfg, imgs, tgts, mask.bool().expand(n, L), valid.clone(), seg_type, merge)
    lo.backward()
    worst = _worst_gradient(m, Po)
    print("SegGPT ensemble under autograd at 10 x 5: loss %.6f vs oracle %.6f, worst gradient %s %.2e" % ((loss.item(), lo.item()) + worst))
    assert abs(loss.item() - lo.item()) < 1e-4 * abs(lo.item()) and worst[1] < 2e-3, (loss.item(), lo.item(), worst)
    assert all(m.get_parameter(t).grad is not None and float(m.get_parameter(t).grad.abs().max()) > 0 for t in ("type_token_cls", "type_token_ins"))


def test_train_mode_at_10x5_with_a_dropped_sample_vs_oracle():
    """DropPath at another size: the any-grid kernels compute a dropped sample, whose dout rows are zeros.  _drop_override drops sample 1 in
    block 2 (factor 0; the oracle takes one factor per block and sample, shared by the block's two branches) -- gradients against the
    oracle given the same factors, at the fp32 gates of the existing train-mode test (loss 1e-4, every gradient 2e-3 of its largest entry)."""
    cfg = C.config("A")
    m, P = build(cfg, C.CASES["A"][1], "fp32")
    m.grad_at_any_size(True)
    m.train()
    imgs, tgts, mask, valid = C.inputs("A")
    scales, over = [], []
    for i, blk in enumerate(m.blocks):
        if blk.drop_path_prob <= 0.0:
            scales.append(None)
            over.append((None, None))
            continue
        bc = 2 * C.BATCH if i <= cfg.merge_idx else C.BATCH
        sc = torch.full((bc,), 1.0 / (1.0 - blk.drop_path_prob))
        if i == 2:
            sc[1] = 0.0
        scales.append(sc)
        over.append((sc.cuda(), sc.cuda()))
    assert float(scales[2].min()) == 0.0
    m._drop_override = over
    loss, _, _ = m(imgs.cuda(), tgts.cuda(), bool_masked_pos=mask.reshape(C.BATCH, *C.run_config("A").grid).cuda(), valid=valid.clone().cuda())
    loss.backward()
    Po = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    lo, _, _ = O.forward(Po, cfg, imgs, tgts, mask, valid.clone(), drop_scales=scales)
    lo.backward()
    worst = _worst_gradient(m, Po)
    print("train mode at 10 x 5, sample 1 dropped in block 2: loss %.6f vs oracle %.6f, worst gradient %s %.2e" % ((loss.item(), lo.item()) + worst))
    assert abs(loss.item() - lo.item()) < 1e-4 * abs(lo.item()) and worst[1] < 2e-3, (loss.item(), lo.item(), worst)


def test_small_model_gradients_at_70x35_vs_oracle_in_fp64():
    """The evaluation recipe's grid, 70 x 35 tokens (L = 2450; 4900 and 2450 rows: multiples of neither 32 nor 128), through every backward
    entry point of the step on the small model, B = 1, fp32 build against the oracle in float64 on the device: the loss at 1e-4 and every
    gradient tensor at 1e-3 (relative Frobenius), the fp32 gates of tests/test_model_gpu.py::test_vit_huge_full_width_vs_oracle_in_fp64."""
    cfg = O.small_config()
    run = dataclasses.replace(cfg, img_size=(1120, 560))
    m, P = build(cfg, 93, "fp32")
    m.grad_at_any_size(True)
    imgs, tgts, mask, valid = O.synthetic_batch(run, 1, 94, "half")
    r0 = _routes()
    loss, pred, _ = m(imgs.cuda(), tgts.cuda(), bool_masked_pos=mask.reshape(1, 70, 35).cuda(), valid=valid.clone().cuda())
    loss.backward()
    d = tuple(b - a for a, b in zip(r0, _routes()))
    assert d == (cfg.depth, cfg.depth, 0, 0) and pred.shape[1] == 2450, d
    grads = {n: p.grad.double() for n, p in m.named_parameters()}
    lo, po, go = _oracle_on_device(cfg, P, imgs, tgts, mask, valid, torch.float64)
    rf = lambda a, b: float((a - b).norm() / b.norm().clamp_min(1e-30))
    e_loss, e_pred = abs(loss.item() - lo) / abs(lo), rf(pred.detach().double(), po)
    worst = max((rf(grads[n].reshape(go[n].shape), go[n]), n) for n in grads)
    print("small model at 1120 x 560 (70 x 35 tokens) fp32 build vs fp64 oracle: loss %.2e, pred %.2e, worst gradient %.2e (%s)" % ((e_loss, e_pred) + worst))
    assert e_loss < 1e-4 and e_pred < 2e-4 and worst[0] < 1e-3, (e_loss, e_pred, worst)
