"""The any-grid attention backward (csrc/attn_any_bwd.hip, pa_attn_any_bwd) without a tolerance: the tied-winner and exact gather cases of
tests/exact_cases.py on ragged token grids, in both builds and both head dims (exact_cases.ANY_BWD_ROUTES), and once more through the
adjoint of the rel-pos table resize.

What is new in that kernel is index arithmetic -- the walk of dS into the per-query row and column gradient tables (three branches on Wp,
the + 4 keys of half-wave 1, the per-tile carry), the dG emit, keys >= L and query rows >= L in two kernels, the aux tile that hands lse and
Delta to the dK / dV kernel -- and one such error touches one key of one tile, one table entry or one query row: far inside the 1.6e-2 of the
largest entry that tests/test_any_size_grad_gpu.py::test_attn_any_bwd_vs_float64_autograd allows.  Here every value is exact, so each of
them, done wrong, moves some element by a whole quantum (tests/test_exact_cases_cpu.py: test_every_named_wrong_backward_is_caught, on an
fp64 algebra over the kernel's own key walk, which without a fault equals the fp64 autograd of attn_reference bit for bit).
  * tie kinds: 1, 2 or 4 keys at logit exactly 0, every other key >= 192 below, on grids with any L: the L % 4 keys of
    exact_cases.tie_loners stay outside the groups of four.  The forward must give the exact out and lse first
    (test_attention_any_exact_gpu.assert_expected: the backward consumes them, so a failure is attributed to the right kernel).  bf16 build:
    dQ, dK, dV torch.equal to the exact answer rounded ONCE to bf16, drcat[:2Hp - 1 + 2Wp - 1] torch.equal to the exact answer, the pad rows
    exact zeros.  Exceptions to equality in the bf16 build: none.  The arithmetic is that of tests/test_attention_ties_gpu.py's generic
    route: the winners' Q.K^T is the integer 0, the bias tables are exactly 0, the exponent is -lse2 = -log2 n (attn_any.hip:177,
    attn_any_bwd.hip:74, :163), P = 1 / n, dS = P (dP - Delta) a multiple of 1/16 that bf16 holds (:221), the row and column sums of the
    tables (:176-218) sums of at most four such values that bf16 holds again when dG is packed (:272), every fp32 sum below 2^24 units.
    fp32 build: every element within exact_cases.any_bwd_fp32_bounds, derived there from the kernel's lines and below half a quantum in
    every element of every case (asserted on the CPU); lse within 1e-6 absolute; the count of inexact elements is printed.
  * gather kinds and below_zero (dS = 0), on the tie grids and on 1 x 1, 2 x 1, 11 x 2, 5 x 2: dQ, dK and drcat exactly zero, dV the
    scatter-add of dO rows as tests/test_attention_exact_gpu.py asserts it (bf16 bit for bit but on bias_rank, fp32 within dv_fp32_bound).
    below_zero: a key >= L left alive with its zeroed K row would sit at logit 0 against rows at -150 and below -- its p overflows.
  * every case: pa_attn_any_bwd_launches moves by one per call and neither the forward's counter nor ops.attn_launch_counts() moves; a
    second run gives the same bits; need_drcat=False gives the same dqkv bits; sample 0 once more through the C ABI into a dqkv pre-filled
    with a sentinel, at a row pitch wider than 3 H hd and with a whole tile of rows behind the sample: every column beyond 3 H hd and every
    row behind L keeps the sentinel (a stored row >= L of either kernel would land there).
  * (8, 4), the aligned grid: ops.attn_bwd returns the same values under the same equalities.
  * the chain: attn_any_bwd, then relpos_resize_bwd from table lengths 15 and 9 to the stored 45 and 27 (dyadic pairs), torch.equal to
    any_size_grad_cases.resize_adjoint_statement of the exact drcat.
No tolerance of this file is taken from the kernel's output; the lse gates are tests/test_attention_exact_gpu.py's LSE_GATE.

Kinds left out on a grid (exact_cases.ANY_BWD_LEFT_OUT, each with the CPU condition it fails): a dense dO where V's magnitudes make some dS
need a ninth bit (most grids at head dim 80, 4 x 33 and 31 x 19 at 64), tie_near on 12 x 3 (dK a multiple of 1/64), tie_quarter_sparse where
a tie row of the last query tile has dS = 0.  Found by these cases: nothing -- every case returned the exact bits in the bf16 build
(profiles/attention_any_bwd_exact_gpu_tests.log).

What these tests cannot see: unequal probabilities within a row, the rounding of a dS that bf16 does not hold, 70 x 35 itself
(position_coded_v holds Hp, Wp <= 63).  The tolerance test keeps that job."""
import pytest
import torch

from tests import exact_cases as X
from tests.any_size_grad_cases import resize_adjoint_statement
from tests.test_attention_any_exact_gpu import PAD_COLS, SENTINEL, assert_expected, same_bits
from tests.test_attention_exact_gpu import DTYPES, DV_GATE_BF16, assert_exactly_zero, explain_rows, relerr
from tests.test_attention_ties_gpu import explain_offset_channel, explain_table, once_to_bf16

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from painter_amd import ops, ops_anysize

DEV = "cuda"


def counters():
    return ops_anysize.attn_any_bwd_launches(), ops_anysize.attn_any_launches(), ops.attn_launch_counts()


def forward_and_backward(case, exp, tname):
    """attn_any_fwd, checked, then attn_any_bwd -> (device operands, (dqkv, drcat) on the host)."""
    T = DTYPES[tname]
    B, H, Hp, Wp, L = case.B, case.H, case.Hp, case.Wp, case.L
    qkv, dout = case.qkv.to(T).to(DEV), case.dout.to(T).to(DEV)
    rel_h, rel_w = case.rel_h.to(DEV), case.rel_w.to(DEV)
    rcat, rcatT = ops.relpos_pack(rel_h, rel_w, Hp, Wp, T), ops.relpos_pack_t(rel_h, rel_w, Hp, Wp, T)
    n0 = counters()
    out, lse = ops_anysize.attn_any_fwd(qkv, rcat, B, L, H, Hp, Wp, case.scale)
    n1 = counters()
    assert n1 == (n0[0], n0[1] + 1, n0[2])
    assert_expected(case, exp, out.cpu(), lse.cpu(), tname, "pa_attn_any_fwd")
    dqkv, drcat = ops_anysize.attn_any_bwd(qkv, rcat, rcatT, out, dout, lse, B, L, H, Hp, Wp, case.scale)
    assert counters() == (n1[0] + 1, n1[1], n1[2])                        # its own counter moves by one, the forward's and the old slots do not
    assert dqkv.dtype == T and dqkv.shape == qkv.shape and drcat.dtype == torch.float32 and drcat.shape == (rcat.shape[0], case.hd)
    return (qkv, rcat, rcatT, out, dout, lse), (dqkv.cpu(), drcat.cpu())


def assert_backward(case, exp, tname, dqkv, drcat, who):
    """The equalities of the module docstring on one (dqkv, drcat); prints the fp32 build's figures."""
    D, nrows = case.H * case.hd, 2 * case.Hp + 2 * case.Wp - 2
    for name, t in (("dqkv", dqkv), ("drcat", drcat)):
        assert bool(torch.isfinite(t.float()).all()), "%s: %s is not finite (%d entries)" % (who, name, int((~torch.isfinite(t.float())).sum()))
    assert not bool(drcat[nrows:].any()), who + ": the pad rows of drcat are not zero"
    got = dict(dq=dqkv[:, :D].double(), dk=dqkv[:, D:2 * D].double(), dv=dqkv[:, 2 * D:].double(), drcat=drcat[:nrows].double())
    if case.kind not in X.TIE_KINDS:
        # as tests/test_attention_exact_gpu.py: check
        assert_exactly_zero(case, "dq", dqkv[:, :D])
        assert_exactly_zero(case, "dk", dqkv[:, D:2 * D])
        assert_exactly_zero(case, "drcat", drcat)
        dv, want = got["dv"], exp.dv.double()
        if tname == "bf16" and case.kind != "bias_rank":
            assert torch.equal(dv, want), who + ": " + explain_rows(case, "dv", dv, want)
        elif tname == "bf16":
            e_v = relerr(dv, want)
            print("%s dv %s %dx%d: %d of %d entries differ from the scatter-add, rel-max %.2e" % (who, case.kind, case.Hp, case.Wp, int((dv != want).sum()), dv.numel(), e_v))
            assert e_v < DV_GATE_BF16, e_v
        else:
            bound = X.dv_fp32_bound(case, exp)
            err = (dv - want).abs()
            assert bool((err <= bound).all()), who + ": " + explain_rows(case, "dv (beyond its bound)", torch.where(err <= bound, want, dv), want)
        return
    if tname == "bf16":
        for name in ("dq", "dk", "dv"):
            want = once_to_bf16(getattr(exp, name)).double()
            assert torch.equal(got[name], want), (who + ": " + explain_rows(case, name, got[name], want)
                                                  + (explain_offset_channel(case, got[name], want) if name == "dq" else ""))
        assert torch.equal(got["drcat"], exp.drcat), who + ": " + explain_table(case, got["drcat"], exp.drcat)
        return
    bound = X.any_bwd_fp32_bounds(case, X.tie_algebra(case))
    worst = {}
    for name in ("dq", "dk", "dv", "drcat"):
        want = getattr(exp, name)
        err = (got[name] - want).abs()
        worst[name] = float((err / bound[name].clamp_min(1e-300)).max()) if float(err.max()) else 0.0
        ok = err <= bound[name]
        if name == "drcat":
            assert bool(ok.all()), who + ": " + explain_table(case, torch.where(ok, want, got[name]), want)
        else:
            assert bool(ok.all()), who + ": " + explain_rows(case, name + " (beyond its bound)", torch.where(ok, want, got[name]), want)
    print("fp32 %s %s %dx%dx%dx%d hd%d: entries off the exact answer dq %d dk %d dv %d drcat %d; worst error / bound %s"
          % (who, case.kind, case.B, case.H, case.Hp, case.Wp, case.hd, *(int((got[n] != getattr(exp, n)).sum()) for n in ("dq", "dk", "dv", "drcat")),
             {n: "%.3f" % v for n, v in worst.items()}))


def into_prefilled(case, T, qkv, rcat, rcatT, out, dout, lse):
    """Sample 0 alone through the C ABI: qkv and dqkv at a row pitch of 3 H hd + 16, dqkv [L + 32 rows] pre-filled with a sentinel, no table
    gradient -> dqkv on the host.  The backward twin of test_attention_any_exact_gpu.into_prefilled."""
    H, L, Hp, Wp, hd = case.H, case.L, case.Hp, case.Wp, case.hd
    W = 3 * H * hd
    wide = torch.zeros((L + 32, W + PAD_COLS), dtype=T, device=DEV)
    wide[:L, :W] = qkv[:L]
    dqkv = torch.full((L + 32, W + PAD_COLS), SENTINEL, dtype=T, device=DEV)
    nbytes = ops_anysize.lib.pa_attn_any_bwd_workspace_bytes(ops.code(T), 1, L, H, Hp, Wp, hd)
    assert nbytes > 0
    ws = ops.workspace(nbytes, qkv.device)
    ops_anysize.check(ops_anysize.lib.pa_attn_any_bwd(ops.code(T), ops.p(wide), wide.stride(0), ops.p(rcat), ops.p(rcatT), ops.p(out), out.stride(0),
                                                      ops.p(dout), dout.stride(0), ops.p(lse), ops.p(dqkv), 0, ops.p(ws), 1, L, H, Hp, Wp, hd,
                                                      float(case.scale), ops.stream()), "pa_attn_any_bwd")
    return dqkv.cpu()


def check(route, kind, grid):
    tname, hd, counter, _ = X.ANY_BWD_ROUTES[route]
    assert counter == "pa_attn_any_bwd_launches"
    T = DTYPES[tname]
    case, exp = X.any_case(kind, *grid, hd)
    B, H, Hp, Wp, L = case.B, case.H, case.Hp, case.Wp, case.L
    W = 3 * H * hd
    dev, (dqkv, drcat) = forward_and_backward(case, exp, tname)
    qkv, rcat, rcatT, out, dout, lse = dev
    assert_backward(case, exp, tname, dqkv, drcat, "pa_attn_any_bwd")

    n0 = counters()
    again = ops_anysize.attn_any_bwd(qkv, rcat, rcatT, out, dout, lse, B, L, H, Hp, Wp, case.scale)
    frozen = ops_anysize.attn_any_bwd(qkv, rcat, rcatT, out, dout, lse, B, L, H, Hp, Wp, case.scale, need_drcat=False)
    assert same_bits(dqkv, again[0].cpu()) and same_bits(drcat, again[1].cpu()), "a second run gives other bits"
    assert frozen[1] is None and same_bits(dqkv, frozen[0].cpu()), "need_drcat=False gives other dqkv bits"

    wide = into_prefilled(case, T, qkv, rcat, rcatT, out[:L], dout[:L], lse[:H])
    assert counters() == (n0[0] + 3, n0[1], n0[2])
    assert same_bits(wide[:L, :W], dqkv[:L]), "sample 0 alone, at a wider pitch, gives other bits"
    assert bool((wide[:L, W:].float() == SENTINEL).all()), "columns beyond 3 H hd were written"
    touched = (wide[L:].float() != SENTINEL).any(1).nonzero().flatten().tolist()
    assert not touched, "rows behind the sample were written: rows L + %s (L = %d)" % (touched[:8], L)

    if ops_anysize.attn_fwd_takes(L, Hp, Wp):
        c0 = ops.attn_launch_counts()
        old_out, old_lse = ops.attn_fwd(qkv, rcat, B, L, H, Hp, Wp, case.scale)
        old, old_drcat = ops.attn_bwd(qkv, rcat, rcatT, old_out, dout, old_lse, B, L, H, Hp, Wp, case.scale)
        c1 = ops.attn_launch_counts()
        assert sum(c1["bwd"]) == sum(c0["bwd"]) + 1 and ops_anysize.attn_any_bwd_launches() == n0[0] + 3
        assert_backward(case, exp, tname, old.cpu(), old_drcat.cpu(), "pa_attn_bwd")
        if tname == "bf16" or kind not in X.TIE_KINDS:
            assert torch.equal(old.cpu().float(), dqkv.float()) or kind == "bias_rank"
            assert torch.equal(old_drcat.cpu(), drcat)
    else:
        assert grid != X.ANY_BWD_ALIGNED


PARAMS = X.any_bwd_route_params()


@pytest.mark.parametrize("route,kind,B,H,Hp,Wp", PARAMS, ids=["%s-%s-%dx%dx%dx%d" % p for p in PARAMS])
def test_any_grid_attention_backward_is_exact(route, kind, B, H, Hp, Wp):
    """Every route of exact_cases.ANY_BWD_ROUTES on every kind its grids run (exact_cases.any_bwd_kinds); what is asserted: the module
    docstring."""
    check(route, kind, (B, H, Hp, Wp))


def test_exact_chain_through_the_resize_adjoint():
    """A tie case on 8 x 5 (table lengths 15 and 9), attn_any_bwd, then relpos_resize_bwd to the stored lengths 45 and 27: the exact drcat
    is a table of multiples of 1/32 below 2^15 and the adjoint's weights on these length pairs are dyadic rationals of a few bits
    (tests/test_any_size_grad_cpu.py asserts that CPU float32 autograd of the resize on this very drcat equals float64 bit for bit), so
    the chain must return resize_adjoint_statement of the exact drcat.  In the bf16 build, whose drcat is held to equality; the fp32
    build's is held to a bound, which promises no exact input to the adjoint."""
    tname = "bf16"
    kind, grid, hd = X.ANY_BWD_CHAIN
    case, exp = X.any_case(kind, *grid, hd)
    nh, nw = 2 * case.Hp - 1, 2 * case.Wp - 1
    sh, sw = 3 * nh, 3 * nw
    assert (sh, sw) == (45, 27)
    dev, (dqkv, drcat) = forward_and_backward(case, exp, tname)
    assert_backward(case, exp, tname, dqkv, drcat, "pa_attn_any_bwd")
    got = ops_anysize.relpos_resize_bwd(drcat.to(DEV), sh, sw, nh, nw).cpu()
    assert got.shape == (sh + sw, hd)
    for name, g, res, n in (("rel_pos_h", exp.drcat[:nh], got[:sh], sh), ("rel_pos_w", exp.drcat[nh:], got[sh:], sw)):
        want = resize_adjoint_statement(g, n)
        bad = (res.double() != want).nonzero()
        assert not len(bad), ("%s %d <- %d: %d of %d entries differ from the float64 statement; first: row %d channel %d, got %r, expected %r"
                              % (name, n, g.shape[0], len(bad), res.numel(), int(bad[0][0]), int(bad[0][1]), float(res[tuple(bad[0])]),
                                 float(want[tuple(bad[0])])))
