"""The any-grid attention forward (csrc/attn_any.hip, pa_attn_any_fwd) without a tolerance: the exact gather and tied-winner cases of
tests/exact_cases.py on ragged token grids, forward only, in both builds and both head dims (exact_cases.ANY_ROUTES).

The kernel differs from the generic forward only in index arithmetic -- a 4-key run that crosses a key row, a column table that repeats its
first three entries, a (kh, kw) stepping branch for Wp < 4, a per-tile carry, a masked partial last tile, query rows >= L that run on a
copy of row L - 1 -- and each of those, done wrong, moves some out element of some case here by a whole quantum
(tests/test_exact_cases_cpu.py: test_every_named_wrong_forward_is_caught, on an fp64 algebra over the kernel's own key walk).
  * gather kinds and below_zero: one key leads every row by >= 150, so out[q] is the V row of that key BIT FOR BIT in both builds;
    bias_rank (K = 0, the tables alone decide, margin 256) is the case that sees a bias entry of the wrong key row or column, below_zero
    (every logit <= -150) the one in which a key >= L left alive with its zeroed K row wins every row and returns zeros;
  * tie kinds (grids with L % 4 == 0): 1, 2 or 4 winners at logit exactly 0 and q . R exactly 0.  The forward computes P = exp2(0) = 1,
    l = n and 1 / l, all exact, so out = the mean of the winners' V rows is held to equality in BOTH builds; a key >= L whose logit is
    not -inf lands at exactly 0 and joins the tie, a whole-quantum error;
  * lse at test_attn_fwd's gates (ties in fp32: 1e-6 absolute, as tests/test_attention_ties_gpu.py) -- the only tolerances in this file;
  * every case: the same bits from a second run; the any-grid launch counter moves by one and ops.attn_launch_counts() does not; sample
    0's operands once more, through the C ABI, into an out buffer pre-filled with a sentinel whose row stride is larger than H * hd and
    which has room for a whole tile of rows behind the sample: the columns beyond H * hd and every row behind the sample keep the
    sentinel (a stored copy of row L - 1 would land there), and so does lse behind its last entry;
  * the aligned grids also run ops.attn_fwd, under the same equalities: both kernels equal the expectation, hence each other.

What these tests cannot see: 70 x 35 itself (position_coded_v holds Hp, Wp <= 63; 35 x 17 and 62 x 31 stand in) and unequal probabilities
within a row.  tests/test_any_size_gpu.py::test_attn_any_vs_float64 keeps that job."""
import pytest
import torch

from tests import exact_cases as X
from tests.test_attention_exact_gpu import DTYPES, LSE_GATE, relerr
from tests.test_attention_exact_gpu import explain_out as explain_gather
from tests.test_attention_ties_gpu import explain_out as explain_tie

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from painter_amd import ops, ops_anysize

DEV = "cuda"
SENTINEL = 24576.0                                       # bf16 holds it; no expected value comes near
PAD_COLS = 16                                            # keeps the row stride a multiple of 16 bytes in both builds


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def assert_expected(case, exp, out, lse, tname, who):
    assert bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(lse).all()), who
    if case.kind in X.TIE_KINDS:
        assert torch.equal(out.double(), exp.out), who + ": " + explain_tie(case, exp, out)
        if tname == "fp32":
            assert float((lse.double() - exp.lse).abs().max()) <= 1e-6, who
    else:
        assert torch.equal(out.float(), exp.out), who + ": " + explain_gather(case, exp, out)
    e_l = relerr(lse, exp.lse)
    assert e_l < LSE_GATE[tname], (who, e_l)


def into_prefilled(case, qkv, rcat, T):
    """Sample 0 alone through the C ABI into sentinel-filled buffers: out [L + 32 rows, H * hd + 16 columns], lse [H * L + 32]."""
    H, L, Hp, Wp, hd = case.H, case.L, case.Hp, case.Wp, case.hd
    out = torch.full((L + 32, H * hd + PAD_COLS), SENTINEL, dtype=T, device=DEV)
    lse = torch.full((H * L + 32,), SENTINEL, dtype=torch.float32, device=DEV)
    ops_anysize.check(ops_anysize.lib.pa_attn_any_fwd(ops.code(T), ops.p(qkv), qkv.stride(0), ops.p(rcat), ops.p(out), out.stride(0), ops.p(lse),
                                                      1, L, H, Hp, Wp, hd, float(case.scale), ops.stream()), "pa_attn_any_fwd")
    return out.cpu(), lse.cpu()


def check(route, kind, grid):
    tname, hd, counter, _ = X.ANY_ROUTES[route]
    assert counter == "pa_attn_any_launches"
    T = DTYPES[tname]
    case, exp = X.any_case(kind, *grid, hd)
    B, H, Hp, Wp, L = case.B, case.H, case.Hp, case.Wp, case.L
    D = H * hd
    qkv = case.qkv.to(T).to(DEV)
    rcat = ops.relpos_pack(case.rel_h.to(DEV), case.rel_w.to(DEV), Hp, Wp, T)

    n0, c0 = ops_anysize.attn_any_launches(), ops.attn_launch_counts()
    out, lse = ops_anysize.attn_any_fwd(qkv, rcat, B, L, H, Hp, Wp, case.scale)
    assert ops_anysize.attn_any_launches() == n0 + 1 and ops.attn_launch_counts() == c0
    assert out.dtype == T and out.shape == (B * L, D) and lse.shape == (B * H, L)
    out, lse = out.cpu(), lse.cpu()
    assert_expected(case, exp, out, lse, tname, "pa_attn_any_fwd")

    again = ops_anysize.attn_any_fwd(qkv, rcat, B, L, H, Hp, Wp, case.scale)
    assert same_bits(out, again[0].cpu()) and same_bits(lse, again[1].cpu())

    n0 = ops_anysize.attn_any_launches()
    wide, wide_lse = into_prefilled(case, qkv[:L], rcat, T)
    assert ops_anysize.attn_any_launches() == n0 + 1 and ops.attn_launch_counts() == c0
    assert same_bits(wide[:L, :D], out[:L]) and same_bits(wide_lse[:H * L], lse[:H].reshape(-1))
    assert bool((wide[:L, D:].float() == SENTINEL).all()), "columns beyond H * hd were written"
    touched = (wide[L:].float() != SENTINEL).any(1).nonzero().flatten().tolist()
    assert not touched, "rows behind the sample were written: rows L + %s (L = %d)" % (touched[:8], L)
    assert bool((wide_lse[H * L:] == SENTINEL).all()), "lse was written behind its last entry"

    if ops_anysize.attn_fwd_takes(L, Hp, Wp):
        c0 = ops.attn_launch_counts()
        old, old_lse = ops.attn_fwd(qkv, rcat, B, L, H, Hp, Wp, case.scale)
        c1 = ops.attn_launch_counts()
        assert sum(c1["fwd"]) == sum(c0["fwd"]) + 1 and ops_anysize.attn_any_launches() == n0 + 1
        assert_expected(case, exp, old.cpu(), old_lse.cpu(), tname, "pa_attn_fwd")
        assert torch.equal(old.cpu().float(), out.float())
    else:
        assert grid not in X.ANY_ALIGNED


PARAMS = X.any_route_params()


@pytest.mark.parametrize("route,kind,B,H,Hp,Wp", PARAMS, ids=["%s-%s-%dx%dx%dx%d" % p for p in PARAMS])
def test_any_grid_attention_is_exact(route, kind, B, H, Hp, Wp):
    """Every route of exact_cases.ANY_ROUTES on every kind its grids run (exact_cases.any_kinds); what is asserted: the module docstring."""
    check(route, kind, (B, H, Hp, Wp))
