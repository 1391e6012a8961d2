"""Attention without a tolerance, with a NON-ZERO dS: several keys tie exactly for first place (tests/exact_cases.py, tie_case), on every
kernel route of tests/test_attention_exact_gpu.py.

In every query row 1, 2 or 4 keys sit at logit exactly 0 (all three counts inside every 32-row tile, the last rows of the grid among the
tie rows) and every other key is >= 192 below, so P is exactly 1/n on the winners and 0 elsewhere, l = n, lse = log n, and every quantity
of the forward and the backward is a dyadic rational of a few bits: the fp64 autograd of attn_reference IS the exact answer (to 1e-80;
tests/test_exact_cases_cpu.py asserts this and every other condition below, for every case, without a GPU).  The bf16 build must return
  * out: the mean of the winners' position-coded V rows, exact quarters, bit for bit -- torch.equal, no exception on any route;
  * dQ, dK, dV: the exact answer rounded ONCE to bf16; both table gradients (fp32): the exact answer as it stands -- they are sums of exact
    products whose partial sums fp32 holds exactly in any order (sum of |terms| below 2^24 units of the finest term);
  * the same bits on a second run, and value for value the same from prep="launch" as from the fused generation-3 backward.
What that rests on, kernel by kernel: the winners' Q.K^T is the integer 0 (the shift channels put the row's top logit into the product
itself) and the per-query bias tables are exactly 0 (q is zero on the one channel where the tables are not), so the backward's exponent at
a winner is 0 * c - lse * log2e; lse = (0 + log2 n) * LN2_F (attn_fwd.hip:150, attn2.hip:206, attn3.hip:204) and fl(LN2_F * LOG2E_F) = 1, so
the generic and generation-2 kernels take exp2 of -log2 n itself; generation 3 reads -lse / scale back from a bf16 hi + lo pair
(attn3.hip:208-211), 2^-16 relative off, which moves P by 1e-5 of itself: P = 1/n once it is rounded to bf16, dS = P (dP - Delta) -- a
multiple of 1/16 that bf16 holds -- once it is packed for the MFMAs, and the per-query bias gradient (its class sums) likewise.

The offset channel (q = K = 0, rel_pos_h[j] = rel_pos_w[j] = j + 1) makes dQ there sum_k dS[q, k] (jh(q, k) + jw(q, k) + 2): a wrong entry
is reported with the winners' dS and table rows and with the shift of table rows that would explain it.

Exceptions to equality in the bf16 build: none.  Every route returned the exact bits (profiles/attention_ties_gpu_tests.log).

Found by these cases: the generation-2 and generation-3 forward returned NaN for every row whose first 32 logits all lie below -88.7 -- here
every row without a winner among the first 32 keys (test_forward_with_a_first_key_tile_far_below_zero, fixed with it).

fp32 build: P is exp2 of a rounded lse and dS a rounded product, so equality is not promised; every element is held to
exact_cases.tie_fp32_bounds, (sum of |terms|) * c * 2^-22 with c derived there from the kernels' lines: 2.25 for dS, N / 4 for a sum of N
non-zero terms, and for the table gradients the split-K structure of their GEMM (per slab of token rows N_s / 4 of the slab's sum, then
S / 4 for the reduction of the S slabs).  This bound is below half a quantum -- the smallest spacing of the expected values of the
tensor -- in every element of dQ, dK, dV and both table gradients of every case (asserted on the CPU; largest 0.05 quanta for dQ, 0.32
for a table row), so a value one quantum off cannot pass in the fp32 build either.  lse is additionally held to 1e-6 absolute (0, log 2,
log 4).  (Measured, profiles/attention_ties_gpu_tests.log: the fp32 build returned the exact answer in every element of all 69 cases.)
These are this file's own assertions; the 1.6e-2 / 5e-2 / TOL gates of the tolerance tests are not used (LSE_GATE of the gather tests is).

What these tests cannot see: unequal probabilities within a row, and the rounding of a dS that bf16 does not hold; the per-query bias
tables are zero in the forward (bias_rank of the gather tests covers those).  The tolerance tests keep that job."""
import pytest
import torch

from tests import exact_cases as X
from tests.test_attention_exact_gpu import DTYPES, LSE_GATE, explain_rows, generation, relerr, run      # noqa: F401 (generation is a fixture)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from painter_amd import ops


def once_to_bf16(t):
    """fp64 dyadic values -> bf16 in one rounding (they fit fp32 exactly: below 2^15 in multiples of 2^-5)."""
    f = t.float()
    assert torch.equal(f.double(), t)
    return f.to(torch.bfloat16).float()


def explain_out(case, exp, out):
    B, H, L, hd = case.B, case.H, case.L, case.hd
    got, want = out.float().reshape(B, L, H, hd), exp.out.float().reshape(B, L, H, hd)
    bad = (got != want).any(-1)
    b, q, h = (int(v) for v in bad.nonzero()[0])
    one = X.decode_v_row(got[b, q, h])
    return ("%d of %d output rows wrong; first: sample %d head %d query %d (%d winners): %s"
            % (int(bad.sum()), B * L * H, b, h, q, int(exp.nwin[b, h, q]),
               ("a single V row, of key (kh %(kh)d, kw %(kw)d) of head %(head)d, sample %(sample)d: the tie was lost to one winner" % one) if one
               else "no single V row: %s, expected %s" % (got[b, q, h].tolist(), want[b, q, h].tolist())))


def explain_offset_channel(case, got, want):
    """For the first wrong dQ entry in an offset channel: the winners of that row with their dS and table rows, and the table-row shift
    that would explain the difference."""
    B, H, L, hd, Hp, Wp = case.B, case.H, case.L, case.hd, case.Hp, case.Wp
    offset = X.tie_layout(hd)[4]
    g, w = got.reshape(B * L, H, hd)[:, :, offset], want.reshape(B * L, H, hd)[:, :, offset]
    bad = (g != w).nonzero()
    if not len(bad):
        return ""
    r, h = (int(v) for v in bad[0])
    b, q = r // L, r % L
    alg = X.tie_algebra(case)
    ds = alg["dS"][b * H + h, q]
    lines = []
    for k in ds.nonzero().flatten().tolist():
        jh, jw = q // Wp - k // Wp + Hp - 1, q % Wp - k % Wp + Wp - 1
        d = float(g[r, h] - w[r, h]) / float(ds[k])
        lines.append("key %d (kh %d, kw %d): dS %g, rel_pos_h row %d, rel_pos_w row %d; alone it explains the difference with rows %g off"
                     % (k, k // Wp, k % Wp, float(ds[k]), jh, jw, d))
    return ("\n  offset channel %d, first wrong: sample %d head %d query %d (qh %d, qw %d): got %g, expected %g = sum dS (jh + jw + 2) over\n    "
            % (offset, b, h, q, q // Wp, q % Wp, float(g[r, h]), float(w[r, h])) + "\n    ".join(lines))


def explain_table(case, got, want):
    nh = 2 * case.Hp - 1
    bad = got != want
    j, c = (int(v) for v in bad.nonzero()[0])
    return ("drcat: %d of %d entries wrong; first: row %d of %s, channel %d: got %r, expected %r"
            % (int(bad.sum()), bad.numel(), j if j < nh else j - nh, "rel_pos_h" if j < nh else "rel_pos_w", c, float(got[j, c]), float(want[j, c])))


def check(route_spec, kind, grid, prep="fused"):
    tname, hd, _, family, _ = route_spec
    T = DTYPES[tname]
    case, exp = X.tie_attn_case(kind, *grid, hd)
    D, nrows = case.H * hd, exp.drcat.shape[0]
    (out, lse, dqkv, drcat), fam = run(case, T, prep)
    for k in ("fwd", "bwd"):
        assert fam[k][family] >= 1 and sum(fam[k]) == fam[k][family], (k, fam[k])
    assert out.dtype == T and dqkv.dtype == T and drcat.dtype == torch.float32
    for name, t in (("out", out), ("lse", lse), ("dqkv", dqkv), ("drcat", drcat)):
        assert bool(torch.isfinite(t.float()).all()), name
    # forward: exact quarters, bit for bit on every route and in both builds
    assert torch.equal(out.double(), exp.out), explain_out(case, exp, out)
    e_l = relerr(lse, exp.lse)
    assert e_l < LSE_GATE[tname], e_l
    got = dict(dq=dqkv[:, :D].double(), dk=dqkv[:, D:2 * D].double(), dv=dqkv[:, 2 * D:].double(), drcat=drcat[:nrows].double())
    assert float(drcat[nrows:].abs().max()) == 0.0 if drcat.shape[0] > nrows else True
    if tname == "bf16":
        for name in ("dq", "dk", "dv"):
            want = once_to_bf16(getattr(exp, name)).double()
            assert torch.equal(got[name], want), (explain_rows(case, name, got[name], want)
                                                  + (explain_offset_channel(case, got[name], want) if name == "dq" else ""))
        assert torch.equal(got["drcat"], exp.drcat), explain_table(case, got["drcat"], exp.drcat)
    else:
        assert float((lse.double() - exp.lse).abs().max()) <= 1e-6
        bound = X.tie_fp32_bounds(case, X.tie_algebra(case))
        worst = {}
        for name in ("dq", "dk", "dv", "drcat"):
            want = getattr(exp, name)
            err = (got[name] - want).abs()
            worst[name] = float((err / bound[name].clamp_min(1e-300)).max()) if float(err.max()) else 0.0
            ok = err <= bound[name]
            if name == "drcat":
                assert bool(ok.all()), explain_table(case, torch.where(ok, want, got[name]), want)
            else:
                assert bool(ok.all()), explain_rows(case, name + " (beyond its bound)", torch.where(ok, want, got[name]), want)
        print("fp32 %s %s hd%d: entries off the exact answer dq %d dk %d dv %d drcat %d; worst error / bound %s"
              % (kind, grid, hd, *(int((got[n] != getattr(exp, n)).sum()) for n in ("dq", "dk", "dv", "drcat")),
                 {n: "%.3f" % v for n, v in worst.items()}))
    # a second run gives the same bits
    again, _ = run(case, T, prep)
    for name, a, b in zip(("out", "lse", "dqkv", "drcat"), (out, lse, dqkv, drcat), again):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), name
    return out, lse, dqkv, drcat


def _id(p):
    return "%s-%s-%dx%dx%dx%d" % p


ROUTE_PARAMS = X.tie_route_params(X.ATTN_ROUTES)
SHORT_PARAMS = X.tie_route_params(X.SHORT_ROUTES)


@pytest.mark.parametrize("route,kind,B,H,Hp,Wp", ROUTE_PARAMS, ids=[_id(p) for p in ROUTE_PARAMS])
def test_tied_winners_give_the_exact_gradients(route, kind, B, H, Hp, Wp, generation):
    """Every route of ATTN_ROUTES (build, head dim, generation, grids; asserted with the launch counters) on the three placements of the
    tied keys -- neighbours, a quarter of the grid apart, mirrored -- with a dense and a sparse dO (exact_cases.tie_kinds).  On the full
    grid the last 32 query rows, the one live wave of the 13th workgroup, are tie rows like all others."""
    spec = X.ATTN_ROUTES[route]
    generation(spec[2])
    check(spec, kind, (B, H, Hp, Wp))


@pytest.mark.parametrize("kind,grid", X.TIE_PREP_LAUNCH_CASES, ids=["%s-%dx%dx%dx%d" % ((k,) + g) for k, g in X.TIE_PREP_LAUNCH_CASES])
def test_generation_3_backward_with_the_prep_launch_gives_the_same_exact_gradients(kind, grid, generation):
    """prep="launch" against the fused default: the same assertions on each, and out, lse, dqkv and drcat value for value the same.  Here
    Delta is a non-zero multiple of 1/4 that differs from row to row and -lse / scale one of three values: a prep kernel that wrote
    either into the wrong row's field, or split it differently, changes dS by at least 1/16 somewhere."""
    generation(0)
    spec = X.ATTN_ROUTES["bf16_hd64_gen3"]
    fused = check(spec, kind, grid)
    launch = check(spec, kind, grid, prep="launch")
    for name, a, b in zip(("out", "lse", "dqkv", "drcat"), fused, launch):
        assert torch.equal(a.float(), b.float()), (name, int((a.float() != b.float()).sum()))


@pytest.mark.parametrize("route,kind,B,H,Hp,Wp", SHORT_PARAMS, ids=[_id(p) for p in SHORT_PARAMS])
def test_tied_winners_on_the_shortest_generation_2_grids(route, kind, B, H, Hp, Wp, generation):
    """(4, 16) and (4, 24), head dim 64 and 80: two and three key tiles, so a mirrored or quarter-apart group has a member in every tile."""
    spec = X.SHORT_ROUTES[route]
    generation(spec[2])
    check(spec, kind, (B, H, Hp, Wp))



@pytest.mark.parametrize("hd,gen_,family,Hp,Wp", [(64, 0, 1, 8, 12), (64, 0, 2, 8, 28), (64, 2, 1, 8, 28), (80, 0, 1, 8, 12)],
                         ids=["gen2", "gen3", "gen2_forced", "gen2_hd80"])
def test_forward_with_a_first_key_tile_far_below_zero(hd, gen_, family, Hp, Wp, generation):
    """Found by the tie cases: the generation-2 and generation-3 forward kernels start their running maximum at 0 and re-base it in the
    first key tile by the tile's own maximum, rescaling l and O -- both still zero -- by exp2(-max).  A row whose first 32 logits all lie below
    -128 ln 2 = -88.7 made that factor inf and the row's out and lse NaN for good (attn2.hip:160-166, attn3.hip:159-165; the generic
    kernel starts at -inf and never had it).  Gaussian operands at test_attn_fwd's gates, with EVERY logit moved down by 200 through one
    channel of q and K: softmax does not change, lse drops by 200."""
    from tests.test_kernels_gpu import attn_reference, gen
    generation(gen_)
    B, H, L = 1, 2, Hp * Wp
    T = torch.bfloat16
    qkv = gen((B * L, 3 * H * hd), 1, 1.0, T).reshape(B * L, 3, H, hd).clone()
    qkv[:, 0, :, 5] = 40.0                            # q
    qkv[:, 1, :, 5] = -40.0                           # K: 0.125 * 40 * -40 = -200 on every logit
    qkv = qkv.reshape(B * L, 3 * H * hd)
    rel_h, rel_w = gen((2 * Hp - 1, hd), 2, 0.2), gen((2 * Wp - 1, hd), 3, 0.2)
    rel_h[:, 5], rel_w[:, 5] = 0.0, 0.0
    rcat = ops.relpos_pack(rel_h, rel_w, Hp, Wp, T)
    c0 = ops.attn_launch_counts()
    out, lse = ops.attn_fwd(qkv, rcat, B, L, H, Hp, Wp, 0.125)
    c1 = ops.attn_launch_counts()
    assert c1["fwd"][family] - c0["fwd"][family] == 1
    ref, lse_ref = attn_reference(qkv, rcat[: 2 * Hp - 1], rcat[2 * Hp - 1: 2 * Hp + 2 * Wp - 2], B, L, H, Hp, Wp, 0.125)
    assert float(lse_ref.max()) < -150
    assert bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(lse).all()), (int(torch.isnan(out.float()).sum()), int(torch.isnan(lse).sum()))
    assert relerr(lse, lse_ref) < 2e-3 and relerr(out.float(), ref) < 1.2e-2, (relerr(lse, lse_ref), relerr(out.float(), ref))
