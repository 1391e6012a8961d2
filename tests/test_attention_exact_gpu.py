"""Attention without a tolerance: softmax as an exact gather (tests/exact_cases.py), on every kernel route.

One key's logit exceeds every other key's by >= 150 in every query row (asserted for every case by tests/test_exact_cases_cpu.py), so
  * forward: the winner's tile re-bases the running maximum in every route (150 * log2(e) = 216 > the 2^6 re-base threshold of generations
    2 and 3), P = exp2(0) = 1 there and exp2(<= -216) = 0 everywhere else, whatever the tiles before it had accumulated is multiplied by
    exp2(-(216 - 64)) = 0, l = 1, and out[q] is the V row of key t(q) BIT FOR BIT -- torch.equal, no exception on any route;
  * backward: dP and Delta are integers fp32 holds exactly (also as the bf16 hi + lo pair generation 3 stores), so dP - Delta is exactly 0
    at the winner and P is exactly 0 elsewhere: dS, hence dQ, dK and the rel-pos table gradient, are EXACTLY zero (-0.0 accepted), finite;
  * dV = P^T dO is the integer scatter-add of dO rows wherever P is exactly one-hot in the backward too.

Where dV is NOT asserted bit for bit (the documented exception; equality holds everywhere else).  Every backward kernel recomputes
P = exp2(s * scale * log2e - lse * log2e) from the lse the forward stored in natural-log units:
    attn_fwd.hip:150   lse[(size_t)bh * L + q] = (m + __builtin_amdgcn_logf(lt)) * LN2_F;
    attn_bwd.hip:139   lse2 = lse[(size_t)bh * L + q] * LOG2E_F;
    attn2.hip:206 / :286 and attn3.hip:204 / :343 are the same two lines; attn3.hip:208-211 stores -lse / scale as bf16 hi + lo.
m * LN2_F * LOG2E_F is not m: two fp32 roundings and two rounded constants, at most 2^-22 of m together.  At the winner the exponent is
therefore not 0 but up to |logit| * log2e * 2^-22, and P = 1 +- |logit| * 2^-22 (dS is unharmed: P times an exact zero).
  * bf16 build, content cases (|logit| <= 800): |P - 1| <= 1.9e-4, far inside the half ulp of bf16 below 1 (2^-9 = 1.95e-3): P rounds to
    exactly 1 when it is packed for the dV MFMA.  dV IS asserted bit for bit.
  * bf16 build, bias_rank (|logit| up to 4.2e4, P = 1 +- 1e-2): equality cannot hold by construction.  dV against the fp64 reference (which
    is the scatter-add: fp64's softmax is one-hot to 1e-65) at the existing gate of the backward tests, 1.6e-2 of the largest entry.
    (Measured, profiles/exact_gather_gpu_tests.log: 332 of 100,352 dV entries differ at the full grid, rel-max 1.95e-3 -- one bf16 ulp of
    P; none at the smaller grids.)
  * fp32 build: P stays fp32, so dV[k] = sum over its queries of P_q dO_q differs from the integer by at most
    sum_q |dO_q| |logit_q| 2^-22 + A[k] N[k] 2^-24, with logit_q the query's own winning logit, A = the scatter-add of |dO| and N = the
    number of queries of key k (fp32 accumulation): exact_cases.dv_fp32_bound, asserted element by element against the int64 scatter-add.
    This is a tolerance of this file's own making, not one of the suite's gates.  It stays sharp enough to see one missing or doubled dO
    row (an error of 1): tests/test_exact_cases_cpu.py asserts that it is below 1/2 in every element of every case (largest: 0.23 where
    1568 queries meet in one key; 0.04 on bias_rank, where |logit| reaches 4e4 but at most 8 queries share a key).

What these tests cannot see: a one-hot softmax makes dS exactly zero and keeps the normaliser at 1.  tests/test_attention_ties_gpu.py
takes both from there -- tied winners, P = 1/n, a non-zero dyadic dS, dQ, dK and table gradients held to equality on the same routes;
unequal probabilities within a row and the rounding of a non-dyadic dS stay with the tolerance tests."""
import pytest
import torch

from tests import exact_cases as X

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from painter_amd import ops
    from painter_amd._lib import lib

DEV = "cuda"
DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}
LSE_GATE = {"bf16": 2e-3, "fp32": 1e-5}                  # test_attn_fwd's gates
DV_GATE_BF16 = 1.6e-2                                    # test_attn_bwd's gate


@pytest.fixture
def generation():
    """pa_attn_set_generation for the duration of one test (0 = default: generation 3 where it applies; 2 = never generation 3)."""
    def set_(g):
        assert lib.pa_attn_set_generation(g) == 0
    yield set_
    lib.pa_attn_set_generation(0)


def relerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def run(case, T, prep="fused"):
    """Forward + backward through the C ABI -> (out, lse, dqkv, drcat) on the host, and the kernel families the launch counters saw."""
    B, H, Hp, Wp, L = case.B, case.H, case.Hp, case.Wp, case.L
    qkv, dout = case.qkv.to(T).to(DEV), case.dout.to(T).to(DEV)
    rel_h, rel_w = case.rel_h.to(DEV), case.rel_w.to(DEV)
    rcat, rcatT = ops.relpos_pack(rel_h, rel_w, Hp, Wp, T), ops.relpos_pack_t(rel_h, rel_w, Hp, Wp, T)
    c0 = ops.attn_launch_counts()
    out, lse, tables = ops.attn_fwd(qkv, rcat, B, L, H, Hp, Wp, case.scale, need_tables=True)
    dqkv, dG = ops.attn_bwd_core(qkv, rcat, rcatT, out, dout, lse, B, L, H, Hp, Wp, case.scale, tables=tables, prep=prep)
    drcat = ops.attn_bwd_relpos(dG, qkv, rcat.shape[0], B, L, H, Hp, Wp)
    c1 = ops.attn_launch_counts()
    fam = {k: [c1[k][i] - c0[k][i] for i in range(3)] for k in ("fwd", "bwd")}
    return (out.cpu(), lse.cpu(), dqkv.cpu(), drcat.cpu()), fam


def explain_out(case, exp, out):
    """The count of wrong output rows and what arrived in the first one."""
    B, H, L, hd = case.B, case.H, case.L, case.hd
    got, want = out.float().reshape(B, L, H, hd), exp.out.reshape(B, L, H, hd)
    bad = (got != want).any(-1)
    b, q, h = (int(v) for v in bad.nonzero()[0])
    t = int(exp.target[b, h, q])
    arrived = X.decode_v_row(got[b, q, h])
    return ("%d of %d output rows wrong; first: sample %d head %d query %d (qh %d, qw %d) expects key %d (kh %d, kw %d), got %s"
            % (int(bad.sum()), B * L * H, b, h, q, q // case.Wp, q % case.Wp, t, t // case.Wp, t % case.Wp,
               ("the V row of key (kh %(kh)d, kw %(kw)d) of head %(head)d, sample %(sample)d" % arrived) if arrived
               else "no V row: %s" % got[b, q, h].tolist()))


def explain_rows(case, name, got, want):
    """The count of wrong entries of a [B*L, H*hd] gradient and the first one."""
    bad = got != want
    r, c = (int(v) for v in bad.nonzero()[0])
    return ("%s: %d of %d entries wrong; first: sample %d token %d head %d channel %d: got %r, expected %r"
            % (name, int(bad.sum()), bad.numel(), r // case.L, r % case.L, c // case.hd, c % case.hd, float(got[r, c]), float(want[r, c])))


def assert_exactly_zero(case, name, t):
    t = t.float()
    assert bool(torch.isfinite(t).all()), "%s is not finite (%d entries)" % (name, int((~torch.isfinite(t)).sum()))
    if name == "drcat":
        assert not bool((t != 0).any()), "drcat: %d non-zero entries; first at %s" % (int((t != 0).sum()), (t != 0).nonzero()[0].tolist())
    else:
        assert not bool((t != 0).any()), explain_rows(case, name, t, torch.zeros_like(t))       # -0.0 == 0


def check(route_spec, kind, grid, prep="fused"):
    tname, hd, _, family, _ = route_spec
    T = DTYPES[tname]
    case, exp = X.attn_case(kind, *grid, hd)
    D = case.H * hd
    (out, lse, dqkv, drcat), fam = run(case, T, prep)
    for k in ("fwd", "bwd"):
        assert fam[k][family] >= 1 and sum(fam[k]) == fam[k][family], (k, fam[k])
    assert out.dtype == T and dqkv.dtype == T
    # forward: the gathered V rows, bit for bit -- no exception on any route
    assert torch.equal(out.float(), exp.out), explain_out(case, exp, out)
    e_l = relerr(lse, exp.lse)
    assert e_l < LSE_GATE[tname], e_l
    # backward: dQ, dK and the table gradient exactly zero
    assert_exactly_zero(case, "dq", dqkv[:, :D])
    assert_exactly_zero(case, "dk", dqkv[:, D:2 * D])
    assert_exactly_zero(case, "drcat", drcat)
    dv = dqkv[:, 2 * D:].double()
    assert bool(torch.isfinite(dv).all())
    want = exp.dv.double()
    if tname == "bf16" and kind != "bias_rank":
        assert torch.equal(dv, want), explain_rows(case, "dv", dv, want)
    elif tname == "bf16":
        e_v = relerr(dv, want)
        print("dv %s %s: %d of %d entries differ from the scatter-add, rel-max %.2e" % (kind, grid, int((dv != want).sum()), dv.numel(), e_v))
        assert e_v < DV_GATE_BF16, e_v
    else:
        bound = X.dv_fp32_bound(case, exp)
        err = (dv - want).abs()
        print("dv %s %s: %d of %d entries differ from the scatter-add, worst error / bound %.3f"
              % (kind, grid, int((dv != want).sum()), dv.numel(), float((err / bound.clamp_min(1e-300)).max())))
        assert bool((err <= bound).all()), explain_rows(case, "dv (beyond its bound)", torch.where(err <= bound, want, dv), want)
    # a second run gives the same bits
    again, _ = run(case, T, prep)
    for name, a, b in zip(("out", "lse", "dqkv", "drcat"), (out, lse, dqkv, drcat), again):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), name
    return out, lse, dqkv, drcat


def _id(p):
    return "%s-%s-%dx%dx%dx%d" % p


ROUTE_PARAMS = X.route_params(X.ATTN_ROUTES)
SHORT_PARAMS = X.route_params(X.SHORT_ROUTES)


@pytest.mark.parametrize("route,kind,B,H,Hp,Wp", ROUTE_PARAMS, ids=[_id(p) for p in ROUTE_PARAMS])
def test_attention_is_an_exact_gather(route, kind, B, H, Hp, Wp, generation):
    """Every route (tests/exact_cases.py, ATTN_ROUTES: build, head dim, generation, grids) on the five target maps and on bias_rank; the
    route is asserted with the launch counters.  Equalities and the one documented exception: the module docstring."""
    spec = X.ATTN_ROUTES[route]
    generation(spec[2])
    check(spec, kind, (B, H, Hp, Wp))


@pytest.mark.parametrize("kind,grid", X.PREP_LAUNCH_CASES, ids=["%s-%dx%dx%dx%d" % ((k,) + g) for k, g in X.PREP_LAUNCH_CASES])
def test_generation_3_backward_with_the_prep_launch_is_the_same_exact_result(kind, grid, generation):
    """prep="launch" (pa_attn_bwd_prep writes Delta and the lse fields into the table tiles in front of the backward) against the fused
    default on one grid (and bias_rank on the full grid too): the same assertions on each route, and ALL of out, lse, dqkv (dV included, on every kind) and drcat the same
    between the two -- value for value, which for floats is bit for bit apart from the sign of a zero.  Both routes write -lse / scale as
    the same bf16 hi + lo pair from the same stored lse (attn3.hip:208-211 and the prep kernel), and Delta is an integer here, so its
    summation order does not matter.  bias_rank is the sensitive case: with |lse / scale| up to 3.4e5 the lo half of the lse field decides
    the bf16 bits of P, and with them dV (at the full grid some of them are not the bits of 1); on the content cases P rounds to 1 and a
    wrong lo half would hide."""
    generation(0)
    spec = X.ATTN_ROUTES["bf16_hd64_gen3"]
    fused = check(spec, kind, grid)
    launch = check(spec, kind, grid, prep="launch")
    for name, a, b in zip(("out", "lse", "dqkv", "drcat"), fused, launch):
        assert torch.equal(a.float(), b.float()), (name, int((a.float() != b.float()).sum()))


@pytest.mark.parametrize("route,kind,B,H,Hp,Wp", SHORT_PARAMS, ids=[_id(p) for p in SHORT_PARAMS])
def test_attention_is_an_exact_gather_on_the_shortest_generation_2_grids(route, kind, B, H, Hp, Wp, generation):
    """(4, 16) and (4, 24): L = 64 and L = 96, two and three key tiles, half of the workgroup's waves without a query tile; head dim 64 and
    80.  The shortest grids that reach the generation-2 kernels: attn2_ok (attn2.hip:576) alone would also admit (2, 16), but pa_attn_fwd /
    pa_attn_bwd return an error for Hp % 4 != 0 before they dispatch.  New to the suite; kept apart and run after the rest."""
    spec = X.SHORT_ROUTES[route]
    generation(spec[2])
    check(spec, kind, (B, H, Hp, Wp))
