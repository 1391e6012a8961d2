"""The conditions tests/test_attention_exact_gpu.py and tests/test_conv3x3_exact_gpu.py rest on, asserted on the CPU for every case those
files build (the parametrisations are shared through tests/exact_cases.py); and for tests/test_attention_any_exact_gpu.py, together with
the named wrong forwards its cases must see."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import exact_cases as X

ATTN_SHAPES = X.attn_shapes()
CONV_SHAPES = [(kind,) + X.CONV_ROUTES[route][1] for route in X.CONV_ROUTES for kind in X.CONV_KINDS]


def bf16_exact_integers(t):
    return bool((t == t.round()).all()) and torch.equal(t.to(torch.bfloat16).float(), t.float())


def test_the_gpu_parametrisation_covers_what_it_says():
    """Every route runs all five target maps and bias_rank; the full-size grid runs reversal, both fan-in maps and bias_rank; the short
    grids are in a parametrisation of their own."""
    params = X.route_params(X.ATTN_ROUTES)
    for route, spec in X.ATTN_ROUTES.items():
        for grid in spec[4]:
            kinds = {p[1] for p in params if p[0] == route and p[2:] == grid}
            assert kinds == set(X.FULL_GRID_KINDS if grid == X.FULL_GRID else X.ATTN_KINDS), (route, grid)
    assert X.FULL_GRID[2] * X.FULL_GRID[3] == 1568 and X.FULL_GRID[:2] == (1, 1)
    assert not {p[2:] for p in params} & set(X.SHORT_GRIDS)
    assert {p[2:] for p in X.route_params(X.SHORT_ROUTES)} == set(X.SHORT_GRIDS)
    assert max(B * H * Hp * Wp for _, _, B, H, Hp, Wp in params) == 4 * 16 * 28 and len(ATTN_SHAPES) == len(set(ATTN_SHAPES))


@pytest.mark.parametrize("kind,B,H,Hp,Wp,hd", ATTN_SHAPES, ids=["%s-%dx%dx%dx%d-hd%d" % s for s in ATTN_SHAPES])
def test_attention_case_margins_and_integer_bounds(kind, B, H, Hp, Wp, hd):
    case, exp = X.attn_case(kind, B, H, Hp, Wp, hd)
    L = Hp * Wp
    # every row, none excluded: the winner leads by >= 150, so exp() of every other term is zero in fp32
    assert exp.margin.shape == (B, H, L) and float(exp.margin.min()) >= X.MIN_MARGIN, float(exp.margin.min())
    print("%s B%d H%d %dx%d hd%d: margin >= %.0f over all %d rows (0 excluded), largest logit %.0f, largest |dV| %d"
          % (kind, B, H, Hp, Wp, hd, float(exp.margin.min()), exp.margin.numel(), float(exp.top.max()), int(exp.dv.abs().max())))
    # the argmax of the fp64 logits is the map the builder meant
    if kind != "bias_rank":
        g = torch.Generator().manual_seed(0)
        if kind != "permutation":
            assert torch.equal(exp.target, X._target_map(kind, B, H, L, g))
        else:
            assert all(torch.equal(exp.target[b, h].sort().values, torch.arange(L)) for b in range(B) for h in range(H))
            assert not torch.equal(exp.target[0, 0], exp.target[-1, -1])              # another permutation per (sample, head)
        assert float(exp.top.min()) >= 384 and case.rel_h.abs().max() == 0 and case.rel_w.abs().max() == 0
    # fp64's lse is the winning logit (the other terms vanish below fp64's epsilon as well)
    assert torch.equal(exp.lse.reshape(B, H, L), exp.top)
    # operands: integers that survive bf16; scale a power of two
    for name in ("qkv", "rel_h", "rel_w", "dout"):
        assert bf16_exact_integers(getattr(case, name)), name
    assert case.scale == 0.125 and set(case.dout.unique().tolist()) <= {-1.0, 0.0, 1.0}
    v = case.qkv.reshape(B, L, 3, H, hd)[:, :, 2]
    assert 1 <= float(v.abs().min()) and float(v.abs().max()) <= 64
    # every logit, dP and Delta is an integer below 2^24 (Delta below 2^16: exact as a bf16 hi + lo pair); -lse / scale a multiple of 2^11
    # below 2^19 on bias_rank
    assert torch.equal(exp.top, exp.top.round()) and float(exp.top.abs().max()) < 2 ** 24
    assert hd * 64 < 2 ** 16
    if kind == "bias_rank":
        assert bool(((exp.top / case.scale) % 2048 == 0).all()) and float(exp.top.max() / case.scale) < 2 ** 19
    # expected outputs: bf16 holds every one (|.| <= 256), fp32 too (< 2^24)
    assert bf16_exact_integers(exp.out) and float(exp.out.abs().max()) <= 256
    assert int(exp.dv.abs().max()) <= 256 and bf16_exact_integers(exp.dv.float())
    # the fp32 build's dV bound never reaches 1/2: one missing or doubled dO row (an error of 1) cannot hide inside it
    assert float(X.dv_fp32_bound(case, exp).max()) < 0.5
    # position code: every (sample, head, key) row of V decodes to itself
    for b, k, h in ((0, 0, 0), (B - 1, L - 1, H - 1), (B - 1, L // 2 + 1, 0)):
        assert X.decode_v_row(v[b, k, h]) == dict(kh=k // Wp, kw=k % Wp, head=h, sample=b)
    assert X.decode_v_row(0.5 * v[0, 0, 0]) is None and X.decode_v_row(v[0, 0, 0].roll(1)) is None and X.decode_v_row(torch.zeros(hd)) is None


@pytest.mark.parametrize("kind,B,H,Hp,Wp,hd", [s for s in ATTN_SHAPES if s[0] == "bias_rank"],
                         ids=["%dx%dx%dx%d-hd%d" % s[1:] for s in ATTN_SHAPES if s[0] == "bias_rank"])
def test_bias_rank_tables_decide_alone(kind, B, H, Hp, Wp, hd):
    """logit(q, k) = 256 * (w_h(qh - kh + Hp - 1) + w_w(qw - kw + Wp - 1)); the winner of query (qh, qw) is the key at the best reachable
    row offset and the best reachable column offset, the runner-up differs from it in exactly one of the two.

    `Each table row is the winner of at least one query` would be the stronger statement.  No table can meet it: the queries of one query row share one
    window of Hp consecutive rows of the 2 Hp - 1 row table, so at most Hp table rows ever win (Wp of 2 Wp - 1), and counting runners-up
    as well at most 2 Hp.  What holds, and what the exactness needs, is asserted instead: every table row is REACHABLE by some query and
    is therefore a competitor there -- read in place of the winner's row it changes that query's logit by a multiple of 256, at least 256
    -- and the rows that do win are exactly the sliding-window maxima of the seeded permutations."""
    case, exp = X.attn_case(kind, B, H, Hp, Wp, hd)
    L = Hp * Wp
    wh, ww = case.rel_h[:, 0].long(), case.rel_w[:, 0].long()
    assert torch.equal(wh.sort().values, torch.arange(2 * Hp - 1)) and torch.equal(ww.sort().values, torch.arange(2 * Wp - 1))
    assert float(case.rel_h[:, 32:].abs().max()) == 0 and float(case.rel_w[:, 32:].abs().max()) == 0
    q = torch.arange(L)
    qh, qw = q // Wp, q % Wp
    best_kh = torch.stack([(wh[h + Hp - 1 - torch.arange(Hp)]).argmax() for h in range(Hp)])       # per query row: kh of the best offset
    best_kw = torch.stack([(ww[w + Wp - 1 - torch.arange(Wp)]).argmax() for w in range(Wp)])
    want = best_kh[qh] * Wp + best_kw[qw]
    assert torch.equal(exp.target, want[None, None].expand(B, H, L))
    th, tw = exp.target // Wp, exp.target % Wp
    rh, rw = exp.runner_up // Wp, exp.runner_up % Wp
    assert bool(((th == rh) ^ (tw == rw)).all())
    assert bool((exp.margin % 256 == 0).all()) and float(exp.margin.min()) >= 256
    # every table row is reachable (offset qh - kh + Hp - 1 over the grid), and the winning rows are the window maxima
    reach_h = {int(a - b + Hp - 1) for a in range(Hp) for b in range(Hp)}
    reach_w = {int(a - b + Wp - 1) for a in range(Wp) for b in range(Wp)}
    assert reach_h == set(range(2 * Hp - 1)) and reach_w == set(range(2 * Wp - 1))
    win_h = {int(v) for v in (qh[None, None] - th + Hp - 1).unique()}
    win_w = {int(v) for v in (qw[None, None] - tw + Wp - 1).unique()}
    assert win_h == {int(wh[h:h + Hp].argmax()) + h for h in range(Hp)} and win_w == {int(ww[w:w + Wp].argmax()) + w for w in range(Wp)}
    assert 1 <= len(win_h) <= Hp and 1 <= len(win_w) <= Wp
    print("bias_rank %dx%d: %d of %d rel_pos_h rows and %d of %d rel_pos_w rows win a query" % (Hp, Wp, len(win_h), 2 * Hp - 1, len(win_w), 2 * Wp - 1))


@pytest.mark.parametrize("kind,B,Hi,Wi", CONV_SHAPES, ids=["%s-%dx%dx%d" % s for s in CONV_SHAPES])
def test_conv_case_references_equal_torch_conv_and_stay_exact(kind, B, Hi, Wi):
    case, exp = X.conv_case(kind, B, Hi, Wi)
    nchw = lambda t: t.double().permute(0, 3, 1, 2)
    y = F.conv2d(nchw(case.x), case.w3.double(), case.b3.double(), padding=1)
    dx = F.conv_transpose2d(nchw(case.dy), case.w3.double(), padding=1)
    dw = torch.nn.grad.conv2d_weight(nchw(case.x), case.w3.shape, nchw(case.dy_w), padding=1)
    assert torch.equal(nchw(exp.y3), y) and torch.equal(nchw(exp.dx), dx) and torch.equal(exp.dw.double(), dw)
    for name in ("x", "dy", "dy_w", "w3", "b3"):
        assert bf16_exact_integers(getattr(case, name)), name
    assert int(exp.y3.abs().max()) <= 256 and int(exp.dx.abs().max()) <= 256 and int(exp.dw.abs().max()) < 2 ** 24
    assert bf16_exact_integers(exp.y3.float()) and bf16_exact_integers(exp.dx.float())
    assert float(case.b3.abs().max()) <= 8
    P = [spec[2] for spec in X.CONV_ROUTES.values() if spec[1] == (B, Hi, Wi)][0]
    tok = X.unshuffle(exp.dx, B, Hi // P, Wi // P, P)
    assert tok.shape == (B * (Hi // P) * (Wi // P), P * P * 64) and tok[1, 64 + 3] == exp.dx[0, 0, P + 1, 3]      # token 1 = patch (0, 1), pixel (0, 1)
    if kind == "int":
        assert set(case.x.unique().tolist()) == {-1.0, 0.0, 1.0} and abs(float((case.x != 0).float().mean()) - 1 / 3) < 0.02
        assert abs(float((case.dy != 0).float().mean()) - 1 / 3) < 0.02 and set(case.w3.unique().tolist()) == {-1.0, 0.0, 1.0}
        assert int(exp.dw.abs().max()) > 0
        return
    # stamp: the pixels the issue names, one channel each, stamps that do not overlap
    px = {(b, r, c) for b, r, c, _ in case.hot}
    assert {(0, 0, 0), (0, 0, Wi - 1), (0, Hi - 1, 0), (0, Hi - 1, Wi - 1), (0, 0, Wi // 2), (0, Hi - 1, Wi // 2), (0, Hi // 2, 0),
            (0, Hi // 2, Wi - 1), (1, 0, 0)} <= px
    assert {1, 2, 3, 4} <= {r for _, r, _ in px} and ((Wi <= 64) or {63, 64} <= {c for _, _, c in px})
    assert len({ch for *_, ch in case.hot}) == len(case.hot) and int(case.x.sum()) == len(case.hot) == int(case.dy_w.sum())
    assert float(case.w3.abs().max()) <= 81 and float(case.w3.abs().min()) >= 1
    w3, b3 = case.w3.long(), case.b3.long()
    stamped = torch.zeros(B, Hi, Wi, dtype=torch.bool)
    for b, r, c, ch in case.hot:
        for ky in range(3):
            for kx in range(3):
                h, w = r + 1 - ky, c + 1 - kx                      # the output pixel that sees the hot pixel through tap (ky, kx)
                if 0 <= h < Hi and 0 <= w < Wi:
                    assert torch.equal(exp.y3[b, h, w], w3[:, ch, ky, kx] + b3) and not stamped[b, h, w]
                    stamped[b, h, w] = True
                    assert X.decode_stamp(float(w3[5, ch, ky, kx])) == dict(ky=ky, kx=kx, ci_mod_8=ch % 8)
                h, w = r - 1 + ky, c - 1 + kx                      # data gradient: the un-flipped kernel, the input channels of output channel ch
                if 0 <= h < Hi and 0 <= w < Wi:
                    assert torch.equal(exp.dx[b, h, w], w3[ch, :, ky, kx])
    assert torch.equal(exp.y3[~stamped], b3.expand(int((~stamped).sum()), 64)) and int(exp.dx[~stamped].abs().max()) == 0
    # weight gradient: a count of coincidences one tap apart, among them pairs across rows 1 | 2 and 3 | 4 and columns 63 | 64; the hot first
    # pixel of sample 1 and the hot last pixel of sample 0 are no neighbours
    assert int(exp.dw.min()) == 0 and int(exp.dw.sum()) >= len(case.hot) and int(exp.dw.max()) <= 2
    hx, hy = case.x.sum(-1), case.dy_w.sum(-1)
    near = lambda a, b_, axis: bool(((hx.select(axis, a) > 0).any(1) & (hy.select(axis, b_) > 0).any(1)).any())     # same sample: x hot in row / col a, dy in b_
    assert near(1, 2, 1) and near(2, 1, 1) and near(3, 4, 1) and near(4, 3, 1)
    if Wi > 64:
        assert near(63, 64, 2) and near(64, 63, 2)
    assert hx[0, Hi - 1, Wi - 1] == 1 and hy[1, 0, 0] + hy[1, 0, 1] + hy[1, 1, 0] + hy[1, 1, 1] >= 1


# ------------------------------------------------------------------------------------------------ tied winners
TIE_SHAPES = X.tie_shapes()
OLD_GATE_BF16 = 1.6e-2                                  # test_attn_bwd's: max|a - b| / max|b| over the whole tensor


def bf16_exact(t):
    return torch.equal(t.float().to(torch.bfloat16).double(), t.double())


def bf16_hi_lo_exact(t):
    hi = t.float().to(torch.bfloat16).float()
    lo = (t.float() - hi).to(torch.bfloat16).float()
    return torch.equal((hi.double() + lo.double()), t.double())


def test_the_tie_parametrisation_covers_what_it_says():
    """Every route and grid of the gather tests runs the three placements; with a dense and a sparse dO on the head-dim-64 grids below the
    full one, with the sparse one elsewhere; the full grid once per placement; the prep-launch route all six kinds and the full grid."""
    assert X.TIE_KINDS == ("tie_near", "tie_quarter", "tie_mirror", "tie_near_sparse", "tie_quarter_sparse", "tie_mirror_sparse")
    for routes in (X.ATTN_ROUTES, X.SHORT_ROUTES):
        params = X.tie_route_params(routes)
        assert {p[0] for p in params} == set(routes)
        for route, spec in routes.items():
            for grid in spec[4]:
                kinds = [p[1] for p in params if p[0] == route and p[2:] == grid]
                assert {k.replace("tie_", "").replace("_sparse", "") for k in kinds} == set(X.TIE_PLACEMENTS), (route, grid)
                assert len(kinds) == (6 if spec[1] == 64 and grid != X.FULL_GRID else 3) and len(set(kinds)) == len(kinds)
    assert [g for _, g in X.TIE_PREP_LAUNCH_CASES] == [X.PREP_LAUNCH_GRID] * 6 + [X.FULL_GRID]
    assert len(TIE_SHAPES) == len(set(TIE_SHAPES))


@pytest.mark.parametrize("kind,B,H,Hp,Wp,hd", TIE_SHAPES, ids=["%s-%dx%dx%dx%d-hd%d" % s for s in TIE_SHAPES])
def test_tie_case_conditions_and_sensitivity(kind, B, H, Hp, Wp, hd):
    """What tests/test_attention_ties_gpu.py rests on, for every case it builds.

    Sensitivity: five wrong backward kernels (exact_cases.tie_algebra) each move at least one tensor by many quanta (148 at the least),
    far outside the fp32 build's bound (46,000 times it at the least, taken at the element the fault moves most and only where the
    bound is not 0; for the faults that touch the tables, on the tables).  NONE of them stays inside the gate of the tolerance tests (max|a - b| / max|b| < 1.6e-2) on these cases: the smallest
    measure over all cases is 0.11 (last_key_row), and on Gaussian operands of test_attn_bwd's kind they are gross
    as well (0.35 and more) -- each of the five is wrong in every row.  The faults the tolerance tests cannot see are the local ones (one
    row, one slot, one column of one workgroup); here those are visible for another reason, asserted below: every value is exact, so
    any single wrong contribution is at least one quantum."""
    case, exp = X.tie_attn_case(kind, B, H, Hp, Wp, hd)
    alg = X.tie_algebra(case)
    L, D, nh = Hp * Wp, H * hd, 2 * Hp - 1
    active, s1, s2, shift, offset = X.tie_layout(hd)
    assert len(set(active + s1 + s2 + shift + [offset])) == hd
    # winners: 1, 2 or 4 per row at logit exactly 0, all three counts, the pattern the builder meant (the last rows of the grid are tie rows);
    # everyone else >= 150 below
    assert torch.equal(exp.nwin, X.tie_winner_count(L)[None, None].expand(B, H, L)) and set(exp.nwin.unique().tolist()) == {1, 2, 4}
    assert int(exp.nwin[0, 0, L - 1]) == 4 and int(exp.nwin[0, 0, L - 3]) == 2 and float(exp.loser) <= -X.MIN_MARGIN
    for tile in range(L // 32):
        assert set(exp.nwin[0, 0, 32 * tile:32 * tile + 32].tolist()) == {1, 2, 4}
    logits = alg["logits"]
    assert float(logits.max()) == 0 and torch.equal((logits == 0).sum(-1).reshape(B, H, L), exp.nwin)
    members = X.tie_members(kind.split("_")[1], L)
    assert torch.equal(members.flatten().sort().values, torch.arange(L))
    win = (logits.reshape(B, H, L, L) == 0)
    for n, want in ((4, (4,)), (2, (2,))):                # the winners of a row are members of ONE group: all four, or a member and its partner m ^ 2
        rows = win[0, 0][exp.nwin[0, 0] == n]
        in_group = rows[:, members].sum(-1)                # [rows, L/4]
        assert bool((in_group.max(-1).values == n).all())
        if n == 2:
            pair = rows[:, members][in_group == 2]         # [rows, 4]
            assert bool((pair[:, 0] == pair[:, 2]).all() and (pair[:, 1] == pair[:, 3]).all())
    t = win.float().argmax(-1)
    assert not torch.equal(t[0, 0], t[-1, -1]) or B * H == 1                      # another target permutation per (sample, head)
    # operands are bf16-exact; so are scale * q and the per-query bias tables, which are zero (q is zero where the tables are not)
    for name in ("qkv", "rel_h", "rel_w", "dout"):
        assert bf16_exact_integers(getattr(case, name)), name
    q = case.qkv.reshape(B, L, 3, H, hd)[:, :, 0]
    assert bf16_exact(q * case.scale) and case.scale == 0.125
    assert float(alg["Gh"].abs().max()) == 0 and float(alg["Gw"].abs().max()) == 0
    assert float(case.rel_h.abs().sum()) == float(case.rel_h[:, offset].sum()) == nh * (nh + 1) / 2
    assert float(case.rel_w.abs().sum()) == float(case.rel_w[:, offset].sum()) == Wp * (2 * Wp - 1)
    assert set(case.dout.unique().tolist()) == {-1.0, 0.0, 1.0}
    density = float((case.dout != 0).float().mean())
    assert abs(density - (1 / 16 if kind.endswith("sparse") else 2 / 3)) < 0.02
    # every fp32 accumulation is exact: sum of |terms| in units of 1/64 (the finest any term has) below 2^24
    sums = X.tie_exact_sums(case, alg)
    assert max(sums.values()) < 2 ** 24, sums
    assert bool((alg["dS"] * 16 == (alg["dS"] * 16).round()).all()) and bool((alg["P"] * 4 == (alg["P"] * 4).round()).all())
    # what the bf16 kernels pack into 16 bits: out, P, dS and the per-query bias gradient survive bf16; Delta and -lse / scale a hi + lo pair
    for name in ("out", "P", "dS", "dG_h", "dG_w"):
        assert bf16_exact(alg[name]), (name, int((alg[name].float().to(torch.bfloat16).double() != alg[name]).sum()))
    assert bf16_hi_lo_exact(alg["delta"])
    x = -exp.lse.float() / case.scale                     # the fp32 value the forward splits (lse itself is log 1, log 2 or log 4 rounded to fp32)
    hi = x.to(torch.bfloat16).float()
    back = (hi + (x - hi).to(torch.bfloat16).float()).double() * case.scale
    assert float((torch.exp(-exp.lse.float().double() - back) - 1).abs().max()) < 2.0 ** -11
    assert torch.equal(exp.lse, torch.log(exp.nwin.double()).reshape(B * H, L))
    # expectations: autograd == the hand algebra, dyadic (times 32 an integer), non-zero where the issue says
    for name, a, b in (("out", exp.out, alg["out"]), ("dq", exp.dq, alg["dq"]), ("dk", exp.dk, alg["dk"]), ("dv", exp.dv, alg["dv"]),
                       ("drh", exp.drcat[:nh], alg["drh"]), ("drw", exp.drcat[nh:], alg["drw"])):
        assert float((a - b).abs().max()) < 1e-9 and float((a * 32 - (a * 32).round()).abs().max()) < 1e-9, name
        assert float(a.abs().max()) < 2 ** 15
    # (dQ of a tie row is zero on the channels its winners share: sum_k dS = 0.  The flip sets and the offset channel carry it.)
    off_dq = exp.dq.reshape(B * L, H, hd)[:, :, offset]
    assert bf16_exact(exp.out) and float((exp.dq != 0).double().mean()) > 0.02 and float((off_dq != 0).double().mean()) > 0.3
    assert float((exp.dk != 0).double().mean()) > 0.4
    assert float((exp.drcat[:nh].abs().sum(1) != 0).double().mean()) > 0.5
    if "quarter" not in kind:                             # a quarter of the grid apart is a whole number of key rows: the same key column, no rel_pos_w gradient
        assert float((exp.drcat[nh:].abs().sum(1) != 0).double().mean()) > 0.5
    # the fp32 build's bound: below half a quantum in every element of dq, dk, dv and both table gradients (largest: 0.05 of a quantum for
    # dq, 0.32 for a table row), so no value one quantum off can hide inside it
    bound = X.tie_fp32_bounds(case, alg)
    quanta = {n: X.tie_quantum(getattr(exp, n)) for n in ("dq", "dk", "dv", "drcat")}
    ratio = {n: float(bound[n].max()) / quanta[n] for n in bound}
    print("%s %dx%dx%dx%d hd%d: quanta %s; fp32 bound / quantum %s" % (kind, B, H, Hp, Wp, hd, quanta, {n: "%.3f" % r for n, r in ratio.items()}))
    assert min(quanta.values()) >= 1 / 32
    assert max(ratio.values()) < 0.5, ratio
    # sensitivity
    want = dict(dq=alg["dq"], dk=alg["dk"], dv=alg["dv"], drcat=torch.cat([alg["drh"], alg["drw"]], 0))
    line = []
    for fault in X.TIE_FAULTS:
        w = X.tie_algebra(case, fault)
        got = dict(dq=w["dq"], dk=w["dk"], dv=w["dv"], drcat=torch.cat([w["drh"], w["drw"]], 0))
        diff = {n: (got[n] - want[n]).abs() for n in want}
        seen = {n: float(diff[n].max()) / quanta[n] for n in want}
        # ... against the bound only where there is one: where it is 0 every term is 0 and the fp32 build has to return 0 itself
        # ... and at the element the fault moves most, not at one whose bound happens to be tiny
        at = {n: int((diff[n] * (bound[n] > 0)).argmax()) for n in want}
        beyond = {n: float(diff[n].flatten()[at[n]] / bound[n].flatten()[at[n]].clamp_min(1e-300)) for n in want}
        measure = max(float(diff[n].max() / want[n].abs().max().clamp_min(1e-30)) for n in ("dq", "dk", "dv"))
        measure = max(measure, float(diff["drcat"][:nh].max() / want["drcat"][:nh].abs().max().clamp_min(1e-30)),
                      float(diff["drcat"][nh:].max() / want["drcat"][nh:].abs().max().clamp_min(1e-30)) if float(want["drcat"][nh:].abs().max()) else 0.0)
        tables_only = fault in ("last_key_row", "dg_column_dropped")           # these two change nothing but d rel_pos_h
        far = beyond["drcat"] if tables_only or fault == "kh_class_phase" else max(beyond.values())
        line.append("%s: %.0f quanta, %.0f x the fp32 bound, old measure %.2g" % (fault, max(seen.values()), far, measure))
        assert max(seen.values()) >= 1, (fault, seen)
        assert far >= 16, (fault, beyond)
        assert not tables_only or max(seen[n] for n in ("dq", "dk", "dv")) == 0
    print("  " + "; ".join(line))


# ------------------------------------------------------------------------------------------------ attention on any token grid
ANY_SHAPES = X.any_shapes()
_ANY_IDS = ["%s-%dx%dx%dx%d-hd%d" % s for s in ANY_SHAPES]


def test_the_any_grid_parametrisation_covers_what_it_says():
    """Four routes (bf16 / fp32, head dim 64 / 80) on the any-grid launch counter; the six gather kinds and below_zero on every ragged and
    every aligned grid, the six tie kinds wherever L % 4 == 0 and on the two tie grids, bias_rank alone at 62 x 31; head dim 80 up to
    L = 200.  70 x 35 is not here: position_coded_v holds Hp, Wp <= 63, and that grid stays with the tolerance test."""
    params = X.any_route_params()
    assert set(X.ANY_ROUTES) == {"any_%s_hd%d" % (t, hd) for t in ("bf16", "fp32") for hd in (64, 80)}
    ragged = {(2, 2, 2, 1), (2, 2, 6, 3), (2, 2, 11, 2), (1, 2, 3, 11), (2, 2, 9, 7), (2, 2, 10, 5), (2, 2, 5, 13), (2, 2, 4, 33),
              (2, 2, 12, 6), (1, 1, 35, 17)}
    assert set(X.ANY_RAGGED) == ragged and X.ANY_BIAS_ONLY == (1, 1, 62, 31) and X.ANY_ALIGNED == [(2, 2, 8, 4), (2, 2, 8, 28)]
    assert X.ANY_TIE_ONLY == [(2, 2, 10, 6), (2, 2, 12, 3)]
    for route, (tname, hd, counter, grids) in X.ANY_ROUTES.items():
        assert counter == "pa_attn_any_launches" and route == "any_%s_hd%d" % (tname, hd)
        every = X.ANY_RAGGED + [X.ANY_BIAS_ONLY] + X.ANY_ALIGNED + X.ANY_TIE_ONLY
        assert grids == [g for g in every if hd == 64 or g[2] * g[3] <= 200]
        assert hd == 64 or {g for g in every if g not in grids} == {(1, 1, 35, 17), (1, 1, 62, 31), (2, 2, 8, 28)}
        for grid in grids:
            kinds = [p[1] for p in params if p[0] == route and p[2:] == grid]
            assert len(kinds) == len(set(kinds))
            L = grid[2] * grid[3]
            if grid == X.ANY_BIAS_ONLY:
                assert kinds == ["bias_rank"]
            elif grid in X.ANY_TIE_ONLY:
                assert set(kinds) == set(X.TIE_KINDS) and L % 4 == 0 and L % 32 != 0
            else:
                assert set(kinds) == set(X.ATTN_KINDS) | {"below_zero"} | (set(X.TIE_KINDS) if L % 4 == 0 else set())
    tie_grids = {p[2:] for p in params if p[1] in X.TIE_KINDS}
    assert {(2, 2, 12, 6), (2, 2, 4, 33), (2, 2, 8, 4), (2, 2, 10, 6), (2, 2, 12, 3)} <= tie_grids
    assert not any(ops_takes(g) for g in X.ANY_RAGGED + [X.ANY_BIAS_ONLY] + X.ANY_TIE_ONLY) and all(ops_takes(g) for g in X.ANY_ALIGNED)
    assert max(B * H * Hp * Wp for _, _, B, H, Hp, Wp in params) == 1922 and len(ANY_SHAPES) == len(set(ANY_SHAPES))


def ops_takes(grid):
    """pa_attn_fwd's shape conditions (include/painter_hip.h), restated without importing the library."""
    _, _, Hp, Wp = grid
    return Hp * Wp % 32 == 0 and Hp % 4 == 0 and Wp % 4 == 0


@pytest.mark.parametrize("Hp,Wp", sorted({s[3:5] for s in ANY_SHAPES}), ids=lambda v: str(v))
def test_any_key_walk_without_a_fault_is_row_major(Hp, Wp):
    """The walk of attn_any.hip restated (exact_cases.any_key_walk) visits key k at (k // Wp, k % Wp); keys >= L clamp to the last row."""
    L = Hp * Wp
    kh, kw, zero = X.any_key_walk(L, Hp, Wp)
    k = torch.arange(kh.numel())
    assert kh.numel() == (L + 31) // 32 * 32 and not bool(zero.any())
    assert torch.equal(kh, (k // Wp).clamp_max(Hp - 1)) and torch.equal(kw, k % Wp)
    # each walk fault moves some key < L exactly where its name says, or the grid has no such key
    crossing = (k // Wp != (k - k % 4) // Wp) & (k < L)                     # keys behind a row crossing inside their 4-key run
    fh, _, _ = X.any_key_walk(L, Hp, Wp, "row_of_first_key")
    assert torch.equal((fh != kh) & (k < L), crossing) and torch.equal(fh[crossing], ((k - k % 4) // Wp)[crossing])
    _, fw, fz = X.any_key_walk(L, Hp, Wp, "column_wrap_zero")
    assert torch.equal(fz & (k < L), crossing) and torch.equal(fw, kw)
    ch, cw, _ = X.any_key_walk(L, Hp, Wp, "carry_lost")
    assert torch.equal(cw, kw) and bool((ch <= kh).all()) and torch.equal(ch[:32], kh[:32])
    if 32 % Wp == 0 or L <= 32:                                              # no wrap ever, or no second tile: nothing to lose
        assert torch.equal(ch, kh)


@functools.lru_cache(maxsize=None)
def any_fault_rows(kind, B, H, Hp, Wp, hd):
    """-> (quantum of the expected out, {fault: number of (token, head) output rows the wrong forward moves by at least one quantum})."""
    case, exp = X.any_case(kind, B, H, Hp, Wp, hd)
    want = exp.out.double()
    quantum = X.tie_quantum(want)
    rows = {}
    for fault in X.ANY_FAULTS:
        got = X.any_algebra(case, fault)["out"]
        diff = torch.nan_to_num((got - want).abs(), nan=float("inf"))        # 0 / 0 of a row without keys counts as wrong
        rows[fault] = int((diff.reshape(B * Hp * Wp, H, hd).max(-1).values >= quantum).sum())
    return quantum, rows


@pytest.mark.parametrize("kind,B,H,Hp,Wp,hd", ANY_SHAPES, ids=_ANY_IDS)
def test_any_grid_case_conditions(kind, B, H, Hp, Wp, hd):
    """What tests/test_attention_any_exact_gpu.py rests on, for every case it builds: the margin, integer operands that bf16 holds, an
    expected out that bf16 holds, and -- the forward algebra over the kernel's own key walk gives the expectation bit for bit."""
    case, exp = X.any_case(kind, B, H, Hp, Wp, hd)
    L = Hp * Wp
    alg = X.any_algebra(case)
    for name in ("qkv", "rel_h", "rel_w"):
        assert bf16_exact_integers(getattr(case, name)), name
    assert case.scale == 0.125 and (case.B, case.H, case.Hp, case.Wp, case.hd, case.kind) == (B, H, Hp, Wp, hd, kind)
    assert torch.equal(alg["out"], exp.out.double()) and bf16_exact(exp.out) and alg["logits"].shape == (B * H, L, (L + 31) // 32 * 32)
    assert float((alg["lse"] - exp.lse).abs().max()) < 1e-9
    logits = alg["logits"][..., :L]
    assert bool(torch.isinf(alg["logits"][..., L:]).all()) and bool((logits == logits.round()).all()) and float(logits.abs().max()) < 2 ** 24
    quantum, rows = any_fault_rows(kind, B, H, Hp, Wp, hd)
    if kind in X.TIE_KINDS:
        # the conditions of test_tie_case_conditions_and_sensitivity, restricted to the forward quantities
        assert torch.equal(exp.nwin, X.tie_winner_count(L)[None, None].expand(B, H, L)) and set(exp.nwin.unique().tolist()) == {1, 2, 4}
        assert int(exp.nwin[0, 0, L - 1]) == 4 and int(exp.nwin[0, 0, L - 3]) == 2 and float(exp.loser) <= -X.MIN_MARGIN
        for tile in range(L // 32):
            assert set(exp.nwin[0, 0, 32 * tile:32 * tile + 32].tolist()) == {1, 2, 4}
        assert float(logits.max()) == 0 and torch.equal((logits == 0).sum(-1).reshape(B, H, L), exp.nwin)
        q = case.qkv.reshape(B, L, 3, H, hd)[:, :, 0]
        assert bf16_exact(q * case.scale)
        assert float((q.double() @ case.rel_h.double().t()).abs().max()) == 0 and float((q.double() @ case.rel_w.double().t()).abs().max()) == 0
        assert torch.equal(exp.lse, torch.log(exp.nwin.double()).reshape(B * H, L))
        assert quantum in (0.25, 0.5, 1.0) and float((exp.out * 4 - (exp.out * 4).round()).abs().max()) == 0
        # P = 1 / n and l = n exactly, and the fp32 sum of the winners' V rows is exact: |V| <= 64, four terms
        assert float(X.tie_exact_sums(case, X.tie_algebra(case))["out"]) < 2 ** 24
        if L % 32:                    # a key >= L left alive sits at exactly 0 and joins every row's tie: V / n becomes V / (n + phantoms)
            assert rows["tail_keys_alive"] == B * H * L
    else:
        assert exp.margin.shape == (B, H, L) and float(exp.margin.min()) >= X.MIN_MARGIN, float(exp.margin.min())
        assert torch.equal(exp.lse.reshape(B, H, L), exp.top) and torch.equal(exp.top, exp.top.round())
        assert bf16_exact_integers(exp.out) and 1 <= float(exp.out.abs().min()) and float(exp.out.abs().max()) <= 64 and quantum >= 1
    if kind == "below_zero":
        assert float(exp.top.max()) <= -150 and float(logits.max()) <= -150
        assert all(torch.equal(exp.target[b, h].sort().values, torch.arange(L)) for b in range(B) for h in range(H))
        assert float(case.rel_h.abs().max()) == 0 and float(case.rel_w.abs().max()) == 0
        kq = case.qkv.reshape(B, L, 3, H, hd)
        assert bool((kq[:, :, 1, :, X.BELOW_ZERO_CHANNEL] == -8 * (hd + 24)).all()) and set(kq[:, :, 0, :, X.BELOW_ZERO_CHANNEL].unique().tolist()) == set(X.AMPLITUDES[:min(L, 3)])
        if L % 32:                    # a zero-K key >= L left alive wins every row by >= 150 and returns its zero V row
            assert rows["tail_keys_alive"] == B * H * L
            assert float(X.any_algebra(case, "tail_keys_alive")["out"].abs().max()) < 1e-60      # (fp64 keeps exp(-150); fp32 does not)
    if kind == "all_to_last":
        assert rows["last_key_dropped"] == B * H * L
        assert L % 32 == 0 or rows["tail_tile_dropped"] == B * H * L
    if L % 32 == 0:
        assert rows["tail_keys_alive"] == rows["tail_tile_dropped"] == rows["pad_row_stored"] == 0
    elif B > 1:
        # rows >= L of the last query tile are copies of row L - 1; stored, they land on the next sample's first rows, whose expected
        # content differs in every row and head (V names its sample).  On the device this is also held through a pre-filled out buffer.
        n = min((L + 31) // 32 * 32 - L, L)
        assert rows["pad_row_stored"] == (B - 1) * H * n
        want = exp.out.double().reshape(B, L, H, hd)
        assert bool((want[1:, :n] != want[:-1, L - 1:L]).any(-1).all())
    print("%s %dx%dx%dx%d hd%d: quantum %g; output rows (of %d) each wrong forward moves: %s" % (kind, B, H, Hp, Wp, hd, quantum, B * H * L, rows))


@pytest.mark.parametrize("hd", [64, 80])
@pytest.mark.parametrize("fault", X.ANY_FAULTS)
def test_every_named_wrong_forward_is_caught(fault, hd):
    """Each wrong forward of exact_cases.any_algebra changes some out element of some case by at least one quantum -- for either head dim, and
    for the two faults of the 4-key run also in each of the kernel's two branches (Wp < 4: stepping per key; Wp >= 4: two row entries and a
    select).  A condition, not a measurement: a fault no case sees wants another case."""
    seen = {True: [], False: []}
    for s in ANY_SHAPES:
        if s[5] == hd and any_fault_rows(*s)[1][fault]:
            seen[s[4] < 4].append("%s %dx%d: %d rows" % (s[0], s[3], s[4], any_fault_rows(*s)[1][fault]))
    print("%s hd%d: caught by %d cases with Wp < 4, %d with Wp >= 4; first %s" % (fault, hd, len(seen[True]), len(seen[False]), (seen[True] + seen[False])[:3]))
    assert seen[True] or seen[False], fault
    if fault in ("row_of_first_key", "column_wrap_zero"):
        assert seen[True] and seen[False], (fault, seen)


ANY_BIAS_SHAPES = [s for s in ANY_SHAPES if s[0] == "bias_rank" and s not in ATTN_SHAPES]


@pytest.mark.parametrize("kind,B,H,Hp,Wp,hd", ANY_BIAS_SHAPES, ids=["%dx%dx%dx%d-hd%d" % s[1:] for s in ANY_BIAS_SHAPES])
def test_bias_rank_tables_decide_alone_on_ragged_grids(kind, B, H, Hp, Wp, hd):
    """test_bias_rank_tables_decide_alone on the grids only the any-grid kernel takes: one right (kh, kw) per query, margin a multiple of 256."""
    test_bias_rank_tables_decide_alone(kind, B, H, Hp, Wp, hd)


# ------------------------------------------------------------------------------------------------ attention on any token grid: the backward
ANY_BWD_SHAPES = X.any_bwd_shapes()
ANY_BWD_TIE_SHAPES = [s for s in ANY_BWD_SHAPES if s[0] in X.TIE_KINDS]
ANY_BWD_NEW_GATHER_SHAPES = [s for s in ANY_BWD_SHAPES if s[0] not in X.TIE_KINDS and s not in ANY_SHAPES]
_id6 = lambda s: "%s-%dx%dx%dx%d-hd%d" % s
# sha256 over the bytes of qkv, rel_h, rel_w and dout of three tie cases with L % 4 == 0, one per placement, taken before tie_case admitted
# ragged grids
TIE_DIGESTS = {("tie_near", 2, 2, 8, 4, 64): "099de30c1da1bdd4c83087575973174fa52e72473069f2238c81d452f446cde0",
               ("tie_quarter_sparse", 2, 2, 12, 6, 80): "cd8df4ddc2cbde662a66107f93758c4f120e62bae434356e38d0e00466d7d189",
               ("tie_mirror", 2, 2, 8, 28, 64): "c3246b28191afaa61ac94c2cb8783f4cffe86a44322be48cbb31404589abf536"}


@pytest.mark.parametrize("shape", sorted(TIE_DIGESTS), ids=_id6)
def test_tie_cases_with_L_a_multiple_of_four_are_unchanged(shape):
    """Lifting L % 4 == 0 from tie_case left the same seeds and the same draws where L % 4 == 0: the existing tie tests and their recorded
    logs keep their meaning."""
    import hashlib
    case, _ = X.tie_attn_case(*shape)
    h = hashlib.sha256()
    for name in ("qkv", "rel_h", "rel_w", "dout"):
        h.update(getattr(case, name).contiguous().numpy().tobytes())
    assert h.hexdigest() == TIE_DIGESTS[shape]
    assert X.tie_loners(case.L, case.Wp) == [] and torch.equal(X.tie_members("near", 32), (4 * torch.arange(8)[:, None] + 2 + torch.arange(4)) % 32)


@pytest.mark.parametrize("Hp,Wp", sorted({s[3:5] for s in ANY_BWD_SHAPES} | {(5, 2), (7, 1), (4, 3), (70, 35)}), ids=lambda v: str(v))
def test_loners_and_groups_on_any_grid(Hp, Wp):
    """tie_loners: L % 4 keys, valid, distinct, off key 0 and key L - 1, outside the last 32-key tile wherever there is a second tile, and
    inside neither border key row nor border tile where the grid has such keys; the groups of four cover every other key exactly once."""
    L = Hp * Wp
    if L < 4:                             # (5 x 2 gave a negative key in the first draft of this; 1 x 1 and 2 x 1 have no room at all)
        with pytest.raises(ValueError, match="gather kinds"):
            X.tie_loners(L, Wp)
        return
    loners = X.tie_loners(L, Wp)
    assert len(loners) == len(set(loners)) == L % 4 and all(0 < k < L - 1 for k in loners)
    last = (L - 1) // 32 * 32
    if L > 32:
        assert all(k < last for k in loners)
    if len([k for k in range(L) if Wp <= k < L - Wp and 32 <= k < last]) >= L % 4:
        assert all(Wp <= k < L - Wp and 32 <= k < last for k in loners)
    if L >= 4:
        for placement in X.TIE_PLACEMENTS:
            m = X.tie_members(placement, L, Wp)
            assert m.shape == (L // 4, 4) and sorted(m.flatten().tolist() + loners) == list(range(L))
        assert L < 8 or {L - 2, L - 1, 0, 1} == set(X.tie_members("near", L, Wp)[-1].tolist())      # the last keys pair up with the first


def test_the_any_grid_backward_parametrisation_covers_what_it_says():
    """Four routes on the backward's own launch counter; the gather kinds and below_zero on every grid; the tie kinds on the ten tie grids,
    minus the kinds ANY_BWD_LEFT_OUT names; and the caps: every tie grid keeps a dense kind at head dim 64 or all three sparse placements,
    every route all three placements on at least three ragged grids."""
    params = X.any_bwd_route_params()
    assert set(X.ANY_BWD_ROUTES) == {"any_bwd_%s_hd%d" % (t, hd) for t in ("bf16", "fp32") for hd in (64, 80)}
    assert set(X.ANY_BWD_TIE_GRIDS) == {(2, 2, 12, 3), (2, 2, 6, 3), (2, 2, 9, 7), (2, 2, 10, 5), (2, 2, 12, 6), (1, 2, 3, 11), (2, 2, 5, 13),
                                        (2, 2, 4, 33), (2, 2, 8, 4), (2, 2, 31, 19)}
    assert X.ANY_BWD_GATHER_ONLY == [(2, 2, 1, 1), (2, 2, 2, 1), (2, 2, 11, 2), (2, 2, 5, 2)]
    assert {g[2] * g[3] for g in X.ANY_BWD_TIE_GRIDS} >= {18, 33, 36, 50, 63, 65} and max(g[2] * g[3] for g in X.ANY_BWD_TIE_GRIDS) == 589
    assert {len(X.tie_loners(g[2] * g[3], g[3])) for g in X.ANY_BWD_TIE_GRIDS} == {0, 1, 2, 3}
    assert all(ops_takes(g) == (g == X.ANY_BWD_ALIGNED) for g in X.ANY_BWD_TIE_GRIDS + X.ANY_BWD_GATHER_ONLY)
    placements = lambda kinds: {k.replace("tie_", "").replace("_sparse", "") for k in kinds if k in X.TIE_KINDS}
    for route, (tname, hd, counter, grids) in X.ANY_BWD_ROUTES.items():
        assert counter == "pa_attn_any_bwd_launches" and route == "any_bwd_%s_hd%d" % (tname, hd)
        assert grids == X.ANY_BWD_TIE_GRIDS + X.ANY_BWD_GATHER_ONLY
        full = 0
        for grid in grids:
            kinds = [p[1] for p in params if p[0] == route and p[2:] == grid]
            assert len(kinds) == len(set(kinds)) and set(X.ANY_KINDS) <= set(kinds)
            if grid in X.ANY_BWD_GATHER_ONLY:
                assert set(kinds) == set(X.ANY_KINDS)
                continue
            left = dict(X.ANY_BWD_LEFT_OUT.get((hd, grid), {}), **(X.ANY_BWD_LEFT_OUT_FP32.get((hd, grid), {}) if tname == "fp32" else {}))
            assert set(kinds) == set(X.ANY_KINDS) | (set(X.TIE_KINDS) - set(left)) and all(left.values())
            full += placements(kinds) == set(X.TIE_PLACEMENTS) and not ops_takes(grid)
            if hd == 64:                  # the cap of a grid
                assert set(kinds) & set(X.TIE_KINDS[:3]) or set(X.TIE_KINDS[3:]) <= set(kinds), (route, grid, kinds)
        assert full >= 3, (route, full)   # the cap of a route
    kind, grid, hd = X.ANY_BWD_CHAIN
    assert (2 * grid[2] - 1, 2 * grid[3] - 1) == (15, 9) and kind in X.TIE_KINDS and len(ANY_BWD_SHAPES) == len(set(ANY_BWD_SHAPES))


@pytest.mark.parametrize("Hp,Wp", sorted({s[3:5] for s in ANY_BWD_SHAPES}), ids=lambda v: str(v))
def test_any_bwd_key_walk_without_a_fault_is_row_major(Hp, Wp):
    """Kernel A's walk restated (exact_cases.any_bwd_key_walk) reads and adds key k at (k // Wp, k % Wp); each walk fault moves some key
    < L, or the grid has no key that could show it."""
    L = Hp * Wp
    bh, bw, rh, cw = X.any_bwd_key_walk(L, Hp, Wp)
    k = torch.arange(bh.numel())
    live = k < L
    assert torch.equal(bh, (k // Wp).clamp_max(Hp - 1)) and torch.equal(bw, k % Wp) and torch.equal(cw, k % Wp)
    assert torch.equal(rh[live], (k // Wp)[live]) and bool((rh[~live] >= Hp - 1).all())
    moved = {}
    for fault in ("row_carry_lost_in_group", "half1_offset_no_wrap", "tile_carry_lost", "column_wrap_lost"):
        f = X.any_bwd_key_walk(L, Hp, Wp, fault)
        moved[fault] = int(sum(((a != b) & live).sum() for a, b in zip(f, (bh, bw, rh, cw))))
    crossing8 = (k // Wp != (k - k % 8) // Wp) & live
    assert moved["row_carry_lost_in_group"] == (int(crossing8.sum()) if Wp >= 8 else 0)
    assert (moved["column_wrap_lost"] > 0) == (L > 1 and bool(crossing8.any() or Wp < 8 and L > Wp))
    grp = torch.arange(bh.numel() // 8)                                      # (tile, register group): a carry its first key has seen by then
    first = 32 * (grp // 4) + 8 * (grp % 4)
    carried = (first // Wp != (8 * (grp % 4)) // Wp + (grp // 4) * (32 // Wp)) & (first < L)
    assert (moved["tile_carry_lost"] > 0) == bool(carried.any()) and (not carried.any() or (32 % Wp != 0 and L > 32))
    print("%dx%d: key slots each walk fault moves: %s" % (Hp, Wp, moved))


@functools.lru_cache(maxsize=None)
def any_bwd_base(shape):
    """-> (case, expectation, tie_algebra, {name: expected tensor}, {name: quantum}, {name: fp32 bound}) of one built shape."""
    case, exp = X.any_case(*shape)
    alg = X.tie_algebra(case)
    if shape[0] in X.TIE_KINDS:
        want = dict(dq=exp.dq, dk=exp.dk, dv=exp.dv, drcat=exp.drcat)
        return case, exp, alg, want, {n: X.tie_quantum(t) for n, t in want.items()}, X.any_bwd_fp32_bounds(case, alg)
    zero = torch.zeros_like(exp.dv, dtype=torch.float64)
    want = dict(dq=zero, dk=zero, dv=exp.dv.double(), drcat=torch.zeros(2 * case.Hp + 2 * case.Wp - 2, case.hd, dtype=torch.float64))
    bound = dict(dq=zero, dk=zero, dv=X.dv_fp32_bound(case, exp), drcat=want["drcat"])
    return case, exp, alg, want, dict.fromkeys(want, 1.0), bound


@pytest.mark.parametrize("shape", ANY_BWD_TIE_SHAPES, ids=_id6)
def test_any_bwd_tie_case_conditions(shape):
    """What tests/test_attention_any_bwd_exact_gpu.py rests on, for every tie case it builds: the conditions of
    test_tie_case_conditions_and_sensitivity as exact_cases.any_bwd_condition_failed states them for ragged grids (winner counts from the
    logits with 1, 2 and 4 present, four winners in the last row, the last key tile in full groups with a non-zero dS in every key, a
    non-zero dS in every tie row of the last query tile, the margin, fp32 sums below 2^24 units, out / P / dS / dG bf16-exact, expectations
    dyadic to 1/32, the fp32 bound below half a quantum), and here: integer operands, zero bias tables in the forward, Delta exact as
    hi + lo, the non-zero fractions, autograd == the hand algebra == the algebra over the kernel's own walk."""
    kind, B, H, Hp, Wp, hd = shape
    case, exp, alg, want, quanta, bound = any_bwd_base(shape)
    L, nh = Hp * Wp, 2 * Hp - 1
    assert X.any_bwd_condition_failed(case, exp, alg, fp32=True) is None
    assert torch.equal(exp.nwin, X.tie_winner_count(L)[None, None].expand(B, H, L))          # the loners went to one-winner rows
    offset = X.tie_layout(hd)[4]
    for name in ("qkv", "rel_h", "rel_w", "dout"):
        assert bf16_exact_integers(getattr(case, name)), name
    q = case.qkv.reshape(B, L, 3, H, hd)[:, :, 0]
    assert bf16_exact(q * case.scale) and case.scale == 0.125
    assert float(alg["Gh"].abs().max()) == 0 and float(alg["Gw"].abs().max()) == 0
    assert float(case.rel_h.abs().sum()) == float(case.rel_h[:, offset].sum()) == nh * (nh + 1) / 2
    assert bf16_hi_lo_exact(alg["delta"]) and torch.equal(exp.lse, torch.log(exp.nwin.double()).reshape(B * H, L))
    density = float((case.dout != 0).float().mean())
    assert abs(density - (1 / 16 if kind.endswith("sparse") else 2 / 3)) < 0.02
    for name, a, b in (("out", exp.out, alg["out"]), ("dq", exp.dq, alg["dq"]), ("dk", exp.dk, alg["dk"]), ("dv", exp.dv, alg["dv"]),
                       ("drh", exp.drcat[:nh], alg["drh"]), ("drw", exp.drcat[nh:], alg["drw"])):
        assert float((a - b).abs().max()) < 1e-9, name
    # the non-zero fractions, as today (a loner's dK row is zero: at most 3 of L keys)
    off_dq = exp.dq.reshape(B * L, H, hd)[:, :, offset]
    assert bf16_exact(exp.out) and float((exp.dq != 0).double().mean()) > 0.02 and float((off_dq != 0).double().mean()) > 0.3
    assert float((exp.dk != 0).double().mean()) > 0.4 and float((exp.drcat[:nh].abs().sum(1) != 0).double().mean()) > 0.5
    if "quarter" not in kind:
        assert float((exp.drcat[nh:].abs().sum(1) != 0).double().mean()) > 0.5
    assert min(quanta.values()) >= 1 / 32
    # the kernel's own walk, without a fault, is the hand algebra: dS, the tables, dG, dq, dk, dv and both table gradients
    walk = X.any_bwd_algebra(case, base=alg)
    for name in ("dS", "dG_h", "dG_w", "dq", "dk", "dv", "drh", "drw"):
        assert torch.equal(walk[name], alg[name]), name
    key = torch.arange(L)
    for tab, idx, n in ((walk["tab_h"], key // Wp, Hp), (walk["tab_w"], key % Wp, Wp)):
        assert torch.equal(tab, torch.zeros(B * H, L, n, dtype=torch.float64).index_add_(2, idx, alg["dS"]))
    ratio = {n: float(bound[n].max()) / quanta[n] for n in bound}
    print("%s %dx%dx%dx%d hd%d: loners %s; quanta %s; fp32 bound / quantum %s; largest fp32 sum 2^%.1f units"
          % (shape + (X.tie_loners(L, Wp), quanta, {n: "%.3f" % r for n, r in ratio.items()},
                      torch.log2(torch.tensor(max(X.tie_exact_sums(case, alg).values()))).item())))
    assert max(ratio.values()) < 0.5, ratio


LEFT_OUT = [(kind,) + grid + (hd,) for (hd, grid), kinds in list(X.ANY_BWD_LEFT_OUT.items()) + list(X.ANY_BWD_LEFT_OUT_FP32.items()) for kind in kinds]


@pytest.mark.parametrize("shape", LEFT_OUT, ids=_id6)
def test_every_kind_left_out_fails_the_condition_it_is_listed_with(shape):
    kind, B, H, Hp, Wp, hd = shape
    case, exp = X.tie_attn_case(*shape)
    said = dict(X.ANY_BWD_LEFT_OUT.get((hd, (B, H, Hp, Wp)), {}), **X.ANY_BWD_LEFT_OUT_FP32.get((hd, (B, H, Hp, Wp)), {}))[kind]
    assert X.any_bwd_condition_failed(case, exp, X.tie_algebra(case), fp32=True) == said


@pytest.mark.parametrize("shape", ANY_BWD_NEW_GATHER_SHAPES, ids=_id6)
def test_any_bwd_gather_case_conditions_on_the_new_grids(shape):
    """The gather kinds on the grids tests/test_attention_any_exact_gpu.py does not run (the others: test_any_grid_case_conditions): the
    margin, integer operands, an integer dV whose fp32 bound stays below 1/2, and a backward that is zero but for dV in the walk algebra."""
    kind, B, H, Hp, Wp, hd = shape
    case, exp, alg, want, _, bound = any_bwd_base(shape)
    L = Hp * Wp
    assert exp.margin.shape == (B, H, L) and float(exp.margin.min()) >= X.MIN_MARGIN, float(exp.margin.min())
    for name in ("qkv", "rel_h", "rel_w", "dout"):
        assert bf16_exact_integers(getattr(case, name)), name
    assert bf16_exact_integers(exp.out) and bf16_exact_integers(exp.dv.float()) and float(bound["dv"].max()) < 0.5
    assert torch.equal(exp.lse.reshape(B, H, L), exp.top) and torch.equal(exp.top, exp.top.round()) and float(exp.top.abs().max()) < 2 ** 24
    walk = X.any_bwd_algebra(case, base=alg)
    for name in ("dq", "dk", "drcat"):
        assert float(walk[name].abs().max()) < 1e-50, name
    assert float((walk["dv"] - want["dv"]).abs().max()) < 1e-50
    if kind == "below_zero":
        assert float(exp.top.max()) <= -150


def _fault_effect(shape, fault):
    """-> (largest move in quanta, the same in units of the fp32 bound at the element moved most, the max-norm measure of the tolerance
    test) of one wrong backward on one built case; non-finite values count as infinitely far."""
    case, exp, alg, want, quanta, bound = any_bwd_base(shape)
    got = X.any_bwd_algebra(case, fault, base=alg)
    nh = 2 * case.Hp - 1
    seen = beyond = measure = 0.0
    for n in want:
        diff = torch.nan_to_num((got[n] - want[n]).abs(), nan=float("inf"), posinf=float("inf"))
        top = float(diff.max())
        if top < quanta[n]:
            continue
        seen = max(seen, top / quanta[n])
        at = int(diff.argmax())
        b = float(bound[n].flatten()[at])
        beyond = max(beyond, top / b if b > 0 else float("inf"))
    whole = max(float(want[n].abs().max()) for n in ("dq", "dk", "dv"))
    parts = [(got[n], want[n], whole) for n in ("dq", "dk", "dv")]
    whole_r = float(want["drcat"].abs().max())
    parts += [(got["drcat"][:nh], want["drcat"][:nh], whole_r), (got["drcat"][nh:], want["drcat"][nh:], whole_r)]
    for g, w, wh in parts:
        d = float(torch.nan_to_num((g - w).abs(), nan=float("inf"), posinf=float("inf")).max())
        scale = float(w.abs().max()) or wh
        measure = max(measure, d / scale if scale else (float("inf") if d else 0.0))
    return seen, beyond, measure


# the shapes the sensitivity test walks: every tie case, and the two gather kinds whose logits a wrong walk or a live tail key can move
FAULT_SHAPES = ANY_BWD_TIE_SHAPES + [s for s in ANY_BWD_SHAPES if s[0] in ("bias_rank", "below_zero")]


@pytest.mark.parametrize("fault", X.ANY_BWD_FAULTS)
def test_every_named_wrong_backward_is_caught(fault):
    """Each wrong backward of exact_cases.any_bwd_algebra moves some element of dq, dk, dv or drcat of some built case by at least one
    quantum, and by at least 16 times the fp32 build's bound at that element (every built case runs in both builds).  A condition, not a
    measurement: a fault no case sees wants another case.  Printed per fault: how many cases catch it, and the max-norm measure
    (max|a - b| / max|b| per tensor, the tolerance test's, gates 5e-5 fp32 and 1.6e-2 bf16) the fault has on the cases that catch it --
    where the smallest is below the gate, a case of that size would have hidden it."""
    caught = []
    for s in FAULT_SHAPES:
        seen, beyond, measure = _fault_effect(s, fault)
        if seen >= 1 and beyond >= 16:
            caught.append((measure, seen, s))
    assert caught, fault
    tie = [c for c in caught if c[2][0] in X.TIE_KINDS]
    lo, hi = min(caught), max(caught)
    print("%s: caught by %d of %d cases (%d tie cases); old measure between %.2g (%s, %.0f quanta) and %.2g (%s); below the bf16 gate 1.6e-2 on %d"
          % (fault, len(caught), len(FAULT_SHAPES), len(tie), lo[0], _id6(lo[2]), lo[1], hi[0], _id6(hi[2]), sum(c[0] < OLD_GATE_BF16 for c in caught)))
    if fault == "half1_offset_no_wrap":
        assert all(c[2][0] == "bias_rank" for c in caught)         # the tie cases' bias tables are zero in the forward: the read cannot show
    else:
        assert tie, fault
    if fault in ("row_carry_lost_in_group", "column_wrap_lost", "tile_carry_lost", "dg_emit_off_by_one", "aux_row_shift"):
        assert {c[2][5] for c in caught} == {64, 80}
