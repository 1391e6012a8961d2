"""The conditions tests/test_attention_exact_gpu.py and tests/test_conv3x3_exact_gpu.py rest on, asserted on the CPU for every case those
files build (the parametrisations are shared through tests/exact_cases.py)."""
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
