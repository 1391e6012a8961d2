"""The conditions tests/test_gemm_exact_gpu.py rests on, asserted on the CPU for every case that file runs (the parametrisations are shared
through tests/gemm_exact_cases.py): operands and references are exact in their dtypes, every case reaches the engine its table claims (by
Python copies of the C++ route rules), the split plans contain every kind of plan, the fmaf emulation of the 8-bit GELU' code equals a
Fraction computation, and every named wrong kernel is seen by the cases.  The last test prints, per family, the routes covered and the split plans found (`pytest -s` prints the per-case lines too)."""
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import gemm_exact_cases as G


def bf16_exact(t):
    t = t.double()
    return torch.equal(t.to(torch.bfloat16).double(), t)


def f32_exact(t):
    t = t.double()
    return torch.equal(t.float().double(), t)


def operands_ok(case, dtype):
    """integers the operand dtype holds; every partial sum an integer below 2^24 (K times the largest entries)"""
    a, b = case["a"], case["b"]
    assert a.dtype == b.dtype == torch.int64
    if dtype == G.BF16:
        assert bf16_exact(a) and bf16_exact(b)
    K = a.shape[1]
    bound = K * int(a.abs().max()) * int(b.abs().max()) + (0 if case["bias"] is None else int(case["bias"].abs().max()))
    assert bound < 2 ** 24, bound
    if case["bias"] is not None:
        assert int(case["bias"].abs().max()) <= 8


def differs(a, b):
    return not torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ 1. generic engine
def test_generic_shapes_cover_every_value_in_every_layout():
    params = G.generic_params()
    assert len(params) == len(set(params)) and len(params) <= 40
    for layout in G.LAYOUTS:
        for dtype in G.DTYPES:
            mine = [p[2:] for p in params if p[:2] == (layout, dtype)]
            rows = {1: 4, 65: 68, 129: 132} if layout == "wgrad" else {}        # pa_linear_wgrad: output rows % 4
            assert {s[0] for s in mine} >= {rows.get(r, r) for r in (1, 8, 65, 129, 200)}, (layout, dtype)
            assert {s[1] for s in mine} >= {8, 72, 136, 264}, (layout, dtype)
            assert {s[2] for s in mine} >= {8, 72, 136, 200}, (layout, dtype)
            assert (36 in {s[2] for s in mine}) == (dtype == G.F32 and layout != "dgrad"), (layout, dtype)
    print("generic engine: %d cases, all on the generic engine; per layout and dtype %s"
          % (len(params), {k: sum(1 for p in params if p[:2] == k) for k in sorted({p[:2] for p in params})}))


@pytest.mark.parametrize("layout,dtype,R,C,K", G.generic_params(), ids=lambda v: str(v))
def test_generic_case_conditions(layout, dtype, R, C, K):
    assert G.ROUTE_OF[layout](dtype, R, C, K) == "generic"
    bk = G.ENGINE_BK[dtype]
    assert K % bk != 0 and K % (8 if dtype == G.BF16 else 4) == 0           # ends inside a K tile; the ABI's rule
    if layout == "dgrad":
        assert K % 8 == 0 and C % 4 == 0                                        # pa_linear_dgrad_skip
    if layout == "wgrad":
        assert R % 4 == 0 and C % 4 == 0                                        # pa_linear_wgrad
    for kind in ("tern", "coded"):
        case = G.gemm_case(layout, R, C, K, kind)
        operands_ok(case, dtype)
        ref = G.gemm_ref(case)
        out_bf16 = dtype == G.BF16 and layout != "wgrad"
        assert bf16_exact(ref) if out_bf16 else int(ref.abs().max()) < 2 ** 24
        # a dropped K tail is seen by every case of the route (tied to it: every contraction here ends inside a tile)
        # -- on ternary operands; the position-coded ones where their rows' indices (7 i) % K reach the tail
        if kind == "tern" or int(case["idx"].max()) >= K // bk * bk:
            assert differs(G.gemm_ref(case, dtype, wrong="k_tail_dropped"), ref), (kind, "k tail")
        if kind == "coded":
            assert all(G.named_k(case, i, j, ref[i, j]) == int(case["idx"][i]) for i in (0, R - 1) for j in (0, C - 1))
    if layout == "wgrad":
        plan = G.split_plan(dtype, R, C, K)
        print("generic weight gradient %s %s: splits, klen, non-empty, last = %s (%s)" % (dtype, (R, C, K), plan, G.plan_kind(plan)))


# ------------------------------------------------------------------------------------------------ 2. split plans
def test_split_plans_contain_every_kind():
    kinds = {}
    for dtype, R, C, K in G.split_params():
        plan = G.split_plan(dtype, R, C, K)
        kinds.setdefault(G.plan_kind(plan), []).append((dtype, R, C, K, plan))
        assert G.route_wgrad(dtype, R, C, K) == "generic"
    for kind in ("single", "all_full", "ragged_last", "empty_splits"):
        assert kinds.get(kind), "no case with a %s plan any more" % kind
        print("split plans, %s: %s" % (kind, ["%s %dx%d K=%d -> %d x %d, %d non-empty, last %d" % ((d, R, C, K) + p) for d, R, C, K, p in kinds[kind]]))
    # the figures the case list was chosen by
    assert G.split_plan(G.BF16, 64, 64, 100)[:1] == (2,) and G.split_plan(G.F32, 64, 64, 100)[:1] == (4,)
    assert G.split_plan(G.BF16, 64, 64, 296)[:1] == (5,) and G.split_plan(G.F32, 64, 64, 296)[:1] == (10,)
    assert G.split_plan(G.BF16, 64, 64, 1000)[:1] == (16,) and G.split_plan(G.F32, 64, 64, 1000)[:1] == (32,)
    for R, C in G.SPLIT_OUTPUTS:
        assert G.split_plan(G.BF16, R, C, 4100) == (64, 128, 33, 4) and G.split_plan(G.F32, R, C, 4100) == (64, 96, 43, 68)
        assert G.split_plan(G.BF16, R, C, 40)[0] == 1
    # an empty-split plan's last non-empty split is ragged too
    assert all(p[3] < p[1] for _, _, _, _, p in kinds["empty_splits"])
    # the slab buffer of the largest plan: 64 slabs of 72 x 200 floats
    assert 64 * 72 * 200 * 4 < 4 << 20


@pytest.mark.parametrize("dtype,R,C,K", G.split_params(), ids=lambda v: str(v))
def test_split_case_conditions(dtype, R, C, K):
    case = G.gemm_case("wgrad", R, C, K)
    operands_ok(case, dtype)
    plan = G.split_plan(dtype, R, C, K)
    ref = G.gemm_ref(case)
    if plan[0] > 1:
        assert differs(G.gemm_ref(case, dtype, plan, "last_split_dropped"), ref)
    if plan[2] < plan[0]:
        assert differs(G.gemm_ref(case, dtype, plan, "empty_split_reads_first"), ref)
    if K % G.ENGINE_BK[dtype]:
        assert differs(G.gemm_ref(case, dtype, plan, "k_tail_dropped"), ref)


@pytest.mark.parametrize("R,C,K", G.SPLIT_CODED)
def test_split_coded_case_names_the_split(R, C, K):
    case = G.gemm_case("wgrad", R, C, K, "coded")
    ref = G.gemm_ref(case)
    for dtype in G.DTYPES:
        operands_ok(case, dtype)
        s, klen, live, _ = plan = G.split_plan(dtype, R, C, K)
        assert klen % G.code_group(K) == 0                                      # a code group lies in one split
        assert {int(k) // klen for k in case["idx"]} == set(range(live)), "the rows do not reach every non-empty split"
        for wrong in ("last_split_dropped", "empty_split_reads_first", "k_tail_dropped"):
            assert differs(G.gemm_ref(case, dtype, plan, wrong), ref), (dtype, wrong)
    for i in range(R):
        k = G.named_k(case, i, 0, ref[i, 0])
        assert k <= int(case["idx"][i]) < k + G.code_group(K)


# ------------------------------------------------------------------------------------------------ 3. residual epilogue
@pytest.mark.parametrize("route,dtype,R,C,K,rps", G.resid_params(), ids=lambda v: str(v))
def test_resid_case_conditions(route, dtype, R, C, K, rps):
    assert G.route_fwd(dtype, R, C, K) == route
    case = G.resid_case(R, C, K, rps)
    operands_ok(case, dtype)
    ref = G.resid_ref(case)
    assert f32_exact(ref) and f32_exact(case["resid"]) and float(case["resid"].abs().max()) <= 1024
    assert torch.equal(ref * 2, (ref * 2).round()) and float(ref.abs().max()) < 2 ** 13          # half-integers
    rs = case["rowscale"]
    assert set(rs.tolist()) <= set(G.ROWSCALES) and bool((rs == 0).any()) and rs.numel() == (R + rps - 1) // rps
    dropped = (rs == 0)[torch.arange(R) // rps]
    assert torch.equal(ref[dropped], case["resid"][dropped])
    assert differs(G.resid_ref(case, "rowscale_by_128"), ref)                   # every case: no rps here is 128
    if route == "g256":                                                         # tied to the split fp32 column layout of that kernel
        assert differs(G.resid_ref(case, "bias_halves_swapped"), ref)
    if C == 264:
        assert C % 64 == 8 and (C - 8) + 32 >= C                               # the last group's j + 32 half is outside
    print("residual epilogue %s %s rps %d -> %s, %d of %d samples dropped" % (dtype, (R, C, K), rps, route, int((rs == 0).sum()), rs.numel()))


def test_resid_skip_case_conditions():
    R, C, K, rps = G.RESID_SKIP
    assert G.route_fwd(G.BF16, R, C, K) == "g256" and R == 2 * rps and rps % 256 == 0      # 256-row tiles: tile 1 = sample 1, all dropped
    for scales in G.RESID_SKIP_SCALES:
        case = G.resid_case(R, C, K, rps, tuple(scales))
        ref = G.resid_ref(case)
        assert f32_exact(ref) and torch.equal(ref[rps:], case["resid"][rps:]) and differs(ref[:rps], case["resid"][:rps])
        assert bool(case["a"][rps:].abs().sum() > 0)                            # the dropped sample's operand rows are not zero


# ------------------------------------------------------------------------------------------------ 4. pixel shuffle
@pytest.mark.parametrize("dtype,kind,B,Hp,Wp,P,C,K", G.pixshuf_params(), ids=lambda v: str(v))
def test_pixshuf_case_conditions(dtype, kind, B, Hp, Wp, P, C, K):
    claimed = dict(G.PIXSHUF_CASES)[(B, Hp, Wp, P, C, K)]
    assert G.route_pixshuf(dtype, B, Hp, Wp, P, C, K) == (claimed if dtype == G.BF16 else "generic")
    assert K % 8 == 0
    case = G.pixshuf_case(kind, B, Hp, Wp, P, C, K)
    operands_ok(case, dtype)
    ref = G.pixshuf_ref(case, B, Hp, Wp, P, C)
    assert ref.shape == (B, Hp * P, Wp * P, C) and bf16_exact(ref)
    assert differs(G.pixshuf_ref(case, B, Hp, Wp, P, C, "pq_swapped"), ref)
    # the model's own formula, element by element on a few corners
    y = (case["a"] @ case["b"] + case["bias"]).reshape(B, Hp, Wp, P, P, C)
    for b, h, w, p, q, c in ((0, 0, 0, 0, 1, 0), (B - 1, Hp - 1, Wp - 1, P - 1, 0, C - 1), (0, Hp - 1, 0, 1, P - 1, C // 2)):
        assert ref[b, h * P + p, w * P + q, c] == y[b, h, w, p, q, c]
    s = G.pixshuf_sign(P, C).reshape(P, P, C)
    assert differs(s.transpose(0, 1), s) and all(differs(s.roll(k, 2), s) for k in range(1, C))
    print("pixel shuffle %s %s %s -> %s" % (dtype, kind, (B, Hp, Wp, P, C, K), G.route_pixshuf(dtype, B, Hp, Wp, P, C, K)))


def test_pixshuf_params_cover_the_routes():
    params = G.pixshuf_params()
    assert {p[0] for p in params if G.route_pixshuf(*((p[0],) + p[2:])) == "g256"} == {G.BF16}
    generic = {(p[0],) + p[2:] for p in params if G.route_pixshuf(*((p[0],) + p[2:])) == "generic"}
    assert {g[0] for g in generic} == {G.BF16, G.F32} and (G.BF16, 2, 2, 3, 4, 4, 128) in generic and (G.BF16, 2, 2, 3, 4, 8, 72) in generic


# ------------------------------------------------------------------------------------------------ 5. GELU' epilogue
def test_g8_value_is_the_fused_multiply_add():
    """the fp64 expression is exact for all 256 codes, so its one rounding to fp32 is fmaf's; ops.gelu_aux_decode returns those bits"""
    from painter_amd import ops
    assert float(G.G8_STEP) == float(np.float32(np.float32(1.26) / np.float32(255))) and float(G.G8_OFF) == float(np.float32(0.13))
    q = np.arange(256)
    f64 = q.astype(np.float64) * np.float64(G.G8_STEP) - np.float64(G.G8_OFF)
    got = G.g8_value(q)
    old = 0
    for k in range(256):
        exact = G.g8_value_fraction(k)
        assert Fraction(float(f64[k])) == exact, k
        # round to nearest: no other fp32 number is closer to the exact value
        v = np.float32(got[k])
        lo, hi = np.nextafter(v, np.float32(-np.inf)), np.nextafter(v, np.float32(np.inf))
        err = abs(Fraction(float(v)) - exact)
        assert err <= abs(Fraction(float(lo)) - exact) and err <= abs(Fraction(float(hi)) - exact), k
        old += int(G.g8_value_old(k) != v)
    assert old == 55, old                  # the codes at which the earlier decode (fp32 multiply, fp32 subtract) was another number
    dec = ops.gelu_aux_decode(torch.arange(256, dtype=torch.uint8))
    assert dec.dtype == torch.float32 and np.array_equal(dec.numpy().view(np.uint32), got.view(np.uint32))
    # the encoder's codes decode to within half a step of what was encoded, as before
    g = torch.linspace(-0.129, 1.129, 1001, dtype=torch.float64)
    assert float((ops.gelu_aux_decode(ops.gelu_aux_encode(g)).double() - g).abs().max()) <= 0.5 * 1.26 / 255 + 1e-6


@pytest.mark.parametrize("route,R,C,K,pad", G.DGELU_CASES, ids=lambda v: str(v))
def test_dgelu_case_conditions(route, R, C, K, pad):
    assert G.route_dgrad(G.BF16, R, C, K) == route and (C + pad) % 8 == 0
    case = G.dgelu_case(R, C, K, pad)
    operands_ok(case, G.BF16)
    assert set(case["aux"].unique().tolist()) == set(range(256))               # all 256 codes
    v = case["a"] @ case["b"]
    assert int(v.abs().max()) < 2 ** 24 and int(v.abs().max()) * 2 ** 24 < 2 ** 53          # v g: exact in fp64
    ref = G.dgelu_ref(case)
    assert ref.dtype == torch.bfloat16 and ref.shape == (R, C)
    assert differs(G.dgelu_ref(case, "aux_pitch_doubled"), ref)                 # every case, padded or not
    print("GELU' epilogue %s pad %d -> %s" % ((R, C, K), pad, route))


def test_dgelu_colsum_case_conditions():
    seen_old = False
    for R, C, K, knobs, rows in G.DGELU_CS_CASES:
        assert G.route_dgrad(G.BF16, R, C, K) == "g256" and C % 8 == 0
        assert {0, R - 1} <= set(rows)
        for r in rows:
            case = G.dgelu_case(R, C, K, 0, r)
            assert int(case["a"].abs().sum()) == int(case["a"][r].abs().sum()) > 0
            ref = G.dgelu_colsum_ref(case, r)
            assert ref.dtype == torch.float32 and bool((ref != 0).any())
            seen_old |= differs(G.dgelu_colsum_ref(case, r, "old_decode"), ref)
    assert seen_old                        # the earlier decode arithmetic shows in the fp32 sums (a bf16 store hides most of it)
    assert G.DGELU_CS_CASES[0][4] == (0, 127, 128, 255, 256, 327) and G.DGELU_CS_CASES[2][0] >= 512       # a mixed plan needs >= 512 rows
    R, C, K, rows = G.DGELU_CS_GENERIC
    assert G.route_dgrad(G.BF16, R, C, K) == "generic"


# ------------------------------------------------------------------------------------------------ 6. GELU forward
@pytest.mark.parametrize("route,R,C,K", G.GELU_CASES, ids=lambda v: str(v))
def test_gelu_case_conditions(route, R, C, K):
    assert G.route_fwd(G.BF16, R, C, K) == route
    case = G.gemm_case("fwd", R, C, K)
    operands_ok(case, G.BF16)
    pre = G.gemm_ref(case)
    assert bf16_exact(pre)                                                      # the epilogue's rounding of pre to bf16 changes nothing
    n = pre.unique().numel()
    assert n >= 40 and pre.numel() / n >= 50                                    # many values, each at many (row, column) places
    print("GELU forward %s -> %s: %d distinct pre-activations in [%d, %d]" % ((R, C, K), route, n, int(pre.min()), int(pre.max())))


# ------------------------------------------------------------------------------------------------ 7. reductions
def test_slab_cases_reach_both_kernels():
    params = G.slab_params()
    assert {k for _, _, k in params} == {"wide", "tree"}
    assert {(n, nz) for n, nz, k in params if k == "wide"} == {(n, nz) for n in G.SLAB_N_LARGE for nz in (1, 3, 16)}
    assert all(G.slab_kernel(n, 17) == "tree" for n in G.SLAB_N_LARGE) and all(n % 4 == 0 for n, _, _ in params)
    assert {n for n, _, _ in params} == {4, 68, 260, 2 ** 18, 2 ** 18 + 4} and {nz for _, nz, _ in params} == {1, 3, 16, 17, 33, 64}
    assert max((n + 8) * nz * 4 for n, nz, _ in params) < 18 << 20
    for n, nz, kernel in params[:18] + params[-2:]:
        for pad in G.SLAB_STRIDE_PAD:
            slabs, prior = G.slab_case(n, nz, pad)
            assert (n + pad) % 4 == 0 and int(slabs[:, :n].abs().max()) <= 3 and nz * 3 + 50 < 2 ** 24
            assert differs(G.slab_ref(slabs, prior, n, 1, "accumulate_ignored"), G.slab_ref(slabs, prior, n, 1))
    print("slab reduce: %s" % {k: sorted({(n, nz) for n, nz, kk in params if kk == k}) for k in ("wide", "tree")})


def test_colsum_cases_straddle_the_chunk_switch():
    params = G.colsum_params()
    assert {G.colsum_rows_per_chunk(M) for _, M, _, _ in params} == {32, 128}
    assert G.colsum_rows_per_chunk(4095) == 32 and G.colsum_rows_per_chunk(4096) == 128
    assert any(pad for _, _, _, pad in params)
    for dtype, M, N, pad in params:
        assert N % 8 == 0 and (N + 2 * pad) % 8 == 0 and pad % 8 == 0 and M * 3 < 2 ** 24
        x = G.colsum_case(M, N, pad)
        assert bf16_exact(x)
        counts = G.live_counts(M)
        assert {0, 1, M} <= set(counts) and (M <= 2 or any(0 < c % G.colsum_rows_per_chunk(M) and 1 < c < M for c in counts))
        for count in counts:
            xl = G.colsum_case(M, N, pad, count)
            assert bf16_exact(xl)
            if count < M:
                assert differs(G.colsum_ref(xl, N, pad, count, "dead_rows_summed"), G.colsum_ref(xl, N, pad, count))
    print("column sums: rows per chunk %s" % {M: G.colsum_rows_per_chunk(M) for M in G.COLSUM_M})


def test_every_named_wrong_kernel_is_asserted_above():
    import inspect
    import sys
    src = inspect.getsource(sys.modules[__name__])
    for wrong in G.WRONG_KERNELS:
        assert src.count('"%s"' % wrong) >= 1, wrong


def test_report_routes_and_split_plans(capsys):
    """per family, the routes covered and the split plans found (printed past the capture, so that `pytest -q` shows it)"""
    def count(pairs):
        out = {}
        for k in pairs:
            out[k] = out.get(k, 0) + 1
        return dict(sorted(out.items()))

    lines = ["generic engine      %s" % count("%s/%s -> %s" % (l, d, G.ROUTE_OF[l](d, R, C, K)) for l, d, R, C, K in G.generic_params())]
    plans = {}
    for d, R, C, K in G.split_params():
        s, klen, live, last = G.split_plan(d, R, C, K)
        plans.setdefault(G.plan_kind((s, klen, live, last)), set()).add("%s K=%d: %d x %d, %d non-empty, last %d" % (d, K, s, klen, live, last))
    lines += ["split plans         %s: %s" % (k, sorted(v)) for k, v in sorted(plans.items())]
    lines.append("residual epilogue  %s" % count("%s -> %s" % (d, G.route_fwd(d, R, C, K)) for _, d, R, C, K, _ in G.resid_params()))
    lines.append("pixel shuffle      %s" % count("%s -> %s" % (p[0], G.route_pixshuf(p[0], *p[2:])) for p in G.pixshuf_params()))
    lines.append("GELU' epilogue     %s" % count("bf16 -> %s" % G.route_dgrad(G.BF16, R, C, K) for _, R, C, K, _ in G.DGELU_CASES))
    lines.append("GELU' column sums  %s" % count("bf16 -> %s" % G.route_dgrad(G.BF16, *c[:3]) for c in G.DGELU_CS_CASES + [G.DGELU_CS_GENERIC]))
    lines.append("GELU forward       %s" % count("bf16 -> %s" % G.route_fwd(G.BF16, R, C, K) for _, R, C, K in G.GELU_CASES))
    lines.append("slab reduce        %s" % count(k for _, _, k in G.slab_params()))
    lines.append("column sums        %s" % count("%d rows per chunk" % G.colsum_rows_per_chunk(M) for _, M, _, _ in G.colsum_params()))
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    assert len(lines) >= 12
