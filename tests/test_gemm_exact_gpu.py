"""The linear layers' kernels WITHOUT a tolerance (csrc/gemm.hip): the generic MFMA engine in both dtypes and all three layouts with ragged
rows, columns and K tails; its split-K weight gradient with ragged and empty splits; the residual, pixel-shuffle and GELU' epilogues on both
engines; the column sums of the GELU' epilogue; pa_slab_reduce, pa_colsum and pa_colsum_live.  Every case is built in
tests/gemm_exact_cases.py from integers, so the kernels' results must EQUAL the int64 (or fp64-exact) references there, whatever the
grouping of the sums; tests/test_gemm_exact_cases_cpu.py proves, without a GPU, the conditions that rests on and the engine every case
reaches.  This file only runs kernels and compares.  Outputs a kernel must fully overwrite are pre-filled with NaN.

The GELU forward epilogue has no bit reference (the function value is an approximation): on integer pre-activations its act and aux must be
FUNCTIONS of the pre-activation -- equal bits wherever the integer is equal -- and lie within the project's gates of fp64 GELU / GELU'."""
import math

import pytest
import torch

from tests import gemm_exact_cases as G

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from painter_amd import ops
    from painter_amd._lib import EPI_BIAS, EPI_BIAS_F32, EPI_BIAS_GELU, EPI_BIAS_RESID, check, lib

DEV = "cuda"
TD = {G.BF16: torch.bfloat16, G.F32: torch.float32}
NAN = float("nan")


def dev(t, dtype=None):
    return t.to(DEV) if dtype is None else t.to(dtype).to(DEV)


def nans(shape, dtype):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


def exact(out, ref, what, case=None):
    """out must hold exactly the numbers of ref (int64 / fp64 / bf16, on the host); names the first element that does not, the rows and
    columns hit and -- position-coded operands -- the contraction index the wrong element names"""
    got, want = out.detach().cpu().double(), ref.double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    got, want = got.reshape(-1, got.shape[-1]), want.reshape(-1, want.shape[-1])
    if torch.equal(got, want):
        return
    bad = (got != want).nonzero()
    i, j = (int(v) for v in bad[0])
    msg = "%s: %d of %d elements differ, first at (%d, %d): got %r, want %r; rows hit %s, columns hit %s" \
          % (what, bad.shape[0], want.numel(), i, j, float(got[i, j]), float(want[i, j]), sorted(set(bad[:, 0].tolist()))[:8],
             sorted(set(bad[:, 1].tolist()))[:8])
    if case is not None and case.get("idx") is not None and got.shape[0] == case["idx"].numel() and math.isfinite(float(got[i, j])):
        msg += "; the element should take k = %d and holds the value of k = %d" % (int(case["idx"][i]), G.named_k(case, i, j, got[i, j]))
    raise AssertionError(msg)


class knobs:
    """pa_debug_set knobs, restored on exit"""
    def __init__(self, values):
        self.values = values

    def __enter__(self):
        self.saved = {k: lib.pa_debug_get(k) for k in self.values}
        for k, v in self.values.items():
            check(lib.pa_debug_set(k, v), "pa_debug_set")

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            lib.pa_debug_set(k, v)


def poison_wgrad_workspace(T, K, R, C):
    """NaN in the slab workspace the next ops.linear_wgrad of this shape uses: every slab, an empty split's too, must be written"""
    nbytes = lib.pa_linear_wgrad_workspace_bytes(ops.code(T), K, R, C)
    ws = ops.workspace(nbytes, torch.device(DEV, torch.cuda.current_device()))
    ws.view(torch.float32).fill_(NAN)


def run_layout(layout, dtype, case, what):
    """the logical case on one layout, every epilogue that is a plain sum; compares with the reference"""
    T = TD[dtype]
    a, b = case["a"], case["b"]
    R, K = a.shape
    C = b.shape[1]
    ref = G.gemm_ref(case)
    if layout == "fwd":
        x, w = dev(a, T), dev(b.t().contiguous(), T)
        bias = torch.zeros(C, device=DEV) if case["bias"] is None else dev(case["bias"], torch.float32)
        for epi, odt in ((EPI_BIAS_F32, torch.float32), (EPI_BIAS, T)):
            out = ops.linear_fwd(x, w, bias, epi, out=nans((R, C), odt))
            exact(out, ref, "%s forward %s epilogue %d" % (what, dtype, epi), case)
    elif layout == "dgrad":
        out = ops.linear_dgrad(dev(a, T), dev(b, T), out=nans((R, C), T))
        exact(out, ref, "%s data gradient %s" % (what, dtype), case)
    else:
        poison_wgrad_workspace(T, K, R, C)
        out = ops.linear_wgrad(dev(a.t().contiguous(), T), dev(b, T), out=nans((R, C), torch.float32))
        exact(out, ref, "%s weight gradient %s, plan %s" % (what, dtype, G.split_plan(dtype, R, C, K)), case)


# ------------------------------------------------------------------------------------------------ 1. the generic engine
@pytest.mark.parametrize("layout,dtype,R,C,K", G.generic_params(), ids=lambda v: str(v))
def test_generic_engine_exact(layout, dtype, R, C, K):
    for kind in ("tern", "coded"):
        run_layout(layout, dtype, G.gemm_case(layout, R, C, K, kind), "%s %s" % (kind, (R, C, K)))


# ------------------------------------------------------------------------------------------------ 2. split-K weight gradient
@pytest.mark.parametrize("dtype,R,C,K", G.split_params(), ids=lambda v: str(v))
def test_generic_weight_gradient_split_plans(dtype, R, C, K):
    run_layout("wgrad", dtype, G.gemm_case("wgrad", R, C, K), "tern %s" % ((R, C, K),))


@pytest.mark.parametrize("dtype", G.DTYPES)
@pytest.mark.parametrize("R,C,K", G.SPLIT_CODED)
def test_generic_weight_gradient_position_coded(dtype, R, C, K):
    """a wrong element names the group of 32 contraction indices that reached it, hence the split"""
    run_layout("wgrad", dtype, G.gemm_case("wgrad", R, C, K, "coded"), "coded %s" % ((R, C, K),))


# ------------------------------------------------------------------------------------------------ 3. residual epilogue
def run_resid(dtype, case, what, **kw):
    T = TD[dtype]
    R, C = case["resid"].shape
    resid = dev(case["resid"], torch.float32)
    rs = dev(case["rowscale"], torch.float32)
    out = ops.linear_fwd(dev(case["a"], T), dev(case["b"].t().contiguous(), T), dev(case["bias"], torch.float32), EPI_BIAS_RESID,
                         out=nans((R, C), torch.float32), resid=resid, rowscale=rs, rows_per_sample=case["rps"], **kw)
    exact(out, G.resid_ref(case), what)
    dropped = dev((case["rowscale"] == 0)[torch.arange(R) // case["rps"]])
    assert bool(dropped.any())
    assert torch.equal(out[dropped].view(torch.int32), resid[dropped].view(torch.int32)), what + ": dropped rows are not the bits of resid"


@pytest.mark.parametrize("route,dtype,R,C,K,rps", G.resid_params(), ids=lambda v: str(v))
def test_residual_epilogue_exact(route, dtype, R, C, K, rps):
    run_resid(dtype, G.resid_case(R, C, K, rps), "residual epilogue %s %s rps %d (%s)" % (dtype, (R, C, K), rps, route))


@pytest.mark.parametrize("scales", G.RESID_SKIP_SCALES, ids=lambda v: str(v))
def test_residual_epilogue_under_tile_skip(scales):
    """512 rows, 256 per sample, sample 1 dropped, 256-row tiles: its tile runs the epilogue alone, on a zero accumulator"""
    R, C, K, rps = G.RESID_SKIP
    case = G.resid_case(R, C, K, rps, tuple(scales))
    with knobs({4: 1, 16: 2}):
        run_resid(G.BF16, case, "residual epilogue, sample 1 skipped, factors %s" % (scales,), rowskip=dev(case["rowscale"], torch.float32),
                  skip_rows_per_sample=rps)


# ------------------------------------------------------------------------------------------------ 4. pixel shuffle
@pytest.mark.parametrize("dtype,kind,B,Hp,Wp,P,C,K", G.pixshuf_params(), ids=lambda v: str(v))
def test_pixel_shuffle_exact(dtype, kind, B, Hp, Wp, P, C, K):
    T = TD[dtype]
    case = G.pixshuf_case(kind, B, Hp, Wp, P, C, K)
    x, w, bias = dev(case["a"], T), dev(case["b"].t().contiguous(), T), dev(case["bias"], torch.float32)
    out = nans((B, Hp * P, Wp * P, C), T)
    check(lib.pa_linear_pixshuf(ops.code(T), ops.p(x), x.stride(0), ops.p(w), ops.p(bias), ops.p(out), B, Hp, Wp, P, C, K, ops.stream()),
          "pa_linear_pixshuf")
    ref = G.pixshuf_ref(case, B, Hp, Wp, P, C)
    what = "pixel shuffle %s %s %s" % (dtype, kind, (B, Hp, Wp, P, C, K))
    if kind == "coded" and not torch.equal(out.cpu().double(), ref.double()):
        # which token row's k arrived: |value| names k, the token is the one whose one-hot index that is
        got = out.cpu().double()
        bad = (got != ref.double()).nonzero()
        y, xx, c = (int(v) for v in bad[0][1:])
        b0 = int(bad[0][0])
        tok = (b0 * Hp + (y % (Hp * P)) // P) * Wp + xx // P
        what += ": image (%d, %d, %d, %d) = token %d (p, q) = (%d, %d) should take k = %d, holds |code| %s" \
                % (b0, y, xx, c, tok, y % P, xx % P, int(case["idx"][tok]), float(got[tuple(bad[0].tolist())]))
    exact(out, ref, what)
    exact(ops.linear_pixshuf(x, w, bias, B, Hp, Wp, P, C), ref, what + " (ops.linear_pixshuf)")


# ------------------------------------------------------------------------------------------------ 5. GELU' from the 8-bit code
def padded_pair(case):
    """-> (out bf16 [R, C] NaN, aux uint8 [R, C], the two buffers): column-slice views of [R, C + pad] buffers"""
    R, C = case["aux"].shape
    ld = C + case["pad"]
    obuf = nans((R, ld), torch.bfloat16)
    abuf = torch.full((R, ld), 255, dtype=torch.uint8, device=DEV)
    abuf[:, :C] = dev(case["aux"])
    return obuf[:, :C], abuf[:, :C], obuf


@pytest.mark.parametrize("with_colsum", [False, True], ids=["plain", "colsum"])
@pytest.mark.parametrize("route,R,C,K,pad", G.DGELU_CASES, ids=lambda v: str(v))
def test_dgelu_epilogue_exact(route, R, C, K, pad, with_colsum):
    case = G.dgelu_case(R, C, K, pad)
    out, aux, obuf = padded_pair(case)
    cs = nans((C,), torch.float32) if with_colsum else None
    got = ops.linear_dgrad(dev(case["a"], torch.bfloat16), dev(case["b"], torch.bfloat16), gelu_aux=aux, out=out, colsum_out=cs)
    assert got.data_ptr() == out.data_ptr()
    exact(out, G.dgelu_ref(case), "GELU' epilogue %s pad %d (%s)%s" % ((R, C, K), pad, route, ", with column sums" if with_colsum else ""))
    if pad:
        assert bool(torch.isnan(obuf[:, C:]).all()), "the columns between the row pitch and the width were written"
    if with_colsum:      # dense dY: the order of the sums is the kernel's; what they must be is one fp32 rounding per term away from the fp64 sum
        # (R fp32 additions: |error| <= R 2^-24 sum |term| per column; the generic route sums the bf16 values it stored)
        terms = G.dgelu_ref(case, stored=route == "generic").double()
        assert bool(((cs.cpu().double() - terms.sum(0)).abs() <= R * 2.0 ** -24 * terms.abs().sum(0)).all())


def run_dgelu_colsum(R, C, K, rows, what, from_stored=False):
    w = dev(G.dgelu_case(R, C, K)["b"], torch.bfloat16)
    for r in rows:
        case = G.dgelu_case(R, C, K, 0, r)
        out, aux, _ = padded_pair(case)
        cs = nans((C,), torch.float32)
        ops.linear_dgrad(dev(case["a"], torch.bfloat16), w, gelu_aux=aux, out=out, colsum_out=cs)
        exact(out, G.dgelu_ref(case), "%s, dy row %d alone: dX" % (what, r))
        exact(cs[None], G.dgelu_colsum_ref(case, r, from_stored=from_stored)[None], "%s, dy row %d alone: column sums" % (what, r))


@pytest.mark.parametrize("R,C,K,kn,rows", G.DGELU_CS_CASES, ids=lambda v: str(v))
def test_dgelu_column_sums_exact(R, C, K, kn, rows):
    """one non-zero dY row: every partial sum of Epi4DGeluCS is fmaf(v, g, 0) = float32(v g) plus zeros"""
    with knobs({4: 0, 12: 0, 14: 0, **kn}):
        run_dgelu_colsum(R, C, K, rows, "GELU' column sums %s knobs %s" % ((R, C, K), kn))


def test_dgelu_column_sums_generic_route():
    """EpiDGelu<bf16>, then pa_colsum over the stored bf16 rows: the sums are the stored values of the one non-zero row"""
    R, C, K, rows = G.DGELU_CS_GENERIC
    run_dgelu_colsum(R, C, K, rows, "GELU' column sums %s generic" % ((R, C, K),), from_stored=True)


# ------------------------------------------------------------------------------------------------ 6. GELU forward
@pytest.mark.parametrize("route,R,C,K", G.GELU_CASES, ids=lambda v: str(v))
def test_gelu_epilogue_is_a_function_of_the_pre_activation(route, R, C, K):
    """Integer pre-activations (ternary operands, integer bias), each value at many (row, column) places.  Tolerance-free: act and the
    8-bit code are functions of the pre-activation alone, so all places that hold the same integer hold the same bits -- a lane- or
    pair-dependent error in gelu_both2 / gelu_fast2 / gelu_parts or in the byte packing breaks that.  Then, per distinct value, against fp64:
    act within 2^-8 of the value + 4e-7 |x| (gemm_exact_cases.GELU_ACT_*), the decoded code within half a step + 1e-5.
    need_aux=False must return the same act bits: on the generic engine it is the same code without the aux store; on the 256 x 256 kernel
    gelu_fast2 replaces gelu_both2, and both take x * cdf from the one gelu_parts2 (common.h), so they are meant to agree bit for bit."""
    case = G.gemm_case("fwd", R, C, K)
    x, w, bias = dev(case["a"], torch.bfloat16), dev(case["b"].t().contiguous(), torch.bfloat16), dev(case["bias"], torch.float32)
    pre = G.gemm_ref(case)
    act = nans((R, C), torch.bfloat16)
    aux = torch.zeros((R, C), dtype=torch.uint8, device=DEV)
    ops.linear_fwd(x, w, bias, EPI_BIAS_GELU, out=act, out2=aux)
    act2 = nans((R, C), torch.bfloat16)
    ops.linear_fwd(x, w, bias, EPI_BIAS_GELU, out=act2, out2=None)
    exact(ops.linear_fwd(x, w, bias, EPI_BIAS), pre, "the pre-activation itself")
    vals, inv = pre.reshape(-1).unique(return_inverse=True)
    abits, codes = act.cpu().view(torch.int16).reshape(-1).long(), aux.cpu().reshape(-1).long()
    for name, v in (("act", abits), ("aux", codes)):
        rep = torch.zeros(vals.numel(), dtype=torch.int64).scatter(0, inv, v)          # one member's bits per value
        bad = (v != rep[inv]).nonzero()
        assert bad.numel() == 0, "%s %s: %s is no function of the pre-activation: %d places, first (%d, %d) with pre %d" \
            % (route, (R, C, K), name, bad.shape[0], int(bad[0]) // C, int(bad[0]) % C, int(pre.reshape(-1)[bad[0]]))
    assert torch.equal(act2.view(torch.int16), act.view(torch.int16)), "need_aux=False changes act (%s)" % route
    first = torch.zeros(vals.numel(), dtype=torch.int64).scatter(0, inv, torch.arange(inv.numel()))
    a_val = act.cpu().reshape(-1)[first].double()
    g_val = ops.gelu_aux_decode(aux.reshape(-1)[dev(first)]).cpu().double()
    gelu, dgelu = G.gelu_fp64(vals)
    err_a, gate_a = (a_val - gelu).abs(), G.GELU_ACT_REL * gelu.abs() + G.GELU_ACT_CDF_ABS * vals.double().abs()
    worst = int((err_a / gate_a.clamp_min(1e-300)).argmax())
    rel = float((err_a / gelu.abs().clamp_min(1e-300))[gelu.abs() > 1e-3].max())
    err_g = float((g_val - dgelu).abs().max())
    print("GELU forward %s (%s): %d distinct pre-activations in [%d, %d]; act: largest error %.3e of the value (where |gelu| > 1e-3; gate 2^-8 "
          "= %.3e), largest share of its gate at pre %d: |err| %.3e against %.3e; tensor-wide %.3e of max |gelu| (gate 2^-8); decoded aux: largest "
          "|err| %.3e (gate %.3e)" % ((R, C, K), route, vals.numel(), int(vals.min()), int(vals.max()), rel, G.GELU_ACT_REL, int(vals[worst]),
                                     float(err_a[worst]), float(gate_a[worst]), float(err_a.max() / gelu.abs().max()), err_g, G.GELU_AUX_ABS))
    assert bool((err_a <= gate_a).all()), (int(vals[worst]), float(err_a[worst]), float(gate_a[worst]))
    assert float(err_a.max() / gelu.abs().max()) < 2.0 ** -8
    assert err_g < G.GELU_AUX_ABS


# ------------------------------------------------------------------------------------------------ 7. reductions
@pytest.mark.parametrize("n,nz,kernel", G.slab_params(), ids=lambda v: str(v))
def test_slab_reduce_exact(n, nz, kernel):
    for pad in G.SLAB_STRIDE_PAD:
        slabs, prior = G.slab_case(n, nz, pad)
        src = dev(slabs, torch.float32)
        for acc in (0, 1):
            out = dev(prior, torch.float32) if acc else nans((n,), torch.float32)
            assert lib.pa_slab_reduce(src.data_ptr(), out.data_ptr(), n, nz, n + pad, acc, ops.stream()) == 0
            exact(out[None], G.slab_ref(slabs, prior, n, acc)[None], "slab reduce n %d nz %d stride %d accumulate %d (%s kernel)" % (n, nz, n + pad, acc, kernel))


@pytest.mark.parametrize("dtype,M,N,pad", G.colsum_params(), ids=lambda v: str(v))
def test_column_sums_exact(dtype, M, N, pad):
    T = TD[dtype]
    x = G.colsum_case(M, N, pad)
    xd = dev(x, T)[:, pad:pad + N]
    assert xd.stride(0) == N + 2 * pad
    exact(ops.colsum(xd, out=nans((N,), torch.float32))[None], G.colsum_ref(x, N, pad)[None], "column sums %s %s pad %d" % (dtype, (M, N), pad))
    for count in G.live_counts(M):
        x = G.colsum_case(M, N, pad, count)
        xd = dev(x, T)[:, pad:pad + N]
        cnt = torch.tensor([count], dtype=torch.int32, device=DEV)
        exact(ops.colsum_live(xd, cnt, out=nans((N,), torch.float32))[None], G.colsum_ref(x, N, pad, count)[None],
              "column sums of the first %d rows %s %s pad %d" % (count, dtype, (M, N), pad))
