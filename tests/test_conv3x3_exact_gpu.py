"""The decoder's 3x3 convolution (64 -> 64, padding 1) without a tolerance: integer operands, int64 references (tests/exact_cases.py).

Every product and every partial sum is an integer fp32 holds exactly, and every expected bf16 output has magnitude <= 256
(tests/test_exact_cases_cpu.py asserts both), so the conv output in front of the tail (y3), the data gradient behind the inverse pixel
shuffle and the weight gradient must EQUAL the reference -- integer sums do not depend on the order of summation, so the weight gradient
is equal for every workgroup cap as well.  One wrong halo pixel at a 64-pixel strip boundary, a 4-row (forward) or 2-row (weight
gradient) tile boundary or between two samples is one tap of nine on a few pixels: far inside the 1e-2 gates of the tolerance tests,
and a failed equality here.  The stamp case names the tap and the channel that arrived.

pred is not exact (LayerNorm, GELU): it is checked as in the tolerance tests, against fp64 of the tail on the stored y3."""
import pytest
import torch

from tests import exact_cases as X

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from painter_amd import ops
    from painter_amd._lib import lib

DEV = "cuda"
DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}
PRED_GATE = {"bf16": 2e-3, "fp32": 2e-5}                 # test_conv64_bf16_tile_kernels / test_decoder_conv_and_tail_at_patch_14_full_size
EPS = 1e-6
CASES = [(route, kind) for route in X.CONV_ROUTES for kind in X.CONV_KINDS]


def gen(shape, seed, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).to(DEV)


def nearest_hot(case, b, h, w):
    """The hot pixel of sample b within one tap of (h, w) -> (row, col, channel, ky, kx as the FORWARD conv sees it), or None."""
    for (hb, r, c, ch) in case.hot:
        if hb == b and abs(r - h) <= 1 and abs(c - w) <= 1:
            return r, c, ch, r - h + 1, c - w + 1
    return None


def explain_nhwc(case, name, got, want, flipped):
    """The count of wrong entries of an NHWC result and the first one; in the stamp case also the tap that should have arrived there and the
    tap the value that did arrive belongs to.  flipped: the data gradient (tap 8 - tap of the forward conv)."""
    bad = got != want
    b, h, w, c = (int(v) for v in bad.nonzero()[0])
    msg = "%s: %d of %d entries wrong; first: sample %d row %d col %d channel %d: got %r, expected %r" \
        % (name, int(bad.sum()), bad.numel(), b, h, w, c, float(got[b, h, w, c]), float(want[b, h, w, c]))
    if case.kind == "stamp":
        hot = nearest_hot(case, b, h, w)
        base = 0.0 if flipped else float(case.b3[c])
        if hot is None:
            msg += "; no hot pixel within one tap: expected %s alone" % ("zero" if flipped else "the bias")
        else:
            ky, kx = (2 - hot[3], 2 - hot[4]) if flipped else (hot[3], hot[4])
            msg += "; hot pixel (row %d, col %d, channel %d) -> expected tap (ky %d, kx %d)" % (hot[0], hot[1], hot[2], ky, kx)
        msg += "; the value that arrived decodes to %s, the expected one to %s" \
            % (X.decode_stamp(float(got[b, h, w, c]) - base), X.decode_stamp(float(want[b, h, w, c]) - base))
    return msg


@pytest.mark.parametrize("route,kind", CASES, ids=["%s-%s" % c for c in CASES])
def test_conv3x3_forward_data_gradient_and_weight_gradient_equal_int64(route, kind):
    """Routes (tests/exact_cases.py, CONV_ROUTES): the bf16 tile kernels of conv64.h at 2 x 8 x 128 (two 64-pixel strips, two forward and four
    weight-gradient tile rows, two samples), the bf16 gather engine at 2 x 16 x 96 (P 16) and 2 x 28 x 56 (P 14), the fp32 build at 2 x 8 x 64."""
    tname, (B, Hi, Wi), P, tile = X.CONV_ROUTES[route]
    T = DTYPES[tname]
    Hp, Wp = Hi // P, Wi // P
    assert tile == (T == torch.bfloat16 and Hi % 4 == 0 and Wi % 64 == 0)                # c64::ok: which kernels the shape takes
    case, exp = X.conv_case(kind, B, Hi, Wi)
    x, dy, dy_w = case.x.to(T).to(DEV), case.dy.to(T).to(DEV), case.dy_w.to(T).to(DEV)
    b3 = case.b3.to(DEV)
    gamma, beta, w1, b1 = 1.0 + gen((64,), 4, 0.1), gen((64,), 5, 0.1), gen((3, 64), 6, 0.1), gen((3,), 7, 0.1)
    w3r, wf = ops.conv3x3_pack(case.w3.to(DEV), T)
    # forward: the conv output in front of the tail
    pred, y3 = ops.decoder_tail_fwd(x, w3r, b3, gamma, beta, w1, b1, EPS, save_y3=True)
    got, want = y3.double().cpu(), exp.y3.double()
    assert torch.equal(got, want), explain_nhwc(case, "y3", got, want, False)
    ref = X.tail_reference(y3, gamma, beta, w1, b1, EPS)
    e_p = float((pred.double() - ref).abs().max() / ref.abs().max())
    assert e_p < PRED_GATE[tname], e_p
    # data gradient behind the inverse pixel shuffle
    dE = ops.conv3x3_dgrad_unshuffle(dy, wf, B, Hp, Wp, P).double().cpu()
    want = X.unshuffle(exp.dx, B, Hp, Wp, P).double()
    if not torch.equal(dE, want):
        back = lambda t: t.reshape(B, Hp, Wp, P, P, 64).permute(0, 1, 3, 2, 4, 5).reshape(B, Hi, Wi, 64)
        assert torch.equal(back(dE), exp.dx.double()), explain_nhwc(case, "dgrad", back(dE), exp.dx.double(), True)
        raise AssertionError("dgrad: right values, wrong place behind the inverse pixel shuffle")
    # weight gradient, at every workgroup cap on the tile route (one tile per workgroup ... every tile in one workgroup's walk)
    want = exp.dw.double()
    saved = lib.pa_debug_get(9)
    try:
        for cap in (X.WGRAD_CAPS if tile else (0,)):
            assert lib.pa_debug_set(9, cap) == 0
            dw = ops.conv3x3_wgrad(dy_w, x).double().cpu()
            if not torch.equal(dw, want):
                bad = dw != want
                co, ci, ky, kx = (int(v) for v in bad.nonzero()[0])
                raise AssertionError("wgrad (cap %d): %d of %d entries wrong; first: cout %d cin %d tap (ky %d, kx %d): got %r, expected %r"
                                     % (cap, int(bad.sum()), bad.numel(), co, ci, ky, kx, float(dw[co, ci, ky, kx]), float(want[co, ci, ky, kx])))
    finally:
        lib.pa_debug_set(9, saved)
