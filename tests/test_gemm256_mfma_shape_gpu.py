"""The 256 x 256 bf16 GEMM (csrc/gemm256.h) under either MFMA shape of its main loop (G256_MFMA16_MASK: 32x32x16 or 16x16x32 per
family), checked WITHOUT a tolerance: operands with entries in {-1, 0, 1} and contraction lengths of 128 / 256 make every product and
every partial sum an integer of magnitude <= 256 -- exact in fp32 and in bf16 -- so the result must EQUAL an int64 matmul, whatever
the grouping of the sums.  A fragment read from the wrong row block, a k-step paired with the wrong k-step of the other operand or an
accumulator quarter staged to the wrong place of the epilogue moves integers around and cannot hide in a bf16 tolerance.

Shapes are (rows, columns, contraction) of the OUTPUT, the same for the three layouts:
    forward          x [rows, c] . w [columns, c]^T           K-major x K-major
    data gradient    dy [rows, c] . w [c, columns]            K-major x M-major
    weight gradient  dy [c, rows]^T . x [c, columns]          M-major x M-major   (fp32 output)
(256, 256, 128) is one tile and the shortest loop the kernel runs (two K tiles), (328, 264, 256) has ragged rows and columns (clamped
operand rows, masked stores; its weight gradient is outside the kernel's shapes -- rows and columns must be multiples of 256 there -- and
runs on the generic engine, where the same equality holds), (512, 512, 128) has several tiles per wave row and wave column.
The weight gradient's K split follows from the contraction length at these sizes (at most a quarter of the K tiles, gemm.hip:
wgrad_fast_splits): 128 and 256 give one split at every value of knob 3; a contraction of 512 -- sums <= 512, still exact in the
fp32 output -- gives two, at both values of the knob too.

The last test repeats the fp64 gates of test_kernels_gpu.py::test_gemm256_bf16_tight_gates_against_fp64 (5e-6 sqrt(K) for fp32 outputs,
2^-8 for bf16 outputs) on random operands, per layout.

tests/test_gemm_exact_gpu.py does the same for what this file leaves out: the generic engine, split plans, the other epilogues, the reductions."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from painter_amd import ops
    from painter_amd._lib import EPI_BIAS, EPI_BIAS_F32, lib

DEV = "cuda"
BF = torch.bfloat16
SHAPES = [(256, 256, 128), (328, 264, 256), (512, 512, 128)]


def tern(shape, seed):
    """int64 entries in {-1, 0, 1} (a third each)"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 3, shape, generator=g) - 1).to(DEV)


def imm(a, b):
    """the int64 product (on the host: the device has no integer matmul), back on the device"""
    return (a.cpu() @ b.cpu()).to(DEV)


def bias_int(n, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 17, (n,), generator=g) - 8).to(DEV)


def exact(out, ref, what):
    """out (bf16 / fp32) must hold exactly the integers of ref (int64); names the first element that does not"""
    assert int(ref.abs().max()) <= 256, "test operands: the reference leaves the exact range of bf16"
    got = out.double().to(torch.int64)
    if torch.equal(got, ref) and torch.equal(got.double(), out.double()):
        return
    bad = (out.double() != ref.double()).nonzero()
    i, j = (int(v) for v in bad[0])
    raise AssertionError("%s: %d of %d elements differ, first at (%d, %d): got %r, want %d; rows hit %s, columns hit %s"
                         % (what, bad.shape[0], ref.numel(), i, j, float(out[i, j]), int(ref[i, j]),
                            sorted(set(bad[:, 0].tolist()))[:8], sorted(set(bad[:, 1].tolist()))[:8]))


def fwd_case(R, C, K, seed=0, **kw):
    x, w, b = tern((R, K), seed + 1), tern((C, K), seed + 2), bias_int(C, seed + 3)
    ref = imm(x, w.t()) + b
    for epi in (EPI_BIAS_F32, EPI_BIAS):
        out = ops.linear_fwd(x.to(BF), w.to(BF), b.float(), epi, **kw)
        assert out.dtype == (torch.float32 if epi == EPI_BIAS_F32 else BF)
        exact(out, ref, "forward %s epilogue %d" % ((R, C, K), epi))


def dgrad_case(R, C, K, seed=0):
    dy, w = tern((R, K), seed + 4), tern((K, C), seed + 5)
    exact(ops.linear_dgrad(dy.to(BF), w.to(BF)), imm(dy, w), "data gradient %s" % ((R, C, K),))


def wgrad_case(R, C, K, seed=0):
    dy, x = tern((K, R), seed + 6), tern((K, C), seed + 7)
    ref = imm(dy.t(), x)
    saved = lib.pa_debug_get(3)
    try:
        for target in (16, 256):
            lib.pa_debug_set(3, target)
            out = ops.linear_wgrad(dy.to(BF), x.to(BF))
            assert out.dtype == torch.float32
            exact(out, ref, "weight gradient %s, knob 3 = %d" % ((R, C, K), target))
    finally:
        lib.pa_debug_set(3, saved)


@pytest.mark.parametrize("R,C,K", SHAPES)
def test_exact_integer_forward(R, C, K):
    fwd_case(R, C, K)


@pytest.mark.parametrize("R,C,K", SHAPES)
def test_exact_integer_data_gradient(R, C, K):
    dgrad_case(R, C, K)


@pytest.mark.parametrize("R,C,K", SHAPES + [(256, 256, 512), (512, 512, 512)])
def test_exact_integer_weight_gradient(R, C, K):
    """(contraction 512: two K splits + the slab sum)"""
    wgrad_case(R, C, K)


def coded(K):
    """w_k [K]: the k index as a bf16-exact integer, k - K / 2"""
    return torch.arange(K, device=DEV) - K // 2


@pytest.mark.parametrize("R,C,K", SHAPES)
def test_position_coded_operand(R, C, K):
    """One 1 per row of the first operand, at contraction index (7 i) % K of row i: output row i must be that k's slice of the other operand,
    whose entries are +- (k - K / 2) (sign by the other index, so that a transposed result does not pass): a wrong element NAMES the k index
    that reached its lane instead."""
    def hot(rows):
        m = torch.zeros((rows, K), dtype=torch.int64, device=DEV)
        idx = (7 * torch.arange(rows, device=DEV)) % K
        m[torch.arange(rows, device=DEV), idx] = 1
        return m, idx

    def check(out, idx, sign, what):
        want = sign[None, :] * coded(K)[idx][:, None]
        got = out.double().to(torch.int64)
        if torch.equal(got, want):
            return
        bad = (got != want).nonzero()
        i, j = (int(v) for v in bad[0])
        raise AssertionError("%s %s: %d elements differ; first: output (%d, %d) should take k = %d and holds the value of k = %d (sign %+d)"
                             % (what, (R, C, K), bad.shape[0], i, j, int(idx[i]), int(got[i, j]) * int(sign[j]) + K // 2,
                                int(sign[j])))

    sign = 1 - 2 * (torch.arange(C, device=DEV) % 2)
    x, idx = hot(R)
    w = sign[:, None] * coded(K)[None, :]                                 # [C, K]
    check(ops.linear_fwd(x.to(BF), w.to(BF), torch.zeros(C, device=DEV), EPI_BIAS_F32), idx, sign, "forward")
    check(ops.linear_dgrad(x.to(BF), w.t().contiguous().to(BF)), idx, sign, "data gradient")
    dyT, idx = hot(R)                                                     # dy [K, R] = its transpose: one 1 per COLUMN of dy
    check(ops.linear_wgrad(dyT.t().contiguous().to(BF), w.t().contiguous().to(BF)), idx, sign, "weight gradient")


def test_exact_integer_tile_variants():
    """The other instantiations of the forward and data-gradient families on the same kind of operands: 224-row tiles (knob 4 = 2, 448 rows),
    a forced mixed plan (knobs 12 = 2 and 14 = 1, 384 rows = one full tile + one half tile), and a skipped row tile (512 rows, 256 per sample,
    sample 1 dropped: its rows must be the epilogue of a zero accumulator -- the bias -- although its operand rows are not zero)."""
    saved = {k: lib.pa_debug_get(k) for k in (4, 12, 14)}
    try:
        lib.pa_debug_set(4, 2)
        fwd_case(448, 256, 128, seed=10)
        dgrad_case(448, 256, 128, seed=10)
        lib.pa_debug_set(4, saved[4])
        lib.pa_debug_set(12, 2)
        lib.pa_debug_set(14, 1)
        fwd_case(384, 256, 128, seed=20)
        dgrad_case(384, 256, 128, seed=20)
        fwd_case(640, 256, 128, seed=25)         # (a mixed plan needs >= 512 rows, gemm256.h tile_plan: one full tile + three half tiles)
        dgrad_case(640, 256, 128, seed=25)
    finally:
        for k, v in saved.items():
            lib.pa_debug_set(k, v)
    # (256-row tiles, knob 4 = 1: the tile rule would take 224-row tiles here, whose second tile holds rows of both samples and is computed)
    R, C, K, rps = 512, 256, 128, 256
    f = torch.tensor([1.0, 0.0], device=DEV)
    x, w, b = tern((R, K), 31), tern((C, K), 32), bias_int(C, 33)
    ref = imm(x, w.t()) + b
    ref[rps:] = b
    dy, wd = tern((R, K), 34), tern((K, C), 35)
    dy[rps:] = 0                                                          # (the contract of the data gradient: dY rows of a dropped sample are zero)
    try:
        lib.pa_debug_set(4, 1)
        # (the bf16 bias epilogue: the fp32 one has no skipping route)
        exact(ops.linear_fwd(x.to(BF), w.to(BF), b.float(), EPI_BIAS, rowskip=f, skip_rows_per_sample=rps), ref, "forward, sample 1 skipped")
        exact(ops.linear_dgrad(dy.to(BF), wd.to(BF), rowskip=f, rows_per_sample=rps), imm(dy, wd), "data gradient, sample 1 skipped")
    finally:
        lib.pa_debug_set(4, saved[4])


def _rel64(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def gen(shape, seed, scale=1.0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype).to(DEV)


def test_random_operands_against_fp64():
    """(3136, 3072, 1024) as test_kernels_gpu.py reads it -- x [M, K], w [N, K], dy [M, N] -- with other seeds; the weight gradient also over
    3200 rows, a contraction length the 256 x 256 kernel takes (a multiple of 128; 3136 is not and runs on the generic engine)."""
    M, N, K = 3136, 3072, 1024
    x, w, b = gen((M, K), 41, 1.0, BF), gen((N, K), 42, 0.05, BF), gen((N,), 43)
    ref = x.double() @ w.double().t() + b.double()
    errs = {}
    errs["bias_bf16"] = _rel64(ops.linear_fwd(x, w, b, EPI_BIAS), ref)
    errs["bias_f32"] = _rel64(ops.linear_fwd(x, w, b, EPI_BIAS_F32), ref)
    dy = gen((M, N), 44, 1.0, BF)
    errs["dgrad_bf16"] = _rel64(ops.linear_dgrad(dy, w), dy.double() @ w.double())
    errs["wgrad_f32"] = _rel64(ops.linear_wgrad(dy, x), dy.double().t() @ x.double())
    dy2, x2 = gen((3200, N), 45, 1.0, BF), gen((3200, K), 46, 1.0, BF)
    errs["wgrad_3200_f32"] = _rel64(ops.linear_wgrad(dy2, x2), dy2.double().t() @ x2.double())
    print("gemm256 mfma shape, random operands, measured:", {k: "%.2e" % v for k, v in errs.items()})
    f32_gate, bf16_gate = 5e-6 * math.sqrt(K), 2.0 ** -8
    for k, v in errs.items():
        assert v < (f32_gate if k.endswith("f32") else bf16_gate), (k, errs)
