"""Operands for which the linear layers' kernels (csrc/gemm.hip: the generic MFMA engine of csrc/gemm_engine.h, the 256 x 256 bf16 kernel of
csrc/gemm256.h, their fused epilogues, the slab and column-sum reductions) have an EXACT answer, built on the CPU in plain torch / numpy.

Everything is an integer (or a half-integer, or one documented rounding of an exact product): entries in {-1, 0, 1}, integer biases in
[-8, 8], position-coded operands whose wrong elements name the contraction index that reached them.  References are int64 matmuls; the
GELU' epilogue's reference is the kernel's documented arithmetic evaluated in fp64, where it is exact, and rounded as the kernel rounds.

Shapes are (rows, columns, contraction) of the OUTPUT, as in tests/test_gemm256_mfma_shape_gpu.py; a case is held in its LOGICAL form
a [rows, contraction], b [contraction, columns] and laid out per call by the GPU file:
    forward          x = a, w = b^T             data gradient    dy = a, w = b             weight gradient  dy = a^T, x = b   (fp32 output)

The route tables say which engine a shape must reach; route_*() below are Python copies of the C++ rules (g256::ok, wgrad_fast,
wgrad_splits + launch_gemm's klen, pa_slab_reduce's kernel choice, colsum_rows_per_chunk) and tests/test_gemm_exact_cases_cpu.py asserts
every claim with them, together with the exactness conditions, without a GPU.  Every reference takes an optional wrong= naming one
defect (WRONG_KERNELS); the CPU test asserts that the cases see each of them.

The parametrisations of tests/test_gemm_exact_gpu.py live here."""
import functools
from fractions import Fraction

import numpy as np
import torch

from tests.exact_cases import _sign

BF16, F32 = "bf16", "fp32"
DTYPES = (BF16, F32)
ENGINE_BK = {BF16: 64, F32: 32}          # K elements of one tile of the generic engine (common.h: TT<T>::BK)

WRONG_KERNELS = ("k_tail_dropped", "last_split_dropped", "empty_split_reads_first", "bias_halves_swapped", "rowscale_by_128",
                 "pq_swapped", "aux_pitch_doubled", "old_decode", "dead_rows_summed", "accumulate_ignored")


# ------------------------------------------------------------------------------------------------ the C++ rules, in Python
def g256_ok(M, N, K, amm, bmm, lda, ldb):
    """gemm256.h: ok() (without its 4 GiB operand bound, which nothing here approaches)."""
    if K % 128 or M < 8 or N < 8 or N % 8:
        return False
    if (amm and M % 8) or (bmm and N % 8):
        return False
    return lda % 8 == 0 and ldb % 8 == 0


def route_fwd(dtype, R, C, K):
    """linear_fwd_t / linear_pixshuf_t (without the latter's C % 8 rule): x [R, K] . w [C, K]^T, both contiguous."""
    return "g256" if dtype == BF16 and g256_ok(R, C, K, False, False, K, K) else "generic"


def route_dgrad(dtype, R, C, K):
    """linear_dgrad_t: dy [R, K] . w [K, C], both contiguous."""
    return "g256" if dtype == BF16 and g256_ok(R, C, K, False, True, K, C) else "generic"


def wgrad_fast(dtype, R, C, K):
    """gemm.hip: wgrad_fast for dy [K, R], x [K, C] contiguous."""
    return dtype == BF16 and g256_ok(R, C, K, True, True, R, C) and C % 4 == 0 and R % 256 == 0 and C % 256 == 0


def route_wgrad(dtype, R, C, K):
    return "g256" if wgrad_fast(dtype, R, C, K) else "generic"


def wgrad_splits(contraction, rows, cols, bk):
    """gemm.hip: wgrad_splits(M, N, K, bk) with M the contraction length"""
    tiles = ((rows + 127) // 128) * ((cols + 127) // 128)
    nku = (contraction + bk - 1) // bk
    return max(1, min((640 + tiles - 1) // tiles, nku, 64))


def split_plan(dtype, R, C, K):
    """-> (splits, klen, non-empty splits, length of the last non-empty split) of the generic weight gradient: wgrad_splits, then
    launch_gemm's klen = ceil(K tiles / splits) K tiles; split z contracts [z klen, min(K, (z + 1) klen))."""
    bk = ENGINE_BK[dtype]
    s = wgrad_splits(K, R, C, bk)
    nku = (K + bk - 1) // bk
    klen = ((nku + s - 1) // s) * bk
    live = min(s, (K + klen - 1) // klen)
    return s, klen, live, K - (live - 1) * klen


def plan_kind(plan):
    s, klen, live, last = plan
    if s == 1:
        return "single"
    if live < s:
        return "empty_splits"
    return "all_full" if last == klen else "ragged_last"


def slab_kernel(n, nz):
    """pa_slab_reduce: "wide" = slab_reduce_wide_kernel (one float4 per thread), "tree" = slab_reduce_kernel (16 z-lanes through LDS)"""
    return "wide" if nz <= 16 and n >= (1 << 18) else "tree"


def colsum_rows_per_chunk(M):
    return 128 if M >= 4096 else 32


# ------------------------------------------------------------------------------------------------ operands
def tern(shape, seed):
    """int64 entries in {-1, 0, 1} (a third each)"""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 3, shape, generator=g) - 1


def bias_int(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 17, (n,), generator=g) - 8


def code_group(K):
    """contraction indices per code value of a position-coded operand: 1 up to K = 256, a power of two beyond (4100 -> 32, which divides
    the split lengths 128 and 96 of that contraction: a code names its split)"""
    g = 1
    while K > 256 * g:
        g *= 2
    return g


def coded(K):
    """[K]: the k index (its group of code_group(K) indices) as a bf16-exact integer around zero"""
    g = code_group(K)
    return torch.arange(K) // g - (K // g) // 2


def hot(rows, K):
    """-> (a [rows, K] with one 1 per row, idx [rows]): at contraction index (7 i) % K; a long contraction (7 rows < K) is stepped through
    in K // rows + 1, the last row at K - 1, so that the rows reach every split of it (the last one may be a few indices short)"""
    step = 7 if 7 * rows >= K or K <= 256 else K // rows + 1
    idx = (step * torch.arange(rows)) % K
    if step != 7:
        idx[-1] = K - 1
    a = torch.zeros((rows, K), dtype=torch.int64)
    a[torch.arange(rows), idx] = 1
    return a, idx


def col_sign(C):
    return 1 - 2 * (torch.arange(C) % 2)


def contract(a, b, dtype=None, plan=None, wrong=None):
    """int64 a [R, K] . b [K, C]; wrong: what a kernel with that defect would return"""
    K = a.shape[1]
    if wrong == "k_tail_dropped":                       # the K tail behind the last full K tile
        kf = K // ENGINE_BK[dtype] * ENGINE_BK[dtype]
        return a[:, :kf] @ b[:kf]
    if wrong == "last_split_dropped":
        _, klen, live, _ = plan
        return a[:, :(live - 1) * klen] @ b[:(live - 1) * klen]
    if wrong == "empty_split_reads_first":
        s, klen, live, _ = plan
        return a @ b + (s - live) * (a[:, :klen] @ b[:klen])
    assert wrong is None, wrong
    return a @ b


@functools.lru_cache(maxsize=None)
def gemm_case(layout, R, C, K, kind="tern"):
    """-> dict(a [R, K], b [K, C], bias [C] or None, idx): the logical operands.  kind "coded": a has one 1 per row, b[k][c] = +- code(k),
    the sign by the column (a transposed result does not pass), so output row i holds the code of idx[i]."""
    seed = {"fwd": 1, "dgrad": 4, "wgrad": 6}[layout]
    if kind == "coded":
        a, idx = hot(R, K)
        return dict(a=a, b=coded(K)[:, None] * col_sign(C)[None, :], bias=None, idx=idx)
    return dict(a=tern((R, K), seed), b=tern((K, C), seed + 1), bias=bias_int(C, seed + 2) if layout == "fwd" else None, idx=None)


def gemm_ref(case, dtype=None, plan=None, wrong=None):
    ref = contract(case["a"], case["b"], dtype, plan, wrong)
    return ref if case["bias"] is None else ref + case["bias"]


def named_k(case, i, j, value):
    """the contraction index (first of its code group) a position-coded output element names"""
    K = case["a"].shape[1]
    g = code_group(K)
    return (int(value) * int(col_sign(case["b"].shape[1])[j]) + (K // g) // 2) * g


# ------------------------------------------------------------------------------------------------ 1. the generic engine, three layouts
# contraction lengths the 256 x 256 kernel refuses (K % 128) and that end inside a K tile of the generic engine (64 bf16 / 32 fp32 elements):
# 8, 72, 136, 200 (K % 8, the ABI's rule for bf16) and, fp32 forward and weight gradient only, 36 (the data gradient's ABI wants a
# contraction % 8 in both dtypes).  Rows 1 / 8 / 65 / 129 / 200 and columns 8 / 72 / 136 / 264 straddle the 128 x 128 workgroup tile and
# the 64 x 64 wave tile.  Every value appears in every layout and dtype -- except that pa_linear_wgrad refuses output rows that are no
# multiple of 4 (OpT::vec reads four of them at once): the weight gradient takes 4 / 68 / 132 for 1 / 65 / 129.
GENERIC_SHAPES = [(1, 8, 8), (8, 72, 72), (65, 136, 136), (129, 264, 200), (200, 72, 136)]
GENERIC_WGRAD_SHAPES = [(4, 8, 8), (8, 72, 72), (68, 136, 136), (132, 264, 200), (200, 72, 136)]
GENERIC_F32_ONLY = {"fwd": [(65, 8, 36)], "dgrad": [], "wgrad": [(68, 8, 36)]}
LAYOUTS = ("fwd", "dgrad", "wgrad")
ROUTE_OF = {"fwd": route_fwd, "dgrad": route_dgrad, "wgrad": route_wgrad}


def generic_params():
    """-> [(layout, dtype, R, C, K)], every one on the generic engine"""
    out = []
    for layout in LAYOUTS:
        for dtype in DTYPES:
            shapes = GENERIC_WGRAD_SHAPES if layout == "wgrad" else GENERIC_SHAPES
            out += [(layout, dtype) + s for s in shapes + (GENERIC_F32_ONLY[layout] if dtype == F32 else [])]
    return out


# ------------------------------------------------------------------------------------------------ 2. generic weight gradient, K splits
SPLIT_OUTPUTS = [(64, 64), (72, 200)]
# 40: one split in bf16, 32 + 8 in fp32; 100: 2 / 4 splits, the last ragged; 128: 2 / 4 splits, every one full; 296: 5 / 10; 1000: 16 / 32;
# 4100: 64 splits of 128 (bf16: 33 hold data, the 33rd 4 rows) or 96 (fp32: 43 hold data, the 43rd 68 rows), the rest write zero slabs
SPLIT_CONTRACTIONS = [40, 100, 128, 296, 1000, 4100]
SPLIT_CODED = [(72, 200, 4100)]


def split_params():
    return [(dtype, R, C, K) for dtype in DTYPES for R, C in SPLIT_OUTPUTS for K in SPLIT_CONTRACTIONS]


# ------------------------------------------------------------------------------------------------ 3. residual + DropPath row scale
# out = resid + rowscale[i / rps] * (acc + bias), fp32.  264 columns: the last 8-column group of the 256 x 256 kernel starts at 256, so its
# second store44 half (columns 288..291) lies outside the matrix and must be neither loaded (bias, resid) nor stored.
RESID_CASES = [("g256", BF16, 328, 264, 256), ("g256", BF16, 512, 512, 128), ("generic", BF16, 200, 72, 72), ("generic", F32, 200, 72, 72)]
RESID_RPS = (100, 1)                     # 100 crosses the 64-row wave tiles and the 128- / 256-row workgroup tiles; 1: a factor per row
ROWSCALES = (0.0, 0.5, 1.0, 2.0, 4.0)    # powers of two and zero: every product and sum is an integer or half-integer, FMA or not
RESID_SKIP = (512, 256, 128, 256)        # (R, C, K, rows per sample): sample 1 dropped, 256-row tiles (knob 4 = 1)
RESID_SKIP_SCALES = ([1.0, 0.0], [2.0, 0.0])


def resid_params():
    return [c + (rps,) for c in RESID_CASES for rps in RESID_RPS]


@functools.lru_cache(maxsize=None)
def resid_case(R, C, K, rps, scales=None):
    g = torch.Generator().manual_seed(50 + rps)
    case = dict(gemm_case("fwd", R, C, K))
    case["resid"] = (torch.randint(0, 2049, (R, C), generator=g) - 1024).double()
    ns = (R + rps - 1) // rps
    if scales is None:
        rs = torch.tensor(ROWSCALES, dtype=torch.float64)[torch.randint(0, len(ROWSCALES), (ns,), generator=g)]
        rs[1 % ns] = 0.0                  # at least one dropped sample, and not the first
        rs[0] = 2.0
    else:
        rs = torch.tensor(scales, dtype=torch.float64)
    case["rowscale"], case["rps"] = rs, rps
    return case


def resid_ref(case, wrong=None):
    """fp64 (exact: half-integers below 2^13)"""
    R, C = case["resid"].shape
    bias = case["bias"]
    if wrong == "bias_halves_swapped":    # the bias of columns j+32.. added to columns j.. and the other way round (zero where that is outside)
        src = torch.arange(C) ^ 32
        bias = torch.where(src < C, bias[src.clamp(max=C - 1)], torch.zeros_like(bias))
    rows = torch.arange(R)
    si = (rows // 128).clamp(max=case["rowscale"].numel() - 1) if wrong == "rowscale_by_128" else rows // case["rps"]
    assert wrong in (None, "bias_halves_swapped", "rowscale_by_128"), wrong
    return case["resid"] + case["rowscale"][si][:, None] * (case["a"] @ case["b"] + bias).double()


# ------------------------------------------------------------------------------------------------ 4. pixel shuffle
# (B, Hp, Wp, P, C, K) -> x [B Hp Wp, K] . w [P P C, K]^T, stored as the NHWC image [B, Hp P, Wp P, C]
PIXSHUF_CASES = [((2, 2, 3, 4, 8, 128), "g256"),        # Hp != Wp, 12 token rows
                 ((1, 3, 5, 2, 40, 128), "g256"),       # C no power of two
                 ((2, 2, 3, 4, 4, 128), "generic"),     # C % 8 != 0: bf16 leaves the 256 x 256 kernel, whose store covers 8 channels
                 ((2, 2, 3, 4, 8, 72), "generic")]      # by its K
PIXSHUF_KINDS = ("coded", "tern")


def route_pixshuf(dtype, B, Hp, Wp, P, C, K):
    return "g256" if route_fwd(dtype, B * Hp * Wp, P * P * C, K) == "g256" and C % 8 == 0 else "generic"


def pixshuf_params():
    """bf16 everywhere; fp32 on the shapes that are generic in bf16 too"""
    return [(dtype, kind) + shape for shape, route in PIXSHUF_CASES for dtype in DTYPES if dtype == BF16 or route == "generic"
            for kind in PIXSHUF_KINDS]


def pixshuf_sign(P, C):
    """[P P C]: the bit-parity sign of the channel, negated where p > q: no swap of p and q and no shift of c maps it onto itself"""
    s = torch.tensor([_sign(c) for c in range(C)])
    pp, qq = torch.meshgrid(torch.arange(P), torch.arange(P), indexing="ij")
    return ((1 - 2 * (pp > qq).long())[:, :, None] * s[None, None, :]).reshape(-1)


@functools.lru_cache(maxsize=None)
def pixshuf_case(kind, B, Hp, Wp, P, C, K):
    M, N = B * Hp * Wp, P * P * C
    if kind == "coded":
        a, idx = hot(M, K)
        return dict(a=a, b=coded(K)[:, None] * pixshuf_sign(P, C)[None, :], bias=torch.zeros(N, dtype=torch.int64), idx=idx)
    return dict(a=tern((M, K), 61), b=tern((K, N), 62), bias=bias_int(N, 63), idx=None)


def pixshuf_ref(case, B, Hp, Wp, P, C, wrong=None):
    """int64 NHWC [B, Hp P, Wp P, C]: the product permuted as the model does (models_painter.py: einsum("nhwpqc->nchpwq"), NCHW)"""
    y = (case["a"] @ case["b"] + case["bias"]).reshape(B, Hp, Wp, P, P, C)
    assert wrong in (None, "pq_swapped"), wrong
    nchw = torch.einsum("nhwqpc->nchpwq" if wrong == "pq_swapped" else "nhwpqc->nchpwq", y).reshape(B, C, Hp * P, Wp * P)
    return nchw.permute(0, 2, 3, 1).contiguous()


# ------------------------------------------------------------------------------------------------ 5. GELU' from the 8-bit code (bf16)
G8_STEP = np.float32(1.26) / np.float32(255)         # constexpr float G8_STEP = 1.26f / 255.f: an fp32 division
G8_OFF = np.float32(0.13)


def g8_value(q):
    """the bits of the kernels' g8_value(q) = fmaf((float)q, G8_STEP, -G8_OFF): the expression is exact in fp64 (an 8-bit integer times a
    24-bit constant, minus a 24-bit constant of a nearby exponent -- test_gemm_exact_cases_cpu.py checks all 256 codes against
    fractions.Fraction), so ONE rounding to fp32 is the fused multiply-add.  q: numpy integers -> float32"""
    return (np.asarray(q, dtype=np.float64) * np.float64(G8_STEP) - np.float64(G8_OFF)).astype(np.float32)


def g8_value_fraction(q):
    return Fraction(int(q)) * Fraction(float(G8_STEP)) - Fraction(float(G8_OFF))


def g8_value_old(q):
    """what ops.gelu_aux_decode computed before: fp32 multiply by the fp64 quotient's rounding, then an fp32 subtraction"""
    return np.asarray(q, dtype=np.float32) * np.float32(1.26 / 255.0) - np.float32(0.13)


# (route, R, C, K, pad): pad > 0 = `out` and `aux` are column-slice views with a row pitch of C + pad (elements of out = bytes of aux)
DGELU_CASES = [("g256", 328, 264, 256, 0), ("g256", 512, 512, 128, 0), ("generic", 200, 72, 72, 0), ("g256", 328, 264, 256, 24),
               ("generic", 200, 72, 72, 24)]
# column sums of Epi4DGeluCS: (R, C, K, knobs {knob: value}, the dy rows that are non-zero, one at a time)
DGELU_CS_CASES = [(328, 264, 256, {4: 1}, (0, 127, 128, 255, 256, 327)),            # 256-row tiles
                  (328, 264, 256, {4: 2}, (0, 127, 128, 255, 256, 327)),            # 224-row tiles
                  (640, 264, 256, {12: 2, 14: 1}, (0, 255, 256, 383, 384, 639))]    # forced mixed plan: one full tile + three half tiles
DGELU_CS_GENERIC = (200, 72, 72, (0, 63, 64, 127, 128, 199))                        # EpiDGelu<bf16> + pa_colsum over the stored bf16 rows


def aux_codes(R, C):
    i, j = torch.meshgrid(torch.arange(R), torch.arange(C), indexing="ij")
    return ((7 * i + 13 * j) % 256).to(torch.uint8)


@functools.lru_cache(maxsize=None)
def dgelu_case(R, C, K, pad=0, hot_row=None):
    case = dict(gemm_case("dgrad", R, C, K))
    if hot_row is not None:
        a = torch.zeros_like(case["a"])
        a[hot_row] = case["a"][hot_row]
        case["a"] = a
    case["aux"], case["pad"] = aux_codes(R, C), pad
    return case


def dgelu_ref(case, wrong=None, stored=True):
    """-> the product v g8_value(code): v = dY . W an exact integer, the product exact in fp64, rounded to fp32 (the kernel's fp32 multiply)
    and -- stored=True -- from there to bf16 (round to nearest even both times): bf16 [R, C]; stored=False: the fp32 values"""
    R, C = case["aux"].shape
    v = (case["a"] @ case["b"]).numpy().astype(np.float64)
    q = case["aux"].numpy()
    if wrong == "aux_pitch_doubled":     # row i of the codes read at byte i * 2 ld of the buffer (wrapped, where the host model must stay inside it)
        ld = C + case["pad"]
        flat = np.zeros(R * ld, dtype=np.uint8)
        flat.reshape(R, ld)[:, :C] = q
        i, j = np.meshgrid(np.arange(R), np.arange(C), indexing="ij")
        q = flat[(i * 2 * ld + j) % flat.size]
    g = g8_value_old(q) if wrong == "old_decode" else g8_value(q)
    assert wrong in (None, "aux_pitch_doubled", "old_decode"), wrong
    prod = torch.from_numpy((v * g.astype(np.float64)).astype(np.float32))
    return prod.to(torch.bfloat16) if stored else prod


def dgelu_colsum_ref(case, hot_row, wrong=None, from_stored=False):
    """fp32 [C]: ONE non-zero dy row, so every partial sum is fmaf(v, g, 0) = float32(v g) plus zeros, in any order.  from_stored: the sums
    of the bf16 values as stored (the generic route's separate pa_colsum pass)."""
    row = dgelu_ref(case, wrong, stored=from_stored)[hot_row].float()
    return row + 0.0                     # (a -0 product and +0 partial sums add to +0; torch.equal does not tell them apart anyway)


# ------------------------------------------------------------------------------------------------ 6. GELU forward
GELU_CASES = [("g256", 328, 264, 256), ("generic", 200, 72, 72)]
# act: one bf16 rounding of x cdf(x) (2^-9 of the value) + the erf approximation (A-S 7.1.26, 1.5e-7 absolute on erf = 0.75e-7 on the cdf, and
# a few fp32 roundings of a value <= 1: together < 4e-7) times |x|; the project's gate for act is 2^-8 of max |gelu| over the tensor
# (tests/test_kernels_gpu.py: test_gemm256_bf16_tight_gates_against_fp64) -- held here per element, which is stricter
GELU_ACT_REL, GELU_ACT_CDF_ABS = 2.0 ** -8, 4e-7
GELU_AUX_ABS = 0.5 * 1.26 / 255 + 1e-5   # tests/test_kernels_gpu.py: check_gelu_pair


def gelu_fp64(pre):
    x = pre.double()
    cdf = 0.5 * (1.0 + torch.erf(x * 0.7071067811865476))
    return x * cdf, cdf + x * torch.exp(-0.5 * x * x) * 0.3989422804014327


# ------------------------------------------------------------------------------------------------ 7. reductions
# pa_slab_reduce(in, out, n, nz, stride, accumulate).  Small n: every nz; n >= 2^18, where nz <= 16 takes the wide kernel: nz up to 17 (one
# past the switch; 2^18 x 17 floats = 17.8 MB -- 33 / 64 slabs of that length would be 35 / 67 MB of host-made integers for the tree kernel,
# which the small n already run at those nz)
SLAB_N_SMALL, SLAB_N_LARGE = (4, 68, 260), (1 << 18, (1 << 18) + 4)
SLAB_NZ_SMALL, SLAB_NZ_LARGE = (1, 3, 16, 17, 33, 64), (1, 3, 16, 17)
SLAB_STRIDE_PAD = (0, 8)


def slab_params():
    """-> [(n, nz, kernel)]; each runs stride n and n + 8, accumulate 0 and 1"""
    return [(n, nz, slab_kernel(n, nz)) for n in SLAB_N_SMALL for nz in SLAB_NZ_SMALL] + \
           [(n, nz, slab_kernel(n, nz)) for n in SLAB_N_LARGE for nz in SLAB_NZ_LARGE]


def small_ints(shape, seed, lo=-3, hi=3):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g, dtype=torch.int8)


def slab_case(n, nz, pad):
    """-> (slabs int8 [nz, n + pad] -- the pad columns hold 100, which no sum may contain --, prior int8 [n])"""
    slabs = small_ints((nz, n + pad), 71 + nz)
    slabs[:, n:] = 100
    return slabs, small_ints((n,), 72, -50, 50)


def slab_ref(slabs, prior, n, accumulate, wrong=None):
    assert wrong in (None, "accumulate_ignored"), wrong
    s = slabs[:, :n].sum(0, dtype=torch.int64)
    return s + prior.long() if accumulate and wrong is None else s


COLSUM_M = (1, 31, 33, 4095, 4096, 4100)     # 32 rows per chunk below 4096, 128 from there
COLSUM_N = (8, 264)
COLSUM_VIEW = (33, 264, 16)                  # (M, N, pad): a column slice of a [M, N + 2 pad] matrix starting at column pad
DEAD_ROW_VALUE = 1024                        # what rows at and beyond a live count hold


def colsum_params():
    return [(dtype, M, N, 0) for dtype in DTYPES for M in COLSUM_M for N in COLSUM_N] + [(dtype,) + COLSUM_VIEW for dtype in DTYPES]


def live_counts(M):
    """0, 1, M and a count that ends inside a chunk"""
    rpc = colsum_rows_per_chunk(M)
    inside = (M // 2) // rpc * rpc + rpc // 2 + 1
    return sorted({0, 1, M, min(inside, M - 1) if M > 2 else 1})


def colsum_case(M, N, pad, count=None):
    """int8 [M, N + 2 pad] (the columns outside the view hold 100); rows at and beyond `count`: DEAD_ROW_VALUE"""
    x = small_ints((M, N + 2 * pad), 81).to(torch.int16)
    if pad:
        x[:, :pad] = 100
        x[:, pad + N:] = 100
    if count is not None:
        x[count:] = DEAD_ROW_VALUE
    return x


def colsum_ref(x, N, pad, count=None, wrong=None):
    assert wrong in (None, "dead_rows_summed"), wrong
    rows = x if count is None or wrong == "dead_rows_summed" else x[:count]
    return rows[:, pad:pad + N].sum(0, dtype=torch.int64)
