"""The kernels of the ViT-H/14 step (BASELINE configs[4], `bench.py --model vit_huge`) at their real shapes, against fp64.

Every other ViT-H/14 test runs embed 160 with 2 heads; the kernels pick their code paths by shape, and at embed 1280 / 16 heads / the
64 x 32 token grid / B = 4 they take paths those shapes never reach: 224-row GEMM tiles with a ragged last tile (8192 = 36 x 224 + 128),
mixed full + half tile plans, 5-column-tile weight gradients and the 75-tile qkv gradient, the head_dim-80 generation-2 attention
kernels at 16 heads, the pixel-shuffle epilogues at P = 14, the generic patch-embedding gather with K = 588.

Every shape is derived from oracle.painter_oracle.vit_huge_config() and the per-GPU batch.  References are torch in fp64 on the device.
Gates, for operands that are exact in bf16 (test_kernels_gpu.py, test_gemm256_bf16_tight_gates_against_fp64): fp32 outputs within
5e-6 * sqrt(K) of max |ref|, bf16 outputs within 2^-8 of max |ref| (one rounding of the result); elsewhere the gate of the existing test
of the same kernel family.  Each test prints what it measured."""
import contextlib
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import painter_oracle as O

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from painter_amd import hostmath, ops
    from painter_amd._lib import EPI_BIAS, EPI_BIAS_F32, EPI_BIAS_RESID, lib
    from tests.test_kernels_gpu import _layernorm_fwd_bwd, attn_reference, gelu_aux_of, gelu_aux_values, gelu_grad_ref

DEV = "cuda"
CFG = O.vit_huge_config()
BATCH = 4                                        # per-GPU batch of bench.py --model vit_huge (configs[4]'s per-GPU half)
HP, WP = CFG.grid                                # 64 x 32 tokens
L = HP * WP
D = CFG.embed_dim
HEADS = CFG.num_heads
HD = D // HEADS
P = CFG.patch_size
HI, WI = CFG.img_size
C_DEC = CFG.decoder_embed_dim
HIDDEN = int(D * CFG.mlp_ratio)
M_PRE, M_POST = 2 * BATCH * L, BATCH * L         # token rows before / after the stream merge (both streams, then one)
LAYERS = {"qkv": (3 * D, D), "proj": (D, D), "fc1": (HIDDEN, D), "fc2": (D, HIDDEN)}     # nn.Linear (out N, in K)
LAYER_CASES = [(name, M) for M in (M_PRE, M_POST) for name in LAYERS]
BF16_GATE = 2.0 ** -8


def f32_gate(K):
    return 5e-6 * math.sqrt(K)


def gen(shape, seed, scale=1.0, dtype=torch.float32):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(shape, generator=g, device=DEV) * scale).to(dtype)


def rel(a, ref):
    """max |a - ref| / max |ref|, in fp64 on the device."""
    a, ref = a.double(), ref.double()
    return float((a - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


@contextlib.contextmanager
def knobs(settings):
    """pa_debug_set(k, v) for every {k: v} for the duration of the block; the values found before are restored afterwards."""
    saved = {k: lib.pa_debug_get(k) for k in settings}
    try:
        for k, v in settings.items():
            assert lib.pa_debug_set(k, v) == 0
        yield
    finally:
        for k, v in saved.items():
            lib.pa_debug_set(k, v)


def report(what, errs):
    print("%s:" % what, {k: "%.2e" % v for k, v in errs.items()})


# ------------------------------------------------------------------------------------------------ gemm256
@pytest.mark.parametrize("layer,M", LAYER_CASES)
def test_gemm256_forward_epilogues_vs_fp64(layer, M):
    """Every epilogue the encoder blocks run: bias (bf16 out), bias (fp32 out), bias + erf-GELU with the 8-bit GELU' code, bias + residual
    + per-sample DropPath row scale (rows_per_sample = L)."""
    N, K = LAYERS[layer]
    T = torch.bfloat16
    x, w, b = gen((M, K), 1, 1.0, T), gen((N, K), 2, 0.05, T), gen((N,), 3)
    ref = x.double() @ w.double().t() + b.double()
    errs = {"bias_bf16": rel(ops.linear_fwd(x, w, b, EPI_BIAS), ref), "bias_f32": rel(ops.linear_fwd(x, w, b, EPI_BIAS_F32), ref)}
    act, aux = ops.linear_gelu(x, w, b)
    pre = ops.linear_fwd(x, w, b, EPI_BIAS)      # the bits in front of the GELU (same operands, same accumulation order)
    errs["gelu_act_bf16"] = rel(act, F.gelu(pre.double()))
    errs["gelu_aux_bf16"] = rel(ops.gelu_aux_decode(aux), gelu_grad_ref(pre))
    del act, aux, pre
    resid = gen((M, N), 4)
    rowscale = gen((M // L,), 5).abs() + 0.5
    out = ops.linear_fwd(x, w, b, EPI_BIAS_RESID, resid=resid, rowscale=rowscale, rows_per_sample=L)
    errs["resid_f32"] = rel(out, resid.double() + rowscale.double().repeat_interleave(L)[:, None] * ref)
    report("gemm256 forward %s M=%d N=%d K=%d" % (layer, M, N, K), errs)
    for k, v in errs.items():
        assert v < (f32_gate(K) if k.endswith("f32") else BF16_GATE), (k, errs)


@pytest.mark.parametrize("layer,M", LAYER_CASES)
def test_gemm256_data_gradient_epilogues_vs_fp64(layer, M):
    """dX [M, K] = dY [M, N] . W [N, K]: plain, times the decoded GELU' code, and with the column sums of the stored dX from the
    epilogue (what fc2's data gradient hands to fc1's bias gradient)."""
    N, K = LAYERS[layer]
    T = torch.bfloat16
    dy, w = gen((M, N), 6, 1.0, T), gen((N, K), 7, 0.05, T)
    aux = gelu_aux_of(gen((M, K), 9, 1.0, T))
    dx_ref = dy.double() @ w.double()
    plain = ops.linear_dgrad(dy, w)
    errs = {"dgrad_bf16": rel(plain, dx_ref)}
    cs = torch.full((K,), float("nan"), device=DEV)
    dxg = ops.linear_dgrad(dy, w, gelu_aux=aux, colsum_out=cs)
    assert torch.equal(dxg, ops.linear_dgrad(dy, w, gelu_aux=aux))              # the extra output changes nothing else
    dxg_ref = dx_ref * gelu_aux_values(aux)
    errs["dgrad_dgelu_bf16"] = rel(dxg, dxg_ref)
    errs["colsum_vs_stored"] = rel(cs, dxg.double().sum(0))
    errs["colsum_vs_fp64"] = rel(cs, dxg_ref.sum(0))
    report("gemm256 data gradient %s M=%d N=%d K=%d" % (layer, M, N, K), errs)
    assert errs["dgrad_bf16"] < BF16_GATE and errs["dgrad_dgelu_bf16"] < BF16_GATE, errs
    assert errs["colsum_vs_stored"] < 4e-3 and errs["colsum_vs_fp64"] < 2e-4, errs       # test_linear_dgrad_column_sums_from_the_epilogue's gates


@pytest.mark.parametrize("layer,M", LAYER_CASES)
def test_gemm256_weight_gradient_vs_fp64_at_every_split_target(layer, M):
    """dW [N, K] = dY^T . X over M rows, at the stand-alone workgroup target (knob 3 = 0: 256), the side-stream target the engine sets
    (96) and a small one (16: one split, no slab reduction).  qkv's 75 column tiles are the case wgrad_fast_splits rounds up from."""
    N, K = LAYERS[layer]
    T = torch.bfloat16
    dy, x = gen((M, N), 6, 1.0, T), gen((M, K), 8, 1.0, T)
    ref = dy.double().t() @ x.double()
    errs = {}
    for target in (0, 96, 16):
        with knobs({3: target}):
            dw = ops.linear_wgrad(dy, x)
            errs["wgrad_f32@%d" % target] = rel(dw, ref)
            assert torch.equal(dw, ops.linear_wgrad(dy, x)), target        # fixed reduction order: the same bits run to run
    report("gemm256 weight gradient %s M=%d N=%d K=%d" % (layer, M, N, K), errs)
    assert max(errs.values()) < f32_gate(K), errs


def _plans(M):
    """name -> knobs of every tile plan: uniform 256-row tiles (the reference), uniform 224-row tiles, the rule without mixed plans, the
    rule itself, and two forced mixed plans (knob 12 = 2, knob 14 = nfull full 256-row tiles, half tiles of 128 rows after them)."""
    return {"256": {4: 1}, "224": {4: 2}, "no_mixed": {4: 0, 12: 1}, "rule": {4: 0, 12: 0},
            "mixed_most_full": {4: 0, 12: 2, 14: (M - 1) // 256}, "mixed_half_full": {4: 0, 12: 2, 14: M // 512}}


@pytest.mark.parametrize("layer,M", LAYER_CASES + [(name, M_POST - 112) for name in LAYERS])
def test_gemm256_tile_plans_bit_identical_to_uniform_256_row_tiles(layer, M):
    """Every tile plan keeps the ascending K order per output element, so every forward and data-gradient epilogue must return the bits of
    the uniform 256-row plan; the column sums agree to fp32 summation order (another number of partial rows).  The ViT-H row counts are
    multiples of 128, so the last half tile of a mixed plan is always full there: M = B*L - 112 adds a last half tile of 16 rows (and a
    last 224-row tile of 16 rows)."""
    N, K = LAYERS[layer]
    T = torch.bfloat16
    x, w, b = gen((M, K), 1, 1.0, T), gen((N, K), 2, 0.05, T), gen((N,), 3)
    resid = gen((M, N), 4)
    rowscale = gen(((M + L - 1) // L,), 5).abs() + 0.5
    dy, w2 = gen((M, N), 6, 1.0, T), gen((N, K), 7, 0.05, T)
    aux2 = torch.randint(0, 256, (M, K), dtype=torch.uint8, generator=torch.Generator(device=DEV).manual_seed(9), device=DEV)

    def run():
        act, aux = ops.linear_gelu(x, w, b)
        cs = torch.full((K,), float("nan"), device=DEV)
        res = [ops.linear_fwd(x, w, b, EPI_BIAS), ops.linear_fwd(x, w, b, EPI_BIAS_F32), act, aux,
               ops.linear_fwd(x, w, b, EPI_BIAS_RESID, resid=resid, rowscale=rowscale, rows_per_sample=L),
               ops.linear_dgrad(dy, w2), ops.linear_dgrad(dy, w2, gelu_aux=aux2, colsum_out=cs)]
        return res, cs

    out = {}
    for name, kv in _plans(M).items():
        with knobs(kv):
            out[name] = run()
    ref, cs_ref = out["256"]
    errs = {}
    for name, (got, cs) in out.items():
        for i, (a, r) in enumerate(zip(got, ref)):
            assert torch.equal(a, r), (name, i)
        errs[name] = rel(cs, cs_ref)
    report("gemm256 tile plans %s M=%d: column sums vs the 256-row plan" % (layer, M), errs)
    assert max(errs.values()) < 1e-5, errs
    assert rel(ref[1], x.double() @ w.double().t() + b.double()) < f32_gate(K)


def _pixshuf_ref(x, w, b, batch, hp, wp, p, c):
    r = (x.double() @ w.double().t() + b.double()).reshape(batch, hp, wp, p, p, c)
    return torch.einsum("nhwpqc->nchpwq", r).reshape(batch, c, hp * p, wp * p).permute(0, 2, 3, 1)


@pytest.mark.parametrize("model", ["vit_huge", "vit_large"])
def test_decoder_embedding_pixel_shuffle_epilogue_vs_fp64(model):
    """decoder_embed (Linear(4 D -> P*P*64) over the four tapped blocks' features) with the pixel shuffle in its epilogue: ViT-H/14 (K 5120,
    N 12544, P 14, M 8192; the rule picks a mixed plan) and ViT-L (K 4096, N 16384, P 16, M 12544), bf16 under the rule, a forced mixed
    plan and uniform 256-row tiles (bit-identical), and fp32."""
    if model == "vit_huge":
        cfg, batch = CFG, BATCH
    else:
        cfg, batch = O.vit_large_config(), 8            # bench.py's ViT-L per-GPU batch
    hp, wp = cfg.grid
    p, c, K = cfg.patch_size, cfg.decoder_embed_dim, len(cfg.taps) * cfg.embed_dim
    M, N = batch * hp * wp, p * p * cfg.decoder_embed_dim
    errs = {}
    for T in (torch.bfloat16, torch.float32):
        x, w, b = gen((M, K), 1, 1.0, T), gen((N, K), 2, 0.02, T), gen((N,), 3)
        ref = _pixshuf_ref(x, w, b, batch, hp, wp, p, c)
        out = ops.linear_pixshuf(x, w, b, batch, hp, wp, p, c)
        if T == torch.bfloat16:
            errs["bf16_rule"] = rel(out, ref)
            with knobs({4: 0, 12: 2, 14: (M - 1) // 256}):
                mixed = ops.linear_pixshuf(x, w, b, batch, hp, wp, p, c)
            with knobs({4: 1}):
                uniform = ops.linear_pixshuf(x, w, b, batch, hp, wp, p, c)
            errs["bf16_mixed"] = rel(mixed, ref)
            assert torch.equal(out, uniform) and torch.equal(mixed, uniform)
        else:
            errs["f32"] = rel(out, ref)
        del x, w, ref, out
    report("decoder embedding + pixel shuffle %s M=%d N=%d K=%d P=%d" % (model, M, N, K, p), errs)
    assert errs["bf16_rule"] < BF16_GATE and errs["bf16_mixed"] < BF16_GATE and errs["f32"] < 2e-5, errs     # fp32: test_linear_fwd_epilogues' gate


# ------------------------------------------------------------------------------------------------ attention
@pytest.mark.parametrize("T", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("nseq", [2 * BATCH, BATCH])
def test_attention_head_dim_80_sixteen_heads_vs_fp64(T, nseq):
    """Windowless rel-pos attention at ViT-H/14 width: 16 heads of 80 on the 64 x 32 grid, 2B sequences before the stream merge, B after.
    Forward (out, lse) and backward (dq, dk, dv, both rel-pos tables; the table gradient at the stand-alone and the side-stream split
    count, knob 6) against attn_reference; gates of test_attn_head_dim_80_fwd_bwd.  bf16 must run the generation-2 head_dim-80 kernels."""
    nh, nw = 2 * HP - 1, 2 * WP - 1
    scale = HD ** -0.5
    qkv = gen((nseq * L, 3 * D), 1, 1.0, T)
    rel_h, rel_w = gen((nh, HD), 2, 0.2), gen((nw, HD), 3, 0.2)
    dout = gen((nseq * L, D), 4, 1.0, T)
    rcat, rcatT = ops.relpos_pack(rel_h, rel_w, HP, WP, T), ops.relpos_pack_t(rel_h, rel_w, HP, WP, T)
    c0 = ops.attn_launch_counts()
    out, lse = ops.attn_fwd(qkv, rcat, nseq, L, HEADS, HP, WP, scale)
    dqkv, dG = ops.attn_bwd_core(qkv, rcat, rcatT, out, dout, lse, nseq, L, HEADS, HP, WP, scale)
    drcat = {}
    for splits in (0, 8):
        with knobs({6: splits}):
            drcat[splits] = ops.attn_bwd_relpos(dG, qkv, rcat.shape[0], nseq, L, HEADS, HP, WP)
    c1 = ops.attn_launch_counts()
    fam = 1 if T == torch.bfloat16 else 0                  # (generic, generation 2, generation 3)
    for k in ("fwd", "bwd"):
        d = [c1[k][i] - c0[k][i] for i in range(3)]
        assert d[fam] >= 1 and sum(d) == d[fam], (k, d)
    q64 = qkv.double().clone().requires_grad_(True)
    rh64 = rcat[:nh].double().clone().requires_grad_(True)
    rw64 = rcat[nh:nh + nw].double().clone().requires_grad_(True)
    ref, lse_ref = attn_reference(q64, rh64, rw64, nseq, L, HEADS, HP, WP, scale)
    errs = {"out": rel(out, ref.detach()), "lse": rel(lse, lse_ref.detach())}
    ref.backward(dout.double())
    del ref, lse_ref
    errs.update(dq=rel(dqkv[:, :D], q64.grad[:, :D]), dk=rel(dqkv[:, D:2 * D], q64.grad[:, D:2 * D]), dv=rel(dqkv[:, 2 * D:], q64.grad[:, 2 * D:]))
    for s, dr in drcat.items():
        errs["drh@%d" % s], errs["drw@%d" % s] = rel(dr[:nh], rh64.grad), rel(dr[nh:nh + nw], rw64.grad)
        assert dr.shape[0] == nh + nw or float(dr[nh + nw:].abs().max()) == 0.0
    report("attention hd %d, %d heads, %d sequences, %s" % (HD, HEADS, nseq, T), errs)
    bf = T == torch.bfloat16
    assert errs["lse"] < (2e-3 if bf else 1e-5) and errs["out"] < (1.2e-2 if bf else 2e-5), errs
    assert max(v for k, v in errs.items() if k not in ("out", "lse")) < (1.6e-2 if bf else 5e-5), errs


# ------------------------------------------------------------------------------------------------ decoder 3x3 conv + tail
def _conv3x3(x, w):
    """NHWC x [B, H, W, Cin], w [Cout, Cin, 3, 3], padding 1 -> [B, H, W, Cout]: nine shifted channel matmuls (same arithmetic as
    conv2d; torch's fp64 conv is no GPU kernel)."""
    H, W = x.shape[1], x.shape[2]
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    y = 0
    for ky in range(3):
        for kx in range(3):
            y = y + xp[:, ky:ky + H, kx:kx + W, :] @ w[:, :, ky, kx].t()
    return y


def _conv3x3_dgrad(dy, w):
    """conv_transpose2d(dy, w, padding=1) in NHWC: dx[h, w] = sum over taps of dy[h + 1 - ky, w + 1 - kx] . W[:, :, ky, kx]."""
    H, W = dy.shape[1], dy.shape[2]
    dp = F.pad(dy, (0, 0, 1, 1, 1, 1))
    dx = 0
    for ky in range(3):
        for kx in range(3):
            dx = dx + dp[:, 2 - ky:2 - ky + H, 2 - kx:2 - kx + W, :] @ w[:, :, ky, kx]
    return dx


def _conv3x3_wgrad(dy, x):
    """torch.nn.grad.conv2d_weight(x, (Cout, Cin, 3, 3), dy, padding=1) in NHWC."""
    H, W = x.shape[1], x.shape[2]
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    d2 = dy.reshape(-1, dy.shape[3]).t()
    return torch.stack([torch.stack([d2 @ xp[:, ky:ky + H, kx:kx + W, :].reshape(-1, x.shape[3]) for kx in range(3)], -1)
                        for ky in range(3)], -2)


def test_shifted_matmul_conv_references_equal_torch_conv():
    """The three helpers above against torch's own conv2d, conv_transpose2d and conv2d_weight (fp64, CPU, small)."""
    g = torch.Generator().manual_seed(0)
    x, dy, w = torch.randn(2, 9, 13, 8, generator=g, dtype=torch.float64), torch.randn(2, 9, 13, 6, generator=g, dtype=torch.float64), \
        torch.randn(6, 8, 3, 3, generator=g, dtype=torch.float64)
    nchw = lambda t: t.permute(0, 3, 1, 2)
    assert torch.allclose(nchw(_conv3x3(x, w)), F.conv2d(nchw(x), w, padding=1), rtol=0, atol=1e-12)
    assert torch.allclose(nchw(_conv3x3_dgrad(dy, w)), F.conv_transpose2d(nchw(dy), w, padding=1), rtol=0, atol=1e-12)
    assert torch.allclose(_conv3x3_wgrad(dy, x), torch.nn.grad.conv2d_weight(nchw(x), w.shape, nchw(dy), padding=1), rtol=0, atol=1e-12)


def _tail(y, gamma, beta, w1, b1, eps):
    """LayerNorm2D(64) . GELU . Conv1x1(64 -> 3) on NHWC y (models_painter.py:328-333) -> NCHW pred."""
    u = y.mean(-1, keepdim=True)
    v = (y - u).pow(2).mean(-1, keepdim=True)
    z = (y - u) / torch.sqrt(v + eps) * gamma + beta
    return (F.gelu(z) @ w1.t() + b1).permute(0, 3, 1, 2)


@pytest.mark.parametrize("T,wp", [(torch.bfloat16, WP), (torch.float32, WP), (torch.bfloat16, WP - 1)])
def test_decoder_conv_and_tail_at_patch_14_full_size(T, wp):
    """Decoder 3x3 conv (64 -> 64) and tail at ViT-H/14's image size, B = 4: pa_decoder_tail_fwd (y3, pred), pa_conv3x3_dgrad_unshuffle
    (the inverse pixel shuffle at P = 14: 4.6 patches per 64-pixel tile row), pa_conv3x3_wgrad, pa_decoder_tail_bwd_pointwise.  bf16 on
    the 896 x 448 image takes the tile kernels (csrc/conv64.h); fp32 and bf16 at 896 x 434 (Wi % 64 != 0) the generic path."""
    hi, wi = HP * P, wp * P
    assert (wi % 64 == 0) == (wp == WP)
    eps = CFG.ln_eps
    x = gen((BATCH, hi, wi, C_DEC), 1, 1.0, T)
    w3 = gen((C_DEC, C_DEC, 3, 3), 2, 0.05)
    b3, gamma, beta = gen((C_DEC,), 3, 0.1), 1.0 + gen((C_DEC,), 4, 0.1), gen((C_DEC,), 5, 0.1)
    w1, b1 = gen((3, C_DEC), 6, 0.1), gen((3,), 7, 0.1)
    w3r, wf = ops.conv3x3_pack(w3, T)
    w3q = w3.to(T).double()
    bf = T == torch.bfloat16
    errs = {}
    pred, y3 = ops.decoder_tail_fwd(x, w3r, b3, gamma, beta, w1, b1, eps, save_y3=True)
    errs["y3"] = rel(y3, _conv3x3(x.double(), w3q) + b3.double())
    errs["pred"] = rel(pred, _tail(y3.double(), gamma.double(), beta.double(), w1.double(), b1.double(), eps))     # of the stored y3 bits
    dy = gen((BATCH, hi, wi, C_DEC), 8, 1.0, T)
    dE = ops.conv3x3_dgrad_unshuffle(dy, wf, BATCH, HP, wp, P)
    dx = _conv3x3_dgrad(dy.double(), w3q)
    errs["dgrad_unshuffle"] = rel(dE, dx.reshape(BATCH, HP, P, wp, P, C_DEC).permute(0, 1, 3, 2, 4, 5).reshape(BATCH * HP * wp, P * P * C_DEC))
    del dx, dE
    dw = ops.conv3x3_wgrad(dy, x)
    errs["wgrad"] = rel(dw, _conv3x3_wgrad(dy.double(), x.double()))
    assert torch.equal(dw, ops.conv3x3_wgrad(dy, x))
    # point-wise tail backward on the stored y3, against fp64 autograd
    dpred = gen((BATCH, 3, hi, wi), 9)
    dy3, grads = ops.decoder_tail_bwd_pointwise(dpred, y3, gamma, beta, w1, eps)
    y = y3.double().clone().requires_grad_(True)
    g64, be64, w64, b64 = (t.double().clone().requires_grad_(True) for t in (gamma, beta, w1, torch.zeros(3, device=DEV)))
    _tail(y, g64, be64, w64, b64, eps).backward(dpred.double())
    errs.update(dy3=rel(dy3, y.grad), dgamma=rel(grads[0:64], g64.grad), dbeta=rel(grads[64:128], be64.grad),
                dw1=rel(grads[128:320].reshape(3, 64), w64.grad), db1=rel(grads[320:323], b64.grad))
    report("decoder conv + tail %s B=%d %dx%d P=%d" % (T, BATCH, hi, wi, P), errs)
    assert errs["y3"] < (BF16_GATE if bf else f32_gate(9 * C_DEC)), errs
    assert errs["dgrad_unshuffle"] < (BF16_GATE if bf else f32_gate(9 * C_DEC)), errs
    assert errs["pred"] < (2e-3 if bf else 2e-5), errs                               # test_conv64_bf16_tile_kernels' gate (bf16)
    assert errs["wgrad"] < 1e-4, errs                                                # test_conv64_bf16_tile_kernels' gate
    assert errs["dy3"] < (1e-2 if bf else 2e-5), errs                                # test_decoder_tail_pointwise_backward_vs_autograd's gates
    assert max(errs[k] for k in ("dgamma", "dbeta", "dw1", "db1")) < (2e-4 if bf else 2e-5), errs


# ------------------------------------------------------------------------------------------------ patch embedding
def _cols(im, T):
    """im2col of Conv2d(3, D, P, stride P) on the T-rounded image: [B*L, 3*P*P], k = c*P*P + ph*P + pw."""
    b = im.shape[0]
    return im.to(T).double().reshape(b, 3, HP, P, WP, P).permute(0, 2, 4, 1, 3, 5).reshape(b * L, 3 * P * P)


@pytest.mark.parametrize("T", [torch.bfloat16, torch.float32])
def test_patch_embedding_at_patch_14_full_width(T):
    """Patch embedding at P = 14, D = 1280 on the 64 x 32 grid, B = 4 (K = 588: the generic gather on the zero-padded weight pack):
    token assembly in Painter and SegGPT modes, the weight gradient and pa_patch_embed_dgrad, against fp64."""
    K = 3 * P * P
    imgs, tgts = gen((BATCH, 3, HI, WI), 1), gen((BATCH, 3, HI, WI), 2)
    w, bias = gen((D, 3, P, P), 3, 0.05), gen((D,), 4, 0.1)
    mask_token, seg_x, seg_y = gen((D,), 5, 0.3), gen((D,), 6, 0.3), gen((D,), 7, 0.3)
    pos = gen((L, D), 8, 0.2)
    tcls, tins = gen((D,), 9, 0.3), gen((D,), 10, 0.3)
    seg_type = torch.tensor([0.0, 1.0, 1.0, 0.0], device=DEV)[:BATCH]
    mask = torch.rand(BATCH, L, generator=torch.Generator(device=DEV).manual_seed(11), device=DEV) < 0.4
    wop = ops.patch_weight_pack(w, T, P)
    assert wop.shape == (D, (K + 7) // 8 * 8) and torch.equal(wop[:, :K], w.to(T).reshape(D, K))
    assert not ops.patch_cols_ok(T, BATCH, L, P, D)
    cx, cy = _cols(imgs, T), _cols(tgts, T)
    wq = wop[:, :K].double()
    m = mask.double().reshape(BATCH * L, 1)
    ex = cx @ wq.t() + bias.double() + seg_x.double() + pos.double().repeat(BATCH, 1)
    ey = (cy @ wq.t() + bias.double()) * (1 - m) + mask_token.double() * m + seg_y.double() + pos.double().repeat(BATCH, 1)
    errs = {}
    for seggpt in (False, True):
        tok = ops.patch_embed_fwd(T, imgs, tgts, wop, bias, mask_token, seg_x, seg_y, pos, mask.to(torch.uint8), tcls if seggpt else None,
                                  tins if seggpt else None, seg_type if seggpt else None, BATCH, HP, WP, P, D)
        ref = torch.cat([ex, ey], 0)
        if seggpt:          # models_seggpt.py:415-420: type 0 -> type_token_cls, type 1 -> type_token_ins, per sample, both streams
            st = seg_type.double().repeat_interleave(L)[:, None]
            ref = ref + (tcls.double() * (st == 0) + tins.double() * (st == 1)).repeat(2, 1)
        errs["tokens_seggpt" if seggpt else "tokens_painter"] = rel(tok, ref)
    del ex, ey, ref, tok
    dpe = gen((2 * BATCH * L, D), 12, 1.0, T)
    dw = ops.patch_embed_wgrad(dpe, imgs, tgts, BATCH, HP, WP, P, D)
    errs["wgrad"] = rel(dw, dpe.double()[:BATCH * L].t() @ cx + dpe.double()[BATCH * L:].t() @ cy)
    dps = gen((2 * BATCH * L, D), 13, 1e-2, T)
    di, dt = ops.patch_embed_dgrad(dps, wop, BATCH, HP, WP, P, D)
    fold = lambda c: c.reshape(BATCH, HP, WP, 3, P, P).permute(0, 3, 1, 4, 2, 5).reshape(BATCH, 3, HI, WI)
    dcols = dps.double() @ wq
    errs["dgrad_imgs"], errs["dgrad_tgts"] = rel(di, fold(dcols[:BATCH * L])), rel(dt, fold(dcols[BATCH * L:]))
    report("patch embedding %s B=%d P=%d D=%d %dx%d" % (T, BATCH, P, D, HP, WP), errs)
    bf = T == torch.bfloat16
    assert max(errs["tokens_painter"], errs["tokens_seggpt"]) < (f32_gate(K) if bf else 2e-6), errs
    assert errs["wgrad"] < (2e-5 if bf else 2e-6), errs                  # test_patch_embed_and_token_assembly_in_isolation's gates
    assert max(errs["dgrad_imgs"], errs["dgrad_tgts"]) < 1e-5, errs     # test_patch_embed_dgrad_kernel_vs_fp64's gate


# ------------------------------------------------------------------------------------------------ row and element kernels
@pytest.mark.parametrize("T", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("R", [M_PRE, M_POST])
def test_layernorm_fwd_bwd_at_vit_huge_width(T, R, variant):
    """LayerNorm forward / backward (dres, T copy scaled by the row scale, dgamma / dbeta, the fused dxT column sums) at D = 1280 over
    the step's row counts, both backward variants (knob 10); test_layernorm_fwd_bwd's checks and gates."""
    with knobs({10: variant}):
        _layernorm_fwd_bwd(T, R, D)


@pytest.mark.parametrize("T", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("N", sorted({n for n, _ in LAYERS.values()}))
def test_colsum_at_vit_huge_widths(T, N):
    """pa_colsum (bias gradients of the N-wide layers) over both row counts against an fp64 sum; test_linear_backward's gate."""
    errs = {}
    for M in (M_PRE, M_POST):
        x = gen((M, N), 1, 1.0, T)
        errs["M=%d" % M] = rel(ops.colsum(x), x.double().sum(0))
    report("colsum %s N=%d" % (T, N), errs)
    assert max(errs.values()) < 1e-5, errs


def test_abs_pos_resize_from_the_pretraining_grid_at_vit_huge_width():
    """pa_pos_fwd / pa_pos_bwd: the 16 x 16 pre-training position grid (224 / 14) resized bicubically to 64 x 32 at D = 1280, against
    F.interpolate and its autograd in fp64; test_abs_pos_resize_operator_sparse_rows_fwd_bwd's gate."""
    src = CFG.pretrain_img_size // P
    S = src * src
    M = hostmath.abs_pos_operator(src, HP, WP)
    dev = lambda t: (torch.from_numpy(t[0]).to(DEV), torch.from_numpy(t[1]).to(DEV))
    fwd, bwd = dev(hostmath.sparse_rows(M)), dev(hostmath.sparse_rows(M.T))
    pe = gen((S, D), 1)
    pos = ops.pos_fwd(fwd, pe, L, D)
    pe64 = pe.double().clone().requires_grad_(True)
    ref = F.interpolate(pe64.reshape(1, src, src, D).permute(0, 3, 1, 2), size=(HP, WP), mode="bicubic", align_corners=False)
    ref = ref.permute(0, 2, 3, 1).reshape(L, D)
    gx, gy = gen((L, D), 2), gen((L, D), 3)
    dpe = torch.empty((S, D), device=DEV)
    ops.pos_bwd(bwd, gx, gy, dpe, S, D)
    ref.backward((gx + gy).double())
    errs = {"pos_fwd": rel(pos, ref.detach()), "pos_bwd": rel(dpe, pe64.grad)}
    report("abs pos %dx%d -> %dx%d D=%d" % (src, src, HP, WP, D), errs)
    assert max(errs.values()) < 2e-6, errs
