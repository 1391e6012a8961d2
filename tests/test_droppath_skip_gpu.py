"""DropPath skipping (include/painter_hip.h, ABI 7): the attention workgroups and GEMM row tiles of samples whose DropPath factor is 0 do
no work.  Every check here compares the SAME call with skipping switched on and off (pa_debug_set knob 16):

  kernel level   kept samples bit-identical; dropped samples hold the documented values (zeros / the epilogue of a zero accumulator);
                 with NaN written over the inputs of the dropped samples the kept outputs do not move and the dropped outputs stay
                 finite -- which fails if skipping is silently inactive, because then the NaNs are read and come out;
  model level    loss, pred, every parameter gradient and the input gradients are equal element for element.

Equality is torch.equal on values: the sign of an exact zero is the one thing allowed to differ."""
from functools import partial

import pytest
import torch
import torch.nn as nn

from oracle import painter_oracle as O

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from painter_amd import models_painter, models_seggpt, ops
    from painter_amd._lib import EPI_BIAS, EPI_BIAS_RESID

DEV = "cuda"
BF = torch.bfloat16
KEEP = 1.0 / 0.9


@pytest.fixture(autouse=True)
def _restore_switch():
    old = ops.drop_skip() if torch.cuda.is_available() else None
    yield
    if old is not None:
        ops.drop_skip(old)


def gen(shape, seed, scale=1.0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype).to(DEV)


def patterns(n):
    """name -> list of dropped samples: nobody, sample 0, the last sample, two adjacent samples, every sample"""
    return {"none": [], "first": [0], "last": [n - 1], "adjacent": [n // 2 - 1, n // 2], "all": list(range(n))}


def factors(n, dropped):
    f = torch.full((n,), KEEP, dtype=torch.float32)
    f[dropped] = 0.0
    return f.to(DEV)


def runs(dropped):
    """maximal runs [a, b) of consecutive dropped samples"""
    out, d = [], sorted(dropped)
    for s in d:
        if out and out[-1][1] == s:
            out[-1][1] = s + 1
        else:
            out.append([s, s + 1])
    return out


def row_mask(n, rps, dropped, margin=0):
    """bool [n * rps]: rows of dropped samples, without the first and last `margin` rows of every dropped run"""
    m = torch.zeros(n * rps, dtype=torch.bool)
    for a, b in runs(dropped):
        lo, hi = a * rps + margin, b * rps - margin
        if hi > lo:
            m[lo:hi] = True
    return m.to(DEV)


def both(fn):
    """fn() with skipping off, then on"""
    ops.drop_skip(1)
    off = fn()
    ops.drop_skip(2)
    on = fn()
    torch.cuda.synchronize()
    return off, on


def beside_mfma_load(fn, ref, rounds=4, per_round=3):
    """fn() on the current stream while bf16 MFMA weight-gradient GEMMs run on a second stream: every result bit-identical to `ref`"""
    sdy, sx = gen((12544, 1024), 6, 1.0, BF), gen((12544, 1024), 7, 1.0, BF)
    side = torch.cuda.Stream()
    bad = torch.zeros((), dtype=torch.int64, device=DEV)
    for _ in range(rounds):
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                ops.linear_wgrad(sdy, sx)
        for _ in range(per_round):
            diff = torch.zeros((), dtype=torch.bool, device=DEV)
            for a, b in zip(fn(), ref):
                diff = diff | torch.ne(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)).any()
            bad += diff
        torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    return int(bad.item())


# ------------------------------------------------------------------------------------------------ GEMM row tiles
# (n samples, rows per sample, D, hidden): the two ViT-L stream widths of a B = 8 step, and a small shape whose samples are 2.5 tiles long
GEMM_SHAPES = [(8, 1568, 1024, 4096), (16, 1568, 1024, 4096), (4, 640, 256, 1024)]


def _gemm_ops(n, rps, D, hid):
    """name -> (K of the A operand, fn(A, factor vector or None) -> tuple of outputs).  A's dropped rows are what the test varies."""
    R = n * rps
    w_qkv, b_qkv = gen((3 * D, D), 11, 0.03, BF), gen((3 * D,), 12, 0.5)
    w_fc1, b_fc1 = gen((hid, D), 13, 0.03, BF), gen((hid,), 14, 0.5)
    w_proj, b_proj = gen((D, D), 15, 0.03, BF), gen((D,), 16, 0.5)
    w_fc2, b_fc2 = gen((D, hid), 17, 0.02, BF), gen((D,), 18, 0.5)
    resid = gen((R, D), 19)
    aux = torch.randint(0, 256, (R, hid), dtype=torch.uint8, generator=torch.Generator().manual_seed(20)).to(DEV)

    def fc2_dgrad(a, f):
        cs = torch.empty((hid,), dtype=torch.float32, device=DEV)
        dx = ops.linear_dgrad(a, w_fc2, gelu_aux=aux, colsum_out=cs, rowskip=f, rows_per_sample=rps)
        return dx, cs

    return {
        "qkv_fwd": (D, lambda a, f: (ops.linear_fwd(a, w_qkv, b_qkv, EPI_BIAS, rowskip=f, skip_rows_per_sample=rps),)),
        "fc1_gelu_fwd": (D, lambda a, f: ops.linear_gelu(a, w_fc1, b_fc1, need_aux=True, rowskip=f, rows_per_sample=rps)),
        "proj_resid_fwd": (D, lambda a, f: (ops.linear_fwd(a, w_proj, b_proj, EPI_BIAS_RESID, resid=resid, rowscale=f, rows_per_sample=rps, rowskip=f),)),
        "fc2_resid_fwd": (hid, lambda a, f: (ops.linear_fwd(a, w_fc2, b_fc2, EPI_BIAS_RESID, resid=resid, rowscale=f, rows_per_sample=rps, rowskip=f),)),
        "proj_dgrad": (D, lambda a, f: (ops.linear_dgrad(a, w_proj, rowskip=f, rows_per_sample=rps),)),
        "qkv_dgrad": (3 * D, lambda a, f: (ops.linear_dgrad(a, w_qkv, rowskip=f, rows_per_sample=rps),)),
        "fc1_dgrad": (hid, lambda a, f: (ops.linear_dgrad(a, w_fc1, rowskip=f, rows_per_sample=rps),)),
        "fc2_dgrad_gelu_colsum": (D, fc2_dgrad),
    }


@pytest.mark.parametrize("n,rps,D,hid", GEMM_SHAPES)
def test_gemm_row_tiles_of_dropped_samples_are_not_computed(n, rps, D, hid):
    R = n * rps
    table = _gemm_ops(n, rps, D, hid)
    for name, (K, fn) in table.items():
        dgrad = "dgrad" in name
        a0 = gen((R, K), 30 + K % 7, 1.0, BF)
        for pname, dropped in patterns(n).items():
            f = factors(n, dropped)
            drop_rows, deep_rows = row_mask(n, rps, dropped), row_mask(n, rps, dropped, 256)
            a = a0.clone()
            if dgrad:
                a[drop_rows] = 0          # a data gradient's dY rows of a dropped sample ARE zero (the LayerNorm backward multiplied them by the factor)
            off, on = both(lambda: fn(a, f))
            # what a skipped tile writes: the epilogue of a zero accumulator = the same call on zero A rows, skipping off
            az = a.clone()
            az[drop_rows] = 0
            ops.drop_skip(1)
            zero = fn(az, f)
            ops.drop_skip(2)
            tag = "%s %s n=%d" % (name, pname, n)
            for o_off, o_on, o_zero in zip(off, on, zero):
                if o_on.dim() == 1:          # the column sums of dX: zero rows add nothing
                    assert torch.equal(o_on, o_off), tag
                    continue
                assert torch.equal(o_on[~drop_rows].view(torch.uint8), o_off[~drop_rows].view(torch.uint8)), tag      # kept samples: the same bits
                # every row of a dropped sample holds either the ordinary result (a tile that also touches a kept sample) or the zero-accumulator
                # epilogue; the rows further than a tile from a kept sample hold the latter
                same = (o_on == o_off).all(dim=1) | (o_on == o_zero).all(dim=1)
                assert bool(same[drop_rows].all()), tag
                assert torch.equal(o_on[deep_rows], o_zero[deep_rows]), tag
            # NaN over the A rows of the dropped runs, except their first and last 256 rows (no tile of any plan that touches the remaining rows
            # reaches a kept sample): not read -> the kept outputs do not move, the outputs of those rows are finite
            if dropped:
                an = a.clone()
                an[deep_rows] = float("nan")
                assert bool(deep_rows.any())
                ops.drop_skip(2)
                nan_on = fn(an, f)
                torch.cuda.synchronize()
                for o_on, o_nan in zip(on, nan_on):
                    if o_on.dim() == 1:
                        assert torch.equal(o_nan, o_on), tag
                        continue
                    assert torch.equal(o_nan[~drop_rows].view(torch.uint8), o_on[~drop_rows].view(torch.uint8)), tag
                    assert bool(torch.isfinite(o_nan[deep_rows].float()).all()), tag
                    assert torch.equal(o_nan[deep_rows], o_on[deep_rows]), tag


def test_gemm_skipping_bitstable_beside_concurrent_mfma_kernels():
    n, rps, D, hid = GEMM_SHAPES[0]
    table = _gemm_ops(n, rps, D, hid)
    f = factors(n, [2, 3])
    ops.drop_skip(2)
    for name in ("fc1_gelu_fwd", "fc2_resid_fwd", "fc2_dgrad_gelu_colsum"):
        K, fn = table[name]
        a = gen((n * rps, K), 41, 1.0, BF)
        a[row_mask(n, rps, [2, 3])] = 0
        ref = fn(a, f)
        torch.cuda.synchronize()
        assert beside_mfma_load(lambda: fn(a, f), ref) == 0, name


# ------------------------------------------------------------------------------------------------ attention
ATTN_SHAPES = [(8, 16, 56), (16, 16, 56), (4, 2, 8)]          # (samples, heads, Hp); key rows of 28 tokens: the generation-3 kernels


def _attn_inputs(n, H, Hp):
    Wp, hd = 28, 64
    L = Hp * Wp
    qkv = gen((n * L, 3 * H * hd), 51, 1.0, BF)
    rh, rw = gen((2 * Hp - 1, hd), 52, 0.2), gen((2 * Wp - 1, hd), 53, 0.2)
    rcat, rcatT = ops.relpos_pack(rh, rw, Hp, Wp, BF), ops.relpos_pack_t(rh, rw, Hp, Wp, BF)
    dout = gen((n * L, H * hd), 54, 1.0, BF)
    return L, Wp, qkv, rcat, rcatT, dout


def _attn_step(qkv, rcat, rcatT, dout, f, n, L, H, Hp, Wp):
    out, lse, tables = ops.attn_fwd(qkv, rcat, n, L, H, Hp, Wp, 0.125, need_tables=True, rowskip=f)
    assert tables is not None          # the generation-3 kernels ran
    dqkv, part = ops.attn_bwd_core(qkv, rcat, rcatT, out, dout, lse, n, L, H, Hp, Wp, 0.125, tables=tables, rowskip=f)
    drcat = ops.attn_bwd_relpos(part, qkv, rcat.shape[0], n, L, H, Hp, Wp)
    return out, lse, tables, dqkv, drcat


@pytest.mark.parametrize("n,H,Hp", ATTN_SHAPES)
def test_attention_of_dropped_samples_is_not_computed(n, H, Hp):
    L, Wp, qkv, rcat, rcatT, dout0 = _attn_inputs(n, H, Hp)
    for pname, dropped in patterns(n).items():
        f = factors(n, dropped)
        drop_rows = row_mask(n, L, dropped)
        ds = torch.zeros(n, dtype=torch.bool, device=DEV)
        ds[dropped] = True
        dout = dout0.clone()
        dout[drop_rows] = 0               # the branch gradient of a dropped sample is zero
        off, on = both(lambda: _attn_step(qkv, rcat, rcatT, dout, f, n, L, H, Hp, Wp))
        tag = "%s n=%d" % (pname, n)
        per_sample = lambda t: t.reshape(n, -1)
        for k, (o_off, o_on) in enumerate(zip(off[:4], on[:4])):          # out, lse, tables, dqkv: per-sample blocks
            a, b = per_sample(o_off), per_sample(o_on)
            assert torch.equal(a[~ds].view(torch.uint8), b[~ds].view(torch.uint8)), (tag, k)          # kept samples: the same bits
            assert float(b[ds].float().abs().sum()) == 0.0, (tag, k)                                   # dropped samples: zeros
        assert float(per_sample(off[3])[ds].float().abs().sum()) == 0.0, tag          # (the premise: dO = 0 gives dq = dk = dv = 0 without skipping too)
        assert torch.equal(on[4], off[4]), tag                                         # the rel-pos table gradient
        if dropped:
            # NaN over ALL q / k / v / dO rows of the dropped samples: never read
            qn, dn = qkv.clone(), dout.clone()
            qn[drop_rows] = float("nan")
            dn[drop_rows] = float("nan")
            ops.drop_skip(2)
            nan_on = _attn_step(qn, rcat, rcatT, dn, f, n, L, H, Hp, Wp)
            torch.cuda.synchronize()
            for k, (o_on, o_nan) in enumerate(zip(on[:4], nan_on[:4])):
                a, b = per_sample(o_on), per_sample(o_nan)
                assert torch.equal(a[~ds].view(torch.uint8), b[~ds].view(torch.uint8)), (tag, k)
                assert bool(torch.isfinite(b[ds].float()).all()) and float(b[ds].float().abs().sum()) == 0.0, (tag, k)
            assert torch.equal(nan_on[4], on[4]), tag


def test_attention_skipping_bitstable_beside_concurrent_mfma_kernels():
    n, H, Hp = 4, 16, 56
    L, Wp, qkv, rcat, rcatT, dout = _attn_inputs(n, H, Hp)
    f = factors(n, [1, 2])
    dout[row_mask(n, L, [1, 2])] = 0
    ops.drop_skip(2)
    ref = _attn_step(qkv, rcat, rcatT, dout, f, n, L, H, Hp, Wp)
    torch.cuda.synchronize()
    assert beside_mfma_load(lambda: _attn_step(qkv, rcat, rcatT, dout, f, n, L, H, Hp, Wp), ref) == 0


# ------------------------------------------------------------------------------------------------ whole model
def build(cfg, seed, dtype):
    cls = models_seggpt.SegGPT if cfg.seggpt else models_painter.Painter
    m = cls(img_size=cfg.img_size, patch_size=cfg.patch_size, embed_dim=cfg.embed_dim, depth=cfg.depth, num_heads=cfg.num_heads,
            drop_path_rate=0.1, window_size=14, qkv_bias=True, mlp_ratio=4, norm_layer=partial(nn.LayerNorm, eps=1e-6),
            window_block_indexes=(), residual_block_indexes=[], use_rel_pos=True, out_feature="last_feat",
            decoder_embed_dim=cfg.decoder_embed_dim, loss_func=cfg.loss_func, compute_dtype=dtype,
            **({} if cfg.depth == 24 else {"feature_taps": cfg.taps}))
    m.load_state_dict(O.random_params(cfg, seed), strict=True)
    return m.cuda().train()


def drop_override(cfg, batch, seed):
    """Factor vectors with zeros before and after the stream merge, in both branches, different samples per branch, and one block (the one
    behind the merge) in which every sample of both branches is dropped."""
    g = torch.Generator().manual_seed(seed)
    over = [(None, None)]
    for i in range(1, cfg.depth):
        keep = 1.0 - 0.1 * i / (cfg.depth - 1)
        bc = 2 * batch if i <= cfg.merge_idx else batch
        pair = []
        for br in range(2):
            s = torch.floor(keep + torch.rand(bc, generator=g)) / keep
            if i in (1, cfg.merge_idx, cfg.merge_idx + 2, cfg.depth - 1):
                s[(i + br) % bc] = 0.0
            if i == cfg.merge_idx + 1:
                s[:] = 0.0
            pair.append(s.to(DEV).contiguous())
        over.append(tuple(pair))
    return over


def step(m, cfg, imgs, tgts, mask, valid, seg_type=None, merge=-1):
    for p in m.parameters():
        p.grad = None
    xi, xt = imgs.cuda().requires_grad_(True), tgts.cuda().requires_grad_(True)
    if cfg.seggpt:
        loss, pred, _ = m(xi, xt, mask.cuda(), valid.clone().cuda(), seg_type.cuda(), merge)
    else:
        loss, pred, _ = m(xi, xt, bool_masked_pos=mask.reshape(imgs.shape[0], *cfg.grid).cuda(), valid=valid.clone().cuda())
    loss.backward()
    torch.cuda.synchronize()
    out = {"loss": loss.detach().clone(), "pred": pred.detach().clone(), "d imgs": xi.grad, "d tgts": xt.grad}
    for name, p in m.named_parameters():
        if p.requires_grad and p.grad is not None:
            out[name] = p.grad.clone()
    return out


def assert_same(off, on, tag):
    assert off.keys() == on.keys(), tag
    for k in off:
        assert bool(torch.isfinite(off[k]).all()), (tag, k)
        assert torch.equal(off[k], on[k]), (tag, k)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("which", ["small", "vit_large"])
def test_model_step_equal_with_and_without_skipping(which, dtype):
    cfg = O.small_config() if which == "small" else O.vit_large_config()
    batch = 2
    m = build(cfg, 61, dtype)
    m._drop_override = drop_override(cfg, batch, 62)
    imgs, tgts, mask, valid = O.synthetic_batch(cfg, batch, 63, "half")
    counts0 = ops.attn_launch_counts()
    off, on = both(lambda: step(m, cfg, imgs, tgts, mask, valid))
    assert_same(off, on, (which, dtype))
    assert len(off) > 4 + 12 * cfg.depth          # every parameter gradient was compared
    if which == "vit_large" and dtype == "bf16":  # (the configuration in which the skipping kernels really run)
        c = ops.attn_launch_counts()
        assert c["fwd"][2] > counts0["fwd"][2] and c["bwd"][2] > counts0["bwd"][2]
    # a partly frozen model: only the decoder and the last block are trained
    for name, p in m.named_parameters():
        p.requires_grad_(name.startswith("decoder_") or name.startswith("blocks.%d." % (cfg.depth - 1)))
    off, on = both(lambda: step(m, cfg, imgs, tgts, mask, valid))
    assert_same(off, on, (which, dtype, "partly frozen"))
    assert 4 < len(off) < 4 + 12 * cfg.depth


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("which,merge", [("small", 0), ("small", 1), ("vit_large", 1)])
def test_seggpt_train_step_with_feature_ensemble_equal_with_and_without_skipping(which, merge, dtype):
    """Zeros in the attention factors of ensemble blocks: equal as well, because the engine passes no vector for those attention branches (a
    dropped sample's proj output still enters the other samples' group mean); their MLP branches, and the blocks in front of
    merge_between_batch, do skip."""
    cfg = O.small_config(seggpt=True) if which == "small" else O.vit_large_config(seggpt=True)
    n = 2
    m = build(cfg, 71, dtype)
    m._drop_override = drop_override(cfg, n, 72)
    imgs, tgts, _, valid = O.synthetic_batch(cfg, n, 73, "half")
    L = cfg.grid[0] * cfg.grid[1]
    mask = torch.zeros(1, L)
    mask[:, L // 2:] = 1
    seg_type = torch.ones(n, 1)
    seg_type[0] = 0
    off, on = both(lambda: step(m, cfg, imgs, tgts, mask, valid, seg_type, merge))
    assert_same(off, on, (which, merge, dtype))
