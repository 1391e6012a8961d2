"""Decoder backward over the token rows the loss mask leaves live (include/painter_hip.h "live rows").

The loss is taken over masked patches only, the decoder tail is point-wise per pixel and the 3 x 3 convolution has a one-pixel halo, so the
gradient dE entering decoder_embed is exactly zero on every token without a masked patch in its 3 x 3 grid neighbourhood.  The live-row route
compacts the other rows and runs both decoder_embed GEMMs and the bias sum over them alone.  Checked here:

  map       the live-row map against a numpy dilation + cumulative sum, exactly;
  premise   the dense dE really is zero on the dead rows, and the compact dE holds the live rows of the dense one bit for bit;
  dgrad     the compact data gradient scattered back = the dense launch on the same rows, bit for bit; dead rows zero; NaN behind the
            padded rows is never read;
  wgrad     the weight gradient and the bias sum over the compact rows against fp64, at the gate of test_gemm256_bf16_tight_gates_against_fp64
            (5e-6 * sqrt(contraction length)) and at most 1.5 x the dense route's own error on the same operands; twice for bit-stability;
  model     switch on versus off (pa_debug_set knob 17): loss, pred and every gradient equal, except decoder_embed.weight / .bias, which sum
            the same non-zero terms grouped differently and are held to the same gate.

Equality is torch.equal on values wherever zeros are involved: the sign of an exact zero is the one thing allowed to differ."""
import math
import random

import numpy as np
import pytest
import torch

from oracle import painter_oracle as O

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from painter_amd import ops
    from painter_amd.masking_generator import MaskingGenerator
    from tests.test_droppath_skip_gpu import build, drop_override, step

DEV = "cuda"
BF = torch.bfloat16
NAN = float("nan")


@pytest.fixture(autouse=True)
def _restore_switch():
    old = ops.decoder_rows() if torch.cuda.is_available() else None
    yield
    if old is not None:
        ops.decoder_rows(old)


def gen(shape, seed, scale=1.0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype).to(DEV)


def bits(t):
    return t.contiguous().view(torch.uint8)


def pad128(n):
    return (n + 127) // 128 * 128


def grid_masks(Hp, Wp):
    """name -> uint8 [Hp, Wp]"""
    m = {k: np.zeros((Hp, Wp), dtype=np.uint8) for k in ("empty", "corner", "last_col", "last_patch", "checker", "bottom_half")}
    m["full"] = np.ones((Hp, Wp), dtype=np.uint8)
    m["corner"][0, 0] = 1
    m["last_col"][Hp // 2 - 1, Wp - 1] = 1          # must not wrap into column 0 of the next grid row
    m["last_patch"][Hp - 1, Wp - 1] = 1            # (of sample 0: must not leak into the first patches of sample 1)
    m["checker"][::2, ::2] = 1
    m["checker"][1::2, 1::2] = 1
    m["bottom_half"][Hp // 2:, :] = 1
    return m


def batch_masks(Hp, Wp, B):
    """name -> uint8 [B, L]: sample 0 carries the named mask, the other samples carry other ones (a different mask per sample)"""
    gm = grid_masks(Hp, Wp)
    names = list(gm)
    out = {}
    for i, k in enumerate(names):
        rows = [gm[k]] + [gm["empty"] if k == "last_patch" else gm[names[(i + 2 * s + 1) % len(names)]] for s in range(1, B)]
        out[k] = np.stack([r.reshape(-1) for r in rows])
    return out


def live_ref(mask, B, Hp, Wp):
    """numpy: 3 x 3 dilation per sample (no wrap, no leak), then the cumulative sum -> (rowmap, live list)"""
    m = np.broadcast_to(mask.reshape(-1, Hp, Wp), (B, Hp, Wp)).astype(bool)
    p = np.zeros((B, Hp + 2, Wp + 2), dtype=bool)
    p[:, 1:-1, 1:-1] = m
    d = np.zeros((B, Hp, Wp), dtype=bool)
    for di in range(3):
        for dj in range(3):
            d |= p[:, di:di + Hp, dj:dj + Wp]
    d = d.reshape(-1)
    rowmap = np.where(d, np.cumsum(d) - 1, -1).astype(np.int32)
    return rowmap, np.nonzero(d)[0].astype(np.int32)


# ------------------------------------------------------------------------------------------------ the map
@pytest.mark.parametrize("Hp,Wp", [(8, 4), (6, 5)])
def test_live_row_map_equals_numpy_dilation(Hp, Wp):
    B = 3
    cases = [(k, v) for k, v in batch_masks(Hp, Wp, B).items()]
    cases += [("shared " + k, v.reshape(1, -1)) for k, v in grid_masks(Hp, Wp).items()]
    for name, mask in cases:
        rowmap, live, count = ops.live_rows(torch.from_numpy(mask.copy()).to(DEV), B, Hp, Wp)
        rm, lv = live_ref(mask, B, Hp, Wp)
        n = int(count.item())
        assert n == lv.shape[0], name
        assert np.array_equal(rowmap.cpu().numpy(), rm), name
        assert np.array_equal(live.cpu().numpy()[:n], lv), name
    # the two traps by value: a patch in the last column does not reach column 0 of the next row; sample 0's last patch does not reach sample 1
    rm, _ = live_ref(grid_masks(Hp, Wp)["last_col"].reshape(1, -1), 1, Hp, Wp)
    assert rm[(Hp // 2) * Wp] == -1 and rm[(Hp // 2 - 1) * Wp + Wp - 1] >= 0
    rm, _ = live_ref(batch_masks(Hp, Wp, B)["last_patch"], B, Hp, Wp)
    assert (rm[Hp * Wp:] == -1).all() and rm[Hp * Wp - 1] >= 0


# ------------------------------------------------------------------------------------------------ the premise
def _tail_inputs(B, Hp, Wp, P):
    Hi, Wi = Hp * P, Wp * P
    pred, tgts = gen((B, 3, Hi, Wi), 1), gen((B, 3, Hi, Wi), 2)
    valid = (torch.rand((B, 3, Hi, Wi), generator=torch.Generator().manual_seed(3)) < 0.9).float().to(DEV)
    dloss = torch.full((1,), 1.5, device=DEV)
    loss_out = torch.tensor([0.3, 41.0], device=DEV)
    y3 = gen((B, Hi, Wi, 64), 4, 1.0, BF)
    gamma, beta, w1 = gen((64,), 5).abs() + 0.5, gen((64,), 6, 0.3), gen((3, 64), 7, 0.2)
    _, wf = ops.conv3x3_pack(gen((64, 64, 3, 3), 8, 0.05), BF)
    return pred, tgts, valid, dloss, loss_out, y3, gamma, beta, w1, wf


@pytest.mark.parametrize("Hp,Wp", [(4, 3), (4, 4)])          # 4 x 3 (48 pixels wide): the gather engine; 4 x 4: the tile kernel and its dead-tile exit
def test_dense_dE_is_zero_on_dead_rows_and_compact_dE_holds_the_live_rows(Hp, Wp):
    B, P = 2, 16
    pred, tgts, valid, dloss, loss_out, y3, gamma, beta, w1, wf = _tail_inputs(B, Hp, Wp, P)
    M, Mp = B * Hp * Wp, pad128(B * Hp * Wp) + 128          # (one more block of rows than the entry point asks for: nobody may touch it)
    for name, mask in batch_masks(Hp, Wp, B).items():
        mask_u8 = torch.from_numpy(mask.copy()).to(DEV)
        dpred = ops.loss_bwd(pred, tgts, valid, mask_u8, dloss, loss_out, P, "smoothl1")
        dy3, _ = ops.decoder_tail_bwd_pointwise(dpred, y3, gamma, beta, w1, 1e-6)
        dE = ops.conv3x3_dgrad_unshuffle(dy3, wf, B, Hp, Wp, P)
        assert bool(torch.isfinite(dE.float()).all()), name
        rowmap, live, count = ops.live_rows(mask_u8, B, Hp, Wp)
        rm, lv = live_ref(mask, B, Hp, Wp)
        n = lv.shape[0]
        dead = torch.from_numpy(rm < 0).to(DEV)
        assert float(dE[dead].float().abs().sum()) == 0.0, name                      # the premise of the whole route
        if name not in ("empty",):
            assert float(dE.float().abs().sum()) > 0.0, name
        buf = torch.full((Mp, P * P * 64), NAN, dtype=BF, device=DEV)
        ops.conv3x3_dgrad_unshuffle_live(dy3, wf, rowmap, count, B, Hp, Wp, P, out=buf[:pad128(M)])
        torch.cuda.synchronize()
        assert torch.equal(bits(buf[:n]), bits(dE[torch.from_numpy(lv).long().to(DEV)])), name
        assert float(buf[n:pad128(n)].float().abs().sum()) == 0.0, name              # zero padding up to 128 rows (NaN would fail)
        assert bool(torch.isnan(buf[pad128(n):].float()).all()), name                # rows beyond: untouched


# ------------------------------------------------------------------------------------------------ data gradient
@pytest.mark.parametrize("width", [256, 512])
def test_compact_data_gradient_scattered_back_equals_the_dense_launch(width):
    M, Kc = 700, 256
    a = gen((pad128(M), Kc), 11, 1.0, BF)
    w = gen((Kc, width), 12, 0.05, BF)
    dense = ops.linear_dgrad(a[:M], w)
    for count in (0, 1, 255, 256, 257, 700):
        perm = torch.randperm(M, generator=torch.Generator().manual_seed(100 + count))[:count]
        lv = torch.sort(perm).values.to(torch.int32)
        rm = torch.full((M,), -1, dtype=torch.int32)
        rm[lv.long()] = torch.arange(count, dtype=torch.int32)
        live = torch.zeros(M, dtype=torch.int32)
        live[:count] = lv
        an = a.clone()
        an[pad128(count):] = NAN
        out = torch.full((M, width), NAN, dtype=BF, device=DEV)
        ops.linear_dgrad(an, w, out=out, live=(live.to(DEV), rm.to(DEV), torch.tensor([count], dtype=torch.int32, device=DEV)))
        torch.cuda.synchronize()
        tag = (width, count)
        assert bool(torch.isfinite(out.float()).all()), tag
        assert torch.equal(bits(out[lv.long().to(DEV)]), bits(dense[:count])), tag
        dead = (rm < 0).to(DEV)
        assert float(out[dead].float().abs().sum()) == 0.0, tag


# ------------------------------------------------------------------------------------------------ weight gradient and column sum
def _rel64(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def test_compact_weight_gradient_and_column_sum_against_fp64():
    M, N, K = 640, 256, 256
    dy0, x0 = gen((M, N), 21, 1.0, BF), gen((M, K), 22, 1.0, BF)
    for count in (0, 1, 127, 128, 129, 640):
        pad = pad128(count)
        dy, x = dy0.clone(), x0.clone()
        dy[count:pad] = 0
        x[count:pad] = 0
        dy[pad:] = NAN
        x[pad:] = NAN
        cnt = torch.tensor([count], dtype=torch.int32, device=DEV)
        dw = ops.linear_wgrad_live(dy, x, cnt)
        db = ops.colsum_live(dy, cnt)
        dw2, db2 = ops.linear_wgrad_live(dy, x, cnt), ops.colsum_live(dy, cnt)
        torch.cuda.synchronize()
        assert torch.equal(bits(dw), bits(dw2)) and torch.equal(bits(db), bits(db2)), count
        assert bool(torch.isfinite(dw).all()) and bool(torch.isfinite(db).all()), count
        if count == 0:
            assert float(dw.abs().sum()) == 0.0 and float(db.abs().sum()) == 0.0
            continue
        ref_w = dy[:count].double().t() @ x[:count].double()
        ref_b = dy[:count].double().sum(0)
        # the dense route on the same operands: the full-length kernels over the zero-padded rows
        dense_w, dense_b = ops.linear_wgrad(dy[:pad], x[:pad]), ops.colsum(dy[:count])
        gate = 5e-6 * math.sqrt(count)
        for what, got, dense, ref in (("weight", dw, dense_w, ref_w), ("bias", db, dense_b, ref_b)):
            e_live, e_dense = _rel64(got, ref), _rel64(dense, ref)
            print("decoder live rows, count %d, %s: error vs fp64 compact %.3e, dense %.3e (gate %.3e)" % (count, what, e_live, e_dense, gate))
            assert e_live < gate, (count, what, e_live, gate)
            assert e_live <= 1.5 * e_dense, (count, what, e_live, e_dense)


# ------------------------------------------------------------------------------------------------ whole model
LOOSE = ("decoder_embed.weight", "decoder_embed.bias")


def _both(fn):
    ops.decoder_rows(1)
    off = fn()
    ops.decoder_rows(2)
    on = fn()
    torch.cuda.synchronize()
    return off, on


def _compare(off, on, tag, rows, loose=LOOSE):
    assert off.keys() == on.keys(), tag
    gate = 5e-6 * math.sqrt(rows)
    for k in off:
        assert bool(torch.isfinite(off[k]).all()) and bool(torch.isfinite(on[k]).all()), (tag, k)
        if k in loose:
            d = _rel64(on[k], off[k])
            print("decoder live rows, model %s: %s on vs off %.3e (gate %.3e)" % (tag, k, d, gate))
            assert d < gate, (tag, k, d, gate)
        else:
            assert torch.equal(off[k], on[k]), (tag, k)


def _block_mask(grid, seed):
    random.seed(seed)
    np.random.seed(seed)
    L = grid[0] * grid[1]
    return MaskingGenerator(tuple(grid), L // 2, min_num_patches=2, max_num_patches=L // 4)().reshape(-1)


def test_model_step_equal_with_and_without_live_rows():
    cfg = O.small_config()
    batch = 2
    L = cfg.grid[0] * cfg.grid[1]
    m = build(cfg, 81, "bf16")
    m._drop_override = drop_override(cfg, batch, 82)
    imgs, tgts, half, valid = O.synthetic_batch(cfg, batch, 83, "half")
    block = torch.from_numpy(np.stack([_block_mask(cfg.grid, 84 + b) for b in range(batch)])).to(torch.int32)
    masks = {"bottom_half": half, "block": block, "all": torch.ones_like(half), "none": torch.zeros_like(half)}
    assert ops.decoder_live_ok(BF, batch, cfg.grid[0], cfg.grid[1], cfg.patch_size, 4 * cfg.embed_dim)          # the route under test really runs
    for name, mask in masks.items():
        off, on = _both(lambda: step(m, cfg, imgs, tgts, mask, valid))
        _compare(off, on, name, batch * L)
        assert len(off) > 4 + 12 * cfg.depth and all(k in off for k in LOOSE)
        if name == "none":
            assert float(on["decoder_embed.weight"].abs().sum()) == 0.0 and float(on["decoder_embed.bias"].abs().sum()) == 0.0
    # a partly frozen model (decoder and last block trained)
    for pname, p in m.named_parameters():
        p.requires_grad_(pname.startswith("decoder_") or pname.startswith("blocks.%d." % (cfg.depth - 1)))
    off, on = _both(lambda: step(m, cfg, imgs, tgts, block, valid))
    _compare(off, on, "partly frozen", batch * L)


def test_seggpt_step_with_shared_mask_equal_with_and_without_live_rows():
    cfg = O.small_config(seggpt=True)
    n = 2
    L = cfg.grid[0] * cfg.grid[1]
    m = build(cfg, 91, "bf16")
    m._drop_override = drop_override(cfg, n, 92)
    imgs, tgts, _, valid = O.synthetic_batch(cfg, n, 93, "half")
    mask = torch.zeros(1, L)
    mask[:, L // 2:] = 1
    seg_type = torch.ones(n, 1)
    seg_type[0] = 0
    off, on = _both(lambda: step(m, cfg, imgs, tgts, mask, valid, seg_type, 1))
    _compare(off, on, "seggpt", n * L)


def test_gradient_on_pred_patch_keeps_the_dense_route():
    """A gradient on the returned pred_patch makes every row live: the dense route runs whatever the switch says -- the same bits everywhere."""
    cfg = O.small_config()
    batch = 2
    m = build(cfg, 95, "bf16")
    m._drop_override = drop_override(cfg, batch, 96)
    imgs, tgts, mask, valid = O.synthetic_batch(cfg, batch, 97, "half")
    wgt = gen((batch, cfg.grid[0] * cfg.grid[1], 3 * cfg.patch_size ** 2), 98, 1e-3)

    def run():
        for p in m.parameters():
            p.grad = None
        loss, pred, _ = m(imgs.cuda(), tgts.cuda(), bool_masked_pos=mask.reshape(batch, *cfg.grid).cuda(), valid=valid.clone().cuda())
        (loss + (pred * wgt).sum()).backward()
        torch.cuda.synchronize()
        return {name: p.grad.clone() for name, p in m.named_parameters() if p.grad is not None}

    off, on = _both(run)
    _compare(off, on, "dpatch", 1, loose=())
    # every token row of dE is non-zero here, the dead ones included
    assert float(on["decoder_embed.bias"].abs().sum()) > 0.0
