"""The two-stream backward (engine._Streams: parameter gradients on a side stream) against the one-stream backward: the same step with
HotPath.use_side_stream off and on gives the same loss and the same gradients, bit for bit, with the same key sets.

The premise: no kernel, argument or split count depends on the stream -- the side-stream sizing knobs are set once at import, not by
use_side_stream, and no bf16 kernel uses atomics -- so any difference is an ordering fault between the streams (a missing wait, a buffer
recycled while the other stream still reads it).  The cases are the smallest shapes that reach each special ordering path."""
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

BF = torch.bfloat16


def _block_masks(cfg, batch, seed):
    out = []
    L = cfg.grid[0] * cfg.grid[1]
    for b in range(batch):
        random.seed(seed + b)
        np.random.seed(seed + b)
        out.append(MaskingGenerator(tuple(cfg.grid), L // 2, min_num_patches=2, max_num_patches=L // 4)().reshape(-1))
    return torch.from_numpy(np.stack(out)).to(torch.int32)


def _one_and_two_streams(m, fn):
    """fn() with the one-stream backward, then with the two-stream backward"""
    old = m._hot.use_side_stream
    try:
        m._hot.use_side_stream = False
        one = fn()
        m._hot.use_side_stream = True
        two = fn()
    finally:
        m._hot.use_side_stream = old
    return one, two


def _assert_equal(one, two, tag, min_keys):
    assert one.keys() == two.keys(), tag
    assert len(one) >= min_keys, (tag, len(one))
    for k in one:
        assert bool(torch.isfinite(one[k]).all()), (tag, k)
        assert torch.equal(one[k], two[k]), (tag, k)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_painter_step_with_block_mask_and_droppath(dtype):
    """bf16: the live-row decoder route with its shared rowmap / live / count allocation, the deferred LayerNorm reductions through the
    workspace ring (24 blocks > LN_RING) and the flat small-gradient buffers.  fp32: the dense decoder route and the generic kernels."""
    cfg = O.small_config()
    batch = 2
    m = build(cfg, 101, dtype)
    assert cfg.depth > m._hot.LN_RING
    m._drop_override = drop_override(cfg, batch, 102)
    imgs, tgts, _, valid = O.synthetic_batch(cfg, batch, 103, "half")
    mask = _block_masks(cfg, batch, 104)
    live = ops.decoder_live_ok(BF if dtype == "bf16" else torch.float32, batch, cfg.grid[0], cfg.grid[1], cfg.patch_size, 4 * cfg.embed_dim)
    assert live == (dtype == "bf16")
    one, two = _one_and_two_streams(m, lambda: step(m, cfg, imgs, tgts, mask, valid))
    _assert_equal(one, two, dtype, 4 + 12 * cfg.depth + 1)


def test_seggpt_step_with_feature_ensemble_and_shared_mask():
    """The ensemble branch of the backward, whose attention dY is re-written into the dyA buffer, and a [1, L] mask."""
    cfg = O.small_config(seggpt=True)
    n = 2
    m = build(cfg, 111, "bf16")
    m._drop_override = drop_override(cfg, n, 112)
    imgs, tgts, _, valid = O.synthetic_batch(cfg, n, 113, "half")
    L = cfg.grid[0] * cfg.grid[1]
    mask = torch.zeros(1, L)
    mask[:, L // 2:] = 1
    seg_type = torch.ones(n, 1)
    seg_type[0] = 0
    one, two = _one_and_two_streams(m, lambda: step(m, cfg, imgs, tgts, mask, valid, seg_type, 1))
    _assert_equal(one, two, "seggpt", 4 + 12 * cfg.depth + 1)


def test_partly_frozen_layers():
    """param_grads computes what is wanted of {weight gradient, bias sum}: every weight frozen with the biases trained, the reverse, and only
    the decoder and the last block trained."""
    cfg = O.small_config()
    batch = 2
    m = build(cfg, 121, "bf16")
    m._drop_override = drop_override(cfg, batch, 122)
    imgs, tgts, _, valid = O.synthetic_batch(cfg, batch, 123, "half")
    mask = _block_masks(cfg, batch, 124)
    names = [n for n, _ in m.named_parameters()]
    freezes = {
        "weights frozen": lambda n: not n.endswith(".weight"),
        "biases frozen": lambda n: n.endswith(".weight"),
        "decoder and last block": lambda n: n.startswith("decoder_") or n.startswith("blocks.%d." % (cfg.depth - 1)),
    }
    for tag, trained in freezes.items():
        for n, p in m.named_parameters():
            p.requires_grad_(trained(n))
        one, two = _one_and_two_streams(m, lambda: step(m, cfg, imgs, tgts, mask, valid))
        _assert_equal(one, two, tag, 5)
        assert all(trained(k) for k in one if k in names), tag


def test_wide_grid_with_relpos_partials():
    """A 56 x 28 token grid at small width: the generation-3 dQ kernel's rel-pos partials, reduced on the side stream, and the gemm256 shapes."""
    cfg = O.OracleConfig(img_size=(896, 448), patch_size=16, embed_dim=128, depth=16, num_heads=2, taps=(3, 7, 11, 15))
    m = build(cfg, 131, "bf16")
    m._drop_override = drop_override(cfg, 1, 132)
    imgs, tgts, _, valid = O.synthetic_batch(cfg, 1, 133, "half")
    mask = _block_masks(cfg, 1, 134)
    c0 = ops.attn_launch_counts()
    one, two = _one_and_two_streams(m, lambda: step(m, cfg, imgs, tgts, mask, valid))
    c1 = ops.attn_launch_counts()
    assert c1["fwd"][2] > c0["fwd"][2] and c1["bwd"][2] > c0["bwd"][2]          # the generation-3 kernels (partial route) really ran
    _assert_equal(one, two, "wide grid", 4 + 12 * cfg.depth + 1)
