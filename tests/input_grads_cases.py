"""Inputs of the input-gradient cases (tests/golden/make_golden_input_grads.py writes tests/golden/input_grads.npz from them with the
unmodified reference; tests/test_input_grads_golden_cpu.py and tests/test_input_grads_gpu.py rebuild the same inputs).  Parameters come
from oracle.painter_oracle.random_params(cfg, seed): the fixture stores seeds and results only."""
import torch

from oracle import painter_oracle as O

VITL_STRIDE = 97          # ViT-L: every 97th element of the flattened d imgs / d tgts
SAMPLE_STRIDE = 5         # the cases stored as strided samples (the fixture must stay below 1 MiB)


def _dark_target(cfg, tgts, b, seed):
    """Sample b's target nearly black (de-normalised values in [0, 1e-3)): its unmasked sum stays far below the ignore rule's 300
    (models_painter.py:446-448), so Painter zeroes its `valid` -- the loss ignores it, its target still feeds the encoder."""
    g = torch.Generator().manual_seed(seed)
    H, W = cfg.img_size
    mean = torch.tensor(O.IMAGENET_MEAN)[:, None, None]
    std = torch.tensor(O.IMAGENET_STD)[:, None, None]
    tgts[b] = (torch.rand(3, H, W, generator=g) * 1e-3 - mean) / std


def painter_case():
    """Painter small_config, B = 2, one seeded random 50 % mask, the ignore rule hitting sample 1.  -> (cfg, seed_p, imgs, tgts, mask, valid)."""
    cfg = O.small_config()
    imgs, tgts, mask, valid = O.synthetic_batch(cfg, 2, 51, "random")
    _dark_target(cfg, tgts, 1, 52)
    return cfg, 41, imgs, tgts, mask, valid


def pred_probe(cfg, batch, seed=53):
    """r of the objective loss + (pred_patch * r).sum()."""
    g = torch.Generator().manual_seed(seed)
    L = cfg.grid[0] * cfg.grid[1]
    return torch.randn(batch, L, 3 * cfg.patch_size ** 2, generator=g) * 1e-2


def seggpt_case():
    """SegGPT small_config, N = 3 prompts, feature ensemble from block 0 (merge_between_batch = 0), bottom-half mask shared by the prompts,
    both segmentation types.  -> (cfg, seed_p, imgs, tgts, mask [1, L], valid, seg_type [N, 1], merge)."""
    cfg = O.small_config(seggpt=True)
    imgs, tgts, _, valid = O.synthetic_batch(cfg, 3, 54, "half")
    L = cfg.grid[0] * cfg.grid[1]
    mask = torch.zeros(1, L)
    mask[:, L // 2:] = 1
    seg_type = torch.ones(3, 1)
    seg_type[0] = 0
    return cfg, 43, imgs, tgts, mask, valid, seg_type, 0


def h14_case():
    """Patch 14 (the generic input-gradient path): h14_small_config at depth 24 (the reference's own taps), B = 2, random mask."""
    cfg = O.h14_small_config(depth=24)
    imgs, tgts, mask, valid = O.synthetic_batch(cfg, 2, 55, "random")
    return cfg, 45, imgs, tgts, mask, valid


def vitl_case():
    """ViT-L 896 x 448, B = 1: the inputs of tests/golden/painter_vitl.npz."""
    cfg = O.vit_large_config()
    imgs, tgts, mask, valid = O.synthetic_batch(cfg, 1, 1234, "random")
    return cfg, 1, imgs, tgts, mask, valid
