"""Shared inputs of the scoring tests: seeded painted semantic pictures with ground-truth label maps, depth pictures with ground-truth
depth maps, and the case lists of the fixture (tests/golden/painter_score.npz).  TEST INFRASTRUCTURE.

A semantic case is what a network paints for one photo -- flat regions in palette colours under a box blur and Gaussian noise -- and a
label map that agrees with it inside the regions and not along their borders: the clean regions' labels, each pixel taking the label of a
seeded neighbour up to two pixels away, with a band of the ignore label 255 across the picture.  K = 133 pictures are
tests/painter_pano_cases.picture_pair's; K = 150 pictures are painted here in the ADE20K colours of tests/golden/painter_eval_io.npz."""
import os

import numpy as np

from tests import painter_pano_cases as P

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
IGNORE = 255


def ade_palette():
    """int32 [150][3]: the colour list of data/ade20k/gen_color_ade20k_sem.py as the unmodified reference produced it."""
    return np.load(os.path.join(GOLDEN, "painter_eval_io.npz"))["palette"]


def coco_palette():
    from painter_amd.painter_engine import semantic_palette
    return semantic_palette()


def _labels_of(clean, palette):
    """A picture whose pixels are palette colours exactly -> uint8 [h][w] labels."""
    code = lambda a: (a[..., 0].astype(np.int64) << 16) | (a[..., 1].astype(np.int64) << 8) | a[..., 2].astype(np.int64)
    pal = code(np.asarray(palette).astype(np.int64))
    order = np.argsort(pal)
    at = np.searchsorted(pal[order], code(clean))
    labels = order[np.minimum(at, len(pal) - 1)]
    assert (pal[labels] == code(clean)).all()
    return labels.astype(np.uint8)


def _ground_truth(labels, seed, band=True):
    """Blurred label regions: every pixel takes the label of a neighbour up to two pixels away; three rows of the ignore label."""
    h, w = labels.shape
    rng = np.random.default_rng(seed + 77)
    yy, xx = np.mgrid[0:h, 0:w]
    gt = labels[np.clip(yy + rng.integers(-2, 3, (h, w)), 0, h - 1), np.clip(xx + rng.integers(-2, 3, (h, w)), 0, w - 1)].copy()
    if band:
        gt[h // 3:h // 3 + 3] = IGNORE
    return gt


def painted(seed, h, w, palette, n_obj=12, blur=1, noise=3.0):
    """Ellipses over five vertical bands, every region in the colour of a random class of `palette` -> (picture uint8 [h][w][3] after
    blur and noise, labels uint8 [h][w] of the clean regions)."""
    pal = np.asarray(palette, dtype=np.float64)
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    labels = np.zeros((h, w), np.uint8)
    edges = np.linspace(0, w, 6).astype(int)
    for b, c in enumerate(rng.choice(len(pal), 5, replace=False)):
        labels[:, edges[b]:edges[b + 1]] = c
    for _ in range(n_obj):
        cy, cx = rng.uniform(0.05, 0.95) * h, rng.uniform(0.05, 0.95) * w
        ry, rx = rng.uniform(0.06, 0.25) * h, rng.uniform(0.06, 0.25) * w
        labels[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0] = rng.integers(0, len(pal))
    img = pal[labels]
    if blur:
        k = 2 * blur + 1
        pad = np.pad(img, ((blur, blur), (blur, blur), (0, 0)), mode="edge")
        img = sum(pad[dy:dy + h, dx:dx + w] for dy in range(k) for dx in range(k)) / (k * k)
    img = img + rng.normal(0.0, noise, img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8), labels


def semseg_case(which, seed, h, w, noise=3.0):
    """which: "coco" (K = 133) or "ade" (K = 150) -> (picture uint8 [h][w][3], ground truth uint8 [h][w], palette [K][3])."""
    if which == "coco":
        pal = coco_palette()
        pic = P.picture_pair(seed, h, w, noise=noise)[0]
        labels = _labels_of(P.picture_pair(seed, h, w, blur=0, noise=0.0)[0], pal)
    else:
        pal = ade_palette()
        pic, labels = painted(seed, h, w, pal, noise=noise)
    return pic, _ground_truth(labels, seed), pal


def synthetic_palette(k, seed=9):
    """k distinct integer colours."""
    codes = np.random.default_rng(seed).choice(1 << 24, k, replace=False)
    return np.stack([codes >> 16, (codes >> 8) & 255, codes & 255], -1).astype(np.float32)


def noisy_case(seed, h, w, palette, ignore=True):
    """A picture near the palette's colours pixel by pixel and labels that agree with it about half of the time."""
    rng = np.random.default_rng(seed)
    k = len(palette)
    labels = rng.integers(0, k, (h, w))
    pic = np.clip(np.asarray(palette)[labels] + rng.integers(-6, 7, (h, w, 3)), 0, 255).astype(np.uint8)
    gt = np.where(rng.random((h, w)) < 0.5, labels, rng.integers(0, k, (h, w)))
    if ignore:
        gt[rng.random((h, w)) < 0.05] = IGNORE
    return pic, gt.astype(np.uint8)


# name -> (palette, seed, height, width, dist_types).  96 x 128 and 61 x 83 (5063 pixels: no multiple of 64) per evaluator; all three
# distances on one case.
SEMSEG = {
    "coco_96x128": ("coco", 1, 96, 128, ("abs",)),
    "coco_61x83": ("coco", 3, 61, 83, ("abs", "square", "mean")),
    "ade_96x128": ("ade", 5, 96, 128, ("abs",)),
    "ade_61x83": ("ade", 7, 61, 83, ("abs",)),
}


def semseg_fixture_case(name):
    which, seed, h, w, _ = SEMSEG[name]
    return semseg_case(which, seed, h, w)


def depth_case(seed, h, w, noise=400.0):
    """-> (prediction int32 [h][w], ground truth uint16 [h][w]), millimetres.  The ground truth is a smooth field of 0.4 .. 11 m with a
    block of zeros (no measurement), the value 1 (exactly min_depth) and values at and above 10 m; the prediction is the ground truth
    plus noise clipped to 0 .. 10000 as the decode writes it, with zeros and a patch above 10 m."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    field = 400 + 10600 * (0.5 + 0.5 * np.sin(yy / max(h, 2) * 3.1 + seed) * np.cos(xx / max(w, 2) * 4.3))
    gt = np.clip(np.rint(field + rng.normal(0, 30, (h, w))), 0, 65535).astype(np.uint16)
    gt[h // 5:h // 5 + max(h // 8, 1), w // 6:w // 6 + max(w // 5, 1)] = 0
    flat = gt.reshape(-1)
    spots = rng.choice(flat.size, min(24, flat.size), replace=False)
    flat[spots[0::4]], flat[spots[1::4]], flat[spots[2::4]], flat[spots[3::4]] = 1, 10000, 10001, 9999
    pred = np.clip(np.rint(gt.astype(np.float64) + rng.normal(0, noise, (h, w))), 0, 10000).astype(np.int32)
    pred[rng.random((h, w)) < 0.01] = 0
    patch = pred[h // 2:h // 2 + max(h // 10, 1), w // 2:w // 2 + max(w // 10, 1)]
    patch[...] = 10000 + rng.integers(1, 2500, patch.shape)
    return pred, gt


# name -> (seed, height, width, dict of the evaluation's arguments): the 480 x 640 pictures of NYUv2 with `--max_depth_eval 10
# --eigen_crop` and with the script's defaults, and a small odd size without a crop.
DEPTH = {
    "nyu_eigen": (11, 480, 640, dict(max_depth=10.0, crop="eigen")),
    "nyu_defaults": (12, 480, 640, {}),
    "odd_eigen_range": (13, 37, 53, dict(max_depth=10.0)),
    "odd_defaults": (14, 37, 53, {}),
}


def depth_fixture_case(name):
    seed, h, w, _ = DEPTH[name]
    return depth_case(seed, h, w)
