"""The definition of the pose keypoint decode, in numpy, slow and obvious: full float32 heat maps on purpose.  TEST INFRASTRUCTURE.

Two parts with two sources.
  * `heatmaps` restates TopDownCustom.forward_pseudo_test up to its `output_heatmap` (Painter/eval/mmpose_custom/model/top_down.py:
    163-258): classify by the (G, B) palette, heat = float32(R) / 255 on the pixel's own channel, flip_back of the flipped picture's
    heat maps, the one-column shift, `(a + b) / 2` in float32.  tests/golden/painter_pose.npz pins it to the unmodified file bit for
    bit (tests/golden/make_golden_painter_pose.py asserts equality on every case before it writes).
  * `peaks` states mmpose 0.x `keypoints_from_heatmaps(post_process='default', unbiased=False, use_udp=False)` with its
    `_get_max_preds`, and `to_image` its `transform_preds(use_udp=False)`.  mmpose is not available where this project is built, so that
    rule is TAKEN FROM mmpose's published source and could not be re-verified against it; for that part this file IS the definition.

Float32 addition decides ties: T[a] + T[b] with T[i] = float32(i) / 255 takes more than one value for one integer a + b (T[0] + T[3] !=
T[1] + T[2]), so the argmax and the neighbour signs are those of the float32 arrays below, not of integer sums."""
import numpy as np


def pose_palette(num_locations=17):
    """define_colors_gb_mean_sep (data/pipelines/custom_transform.py:10-33) plus the background row (top_down.py:28-30) -> int32 [n + 1][2]."""
    per = int(num_locations ** (1 / 2)) + 1
    sep = 256 // per
    rows = [(255 - (k // per) * sep, 255 - (k % per) * sep) for k in range(num_locations)] + [(0, 0)]
    return np.array(rows, np.int32)


def pair_table(flip_pairs, k):
    pair = np.arange(k, dtype=np.int32)
    for a, b in flip_pairs:
        pair[a], pair[b] = b, a
    return pair


def classify(pictures, palette):
    """uint8 [n][H][W][3] -> int64 [n][H][W]: first minimum of |G - g| + |B - b| over the palette rows (top_down.py:234-239)."""
    gb = pictures[..., 1:].astype(np.int64)[:, None]                                   # [n][1][H][W][2]
    d = np.abs(gb - np.asarray(palette, np.int64)[None, :, None, None, :]).sum(-1)      # [n][K + 1][H][W]
    return d.argmin(1)                                                                  # numpy's argmin: the first minimum


def heat(pictures, palette):
    """decode_images_to_heatmaps_minmax (top_down.py:219-258) -> float32 [n][K][H][W]."""
    pictures = np.asarray(pictures)
    k = len(palette) - 1
    cls = classify(pictures, palette)
    r = pictures[..., 0].astype(np.float32)
    maps = np.stack([(cls == c) * r for c in range(k)], 1).astype(np.float32)
    out = maps / 255.
    assert out.dtype == np.float32
    return out


def flip_back(maps, pair):
    """mmpose's flip_back for GaussianHeatmap targets: swap the channels of every pair, mirror the last axis."""
    return maps[:, np.asarray(pair)][..., ::-1].copy()


def heatmaps(pictures, flipped=None, palette=None, pair=None, shift=True):
    """`output_heatmap` of forward_pseudo_test (top_down.py:172-205) -> float32 [n][K][H][W]."""
    palette = pose_palette() if palette is None else np.asarray(palette)
    out = heat(pictures, palette)
    if flipped is None:
        return out
    f = flip_back(heat(flipped, palette), pair)
    if shift:
        f[:, :, :, 1:] = f.copy()[:, :, :, :-1]
    out = out + f
    out = out / 2
    assert out.dtype == np.float32
    return out


def peaks(maps):
    """float32 [n][K][H][W] -> preds float32 [n][K][2] (x, y), maxvals float32 [n][K]."""
    maps = np.asarray(maps)
    assert maps.dtype == np.float32
    n, k, h, w = maps.shape
    flat = maps.reshape(n, k, -1)
    idx = flat.argmax(2)                                   # the first index of the maximum
    maxvals = flat.max(2).astype(np.float32)
    preds = np.stack([idx % w, idx // w], -1).astype(np.float32)
    preds[maxvals <= 0] = -1
    for i in range(n):
        for c in range(k):
            m = maps[i, c]
            px, py = int(preds[i, c, 0]), int(preds[i, c, 1])
            if 1 < px < w - 1 and 1 < py < h - 1:
                diff = np.array([m[py][px + 1] - m[py][px - 1], m[py + 1][px] - m[py - 1][px]])
                preds[i, c] += np.sign(diff) * .25
    return preds, maxvals


def keypoints(pictures, flipped=None, palette=None, pair=None, shift=True):
    preds, maxvals = peaks(heatmaps(pictures, flipped, palette, pair, shift))
    return dict(preds=preds, maxvals=maxvals)


def peaks_integer(pictures, flipped, palette, pair, shift=True):
    """What an implementation on integer sums R_P + R_Q would report as the first maximum: -> int64 [n][K] flat indices.  Only to show
    that a case separates it from the float32 rule."""
    k = len(palette) - 1

    def ints(p):
        cls = classify(np.asarray(p), palette)
        return np.stack([(cls == c) * np.asarray(p)[..., 0].astype(np.int64) for c in range(k)], 1)
    f = flip_back(ints(flipped), pair)
    if shift:
        f[:, :, :, 1:] = f.copy()[:, :, :, :-1]
    s = ints(pictures) + f
    return s.reshape(s.shape[0], k, -1).argmax(2)


def to_image(preds, center, scale, heatmap_size):
    """mmpose's transform_preds(coords, center, scale, output_size, use_udp=False), stated independently of the product's."""
    preds = np.asarray(preds)
    scale = np.asarray(scale, np.float64) * 200.0
    sx, sy = scale[0] / heatmap_size[0], scale[1] / heatmap_size[1]
    out = np.ones_like(preds)
    out[:, 0] = preds[:, 0] * sx + center[0] - scale[0] * 0.5
    out[:, 1] = preds[:, 1] * sy + center[1] - scale[1] * 0.5
    return out
