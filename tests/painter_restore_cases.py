"""Shared inputs of the restoration-scoring tests: seeded (prediction, ground truth) picture pairs and the case list of the fixture
(tests/golden/painter_restore.npz).  TEST INFRASTRUCTURE.

A ground truth is a smooth colour field with texture, as uint8; a prediction is the ground truth / 255 plus a smooth error and noise,
pushed past 0 and 1 in places so that the clip matters.  Kinds:
  natural        the above; the prediction leaves [0, 1] at both ends.
  perfect        prediction == gt / 255. exactly.
  near_constant  a ground truth of 127 / 128 and a prediction within 1e-6 of it: x x and ux ux agree to ~12 digits, the
                 cancellation-heavy case of uxx - ux ux.
  ties           (Y cases) a ground truth made of colours whose Y ties exactly at one half, next to their neighbours.
The uint8 prediction of the Y metric is the `saved` picture of the float64 one: uint8(clip * 255)."""
import numpy as np

# (R, G, B) with (65481 R + 128553 G + 24966 B) mod 255000 == 127500: eight of the 194 colours whose Y ties at one half
TIE_COLOURS = ((0, 204, 68), (30, 186, 82), (58, 18, 128), (94, 140, 151), (132, 102, 247), (172, 116, 70), (205, 217, 209), (233, 49, 255))


def ground_truth(seed, h, w):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([0.5 + 0.45 * np.sin(yy / 9.0 + seed + c) * np.cos(xx / 7.0 - c) for c in range(3)], -1)
    base += rng.normal(0, 0.06, (h, w, 3))
    base[: max(h // 6, 1), : max(w // 5, 1)] = 0.0                       # a black and a white corner: the prediction's noise is clipped there
    base[-max(h // 6, 1):, -max(w // 5, 1):] = 1.0
    return np.clip(np.rint(base * 255), 0, 255).astype(np.uint8)


def case(kind, seed, h, w):
    """-> (prediction float64 [h][w][3], ground truth uint8 [h][w][3])."""
    rng = np.random.default_rng(seed + 1000)
    if kind == "near_constant":
        gt = (127 + (rng.random((h, w, 3)) < 0.5)).astype(np.uint8)
        return gt / 255. + rng.normal(0, 1e-6, (h, w, 3)), gt
    gt = ground_truth(seed, h, w)
    if kind == "ties":
        ties = np.array(TIE_COLOURS, np.uint8)
        pick = rng.integers(0, len(ties), (h, w))
        gt = np.where((rng.random((h, w)) < 0.5)[..., None], ties[pick], gt).astype(np.uint8)
    if kind == "perfect":
        return gt / 255., gt
    assert kind in ("natural", "ties"), kind
    yy, xx = np.mgrid[0:h, 0:w]
    pred = gt / 255. + 0.05 * np.sin(yy / 5.0)[..., None] * np.cos(xx / 11.0)[..., None] + rng.normal(0, 0.04, (h, w, 3))
    return pred, gt


def saved(pred):
    return (np.clip(pred, 0, 1) * 255).astype(np.uint8)


# name -> (kind, seed, height, width, metrics): what tests/golden/painter_restore.npz holds numbers for
FIXTURE = {
    "natural_61x83": ("natural", 1, 61, 83, ("skimage", "matlab_y")),
    "natural_97x131": ("natural", 2, 97, 131, ("skimage", "matlab_y")),
    "perfect_40x52": ("perfect", 3, 40, 52, ("skimage", "matlab_y")),
    "near_constant_61x83": ("near_constant", 4, 61, 83, ("skimage", "matlab_y")),
    "ties_33x47": ("ties", 5, 33, 47, ("matlab_y",)),
    "one_window_7x7": ("natural", 6, 7, 7, ("skimage",)),
}


def fixture_case(name):
    kind, seed, h, w, _ = FIXTURE[name]
    return case(kind, seed, h, w)


def inputs(pred, gt, metric):
    """The pair as the metric takes it: the float64 prediction, or its saved uint8 picture.  The saved picture of a perfect prediction
    is the ground truth itself: uint8(g / 255. * 255) truncates to g - 1 for some g, which is the script's rounding and not an error of the
    restoration."""
    if metric == "skimage":
        return pred, gt
    return (gt.copy() if np.array_equal(pred, gt / 255.) else saved(pred)), gt
