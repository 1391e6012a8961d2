"""Shared inputs of the pose keypoint tests: seeded synthetic painted `coco_pose` pictures with their flipped twins, and hand-built
boxes that each isolate one rule.  TEST INFRASTRUCTURE.

A painted pose picture shows every keypoint as a Gaussian blob in R with the keypoint's palette colour in G / B on a black background.
The flipped twin is what the network paints for the mirrored box: the blobs at mirrored columns, left / right classes swapped, its own
noise.  Noise is bounded (+-`noise` per channel) and a few percent of the pixels get a uniformly random colour, so that classification
sees colours anywhere between the palette's, ties included."""
import numpy as np

from tests import painter_pose_host as H

FLIP_PAIRS = [[1, 2], [3, 4], [5, 6], [7, 8], [9, 10], [11, 12], [13, 14], [15, 16]]       # configs/_base_/coco.py: the `swap` fields
K = 17
PALETTE = H.pose_palette(K)
PAIR = H.pair_table(FLIP_PAIRS, K)


def painted_pair(seed, n, h, w, palette=PALETTE, pair=PAIR, noise=12, speckle=0.03, absent=0.15):
    """-> (pictures, flipped) uint8 [n][h][w][3]."""
    rng = np.random.default_rng(seed)
    k = len(palette) - 1
    yy, xx = np.mgrid[0:h, 0:w]

    def paint(centres, classes, sigma):
        r = np.zeros((h, w))
        cls = np.full((h, w), k)
        for (cy, cx), c, s in zip(centres, classes, sigma):
            g = 255.0 * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
            take = (g > r) & (g >= 6)
            r[take], cls[take] = g[take], c
        img = np.concatenate([r[..., None], np.asarray(palette, np.float64)[cls]], -1)
        img = img + rng.integers(-noise, noise + 1, img.shape)
        wild = rng.random((h, w)) < speckle
        img[wild] = rng.integers(0, 256, (int(wild.sum()), 3))
        return np.clip(np.rint(img), 0, 255).astype(np.uint8)

    pics, flips = [], []
    for _ in range(n):
        present = np.flatnonzero(rng.random(k) >= absent)
        centres = np.stack([rng.uniform(0, h - 1, len(present)), rng.uniform(0, w - 1, len(present))], -1)
        sigma = rng.uniform(0.6, max(0.8, min(h, w) / 16), len(present))
        pics.append(paint(centres, present, sigma))
        seen = rng.random(len(present)) >= absent / 2                        # the twin misses some keypoints and moves the others a little
        twin = np.stack([centres[:, 0] + rng.uniform(-0.7, 0.7, len(present)), w - 1 - centres[:, 1] + rng.uniform(-0.7, 0.7, len(present))], -1)
        flips.append(paint(twin[seen], np.asarray(pair)[present[seen]], sigma[seen]))
    return np.stack(pics), np.stack(flips)


# name -> (seed, n, h, w): the shapes the device tests sweep.  1 < px < w - 1 has no solution at w = 3, exactly one at w = 4 (px = 2) and two
# at w = 5; 8 x 6 and 33 x 17 are no multiple of a wave or a workgroup's chunk; 70 x 61 = 4270 pixels spans three chunks of 2048.
SHAPES = {
    "3x3": (11, 3, 3, 3),
    "4x4": (12, 3, 4, 4),
    "5x5": (13, 3, 5, 5),
    "8x6": (14, 3, 8, 6),
    "33x17": (15, 3, 33, 17),
    "70x61": (16, 1, 70, 61),
    "many": (17, 33, 8, 6),
}
FIXTURE = ["3x3", "4x4", "5x5", "8x6", "33x17"]             # stored with the reference's full heat maps (and the hand-built boxes)
FULL = (21, 1, 256, 192)                                    # stored with the reference's per-channel summary


def shape_pair(name):
    seed, n, h, w = SHAPES[name]
    small = dict(noise=8) if min(h, w) <= 5 else {}
    return painted_pair(seed, n, h, w, **small)


def full_pair():
    return painted_pair(*FULL)


def custom_palette(k, seed=5):
    """k distinct random (G, B) colours plus the background row (0, 0), and a pairing of the channels (the last one of an odd k pairs
    with itself)."""
    rng = np.random.default_rng(seed)
    colours = set()
    while len(colours) < k:
        colours.add((int(rng.integers(40, 256)), int(rng.integers(40, 256))))
    pal = np.array(sorted(colours, key=lambda c: rng.random()) + [(0, 0)], np.int32)
    pairs = [[i, i + 1] for i in range(0, k - 1, 2)]
    return pal, pairs


def ties(palette=PALETTE):
    """Every (g, b) whose nearest palette row is not unique -> list of (g, b, first, second), in (g, b) order."""
    g, b = np.mgrid[0:256, 0:256]
    d = np.abs(g[..., None] - palette[:, 0]) + np.abs(b[..., None] - palette[:, 1])
    order = np.argsort(d, -1, kind="stable")
    first, second = order[..., 0], order[..., 1]
    tie = np.take_along_axis(d, first[..., None], -1)[..., 0] == np.take_along_axis(d, second[..., None], -1)[..., 0]
    return [(int(y), int(x), int(first[y, x]), int(second[y, x])) for y, x in zip(*np.nonzero(tie))]


# ---- hand-built boxes, 9 x 11, default palette, COCO pairs, flip test with shift.  Q's column xq lands on column w - xq (xq >= 1); column
# w - 1 of Q lands on columns 0 AND 1; column 0 of Q lands nowhere.
HAND_H, HAND_W = 9, 11
HAND_NAMES = ["float_sum", "equal_values", "gb_tie", "only_flipped", "edges", "equal_neighbours", "classes_differ", "column0"]


def _qx(x):
    return HAND_W - 1 if x == 0 else HAND_W - x


def hand_boxes():
    """-> (pictures, flipped, expect): expect = {(box, channel): (x, y, maxval as a float32 expression of T)} for the flip test with
    shift; every channel of a box that is not listed is absent: (-1, -1, 0)."""
    n = len(HAND_NAMES)
    P = np.zeros((n, HAND_H, HAND_W, 3), np.uint8)
    Q = np.zeros_like(P)
    T = np.arange(256, dtype=np.float32) / 255.
    two = np.float32(2)

    def put(pic, box, y, x, k, r, gb=None):
        pic[box, y, x] = (r,) + (tuple(PALETTE[k]) if gb is None else gb)
    expect = {}
    # 0: T[0] + T[3] < T[1] + T[2] in float32 although 0 + 3 == 1 + 2: the float-larger pixel comes LATER in row-major order
    put(P, 0, 4, 3, 0, 0), put(Q, 0, 4, _qx(3), 0, 3)
    put(P, 0, 4, 7, 0, 1), put(Q, 0, 4, _qx(7), 0, 2)
    expect[(0, 0)] = (7, 4, (T[1] + T[2]) / two)
    # 1: two pixels with one value: the first in row-major order wins; its right neighbour pulls x by + 0.25
    put(P, 1, 2, 8, 2, 200), put(P, 1, 6, 2, 2, 200), put(P, 1, 2, 9, 2, 100)
    expect[(1, 2)] = (8.25, 2, T[200] / two)
    # 2: a (G, B) at equal distance from two keypoint colours belongs to the first; the second stays absent
    g, b, first, second = [t for t in ties() if t[3] < K][0]
    put(P, 2, 5, 5, first, 180, gb=(g, b))
    expect[(2, first)] = (5, 5, T[180] / two)
    # 3: a channel that only the flipped picture shows: left_shoulder (5) there is right_shoulder (6) here, at column w - 4
    put(Q, 3, 3, 4, 5, 220)
    expect[(3, 6)] = (HAND_W - 4, 3, T[220] / two)
    # 4: peaks at columns 0, 1, w - 2, w - 1 and rows 0, 1, h - 2, h - 1, each with a weaker neighbour towards the inside: only column
    # w - 2 and row h - 2 satisfy 1 < p < size - 1 (with the other coordinate inside) and move
    for k, (y, x, ny, nx) in enumerate([(2, 0, 2, 1), (3, 1, 3, 2), (4, HAND_W - 2, 4, HAND_W - 3), (5, HAND_W - 1, 5, HAND_W - 2),
                                        (0, 4, 1, 4), (1, 5, 2, 5), (HAND_H - 2, 6, HAND_H - 3, 6), (HAND_H - 1, 7, HAND_H - 2, 7)]):
        put(P, 4, y, x, k, 250), put(P, 4, ny, nx, k, 100)
        expect[(4, k)] = (x, y, T[250] / two)
    expect[(4, 2)] = (HAND_W - 2 - 0.25, 4, T[250] / two)
    expect[(4, 6)] = (6, HAND_H - 2 - 0.25, T[250] / two)
    # 5: equal left and right neighbours: sign 0 in x; the lower neighbour is larger: + 0.25 in y
    put(P, 5, 4, 5, 9, 240), put(P, 5, 4, 4, 9, 90), put(P, 5, 4, 6, 9, 90), put(P, 5, 3, 5, 9, 50), put(P, 5, 5, 5, 9, 120)
    expect[(5, 9)] = (5, 4.25, T[240] / two)
    # 6: one pixel, two classes: left_ear (3) in the picture, left_shoulder (5) -> right_shoulder (6) from the flipped one
    put(P, 6, 4, 4, 3, 200), put(Q, 6, 4, _qx(4), 5, 150)
    expect[(6, 3)] = (4, 4, T[200] / two)
    expect[(6, 6)] = (4, 4, T[150] / two)
    # 7: the flipped picture's last column lands on columns 0 and 1 with one value: column 0 is first
    put(Q, 7, 4, HAND_W - 1, 0, 210), put(Q, 7, 4, HAND_W - 2, 0, 100)
    expect[(7, 0)] = (0, 4, T[210] / two)
    return P, Q, expect


def hand_expected():
    """-> preds float32 [n][17][2], maxvals float32 [n][17] from `expect`."""
    _, _, expect = hand_boxes()
    preds = np.full((len(HAND_NAMES), K, 2), -1, np.float32)
    maxvals = np.zeros((len(HAND_NAMES), K), np.float32)
    for (box, k), (x, y, m) in expect.items():
        preds[box, k], maxvals[box, k] = (x, y), m
    return preds, maxvals
