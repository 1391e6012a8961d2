"""The masks of the RLE tests (tests/test_painter_rle_cpu.py, tests/test_painter_rle_gpu.py) and the literal vectors of the format:
mask[y, x], shape (h, w).  Not a test."""
import functools

import numpy as np


def _set(shape, *points):
    m = np.zeros(shape, bool)
    for p in points:
        m[p] = True
    return m


def _table():
    t5x7 = np.zeros((5, 7), bool)
    t5x7[1:4, 2:5] = True
    t40 = np.zeros((40, 50), bool)
    t40[0:3, 0] = True
    t40[5:40, 1:3] = True
    t40[10, 30] = True
    return [
        ("zeros-2x2", np.zeros((2, 2), bool), [4], "4"),
        ("ones-2x2", np.ones((2, 2), bool), [0, 4], "04"),
        ("three-points-3x4", _set((3, 4), (1, 1), (2, 1), (0, 2)), [4, 3, 5], "435"),
        ("block-5x7", t5x7, [11, 3, 2, 3, 2, 3, 11], ";320009"),
        ("negative-delta-40x50", t40, [0, 3, 42, 35, 5, 35, 1090, 1, 789], "03Z1P1kN0mQ1nNcF"),
        ("column-wrap-480x640", _set((480, 640), (479, 0), (0, 1)), [479, 2, 306719], "o>2o`[9"),
        ("five-characters-2000x2000", _set((2000, 2000), (5, 5), (1999, 1999)), [10005, 1, 3989993, 1], "eh91Y_hi30"),
    ]


@functools.lru_cache(maxsize=None)
def table():
    """(name, mask, counts, string): the vectors of the format, as literals."""
    return _table()


def checkerboard(h, w):
    y, x = np.mgrid[:h, :w]
    return ((y + x) & 1).astype(bool)


@functools.lru_cache(maxsize=None)
def cases():
    """(name, mask): every shape the device tests run, the table included.  Read only."""
    rng = np.random.RandomState(20)
    out = [(name, mask) for name, mask, _, _ in table()]
    out += [
        ("1x1-zero", np.zeros((1, 1), bool)),
        ("1x1-one", np.ones((1, 1), bool)),
        ("row-1x70", rng.rand(1, 70) < 0.4),
        ("column-70x1", rng.rand(70, 1) < 0.4),
        ("random-33x64", rng.rand(33, 64) < 0.3),
        ("random-37x53", rng.rand(37, 53) < 0.3),
        ("zeros-37x53", np.zeros((37, 53), bool)),
        ("ones-37x53", np.ones((37, 53), bool)),
        ("first-pixel-37x53", _set((37, 53), (0, 0))),
        ("last-pixel-37x53", _set((37, 53), (36, 52))),
        ("wide-3x2500", rng.rand(3, 2500) < 0.3),
        ("tall-2500x3", rng.rand(2500, 3) < 0.3),
        ("checkerboard-48x64", checkerboard(48, 64)),
    ]
    for _, m in out:
        m.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def batch(h=61, w=83, n=37, seed=5):
    """Masks of very different run counts in one batch: empty, full, blobs, noise, a checkerboard -> bool [n][h][w]."""
    rng = np.random.RandomState(seed)
    masks = np.zeros((n, h, w), bool)
    for i in range(n):
        kind = i % 6
        if kind == 1:
            masks[i] = True
        elif kind == 2:
            y0, x0 = rng.randint(0, h - 8), rng.randint(0, w - 8)
            masks[i, y0:y0 + rng.randint(1, 30), x0:x0 + rng.randint(1, 40)] = True
        elif kind == 3:
            masks[i] = rng.rand(h, w) < 0.5
        elif kind == 4:
            masks[i] = checkerboard(h, w)
        elif kind == 5:
            masks[i] = rng.rand(h, w) < 0.02
    masks.setflags(write=False)
    return masks


def malformed(h, w):
    """(name, counts, flag) for the mask size (h, w): strings and count lists the decode refuses, one per flag value it can give from
    the bytes alone (5 and 6 depend on the workspace and the spans: the device test builds those)."""
    from tests import painter_rle_host as H
    n = h * w
    good = H.to_string([n - 3, 3])
    return [
        ("empty-string", b"", 1),
        ("one-run-too-many", H.to_string([n - 3, 3, 1]), 1),
        ("short", H.to_string([n - 4, 3]), 1),
        ("negative-after-delta", H.to_string([1, 2, 3]) + bytes([48 + 0x1b]), 2),        # the fourth value is -5: 2 - 5 < 0
        ("ends-inside-a-value", good + bytes([48 + 0x21]), 3),
        ("eight-groups", bytes([48 + 0x21] * 7 + [48 + 0x01]) + good, 4),
        ("byte-below-0", good[:-1] + b" " + good[-1:], 7),
        ("byte-above-o", good + b"p", 7),
        ("uncompressed-overshoot", [n - 3, 3, 1], 1),
        ("uncompressed-empty", [], 1),
    ]
