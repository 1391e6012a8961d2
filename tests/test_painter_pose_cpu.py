"""The pose keypoint definition (tests/painter_pose_host.py) against what the unmodified reference produced (tests/golden/
painter_pose.npz: TopDownCustom.forward_pseudo_test's `output_heatmap`), and its peak rule -- taken from mmpose's published source, not
verifiable here -- against hand-written expectations.  No GPU."""
import os

import numpy as np
import pytest

from tests import painter_pose_cases as C
from tests import painter_pose_host as H


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "painter_pose.npz"))


def _pair(golden, name):
    return golden[name + ".pictures"], golden[name + ".flipped"]


@pytest.mark.parametrize("name", C.FIXTURE + ["hand"])
@pytest.mark.parametrize("mode", ["flip", "plain"])
def test_host_heatmaps_equal_the_reference(golden, name, mode):
    p, q = _pair(golden, name)
    got = H.heatmaps(p, q if mode == "flip" else None, golden["palette"], C.PAIR, shift=True)
    ref = golden["%s.%s.heatmaps" % (name, mode)]
    assert got.dtype == ref.dtype == np.float32 and got.shape == ref.shape and got.tobytes() == ref.tobytes()
    preds, maxvals = H.peaks(got)
    assert np.array_equal(preds, golden["%s.%s.preds" % (name, mode)]) and np.array_equal(maxvals, golden["%s.%s.maxvals" % (name, mode)])


@pytest.mark.parametrize("mode", ["flip", "plain"])
def test_host_heatmaps_equal_the_reference_at_full_size(golden, mode):
    """256 x 192: the fixture holds per channel the reference's maximum, first argmax and the four neighbours of the peak."""
    p, q = _pair(golden, "full")
    assert p.shape == (1, 256, 192, 3) and len(np.unique(p[..., 0])) == 256          # every R value: the whole table T
    got = H.heatmaps(p, q if mode == "flip" else None, golden["palette"], C.PAIR, shift=True)
    flat = got.reshape(1, C.K, -1)
    idx = golden["full.%s.argmax" % mode]
    assert np.array_equal(flat.argmax(2), idx) and np.array_equal(flat.max(2), golden["full.%s.max" % mode])
    pad = np.pad(got, ((0, 0), (0, 0), (1, 1), (1, 1)))
    for k in range(C.K):
        y, x = idx[0, k] // 192 + 1, idx[0, k] % 192 + 1
        assert np.array_equal(np.array([pad[0, k, y, x - 1], pad[0, k, y, x + 1], pad[0, k, y - 1, x], pad[0, k, y + 1, x]]),
                              golden["full.%s.neighbours" % mode][0, k])
    preds, maxvals = H.peaks(got)
    assert np.array_equal(preds, golden["full.%s.preds" % mode]) and np.array_equal(maxvals, golden["full.%s.maxvals" % mode])
    assert (maxvals > 0).all() and (preds != np.floor(preds)).any()


def test_fixture_pictures_are_the_cases(golden):
    for name in C.FIXTURE:
        p, q = C.shape_pair(name)
        assert np.array_equal(p, golden[name + ".pictures"]) and np.array_equal(q, golden[name + ".flipped"])
    p, q, _ = C.hand_boxes()
    assert np.array_equal(p, golden["hand.pictures"]) and np.array_equal(q, golden["hand.flipped"])


def test_palette_and_pairs(golden):
    from painter_amd import painter_engine as E
    pal = golden["palette"]
    assert pal.shape == (18, 2) and np.array_equal(pal, H.pose_palette()) and np.array_equal(pal, E.pose_palette())
    assert E.pose_palette().dtype == np.int32 and not E.pose_palette().flags.writeable and E.pose_palette() is E.pose_palette()
    assert tuple(pal[0]) == (255, 255) and tuple(pal[16]) == (102, 204) and tuple(pal[17]) == (0, 0)
    assert [list(p) for p in E.COCO_FLIP_PAIRS] == C.FLIP_PAIRS
    assert np.array_equal(C.PAIR[C.PAIR], np.arange(17)) and C.PAIR[0] == 0 and C.PAIR[5] == 6
    assert np.array_equal(E.pose_palette(4), H.pose_palette(4)) and E.pose_palette(4).shape == (5, 2)


def test_table_of_unit_values():
    """float32(i) / 255 is what the double quotient rounds to, for every byte: the kernels compute the table that way."""
    i = np.arange(256)
    assert np.array_equal(i.astype(np.float32) / 255., (i.astype(np.float64) / 255.).astype(np.float32))


def test_float32_sums_split_integer_ties():
    t = np.arange(256, dtype=np.float32) / 255.
    sums = {}
    for a in range(256):
        for b in range(256):
            sums.setdefault(a + b, set()).add(float(t[a] + t[b]))
    assert len(sums) == 511 and sum(len(v) > 1 for v in sums.values()) == 127
    assert t[0] + t[3] < t[1] + t[2]


def test_hand_built_boxes():
    p, q, expect = C.hand_boxes()
    preds, maxvals = C.hand_expected()
    got = H.keypoints(p, q, C.PALETTE, C.PAIR, shift=True)
    assert np.array_equal(got["preds"], preds) and np.array_equal(got["maxvals"], maxvals)
    assert len(expect) == 16 and (maxvals[0] > 0).sum() == 1
    # what the boxes are there for
    g, b, first, second = [t for t in C.ties() if t[3] < C.K][0]
    assert first < second and maxvals[2, first] > 0 and maxvals[2, second] == 0                  # the first of two equidistant colours
    assert maxvals[3, 5] == 0 and maxvals[3, 6] > 0                                               # only the flipped picture shows it
    assert tuple(preds[5, 9]) == (5.0, 4.25)                                                      # sign(0) = 0
    assert tuple(preds[6, 3]) == tuple(preds[6, 6]) == (4.0, 4.0) and maxvals[6, 3] != maxvals[6, 6]
    assert tuple(preds[7, 0]) == (0.0, 4.0)
    assert any(t[3] == C.K for t in C.ties())                                                     # ties with the background exist too


def test_the_sum_case_bites():
    """Integer sums tie (0 + 3 == 1 + 2) and report the first pixel; the reference's float32 sums report the later one."""
    p, q, _ = C.hand_boxes()
    integer = H.peaks_integer(p[:1], q[:1], C.PALETTE, C.PAIR)[0, 0]
    floats = H.heatmaps(p[:1], q[:1], C.PALETTE, C.PAIR)[0, 0].argmax()
    assert (integer % C.HAND_W, integer // C.HAND_W) == (3, 4) and (floats % C.HAND_W, floats // C.HAND_W) == (7, 4)


def test_small_widths_have_the_interior_the_rule_says():
    """1 < px < w - 1: none at w = 3, px = 2 at w = 4."""
    for w, moves in ((3, False), (4, True)):
        maps = np.zeros((1, 1, w, w), np.float32)
        c = w // 2
        maps[0, 0, c, c], maps[0, 0, c, c - 1] = 1.0, 0.5
        preds, _ = H.peaks(maps)
        assert tuple(preds[0, 0]) == ((c - 0.25, c) if moves else (c, c))


def test_no_flip_and_no_shift():
    p, q = C.shape_pair("8x6")
    plain = H.heatmaps(p, None, C.PALETTE, C.PAIR)
    assert np.array_equal(plain, H.heat(p, C.PALETTE))
    unshifted = H.heatmaps(p, q, C.PALETTE, C.PAIR, shift=False)
    f = H.heat(q, C.PALETTE)[:, C.PAIR][..., ::-1]
    assert np.array_equal(unshifted, (plain + f) / 2) and not np.array_equal(unshifted, H.heatmaps(p, q, C.PALETTE, C.PAIR))


def test_to_image_matches_its_formula():
    from painter_amd import painter_engine as E
    rng = np.random.default_rng(3)
    for center, scale in (((320.5, 240.25), (1.2, 1.6)), ((37.0, 411.0), (0.45, 0.6))):
        preds = rng.uniform(-1, 192, (17, 2)).astype(np.float32)
        got = E.to_image(preds, center, scale, (192, 256))
        assert got.shape == (17, 2) and np.array_equal(got, H.to_image(preds, center, scale, (192, 256)))
        w, h = scale[0] * 200.0, scale[1] * 200.0
        for k in (0, 16):
            assert got[k, 0] == np.float32(float(preds[k, 0]) * (w / 192) + center[0] - w * 0.5)
            assert got[k, 1] == np.float32(float(preds[k, 1]) * (h / 256) + center[1] - h * 0.5)
    corner = E.to_image(np.array([[0.0, 0.0], [192.0, 256.0]], np.float32), (100.0, 100.0), (0.96, 1.28), (192, 256))
    assert np.allclose(corner, [[4.0, -28.0], [196.0, 228.0]])
