"""The target encoders without a GPU: the host statement (tests/painter_paint_host.py) against the pictures the unmodified reference
generators produced (tests/golden/painter_paint.npz), the formulas the kernels rely on, the wrappers' argument checks, the new header, and
the round-trip conditions of tests/test_painter_paint_gpu.py on the host statement and the existing host decoders alone."""
import functools
import os

import numpy as np
import pytest

from painter_amd import _lib
from painter_amd import painter_engine as E
from tests import painter_inst_host as IH
from tests import painter_paint_cases as C
from tests import painter_paint_host as H
from tests import painter_pose_host as PH
from tests.guard_bands import abi_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAINT_HEADER = os.path.join(ROOT, "include", "painter_paint.h")
SYMBOLS = {"pa_paint_semantic", "pa_paint_instances_workspace_bytes", "pa_paint_instances", "pa_paint_pose"}


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "painter_paint.npz")))


def test_the_cases_are_the_ones_the_fixture_was_made_from():
    assert str(golden()["inputs.digest"]) == C.input_digest()


def test_semantic_statement_equals_the_reference():
    g = golden()
    assert np.array_equal(g["semantic.palette"], H.ade_palette()) and np.array_equal(E.semantic_palette(150, 6), H.ade_palette())
    for name, labels in C.semantic_cases():
        pic, bad = H.semantic(labels, g["semantic.palette"])
        assert bad == 0 and pic.tobytes() == g["semantic." + name].tobytes() and pic.shape == g["semantic." + name].shape, name
    good, bad = C.semantic_bad_case()
    assert H.semantic(good, H.ade_palette())[1] == 0 and H.semantic(bad, H.ade_palette())[1] == 2


def test_panoptic_statement_equals_the_reference():
    g = golden()
    assert np.array_equal(g["panoptic.palette"], E.semantic_palette())
    painted = 0
    for name, ids, segments in C.panoptic_cases():
        pic = H.panoptic_semantic(ids, segments, C.CATEGORY_INDEX, g["panoptic.palette"])
        ref = g["panoptic." + name]
        if ref.size == 0:
            assert not segments and not pic.any()                   # the script skips an annotation without segments
        else:
            assert pic.shape == ref.shape and pic.tobytes() == ref.tobytes(), name
            painted += 1
    assert painted == 4
    # the duplicate id takes the later row's colour, the unlisted id stays black
    name, ids, segments = C.panoptic_cases()[0]
    pic = H.panoptic_semantic(ids, segments, C.CATEGORY_INDEX, g["panoptic.palette"])
    assert (pic[ids == 3592] == g["panoptic.palette"][99]).all() and (ids == 3592).any()
    assert not pic[ids == 77].any() and (ids == 77).any() and pic[ids == 16777215].any()


def test_instance_statement_equals_the_reference():
    g = golden()
    seen = 0
    for method in ("mass_center", "geo_center"):
        for name, masks, disjoint in C.instance_cases():
            key = "instances.%s.%s" % (method, name)
            assert (key in g) == (disjoint and (method == "mass_center" or name.endswith("37x53"))), key
            if key not in g:
                continue
            pic, cells, empty = H.instances(masks, method, C.geo_boxes(masks))
            if g[key].size == 0:
                assert empty and not pic.any(), key
            else:
                assert not empty and pic.shape == g[key].shape and pic.tobytes() == g[key].tobytes(), key
            seen += 1
    assert seen == 20


def test_pose_statement_equals_the_reference():
    g = golden()
    assert np.array_equal(g["pose.colours"], H.pose_colours()) and np.array_equal(E.pose_palette()[:-1], H.pose_colours())
    for name, joints, visible, size in C.pose_cases():
        pics = np.stack([H.pose(j, v, size)[0] for j, v in zip(joints, visible)])
        dense = np.stack([H.pose_fast(j, v, size)[0] for j, v in zip(joints, visible)])
        assert pics.tobytes() == dense.tobytes(), name
        if size == (192, 256):
            assert pics.shape == g["pose." + name].shape and pics.tobytes() == g["pose." + name].tobytes(), name
        else:
            assert "pose." + name not in g                           # the reference's buffer is 17 x 256 x 192
    j, v = C.pose_boxes(192, 256)
    assert not H.pose(j[2], v[2])[0].any()                           # all joints invisible: black
    w = H.pose(j[1], v[1])[1]
    assert (w[0] != w[1]).any() and (w[1] == 0).any() and (w[0] == 1).any()      # reach in for one sigma only; fully out; reach in


def test_the_truncation_quirk():
    """sigma = 1.5, mu < 5: int(mu - 4.5) truncates toward zero, the patch is 9 wide and its centre, ul + 5, is not mu."""
    for mu, ul, br in ((0, -4, 5), (4, 0, 9), (5, 0, 10), (6, 1, 11), (-6.5, -10, 0)):      # (int(-6.5 + 0.5) = -6: that truncates too)
        rects, weights = E.msra_rectangles(np.array([[[mu, 100.0]]], np.float32), np.ones((1, 1)), (192, 256), 1.5)
        assert rects[0, 0, 0] == ul and rects[0, 0, 2] == br and weights[0, 0] == 1, (mu, rects)
    for sigma in (1.5, 3):
        j, v = C.pose_boxes(192, 256)
        rects, weights = E.msra_rectangles(j, v, (192, 256), sigma)
        for b in range(len(j)):
            _, w, r = H.msra_target(j[b], v[b], (192, 256), sigma)
            assert np.array_equal(rects[b], r) and np.array_equal(weights[b], w[:, 0])


def test_cell_formula_against_the_location_palette():
    pal = E.location_palette()
    assert pal.shape == (6400, 3)
    rows = set()
    for ay in range(80):
        for ax in range(80):
            assert np.array_equal(pal[H.cell_row(ax, ay)], H.location_colour(ax, ay)), (ax, ay)
            rows.add(H.cell_row(ax, ay))
    assert rows == set(range(6400))


@pytest.mark.parametrize("sigma", [1.5, 3])
def test_distance_table(sigma):
    table, f, c = H.d2_table(sigma)
    assert f.dtype == np.float32 and (np.diff(f) < 0).all() and c == {1.5: 5, 3: 9}[sigma]
    g, c2 = H.msra_patch(sigma)
    assert c2 == c and g.dtype == np.float32 and g.shape == {1.5: (10, 10), 3: (19, 19)}[sigma]
    y, x = np.mgrid[0:g.shape[0], 0:g.shape[1]]
    d2 = (x - c) ** 2 + (y - c) ** 2
    assert np.array_equal(f[d2], g) and np.array_equal(table[d2], (g * 255.).astype(np.uint8)) and d2.max() == len(table) - 1
    mine, mine_f, mine_c = E.msra_table(sigma)
    assert np.array_equal(mine, table) and np.array_equal(mine_f, f) and mine_c == c and table[0] == 255


class _NoDevice:
    def __getattr__(self, name):
        raise AssertionError("the library was reached: %s" % name)


def test_wrapper_checks_raise_before_any_device_call(monkeypatch):
    monkeypatch.setattr(E, "lib", _NoDevice())
    monkeypatch.setattr(E, "_device", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the device was asked for")))
    labels = np.zeros((5, 7), np.uint8)
    for bad in (labels.astype(np.int64), labels.astype(np.float32), np.zeros((5, 7, 3), np.uint8), np.zeros(5, np.uint8), np.zeros((0, 7), np.uint8)):
        with pytest.raises(ValueError, match="picture 0"):
            E.paint_semantic(bad)
    with pytest.raises(ValueError, match="no pictures"):
        E.paint_semantic([])
    with pytest.raises(ValueError, match="palette"):
        E.paint_semantic(labels, palette=np.zeros((3, 4)))
    with pytest.raises(ValueError, match="palette"):
        E.paint_semantic(labels, palette=np.full((3, 3), 256))
    with pytest.raises(ValueError, match="at most 1024"):
        E.paint_semantic(labels, palette=np.zeros((1025, 3)))
    ids = np.zeros((5, 7), np.int32)
    with pytest.raises(ValueError, match="picture 0"):
        E.paint_panoptic_semantic(labels, [], {})
    with pytest.raises(ValueError, match="1 pictures, 2 segment lists"):
        E.paint_panoptic_semantic([ids], [[], []], {})
    with pytest.raises(KeyError):
        E.paint_panoptic_semantic(ids, [(1, 7)], {8: 0})
    with pytest.raises(ValueError, match="colour index 133"):
        E.paint_panoptic_semantic(ids, [dict(id=1, category_id=7)], {7: 133})
    with pytest.raises(ValueError, match="segment id"):
        E.paint_panoptic_semantic(ids, [(-1, 7)], {7: 0})
    with pytest.raises(ValueError, match="at most 1024"):
        E.paint_panoptic_semantic(ids, [(k, 7) for k in range(1025)], {7: 0})
    masks = np.zeros((2, 5, 7), bool)
    with pytest.raises(NotImplementedError):
        E.paint_instances(masks, method="box_center")
    with pytest.raises(ValueError, match="geo_center"):
        E.paint_instances(masks, method="geo_center")
    with pytest.raises(ValueError, match="geo_center"):
        E.paint_instances(masks, boxes=np.zeros((2, 4)))
    with pytest.raises(ValueError, match="palette"):
        E.paint_instances(masks, palette=np.zeros((100, 3)))
    with pytest.raises(ValueError, match="size="):
        E.paint_instances(np.zeros((2, 2), np.uint32))
    with pytest.raises(ValueError, match="at most 4096"):
        E.paint_instances(np.zeros((4097, 1, 1), bool))
    with pytest.raises(ValueError, match=r"boxes are \[n\]\[4\]"):
        E.paint_instances(masks, method="geo_center", boxes=np.zeros((3, 4)))
    with pytest.raises(ValueError, match="box 1 lies outside"):
        E.paint_instances(masks, method="geo_center", boxes=np.array([[0, 0, 2, 2], [6, 0, 9, 2]], np.float32))
    j, v = np.zeros((1, 17, 3), np.float32), np.ones((1, 17, 3), np.float32)
    with pytest.raises(ValueError, match="joints"):
        E.paint_pose(j[0], v[0])
    with pytest.raises(ValueError, match="joints"):
        E.paint_pose(np.zeros((1, 33, 2)), np.ones((1, 33)))
    with pytest.raises(ValueError, match="joints"):
        E.paint_pose(j, v[:, :16])
    with pytest.raises(ValueError, match="sigmas"):
        E.paint_pose(j, v, sigmas=(1.5,))
    with pytest.raises(ValueError, match="18 joints, the palette has 17"):
        E.paint_pose(np.zeros((1, 18, 2)), np.ones((1, 18)))
    with pytest.raises(ValueError, match="strictly decreasing"):
        E.paint_pose(j, v, sigmas=(1.5, 40))


def test_the_header_parses_and_is_loaded():
    protos = _lib.parse_header(PAINT_HEADER)
    assert set(protos) == SYMBOLS == abi_symbols(open(PAINT_HEADER).read())
    assert PAINT_HEADER in [os.path.abspath(p) for p in _lib.MORE_HEADERS]
    assert not SYMBOLS & set(_lib.parse_header())                   # the new entry points appear only in painter_paint.h
    assert len(protos["pa_paint_instances"][1]) == 11 and len(protos["pa_paint_pose"][1]) == 11 and len(protos["pa_paint_semantic"][1]) == 7
    import ctypes
    assert ctypes.sizeof(E.PaintJob) == 40
    text = open(PAINT_HEADER).read()
    for name, value in (("PA_PAINT_MAX_COLOURS", E.PAINT_MAX_COLOURS), ("PA_PAINT_MAX_SEGMENTS", E.PAINT_MAX_SEGMENTS), ("PA_PAINT_MAX_MASKS", E.PAINT_MAX_MASKS),
                        ("PA_PAINT_CELLS", E.PAINT_CELLS), ("PA_PAINT_MAX_JOINTS", E.PAINT_MAX_JOINTS), ("PA_PAINT_MAX_TABLE", E.PAINT_MAX_TABLE)):
        assert "#define %s %d\n" % (name, value) in text
    assert E.PAINT_MAX_MASKS >= 1024
    from painter_amd import build
    assert PAINT_HEADER in build.headers() and build.EXTRA["painter_paint.hip"] == ["-ffp-contract=off"]


# ---- the round trips of the GPU tests, on the host statement and the host decoders
def argmin_classes(picture, palette):
    d = np.abs(picture[:, :, None, :].astype(np.int64) - np.asarray(palette, np.int64)[None, None]).sum(-1)
    return d.argmin(-1)


def test_round_trip_semantic_on_the_host():
    labels = C.semantic_cases()[1][1]
    pic, _ = H.semantic(labels, H.ade_palette())
    got = argmin_classes(pic, H.ade_palette())
    assert np.array_equal(got[labels > 0], labels[labels > 0] - 1) and (labels > 0).sum() > 1000


def round_trip_rows(masks):
    """The palette rows of the masks' cells: pairwise distinct is what the round trip asks."""
    _, cells, _ = H.instances(masks)
    rows = [H.cell_row(int(ax), int(ay)) for ax, ay in cells]
    assert len(set(rows)) == len(rows)
    return rows


def test_round_trip_instances_on_the_host():
    masks = C.roundtrip_masks()
    pic, cells, empty = H.instances(masks)
    rows = round_trip_rows(masks)
    # dist_thr 4: a pixel belongs to a colour when L1 / 3 < 4, and neighbouring cells' colours are 13 apart (13 / 3 > 4)
    out = IH.decode(pic, E.location_palette(), [4.0])
    assert not empty and not out["empty"] and len(out["candidates"]) == len(masks)
    for cand, got in zip(out["candidates"], out["masks"]):
        assert np.array_equal(got, masks[rows.index(int(cand))])
    assert sorted(int(c) for c in out["candidates"]) == sorted(rows)


def pose_round_trip_set(pictures, joints, visible, size):
    """-> [(box, joint, mu_x, mu_y)]: live joints whose centre pixel carries their own colour at R = 255, strictly inside the border rule of
    the peak refinement (1 < x < W - 1, 1 < y < H - 1), whose four neighbours carry that colour too with equal R left / right and up /
    down -- read off the HOST statement's picture."""
    W, H_ = size
    colours = H.pose_colours()
    rects, weights = E.msra_rectangles(joints, visible, size, 3)
    out = []
    for b in range(len(joints)):
        p = pictures[b]
        for k in range(joints.shape[1]):
            mx, my = int(rects[b, k, 0]) + 9, int(rects[b, k, 1]) + 9
            if weights[b, k] != 1 or not (1 < mx < W - 1 and 1 < my < H_ - 1):
                continue
            own = lambda y, x: tuple(p[y, x, 1:]) == tuple(colours[k])
            if own(my, mx) and p[my, mx, 0] == 255 and own(my, mx - 1) and own(my, mx + 1) and own(my - 1, mx) and own(my + 1, mx) and \
                    p[my, mx - 1, 0] == p[my, mx + 1, 0] and p[my - 1, mx, 0] == p[my + 1, mx, 0]:
                out.append((b, k, mx, my))
    return out


@pytest.mark.parametrize("size", C.POSE_SIZES)
def test_round_trip_pose_on_the_host(size):
    joints, visible = C.pose_boxes(*size)
    pics = np.stack([H.pose(j, v, size)[0] for j, v in zip(joints, visible)])
    kp = PH.keypoints(pics)
    chosen = pose_round_trip_set(pics, joints, visible, size)
    # boxes 1 (on or beyond the border), 2 (black) and 4 (one cluster: every centre collides) cannot qualify by construction
    assert len(chosen) >= 8 and {b for b, _, _, _ in chosen} == {0, 3}
    for b, k, mx, my in chosen:
        assert kp["preds"][b, k].tolist() == [mx, my] and kp["maxvals"][b, k] == 1, (b, k)
    assert (kp["maxvals"][2] == 0).all()                             # the black picture: no channel shows
