"""The definition of the boundary-IoU branch (tests/painter_boundary_host.py) held to an independent second statement of the erosion, to
hand-written cases and to `painter_engine.semseg_scores`, and what can be said about the new entry points without a GPU.

No fixture of the reference exists for this branch: its evaluators need detectron2 and cv2, which are not available where this project is
tested.  The definition is restated from detectron2's published source and unverified against detectron2 / cv2."""
import inspect
import os

import numpy as np
import pytest

from tests import painter_boundary_host as B
from tests import painter_score_cases as C

OLD_KEYS = {"mIoU", "fwIoU", "mACC", "pACC", "IoU", "ACC"}


@pytest.mark.parametrize("h,w,ratio,d", B.SHAPES)
def test_the_two_statements_of_the_erosion_agree(h, w, ratio, d):
    from painter_amd import painter_engine as E
    assert B.dilation(h, w, ratio) == d and E.boundary_dilation(h, w, ratio) == d
    _, _, pal, pred, gtk = B.label_maps(h, w)
    for m in (pred, gtk):
        got = B.boundary(m, d)
        assert got.dtype == np.uint8 and got.shape == (h, w) and np.array_equal(got, B.boundary_iterated(m, d))
        assert (got <= m).all()
        if 2 * d + 1 > min(h, w):
            assert np.array_equal(got, m)                              # boundary everywhere
    assert gtk.max() == len(pal) or h * w < 100                       # the ignore band is there as label K


def test_dilation_rounds_half_to_even_and_is_at_least_one():
    from painter_amd import painter_engine as E
    assert E.boundary_dilation(30, 40, .05) == 2 and E.boundary_dilation(30, 40, .07) == 4          # 2.5 -> 2, 3.5 -> 4
    assert E.boundary_dilation(480, 640) == 16 and E.boundary_dilation(512, 683) == 17 and E.boundary_dilation(3, 4, .01) == 1
    assert inspect.signature(E.boundary_dilation).parameters["dilation_ratio"].default == 0.02
    assert inspect.signature(E.label_boundary).parameters["dilation_ratio"].default == 0.02


@pytest.mark.parametrize("name", list(C.SEMSEG))
def test_fixture_cases_are_not_trivially_empty(name):
    pic, gt, pal = C.semseg_fixture_case(name)
    k = len(pal)
    conf, bconf, invalid = B.boundary_confusion([pic], [gt], pal)
    assert invalid == 0 and bconf.sum() == conf.sum() == gt.size
    off = bconf.copy()
    off[np.arange(k + 1), np.arange(k + 1)] = 0
    assert 340 <= np.count_nonzero(off) <= 739
    assert bconf[k].sum() == 0 and bconf[:, k].sum() > 0             # a class map holds no K; the ignore band does
    assert bconf[0, 0] > 0


def test_a_wide_window_leaves_no_pixel_off_the_boundary():
    """61 x 83 at ratio 0.35: d = 36, 73 > 61, every window leaves the picture, so both maps are their own boundary and the boundary
    matrix IS the confusion matrix; no pixel is in bin (0, 0)."""
    pic, gt, pal, pred, _ = B.label_maps(61, 83)
    conf, bconf, _ = B.boundary_confusion([pic], [gt], pal, dilation_ratio=.35)
    assert B.dilation(61, 83, .35) == 36 and np.array_equal(B.boundary(pred, 36), pred)
    assert bconf.sum() == 5063 and np.array_equal(bconf, conf) and bconf[0, 0] == 0


def test_boundary_on_a_hand_case():
    """A 7 x 9 map of label 5 with a 3 x 3 block of label 2, d = 1: the outer ring keeps its 5 (a window that leaves the picture holds a
    0), the pixels around the block see a 2 (5 - 2 = 3), the block's own pixels and the rest are 0."""
    m = np.full((7, 9), 5, np.uint8)
    m[2:5, 3:6] = 2
    want = np.array([[5, 5, 5, 5, 5, 5, 5, 5, 5],
                     [5, 0, 3, 3, 3, 3, 3, 0, 5],
                     [5, 0, 3, 0, 0, 0, 3, 0, 5],
                     [5, 0, 3, 0, 0, 0, 3, 0, 5],
                     [5, 0, 3, 0, 0, 0, 3, 0, 5],
                     [5, 0, 3, 3, 3, 3, 3, 0, 5],
                     [5, 5, 5, 5, 5, 5, 5, 5, 5]], np.uint8)
    assert np.array_equal(B.boundary(m, 1), want) and np.array_equal(B.boundary_iterated(m, 1), want)


@pytest.mark.parametrize("h,w,d", [(20, 30, 3), (9, 40, 4), (9, 9, 5)])
def test_boundary_of_uniform_maps(h, w, d):
    m = np.full((h, w), 7, np.uint8)
    want = m.copy()
    want[d:h - d, d:w - d] = 0                                         # a frame of width d; nothing inside it where 2d + 1 > h
    assert np.array_equal(B.boundary(m, d), want) and np.array_equal(B.boundary_iterated(m, d), want)
    zeros = np.zeros((h, w), np.uint8)
    assert not B.boundary(zeros, d).any() and not B.boundary_iterated(zeros, d).any()


def test_scores_on_a_hand_matrix_pair():
    """K = 3.  Class 0: b_iou < iou; class 1: b_iou > iou; class 2: absent from the ground truth (iou NaN) but on both boundaries
    (b_iou not NaN) -> min stays NaN.  A second pair: class 1 nowhere on a boundary (b_union == 0, b_iou NaN) -> min is the iou."""
    from painter_amd import painter_engine as E
    conf = np.array([[6, 1, 0, 5],
                     [2, 3, 0, 7],
                     [1, 1, 0, 9],
                     [0, 0, 0, 0]], np.int64)
    bconf = np.array([[20, 2, 1, 4],
                      [9, 5, 0, 1],
                      [3, 0, 2, 2],
                      [0, 0, 0, 0]], np.int64)
    iou = np.array([6 / 10, 3 / 7, np.nan])
    b_iou = np.array([20 / (32 + 23 - 20), 5 / (7 + 14 - 5), 2 / (3 + 5 - 2)])
    bconf[1, 1] = 13                                                   # 13 / (15 + 22 - 13) > 3 / 7
    b_iou[1] = 13 / 24
    assert b_iou[0] < iou[0] and b_iou[1] > iou[1]
    for s in (E.semseg_scores(conf, bconf), dict(B.boundary_scores(conf, bconf))):
        assert np.allclose(s["BoundaryIoU"], 100 * b_iou, rtol=1e-15, atol=0)
        assert np.allclose(s["minIoU_BIoU"][:2], [100 * b_iou[0], 100 * iou[1]], rtol=1e-15, atol=0) and np.isnan(s["minIoU_BIoU"][2])
    empty = bconf.copy()
    empty[1, :3], empty[:3, 1] = 0, 0
    got, want = E.semseg_scores(conf, empty), B.boundary_scores(conf, empty)
    assert np.isnan(got["BoundaryIoU"][1]) and got["minIoU_BIoU"][1] == got["IoU"][1] == 100 * 3 / 7
    for s in (E.semseg_scores(conf, bconf), got):
        assert set(s) == OLD_KEYS | {"BoundaryIoU", "minIoU_BIoU"} and s["BoundaryIoU"].dtype == s["minIoU_BIoU"].dtype == np.float64
    for key in want:
        assert np.array_equal(got[key], want[key], equal_nan=True)
    # the old six are what they were, and alone without a boundary matrix
    alone = E.semseg_scores(conf)
    assert set(alone) == OLD_KEYS and all(np.array_equal(alone[key], got[key], equal_nan=True) for key in alone)
    assert list(inspect.signature(E.semseg_scores).parameters) == ["matrix", "boundary_matrix"]


def test_scores_of_a_seeded_case_equal_the_statement():
    from painter_amd import painter_engine as E
    pic, gt, pal = C.semseg_fixture_case("ade_61x83")
    conf, bconf, _ = B.boundary_confusion([pic], [gt], pal)
    got, want = E.semseg_scores(conf, bconf), B.boundary_scores(conf, bconf)
    assert np.isfinite(got["BoundaryIoU"]).sum() >= 5
    for key in want:
        assert np.array_equal(got[key], want[key], equal_nan=True), key


def test_header_declares_and_library_resolves_the_entry_points():
    from painter_amd._lib import lib, parse_header
    protos = parse_header()
    for name in ("pa_semseg_boundary_confusion", "pa_semseg_boundary_workspace_bytes", "pa_label_boundary"):
        assert name in protos
        assert getattr(lib, name) is not None
    assert len(protos["pa_semseg_boundary_confusion"][1]) == 13 and len(protos["pa_label_boundary"][1]) == 7
    assert len(protos["pa_semseg_confusion"][1]) == 11                 # unchanged
    assert lib.pa_abi_version() == 9
    # four byte maps of total_pixels rounded up to 16
    assert lib.pa_semseg_boundary_workspace_bytes(5063) == 4 * 5072 and lib.pa_semseg_boundary_workspace_bytes(1) == 64
    assert lib.pa_semseg_boundary_workspace_bytes(1 << 31) == 4 << 31
    assert lib.pa_semseg_boundary_workspace_bytes(0) == lib.pa_semseg_boundary_workspace_bytes(-5) == -1
    assert lib.pa_semseg_boundary_workspace_bytes((1 << 31) + 1) == -1
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "painter_hip.h")).read()
    assert "pa_boundary_job" in header and "without its boundary branch" in header


def test_signatures_and_job_record():
    from painter_amd import painter_engine as E

    def defaults(fn):
        return {k: v.default for k, v in inspect.signature(fn).parameters.items() if v.default is not inspect.Parameter.empty}
    assert defaults(E.SemsegBoundaryScore.__init__) == dict(dist_type="abs", ignore_label=255, dilation_ratio=0.02, device="cuda")
    assert defaults(E.SemsegScore.__init__) == dict(dist_type="abs", ignore_label=255, device="cuda")
    assert issubclass(E.SemsegBoundaryScore, E.SemsegScore)
    assert E.ctypes.sizeof(E.BoundaryJob) == 32 and E.ctypes.sizeof(E.ScoreJob) == 24
    assert [f[0] for f in E.BoundaryJob._fields_] == ["picture", "gt", "h", "w", "d", "reserved"] and E.BoundaryJob.d.offset == 24


def test_refusals_before_anything_touches_a_device():
    from painter_amd import painter_engine as E
    pal = C.coco_palette()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.SemsegBoundaryScore(pal, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.label_boundary(np.zeros((4, 4), np.uint8), device="cpu")
    with pytest.raises(ValueError, match="detectron2"):
        E.SemsegBoundaryScore(C.synthetic_palette(255))
    for ratio in (0.0, -0.02, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="dilation_ratio"):
            E.SemsegBoundaryScore(pal, dilation_ratio=ratio)
        with pytest.raises(ValueError, match="dilation_ratio"):
            E.label_boundary(np.zeros((4, 4), np.uint8), dilation_ratio=ratio)
        with pytest.raises(ValueError, match="dilation_ratio"):
            E.boundary_dilation(4, 4, ratio)
