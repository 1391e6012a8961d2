"""The scoring definition (tests/painter_score_host.py) against what the unmodified reference produced (tests/golden/painter_score.npz:
SemSegEvaluatorCustom.process of both semantic evaluators, eval / compute_errors of nyuv2_depth/eval_with_pngs.py), the final ratios on
a hand-written matrix, and what can be said about the entry points without a GPU."""
import inspect
import os

import numpy as np
import pytest

from tests import painter_score_cases as C
from tests import painter_score_host as H


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "painter_score.npz"))


def fixture_matrix(golden, name, dist_type, k):
    conf = np.zeros((k + 1) ** 2, np.int64)
    conf[golden["semseg.%s.%s.bins" % (name, dist_type)]] = golden["semseg.%s.%s.counts" % (name, dist_type)]
    return conf.reshape(k + 1, k + 1)


SEMSEG_CASES = [(name, d) for name, case in C.SEMSEG.items() for d in case[4]]


def test_header_declares_and_library_resolves_the_entry_points():
    from painter_amd._lib import lib, parse_header
    protos = parse_header()
    for name in ("pa_semseg_confusion", "pa_semseg_lds_bins", "pa_depth_errors", "pa_depth_workspace_bytes"):
        assert name in protos
        assert getattr(lib, name) is not None
    assert len(protos["pa_semseg_confusion"][1]) == 11 and len(protos["pa_depth_errors"][1]) == 8
    assert lib.pa_abi_version() == 9
    # the LDS budget: 12 K bytes of palette rounded up to 16, plus 4 (K + 1)^2 bytes of bins, within 160 KB -- K = 199 is the last that fits
    for k in (1, 133, 150, 199, 200, 255):
        fits = -(-12 * k // 16) * 16 + 4 * (k + 1) ** 2 <= 160 * 1024
        assert lib.pa_semseg_lds_bins(k) == int(fits) == int(k <= 199)
    assert lib.pa_semseg_lds_bins(0) == lib.pa_semseg_lds_bins(256) == 0
    assert lib.pa_depth_workspace_bytes(8) == 8 * 32 * 10 * 8 and lib.pa_depth_workspace_bytes(0) == lib.pa_depth_workspace_bytes(65536) == -1


@pytest.mark.parametrize("name,dist_type", SEMSEG_CASES)
def test_host_confusion_equals_the_reference(golden, name, dist_type):
    pic, gt, pal = C.semseg_fixture_case(name)
    ref = fixture_matrix(golden, name, dist_type, len(pal))
    got, invalid = H.confusion([pic], [gt], pal, dist_type)
    assert invalid == 0 and got.dtype == np.int64 and np.array_equal(got, ref)
    assert ref.sum() == pic.shape[0] * pic.shape[1] and ref[:, -1].sum() == (gt == C.IGNORE).sum() > 0 and ref[-1].sum() == 0


def test_fixture_covers_what_it_is_there_for(golden):
    off = 0
    for name, dist_type in SEMSEG_CASES:
        k = len(C.semseg_fixture_case(name)[2])
        idx = golden["semseg.%s.%s.bins" % (name, dist_type)]
        off += int((idx // (k + 1) != idx % (k + 1)).sum())
    assert off >= 20
    assert {len(C.semseg_fixture_case(n)[2]) for n in C.SEMSEG} == {133, 150}
    assert {d for _, d in SEMSEG_CASES} == {"abs", "square", "mean"}


@pytest.mark.parametrize("name", list(C.DEPTH))
def test_host_depth_errors_equal_the_reference(golden, name):
    """n and the counts exactly (d1 .. d3 after rounding to float32); the six sums within 4 x the deviation the float32 reference showed
    from the statement when the fixture was made, per case and metric -- the margin over its own summation noise, measured."""
    pred, gt = C.depth_fixture_case(name)
    kw = C.DEPTH[name][3]
    sums, abs_log, clamp = H.depth_sums(pred, gt, **kw)
    ref, dev = golden["depth.%s.reference" % name], golden["depth.%s.ref_dev" % name]
    assert ref.dtype == np.float32 and ref.shape == (9,) and dev.shape == (6,)
    assert np.array_equal(sums, golden["depth.%s.sums" % name])
    assert np.array_equal(np.float32(sums[1:4] / sums[0]), ref[6:9])
    got = H.depth_metrics(sums)
    err = np.abs(got[:6] - ref[:6].astype(np.float64)) / np.abs(ref[:6].astype(np.float64))
    assert (err <= 4 * dev).all(), (err, dev)
    assert abs_log >= abs(sums[8])
    if name == "nyu_eigen":
        assert clamp["low"] > 0 and clamp["high"] > 0


def test_depth_statement_on_a_hand_case():
    """Two valid pixels, one clamped prediction, one pixel at min_depth, one at max_depth, one outside the box."""
    gt = np.array([[2000, 1, 10000, 4000, 3000]], np.uint16)
    pred = np.array([[2500, 5, 5, 0, 3000]], np.int32)
    sums, abs_log, clamp = H.depth_sums(pred, gt, max_depth=10.0, crop=(0, 1, 0, 4))
    assert sums[0] == 2 and clamp == dict(low=1, high=0)
    assert list(sums[1:4]) == [0, 1, 1]                                  # 2.5 / 2 = 1.25 is not < 1.25; 4 / 0.001 is far off
    p, g = np.float32(2.5), np.float32(2.0)
    p2, g2 = np.float32(1e-3), np.float32(4.0)
    assert sums[4] == (float(g) - float(p)) ** 2 + (float(g2) - float(p2)) ** 2
    empty = H.depth_sums(pred, np.zeros_like(gt))[0]
    assert empty[0] == 0 and np.isnan(H.depth_metrics(empty)).all()


def test_scores_on_a_hand_matrix():
    """K = 3: class 2 is absent from the ground truth (but predicted), the last column holds ignored pixels."""
    from painter_amd import painter_engine as E
    conf = np.array([[6, 1, 0, 5],
                     [2, 3, 0, 7],
                     [1, 1, 0, 9],
                     [0, 0, 0, 0]], np.int64)
    for s in (H.scores(conf), E.semseg_scores(conf)):
        iou0, iou1 = 6 / (9 + 7 - 6), 3 / (5 + 5 - 3)
        assert np.isclose(s["IoU"][:2], [100 * iou0, 100 * iou1]).all() and np.isnan(s["IoU"][2]) and np.isnan(s["ACC"][2])
        assert np.isclose(s["mIoU"], 100 * (iou0 + iou1) / 2)            # the absent class is in neither the sum nor the count
        assert np.isclose(s["mACC"], 100 * (6 / 9 + 3 / 5) / 2)
        assert np.isclose(s["pACC"], 100 * 9 / 14)                       # the 21 ignored pixels are nowhere
        assert np.isclose(s["fwIoU"], 100 * (iou0 * 9 / 14 + iou1 * 5 / 14))
    without = conf.copy()
    without[:, -1] = 0
    a, b = E.semseg_scores(conf), E.semseg_scores(without)
    assert all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)
    a, b = H.scores(conf), E.semseg_scores(conf)
    assert all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)


def test_signatures_repeat_the_default_table():
    from painter_amd import painter_engine as E

    def defaults(fn):
        return {k: v.default for k, v in inspect.signature(fn).parameters.items() if v.default is not inspect.Parameter.empty}
    assert E.DEPTH_DEFAULTS == dict(min_depth=1e-3, max_depth=80.0, crop=None, divisor=1000.0)
    for fn in (E.depth_errors, E.DepthErrors.__init__):
        have = defaults(fn)
        assert set(E.DEPTH_DEFAULTS) <= set(have) and all(have[k] == v for k, v in E.DEPTH_DEFAULTS.items()), fn.__qualname__
    assert list(inspect.signature(E.DepthErrors.__init__).parameters)[3:7] == list(E.DEPTH_DEFAULTS)          # passed on by position
    assert defaults(E.SemsegScore.__init__) == dict(dist_type="abs", ignore_label=255, device="cuda")
    assert E.EIGEN_CROP == H.EIGEN_CROP == (45, 471, 41, 601)
    for name in ("pa_score_job", "pa_depth_job"):
        assert name in open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "painter_hip.h")).read()
    assert E.ctypes.sizeof(E.ScoreJob) == 24 and E.ctypes.sizeof(E.DepthJob) == 40


def test_a_cpu_device_is_refused():
    import torch
    from painter_amd import painter_engine as E
    pal = C.coco_palette()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.SemsegScore(pal, device="cpu")
    pred, gt = np.zeros((4, 4), np.int32), np.zeros((4, 4), np.uint16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.depth_errors([pred], [gt], device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.depth_errors([torch.zeros((4, 4), dtype=torch.int32)], [gt])


def test_arguments_are_refused_before_anything_is_enqueued():
    """The engine entry points check task, keywords, sizes and crop before the first forward: an engine that would fail on any use
    proves nothing ran."""
    import types
    from painter_amd import painter_engine as E
    pictures = [np.zeros((8, 6, 3), np.uint8)]
    depth = types.SimpleNamespace(task="nyuv2_depth")
    with pytest.raises(ValueError, match="nyuv2_depth"):
        E.PainterEngine.run_depth_errors(types.SimpleNamespace(task="ade20k_semseg"), pictures, [np.zeros((8, 6), np.uint16)])
    with pytest.raises(ValueError, match="ade20k_semseg"):
        E.PainterEngine.run_semseg_score(depth, pictures, [np.zeros((8, 6), np.uint8)], None)
    with pytest.raises(TypeError, match="unexpected"):
        E.PainterEngine.run_depth_errors(depth, pictures, [np.zeros((8, 6), np.uint16)], dist_type="abs")
    with pytest.raises(ValueError, match="ground truth"):
        E.PainterEngine.run_depth_errors(depth, pictures, [np.zeros((6, 8), np.uint16)])
    with pytest.raises(ValueError, match="eigen"):
        E.PainterEngine.run_depth_errors(depth, pictures, [np.zeros((8, 6), np.uint16)], crop="eigen")
    with pytest.raises(ValueError, match="ground truth"):
        E.PainterEngine.run_semseg_score(types.SimpleNamespace(task="coco_pano_semseg"), pictures, [np.zeros((6, 8), np.uint8)], None)
    with pytest.raises(ValueError, match="leaves"):
        E._crop_box((0, 9, 0, 6), 8, 6)
    assert E._crop_box(None, 8, 6) == (0, 8, 0, 6) and E._crop_box("eigen", 480, 640) == (45, 471, 41, 601)
