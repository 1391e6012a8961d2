"""GPU parity of the scoring routes (csrc/painter_score.hip through the C ABI and painter_amd/painter_engine.py) against
tests/painter_score_host.py -- the definition -- and against what the unmodified reference produced (tests/golden/painter_score.npz).

The bars.  Confusion matrices are integers: everything is equal.  Depth: n and the three threshold counts are equal (their float32 steps
are the reference's); each of the six float64 sums is compared with the exactly rounded sum (math.fsum) of the statement's terms within
1e-9 * sum |terms|: the device adds at most ~2.4e5 float64 terms per picture, each addition within 2^-53 relative of the running sum
(<= 2.4e5 * 1.1e-16 = 3e-11 of sum |terms| in all), and its log / log10 are within a few ulp (~1e-15 relative per term) of numpy's."""
import os

import numpy as np
import pytest
import torch

from tests import painter_score_cases as C
from tests import painter_score_host as H

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from painter_amd import painter_engine as E
    from painter_amd._lib import lib

INVALID = 1                                            # hipErrorInvalidValue
SEMSEG_CASES = [(name, d) for name, case in C.SEMSEG.items() for d in case[4]]


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "painter_score.npz"))


def fixture_matrix(golden, name, dist_type, k):
    conf = np.zeros((k + 1) ** 2, np.int64)
    conf[golden["semseg.%s.%s.bins" % (name, dist_type)]] = golden["semseg.%s.%s.counts" % (name, dist_type)]
    return conf.reshape(k + 1, k + 1)


def device_matrix(pictures, gts, palette, dist_type="abs", **kw):
    return E.SemsegScore(palette, dist_type, **kw).add(pictures, gts).matrix()


# ---- 1. the unmodified reference
@pytest.mark.parametrize("name,dist_type", SEMSEG_CASES)
def test_confusion_matrix_reproduces_the_reference(golden, name, dist_type):
    pic, gt, pal = C.semseg_fixture_case(name)
    ref = fixture_matrix(golden, name, dist_type, len(pal))
    got = device_matrix([pic], [gt], pal, dist_type)
    assert got.dtype == np.int64 and got.shape == ref.shape and got.tobytes() == ref.tobytes()


# ---- 2. the definition, on the smallest shapes that can break it
def test_confusion_equals_the_host_statement_on_small_and_mixed_shapes():
    pal = C.coco_palette()
    pic, gt, _ = C.semseg_case("coco", 3, 61, 83)                       # 5063 pixels: five chunks, the last wave partly filled
    assert np.array_equal(device_matrix([pic], [gt], pal), H.confusion([pic], [gt], pal)[0])
    pairs = [C.semseg_case("coco", 20 + i, h, w)[:2] for i, (h, w) in enumerate(((1, 1), (1, 300), (300, 1), (61, 83)))]
    pics, gts = [p for p, _ in pairs], [g for _, g in pairs]
    whole = device_matrix(pics, gts, pal)
    assert np.array_equal(whole, H.confusion(pics, gts, pal)[0]) and whole.sum() == 1 + 300 + 300 + 5063
    # two calls of add equal one call with both lists; reset gives zeros
    score = E.SemsegScore(pal)
    score.add(pics[:2], gts[:2])
    score.add(pics[2:], gts[2:])
    assert np.array_equal(score.matrix(), whole)
    score.reset()
    assert not score.matrix().any() and score.add([], []) is score


def test_confusion_of_uniform_inputs():
    pal = C.coco_palette()
    pic, gt, _ = C.semseg_case("coco", 3, 61, 83)
    ignored = device_matrix([pic], [np.full_like(gt, C.IGNORE)], pal)             # everything in the ignore column
    assert ignored[:, :-1].sum() == 0 and np.array_equal(ignored, H.confusion([pic], [np.full_like(gt, C.IGNORE)], pal)[0])
    # one colour, one label: every lane of every wave hits the same bin
    flat = np.empty((96, 128, 3), np.uint8)
    flat[:] = pal[17].astype(np.uint8)
    one = device_matrix([flat], [np.full((96, 128), 40, np.uint8)], pal)
    assert one[17, 40] == 12288 and one.sum() == 12288
    # row sums are the histogram of the class map
    rows = device_matrix([pic], [gt], pal).sum(1)
    assert np.array_equal(rows[:-1], np.bincount(E.class_map(pic, np.array(pal)).reshape(-1), minlength=len(pal))) and rows[-1] == 0


@pytest.mark.parametrize("k", [199, 200, 255])
def test_bins_in_lds_and_in_memory(k):
    """The workgroup's bins fit in LDS up to K = 199; from K = 200 the runs add to memory.  Both, and the forced direct form, equal the
    statement."""
    assert lib.pa_semseg_lds_bins(k) == int(k <= 199)
    pal = C.synthetic_palette(k)
    pic, gt = C.noisy_case(k, 61, 83, pal, ignore=k < 255)                # at K = 255 the ignore label 255 is the byte's last value
    ref = H.confusion([pic], [gt], pal)[0]
    assert np.array_equal(device_matrix([pic], [gt], pal), ref) and (ref[np.arange(k), np.arange(k)] > 0).any()
    forced = E.SemsegScore(pal)
    forced.bins = 1
    assert np.array_equal(forced.add([pic], [gt]).matrix(), ref)


def test_invalid_labels_are_counted_and_reported():
    pal = C.coco_palette()
    pic, gt, _ = C.semseg_case("coco", 3, 61, 83)
    bad = gt.copy()
    bad[5, :7], bad[9, 3] = 133, 254
    score = E.SemsegScore(pal).add([pic], [bad])
    with pytest.raises(ValueError, match=r"\b8 ground-truth pixels"):
        score.matrix()
    ref, invalid = H.confusion([pic], [bad], pal)
    assert invalid == 8
    a = score.out.cpu().numpy()
    assert np.array_equal(E._section(a, score.at, "conf").reshape(134, 134), ref) and ref.sum() == 5063 - 8


# ---- 3. depth
def _check_depth(pred, gt, kw, got_metrics, got_n, sums_dev):
    sums, abs_log, _ = H.depth_sums(pred, gt, **kw)
    assert np.array_equal(sums_dev[:4], sums[:4]) and got_n == sums[0]
    scale = np.array([sums[4], sums[5], sums[6], sums[7], abs_log, sums[9]])          # all terms but the signed one are >= 0
    err = np.abs(sums_dev[4:] - sums[4:])
    print("depth sums: device - statement", err, "bound", 1e-9 * scale)
    assert (err <= 1e-9 * scale).all(), (err, 1e-9 * scale)
    if sums[0]:
        assert np.allclose(got_metrics, H.depth_metrics(sums), rtol=1e-7, atol=0)
    else:
        assert np.isnan(got_metrics).all()


@pytest.mark.parametrize("name", list(C.DEPTH))
def test_depth_errors_reproduce_the_reference_and_the_statement(golden, name):
    pred, gt = C.depth_fixture_case(name)
    kw = C.DEPTH[name][3]
    job = E.DepthErrors([torch.from_numpy(pred).cuda()], [torch.from_numpy(gt.view(np.int16)).cuda()], **dict(E.DEPTH_DEFAULTS, **kw))
    sums_dev = job.sums()[0]
    metrics, n = E.depth_errors([pred], [gt], **kw)
    assert metrics.shape == (1, 9) and metrics.dtype == np.float64 and n.dtype == np.int64
    _check_depth(pred, gt, kw, metrics[0], n[0], sums_dev)
    ref, dev = golden["depth.%s.reference" % name], golden["depth.%s.ref_dev" % name]
    assert np.array_equal(np.float32(metrics[0, 6:]), ref[6:])
    err = np.abs(metrics[0, :6] - ref[:6].astype(np.float64)) / np.abs(ref[:6].astype(np.float64))
    print("depth: relative distance to the reference", err, "4 x ref_dev", 4 * dev)
    assert (err <= 4 * dev).all(), (err, 4 * dev)


def test_depth_errors_of_boxes_empty_pictures_and_mixed_sizes():
    big, small = C.depth_case(31, 64, 80), C.depth_case(32, 37, 53)
    preds, gts = [big[0], small[0]], [big[1], small[1]]
    both_m, both_n = E.depth_errors(preds, gts, max_depth=10.0)                        # two sizes in one table
    sums = E.DepthErrors([torch.from_numpy(p).cuda() for p in preds], [torch.from_numpy(g.view(np.int16)).cuda() for g in gts],
                         max_depth=10.0).sums()
    for i in range(2):
        _check_depth(preds[i], gts[i], dict(max_depth=10.0), both_m[i], both_n[i], sums[i])
        alone_m, alone_n = E.depth_errors(preds[i:i + 1], gts[i:i + 1], max_depth=10.0)
        assert alone_m.tobytes() == both_m[i:i + 1].tobytes() and alone_n[0] == both_n[i]
    # a box of one pixel
    y, x = 20, 30
    assert small[1][y, x] > 1
    one_m, one_n = E.depth_errors([small[0]], [small[1]], crop=(y, y + 1, x, x + 1))
    assert one_n[0] == 1
    _check_depth(small[0], small[1], dict(crop=(y, y + 1, x, x + 1)), one_m[0], one_n[0],
                 E.DepthErrors([torch.from_numpy(small[0]).cuda()], [torch.from_numpy(small[1].view(np.int16)).cuda()],
                               crop=(y, y + 1, x, x + 1)).sums()[0])
    # no valid pixel: nine NaN and n = 0, as the reference's mean of nothing
    none_m, none_n = E.depth_errors([small[0]], [np.zeros_like(small[1])])
    assert none_n[0] == 0 and np.isnan(none_m).all()
    empty_m, empty_n = E.depth_errors([small[0]], [small[1]], crop=(5, 5, 0, 53))
    assert empty_n[0] == 0 and np.isnan(empty_m).all()
    assert E.depth_errors([], [])[0].shape == (0, 9)


# ---- 4. determinism, inputs
def test_two_runs_give_identical_bytes_and_tensors_equal_arrays():
    pic, gt, pal = C.semseg_fixture_case("ade_96x128")
    first, again = device_matrix([pic], [gt], pal), device_matrix([pic], [gt], pal)
    assert first.tobytes() == again.tobytes()
    dev = device_matrix([torch.from_numpy(pic).cuda()], [torch.from_numpy(gt).cuda()], pal)
    assert first.tobytes() == dev.tobytes()
    pred, dgt = C.depth_case(33, 120, 160)
    a, b = E.depth_errors([pred], [dgt], max_depth=10.0), E.depth_errors([pred], [dgt], max_depth=10.0)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[1][0] > 0
    tensors = [torch.from_numpy(pred).cuda()], [torch.from_numpy(dgt.view(np.int16)).cuda()]
    sums = [E.DepthErrors(*tensors, max_depth=10.0).sums() for _ in range(2)]
    assert sums[0].tobytes() == sums[1].tobytes()
    c = E.depth_errors(*tensors, max_depth=10.0)
    assert a[0].tobytes() == c[0].tobytes()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.SemsegScore(pal).add([torch.from_numpy(pic)], [gt])


# ---- 5. the engine
def _engine(task, bs):
    from tests import painter_eval_cases as PC
    return E.PainterEngine(PC.StandInModel(), "cuda", task, *PC.prompt_pair(), input_size=PC.RES, batch_size=bs)


def test_run_semseg_score_equals_scoring_the_pictures_run_returns():
    from tests import painter_eval_cases as PC
    queries = [PC.picture(91, 64, 48), PC.picture(92, 60, 80), PC.picture(93, 45, 70)]
    sizes = [(24, 32), (40, 30), (35, 23)]                              # (width, height)
    pal = C.ade_palette()
    rng = np.random.default_rng(5)
    gts = [rng.integers(0, 150, (h, w)).astype(np.uint8) for w, h in sizes]
    gts[1][3] = C.IGNORE
    painted = _engine("ade20k_semseg", 8).run(queries, sizes)
    ref = device_matrix(painted, gts, pal)
    assert ref.sum() == sum(w * h for w, h in sizes) and np.array_equal(ref, H.confusion(painted, gts, pal)[0])
    for bs in (1, 2, 8):
        score = E.SemsegScore(pal)
        assert _engine("ade20k_semseg", bs).run_semseg_score(queries, gts, score, sizes) is score
        assert np.array_equal(score.matrix(), ref), bs
    assert set(E.SemsegScore(pal).add(painted, gts).scores()) == {"mIoU", "fwIoU", "mACC", "pACC", "IoU", "ACC"}


def test_run_depth_errors_equals_scoring_the_pictures_run_returns():
    from tests import painter_eval_cases as PC
    queries = [PC.picture(91, 64, 48), PC.picture(92, 60, 80), PC.picture(93, 45, 70)]
    sizes = [(24, 32), (40, 30), (35, 23)]
    rng = np.random.default_rng(6)
    gts = [rng.integers(0, 11000, (h, w)).astype(np.uint16) for w, h in sizes]
    painted = _engine("nyuv2_depth", 8).run(queries, sizes)
    assert painted[0].dtype == np.int32 and painted[0].shape == (32, 24)
    ref = E.depth_errors(painted, gts, max_depth=10.0)
    assert (ref[1] > 0).all()
    for bs in (1, 2, 8):
        got = _engine("nyuv2_depth", bs).run_depth_errors(queries, gts, sizes, max_depth=10.0)
        assert got[0].tobytes() == ref[0].tobytes() and np.array_equal(got[1], ref[1]), bs


# ---- 6. refusals
def test_engine_refusals():
    from tests import painter_eval_cases as PC
    queries = [PC.picture(91, 64, 48)]
    pal = C.coco_palette()
    with pytest.raises(ValueError, match="ade20k_semseg"):
        _engine("coco_pose", 2).run_semseg_score(queries, [np.zeros((64, 48), np.uint8)], E.SemsegScore(pal))
    with pytest.raises(ValueError, match="nyuv2_depth"):
        _engine("ade20k_semseg", 2).run_depth_errors(queries, [np.zeros((64, 48), np.uint16)])
    with pytest.raises(ValueError, match="ground truth"):
        E.SemsegScore(pal).add([np.zeros((8, 6, 3), np.uint8)], [np.zeros((6, 8), np.uint8)])
    with pytest.raises(ValueError, match="ground truth"):
        E.depth_errors([np.zeros((8, 6), np.int32)], [np.zeros((8, 7), np.uint16)])
    with pytest.raises(ValueError, match="eigen"):
        E.depth_errors([np.zeros((8, 6), np.int32)], [np.zeros((8, 6), np.uint16)], crop="eigen")
    with pytest.raises(TypeError, match="unexpected"):
        _engine("nyuv2_depth", 2).run_depth_errors(queries, [np.zeros((64, 48), np.uint16)], dist_thr=3.0)
    with pytest.raises(NotImplementedError):
        E.SemsegScore(pal, dist_type="cubic")
    with pytest.raises(RuntimeError, match="pa_semseg_confusion"):
        E.SemsegScore(C.synthetic_palette(256)).add([np.zeros((4, 4, 3), np.uint8)], [np.zeros((4, 4), np.uint8)])
    with pytest.raises(RuntimeError, match="pa_depth_errors"):
        E.depth_errors([np.zeros((8, 6), np.int32)], [np.zeros((8, 6), np.uint16)], min_depth=5.0, max_depth=1.0)


def test_entry_points_refuse_bad_arguments():
    """hipErrorInvalidValue (1) before anything is launched: no pointer is touched."""
    a = 256                                            # a non-null, aligned, never dereferenced address
    ok = dict(n_jobs=2, total=100, k=133, dist=0, bins=0)

    def conf(c, ptrs=None):
        jobs, pal, out, inv = ptrs or [a] * 4
        return lib.pa_semseg_confusion(jobs, c["n_jobs"], c["total"], pal, c["k"], c["dist"], 255, c["bins"], out, inv, 0)

    for change in (dict(n_jobs=0), dict(n_jobs=65536), dict(total=0), dict(total=(1 << 31) + 1), dict(k=0), dict(k=256), dict(dist=-1),
                   dict(dist=3), dict(bins=2)):
        assert conf(dict(ok, **change)) == INVALID, change
    for null in range(4):
        assert conf(ok, [0 if i == null else a for i in range(4)]) == INVALID, null
    assert conf(ok, [a, a, a + 4, a]) == INVALID                       # misaligned matrix

    def depth(n_jobs=2, divisor=1000.0, lo=1e-3, hi=80.0, ptrs=None):
        jobs, out, ws = ptrs or [a] * 3
        return lib.pa_depth_errors(jobs, n_jobs, divisor, lo, hi, out, ws, 0)

    for kw in (dict(n_jobs=0), dict(n_jobs=65536), dict(divisor=0.0), dict(divisor=float("nan")), dict(lo=0.0), dict(lo=80.0),
               dict(hi=float("inf")), dict(lo=float("nan"))):
        assert depth(**kw) == INVALID, kw
    for null in range(3):
        assert depth(ptrs=[0 if i == null else a for i in range(3)]) == INVALID, null
    assert depth(ptrs=[a, a + 4, a]) == INVALID
