"""GPU parity of panoptic quality (csrc/painter_pq.hip through painter_engine.PanopticQuality) against tests/painter_pq_host.py -- the
definition, restated from panopticapi's published source and unverified against panopticapi.

The bar: tp, fp, fn are integers and equal; the IoU sums are float64 sums of correctly rounded quotients of integers, added in the
statement's order (pictures as added, matches in ascending (g, p)) by one thread per category, so they are equal as bytes."""
import os

import numpy as np
import pytest
import torch

from tests import painter_pq_cases as C
from tests import painter_pq_host as H

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from painter_amd import painter_engine as E
    from painter_amd._lib import lib


def quality(cases, bins=0, caps=(1, 1), gt="gt", k=C.K, n_things=C.THINGS, score=None):
    score = score or E.PanopticQuality(k, n_things)
    score.bins, score.min_caps = bins, caps
    got = score.add([c["pred"] for c in cases], [c["pred_segments"] for c in cases], [c[gt] for c in cases], [c["gt_segments"] for c in cases])
    assert got is score
    return score


def statement(cases, k=C.K):
    return H.pq([c["pred"] for c in cases], [c["pred_segments"] for c in cases], [c["gt"] for c in cases], [c["gt_segments"] for c in cases], k)


def same(counts, ref):
    tp, fp, fn, iou = counts
    assert tp.dtype == fp.dtype == fn.dtype == np.int64 and iou.dtype == np.float64
    assert np.array_equal(tp, ref[0]) and np.array_equal(fp, ref[1]) and np.array_equal(fn, ref[2]), (tp, ref[0], fp, ref[1], fn, ref[2])
    assert iou.tobytes() == ref[3].tobytes(), (iou, ref[3])


@pytest.fixture(scope="module")
def odd():
    """61 x 83 = 5063 pixels: three chunks of 2048, the last wave partly filled; 7 ground-truth and 9 predicted segments, noise, one
    crowd segment, VOID on both sides, one unlisted ground-truth id.  -> (case, statement)."""
    case = C.case(3, 61, 83, 7, 9, noise=0.05)
    ref, flags = statement([case])
    assert flags == [0] and ref[0].sum() >= 2 and ref[1].sum() >= 1 and ref[2].sum() >= 1
    return case, ref


@pytest.fixture(scope="module")
def mixed():
    """1 x 1 without any segment (G = 0, predicted count 0), 1 x 300, 300 x 1 and 61 x 83, table sizes all different."""
    cases = [C.case(20, 1, 1, 0, 0), C.case(21, 1, 300, 2, 3, noise=0.1, crowd=0), C.case(22, 300, 1, 4, 2, noise=0.1),
             C.case(23, 61, 83, 7, 9, noise=0.05)]
    assert not cases[0]["gt_segments"] and not cases[0]["pred_segments"]
    assert len({len(c["gt_segments"]) for c in cases}) == 4
    ref, flags = statement(cases)
    assert flags == [0, 0, 0, 0] and ref[0].sum() >= 2
    return cases, ref


def test_odd_size_equals_the_statement(odd):
    case, ref = odd
    same(quality([case]).counts(), ref)
    assert set(quality([case]).result()) == {"PQ", "SQ", "RQ", "PQ_th", "SQ_th", "RQ_th", "PQ_st", "SQ_st", "RQ_st", "per_class", "n"}
    host = H.averages(*ref, [c < C.THINGS for c in range(C.K)])
    got = quality([case]).result()
    assert all(got[k] == host[k] or (np.isnan(got[k]) and np.isnan(host[k])) for k in host if k not in ("per_class", "n")) and got["n"] == host["n"]


def test_mixed_batch_equals_the_statement(mixed):
    cases, ref = mixed
    same(quality(cases).counts(), ref)


@pytest.mark.parametrize("bins,caps,lds", [(0, (1, 1), 1), (1, (1, 1), 1), (0, (254, 255), 0)])
def test_both_bin_routes(odd, mixed, bins, caps, lds):
    assert lib.pa_pq_lds_bins(max(caps[0], 7), max(caps[1], 9)) == lds
    same(quality([odd[0]], bins, caps).counts(), odd[1])
    same(quality(mixed[0], bins, caps).counts(), mixed[1])


def test_uniform_input():
    """One predicted and one ground-truth segment cover 96 x 128: every lane of every wave hits one bin."""
    case = dict(pred=np.full((96, 128), 1, np.int32), pred_segments=[dict(id=1, category_id=17)], gt=np.full((96, 128), 0x123456, np.int32),
                gt_segments=[dict(id=0x123456, category_id=17, iscrowd=0, area=12288)])
    for bins in (0, 1):
        score = quality([case], bins)
        tp, fp, fn, iou = score.counts()
        assert tp[17] == 1 and tp.sum() == 1 and not fp.any() and not fn.any() and iou[17] == 1.0 and iou.sum() == 1.0
    # the count itself: with area None the union is 12288 + C - C, so any other count would move the IoU off 1.0 only with VOID;
    # read the job's matrix where the launch left it
    ws = np.frombuffer(score._last[4].cpu().numpy().tobytes()[:4 * 3 * 2], np.uint32).reshape(3, 2)
    assert ws[1, 1] == 12288 and ws.sum() == 12288


def test_repeated_adds_and_reset(mixed):
    cases, ref = mixed
    score = quality(cases[:2])
    quality(cases[2:], score=score)
    same(score.counts(), ref)
    score.reset()
    assert not any(v.any() for v in score.counts())
    assert score.add([], [], [], []) is score and not any(v.any() for v in score.counts())


def test_two_runs_give_identical_bytes_and_tensors_equal_arrays(mixed):
    cases, ref = mixed
    a, b = quality(cases).counts(), quality(cases).counts()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    dev = E.PanopticQuality().add([torch.from_numpy(c["pred"]).cuda() for c in cases], [c["pred_segments"] for c in cases],
                                  [torch.from_numpy(c["gt"]).cuda() for c in cases], [c["gt_segments"] for c in cases]).counts()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, dev))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.PanopticQuality().add([torch.from_numpy(cases[0]["pred"])], [[]], [cases[0]["gt"]], [[]])


def test_rgb_ground_truth_equals_the_int32_form(odd, mixed):
    same(quality([odd[0]], gt="gt_rgb").counts(), odd[1])
    same(quality(mixed[0], gt="gt_rgb").counts(), mixed[1])


def _seg(i, cat=0, crowd=0, area=None):
    return dict(id=i, category_id=cat, iscrowd=crowd, area=area)


FLAG_CASES = [
    (0, [[5]], [], [[0]], []),
    (1, [[0]], [_seg(1)], [[0]], []),
    (2, [[1]], [_seg(1, 3)], [[0]], []),
    (3, [[1]], [_seg(1)], [[7]], [_seg(7, area=0)]),
    (4, [[1, 1]], [_seg(1)], [[7, 8]], [_seg(7, area=0), _seg(8, area=0)]),
    (5, [[1]], [_seg(1)], [[7]], [_seg(7, area=1), _seg(7, area=1)]),
]


@pytest.mark.parametrize("bit,pred,pred_segments,gt,gt_segments", FLAG_CASES)
def test_each_flag_bit_from_its_smallest_input(bit, pred, pred_segments, gt, gt_segments):
    good = dict(pred=np.array([[1, 1]], np.int32), pred_segments=[_seg(1)], gt=np.array([[7, 7]], np.int32), gt_segments=[_seg(7, area=2)])
    bad = dict(pred=np.array(pred, np.int32), pred_segments=pred_segments, gt=np.array(gt, np.int32), gt_segments=gt_segments)
    ref, flags = statement([good, bad, good], 3)
    assert flags == [0, 1 << bit, 0] and ref[0].tolist() == [2, 0, 0]
    score = quality([good, bad, good], k=3, n_things=2)
    with pytest.raises(ValueError, match=r"picture 1 is refused \(flag bit %d," % bit):
        score.result()
    with pytest.raises(ValueError, match="picture 1 "):
        score.counts()
    assert score._flags[0].cpu().numpy().view(np.uint32).tolist() == flags
    a = score.out.cpu().numpy()                            # the flagged picture added nothing, the others did
    same(tuple(E._section(a, score.at, name) for name in ("tp", "fp", "fn", "iou")), ref)


def test_categories_table_maps_data_set_ids(odd):
    case, ref = odd
    cats = [dict(id=1000 + 7 * c, isthing=int(c % 2)) for c in range(C.K)]
    remap = lambda segs: [dict(s, category_id=1000 + 7 * s["category_id"]) for s in segs]
    score = E.PanopticQuality(categories=cats).add([case["pred"]], [remap(case["pred_segments"])], [case["gt"]], [remap(case["gt_segments"])])
    same(score.counts(), ref)
    res = score.result()
    assert set(res["per_class"]) == {c["id"] for c in cats} and res["n"]["Things"] + res["n"]["Stuff"] == res["n"]["All"]
    unknown = E.PanopticQuality(categories=cats).add([case["pred"]], [case["pred_segments"]], [case["gt"]], [remap(case["gt_segments"])])
    with pytest.raises(ValueError, match="flag bit 2"):
        unknown.counts()


def test_chained_behind_the_panoptic_decode(golden_dir):
    """add_decodes on a launched decode equals add on what panoptic() copied back, and the decode's own result is untouched by it."""
    golden = np.load(os.path.join(golden_dir, "painter_pano.npz"))
    sem, inst = golden["defaults.semseg"], golden["defaults.inst"]
    kw = dict(overlap_threshold=0.5, stuff_area_thresh=256, instances_score_thresh=0.55)
    plain = E.panoptic(sem, inst, **kw)
    assert np.array_equal(plain["panoptic"], golden["defaults.panoptic"]) and len(plain["segments"]) >= 3
    gt, gt_segments = C.gt_for_map(11, plain["panoptic"], plain["segments"])
    ref, flags = H.pq([plain["panoptic"]], [plain["segments"]], [gt], [gt_segments])
    assert flags == [0] and ref[0].sum() >= 1 and ref[1].sum() + ref[2].sum() >= 1
    copied = E.PanopticQuality().add([plain["panoptic"]], [plain["segments"]], [gt], [gt_segments]).counts()
    same(copied, ref)
    dec = E._launch_panoptic(torch.from_numpy(sem).cuda(), torch.from_numpy(inst).cuda(), None, None, 80, dict(dist_type="abs", **kw), {})
    chained = E.PanopticQuality().add_decodes([dec], [gt], [gt_segments])
    res = dec.result()
    assert sorted(res) == sorted(plain)
    for key in plain:
        assert res[key] == plain[key] if key == "segments" else res[key].tobytes() == plain[key].tobytes(), key
    got = chained.counts()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got, copied))


def test_run_panoptic_quality_equals_scoring_what_run_panoptic_returns():
    from tests import painter_eval_cases as PC
    pictures = [PC.picture(81, 60, 80), PC.picture(82, 45, 70), PC.picture(83, 64, 48)]
    kw = dict(dist_thr=[30.0], nms_pre=150, max_num=20, stuff_area_thresh=64, instances_score_thresh=0.0, overlap_threshold=0.4)
    target = PC.picture(PC.PROMPT[0] + 200, PC.PROMPT[1], PC.PROMPT[2], flat=True)

    def engine(task, bs, tgt=None):
        img, own = PC.prompt_pair()
        return E.PainterEngine(PC.StandInModel(), "cuda", task, img, own if tgt is None else tgt, input_size=PC.RES, batch_size=bs)
    results = E.run_panoptic(engine("coco_pano_semseg", 8), engine("coco_pano_inst", 8, target), pictures, **kw)
    annotations = [C.gt_for_map(30 + i, r["panoptic"], r["segments"]) for i, r in enumerate(results)]
    gts, segs = [a[0] for a in annotations], [a[1] for a in annotations]
    ref, flags = H.pq([r["panoptic"] for r in results], [r["segments"] for r in results], gts, segs)
    assert flags == [0, 0, 0] and ref[0].sum() >= 1
    for bs in (2, 8):
        score = E.PanopticQuality()
        assert E.run_panoptic_quality(engine("coco_pano_semseg", bs), engine("coco_pano_inst", bs, target), pictures, gts, segs, score, **kw) is score
        same(score.counts(), ref)
    with pytest.raises(ValueError, match="coco_pano_semseg"):
        E.run_panoptic_quality(engine("coco_pano_inst", 2), engine("coco_pano_inst", 2), pictures, gts, segs, E.PanopticQuality())
    with pytest.raises(ValueError, match="ground truth"):
        E.run_panoptic_quality(engine("coco_pano_semseg", 2), engine("coco_pano_inst", 2, target), pictures, gts[::-1], segs, E.PanopticQuality())
