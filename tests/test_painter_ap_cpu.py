"""The instance-AP statement (tests/painter_ap_host.py) on cases whose answer is known by construction -- the expectations are literals,
within 1e-12 because precision carries COCOeval's np.spacing(1) term (a perfect prediction gives 0.9999999999999998) -- and what can be said
about the entry points without a GPU.  The statement is restated from pycocotools' published source and unverified against pycocotools,
which is not available here."""
import numpy as np
import pytest

from tests import painter_ap_cases as C
from tests import painter_ap_host as H

RANGES = C.SMALL_RANGES


def box(y0, y1, x0, x1, h=12, w=16):
    m = np.zeros((h, w), bool)
    m[y0:y1, x0:x1] = True
    return m


def dets(masks, scores, classes=None):
    return dict(masks=np.stack(masks), scores=np.array(scores, np.float32), classes=None if classes is None else np.array(classes, np.int32))


def gts(masks, anns):
    return dict(masks=np.stack(masks) if masks else np.zeros((0, 12, 16), bool),
                annotations=[dict(category_id=c, iscrowd=crowd, area=None) for c, crowd in anns])


def close(got, want):
    return abs(got - want) <= 1e-12


def test_the_higher_scored_detection_misses_and_the_lower_one_is_exact():
    g = box(2, 8, 3, 9)
    res = H.instance_ap([(dets([box(9, 11, 11, 15), g], [0.9, 0.5]), gts([g], [(0, 0)]))], 3, "agnostic", area_ranges=RANGES)
    assert close(res["AP"], 0.5) and close(res["AP50"], 0.5) and close(res["AP75"], 0.5)
    assert res["AR1"] == 0.0 and close(res["AR10"], 1.0) and close(res["AR100"], 1.0)


def test_an_identical_prediction_gives_one():
    g = box(2, 8, 3, 9)
    res = H.instance_ap([(dets([g], [0.7]), gts([g], [(0, 0)]))], 3, "agnostic", area_ranges=RANGES)
    assert close(res["AP"], 1.0) and res["AP"] == 0.9999999999999998 and close(res["AR1"], 1.0)
    # 36 pixels: both edges of a range belong to it, so small (0, 36) and medium (36, 400) both hold it
    assert close(res["APs"], 1.0) and close(res["APm"], 1.0) and res["APl"] == -1.0


def test_a_detection_inside_a_crowd_region_is_ignored_not_a_false_positive():
    g, crowd = box(2, 8, 3, 9), box(0, 12, 10, 16)
    pic = (dets([box(1, 5, 11, 15), g], [0.9, 0.5]), gts([g, crowd], [(0, 0), (0, 1)]))
    res = H.instance_ap([pic], 3, "agnostic", area_ranges=RANGES)
    assert close(res["AP"], 1.0) and close(res["AR10"], 1.0)
    assert res["AR1"] == 0.0                                            # the cut to one detection keeps the ignored one only
    rec, flags = H.picture_records(*pic, 3, ("agnostic",), H.IOU_THRS, RANGES)
    assert flags == 0 and rec["index"].tolist() == [0, 1]
    assert rec["matched"][0, 0] & np.uint64(1) and rec["ignored"][0, 0] & np.uint64(1)      # matched to the crowd region, so ignored
    assert rec["matched"][1, 0] & np.uint64(1) and not rec["ignored"][1, 0] & np.uint64(1)
    # without the crowd region the same detection is a false positive ahead of the true positive
    assert close(H.instance_ap([(pic[0], gts([g], [(0, 0)]))], 3, "agnostic", area_ranges=RANGES)["AP"], 0.5)


def test_an_empty_detection_on_a_picture_with_one_ground_truth():
    res = H.instance_ap([(H.empty_detections(12, 16), gts([box(2, 8, 3, 9)], [(0, 0)]))], 3, "agnostic", area_ranges=RANGES)
    assert res["AP"] == 0.0 and res["AR1"] == 0.0 and res["AR100"] == 0.0
    rec, _ = H.picture_records(H.empty_detections(12, 16), gts([box(2, 8, 3, 9)], [(0, 0)]), 3, ("agnostic",), H.IOU_THRS, RANGES)
    T = len(H.IOU_THRS)
    assert rec["matched"][0, 0] == 0 and rec["area"][0] == 0
    # area 0 lies in `all` and `small`: a false positive there, ignored in `medium` and `large`
    assert rec["ignored"][0, 0] == np.uint64(((1 << 2 * T) - 1) << 2 * T)


def test_per_class_with_a_detection_of_the_wrong_class():
    g = box(2, 8, 3, 9)
    pic = (dets([g], [0.7], [1]), gts([g], [(0, 0)]))
    res = H.instance_ap([pic], 3, "per_class", area_ranges=RANGES)
    assert res["per_class"] == [0.0, -1.0, -1.0] and res["AP"] == 0.0 and res["AR100"] == 0.0       # class 0 misses; class 1 has no ground truth
    rec, _ = H.picture_records(*pic, 3, H.MODES, H.IOU_THRS, RANGES)
    assert rec["matched"][0, 0] & np.uint64(1) and rec["matched"][0, 1] == 0                 # agnostic matches it, per class nothing does
    assert not rec["ignored"][0, 1] & np.uint64(1)                                            # a false positive for class 1
    assert close(H.instance_ap([pic], 3, "agnostic", area_ranges=RANGES)["AP"], 1.0)


def test_the_annotations_area_decides_the_range_and_the_pixel_count_the_iou():
    g = box(2, 8, 3, 9)                                                                       # 36 pixels
    truth = dict(masks=g[None], annotations=[dict(category_id=0, iscrowd=0, area=20.0)])
    res = H.instance_ap([(dets([g], [0.7]), truth)], 3, "agnostic", area_ranges=RANGES)
    assert close(res["APs"], 1.0) and res["APm"] == -1.0 and close(res["AP"], 1.0)


def test_records_of_all_detections_hold_every_cut():
    """picture_records matches all detections; its first m records are evaluateImg's answer for maxDet = m, per class too."""
    d, g = C.case(1, 61, 83, 7, 12)
    rec, flags = H.picture_records(d, g, C.K, H.MODES, H.IOU_THRS, RANGES)
    assert flags == 0 and len(rec) == 12
    T = len(H.IOU_THRS)
    for a, area in enumerate(RANGES):
        for t in (0, 4, 9):
            bit = np.uint64(1 << (a * T + t))
            for m in (1, 3, 12):
                idx, matched, ignored = H.evaluate_picture(d, g, H.IOU_THRS[t], area, m)
                assert idx.tolist() == rec["index"][:m].tolist()
                assert (((rec["matched"][:m, 0] & bit) != 0) == matched).all() and (((rec["ignored"][:m, 0] & bit) != 0) == ignored).all()
                for k in range(C.K):
                    idx, matched, ignored = H.evaluate_picture(d, g, H.IOU_THRS[t], area, m, category=k)
                    mine = rec[rec["category"] == k][:m]
                    assert idx.tolist() == mine["index"].tolist()
                    assert (((mine["matched"][:, 1] & bit) != 0) == matched).all() and (((mine["ignored"][:, 1] & bit) != 0) == ignored).all()


def test_generated_cases_hold_what_they_are_there_for():
    d, g = C.case(1, 61, 83, 7, 12)
    assert C.not_vacuous(d, g)
    assert sum(a["iscrowd"] for a in g["annotations"]) == 1 and len(set(d["classes"].tolist())) == 3
    assert 0 < H.instance_ap([(d, g)], C.K, "per_class", area_ranges=RANGES)["AP"] < 1
    assert np.array_equal(C.bits_of(d["masks"]).shape, (12, 159))


def random_records(seed, n_pictures, k, bits):
    """Records and annotations that no matching produced: what accumulate does with them does not depend on where they come from."""
    rng = np.random.default_rng(seed)
    records, annotations = [], []
    for _ in range(n_pictures):
        n = int(rng.integers(0, 9))
        rec = np.zeros(n, H.RECORD)
        rec["score"] = np.sort((np.round(rng.random(n) * 8) / 8).astype(np.float32))[::-1]
        rec["area"], rec["category"], rec["index"] = rng.integers(0, 900, n), rng.integers(0, k, n), rng.permutation(n)
        rec["matched"] = rng.integers(0, 1 << bits, (n, 2), dtype=np.uint64)
        rec["ignored"] = rng.integers(0, 1 << bits, (n, 2), dtype=np.uint64) & rng.integers(0, 1 << bits, (n, 2), dtype=np.uint64)
        records.append(rec)
        annotations.append([dict(category_id=int(rng.integers(0, k)), iscrowd=int(rng.random() < 0.2), area=float(rng.integers(1, 900)))
                            for _ in range(int(rng.integers(0, 6)))])
    return records, annotations


@pytest.mark.parametrize("mode", H.MODES)
def test_instance_ap_metrics_equals_the_statements_accumulate(mode):
    from painter_amd import painter_engine as E
    records, annotations = random_records(5, 7, C.K, 40)
    assert E.AP_RECORD == H.RECORD and E.AP_MODES == H.MODES
    precision, recall = H.accumulate(records, annotations, C.K, mode, H.IOU_THRS, H.REC_THRS, (1, 3, 100), RANGES)
    want = H.summarize(precision, recall, H.IOU_THRS, (1, 3, 100))
    got = E.instance_ap_metrics(records, annotations, C.K, mode, None, None, (1, 3, 100), RANGES)
    assert (precision > -1).any()
    assert got["precision"].tobytes() == precision.tobytes() and got["recall"].tobytes() == recall.tobytes()
    assert all(got[key] == want[key] for key in want) and set(want) == {"AP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR3", "AR100", "ARs",
                                                                         "ARm", "ARl"}
    assert ("per_class" in got) == (mode == "per_class")
    # other thresholds: AP50 / AP75 have no entry
    other = E.instance_ap_metrics(records, annotations, C.K, mode, [0.3, 0.6], None, (1, 3, 100), RANGES[:2])
    assert other["AP50"] == -1.0 and other["APm"] == -1.0 and other["precision"].shape[0] == 2


def test_header_declares_and_library_resolves_the_entry_points():
    from painter_amd import painter_engine as E
    from painter_amd._lib import lib, parse_header
    protos = parse_header()
    for name in ("pa_ap_add", "pa_ap_workspace_bytes", "pa_ap_workspace_offset"):
        assert name in protos and getattr(lib, name) is not None
    assert len(protos["pa_ap_add"][1]) == 16
    assert lib.pa_abi_version() == 9
    assert E.ctypes.sizeof(E.ApJob) == 72 and E.AP_GT.itemsize == 16 and E.AP_RECORD.itemsize == 48
    up16 = lambda x: -(-x // 16) * 16
    for n, d, g in ((1, 1, 1), (3, 100, 93), (7, 128, 128)):
        darea = up16(4 * n * d * g)
        gpix = up16(darea + 4 * n * d)
        order = up16(gpix + 4 * n * g)
        bits = up16(order + 4 * n * d)
        assert lib.pa_ap_workspace_bytes(n, d, g) == bits + 32 * n * d, (n, d, g)
        assert [lib.pa_ap_workspace_offset(n, d, g, which) for which in range(5)] == [0, darea, gpix, order, bits]
    for bad in ((0, 10, 10), (65536, 10, 10), (2, 0, 10), (2, 129, 10), (2, 10, 0), (2, 10, 129), (2, -1, 10)):
        assert lib.pa_ap_workspace_bytes(*bad) == -1, bad
        assert lib.pa_ap_workspace_offset(*bad, 0) == -1, bad
    assert lib.pa_ap_workspace_offset(2, 10, 10, 5) == -1 and lib.pa_ap_workspace_offset(2, 10, 10, -1) == -1


def test_entry_point_refuses_bad_arguments_before_anything_is_enqueued():
    """hipErrorInvalidValue (1): no pointer is touched, so this needs no GPU."""
    from painter_amd._lib import lib
    a = 256
    ok = dict(n=2, words=159, d=12, g=7, k=3, modes=3, t=10, r=4)

    def add(c, ptrs=None):
        jobs, thrs, ranges, records, counts, flags, ws = ptrs or [a] * 7
        return lib.pa_ap_add(jobs, c["n"], c["words"], c["d"], c["g"], c["k"], c["modes"], thrs, c["t"], ranges, c["r"], records, counts, flags,
                             ws, 0)

    for change in (dict(n=0), dict(n=65536), dict(words=0), dict(words=(1 << 26) + 1), dict(d=0), dict(d=129), dict(g=0), dict(g=129),
                   dict(k=0), dict(k=1025), dict(modes=0), dict(modes=4), dict(t=0), dict(r=0), dict(t=13, r=5), dict(t=65, r=1)):
        assert add(dict(ok, **change)) == 1, change
    for null in range(7):
        assert add(ok, [0 if i == null else a for i in range(7)]) == 1, null
    for at, off in ((0, 4), (1, 4), (2, 4), (3, 4), (4, 2), (5, 2), (6, 8)):          # misaligned table, parameters, records, words, workspace
        assert add(ok, [a + off if i == at else a for i in range(7)]) == 1, at


def test_a_cpu_device_is_refused():
    from painter_amd import painter_engine as E
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.InstanceAP(device="cpu")
