"""The panoptic-quality statement (tests/painter_pq_host.py) on cases whose answer is known by construction -- the expectations are
literals -- and what can be said about the entry points without a GPU.  The statement is restated from panopticapi's published source and
unverified against panopticapi, which is not available here."""
import math

import numpy as np
import pytest

from tests import painter_pq_host as H


def i32(*rows):
    return np.array(rows, np.int32)


def gts(*entries):
    """(id, category, iscrowd, area) -> ground-truth table with rank = position."""
    return [(i, c, crowd, area, rank) for rank, (i, c, crowd, area) in enumerate(entries)]


def one(pred, pred_table, gt, gt_table, k=3):
    (tp, fp, fn, iou), flags = H.accumulate([(pred, pred_table, gt, gt_table)], k)
    return tp.tolist(), fp.tolist(), fn.tolist(), iou.tolist(), flags[0]


def test_equal_maps_give_a_hundred():
    m = i32([1, 1, 2, 2, 3, 3])
    tp, fp, fn, iou, flags = one(m, [(1, 0), (2, 1), (3, 2)], m, gts((1, 0, 0, 2), (2, 1, 0, 2), (3, 2, 0, 2)))
    assert (tp, fp, fn, iou, flags) == ([1, 1, 1], [0, 0, 0], [0, 0, 0], [1.0, 1.0, 1.0], 0)
    res = H.averages(tp, fp, fn, iou, [True, True, False])
    for key in ("PQ", "SQ", "RQ", "PQ_th", "SQ_th", "RQ_th", "PQ_st", "SQ_st", "RQ_st"):
        assert res[key] == 100.0, key
    assert res["n"] == dict(All=3, Things=2, Stuff=1) and res["per_class"] == [(100.0, 100.0, 100.0)] * 3


def test_iou_of_exactly_one_half_is_no_match_and_an_unlisted_id_counts_toward_the_predicted_area_only():
    """C = 2, ground-truth area 2, predicted area 4 (the other two pixels lie on an id the annotation does not list: they stay in the
    union, where VOID pixels would leave it): 2 / 4 is not > 0.5."""
    assert one(i32([1, 1, 1, 1]), [(1, 0)], i32([7, 7, 9, 9]), gts((7, 0, 0, 2))) == ([0, 0, 0], [1, 0, 0], [1, 0, 0], [0.0, 0.0, 0.0], 0)


def test_iou_of_three_fifths_matches():
    assert one(i32([1, 1, 1, 1, 1]), [(1, 0)], i32([7, 7, 7, 9, 9]), gts((7, 0, 0, 3))) == ([1, 0, 0], [0, 0, 0], [0, 0, 0], [0.6, 0.0, 0.0], 0)


def test_void_under_a_prediction_leaves_the_union():
    assert one(i32([1, 1, 1, 1, 1, 1]), [(1, 0)], i32([0, 0, 7, 7, 7, 7]), gts((7, 0, 0, 4))) == ([1, 0, 0], [0, 0, 0], [0, 0, 0], [1.0, 0.0, 0.0], 0)
    # a category apart: no match, and the prediction (a third on VOID) is a false positive
    assert one(i32([1, 1, 1, 1, 1, 1]), [(1, 1)], i32([0, 0, 7, 7, 7, 7]), gts((7, 0, 0, 4))) == ([0, 0, 0], [0, 1, 0], [1, 0, 0], [0.0, 0.0, 0.0], 0)


def test_false_positive_rule_on_void():
    assert one(i32([1, 1, 1, 1, 1]), [(1, 0)], i32([0, 0, 0, 9, 9]), [])[1] == [0, 0, 0]          # 60 % on VOID: not counted
    assert one(i32([1, 1, 1, 1]), [(1, 0)], i32([0, 0, 9, 9]), [])[1] == [1, 0, 0]                # exactly 50 %: counted


def test_crowd_segments():
    m = i32([1, 1, 1, 1])
    # on a crowd segment of its own category: no false positive; the crowd segment is never matched and never a false negative
    assert one(m, [(1, 0)], i32([7, 7, 7, 7]), gts((7, 0, 1, 4))) == ([0, 0, 0], [0, 0, 0], [0, 0, 0], [0.0, 0.0, 0.0], 0)
    # on a crowd segment of another category: a false positive
    assert one(m, [(1, 0)], i32([7, 7, 7, 7]), gts((7, 1, 1, 4))) == ([0, 0, 0], [1, 0, 0], [0, 0, 0], [0.0, 0.0, 0.0], 0)
    # two crowd segments of one category: the one listed later is used, whatever its id
    gt = i32([7, 5, 5, 5])
    seg = lambda i: dict(id=i, category_id=0, iscrowd=1, area=None)
    pred_segments = [dict(id=1, category_id=0)]
    (_, fp, _, _), flags = H.pq([m], [pred_segments], [gt], [[seg(5), seg(7)]], 3, 2)
    assert fp.tolist() == [1, 0, 0] and flags == [0]                      # 7 is used: one pixel of four
    (_, fp, _, _), flags = H.pq([m], [pred_segments], [gt], [[seg(7), seg(5)]], 3, 2)
    assert fp.tolist() == [0, 0, 0] and flags == [0]                      # 5 is used: three pixels of four


@pytest.mark.parametrize("bit,pred,pred_table,gt,gt_table", [
    (0, i32([5]), [], i32([0]), []),                                                    # a predicted id that is not listed
    (1, i32([0]), [(1, 0)], i32([0]), []),                                              # a listed predicted segment without a pixel
    (2, i32([1]), [(1, 3)], i32([0]), []),                                              # category 3 of 3
    (3, i32([1]), [(1, 0)], i32([7]), gts((7, 0, 0, 0))),                               # the annotation says area 0: union 1 + 0 - 1
    (4, i32([1, 1]), [(1, 0)], i32([7, 8]), gts((7, 0, 0, 0), (8, 0, 0, 0))),           # two areas of 0: both reach IoU 1 with one p
    (5, i32([1]), [(1, 0)], i32([7]), gts((7, 0, 0, 1), (7, 0, 0, 1))),                 # a repeated id
])
def test_each_flag_bit_from_its_smallest_input(bit, pred, pred_table, gt, gt_table):
    good = (i32([1, 1]), [(1, 0)], i32([7, 7]), gts((7, 0, 0, 2)))
    (tp, fp, fn, iou), flags = H.accumulate([good, (pred, pred_table, gt, gt_table), good], 3)
    assert flags == [0, 1 << bit, 0]
    assert (tp.tolist(), fp.tolist(), fn.tolist(), iou.tolist()) == ([2, 0, 0], [0, 0, 0], [0, 0, 0], [2.0, 0.0, 0.0])
    assert (H.UNLISTED, H.EMPTY, H.CATEGORY, H.UNION, H.TWICE, H.ORDER)[bit] == 1 << bit


def test_descending_ids_raise_bit_five_and_the_python_layer_sorts():
    assert one(i32([1, 2]), [(2, 0), (1, 0)], i32([0, 0]), [])[4] == H.ORDER
    pt, gt = H.tables([dict(id=2, category_id=10), dict(id=1, category_id=30)], [dict(id=9, category_id=30, iscrowd=0, area=4),
                                                                                 dict(id=3, category_id=20, iscrowd=1, area=None)],
                      index={10: 0, 30: 1})
    assert pt == [(1, 1), (2, 0)] and gt == [(3, -1, 1, None, 1), (9, 1, 0, 4, 0)]


def test_a_group_without_counts_gives_nan():
    from painter_amd import painter_engine as E
    tp, fp, fn, iou = [2, 0, 0], [1, 0, 0], [0, 0, 0], [1.5, 0.0, 0.0]
    for res in (H.averages(tp, fp, fn, iou, [True, False, False]), E.pq_averages(tp, fp, fn, iou, [True, False, False])):
        assert res["PQ"] == res["PQ_th"] == 100 * (1.5 / 2.5) and res["SQ"] == 75.0 and res["RQ"] == 80.0
        assert all(math.isnan(res[k]) for k in ("PQ_st", "SQ_st", "RQ_st")) and res["n"] == dict(All=1, Things=1, Stuff=0)
    # a category with false negatives only: sq = 0 and it is averaged
    res = E.pq_averages([2, 0, 0], [1, 0, 0], [0, 3, 0], [1.5, 0.0, 0.0], [True, False, False], labels=[11, 22, 33])
    assert res["PQ_st"] == 0.0 and res["SQ_st"] == 0.0 and res["n"] == dict(All=2, Things=1, Stuff=1) and res["PQ"] == 100 * (0.6 / 2)
    assert res["per_class"][22] == dict(pq=0.0, sq=0.0, rq=0.0) and res["per_class"][11]["sq"] == 75.0
    ref = H.averages([2, 0, 0], [1, 0, 0], [0, 3, 0], [1.5, 0.0, 0.0], [True, False, False])
    assert all(res[k] == ref[k] for k in ref if k not in ("per_class", "n"))


def test_generated_cases_hold_what_they_are_there_for():
    from tests import painter_pq_cases as C
    c = C.case(3, 61, 83, 7, 9, noise=0.05)
    (tp, fp, fn, iou), flags = H.pq([c["pred"]], [c["pred_segments"]], [c["gt"]], [c["gt_segments"]])
    assert flags == [0] and tp.sum() >= 2 and fp.sum() >= 1 and fn.sum() >= 1
    assert (c["gt"] == 0).any() and (c["pred"] == 0).any() and sum(s["iscrowd"] for s in c["gt_segments"]) == 1
    assert len(set(np.unique(c["gt"]).tolist()) - {0} - {s["id"] for s in c["gt_segments"]}) == 1          # one unlisted id
    assert np.array_equal(H.gt_ids(c["gt_rgb"]), c["gt"])


def test_header_declares_and_library_resolves_the_entry_points():
    from painter_amd import painter_engine as E
    from painter_amd._lib import lib, parse_header
    protos = parse_header()
    for name in ("pa_pq_add", "pa_pq_lds_bins", "pa_pq_workspace_bytes"):
        assert name in protos and getattr(lib, name) is not None
    assert len(protos["pa_pq_add"][1]) == 14
    assert lib.pa_abi_version() == 9
    assert E.ctypes.sizeof(E.PqJob) == 64 and E.GT_SEGMENT.itemsize == 24 and E.SEGMENT.itemsize == 24
    # the LDS budget: two maps of 512 keys and 512 values (8 KB), plus 4 (G_cap + 2)(P_cap + 1) bytes of bins, within 160 KB
    for g, p in ((1, 1), (30, 20), (100, 153), (250, 153), (251, 153), (254, 153), (254, 255), (150, 255)):
        fits = 8192 + 4 * (g + 2) * (p + 1) <= 160 * 1024
        assert lib.pa_pq_lds_bins(g, p) == int(fits), (g, p)
    assert lib.pa_pq_lds_bins(250, 153) == 1 and lib.pa_pq_lds_bins(251, 153) == 0 and lib.pa_pq_lds_bins(254, 255) == 0
    for g, p in ((0, 1), (1, 0), (255, 1), (1, 256), (-1, 5)):
        assert lib.pa_pq_lds_bins(g, p) == 0, (g, p)
    up16 = lambda x: -(-x // 16) * 16
    for n, g, p, k in ((2, 10, 20, 133), (1, 1, 1, 1), (7, 254, 255, 1024)):
        want = up16(up16(4 * n * (g + 2) * (p + 1)) + 12 * n * g) + 8 * n * k
        assert lib.pa_pq_workspace_bytes(n, g, p, k) == want, (n, g, p, k)
    for bad in ((0, 10, 20, 133), (65536, 10, 20, 133), (2, 0, 20, 133), (2, 255, 20, 133), (2, 10, 0, 133), (2, 10, 256, 133),
                (2, 10, 20, 0), (2, 10, 20, 1025)):
        assert lib.pa_pq_workspace_bytes(*bad) == -1, bad


def test_entry_point_refuses_bad_arguments_before_anything_is_enqueued():
    """hipErrorInvalidValue (1): no pointer is touched, so this needs no GPU."""
    from painter_amd._lib import lib
    a = 256
    ok = dict(n=2, pixels=100, g=10, p=20, k=133, bins=0)

    def add(c, ptrs=None):
        jobs, tp, fp, fn, iou, flags, ws = ptrs or [a] * 7
        return lib.pa_pq_add(jobs, c["n"], c["pixels"], c["g"], c["p"], c["k"], c["bins"], tp, fp, fn, iou, flags, ws, 0)

    for change in (dict(n=0), dict(n=65536), dict(pixels=0), dict(pixels=(1 << 31) + 1), dict(g=0), dict(g=255), dict(p=0), dict(p=256),
                   dict(k=0), dict(k=1025), dict(bins=-1), dict(bins=2)):
        assert add(dict(ok, **change)) == 1, change
    for null in range(7):
        assert add(ok, [0 if i == null else a for i in range(7)]) == 1, null
    for at, off in ((1, 4), (4, 4), (5, 2), (6, 8)):                       # misaligned accumulators, flags, workspace
        assert add(ok, [a + off if i == at else a for i in range(7)]) == 1, at


def test_a_cpu_device_is_refused():
    from painter_amd import painter_engine as E
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.PanopticQuality(device="cpu")
