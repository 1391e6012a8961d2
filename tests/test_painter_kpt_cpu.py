"""The keypoint-AP statement (tests/painter_kpt_host.py) on cases whose answer is known by construction, the nudge condition of every
generated case the device tests use, and what can be said about the entry points without a GPU.  The statement restates mmpose's oks_nms
and xtcocotools' COCOeval from their published source and is unverified against mmpose / xtcocotools, which are not available here."""
import numpy as np
import pytest

from tests import painter_kpt_cases as C
from tests import painter_kpt_host as H

K = 17


def pose_of(xy, v=1.0):
    xy = np.asarray(xy, np.float32)
    return np.concatenate([xy, np.full((len(xy), 1), v, np.float32)], 1)


def ann(xy, vis=2, area=4000.0, bbox=(0, 0, 10, 10), iscrowd=0):
    kp = np.concatenate([np.asarray(xy, np.float64), np.full((len(xy), 1), float(vis))], 1)
    return dict(keypoints=kp.ravel().tolist(), area=area, bbox=list(bbox), iscrowd=iscrowd, num_keypoints=int(vis > 0) * len(xy))


def grid(x0, y0, k=K):
    """k keypoints on a small grid with its corner at (x0, y0): 40 x 30 pixels."""
    i = np.arange(k)
    return np.stack([x0 + 10.0 * (i % 5), y0 + 10.0 * (i // 5)], -1)


def bits(rec, name, a=0, T=10):
    return [[bool(int(w) >> (a * T + t) & 1) for t in range(T)] for w in rec[name]]


def test_one_box_on_its_ground_truth_gives_one():
    xy = grid(100, 100)
    out = H.photo_records([pose_of(xy)], [0.8], [12000.0], [ann(xy)])
    assert out["flags"] == 0 and out["oks"].tolist() == [[1.0]] and out["records"]["area"][0] == 40.0 * 30.0
    assert all(bits(out["records"], "matched")[0]) and not any(bits(out["records"], "ignored")[0])
    res = H.keypoint_ap({1: out["records"]}, {1: [ann(xy)]})
    assert abs(res["AP"] - 1.0) <= 1e-12 and res["AR"] == 1.0 and abs(res["APm"] - 1.0) <= 1e-12 and res["APl"] == -1.0


def test_rescoring():
    m = np.array([0.2, 0.1, 0.0, 0.2], np.float32)              # none above float32(0.2)
    assert H.rescore(m, 0.9) == 0 and H.rescore(m, 0.9).dtype == np.float32
    m[2] = 0.625
    assert H.rescore(m, 0.75) == np.float32(0.625) * np.float32(0.75)
    m = np.array([0.3, 0.7, 0.9], np.float32)                   # a float32 running sum, one division, one multiply
    want = np.float32(np.float32(np.float32(np.float32(0.3) + np.float32(0.7)) + np.float32(0.9)) / np.float32(3)) * np.float32(0.6)
    assert H.rescore(m, 0.6) == want
    assert H.box_area([0.9, 1.3]) == np.float32(np.float32(0.9) * np.float32(200)) * np.float32(np.float32(1.3) * np.float32(200))


def test_a_duplicate_bbox_id_keeps_the_first():
    assert H.unique_rows([5, 3, 5, 1, 3]).tolist() == [3, 1, 0]
    xy = grid(100, 100)
    pose = np.stack([pose_of(xy), pose_of(xy + 300), pose_of(xy + 300)])
    gt = {1: [ann(xy + 300)]}
    out = H.dataset_records(pose, [0.9, 0.8, 0.7], [12000.0] * 3, [1, 1, 1], [4, 2, 4], gt)[1]
    assert out["records"]["row"].tolist() == [0, 1]            # box 2 repeats id 4 and is gone; order by score
    assert bits(out["records"], "matched")[0][0] is False and all(bits(out["records"], "matched")[1])


def test_nms():
    xy = grid(100, 100)
    same = np.stack([pose_of(xy), pose_of(xy)])
    order, alive = H.oks_nms(same, [0.5, 0.9], [12000.0, 12000.0])
    assert order.tolist() == [1, 0] and alive.tolist() == [True, False]          # the lower-scored of two identical poses goes
    order, alive = H.oks_nms(same, [0.5, 0.5], [12000.0, 12000.0])
    assert order.tolist() == [1, 0] and alive.tolist() == [True, False]          # equal scores: the higher row is the pivot
    order, alive = H.oks_nms(same, [0.5, 0.5], [12000.0, 12000.0], use_nms=False)
    assert order.tolist() == [0, 1] and alive.all()                              # without NMS: COCOeval's stable sort, the lower row first
    far = np.stack([pose_of(xy), pose_of(xy + 200)])
    order, alive = H.oks_nms(far, [0.5, 0.9], [12000.0, 12000.0])
    assert alive.all() and H.nms_oks(far[0], far[1:], 12000.0, [12000.0])[0] < 1e-3
    assert H.nms_oks(same[0], same[1:], 1.0, [1.0])[0] == np.float32(1)


def test_a_ground_truth_without_keypoints_takes_the_box_distance_branch_and_is_ignored():
    xy = grid(100, 100)
    empty = ann(np.zeros((K, 2)), vis=0, area=5000.0, bbox=(100, 100, 40, 30))
    assert empty["num_keypoints"] == 0
    # every keypoint lies within (x - w, x + 2 w) x (y - h, y + 2 h): dx = dy = 0, OKS exactly 1
    assert H.eval_oks(pose_of(xy), empty["keypoints"], empty) == 1.0
    # 100 pixels right of x + 2 w = 180: dx = xd - 180 for every keypoint
    shifted = xy + [180.0, 0.0]
    var = (H.SIGMAS * 2) ** 2
    want = sum(np.exp(-((shifted[:, 0] - 180.0) ** 2 / var / (5000.0 + H.EPS) / 2))) / K
    assert abs(H.eval_oks(pose_of(shifted), empty["keypoints"], empty) - want) <= 1e-15
    out = H.photo_records([pose_of(xy)], [0.8], [12000.0], [empty])
    assert all(bits(out["records"], "matched")[0]) and all(bits(out["records"], "ignored")[0])      # ignored, not a false positive
    res = H.keypoint_ap({1: out["records"]}, {1: [empty]})
    assert res["AP"] == -1.0                                    # no ground truth counts


def test_an_unmatched_detection_outside_medium_is_ignored_there():
    xy = grid(100, 100)                                         # 40 x 30 = 1200 pixels: inside medium (1024, 9216)
    big = grid(300, 100) * [1.0, 1.0] + np.stack([np.arange(K) % 5 * 30.0, np.arange(K) // 5 * 30.0], -1)      # 160 x 120 = 19200
    out = H.photo_records([pose_of(xy), pose_of(big)], [0.9, 0.8], [12000.0, 12000.0], [])
    rec = out["records"]
    assert rec["area"].tolist() == [1200.0, 19200.0] and (rec["matched"] == 0).all()
    assert not any(bits(rec, "ignored", 0)[1]) and all(bits(rec, "ignored", 1)[1]) and not any(bits(rec, "ignored", 2)[1])
    assert not any(bits(rec, "ignored", 1)[0]) and all(bits(rec, "ignored", 2)[0])


def test_the_twenty_first_survivor_is_never_evaluated():
    case = C.case("twenty_one")
    out = case["statement"][3]
    assert out["alive"].sum() == 21 and len(out["records"]) == 20 and out["oks"].shape == (20, 2)
    scores = H.poses(case["preds"], case["maxvals"], case["centers"], case["scales"], case["box_scores"], C.HEAT)[1]
    last = int(out["order"][-1])
    assert scores[last] == scores.min() and sorted(out["records"]["row"].tolist()) == [r for r in range(21) if r != last]


def test_to_image_equals_the_engines():
    from painter_amd import painter_engine as E
    rng = np.random.default_rng(3)
    for _ in range(20):
        preds = (np.round(rng.uniform(-1, 255, (K, 2)) * 4) / 4).astype(np.float32)
        center, scale = rng.uniform(0, 640, 2).astype(np.float32), rng.uniform(0.2, 3, 2).astype(np.float32)
        got, want = H.to_image(preds, center, scale, C.HEAT), E.to_image(preds, center, scale, C.HEAT)
        assert got.dtype == np.float32 and got.tobytes() == want.astype(np.float32).tobytes()


def random_records(seed, images):
    """Records and annotations that no matching produced: what accumulate does with them does not depend on where they come from."""
    rng = np.random.default_rng(seed)
    records, gt = {}, {}
    for image in images:
        n = int(rng.integers(0, 9))
        rec = np.zeros(n, H.RECORD)
        rec["score"] = np.sort((np.round(rng.random(n) * 8) / 8).astype(np.float32))[::-1]
        rec["row"], rec["area"] = rng.permutation(n), rng.uniform(0, 2e4, n)
        rec["matched"] = rng.integers(0, 1 << 30, n, dtype=np.uint64)
        rec["ignored"] = rng.integers(0, 1 << 30, n, dtype=np.uint64) & rng.integers(0, 1 << 30, n, dtype=np.uint64)
        records[image] = rec
        gt[image] = [dict(keypoints=[0.0] * 51, area=float(rng.integers(1, 20000)), bbox=[0, 0, 1, 1], iscrowd=int(rng.random() < 0.2),
                          num_keypoints=int(rng.integers(0, 4))) for _ in range(int(rng.integers(0, 6)))]
    return records, gt


def test_keypoint_ap_metrics_equals_the_statements_accumulate():
    from painter_amd import painter_engine as E
    records, gt = random_records(5, [9, 3, 7, 1, 12, 5, 2])
    assert E.KPT_RECORD == H.RECORD and tuple(E.COCO_SIGMAS) == tuple(H.SIGMAS.tolist()) and E.KPT_AREA_RANGES == H.AREA_RANGES
    for max_dets in ((20,), (1, 3)):
        precision, recall = H.accumulate(records, gt, max_dets=max_dets)
        want = H.summarize(precision, recall)
        got = E.keypoint_ap_metrics(records, gt, max_dets=max_dets)
        assert (precision > -1).any()
        assert got["precision"].tobytes() == precision.tobytes() and got["recall"].tobytes() == recall.tobytes()
        assert all(got[key] == want[key] for key in want)
        assert set(want) == {"AP", "AP50", "AP75", "APm", "APl", "AR", "AR50", "AR75", "ARm", "ARl"}
    other = E.keypoint_ap_metrics(records, gt, [0.3, 0.6], None, H.AREA_RANGES[:1])
    assert other["AP50"] == -1.0 and other["APm"] == -1.0 and other["ARl"] == -1.0 and other["precision"].shape[0] == 2


def test_header_declares_and_library_resolves_the_entry_points():
    from painter_amd import painter_engine as E
    from painter_amd._lib import lib, parse_header
    protos = parse_header()
    for name in ("pa_kpt_poses", "pa_kpt_evaluate", "pa_kpt_workspace_bytes", "pa_kpt_workspace_offset"):
        assert name in protos and getattr(lib, name) is not None
    assert len(protos["pa_kpt_poses"][1]) == 12 and len(protos["pa_kpt_evaluate"][1]) == 22
    assert lib.pa_abi_version() == 9
    assert E.ctypes.sizeof(E.KptJob) == 32 and E.KPT_GT.itemsize == 48 and E.KPT_RECORD.itemsize == 32
    up16 = lambda x: -(-x // 16) * 16
    for n, d, g, m in ((1, 1, 1, 1), (3, 130, 9, 20), (7, 1024, 128, 64)):
        alive = up16(4 * n * d)
        oks = up16(alive + 4 * n * d)
        assert lib.pa_kpt_workspace_bytes(n, d, g, m) == oks + 8 * n * m * g, (n, d, g, m)
        assert [lib.pa_kpt_workspace_offset(n, d, g, m, which) for which in range(3)] == [0, alive, oks]
    for bad in ((0, 10, 10, 20), (65536, 10, 10, 20), (2, 0, 10, 20), (2, 1025, 10, 20), (2, 10, 0, 20), (2, 10, 129, 20), (2, 10, 10, 0),
                (2, 10, 10, 65), (2, -1, 10, 20)):
        assert lib.pa_kpt_workspace_bytes(*bad) == -1, bad
        assert lib.pa_kpt_workspace_offset(*bad, 0) == -1, bad
    assert lib.pa_kpt_workspace_offset(2, 10, 10, 20, 3) == -1 and lib.pa_kpt_workspace_offset(2, 10, 10, 20, -1) == -1


def test_entry_points_refuse_bad_arguments_before_anything_is_enqueued():
    """hipErrorInvalidValue (1): no pointer is touched, so this needs no GPU."""
    from painter_amd._lib import lib
    a, nan = 256, float("nan")
    ok = dict(n=3, k=17, w=192, h=256, vis=0.2)

    def poses(c, ptrs=None):
        preds, maxvals, boxes, out, scores, areas = ptrs or [a] * 6
        return lib.pa_kpt_poses(preds, maxvals, boxes, c["n"], c["k"], c["w"], c["h"], c["vis"], out, scores, areas, 0)

    for change in (dict(n=0), dict(n=(1 << 24) + 1), dict(k=0), dict(k=33), dict(w=0), dict(h=0), dict(vis=nan)):
        assert poses(dict(ok, **change)) == 1, change
    for null in range(6):
        assert poses(ok, [0 if i == null else a for i in range(6)]) == 1, null
    for at, off in ((0, 4), (1, 2), (2, 2), (3, 2), (4, 2), (5, 2)):
        assert poses(ok, [a + off if i == at else a for i in range(6)]) == 1, at

    ok = dict(n=2, rows=70, d=65, g=9, k=17, thr=0.9, m=20, t=10, r=3)

    def evaluate(c, ptrs=None):
        jobs, pose, scores, areas, sigmas, thrs, ranges, records, counts, survivors, flags, ws = ptrs or [a] * 12
        return lib.pa_kpt_evaluate(jobs, c["n"], pose, scores, areas, c["rows"], c["d"], c["g"], c["k"], sigmas, c["thr"], c["m"], thrs, c["t"],
                                   ranges, c["r"], records, counts, survivors, flags, ws, 0)

    for change in (dict(n=0), dict(n=65536), dict(rows=0), dict(rows=(1 << 24) + 1), dict(d=0), dict(d=1025), dict(g=0), dict(g=129), dict(k=0),
                   dict(k=33), dict(thr=nan), dict(m=0), dict(m=65), dict(t=0), dict(r=0), dict(t=13, r=5), dict(t=65, r=1)):
        assert evaluate(dict(ok, **change)) == 1, change
    for null in range(12):
        assert evaluate(ok, [0 if i == null else a for i in range(12)]) == 1, null
    for at, off in ((0, 4), (1, 2), (2, 2), (3, 2), (4, 4), (5, 4), (6, 4), (7, 4), (8, 2), (9, 2), (10, 2), (11, 8)):
        assert evaluate(ok, [a + off if i == at else a for i in range(12)]) == 1, at


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_generated_cases_keep_their_decisions_under_the_nudge(name):
    """Every case the device tests use: records, orders and survivors are identical with every OKS scaled by 1 -+ 1e-9.  Exempt is only
    the case built from OKS exactly 1.0 at a threshold of 1.0, where both sides are exact; there the exactness itself is asserted."""
    case = C.case(name)
    holds, ref = C.stable(case)
    assert C.same_decisions(ref, case["statement"])
    if name in C.EXACT:
        out = ref[3]
        assert not holds                                         # 1 - 1e-9 < min(1.0, 1 - 1e-10): the nudge would flip it
        assert (np.diag(out["oks"][:2]) == 1.0).all() and [b[2] for b in bits(out["records"], "matched", 0, 3)[:2]] == [True, True]
    else:
        assert holds


def test_cases_hold_what_they_are_there_for():
    mixed = C.case("mixed")
    assert [(len(r["order"]), len(mixed["ground_truth"][i])) for i, r in mixed["statement"].items()] == C.MIXED
    crowded = C.case("crowded")["statement"][7]
    assert len(crowded["order"]) == 1024 and 20 < crowded["alive"].sum() < 1024
    far = C.case("far")["statement"][3]
    assert (far["oks"] == 0).all() and far["alive"].all() and (far["records"]["matched"] == 0).all()
    hand = C.case("hand_made")
    out = hand["statement"][1]
    assert abs(out["oks"][0, 0] - hand["oks"]) <= 1e-15 and out["records"]["matched"].tolist() == [1, 0] and out["alive"].all()
    second = C.case("second_word")
    assert [(len(r["order"]), len(second["ground_truth"][i])) for i, r in second["statement"].items()] == C.SECOND_WORD
    evaluated, high, unmatched, ignored = C.second_word_facts(second, second["statement"])
    assert evaluated == 64 and high >= 1 and unmatched >= 1 and ignored >= 1, (evaluated, high, unmatched, ignored)
    # the same three facts in the records' own bits: bit 0 = (all, 0.5); a detection on a ground truth >= 64 has it set, an unmatched one not
    rec = second["statement"][100]["records"]
    assert int((rec["matched"] & np.uint64(1) != 0).sum()) == 64 - unmatched


def test_a_cpu_device_is_refused():
    from painter_amd import painter_engine as E
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.KeypointAP({}, device="cpu")
